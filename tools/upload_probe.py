#!/usr/bin/env python3
"""What a scene update costs: splat_upload_scene (host buffers: Morton order and block bounds on one host thread, 276 B per
Gaussian across PCIe) against splat_upload_scene_device (the same buffers already in device memory: order, bounds and
packing on the GPU), on one context each, for the scenes of bench.WORKLOADS.
usage: upload_probe.py [--out profiles/device_upload.json] [workload ...]     (default: C2 C3 C3s C5)
Per scene: the wall time of the call (median of five, after a 120000-Gaussian warm-up upload on the same context), the
device time of the sort alone (HIP events around its twelve launches) and the peak of splat_device_bytes on a context that
has seen nothing but that one upload.  The layouts of the two contexts are compared as well."""
import ctypes as C
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import splat_amd
from bench import WORKLOADS, make_scene

argv = sys.argv[1:]
out_path = "profiles/device_upload.json"
if argv[:1] == ["--out"]:
    out_path, argv = argv[1], argv[2:]
REPEATS = 5


def timed(fn):
    ts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def sort_ms(R):
    v = C.c_double()
    R._L.splat_debug_upload_sort_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    R._check(R._L.splat_debug_upload_sort_ms(R._h, C.byref(v)))
    return v.value


def fresh_peak(upload):
    R = splat_amd.Renderer()
    try:
        return upload(R)
    finally:
        R.close()


warm = splat_amd.synthetic_scene(120000, 71)
results = {}
for wl in (argv or ["C2", "C3", "C3s", "C5"]):
    n = WORKLOADS[wl][0]
    g = make_scene(wl)
    H, D = splat_amd.Renderer(), splat_amd.Renderer()
    g.compute_cov3d(H)
    warm.compute_cov3d(H)
    H.upload(warm)
    host_ms, host_all = timed(lambda: H.upload(g))
    dw = warm.to_device(D)
    dw.upload()
    dw.free()
    d = g.to_device(D)                      # (the caller's buffers: allocated through D, so D's byte counts include them)
    sorts = []

    def dev_upload():
        d.upload()
        sorts.append(sort_ms(D))
    dev_ms, dev_all = timed(dev_upload)
    oh, bh = H.scene_layout()
    od, bd = D.scene_layout()
    nan = np.isnan(bh) & np.isnan(bd)
    same = bool(np.array_equal(oh, od) and not ((bh.view(np.uint32) != bd.view(np.uint32)) & ~nan).any())
    H.close()
    # peaks on contexts that have seen one upload and nothing else; the device path's inputs belong to another context
    def host_once(R):
        R.upload(g)
        return R.device_bytes()[1]

    def dev_once(R):
        R.upload_device(d.positions, d.cov3d, d.opacities, d.sh, n=d.n)
        return R.device_bytes()[1]
    host_peak = fresh_peak(host_once)
    dev_peak = fresh_peak(dev_once)
    d.free()
    D.close()
    results[wl] = {"n_gaussians": n,
                   "host_upload_ms": round(host_ms, 3), "host_upload_ms_all": [round(t, 3) for t in host_all],
                   "device_upload_ms": round(dev_ms, 3), "device_upload_ms_all": [round(t, 3) for t in dev_all],
                   "device_sort_ms": round(statistics.median(sorts), 4),
                   "host_peak_bytes": host_peak, "device_peak_bytes": dev_peak, "layouts_equal": same}
    print(wl, json.dumps(results[wl]), flush=True)
    del g, d
doc = {"what": "wall time of one scene upload, median of %d, after a 120000-Gaussian warm-up upload on the same context: "
               "splat_upload_scene (host buffers) against splat_upload_scene_device (device buffers); device time of the sort "
               "alone from HIP events; peak of splat_device_bytes on a fresh context after the one upload" % REPEATS,
       "command": "python tools/upload_probe.py", "scenes": results}
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

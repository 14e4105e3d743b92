#!/usr/bin/env python3
"""What loading a PLY costs: the host path (load_from_ply on all host threads + compute_cov3d + upload: decode, exp /
sigmoid and recentring on the CPU, 276 B per Gaussian across PCIe) against Renderer.load_ply (the payload across PCIe once
as raw bytes, everything else on the GPU), in one process, on one context each, for PLY files of bench.WORKLOADS' scenes.
usage: ply_load_probe.py [--out profiles/ply_load.json] [workload ...]     (default: C3 C2)
Per scene: the file is written to a temporary directory and read once (file cache warm); then the wall time of each path,
median of five, after a 120000-Gaussian warm-up load on the same context; the device time of ply_decode_kernel,
recentre_sum_kernel and the subtract kernel from HIP events around them (median of the five loads); whether the two
contexts hold the same scene (order and block bounds)."""
import ctypes as C
import json
import os
import socket
import statistics
import sys
import tempfile
import time

sys.path.insert(0, ".")
import numpy as np
import splat_amd
from bench import SURFACE_WORKLOADS, WORKLOADS

argv = sys.argv[1:]
out_path = "profiles/ply_load.json"
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


def kernel_ms(R):
    v = (C.c_double * 3)()
    R._L.splat_debug_ply_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    R._check(R._L.splat_debug_ply_ms(R._h, v))
    return list(v)


def host_load(R, path):
    g = splat_amd.load_from_ply(path)
    g.compute_cov3d(R)
    R.upload(g)


results = {}
with tempfile.TemporaryDirectory() as tmp:
    warm = os.path.join(tmp, "warm.ply")
    splat_amd.write_ply(warm, splat_amd.synthetic_raw(120000, 71), 120000)
    for wl in (argv or ["C3", "C2"]):
        n, _, _, seed = WORKLOADS[wl]
        path = os.path.join(tmp, wl + ".ply")
        splat_amd.write_ply(path, (splat_amd.synthetic_surface_raw if wl in SURFACE_WORKLOADS else splat_amd.synthetic_raw)(n, seed), n)
        with open(path, "rb") as f:                          # file cache warm
            while f.read(1 << 26):
                pass
        H, D = splat_amd.Renderer(), splat_amd.Renderer()
        host_load(H, warm)
        host_ms, host_all = timed(lambda: host_load(H, path))
        D.load_ply(warm)
        kern = []

        def device_load():
            D.load_ply(path)
            kern.append(kernel_ms(D))
        dev_ms, dev_all = timed(device_load)
        oh, bh = H.scene_layout()
        od, bd = D.scene_layout()
        nan = np.isnan(bh) & np.isnan(bd)
        same = bool(np.array_equal(oh, od) and not ((bh.view(np.uint32) != bd.view(np.uint32)) & ~nan).any())
        H.close()
        D.close()
        med = [statistics.median(k[i] for k in kern) for i in range(3)]
        results[wl] = {"n_gaussians": n, "file_bytes": os.path.getsize(path),
                       "host_path_ms": round(host_ms, 3), "host_path_ms_all": [round(t, 3) for t in host_all],
                       "load_ply_ms": round(dev_ms, 3), "load_ply_ms_all": [round(t, 3) for t in dev_all],
                       "ply_decode_kernel_ms": round(med[0], 4), "recentre_sum_kernel_ms": round(med[1], 4),
                       "recentre_sub_kernel_ms": round(med[2], 4), "layouts_equal": same}
        print(wl, json.dumps(results[wl]), flush=True)
        os.remove(path)
doc = {"what": "wall time of loading a PLY file into a rendering context, median of %d in one process, file cache warm, after a "
               "120000-Gaussian warm-up load on the same context: load_from_ply + compute_cov3d + upload (host path) against "
               "Renderer.load_ply (payload to the device as raw bytes; decode, activations, recentring, K0 and upload on the GPU); "
               "device time of the three new kernels from HIP events" % REPEATS,
       "command": "python tools/ply_load_probe.py", "box": socket.gethostname(), "host_threads": os.cpu_count(), "scenes": results}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

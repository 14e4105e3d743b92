#!/usr/bin/env python3
"""What taking Gaussians out of a resident scene costs: splat_remove_gaussians_device with 1 %, 50 % and 99 % of the Gaussians
removed, by a random mask and by a contiguous run of original indices -- and, beside it in the same run, the route a caller had
before: splat_selection_indices_device of the complement, splat_read_gaussians_device of all four fields into buffers of its own
(248 B per Gaussian) and splat_upload_scene_device of those, which frees, allocates and sorts everything again.  The complement
mask and the buffers are made before the clock starts.  Every repetition starts from a fresh device upload of the whole scene
and a frame of it.
usage: remove_probe.py [--out profiles/scene_remove.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians, 1080p)
Per case: the wall time of the synchronous call(s), median over the repetitions; K1's device time and n_blocks_culled of a
frame before and after.  Nothing is gated: nobody has measured these kernels before."""
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
out_path, reps = "profiles/scene_remove.json", 21
while argv[:1] and argv[0].startswith("--"):
    if argv[0] == "--out":
        out_path = argv[1]
    elif argv[0] == "--reps":
        reps = int(argv[1])
    else:
        sys.exit(__doc__)
    argv = argv[2:]
wl = argv[0] if argv else "C3"
n, W, H, _ = WORKLOADS[wl]

R = splat_amd.Renderer()
g = make_scene(wl)
g.compute_cov3d(R)
d = g.to_device(R)
cam = splat_amd.Camera(H, W, (0.0, 0.0, 5.0))
cam.update_camera_pose()
cam_c = cam.to_c(0.01, 15)
image = R.device_image(np.zeros((H, W), np.uint32))
held = []


def device_alloc(nbytes):
    p = R._L.splat_device_alloc(R._h, max(int(nbytes), 4))
    if not p:
        raise MemoryError("splat_device_alloc(%d)" % nbytes)
    held.append(p)
    return p


def device_array(a):
    a = np.ascontiguousarray(a)
    p = device_alloc(a.nbytes)
    R._check(R._L.splat_device_upload(R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
    return p


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def k1_frame():
    st = R.render_frame_device(cam_c, image, sync=True, want_stats=True)
    return st.ms_preprocess, int(st.n_blocks_culled)


# the caller's buffers of the old route: indices and the four fields, sized for the whole scene
index = device_alloc(4 * n)
rows = dict(positions=device_alloc(16 * n), cov3d=device_alloc(36 * n), opacities=device_alloc(4 * n), sh=device_alloc(192 * n))
CASES = []
for pct in (1, 50, 99):
    k = n * pct // 100
    rnd = np.zeros(n, np.uint8)
    rnd[np.random.default_rng(pct).choice(n, k, replace=False)] = 1
    run = np.zeros(n, np.uint8)
    run[(n - k) // 2: (n - k) // 2 + k] = 1
    for shape, gone in (("random", rnd), ("contiguous", run)):
        CASES.append(("%dpct_%s" % (pct, shape), n - k, device_array(gone), device_array(1 - gone)))


def old_route(stay_mask, left):
    assert R.selection_indices(stay_mask, index, n=n, capacity=n) == left
    R.read_indexed(index, k=left, **rows)
    R.upload_device(rows["positions"], rows["cov3d"], rows["opacities"], rows["sh"], n=left)


results = {name: {"remove": [], "reupload": [], "k1_before": [], "k1_after": [], "culled_before": [], "culled_after": [],
                  "k1_after_reupload": [], "culled_after_reupload": []} for name, _, _, _ in CASES}
for _ in range(reps + 1):                                 # (the first round warms everything up and is not kept)
    for name, left, gone_mask, stay_mask in CASES:
        r = results[name]
        for route in ("remove", "reupload"):
            d.upload()
            k1_frame()
            before = k1_frame()
            if route == "remove":
                r[route].append(timed(lambda: R.remove(gone_mask, n=n)))
            else:
                r[route].append(timed(lambda: old_route(stay_mask, left)))
            assert R.n == left
            k1_frame()
            after = k1_frame()
            if route == "remove":
                r["k1_before"].append(before[0]); r["culled_before"].append(before[1])
                r["k1_after"].append(after[0]); r["culled_after"].append(after[1])
            else:
                r["k1_after_reupload"].append(after[0]); r["culled_after_reupload"].append(after[1])
dropped = R.frames_dropped()
R.device_free(image)
for p in held:
    R.device_free(p)
d.free()
R.close()


def med(v):
    return round(statistics.median(v[1:]), 4)


cases = {}
for name, left, _, _ in CASES:
    r = results[name]
    cases[name] = {"n_after": left, "remove_ms": med(r["remove"]), "remove_ms_min": round(min(r["remove"][1:]), 4),
                   "remove_ms_max": round(max(r["remove"][1:]), 4), "indices_read_upload_ms": med(r["reupload"]),
                   "indices_read_upload_ms_min": round(min(r["reupload"][1:]), 4),
                   "k1_ms_before": med(r["k1_before"]), "k1_ms_after": med(r["k1_after"]), "k1_ms_after_reupload": med(r["k1_after_reupload"]),
                   "n_blocks_culled_before": int(med(r["culled_before"])), "n_blocks_culled_after": int(med(r["culled_after"])),
                   "n_blocks_culled_after_reupload": int(med(r["culled_after_reupload"]))}
doc = {"what": "wall time of the synchronous Renderer.remove, medians of %d repetitions, each from a fresh device upload of the whole "
               "scene and two frames of %d x %d; indices_read_upload_ms: the route without it in the same run (selection_indices of "
               "the complement + read_indexed of four fields + upload_device; the complement mask and the buffers made beforehand); "
               "k1_ms_*: K1's device time of the second frame before / after; n_blocks_culled_*: that frame's culled K1 blocks"
               % (reps, W, H),
       "command": "python tools/remove_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps, "frames_dropped": dropped,
       "cases": cases}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

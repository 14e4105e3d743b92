#!/usr/bin/env python3
"""What moving or reading back part of a resident scene costs: splat_transform_scene_device and
splat_transform_gaussians_device (1 %, 50 %, 100 % of the Gaussians selected), splat_read_scene_device and
splat_read_gaussians_device (positions and covariances of the same rows) -- and, beside them, the route a caller had before:
splat_update_gaussians_device of PRECOMPUTED positions and covariances for the same rows (computing them is not in it).
Also splat_rotate_sh_scene_device and splat_rotate_sh_gaussians_device with the transform's rotation, whole and for the same rows.
All on one context, with the same data, alternated in one run.
usage: transform_probe.py [--out profiles/scene_transform.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians)
Per operation: the wall time of the synchronous call, median over the repetitions; K1's device time per frame from the
statistics of the frames rendered in between.  Nothing is gated: nobody has measured these kernels before."""
import ctypes as C
import json
import math
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import splat_amd
from bench import WORKLOADS, make_scene

argv = sys.argv[1:]
out_path, reps = "profiles/scene_transform.json", 21
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
# one degree about the vertical axis through the origin: the scene stays where the camera sees it, however often it is applied
t = math.radians(1.0)
M = np.array([[math.cos(t), 0, math.sin(t), 0], [0, 1, 0, 0], [-math.sin(t), 0, math.cos(t), 0]], np.float32)


def device_alloc(nbytes):
    p = R._L.splat_device_alloc(R._h, nbytes)
    if not p:
        raise MemoryError("splat_device_alloc(%d)" % nbytes)
    held.append(p)
    return p


def device_array(a):
    a = np.ascontiguousarray(a)
    p = device_alloc(a.nbytes)
    R._check(R._L.splat_device_upload(R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
    return p


out_pos, out_cov = device_alloc(16 * n), device_alloc(36 * n)
ROT = np.ascontiguousarray(M[:, :3])
OPS = [("transform_scene", lambda: R.transform(M)),
       ("rotate_sh_scene", lambda: R.rotate_sh(ROT)),
       ("read_scene_pos_cov", lambda: R.read_device(positions=out_pos, cov3d=out_cov, n=n))]
for pct in (1, 50, 100):
    k = n * pct // 100
    idx = np.random.default_rng(pct).choice(n, k, replace=False).astype(np.uint32)
    a = dict(index=device_array(idx), k=k)
    rows = dict(positions=device_array(g.positions[idx]), cov3d=device_array(g.cov3d[idx]))
    OPS += [("transform_indexed_%dpct" % pct, lambda a=a: R.transform(M, **a)),
            ("read_indexed_pos_cov_%dpct" % pct, lambda a=a: R.read_indexed(positions=out_pos, cov3d=out_cov, **a)),
            ("update_indexed_pos_cov_%dpct" % pct, lambda a=a, rows=rows: R.update_indexed(**a, **rows)),
            ("rotate_sh_indexed_%dpct" % pct, lambda a=a: R.rotate_sh(ROT, **a))]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


d.upload()
for _ in range(3):                                    # key buffers, per-tile arrays, the inverse order: made before the clock starts
    R.render_frame_device(cam_c, image, sync=True)
OPS[3][1]()
call = {name: [] for name, _ in OPS}
k1 = []
for _ in range(reps):
    for name, fn in OPS:
        call[name].append(timed(fn))
        k1.append(R.render_frame_device(cam_c, image, sync=True, want_stats=True).ms_preprocess)
dropped = R.frames_dropped()
R.device_free(image)
for p in held:
    R.device_free(p)
d.free()
R.close()

results = {name: {"call_ms": round(statistics.median(call[name]), 4), "call_ms_min": round(min(call[name]), 4),
                  "call_ms_max": round(max(call[name]), 4)} for name, _ in OPS}
doc = {"what": "wall time of one synchronous call on the resident scene, medians of %d repetitions, the operations alternated in one "
               "run on one context with the same data (a frame of %d x %d between any two); update_indexed_* is the route through "
               "precomputed values for the same rows, computing them excluded; k1_ms_per_frame: K1's device time in the frames "
               "between the calls" % (reps, W, H),
       "command": "python tools/transform_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps,
       "k1_ms_per_frame": round(statistics.median(k1), 4), "frames_dropped": dropped, "operations": results}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

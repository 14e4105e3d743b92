#!/usr/bin/env python3
"""What a change to a resident scene costs: the re-upload (splat_upload_scene_device -- before the in-place edits, the only
way) against splat_update_scene_device (all fields, positions only, opacities only) and splat_update_gaussians_device
(k = 1 000 and k = 100 000, all fields), on one context, with the same data, alternated in one run.
usage: update_probe.py [--out profiles/scene_update.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians)
Per operation: the wall time of the call and of the first frame after it (a synchronous splat_render_frame_device at the
workload's size), medians over the repetitions.  The all-fields update does a strict subset of the re-upload's work: the
probe exits with 1 when it is slower."""
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
out_path, reps = "profiles/scene_update.json", 21
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


def device_array(a):
    a = np.ascontiguousarray(a)
    p = R._L.splat_device_alloc(R._h, a.nbytes)
    if not p:
        raise MemoryError("splat_device_alloc(%d)" % a.nbytes)
    held.append(p)
    R._check(R._L.splat_device_upload(R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
    return p


def indexed(k):
    idx = np.random.default_rng(k).choice(n, k, replace=False).astype(np.uint32)
    a = dict(index=device_array(idx), k=k, positions=device_array(g.positions[idx]), cov3d=device_array(g.cov3d[idx]),
             opacities=device_array(g.opacities[idx]), sh=device_array(g.sh[idx]))
    return lambda: R.update_indexed(**a)


OPS = [("upload_scene_device", d.upload),
       ("update_all_fields", lambda: R.update_device(d.positions, d.cov3d, d.opacities, d.sh, n=n)),
       ("update_positions", lambda: R.update_device(positions=d.positions, n=n)),
       ("update_opacities", lambda: R.update_device(opacities=d.opacities, n=n)),
       ("update_indexed_1000", indexed(1000)),
       ("update_indexed_100000", indexed(100000))]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


d.upload()
for _ in range(3):                                    # key buffers, per-tile arrays, the inverse order: made before the clock starts
    R.render_frame_device(cam_c, image, sync=True)
OPS[4][1]()
call = {name: [] for name, _ in OPS}
first = {name: [] for name, _ in OPS}
for _ in range(reps):
    for name, fn in OPS:
        call[name].append(timed(fn))
        first[name].append(timed(lambda: R.render_frame_device(cam_c, image, sync=True)))
at_rest = [timed(lambda: R.render_frame_device(cam_c, image, sync=True)) for _ in range(reps)]
dropped = R.frames_dropped()
R.device_free(image)
for p in held:
    R.device_free(p)
d.free()
R.close()

results = {name: {"call_ms": round(statistics.median(call[name]), 4), "first_frame_ms": round(statistics.median(first[name]), 4),
                  "call_ms_min": round(min(call[name]), 4), "call_ms_max": round(max(call[name]), 4)} for name, _ in OPS}
ok = results["update_all_fields"]["call_ms"] <= results["upload_scene_device"]["call_ms"]
doc = {"what": "wall time of one change to the resident scene and of the first frame after it (synchronous, %d x %d), medians of %d "
               "repetitions, the operations alternated in one run on one context with the same data; the yardstick is the "
               "re-upload (upload_scene_device)" % (W, H, reps),
       "command": "python tools/update_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps,
       "frame_at_rest_ms": round(statistics.median(at_rest), 4), "frames_dropped": dropped,
       "all_fields_update_not_slower_than_upload": bool(ok), "operations": results}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
sys.exit(0 if ok else 1)

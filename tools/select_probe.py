#!/usr/bin/env python3
"""What a selection costs: one rectangle-and-mask selection (splat_select_device: screen test by centre with a painted pixel
mask) and one compaction (splat_selection_indices_device) at 1 %, 50 % and 100 % selected, on the resident scene of a
workload, beside the same run's K1 time per frame from splat_get_timing -- K1 reads the geometry planes the screen test
reads (and the SH planes on top), so it is the bandwidth yardstick.
usage: select_probe.py [--out profiles/select.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians at 1080p)
Per operation: the wall time of the call (synchronous: temporaries, kernels, the count's read-back), median / min / max over
the repetitions.  Nothing is asserted on the times; the counts are checked against what was put in."""
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
out_path, reps = "profiles/select.json", 21
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
R.upload(g)
cam = splat_amd.Camera(H, W, (0.0, 0.0, 5.0))
cam.update_camera_pose()
cam_c = cam.to_c(0.01, 15)
image = R.device_image(np.zeros((H, W), np.uint32))
held = [image]


def device_array(a):
    a = np.ascontiguousarray(a)
    p = R._L.splat_device_alloc(R._h, a.nbytes)
    if not p:
        raise MemoryError("splat_device_alloc(%d)" % a.nbytes)
    held.append(p)
    R._check(R._L.splat_device_upload(R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
    return p


def timed(fn):
    t0 = time.perf_counter()
    v = fn()
    return (time.perf_counter() - t0) * 1e3, v


yy, xx = np.mgrid[0:H, 0:W]
brush = device_array(((((xx - W // 2) ** 2 + (yy - H // 2) ** 2) <= (H // 3) ** 2)).astype(np.uint8))      # a painted disc
rect = (W // 8, H // 8, W - W // 8, H - H // 8)
selection = device_array(np.zeros(n, np.uint8))
indices = device_array(np.zeros(n, np.uint32))
rng = np.random.default_rng(1)
masks = {}
for name, density in (("1_percent", 0.01), ("50_percent", 0.5), ("100_percent", 1.0)):
    m = (rng.random(n) < density).astype(np.uint8)
    masks[name] = (device_array(m), int(m.sum()))

for _ in range(3):                                    # key buffers and per-tile arrays: made before the clock starts
    R.render_frame_device(cam_c, image, sync=True)
R.timing(reset=True)
times = {"select_rect_and_mask": []}
times.update({"indices_" + name: [] for name in masks})
selected = None
for _ in range(reps):
    for _ in range(8):                                # frames between the selections, as an editor has them: every eighth carries events
        R.render_frame_device(cam_c, image, sync=False)
    R.sync()                                          # (the call would wait for them itself: not on its clock)
    t, k = timed(lambda: R.select(selection, cam_c, rect=rect, pixel_mask=brush))
    times["select_rect_and_mask"].append(t)
    assert selected in (None, k)
    selected = k
    for name, (p, count) in masks.items():
        t, k = timed(lambda: R.selection_indices(p, indices, n=n, capacity=n))
        times["indices_" + name].append(t)
        assert k == count, (name, k, count)
R.sync()
ms, frames = R.timing(reset=True)
dropped = R.frames_dropped()
for p in held:
    R.device_free(p)
R.close()

doc = {"what": "wall time of one synchronous selection call on the resident scene (%d x %d target), medians of %d repetitions with "
               "frames in between; k1_ms_per_frame is the same run's device time of K1 per frame (splat_get_timing): the "
               "bandwidth yardstick.  Nothing is asserted on these times." % (W, H, reps),
       "command": "python tools/select_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps,
       "selected_by_rect_and_mask": selected, "k1_ms_per_frame": round(ms["preprocess"] / frames, 4) if frames else None,
       "timed_frames": frames, "frames_dropped": dropped,
       "operations": {name: {"call_ms": round(statistics.median(v), 4), "call_ms_min": round(min(v), 4), "call_ms_max": round(max(v), 4)}
                      for name, v in times.items()}}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

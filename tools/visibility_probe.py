#!/usr/bin/env python3
"""What a visibility query costs: Renderer.visibility (splat_visibility_device) on the resident scene of a workload with
weight_min 1/255 and 0, over the whole target and over a 256x256 rectangle at its middle -- beside one synchronous statistics
frame of the same camera (the query bins the view like a two-pass frame and walks every list: a frame is what it is to be read
against) and a selection by a SCREEN rectangle (splat_select_device: one projection per Gaussian, no lists), in the same run.
usage: visibility_probe.py [--out profiles/visibility.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians at 1080p)
Per operation: the wall time of the synchronous call (binning, the call's key buffers, the sort launches, the walk), median /
min / max over the repetitions.  Nothing is asserted on the times.  Also recorded: how many Gaussians are seen at each
weight_min over the whole target, the pairs of the view and what the call leaves in splat_device_bytes()."""
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
out_path, reps = "profiles/visibility.json", 21
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
selection = R._L.splat_device_alloc(R._h, n)
pixels = R._L.splat_device_alloc(R._h, 4 * n)
max_weight = R._L.splat_device_alloc(R._h, 4 * n)
weight_sum = R._L.splat_device_alloc(R._h, 8 * n)
assert selection and pixels and max_weight and weight_sum


def timed(fn):
    t0 = time.perf_counter()
    v = fn()
    return (time.perf_counter() - t0) * 1e3, v


rect = (W // 2 - 128, H // 2 - 128, W // 2 + 127, H // 2 + 127)
cases = [("weight_min_1_255_whole", 1.0 / 255.0, None), ("weight_min_0_whole", 0.0, None),
         ("weight_min_1_255_rect_256", 1.0 / 255.0, rect), ("weight_min_0_rect_256", 0.0, rect)]


def query(weight_min, region):
    return R.visibility(cam_c, weight_min=weight_min, rect=region, pixels=pixels, max_weight=max_weight, weight_sum=weight_sum)


for _ in range(3):                                    # key buffers and per-tile arrays: made before the clock starts
    R.render_frame_device(cam_c, image, sync=True)
held_before = R.device_bytes()[0]
query(1.0 / 255.0, None)                              # the slot's two-pass buffers: made before the clock starts, too
held_after = R.device_bytes()[0]
times = {"visibility_" + name: [] for name, _, _ in cases}
times["statistics_frame"] = []
times["select_screen_touch_rect_256"] = []
n_pairs = 0
for _ in range(reps):
    for _ in range(8):                                # frames between the calls, as an editor has them
        R.render_frame_device(cam_c, image, sync=False)
    R.sync()                                          # (the call would wait for them itself: not on its clock)
    t, st = timed(lambda: R.render_frame_device(cam_c, image, sync=True, want_stats=True))
    times["statistics_frame"].append(t)
    n_pairs = int(st.n_pairs)
    t, _ = timed(lambda: R.select(selection, cam_c, rect=rect, rule="touch"))
    times["select_screen_touch_rect_256"].append(t)
    for name, weight_min, region in cases:
        t, _ = timed(lambda: query(weight_min, region))
        times["visibility_" + name].append(t)
R.sync()
dropped = R.frames_dropped()

seen = {}
for name, weight_min, region in cases[:2]:            # (outside the clock)
    query(weight_min, region)
    p = np.zeros(n, np.uint32)
    R._check(R._L.splat_device_download(R._h, C.c_void_p(p.ctypes.data), C.c_void_p(pixels), p.nbytes))
    seen[name] = {"gaussians_seen": int((p > 0).sum()), "most_pixels": int(p.max())}
held_end = R.device_bytes()[0]
for p in (selection, pixels, max_weight, weight_sum, image):
    R.device_free(p)
R.close()

doc = {"what": "wall time of one synchronous Renderer.visibility on the resident scene (%d x %d target), all three outputs, medians of "
               "%d repetitions with frames in between, beside one synchronous statistics frame of the same camera and a select by "
               "a SCREEN rectangle (touch rule, the same 256x256 pixels) in the same run.  Nothing is asserted on these times." % (W, H, reps),
       "command": "python tools/visibility_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps, "n_pairs": n_pairs,
       "frames_dropped": dropped, "seen": seen,
       "device_bytes": {"before_first_query": held_before, "after_first_query": held_after, "at_the_end": held_end},
       "operations": {name: {"call_ms": round(statistics.median(v), 4), "call_ms_min": round(min(v), 4), "call_ms_max": round(max(v), 4)}
                      for name, v in times.items()}}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

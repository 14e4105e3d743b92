#!/usr/bin/env python3
"""What a pick costs: Renderer.pick (splat_pick_device) of 1, 64 and 256 pixels on the resident scene of a workload, the pixels
once scattered over the target and once packed in a 16x16 block at its middle, with max_hits 1024 and layers 0 and 64 (and max_hits 4096 once) --
beside a selection by a SCREEN rectangle (splat_select_device: the same one-thread-per-slot projection, no fragments, no
lists) and the same run's K1 time per frame from splat_get_timing.  Those two are what the pick is to be read against.
usage: pick_probe.py [--out profiles/pick.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians at 1080p)
Per operation: the wall time of the synchronous call (temporaries, the two kernels, the results' copy down), median / min /
max over the repetitions.  Nothing is asserted on the times.  Also recorded: the largest n_hits any queried pixel had, and
for every pixel that came back TRUNCATED at max_hits 1024 or 4096 how many hits it had -- the number that says whether the
cap wants a follow-up."""
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
out_path, reps = "profiles/pick.json", 21
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
R.set_option(splat_amd._lib.OPT_RETAIN_LISTS, 0)      # the frames between the calls bin, so that K1 is on the same run's clock
g = make_scene(wl)
g.compute_cov3d(R)
R.upload(g)
cam = splat_amd.Camera(H, W, (0.0, 0.0, 5.0))
cam.update_camera_pose()
cam_c = cam.to_c(0.01, 15)
image = R.device_image(np.zeros((H, W), np.uint32))
selection = R._L.splat_device_alloc(R._h, n)
assert selection


def timed(fn):
    t0 = time.perf_counter()
    v = fn()
    return (time.perf_counter() - t0) * 1e3, v


rng = np.random.default_rng(1)
scattered = np.stack([rng.integers(0, W, 256), rng.integers(0, H, 256)], 1).astype(np.int32)
scattered[0] = (W // 2, H // 2)
yy, xx = np.mgrid[0:16, 0:16]
packed = np.stack([xx.ravel() + W // 2 - 8, yy.ravel() + H // 2 - 8], 1).astype(np.int32)
packed = packed[np.argsort(np.abs(packed[:, 0] - W // 2) + np.abs(packed[:, 1] - H // 2), kind="stable")]   # prefixes grow from the middle
sets = {"scattered": scattered, "packed": packed}
cases = [(name, count, layers, 1024) for name in sets for count in (1, 64, 256) for layers in (0, 64)]
cases += [(name, count, 0, 4096) for name in sets for count in (1, 256)]        # ... and with the largest list, should 1024 truncate
rect = (W // 2 - 8, H // 2 - 8, W // 2 + 7, H // 2 + 7)

for _ in range(3):                                    # key buffers and per-tile arrays: made before the clock starts
    R.render_frame_device(cam_c, image, sync=True)
R.timing(reset=True)
times = {"pick_%s_%d_layers_%d_max_hits_%d" % c: [] for c in cases}
times["select_screen_touch_rect"] = []
for _ in range(reps):
    for _ in range(8):                                # frames between the calls, as an editor has them
        R.render_frame_device(cam_c, image, sync=False)
    R.sync()                                          # (the call would wait for them itself: not on its clock)
    t, _ = timed(lambda: R.select(selection, cam_c, rect=rect, rule="touch"))
    times["select_screen_touch_rect"].append(t)
    for name, count, layers, max_hits in cases:
        t, _ = timed(lambda: R.pick(cam_c, sets[name][:count], max_hits=max_hits, layers=layers))
        times["pick_%s_%d_layers_%d_max_hits_%d" % (name, count, layers, max_hits)].append(t)
R.sync()
ms, frames = R.timing(reset=True)
dropped = R.frames_dropped()

# the hit counts, and what the caps cut (outside the clock)
counts = {name: R.pick(cam_c, sets[name], max_hits=1024) for name in sets}
truncated = {}
for cap in (1024, 4096):
    truncated[str(cap)] = {}
    for name in sets:
        r = R.pick(cam_c, sets[name], max_hits=cap)
        cut = r["n_hits"][(r["flags"] & 1) != 0]
        truncated[str(cap)][name] = {"pixels": int(cut.size), "n_hits_min": int(cut.min()) if cut.size else None,
                                     "n_hits_max": int(cut.max()) if cut.size else None}
R.device_free(selection)
R.device_free(image)
R.close()

doc = {"what": "wall time of one synchronous Renderer.pick on the resident scene (%d x %d target), medians of %d "
               "repetitions with frames in between, beside a select by a SCREEN rectangle (touch rule, the packed block's 16x16 "
               "pixels) and the same run's device time of K1 per frame (splat_get_timing).  Nothing is asserted on these times." % (W, H, reps),
       "command": "python tools/pick_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps,
       "k1_ms_per_frame": round(ms["preprocess"] / frames, 4) if frames else None, "timed_frames": frames, "frames_dropped": dropped,
       "n_hits": {name: {"max": int(r["n_hits"].max()), "median": float(np.median(r["n_hits"])), "pixels_with_hits": int((r["n_hits"] > 0).sum())}
                  for name, r in counts.items()},
       "truncated_pixels": truncated,
       "operations": {name: {"call_ms": round(statistics.median(v), 4), "call_ms_min": round(min(v), 4), "call_ms_max": round(max(v), 4)}
                      for name, v in times.items()}}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

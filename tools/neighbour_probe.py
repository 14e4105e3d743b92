#!/usr/bin/env python3
"""What a selection by neighbourhood costs (splat_select_neighbours_device) on the resident scene of a workload, beside the
same run's K1 time per frame from splat_get_timing.
usage: neighbour_probe.py [--out profiles/select_neighbours.json] [--reps 9] [--leg-seconds 4] [--pairs-per-block N] [workload]
(default workload: C3)
Three radii are derived from the scene: 1, 2 and 4 times the median nearest-neighbour distance of a sample of 256 Gaussians
(all pairs against the whole scene, numpy).  At each radius four legs: every Gaussian a source / a random 10 % source mask,
each counted without a bound / with at_most=7 (the floater test: a lane stops at 8).  Per leg: block_pairs, how many pass,
and the wall time of the synchronous call (temporaries, the three kernels, two read-backs), median / min / max.
Every leg runs under its own time limit, which ends the REPETITIONS and never a call: a leg stops repeating once
--leg-seconds have gone, and when one call alone took longer than that, the larger radii of the same kind are not run but
recorded as skipped.  A synchronous call cannot be cut short; what bounds one call is max_block_pairs.  It stays at the
binding's default (64 per block), so a radius that turns out too large is refused by the library -- recorded with its
block_pairs -- instead of running for minutes; --pairs-per-block N raises it to N per block for a scene whose blocks' bounds
overlap more than that at any radius (the refusals of a default run say so).  Nothing is asserted on the times."""
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
out_path, reps, leg_seconds, per_block = "profiles/select_neighbours.json", 9, 4.0, None
while argv[:1] and argv[0].startswith("--"):
    if argv[0] == "--out":
        out_path = argv[1]
    elif argv[0] == "--reps":
        reps = int(argv[1])
    elif argv[0] == "--leg-seconds":
        leg_seconds = float(argv[1])
    elif argv[0] == "--pairs-per-block":
        per_block = int(argv[1])
    else:
        sys.exit(__doc__)
    argv = argv[2:]
wl = argv[0] if argv else "C3"
n, W, H, _ = WORKLOADS[wl]
limit = None if per_block is None else per_block * ((n + 255) // 256)          # (None: the binding's default)

R = splat_amd.Renderer()
# the camera stands still and the call only reads, so the frames between the calls would be composited from retained lists and
# K1 would not run: retention is off here, so that every frame bins and the K1 yardstick is a frame's
R.set_option(splat_amd._lib.OPT_RETAIN_LISTS, 0)
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


# the radii: from the nearest-neighbour distances of a sample
rng = np.random.default_rng(1)
pos = np.ascontiguousarray(g.positions[:, :3], np.float32)
sample = rng.choice(n, size=min(256, n), replace=False)
nearest = np.full(len(sample), np.inf, np.float32)
for j0 in range(0, n, 1 << 16):
    d = pos[sample, None, :] - pos[None, j0:j0 + (1 << 16), :]
    d2 = (d * d).sum(2)
    hit = (sample[:, None] == np.arange(j0, min(n, j0 + (1 << 16)))[None, :])
    d2[hit] = np.inf
    nearest = np.minimum(nearest, d2.min(1))
nn = float(np.median(np.sqrt(nearest)))
radii = [nn, 2.0 * nn, 4.0 * nn]

selection = device_array(np.zeros(n, np.uint8))
mask_h = (rng.random(n) < 0.1).astype(np.uint8)
mask = device_array(mask_h)

for _ in range(3):                                    # key buffers and per-tile arrays: made before the clock starts
    R.render_frame_device(cam_c, image, sync=True)
R.timing(reset=True)
legs = []
too_slow = set()
for radius in radii:
    for masked in (False, True):
        for at_most in (None, 7):
            kind = (masked, at_most)
            leg = {"radius": radius, "radius_in_nn": round(radius / nn, 3), "source": "10_percent_mask" if masked else "all", "at_most": at_most}
            legs.append(leg)
            if kind in too_slow:
                leg["skipped"] = "a smaller radius of this kind took longer than the leg's time limit"
                continue
            times, t_leg = [], time.perf_counter()
            while len(times) < reps and time.perf_counter() - t_leg < leg_seconds:
                for _ in range(8):                    # frames between the calls, as an editor has them
                    R.render_frame_device(cam_c, image, sync=False)
                R.sync()                              # (the call would wait for them itself: not on its clock)
                t0 = time.perf_counter()
                try:
                    k = R.select_neighbours(selection, radius, source=mask if masked else None, at_most=at_most, max_block_pairs=limit)
                except splat_amd.SplatError as e:
                    leg["refused"] = str(e)
                    break
                finally:
                    leg["block_pairs"] = R.block_pairs
                times.append((time.perf_counter() - t0) * 1e3)
                assert leg.setdefault("passed", k) == k
            if times:
                leg.update(call_ms=round(statistics.median(times), 4), call_ms_min=round(min(times), 4), call_ms_max=round(max(times), 4),
                           repetitions=len(times))
                if max(times) > leg_seconds * 1e3:
                    too_slow.add(kind)
R.sync()
ms, frames = R.timing(reset=True)
dropped = R.frames_dropped()
for p in held:
    R.device_free(p)
R.close()

doc = {"what": "wall time of one synchronous splat_select_neighbours_device call on the resident scene, medians of up to %d repetitions "
               "(at most %g s per leg) with frames in between; radii are multiples of nn_median, the median nearest-neighbour distance "
               "of 256 sampled Gaussians; k1_ms_per_frame is the same run's device time of K1 per frame (splat_get_timing; retained lists are "
               "switched off, so that every frame between the calls bins).  "
               "max_block_pairs is %s per block.  Nothing is asserted on these times."
               % (reps, leg_seconds, "the binding's default, 64" if per_block is None else "%d" % per_block),
       "command": "python tools/neighbour_probe.py" + ("" if per_block is None else " --pairs-per-block %d" % per_block), "workload": wl, "n_gaussians": n, "n_blocks": (n + 255) // 256,
       "max_block_pairs": 64 * ((n + 255) // 256) if limit is None else limit, "nn_median": nn, "radii": radii, "source_mask_selected": int(mask_h.sum()),
       "k1_ms_per_frame": round(ms["preprocess"] / frames, 4) if frames else None, "timed_frames": frames, "frames_dropped": dropped,
       "legs": legs}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

#!/usr/bin/env python3
"""What the colour tools cost on a resident scene: splat_eval_colours_device (whole), splat_select_colour_device,
splat_recolour_scene_device and splat_recolour_gaussians_device (1 %, 50 %, 100 % of the Gaussians, in random order) -- and,
beside them in the same run, the route a caller had before: read_indexed of sh, a torch matmul of the 16 coefficients by A^T (the
offset added to band 0) and update_indexed of sh for the same rows; splat_rotate_sh_scene_device, which moves 576 MB where a
whole recolour moves 624 MB; and K1's device time per frame.  All on one context, with the same data, alternated in one run.
usage: colour_probe.py [--out profiles/colour_tools.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians)
Per operation: the wall time of the synchronous call, median over the repetitions.  Nothing is gated: nobody has measured these
kernels before."""
import ctypes as C
import json
import math
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch
import splat_amd
from bench import WORKLOADS, make_scene

argv = sys.argv[1:]
out_path, reps = "profiles/colour_tools.json", 21
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
dev = torch.device("cuda", 0)
# a grade that stays where it is however often it is applied: the identity but for a contrast of 1 + 2^-10 and its inverse, in turn
GRADES = [splat_amd.colour_matrix(contrast=1.0 + 2.0 ** -10), splat_amd.colour_matrix(contrast=1.0 / (1.0 + 2.0 ** -10))]
turn = [0]
t = math.radians(1.0)
ROT = np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]], np.float32)


def grade():
    turn[0] ^= 1
    return GRADES[turn[0]]


rgb_all = torch.empty((n, 3), dtype=torch.float32, device=dev)
sel = torch.zeros(n, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def matmul_route(idx, rows):
    """the same edit without the recolour: 192 B of sh a Gaussian read into compact rows, mapped by torch, written back"""
    m = torch.from_numpy(grade()).to(dev)
    R.read_indexed(idx, sh=rows)
    c = rows.view(-1, 16, 3) @ m[:, :3].T
    o = (m[:, 3] + 0.5 * m[:, :3].sum(1) - 0.5) / 0.28209479177387814
    c[:, 0] += o
    R.update_indexed(idx, sh=c.view(-1, 48).contiguous())


OPS = [("colours_scene", lambda: R.colours(cam_c, out=rgb_all)),
       ("select_colour", lambda: R.select_colour(cam_c, sel, rgb=(0.5, 0.5, 0.5), tolerance=0.2)),
       ("recolour_scene", lambda: R.recolour(grade())),
       ("rotate_sh_scene", lambda: R.rotate_sh(ROT))]
for pct in (1, 50, 100):
    k = n * pct // 100
    idx = torch.from_numpy(np.random.default_rng(pct).choice(n, k, replace=False).astype(np.int32)).to(dev)
    rows = torch.empty((k, 48), dtype=torch.float32, device=dev)
    OPS += [("recolour_indexed_%dpct" % pct, lambda idx=idx: R.recolour(grade(), idx)),
            ("read_matmul_update_sh_%dpct" % pct, lambda idx=idx, rows=rows: matmul_route(idx, rows))]
torch.cuda.synchronize()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


d.upload()
for _ in range(3):                                    # key buffers, per-tile arrays, the inverse order: made before the clock starts
    R.render_frame_device(cam_c, image, sync=True)
for name, fn in OPS:
    fn()
call = {name: [] for name, _ in OPS}
k1 = []
for _ in range(reps):
    for name, fn in OPS:
        call[name].append(timed(fn))
        k1.append(R.render_frame_device(cam_c, image, sync=True, want_stats=True).ms_preprocess)
dropped = R.frames_dropped()
R.device_free(image)
d.free()
R.close()

results = {name: {"call_ms": round(statistics.median(call[name]), 4), "call_ms_min": round(min(call[name]), 4),
                  "call_ms_max": round(max(call[name]), 4)} for name, _ in OPS}
doc = {"what": "wall time of one synchronous call on the resident scene, medians of %d repetitions, the operations alternated in one "
               "run on one context with the same data (a frame of %d x %d between any two); read_matmul_update_sh_* is the route "
               "without the recolour for the same rows (read_indexed of sh, a torch matmul, update_indexed of sh); a whole recolour "
               "moves 416 B a Gaussian, rotate_sh 384 B; k1_ms_per_frame: K1's device time in the frames between the calls"
               % (reps, W, H),
       "command": "python tools/colour_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps,
       "k1_ms_per_frame": round(statistics.median(k1), 4), "frames_dropped": dropped, "operations": results}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

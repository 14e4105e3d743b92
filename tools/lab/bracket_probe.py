#!/usr/bin/env python3
"""How much of a retained frame's exact walk carries the bracket's second state (profiles/proven_starts_ab.txt).
usage: SPLAT_DBG_BRACKET_COUNT=1 python tools/lab/bracket_probe.py [workload=C3] [frames at rest=200]
Renders `frames` asynchronous frames of the bench pose, then statistics frames at rest: with the debug switch set, a statistics
frame composited from retained lists reports the (wave, record) steps walked with both states as n_iter_scan."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch, splat_amd
from bench import WORKLOADS, make_scene
wl = sys.argv[1] if len(sys.argv) > 1 else "C3"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 200
n, W, H, seed = WORKLOADS[wl]
R = splat_amd.Renderer(); g = make_scene(wl); g.compute_cov3d(R); R.upload(g)
img = torch.zeros((H, W), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
cam = splat_amd.Camera(H, W, (0.0, 0.0, 5.0)); cam.update_camera_pose()
p = cam.to_c(0.01, 15)
from splat_amd.renderer import SplatError
for k in range(frames):
    R.render_frame_device(p, img.data_ptr())
    if k == 9 or k == frames - 1:
        # (the first frames of a large scene may outgrow storage sized from nothing: skipped, reported once, sized right after)
        try:
            R.sync()
        except SplatError as e:
            if e.code != splat_amd._lib.ERR_CAPACITY:
                raise
torch.cuda.synchronize()
for k in range(3):
    r0 = R.frames_retained()
    st = R.render_frame_device(p, img.data_ptr(), sync=True, want_stats=True)
    print("%s after %d frames at rest, statistics frame %d (retained: %s): n_iter_scan %d  n_iter_blend %d  scan / blend %.4f  "
          "fallbacks %d  dropped %d" %
          (wl, frames, k, R.frames_retained() > r0, st.n_iter_scan, st.n_iter_blend, st.n_iter_scan / max(st.n_iter_blend, 1),
           st.n_fallback, R.frames_dropped()))
R.close()

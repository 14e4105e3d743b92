#!/usr/bin/env python3
"""Retained lists under rocprofv3 --kernel-trace --stats (profiles/retain_lists_*): C3, asynchronous device-resident frames.
usage: retain_trace.py rest [frames]   -- `frames` frames of the bench pose (the writer is the fourth)
       retain_trace.py move            -- 13 frames, every one 1 degree of yaw on from the last (nothing to retain)
Prints the frames' checksums and, where the library has it, splat_frames_retained."""
import math, sys, time, zlib
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch, splat_amd
from bench import WORKLOADS, make_scene
what = sys.argv[1] if len(sys.argv) > 1 else "rest"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 200
n, W, H, seed = WORKLOADS["C3"]
R = splat_amd.Renderer(); g = make_scene("C3"); g.compute_cov3d(R); R.upload(g)
img = torch.zeros((H, W), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
cam = splat_amd.Camera(H, W, (0.0, 0.0, 5.0)); cam.update_camera_pose()
if what == "move":
    poses = []
    for k in range(13):
        poses.append(cam.to_c(0.01, 15))
        cam.update_yaw_angle(math.radians(1.0)); cam.update_camera_pose()
else:
    poses = [cam.to_c(0.01, 15)] * frames
sums = []
t0 = time.perf_counter()
for k, p in enumerate(poses):
    R.render_frame_device(p, img.data_ptr(), sync=(what == "move"))
    if what == "move":
        sums.append(zlib.crc32(img.cpu().numpy().tobytes()))
R.sync(); torch.cuda.synchronize()
dt = time.perf_counter() - t0
sums.append(zlib.crc32(img.cpu().numpy().tobytes()))
retained = R.frames_retained() if hasattr(R, "frames_retained") else "n/a"
print("%s: %d frames, %.3f ms a frame, %d dropped, retained %s, checksums %s" %
      (what, len(poses), 1e3 * dt / len(poses), R.frames_dropped(), retained, " ".join("%08x" % s for s in sums)))
R.close()

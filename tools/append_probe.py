#!/usr/bin/env python3
"""What adding Gaussians to a resident scene and putting its slots back in order cost: splat_append_gaussians_device of 1 %,
10 % and 100 % of n rows drawn from the same cloud, and splat_reorder_scene_device in two situations -- after an append of 10 %,
and after an indexed transform that moves a random 10 % of the Gaussians by a scene diameter -- and, beside each in the same
run, the route a caller had before: splat_read_scene_device of all four fields into buffers of its own (for the append: with
the new rows copied behind them on the device) and splat_upload_scene_device of those, which frees, allocates and sorts
everything again.  The buffers are made before the clock starts.  Every repetition starts from a fresh device upload of the
whole scene and two frames of it.
usage: append_probe.py [--out profiles/scene_append.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians, 1080p)
Per case: the wall time of the synchronous call(s), median over the repetitions.  For the reorders also K1's device time and
n_blocks_culled of a frame at the benchmark's pose and select_neighbours' block-pair count at the README's smallest radius,
before and after the reorder and after the re-upload.  Nothing is gated: nobody has measured these kernels before."""
import ctypes as C
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import splat_amd
from splat_amd import _lib
from bench import WORKLOADS, make_scene

argv = sys.argv[1:]
out_path, reps = "profiles/scene_append.json", 21
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
RADIUS = 0.026                                            # the README's smallest: the median nearest-neighbour distance of C3
PER = (("positions", 4), ("cov3d", 9), ("opacities", 1), ("sh", 48))

R = splat_amd.Renderer()
g = make_scene(wl)
g.compute_cov3d(R)
d = g.to_device(R)
dx = g.subset(np.random.default_rng(1).permutation(n)).to_device(R)      # the rows to append: any prefix is a draw from the same cloud
cam = splat_amd.Camera(H, W, (0.0, 0.0, 5.0))
cam.update_camera_pose()
cam_c = cam.to_c(0.01, 15)
image = R.device_image(np.zeros((H, W), np.uint32))
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
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


def block_pairs():
    """the ordered pairs of K1 blocks within RADIUS of each other: the call is refused behind the count, nothing is selected"""
    try:
        R.select_neighbours(scratch_sel, RADIUS, max_block_pairs=1)
    except splat_amd.SplatError as e:
        if e.code != _lib.ERR_CAPACITY:
            raise
    return int(R.block_pairs)


# the caller's buffers of the old route: the four fields, sized for twice the scene
cat = {f: device_alloc(4 * per * 2 * n) for f, per in PER}
scratch_sel = device_alloc(2 * n)
extent = g.positions[:, :3].max(0) - g.positions[:, :3].min(0)
diameter = float(np.sqrt((extent.astype(np.float64) ** 2).sum()))
shift = np.array([[1, 0, 0, diameter], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
tenth = n // 10
moved_idx = device_array(np.random.default_rng(2).permutation(n)[:tenth].astype(np.uint32))


def append_rows(m):
    assert R.append(dx.positions, dx.cov3d, dx.opacities, dx.sh, m=m) == n + m


def read_concat_upload(m):
    R.read_device(n=n, **cat)
    for f, per in PER:
        if m:
            assert hip.hipMemcpy(cat[f] + 4 * per * n, getattr(dx, f), 4 * per * m, 3) == 0      # (device to device)
    R.upload_device(cat["positions"], cat["cov3d"], cat["opacities"], cat["sh"], n=n + m)


def read_upload():
    k = R.n
    R.read_device(n=k, **cat)
    R.upload_device(cat["positions"], cat["cov3d"], cat["opacities"], cat["sh"], n=k)


def start():
    d.upload()
    k1_frame()
    k1_frame()


APPENDS = [("append_%dpct" % pct, n * pct // 100) for pct in (1, 10, 100)]
SITUATIONS = {"after_append_10pct": lambda: append_rows(tenth), "after_moving_10pct": lambda: R.transform(shift, moved_idx, k=tenth)}
results = {name: {"append": [], "reupload": []} for name, _ in APPENDS}
for name in SITUATIONS:
    results[name] = {k: [] for k in ("reorder", "reupload", "moved", "k1_before", "culled_before", "pairs_before", "k1_after", "culled_after",
                                     "pairs_after", "k1_after_reupload", "culled_after_reupload", "pairs_after_reupload")}
for _ in range(reps + 1):                                 # (the first round warms everything up and is not kept)
    for name, m in APPENDS:
        start()
        results[name]["append"].append(timed(lambda: append_rows(m)))
        start()
        results[name]["reupload"].append(timed(lambda: read_concat_upload(m)))
        assert R.n == n + m
    for name, prepare in SITUATIONS.items():
        r = results[name]
        for route in ("reorder", "reupload"):
            start()
            prepare()
            k1_frame()
            before = k1_frame() + (block_pairs(),)
            if route == "reorder":
                moved = []
                r[route].append(timed(lambda: moved.append(R.reorder())))
                r["moved"].append(moved[0])
            else:
                r[route].append(timed(read_upload))
            k1_frame()
            after = k1_frame() + (block_pairs(),)
            if route == "reorder":
                for key, v in zip(("k1_before", "culled_before", "pairs_before"), before):
                    r[key].append(v)
                for key, v in zip(("k1_after", "culled_after", "pairs_after"), after):
                    r[key].append(v)
            else:
                for key, v in zip(("k1_after_reupload", "culled_after_reupload", "pairs_after_reupload"), after):
                    r[key].append(v)
dropped = R.frames_dropped()
R.device_free(image)
for p in held:
    R.device_free(p)
d.free()
dx.free()
R.close()


def med(v):
    return round(statistics.median(v[1:]), 4)


cases = {}
for name, m in APPENDS:
    r = results[name]
    cases[name] = {"m": m, "n_after": n + m, "append_ms": med(r["append"]), "append_ms_min": round(min(r["append"][1:]), 4),
                   "append_ms_max": round(max(r["append"][1:]), 4), "read_concat_upload_ms": med(r["reupload"]),
                   "read_concat_upload_ms_min": round(min(r["reupload"][1:]), 4)}
for name in SITUATIONS:
    r = results[name]
    cases["reorder_" + name] = {"n": n + tenth if "append" in name else n, "slots_moved": int(med(r["moved"])),
                                "reorder_ms": med(r["reorder"]), "reorder_ms_min": round(min(r["reorder"][1:]), 4),
                                "reorder_ms_max": round(max(r["reorder"][1:]), 4), "read_upload_ms": med(r["reupload"]),
                                "read_upload_ms_min": round(min(r["reupload"][1:]), 4),
                                "k1_ms_before": med(r["k1_before"]), "k1_ms_after": med(r["k1_after"]), "k1_ms_after_reupload": med(r["k1_after_reupload"]),
                                "n_blocks_culled_before": int(med(r["culled_before"])), "n_blocks_culled_after": int(med(r["culled_after"])),
                                "n_blocks_culled_after_reupload": int(med(r["culled_after_reupload"])),
                                "block_pairs_before": int(med(r["pairs_before"])), "block_pairs_after": int(med(r["pairs_after"])),
                                "block_pairs_after_reupload": int(med(r["pairs_after_reupload"]))}
doc = {"what": "wall time of the synchronous Renderer.append and Renderer.reorder, medians of %d repetitions, each from a fresh device "
               "upload of the whole scene and two frames of %d x %d; read_concat_upload_ms / read_upload_ms: the route without them in the "
               "same run (read_device of four fields + the new rows copied behind them on the device + upload_device, into buffers made "
               "beforehand); k1_ms_*: K1's device time of the second frame before / after; n_blocks_culled_*: that frame's culled K1 blocks; "
               "block_pairs_*: select_neighbours' ordered block pairs within r = %g; the moved tenth is translated by the scene's "
               "diameter (%.3f) along x" % (reps, W, H, RADIUS, diameter),
       "command": "python tools/append_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps, "frames_dropped": dropped,
       "cases": cases}
print(json.dumps(doc, indent=1))
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")

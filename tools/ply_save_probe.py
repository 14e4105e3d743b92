#!/usr/bin/env python3
"""What saving a resident scene costs: Renderer.encode_ply_rows for the whole scene and by index (1 %, 50 %, 100 % of the
Gaussians, ascending and in random order), Renderer.save_ply end to end (the file write included) -- and, beside them in the
same run, the route a user had before: read_device, the download, numpy.linalg.eigh, the logs, write_ply.
usage: ply_save_probe.py [--out profiles/ply_save.json] [--reps 21] [workload]     (default: C3, 1.5 M Gaussians)
       ply_save_probe.py --accuracy [--out profiles/ply_save_accuracy.json]         (no GPU: the host compile of the header)
Per operation: the wall time of the synchronous call, median over the repetitions (the numpy route: over 3, it takes
seconds).  --accuracy: per covariance class of tests/ply_encode_cases.py the worst e(S) = max|S' - S| / ||S||_F, in units of
2^-24, of the header's chain and of the float64 numpy.linalg.eigh reference, both through the loader
(tests/test_ply_encode_math_host.py asserts header <= 2 x reference).  Nothing is gated here."""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np

argv = sys.argv[1:]
out_path, reps, accuracy = None, 21, False
while argv[:1] and argv[0].startswith("--"):
    if argv[0] == "--accuracy":
        accuracy = True
        argv = argv[1:]
        continue
    if argv[0] == "--out":
        out_path = argv[1]
    elif argv[0] == "--reps":
        reps = int(argv[1])
    else:
        sys.exit(__doc__)
    argv = argv[2:]
f32, f64 = np.float32, np.float64


def write(doc, path):
    print(json.dumps(doc, indent=1))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if accuracy:
    import pathlib
    import ply_encode_cases as E
    from test_ply_encode_math_host import encode_rows, loader_cov
    classes = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in E.CLASSES + ("edges",):
            S = E.edge_covariances() if name == "edges" else E.covariances(name)
            logs, _, quat = encode_rows(S)
            rlogs, rquat = E.reference_encode(S)
            ours, ref = loader_cov(logs, quat, pathlib.Path(tmp), name), loader_cov(rlogs, rquat, pathlib.Path(tmp), name + "_ref")
            e, r = E.relative_error(ours, S).max() * 2 ** 24, E.relative_error(ref, S).max() * 2 ** 24
            classes[name] = {"matrices": len(S), "header_worst_e": round(float(e), 3), "float64_eigh_worst_e": round(float(r), 3),
                             "ratio": round(float(e / r), 3)}
    write({"what": "covariance -> PLY row -> what the loader reads back (write_ply, load_from_ply, splat_host_cov3d): worst "
                   "e(S) = max|S' - S| / ||S||_F per class, in units of 2^-24; header: the HOST compile of splat_ply_encode_math.h (the "
                   "device compile gives the same bits: tests/test_gpu_ply_encode.py); float64_eigh: numpy.linalg.eigh, sqrt, log and "
                   "Shepperd in float64, rounded to float32 once",
           "command": "python tools/ply_save_probe.py --accuracy", "classes": classes}, out_path or "profiles/ply_save_accuracy.json")
    sys.exit(0)

import splat_amd
from bench import WORKLOADS, make_scene

wl = argv[0] if argv else "C3"
n, W, H, _ = WORKLOADS[wl]
R = splat_amd.Renderer()
g = make_scene(wl)
g.compute_cov3d(R)
d = g.to_device(R)
d.upload()
held = []


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


def download(p, shape):
    out = np.empty(shape, f32)
    R._check(R._L.splat_device_download(R._h, C.c_void_p(out.ctypes.data), C.c_void_p(p), out.nbytes))
    return out


tmp = tempfile.mkdtemp()
rows = device_alloc(n * 248)
bufs = dict(positions=device_alloc(16 * n), cov3d=device_alloc(36 * n), opacities=device_alloc(4 * n), sh=device_alloc(192 * n))
OPS = [("encode_scene", lambda: R.encode_ply_rows(rows, splat_amd.inria_layout(n)))]
for pct in (1, 50, 100):
    k = n * pct // 100
    idx = np.random.default_rng(pct).choice(n, k, replace=False).astype(np.uint32)
    for order, ix in (("ascending", np.sort(idx)), ("random", idx)):
        a = dict(index=device_array(ix), k=k)
        OPS.append(("encode_indexed_%dpct_%s" % (pct, order), lambda a=a, k=k: R.encode_ply_rows(rows, splat_amd.inria_layout(k), **a)))


def by_hand():
    """what a user does today: everything down, the decomposition and the activations' inverses in numpy, write_ply"""
    R.read_device(n=n, **bufs)
    pos, cov = download(bufs["positions"], (n, 4)), download(bufs["cov3d"], (n, 9))
    op, sh = download(bufs["opacities"], (n,)), download(bufs["sh"], (n, 48))
    lam, V = np.linalg.eigh(cov.astype(f64).reshape(n, 3, 3))
    V[np.linalg.det(V) < 0, :, 2] *= -1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        logs = (0.5 * np.log(np.maximum(lam, 0.0))).astype(f32)
        logit = np.log(op.astype(f64) / (1.0 - op.astype(f64))).astype(f32)
    # (the trace branch alone: the other three of Shepperd's are left out, which only flatters this route's time)
    w = 0.5 * np.sqrt(np.maximum(1.0 + V[:, 0, 0] + V[:, 1, 1] + V[:, 2, 2], 1e-300))
    q = np.stack([w, (V[:, 2, 1] - V[:, 1, 2]) / (4 * w), (V[:, 0, 2] - V[:, 2, 0]) / (4 * w), (V[:, 1, 0] - V[:, 0, 1]) / (4 * w)], 1).astype(f32)
    raw = {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "opacity": logit}
    raw.update({"scale_%d" % a: logs[:, a] for a in range(3)})
    raw.update({"rot_%d" % a: q[:, a] for a in range(4)})
    raw.update({"f_dc_%d" % a: sh[:, a] for a in range(3)})
    raw.update({"f_rest_%d" % a: sh[:, 3 + a] for a in range(45)})
    splat_amd.write_ply(os.path.join(tmp, "hand.ply"), raw, n)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


for name, fn in OPS[:3]:                              # the inverse order, the allocator's pools: made before the clock starts
    fn()
call = {name: [] for name, _ in OPS}
for _ in range(reps):
    for name, fn in OPS:
        call[name].append(timed(fn))
# the two routes that end in a file, each in a loop of its own: a call that follows 0.2 s of host work finds the GPU's clocks
# down, which is no property of that call
SAVE = "save_ply_scene_with_file_write"
R.save_ply(os.path.join(tmp, "gpu.ply"))
call[SAVE] = [timed(lambda: R.save_ply(os.path.join(tmp, "gpu.ply"))) for _ in range(reps)]
OPS.append((SAVE, None))
hand = [timed(by_hand) for _ in range(min(reps, 3))]
size = os.path.getsize(os.path.join(tmp, "gpu.ply"))
for f in ("gpu.ply", "hand.ply"):
    os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
for p in held:
    R.device_free(p)
d.free()
R.close()

results = {name: {"call_ms": round(statistics.median(call[name]), 4), "call_ms_min": round(min(call[name]), 4),
                  "call_ms_max": round(max(call[name]), 4)} for name, _ in OPS}
results["by_hand_read_download_eigh_logs_write_ply"] = {"call_ms": round(statistics.median(hand), 1), "call_ms_min": round(min(hand), 1),
                                                         "call_ms_max": round(max(hand), 1), "repetitions": len(hand)}
write({"what": "wall time of one synchronous call on the resident scene, medians of %d repetitions, the encode_* operations alternated in one "
               "run on one context, the two routes into a file in loops of their own behind them; encode_*: rows into a device buffer (248-byte INRIA rows); save_ply_*: header, encode into a temporary "
               "device buffer, one copy down, the file write (a %d-byte file in the system's temporary directory); by_hand_*: the "
               "route without the encoder" % (reps, size),
       "command": "python tools/ply_save_probe.py", "workload": wl, "n_gaussians": n, "repetitions": reps, "operations": results},
      out_path or "profiles/ply_save.json")

"""Start refinement at rest on the GPU (SPLAT_OPT_START_REFINE): a camera at rest lets half of the tiles a frame test a
shallower start for their waves' exact walks and keep it where the bracket closes; a probe whose bracket stays open walks
again from the known-good start.  The bracket is proven anew on every frame, so the frames are the ones rendered without
refinement, byte for byte, whatever the probes did -- and once the steps have converged no probe fails any more."""
import ctypes as C
import os

import numpy as np
import pytest

import splat_amd
from oracle import oracle as O
from splat_amd import _lib
from helpers import scene_dict, oracle_camera, image_diff
from bench import WORKLOADS, make_scene

pytestmark = pytest.mark.gpu

FRAMES = 120            # frames at rest per run
RING = 4                # device images in flight between two downloads


def probe_failures(R):
    f = R._L.splat_debug_probe_failures
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]
    n = C.c_uint64()
    assert f(R._h, C.byref(n)) == 0
    return int(n.value)


def run_at_rest(g, W, H, refine, mode=0, frames=FRAMES):
    """`frames` asynchronous frames of the bench pose (RING in flight), every one downloaded; then eight statistics frames.
    Returns (frames, probe failures of the statistics frames, their blend iterations)."""
    R = splat_amd.Renderer(mode=mode) if mode else splat_amd.Renderer()
    try:
        g.compute_cov3d(R)
        R.upload(g)
        R.set_option(_lib.OPT_START_REFINE, refine)
        cam = splat_amd.Camera(H, W, (0.0, 0.0, 5.0))
        cam.update_camera_pose()
        c = cam.to_c(0.01, 15)
        imgs = [R.device_image(np.zeros((H, W), np.uint32)) for _ in range(RING)]
        out = []
        for k0 in range(0, frames, RING):
            for img in imgs:
                R.render_frame_device(c, img)
            R.sync()
            out += [R.device_download(img, H, W) for img in imgs]
        fails, blend = [], []
        for k in range(8):                     # every tile's turn, four times over
            st = R.render_frame_device(c, imgs[k % RING], sync=True, want_stats=True)
            fails.append(probe_failures(R))
            blend.append(int(st.n_iter_blend))
            out.append(R.device_download(imgs[k % RING], H, W))
        assert R.frames_dropped() == 0
        for img in imgs:
            R.device_free(img)
        return out, fails, blend
    finally:
        R.close()


@pytest.mark.parametrize("wl", ["C2", "C3"])
def test_refinement_at_rest_changes_no_byte_and_converges(wl):
    n, W, H, seed = WORKLOADS[wl]
    g = make_scene(wl)
    on, fails_on, blend_on = run_at_rest(g, W, H, 1)
    off, fails_off, blend_off = run_at_rest(g, W, H, 0)
    assert len(on) == len(off) >= 100
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a, b), (wl, k, int((a != b).sum()))
    assert fails_off == [0] * 8
    assert fails_on == [0] * 8, fails_on            # converged: no probe fails any more
    assert sum(blend_on) <= sum(blend_off), (blend_on, blend_off)
    ref, _ = O.render(scene_dict(g), oracle_camera(_bench_cam(W, H), 0.01), nthreads=os.cpu_count() or 8)
    mx, cnt = image_diff(on[-1], ref)
    assert mx <= 1 and cnt <= 1e-4 * W * H, (wl, mx, cnt)


def test_refinement_in_libm_exp_mode_is_the_oracle_bit_for_bit():
    n, W, H, seed = WORKLOADS["C3"]
    g = make_scene("C3")
    frames, fails, _ = run_at_rest(g, W, H, 1, mode=splat_amd.MODE_LIBM_EXP, frames=48)
    ref, _ = O.render(scene_dict(g), oracle_camera(_bench_cam(W, H), 0.01), nthreads=os.cpu_count() or 8)
    for k in (len(frames) - 9, len(frames) - 1):
        assert np.array_equal(frames[k], ref), (k, image_diff(frames[k], ref))


def _bench_cam(W, H):
    cam = splat_amd.Camera(H, W, (0.0, 0.0, 5.0))
    cam.update_camera_pose()
    return cam

"""The reprojection's device pass (csrc/frt_accum.hip: k_accum_reproject) against the host pass, which is its definition
(host/frt_reproject.c; pinned against a numpy reference in test_reproject_cpu.py): bit for bit on the cases of that
test, from host arrays and from device tensors, through later adds, and through GpuRenderer.temporal()."""
import numpy as np
import pytest

from conftest import load_scene

import reproject_ref as ref
from reproject_ref import PAIRS, SIZES, get_case

pytestmark = pytest.mark.gpu

SEED = 0x5EED


@pytest.fixture(scope="module")
def rt(built):
    from fast_ray_tracer_amd import runtime
    runtime.host_lib()
    return runtime


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def filled(rt, xs, device):
    acc = rt.Accumulator(xs.shape[1], device=device)
    for x in xs:
        acc.add(x)
    return acc


def counts(st):
    return (st.pixels, st.reprojected, st.missed, st.no_history)


def host_result(rt, c, extra):
    """The host pass on a case: (resolve after the reprojection, resolve after `extra` more adds, stats)."""
    src, dst = filled(rt, c["xs"], None), filled(rt, c["xs"][:1] + 2.0, None)
    try:
        st = rt.reproject(dst, src, c["prev"], c["pfeat"], c["cur"], c["cfeat"], c["params"], stats=True)
        first = dst.resolve(stats=True)
        for x in extra:
            dst.add(x)
        return first, dst.resolve(stats=True), st
    finally:
        src.close()
        dst.close()


@pytest.mark.parametrize("name", PAIRS)
@pytest.mark.parametrize("w,h", SIZES)
def test_device_pass_is_the_host_pass(rt, w, h, name):
    """The sizes around one wave's width and one block's height, and 3 x 17 blocks with ragged edges; every camera
    pair of the host test. From host arrays and from device tensors; the destination's earlier samples are gone; one
    more add shows the m2 of the pixels whose count is 1."""
    import torch
    c = get_case(rt, w, h, name)
    extra = c["xs"][1:2]
    (want_mean, want_var, want_rst), (want_mean2, want_var2, _), hst = host_result(rt, c, extra)
    src, dst = filled(rt, c["xs"], 0), filled(rt, c["xs"][::-1][:3] + 1.0, 0)
    try:
        st = rt.reproject(dst, src, c["prev"], c["pfeat"], c["cur"], c["cfeat"], c["params"], stats=True)
        mean, var, rst = dst.resolve(stats=True)
        assert _same_bits(mean, want_mean) and _same_bits(var, want_var)
        assert counts(st) == counts(hst) and st.device == 0 and st.kernel_ms > 0
        assert (rst.frames, rst.skipped) == (want_rst.frames, 0)
        for x in extra:
            dst.add(x)
        mean, var = dst.resolve()
        assert _same_bits(mean, want_mean2) and _same_bits(var, want_var2)
        # from device tensors, into a destination that holds the result of the round above
        tensors = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in c["pfeat"] + c["cfeat"]]
        torch.cuda.synchronize()
        ptrs = [t.data_ptr() for t in tensors]
        st = rt.reproject(dst, src, c["prev"], (ptrs[0], ptrs[1]), c["cur"], (ptrs[2], ptrs[3]), c["params"],
                          stats=True)
        mean, var = dst.resolve()
        assert _same_bits(mean, want_mean) and _same_bits(var, want_var)
        assert counts(st) == counts(hst) and st.kernel_ms > 0
        for t, a in zip(tensors, c["pfeat"] + c["cfeat"]):  # (the features are left alone)
            assert np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8))
        # and the source
        smean, svar = src.resolve()
        hsrc = filled(rt, c["xs"], None)
        try:
            hmean, hvar = hsrc.resolve()
        finally:
            hsrc.close()
        assert _same_bits(smean, hmean) and _same_bits(svar, hvar)
    finally:
        src.close()
        dst.close()


def test_adds_continue_from_the_reprojected_state(rt):
    c = get_case(rt, 130, 67, "pan")
    extra = c["xs"][2:4]
    _, (want_mean, want_var, want_rst), _ = host_result(rt, c, extra)
    src, dst = filled(rt, c["xs"], 0), rt.Accumulator(130 * 67, device=0)
    try:
        rt.reproject(dst, src, c["prev"], c["pfeat"], c["cur"], c["cfeat"], c["params"])
        for x in extra:
            dst.add(x)
        mean, var, rst = dst.resolve(stats=True)
        assert _same_bits(mean, want_mean) and _same_bits(var, want_var)
        assert (rst.frames, rst.skipped) == (want_rst.frames, want_rst.skipped) and rst.frames == 2 + 2
    finally:
        src.close()
        dst.close()


def test_refusals_on_the_device(rt):
    c = get_case(rt, 65, 3, "pan")
    src, dst, host = filled(rt, c["xs"], 0), filled(rt, c["xs"][:2], 0), filled(rt, c["xs"][:2], None)
    small = rt.Accumulator(65 * 3 - 1, device=0)
    try:
        before = dst.resolve()

        def refused(match, d=dst, s=src, params=None, pf=c["pfeat"]):
            with pytest.raises(RuntimeError, match=match):
                rt.reproject(d, s, c["prev"], pf, c["cur"], c["cfeat"], params)
            after = dst.resolve(stats=True)
            assert _same_bits(after[0], before[0]) and _same_bits(after[1], before[1]) and after[2].frames == 2

        refused("destination is the source", s=dst)
        refused("different devices", d=host)
        refused("different devices", s=host)
        refused("npixels", s=small)
        refused("normal_cos", params={"normal_cos": float("nan")})
        refused("max_history", params={"max_history": 0})
    finally:
        for a in (src, dst, host, small):
            a.close()


def _moved(scene):
    """The cornell box from a little to the right of its own camera and a step nearer (its box is 3 across, its eye
    2.75 away, on the face of the slab that closes the room behind it: a view moved sideways alone starts inside)."""
    return scene.view((0.12, 0.03, -2.6), (0.0, 0.0, 0.0))


def test_temporal_accumulator_is_the_composition_by_hand(rt):
    """cornell_shipped_48_4x4: two frames at the scene's view, then one at a moved view. The result at the moved view
    is the host composition of the TemporalAccumulator's docstring, bit for bit, whatever the batch size."""
    scene = load_scene("cornell_shipped_48_4x4")
    view = _moved(scene)
    r = rt.GpuRenderer(scene)
    h, w = scene.height, scene.width
    a, b = rt.Accumulator((h, w), device=None), rt.Accumulator((h, w), device=None)
    try:
        feats_a = r.render_features(seed=SEED)
        for k in range(2):
            a.add(r.render(seed=SEED + k))
        want_a = a.resolve()
        r.set_camera(view)
        feats_b = r.render_features(seed=SEED + 2)
        hst = rt.reproject(b, a, scene, feats_a, view, feats_b, stats=True)
        b.add(r.render(seed=SEED + 2))
        want_b = b.resolve()
        assert hst.reprojected > 0 and hst.no_history > 0
        for batch in (0, 4096):
            t = r.temporal(seed=SEED)
            try:
                got_a = t.render(scene, frames=2, batch_samples=batch)
                assert _same_bits(got_a[0], want_a[0]) and _same_bits(got_a[1], want_a[1])
                mean, var, info = t.render(view, frames=1, batch_samples=batch, stats=True)
                assert _same_bits(mean, want_b[0]) and _same_bits(var, want_b[1])
                rp = info["reproject"]
                assert (rp["reprojected"], rp["missed"], rp["no_history"]) == (hst.reprojected, hst.missed,
                                                                              hst.no_history)
                assert rp["kernel_ms"] > 0 and info["first_frame"] == 2 and info["restarts"] == 0
                assert info["frame"].errors == 0
            finally:
                t.close()
        print("cornell_shipped_48_4x4 moved: %d reprojected, %d without history, %d missed"
              % (hst.reprojected, hst.no_history, hst.missed))
    finally:
        a.close()
        b.close()
        r.close()


def test_temporal_deterministic_scene_identical_view(rt):
    """checkered_sphere_200 has nothing stochastic: a second call under the same view finds history everywhere,
    leaves the mean within reproject_ref.identity_bound of the frame, and the variance at 0."""
    scene = load_scene("checkered_sphere_200")
    r = rt.GpuRenderer(scene)
    try:
        frame = r.render(seed=SEED)
        depth = r.render_features(seed=SEED)["depth"]
        t = r.temporal(seed=SEED)
        try:
            t.render(scene)
            mean, var, info = t.render(scene, stats=True)
        finally:
            t.close()
        rp = info["reproject"]
        valid = depth > 0
        assert rp["no_history"] == 0 and rp["reprojected"] == valid.sum() > 0
        cam = rt.flat_camera(scene)
        bound = ref.identity_bound(scene.width, scene.height, frame, 5.0, float(depth[valid].min()),
                                   cam.canvas_distance / cam.pixel_size)
        moved = float(np.abs(mean - frame)[valid].max())
        print("checkered_sphere_200 under the same view: the mean moves by %.3e (bound %.3e)" % (moved, bound))
        assert moved <= bound
        assert not var[..., :3].any() and (var[..., 3][valid] == 2.0).all()
    finally:
        r.close()


def test_temporal_restart_and_denoise_guard(rt):
    scene = load_scene("cornell_shipped_48_4x4")
    r = rt.GpuRenderer(scene)
    try:
        want = r.render_accumulated_denoised(2, seed=SEED)
        t = r.temporal(seed=SEED)
        try:
            with pytest.raises(ValueError, match="frames >= 2"):
                t.render(scene, frames=1, denoise=True)
            mean, var, info = t.render(scene, frames=2, denoise=True, stats=True)
            assert _same_bits(mean, want[0]) and _same_bits(var, want[1]) and info["reproject"] is None
            # a view of another size: the history restarts, and the frame is the one its seed renders
            other = scene.view((0.3, 0.2, -2.0), (0, 0, 0), hsize=40, vsize=32)
            mean, var, info = t.render(other, frames=1, stats=True)
            assert info["restarts"] == 1 and info["reproject"] is None and info["first_frame"] == 2
            assert mean.shape == (32, 40, 4) and (var[..., 3] == 1.0).all() and not var[..., :3].any()
            assert _same_bits(mean, r.render(seed=SEED + 2))
            # and on from there, in the new size
            mean, var, info = t.render(other, frames=1, stats=True)
            assert info["restarts"] == 1 and info["reproject"]["reprojected"] > 0 and (var[..., 3] <= 2.0).all()
        finally:
            t.close()
    finally:
        r.close()

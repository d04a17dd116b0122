"""Adaptive sampling (p3d_adaptive, include/p3d.h) on the GPU.

Every (pixel, sample) has its own RNG stream and a pixel's samples are added in sample order, so a pixel that stopped
after k samples must hold exactly the bits a plain accumulator (p3d_accum) holds for it after k samples, and with
rel_error = 0 the frame is the one-shot frame."""

import numpy as np
import pytest

from conftest import scene_path
from frame_checks import CORNELL, assert_same_bits, cached_device_scenes
import p3d_amd as p3d

pytestmark = pytest.mark.gpu

device_scene = cached_device_scenes()

SUB_RECT = p3d.Tile(13, 9, 67, 45, 0, 1)  # edges that are not whole 4x4 / 8x8 tiles (scene at 96x64)


def cornell_cfg(accel=p3d.ACCEL_BVH, spp=8, **kw):
    return p3d.pathtrace_config(accel=accel, spp_sqrt=spp, max_depth=20, dof=0, seed=0x5EED, **kw)


def ulp_diff(a, b):
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def rel_err_numpy(state):
    """include/p3d.h "Error metric" in float32, same operations in the same order."""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        S = state["sum"].astype(f)
        n = state["samples"].astype(f)
        Y = (f(0.2126) * S[..., 0] + f(0.7152) * S[..., 1]) + f(0.0722) * S[..., 2]
        m = Y / n
        v = np.fmax((state["sum_y2"] - Y * m) / (n - f(1.0)), f(0.0))
        return (np.sqrt(v / n) / (m + f(1.0e-3))).astype(f)


@pytest.mark.parametrize("accel", [p3d.ACCEL_BVH, p3d.ACCEL_GRID, p3d.ACCEL_NONE])
@pytest.mark.parametrize("tile", ["full", "sub_rect", "stripe"])
def test_zero_threshold_is_the_one_shot_frame(accel, tile):
    dev = device_scene(CORNELL, (96, 64))
    cfg = cornell_cfg(accel, spp=8)
    t = {"full": dev.full_tile(), "sub_rect": SUB_RECT, "stripe": p3d.stripe_tile((96, 64), 1, 2, stripe_h=8)}[tile]
    rgb, hit, u8, _ = dev.render(cfg, tile=t, want_rgb8=True)
    ad = dev.adaptive(cfg, 0.0, min_samples=2, tile=t)
    try:
        for n in (1, 1, 1, 13, 16, 32):  # one lane per pixel, then four lanes and the in-order ring
            a_rgb, a_hit, a_samples, a_u8, _ = ad.render(n, want_rgb8=True)
            assert ad.active_pixels == t.w * t.h
        assert ad.samples_done == 64
    finally:
        ad.close()
    assert (a_samples == 64).all()
    assert_same_bits((a_rgb, a_hit, a_u8), (rgb, hit, u8), "rel_error 0")


SCHEDULE = [16, 16, 16, 16, 32, 32, 32, 32, 64]  # 256 samples


def stopped_frame(dev, cfg, rel_error, min_samples=16, schedule=SCHEDULE):
    """Adaptive passes with read_state() after each: [(samples done, out, state, active before the pass)]."""
    ad = dev.adaptive(cfg, rel_error, min_samples=min_samples)
    log = []
    try:
        for n in schedule:
            active = ad.active_pixels
            rgb, hit, samples, u8, st = ad.render(n, want_rgb8=True)
            log.append((ad.samples_done, (rgb, hit, samples, u8, st), ad.read_state(), active))
    finally:
        ad.close()
    return log


def threshold_for(dev, cfg, quantile, samples=64):
    """A rel_error that about `quantile` of the pixels are below after `samples` samples (a rule that stops a share)."""
    ad = dev.adaptive(cfg, 0.0, min_samples=2)
    try:
        ad.render(samples)
        return float(np.quantile(ad.read_state()["rel_err"], quantile))
    finally:
        ad.close()


def test_stopped_pixels_hold_the_plain_accumulator_bits():
    dev = device_scene(CORNELL, (128, 128))
    cfg = cornell_cfg(spp=16)
    log = stopped_frame(dev, cfg, threshold_for(dev, cfg, 0.5, samples=256))
    samples = log[-1][1][2]
    early = float((samples < 256).mean())
    assert 0.1 < early < 0.9, "share stopped early %.3f" % early
    acc = dev.accumulator(cfg)
    snaps = {}
    try:
        for n in SCHEDULE:
            rgb, hit, u8, _ = acc.render(n, want_rgb8=True)
            snaps[acc.samples_done] = (rgb, hit, u8)
    finally:
        acc.close()
    rgb, hit, _, u8, _ = log[-1][1]
    for k, (s_rgb, s_hit, s_u8) in snaps.items():
        m = samples == k
        if m.any():
            assert_same_bits((rgb, hit, u8), (s_rgb, s_hit, s_u8), "pixels stopped at %d" % k, where=m)
    assert set(np.unique(samples)) <= set(snaps)


def test_decision_rule():
    dev = device_scene(CORNELL, (96, 64))
    cfg = cornell_cfg(spp=16)
    thr, min_samples = threshold_for(dev, cfg, 0.4), 32
    log = stopped_frame(dev, cfg, thr, min_samples=min_samples)
    assert 0 < int((log[-1][2]["samples"] < 256).sum()) < 96 * 64
    boundaries = {done for done, _, _, _ in log}
    for i, (done, out, state, _) in enumerate(log):
        samples = state["samples"]
        assert np.array_equal(samples, out[2])
        assert set(np.unique(samples)) <= boundaries
        ok = samples >= 2
        ref = rel_err_numpy(state)
        assert (ulp_diff(state["rel_err"][ok], ref[ok]) <= 2).all(), "rel_err off by more than 2 ulp after pass %d" % i
        # the next pass's active pixels are the ones with samples == done; the rule says who those are
        active_next = log[i + 1][3] if i + 1 < len(log) else None
        rendered = samples == done
        should_stop = (samples >= min_samples) & ~np.signbit(ref) & (ref < np.float32(thr))  # include/p3d.h "Decision"
        near = ulp_diff(ref, np.full_like(ref, thr)) <= 2
        still = rendered & ~should_stop
        if active_next is not None:
            lo, hi = int((still & ~near).sum()), int((still | (rendered & near)).sum())
            assert lo <= active_next <= hi
        stopped = samples < done
        assert (samples[stopped] >= min_samples).all()
        if i + 1 < len(log):
            nxt = log[i + 1][2]["samples"]
            cont = nxt > samples  # rendered again in the next pass
            assert not (cont & should_stop & ~near).any(), "a pixel the rule stops took more samples"
            assert not (rendered & ~should_stop & ~near & ~cont).any(), "a pixel the rule keeps stopped"


def test_sum_y2_is_the_sum_of_squared_luminance():
    dev = device_scene(CORNELL, (96, 64))
    cfg = cornell_cfg(spp=4)
    tile = p3d.Tile(40, 24, 16, 16, 0, 1)
    ad = dev.adaptive(cfg, 0.0, min_samples=2, tile=tile)
    prev = np.zeros((16, 16, 3), np.float32)
    y2 = np.zeros((16, 16), np.float64)
    try:
        for _ in range(16):
            ad.render(1)
            st = ad.read_state()
            L = (st["sum"].astype(np.float64) - prev.astype(np.float64))
            y = 0.2126 * L[..., 0] + 0.7152 * L[..., 1] + 0.0722 * L[..., 2]
            y2 += y * y
            prev = st["sum"]
    finally:
        ad.close()
    assert np.allclose(st["sum_y2"], y2, rtol=1e-4, atol=1e-6)


def test_device_form_matches_the_host_form():
    import torch
    dev = device_scene(CORNELL, (96, 64))
    cfg = cornell_cfg(spp=8)
    thr = threshold_for(dev, cfg, 0.4, samples=16)
    host = stopped_frame(dev, cfg, thr, schedule=[16, 16, 32])[-1][1]
    d_rgb = torch.zeros((64, 96, 3), dtype=torch.float32, device="cuda")
    d_hit = torch.zeros((64, 96), dtype=torch.int32, device="cuda")
    d_u8 = torch.zeros((64, 96, 3), dtype=torch.uint8, device="cuda")
    d_samples = torch.zeros((64, 96), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ad = dev.adaptive(cfg, thr)
    with torch.cuda.stream(s):
        for n in (16, 16, 32):
            ad.render_device(n, d_rgb.data_ptr(), d_hit.data_ptr(), d_u8.data_ptr(), d_samples.data_ptr(), stream=s)
    s.synchronize()
    assert dev.status() == 0
    ad.close()
    rgb, hit, samples, u8, _ = host
    assert np.array_equal(d_samples.cpu().numpy().view(np.uint32), samples)
    assert_same_bits((d_rgb.cpu().numpy(), d_hit.cpu().numpy(), d_u8.cpu().numpy()), (rgb, hit, u8), "device form")


def test_counters():
    dev = device_scene(CORNELL, (96, 64))
    cfg = cornell_cfg(spp=8, collect_stats=1)
    log = stopped_frame(dev, cfg, threshold_for(dev, cfg, 0.4, samples=16), schedule=[16, 16, 16, 16])
    total = 0
    for _, out, _, active in log:
        st = out[4]
        assert st.pixels == active
        total += st.rays_primary
    assert total == int(log[-1][1][2].sum())
    assert log[0][3] == 96 * 64


def test_refusals_and_reset():
    dev = device_scene(CORNELL, (96, 64))
    cfg = cornell_cfg(spp=8)
    with pytest.raises(p3d.P3DError) as e:
        dev.adaptive(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, antialiasing=1, spp_sqrt=3), 0.05)
    assert e.value.code == -3
    with pytest.raises(p3d.P3DError) as e:
        dev.adaptive(cornell_cfg(antialiasing=0), 0.05)
    assert e.value.code == -3
    for kw in (dict(rel_error=float("nan")), dict(rel_error=-0.1), dict(rel_error=0.05, min_samples=1),
               dict(rel_error=0.05, min_samples=65), dict(rel_error=0.05, reserved=(0, 1))):
        with pytest.raises(p3d.P3DError) as e:
            dev.adaptive(cfg, **kw)
        assert e.value.code == -1, kw
    ad = dev.adaptive(cfg, 0.05)
    try:
        first = [ad.render(n, want_rgb8=True) for n in (16, 16)]
        with pytest.raises(p3d.P3DError):
            ad.render(33)
        with pytest.raises(p3d.P3DError):
            ad.render(0)
        assert ad.samples_done == 32
        st = ad.read_state()
        assert (st["samples"] == first[-1][2]).all()
        ad.reset()
        assert ad.samples_done == 0 and ad.active_pixels == 96 * 64
        again = [ad.render(n, want_rgb8=True) for n in (16, 16)]
    finally:
        ad.close()
    for a, b in zip(first, again):
        assert np.array_equal(a[2], b[2])
        assert_same_bits((a[0], a[1], a[3]), (b[0], b[1], b[3]), "after reset")


def test_render_adaptive_generator():
    dev = device_scene(scene_path("path_balls.p3f"), (64, 64))
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=8, max_depth=20, seed=21)
    seen = list(dev.render_adaptive(cfg, 16, 0.0))
    assert [s for s, _, _ in seen] == [16, 32, 48, 64]
    rgb, hit, _ = dev.render(cfg)
    last = seen[-1][2]
    assert np.array_equal(last[1], hit) and np.array_equal(last[0].view(np.uint32), rgb.view(np.uint32))
    assert all(active == 64 * 64 for _, active, _ in seen)

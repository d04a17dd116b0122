"""GPU parity: the HIP path (through the C-ABI of include/p3d.h) against the CPU oracle.

Bars (north_star): hit IDs bit-exact; float RGB within 1e-4 per channel.  What is asserted is tighter:
  * P3D_STACK_LITERAL (the default): Whitted frames over the BVH are compared with the oracle in the
    reference-LITERAL semantics — one member hit_stack for the whole frame, zero-weight reflection rays
    traced (the mode in which the oracle reproduces the reference's own frames bit for bit) — and must be
    BIT-IDENTICAL: hit IDs and every colour bit.
  * P3D_STACK_PER_PIXEL (and every path that has no such stack: accel None / UGrid, the path tracer):
    compared with the oracle in the same semantics (hit_stack emptied at every primary sample,
    zero-weight rays skipped); Whitted colours bit-identical up to libm pow() (<= 2e-6), all ray and
    test counters identical query by query.
"""
import os

import numpy as np
import pytest

from conftest import scene_path
from frame_checks import COUNTERS, TOL, _pair, assert_bit_identical, check_whitted, oracle_cfg_like, per_pixel
from oracle import binding as ob
import p3d_amd as p3d

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_GRID, p3d.ACCEL_BVH])
@pytest.mark.parametrize("depth", [0, 1, 4])
def test_whitted_balls_low_256(accel, depth):
    """cfg1 / cfg2 of BASELINE.json at 256x256 (oracle finishes in < 1 s)."""
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    hs.set_resolution(256, 256)
    dev = p3d.DeviceScene(hs, bvh=True, grid=True)
    sc = ob.Scene(scene_path("balls_low.p3f"))
    sc.set_resolution(256, 256)
    _, _, st = check_whitted(dev, sc, p3d.whitted_config(accel=accel, max_depth=depth))
    if accel == p3d.ACCEL_BVH:  # the hand-off really happened: some pixels start on a leftover that changes their first hit
        assert st.handoff_checked > 100 and st.handoff_redone > 10 and 1 <= st.handoff_rounds <= 4


@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_GRID, p3d.ACCEL_BVH])
def test_whitted_triangle_soup(tri5k_path, accel):
    """5000 random triangles, depth 6: scene too big for LDS staging -> global-memory path,
    deep BVH, node stack spill area in use."""
    dev, sc = _pair(tri5k_path, res=(192, 192))
    check_whitted(dev, sc, p3d.whitted_config(accel=accel, max_depth=6), max_stack=True)


@pytest.mark.parametrize("scene,legacy", [("balls_box.p3f", True), ("box.p3f", True), ("mount_low.p3f", True),
                                          ("tri_low.p3f", True), ("balls_medium.p3f", True),
                                          ("path_glass.p3f", False), ("balls_dof.p3f", False)])
@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_GRID, p3d.ACCEL_BVH])
def test_whitted_other_scenes(scene, legacy, accel):
    """aaBox objects, transmissive materials (refraction chain, `inside` rays, zero-weight reflection rays under
    P3D_STACK_LITERAL), legacy `f` lines."""
    dev, sc = _pair(scene_path(scene), res=(160, 160), legacy=legacy)
    check_whitted(dev, sc, p3d.whitted_config(accel=accel, max_depth=5))


def test_empty_scene_renders_background():
    """balls_medium through the shipped parser = 0 objects: every pixel is bclr."""
    dev, sc = _pair(scene_path("balls_medium.p3f"), res=(64, 64), grid=False)
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        rgb, hit, st = dev.render(p3d.whitted_config(accel=accel, max_depth=3, collect_stats=1))
        assert (hit == -1).all()
        assert (rgb == sc.background()[None, None, :]).all()
        assert st.rays == 64 * 64


@pytest.mark.parametrize("kw", [dict(antialiasing=1, spp_sqrt=3), dict(antialiasing=1, spp_sqrt=2, soft_shadows=1),
                                dict(antialiasing=1, spp_sqrt=2, sample_mode=1),
                                dict(antialiasing=1, spp_sqrt=2, depth_of_field=1, sample_disk=1),
                                dict(antialiasing=1, spp_sqrt=2, depth_of_field=1, sample_disk=0)])
def test_whitted_sampling_modes(kw):
    """AA jitter / tent, soft shadows with per-sample light jitter, thin-lens DOF (main.cpp:758-802,180-186).  Under
    P3D_STACK_LITERAL the samples of a pixel hand the stack to each other in order, the last one to the next pixel."""
    dev, sc = _pair(scene_path("balls_dof.p3f" if kw.get("depth_of_field") else "balls_low.p3f"), res=(96, 96))
    check_whitted(dev, sc, p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, seed=77, **kw))


def test_soft_shadows_by_light_replication():
    """!ANTIALIASING && SOFT_SHADOWS: every light becomes SPP x SPP lights (main.cpp:725-745)."""
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    hs.set_resolution(96, 96)
    hs.replicate_lights(3, 0.5)
    sc = ob.Scene(scene_path("balls_low.p3f"))
    sc.set_resolution(96, 96)
    sc.replicate_lights(3, 0.5)
    assert sc.counts()["lights"] == 27
    dev = p3d.DeviceScene(hs, bvh=True, grid=False)
    check_whitted(dev, sc, p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=2, soft_shadows=1), tol=5e-6)


@pytest.mark.parametrize("scene,accel,dof", [("path_balls.p3f", p3d.ACCEL_BVH, 0), ("path_balls.p3f", p3d.ACCEL_NONE, 0),
                                             ("path_mirror.p3f", p3d.ACCEL_BVH, 0), ("path_glass.p3f", p3d.ACCEL_BVH, 0),
                                             ("path_glass.p3f", p3d.ACCEL_GRID, 0), ("path_dof.p3f", p3d.ACCEL_BVH, 1),
                                             ("path_balls_low.p3f", p3d.ACCEL_BVH, 0)])
def test_path_tracer(scene, accel, dof):
    """Radiance (main.cpp:313-516): diffuse + NEE, mirror, dielectric (both-branch and Russian
    roulette), RR termination; same RNG streams and detmath on both sides.  The kernel sums
    radiance outermost-first, the oracle innermost-first: tolerance, not bit equality."""
    dev, sc = _pair(scene_path(scene), res=(96, 96))
    cfg = p3d.pathtrace_config(accel=accel, spp_sqrt=4, max_depth=20, dof=dof, seed=0x5EED, collect_stats=1)
    rgb, hit, st = dev.render(cfg)
    o_rgb, o_hit, o_st = sc.render(oracle_cfg_like(cfg))
    assert (hit == o_hit).all()
    scale = max(1.0, float(np.abs(o_rgb).max()))
    assert np.abs(rgb - o_rgb).max() <= TOL * scale
    # identical paths: every ray class and every test count agrees exactly
    for k in ("rays_primary", "rays_bounce", "rays_light", "node_tests", "sphere_tests", "tri_tests", "shaded_hits"):
        assert getattr(st, k) == getattr(o_st, k), k


@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_GRID, p3d.ACCEL_BVH])
def test_batched_trace_queries(accel, tri5k_path):
    """p3d_trace_closest / p3d_trace_any = BVH::intersect_bvh / bool_intersect_bvh, Grid::Traverse x2
    and the brute-force loops, on random rays incl. axis-parallel and unnormalised directions."""
    rng = np.random.default_rng(5)
    for scene in (scene_path("balls_low.p3f"), tri5k_path, scene_path("path_glass.p3f")):
        dev, sc = _pair(scene)
        n = 4096
        o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
        d = rng.standard_normal((n, 3)).astype(np.float32)
        d[:64, 0] = 0.0          # axis-parallel: 1/0 = inf in the slab test
        d[64:128, 1:] = 0.0
        d[128:1024] *= rng.uniform(0.2, 5, (896, 1)).astype(np.float32)   # unnormalised (Q8)
        hit, hp, t = dev.trace_closest(accel, o, d, want_t=True)
        o_hit, o_t, o_hp = sc.trace_closest(accel, o, d)
        assert (hit == o_hit).all()
        m = hit >= 0
        assert (hp[m].view(np.uint32) == o_hp[m].view(np.uint32)).all()
        assert (t.view(np.uint32) == o_t.view(np.uint32)).all()  # tmin / min_t of the traversal, FLT_MAX on a miss
        occ = dev.trace_any(accel, o, d)
        assert (occ == sc.trace_any(accel, o, d)).all()


def test_stripe_sharding_is_bit_invariant():
    """Multi-GPU partition: any rank count / stripe height gives the same bits.  Under P3D_STACK_LITERAL
    (the default) a stripe's first row starts on what the frame's pixels below it leave on the stack: the stripe
    renders the chain of pixels in front of it (halo_find_kernel) — so stripes and sub-rectangles reproduce the
    full frame, which itself equals the oracle's serial order."""
    dev, sc = _pair(scene_path("balls_low.p3f"), res=(128, 128), grid=False)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3)
    full, full_hit, _ = dev.render(cfg)
    o_rgb, o_hit, _ = sc.render(oracle_cfg_like(cfg))
    assert_bit_identical((full, full_hit), (o_rgb, o_hit), "full frame")
    for world, sh in ((2, 8), (4, 16), (8, 16), (2, 4)):
        out = np.zeros_like(full)
        out_hit = np.zeros_like(full_hit)
        for rank in range(world):
            t = p3d.stripe_tile((128, 128), rank, world, sh)
            rgb, hit, _ = dev.render(cfg, tile=t)
            rows = p3d.stripe_rows((128, 128), rank, world, sh)
            out[rows] = rgb
            out_hit[rows] = hit
        assert (out.view(np.uint32) == full.view(np.uint32)).all() and (out_hit == full_hit).all()
    # sub-rectangle
    t = p3d.Tile(40, 24, 50, 33, 0, 1)
    rgb, hit, _ = dev.render(cfg, tile=t)
    assert (rgb.view(np.uint32) == full[24:57, 40:90].view(np.uint32)).all()
    # path tracer: 8x8 tiles with one lane per pixel (9 spp) and 4x4 tiles with four lanes per pixel (16 spp)
    dev, _ = _pair(scene_path("path_glass.p3f"), res=(64, 64), grid=False)
    for spp_sqrt in (3, 4):
        cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=spp_sqrt, max_depth=12, seed=7)
        full, full_hit, _ = dev.render(cfg)
        for world, sh in ((2, 8), (4, 4), (2, 16)):
            out = np.zeros_like(full)
            out_hit = np.zeros_like(full_hit)
            for rank in range(world):
                rgb, hit, _ = dev.render(cfg, tile=p3d.stripe_tile((64, 64), rank, world, sh))
                rows = p3d.stripe_rows((64, 64), rank, world, sh)
                out[rows] = rgb
                out_hit[rows] = hit
            assert (out.view(np.uint32) == full.view(np.uint32)).all() and (out_hit == full_hit).all()
        rgb, hit, _ = dev.render(cfg, tile=p3d.Tile(10, 6, 37, 29, 0, 1))
        assert (rgb.view(np.uint32) == full[6:35, 10:47].view(np.uint32)).all()


@pytest.mark.parametrize("kw,res,depth", [(dict(), 1024, 4),
                                          (dict(antialiasing=1, spp_sqrt=2, soft_shadows=1, depth_of_field=1), 1024, 4),
                                          (dict(), 2048, 250)])  # 4 KB of level records per thread: 8 launches of 8192 tiles
def test_tile_order_never_changes_a_result(kw, res, depth):
    """p3d_config.tile_order is scheduling only: the frame-order launch, the launch that records the
    tile costs and the launches that use the recorded schedule write the same bits (also with a
    striped tile and with a frame that needs more than one launch)."""
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    hs.set_resolution(res, res)
    dev = p3d.DeviceScene(hs, bvh=True)
    mk = lambda order: p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=depth, tile_order=order, **kw)
    tiles = [None, p3d.stripe_tile((res, res), 1, 2, 8)] if res == 1024 else [None]
    for t in tiles:
        ref = dev.render(mk(p3d.TILE_ORDER_FRAME), tile=t, want_rgb8=True, stats=False)
        for _ in range(3):  # 1st: frame order + cost recording, 2nd and 3rd: scheduled
            out = dev.render(mk(p3d.TILE_ORDER_COST), tile=t, want_rgb8=True, stats=False)
            assert (out[0].view(np.uint32) == ref[0].view(np.uint32)).all()
            assert (out[1] == ref[1]).all() and (out[2] == ref[2]).all()
    # the counters of a scheduled launch are those of the frame-order launch
    a = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=depth, tile_order=p3d.TILE_ORDER_FRAME, collect_stats=1, **kw))[2]
    b = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=depth, tile_order=p3d.TILE_ORDER_COST, collect_stats=1, **kw))[2]
    for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "node_tests", "sphere_tests", "tri_tests",
              "shaded_hits", "pixels"):
        assert getattr(a, k) == getattr(b, k), k
    with pytest.raises(p3d.P3DError) as e:
        dev.render(mk(7))
    assert e.value.code == -1


@pytest.mark.parametrize("scene,legacy", [("balls_low.p3f", False), ("balls_high.p3f", True), ("mount_very_high.p3f", True),
                                          ("tri5k", False), ("path_glass.p3f", False)])
def test_device_built_bvh_finds_the_same_closest_hits(scene, legacy, tri5k_path):
    """p3d_scene_create_device_bvh (linear BVH built on the GPU): not the reference's tree, so only what
    must not depend on the tree is compared — the nearest intersection of batched rays and the
    primary-hit image against the reference-exact BVH, the closest hits also against brute force."""
    path = tri5k_path if scene == "tri5k" else scene_path(scene)
    hs = p3d.HostScene(path, legacy_f11=legacy)
    hs.set_resolution(192, 192)
    exact = p3d.DeviceScene(hs, bvh=True)
    built = p3d.DeviceScene(hs, bvh="device")
    assert built.device_bvh_ms is not None and built.device_bvh_ms > 0
    rng = np.random.default_rng(5)
    n = 40000
    o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    d = (rng.uniform(-1, 1, (n, 3)) - o).astype(np.float32)  # aimed at the middle of the scene
    d[: n // 8, rng.integers(0, 3)] = 0  # axis-parallel directions too
    d /= np.linalg.norm(d, axis=1, keepdims=True)  # unit directions, as the renderer's rays (a raw direction mixes
    #                                                units: the hit point is d * t with d re-normalised on the way, Q8)
    hit_e, p_e = exact.trace_closest(p3d.ACCEL_BVH, o, d)
    hit_b, p_b = built.trace_closest(p3d.ACCEL_BVH, o, d)
    sc = ob.Scene(path, legacy_f11=legacy)
    hit_n, _, p_n = sc.trace_closest(0, o, d)  # the ORACLE's object loop (main.cpp:116-124): a tree-independent answer
    # The three back ends agree except on grazing rays: every sphere test re-normalises the traversal's copy of
    # the ray (Q8), so the direction a later test sees depends on the tests before it — the reference's own BVH
    # and its own brute-force loop disagree on the same handful of rays (4 of 200 000 on balls_high).
    for other in (hit_e, hit_n):
        assert ((other >= 0) != (hit_b >= 0)).mean() < 1e-4
        assert (other != hit_b).mean() < 1e-3
    m = (hit_b >= 0) & (hit_e == hit_b)
    assert m.sum() > n // 100
    # hit points agree to rounding, not to the bit, for the same reason; for a small sphere far from the origin
    # b*b - c cancels (balls_high: 0.2 % of the hits move by ~1e-4 along the ray between ANY two back ends)
    far = np.abs(p_e[m] - p_b[m]).max(-1) > 1e-5 * max(1.0, float(np.abs(p_e[m]).max()))
    assert far.mean() < 1e-2 and np.abs(p_e[m] - p_b[m]).max() < 1e-2
    # primary-hit image and a depth-0 frame (no shadow feelers when there are no lights is not given: compare IDs only)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=0)
    _, img_e, _ = exact.render(cfg)
    _, img_b, _ = built.render(cfg)
    assert (img_e != img_b).mean() < 1e-3  # seams: pixels whose ray meets two objects at exactly the same t
    # the occlusion queries of a CORRECT any-hit would agree; the reference's any-hit (Q1) depends on the tree,
    # so only the trivially tree-independent direction is checked: a ray that hits nothing is not occluded
    occ_b = built.trace_any(p3d.ACCEL_BVH, o, d)
    assert not occ_b[(hit_b < 0) & (hit_n < 0) & (hit_e < 0)].any()


@pytest.mark.parametrize("kw", [dict(spp_sqrt=2), dict(spp_sqrt=3, soft_shadows=1), dict(spp_sqrt=2, soft_shadows=1, depth_of_field=1, sample_disk=0),
                                dict(spp_sqrt=5, sample_mode=p3d.SAMPLE_TENT)])
def test_antialiased_whitted_over_a_scene_traversed_from_l2(kw, tri5k_path):
    """Anti-aliased Whitted over a scene too big for LDS.  P3D_STACK_PER_PIXEL takes the four-lanes-per-pixel kernel
    (4x4-pixel tiles, samples handed out by ticket, summed in sample order by lane 0 of the pixel): same bits as the
    oracle's sequential sample loop, counters included.  P3D_STACK_LITERAL keeps one lane per pixel (the samples hand
    the stack to each other in order) and must equal the oracle's serial order bit for bit.  Both invariant under
    striping / sub-rectangles."""
    dev, sc = _pair(tri5k_path, res=(96, 80), grid=False)
    lit = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, antialiasing=1, seed=11, **kw)
    check_whitted(dev, sc, lit, tol=5e-6, counters=("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "node_tests",
                                                    "tri_tests", "shaded_hits", "pixels"))
    for cfg in (lit, per_pixel(lit)):
        cfg.collect_stats = 0
        full, full_hit, _ = dev.render(cfg)
        for world, sh in ((2, 8), (4, 4)):
            out, out_hit = np.zeros_like(full), np.zeros_like(full_hit)
            for rank in range(world):
                a, b, _ = dev.render(cfg, tile=p3d.stripe_tile((96, 80), rank, world, sh))
                rows = p3d.stripe_rows((96, 80), rank, world, sh)
                out[rows], out_hit[rows] = a, b
            assert (out.view(np.uint32) == full.view(np.uint32)).all() and (out_hit == full_hit).all()
        a, _, _ = dev.render(cfg, tile=p3d.Tile(10, 6, 37, 29, 0, 1))
        assert (a.view(np.uint32) == full[6:35, 10:47].view(np.uint32)).all()


@pytest.mark.parametrize("scene,legacy,res,depth", [("tri5k", False, (192, 160), 6), ("balls_high.p3f", True, (160, 160), 4)])
def test_chain_per_level_launches_write_the_same_bits(scene, legacy, res, depth, tri5k_path):
    """p3d_config.chain_launch = P3D_CHAIN_PER_LEVEL (one launch per chain level, child rays compacted into a queue
    and binned by origin cell + direction octant between levels): same queries in the same per-pixel order as the
    megakernel, so the same bits and the same counters, under both stack modes, also for a striped tile (the halo
    chains ride on the level-0 launch); and the literal frame equals the oracle's serial order."""
    dev, sc = _pair(tri5k_path if scene == "tri5k" else scene_path(scene), res=res, legacy=legacy, grid=False)
    for mode in (p3d.STACK_LITERAL, p3d.STACK_PER_PIXEL):
        mega = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=depth, stack_mode=mode, chain_launch=p3d.CHAIN_MEGAKERNEL, collect_stats=1)
        level = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=depth, stack_mode=mode, chain_launch=p3d.CHAIN_PER_LEVEL, collect_stats=1)
        a_rgb, a_hit, a_st = dev.render(mega)
        b_rgb, b_hit, b_st = dev.render(level)
        assert (a_rgb.view(np.uint32) == b_rgb.view(np.uint32)).all() and (a_hit == b_hit).all()
        for k in COUNTERS + ("max_stack", "handoff_checked", "handoff_redone"):
            assert getattr(a_st, k) == getattr(b_st, k), k
        t = p3d.stripe_tile(res, 1, 2, 8)
        rows = p3d.stripe_rows(res, 1, 2, 8)
        s_rgb, s_hit, _ = dev.render(level, tile=t)
        assert (s_rgb.view(np.uint32) == a_rgb[rows].view(np.uint32)).all() and (s_hit == a_hit[rows]).all()
        if mode == p3d.STACK_LITERAL:
            o_rgb, o_hit, _ = sc.render(oracle_cfg_like(level))
            assert_bit_identical((b_rgb, b_hit), (o_rgb, o_hit), "per-level launches, literal hit_stack")
    with pytest.raises(p3d.P3DError) as e:  # not for a scene that is staged in LDS
        small, _ = _pair(scene_path("balls_low.p3f"), res=(64, 64), grid=False)
        small.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=2, chain_launch=p3d.CHAIN_PER_LEVEL))
    assert e.value.code == -3


def test_literal_hand_off_across_several_launches():
    """A frame whose per-thread scratch forces several launches (MAX_DEPTH 1000: 16 KB of level records per thread,
    512x512 pixels): the hand-off records are numbered over the whole tile, the check and the work lists run once after
    the last band — the frame must still be the oracle's serial order bit for bit, counters included."""
    dev, sc = _pair(scene_path("balls_low.p3f"), res=(512, 512), grid=False)
    check_whitted(dev, sc, p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=1000))


def test_sample_loop_backstop_is_an_error_not_a_darker_pixel():
    """The four-lanes-per-pixel kernels hand samples out by ticket inside a wave-uniform loop with a trip bound as
    backstop.  A pixel that ran into the bound would be written with samples missing: the kernel raises a flag and
    the call fails with P3D_ERR_CAPACITY (forced here through the debug trip bound)."""
    dev, _ = _pair(scene_path("path_balls.p3f"), res=(64, 64), grid=False)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=4, max_depth=12, seed=3)
    good, _, _ = dev.render(cfg)
    try:
        dev.debug_limits(trip_bound=5)
        with pytest.raises(p3d.P3DError) as e:
            dev.render(cfg)
        assert e.value.code == -4 and "trip bound" in str(e.value)
    finally:
        dev.debug_limits()
    again, _, _ = dev.render(cfg)  # the flag was cleared with the error; the next call is clean
    assert (again.view(np.uint32) == good.view(np.uint32)).all()


@pytest.mark.parametrize("scene,legacy,res", [("balls_low.p3f", False, (256, 256)), ("balls_medium.p3f", True, (128, 128))])
def test_row_starts_are_certified_or_the_call_fails(scene, legacy, res):
    """A stripe or sub-rectangle starts every row that has no predecessor in the tile on the leftover of the frame
    pixels in front of it.  halo_find_kernel walks back to a pixel whose own first closest hit provably does not depend
    on the stack it finds (no primitive of the scene nearer than its hit, direction stable under re-normalisation) and
    renders the chain from there; if it cannot find one among the pixels it may collect, the call FAILS instead of
    returning a frame that is only probably right.  Shrinking that allowance to one pixel makes the detector fire on a
    sphere scene (the pixel right in front of some row is not certifiable); with the real allowance every stripe and
    sub-rectangle is the full frame bit for bit."""
    dev, _ = _pair(scene_path(scene), res=res, legacy=legacy, grid=False)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4)
    full, full_hit, _ = dev.render(cfg)
    tiles = [p3d.stripe_tile(res, rank, 4, 8) for rank in range(4)] + [p3d.Tile(res[0] // 3, res[1] // 4, res[0] // 2, res[1] // 2, 0, 1)]
    fired = []
    for allowance in (1, 2, 3):
        try:
            dev.debug_limits(halo_chain=allowance)
            n = 0
            for t in tiles:
                try:
                    dev.render(cfg, tile=t)
                except p3d.P3DError as e:
                    assert e.code == -4 and "could not be started" in str(e)
                    n += 1
            fired.append(n)
        finally:
            dev.debug_limits()
    assert fired[0] > 0 and fired[0] >= fired[1] >= fired[2], fired  # fewer pixels allowed, more rows that cannot be certified
    for rank in range(4):
        rgb, hit, _ = dev.render(cfg, tile=tiles[rank])
        rows = p3d.stripe_rows(res, rank, 4, 8)
        assert (rgb.view(np.uint32) == full[rows].view(np.uint32)).all() and (hit == full_hit[rows]).all()
    t = tiles[4]
    rgb, hit, _ = dev.render(cfg, tile=t)
    assert (rgb.view(np.uint32) == full[t.y0:t.y0 + t.h, t.x0:t.x0 + t.w].view(np.uint32)).all()
    assert dev.status() == 0


def test_leftover_pool_that_runs_full_fails_or_falls_back_to_dense_records():
    """P3D_STACK_LITERAL keeps what every pixel leaves on the stack.  Compact records (default): a pool of 8 entries per
    pixel on average; dense records: the worst case of every pixel.  A frame that outgrows the pool must not come back
    wrong: the device-buffer call fails (p3d_scene_status), the host-buffer call renders again with dense records by
    itself - and either way the frame is the one the dense records give (forced here by shrinking the pool)."""
    import torch
    dev, sc = _pair(scene_path("balls_low.p3f"), res=(192, 192), grid=False)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4)
    dense = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, handoff_records=p3d.HANDOFF_DENSE)
    want, want_hit, _ = dev.render(dense)
    got, got_hit, _ = dev.render(cfg)
    assert (got.view(np.uint32) == want.view(np.uint32)).all() and (got_hit == want_hit).all()
    o_rgb, o_hit, _ = sc.render(oracle_cfg_like(cfg))
    assert_bit_identical((want, want_hit), (o_rgb, o_hit), "dense records")
    n = 192 * 192
    buf = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    try:
        dev.debug_limits(leftover_pool=2000)  # this frame leaves about 0.3 entries per pixel: 36 864 pixels need far more than that
        dev.render_device(cfg, dev.full_tile(), d_rgb=buf.data_ptr(), d_hit=buf.data_ptr() + n * 12)
        code = dev.status()
        msg = p3d.lib().p3d_last_error().decode()
        again, again_hit, again_st = dev.render(cfg)  # host-buffer call: falls back to dense records when the pool is too small
    finally:
        dev.debug_limits()
    assert code == -4 and "handoff_records" in msg, (code, msg)
    assert again_st.handoff_dense_retry == 1  # ... and says so
    assert (again.view(np.uint32) == want.view(np.uint32)).all() and (again_hit == want_hit).all()
    assert dev.status() == 0


def test_check_over_the_announced_list_equals_the_check_over_the_tiles(tri5k_path):
    """Round 1 of the hit_stack hand-off has two forms.  Dense records (and every LDS-staged scene): the check launch walks the
    tiles.  Compact records over a scene traversed from global memory: pass 1 announces the units that left something and the
    check launch runs over that list (handoff_check_list_kernel).  Same checks, same frame: full frame and a stripe set,
    both against the oracle's serial order, and the same number of checks and redone units in the statistics."""
    dev, sc = _pair(tri5k_path, res=(192, 160), grid=False)
    compact = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, collect_stats=1)
    dense = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, collect_stats=1, handoff_records=p3d.HANDOFF_DENSE)
    o_rgb, o_hit, _ = sc.render(oracle_cfg_like(compact))
    a, a_hit, a_st = dev.render(compact)
    b, b_hit, b_st = dev.render(dense)
    assert_bit_identical((a, a_hit), (o_rgb, o_hit), "check over the list")
    assert_bit_identical((b, b_hit), (o_rgb, o_hit), "check over the tiles")
    assert a_st.handoff_checked == b_st.handoff_checked > 0 and a_st.handoff_redone == b_st.handoff_redone
    for k in ("rays", "node_tests", "tri_tests"):
        assert getattr(a_st, k) == getattr(b_st, k), k
    res = (192, 160)
    for rank in range(2):
        t = p3d.stripe_tile(res, rank, 2, 8)
        rows = p3d.stripe_rows(res, rank, 2, 8)
        for cfg_ in (compact, dense):
            rgb, hit, _ = dev.render(cfg_, tile=t)
            assert (rgb.view(np.uint32) == o_rgb[rows].view(np.uint32)).all() and (hit == o_hit[rows]).all()
    assert dev.status() == 0


def test_tile_schedules_of_different_kernel_variants_do_not_mix(tri5k_path):
    """The recorded tile schedule belongs to a tile GRID: the literal anti-aliased launch works on 8x8-pixel tiles, the
    per-pixel one over a scene traversed from L2 on 4x4 tiles with four lanes per pixel.  Rendering one after the other
    on one scene (found by the round-3 fuzz campaign: the second launch took the first one's schedule and rendered a
    quarter of its tiles) must give each its own frame, first launch (recording) and second (scheduled)."""
    dev, sc = _pair(tri5k_path, res=(192, 160), grid=False)
    kw = dict(antialiasing=1, spp_sqrt=2, soft_shadows=1, seed=9)
    lit = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, collect_stats=1, **kw)
    pp = per_pixel(lit)
    want = {}
    for name, cfg in (("literal", lit), ("per-pixel", pp)):
        want[name] = sc.render(oracle_cfg_like(cfg))
    for round_ in range(2):
        for name, cfg in (("literal", lit), ("per-pixel", pp)):
            rgb, hit, st = dev.render(cfg)
            o_rgb, o_hit, o_st = want[name]
            assert st.rays_primary == o_st.rays_primary == 192 * 160 * 4, (name, round_)
            assert (hit == o_hit).all() and np.abs(rgb - o_rgb).max() <= 5e-6, (name, round_)


def test_hand_off_that_runs_out_of_rounds_is_an_error_also_without_stats():
    """The hit_stack hand-off iterates its work lists to a fixed point; a list that is still not empty after the round
    bound means the frame is not the serial one.  That must fail the call - also on the asynchronous path (device
    buffers, no `stats`), where only p3d_scene_status can tell (forced here through the debug round bound: balls_low at
    256x256 needs its second round)."""
    import torch
    dev, _ = _pair(scene_path("balls_low.p3f"), res=(256, 256), grid=False)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4)
    good, _, st = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, collect_stats=1))
    assert st.handoff_rounds >= 2
    n = 256 * 256
    buf = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    try:
        dev.debug_limits(max_rounds=1)
        with pytest.raises(p3d.P3DError) as e:
            dev.render(cfg)
        assert e.value.code == -4 and "fixed point" in str(e.value)
        dev.render_device(cfg, dev.full_tile(), d_rgb=buf.data_ptr(), d_hit=buf.data_ptr() + n * 12)  # no stats: returns at once
        assert dev.status() == -4 and "fixed point" in p3d.lib().p3d_last_error().decode()
    finally:
        dev.debug_limits()
    assert dev.status() == 0  # read and cleared
    again, _, _ = dev.render(cfg)
    assert (again.view(np.uint32) == good.view(np.uint32)).all()


def test_per_level_literal_small_tile_on_a_fresh_scene(tri5k_path):
    """The work-list launches behind the per-level launches of a LITERAL frame are the megakernel and index their level
    records by launch thread: on a tile of a few hundred pixels that is more columns than the tile has units.  A fresh
    scene (nothing has grown the scratch yet), a 37x29 sub-rectangle: same bits as the megakernel's."""
    hs = p3d.HostScene(tri5k_path)
    hs.set_resolution(128, 128)
    tile = p3d.Tile(40, 50, 37, 29, 0, 1)
    frames = []
    for chain in (p3d.CHAIN_PER_LEVEL, p3d.CHAIN_MEGAKERNEL):
        dev = p3d.DeviceScene(hs, bvh=True)
        rgb, hit, _ = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, chain_launch=chain), tile=tile)
        assert dev.status() == 0
        frames.append((rgb, hit))
    assert (frames[0][0].view(np.uint32) == frames[1][0].view(np.uint32)).all() and (frames[0][1] == frames[1][1]).all()


@pytest.mark.parametrize("n_objs", [0, 1, 2, 3])
def test_device_built_bvh_tiny_scenes(n_objs, tmp_path):
    """Degenerate sizes of the GPU builder: no object (no tree), one (the root is a leaf), two and three."""
    lines = ["bclr 0.1 0.2 0.3", "v", "from 0 -6 1", "at 0 0 0", "up 0 0 1", "angle 40", "hither 0.01", "resolution 64 64",
             "aperture 0", "focal 1", "l 3 -4 5 1 1 1", "f 0.8 0.3 0.3 0.7 1 1 1 0.3 20 0 1 0 0 0"]
    lines += ["s %g 0 0 0.6" % (1.4 * k - 1.4) for k in range(n_objs)]
    path = str(tmp_path / "tiny.p3f")
    open(path, "w").write("\n".join(lines) + "\n")
    hs = p3d.HostScene(path)
    built = p3d.DeviceScene(hs, bvh="device")
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH if n_objs else p3d.ACCEL_NONE, max_depth=2)
    rgb, hit, _ = built.render(cfg)
    ref_rgb, ref_hit, _ = p3d.DeviceScene(hs, bvh=bool(n_objs)).render(cfg)
    assert (hit == ref_hit).all() and sorted(set(np.unique(hit)) - {-1}) == list(range(n_objs))
    assert np.abs(rgb - ref_rgb).max() <= 1e-4  # spheres side by side, no occluder pairs: shadows agree as well; the
    #                                             order of the sphere tests (Q8) moves reflections in the last digits


def test_rgb8_and_gamma():
    dev, sc = _pair(scene_path("balls_low.p3f"), res=(256, 256), grid=False)
    for gamma in (1.0, 2.2):
        cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=2, gamma=gamma)
        rgb, hit, rgb8, _ = dev.render(cfg, want_rgb8=True)
        _, _, o8, _ = sc.render(oracle_cfg_like(cfg), want_rgb8=True)
        assert (rgb8 == o8).all()  # bytes are exact, also after pow(c, 1/GAMMA) (main.cpp:814-815; pow_spec on the device)


def test_errors_are_reported_not_swallowed():
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    dev = p3d.DeviceScene(hs, bvh=False, grid=False)
    with pytest.raises(p3d.P3DError) as e:
        dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=1))
    assert e.value.code == -1
    with pytest.raises(p3d.P3DError):
        dev.render(p3d.whitted_config(accel=p3d.ACCEL_NONE, max_depth=1), tile=p3d.Tile(0, 0, 4096, 8, 0, 1))
    with pytest.raises(p3d.P3DError):
        p3d.HostScene("/nonexistent.p3f")


def test_full_size_cfg2_matches_reference_frame():
    """BASELINE configs[1] at full size: 1024x1024, depth 4, BVH.  Under P3D_STACK_LITERAL the frame must be the
    reference's own frame BIT FOR BIT (tests/golden/survey_probe/cfg2_bvh: full-frame SHA-256, crops, sub-sampled
    frame), rendered by the instantiation bench.py times (no counters) as well as by the counting one.  With the
    per-pixel stack: within 1e-4 of it, and the ray counts equal the reference's (4 944 908 =
    1 048 576 + 3 600 366 + 295 966)."""
    import hashlib
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "survey_probe", "cfg2_bvh.npz"))
    dev, _ = _pair(scene_path("balls_low.p3f"), res=(1024, 1024), grid=False)
    for collect in (0, 1):
        for _ in range(2):  # first launch of a key: frame order + cost recording; second: scheduled tiles
            rgb, hit, st = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, collect_stats=collect))
            assert hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).hexdigest() == str(g["sha256"])
    assert (rgb[::8, ::8].view(np.uint32) == g["sub8"].view(np.uint32)).all()
    for (x0, y0), crop in zip(g["crop_xy"], g["crops"]):
        assert (rgb[y0:y0 + 64, x0:x0 + 64].view(np.uint32) == crop.view(np.uint32)).all()
    assert st.handoff_redone == 9995 and st.handoff_rounds == 2  # what the serial order implies for this frame
    pp = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, stack_mode=p3d.STACK_PER_PIXEL)
    plain, _, _ = dev.render(pp, stats=False)  # the timed instantiation ...
    pp.collect_stats = 1
    rgb, hit, st = dev.render(pp)              # ... writes the bits of the counting one
    assert (plain.view(np.uint32) == rgb.view(np.uint32)).all()
    assert (st.rays_primary, st.rays_shadow, st.rays_reflect, st.rays_refract) == (1048576, 3600366, 295966, 0)
    assert np.abs(rgb[::8, ::8] - g["sub8"]).max() <= TOL
    for (x0, y0), crop in zip(g["crop_xy"], g["crops"]):
        assert np.abs(rgb[y0:y0 + 64, x0:x0 + 64] - crop).max() <= TOL


def test_full_size_tri100k_matches_reference_frame(tri100k_path):
    """The 100k-triangle scene at the survey's 512x512, depth 6: the reference's frame BIT FOR BIT (SHA-256 of the
    whole frame) under P3D_STACK_LITERAL; triangles never re-normalise the ray, so the per-pixel stack gives the
    same bits here."""
    import hashlib
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "survey_probe", "tri100k_bvh_d6.npz"))
    dev, _ = _pair(tri100k_path, grid=False)
    for mode in (p3d.STACK_LITERAL, p3d.STACK_PER_PIXEL):
        rgb, hit, st = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=6, collect_stats=1, stack_mode=mode))
        assert st.rays == 2887776
        assert hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).hexdigest() == str(g["sha256"])


def test_full_size_cfg4_2048_matches_the_oracle_fixture(tri100k_path):
    """BASELINE configs[3] at its real size: 100k triangles, 2048x2048, Whitted depth 6, BVH.  The oracle needs a minute
    for this frame in the reference's serial order, so its answer was recorded once (tests/golden/fullsize/cfg4.npz,
    make_fullsize_fixtures.py): SHA-256 of the float frame and of the hit IDs, every 8th pixel, four crops, all
    counters.  The literal frame must reproduce all of it, with the counting and with the timed instantiation; the
    per-pixel stack gives the same picture here (triangles never re-normalise a ray) with its own test counts."""
    import hashlib
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "fullsize", "cfg4.npz"))
    want = dict(zip([str(k) for k in g["counter_names"]], [int(v) for v in g["counters"]]))
    hs = p3d.HostScene(tri100k_path)
    hs.set_resolution(2048, 2048)
    dev = p3d.DeviceScene(hs, bvh=True)
    for mode in (p3d.STACK_LITERAL, p3d.STACK_PER_PIXEL):
        for collect in (1, 0):
            rgb, hit, st = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=6, collect_stats=collect, stack_mode=mode))
            assert hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).hexdigest() == str(g["sha256_rgb"])
            assert hashlib.sha256(np.ascontiguousarray(hit).tobytes()).hexdigest() == str(g["sha256_hit"])
            if collect and mode == p3d.STACK_LITERAL:
                for k in COUNTERS:
                    assert getattr(st, k) == want[k], k
                assert st.max_stack >= int(g["max_stack"])
            elif collect:
                for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "shaded_hits", "pixels"):
                    assert getattr(st, k) == want[k], k
    assert (rgb[::8, ::8].view(np.uint32) == g["sub8_rgb"].view(np.uint32)).all() and (hit[::8, ::8] == g["sub8_hit"]).all()
    for (x0, y0), crop in zip(g["crop_xy"], g["crops"]):
        assert (rgb[y0:y0 + 64, x0:x0 + 64].view(np.uint32) == crop.view(np.uint32)).all()


@pytest.mark.parametrize("name", ["cfg3", "cfg5"])
def test_full_size_path_tracer_rows_match_the_oracle_fixture(name):
    """BASELINE configs[2] (256 spp) and configs[4] (4096 spp through the thin lens) at 1024x1024: every 8th image row
    at full width and full sampling (a tile with stripe_h = 1, stripe_stride = 8), against what the oracle rendered for
    those rows in the build container (tests/golden/fullsize/<name>.npz: every 8th pixel of them, and the counters
    summed over the rows).  Same paths on both sides: hit IDs and every counter equal, colours within 1e-4 of the HDR scale."""
    from conftest import GOLDEN, ROOT
    g = np.load(os.path.join(GOLDEN, "fullsize", name + ".npz"))
    want = dict(zip([str(k) for k in g["counter_names"]], [int(v) for v in g["counters"]]))
    rows = g["rows"]
    assert (rows == np.arange(0, 1024, 8)).all()
    lens = tuple(float(v) for v in g["lens"]) if float(g["lens"][0]) != 0 else None
    hs = p3d.HostScene(os.path.join(ROOT, "scenes", "cornell.p3f"))
    hs.set_resolution(1024, 1024)
    if lens:
        hs.set_lens(*lens)
    dev = p3d.DeviceScene(hs, bvh=True)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=int(g["spp_sqrt"]), max_depth=20, dof=1 if lens else 0,
                               seed=int(g["seed"]), collect_stats=1)
    rgb, hit, st = dev.render(cfg, tile=p3d.Tile(0, 0, 1024, len(rows), 1, 8))
    assert (hit[:, ::8] == g["sub8_hit"]).all()
    assert np.abs(rgb[:, ::8] - g["sub8_rgb"]).max() <= TOL * max(1.0, float(np.abs(g["sub8_rgb"]).max()))
    for k in ("rays_primary", "rays_bounce", "rays_light", "node_tests", "sphere_tests", "tri_tests", "shaded_hits", "pixels"):
        assert getattr(st, k) == want[k], k


@pytest.mark.parametrize("lens", [None, (10.0, 1.0)])
def test_cornell_path_tracer(lens):
    """BASELINE configs[2]/[4] scene (scenes/cornell.p3f) at reduced size: 64x64, 16 spp; with the
    thin-lens sampler (aperture 10, SAMPLE_DISK) for the configs[4] variant."""
    from conftest import ROOT
    dev, sc = _pair(os.path.join(ROOT, "scenes", "cornell.p3f"), res=(64, 64), grid=False, lens=lens)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=4, max_depth=20, dof=1 if lens else 0, seed=0x5EED,
                               collect_stats=1)
    rgb, hit, st = dev.render(cfg)
    o_rgb, o_hit, o_st = sc.render(oracle_cfg_like(cfg))
    assert (hit == o_hit).all()
    assert np.abs(rgb - o_rgb).max() <= TOL * max(1.0, float(np.abs(o_rgb).max()))
    assert (st.rays_primary, st.rays_bounce, st.rays_light) == (o_st.rays_primary, o_st.rays_bounce, o_st.rays_light)


def test_p3d_render_cli_writes_the_reference_image(tmp_path):
    """The C++ front end (host/main.cpp, what the reference's main() does without the GL window):
    load -> build BVH -> render on the GPU -> save.  The PPM must hold the oracle's u8 frame."""
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "p3d-raytracer_amd", "p3d_render")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "p3d_render"])
    out = str(tmp_path / "frame.ppm")
    r = subprocess.run([exe, scene_path("balls_low.p3f"), "--whitted", "--accel", "bvh", "--depth", "3", "--aa", "0",
                        "--res", "160", "120", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Done:" in r.stdout and "Image file created" in r.stdout
    raw = open(out, "rb").read()
    header, data = raw[:15], raw[15:]
    assert header == b"P6\n160 120\n255\n"
    img = np.frombuffer(data, np.uint8).reshape(120, 160, 3)[::-1]   # file rows are top-down, img_Data bottom-up
    sc = ob.Scene(scene_path("balls_low.p3f"))
    sc.set_resolution(160, 120)
    _, _, o8, _ = sc.render(ob.whitted_config(2, 3, stack_mode=1, trace_zero_weight=1), want_rgb8=True)  # the reference's order
    assert (img == o8).all()
    # and as the PNG that saveImgFile writes (main.cpp:674-689), decoded by an independent reader
    from PIL import Image
    png = str(tmp_path / "RT_Output.png")
    r = subprocess.run([exe, scene_path("balls_low.p3f"), "--whitted", "--accel", "bvh", "--depth", "3", "--aa", "0",
                        "--res", "160", "120", "--out", png], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    im = Image.open(png)
    assert im.size == (160, 120) and im.mode == "RGB"
    assert (np.asarray(im)[::-1] == o8).all()


def test_p3d_render_gpus_goes_through_rccl_and_writes_the_same_image(tmp_path):
    """`p3d_render --gpus N`: the C++ front end deals the rows to N device scenes in 8-row stripes and brings every GPU's
    part to GPU 0 with one ncclGather (RCCL loaded at run time), SURVEY.md 8(e).  This box has one GPU: N = 1 runs the
    same code path (communicator, stripes with stripe_stride 1, gather, de-interleave) and must write the bytes of the
    plain run; N = 2 must say why it cannot run here."""
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "p3d-raytracer_amd", "p3d_render")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "p3d_render"])
    common = [exe, scene_path("balls_low.p3f"), "--whitted", "--accel", "bvh", "--depth", "3", "--aa", "0", "--res", "160", "128"]
    plain, multi = str(tmp_path / "plain.ppm"), str(tmp_path / "multi.ppm")
    r = subprocess.run(common + ["--out", plain], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(common + ["--out", multi, "--gpus", "1", "--verify"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ncclGather" in r.stdout and "Image file created" in r.stdout
    # --verify: float RGB + hit IDs through a second gather, compared bit for bit with the frame GPU 0 renders alone (the binary
    # does the same at N = 8, exit code 3 on a mismatch)
    assert "verify: frame gathered from 1 GPU(s)" in r.stdout and "bit-identical" in r.stdout, r.stdout
    assert open(plain, "rb").read() == open(multi, "rb").read()
    r = subprocess.run(common + ["--out", multi, "--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "HIP device" in r.stderr


@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_GRID, p3d.ACCEL_BVH])
def test_planes_boxes_and_glass(accel):
    """scenes/planes.p3f: `pl` objects (Plane::intercepts scene.cpp:116-137, default [-1,1]^3 bbox in
    BVH/grid, Q12), an aaBox with its face normals (scene.cpp:229-267) and a refracting sphere."""
    from conftest import ROOT
    dev, sc = _pair(os.path.join(ROOT, "scenes", "planes.p3f"), res=(192, 192))
    rgb, hit, st = check_whitted(dev, sc, p3d.whitted_config(accel=accel, max_depth=4))
    if accel == p3d.ACCEL_NONE:
        assert st.plane_tests > 0 and (hit == 0).any() and (hit == 1).any()


@pytest.mark.parametrize("matte,lights", [
    ("0.8 0.7 0.2 0.9  0.3 0.6 0.9 0 40", "0.9 0.8 0.7"),      # Ks = 0: the kernels leave the Blinn power out (capi_scene_layout.hpp material flag)
    ("0.8 0.7 0.2 0.9  0.3 0.6 0.9 0 1e30", "0.9 0.8 0.7"),    # ... also for a shine that drives every power below 1 to zero
    ("0.8 0.7 0.2 0.9  0.3 0.6 0.9 0 0", "0.9 0.8 0.7"),       # ... and for shine 0 (pow(x, 0) = 1, pow(0, 0) = 1)
    ("0.8 0.7 0.2 0.9  0.3 0.6 0.9 -0.0 40", "0.9 0.8 0.7"),   # Ks = -0 compares equal to 0: flagged as well, the products' signs must survive
    ("0.8 0.7 0.2 0.9  0.3 0.6 0.9 0 40", "0.9 -0.8 0.7"),     # a negative light colour: NOT flagged, the power is computed
    ("0.8 0.7 0.2 0.9  0.3 -0.6 0.9 0 40", "0.9 0.8 0.7"),     # a negative specular colour: not flagged
    ("0.8 0.7 0.2 0.9  0.3 0.6 0.9 0 -3", "0.9 0.8 0.7"),      # a negative shine (pow(0, -3) = inf, times Ks = 0 is a NaN): not flagged
])
def test_materials_whose_specular_term_is_multiplied_away(matte, lights, tmp_path):
    """main.cpp:224 computes pow(H.N, shine) for every unshadowed light and main.cpp:232 multiplies the specular sum by Ks.
    For Ks == 0 with well-behaved colours and shine the kernels skip the power (same bits by construction: DESIGN.md section 4,
    experiments r04 section 13); every variant - flagged or not - must still be the oracle's frame bit for bit."""
    path = str(tmp_path / "matte.p3f")
    with open(path, "w") as f:
        f.write("\n".join([
            "bclr 0.1 0.2 0.3", "v", "from 3.2 2.1 1.9", "at 0 0 0.2", "up 0 0 1", "angle 45", "hither 0.01", "resolution 160 128", "aperture 0", "focal 1",
            "l 4 3 5 %s" % lights, "l -3 2 4 0.5 0.6 0.7",
            "f %s 0 1 0 0 0" % matte,
            "p 3", "-3 -3 0", "3 -3 0", "3 3 0", "p 3", "-3 -3 0", "3 3 0", "-3 3 0",
            "s 0.9 -0.4 0.45 0.45",
            "f 0.9 0.9 0.9 0.4  1 1 1 0.6 60 0 1 0 0 0",
            "s 0 0.3 0.5 0.5", "s -0.9 -0.6 0.3 0.3"]) + "\n")
    dev, sc = _pair(path)
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        check_whitted(dev, sc, p3d.whitted_config(accel=accel, max_depth=3))


@pytest.mark.parametrize("name,spp_sqrt,lens,crop", [("cfg3", 16, None, (448, 440, 96, 96)),
                                                     ("cfg5", 64, (10.0, 1.0), (500, 300, 24, 24))])
def test_baseline_path_tracer_configs_at_full_sampling(name, spp_sqrt, lens, crop):
    """BASELINE configs[2] (256 spp) and configs[4] (4096 spp, thin lens) at their real frame size
    (1024x1024) and sample counts, on a crop the oracle can finish: per-channel tolerance 1e-4 of the
    HDR scale, hit IDs exact, every ray/test counter identical (same paths on both sides)."""
    from conftest import ROOT
    dev, sc = _pair(os.path.join(ROOT, "scenes", "cornell.p3f"), res=(1024, 1024), grid=False, lens=lens)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=spp_sqrt, max_depth=20, dof=1 if lens else 0,
                               seed=0x5EED, collect_stats=1)
    x0, y0, w, h = crop
    rgb, hit, st = dev.render(cfg, tile=p3d.Tile(x0, y0, w, h, 0, 1))
    o_rgb, o_hit, o_st = sc.render(oracle_cfg_like(cfg, threads=16), x0, y0, w, h)
    assert (hit == o_hit).all()
    assert np.abs(rgb - o_rgb).max() <= TOL * max(1.0, float(np.abs(o_rgb).max()))
    for k in ("rays_primary", "rays_bounce", "rays_light", "node_tests", "sphere_tests", "tri_tests"):
        assert getattr(st, k) == getattr(o_st, k), k


def _synthetic_skybox(seed=11):
    """Six faces of different sizes, one of them RGBA: smooth gradients + noise so that a wrong face,
    a flipped axis or an off-by-one texel shows up."""
    rng = np.random.default_rng(seed)
    faces = []
    for i, (w, h, bpp) in enumerate([(64, 64, 3), (96, 48, 3), (33, 57, 4), (64, 64, 3), (128, 16, 3), (17, 17, 3)]):
        yy, xx = np.mgrid[0:h, 0:w]
        f = np.zeros((h, w, bpp), np.uint8)
        f[..., 0] = (xx * 255 // max(w - 1, 1)).astype(np.uint8)
        f[..., 1] = (yy * 255 // max(h - 1, 1)).astype(np.uint8)
        f[..., 2] = (40 * i + rng.integers(0, 30, (h, w))).astype(np.uint8)
        faces.append(f)
    return faces


@pytest.mark.parametrize("scene,integrator", [("balls_low.p3f", p3d.WHITTED), ("path_balls.p3f", p3d.PATHTRACE),
                                              ("balls_medium.p3f", p3d.WHITTED)])
@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_BVH])
def test_skybox_miss_shading(scene, integrator, accel):
    """SKYBOX true (constants.h:30): Scene::GetSkyboxColor (scene.cpp:379-457) on every miss, primary
    and secondary (reflections of the sky in the spheres, environment light in the path tracer).
    balls_medium = empty scene: the whole frame is the cubemap."""
    dev, sc = _pair(scene_path(scene), res=(128, 128), grid=False)
    faces = _synthetic_skybox()
    dev.set_skybox(faces)
    sc.set_skybox(faces)
    if integrator == p3d.WHITTED:
        cfg = p3d.whitted_config(accel=accel, max_depth=3, skybox=1)
        tol = 2e-6
    else:
        cfg = p3d.pathtrace_config(accel=accel, spp_sqrt=3, max_depth=20, skybox=1)
        tol = TOL
    rgb, hit, _ = dev.render(cfg)
    o_rgb, o_hit, _ = sc.render(oracle_cfg_like(cfg, skybox=1))
    assert (hit == o_hit).all()
    assert np.abs(rgb - o_rgb).max() <= tol * max(1.0, float(np.abs(o_rgb).max()))
    if scene == "balls_medium.p3f":
        assert (hit == -1).all() and len(np.unique(rgb.reshape(-1, 3), axis=0)) > 500
    # and the switch is really a switch
    plain, _, _ = dev.render(p3d.whitted_config(accel=accel, max_depth=3, skybox=0))
    assert np.abs(plain - rgb).max() > 0.05


def _write_ppm_faces(folder, faces):
    os.makedirs(folder, exist_ok=True)
    for name, f in zip(p3d.SKYBOX_FACE_FILES, faces):  # file rows are top-down, the faces are kept bottom row first
        rgb = np.ascontiguousarray(f[::-1, :, :3])
        with open(os.path.join(folder, name + ".ppm"), "wb") as out:
            out.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
            out.write(rgb.tobytes())


def test_env_line_loads_the_cubemap_when_the_faces_are_there(tmp_path):
    """`env <dir>` (scene.cpp:605-610: LoadSkybox + SetSkyBoxFlg): the loader reads the six faces when the folder holds
    them as binary PPMs (JPEG decoding is DevIL's job in the reference and nobody's here), next to the scene file or in the
    working directory; binding the host scene to the device scene uploads them.  Same frame as handing the faces over
    through p3d_scene_set_skybox; without the folder the scene still loads and has no cubemap."""
    faces = _synthetic_skybox()
    src = open(scene_path("balls_low.p3f")).read()
    assert "env skybox" in src  # the packaged scenes all name the reference's JPEG folder
    scene = tmp_path / "with_env.p3f"
    scene.write_text(src.replace("env skybox", "env sky_ppm"))
    hs_none = p3d.HostScene(str(scene))
    assert not hs_none.has_skybox()
    _write_ppm_faces(str(tmp_path / "sky_ppm"), faces)
    hs = p3d.HostScene(str(scene))
    assert hs.has_skybox()
    hs.set_resolution(96, 96)
    dev = p3d.DeviceScene(hs, bvh=True)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, skybox=1)
    with pytest.raises(p3d.P3DError):
        dev.render(cfg)           # no cubemap on the device yet
    dev.bind_host()
    rgb, hit, _ = dev.render(cfg)
    ref = p3d.DeviceScene(hs, bvh=True)
    ref.set_skybox([f[:, :, :3] for f in faces])
    want, want_hit, _ = ref.render(cfg)
    assert (rgb.view(np.uint32) == want.view(np.uint32)).all() and (hit == want_hit).all()


def test_env_line_and_front_end_decode_the_shipped_jpeg_faces(tmp_path):
    """The reference's default look from C++ alone: `env <dir>` names a folder of JPEG faces (scene.cpp:605-610, 329-377) and
    the library decodes them (host/jpeg_decode.cpp) - same frame, bit for bit, as handing over the faces PIL decodes; and
    `p3d_render --skybox DIR` on the scene as shipped writes the image `p3d_render` writes for the scene whose env line points
    at the folder."""
    import subprocess
    from conftest import GOLDEN, ROOT
    sky = os.path.join(GOLDEN, "skybox")
    src = open(scene_path("balls_low.p3f")).read()
    scene = tmp_path / "with_env.p3f"
    scene.write_text(src.replace("env skybox", "env " + sky))
    hs = p3d.HostScene(str(scene))
    assert hs.has_skybox()
    hs.set_resolution(128, 128)
    dev = p3d.DeviceScene(hs, bvh=True)
    dev.bind_host()
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, skybox=1)
    rgb, hit, _ = dev.render(cfg)
    ref = p3d.DeviceScene(hs, bvh=True)
    ref.set_skybox(p3d.load_skybox_dir(sky))  # PIL
    want, want_hit, _ = ref.render(cfg)
    assert (rgb.view(np.uint32) == want.view(np.uint32)).all() and (hit == want_hit).all()
    plain, _, _ = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3))
    assert (plain != rgb).any()  # the sky is in the picture (in the mirror spheres: the floor fills this view)
    exe = os.path.join(ROOT, "p3d-raytracer_amd", "p3d_render")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "p3d_render"])
    common = ["--whitted", "--accel", "bvh", "--depth", "3", "--aa", "0", "--res", "128", "128"]
    a, b = str(tmp_path / "env.ppm"), str(tmp_path / "flag.ppm")
    r = subprocess.run([exe, str(scene)] + common + ["--out", a], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Skybox face 5: Image sucessfully loaded." in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, scene_path("balls_low.p3f")] + common + ["--skybox", sky, "--out", b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(a, "rb").read() == open(b, "rb").read()
    img = np.frombuffer(open(a, "rb").read()[-128 * 128 * 3:], np.uint8).reshape(128, 128, 3)[::-1]  # file rows are top-down
    assert (img == (np.minimum(rgb * 255.99, 255.0)).astype(np.uint8)).all()  # u8fromfloat at GAMMA 1 (maths.h:81-86)


@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_GRID, p3d.ACCEL_BVH])
def test_debug_views_of_constants_h(accel):
    """TEST_INTERSECT (constants.h:18: every hit is Color(1,0,0), main.cpp:156 and :359) and DEPTH_MAP (constants.h:33:
    grey = remap(5, 20, 1, 0, min_t) clamped, only without an acceleration structure, main.cpp:127-139) as
    p3d_config.debug_view: bit-identical to the oracle, for rayTracing and (TEST_INTERSECT) for the path tracer."""
    dev, sc = _pair(scene_path("balls_low.p3f"), res=(96, 96))
    for view in (p3d.DEBUG_TEST_INTERSECT, p3d.DEBUG_DEPTH_MAP):
        cfg = p3d.whitted_config(accel=accel, max_depth=3, debug_view=view, collect_stats=1)
        rgb, hit, st = dev.render(cfg)
        o_rgb, o_hit, o_st = sc.render(oracle_cfg_like(cfg))
        assert_bit_identical((rgb, hit), (o_rgb, o_hit), "debug view %d" % view)
        assert st.rays == o_st.rays and st.shaded_hits == o_st.shaded_hits
        if view == p3d.DEBUG_TEST_INTERSECT:
            assert (rgb[hit >= 0] == np.array([1, 0, 0], np.float32)).all() and st.rays == 96 * 96 and st.shaded_hits == 0
        elif accel == p3d.ACCEL_NONE:
            assert (rgb[..., 0] == rgb[..., 1]).all() and (rgb[hit < 0] == 0).all() and 0 < rgb.max() <= 1 and st.rays == 96 * 96
        else:  # DEPTH_MAP does nothing with a grid or BVH: the ordinary frame
            plain, _, _ = dev.render(p3d.whitted_config(accel=accel, max_depth=3))
            assert (plain.view(np.uint32) == rgb.view(np.uint32)).all()
    pt = p3d.pathtrace_config(accel=accel, spp_sqrt=3, max_depth=8, seed=5, debug_view=p3d.DEBUG_TEST_INTERSECT)
    dev2, sc2 = _pair(scene_path("path_balls.p3f"), res=(64, 64))
    rgb, hit, _ = dev2.render(pt)
    o_rgb, o_hit, _ = sc2.render(oracle_cfg_like(pt))
    assert (hit == o_hit).all() and np.abs(rgb - o_rgb).max() <= 1e-6


def test_shipped_cubemap_skybox():
    """SKYBOX true with the reference's own cubemap (Raytracing/skybox/*.jpg, kept as data under
    tests/golden/skybox/): Scene::LoadSkybox's six faces decoded by PIL on both sides (DevIL in the reference; the
    decoder and the SHA-256 of the decoded bytes are recorded in decoded.json), Scene::GetSkyboxColor
    (scene.cpp:379-457) on every miss — primary rays that leave the scene and the sky mirrored in the spheres."""
    import hashlib
    import json
    import PIL
    from conftest import GOLDEN
    sky_dir = os.path.join(GOLDEN, "skybox")
    faces = p3d.load_skybox_dir(sky_dir)
    rec = json.load(open(os.path.join(sky_dir, "decoded.json")))
    if PIL.__version__ == rec["PIL"]:  # same decoder build: same texels as when the fixture was recorded
        for name, f in zip(p3d.SKYBOX_FACE_FILES, faces):
            assert hashlib.sha256(np.ascontiguousarray(f[::-1]).tobytes()).hexdigest() == rec["faces"][name]["decoded_rgb_sha256"], name
    dev, sc = _pair(scene_path("balls_low.p3f"), res=(256, 256), grid=False)
    dev.set_skybox(faces)
    sc.set_skybox(faces)
    rgb, hit, _ = check_whitted(dev, sc, p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, skybox=1))
    plain, _, _ = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, skybox=0))
    assert (np.abs(plain - rgb).max(-1) > 0.02).sum() > 500  # the sky shows in the mirror spheres (the floor fills the view)
    empty, esc = _pair(scene_path("balls_medium.p3f"), res=(128, 128), grid=False)  # shipped parser: 0 objects, every pixel is sky
    empty.set_skybox(faces)
    esc.set_skybox(faces)
    e_rgb, e_hit, _ = check_whitted(empty, esc, p3d.whitted_config(accel=p3d.ACCEL_NONE, max_depth=1, skybox=1))
    assert (e_hit == -1).all() and len(np.unique(e_rgb.reshape(-1, 3), axis=0)) > 500  # the sky is a picture
    d = np.random.default_rng(2).standard_normal((4096, 3)).astype(np.float32)
    d[:16] = np.eye(3, dtype=np.float32)[np.arange(16) % 3] * np.where(np.arange(16) % 2, -1, 1)[:, None]  # exact axes
    got = dev.skybox_color(d)
    want = np.stack([sc.skybox_color(v) for v in d])
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_host_class_query_methods_forward_to_the_device(tmp_path):
    """The reference-named query methods of the host classes: Camera::PrimaryRay x2 (host arithmetic,
    camera.h:65-115), Object::intercepts / getNormal, BVH::intersect_bvh / bool_intersect_bvh, Grid::Traverse x2,
    Scene::LoadSkybox + GetSkyboxColor (each ONE query on the bound device scene; the two BVH queries also in their batched
    overloads, n rays in one launch).  tests/host_api_check.cpp calls
    them as code written against the reference would; every record is compared with the oracle, bit for bit."""
    import subprocess
    from PIL import Image
    from conftest import GOLDEN, ROOT
    exe = str(tmp_path / "host_api_check")
    pkg = os.path.join(ROOT, "p3d-raytracer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"),
                           os.path.join(ROOT, "tests", "host_api_check.cpp"), "-L" + pkg, "-lp3d", "-Wl,-rpath," + pkg, "-o", exe])
    ppm_dir = tmp_path / "sky"
    ppm_dir.mkdir()
    small = []
    for name in p3d.SKYBOX_FACE_FILES:  # small faces: the lookup is what is under test here
        img = Image.open(os.path.join(GOLDEN, "skybox", name + ".jpg")).convert("RGB").resize((96, 64))
        img.save(str(ppm_dir / (name + ".ppm")))
        small.append(np.ascontiguousarray(np.asarray(img)[::-1]))
    scene = scene_path("balls_low.p3f")
    r = subprocess.run([exe, scene, str(ppm_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    sc = ob.Scene(scene)
    sc.set_skybox(small)
    f32 = lambda xs: np.array([float.fromhex(x) for x in xs], np.float32)
    same = lambda a, b: (np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)).all()
    seen = {}
    for line in r.stdout.splitlines():
        tag, *v = line.split()
        if tag == "Skybox":  # "Skybox face N: Image sucessfully loaded." (scene.cpp:352)
            continue
        seen[tag] = seen.get(tag, 0) + 1
        if tag == "UNBOUND":
            assert v == ["0", "0", "0"]  # no device scene bound: the queries fail, nothing is computed on the host
        elif tag == "PRIMARY":
            x = f32(v)
            o, d = sc.primary_ray(x[0], x[1])
            lo, ld = sc.primary_ray_lens(x[2], x[3], x[0], x[1])
            assert same(x[4:7], o) and same(x[7:10], d) and same(x[10:13], lo) and same(x[13:16], ld)
        elif tag == "OBJ":
            obj, x, hit, rest = int(v[0]), f32(v[1:7]), int(v[7]), f32(v[8:12])
            h, t, d_after = sc.object_intercepts(obj, x[0:3], x[3:6])
            assert hit == int(h) and same(rest[1:4], d_after)
            assert same(rest[0], np.float32(t)) if h else rest[0] == -1.0
        elif tag == "NORMAL":
            obj, x = int(v[0]), f32(v[1:7])
            assert same(x[3:6], sc.object_normal(obj, x[0:3]))
        elif tag in ("BVH", "GRID"):
            accel = 2 if tag == "BVH" else 1
            x, hid, hp, occ = f32(v[0:6]), int(v[6]), f32(v[7:10]), int(v[10])
            o_hit, _, o_hp = sc.trace_closest(accel, x[None, 0:3], x[None, 3:6])
            assert hid == int(o_hit[0]) and (hid < 0 or same(hp, o_hp[0]))
            assert occ == int(sc.trace_any(accel, x[None, 0:3], x[None, 3:6])[0])
        elif tag == "SKY":
            x = f32(v)
            assert same(x[3:6], sc.skybox_color(x[0:3]))
    # (BVH: 64 single-ray calls + the same 64 rays through the batched overloads, one launch per query kind)
    assert seen == {"UNBOUND": 1, "PRIMARY": 8, "OBJ": 64, "NORMAL": 64, "BVH": 128, "GRID": 64, "SKY": 64}, seen


def test_skybox_requested_without_cubemap_is_an_error():
    dev, _ = _pair(scene_path("balls_low.p3f"), res=(32, 32), grid=False)
    with pytest.raises(p3d.P3DError):
        dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=1, skybox=1))


@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_GRID, p3d.ACCEL_BVH])
def test_axis_parallel_rays_and_nan_semantics(accel):
    """scenes/axis_aligned.p3f: the centre ray is exactly (0,0,-1): inf in 1/d, NaN on slab planes, an
    edge-on triangle (denominator 0 -> inv_denom inf -> NaN t reported as a hit, A10).  The wave that
    holds such a lane must leave the v_max3/v_min3 fast path; results must still equal the oracle's."""
    from conftest import ROOT
    dev, sc = _pair(os.path.join(ROOT, "scenes", "axis_aligned.p3f"))
    o, d = sc.primary_ray(64.5, 64.5)
    assert d[0] == 0.0 and d[1] == 0.0 and d[2] == -1.0
    check_whitted(dev, sc, p3d.whitted_config(accel=accel, max_depth=4))
    # crafted queries: rays inside triangle planes, along box faces and edges, zero direction components
    q_o = np.array([[0, 0, 5], [0, -3, 0.7], [0, 0, 5], [-1, -1, 5], [1, 0.5, 5], [0, 3, 1.0], [-3, 0, -1.5], [0.5, 0.5, 3]], np.float32)
    q_d = np.array([[0, 0, -1], [0, 1, 0], [0, 0, -2], [0, 0, -1], [0, 0, -1], [0, -1, 0], [1, 0, 0], [0, 0, -1]], np.float32)
    g_hit, g_hp = dev.trace_closest(accel, q_o, q_d)
    c_hit, _, c_hp = sc.trace_closest(accel, q_o, q_d)
    assert (g_hit == c_hit).all()
    ok = g_hit >= 0
    assert (np.isnan(g_hp[ok]) == np.isnan(c_hp[ok])).all()
    fin = ok[:, None] & ~np.isnan(c_hp)
    assert (g_hp[fin].view(np.uint32) == c_hp[fin].view(np.uint32)).all()
    assert (dev.trace_any(accel, q_o, q_d) == sc.trace_any(accel, q_o, q_d)).all()


@pytest.mark.parametrize("scene", ["balls_high.p3f", "mount_high.p3f", "mount_very_high.p3f"])
@pytest.mark.parametrize("accel", [p3d.ACCEL_GRID, p3d.ACCEL_BVH])
def test_large_packaged_scenes(scene, accel):
    """the big packaged scenes (7 381 spheres / 2 048 and 32 768 triangles, legacy `f` lines) as
    BVH and grid stress inputs: too large for LDS staging, deep trees, many sphere re-normalisations."""
    dev, sc = _pair(scene_path(scene), res=(160, 160), legacy=True)
    check_whitted(dev, sc, p3d.whitted_config(accel=accel, max_depth=3), max_stack=True)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_random_scenes_whitted(seed, tmp_path):
    """Differential fuzzing: random spheres / triangles / boxes (/ planes for accel None), random opaque,
    reflective and refractive materials, random camera (sometimes with a lens) and lights; every
    accel; depth 5; no-AA and AA+soft-shadow+DOF variants."""
    from fuzz_scenes import random_scene
    path = random_scene(1000 + seed, str(tmp_path / "fuzz.p3f"), n_planes=1 if seed % 3 == 0 else 0)
    dev, sc = _pair(path)
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_GRID, p3d.ACCEL_BVH):
        kw = dict(antialiasing=1, spp_sqrt=2, soft_shadows=1, depth_of_field=1, sample_disk=seed % 2, seed=seed) if seed % 4 == 1 else {}
        check_whitted(dev, sc, p3d.whitted_config(accel=accel, max_depth=5, **kw), tol=5e-6)


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_random_scenes_path_tracer(seed, tmp_path):
    from fuzz_scenes import random_scene
    path = random_scene(2000 + seed, str(tmp_path / "fuzz_pt.p3f"), n_lights=0, emitters=1 + seed % 3, res=(64, 64))
    dev, sc = _pair(path)
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        cfg = p3d.pathtrace_config(accel=accel, spp_sqrt=3, max_depth=12 + seed, dof=seed % 2, seed=seed, collect_stats=1)
        rgb, hit, st = dev.render(cfg)
        o_rgb, o_hit, o_st = sc.render(oracle_cfg_like(cfg))
        assert (hit == o_hit).all(), (seed, accel)
        m = np.isfinite(o_rgb).all(-1)
        assert (np.isfinite(rgb).all(-1) == m).all()
        assert np.abs(rgb[m] - o_rgb[m]).max() <= TOL * max(1.0, float(np.abs(o_rgb[m]).max())), (seed, accel)
        assert (st.rays_primary, st.rays_bounce, st.rays_light) == (o_st.rays_primary, o_st.rays_bounce, o_st.rays_light), (seed, accel)


def test_frames_in_flight_on_several_scenes_render_the_same_bits():
    """What bench.py's timed loop does on one GPU (INTEGRATION.md "several frames in flight"): consecutive frames go
    round-robin to four device scenes on four HIP streams (the default stream + three others), nothing waits until the
    end.  Every frame that comes out of that — literal hand-off with its dependent launches overlapping other frames'
    pass 1, and the per-pixel stack — must be the frame one scene renders on its own, bit for bit; so must the
    device-detected status of every scene."""
    import torch
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    res = 256
    hs.set_resolution(res, res)
    n = res * res
    for mode in (p3d.STACK_LITERAL, p3d.STACK_PER_PIXEL):
        cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, stack_mode=mode)
        alone = p3d.DeviceScene(hs, bvh=True)
        rgb0, hit0, _ = alone.render(cfg)
        nfl = 4
        scenes = [p3d.DeviceScene(hs, bvh=True) for _ in range(nfl)]
        streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(nfl - 1)]
        bufs = [torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for _ in range(nfl)]
        tile = scenes[0].full_tile()
        for i in range(5 * nfl):  # the last round's frames are the ones compared; the earlier ones keep the chip busy
            k = i % nfl
            scenes[k].render_device(cfg, tile, d_rgb=bufs[k].data_ptr(), d_hit=bufs[k].data_ptr() + n * 12, stream=streams[k].cuda_stream)
        torch.cuda.synchronize()
        for k in range(nfl):
            assert scenes[k].status() == 0
            host = bufs[k].cpu().numpy()
            rgb = host[: n * 12].view(np.float32).reshape(res, res, 3)
            hit = host[n * 12:].view(np.int32).reshape(res, res)
            assert (hit == hit0).all(), (mode, k)
            assert (rgb.view(np.uint32) == np.ascontiguousarray(rgb0).view(np.uint32)).all(), (mode, k)


def test_hand_off_launches_on_a_tail_stream_render_the_same_bits(tri5k_path):
    """p3d_scene_set_tail_stream (include/p3d.h), bench.py's default for literal frames: six device scenes, pass 1 of frame i
    on one of two bulk streams, everything behind it on one of two tail streams, nothing waits until the end.  Every frame must
    be the frame one scene renders alone, bit for bit - over an LDS-staged scene (round 0 over the tiles) and over one
    traversed from global memory (check over pass 1's list); p3d_scene_join makes a third stream wait for a frame; a query on
    the scene (null stream) waits by itself; frames with `stats` do not split and still come out the same."""
    import torch
    for path, res, depth in ((scene_path("balls_low.p3f"), 256, 4), (tri5k_path, 128, 3)):
        hs = p3d.HostScene(path)
        hs.set_resolution(res, res)
        n = res * res
        cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=depth)
        alone = p3d.DeviceScene(hs, bvh=True)
        rgb0, hit0, _ = alone.render(cfg)
        nfl = 6
        scenes = [p3d.DeviceScene(hs, bvh=True) for _ in range(nfl)]
        bulk = [torch.cuda.current_stream(), torch.cuda.Stream()]
        tails = [torch.cuda.Stream(), torch.cuda.Stream()]
        for k, sc in enumerate(scenes):
            sc.set_tail_stream(tails[k % 2])
        bufs = [torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for _ in range(nfl)]
        tile = scenes[0].full_tile()

        def frame_of(buf):
            host = buf.cpu().numpy()
            return host[: n * 12].view(np.float32).reshape(res, res, 3), host[n * 12:].view(np.int32).reshape(res, res)

        def same(buf, what):
            rgb, hit = frame_of(buf)
            assert (hit == hit0).all(), what
            assert (rgb.view(np.uint32) == np.ascontiguousarray(rgb0).view(np.uint32)).all(), what
        for i in range(5 * nfl):
            k = i % nfl
            scenes[k].render_device(cfg, tile, d_rgb=bufs[k].data_ptr(), d_hit=bufs[k].data_ptr() + n * 12, stream=bulk[k % 2].cuda_stream)
        # a third stream copies scene 0's frame as soon as that frame - tail included - is done
        side = torch.cuda.Stream()
        scenes[0].join(side)
        with torch.cuda.stream(side):
            copy0 = bufs[0].clone()
        side.synchronize()
        same(copy0, "joined copy")
        torch.cuda.synchronize()
        for k in range(nfl):
            assert scenes[k].status() == 0
            same(bufs[k], k)
        # a split frame, then at once a query on the same scene (null stream): the query waits for the tail by itself
        scenes[1].render_device(cfg, tile, d_rgb=bufs[1].data_ptr(), d_hit=bufs[1].data_ptr() + n * 12, stream=bulk[1].cuda_stream)
        o = np.array([[0.0, 0.0, 5.0]], np.float32)
        d = np.array([[0.0, 0.0, -1.0]], np.float32)
        hit_a, _ = scenes[1].trace_closest(p3d.ACCEL_BVH, o, d)
        hit_b, _ = alone.trace_closest(p3d.ACCEL_BVH, o, d)
        assert (hit_a == hit_b).all()
        scenes[1].join(host_wait=True)
        same(bufs[1], "after the query")
        # with stats the frame stays on the caller's stream (timed as a whole) and is the same frame
        rgb, hit, st = scenes[2].render(cfg)
        assert (hit == hit0).all() and (rgb.view(np.uint32) == np.ascontiguousarray(rgb0).view(np.uint32)).all()
        scenes[3].set_tail_stream(None)
        scenes[3].render_device(cfg, tile, d_rgb=bufs[3].data_ptr(), d_hit=bufs[3].data_ptr() + n * 12, stream=bulk[1].cuda_stream)
        bulk[1].synchronize()
        same(bufs[3], "tail stream switched off")


def test_bench_contract_json_line():
    """bench.py --full prints ONE JSON line with the driver's keys plus `roofline` and `cpu_baseline`.  The headline value is
    the LITERAL frame (bit-identical to the reference's order); the roofline is a bound (frac <= 1 whenever the PMC
    summary of this workload matches the kernel sources, null otherwise — stale counters are not quoted)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "5", "--warmup", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "frame", "per_pixel_stack"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["vs_baseline"] is None
    assert d["config"]["rays_per_frame"] == 4944908 and "workload" in d["config"] and "model" not in d["config"]
    assert d["config"]["stack_mode"] == "literal" and d["frame"]["handoff"]["redone"] == 9995 and d["config"]["frames_in_flight"] == 6 and d["config"]["frames_in_flight_check"].endswith(": ok")
    assert d["config"]["streams"].startswith("2 bulk (pass 1) + 2 tail")  # p3d_scene_set_tail_stream: the default for literal frames
    assert d["frame"]["cold_kernel_ms"] >= d["frame"]["kernel_ms"] * 0.9
    rf = d["roofline"]
    assert rf["bound"] == "valu_issue" and rf["unit"] == "Gwave-instr/s" and abs(rf["peak"] - 1228.8) < 1e-6
    if rf["frac"] is not None:
        assert 0 < rf["frac"] <= 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
        assert 0 < rf["hbm"]["frac"] <= 1.0 and rf["traffic"] > 0
    else:
        assert "PMC summary" in rf["source"]
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and "sample" in cb
    assert cb["one_socket"]["cores"] >= 1 and cb["one_socket"]["value"] > 0
    assert d["value"] > 100 * cb["value"] and d["per_pixel_stack"]["value"] > d["value"]
    # round 3: the single-frame figures next to the throughput, the repeats behind the median, the CPU runs behind theirs
    assert len(d["ms_per_step_repeats"]) >= 5 and min(d["ms_per_step_repeats"]) <= d["ms_per_step"] <= max(d["ms_per_step_repeats"])
    assert abs(d["latency_ms_single_frame"] - d["frame"]["kernel_ms"]) < 1e-9
    assert abs(d["value_single_frame"] - 4944908 / (d["latency_ms_single_frame"] * 1e3)) < 0.01 * d["value_single_frame"]
    assert rf["algorithmic"]["frac_vs_hbm"] > 0 and rf["algorithmic"]["frac_vs_lds"] is not None
    assert len(cb["one_socket"]["runs"]) == 3 and cb["one_socket"]["cores"] <= cb["one_socket"]["logical_cpus"]


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run (no --full) times exactly --steps steps once and prints the headline only; --dump-outputs writes
    the frame of the last timed step, and that frame is, bit for bit, what one scene renders for the same workload."""
    import json
    import subprocess
    import sys
    from conftest import ROOT, SCENES
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "Mrays/s (primary+secondary)" and d["unit"] == "Mrays/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert d["config"]["rays_per_frame"] == 4944908
    assert abs(d["value"] - 4944908 / (d["ms_per_step"] * 1e3)) < 0.01 * d["value"]
    for k in ("roofline", "cpu_baseline", "per_pixel_stack", "frame", "ms_per_step_repeats"):
        assert k not in d, k
    rgb, hit, rgb8 = (np.load(str(out / (n + ".npy"))) for n in ("rgb", "hit", "rgb8"))
    assert rgb.dtype == np.float32 and hit.dtype == np.float64 and rgb8.dtype == np.float32
    assert rgb.shape == (1024, 1024, 3) and hit.shape == (1024, 1024) and rgb8.shape == (1024, 1024, 3)
    hs = p3d.HostScene(os.path.join(SCENES, "balls_low.p3f"))
    hs.set_resolution(1024, 1024)
    dev = p3d.DeviceScene(hs, bvh=True)
    e_rgb, e_hit, e_rgb8, _ = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4), want_rgb8=True)
    assert (hit == e_hit).all() and (rgb.view(np.uint32) == e_rgb.view(np.uint32)).all() and (rgb8 == e_rgb8).all()


def test_rccl_gather_path_runs_with_one_rank(tri100k_path, tmp_path):
    """The production collective - torch.distributed backend "nccl" = RCCL, device tensors, bench.py's double-buffered
    send / finish / drain around p3d.gather_frame and p3d.assemble_frame - executed on this one-GPU box: `--force-dist`
    takes the N > 1 path with a single rank, launched the way the driver launches ranks.  The assembled frame must equal
    the frame rendered directly, bit for bit (bench.py checks and reports that itself), and so must the frame that
    --dump-outputs writes from rank 0's assembled frames."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    port = 31500 + os.getpid() % 2000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--backend", "nccl",
           "--workload", "tri100k", "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "out")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 1 and d["steps"] == 4
    par = d["config"]["parallelism"]
    assert "RCCL" in par and "gathered frame vs single-GPU frame: ok" in par, par
    assert d["single_gpu_same_workload"]["value"] > 0 and d["value"] > 0
    rgb, hit = np.load(str(tmp_path / "out" / "rgb.npy")), np.load(str(tmp_path / "out" / "hit.npy"))
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["hit.npy", "rgb.npy"]  # the f32 gather: no u8 image on rank 0
    assert rgb.dtype == np.float32 and rgb.shape == (1024, 1024, 3) and hit.dtype == np.float64 and hit.shape == (1024, 1024)
    hs = p3d.HostScene(tri100k_path)
    hs.set_resolution(1024, 1024)
    e_rgb, e_hit, _ = p3d.DeviceScene(hs, bvh=True).render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=6))
    assert (hit == e_hit).all() and (rgb.view(np.uint32) == e_rgb.view(np.uint32)).all()


def test_two_ranks_on_one_gpu_gather_the_single_gpu_frame():
    """The N > 1 path of bench.py end to end, as the driver launches it (torch.distributed.run, one process per rank),
    rehearsed with two ranks sharing the one GPU of this box and a host-staged gloo gather: stripes with halo chains
    (P3D_STACK_LITERAL), one collective per frame of float RGB + hit IDs, de-interleave on rank 0 — and the gathered
    frame must equal, bit for bit, the frame one GPU renders alone."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    port = 29500 + os.getpid() % 2000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "tri100k",
           "--gather", "f32", "--steps", "3", "--warmup", "1", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["stack_mode"] == "literal"
    assert "gathered frame vs single-GPU frame: ok" in d["config"]["parallelism"], d["config"]["parallelism"]
    assert d["config"]["rays_per_frame"] == 11546584  # both ranks' rays = the whole frame's
    one = d["single_gpu_same_workload"]  # the N = 1 point of the same workload, timed on rank 0 outside the timed region
    assert one["ms_per_step"] > 0 and abs(one["value"] - 11546584 / (one["ms_per_step"] * 1e-3) / 1e6) < 0.01 * one["value"]


def test_pow_spec_matches_libm_after_float_rounding(tmp_path):
    """pow_spec (device_core.hpp) replaces libm's double pow of main.cpp:224 in the kernels; only its
    float-rounded value is observable.  2M inputs (x in [0,1], the packaged shine values and random
    exponents): relative error < 1e-12 and at most a handful of float roundings different from libm."""
    import re
    import subprocess
    from conftest import ROOT
    exe = str(tmp_path / "pow_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "p3d-raytracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pow_spec_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    m = re.search(r"worst_rel=([0-9.e+-]+) float_mismatches=(\d+)", out)
    assert m, out
    assert float(m.group(1)) < 1e-12 and int(m.group(2)) <= 4, out


def test_scene_create_rejects_malformed_descriptors():
    """Every index a lane can follow is validated on upload (a wild index in a kernel could take the
    whole host down): corrupt one field at a time and expect P3D_ERR_INVALID / CAPACITY, never a crash.
    A too-small bvh_max_depth is corrected from the node array (the stack capacity depends on it)."""
    import ctypes as C
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    good = hs.desc(bvh=True, grid=True)
    L = p3d.lib()

    def try_create(mutate):
        d = p3d.SceneDesc.from_buffer_copy(bytes(good))
        nodes = (p3d.BvhNode * good.n_bvh_nodes)(*[good.bvh_nodes[i] for i in range(good.n_bvh_nodes)])
        order = (C.c_uint32 * good.n_bvh_prim_index)(*[good.bvh_prim_index[i] for i in range(good.n_bvh_prim_index)])
        prims = (p3d.Prim * good.n_prims)(*[good.prims[i] for i in range(good.n_prims)])
        items = (C.c_uint32 * good.grid.n_items)(*[good.grid.cell_items[i] for i in range(good.grid.n_items)])
        d.bvh_nodes, d.bvh_prim_index, d.prims = nodes, order, prims
        d.grid.cell_items = items
        mutate(d, nodes, order, prims, items)
        h = C.c_void_p()
        rc = L.p3d_scene_create(C.byref(d), 0, C.byref(h))
        if rc == 0:
            L.p3d_scene_destroy(h)
        return rc

    def share_a_child_pair(d, n, o, p, it):  # two inner nodes with the same children: a DAG, not a tree
        inner = [i for i in range(good.n_bvh_nodes) if not (n[i].count_leaf & 0x80000000)]
        a, b = inner[1], inner[2]
        n[a].index = max(n[a].index, n[b].index)
        n[b].index = n[a].index
        assert n[a].index > max(a, b)

    def overlap_child_pairs(d, n, o, p, it):  # (k+1, k+2) and (k+2, k+3): the shape the relabelling walk would re-visit exponentially
        inner = [i for i in range(good.n_bvh_nodes) if not (n[i].count_leaf & 0x80000000) and n[i].index + 2 < good.n_bvh_nodes]
        a = inner[1]
        b = [i for i in inner if i > a][0]
        n[b].index = n[a].index + 1

    assert try_create(lambda d, n, o, p, it: None) == 0
    bad = [
        share_a_child_pair,
        overlap_child_pairs,
        lambda d, n, o, p, it: setattr(p[3], "material", 99),
        lambda d, n, o, p, it: setattr(p[0], "type", 7),
        lambda d, n, o, p, it: setattr(n[0], "index", 1000),        # child pair beyond the array
        lambda d, n, o, p, it: setattr(n[4], "index", 1),           # child in front of its parent (cycle)
        lambda d, n, o, p, it: setattr(o, "_x", None) or o.__setitem__(0, 500),   # object index out of range
        lambda d, n, o, p, it: it.__setitem__(0, 12345),            # grid item out of range
        lambda d, n, o, p, it: setattr(d, "n_bvh_prim_index", 3),
        lambda d, n, o, p, it: setattr(d, "abi_version", 99),
    ]
    for i, m in enumerate(bad):
        rc = try_create(m)
        assert rc in (-1, -4), (i, rc)
    # wrong depth hint: accepted, corrected internally, rendering still matches
    assert try_create(lambda d, n, o, p, it: setattr(d, "bvh_max_depth", 1)) == 0

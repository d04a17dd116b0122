"""Every render kernel csrc/capi_dispatch.hpp instantiates is launched by some test and held to the CPU oracle.

The four render test files used to launch 101 of the 180 whitted_kernel / pt_kernel / pt_adaptive_kernel / feature_kernel /
wf_level_kernel / handoff_check_* instantiations (profiles/dispatch/).  The cases here reach the rest: the path tracer and
its adaptive passes over a scene too big for LDS (windowed, spilling stack; emitters and deferred dielectric branches from
global memory), feature buffers with the window stack, Whitted over a staged scene with the spilling stack
(FramePlan::lds_spill), the object loop and the grid from L2 with anti-aliasing, literal anti-aliased frames with zero-weight
reflection rays (GHOSTS), and the per-level launches without counters.

Which kernel a configuration reaches is the plan's decision (csrc/capi_frame_plan.hpp) and the choosers are pure functions
of it, so every case FIRST asserts the plan flags it claims (DeviceScene.frame_plan) and cannot fall back unnoticed to a
kernel another test covers.  The comparisons and tolerances are those of tests/test_gpu_parity.py: literal frames
bit-identical with every counter equal; per-pixel and non-BVH Whitted within 2e-6 (5e-6 on random_scene scenes) with hit IDs
and COUNTERS equal, the kernels without counters included (check_whitted); path-traced frames with equal hit IDs, within
TOL * max(1, max|oracle|) and every ray / test counter of test_path_tracer equal.

Sizes (tests/test_kernel_variant_scenes.py checks them without a GPU), from the layout rule of csrc/capi_scene_layout.hpp (float4s; a BVH Whitted frame stages
2 * nodes + 4 * prims + 4 * materials + 2 * lights, every other frame 3 * prims more) and plan_frame: a Whitted scene is
staged up to 26 KB, a path-traced one up to 16 KB; a staged Whitted scene gets the spilling stack when its stack bound
(lights + 1) * (tree depth - 1) exceeds 24 or scene + stack exceed 20 KB.  balls_medium.p3f (legacy `f` lines) is 9.6 KB
with a bound of 32: staged + spill over the BVH, but its 13.9 KB with the object-order geometry fit for the object loop and
the grid (bound 1), which would land on kernels other tests cover: those two accels take the generated scene.  The generated "spill_spheres" scene below is 24.3 KB with that geometry: staged + spill on every accel.
"""
import numpy as np
import pytest

from frame_checks import TOL, _pair, assert_same_bits, check_whitted, oracle_cfg_like
import p3d_amd as p3d
from variant_scenes import ACCEL_IDS, ACCEL_VALUES, FRAMES, PT_FRAME, scene_files  # noqa: F401 (scene_files is a fixture)

pytestmark = pytest.mark.gpu

PT_COUNTERS = ("rays_primary", "rays_bounce", "rays_light", "node_tests", "sphere_tests", "tri_tests", "shaded_hits")  # test_path_tracer


# ---- device scene + oracle scene per (name, frame), made once ----


@pytest.fixture(scope="module")
def pairs(scene_files):
    made = {}

    def get(name, res, lens=None):
        key = (name, res, lens)
        if key not in made:
            path, legacy = scene_files[name]
            made[key] = _pair(path, res=res, legacy=legacy, lens=lens)
        return made[key]
    return get


# ---- 1. pt_kernel from L2 ----

def pt_cfg(accel, spp_sqrt, stats, dof=0):
    return p3d.pathtrace_config(accel=accel, spp_sqrt=spp_sqrt, max_depth=20, dof=dof, seed=0x5EED, collect_stats=stats)


class PtFrames:
    """One-shot path-traced frames over PT_FRAME: each oracle frame is rendered once, each GPU frame is rendered and held to
    it once (counters included when stats are on); the plan flags a caller claims are asserted on every call."""

    def __init__(self, pairs):
        self.pairs, self.oracle, self.gpu = pairs, {}, {}

    def __call__(self, name, accel, spp_sqrt, stats, dof=0, lens=None, want=None):
        """-> ((rgb, hit, rgb8), oracle stats)"""
        dev, sc = self.pairs(name, PT_FRAME, lens)
        cfg = pt_cfg(accel, spp_sqrt, stats, dof)
        plan = dev.frame_plan(cfg)
        assert plan.pt and not plan.literal and plan.sub4 == (spp_sqrt >= 4)
        for k, v in (want or {}).items():
            assert getattr(plan, k) == v, (k, plan)
        okey = (name, accel, spp_sqrt, dof, lens)
        if okey not in self.oracle:
            self.oracle[okey] = sc.render(oracle_cfg_like(cfg))
        o_rgb, o_hit, o_st = self.oracle[okey]
        if name == "pt_l2" and accel == p3d.ACCEL_BVH:  # entries really sink out of the LDS window into the backing array
            assert plan.spill_entries > plan.cap and plan.bound == plan.spill_entries, plan
            assert o_st.max_stack >= 10 and o_st.max_stack > plan.cap, "the oracle's stack: %d, the LDS window: %d" % (o_st.max_stack, plan.cap)
        key = okey + (stats,)
        if key not in self.gpu:
            rgb, hit, u8, st = dev.render(cfg, want_rgb8=True)
            assert (hit == o_hit).all(), "hit IDs differ in %d pixels" % int((hit != o_hit).sum())
            assert (hit >= 0).sum() > hit.size // 8
            m = np.isfinite(o_rgb).all(-1)
            assert (np.isfinite(rgb).all(-1) == m).all()
            err, bound = np.abs(rgb[m] - o_rgb[m]), TOL * max(1.0, float(np.abs(o_rgb[m]).max()))
            print("pt frame %s: max |diff| %.3g of %.3g" % (key, err.max(), bound))
            assert err.max() <= bound, "max |diff| %g in %d px, bound %g" % (err.max(), int((err.max(-1) > bound).sum()), bound)
            if stats:
                for k in PT_COUNTERS:
                    assert getattr(st, k) == getattr(o_st, k), k
            self.gpu[key] = (rgb, hit, u8)
        return self.gpu[key], o_st


@pytest.fixture(scope="module")
def pt_frame(pairs):
    return PtFrames(pairs)


L2 = dict(lds_scene=False, lds_spill=False, stack_mode=p3d.STACK_WINDOW)
STAGED_PT = dict(lds_scene=True, lds_spill=False, stack_mode=p3d.STACK_LDS8)


@pytest.mark.parametrize("stats", [1, 0], ids=["stats", "plain"])
@pytest.mark.parametrize("spp_sqrt", [3, 4], ids=["sub1", "sub4"])
@pytest.mark.parametrize("accel", ACCEL_VALUES, ids=ACCEL_IDS)
def test_path_tracer_over_a_scene_traversed_from_l2(pt_frame, accel, spp_sqrt, stats):
    """pt_kernel<A, false, STATS, SUB>: windowed stack, emitters and deferred dielectric branches from global memory."""
    pt_frame("pt_l2", accel, spp_sqrt, stats, want=L2)


def test_path_tracer_from_l2_with_a_lens(pt_frame):
    pt_frame("pt_l2", p3d.ACCEL_BVH, 4, 1, dof=1, lens=(10.0, 1.0), want=L2)


def test_path_tracer_staged_grid_one_lane_per_pixel_with_counters(pt_frame):
    """pt_kernel<1, true, true, 1>"""
    pt_frame("path_glass", p3d.ACCEL_GRID, 3, 1, want=STAGED_PT)


# ---- 2. pt_adaptive_kernel: with rel_error = 0 the passes add up to the one-shot frame, bit for bit ----

@pytest.mark.parametrize("spp_sqrt,passes", [(3, (1,) * 9), (6, (16, 20))], ids=["sub1", "sub4"])
@pytest.mark.parametrize("accel", ACCEL_VALUES, ids=ACCEL_IDS)
@pytest.mark.parametrize("name,stats", [("pt_l2", 1), ("pt_l2", 0), ("path_glass", 1)], ids=["l2-stats", "l2-plain", "staged-stats"])
def test_adaptive_passes_with_zero_threshold_are_the_one_shot_frame(pairs, pt_frame, name, accel, spp_sqrt, passes, stats):
    """pt_adaptive_kernel<A, false, *, *> over PT-L2 and <A, true, true, *> over a staged scene (tests/test_gpu_adaptive.py
    runs the staged passes without counters).  The one-shot frame is held to the oracle (pt_frame); with counters, the
    passes' counters add up to the oracle's."""
    want = L2 if name == "pt_l2" else STAGED_PT
    one_shot, o_st = pt_frame(name, accel, spp_sqrt, stats, want=want)
    dev, _ = pairs(name, PT_FRAME, None)
    cfg = pt_cfg(accel, spp_sqrt, stats)
    assert sum(passes) == spp_sqrt * spp_sqrt
    done = 0
    for n in passes:
        plan = dev.frame_plan(cfg, samples=(done, done + n), mode="adaptive")
        assert plan.pt and plan.sub4 == (n >= 16) and all(getattr(plan, k) == v for k, v in want.items()), plan
        done += n
    ad = dev.adaptive(cfg, 0.0, min_samples=2)
    total = dict.fromkeys(PT_COUNTERS, 0)
    try:
        for n in passes:
            rgb, hit, samples, u8, st = ad.render(n, want_rgb8=True)
            assert ad.active_pixels == PT_FRAME[0] * PT_FRAME[1]  # rel_error = 0 never stops a pixel (include/p3d.h "Decision")
            for k in PT_COUNTERS:
                total[k] += getattr(st, k)
    finally:
        ad.close()
    assert (samples == spp_sqrt * spp_sqrt).all()
    assert_same_bits((rgb, hit, u8), one_shot, "rel_error 0, passes %s" % (passes,))
    if stats:
        for k in PT_COUNTERS:
            assert total[k] == getattr(o_st, k), k


def test_a_pixel_with_negative_mean_luminance_never_counts_as_converged(pairs):
    """include/p3d.h "Decision": the reference's radiance can be negative behind glass, and PT-L2 has a pixel whose mean
    luminance falls below -1e-3 after some samples - the denominator of the error metric is negative there and rel_err with
    it.  Such a pixel is not converged under any threshold: with rel_error = 0 it stays active like every other pixel, and
    under a threshold every finite estimate is below it goes on while the others stop."""
    dev, _ = pairs("pt_l2", PT_FRAME, None)
    cfg = pt_cfg(p3d.ACCEL_BVH, 3, 0)
    shape = (PT_FRAME[1], PT_FRAME[0])

    def luminance(state, n):
        S = state["sum"].astype(np.float64)
        return (0.2126 * S[..., 0] + 0.7152 * S[..., 1] + 0.0722 * S[..., 2]) / n

    # rel_error = 0: nothing stops; the first pass (from min_samples = 2 samples on) that leaves a pixel with a negative estimate
    first = None
    ad = dev.adaptive(cfg, 0.0, min_samples=2)
    try:
        for done in range(1, 10):
            ad.render(1)
            assert ad.active_pixels == shape[0] * shape[1]
            state = ad.read_state()
            neg = np.signbit(state["rel_err"])
            assert (luminance(state, done)[neg] < -0.9e-3).all()  # a set sign bit is a negative denominator m + 1e-3, nothing else
            if first is None and done >= 2 and neg.any():
                first = done
    finally:
        ad.close()
    assert first is not None and first < 9, "PT-L2 no longer has a pixel with a mean luminance below -1e-3 before its last sample"

    # a threshold every finite estimate is below, min_samples = that pass: the rule, pass by pass, from the states read back
    thr = np.float32(1e30)
    ad = dev.adaptive(cfg, float(thr), min_samples=first)
    active, went_on = np.ones(shape, bool), np.zeros(shape, bool)
    try:
        for done in range(1, 10):
            assert ad.active_pixels == int(active.sum())
            if not active.any():
                break
            samples = ad.render(1)[2]
            state = ad.read_state()
            assert np.array_equal(samples, state["samples"]) and (samples[active] == done).all()
            e = state["rel_err"]
            with np.errstate(invalid="ignore"):
                stop = active & (done >= first) & ~np.signbit(e) & (e < thr)
            if done == first:
                went_on = active & np.signbit(e)
            active &= ~stop
    finally:
        ad.close()
    assert went_on.any() and (state["samples"][went_on] > first).all()  # the negative pixels took samples beyond that pass
    assert int((state["samples"] == first).sum()) > shape[0] * shape[1] // 2  # (while most pixels stopped there)


# ---- 3. feature_kernel with the window stack ----

# (scene, accel) of the staged + spill cases: balls_medium over the BVH, the generated scene on every accel.  balls_medium
# over the object loop and the grid fits LDS whole (module docstring) and would land on kernels other tests cover.
SPILL_CASES = [("balls_medium", p3d.ACCEL_BVH)] + [("spill_spheres", a) for a in ACCEL_VALUES]
SPILL_IDS = ["balls_medium-bvh"] + ["spill_spheres-" + a for a in ACCEL_IDS]


@pytest.mark.parametrize("name,accel", [("tri5k", a) for a in ACCEL_VALUES] + SPILL_CASES, ids=["tri5k-" + a for a in ACCEL_IDS] + SPILL_IDS)
def test_pixel_centre_features_with_the_window_stack(pairs, name, accel):
    """test_gpu_denoise.test_pixel_centre_features_match_the_traversal over a scene traversed from L2 and over staged + spill
    scenes (feature_kernel<A, false, kStackWindow>, <A, true, kStackWindow>), the first hits also held to the oracle's."""
    w, h = FRAMES[0]
    dev, sc = pairs(name, FRAMES[0])
    cfg = p3d.whitted_config(accel=accel, max_depth=2)
    plan = dev.frame_plan(cfg, mode="features")
    staged = name != "tri5k"
    assert not plan.pt and plan.lds_scene == staged and plan.lds_spill == staged and plan.stack_mode == p3d.STACK_WINDOW, plan
    if accel == p3d.ACCEL_BVH:
        assert plan.spill_entries > plan.cap
    nd, ac = dev.render_features(cfg)
    rays = [sc.primary_ray(x + 0.5, y + 0.5) for y in range(h) for x in range(w)]
    o = np.array([r[0] for r in rays], np.float32)
    d = np.array([r[1] for r in rays], np.float32)
    hit, t, hp = sc.trace_closest(accel, o, d)
    hit, t, hp, d = hit.reshape(h, w), t.reshape(h, w), hp.reshape(h, w, 3), d.reshape(h, w, 3)
    m = hit >= 0
    assert m.sum() > 256  # (several waves' worth of pixels hit something)
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    assert np.array_equal(ac[..., 3] == 1.0, m) and (ac[..., 3][~m] == 0).all()
    assert (nd[~m] == 0).all() and (ac[~m] == 0).all()
    assert np.array_equal(bits(nd[..., 3][m]), bits(t[m]))
    arr = dev.host.arrays()
    assert np.array_equal(bits(ac[..., :3][m]), bits(arr["materials"][:, 0:3][arr["prim_material"][hit[m]]]))
    norm = np.zeros((h, w, 3), np.float32)
    for obj in np.unique(hit[m]):
        sel = hit == obj
        norm[sel] = dev.object_normal(int(obj), hp[sel])
    f = np.float32
    dn = (norm[..., 0] * d[..., 0] + norm[..., 1] * d[..., 1]) + norm[..., 2] * d[..., 2]
    norml = np.where((dn < f(0))[..., None], norm, norm * f(-1.0))
    decided = m & (np.abs(dn) >= 1e-6)  # (where the dot is ~0 the sign rule may fall either way)
    assert np.array_equal(bits(nd[..., :3][decided]), bits(norml[decided]))
    rest = m & ~decided
    assert ((nd[..., :3][rest] == norm[rest]).all(-1) | (nd[..., :3][rest] == -norm[rest]).all(-1)).all()


# ---- 4. Whitted over staged + spill scenes ----

def aa_kw(spp_sqrt):
    return dict(antialiasing=1, spp_sqrt=spp_sqrt, seed=11) if spp_sqrt else {}


@pytest.mark.parametrize("res", FRAMES, ids=["64x48", "72x40"])
@pytest.mark.parametrize("spp_sqrt", [0, 2], ids=["noaa", "aa"])
@pytest.mark.parametrize("name,accel", SPILL_CASES, ids=SPILL_IDS)
def test_whitted_per_pixel_stack_over_staged_spill_scenes(pairs, name, accel, spp_sqrt, res):
    """whitted_kernel<A, true, STATS, AA, true, 1, 0>, with and without counters (check_whitted)"""
    dev, sc = pairs(name, res)
    cfg = p3d.whitted_config(accel=accel, max_depth=4, stack_mode=p3d.STACK_PER_PIXEL, **aa_kw(spp_sqrt))
    plan = dev.frame_plan(cfg)
    assert plan.lds_scene and plan.lds_spill and not plan.literal and not plan.sub4 and not plan.pt, plan
    assert plan.stack_mode == p3d.STACK_WINDOW
    if accel == p3d.ACCEL_BVH:
        assert plan.bound > 24 and plan.cap < plan.bound and plan.spill_entries == plan.bound, plan
    _, _, st = check_whitted(dev, sc, cfg)
    assert st.shaded_hits > 256


@pytest.mark.parametrize("res", FRAMES, ids=["64x48", "72x40"])
@pytest.mark.parametrize("name,spp_sqrt", [("balls_medium", 2), ("spill_spheres", 0), ("spill_spheres", 2)])
def test_whitted_literal_over_staged_spill_scenes(pairs, name, spp_sqrt, res):
    """Pass1, RepairTiles, RepairList (whitted_kernel<2, true, STATS, AA, true, 1, 1 / 3 / 2, GHOSTS>) and CheckEntries of a literal
    frame: anti-aliased without GHOSTS, and with GHOSTS with and without anti-aliasing; stats, plain and tail stream."""
    dev, sc = pairs(name, res)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, **aa_kw(spp_sqrt))
    plan = dev.frame_plan(cfg)
    assert plan.literal and plan.lds_scene and plan.lds_spill and plan.repair_tiles and not plan.per_level and not plan.sub4, plan
    assert plan.zero_weight_reflections == (name == "spill_spheres") and plan.bound > 24 and plan.spill_entries == plan.bound, plan
    _, _, st = check_whitted(dev, sc, cfg)
    assert st.handoff_checked > 0
    if name == "spill_spheres":
        assert st.rays_refract > 0  # (glass spheres are in view: the zero-weight reflection rays exist)


def test_object_loop_staged_antialiased_without_counters(pairs):
    """whitted_kernel<0, true, false, true, false, 1, 0>: check_whitted's render without counters"""
    dev, sc = pairs("balls_low", FRAMES[0])
    cfg = p3d.whitted_config(accel=p3d.ACCEL_NONE, max_depth=3, **aa_kw(2))
    plan = dev.frame_plan(cfg)
    assert plan.lds_scene and not plan.lds_spill and not plan.sub4 and plan.stack_mode == p3d.STACK_LDS6, plan
    check_whitted(dev, sc, cfg)


# ---- 5. Whitted from L2 on the object loop and the grid ----

@pytest.mark.parametrize("spp_sqrt", [0, 1, 2], ids=["noaa", "aa-sub1", "aa-sub4"])
@pytest.mark.parametrize("accel", [p3d.ACCEL_NONE, p3d.ACCEL_GRID], ids=["none", "grid"])
def test_whitted_object_loop_and_grid_from_l2(pairs, accel, spp_sqrt):
    """whitted_kernel<0 or 1, false, STATS, AA, true, SUB, 0> over the 5 000-triangle soup: one sample per pixel of an
    anti-aliased frame keeps one lane per pixel, four take four lanes."""
    dev, sc = pairs("tri5k", FRAMES[0])
    cfg = p3d.whitted_config(accel=accel, max_depth=3, **aa_kw(spp_sqrt))
    plan = dev.frame_plan(cfg)
    assert not plan.lds_scene and not plan.lds_spill and not plan.literal and plan.sub4 == (spp_sqrt == 2), plan
    assert plan.stack_mode == p3d.STACK_WINDOW and plan.spill_entries == 0
    _, _, st = check_whitted(dev, sc, cfg)
    assert st.shaded_hits > 256


# ---- 6. the remaining literal and per-level cases ----

@pytest.mark.parametrize("res", FRAMES, ids=["64x48", "72x40"])
def test_whitted_literal_antialiased_from_l2_with_zero_weight_reflections(pairs, res):
    """Pass1 and RepairList with GHOSTS over a scene traversed from L2 (whitted_kernel<2, false, STATS, true, true, 1, 1 / 2, true>)"""
    dev, sc = pairs("l2_ghosts", res)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, **aa_kw(2))
    plan = dev.frame_plan(cfg)
    assert plan.literal and not plan.lds_scene and not plan.repair_tiles and not plan.sub4 and not plan.per_level, plan
    assert plan.zero_weight_reflections and plan.spill_entries > plan.cap, plan
    _, _, st = check_whitted(dev, sc, cfg, tol=5e-6)
    assert st.handoff_checked > 0 and st.rays_refract > 0


def test_per_level_launches_per_pixel_stack_without_counters(pairs):
    """wf_level_kernel<false, 0> (and <true, 0>): check_whitted renders both and holds both to the oracle's per-pixel frame."""
    dev, sc = pairs("tri5k", FRAMES[0])
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, stack_mode=p3d.STACK_PER_PIXEL, chain_launch=p3d.CHAIN_PER_LEVEL)
    plan = dev.frame_plan(cfg)
    assert plan.per_level and not plan.literal and not plan.lds_scene and plan.spill_entries > plan.cap, plan
    _, _, st = check_whitted(dev, sc, cfg, max_stack=True)
    assert st.rays_reflect > 0  # (more than one level was launched)

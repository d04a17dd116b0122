"""What a test needs to render frames and compare them: scene constructors, the oracle-parity checks of Whitted frames, frame
lists with their counters, bit-for-bit assertions on frames, trees and grids, and the scene constants several modules share.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/").
tests/test_shared_checks.py holds the assertions here to the smallest difference each exists to catch."""
import os

import numpy as np

import p3d_amd as p3d
from conftest import GOLDEN, ROOT
from lbvh_reference import TREE_KEYS, assert_same_tree  # noqa: F401 (the one definition; test modules take them from here)
from oracle import binding as ob

CORNELL = os.path.join(ROOT, "scenes", "cornell.p3f")
PLANES = os.path.join(ROOT, "scenes", "planes.p3f")
ACCELS = {"none": p3d.ACCEL_NONE, "grid": p3d.ACCEL_GRID, "bvh": p3d.ACCEL_BVH}
TOL = 1e-4
# the oracle's counters of a Whitted frame (check_whitted)
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "node_tests", "sphere_tests", "tri_tests",
            "box_tests", "plane_tests", "shaded_hits", "pixels")
# what two renders of one scene by the library are compared in (frames): Whitted and path-traced ray classes, every test count
RENDER_COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_bounce", "rays_light", "node_tests",
                   "sphere_tests", "tri_tests", "box_tests", "plane_tests", "shaded_hits")
GRID_KEYS = ("grid_bmin", "grid_bmax", "grid_cell_start", "grid_cell_items")


# ---- scenes ----------------------------------------------------------------------------------------------------------------------

def load(path, res, legacy_f11=False):
    """The host scene of a file at res x res"""
    hs = p3d.HostScene(path, legacy_f11=legacy_f11)
    hs.set_resolution(res, res)
    return hs


def device_scene(path, res, legacy_f11=False, lens=None, sky=False, bvh=True, grid=True):
    """A device scene of a file at res = (w, h), built anew at every call (a module that wants one per key caches it itself)"""
    hs = p3d.HostScene(path, legacy_f11=legacy_f11)
    hs.set_resolution(*res)
    if lens:
        hs.set_lens(*lens)
    dev = p3d.DeviceScene(hs, bvh=bvh, grid=grid)
    if sky:
        dev.set_skybox(p3d.load_skybox_dir(os.path.join(GOLDEN, "skybox")))
    return dev


def cached_device_scenes():
    """device_scene behind a cache of the caller's own: one scene per set of arguments, for the module that asks"""
    made = {}

    def get(path, res, legacy_f11=False, lens=None, sky=False, bvh=True, grid=True):
        key = (path, res, legacy_f11, lens, sky, bvh, grid)
        if key not in made:
            made[key] = device_scene(*key)
        return made[key]
    return get


def _pair(scene_file, res=None, legacy=False, bvh=True, grid=True, lens=None):
    """(device scene, oracle scene) of one file"""
    hs = p3d.HostScene(scene_file, legacy_f11=legacy)
    sc = ob.Scene(scene_file, legacy_f11=legacy)
    if res:
        hs.set_resolution(*res)
        sc.set_resolution(*res)
    if lens:
        hs.set_lens(*lens)
        sc.set_lens(*lens)
    return p3d.DeviceScene(hs, bvh=bvh, grid=grid), sc


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rays(n=40000, seed=5, axis_parallel=False):
    """n rays from a box around the scenes towards their middle; axis_parallel zeroes one component of the first eighth"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    d = (rng.uniform(-1, 1, (n, 3)) - o).astype(np.float32)
    if axis_parallel:
        d[: n // 8, rng.integers(0, 3)] = 0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


def tile_of(t):
    return None if t is None else p3d.Tile(t[0], t[1], t[2], t[3], 0, 1)


# ---- bits ------------------------------------------------------------------------------------------------------------------------

def as_bytes(a):
    return np.ascontiguousarray(a).tobytes()


def f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f64_bytes(x):
    return np.float64(x).tobytes()


def same_bits(a, b):
    """float32 arrays equal in shape and in every bit -> bool"""
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def same_bits_or_nan(a, b):
    """float32 arrays equal in bits, a NaN on both sides counting as equal -> mask"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s for %s" % (what, got.shape, want.shape)
    same = (f32_bits(got) == f32_bits(want)) if got.dtype == np.float32 else (got == want)
    assert same.all(), "%s: %d of %d values differ, first at %s" % (what, int((~same).sum()), same.size, np.argwhere(~same)[0])


def assert_same_bits(a, b, what, where=None):
    """(rgb, hit, rgb8) twice: hit IDs, every colour bit and the bytes equal, in the pixels of the mask `where` (all of them)"""
    rgb_a, hit_a, u8_a = a
    rgb_b, hit_b, u8_b = b
    m = np.ones(hit_a.shape, bool) if where is None else where
    assert np.array_equal(hit_a[m], hit_b[m]), "%s: hit IDs differ in %d pixels" % (what, int((hit_a[m] != hit_b[m]).sum()))
    bad = (rgb_a.view(np.uint32) != rgb_b.view(np.uint32)).any(-1) & m
    assert not bad.any(), "%s: %d pixels differ in some colour bit, max |diff| %g" % (
        what, int(bad.sum()), float(np.abs(rgb_a - rgb_b)[m].max()))
    assert np.array_equal(u8_a[m], u8_b[m]), "%s: rgb8 differs" % what


# ---- frame lists: [(label, rgb, hit, {counter: value})] --------------------------------------------------------------------------

def frames(dev, configs, skip_unsupported=True):
    """One render per (label, cfg).  skip_unsupported leaves out a cfg the scene refuses with P3D_ERR_UNSUPPORTED (a scene that
    has no such mode), but not all of them."""
    out = []
    for label, cfg in configs:
        try:
            rgb, hit, st = dev.render(cfg)
        except p3d.P3DError as e:
            if not skip_unsupported or e.code != -3:  # P3D_ERR_UNSUPPORTED
                raise
            continue
        out.append((label, rgb, hit, {k: getattr(st, k) for k in RENDER_COUNTERS}))
    assert out
    return out


def assert_same_frames(a, b, what):
    assert [f[0] for f in a] == [f[0] for f in b]
    for (label, rgb_a, hit_a, st_a), (_, rgb_b, hit_b, st_b) in zip(a, b):
        assert np.array_equal(hit_a, hit_b), "%s, %s: hit IDs differ in %d pixels" % (what, label, int((hit_a != hit_b).sum()))
        bad = (rgb_a.view(np.uint32) != rgb_b.view(np.uint32)).any(-1)
        assert not bad.any(), "%s, %s: %d pixels differ in some colour bit, max |diff| %g" % (
            what, label, int(bad.sum()), float(np.abs(rgb_a - rgb_b).max()))
        assert st_a == st_b, "%s, %s: counters %s / %s" % (what, label, st_a, st_b)


def frames_differ(a, b):
    """Some pixel's colour bits or hit ID changed (a Whitted frame of a scene without lights is black: the IDs tell)"""
    return any((ra.view(np.uint32) != rb.view(np.uint32)).any() or (ha != hb).any() for (_, ra, ha, _), (_, rb, hb, _) in zip(a, b))


def assert_same_grid(got, want, what):
    assert tuple(got["grid_n"]) == tuple(want["grid_n"]), "%s: %s cells, the host has %s" % (what, got["grid_n"], want["grid_n"])
    for k in GRID_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, "%s: %s has shape %s, the host's %s" % (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), "%s: %s differs in %d entries" % (what, k, int((got[k] != want[k]).sum()))


# ---- Whitted frames against the CPU oracle ---------------------------------------------------------------------------------------

def literal_applies(cfg):
    """P3D_STACK_LITERAL changes something only where the reference has a stack that outlives a query:
    rayTracing over the BVH (include/p3d.h)."""
    pt = cfg.integrator == p3d.PATHTRACE and cfg.antialiasing
    return cfg.stack_mode == p3d.STACK_LITERAL and cfg.accel == p3d.ACCEL_BVH and not pt


def oracle_cfg_like(cfg, **kw):
    lit = literal_applies(cfg)
    base = dict(integrator=cfg.integrator, accel=cfg.accel, max_depth=cfg.max_depth, spp_sqrt=cfg.spp_sqrt,
                antialiasing=cfg.antialiasing, depth_of_field=cfg.depth_of_field, sample_disk=cfg.sample_disk,
                soft_shadows=cfg.soft_shadows, sample_mode=cfg.sample_mode, light_side=cfg.light_side,
                gamma=cfg.gamma, skybox=cfg.skybox, seed=cfg.seed, debug_view=cfg.debug_view, rng_mode=0, stack_mode=1 if lit else 0,
                trace_zero_weight=1 if lit else 0, math_mode=0, threads=1 if lit else 8)
    base.update(kw)
    return ob.default_config(**base)


def per_pixel(cfg):
    """The same configuration with the stack emptied at every primary sample (P3D_STACK_PER_PIXEL)."""
    c = p3d.Config.from_buffer_copy(bytes(cfg))
    c.stack_mode = p3d.STACK_PER_PIXEL
    return c


def assert_bit_identical(gpu, orc, what=""):
    rgb_g, hit_g = gpu
    rgb_o, hit_o = orc
    assert (hit_g == hit_o).all(), "%s: hit IDs differ in %d pixels" % (what, int((hit_g != hit_o).sum()))
    diff = rgb_g.view(np.uint32) != rgb_o.view(np.uint32)
    nan_both = np.isnan(rgb_g) & np.isnan(rgb_o)
    bad = (diff & ~nan_both).any(-1)
    assert not bad.any(), "%s: %d pixels differ in some colour bit, max |diff| %g" % (
        what, int(bad.sum()), float(np.nanmax(np.abs(rgb_g - rgb_o))))


_TAIL = []


def _render_with_tail_stream(dev, cfg):
    """The device-buffer call without stats, the launches behind pass 1 on a second stream; -> (rgb, hit) on the host."""
    import torch
    if not _TAIL:
        _TAIL.append(torch.cuda.Stream())
    tile = dev.full_tile()
    n = tile.w * tile.h
    buf = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    dev.set_tail_stream(_TAIL[0])
    try:
        dev.render_device(cfg, tile, d_rgb=buf.data_ptr(), d_hit=buf.data_ptr() + n * 12, stream=torch.cuda.current_stream().cuda_stream)
        dev.join(host_wait=True)
        assert dev.status() == 0, p3d.lib().p3d_last_error().decode()
    finally:
        dev.set_tail_stream(None)
    host = buf.cpu().numpy()
    return host[: n * 12].view(np.float32).reshape(tile.h, tile.w, 3), host[n * 12:].view(np.int32).reshape(tile.h, tile.w)


def check_whitted(dev, sc, cfg, tol=2e-6, counters=COUNTERS, max_stack=False):
    """cfg as given: for the BVH under P3D_STACK_LITERAL the frame must be bit-identical to the oracle's serial
    order and every ray / test counter equal to the oracle's.  Then (BVH) the per-pixel stack, or (other back ends) the one render there is: frame within `tol` of the
    oracle in the same semantics and every counter equal, and the frame of the kernels without counters (collect_stats = 0)
    within the same `tol` of the same oracle frame.  Returns the first render's (rgb, hit, stats)."""
    cfg.collect_stats = 1
    first = dev.render(cfg)
    if literal_applies(cfg):
        o_rgb, o_hit, o_st = sc.render(oracle_cfg_like(cfg))
        assert_bit_identical(first[:2], (o_rgb, o_hit), "literal hit_stack")
        for k in counters:  # what the final frame traced, query by query: redone pixels count once, stale entries visited count
            assert getattr(first[2], k) == getattr(o_st, k), "literal " + k
        assert first[2].max_stack >= o_st.max_stack  # (the deepest stack of anything traced, speculative passes included)
        # ... and the instantiation without counters - the one bench.py times - renders the same bits
        plain_cfg = p3d.Config.from_buffer_copy(bytes(cfg))
        plain_cfg.collect_stats = 0
        plain = dev.render(plain_cfg)
        assert_bit_identical(plain[:2], (o_rgb, o_hit), "literal hit_stack, kernels without counters")
        # ... also with the hand-off launches on a tail stream (p3d_scene_set_tail_stream: how bench.py enqueues literal frames)
        assert_bit_identical(_render_with_tail_stream(dev, plain_cfg), (o_rgb, o_hit), "literal hit_stack, hand-off on a tail stream")
        cfg = per_pixel(cfg)
        rgb, hit, st = dev.render(cfg)
    else:
        rgb, hit, st = first
    o_rgb, o_hit, o_st = sc.render(oracle_cfg_like(cfg))
    # ... and the instantiation without counters - the one a caller who asks for no stats runs - against the same oracle frame
    plain_cfg = p3d.Config.from_buffer_copy(bytes(cfg))
    plain_cfg.collect_stats = 0
    m = np.isfinite(o_rgb).all(-1)
    for what, (f_rgb, f_hit) in (("with counters", (rgb, hit)), ("kernels without counters", dev.render(plain_cfg)[:2])):
        assert (f_hit == o_hit).all(), "%s: hit IDs differ in %d pixels" % (what, int((f_hit != o_hit).sum()))
        assert (np.isfinite(f_rgb).all(-1) == m).all(), what  # NaN pixels (if any) are NaN on both sides
        err = np.abs(f_rgb[m] - o_rgb[m])
        assert err.max() <= tol, "%s: max |diff| %g, %d pixels over %g" % (what, err.max(), int((err.max(-1) > tol).sum()), tol)
    for k in counters:
        assert getattr(st, k) == getattr(o_st, k), k
    if max_stack:
        assert st.max_stack == o_st.max_stack
    return first


def compare(gpu, orc, tol):
    rgb_g, hit_g = gpu
    rgb_o, hit_o = orc
    assert (hit_g == hit_o).all(), "hit IDs differ in %d pixels" % int((hit_g != hit_o).sum())
    d = np.abs(rgb_g - rgb_o)
    assert np.isfinite(rgb_g).all()
    assert d.max() <= tol, "max |diff| %g in %d px" % (d.max(), int((d.max(-1) > tol).sum()))
    return d.max()

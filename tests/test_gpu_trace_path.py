"""Path-traced radiance for rays in device memory (p3d_trace_path_device) and a camera's sample rays
(p3d_camera_sample_rays_device).

The yardstick is exact.  Every (pixel, sample) of a path-traced frame draws from its own RNG stream, so the sample rays of a
camera with the states left after generating them, traced one sample per call and added up in sample order, must give the
frame's sum: rgb / float32(spp) equals dev.render(pathtrace cfg) in every bit, and the first call's hit_id is the frame's.
camera_sample_rays_device itself is held to the oracle's primary_ray / primary_ray_lens fed with the draws of the Python
restatement of the RNG (tests/test_trace_path_api.py pins that to the oracle's stream).  Tolerance 0 everywhere.  Frames are at
most 48 x 40; the deep triangle soup is rendered at 24 x 20."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, scene_path
import device_query_contract as dq
from device_query_contract import INVALID, UNSUPPORTED
from frame_checks import ACCELS, assert_bits, f32_bits, tile_of
from oracle import binding as ob
import p3d_amd as p3d
from rng_reference import next31, seed_stream
import shading_reference as sh

pytestmark = pytest.mark.gpu

RES = (48, 40)
SOUP_RES = (24, 20)
SUB_TILE = (5, 7, 11, 6)  # x0, y0, w, h: a width that is no multiple of 8, rows that start inside a wave tile
SEED = 0x5EED
DEPTHS = (0, 1, 2, 5, 8)  # the roulette sets in at 5
SCENES = ("path_glass", "path_mirror", "path_balls_low", "path_dof", "soup-host", "soup-device")
ACC = p3d.PATH_ACCUMULATE


def write_soup(path, n=800):
    """An emitter sphere over n triangles clustered around the origin (diffuse, mirror and glass groups): the clustering makes
    the tree over them deeper than the 16-entry LDS window of the query stack, host-built or device-built."""
    rng = np.random.default_rng(7)
    lines = ["bclr 0.25 0.3 0.4", "v", "from 0.3 -4.2 1.1", "at 0 0 0", "up 0 0 1", "angle 38", "hither 0.01",
             "resolution %d %d" % SOUP_RES, "aperture 0", "focal 1"]
    mats = ["f 0.75 0.6 0.45 1 0 0 0 0 10 0 1 0 0 0", "f 0.4 0.7 0.5 1 0 0 0 0 10 0 1 0 0 0", "f 0.9 0.9 0.9 0 1 1 1 1 300 0 1 0 0 0",
            "f 0.9 0.95 0.9 0 1 1 1 0 300 1 1.5 0 0 0"]
    u = rng.uniform(-1, 1, (n, 3))
    c, o = np.sign(u) * np.abs(u) ** 4, rng.uniform(-0.09, 0.09, (n, 3, 3))
    for t in range(n):
        if t % (n // 8) == 0:
            lines.append(mats[(t // (n // 8)) % 4])
        lines.append("p 3\n" + "\n".join("%.6f %.6f %.6f" % tuple(c[t] + o[t, k]) for k in range(3)))
    lines += ["f 0 0 0 1 0 0 0 0 10 0 1 9 8 6", "s 0.2 -0.3 1.7 0.35"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """name -> DeviceScene with every accel, made once"""
    soup = write_soup(tmp_path_factory.mktemp("path_query") / "soup.p3f")
    made = {}

    def get(name):
        if name not in made:
            if name.startswith("soup"):
                hs = p3d.HostScene(soup)
                dev = p3d.DeviceScene(hs, bvh="device", grid="device") if name == "soup-device" else p3d.DeviceScene(hs, bvh=True, grid=True)
                depth = dev.export_bvh()["bvh_max_depth"] if name == "soup-device" else hs.desc(bvh=True).bvh_max_depth
                assert depth > 16, "the tree of %s fits the stack window" % name
            else:
                hs = p3d.HostScene(scene_path(name + ".p3f"))
                hs.set_resolution(*RES)
                dev = p3d.DeviceScene(hs, bvh=True, grid=True)
            made[name] = dev
        return made[name]
    return get


def pt_cfg(accel, spp_sqrt, depth, **kw):
    return p3d.pathtrace_config(accel=ACCELS[accel] if isinstance(accel, str) else accel, spp_sqrt=spp_sqrt, max_depth=depth, seed=SEED, **kw)


def frame(dev, cfg, tile=None):
    rgb, hit = dev.render(cfg, tile=tile_of(tile))[:2]
    return rgb.reshape(-1, 3), hit.reshape(-1)


def reconstruct(dev, cfg, tile=None, flags=0, stream=0):
    """The frame of `cfg` from its sample rays: one call per sample, accumulated in sample order -> (sum (n, 3), hit (n,))"""
    import torch
    t = tile_of(tile) or dev.full_tile()
    n = t.w * t.h
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    hit = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    for s in range(cfg.spp_sqrt * cfg.spp_sqrt):
        rays = p3d.camera_sample_rays_device(dev, cfg, s, tile=tile_of(tile), stream=stream)
        out = {"rgb": rgb, "hit_id": hit} if s == 0 else {"rgb": rgb}
        p3d.trace_path_device(dev, cfg.accel, rays["origin"], rays["direction"], cfg.max_depth, samples=1, sample_begin=s, seed=cfg.seed,
                              rng=rays["rng"], flags=flags | ACC, want=("hit_id",) if s == 0 else (), out=out, stream=stream)
    return rgb.cpu().numpy(), hit.cpu().numpy()


def check_reconstruction(dev, cfg, what, tile=None, flags=0):
    total, hit = reconstruct(dev, cfg, tile, flags)
    f_rgb, f_hit = frame(dev, cfg, tile)
    assert_bits(hit, f_hit, what + ": hit_id")
    assert_bits(total / np.float32(cfg.spp_sqrt * cfg.spp_sqrt), f_rgb, what + ": rgb")
    return f_rgb, f_hit


def states_tensor(states):
    import torch
    return torch.from_numpy(np.array(states, dtype=np.uint64).reshape(-1, 2).view(np.int64)).cuda()


def pixel_rays(dev, tile=None):
    return p3d.camera_rays_device(dev, tile=tile_of(tile))


def path(dev, accel, rays, depth, **kw):
    out = p3d.trace_path_device(dev, ACCELS[accel], rays["origin"], rays["direction"], depth, **kw)
    return out["rgb"].cpu().numpy(), out["hit_id"].cpu().numpy()


# ---- 1. sample rays --------------------------------------------------------------------------------------------------------------------

def oracle_sample_rays(sc, res_x, tile, sample, spp_sqrt, antialiasing=1, sample_mode=p3d.SAMPLE_JITTER, depth_of_field=0, sample_disk=0):
    """make_primary (main.cpp:758-787) in float32 / float64 scalars on the draws of the Python RNG, through the oracle's camera
    -> (origin (n, 3), direction (n, 3), states (n, 2) uint64 after the draws)"""
    f = np.float32
    x0, y0, w, h = tile
    si, sj = divmod(sample, spp_sqrt)
    origin, direction, states = [], [], []
    for y in range(y0, y0 + h):
        for x in range(x0, x0 + w):
            st = list(seed_stream(SEED, y * res_x + x, sample))

            def draw():
                st[0], v = next31(st[0], st[1])
                return v
            rand_float = lambda: f(draw()) / f(2147483648.0)
            erand48 = lambda: draw() / 2147483647.0
            if not antialiasing:
                o, d = sc.primary_ray(f(x + 0.5), f(y + 0.5))
            else:
                if sample_mode == p3d.SAMPLE_JITTER:
                    px = f(x) + (f(si) + rand_float()) / f(spp_sqrt)
                    py = f(y) + (f(sj) + rand_float()) / f(spp_sqrt)
                else:
                    r1 = 2 * erand48()
                    dx = math.sqrt(r1) - 1 if r1 < 1 else 1 - math.sqrt(2 - r1)
                    r2 = 2 * erand48()
                    dy = math.sqrt(r2) - 1 if r2 < 1 else 1 - math.sqrt(2 - r2)
                    px, py = f(x + (0.5 + dx) / spp_sqrt), f(y + (0.5 + dy) / spp_sqrt)
                if depth_of_field:
                    if sample_disk:
                        while True:
                            b = rand_float()
                            a = rand_float()
                            lx, ly = a * f(2) - f(1), b * f(2) - f(1)
                            if not lx * lx + ly * ly + f(0) * f(0) >= f(1):
                                break
                    else:
                        lx = (f(si) + rand_float()) / f(spp_sqrt)
                        ly = (f(sj) + rand_float()) / f(spp_sqrt)
                    o, d = sc.primary_ray_lens(lx, ly, px, py)
                else:
                    o, d = sc.primary_ray(px, py)
            origin.append(o)
            direction.append(d)
            states.append(st)
    return np.array(origin, np.float32), np.array(direction, np.float32), np.array(states, dtype=np.uint64)


def test_sample_rays_without_antialiasing_are_the_pixel_centres(scenes):
    dev = scenes("path_balls_low")
    for tile in (None, SUB_TILE):
        x0, y0, w, h = tile or (0, 0) + RES
        centre = pixel_rays(dev, tile)
        cfg = pt_cfg("bvh", 3, 4, antialiasing=0)
        got = p3d.camera_sample_rays_device(dev, cfg, 5, tile=tile_of(tile))
        assert_bits(got["origin"].cpu().numpy(), centre["origin"].cpu().numpy(), "tile %s: origin" % (tile,))
        assert_bits(got["direction"].cpu().numpy(), centre["direction"].cpu().numpy(), "tile %s: direction" % (tile,))
        fresh = [seed_stream(SEED, y * RES[0] + x, 5) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
        assert (got["rng"].cpu().numpy().view(np.uint64) == np.array(fresh, dtype=np.uint64)).all(), "tile %s: the freshly seeded state" % (tile,)
    alone = p3d.camera_sample_rays_device(dev, cfg, 5, want=())
    assert sorted(alone) == ["direction", "origin"]


@pytest.mark.parametrize("mode", ["jitter", "tent", "lens-square", "lens-disk", "tent-lens-disk"])
def test_sample_rays_are_the_oracles(mode, scenes):
    lens = "lens" in mode
    name = "path_dof" if lens else "path_glass"
    dev, sc = scenes(name), ob.Scene(scene_path(name + ".p3f"))
    sc.set_resolution(*RES)
    assert (dev.camera.aperture != 0) == lens
    opts = dict(sample_mode=p3d.SAMPLE_TENT if "tent" in mode else p3d.SAMPLE_JITTER, depth_of_field=int(lens), sample_disk=int("disk" in mode))
    cfg = pt_cfg("bvh", 3, 4, dof=opts["depth_of_field"], sample_mode=opts["sample_mode"], sample_disk=opts["sample_disk"])
    for sample in (0, 5, 8):
        got = p3d.camera_sample_rays_device(dev, cfg, sample, tile=tile_of(SUB_TILE))
        o, d, states = oracle_sample_rays(sc, RES[0], SUB_TILE, sample, 3, **opts)
        what = "%s, sample %d" % (mode, sample)
        assert_bits(got["origin"].cpu().numpy(), o, what + ": origin")
        assert_bits(got["direction"].cpu().numpy(), d, what + ": direction")
        assert (got["rng"].cpu().numpy().view(np.uint64) == states).all(), what + ": the state after the draws"
    if lens:
        assert (f32_bits(o) != f32_bits(o[0])).any(), "every ray starts at the eye: no lens sample"


def test_sample_rays_refusals(scenes):
    import torch
    dev = scenes("path_dof")
    n = RES[0] * RES[1]
    good = {"origin": torch.zeros((n, 3), device="cuda"), "direction": torch.zeros((n, 3), device="cuda"),
            "rng": torch.zeros((n, 2), dtype=torch.int64, device="cuda")}
    L, h = p3d.lib(), dev._h
    o, d, r = (good[k].data_ptr() for k in ("origin", "direction", "rng"))
    cfg = pt_cfg("bvh", 2, 4)
    bad_mode, no_spp = pt_cfg("bvh", 2, 4, sample_mode=2), pt_cfg("bvh", 0, 4)
    other = p3d.look_at(res=(32, 32), **sh.SECOND_VIEW)
    host = np.zeros((n, 2), np.uint64)
    call = lambda cam=None, tile=None, c=cfg, sample=0, o=o, d=d, r=r: L.p3d_camera_sample_rays_device(
        h, C.byref(cam) if cam else None, C.byref(tile) if tile else None, C.byref(c) if c else None, sample, o, d, r, None)
    for what, word, refused in [
        ("another resolution", "32x32", lambda: call(cam=other)),
        ("a tile outside", "tile", lambda: call(tile=p3d.Tile(40, 0, 16, 8, 0, 1))),
        ("a null config", "null config", lambda: call(c=None)),
        ("spp_sqrt 0", "spp_sqrt", lambda: call(c=no_spp)),
        ("sample 4 of 4", "sample must be below", lambda: call(sample=4)),
        ("an unknown sample_mode", "sample_mode", lambda: call(c=bad_mode)),
        ("a null buffer", "null argument", lambda: call(d=None)),
        ("a misaligned buffer", "aligned", lambda: call(o=o + 2)),
        ("a misaligned rng", "8-byte aligned", lambda: call(r=r + 4)),
        ("a host rng", "host memory", lambda: call(r=host.ctypes.data)),
    ]:
        assert refused() == -1, what
        assert word in L.p3d_last_error().decode(), "%s: %s" % (what, L.p3d_last_error())
    torch.cuda.synchronize()
    assert not any(bool(v.any()) for v in good.values()), "a refused call wrote"
    assert call() == 0  # the lens camera of path_dof, with and without depth_of_field
    assert call(c=pt_cfg("bvh", 2, 4, dof=1)) == 0


# ---- 2. frame reconstruction, the main yardstick ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel", list(ACCELS))
@pytest.mark.parametrize("name", SCENES)
def test_the_sample_rays_traced_and_summed_are_the_frame(name, accel, scenes):
    dev = scenes(name)
    dof = int(name == "path_dof")
    mode = p3d.SAMPLE_TENT if name == "path_mirror" else p3d.SAMPLE_JITTER
    lit, differ = 0, 0
    for depth in DEPTHS:
        for spp_sqrt in (1, 2, 4):  # one lane per pixel; from 16 samples the frame's four-lanes-per-pixel kernel
            cfg = pt_cfg(accel, spp_sqrt, depth, dof=dof, sample_mode=mode)
            assert dev.frame_plan(cfg).sub4 == (spp_sqrt == 4)
            f_rgb, f_hit = check_reconstruction(dev, cfg, "%s over %s, depth %d, %d spp" % (name, accel, depth, spp_sqrt * spp_sqrt))
            lit += int((f_hit >= 0).sum())
            if depth == 8 and spp_sqrt == 2:
                shallow = frame(dev, pt_cfg(accel, 2, 1, dof=dof, sample_mode=mode))[0]
                differ = int((f32_bits(shallow) != f32_bits(f_rgb)).any(axis=1).sum())
    assert lit > 0 and differ > 20, "%s: the bounces add nothing to the frame" % name
    assert dev.status() == 0


def test_a_sub_tile_and_the_skybox(scenes):
    dev = scenes("path_glass")
    check_reconstruction(dev, pt_cfg("bvh", 2, 5), "path_glass, sub-tile", tile=SUB_TILE)
    with pytest.raises(p3d.P3DError) as e:
        reconstruct(dev, pt_cfg("bvh", 1, 2), flags=p3d.RADIANCE_SKYBOX)
    assert e.value.code == -1 and "cubemap" in str(e.value)
    dev.set_skybox(p3d.load_skybox_dir(os.path.join(GOLDEN, "skybox")))
    for accel in ACCELS:
        sky, _ = check_reconstruction(dev, pt_cfg(accel, 2, 5, skybox=1), "skybox over %s" % accel, flags=p3d.RADIANCE_SKYBOX)
        plain, _ = check_reconstruction(dev, pt_cfg(accel, 2, 5), "no flag over %s" % accel)
        assert (f32_bits(sky) != f32_bits(plain)).any(axis=1).sum() > 100, "the cubemap shows nowhere"


# ---- 3. the seeded mode is the state mode ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel", ["bvh", "none"])
def test_seeded_and_state_modes(accel, scenes):
    import torch
    dev = scenes("path_glass")
    rays = pixel_rays(dev, SUB_TILE)
    n = rays["origin"].shape[0]
    seed, depth = 0x0123456789ABCDEF, 6
    one = lambda s, **kw: p3d.trace_path_device(dev, ACCELS[accel], rays["origin"], rays["direction"], depth, samples=1, sample_begin=s, seed=seed, **kw)
    for s in (0, 3):
        seeded = one(s)
        given = one(s, rng=states_tensor([seed_stream(seed, i, s) for i in range(n)]))
        assert_bits(given["rgb"].cpu().numpy(), seeded["rgb"].cpu().numpy(), "sample %d over %s: rgb" % (s, accel))
        assert_bits(given["hit_id"].cpu().numpy(), seeded["hit_id"].cpu().numpy(), "sample %d over %s: hit_id" % (s, accel))
    # five samples in one call: five accumulated one-sample calls
    five, hit = path(dev, accel, rays, depth, samples=5, sample_begin=2, seed=seed)
    total = torch.zeros((n, 3), device="cuda")
    for s in range(2, 7):
        one(s, flags=ACC, want=(), out={"rgb": total})
    assert_bits(five, total.cpu().numpy(), "five seeded samples over %s" % accel)
    assert_bits(hit, one(2)["hit_id"].cpu().numpy(), "hit_id of five samples over %s" % accel)
    assert (f32_bits(five) != f32_bits(one(2)["rgb"].cpu().numpy())).any(), "the samples after the first add nothing"
    # with a state: the stream goes on from sample to sample and is written back
    start = states_tensor([seed_stream(77, i, 0) for i in range(n)])
    carried, chained = start.clone(), start.clone()
    five = p3d.trace_path_device(dev, ACCELS[accel], rays["origin"], rays["direction"], depth, samples=5, rng=carried, want=())["rgb"]
    total.zero_()
    for s in range(5):
        one(s, rng=chained, flags=ACC, want=(), out={"rgb": total})
    assert_bits(five.cpu().numpy(), total.cpu().numpy(), "five samples of one stream over %s" % accel)
    assert bool((carried == chained).all()) and bool((carried[:, 0] != start[:, 0]).all()) and bool((carried[:, 1] == start[:, 1]).all())
    assert dev.status() == 0


# ---- 4. lanes are independent ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_shuffled_rays_and_prefixes(accel, scenes):
    import torch
    dev = scenes("path_glass")
    cfg = pt_cfg(accel, 2, 6)
    rays = p3d.camera_sample_rays_device(dev, cfg, 1)
    n = rays["origin"].shape[0]
    want_rgb, want_hit = path(dev, accel, rays, 6, rng=rays["rng"].clone(), samples=2)
    perm = np.random.default_rng(5).permutation(n)
    t_perm = torch.from_numpy(perm).cuda()
    origin, direction, states = (rays[k][t_perm].contiguous() for k in ("origin", "direction", "rng"))
    for m in (1, 63, 64, 65, 129, n):
        part = {"origin": origin[:m].contiguous(), "direction": direction[:m].contiguous()}
        rgb, hit = path(dev, accel, part, 6, rng=states[:m].clone(), samples=2)
        assert_bits(hit, want_hit[perm[:m]], "%d shuffled rays over %s: hit_id" % (m, accel))
        assert_bits(rgb, want_rgb[perm[:m]], "%d shuffled rays over %s: rgb" % (m, accel))
    assert dev.status() == 0


# ---- 5. a live scene -------------------------------------------------------------------------------------------------------------------

def test_behind_pose_device_on_one_stream(tmp_path):
    import torch
    mv = sh.STUDIO_MOVE
    studio = str(tmp_path / "studio.p3f")
    with open(studio, "w") as f:
        f.write(sh.STUDIO.replace("resolution 64 64", "resolution %d %d" % RES))
    posed = p3d.HostScene(studio)
    dev_a = p3d.DeviceScene(posed, bvh="device")  # (no device-built grid: pose_device refuses those scenes)
    dev_b = p3d.DeviceScene(p3d.HostScene(studio), bvh="device")
    rays = pixel_rays(dev_b)
    before = path(dev_b, "bvh", rays, 5, samples=2, seed=SEED)[0]
    assert dev_a.transform_prims(mv["ranges"], mv["xforms"], p3d.UPDATE_REFIT, sphere_scale=mv["sphere_scale"]) > 0
    dev_b.set_rig(mv["ranges"], len(mv["xforms"]))
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        d_x = torch.from_numpy(np.ascontiguousarray(mv["xforms"], np.float32)).cuda(non_blocking=True)
        d_s = torch.from_numpy(mv["sphere_scale"]).cuda(non_blocking=True)
        dev_b.pose_device(d_x, d_s, stream=side)
        got = {a: p3d.trace_path_device(dev_b, ACCELS[a], rays["origin"], rays["direction"], 5, samples=2, seed=SEED, stream=side) for a in ("bvh", "none")}
    side.synchronize()
    for accel, out in got.items():
        rgb, hit = path(dev_a, accel, rays, 5, samples=2, seed=SEED)
        assert_bits(out["hit_id"].cpu().numpy(), hit, "after pose_device over %s: hit_id" % accel)
        assert_bits(out["rgb"].cpu().numpy(), rgb, "after pose_device over %s: rgb" % accel)
        assert (f32_bits(rgb) != f32_bits(before)).any(axis=1).sum() > 100, "the move shows nowhere"
    assert dev_a.status() == 0 and dev_b.status() == 0


# ---- 6. refusals on the device ---------------------------------------------------------------------------------------------------------

def empty_scene_with_a_grid():
    """A scene of no objects under a one-cell grid: the host's loader gives no grid to an empty scene, so the descriptor is made
    by hand and handed to p3d_scene_create; a DeviceScene around the handle"""
    hs = p3d.HostScene(scene_path("balls_medium.p3f"))  # no objects with the shipped parser
    d = p3d.SceneDesc.from_buffer_copy(hs.desc(False, False))
    assert d.n_prims == 0
    start = (C.c_uint32 * 2)(0, 0)
    d.has_grid = 1
    d.grid.bmin[:], d.grid.bmax[:] = (0, 0, 0), (1, 1, 1)
    d.grid.nx = d.grid.ny = d.grid.nz = d.grid.n_cells = 1
    d.grid.n_items = 0
    d.grid.cell_start, d.grid.cell_items = C.cast(start, C.POINTER(C.c_uint32)), None
    dev = p3d.DeviceScene.__new__(p3d.DeviceScene)
    dev._L, dev.device, dev.host, dev.res = p3d.lib(), 0, hs, (d.camera.res_x, d.camera.res_y)
    h = C.c_void_p()
    rc = dev._L.p3d_scene_create(C.byref(d), 0, C.byref(h))
    assert rc == 0, dev._L.p3d_last_error()
    dev._h = h
    return dev


def test_refusals_enqueue_nothing(scenes):
    import torch
    dev = scenes("path_mirror")
    rays = pixel_rays(dev, SUB_TILE)
    n = rays["origin"].shape[0]
    query, inputs = dq.trace_path(4), {"d_origin": rays["origin"], "d_direction": rays["direction"]}
    out = dq.check_buffer_refusals(query, dev, inputs, n)
    rng = torch.full((n + 1, 2), 9, dtype=torch.int64, device="cuda")
    host = np.zeros((n, 3), np.float32)
    empty = empty_scene_with_a_grid()
    no_grid = p3d.DeviceScene(p3d.HostScene(scene_path("path_mirror.p3f")), bvh=True)
    q = lambda accel=p3d.ACCEL_BVH, d=dev, other=query, **more: other.call(d, accel, dict(inputs, **more), query.optional, 0, out)
    dq.assert_refused([
        # d_rng is checked behind the outputs: the contract's count cannot guard it, so it is refused here with n good rows
        ("a misaligned rng", INVALID, "8-byte aligned", lambda: q(d_rng=(rng.data_ptr() + 4, n))),
        ("a host rng", INVALID, "host memory", lambda: q(d_rng=(host.ctypes.data, n))),
        ("the skybox without a cubemap", INVALID, "cubemap", lambda: q(other=dq.trace_path(4, flags=p3d.RADIANCE_SKYBOX))),
        ("a grid over an empty scene", UNSUPPORTED, "empty scene", lambda: q(accel=p3d.ACCEL_GRID, d=empty)),
        ("the object loop over no grid", INVALID, "without a grid", lambda: q(accel=p3d.ACCEL_GRID, d=no_grid)),
    ])
    L = p3d.lib()
    good = dict(inputs, d_rgb=out["rgb"])
    for what, word, other, bufs in [
        ("max_depth 1025", "max_depth", dq.trace_path(1025), good), ("max_depth -1", "max_depth", dq.trace_path(-1), good),
        ("samples = 0", "samples", dq.trace_path(4, samples=0), good), ("samples past 2^32", "2^32", dq.trace_path(4, samples=2, sample_begin=0xffffffff), good),
        ("a flag bit", "unknown flag", dq.trace_path(4, flags=4), good), ("a misaligned rgb", "aligned", query, dict(good, d_rgb=out["rgb"].data_ptr() + 2)),
    ]:
        assert other.raw(dev, p3d.ACCEL_BVH, n, **bufs) == INVALID, what
        assert word in L.p3d_last_error().decode(), "%s: %s" % (what, L.p3d_last_error())
    dq.check_empty_batch(query, dev)
    dq.assert_untouched(out)
    assert bool((rng == 9).all()), "a refused call wrote"
    assert dq.trace_path(4, sample_begin=0xffffffff).raw(dev, p3d.ACCEL_BVH, n, **good) == 0  # the last sample number there is
    assert dev.status() == 0 and empty.status() == 0

"""What a ray sees, for rays in device memory (p3d_trace_radiance_device), and a camera's rays (p3d_camera_rays_device).

The yardstick is exact.  camera_rays_device must give the oracle's Scene.primary_ray(x + .5, y + .5) in every bit, and for
those rays trace_radiance_device must give the floats and hit IDs of the P3D_STACK_PER_PIXEL frame of the same camera without
anti-aliasing, in every bit: the query runs the level body of the frame kernels in the same per-lane order on the same kind
of stack, and test_gpu_kernel_variants.py shows that a frame's bits do not depend on the kernel variant it was rendered by.
Tolerance 0 everywhere but in the float64 model test, which takes shading_reference.check_frame unchanged.  Frames are at
most 64 x 48 (the model's fixed frames: 64 x 64)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, scene_path
import device_query_contract as dq
from device_query_contract import INVALID
from frame_checks import ACCELS, assert_bits, f32_bits, tile_of
from oracle import binding as ob
import p3d_amd as p3d
import shading_reference as sh

pytestmark = pytest.mark.gpu

RES = (64, 48)
SMALL = (48, 40)       # the glass / TIR scenes
SUB_TILE = (5, 7, 27, 13)  # x0, y0, w, h: a width that is no multiple of 8, rows that start inside a wave tile
VIEW_A = dict(from_=(-1.6, 2.2, 1.1), at=(0.1, 0, 0.1), up=(0, 0, 1), angle=50.0)  # of balls_low
VIEW_B = dict(from_=(0.4, -2.6, 0.9), at=(0, 0.2, 0), up=(0, 0, 1), angle=38.0)


def frame(dev, accel, depth, tile=None, skybox=0):
    """The per-pixel frame without anti-aliasing -> (rgb (n, 3), hit (n,)) in the tile's row order"""
    cfg = p3d.whitted_config(accel=ACCELS[accel], max_depth=depth, stack_mode=p3d.STACK_PER_PIXEL, skybox=skybox)
    rgb, hit = dev.render(cfg, tile=tile_of(tile))[:2]
    return rgb.reshape(-1, 3), hit.reshape(-1)


def radiance(dev, accel, rays, depth, **kw):
    out = p3d.trace_radiance_device(dev, ACCELS[accel], rays["origin"], rays["direction"], depth, **kw)
    return out["rgb"].cpu().numpy(), out["hit_id"].cpu().numpy()


def check_view(dev, accel, depth, what, camera=None, tile=None):
    """the radiance of the camera's rays against the frame of that camera (the scene's current one)"""
    rays = p3d.camera_rays_device(dev, camera=camera, tile=tile_of(tile))
    rgb, hit = radiance(dev, accel, rays, depth)
    f_rgb, f_hit = frame(dev, accel, depth, tile)
    what = "%s over %s, depth %d" % (what, accel, depth)
    assert_bits(hit, f_hit, what + ": hit_id")
    assert_bits(rgb, f_rgb, what + ": rgb")
    return f_rgb, f_hit


def host(path, res):
    hs = p3d.HostScene(path)
    hs.set_resolution(*res)
    return hs


def build(hs, device_built):
    return p3d.DeviceScene(hs, bvh="device", grid="device") if device_built else p3d.DeviceScene(hs, bvh=True, grid=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the scenes of shading_reference (studio also seen from SECOND_VIEW) at SMALL, so that no resolution is set afterwards"""
    d = tmp_path_factory.mktemp("radiance")
    texts = dict(sh.SCENES, second_view=sh.STUDIO_SECOND_VIEW)
    paths = {}
    for name, text in texts.items():
        assert "resolution 64 64" in text
        paths[name] = str(d / (name + ".p3f"))
        with open(paths[name], "w") as f:
            f.write(text.replace("resolution 64 64", "resolution %d %d" % SMALL))
    return paths


def oracle_rays(sc, x0, y0, w, h):
    o, d = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    for r in range(h):
        for c in range(w):
            o[r, c], d[r, c] = sc.primary_ray(x0 + c + .5, y0 + r + .5)
    return o.reshape(-1, 3), d.reshape(-1, 3)


# ---- 1. camera rays --------------------------------------------------------------------------------------------------------------------

def test_camera_rays_are_the_oracles_primary_rays(files):
    import torch
    dev = p3d.DeviceScene(p3d.HostScene(files["studio"]), bvh=True)
    views = [("the scene's camera", None, ob.Scene(files["studio"])),
             ("a look_at camera", p3d.look_at(res=SMALL, **sh.SECOND_VIEW), ob.Scene(files["second_view"]))]
    for what, cam, sc in views:
        assert sc.resolution() == SMALL
        for tile in (None, SUB_TILE):
            x0, y0, w, h = tile or (0, 0) + SMALL
            rays = p3d.camera_rays_device(dev, camera=cam, tile=tile_of(tile))
            assert rays["origin"].shape == (w * h, 3) and rays["direction"].dtype == torch.float32
            o, d = oracle_rays(sc, x0, y0, w, h)
            assert_bits(rays["origin"].cpu().numpy(), o, "%s, tile %s: origin" % (what, tile))
            assert_bits(rays["direction"].cpu().numpy(), d, "%s, tile %s: direction" % (what, tile))
    # the frame of balls_low at a resolution set after loading, as the parity runs below use it
    hs, sc = host(scene_path("balls_low.p3f"), RES), ob.Scene(scene_path("balls_low.p3f"))
    sc.set_resolution(*RES)
    rays = p3d.camera_rays_device(p3d.DeviceScene(hs, bvh=True))
    o, d = oracle_rays(sc, 0, 0, *RES)
    assert_bits(rays["origin"].cpu().numpy(), o, "balls_low: origin")
    assert_bits(rays["direction"].cpu().numpy(), d, "balls_low: direction")


def test_camera_rays_refusals(files):
    import torch
    dev = p3d.DeviceScene(p3d.HostScene(files["studio"]), bvh=True)
    n = SMALL[0] * SMALL[1]
    good = {"origin": torch.zeros((n, 3), device="cuda"), "direction": torch.zeros((n, 3), device="cuda")}
    L, h = p3d.lib(), dev._h
    o, d = good["origin"].data_ptr(), good["direction"].data_ptr()
    lens = p3d.look_at(res=SMALL, aperture_ratio=0.05, focal_ratio=1.5, **sh.SECOND_VIEW)
    assert lens.aperture != 0
    other = p3d.look_at(res=(32, 32), **sh.SECOND_VIEW)
    for what, code, word, call in [
        ("a lens camera", -3, "lens", lambda: L.p3d_camera_rays_device(h, C.byref(lens), None, o, d, None)),
        ("another resolution", -1, "32x32", lambda: L.p3d_camera_rays_device(h, C.byref(other), None, o, d, None)),
        ("a tile outside", -1, "tile", lambda: L.p3d_camera_rays_device(h, None, C.byref(p3d.Tile(40, 0, 16, 8, 0, 1)), o, d, None)),
        ("a null buffer", -1, "null argument", lambda: L.p3d_camera_rays_device(h, None, None, o, None, None)),
        ("a misaligned buffer", -1, "aligned", lambda: L.p3d_camera_rays_device(h, None, None, o + 2, d, None)),
    ]:
        assert call() == code, what
        assert word in L.p3d_last_error().decode(), "%s: %s" % (what, L.p3d_last_error())
    torch.cuda.synchronize()
    assert not good["origin"].any() and not good["direction"].any(), "a refused call wrote"


# ---- 2. frame parity, tolerance 0 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device_built", [False, True], ids=["host-built", "device-built"])
@pytest.mark.parametrize("name", ["balls_low"] + list(sh.NO_PLANES))
def test_radiance_of_the_cameras_rays_is_the_per_pixel_frame(name, device_built, files):
    hs = host(scene_path("balls_low.p3f"), RES) if name == "balls_low" else p3d.HostScene(files[name])
    dev = build(hs, device_built)
    res = dev.res
    what = "%s, %s" % (name, "device-built" if device_built else "host-built")
    lit = 0
    for accel in ACCELS:
        for depth in (0, 1, 4):
            f_rgb, f_hit = check_view(dev, accel, depth, what)
            lit += int((f_hit >= 0).sum())
            if depth == 4 and accel == "bvh":
                deeper = frame(dev, accel, 0)[0]
                assert (f32_bits(deeper) != f32_bits(f_rgb)).any(axis=1).sum() > 50, "%s: the chain adds nothing to the frame" % what
    assert lit > 9 * res[0] * res[1] // 8
    check_view(dev, "bvh", 4, what + ", sub-tile", tile=SUB_TILE)
    check_view(dev, "none", 1, what + ", sub-tile", tile=SUB_TILE)
    view = VIEW_A if name == "balls_low" else sh.SECOND_VIEW
    cam = p3d.look_at(res=res, **view)
    rays = p3d.camera_rays_device(dev, camera=cam)  # before the scene has the camera: the rays are the argument's
    dev.set_camera(cam)
    assert_bits(rays["direction"].cpu().numpy(), p3d.camera_rays_device(dev)["direction"].cpu().numpy(), what + ": look_at rays")
    for accel in ACCELS:
        check_view(dev, accel, 4, what + ", look_at view")
    assert dev.status() == 0


def test_planes_through_the_object_loop(files):
    dev = p3d.DeviceScene(p3d.HostScene(files["planes"]), bvh=False, grid=False)
    for depth in (0, 1, 4):
        check_view(dev, "none", depth, "planes")
    assert dev.status() == 0


def test_a_tree_deeper_than_the_window(tri5k_path):
    """the device-built tree over 5000 triangles is deeper than the 16-entry LDS window: the stack's backing array is in use"""
    dev = p3d.DeviceScene(host(tri5k_path, (40, 25)), bvh="device")
    assert dev.export_bvh()["bvh_max_depth"] > 16
    for depth in (1, 4):
        f_rgb, f_hit = check_view(dev, "bvh", depth, "tri5k, device tree")
    assert (f_hit >= 0).any() and (f_hit < 0).any()  # rays that shade and rays that leave, both through the deep tree
    assert dev.status() == 0


def test_the_largest_record_block():
    """max_depth 16 between mirrors: sixteen level records per lane, 16 KB behind the window"""
    dev = p3d.DeviceScene(host(scene_path("balls_low.p3f"), RES), bvh=True)
    f16, _ = check_view(dev, "bvh", p3d.RADIANCE_MAX_DEPTH, "balls_low")
    f4, _ = frame(dev, "bvh", 4)
    assert (f32_bits(f16) != f32_bits(f4)).any(), "no chain of this frame is deeper than 4"
    check_view(dev, "none", p3d.RADIANCE_MAX_DEPTH, "balls_low")


# ---- 3. order and batch ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_shuffled_rays_of_three_views_and_prefixes(accel):
    import torch
    dev = p3d.DeviceScene(host(scene_path("balls_low.p3f"), RES), bvh=True, grid=True)
    cams = [None, p3d.look_at(res=RES, **VIEW_A), p3d.look_at(res=RES, **VIEW_B)]
    rays = [p3d.camera_rays_device(dev, camera=c) for c in cams]
    want_rgb, want_hit = [], []
    for c in cams:
        if c is not None:
            dev.set_camera(c)
        rgb, hit = frame(dev, accel, 4)
        want_rgb.append(rgb)
        want_hit.append(hit)
    want_rgb, want_hit = np.concatenate(want_rgb), np.concatenate(want_hit)
    assert len({tuple(r["direction"][0].tolist()) for r in rays}) == 3
    perm = np.random.default_rng(3).permutation(len(want_hit))
    t_perm = torch.from_numpy(perm).cuda()
    origin = torch.cat([r["origin"] for r in rays])[t_perm].contiguous()
    direction = torch.cat([r["direction"] for r in rays])[t_perm].contiguous()
    for n in (1, 63, 64, 65, 4099):
        rgb, hit = radiance(dev, accel, {"origin": origin[:n].contiguous(), "direction": direction[:n].contiguous()}, 4)
        assert_bits(hit, want_hit[perm[:n]], "%d shuffled rays over %s: hit_id" % (n, accel))
        assert_bits(rgb, want_rgb[perm[:n]], "%d shuffled rays over %s: rgb" % (n, accel))
    assert dev.status() == 0


# ---- 4. skybox -------------------------------------------------------------------------------------------------------------------------

def test_skybox_flag():
    dev = p3d.DeviceScene(host(scene_path("balls_low.p3f"), RES), bvh=True, grid=True)
    rays = p3d.camera_rays_device(dev)
    with pytest.raises(p3d.P3DError) as e:
        p3d.trace_radiance_device(dev, p3d.ACCEL_BVH, rays["origin"], rays["direction"], 4, flags=p3d.RADIANCE_SKYBOX)
    assert e.value.code == -1 and "cubemap" in str(e.value)
    dev.set_skybox(p3d.load_skybox_dir(os.path.join(GOLDEN, "skybox")))
    for accel in ACCELS:
        with_sky, hit = radiance(dev, accel, rays, 4, flags=p3d.RADIANCE_SKYBOX)
        f_rgb, f_hit = frame(dev, accel, 4, skybox=1)
        assert_bits(hit, f_hit, "skybox over %s: hit_id" % accel)
        assert_bits(with_sky, f_rgb, "skybox over %s: rgb" % accel)
        without, _ = radiance(dev, accel, rays, 4)
        assert_bits(without, frame(dev, accel, 4, skybox=0)[0], "no flag over %s: rgb" % accel)
        assert (f32_bits(with_sky) != f32_bits(without)).any(axis=1).sum() > 100, "the cubemap shows nowhere"


# ---- 5. the float64 model --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models(tmp_path_factory):
    paths = sh.write_scenes(tmp_path_factory.mktemp("radiance_model"))
    out = {}
    for name in sh.NO_PLANES:
        scene = sh.load_scene(paths[name])
        out[name] = dict(path=paths[name], chain=sh.trace(scene, max_depth=max(sh.DEPTHS)))
    return out


@pytest.mark.parametrize("name", sh.NO_PLANES)
def test_radiance_against_the_float64_model(name, models):
    """The fixed frames of test_gpu_shading_model.py: the radiance of their rays passes check_frame as their frames do."""
    dev = p3d.DeviceScene(p3d.HostScene(models[name]["path"]), bvh=True, grid=True)
    rays = p3d.camera_rays_device(dev)
    w, h = dev.res
    for accel in ACCELS:
        for depth in sh.DEPTHS:
            rgb, hit = radiance(dev, accel, rays, depth)
            sh.check_frame(sh.fold(models[name]["chain"], depth), rgb.reshape(h, w, 3), hit.reshape(h, w), depth,
                           "radiance of %s over %s, depth %d" % (name, accel, depth), lossy_any_hit=accel == "bvh")
    assert dev.status() == 0


# ---- 6. a live scene -------------------------------------------------------------------------------------------------------------------

def test_behind_pose_device_on_one_stream(files):
    import torch
    mv = sh.STUDIO_MOVE
    dev_a = p3d.DeviceScene(p3d.HostScene(files["studio"]), bvh="device")  # (no device-built grid: pose_device refuses those scenes)
    dev_b = p3d.DeviceScene(p3d.HostScene(files["studio"]), bvh="device")
    before = frame(dev_b, "bvh", 4)[0]
    assert dev_a.transform_prims(mv["ranges"], mv["xforms"], p3d.UPDATE_REFIT, sphere_scale=mv["sphere_scale"]) > 0
    dev_b.set_rig(mv["ranges"], len(mv["xforms"]))
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        d_x = torch.from_numpy(np.ascontiguousarray(mv["xforms"], np.float32)).cuda(non_blocking=True)
        d_s = torch.from_numpy(mv["sphere_scale"]).cuda(non_blocking=True)
        dev_b.pose_device(d_x, d_s, stream=side)
        rays = p3d.camera_rays_device(dev_b, stream=side)
        got = {a: p3d.trace_radiance_device(dev_b, ACCELS[a], rays["origin"], rays["direction"], 4, stream=side) for a in ("bvh", "none")}
    side.synchronize()
    for accel, out in got.items():
        f_rgb, f_hit = frame(dev_a, accel, 4)
        assert_bits(out["hit_id"].cpu().numpy(), f_hit, "after pose_device over %s: hit_id" % accel)
        assert_bits(out["rgb"].cpu().numpy(), f_rgb, "after pose_device over %s: rgb" % accel)
        assert (f32_bits(f_rgb) != f32_bits(before)).any(axis=1).sum() > 100, "the move shows nowhere"
    assert dev_a.status() == 0 and dev_b.status() == 0


# ---- 7. outputs ------------------------------------------------------------------------------------------------------------------------

def test_outputs(files):
    import torch
    dev = p3d.DeviceScene(p3d.HostScene(files["glassbox"]), bvh=True)
    rays = p3d.camera_rays_device(dev)
    n = rays["origin"].shape[0]
    query, inputs = dq.trace_radiance(4), {"d_origin": rays["origin"], "d_direction": rays["direction"]}
    both = p3d.trace_radiance_device(dev, p3d.ACCEL_BVH, rays["origin"], rays["direction"], 4)
    dq.check_callers_outputs(query, dev, p3d.ACCEL_BVH, inputs, {name: t.cpu().numpy() for name, t in both.items()}, "glassbox", optional=("hit_id",))
    # raw (address, rows) pairs; a prefix leaves the rows behind it alone
    rows = torch.full((n, 3), -7.0, device="cuda")
    p3d.trace_radiance_device(dev, p3d.ACCEL_BVH, (rays["origin"].data_ptr(), 100), (rays["direction"].data_ptr(), 100), 4, want=(),
                              out={"rgb": (rows.data_ptr(), 100)})
    assert_bits(rows[:100].cpu().numpy(), both["rgb"][:100].cpu().numpy(), "raw pairs")
    assert (rows[100:] == -7.0).all()
    keep = {"origin": torch.empty((n, 3), device="cuda"), "direction": torch.empty((n, 3), device="cuda")}
    assert p3d.camera_rays_device(dev, out=keep)["direction"] is keep["direction"]
    assert_bits(keep["direction"].cpu().numpy(), rays["direction"].cpu().numpy(), "camera rays into out=")
    # what every device query refuses, and the library's own refusals
    outs = dq.check_buffer_refusals(query, dev, inputs, n)
    L = p3d.lib()
    good = dict(inputs, d_rgb=outs["rgb"])
    for what, word, other, accel in [("max_depth 17", "max_depth", dq.trace_radiance(17), p3d.ACCEL_BVH), ("max_depth -1", "max_depth", dq.trace_radiance(-1), p3d.ACCEL_BVH),
                                     ("a flag bit", "unknown flag", dq.trace_radiance(4, flags=2), p3d.ACCEL_BVH), ("no grid", "grid", query, p3d.ACCEL_GRID)]:
        assert other.raw(dev, accel, n, **good) == INVALID, what
        assert word in L.p3d_last_error().decode(), "%s: %s" % (what, L.p3d_last_error())
    assert query.raw(dev, p3d.ACCEL_BVH, n, **dict(good, d_rgb=outs["rgb"].data_ptr() + 2)) == INVALID and b"aligned" in L.p3d_last_error()
    dq.check_empty_batch(query, dev)
    dq.assert_untouched(outs)
    assert dev.status() == 0

"""The kernels' Whitted frames against the float64 shading model of shading_reference.py: the assertions of
test_shading_reference.py with the GPU frame in the oracle's place.  Accel None and grid in full; over a BVH - uploaded or
device-built, literal stack or per pixel - where the model finds every feeler free, and from below elsewhere.

This is the first yardstick of the frames over device-built trees and grids and after update_prims, transform_prims and
set_camera that is not another GPU route.  Nothing here reads the reference tree or the oracle.  Run with -s for the figures.

The sampled modes (anti-aliasing by jitter and tent, the lens, soft shadows, the skybox: sh.SAMPLED_FRAMES) are held to the model's
mean over a pixel's samples, the draws restated by rng_reference: over uploaded and device-built trees and grids, after
transform_prims and set_camera, in the passes of an accumulator, and - the skybox - along rays from device memory."""
import numpy as np
import pytest

from frame_checks import ACCELS
import p3d_amd as p3d
import shading_reference as sh

pytestmark = pytest.mark.gpu

VARIANTS = {"literal": dict(stack_mode=p3d.STACK_LITERAL, collect_stats=1), "per_pixel": dict(stack_mode=p3d.STACK_PER_PIXEL, collect_stats=1),
            "no_counters": dict(stack_mode=p3d.STACK_LITERAL, collect_stats=0)}
BIG = (192, 160)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """The scene files and the model's chains, built once: name -> dict(path, scene, chain); also studio seen from
    SECOND_VIEW, studio after STUDIO_MOVE and studio at 192 x 160."""
    paths = sh.write_scenes(tmp_path_factory.mktemp("shading_gpu"))
    out = {}
    for name, path in paths.items():
        scene = sh.load_scene(path)
        out[name] = dict(path=path, scene=scene, chain=sh.trace(scene, max_depth=max(sh.DEPTHS)))
    studio = out["studio"]["scene"]
    out["second_view"] = dict(chain=sh.trace(studio, cam=sh.camera(res=(64, 64), **sh.SECOND_VIEW), max_depth=4))
    mv = sh.STUDIO_MOVE
    out["moved"] = dict(chain=sh.trace(studio, objects=sh.moved(studio["objects"], mv["ranges"], mv["xforms"], mv["sphere_scale"]), max_depth=4))
    out["big"] = dict(chain=sh.trace(studio, cam=sh.with_resolution(studio["camera"], BIG), max_depth=4))
    return out


def host(models, name, res=None):
    hs = p3d.HostScene(models[name]["path"])
    if res:
        hs.set_resolution(*res)
    return hs


def check(dev, chain, accel, depth, what, **cfg):
    plain = not cfg.get("collect_stats", 1)
    rgb, hit = dev.render(p3d.whitted_config(accel=ACCELS[accel], max_depth=depth, **cfg), stats=not plain)[:2]
    return sh.check_frame(sh.fold(chain, depth), rgb, hit, depth, "%s over %s, depth %d" % (what, accel, depth), lossy_any_hit=accel == "bvh")


def check_all(dev, chain, what, depths=sh.DEPTHS, accels=tuple(ACCELS), **cfg):
    for accel in accels:
        for depth in depths:
            check(dev, chain, accel, depth, what, **cfg)
    assert dev.status() == 0


# ---- the conditions on the frames, from the model alone -----------------------------------------------------------------------------

def test_left_out_cap_and_branch_coverage(models, sampled):
    frames = [sh.fold(m["chain"], depth) for m in models.values() for depth in sh.DEPTHS]
    for name, m in models.items():
        for depth in sh.DEPTHS:
            sh.well_conditioned(sh.fold(m["chain"], depth), "%s depth %d" % (name, depth))
    for (name, mode), chain in sampled["chain"].items():
        for depth in sh.DEPTHS:
            frames.append(sh.fold(chain, depth))
            sh.well_conditioned(frames[-1], "%s, %s, depth %d" % (name, mode, depth))
    sh.check_coverage(frames, "the frames of this module")


# ---- uploaded scenes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", sh.NO_PLANES)
def test_uploaded_scene_against_the_model(name, variant, models):
    dev = p3d.DeviceScene(host(models, name), bvh=True, grid=True)
    check_all(dev, models[name]["chain"], "%s uploaded, %s" % (name, variant), **VARIANTS[variant])


def test_planes_against_the_model(models):
    dev = p3d.DeviceScene(host(models, "planes"), bvh=False, grid=False)
    check_all(dev, models["planes"]["chain"], "planes", accels=("none",), collect_stats=1)


@pytest.mark.parametrize("mode", ["literal", "per_pixel"])
def test_per_level_launches_against_the_model(mode, models):
    """hall is too big for LDS and its glass has Ks = 0, so one launch per chain level takes it under both stack modes."""
    dev = p3d.DeviceScene(host(models, "hall"), bvh=True, grid=False)
    check_all(dev, models["hall"]["chain"], "hall, one launch per level, %s" % mode, depths=(1, 2, 4), accels=("bvh",),
              chain_launch=p3d.CHAIN_PER_LEVEL, **VARIANTS[mode])


# ---- device-built trees and grids -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sh.NO_PLANES)
def test_device_built_scene_against_the_model(name, models):
    dev = p3d.DeviceScene(host(models, name), bvh="device", grid="device")
    check_all(dev, models[name]["chain"], "%s device-built, literal" % name, accels=("bvh", "grid"), **VARIANTS["literal"])
    check_all(dev, models[name]["chain"], "%s device-built, per pixel" % name, depths=(4,), accels=("bvh",), **VARIANTS["per_pixel"])
    check_all(dev, models[name]["chain"], "%s device-built, no counters" % name, depths=(4,), accels=("bvh", "grid"), **VARIANTS["no_counters"])


def moved_rows(hs):
    rest = hs.arrays()
    mv = sh.STUDIO_MOVE
    return p3d.transformed(rest["prim_type"], rest["prim_v"], mv["ranges"], mv["xforms"], mv["sphere_scale"])


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_after_update_prims_against_the_model(mode, models):
    """A rigid motion of the spheres (which also grow), the wall and the cube scaled by another factor per axis: the model
    gets the float64 result of the same matrices."""
    hs = host(models, "studio")
    dev = p3d.DeviceScene(hs, bvh="device", grid="device")
    check(dev, models["studio"]["chain"], "bvh", 2, "studio before the move", **VARIANTS["literal"])
    objs, rows = moved_rows(hs)
    hs.set_geometry(objs, rows)
    assert dev.update_prims(objs, p3d.UPDATE_REFIT if mode == "refit" else p3d.UPDATE_REBUILD) > 0
    check_all(dev, models["moved"]["chain"], "studio after update_prims (%s)" % mode, depths=(0, 4), **VARIANTS["literal"])
    check_all(dev, models["moved"]["chain"], "studio after update_prims (%s), per pixel" % mode, depths=(4,), accels=("bvh",), **VARIANTS["per_pixel"])


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_after_transform_prims_against_the_model(mode, models):
    dev = p3d.DeviceScene(host(models, "studio"), bvh="device", grid="device")
    mv = sh.STUDIO_MOVE
    assert dev.transform_prims(mv["ranges"], mv["xforms"], p3d.UPDATE_REFIT if mode == "refit" else p3d.UPDATE_REBUILD,
                               sphere_scale=mv["sphere_scale"]) > 0
    check_all(dev, models["moved"]["chain"], "studio after transform_prims (%s)" % mode, depths=(0, 4), **VARIANTS["literal"])
    check_all(dev, models["moved"]["chain"], "studio after transform_prims (%s), no counters" % mode, depths=(4,), accels=("bvh",), **VARIANTS["no_counters"])


def test_after_set_camera_against_the_model(models):
    dev = p3d.DeviceScene(host(models, "studio"), bvh="device", grid="device")
    check(dev, models["studio"]["chain"], "bvh", 2, "studio, first view", **VARIANTS["literal"])
    dev.set_camera(p3d.look_at(res=(64, 64), **sh.SECOND_VIEW))
    check_all(dev, models["second_view"]["chain"], "studio after set_camera", depths=(0, 4), **VARIANTS["literal"])


def test_large_frame_over_a_device_built_tree(models):
    """192 x 160: several tiles for the cost-ordered schedule and the literal hand-off."""
    dev = p3d.DeviceScene(host(models, "studio", BIG), bvh="device", grid=False)
    for depth in (2, 4):
        check(dev, models["big"]["chain"], "bvh", depth, "studio 192 x 160, device-built", **VARIANTS["literal"])
    check(dev, models["big"]["chain"], "bvh", 4, "studio 192 x 160, device-built, frame order", tile_order=p3d.TILE_ORDER_FRAME, **VARIANTS["literal"])
    assert dev.status() == 0


# ---- the sampled modes ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sampled(tmp_path_factory):
    """dict(path: scene name -> file, scene: -> the model's scene, smp: mode -> sampler, chain: (scene, mode) of
    sh.SAMPLED_FRAMES -> the model's chain to depth 4)"""
    paths = sh.write_scenes(tmp_path_factory.mktemp("sampled_gpu"), sh.SAMPLED_SCENES)
    scenes = {name: sh.load_scene(path) for name, path in paths.items()}
    smp = sh.sampled_modes()
    chain = {(name, mode): sh.trace(scenes[name], cam=sh.sampled_camera(scenes[name], name), max_depth=max(sh.DEPTHS), smp=smp[mode])
             for name, mode in sh.SAMPLED_FRAMES}
    return dict(path=paths, scene=scenes, smp=smp, chain=chain)


def sampled_host(sampled, name):
    hs = p3d.HostScene(sampled["path"][name])
    if name == "calm_big":
        hs.set_resolution(*sh.BIG_RES)
    return hs


def sampled_device(sampled, name, **kw):
    dev = p3d.DeviceScene(sampled_host(sampled, name), **kw)
    dev.set_skybox(sh.skybox_faces())
    return dev


def tile_of(name):
    return p3d.Tile(*sh.BIG_WINDOW, 0, 1) if name == "calm_big" else None


def sampled_config(smp, accel, depth, **cfg):
    return p3d.whitted_config(accel=ACCELS[accel], max_depth=depth, **dict(sh.config_fields(smp), **cfg))


def check_sampled(dev, smp, chain, name, accel, depth, what, **cfg):
    plain = not cfg.get("collect_stats", 1)
    rgb, hit = dev.render(sampled_config(smp, accel, depth, **cfg), tile=tile_of(name), stats=not plain)[:2]
    return sh.check_frame(sh.fold(chain, depth), rgb, hit, depth, "%s over %s, depth %d" % (what, accel, depth), lossy_any_hit=accel == "bvh",
                          kind=sh.kind_of(smp))


def check_sampled_all(dev, sampled, name, mode, what, depths=sh.DEPTHS, accels=tuple(ACCELS), **cfg):
    for accel in accels:
        for depth in depths:
            check_sampled(dev, sampled["smp"][mode], sampled["chain"][name, mode], name, accel, depth, "%s, %s, %s" % (name, mode, what), **cfg)
    assert dev.status() == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,mode", sh.SAMPLED_FRAMES)
def test_sampled_uploaded_scene_against_the_model(name, mode, variant, sampled):
    dev = sampled_device(sampled, name, bvh=True, grid=True)
    check_sampled_all(dev, sampled, name, mode, "uploaded, %s" % variant, **VARIANTS[variant])


@pytest.mark.parametrize("name,mode", [("calm", "soft shadows"), ("calm", "lens disk"), ("calm", "tent"), ("adrift", "skybox"),
                                       ("calm_big", "jitter 2x2"), ("calm_big", "soft shadows 2x2")])
def test_sampled_device_built_scene_against_the_model(name, mode, sampled):
    dev = sampled_device(sampled, name, bvh="device", grid="device")
    check_sampled_all(dev, sampled, name, mode, "device-built, literal", depths=(0, 4), accels=("bvh", "grid"), **VARIANTS["literal"])
    check_sampled_all(dev, sampled, name, mode, "device-built, per pixel", depths=(4,), accels=("bvh",), **VARIANTS["per_pixel"])
    check_sampled_all(dev, sampled, name, mode, "device-built, no counters", depths=(4,), accels=("bvh", "grid"), **VARIANTS["no_counters"])


def test_sampled_frames_visit_every_variant_of_the_sample_loop(sampled):
    """The frames above include four lanes a pixel (sub4) and one, scenes staged in LDS and traversed from L2.  sub4 needs a
    scene traversed from L2, four samples in the launch and a stack that is not handed from sample to sample.  The plan
    refuses one launch per level for every anti-aliased frame (capi_frame_plan.hpp: per_level needs antialiasing = 0), so
    none is among them."""
    plans = {}
    for name in ("calm", "calm_big"):
        dev = sampled_device(sampled, name, bvh=True, grid=True)
        smp = sampled["smp"]["jitter 2x2"]
        for variant in ("literal", "per_pixel"):
            for accel in ACCELS:
                plans[name, variant, accel] = dev.frame_plan(sampled_config(smp, accel, 4, **VARIANTS[variant]), tile=tile_of(name))
        with pytest.raises(p3d.P3DError):
            dev.frame_plan(sampled_config(smp, "bvh", 4, chain_launch=p3d.CHAIN_PER_LEVEL, **VARIANTS["per_pixel"]), tile=tile_of(name))
    assert all(p.lds_scene and not p.sub4 for (name, _, _), p in plans.items() if name == "calm")
    assert not any(p.lds_scene for (name, _, _), p in plans.items() if name == "calm_big")
    assert plans["calm_big", "per_pixel", "bvh"].sub4 and plans["calm_big", "literal", "grid"].sub4 and plans["calm_big", "literal", "none"].sub4
    assert plans["calm_big", "literal", "bvh"].literal and not plans["calm_big", "literal", "bvh"].sub4


CALM_MOVE = dict(ranges=[(0, 2, 0)], xforms=np.stack([sh.rigid((0, 1, 0), 20.0, (0, 0, 0.4), (0.1, 0.2, -0.1))]),
                 sphere_scale=np.array([0.9], np.float32))
CALM_SECOND_VIEW = dict(from_=(1.5, 2.6, 5.8), at=(0, 0.8, 0), up=(0, 1, 0), angle=40.0)


def test_sampled_after_transform_prims_against_the_model(sampled):
    """The two spheres of calm turned about a vertical axis, lifted and shrunk, under soft shadows"""
    scene, smp = sampled["scene"]["calm"], sampled["smp"]["soft shadows"]
    chain = sh.trace(scene, objects=sh.moved(scene["objects"], CALM_MOVE["ranges"], CALM_MOVE["xforms"], CALM_MOVE["sphere_scale"]), max_depth=4, smp=smp)
    dev = sampled_device(sampled, "calm", bvh="device", grid="device")
    assert dev.transform_prims(CALM_MOVE["ranges"], CALM_MOVE["xforms"], p3d.UPDATE_REFIT, sphere_scale=CALM_MOVE["sphere_scale"]) > 0
    for accel in ACCELS:
        for depth in (0, 4):
            check_sampled(dev, smp, chain, "calm", accel, depth, "calm after transform_prims, soft shadows", **VARIANTS["literal"])
    check_sampled(dev, smp, chain, "calm", "bvh", 4, "calm after transform_prims, soft shadows, per pixel", **VARIANTS["per_pixel"])
    assert dev.status() == 0


def test_sampled_after_set_camera_against_the_model(sampled):
    """Another eye with the lens of the scene file, set through set_camera: the tent filter with the disk lens"""
    scene, smp = sampled["scene"]["calm"], sampled["smp"]["tent with lens"]
    chain = sh.trace(scene, cam=sh.camera(res=(64, 64), aperture=2.0, focal=1.0, **CALM_SECOND_VIEW), max_depth=4, smp=smp)
    dev = sampled_device(sampled, "calm", bvh="device", grid="device")
    dev.set_camera(p3d.look_at(res=(64, 64), aperture_ratio=2.0, focal_ratio=1.0, **CALM_SECOND_VIEW))
    for accel in ACCELS:
        for depth in (0, 4):
            check_sampled(dev, smp, chain, "calm", accel, depth, "calm after set_camera, tent with lens", **VARIANTS["literal"])
    assert dev.status() == 0


@pytest.mark.parametrize("name,mode,passes", [("calm", "jitter 3x3", (3, 3, 3)), ("calm", "soft shadows", (3, 3, 3)), ("calm_big", "jitter 2x2", (1, 2, 1))])
def test_accumulator_passes_against_the_model(name, mode, passes, sampled):
    """The image after each pass against the model's mean over the samples so far: the order of the samples and the divisor
    of a partial frame.  (An accumulator refuses the literal stack over a BVH.)"""
    dev = sampled_device(sampled, name, bvh=True, grid=True)
    smp, chain = sampled["smp"][mode], sampled["chain"][name, mode]
    for accel, variant in (("bvh", "per_pixel"), ("grid", "literal"), ("none", "no_counters")):
        acc = dev.accumulator(sampled_config(smp, accel, 4, **VARIANTS[variant]), tile_of(name))
        done = 0
        for n in passes:
            rgb, hit = acc.render(n)[:2]
            done += n
            assert acc.samples_done == done
            frame = sh.fold(chain, 4, samples=done)
            ok = frame["margin"] >= sh.THRESHOLD  # (a partial frame leaves out no more than the whole one: no cap of its own)
            held = ok & frame["free"] if accel == "bvh" else ok
            err = float(np.abs(rgb - frame["rgb"])[held].max())
            print("%s, %s over %s: %d of %d samples, %d pixels, max |colour - model| %.3g" % (name, mode, accel, done, acc.total, int(held.sum()), err))
            assert (hit == frame["hit"])[ok].all() and err <= sh.TOL[sh.kind_of(smp)]
            assert float((frame["rgb"] - rgb)[ok].max()) <= sh.TOL[sh.kind_of(smp)]  # from below where an occluder may be lost
        acc.close()
    assert dev.status() == 0


def test_skybox_along_device_rays_against_the_model(sampled):
    """trace_radiance_device with RADIANCE_SKYBOX: rays from above adrift's objects that miss everything, a handful through
    each face, chosen clear of face and texel edges by the model's margin"""
    import torch
    faces = sh.skybox_faces()
    rng = np.random.default_rng(5)
    d = rng.normal(size=(600, 3))
    d[:, 1] = np.abs(d[:, 1]) * np.where(np.arange(600) % 3 == 0, 1.0, -0.02) + 0.0  # a third go up; the rest are nearly level
    d = np.concatenate([d, [[0.1, -1.0, 0.2], [-0.3, -1.0, 0.1], [0.2, -0.9, -0.5], [0.05, -1.0, -0.3], [-0.2, -1.0, -0.2]]]).astype(np.float32)
    o = np.where(d[:, 1:2] < -0.5, np.float32([30.0, 9.0, 0.0]), np.float32([0.0, 9.0, 0.0])).astype(np.float32)
    colour, face, margin = sh.skybox_lookup(faces, d.astype(np.float64))
    ok = margin >= sh.THRESHOLD
    assert all(((face == f) & ok).sum() >= 5 for f in range(6))
    dev = sampled_device(sampled, "adrift", bvh=True, grid=True)
    for accel in ACCELS:
        out = p3d.trace_radiance_device(dev, ACCELS[accel], torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), 2, flags=p3d.RADIANCE_SKYBOX)
        assert (out["hit_id"].cpu().numpy() == -1).all(), accel
        assert np.abs(out["rgb"].cpu().numpy() - colour)[ok].max() <= 1e-6, accel  # a byte / 255.99 in float32
    assert dev.status() == 0

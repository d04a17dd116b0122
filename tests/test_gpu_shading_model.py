"""The kernels' Whitted frames against the float64 shading model of shading_reference.py: the assertions of
test_shading_reference.py with the GPU frame in the oracle's place.  Accel None and grid in full; over a BVH - uploaded or
device-built, literal stack or per pixel - where the model finds every feeler free, and from below elsewhere.

This is the first yardstick of the frames over device-built trees and grids and after update_prims, transform_prims and
set_camera that is not another GPU route.  Nothing here reads the reference tree or the oracle.  Run with -s for the figures."""
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

def test_left_out_cap_and_branch_coverage(models):
    frames = [sh.fold(m["chain"], depth) for m in models.values() for depth in sh.DEPTHS]
    for name, m in models.items():
        for depth in sh.DEPTHS:
            sh.well_conditioned(sh.fold(m["chain"], depth), "%s depth %d" % (name, depth))
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

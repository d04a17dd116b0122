"""The CPU oracle's Whitted frames against the float64 shading model of shading_reference.py, without a GPU: one ray per pixel,
maximum depth 0, 1, 2 and 4, over the authored scenes of the model's module.

  accel None and grid   shadows are brute force (Q6): on well-conditioned pixels the primary hit ID is the model's and every
                        colour component is within shading_reference.TOL.
  the oracle's BVH      its any-hit can lose an occluder but never invent one (Q1): the same where the model finds every feeler
                        of the chain free; elsewhere every component is at least the model's minus the tolerance.

Every frame asserts the 15 % cap on the pixels left out; the module's frames together must show every branch of the chain in at
least 50 well-conditioned pixels.  Run with -s to see the shares, the counts and the errors behind MEASURED."""
import numpy as np
import pytest

import shading_reference as sh
from oracle import binding as ob

ACCELS = {"none": 0, "grid": 1, "bvh": 2}
FRAMES = [(name, accel) for name in sh.NO_PLANES for accel in ACCELS] + [("planes", "none")]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """name -> (oracle scene, the model's scene, the model's chain to depth 4)"""
    paths = sh.write_scenes(tmp_path_factory.mktemp("shading"))
    out = {}
    for name, path in paths.items():
        model = sh.load_scene(path)
        out[name] = (ob.Scene(path), model, sh.trace(model, max_depth=max(sh.DEPTHS)))
    return out


# ---- the model by itself ----------------------------------------------------------------------------------------------------------

ONE_PIXEL = """bclr 0.25 0.5 0.75
v
from 0 0 5
at 0 0 0
up 0 1 0
angle 30
hither 0.01
resolution 1 1
aperture 0
focal 1
l 0 0 10 0.5 0.5 0.5
f 0.8 0.4 0.2 0.5 1 1 1 %s 20 %s 1.5 0 0 0
s 0 0 0 1
"""


def one_pixel(tmp_path, ks, t, depth):
    path = tmp_path / "one_pixel.p3f"
    path.write_text(ONE_PIXEL % (ks, t))
    return sh.fold(sh.trace(sh.load_scene(str(path)), max_depth=depth), depth)


def test_model_closed_form_local_term_and_mirror(tmp_path):
    """The one ray meets the sphere head on with the light behind the eye: N = l = h = (0, 0, 1), so the local term is
    Kd cd col + Ks cs col, and the mirror ray goes straight back into the background."""
    f = one_pixel(tmp_path, "0.5", "0", 0)
    local = 0.5 * np.array([0.8, 0.4, 0.2]) * 0.5 + 0.5 * 0.5
    assert np.allclose(f["rgb"][0, 0], local, rtol=0, atol=1e-7) and f["hit"][0, 0] == 0 and f["levels"][0, 0] == 1
    f = one_pixel(tmp_path, "0.5", "0", 1)
    assert np.allclose(f["rgb"][0, 0], local + 0.5 * np.array([0.25, 0.5, 0.75]), rtol=0, atol=1e-7)
    assert f["has"]["miss after a bounce"][0, 0] and f["has"]["opaque bounce"][0, 0] and f["has"]["lit"][0, 0]


def test_model_closed_form_glass(tmp_path):
    """Head on through a glass ball: straight in, straight out (no shading inside, weight 1 and no Fresnel term), then the
    background; with depth 1 the chain ends inside, where nothing is lit."""
    local = 0.5 * np.array([0.8, 0.4, 0.2]) * 0.5 + 0.5 * 0.5
    f = one_pixel(tmp_path, "0.5", "0.9", 2)
    assert np.allclose(f["rgb"][0, 0], np.minimum(1.0, local + np.array([0.25, 0.5, 0.75])), rtol=0, atol=1e-7)
    assert f["has"]["enter"][0, 0] and f["has"]["leave"][0, 0] and f["has"]["inner-level clamp"][0, 0] == False
    f = one_pixel(tmp_path, "0.5", "0.9", 1)
    assert np.allclose(f["rgb"][0, 0], local, rtol=0, atol=1e-7)


def test_model_clamps_every_level(tmp_path):
    """A mirror of Ks 0.5 showing a background of 3: the level below is not clamped (a miss), this one is."""
    path = tmp_path / "bright.p3f"
    path.write_text((ONE_PIXEL % ("0.5", "0")).replace("bclr 0.25 0.5 0.75", "bclr 3 3 3"))
    f = sh.fold(sh.trace(sh.load_scene(str(path)), max_depth=1), 1)
    assert (f["rgb"][0, 0] == 1.0).all()


def test_the_models_scene_is_the_oracles(scenes):
    for name, (sc, model, _) in scenes.items():
        c = sc.counts()
        assert (c["objects"], c["lights"], c["materials"]) == (len(model["objects"]), len(model["lights"]), len(model["materials"])), name
        assert (sc.background() == model["bclr"]).all(), name
        for i, light in enumerate(model["lights"]):
            assert (np.concatenate(sc.light(i)) == light).all(), (name, i)
        for i, m in enumerate(model["materials"]):
            assert (sc.material(i)[:11] == m[:11]).all(), (name, i)
        for i, k in enumerate(model["material"]):
            assert sc.object(i)["material"] == k, (name, i)


def test_primary_rays_against_the_oracle(scenes):
    sc, model, _ = scenes["glassbox"]
    o, d = sh.primary_rays(model["camera"])
    for x, y in ((0, 0), (63, 0), (17, 40), (63, 63)):
        oo, dd = sc.primary_ray(x + 0.5, y + 0.5)
        assert np.abs(dd - d[y * 64 + x]).max() <= 4 * sh.geo.ULP and (oo == o[0]).all(), (x, y)


# ---- the conditions on the frames, from the model alone -----------------------------------------------------------------------------

def test_left_out_cap_and_branch_coverage(scenes):
    frames = []
    for name, (_, _, chain) in scenes.items():
        for depth in sh.DEPTHS:
            frames.append(sh.fold(chain, depth))
            _, share = sh.well_conditioned(frames[-1], "%s depth %d" % (name, depth))
            print("%s depth %d: %.1f %% of the pixels left out" % (name, depth, 100 * share))
    sh.check_coverage(frames, "the frames of this module")


# ---- the oracle against the model ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", sh.DEPTHS)
@pytest.mark.parametrize("name,accel", FRAMES)
def test_oracle_frame_against_the_model(name, accel, depth, scenes):
    sc, _, chain = scenes[name]
    rgb, hit, _ = sc.render(ob.whitted_config(ACCELS[accel], depth))
    sh.check_frame(sh.fold(chain, depth), rgb, hit, depth, "oracle %s over %s, depth %d" % (name, accel, depth), lossy_any_hit=accel == "bvh")


def test_the_bvh_rule_has_something_to_hold(scenes):
    """Both halves of the rule for the BVH see pixels: chains with every feeler free, and chains with a shadowed one."""
    for name in sh.NO_PLANES:
        f = sh.fold(scenes[name][2], 4)
        ok = f["margin"] >= sh.THRESHOLD
        assert (ok & f["free"]).sum() > 500 and (ok & ~f["free"]).sum() > 500, name


# ---- the views and the moved geometry of the GPU suite, checked here against the oracle first ----------------------------------------

def test_oracle_second_view_against_the_model(tmp_path):
    path = tmp_path / "second.p3f"
    path.write_text(sh.STUDIO_SECOND_VIEW)
    model = sh.load_scene(str(path))
    assert all((model["camera"][k] == sh.camera(res=(64, 64), **sh.SECOND_VIEW)[k]).all() for k in ("from_", "at", "up"))
    chain = sh.trace(model, max_depth=4)
    sc = ob.Scene(str(path))
    for accel in ACCELS:
        rgb, hit, _ = sc.render(ob.whitted_config(ACCELS[accel], 4))
        sh.check_frame(sh.fold(chain, 4), rgb, hit, 4, "oracle studio, second view, over %s" % accel, lossy_any_hit=accel == "bvh")


def test_oracle_moved_scene_against_the_model(tmp_path):
    """The move of the GPU suite's update tests, written into a scene file in float32: the oracle loads it, the model gets the
    float64 result of the same matrices."""
    from scene_update_helpers import write_moved_p3f
    src = tmp_path / "studio.p3f"
    src.write_text(sh.STUDIO)
    model = sh.load_scene(str(src))
    objects = sh.moved(model["objects"], sh.STUDIO_MOVE["ranges"], sh.STUDIO_MOVE["xforms"], sh.STUDIO_MOVE["sphere_scale"])
    ids = [i for first, count, _ in sh.STUDIO_MOVE["ranges"] for i in range(first, first + count)]
    kinds = np.array([o["kind"] for o in objects])
    dst = write_moved_p3f(str(src), str(tmp_path / "moved.p3f"), kinds, ids, sh.geometry_rows(objects, ids))
    chain = sh.trace(model, objects=objects, max_depth=4)
    still = sh.fold(sh.trace(model, max_depth=4), 4)
    assert (np.abs(sh.fold(chain, 4)["rgb"] - still["rgb"]).max(-1) > 0.05).mean() > 0.2, "the move changes too little"
    sc = ob.Scene(dst)
    for accel in ACCELS:
        for depth in (0, 4):
            rgb, hit, _ = sc.render(ob.whitted_config(ACCELS[accel], depth))
            sh.check_frame(sh.fold(chain, depth), rgb, hit, depth, "oracle studio, moved, over %s, depth %d" % (accel, depth), lossy_any_hit=accel == "bvh")

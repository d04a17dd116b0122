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

def test_left_out_cap_and_branch_coverage(scenes, sampled):
    frames = [sh.fold(chain, depth) for _, _, chain in sampled.values() for depth in sh.DEPTHS]
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


# ---- the sampled modes: anti-aliasing, the tent filter, the lens, soft shadows, the skybox ----------------------------------------------

def test_vectorised_rng_is_the_scalar_one():
    """rng_reference's numpy streams against its Python-integer functions (which test_trace_path_api.py holds to the oracle):
    seeds, pixels and samples at both ends of their ranges, 64 draws each."""
    import rng_reference as rr
    pixel = np.array([0, 1, 63 * 64 + 63, 96 * 80 - 1, 2 ** 31, 2 ** 32 - 1])
    sample = np.array([0, 8, 3, 255, 2 ** 32 - 1, 1])
    for seed in (0, sh.SEED, 2 ** 64 - 1):
        state, inc = rr.seed_stream_v(seed, pixel, sample)
        scalar = [rr.seed_stream(seed, int(p), int(s)) for p, s in zip(pixel, sample)]
        assert [(int(a), int(b)) for a, b in zip(state, inc)] == scalar
        for _ in range(64):
            state, draw = rr.next31_v(state, inc)
            scalar = [rr.next31(st, ic) + (ic,) for st, ic in scalar]
            assert [int(a) for a in state] == [st for st, _, _ in scalar] and [int(d) for d in draw] == [d for _, d, _ in scalar]
            scalar = [(st, ic) for st, _, ic in scalar]


def test_model_draws_are_the_oracles_stream():
    """The model's float32 and double numbers of a draw, against the integers of oracle.binding.rng_stream"""
    d = sh._Draws(sh.SEED, np.array([5 * 64 + 7]), np.array([3]))
    ints = ob.rng_stream(sh.SEED, 5 * 64 + 7, 3, 3).astype(np.int64)
    at = np.arange(1)
    assert d.rand(at)[0] == float(np.float32(ints[0]) / np.float32(2.0 ** 31)) and d.erand(at)[0] == ints[1] / (2.0 ** 31 - 1)
    assert d.rand(at)[0] == float(np.float32(ints[2]) / np.float32(2.0 ** 31))


def test_skybox_lookup_closed_form():
    """Along each axis the texel is the middle one of that face (the two nearest texels of an even side); the helper cubemap's faces and neighbouring texels differ."""
    faces = sh.skybox_faces()
    eye = np.eye(3)
    d = np.stack([-eye[0], eye[0], eye[1], -eye[1], eye[2], -eye[2]]) * 3.0 + 1e-3 * np.array([0.3, 0.2, 0.1])
    colour, face, margin = sh.skybox_lookup(faces, d)
    assert face.tolist() == [0, 1, 2, 3, 4, 5] and (margin > 0.1).sum() == 4  # (the two faces of odd sides: their middle is a texel edge)
    for k, f in enumerate(faces):
        h, w = f.shape[:2]
        assert margin[k] < 0.1 or np.allclose(colour[k], f[(h - 1) // 2, (w - 1) // 2, :3] / 255.99, rtol=0, atol=1e-7), k
        assert (np.abs(np.diff(f[..., :3].astype(int), axis=1)).max(-1) >= 20).all() and (np.abs(np.diff(f[..., :3].astype(int), axis=0)).max(-1) >= 20).all()
    # +x: s grows with z, t with y; a direction towards +z and +y lands right of and above the middle
    c, f, _ = sh.skybox_lookup(faces, np.array([[1.0, 0.5, 0.25]]))
    h, w = faces[1].shape[:2]
    assert f[0] == 1 and np.allclose(c[0], faces[1][int((h - 1) * 0.75), int((w - 1) * 0.625), :3] / 255.99, rtol=0, atol=1e-7)


def test_lens_rays_meet_in_the_plane_of_focus(tmp_path):
    """Every lens point's ray through one image position goes through the same point, focal x |at - from| along the view
    axis; the lens points lie in the plane through the eye."""
    path = tmp_path / "calm.p3f"
    path.write_text(sh.CALM)
    cam = sh.load_scene(str(path))["camera"]
    assert cam["aperture"] == 2.0 and cam["focal"] == 1.0
    lens = (np.array([0.0, 1.0, -0.7, 0.3]), np.array([0.0, -1.0, 0.2, 0.9]))
    o, d = sh.camera_rays(cam, np.full(4, 40.25), np.full(4, 11.5), lens)
    f = cam["at"] - cam["from_"]
    dist = np.sqrt(f @ f)
    t = dist / (d @ (f / dist))
    meet = o + t[:, None] * d
    assert np.abs(meet - meet[0]).max() < 1e-12 and np.abs((o - cam["from_"]) @ f).max() < 1e-12
    assert (o[0] == cam["from_"]).all() and np.abs(d[0] - sh.camera_rays(cam, np.array([40.25]), np.array([11.5]))[1][0]).max() < 1e-15
    width = 2 * dist * np.tan(np.radians(cam["angle"]) / 2) / 64
    assert abs(np.linalg.norm(o[1] - o[0]) - 2.0 * width * np.sqrt(2)) < 1e-12


@pytest.fixture(scope="module")
def sampled(tmp_path_factory):
    """(scene, mode) of sh.SAMPLED_FRAMES -> (oracle scene, sampler, the model's chain to depth 4)"""
    paths = sh.write_scenes(tmp_path_factory.mktemp("sampled"), sh.SAMPLED_SCENES)
    modes = sh.sampled_modes()
    oracle, model, out = {}, {}, {}
    for name, path in paths.items():
        oracle[name], model[name] = ob.Scene(path), sh.load_scene(path)
        oracle[name].set_skybox(sh.skybox_faces())
    oracle["calm_big"].set_resolution(*sh.BIG_RES)
    for name, mode in sh.SAMPLED_FRAMES:
        out[name, mode] = (oracle[name], modes[mode], sh.trace(model[name], cam=sh.sampled_camera(model[name], name), max_depth=max(sh.DEPTHS), smp=modes[mode]))
    return out


def test_sampled_left_out_cap(sampled):
    """The 15 % cap on every sampled frame, from the model alone (test_left_out_cap_and_branch_coverage counts their
    branches together with those of the one-ray frames).  The largest share
    left out over depths 0, 1, 2 and 4, in per cent of the pixels (a pixel is left out when any of its samples is):
      calm      jitter 2x2 9.7, jitter 3x3 12.2, tent 11.5, soft shadows 11.9, lens square 12.5, lens disk 14.8,
                tent with lens (2x2) 11.0, soft shadows with lens (2x2) 11.1, skybox 12.9
      adrift    skybox 12.2, skybox with one sample 5.0
      calm_big  (43 x 37 of 96 x 80) jitter 2x2 13.8, soft shadows 2x2 14.0
    The scenes of the one-ray frames leave out 22 to 34 % at these sample counts (studio) and 17 to 22 % (glassbox): the
    sampled modes have scenes of their own, with fewer edges."""
    frames = []
    for (name, mode), (_, _, chain) in sampled.items():
        for depth in sh.DEPTHS:
            frames.append(sh.fold(chain, depth))
            _, share = sh.well_conditioned(frames[-1], "%s, %s, depth %d" % (name, mode, depth))
            print("%s, %s, depth %d: %.1f %% of the pixels left out" % (name, mode, depth, 100 * share))


ACCEL_SAMPLED = [(name, mode, accel) for name, mode in sh.SAMPLED_FRAMES for accel in ACCELS]


@pytest.mark.parametrize("depth", sh.DEPTHS)
@pytest.mark.parametrize("name,mode,accel", ACCEL_SAMPLED)
def test_oracle_sampled_frame_against_the_model(name, mode, accel, depth, sampled):
    sc, smp, chain = sampled[name, mode]
    tile = sh.BIG_WINDOW if name == "calm_big" else ()
    rgb, hit, _ = sc.render(ob.whitted_config(ACCELS[accel], depth, **sh.config_fields(smp)), *tile)
    sh.check_frame(sh.fold(chain, depth), rgb, hit, depth, "oracle %s, %s, over %s, depth %d" % (name, mode, accel, depth),
                   lossy_any_hit=accel == "bvh", kind=sh.kind_of(smp))


def test_partial_means_of_the_model(sampled):
    """fold(samples=k), what the GPU suite holds an accumulator's passes to: the first k samples in the order s = i * spp + j,
    the first sample's hit ID, margins that only shrink as samples are added, and all nine samples give the whole frame."""
    _, _, chain = sampled["calm", "jitter 3x3"]
    full = sh.fold(chain, 4)
    parts = [sh.fold(chain, 4, samples=k) for k in (3, 6, 9)]
    assert np.array_equal(parts[2]["rgb"], full["rgb"]) and (parts[0]["margin"] >= parts[1]["margin"]).all() and (parts[1]["margin"] >= full["margin"]).all()
    assert (parts[0]["hit"] == full["hit"]).all()
    assert np.abs(parts[0]["rgb"] - full["rgb"]).max() > 0.05  # the samples differ: a partial mean is not the full one

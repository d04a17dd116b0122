"""Camera updates and temporal accumulation (p3d_camera_look_at / p3d_scene_set_camera / p3d_temporal, include/p3d.h) without
a GPU: the entry points are exported, declared and wrapped, the p3d_accum / p3d_adaptive / denoise sets and the ABI version are
untouched, p3d_camera_look_at rebuilds every shipped scene's camera byte for byte, the parameters are checked, the front end
refuses bad --frames / --orbit / --temporal options before it loads a scene, and the numpy statement of the formula behaves on
hand-made cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from api_checks import cli, header_code, refused
from conftest import ROOT, SCENES, scene_path
import p3d_amd as p3d
from temporal_reference import TemporalReference, primary_dirs

CAMERA_SYMBOLS = ["p3d_camera_look_at", "p3d_scene_set_camera", "p3d_scene_camera", "p3d_host_scene_view"]
TEMPORAL_SYMBOLS = ["p3d_temporal_params_default", "p3d_temporal_create", "p3d_temporal_destroy", "p3d_temporal_reset",
                    "p3d_temporal_frames", "p3d_temporal_accumulate", "p3d_temporal_accumulate_device"]
DENOISE_SYMBOLS = ["p3d_render_features", "p3d_render_features_device", "p3d_denoise_params_default", "p3d_denoiser_create",
                   "p3d_denoiser_destroy", "p3d_denoise", "p3d_denoise_device", "p3d_denoise_variance",
                   "p3d_denoise_variance_device"]
ADAPTIVE_SYMBOLS = ["p3d_adaptive_create", "p3d_adaptive_destroy", "p3d_adaptive_reset", "p3d_adaptive_samples_done",
                    "p3d_adaptive_active_pixels", "p3d_adaptive_render", "p3d_adaptive_render_device",
                    "p3d_adaptive_read_state"]
ACCUM_SYMBOLS = ["p3d_accum_create", "p3d_accum_destroy", "p3d_accum_reset", "p3d_accum_samples_done", "p3d_accum_render",
                 "p3d_accum_render_device"]
ALL_SCENES = sorted([os.path.join(SCENES, f[:-3] if f.endswith(".gz") else f) for f in os.listdir(SCENES)
                     if f.endswith((".p3f", ".p3f.gz"))] +
                    [os.path.join(ROOT, "scenes", f) for f in os.listdir(os.path.join(ROOT, "scenes")) if f.endswith(".p3f")])


def test_library_exports_the_new_entry_points():
    lib = p3d.lib()
    for name in CAMERA_SYMBOLS + TEMPORAL_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS, name
    assert lib.p3d_abi_version() == 4


def test_header_declares_them_and_leaves_the_older_sets_alone():
    code = header_code()
    assert "typedef struct p3d_temporal p3d_temporal;" in code and "p3d_temporal_params;" in code
    assert set(re.findall(r"\b(p3d_temporal_[a-z_]+)\s*\(", code)) == set(TEMPORAL_SYMBOLS)
    for name in CAMERA_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert set(re.findall(r"\b(p3d_(?:render_features|denoise|denoiser)[a-z_]*)\s*\(", code)) == set(DENOISE_SYMBOLS)
    assert set(re.findall(r"\b(p3d_adaptive_[a-z_]+)\s*\(", code)) == set(ADAPTIVE_SYMBOLS)
    assert set(re.findall(r"\b(p3d_accum_[a-z_]+)\s*\(", code)) == set(ACCUM_SYMBOLS)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)


def test_python_wrappers():
    assert [f for f, _ in p3d.TemporalParams._fields_] == ["alpha", "alpha_moments", "max_history", "depth_tolerance",
                                                           "normal_tolerance", "variance_min_history", "sigma_normal",
                                                           "sigma_depth", "reserved"]
    assert C.sizeof(p3d.TemporalParams) == 40
    for name in ("run", "run_device", "reset", "frames", "close"):
        assert hasattr(p3d.Temporal, name), name
    assert hasattr(p3d.DeviceScene, "set_camera") and isinstance(p3d.DeviceScene.camera, property)
    d = p3d.temporal_params()
    assert (d.alpha, d.alpha_moments, d.max_history, d.variance_min_history) == (np.float32(0.2), np.float32(0.2), 32.0, 4)
    assert (d.depth_tolerance, d.normal_tolerance) == (np.float32(0.1), np.float32(0.9))
    assert (d.sigma_normal, d.sigma_depth) == (128.0, 1.0) and list(d.reserved) == [0, 0]
    assert p3d.temporal_params(alpha=0.0, max_history=1e6).alpha == 0.0


def _v_block(path):
    """The `v` block of a .p3f as text -> (from, at, up, angle, resolution, aperture, focal), float32 / int."""
    words = open(path).read().split()
    i = words.index("v")
    kv = {}
    for key, n in (("from", 3), ("at", 3), ("up", 3), ("angle", 1), ("hither", 1), ("resolution", 2), ("aperture", 1),
                   ("focal", 1)):
        i = words.index(key, i)
        kv[key] = words[i + 1:i + 1 + n]
        i += n
    f = lambda xs: [np.float32(x) for x in xs]
    return (f(kv["from"]), f(kv["at"]), f(kv["up"]), np.float32(kv["angle"][0]), [int(x) for x in kv["resolution"]],
            np.float32(kv["aperture"][0]), np.float32(kv["focal"][0]))


@pytest.mark.parametrize("path", ALL_SCENES, ids=os.path.basename)
def test_look_at_rebuilds_every_shipped_scene_camera(path):
    path = scene_path(os.path.basename(path)) if path.startswith(SCENES) else path
    hs = p3d.HostScene(path)
    fr, at, up, angle, res, ap, foc = _v_block(path)
    v = hs.view()
    assert list(v["from_"]) == fr and list(v["at"]) == at and list(v["up"]) == up
    assert (v["angle"], v["aperture_ratio"], v["focal_ratio"]) == (angle, ap, foc)
    cam = p3d.look_at(fr, at, up, angle, res, ap, foc)
    assert bytes(cam) == bytes(hs.desc().camera)
    hs.set_resolution(96, 40)  # another resolution: what p3d_host_scene_set_resolution rebuilds
    assert bytes(p3d.look_at(fr, at, up, angle, (96, 40), ap, foc)) == bytes(hs.desc().camera)
    hs.set_lens(2.0, 1.5)
    assert bytes(p3d.look_at(fr, at, up, angle, (96, 40), 2.0, 1.5)) == bytes(hs.desc().camera)


def test_look_at_refuses_a_bad_resolution():
    for res in ((0, 10), (10, -1)):
        with pytest.raises(p3d.P3DError) as e:
            p3d.look_at((0, 0, 1), (0, 0, 0), (0, 1, 0), 45, res)
        assert e.value.code == -1


def _accumulate_rc(prm):
    """p3d_temporal_accumulate without an object: the parameters are checked first, so this needs no device."""
    L = p3d.lib()
    cam = p3d.look_at((0, 0, 1), (0, 0, 0), (0, 1, 0), 45, (4, 4))
    buf = np.zeros(64, np.float32)
    rc = L.p3d_temporal_accumulate(None, C.byref(prm), C.byref(cam), buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                   buf.ctypes.data, None, None)
    return rc, L.p3d_last_error().decode()


def test_params_are_checked():
    nan = float("nan")
    bad = [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan), dict(alpha_moments=2.0), dict(max_history=0.5),
           dict(max_history=nan), dict(depth_tolerance=0.0), dict(depth_tolerance=float("inf")), dict(normal_tolerance=1.5),
           dict(normal_tolerance=-2.0), dict(sigma_normal=-1.0), dict(sigma_depth=nan), dict(variance_min_history=(1 << 24) + 1),
           dict(reserved=(0, 1))]
    for kw in bad:
        rc, msg = _accumulate_rc(p3d.temporal_params(**kw))
        assert rc == -1 and "null argument" not in msg, (kw, msg)
    for kw in (dict(), dict(alpha=0.0, alpha_moments=1.0, max_history=1.0, normal_tolerance=-1.0, sigma_normal=0.0,
                            sigma_depth=0.0, variance_min_history=0)):
        rc, msg = _accumulate_rc(p3d.temporal_params(**kw))
        assert rc == -1 and "null argument" in msg, (kw, msg)  # good parameters: only the missing object is refused


def test_cli_refuses_bad_frames_orbit_and_temporal():
    pt = ["x.p3f", "--pathtrace", "--aa", "1"]
    for v in ("0", "-2", "abc", "2.5", "", "1001"):
        refused(cli(*pt, "--frames", v), "--frames")
    for v in ("nan", "inf", "abc", ""):
        refused(cli(*pt, "--frames", "2", "--orbit", v), "--orbit")
    refused(cli(*pt, "--orbit", "2"), "--orbit")
    refused(cli(*pt, "--temporal", "--denoise", "d.png"), "--temporal")
    refused(cli(*pt, "--frames", "3", "--temporal"), "--temporal")
    refused(cli("x.p3f", "--whitted", "--aa", "1", "--frames", "3", "--temporal", "--denoise", "d.png"), "--whitted")
    refused(cli(*pt, "--frames", "3", "--passes", "2"), "--passes")
    refused(cli(*pt, "--frames", "3", "--gpus", "2"), "--gpus")


# ---- the numpy statement on hand-made cases ----

def _flat_frame(h, w, t=4.0, cov=1.0, colour=(0.5, 0.25, 0.125)):
    nd = np.zeros((h, w, 4), np.float32)
    nd[..., 2] = 1.0
    nd[..., 3] = t
    ac = np.zeros((h, w, 4), np.float32)
    ac[..., :3] = 0.5
    ac[..., 3] = cov
    rgb = np.broadcast_to(np.array(colour, np.float32), (h, w, 3)).copy()
    return rgb, nd, ac


def test_reference_first_frame_is_the_frame():
    cam = p3d.look_at((0, 0, 4), (0, 0, 0), (0, 1, 0), 40, (12, 9))
    rng = np.random.default_rng(3)
    rgb, nd, ac = _flat_frame(9, 12)
    rgb = rng.random((9, 12, 3)).astype(np.float32)
    ref = TemporalReference(12, 9)
    out, var, n, info = ref.run(cam, rgb, nd, ac)
    assert np.array_equal(out, rgb.astype(np.float64)) and (n == 1).all() and not info["ambiguous"].any()


def test_reference_static_camera_is_a_running_mean():
    cam = p3d.look_at((0, 0, 4), (0, 0, 0), (0, 1, 0), 40, (10, 8))
    rng = np.random.default_rng(4)
    _, nd, ac = _flat_frame(8, 10)
    ref = TemporalReference(10, 8)
    frames = [rng.random((8, 10, 3)).astype(np.float32) for _ in range(6)]
    for f in frames:
        out, var, n, _ = ref.run(cam, f, nd, ac, alpha=0.0, alpha_moments=0.0, max_history=100.0)
    assert (n == 6).all()
    assert np.allclose(out, np.mean(np.array(frames, np.float64), 0), rtol=1e-6)
    Y = np.array([(0.2126 * f[..., 0] + 0.7152 * f[..., 1]) + 0.0722 * f[..., 2] for f in np.array(frames, np.float64)])
    assert np.allclose(var, Y.var(0), rtol=1e-5, atol=1e-7)  # n >= 4: the temporal moments' variance


def test_reference_primary_dirs_are_unit_and_centred():
    cam = p3d.look_at((1, 2, 3), (0, 0, 0), (0, 0, 1), 45, (5, 3))
    d = primary_dirs(cam, 5, 3).astype(np.float64)
    assert np.allclose(np.linalg.norm(d, axis=-1), 1, atol=1e-6)
    centre = d[1, 2]  # the middle pixel of an odd-sized image looks along -n
    assert np.allclose(centre, -np.array(cam.n[:]), atol=1e-6)


def test_reference_sideways_pan_shifts_the_history():
    w, h, pan = 16, 6, 1.0
    c0 = p3d.look_at((0, 0, 4), (0, 0, 0), (0, 1, 0), 40, (w, h))
    c1 = p3d.look_at((pan, 0, 4), (pan, 0, 0), (0, 1, 0), 40, (w, h))
    rgb, nd0, ac = _flat_frame(h, w)
    nd1 = nd0.copy()
    # a wall at z = 0 facing the camera: t is the distance along each pixel-centre ray
    for c, nd in ((c0, nd0), (c1, nd1)):
        nd[..., 3] = (4.0 / -primary_dirs(c, w, h).astype(np.float64)[..., 2]).astype(np.float32)
    ref = TemporalReference(w, h)
    ref.run(c0, rgb, nd0, ac)
    out, _, n, info = ref.run(c1, rgb * 2, nd1, ac)
    shift = pan / (2 * 4 * np.tan(np.radians(20)) / h)  # the wall moves this many pixels to the left
    assert 1 < shift < 3
    x = np.arange(w)
    assert (n[:, x + shift >= w] == 1).all() and (n[:, x + shift < w - 1e-2] == 2).all(), n
    assert np.allclose(out[:, x + shift < w - 1e-2], 1.5 * rgb[0, 0])  # the mean of the two frames
    assert not info["ambiguous"].any()

"""Denoising (p3d_render_features / p3d_denoise / p3d_denoise_variance, include/p3d.h) without a GPU: the entry points are
exported, declared and wrapped, the p3d_accum / p3d_adaptive sets and the ABI version are untouched, the front end refuses
bad --denoise options before it loads a scene, and the numpy statement of the filter behaves on hand-made cases."""
import re

import numpy as np

from api_checks import cli, header_code, refused
from atrous_reference import atrous
import p3d_amd as p3d

DENOISE_SYMBOLS = ["p3d_render_features", "p3d_render_features_device", "p3d_denoise_params_default", "p3d_denoiser_create",
                   "p3d_denoiser_destroy", "p3d_denoise", "p3d_denoise_device", "p3d_denoise_variance",
                   "p3d_denoise_variance_device"]
ADAPTIVE_SYMBOLS = ["p3d_adaptive_create", "p3d_adaptive_destroy", "p3d_adaptive_reset", "p3d_adaptive_samples_done",
                    "p3d_adaptive_active_pixels", "p3d_adaptive_render", "p3d_adaptive_render_device",
                    "p3d_adaptive_read_state"]
ACCUM_SYMBOLS = ["p3d_accum_create", "p3d_accum_destroy", "p3d_accum_reset", "p3d_accum_samples_done", "p3d_accum_render",
                 "p3d_accum_render_device"]


def test_library_exports_the_denoise_entry_points():
    lib = p3d.lib()
    for name in DENOISE_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.p3d_abi_version() == 4


def test_header_declares_them_and_leaves_accum_and_adaptive_alone():
    code = header_code()
    assert "typedef struct p3d_denoiser p3d_denoiser;" in code
    assert "p3d_denoise_params" in code
    declared = set(re.findall(r"\b(p3d_(?:render_features|denoise|denoiser)[a-z_]*)\s*\(", code))
    assert declared == set(DENOISE_SYMBOLS)
    assert set(re.findall(r"\b(p3d_adaptive_[a-z_]+)\s*\(", code)) == set(ADAPTIVE_SYMBOLS)
    assert set(re.findall(r"\b(p3d_accum_[a-z_]+)\s*\(", code)) == set(ACCUM_SYMBOLS)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)


def test_python_wrappers():
    assert [f for f, _ in p3d.DenoiseParams._fields_] == ["iterations", "sigma_color", "sigma_luma", "sigma_normal",
                                                          "sigma_depth", "sigma_albedo", "gamma", "reserved"]
    assert hasattr(p3d.DeviceScene, "render_features") and hasattr(p3d.DeviceScene, "render_features_device")
    for name in ("run", "run_device", "close"):
        assert hasattr(p3d.Denoiser, name), name
    assert hasattr(p3d.AdaptiveAccumulator, "variance") and hasattr(p3d.AdaptiveAccumulator, "variance_device")
    d = p3d.denoise_params()
    assert d.iterations == 5 and d.sigma_normal == 128.0 and d.sigma_luma == 64.0 and d.gamma == 1.0
    assert list(d.reserved) == [0, 0]
    assert p3d.denoise_params(iterations=2, sigma_albedo=0.0).iterations == 2
    for name in DENOISE_SYMBOLS:
        assert name in p3d.EXPORTS


def test_cli_refuses_denoise_with_whitted_or_gpus():
    refused(cli("x.p3f", "--whitted", "--aa", "1", "--denoise", "d.png"), "--whitted")
    refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--gpus", "2", "--denoise", "d.png"), "--gpus")
    refused(cli("x.p3f", "--pathtrace", "--aa", "0", "--denoise", "d.png"), "--aa")


def test_cli_refuses_malformed_values():
    for v in ("-1", "9", "abc", "2x", ""):
        refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--denoise", "d.png", "--denoise-iter", v), "--denoise-iter")
    for v in ("-1", "abc", "4.5"):
        refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--denoise", "d.png", "--feature-spp", v), "--feature-spp")
    refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--spp", "2", "--denoise", "d.png", "--feature-spp", "5"), "--feature-spp")
    refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--denoise-iter", "3"), "--denoise")
    refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--denoise"), "--denoise")


def _features(h, w, normal=(0.0, 0.0, 1.0), t=5.0, albedo=(0.5, 0.5, 0.5), cov=1.0):
    nd = np.zeros((h, w, 4))
    nd[..., :3] = normal
    nd[..., 3] = t
    ac = np.zeros((h, w, 4))
    ac[..., :3] = albedo
    ac[..., 3] = cov
    return nd, ac


def test_reference_zero_iterations_is_the_identity():
    rng = np.random.default_rng(1)
    rgb = rng.random((9, 13, 3))
    var = rng.random((9, 13))
    nd, ac = _features(9, 13)
    out, v = atrous(rgb, nd, ac, var, iterations=0)
    assert np.array_equal(out, rgb) and np.array_equal(v, var)


def test_reference_keeps_a_constant_image_constant():
    rgb = np.full((20, 17, 3), 0.3)
    nd, ac = _features(20, 17)
    ac[5:9, 4:12, 3] = 0.0  # uncovered patch: a region of its own, still the same colour
    nd[5:9, 4:12] = 0.0
    ac[5:9, 4:12, :3] = 0.0
    for var in (None, np.full((20, 17), 0.01)):
        out, _ = atrous(rgb, nd, ac, var, iterations=4)
        assert np.allclose(out, 0.3, rtol=0, atol=1e-12)


def test_reference_does_not_mix_orthogonal_half_planes():
    h, w = 16, 24
    rgb = np.zeros((h, w, 3))
    rgb[:, : w // 2] = (1.0, 0.0, 0.0)
    rgb[:, w // 2:] = (0.0, 0.0, 1.0)
    rng = np.random.default_rng(2)
    rgb += rng.normal(0, 0.05, rgb.shape)
    nd, ac = _features(h, w)
    nd[:, w // 2:, :3] = (1.0, 0.0, 0.0)  # the right half faces another way
    out, _ = atrous(rgb, nd, ac, None, iterations=5, sigma_color=1e3, sigma_depth=0.0, sigma_albedo=0.0)
    left, right = out[:, : w // 2], out[:, w // 2:]
    # each half is the mean of its own noisy pixels: no red on the right, no blue on the left
    assert np.abs(left[..., 2]).max() < 0.05 and np.abs(right[..., 0]).max() < 0.05
    assert np.allclose(left[..., 0], 1.0, atol=0.05) and np.allclose(right[..., 2], 1.0, atol=0.05)
    # ... whereas with the normal term off the halves do blend along the edge
    mixed, _ = atrous(rgb, nd, ac, None, iterations=5, sigma_color=1e3, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
    assert mixed[:, w // 2 - 1, 2].mean() > 0.2

"""Adaptive sampling (p3d_adaptive, include/p3d.h) without a GPU: the entry points are exported, declared and wrapped, the
p3d_accum set and the ABI version are untouched, and the front end refuses a malformed --adaptive before it loads a scene."""
import re

from api_checks import cli, header_code, refused
import p3d_amd as p3d

ADAPTIVE_SYMBOLS = ["p3d_adaptive_create", "p3d_adaptive_destroy", "p3d_adaptive_reset", "p3d_adaptive_samples_done",
                    "p3d_adaptive_active_pixels", "p3d_adaptive_render", "p3d_adaptive_render_device",
                    "p3d_adaptive_read_state"]
ACCUM_SYMBOLS = ["p3d_accum_create", "p3d_accum_destroy", "p3d_accum_reset", "p3d_accum_samples_done", "p3d_accum_render",
                 "p3d_accum_render_device"]


def test_library_exports_the_adaptive_entry_points():
    lib = p3d.lib()
    for name in ADAPTIVE_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.p3d_abi_version() == 4


def test_header_declares_them_and_leaves_the_accumulator_alone():
    code = header_code()
    assert "typedef struct p3d_adaptive p3d_adaptive;" in code
    assert "p3d_adaptive_params" in code
    assert set(re.findall(r"\b(p3d_adaptive_[a-z_]+)\s*\(", code)) == set(ADAPTIVE_SYMBOLS)
    assert set(re.findall(r"\b(p3d_accum_[a-z_]+)\s*\(", code)) == set(ACCUM_SYMBOLS)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)


def test_python_wrapper():
    assert hasattr(p3d, "AdaptiveAccumulator")
    for name in ("render", "render_device", "reset", "close", "samples_done", "active_pixels", "read_state"):
        assert hasattr(p3d.AdaptiveAccumulator, name), name
    assert hasattr(p3d.DeviceScene, "adaptive") and hasattr(p3d.DeviceScene, "render_adaptive")
    assert [f for f, _ in p3d.AdaptiveParams._fields_] == ["rel_error", "min_samples", "reserved"]


def test_cli_refuses_adaptive_without_passes():
    refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--adaptive", "0.05"), "--passes")


def test_cli_refuses_adaptive_with_whitted_or_gpus():
    refused(cli("x.p3f", "--whitted", "--aa", "1", "--passes", "2", "--adaptive", "0.05"), "--whitted")
    refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--gpus", "2", "--passes", "2", "--adaptive", "0.05"), "--gpus")


def test_cli_refuses_a_bad_threshold():
    for v in ("-0.1", "abc", "0.05x", "nan"):
        refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--passes", "2", "--adaptive", v), "--adaptive")
    refused(cli("x.p3f", "--pathtrace", "--passes", "2", "--adaptive"), "--adaptive")


def test_cli_refuses_min_spp_out_of_range():
    refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--spp", "4", "--passes", "2", "--adaptive", "0.05", "--min-spp", "1"),
             "--min-spp")
    refused(cli("x.p3f", "--pathtrace", "--aa", "1", "--spp", "4", "--passes", "2", "--adaptive", "0.05", "--min-spp", "17"),
             "--min-spp")

"""Adaptive sampling (p3d_adaptive, include/p3d.h) without a GPU: the entry points are exported, declared and wrapped, the
p3d_accum set and the ABI version are untouched, and the front end refuses a malformed --adaptive before it loads a scene."""
import os
import re
import subprocess

import p3d_amd as p3d
from conftest import ROOT

ADAPTIVE_SYMBOLS = ["p3d_adaptive_create", "p3d_adaptive_destroy", "p3d_adaptive_reset", "p3d_adaptive_samples_done",
                    "p3d_adaptive_active_pixels", "p3d_adaptive_render", "p3d_adaptive_render_device",
                    "p3d_adaptive_read_state"]
ACCUM_SYMBOLS = ["p3d_accum_create", "p3d_accum_destroy", "p3d_accum_reset", "p3d_accum_samples_done", "p3d_accum_render",
                 "p3d_accum_render_device"]
EXE = os.path.join(ROOT, "p3d-raytracer_amd", "p3d_render")


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p3d.h")).read(), flags=re.S)


def test_library_exports_the_adaptive_entry_points():
    lib = p3d.lib()
    for name in ADAPTIVE_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.p3d_abi_version() == 4


def test_header_declares_them_and_leaves_the_accumulator_alone():
    code = _header_code()
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


def _cli(*args):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "p3d_render"], stdout=subprocess.DEVNULL)
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def _refused(r, option):
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert option in r.stderr and "unknown option" not in r.stderr, r.stderr


def test_cli_refuses_adaptive_without_passes():
    _refused(_cli("x.p3f", "--pathtrace", "--aa", "1", "--adaptive", "0.05"), "--passes")


def test_cli_refuses_adaptive_with_whitted_or_gpus():
    _refused(_cli("x.p3f", "--whitted", "--aa", "1", "--passes", "2", "--adaptive", "0.05"), "--whitted")
    _refused(_cli("x.p3f", "--pathtrace", "--aa", "1", "--gpus", "2", "--passes", "2", "--adaptive", "0.05"), "--gpus")


def test_cli_refuses_a_bad_threshold():
    for v in ("-0.1", "abc", "0.05x", "nan"):
        _refused(_cli("x.p3f", "--pathtrace", "--aa", "1", "--passes", "2", "--adaptive", v), "--adaptive")
    _refused(_cli("x.p3f", "--pathtrace", "--passes", "2", "--adaptive"), "--adaptive")


def test_cli_refuses_min_spp_out_of_range():
    _refused(_cli("x.p3f", "--pathtrace", "--aa", "1", "--spp", "4", "--passes", "2", "--adaptive", "0.05", "--min-spp", "1"),
             "--min-spp")
    _refused(_cli("x.p3f", "--pathtrace", "--aa", "1", "--spp", "4", "--passes", "2", "--adaptive", "0.05", "--min-spp", "17"),
             "--min-spp")

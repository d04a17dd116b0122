"""Progressive accumulation (p3d_accum, include/p3d.h) without a GPU: the entry points are exported, declared and wrapped,
the ABI version is unchanged, and the front end refuses a malformed --passes before it loads a scene."""
import os
import re

from api_checks import cli
from conftest import ROOT
import p3d_amd as p3d

ACCUM_SYMBOLS = ["p3d_accum_create", "p3d_accum_destroy", "p3d_accum_reset", "p3d_accum_samples_done", "p3d_accum_render",
                 "p3d_accum_render_device"]


def test_library_exports_the_accumulator():
    lib = p3d.lib()
    for name in ACCUM_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.p3d_abi_version() == 4


def test_header_declares_the_accumulator():
    hdr = open(os.path.join(ROOT, "include", "p3d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "typedef struct p3d_accum p3d_accum;" in code
    declared = set(re.findall(r"\b(p3d_accum_[a-z_]+)\s*\(", code))
    assert declared == set(ACCUM_SYMBOLS)


def test_python_wrapper():
    assert hasattr(p3d, "Accumulator")
    for name in ("render", "render_device", "reset", "close", "samples_done"):
        assert hasattr(p3d.Accumulator, name), name
    assert hasattr(p3d.DeviceScene, "accumulator") and hasattr(p3d.DeviceScene, "render_progressive")


def test_cli_refuses_zero_passes():
    r = cli("--passes", "0", "x.p3f")
    assert r.returncode == 2
    assert "--passes" in r.stderr and "unknown option" not in r.stderr, r.stderr


def test_cli_refuses_passes_without_a_count():
    r = cli("x.p3f", "--passes")
    assert r.returncode == 2 and "--passes" in r.stderr, r.stderr


def test_cli_refuses_more_passes_than_samples_and_passes_with_gpus():
    r = cli("x.p3f", "--spp", "2", "--aa", "1", "--passes", "5")
    assert r.returncode == 2 and "--passes" in r.stderr, r.stderr
    r = cli("x.p3f", "--gpus", "2", "--passes", "2")
    assert r.returncode == 2 and "--gpus" in r.stderr, r.stderr

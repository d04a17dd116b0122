"""What the *_api.py test modules share: the headers without their comments, the command-line renderer and its refusals, and a
device scene whose library must not be called.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import os
import re
import subprocess

import p3d_amd as p3d
from conftest import ROOT

EXE = os.path.join(ROOT, "p3d-raytracer_amd", "p3d_render")


def header_code(name="p3d.h"):
    """include/<name> with its block comments removed"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def cli(*args):
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "p3d_render"], stdout=subprocess.DEVNULL)
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def refused(r, option):
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert option in r.stderr and "unknown option" not in r.stderr, r.stderr


class Untouchable:
    """Stands where the library would: any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def scene_without_a_library():
    dev = p3d.DeviceScene.__new__(p3d.DeviceScene)
    dev._L, dev._h, dev.device, dev.host = Untouchable(), None, 0, None
    return dev

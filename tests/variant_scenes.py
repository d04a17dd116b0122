"""The scenes of the kernel-variant tests: written or picked once per module, with the layout rule that says how many bytes of
a scene a Whitted frame stages.  tests/test_gpu_kernel_variants.py renders them; tests/test_kernel_variant_scenes.py checks
their sizes without a GPU.  `scene_files` is a module-scoped fixture: a test module that imports it by name gets its own.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import numpy as np
import pytest

import p3d_amd as p3d
from conftest import scene_path
from frame_checks import ACCELS
from fuzz_scenes import random_scene

ACCEL_IDS = list(ACCELS)  # none, grid, bvh
ACCEL_VALUES = list(ACCELS.values())
FRAMES = [(64, 48), (72, 40)]  # several waves per launch and several tile bands, whole tiles
PT_FRAME = (48, 40)


def staged_bytes(path, accel, legacy=False):
    """Bytes of the staged range of a Whitted frame by the layout rule, from the host-side descriptor alone."""
    d = p3d.HostScene(path, legacy_f11=legacy).desc(bvh=True)
    f4 = 2 * d.n_bvh_nodes + 3 * d.n_bvh_prim_index + d.n_prims + 4 * d.n_materials + 2 * d.n_lights
    return 16 * (f4 + (3 * d.n_prims if accel != p3d.ACCEL_BVH else 0))


def write_spheres(path, n, mats, lights, seed=1, glass=0):
    """n spheres on a jittered lattice, the first `mats` of them with
    a material of their own (every second one reflective; with glass = g, every g-th transmissive AND reflective), `lights` lights."""
    rng = np.random.default_rng(seed)
    lines = ["bclr 0.1 0.2 0.3", "v", "from 0 -7 2", "at 0 0 0", "up 0 0 1", "angle 45", "hither 0.01", "resolution 64 64",
             "aperture 0", "focal 1"]
    for k in range(lights):
        lines.append("l %g %g %g 0.6 0.6 0.6" % (3 - 2 * k, -4, 5 + k))
    side = max(1, int(np.ceil(n ** (1 / 3))))
    for k in range(n):
        if k < mats:
            if glass and k % glass == glass - 1:
                lines.append("f %g %g %g 0.3 1 1 1 0.4 40 0.8 1.5 0 0 0" % (0.2 + 0.6 * rng.random(), 0.3, 0.8 * rng.random()))
            else:
                lines.append("f %g %g %g 0.7 1 1 1 %g 20 0 1 0 0 0" % (0.2 + 0.6 * rng.random(), 0.3, 0.8 * rng.random(), 0.3 if k % 2 else 0.0))
        x, y, z = k % side, (k // side) % side, k // (side * side)
        s = 3.0 / side
        lines.append("s %g %g %g %g" % ((x - side / 2 + 0.5) * s + 0.1 * s * rng.random(), (y - side / 2 + 0.5) * s, (z - side / 2 + 0.5) * s, 0.33 * s))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory, tri5k_path):
    d = tmp_path_factory.mktemp("variants")
    return {
        # PT-L2: 543 objects, 104 KB, tree depth 12 - the oracle's deepest stack over the BVH is 11 entries, 3 beyond the window
        "pt_l2": (random_scene(2100, str(d / "pt_l2.p3f"), n_spheres=260, n_tris=260, n_boxes=20, n_lights=0, emitters=3, res=PT_FRAME), False),
        "path_glass": (scene_path("path_glass.p3f"), False),
        # W-SPILL
        "balls_medium": (scene_path("balls_medium.p3f"), True),
        # W-SPILL-GHOSTS: 150 spheres, 40 materials (13 of them glass), 3 lights
        "spill_spheres": (write_spheres(str(d / "spill_spheres.p3f"), 150, 40, 3, glass=3), False),
        # W-L2-GHOSTS: 232 objects, 33 KB over the BVH; the "glass" kind of random_scene is transmissive and reflective
        "l2_ghosts": (random_scene(1000, str(d / "l2_ghosts.p3f"), n_spheres=100, n_tris=120, n_boxes=12, res=FRAMES[0]), False),
        # W-L2
        "tri5k": (tri5k_path, False),
        "balls_low": (scene_path("balls_low.p3f"), False),
    }

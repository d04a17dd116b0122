"""What the tests of the shading updates share (p3d_scene_set_materials, p3d_scene_set_lights, p3d_scene_set_shading_device and
the host setters): seeded material and light values, the twin a changed scene is compared with, the readbacks, tiny scenes
with any number of materials and lights, and the scene file of a changed host scene for the oracle.

"Twin": a fresh DeviceScene of a HostScene given the same values through host_set_materials / host_set_lights, built the same
way.  Every comparison with it is in bits.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import numpy as np

import p3d_amd as p3d
from frame_checks import assert_bits, load
from live_scene_checks import HEAD, legacy

RES = 96
# columns of a (n, 16) material row (p3d_material) and of a (n, 8) light row (p3d_light)
DIFF, KD, SPEC, KS, SHINE, T, IOR, REFL, EMIT = slice(0, 3), 3, slice(4, 7), 7, 8, 9, 10, 11, slice(12, 15)
POS, COL = slice(0, 3), slice(4, 7)
THREADS = 256  # shade::kThreads, the workgroup of the stream form's kernel


def host(path, res=RES):
    return load(path, res, legacy_f11=legacy(path))


def light_rows(lights6):
    """(n, 6) rows of HostScene.arrays()["lights"] -> (n, 8) rows of p3d_light"""
    rows = np.zeros((len(lights6), 8), np.float32)
    rows[:, POS], rows[:, COL] = lights6[:, 0:3], lights6[:, 3:6]
    return rows


def tables(hs):
    """(materials (n, 16), lights (n, 8)) of a host scene"""
    a = hs.arrays()
    return a["materials"].copy(), light_rows(a["lights"])


def seeded(mats, lights, seed):
    """New values for every row, within the ranges the scene files use: diffuse and specular colours and Kd in [0, 1], shine
    in [5, 200], every light moved by up to 1 and coloured in [0.3, 1].  Ks in [0.1, 1] with reflection = Ks, as a loader
    leaves them (so that a scene file can say the same), but only where the material is opaque: a transmissive one keeps
    both, and every material its emission, so that no material changes a predicate the stream form skips for."""
    rng = np.random.default_rng(seed)
    m, l = mats.copy(), lights.copy()
    n = len(m)
    m[:, DIFF], m[:, SPEC] = rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, (n, 3))
    m[:, KD], m[:, SHINE] = rng.uniform(0, 1, n), rng.uniform(5, 200, n)
    ks = rng.uniform(0.1, 1, n).astype(np.float32)
    opaque = m[:, T] == 0
    m[opaque, KS] = m[opaque, REFL] = ks[opaque]
    l[:, POS] += rng.uniform(-1, 1, (len(l), 3)).astype(np.float32)
    l[:, COL] = rng.uniform(0.3, 1, (len(l), 3))
    return m, l


def twin(path, build, mats=None, first_mat=0, lights=None, first_light=0, res=RES):
    """A fresh device scene, made by build(host scene), of the file with the rows set on the HOST -> (host scene, device scene)"""
    hs = host(path, res)
    if mats is not None and len(mats):
        p3d.host_set_materials(hs, first_mat, mats)
    if lights is not None and len(lights):
        p3d.host_set_lights(hs, first_light, lights)
    return hs, build(hs)


def assert_readback(dev, mats, lights, what):
    """The device holds exactly these tables (reserved fields 0)"""
    want_m, want_l = mats.copy(), lights.copy()
    want_m[:, 15] = 0
    want_l[:, 3] = want_l[:, 7] = 0
    assert_bits(p3d.scene_materials(dev), want_m, what + ": materials read back")
    assert_bits(p3d.scene_lights(dev), want_l, what + ": lights read back")


def readback(dev):
    return p3d.scene_materials(dev).tobytes(), p3d.scene_lights(dev).tobytes()


def tiny_scene(path, n_mats, n_lights):
    """A .p3f of n_mats materials, each on a sphere of its own in a square facing the camera, and n_lights lights on a line
    above it.  Every second material has Ks == 0: the materials whose pow the kernels may leave out."""
    head = [line for line in HEAD if not line.startswith(("l ", "f "))]
    lights = ["l %.9g -4 5 %.9g %.9g %.9g" % (3.0 * (i + 0.5) / n_lights - 1.5, 1.0 / n_lights, 1.0 / n_lights, 1.0 / n_lights) for i in range(n_lights)]
    side = int(np.ceil(np.sqrt(n_mats)))
    body = []
    for i in range(n_mats):
        ks = 0.0 if i % 2 == 0 else 0.3
        body.append("f %.9g 0.5 %.9g 0.7 1 1 1 %.9g 20 0 1 0 0 0" % (0.3 + 0.6 * (i % 7) / 7, 0.9 - 0.6 * (i % 5) / 5, ks))
        x, z = (i % side + 0.5) / side * 3.0 - 1.5, (i // side + 0.5) / side * 3.0 - 1.5
        body.append("s %.9g 0 %.9g %.9g" % (x, z, 1.2 / side))
    with open(path, "w") as f:
        f.write("\n".join(head + lights + body) + "\n")
    return path


def changed_file(src, dst, mats, lights):
    """The scene file `src` with its `f` and `l` lines replaced, in order, by these rows (14-number `f` lines: reflection is
    not in the grammar, a loader sets it to Ks).  %.9g names a float32 exactly."""
    assert np.array_equal(mats[:, REFL], mats[:, KS]), "a scene file cannot say reflection != Ks"
    fmt = lambda row: " ".join("%.9g" % x for x in row)
    out, i_m, i_l = [], 0, 0
    for line in open(src).read().split("\n"):
        if line.startswith("f "):
            assert len(line.split()) == 15, line
            out.append("f " + fmt(np.concatenate([mats[i_m, 0:11], mats[i_m, EMIT]])))
            i_m += 1
        elif line.startswith("l "):
            out.append("l " + fmt(np.concatenate([lights[i_l, POS], lights[i_l, COL]])))
            i_l += 1
        else:
            out.append(line)
    assert i_m == len(mats) and i_l == len(lights)
    with open(dst, "w") as f:
        f.write("\n".join(out))
    return dst

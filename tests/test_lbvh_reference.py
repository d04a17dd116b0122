"""The model of the device BVH builder (lbvh_reference.py) and the synthetic scenes it is compared on, checked without a GPU:
the model's trees are trees over their objects, its depth is the depth of its own arrays, and the degenerate scenes are as
degenerate as the GPU tests take them to be."""
import numpy as np
import pytest

from conftest import scene_path
import lbvh_reference as ref
import p3d_amd as p3d

SYNTHETIC = {name: (objects, view) for name, objects, view in ref.synthetic_scenes()}
COUNTS = [1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513]


@pytest.fixture(scope="module")
def arrays(tmp_path_factory, tri5k_path):
    """name -> HostScene.arrays() of every scene of this module, loaded once"""
    tmp = tmp_path_factory.mktemp("lbvh")
    paths = {name: ref.write_p3f(str(tmp / (name + ".p3f")), objects, view) for name, (objects, view) in SYNTHETIC.items()}
    for n in COUNTS:
        paths["count%d" % n] = ref.write_p3f(str(tmp / ("count%d.p3f" % n)), ref.counts_scene(n))
    paths.update(balls_low=scene_path("balls_low.p3f"), path_glass=scene_path("path_glass.p3f"), tri5k=tri5k_path)
    return {name: p3d.HostScene(path).arrays() for name, path in paths.items()}


NAMES = list(SYNTHETIC) + ["count%d" % n for n in COUNTS] + ["balls_low", "path_glass", "tri5k"]


@pytest.mark.parametrize("name", NAMES)
def test_the_model_builds_a_tree_over_its_objects(name, arrays):
    a = arrays[name]
    tree = ref.build(a["prim_bmin"], a["prim_bmax"])
    n = a["n_prims"]
    ref.check_boxes(tree, a, name)
    assert tree["bvh_max_depth"] == ref.measured_depth(tree)
    leaves = int(((tree["bvh_count_leaf"] & ref.LEAF) != 0).sum())
    assert len(tree["bvh_index"]) == 2 * leaves - 1 and n / 2 <= leaves <= n
    assert 1 + int(np.ceil(np.log2(n))) <= tree["bvh_max_depth"] <= min(n, 63)  # a binary tree of n leaves; a path splits on at most 62 key bits
    keys = ref.sorted_keys(a["prim_bmin"], a["prim_bmax"])
    assert (np.diff(keys.astype(np.int64)) > 0).all()  # unique (and below 2^62: the int64 view is safe)


def test_no_object_no_tree():
    tree = ref.build(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert tree["bvh_max_depth"] == 0 and all(len(tree[k]) == 0 for k in ref.TREE_KEYS)


def test_a_hand_made_tree():
    """Four unit boxes at x = 0, 1, 2, 3 (cells 0, 341, 682, 1023 of x): the codes differ in the top x bit between objects 1 and
    2, so the root's children are two leaves of two; given out of order, the order array sorts them"""
    x = np.array([3, 0, 2, 1], np.float32)
    bmin = np.stack([x, np.zeros(4, np.float32), np.zeros(4, np.float32)], 1)
    tree = ref.build(bmin, bmin + np.float32(1))
    assert tree["bvh_order"].tolist() == [1, 3, 2, 0]
    assert tree["bvh_index"].tolist() == [1, 0, 2] and tree["bvh_count_leaf"].tolist() == [0, ref.LEAF | 2, ref.LEAF | 2]
    assert tree["bvh_max_depth"] == 3
    assert tree["bvh_bmin"].tolist() == [[0, 0, 0], [0, 0, 0], [2, 0, 0]] and tree["bvh_bmax"].tolist() == [[4, 1, 1], [2, 1, 1], [4, 1, 1]]
    # three objects: [0] | [1, 2] in sorted order -> the root is an inner node with a leaf of one and a leaf of two
    three = ref.build(bmin[1:], bmin[1:] + np.float32(1))  # x = 0, 2, 1 -> cells 0, 1023, 512
    assert three["bvh_order"].tolist() == [0, 2, 1]
    assert three["bvh_index"].tolist() == [1, 0, 1] and three["bvh_count_leaf"].tolist() == [0, ref.LEAF | 1, ref.LEAF | 2]
    assert three["bvh_max_depth"] == 3


def test_the_morton_code_puts_x_on_top():
    lo = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32)
    code = ref.morton_codes(lo, lo)
    full = sum(1 << (3 * i) for i in range(10))
    assert code.tolist() == [0, full << 2, full << 1, full, (full << 2) | (full << 1) | full]
    assert int(code.max()) == (1 << 30) - 1


def test_refit_moves_boxes_and_nothing_else(arrays):
    a = arrays["tri5k"]
    tree = ref.build(a["prim_bmin"], a["prim_bmax"])
    moved = dict(a)
    moved["prim_bmin"] = a["prim_bmin"] + np.float32(0.25) * (np.arange(a["n_prims"]) % 3 == 0)[:, None].astype(np.float32)
    moved["prim_bmax"] = moved["prim_bmin"] + (a["prim_bmax"] - a["prim_bmin"])
    fitted = ref.refit(tree, moved["prim_bmin"], moved["prim_bmax"])
    ref.check_boxes(fitted, moved, "refit")
    for k in ("bvh_index", "bvh_count_leaf", "bvh_order", "bvh_max_depth"):
        assert np.array_equal(fitted[k], tree[k])
    assert fitted["bvh_bmin"].tobytes() != tree["bvh_bmin"].tobytes()


# ---- the synthetic scenes are what the GPU tests take them for ------------------------------------------------------------

def test_the_chain_is_deep(arrays):
    a = arrays["chain"]
    assert a["n_prims"] == 2081
    depth = ref.build(a["prim_bmin"], a["prim_bmax"])["bvh_max_depth"]
    print("chain: model depth %d" % depth)
    assert depth >= 40


def test_the_outlier_squeezes_the_rest_into_one_cell(arrays):
    a = arrays["outlier"]
    code = ref.morton_codes(a["prim_bmin"], a["prim_bmax"])
    assert a["n_prims"] == 3001 and int((code == 0).sum()) == 3000 and int(code.max()) == (1 << 30) - 1
    print("outlier: model depth %d" % ref.build(a["prim_bmin"], a["prim_bmax"])["bvh_max_depth"])


@pytest.mark.parametrize("name,flat_axes", [("flat_triangles", (2,)), ("line", (1, 2)), ("coincident", (0, 1, 2)), ("duplicates", (0, 1, 2))])
def test_flat_axes_give_zero_bits(name, flat_axes, arrays):
    a = arrays[name]
    q = ref.quantised(a["prim_bmin"], a["prim_bmax"])
    for axis in range(3):
        assert (not q[:, axis].any()) == (axis in flat_axes), "%s, axis %d" % (name, axis)
    code = ref.morton_codes(a["prim_bmin"], a["prim_bmax"])
    mask = sum(sum(1 << (3 * i + 2 - axis) for i in range(10)) for axis in flat_axes)
    assert not (code & np.uint64(mask)).any()


@pytest.mark.parametrize("name", ["lattice", "lattice_scaled"])
def test_the_lattice_meets_the_cell_edges_and_the_clamp(name, arrays):
    a = arrays[name]
    assert a["n_prims"] == 16 * 16 * 8
    q = ref.quantised(a["prim_bmin"], a["prim_bmax"])
    assert int(q.max()) == 1023 and int(q.min()) == 0
    if name == "lattice":  # exact: the cell is the tick, and tick 1024 is clamped into cell 1023
        assert sorted(set(q[:, 0].tolist())) == [0, 1, 2, 3, 64, 255, 256, 511, 512, 513, 767, 1020, 1021, 1022, 1023]
        assert sorted(set(q[:, 2].tolist())) == [0, 1, 511, 512, 1021, 1022, 1023]
        assert int((q[:, 0] == 1023).sum()) == 2 * 16 * 8


def test_the_mixed_scene_has_every_kind(tmp_path):
    import fuzz_scenes
    a = p3d.HostScene(fuzz_scenes.random_scene(21, str(tmp_path / "mixed.p3f"), n_spheres=40, n_tris=60, n_boxes=20, n_planes=2)).arrays()
    assert sorted(set(a["prim_type"].tolist())) == [0, 1, 2, 3]
    planes = a["prim_type"] == 3
    assert (a["prim_bmin"][planes] == -1).all() and (a["prim_bmax"][planes] == 1).all()
    assert np.isfinite(a["prim_bmin"]).all() and np.isfinite(a["prim_bmax"]).all()
    ref.check_boxes(ref.build(a["prim_bmin"], a["prim_bmax"]), a, "mixed")

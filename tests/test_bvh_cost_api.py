"""The SAH cost of a device-built tree and the refit that rebuilds by itself (p3d_scene_bvh_cost, p3d_scene_set_auto_rebuild,
p3d_scene_auto_rebuild, include/p3d.h) without a GPU: the entry points and the 32-byte structure are declared, exported and
wrapped, p3d_update_mode keeps its two values, and p3d.tree_cost - the numpy float64 statement of the cost - gives the values
worked out by hand."""
import ctypes as C
import re

import numpy as np

from api_checks import header_code
import p3d_amd as p3d

SYMBOLS = ["p3d_scene_bvh_cost", "p3d_scene_set_auto_rebuild", "p3d_scene_auto_rebuild"]
LEAF = 0x80000000


def _tree(bmin, bmax, index, count_leaf, order):
    return dict(bvh_bmin=np.array(bmin, np.float32), bvh_bmax=np.array(bmax, np.float32), bvh_index=np.array(index, np.uint32),
                bvh_count_leaf=np.array(count_leaf, np.uint32), bvh_order=np.array(order, np.uint32), bvh_max_depth=2)


def test_header_declares_the_entry_points_and_the_structure():
    code = header_code()
    assert re.search(r"typedef\s+struct\s+p3d_bvh_cost\s*\{\s*double\s+sah\s*;\s*double\s+sah_baseline\s*;\s*uint32_t\s+n_inner\s*,\s*n_leaves\s*;"
                     r"\s*uint32_t\s+refits_since_build\s*;\s*uint32_t\s+last_update_rebuilt\s*;\s*\}\s*p3d_bvh_cost\s*;", code)
    assert re.search(r"\bint\s+p3d_scene_bvh_cost\s*\(\s*p3d_scene\s*\*\s*\w+,\s*p3d_bvh_cost\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_scene_set_auto_rebuild\s*\(\s*p3d_scene\s*\*\s*\w+,\s*float\s+\w+\)", code)
    assert re.search(r"\bint\s+p3d_scene_auto_rebuild\s*\(\s*p3d_scene\s*\*\s*\w+,\s*float\s*\*\s*\w+\)", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)


def test_the_update_modes_are_the_two_there_were():
    assert re.search(r"typedef\s+enum\s+p3d_update_mode\s*\{\s*P3D_UPDATE_REFIT\s*=\s*0\s*,\s*P3D_UPDATE_REBUILD\s*=\s*1\s*\}\s*p3d_update_mode\s*;",
                     header_code())
    assert (p3d.UPDATE_REFIT, p3d.UPDATE_REBUILD) == (0, 1)


def test_library_exports_them_and_python_wraps_them():
    lib = p3d.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS, name
    assert lib.p3d_abi_version() == 4
    for name in ("bvh_cost", "set_auto_rebuild", "auto_rebuild"):
        assert hasattr(p3d.DeviceScene, name), name
    assert callable(p3d.tree_cost)


def test_the_structure_is_32_bytes():
    assert C.sizeof(p3d.BvhCost) == 32
    assert [n for n, _ in p3d.BvhCost._fields_] == ["sah", "sah_baseline", "n_inner", "n_leaves", "refits_since_build", "last_update_rebuilt"]
    assert p3d.BvhCost.n_inner.offset == 16 and p3d.BvhCost.last_update_rebuilt.offset == 28


def test_a_null_scene_is_refused():
    lib = p3d.lib()
    cost, ratio = p3d.BvhCost(), C.c_float(7.0)
    assert lib.p3d_scene_bvh_cost(None, C.byref(cost)) == -1  # P3D_ERR_INVALID
    assert b"null" in lib.p3d_last_error()
    assert lib.p3d_scene_set_auto_rebuild(None, 2.0) == -1
    assert lib.p3d_scene_auto_rebuild(None, C.byref(ratio)) == -1
    assert ratio.value == 7.0


def test_tree_cost_of_a_tree_of_three_nodes():
    """Root 4 x 2 x 1: A = (8 + 2) + 4 = 14.  Left, one object, 1 x 2 x 1: A = (2 + 2) + 1 = 5.  Right, two objects, 2 x 1 x 1:
    A = (2 + 1) + 2 = 5.  sah = (14 + 1 * 5 + 2 * 5) / 14."""
    t = _tree([[0, 0, 0], [0, 0, 0], [2, 0, 0]], [[4, 2, 1], [1, 2, 1], [4, 1, 1]], [1, 0, 1], [0, LEAF | 1, LEAF | 2], [0, 1, 2])
    assert p3d.tree_cost(t) == 29.0 / 14.0


def test_tree_cost_of_a_single_leaf_is_1_and_of_a_flat_root_0():
    assert p3d.tree_cost(_tree([[-1, 0, 2]], [[1, 3, 2.5]], [0], [LEAF | 1], [0])) == 1.0
    # a root that is a line: every product has a factor 0
    assert p3d.tree_cost(_tree([[0, 1, 1]], [[5, 1, 1]], [0], [LEAF | 1], [0])) == 0.0
    assert p3d.tree_cost(_tree([[0, 0, 0], [0, 0, 0], [1, 0, 0]], [[2, 0, 0], [1, 0, 0], [2, 0, 0]], [1, 0, 1], [0, LEAF | 1, LEAF | 1], [0, 1])) == 0.0
    empty = _tree(np.zeros((0, 3)), np.zeros((0, 3)), [], [], [])
    assert p3d.tree_cost(empty) == 0.0


def test_tree_cost_takes_the_differences_in_float64():
    """Corners -2^24 and 1: the extent 2^24 + 1 is no float32, and every sum below is an integer under 2^53"""
    lo, hi = np.float32(16777216.0), np.float32(1.0)
    t = _tree([[-lo, -lo, -lo]], [[hi, hi, hi]], [0], [LEAF | 1], [0])
    assert p3d.tree_cost(t) == 1.0
    two = _tree([[-lo, -lo, -lo], [-lo, -lo, -lo], [0, 0, 0]], [[hi, hi, hi], [0, 0, 0], [hi, hi, hi]], [1, 0, 1], [0, LEAF | 1, LEAF | 1], [0, 1])
    d = 16777217.0
    assert p3d.tree_cost(two) == (3 * d * d + 3 * 16777216.0 ** 2 + 3.0) / (3 * d * d)

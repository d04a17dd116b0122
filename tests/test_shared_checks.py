"""The shared assertions of tests/frame_checks.py on synthetic data, without a GPU: each accepts identical inputs (a NaN with
the same bit pattern on both sides included) and raises AssertionError on the smallest difference it exists to catch.  Many
test modules lean on one definition of each: this is what shows that the definition still checks what it says."""
import copy

import numpy as np
import pytest

from frame_checks import (GRID_KEYS, RENDER_COUNTERS, TREE_KEYS, assert_bit_identical, assert_bits, assert_same_bits, assert_same_frames,
                          assert_same_grid, assert_same_tree, frames_differ, same_bits, same_bits_or_nan)

PIXEL = (3, 5)  # the one pixel the differences below touch
NAN_PIXEL = (6, 1)


def frame(seed=1):
    """(rgb, hit, rgb8) of 8 x 8 pixels: finite colours above zero, one NaN, one exact zero"""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(0.25, 1.0, (8, 8, 3)).astype(np.float32)
    rgb[NAN_PIXEL] = np.float32(np.nan)
    rgb[0, 0, 2] = 0.0
    hit = rng.integers(-1, 5, (8, 8)).astype(np.int32)
    return rgb, hit, (rng.uniform(0, 255, (8, 8, 3))).astype(np.uint8)


def one_ulp(f):
    f[0][PIXEL + (1,)] = np.nextafter(f[0][PIXEL + (1,)], np.float32(2))


def minus_zero(f):
    f[0][0, 0, 2] = np.float32(-0.0)


def one_hit_id(f):
    f[1][PIXEL] += 1


def one_rgb8_byte(f):
    f[2][PIXEL + (0,)] ^= 1


PIXEL_CHANGES = [one_ulp, minus_zero, one_hit_id]


def changed(change, seed=1):
    f = frame(seed)
    change(f)
    return f


def frame_list():
    out = []
    for k, label in enumerate(("whitted literal", "whitted per pixel")):
        rgb, hit, _ = frame(10 + k)
        out.append((label, rgb, hit, {name: 1000 * k + i for i, name in enumerate(RENDER_COUNTERS)}))
    return out


def tree():
    """Five nodes (root, an inner node, three leaves) over four objects"""
    leaf = np.uint32(0x80000000)
    rng = np.random.default_rng(2)
    lo = rng.uniform(-1, 0, (5, 3)).astype(np.float32)
    return {"bvh_bmin": lo, "bvh_bmax": lo + np.float32(1.5), "bvh_index": np.array([1, 3, 0, 1, 2], np.uint32),
            "bvh_count_leaf": np.array([2, 2, leaf | 1, leaf | 1, leaf | 2], np.uint32), "bvh_order": np.array([2, 0, 3, 1], np.uint32),
            "bvh_max_depth": 3}


def grid():
    """2 x 1 x 2 cells with five items"""
    return {"grid_n": np.array([2, 1, 2], np.uint32), "grid_bmin": np.array([-1, -2, -3], np.float32), "grid_bmax": np.array([1, 2, 3], np.float32),
            "grid_cell_start": np.array([0, 2, 2, 3, 5], np.uint32), "grid_cell_items": np.array([0, 1, 1, 2, 0], np.uint32)}


def flip_a_byte(a):
    a.view(np.uint8).reshape(-1)[5] ^= 1


def test_identical_inputs_pass_with_a_nan_on_both_sides():
    a, b = frame(), frame()
    assert np.isnan(a[0][NAN_PIXEL]).all() and a[0] is not b[0]
    assert_same_bits(a, b, "same")
    assert_same_bits(a, b, "same", where=np.ones((8, 8), bool))
    assert_bit_identical(a[:2], b[:2], "same")
    for x, y in zip(a, b):
        assert_bits(x, y, "same")
    assert_same_frames(frame_list(), frame_list(), "same")
    assert not frames_differ(frame_list(), frame_list())
    assert_same_tree(tree(), tree(), "same")
    assert_same_grid(grid(), grid(), "same")
    assert same_bits(a[0], b[0]) and same_bits_or_nan(a[0], b[0]).all()


@pytest.mark.parametrize("change", PIXEL_CHANGES + [one_rgb8_byte], ids=lambda c: c.__name__)
def test_assert_same_bits_catches(change):
    with pytest.raises(AssertionError, match="case"):
        assert_same_bits(changed(change), frame(), "case")
    others = np.ones((8, 8), bool)
    others[PIXEL] = others[0, 0] = False
    assert_same_bits(changed(change), frame(), "case", where=others)  # the mask leaves the changed pixel out ...
    with pytest.raises(AssertionError, match="case"):
        assert_same_bits(changed(change), frame(), "case", where=~others)  # ... or holds nothing else


@pytest.mark.parametrize("change", PIXEL_CHANGES, ids=lambda c: c.__name__)
def test_assert_bit_identical_catches(change):
    with pytest.raises(AssertionError, match="case: (hit IDs differ in 1 pixels|1 pixels differ in some colour bit)"):
        assert_bit_identical(changed(change)[:2], frame()[:2], "case")


@pytest.mark.parametrize("change", PIXEL_CHANGES, ids=lambda c: c.__name__)
def test_assert_bits_catches(change):
    got, want = changed(change), frame()
    k = 1 if change is one_hit_id else 0
    with pytest.raises(AssertionError, match="case: 1 of %d values differ" % got[k].size):
        assert_bits(got[k], want[k], "case")
    assert not same_bits(got[0], want[0]) or change is one_hit_id
    assert same_bits_or_nan(got[0], want[0]).all() == (change is one_hit_id)


def test_assert_bits_catches_a_shape_mismatch_with_equal_bytes():
    rgb, hit, _ = frame()
    with pytest.raises(AssertionError, match="shape"):
        assert_bits(rgb.reshape(64, 3), rgb, "case")
    with pytest.raises(AssertionError, match="shape"):
        assert_bits(hit.reshape(64), hit, "case")
    assert not same_bits(rgb.reshape(64, 3), rgb)


@pytest.mark.parametrize("change", PIXEL_CHANGES, ids=lambda c: c.__name__)
def test_assert_same_frames_catches(change):
    a, b = frame_list(), frame_list()
    for f in (a, b):
        f[1][1][NAN_PIXEL] = 0.5  # (so that the message's max |diff| is a number)
    change((a[1][1], a[1][2]))
    with pytest.raises(AssertionError, match="case, whitted per pixel: (hit IDs differ in 1 pixels|1 pixels differ in some colour bit, max)"):
        assert_same_frames(a, b, "case")
    assert frames_differ(a, b)


def test_assert_same_frames_catches_a_counter_and_a_label():
    a, b = frame_list(), frame_list()
    a[0][3]["tri_tests"] += 1
    with pytest.raises(AssertionError, match="case, whitted literal: counters"):
        assert_same_frames(a, b, "case")
    assert not frames_differ(a, b)  # (the pixels are the same)
    a = frame_list()
    a[1] = ("path trace 4 spp",) + a[1][1:]
    with pytest.raises(AssertionError):
        assert_same_frames(a, b, "case")
    with pytest.raises(AssertionError):
        assert_same_frames(b[:1], b, "case")


@pytest.mark.parametrize("key", TREE_KEYS)
def test_assert_same_tree_catches_one_byte(key):
    t = tree()
    flip_a_byte(t[key])
    with pytest.raises(AssertionError, match="case: %s differs in 1 of" % key):
        assert_same_tree(t, tree(), "case")


def test_assert_same_tree_catches_the_depth_and_a_shape():
    t = tree()
    t["bvh_max_depth"] += 1
    with pytest.raises(AssertionError, match="case: bvh_max_depth 4"):
        assert_same_tree(t, tree(), "case")
    t = tree()
    t["bvh_bmin"] = t["bvh_bmin"].reshape(3, 5)
    assert t["bvh_bmin"].tobytes() == tree()["bvh_bmin"].tobytes()
    with pytest.raises(AssertionError, match="case: bvh_bmin has shape"):
        assert_same_tree(t, tree(), "case")


@pytest.mark.parametrize("key", GRID_KEYS)
def test_assert_same_grid_catches_one_byte(key):
    g = grid()
    flip_a_byte(g[key])
    with pytest.raises(AssertionError, match="case: %s differs in 1 entries" % key):
        assert_same_grid(g, grid(), "case")


def test_assert_same_grid_catches_a_cell_count_a_shape_and_a_type():
    g = grid()
    g["grid_n"][1] += 1
    with pytest.raises(AssertionError, match="case: .* cells"):
        assert_same_grid(g, grid(), "case")
    g = grid()
    g["grid_cell_items"] = g["grid_cell_items"].reshape(5, 1)
    with pytest.raises(AssertionError, match="case: grid_cell_items has shape"):
        assert_same_grid(g, grid(), "case")
    g = grid()
    g["grid_cell_start"] = g["grid_cell_start"].view(np.int32)
    with pytest.raises(AssertionError, match="case: grid_cell_start"):
        assert_same_grid(g, grid(), "case")
    assert_same_grid(copy.deepcopy(grid()), grid(), "case")

"""HostScene.nearest_k (p3d_host_scene_nearest_k: the brute-force statement of the k-nearest query, on the CPU) against the
float64 model through nearest_k_reference.check_k, on the five scenes and seeds of test_nearest_reference.py; against
HostScene.nearest at k = 1; the prefix property; the cases whose answer is exact; and the edge inputs."""
import numpy as np
import pytest

from frame_checks import as_bytes
from device_query_contract import INVALID
import intersect_reference as ref
import nearest_k_reference as nk
import nearest_reference as near
import p3d_amd as p3d

SCENES = ("mixed", "mixed_planes", "planes", "axis_aligned", "tri5k")
SEED = {name: 400 + k for k, name in enumerate(SCENES)}  # test_nearest_reference.py's
KS = nk.KS
FLT_MAX = near.FLT_MAX


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    """name -> (host scene, model objects, points, the model's table, its smallest distances sorted)"""
    paths = dict(ref.scene_paths(tmp_path_factory.mktemp("nearest_k")), tri5k=tri5k_path)
    out = {}
    for name in SCENES:
        objs = ref.load_objects(paths[name])
        pts = near.scene_points(objs, SEED[name])
        tab = near.table(objs, pts)
        out[name] = (p3d.HostScene(paths[name]), objs, pts, tab, nk.sorted_table(tab))
    return out


def limits_of(name, srt, k):
    return nk.draw_k_limits(srt, k, SEED[name] + 50 + k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SCENES)
def test_the_host_form_against_the_model(name, k, worlds):
    hs, objs, pts, tab, srt = worlds[name]
    assert len(pts) == near.N_POINTS and len(objs) == hs.arrays()["n_prims"]
    got = hs.nearest_k(pts, k)
    nk.check_k(objs, pts, k, None, got, "nearest_k, %s, k = %d" % (name, k), tab=tab)
    assert (got[0] == min(k, len(objs))).all()  # fewer than k objects (axis_aligned, planes at k = 16): count = objects, then padding


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SCENES)
def test_limits(name, k, worlds):
    hs, objs, pts, tab, srt = worlds[name]
    limits = limits_of(name, srt, k)
    got = hs.nearest_k(pts, k, max_dist=limits)
    nk.check_k(objs, pts, k, limits, got, "nearest_k with limits, %s, k = %d" % (name, k), tab=tab)
    count = got[0]
    for first, bad in ((0, 0.0), (25, -1.5), (50, np.nan)):  # a zero, a negative and a NaN limit keep nothing
        assert (count[first::75] == 0).all() and (np.isnan(limits[first::75]) if np.isnan(bad) else limits[first::75] == bad).all()
    if len(objs) >= k:  # the draw reaches the three sorts of point in every batch of 63 or more
        for start in range(0, len(pts) - 62, 63):
            c = count[start:start + 63]
            assert (c == 0).any() and (c == k).any() and (k == 1 or ((c > 0) & (c < k)).any()), "%s, k = %d, batch at %d" % (name, k, start)
    everything = hs.nearest_k(pts, k, max_dist=np.full(len(pts), np.inf, np.float32))
    assert all(as_bytes(a) == as_bytes(b) for a, b in zip(everything, hs.nearest_k(pts, k)))


@pytest.mark.parametrize("name", SCENES)
def test_k_1_is_the_nearest_query(name, worlds):
    hs, objs, pts, tab, srt = worlds[name]
    for limits in (None, limits_of(name, srt, 1), near.draw_limits(tab.min(0), SEED[name] + 50)):
        count, obj, dist, closest = hs.nearest_k(pts, 1, max_dist=limits)
        one = hs.nearest(pts, max_dist=limits)
        assert as_bytes(obj[:, 0]) == as_bytes(one[0]) and as_bytes(dist[:, 0]) == as_bytes(one[1]) and as_bytes(closest[:, 0]) == as_bytes(one[2])
        assert (count == (one[0] >= 0)).all()


@pytest.mark.parametrize("name", SCENES)
def test_a_smaller_k_is_a_prefix(name, worlds):
    hs, objs, pts, tab, srt = worlds[name]
    for limits in (None, limits_of(name, srt, 4)):
        big = hs.nearest_k(pts, 16, max_dist=limits)
        for k in (1, 2, 4, 5, 15):
            small = hs.nearest_k(pts, k, max_dist=limits)
            assert (small[0] == np.minimum(big[0], k)).all(), "%s: count at k = %d" % (name, k)
            keep = np.arange(k)[None, :] < small[0][:, None]
            for a, b in zip(small[1:], big[1:]):
                assert as_bytes(a[keep]) == as_bytes(b[:, :k][keep]), "%s: the first rows at k = %d" % (name, k)
            nk.check_rows(pts, k, small, "%s, k = %d" % (name, k))


# the EXACT scene of test_nearest_reference.py (small dyadic numbers: every operation of the rule is exact on them), and behind
# it one triangle three times
EXACT = ref.HEAD + """s 4 0 0 1
p 3
0 0 0
2 0 0
0 2 0
box -1 3 -1 1 7 2
s -8 0 0 1
s -4 0 0 1
p 3
0 0 8
2 0 8
0 2 8
p 3
0 0 8
0 2 8
-2 0 8
p 3
0 0 -16
4 0 -16
0 4 -16
p 3
0 0 -16
4 0 -16
0 4 -16
p 3
0 0 -16
4 0 -16
0 4 -16
"""
SPH, TRI, BOX_, SPH_L, SPH_R, TRI_A, TRI_B, TRIPLE_A, TRIPLE_B, TRIPLE_C = range(10)


def test_exact_cases(tmp_path):
    path = tmp_path / "exact.p3f"
    path.write_text(EXACT)
    hs = p3d.HostScene(str(path))
    assert len(ref.load_objects(str(path))) == 10
    above = np.array([[1, 1, -14]], np.float32)  # over the face of the tripled triangle, 2 away; everything else is farther than 13
    for k, want in ((1, [TRIPLE_A]), (2, [TRIPLE_A, TRIPLE_B]), (3, [TRIPLE_A, TRIPLE_B, TRIPLE_C])):
        count, obj, dist, closest = hs.nearest_k(above, k)
        assert count.tolist() == [k] and obj[0].tolist() == want, "ties across the k boundary go to the lower index"
        assert dist[0].tolist() == [2.0] * k and closest[0].tolist() == [[1, 1, -16]] * k
    count, obj, dist, closest = hs.nearest_k(above, 5, max_dist=np.float32([4.0]))
    assert count.tolist() == [3] and obj[0].tolist() == [TRIPLE_A, TRIPLE_B, TRIPLE_C, -1, -1] and dist[0].tolist() == [2.0] * 3 + [float(FLT_MAX)] * 2
    assert closest[0].tolist() == [[1, 1, -16]] * 3 + [[0, 0, 0]] * 2
    # a limit equal to a distance is strict; the next float above it admits all three
    count, obj, dist, closest = hs.nearest_k(above, 3, max_dist=np.float32([2.0]))
    assert count.tolist() == [0] and obj[0].tolist() == [-1] * 3 and (dist == FLT_MAX).all() and not closest.any()
    count, obj, dist, closest = hs.nearest_k(above, 3, max_dist=np.nextafter(np.float32([2.0]), np.float32(np.inf)))
    assert count.tolist() == [3] and obj[0].tolist() == [TRIPLE_A, TRIPLE_B, TRIPLE_C]
    # between the two spheres: both at 1, in index order, then the box (sqrtf(34) away)
    count, obj, dist, closest = hs.nearest_k(np.array([[-6, 0, 0]], np.float32), 3)
    assert count.tolist() == [3] and obj[0].tolist() == [SPH_L, SPH_R, BOX_] and dist[0, :2].tolist() == [1.0, 1.0] and dist[0, 2] == np.sqrt(np.float32(34))
    assert closest[0].tolist() == [[-7, 0, 0], [-5, 0, 0], [-1, 3, 0]]
    count, obj, dist, closest = hs.nearest_k(np.array([[-6, 0, 0]], np.float32), 3, max_dist=np.float32([1.5]))
    assert count.tolist() == [2] and obj[0].tolist() == [SPH_L, SPH_R, -1]
    # above the edge two triangles share: both at 1, the lower index first; k = 1 keeps the lower
    count, obj, dist, closest = hs.nearest_k(np.array([[0, 1, 9]], np.float32), 2)
    assert obj[0].tolist() == [TRI_A, TRI_B] and dist[0].tolist() == [1.0, 1.0] and closest[0].tolist() == [[0, 1, 8]] * 2
    assert hs.nearest_k(np.array([[0, 1, 9]], np.float32), 1)[1][0].tolist() == [TRI_A]


def test_edge_inputs(tmp_path):
    path = tmp_path / "empty.p3f"
    path.write_text(ref.HEAD)
    hs = p3d.HostScene(str(path))
    count, obj, dist, closest = hs.nearest_k(np.zeros((3, 3), np.float32), 4)  # an empty scene
    assert count.tolist() == [0] * 3 and (obj == -1).all() and obj.shape == (3, 4) and (dist == FLT_MAX).all() and not closest.any()
    count, obj, dist, closest = hs.nearest_k(np.zeros((0, 3), np.float32), 4)  # an empty batch
    assert len(count) == 0 and obj.shape == (0, 4) and dist.shape == (0, 4) and closest.shape == (0, 4, 3)
    with pytest.raises(ValueError):
        hs.nearest_k(np.zeros((3, 3), np.float32), 4, max_dist=np.ones(2, np.float32))
    path = tmp_path / "exact.p3f"
    path.write_text(EXACT)
    hs = p3d.HostScene(str(path))
    for k in (0, 17):
        for n in (0, 3):  # k is checked first: an empty batch does not excuse it
            with pytest.raises(p3d.P3DError) as e:
                hs.nearest_k(np.zeros((n, 3), np.float32), k)
            assert e.value.code == INVALID and "k must be" in str(e.value)
    pts = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [1, 1, -14]], np.float32)  # a NaN coordinate: every d2 is a NaN
    count, obj, dist, closest = hs.nearest_k(pts, 3)
    assert count.tolist() == [0, 0, 0, 3] and (obj[:3] == -1).all() and (dist[:3] == FLT_MAX).all() and not closest[:3].any()
    lib = p3d.lib()
    out = np.full(8, 77, np.int32)
    assert lib.p3d_host_scene_nearest_k(hs._h, 2, 4, pts.ctypes.data, None, None, out.ctypes.data, None, None) == INVALID  # a null count
    assert b"null array" in lib.p3d_last_error() and (out == 77).all()
    # the optional outputs may be left out
    cnt = np.zeros(4, np.int32)
    obj2 = np.zeros((4, 3), np.int32)
    assert lib.p3d_host_scene_nearest_k(hs._h, 4, 3, pts.ctypes.data, None, cnt.ctypes.data, obj2.ctypes.data, None, None) == 0
    assert as_bytes(cnt) == as_bytes(count) and as_bytes(obj2) == as_bytes(obj)

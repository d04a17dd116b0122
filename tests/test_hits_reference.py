"""The hit-list query's helpers (hits_reference.py) without a GPU: brute_hits on a hand-made table, the margin on a closed-form
case, and the CPU oracle's brute force (Object::intercepts on a fresh copy of the ray per object, then brute_hits) held to the
float64 model on the scenes and rays the GPU suite (test_gpu_trace_hits.py) runs through the kernels - the four scene_paths
scenes, the slats that fill a list of sixteen, and the closed cube whose crossings tell inside from outside.  Ill-conditioned
rays (all_hits_margin under intersect_reference.THRESHOLD) are left out, their share capped at 5 %; run with -s for the counts."""
import numpy as np
import pytest

import hits_reference as hr
import intersect_reference as ref
from oracle import binding as ob
import segment_reference as seg

INF = np.float32(np.inf)


def test_brute_hits_on_a_hand_made_table():
    nan = np.nan
    #            ray 0     1     2     3     4    5
    t = np.array([[3.0, 1.0, 2.0, 1.0, nan, 1.0],
                  [1.0, 1.0, 9.0, 1.0, 1.0, 2.0],
                  [2.0, 0.5, 2.0, 1.0, 2.0, 3.0]], np.float32)
    hit = np.array([[1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 1, 1], [1, 1, 1, 0, 1, 1]], bool)
    lim = np.array([np.inf, 1.0, 2.5, np.nan, 5.0, 0.0], np.float32)
    count, total, obj, ts = hr.brute_hits((hit, t), lim, 2)
    assert total.tolist() == [3, 1, 2, 0, 2, 0] and count.tolist() == [2, 1, 2, 0, 2, 0]
    # ray 0: sorted by t; ray 1: the limit is strict; ray 2: equal t to the smaller index, a miss does not count; ray 3: a NaN
    # limit; ray 4: a NaN t is never in; ray 5: a zero limit
    assert obj.tolist() == [[1, 2], [2, -1], [0, 2], [-1, -1], [1, 2], [-1, -1]]
    assert ts.tolist() == [[1.0, 2.0], [0.5, hr.FLT_MAX], [2.0, 2.0], [hr.FLT_MAX] * 2, [1.0, 2.0], [hr.FLT_MAX] * 2]
    # a smaller k is a prefix, total does not depend on k, k = 0 is the count alone, and no limit is an infinite one
    c1, t1, o1, s1 = hr.brute_hits((hit, t), lim, 1)
    assert (o1 == obj[:, :1]).all() and (s1 == ts[:, :1]).all() and (t1 == total).all() and (c1 == np.minimum(total, 1)).all()
    c0, t0, o0, s0 = hr.brute_hits((hit, t), lim, 0)
    assert (t0 == total).all() and not c0.any() and o0.shape == (6, 0) and s0.shape == (6, 0)
    free, unlimited = hr.brute_hits((hit, t), None, 16), hr.brute_hits((hit, t), np.full(6, INF), 16)
    assert all((a == b).all() for a, b in zip(free, unlimited)) and free[1].tolist() == [3, 3, 2, 2, 2, 3]
    assert (free[2][:, 3:] == -1).all() and (free[3][:, 3:] == hr.FLT_MAX).all()


def test_margin_on_a_closed_form_case():
    objs = [dict(kind=ref.SPHERE, c=np.array([0., 0, 5]), r=1.0), dict(kind=ref.BOX, mn=np.array([-1., -1, 1]), mx=np.array([1., 1, 2])),
            dict(kind=ref.TRIANGLE, p0=np.array([4., -1, -1]), p1=np.array([4., 1, -1]), p2=np.array([4., 0, 2]))]
    o = np.zeros((6, 3))
    d = np.array([[0, 0, 1]] * 4 + [[1, 0, 0]] * 2, float)
    t_max = np.array([0.5, 1.0, 3.0, np.nan, 4.5, np.inf])
    m = hr.all_hits_margin(objs, o, d, t_max)
    total, obj, t = hr.model_hits(ref._all(objs, o, d), t_max, 2)
    # along z: the box at t = 1, the sphere at 4 behind it; along x: the triangle at 4
    assert total.tolist() == [0, 0, 1, 0, 1, 1] and obj.tolist() == [[-1, -1], [-1, -1], [1, -1], [-1, -1], [2, -1], [2, -1]]
    assert m[1] == 0 and m[3] == 0  # a limit on the hit it decides; a NaN limit
    # the sphere behind the limit counts although the box in front settles "occluded": its own margin, 1 / 49 from a tangent, is
    # smaller than its distance to the limit, 1 / 4
    assert m[2] == pytest.approx(1 / 49)
    assert m[4] == pytest.approx(0.5 / 4) and m[5] > ref.THRESHOLD
    # every hit counts here, not only the best one as for the segment query: an occluded ray with a second, marginal hit
    occ, m_seg = seg.occluded_within(objs, o[2:3], d[2:3], np.array([4.0 + 1e-6]))
    assert occ[0] and m_seg[0] > ref.THRESHOLD > hr.all_hits_margin(objs, o[2:3], d[2:3], np.array([4.0 + 1e-6]))[0]
    # without limits it is no worse than with them, and None means an infinite limit
    assert (hr.all_hits_margin(objs, o, d, None) == hr.all_hits_margin(objs, o, d, np.full(6, np.inf))).all()


@pytest.mark.parametrize("name", ["mixed", "mixed_planes", "planes", "axis_aligned"])
def test_oracle_brute_force_against_the_model(name, tmp_path):
    path = ref.scene_paths(tmp_path)[name]
    sc, objs = ob.Scene(path), ref.load_objects(path)
    o, d = ref.scene_rays(objs, 8)
    table = ref._all(objs, o, d)
    tests = seg.per_object(sc.object_intercepts, len(objs), o, d)
    seen = 0
    for what, t_max in (("no limit", None), ("limits", seg.draw_limits(objs, o, d, 18, table=table))):
        for k in (1, 5, 16):
            got = hr.brute_hits(tests, t_max, k)
            left = hr.check_against_model(objs, o, d, t_max, k, got, "hit list %s, %s, k = %d, the oracle's brute force" % (name, what, k), table)
            assert left <= ref.MAX_LEFT_OUT * len(o)
        total = hr.brute_hits(tests, t_max, 0)[1]
        assert (total == 0).any() and (total >= 2).any(), "%s, %s: no ray without a hit, or none with a hit behind the first" % (name, what)
        seen = max(seen, int(total.max()))
    assert 2 <= seen <= hr.K_MAX  # these scenes never fill a long list: the slats do


def test_the_slats_fill_a_list_and_leave_nothing_out(tmp_path):
    path = hr.write_slats(tmp_path / "slats.p3f")
    sc, objs = ob.Scene(path), ref.load_objects(path)
    assert len(objs) == hr.N_SLATS
    o, d = hr.slat_rays(21, 515)
    table = ref._all(objs, o, d)
    assert table[0].all()  # every ray crosses every slat
    tests = seg.per_object(sc.object_intercepts, len(objs), o, d)
    limits = hr.slat_limits(table, 22)
    assert np.isinf(limits).any() and np.isfinite(limits).any()
    for what, t_max in (("no limit", None), ("limits", limits)):
        margin = hr.all_hits_margin(objs, o, d, t_max, table)
        assert (margin >= ref.THRESHOLD).all(), "slats, %s: %d rays are ill-conditioned" % (what, int((margin < ref.THRESHOLD).sum()))
        for k in (1, 4, 16):
            got = hr.brute_hits(tests, t_max, k)
            assert hr.check_against_model(objs, o, d, t_max, k, got, "hit list slats, %s, k = %d" % (what, k), table) == 0
    count, total, obj, t = hr.brute_hits(tests, None, 16)
    assert (total == hr.N_SLATS).all() and (count == 16).all() and (obj == np.arange(16)[None, :]).all() and (np.diff(t, axis=1) > 0).all()
    total = hr.brute_hits(tests, limits, 0)[1]
    assert total.min() < 16 < total.max()  # lists that the limit leaves short, and full ones


def test_the_parity_of_a_closed_mesh(tmp_path):
    path = hr.write_cube(tmp_path / "cube.p3f")
    sc, objs = ob.Scene(path), ref.load_objects(path)
    assert len(objs) == 12
    o, d, inside = hr.cube_rays(23, 515)
    table = ref._all(objs, o, d)
    ok, left = ref.well_conditioned(hr.all_hits_margin(objs, o, d, None, table), "the cube's rays")
    m_total = hr.model_hits(table, None, 0)[0]
    assert (m_total[ok & inside] == 1).all() and np.isin(m_total[ok & ~inside], (0, 2)).all() and (m_total[ok & ~inside] == 2).any()
    total = hr.brute_hits(seg.per_object(sc.object_intercepts, len(objs), o, d), None, 0)[1]
    assert ((total[ok] & 1) == inside[ok]).all() and (total[ok] == m_total[ok]).all()
    assert inside[ok].sum() > 200 and (~inside)[ok].sum() > 200

"""host_overlap_box (p3d_host_scene_overlap_box: the brute-force statement of the overlap query, on the CPU) against the float64
model of overlap_reference.py, which clips where the rule separates: on the seeded scenes of sweep_reference.scene_paths and one
that holds boxes, 500 boxes each, with and without `solid`; the hand-built exact table, where every bit counts; and the exact
properties of the answer, compared in bytes.  No GPU is needed."""
import numpy as np
import pytest

from frame_checks import as_bytes
import filter_reference as fr
import intersect_reference as ref
import overlap_reference as ov
import p3d_amd as p3d

K_MAX = 16


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """name -> (host scene, the model's objects, lo, hi)"""
    out = {}
    for at, (name, path) in enumerate(sorted(ov.scene_paths(tmp_path_factory.mktemp("overlap")).items())):
        objects = ref.load_objects(path)
        assert 0 < len(objects) <= 300
        out[name] = (p3d.HostScene(path), objects) + ov.scene_boxes(objects, 940 + at)
    return out


@pytest.fixture(scope="module")
def tables(scenes):
    """(scene, solid) -> the model's table at the test's delta, computed once"""
    cache = {}

    def get(name, solid):
        if (name, solid) not in cache:
            _, objects, lo, hi = scenes[name]
            cache[name, solid] = ov.table(objects, lo, hi, solid)
        return cache[name, solid]
    return get


def _overlapping(hs, lo, hi, solid):
    """(objects, boxes) bool from the host form: the lists of a scene of at most 16 objects are complete; a larger scene is asked
    once per block of objects, the others skipped by range"""
    n_objs = int(hs.arrays()["n_prims"])
    got = np.zeros((n_objs, len(lo)), bool)
    for first in range(0, n_objs, K_MAX):
        # everything but [first, first + 16) is named: the range covers what lies in front, the rest is asked block by block
        total, obj = p3d.host_overlap_box(hs, lo, hi, K_MAX, solid=solid, skip_range=np.tile(np.array([[0, first]], np.int32), (len(lo), 1)))
        for i, row in enumerate(obj):
            listed = row[(row >= first) & (row < first + K_MAX)]
            got[listed, i] = True
    return got


@pytest.mark.parametrize("solid", (False, True))
def test_the_host_form_is_the_model(solid, scenes, tables):
    for name, (hs, objects, lo, hi) in scenes.items():
        want, ok, near_by = tables(name, solid)
        got = _overlapping(hs, lo, hi, solid)
        total, _ = p3d.host_overlap_box(hs, lo, hi, 0, solid=solid)
        assert (got.sum(0) == total).all(), name + ": total is not the number of objects listed block by block"
        left, of = int((~ok & near_by).sum()), int(near_by.sum())
        print("%s, solid %d: %d pairs overlap by comparison, %d of them (%.2f %%) and %d others left out; %d overlaps, %d boxes find something"
              % (name, solid, of, left, 100.0 * left / max(of, 1), int((~ok & ~near_by).sum()), int(want.sum()), int(want.any(0).sum())))
        assert left <= ov.MAX_LEFT_OUT * of, "%s: %d of %d pairs are ill-conditioned, over the %g cap" % (name, left, of, ov.MAX_LEFT_OUT)
        wrong = ok & (got != want)
        assert not wrong.any(), "%s, solid %d: %d pairs differ from the model's, first (object, box) %r" % (
            name, solid, int(wrong.sum()), tuple(int(x[0]) for x in np.nonzero(wrong)))
        finds = want.any(0)
        assert 0.3 * len(lo) < finds.sum() < 0.7 * len(lo), name + ": roughly half the boxes are to find something"
        dead = ~(lo <= hi).all(1)
        assert dead.sum() >= len(lo) // 25 and not total[dead].any(), name + ": an inverted box or one with a NaN finds nothing"


def test_the_measured_rung(scenes):
    """Prints, per rung of delta, how many well-conditioned pairs disagree: MEASURED_DELTA is the smallest rung with none"""
    bad = {rung: 0 for rung in ov.RUNGS if rung <= ov.MEASURED_DELTA}  # (the rungs above it were looked at when it was measured)
    for solid in (False, True):
        for name, (hs, objects, lo, hi) in scenes.items():
            got = _overlapping(hs, lo, hi, solid)
            for rung in bad:
                want, ok, _ = ov.table(objects, lo, hi, solid, delta=rung)
                bad[rung] += int((ok & (got != want)).sum())
    print("disagreements on well-conditioned pairs, per rung of delta: %r" % bad)
    assert min(rung for rung in bad if bad[rung] == 0) == ov.MEASURED_DELTA


def test_the_exact_table(tmp_path):
    """Touching cases in small dyadic coordinates: overlap, with no tolerance; and the model agrees"""
    path, planes = tmp_path / "exact.p3f", tmp_path / "exact_planes.p3f"
    path.write_text(ref.HEAD + ov.EXACT_SCENE)
    planes.write_text(ref.HEAD + ov.EXACT_PLANES)
    cases = [(path,) + c for c in ov.EXACT] + [(planes,) + c[:4] + (solid, c[4]) for c in ov.EXACT_PLANE_CASES for solid in (False, True)]
    for file, what, j, lo, hi, solid, want in cases:
        hs, objects = p3d.HostScene(str(file)), ref.load_objects(str(file))
        lo, hi = np.array([lo], np.float32), np.array([hi], np.float32)
        total, obj = p3d.host_overlap_box(hs, lo, hi, 4, solid=solid)
        assert ov.overlaps(objects[j], lo[0].astype(np.float64), hi[0].astype(np.float64), solid) == want, what + ": the model"
        assert (j in obj[0]) == want, "%s: the rule says %r" % (what, obj[0])
        if len(objects) > 2:  # (two planes that are not parallel meet every box large enough; the others lie far apart)
            assert total[0] == int(want) and list(obj[0]) == ([j] if want else [-1]) + [-1] * 3, what


def test_the_exact_properties(scenes):
    """In bytes: total does not depend on k; a smaller k is a prefix of a larger one's; the rows behind total are -1; solid only
    ever adds objects; a filtered query is the query over the thinned scene, indices mapped back"""
    for name, (hs, objects, lo, hi) in scenes.items():
        n_objs = len(objects)
        for solid in (False, True):
            total16, wide = p3d.host_overlap_box(hs, lo, hi, K_MAX, solid=solid)
            total0, none = p3d.host_overlap_box(hs, lo, hi, 0, solid=solid)
            assert none.shape == (len(lo), 0) and as_bytes(total0) == as_bytes(total16), name + ": total at k = 0 and at k = 16"
            assert ((wide >= 0).sum(1) == np.minimum(total16, K_MAX)).all() and (np.diff(np.where(wide < 0, n_objs, wide), axis=1) >= 0).all()
            assert (np.diff(wide, axis=1)[(wide[:, 1:] >= 0)] > 0).all(), name + ": ascending"
            for k in (1, 4, 7):
                total, obj = p3d.host_overlap_box(hs, lo, hi, k, solid=solid)
                assert as_bytes(total) == as_bytes(total16) and as_bytes(obj) == as_bytes(np.ascontiguousarray(wide[:, :k])), "%s, k = %d" % (name, k)
        shell, solid = _overlapping(hs, lo, hi, False), _overlapping(hs, lo, hi, True)
        assert not (shell & ~solid).any(), name + ": solid took an object away"
        if name in ("spheres", "boxes"):  # (the few small spheres of the mixed scenes need not hold a box)
            assert (solid & ~shell).any(), name + ": no box lies inside a sphere or a box"
        # filters: the unfiltered table with the named objects taken out, then counted and listed again
        skip, skip_range = fr.draw(len(lo), n_objs, 8, True, 950, answers=p3d.host_overlap_box(hs, lo, hi, 8)[1])
        named = fr.skipped(n_objs, len(lo), skip, skip_range)
        for s, r in ((skip, skip_range), (skip[:, :1], None), (None, skip_range)):
            thinned = shell & ~fr.skipped(n_objs, len(lo), s, r)
            total, obj = p3d.host_overlap_box(hs, lo, hi, K_MAX, skip=s, skip_range=r)
            assert (total == thinned.sum(0)).all(), name + ": a filtered total"
            for i in range(len(lo)):
                want = np.nonzero(thinned[:, i])[0][:K_MAX]
                assert list(obj[i, :len(want)]) == list(want) and (obj[i, len(want):] == -1).all(), "%s: the filtered list of box %d" % (name, i)
        assert (named & shell).any(), name + ": the filters named nothing that was found"

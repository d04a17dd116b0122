"""The filtered ray queries (include/p3d_filter.h: p3d_trace_any_filtered_device, p3d_trace_hits_filtered_device,
p3d_occlusion_filtered_device) without a GPU: the entry points are declared, exported with the recorded prototypes and wrapped
as functions; what the library refuses before it needs a device; what the wrappers refuse before the library is called; and the
yardstick of the GPU suite (ray_filter_reference.py) on the CPU: the masked tables name no skipped object, the thinned scene
says the same as the mask, and the filters the suite draws leave the float64 model's margins within the unfiltered tests' cap."""
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
from device_query_contract import INVALID
import filter_reference as fr
import hits_reference as hr
import intersect_reference as ref
import p3d_amd as p3d
import ray_filter_reference as rf
import segment_reference as seg

NAMES = ("p3d_trace_any_filtered_device", "p3d_trace_hits_filtered_device", "p3d_occlusion_filtered_device")


def test_the_header_declares_them():
    code, main = header_code("p3d_filter.h"), header_code()
    assert re.search(r'#include\s+"p3d_filter.h"', main) and re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)
    cf, f, i32, u32 = r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*float\s*\*\s*\w+\s*,", r"\s*int32_t\s*\*\s*\w+\s*,", r"\s*uint32_t\s+\w+\s*,"
    filt = r"\s*const\s+int32_t\s*\*\s*\w+\s*," + u32 + r"\s*const\s+int32_t\s*\*\s*\w+\s*,"
    head, stream = r"\s*\(\s*p3d_scene\s*\*\s*\w+,", r"\s*void\s*\*\s*\w+\)"
    assert re.search(r"\bint\s+p3d_trace_any_filtered_device" + head + u32 * 2 + cf * 3 + filt + r"\s*uint8_t\s*\*\s*\w+\s*," + stream, code)
    assert re.search(r"\bint\s+p3d_trace_hits_filtered_device" + head + u32 * 3 + cf * 3 + filt + i32 * 3 + f * 3 + stream, code)
    assert re.search(r"\bint\s+p3d_occlusion_filtered_device" + head + u32 * 2 + cf * 3 + r"\s*const\s+p3d_occlusion_params\s*\*\s*\w+\s*," + filt +
                     r"\s*uint32_t\s*\*\s*\w+\s*," + f + stream, code)


def test_the_library_exports_them_and_python_wraps_them_as_functions():
    lib = p3d.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES and name not in p3d.EXPORTS, name
    VP, U32 = p3d.PROTOTYPES["p3d_trace_any_device"][1][0], p3d.PROTOTYPES["p3d_trace_any_device"][1][1]
    filt = [VP, U32, VP]
    # the unfiltered prototype with (d_skip, n_skip, d_skip_range) in front of its outputs
    for name, outputs in (("p3d_trace_any_filtered_device", 1), ("p3d_trace_hits_filtered_device", 6), ("p3d_occlusion_filtered_device", 2)):
        plain = p3d.PROTOTYPES[name.replace("_filtered", "")][1]
        cut = len(plain) - outputs - 1  # (the stream is last)
        assert p3d.PROTOTYPES[name][1] == plain[:cut] + filt + plain[cut:], name
        assert p3d.PROTOTYPES[name][0] == p3d.PROTOTYPES[name.replace("_filtered", "")][0]
    assert [len(p3d.PROTOTYPES[name][1]) for name in NAMES] == [11, 17, 13]
    for fn in ("trace_any_filtered_device", "trace_hits_filtered_device", "occlusion_filtered_device"):
        assert callable(getattr(p3d, fn)), fn
        assert not hasattr(p3d.DeviceScene, fn) and not hasattr(p3d.HostScene, fn), fn
    # what needs no device: the null scene, under each entry point's own name
    assert lib.p3d_trace_any_filtered_device(None, p3d.ACCEL_BVH, 4, None, None, None, None, 0, None, None, None) == INVALID
    assert b"p3d_trace_any_filtered_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_trace_hits_filtered_device(None, p3d.ACCEL_BVH, 4, 2, None, None, None, None, 0, None, *([None] * 7)) == INVALID
    assert b"p3d_trace_hits_filtered_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_occlusion_filtered_device(None, p3d.ACCEL_BVH, 4, None, None, None, None, None, 0, None, None, None, None) == INVALID
    assert b"p3d_occlusion_filtered_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def test_the_wrappers_refuse_before_the_library_is_called():
    import torch
    raw = (0x1000, 6)
    dev = scene_without_a_library()
    any_, hits, occ = p3d.trace_any_filtered_device, p3d.trace_hits_filtered_device, p3d.occlusion_filtered_device
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    B = p3d.ACCEL_BVH
    cases = []
    for who, rows_of, call in (("trace_any_filtered_device", "rays", lambda **kw: any_(dev, B, raw, raw, t_max=raw, **kw)),
                               ("trace_hits_filtered_device", "rays", lambda **kw: hits(dev, B, raw, raw, 2, **kw)),
                               ("occlusion_filtered_device", "points", lambda **kw: occ(dev, B, raw, raw, 4, **kw))):
        cases += [
            (who + ": a flat list", "skip: shape", lambda call=call: call(skip=i32(6))),
            (who + ": a 3-D list", "skip: shape", lambda call=call: call(skip=i32(6, 2, 2))),
            (who + ": a width that is not the tensor's", "n_skip says 2", lambda call=call: call(skip=i32(6, 3), n_skip=2)),
            (who + ": a raw list without its width", "needs n_skip", lambda call=call: call(skip=raw)),
            (who + ": a list of other rows", "6 %s, 5 skip rows" % rows_of, lambda call=call: call(skip=(0x2000, 5), n_skip=3)),
            (who + ": ranges of other rows", "6 %s, 5 skip ranges" % rows_of, lambda call=call: call(skip_range=(0x2000, 5))),
            (who + ": a CPU list", "skip: the tensor is in host memory", lambda call=call: call(skip=i32(6, 3))),
            (who + ": a float list", "skip: dtype", lambda call=call: call(skip=i32(6, 3).float())),
            (who + ": an (n, 3) range", "skip_range: shape", lambda call=call: call(skip_range=i32(6, 3))),
        ]
    cases += [
        ("the hits: k = 17", "k must be 0 .. 16", lambda: hits(dev, B, raw, raw, 17)),
        ("the hits: k = 0 without total", "want must hold 'total'", lambda: hits(dev, B, raw, raw, 0)),
        ("the hits: an unknown output", "unknown output", lambda: hits(dev, B, raw, raw, 2, want=("colour",))),
        ("occlusion: no samples", "samples must be at least 1", lambda: occ(dev, B, raw, raw, 0)),
        ("occlusion: an unknown output", "unknown output", lambda: occ(dev, B, raw, raw, 4, want=("colour",))),
        ("the any-hit: limits of other rows", "6 origins, 6 directions, 5 limits", lambda: any_(dev, B, raw, raw, t_max=(0x3000, 5))),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == INVALID and word in str(e.value), "%s: %s" % (what, e.value)


# ---- the yardstick, held on the CPU -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ray_filter_api")
    return {name: rf.Case(path, rf.SEED[name]) for name, path in ref.scene_paths(tmp).items() if name in rf.SEED}


@pytest.mark.parametrize("name", list(rf.SEED))
def test_the_masked_tables_are_the_thinned_scene(name, cases):
    """Two statements of "the scene without the named objects" agree on the float64 model: the per-object table with the named
    entries set to "no hit", and the table of a scene from which the objects of a shared range are taken out, indices mapped back"""
    c = cases[name]
    n, n_objs = c.n, len(c.objs)
    for first, count in rf.shared_ranges(n_objs):
        keep = rf.kept(n_objs, first, count)
        thin = ref._all([c.objs[j] for j in keep], c.o, c.d)
        masked = rf.mask_table(c.table, None, np.tile(np.int32([first, count]), (n, 1)))
        t_total, t_obj, t_t = hr.model_hits(thin, None, 4)
        m_total, m_obj, m_t = hr.model_hits(masked, None, 4)
        assert (t_total == m_total).all() and (rf.mapped_back(t_obj, keep) == m_obj).all() and np.array_equal(t_t, m_t, equal_nan=True), (name, first, count)
        assert not ((m_obj >= first) & (m_obj < first + count)).any()
        lim = seg.draw_limits(c.objs, c.o, c.d, 31, table=c.table)
        assert (seg.occluded_within([c.objs[j] for j in keep], c.o, c.d, lim, table=thin)[0] == rf.model_occluded(c.objs, c.o, c.d, lim, masked)[0]).all()


@pytest.mark.parametrize("name", list(rf.SEED))
def test_the_drawn_filters_change_answers_and_stay_within_the_cap(name, cases):
    """Three rows in four skip what the ray would hit first: the filters change what is found; and with the float64 model alone,
    the rays the thinned tables' margins leave out stay within the cap of the unfiltered tests of these scenes
    (intersect_reference.well_conditioned: MAX_LEFT_OUT of a set)"""
    c = cases[name]
    n, n_objs = c.n, len(c.objs)
    first = hr.model_hits(c.table, None, fr.SKIP_MAX)[1]
    changed = 0
    for n_skip in fr.N_SKIPS:
        for ranged in (False, True):
            skip, skip_range = rf.draw(c, n_skip, ranged)
            named = fr.skipped(n_objs, n, skip, skip_range)
            masked = rf.mask_table(c.table, skip, skip_range)
            assert not masked[0][named].any() and (masked[0][~named] == c.table[0][~named]).all()
            for limits in (None, c.limits):
                what = "%s, n_skip = %d%s%s" % (name, n_skip, ", a range" if ranged else "", ", limits" if limits is not None else "")
                ok, left = ref.well_conditioned(rf.hits_margin(c.objs, c.o, c.d, limits, masked), what)  # (asserts the cap)
                ok, left = ref.well_conditioned(rf.model_occluded(c.objs, c.o, c.d, np.full(n, np.inf, np.float32) if limits is None else limits, masked)[1], what)
                got = hr.model_hits(masked, limits, 1)[1][:, 0]
                assert not named[got[got >= 0], np.nonzero(got >= 0)[0]].any(), what
                if n_skip or ranged:
                    changed += int((got != hr.model_hits(c.table, limits, 1)[1][:, 0]).sum())
    assert changed > n, "%s: the filters changed hardly an answer" % name
    assert (first[:, 0] >= 0).any()

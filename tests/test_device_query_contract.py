"""device_query_contract.py without a GPU: its comparers are held to the smallest difference each exists to catch, and every
query description to the prototype of its entry point - the argument count of p3d.PROTOTYPES, the parameter names of the
header, the outputs table in C order - so that a description cannot silently skip a buffer."""
import glob
import os
import re

import numpy as np
import pytest

from api_checks import header_code
from conftest import ROOT
import device_query_contract as dq
import p3d_amd as p3d


def answer():
    """Three rows of a nearest-like answer: found, not found, found"""
    return {"object": np.array([4, -1, 0], np.int32), "dist": np.array([0.5, dq.FLT_MAX, 0.0], np.float32),
            "closest": np.array([[1, 2, 3], [0, 0, 0], [0, 0, 0.25]], np.float32)}


def one_mantissa_bit(a):
    a["dist"].view(np.uint32)[0] ^= 1


def minus_zero(a):
    a["closest"][2, 0] = np.float32(-0.0)


def another_nan(a, b):
    a["dist"].view(np.uint32)[0], b["dist"].view(np.uint32)[0] = 0x7fc00000, 0x7fc00001


def test_assert_same_bits():
    dq.assert_same_bits(answer(), answer(), "equal bytes")
    dq.assert_same_bits(answer()["dist"], answer()["dist"], "equal bytes, arrays")
    nan_a, nan_b = answer(), answer()
    nan_a["dist"][0] = nan_b["dist"][0] = np.float32(np.nan)
    dq.assert_same_bits(nan_a, nan_b, "the same NaN on both sides")
    for change in (one_mantissa_bit, minus_zero):
        b = answer()
        change(b)
        with pytest.raises(AssertionError):
            dq.assert_same_bits(answer(), b, change.__name__)
    a, b = answer(), answer()
    another_nan(a, b)
    assert np.isnan(a["dist"][0]) and np.isnan(b["dist"][0])
    with pytest.raises(AssertionError):
        dq.assert_same_bits(a, b, "two NaNs with different payloads")
    with pytest.raises(AssertionError):
        dq.assert_same_bits(answer(), dict(reversed(list(answer().items()))), "the keys in another order")
    with pytest.raises(AssertionError):
        dq.assert_same_bits(answer(), dict(answer(), object=answer()["object"].astype(np.int64)), "another dtype")
    with pytest.raises(AssertionError):
        dq.assert_same_bits(np.zeros((2, 3), np.float32), np.zeros((3, 2), np.float32), "another shape")


def test_assert_no_answer_values():
    table = p3d._NEAREST_OUTPUTS
    dq.assert_no_answer_values(answer(), table, "exact")
    for name, at, value in (("closest", (1, 2), 1e-30), ("closest", (1, 0), -0.0), ("dist", (1,), np.inf), ("dist", (1,), 0.0), ("object", (1,), -2)):
        a = answer()
        a[name][at] = value
        with pytest.raises(AssertionError):
            dq.assert_no_answer_values(a, table, "%s = %r" % (name, value))
    # with a count: the rows from count on, and only those
    k = {"count": np.array([1, 0], np.int32), "object": np.array([[3, -1], [-1, -1]], np.int32), "t": np.array([[2.0, dq.FLT_MAX]] + [[dq.FLT_MAX] * 2], np.float32),
         "normal": np.zeros((2, 2, 3), np.float32)}
    table = p3d._trace_hits_outputs(2)
    dq.assert_no_answer_values(k, table, "exact")
    for name, at, value in (("t", (0, 1), 3.0), ("normal", (1, 0, 1), 1.0), ("count", (0,), 2), ("object", (0, 1), 5)):
        a = {key: v.copy() for key, v in k.items()}
        a[name][at] = value
        with pytest.raises(AssertionError):
            dq.assert_no_answer_values(a, table, "%s = %r" % (name, value))


def parameters(entry):
    """The parameter names of `entry` as the headers under include/ declare it"""
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % entry, header_code(os.path.basename(path)))
        if found:
            return [re.search(r"(\w+)\s*$", p).group(1) for p in found.group(1).split(",")]
    raise AssertionError("no header declares " + entry)


@pytest.mark.parametrize("query", dq.every_query(), ids=lambda q: q.name)
def test_a_description_names_the_buffers_of_its_entry_point(query):
    names = parameters(query.entry)
    assert len(p3d.PROTOTYPES[query.entry][1]) == len(names) == 3 + len(query.layout) + 1
    assert names[-1] == "hip_stream"
    declared = names[3:-1]
    assert [a if isinstance(a, str) else None for a in query.layout] == [d if d.startswith("d_") else None for d in declared]
    inputs, outputs = [i.name for i in query.inputs], ["d_" + name for name in query.order]
    assert [b for b in query.buffers() if b in inputs] == inputs and [b for b in query.buffers() if b in outputs] == outputs
    assert sorted(query.buffers()) == sorted(inputs + outputs)
    assert set(query.order) == set(query.table) and set(query.required) <= set(query.table)
    assert query.limit is None or query.limit in inputs
    assert all(p3d.PROTOTYPES[query.entry][1][3 + j] is p3d.PROTOTYPES["p3d_scene_status"][1][0] for j, a in enumerate(query.layout) if isinstance(a, str))

"""What enqueue_query (csrc/capi_query.hpp) and _device_query (device_queries.py) promise EVERY query over device tensors,
stated once: a description of each query (Query), one World of scenes by tree, and the scenarios all of them go through -
stream order behind a refit and a pose, the refusals of buffers and accels that enqueue nothing, ragged and empty batches,
and outputs of the caller's.  Every comparison here has tolerance 0.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

from device_geometry_helpers import deformed_mesh
from frame_checks import as_bytes, gpu
from live_scene_checks import plan
import p3d_amd as p3d

INVALID, UNSUPPORTED, CAPACITY = -1, -3, -4  # P3D_ERR_INVALID, P3D_ERR_UNSUPPORTED, P3D_ERR_CAPACITY
FLT_MAX = np.finfo(np.float32).max
BATCHES = [1, 63, 64, 65, 129, 4099]  # kBlock is 64: a lone lane, a full wave, one lane over, a ragged last block of many
BIG = 0x00ffff00  # rows no buffer of a test holds: 200 MB of float32 (n, 3)
TREES = {"host": True, "device": "device", "none": False}  # the tree of a World's device scene -> DeviceScene's bvh=
NONE, BVH = p3d.ACCEL_NONE, p3d.ACCEL_BVH


# ---- bits -------------------------------------------------------------------------------------------------------------------------

def assert_same_bits(a, b, what):
    """Two answers ({name: array}, or two arrays): the same names in the same order, and per name the same dtype, shape and bytes"""
    if not isinstance(a, dict):
        a, b = {"values": a}, {"values": b}
    assert list(a) == list(b), "%s: outputs %r against %r" % (what, list(a), list(b))
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape, "%s: %s is %s %r against %s %r" % (what, name, x.dtype, x.shape, y.dtype, y.shape)
        if as_bytes(x) != as_bytes(y):
            x, y = (np.ascontiguousarray(v).reshape(len(v), -1).view(np.uint8) for v in (x, y))
            rows = np.nonzero((x != y).any(1))[0]
            raise AssertionError("%s: %s differs in %d of %d rows, first at row %d" % (what, name, len(rows), len(x), rows[0]))


def only(got, names):
    """The outputs `names` of an answer, in their order"""
    return {name: got[name] for name in names}


def rows_of(answer, n):
    return {name: v[:n] for name, v in answer.items()}


def assert_no_answer_values(got, table, what):
    """Where nothing was found - object (or hit_id) is -1; with a count: the rows from count on, and only those - the outputs
    of `table` hold exactly FLT_MAX (one number per answer) and +0.0 zeros (vectors)"""
    ids = got["object"] if "object" in got else got["hit_id"]
    assert ids.dtype == np.int32, what
    none = ids < 0
    assert (ids[none] == -1).all(), what + ": an id below -1"
    if "count" in got:
        behind = np.arange(ids.shape[1])[None, :] >= got["count"][:, None]
        assert (none == behind).all(), what + ": the rows behind count"
    for name in table:
        if name in got and got[name].dtype == np.float32:
            v = got[name]
            if v.shape == ids.shape:
                assert (v[none] == FLT_MAX).all(), "%s: %s where nothing was found" % (what, name)
            else:
                assert v.shape == ids.shape + (3,), "%s: %s has shape %r" % (what, name, v.shape)
                assert as_bytes(v[none]) == as_bytes(np.zeros((int(none.sum()), 3), np.float32)), "%s: %s where nothing was found" % (what, name)


def assert_answers(got, want, table, what):
    """The outputs the host form has (`want`, at least as many rows) bit for bit, and the no-answer values exact"""
    assert_same_bits(only(got, want), rows_of(want, len(next(iter(got.values())))), what)
    assert_no_answer_values(got, table, what)


# ---- a query ----------------------------------------------------------------------------------------------------------------------

# One input buffer: its C name (the error messages use it), floats per row (None: one), whether the entry point needs it, and
# its dtype.  guarded: the library checks it in front of the outputs, so a count of BIG over the call's own outputs stops a
# refusal that went missing before any launch; an input checked behind them stays with its module's own refusals
Input = namedtuple("Input", "name cols required dtype guarded", defaults=("float32", True))


class Query:
    """One device query, as far as the shared scenarios need it:
    name: the wrapper's, and "p3d_" + name the C entry point.  layout: the C arguments between (scene, accel, n) and
    hip_stream - a str is the buffer of that C name, anything else is passed as it is (k, max_depth, flags, params).
    inputs: Input rows in C order; limit: the C name of the optional per-row limit.  table: the wrapper's outputs table
    (name -> (dtype, columns)), in the order it returns them; order: the outputs in C order; required: those always there.
    call(dev, accel, inputs, want, stream, out): the wrapper, `inputs` a dict by C name (tensors or raw pairs).
    host_form(hs, world, n, limited): the exact CPU twin's answers by output name, None where there is none.
    witness: the output that shows that an update moved something.  refuses_planes: P3D_ACCEL_BVH over a plane is refused.
    on_stream: the accels asked behind an update; assert_tree(got, brute, hs, world, n, limited, what): how the tree's answers
    are held to a fresh scene's brute force where that is not "every bit".  assert_mixed(got, n) -> bool: found and not found in one batch."""

    def __init__(self, name, layout, inputs, table, order, required, call, limit=None, host_form=None, witness=None, refuses_planes=False,
                 on_stream=(BVH,), assert_tree=None, assert_mixed=None, inputs_of=None):
        self.name, self.entry, self.layout, self.inputs, self.table, self.order, self.required = name, "p3d_" + name, layout, inputs, table, order, required
        self.call, self.limit, self.host_form, self.witness, self.refuses_planes = call, limit, host_form, witness, refuses_planes
        self.on_stream, self.assert_tree, self.assert_mixed = on_stream, assert_tree, assert_mixed
        self.optional = tuple(name for name in table if name not in required)
        if inputs_of is not None:
            self.inputs_of = inputs_of

    def inputs_of(self, world, n, limited=False):
        """The first n rows of the world's device tensors by C name: the required ones, and the limit if `limited`"""
        return {i.name: world.dev[i.name][:n] for i in self.inputs if i.required or (limited and i.name == self.limit)}

    def ask(self, dev, accel, inputs, want=None, stream=0, out=None):
        res = self.call(dev, accel, inputs, self.optional if want is None else want, stream, out)
        return {name: v.cpu().numpy() for name, v in res.items()}

    def raw(self, dev, accel, n, **buffers):
        """The C entry point itself: buffers by C name (a tensor, an address, or left out: NULL), no stream"""
        address = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else x
        args = [C.c_void_p(address(buffers.get(a))) if isinstance(a, str) else a for a in self.layout]
        assert set(buffers) <= set(self.buffers()), set(buffers) - set(self.buffers())
        return getattr(p3d.lib(), self.entry)(dev._h, accel, n, *args, None)

    def buffers(self):
        return [a for a in self.layout if isinstance(a, str)]

    def shape(self, name, n):
        cols = self.table[name][1]
        return (n,) + (() if cols is None else tuple(cols) if isinstance(cols, tuple) else (cols,))

    def outputs(self, n, fill=None):
        """A tensor per output of the table, n rows: empty, or int `fill[0]` and float `fill[1]`"""
        out = {}
        for name, (dtype, _) in self.table.items():
            dt = getattr(torch, dtype)
            out[name] = torch.empty(self.shape(name, n), dtype=dt, device="cuda") if fill is None else \
                torch.full(self.shape(name, n), fill[dt.is_floating_point], dtype=dt, device="cuda")
        return out

    def row_bytes(self, name):
        return int(np.prod(self.shape(name, 1))) * np.dtype(self.table[name][0]).itemsize


def _rays(*more):
    return (Input("d_origin", 3, True), Input("d_direction", 3, True)) + more


def _host(names, answers):
    return dict(zip(names, answers))


def _limit(world, name, n, limited):
    return world.host[name][:n] if limited else None


CLOSEST = Query(
    "trace_closest_device", ("d_origin", "d_direction", "d_t_max", "d_hit_id", "d_t", "d_hit_point", "d_normal"), _rays(Input("d_t_max", None, False)),
    p3d._TRACE_OUTPUTS, ("hit_id", "t", "hit_point", "normal"), ("hit_id",), limit="d_t_max", witness="t",
    call=lambda dev, accel, i, want, stream, out: dev.trace_closest_device(accel, i["d_origin"], i["d_direction"], t_max=i.get("d_t_max"), want=want, stream=stream, out=out))

ANY = Query(
    "trace_any_device", ("d_origin", "d_direction", "d_t_max", "d_occluded"), _rays(Input("d_t_max", None, False)),
    {"occluded": ("uint8", None)}, ("occluded",), ("occluded",), limit="d_t_max", witness="occluded",
    call=lambda dev, accel, i, want, stream, out: dev.trace_any_device(accel, i["d_origin"], i["d_direction"], t_max=i.get("d_t_max"), stream=stream, out=out))

NEAREST = Query(
    "nearest_device", ("d_point", "d_max_dist", "d_object", "d_dist", "d_closest", "d_normal"), (Input("d_point", 3, True), Input("d_max_dist", None, False)),
    p3d._NEAREST_OUTPUTS, ("object", "dist", "closest", "normal"), ("object",), limit="d_max_dist", witness="dist", refuses_planes=True,
    call=lambda dev, accel, i, want, stream, out: dev.nearest_device(accel, i["d_point"], max_dist=i.get("d_max_dist"), want=want, stream=stream, out=out),
    host_form=lambda hs, w, n, limited: _host(("object", "dist", "closest"), hs.nearest(w.host["d_point"][:n], max_dist=_limit(w, "d_max_dist", n, limited))),
    assert_mixed=lambda got, n: 0 < (got["object"] >= 0).sum() < n)


def nearest_k(k):
    """p3d_nearest_k_device at this k; the limits of a world are its limits(k): (host array, device tensor)"""
    def mixed(got, n):
        c = got["count"]  # the three sorts of point in one batch
        return bool((c == 0).any() and (c == k).any() and (k == 1 or ((c > 0) & (c < k)).any()))

    return Query(
        "nearest_k_device", (k, "d_point", "d_max_dist", "d_count", "d_object", "d_dist", "d_closest", "d_normal"),
        (Input("d_point", 3, True), Input("d_max_dist", None, False)), p3d._nearest_k_outputs(k), ("count", "object", "dist", "closest", "normal"),
        ("count", "object"), limit="d_max_dist", witness="dist", refuses_planes=True, assert_mixed=mixed,
        call=lambda dev, accel, i, want, stream, out: dev.nearest_k_device(accel, i["d_point"], k, max_dist=i.get("d_max_dist"), want=want, stream=stream, out=out),
        inputs_of=lambda w, n, limited=False: dict({"d_point": w.dev["d_point"][:n]}, **({"d_max_dist": w.limits(k)[1][:n]} if limited else {})),
        host_form=lambda hs, w, n, limited: _host(("count", "object", "dist", "closest"),
                                                  hs.nearest_k(w.host["d_point"][:n], k, max_dist=w.limits(k)[0][:n] if limited else None)))


def trace_hits(k, **own):
    """p3d_trace_hits_device at this k; `own`: what its module adds (assert_tree: there is no exact CPU twin)"""
    return Query(
        "trace_hits_device", (k, "d_origin", "d_direction", "d_t_max", "d_count", "d_total", "d_object", "d_t", "d_hit_point", "d_normal"),
        _rays(Input("d_t_max", None, False)), p3d._trace_hits_outputs(k), ("count", "total", "object", "t", "hit_point", "normal"),
        ("count", "object") if k else ("total",), limit="d_t_max", witness="t", on_stream=(BVH, NONE),
        call=lambda dev, accel, i, want, stream, out: dev.trace_hits_device(accel, i["d_origin"], i["d_direction"], k, t_max=i.get("d_t_max"), want=want, stream=stream, out=out),
        **own)


SWEEP = Query(
    "sweep_sphere_device", ("d_origin", "d_direction", "d_radius", "d_t_max", "d_object", "d_t", "d_centre", "d_contact", "d_normal"),
    _rays(Input("d_radius", None, True), Input("d_t_max", None, False)), p3d._SWEEP_OUTPUTS, ("object", "t", "centre", "contact", "normal"), ("object",),
    limit="d_t_max", witness="t", refuses_planes=True,
    call=lambda dev, accel, i, want, stream, out: p3d.sweep_sphere_device(dev, accel, i["d_origin"], i["d_direction"], i["d_radius"], t_max=i.get("d_t_max"),
                                                                         want=want, stream=stream, out=out),
    host_form=lambda hs, w, n, limited: _host(("object", "t", "centre", "contact"), p3d.host_sweep_sphere(
        hs, w.host["d_origin"][:n], w.host["d_direction"][:n], w.host["d_radius"][:n], t_max=_limit(w, "d_t_max", n, limited))))


def occlusion(samples, **kw):
    """p3d_occlusion_device with `samples` samples; kw: the other fields of its parameters, as occlusion_device takes them"""
    par = dict(dict(seed=0, samples=samples, sample_begin=0, point_offset=0, flags=0, bias=1e-4, team=0), **kw)
    params = p3d.OcclusionParams(**par)  # (held here: the raw calls pass its address)
    del par["samples"]
    return Query(
        "occlusion_device", ("d_point", "d_normal", "d_max_dist", C.byref(params), "d_unoccluded", "d_bent"),
        (Input("d_point", 3, True), Input("d_normal", 3, True), Input("d_max_dist", None, False)), p3d._OCCLUSION_OUTPUTS, ("unoccluded", "bent"),
        ("unoccluded",), limit="d_max_dist",
        call=lambda dev, accel, i, want, stream, out: p3d.occlusion_device(dev, accel, i["d_point"], i["d_normal"], samples, max_dist=i.get("d_max_dist"),
                                                                          want=want, stream=stream, out=out, **par))


def trace_radiance(max_depth, flags=0):
    return Query(
        "trace_radiance_device", ("d_origin", "d_direction", max_depth, flags, "d_rgb", "d_hit_id"), _rays(), p3d._RADIANCE_OUTPUTS, ("rgb", "hit_id"), ("rgb",),
        call=lambda dev, accel, i, want, stream, out: p3d.trace_radiance_device(dev, accel, i["d_origin"], i["d_direction"], max_depth, flags=flags, want=want,
                                                                               stream=stream, out=out))


def trace_path(max_depth, samples=1, sample_begin=0, seed=0, flags=0):
    return Query(
        "trace_path_device", ("d_origin", "d_direction", max_depth, sample_begin, samples, seed, "d_rng", flags, "d_rgb", "d_hit_id"),
        _rays(Input("d_rng", 2, False, "int64", guarded=False)), p3d._PATH_OUTPUTS, ("rgb", "hit_id"), ("rgb",),
        call=lambda dev, accel, i, want, stream, out: p3d.trace_path_device(dev, accel, i["d_origin"], i["d_direction"], max_depth, samples=samples,
                                                                           sample_begin=sample_begin, seed=seed, rng=i.get("d_rng"), flags=flags, want=want,
                                                                           stream=stream, out=out))


def every_query():
    """One description of each of the queries, for the checks that need no GPU"""
    return [CLOSEST, ANY, NEAREST, nearest_k(3), trace_hits(2), SWEEP, occlusion(4), trace_radiance(4), trace_path(4)]


# ---- a world ----------------------------------------------------------------------------------------------------------------------

class World:
    """One scene: its path, the host scene, the device scenes by tree (`grid`: each with the grid its tree's builder makes),
    and - attached by the module that builds it - the query's inputs by C name on the host (.host) and the device (.dev)"""

    def __init__(self, path, trees, grid=False, legacy=False):
        self.path = path
        self.hs = p3d.HostScene(path, legacy_f11=legacy)
        self.devs = {tree: p3d.DeviceScene(self.hs, bvh=TREES[tree], **({"grid": TREES[tree]} if grid else {})) for tree in trees}
        self.host, self.dev = {}, {}

    def attach(self, **inputs):
        for name, a in inputs.items():
            self.host[name] = np.ascontiguousarray(a)
            self.dev[name] = gpu(self.host[name])

    def accels(self, tree):
        return [NONE] if tree == "none" else [NONE, BVH]

    def back_ends(self):
        """(tree, device scene, accel) for every accel every device scene answers"""
        return [(tree, dev, accel) for tree, dev in self.devs.items() for accel in self.accels(tree)]


def assert_deep(dev):
    assert dev.export_bvh()["bvh_max_depth"] > 16  # deeper than the 16-entry LDS window of the stack: the spill path runs


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def assert_refused(cases):
    """cases: (what, code, a word of the message, call): every call raises P3DError with that code and word"""
    for what, code, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == code and word in str(e.value), "%s: %s" % (what, e.value)


def sentinels(query, n):
    return query.outputs(n, fill=(77, 123.0))


def assert_untouched(outs):
    """after every refusal: no output of sentinels() was written"""
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert bool((t == (123.0 if t.dtype.is_floating_point else 77)).all()), "a refused call wrote " + name


def check_buffer_refusals(query, dev, inputs, n, planes=None):
    """The refusals check_query_buffers, check_accel and the wrapper make for every query, none of which may enqueue anything.
    dev: a scene with a tree; inputs: n good rows per input by C name (an optional one left out is made up here); planes: a
    World of a scene with planes, where the query refuses those under the tree -> the outputs of sentinels(), found untouched,
    for the module's own refusals to go on with (and assert_untouched again)"""
    lib = p3d.lib()
    no_tree = p3d.DeviceScene(p3d.HostScene(dev.host.path), bvh=False)  # (a host scene that has built its tree once keeps it in its descriptor)
    real = {i.name: inputs[i.name] if inputs.get(i.name) is not None else
            torch.zeros((n,) if i.cols is None else (n, i.cols), dtype=getattr(torch, i.dtype), device="cuda") for i in query.inputs}
    needed = {i.name: real[i.name] for i in query.inputs if i.required}
    outs = sentinels(query, n)
    required_outs = {"d_" + name: outs[name] for name in query.required}
    host = np.zeros((n, 4), np.float64)
    # Host memory must be refused BEFORE any launch.  It goes in first, through the entry point itself, with a count no buffer
    # here can serve: were the pointer check to let it through, the next buffer would end behind its allocation: no kernel
    # would ever be given a host address.
    first = query.inputs[0].name
    assert query.raw(dev, BVH, BIG, **dict(needed, **{first: host.ctypes.data}), **required_outs) == INVALID
    assert ("%s is host memory" % first).encode() in lib.p3d_last_error(), lib.p3d_last_error()
    # Every other bad buffer goes in under that count as well, through the wrapper, next to buffers that can serve it: `huge`
    # (never read, never written: every call it is given to is refused) for the inputs, and for the outputs the sentinels -
    # too short, the net under a refusal that went missing - but where a required output itself is the one too short: there
    # the outputs in front of it are `huge` too.
    # (too short: torch hands out pieces of larger allocations, so "behind the allocation" needs a count beyond any of them)
    huge = torch.empty((BIG, 3), device="cuda")
    assert all(torch.zeros((1,) if i.cols is None else (1, i.cols), dtype=getattr(torch, i.dtype)).nbytes <= 12 for i in query.inputs if i.required)
    assert all(query.row_bytes(name) <= 12 for name in query.required)
    far = lambda t: (t.data_ptr(), BIG)
    everywhere = {i.name: far(huge) for i in query.inputs if i.required}
    short_out, huge_out = {name: far(outs[name]) for name in query.required}, {name: far(huge) for name in query.required}
    cases = []
    for i in (i for i in query.inputs if i.guarded):
        cases += [("a misaligned " + i.name, "aligned", dict(everywhere, **{i.name: (real[i.name].data_ptr() + 2, BIG)}), (), short_out),
                  ("a host " + i.name, i.name + " is host memory", dict(everywhere, **{i.name: (host.ctypes.data, BIG)}), (), short_out),
                  (i.name + " too short", i.name + " ends behind its allocation", dict(everywhere, **{i.name: far(real[i.name])}), (), short_out)]
    for name in query.required:
        cases.append(("d_%s too short" % name, "d_%s ends behind its allocation" % name, everywhere, (), dict(huge_out, **{name: far(outs[name])})))
    words = [name for name in query.table if np.dtype(query.table[name][0]).itemsize >= 4]  # (the library aligns floats and int32s)
    for name in [w for w in words if w in query.optional][:1] or words[:1]:
        cases.append(("a misaligned d_" + name, "aligned", everywhere, (name,) if name in query.optional else (),
                      dict(short_out, **{name: (outs[name].data_ptr() + 2, BIG)})))
    for accel in (NONE, BVH):
        assert_refused([("%s, accel %d" % (what, accel), INVALID, word, lambda ins=ins, want=want, out=out: query.call(dev, accel, ins, want, 0, out))
                        for what, word, ins, want, out in cases])
    del huge
    # the accel: one there is not, and the tree of a scene that has none; with good buffers of n rows, as the null pointers below
    scenes = [dev, no_tree]
    accels = [("an unknown accel", INVALID, "accel", dev, 7), ("a scene without a tree", INVALID, "without BVH", no_tree, BVH)]
    if query.refuses_planes and planes is not None:
        scenes.append(p3d.DeviceScene(planes.hs, bvh=True))
        accels.append(("a tree over a scene with planes", UNSUPPORTED, "plane", scenes[-1], BVH))
    assert_refused([(what, code, word, lambda scene=scene, accel=accel: query.call(scene, accel, needed, query.optional, 0, outs))
                    for what, code, word, scene, accel in accels])
    every = dict(needed, **{"d_" + name: t for name, t in outs.items()})
    for name in list(needed) + list(required_outs):
        assert query.raw(dev, BVH, n, **dict(every, **{name: None})) == INVALID, "a null " + name
        assert b"null argument" in lib.p3d_last_error(), "a null %s: %s" % (name, lib.p3d_last_error())
    if len(scenes) == 3:  # the planes are there for the brute force
        assert_same_bits(only(query.ask(scenes[2], NONE, query.inputs_of(planes, n), want=()), query.required),
                         only(query.host_form(planes.hs, planes, n, False), query.required), query.name + ": the brute force over planes")
    assert_untouched(outs)
    assert all(scene.status() == 0 for scene in scenes)
    return outs


# ---- batches and outputs ----------------------------------------------------------------------------------------------------------

def check_ragged_batches(query, world, n, free, limited, what, also=None):
    """The first n rows through every back end of the world, without and with limits: the host form's answers `free` and
    `limited` ({name: array} of at least n rows; None: not asked) bit for bit, and the no-answer values exact.
    also(dev, got, is_limited, what): the module's own checks on each answer"""
    for tree, dev, accel in world.back_ends():
        for is_limited, want in ((False, free), (True, limited)):
            if want is None:
                continue
            label = "%s, %s tree, accel %d, %d rows%s" % (what, tree, accel, n, ", limits" if is_limited else "")
            got = query.ask(dev, accel, query.inputs_of(world, n, is_limited))
            assert_answers(got, want, query.table, label)
            if also is not None:
                also(dev, got, is_limited, label)
        assert dev.status() == 0


def check_empty_batch(query, dev):
    """n == 0 returns 0 and launches nothing, whatever the pointers"""
    for accel in (NONE, BVH):
        assert query.raw(dev, accel, 0) == 0, p3d.lib().p3d_last_error()
    assert dev.status() == 0


def check_callers_outputs(query, dev, accel, inputs, want, what, optional=()):
    """Outputs may be the caller's tensors, which come back themselves, and the optional ones may be left out.  want: the
    answers to these inputs by name: the required outputs and those of `optional`, which the caller's outputs take along"""
    n = len(next(iter(want.values())))
    mine = {name: t for name, t in query.outputs(n, fill=(77, 5.0)).items() if name in query.required or name in optional}
    back = query.call(dev, accel, inputs, tuple(optional), 0, mine)
    assert list(back) == list(mine) and all(back[name] is mine[name] for name in mine), what + ": the caller's outputs"
    assert_same_bits({name: t.cpu().numpy() for name, t in mine.items()}, only(want, mine), what + ": the caller's outputs")
    alone = query.ask(dev, accel, inputs, want=())
    assert_same_bits(alone, only(want, query.required), what + ": the required outputs alone")


# ---- behind an update on the same stream ---------------------------------------------------------------------------------------

def _assert_sees_the_moved_scene(query, world, hs, n, got, what, before):
    """got: {limited: {accel: answers}}, taken behind the update; hs: the host scene given the moved geometry.  The answers are
    those of a fresh scene of that geometry under ACCEL_NONE, the host form's where there is one, and not those of before"""
    fresh = p3d.DeviceScene(hs, bvh=False)
    for limited, by_accel in got.items():
        label = what + (", limits" if limited else "")
        inputs = query.inputs_of(world, n, limited)
        again = query.ask(fresh, NONE, inputs)
        want = query.host_form(hs, world, n, limited) if query.host_form else None
        for accel, answers in by_accel.items():
            if accel == BVH and query.assert_tree:
                query.assert_tree(answers, again, hs, world, n, limited, label)
                continue
            if want is not None:
                assert_answers(answers, want, query.table, "%s, accel %d" % (label, accel))
            assert_same_bits(answers, again, "%s, accel %d, against a fresh scene" % (label, accel))
        # (as it was: the module's cached host answers, or the brute force of one of the world's own device scenes)
        was = before[limited] if before else query.ask(next(iter(world.devs.values())), NONE, inputs)
        assert as_bytes(again[query.witness]) != as_bytes(was[query.witness][:n]), label + ": the update moved nothing the query can see"
    assert fresh.status() == 0


def check_behind_a_refit(query, world, n, soup=None, what="behind a refit", before=None):
    """refit_triangles with moved positions on a side stream, the query (with limits) behind it on that stream, nothing in
    between, the positions still being produced when the calls begin.  world: triangles only; soup(arrays) -> the moved
    (3F, 3) positions (default: every vertex displaced by up to 3 % of the scene's diagonal); before: {limited: the answers of
    the scene as it was}, where the module holds the host form's already"""
    hs = p3d.HostScene(world.path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    soup = deformed_mesh(a, seed=91, fraction=0.03)[2] if soup is None else soup(a)
    base, d_soup = gpu(a["prim_v"].reshape(-1, 3)), gpu(soup)
    inputs = query.inputs_of(world, n, True)
    outs = {accel: query.outputs(n) for accel in query.on_stream}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        wave = base
        for _ in range(50):  # some work in front, so that the positions are still being produced when the calls begin
            wave = torch.sin(wave * 1.5 + 0.25)
        moved = (d_soup + 0.0 * wave).contiguous()
        dev.refit_triangles(0, moved, stream=side)
        for accel in query.on_stream:
            query.call(dev, accel, inputs, query.optional, side, outs[accel])
    side.synchronize()
    got = {accel: {name: t.cpu().numpy() for name, t in outs[accel].items()} for accel in query.on_stream}
    assert as_bytes(moved.cpu().numpy()) == as_bytes(soup)
    hs.set_geometry(*p3d.deformed(a["prim_v"], 0, soup))
    _assert_sees_the_moved_scene(query, world, hs, n, {True: got}, what, before)
    if query.assert_mixed:
        assert query.assert_mixed(got[BVH], n), what + ": found and not found in one batch"
    assert dev.status() == 0


def check_behind_a_pose(query, world, n, limits=(False, True), what="behind a pose", before=None):
    """pose_device on a side stream, the query behind it on that stream - without limits and with them - nothing in between"""
    hs = p3d.HostScene(world.path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    ranges, xforms, scale = plan(a, 93)  # spheres and triangles under a rigid move, boxes under a positive-diagonal one
    dev.set_rig(ranges, 2)
    inputs = {limited: query.inputs_of(world, n, limited) for limited in limits}
    side = torch.cuda.Stream()
    d_x, d_s = gpu(xforms), gpu(scale)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dev.pose_device(d_x, d_s, stream=side)
        res = {limited: {accel: query.call(dev, accel, inputs[limited], query.optional, side, None) for accel in query.on_stream} for limited in limits}
    side.synchronize()
    got = {limited: {accel: {name: t.cpu().numpy() for name, t in r.items()} for accel, r in by_accel.items()} for limited, by_accel in res.items()}
    hs.set_geometry(*p3d.transformed(a["prim_type"], a["prim_v"], ranges, xforms, scale))
    _assert_sees_the_moved_scene(query, world, hs, n, got, what, before)
    assert dev.status() == 0

"""The lights and materials of a live scene (include/p3d_shading.h) on the GPU: p3d_scene_set_materials, p3d_scene_set_lights,
their readbacks and p3d_scene_set_shading_device.

The yardstick is exact.  The "twin" of an updated scene is a fresh DeviceScene of a HostScene given the same values through
host_set_materials / host_set_lights, built the same way; "equal" is assert_same_frames: every colour bit, hit ids and
counters.  Frames are 96 x 96 through live_scene_checks.configs (Whitted depth 4 in the literal and per-pixel modes, the 4-spp
path trace for cornell).  Every comparison has tolerance 0 but the oracle anchor, which has check_whitted's own.  Every scene
that is updated is created by its test.

status() returns the code of p3d_scene_status (it does not raise): a skipped material shows as status() == -1 with the two
counts in p3d_last_error, and a second status() is 0.

Not asserted: that the stream form allocates nothing after a scene's first such call.  There is no instrument for it; it holds
by construction (the counter block is the only allocation, the records are the caller's)."""
import ctypes as C

import numpy as np
import pytest
import torch

import p3d_amd as p3d
from conftest import scene_path
from device_query_contract import INVALID
from frame_checks import CORNELL, assert_same_frames, check_whitted, frames, frames_differ, gpu, same_bits_or_nan
from live_scene_checks import camera_rays, configs, last_error, legacy, produced, trace_outputs
from oracle import binding as ob
from shading_update_checks import (COL, DIFF, EMIT, IOR, KD, KS, REFL, RES, SHINE, T, THREADS, assert_readback, changed_file, host, readback,
                                   seeded, tables, tiny_scene, twin)

pytestmark = pytest.mark.gpu

BUILDS = {
    "balls_low": lambda hs: p3d.DeviceScene(hs, bvh=True, grid=True),  # the host's tree and grid: no geometry update accepts it
    "tri5k": lambda hs: p3d.DeviceScene(hs, bvh="device"),
    "balls_box": lambda hs: p3d.DeviceScene(hs, bvh=True),
    "cornell": lambda hs: p3d.DeviceScene(hs, bvh=True),
}
ACCELS = {"balls_low": (p3d.ACCEL_BVH, p3d.ACCEL_GRID, p3d.ACCEL_NONE), "tri5k": (p3d.ACCEL_BVH, p3d.ACCEL_NONE),
          "balls_box": (p3d.ACCEL_BVH, p3d.ACCEL_NONE), "cornell": (p3d.ACCEL_BVH, p3d.ACCEL_NONE)}


@pytest.fixture
def paths(tri5k_path):
    return {"balls_low": scene_path("balls_low.p3f"), "tri5k": tri5k_path, "balls_box": scene_path("balls_box.p3f"), "cornell": CORNELL}


def all_frames(dev, name):
    return [f for accel in ACCELS[name] for f in frames(dev, configs(name, accel))]


def assert_twin(dev, name, path, mats, lights, what, build=None):
    """dev renders what a fresh scene of the file with these whole tables renders, through every accel it has -> dev's frames"""
    _, fresh = twin(path, build or BUILDS[name], mats, 0, lights, 0)
    now = all_frames(dev, name)
    assert_same_frames(now, all_frames(fresh, name), what)
    return now


def stream_update(dev, mats=None, first_mat=0, lights=None, first_light=0):
    """set_shading_device on a side stream, the rows as device tensors; waits for the stream"""
    side = torch.cuda.Stream()
    d_m = gpu(mats) if mats is not None and len(mats) else None
    d_l = gpu(lights) if lights is not None and len(lights) else None
    torch.cuda.synchronize()
    p3d.set_shading_device(dev, d_m, first_mat, d_l, first_light, stream=side)
    side.synchronize()


# 1. the waiting form is the twin
@pytest.mark.parametrize("name", ["balls_low", "tri5k", "balls_box", "cornell"])
def test_the_waiting_form_is_the_twin(name, paths):
    """Fails on the parent commit: the symbols do not exist"""
    hs = host(paths[name])
    dev = BUILDS[name](hs)
    before = all_frames(dev, name)
    mats, lights = tables(hs)
    assert_readback(dev, mats, lights, "a fresh scene")
    new_m, new_l = seeded(mats, lights, 500 + len(name))
    p3d.set_materials(dev, 0, new_m)
    p3d.set_lights(dev, 0, new_l)  # (cornell has no lights: an empty array, a no-op)
    assert_readback(dev, new_m, new_l, name)
    now = assert_twin(dev, name, paths[name], new_m, new_l, name)
    assert frames_differ(now, before), "the update changed no pixel"
    assert dev.status() == 0


# 2. the derived facts follow
def test_the_emitter_list_follows(paths):
    name = "cornell"
    hs = host(paths[name])
    a = hs.arrays()
    dev = BUILDS[name](hs)
    mats, lights = tables(hs)
    emitting = np.nonzero(mats[:, EMIT].sum(1) > 0)[0]
    spheres = sorted(set(a["prim_material"][a["prim_type"] == 0]))  # P3D_PRIM_SPHERE
    assert list(emitting) == [spheres[-1]] and len(spheres) == 3
    first = all_frames(dev, name)
    assert first[0][3]["rays_light"] > 0
    # the emission moves from the light sphere to the mirror sphere: the list keeps its length, with another object in it
    moved = mats.copy()
    moved[spheres[0], EMIT], moved[emitting[0], EMIT] = mats[emitting[0], EMIT], 0
    p3d.set_materials(dev, 0, moved)
    now = assert_twin(dev, name, paths[name], moved, lights, "the emission moved")  # (rays_light is among the counters compared)
    assert frames_differ(now, first) and now[0][3]["rays_light"] > 0
    # two emitters: the list grows
    both = moved.copy()
    both[emitting[0], EMIT] = mats[emitting[0], EMIT]
    p3d.set_materials(dev, emitting[0], both[emitting[0]:emitting[0] + 1])
    grown = assert_twin(dev, name, paths[name], both, lights, "two emitters")
    assert grown[0][3]["rays_light"] > now[0][3]["rays_light"]
    # no emission at all: the list is empty
    dark = mats.copy()
    dark[:, EMIT] = 0
    p3d.set_materials(dev, 0, dark)
    none = assert_twin(dev, name, paths[name], dark, lights, "no emitter")
    assert none[0][3]["rays_light"] == 0
    p3d.set_materials(dev, 0, mats)
    assert_same_frames(all_frames(dev, name), first, "the file's materials again")
    assert dev.status() == 0


def test_the_literal_variant_follows(paths):
    name = "balls_low"
    hs = host(paths[name])
    dev = BUILDS[name](hs)
    mats, lights = tables(hs)
    mirror = int(np.nonzero((mats[:, REFL] > 0) & (mats[:, T] == 0))[0][0])
    cfg = configs(name)[0][1]
    assert cfg.stack_mode == p3d.STACK_LITERAL
    assert dev.frame_plan(cfg).zero_weight_reflections == 0
    first = all_frames(dev, name)
    glass = mats.copy()
    glass[mirror, T], glass[mirror, IOR] = 0.6, 1.5  # transmissive with reflection > 0: a LITERAL frame traces zero-weight reflections
    p3d.set_materials(dev, mirror, glass[mirror:mirror + 1])
    assert dev.frame_plan(cfg).zero_weight_reflections == 1
    now = assert_twin(dev, name, paths[name], glass, lights, "a mirror made transmissive")
    assert frames_differ(now, first)
    p3d.set_materials(dev, mirror, mats[mirror:mirror + 1])
    assert dev.frame_plan(cfg).zero_weight_reflections == 0
    assert_same_frames(all_frames(dev, name), first, "the mirror again")
    assert dev.status() == 0


def nan_frames(dev, name):
    return [(label, rgb, hit) for label, rgb, hit, _ in all_frames(dev, name)]


@pytest.mark.parametrize("colour", [float("inf"), -0.5])
@pytest.mark.parametrize("form", ["waiting", "stream"])
def test_the_pow_flag_follows(form, colour, paths):
    """balls_low's first material has Ks == 0: under plain lights its pow is left out.  A light colour of +inf makes the term
    inf x 0 = NaN, a negative one makes it a signed zero: the kernels must evaluate it again, as a fresh scene's do"""
    name = "balls_low"
    hs = host(paths[name])
    dev = BUILDS[name](hs)
    mats, lights = tables(hs)
    assert mats[0, KS] == 0 and (lights[:, COL] == 1).all()
    first = all_frames(dev, name)
    odd = lights.copy()
    odd[-1, 4 + 1] = colour
    if form == "waiting":
        p3d.set_lights(dev, len(lights) - 1, odd[-1:])
    else:
        stream_update(dev, lights=odd[-1:], first_light=len(lights) - 1)
    assert_readback(dev, mats, odd, "an odd light")
    _, fresh = twin(paths[name], BUILDS[name], lights=odd)
    got, want = nan_frames(dev, name), nan_frames(fresh, name)
    for (label, rgb_a, hit_a), (_, rgb_b, hit_b) in zip(got, want):
        assert np.array_equal(hit_a, hit_b), label
        assert same_bits_or_nan(rgb_a, rgb_b).all(), "%s: %d values differ" % (label, int((~same_bits_or_nan(rgb_a, rgb_b)).sum()))
    if colour == float("inf"):
        assert np.isnan(want[0][1]).any(), "the twin has no NaN pixel: the flag is not tested"
    if form == "waiting":
        p3d.set_lights(dev, len(lights) - 1, lights[-1:])
    else:
        stream_update(dev, lights=lights[-1:], first_light=len(lights) - 1)
    assert_same_frames(all_frames(dev, name), first, "the light again")
    assert dev.status() == 0


# 3. one oracle anchor
def test_the_changed_scene_is_the_oracles(paths, tmp_path):
    name = "balls_low"
    hs = host(paths[name])
    dev = BUILDS[name](hs)
    mats, lights = tables(hs)
    new_m, new_l = seeded(mats, lights, 500 + len(name))  # the values of test 1
    p3d.set_materials(dev, 0, new_m)
    p3d.set_lights(dev, 0, new_l)
    path = changed_file(paths[name], str(tmp_path / "changed.p3f"), new_m, new_l)
    m2, l2 = tables(host(path))
    assert m2.tobytes() == new_m.tobytes() and l2.tobytes() == new_l.tobytes(), "the file does not say the changed scene"
    sc = ob.Scene(path, legacy_f11=legacy(path))
    sc.set_resolution(RES, RES)
    check_whitted(dev, sc, p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4))


# 4. the stream form is the waiting form
@pytest.mark.parametrize("name, part", [("balls_low", "materials"), ("balls_low", "lights"), ("balls_low", "both"), ("tri5k", "both"),
                                        ("cornell", "materials")])  # (cornell has no lights)
def test_the_stream_form_is_the_waiting_form(name, part, paths):
    hs = host(paths[name])
    dev_w, dev_s = BUILDS[name](hs), BUILDS[name](hs)
    mats, lights = tables(hs)
    new_m, new_l = seeded(mats, lights, 540 + len(name))
    use_m, use_l = part != "lights", part != "materials"
    want_m, want_l = (new_m if use_m else mats), (new_l if use_l else lights)
    _, fresh = twin(paths[name], BUILDS[name], want_m, 0, want_l, 0)
    cam = p3d.camera_rays_device(fresh)
    o, d = cam["origin"], cam["direction"]
    want = p3d.trace_radiance_device(fresh, p3d.ACCEL_BVH, o, d, 4)
    base_m, base_l = gpu(new_m), (gpu(new_l) if len(new_l) else None)
    ballast = torch.linspace(0, 1, 1 << 20, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        slow = produced(ballast, 1.0, rounds=20)
        d_m = (base_m + 0.0 * slow[:base_m.numel()].view(base_m.shape)).contiguous() if use_m else None
        d_l = (base_l + 0.0 * slow[:base_l.numel()].view(base_l.shape)).contiguous() if use_l else None
        p3d.set_shading_device(dev_s, d_m, 0, d_l, 0, stream=side)  # no synchronisation between producer, update and query
        got = p3d.trace_radiance_device(dev_s, p3d.ACCEL_BVH, o, d, 4, stream=side)
    side.synchronize()
    if use_m:
        assert d_m.cpu().numpy().tobytes() == new_m.tobytes()
    if use_l:
        assert d_l.cpu().numpy().tobytes() == new_l.tobytes()
    for k in ("rgb", "hit_id"):
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), "%s of the rays traced behind the update" % k
    if use_m:
        p3d.set_materials(dev_w, 0, new_m)
    if use_l:
        p3d.set_lights(dev_w, 0, new_l)
    assert readback(dev_s) == readback(dev_w)
    assert_readback(dev_s, want_m, want_l, "the stream form")
    assert_same_frames(all_frames(dev_s, name), all_frames(dev_w, name), "%s, %s" % (name, part))
    assert dev_s.status() == 0


# 5. the smallest shapes the kernel can get wrong
PER_PIXEL = [("whitted per pixel", p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3, stack_mode=p3d.STACK_PER_PIXEL, collect_stats=1))]


def nan_equal(a, b, what):
    for (label, rgb_a, hit_a, _), (_, rgb_b, hit_b, _) in zip(a, b):
        assert np.array_equal(hit_a, hit_b), what
        assert same_bits_or_nan(rgb_a, rgb_b).all(), "%s: %d values differ" % (what, int((~same_bits_or_nan(rgb_a, rgb_b)).sum()))


@pytest.mark.parametrize("span", ["first", "last", "all"])
@pytest.mark.parametrize("n_mats, n_lights", [(1, 0), (2, 1), (3, 65), (2, THREADS + 1), (max(257, THREADS + 1), 2)])
def test_the_smallest_shapes(n_mats, n_lights, span, tmp_path):
    """Lights: none (plain), one, more than a wave's lanes, more than a workgroup's threads; materials: more than a workgroup.
    Three stream updates of the span: seeded values; then its last light +inf, which only the reduction over ALL effective
    lights can tell every Ks == 0 material; then the light back"""
    path = tiny_scene(str(tmp_path / "tiny.p3f"), n_mats, n_lights)
    build = lambda hs: p3d.DeviceScene(hs, bvh="device")
    hs = host(path, 64)
    dev = build(hs)
    mats, lights = tables(hs)
    assert mats.shape == (n_mats, 16) and lights.shape == (n_lights, 8)
    new_m, new_l = seeded(mats, lights, 560 + n_mats + n_lights)
    new_m[:, KS] = new_m[:, REFL] = mats[:, KS]  # (the Ks == 0 materials stay so)
    fm, cm = {"first": (0, 1), "last": (n_mats - 1, 1), "all": (0, n_mats)}[span]
    fl, cl = {"first": (0, min(1, n_lights)), "last": (max(n_lights - 1, 0), min(1, n_lights)), "all": (0, n_lights)}[span]
    want_m, want_l = mats.copy(), lights.copy()
    want_m[fm:fm + cm], want_l[fl:fl + cl] = new_m[fm:fm + cm], new_l[fl:fl + cl]
    before = frames(dev, PER_PIXEL)
    stream_update(dev, want_m[fm:fm + cm], fm, want_l[fl:fl + cl], fl)
    assert_readback(dev, want_m, want_l, "the span")
    _, fresh = twin(path, build, want_m, 0, want_l, 0, res=64)
    now = frames(dev, PER_PIXEL)
    assert_same_frames(now, frames(fresh, PER_PIXEL), "%d materials, %d lights, %s" % (n_mats, n_lights, span))
    assert span != "all" or not n_lights or frames_differ(now, before)  # (without lights a Whitted frame of these spheres is black)
    if n_lights:
        odd = want_l.copy()
        odd[fl + cl - 1, COL] = np.inf
        stream_update(dev, lights=odd[fl:fl + cl], first_light=fl)
        assert_readback(dev, want_m, odd, "the odd light")
        _, fresh_odd = twin(path, build, want_m, 0, odd, 0, res=64)
        want_odd = frames(fresh_odd, PER_PIXEL)
        assert np.isnan(want_odd[0][1]).any()
        nan_equal(frames(dev, PER_PIXEL), want_odd, "an infinite light")
        stream_update(dev, lights=want_l[fl:fl + cl], first_light=fl)
        assert_same_frames(frames(dev, PER_PIXEL), now, "the light again")
    assert dev.status() == 0


def test_an_empty_call_is_a_no_op(paths):
    name = "cornell"
    hs = host(paths[name], 64)
    dev = BUILDS[name](hs)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=3, max_depth=8, seed=9)
    acc = dev.accumulator(cfg)
    acc.render(2)
    was = readback(dev)
    L = p3d.lib()
    assert L.p3d_scene_set_shading_device(dev._h, 0, 0, None, 0, 0, None, None) == 0
    assert L.p3d_scene_set_materials(dev._h, 0, 0, None) == 0 and L.p3d_scene_set_lights(dev._h, 0, 0, None) == 0
    p3d.set_shading_device(dev)
    acc.render(1)  # the memos are left alone: the accumulator goes on
    assert acc.samples_done == 3 and readback(dev) == was and dev.status() == 0


# 6. skips
def test_the_stream_form_skips_what_the_host_must_know(paths):
    name = "balls_box"
    hs = host(paths[name])
    dev_s, dev_w = BUILDS[name](hs), BUILDS[name](hs)
    mats, lights = tables(hs)
    assert len(mats) == 3 and (mats[:, EMIT] == 0).all() and (mats[:, T] == 0).all() and (mats[:, REFL] > 0).all()
    new = mats.copy()
    new[0, EMIT] = (2, 2, 2)       # would become emissive
    new[0, DIFF] = (0.1, 0.9, 0.1)
    new[1, T] = 0.5                # would become transmissive and reflective
    new[1, KD] = 0.4
    new[2, DIFF], new[2, SHINE] = (0.2, 0.3, 0.9), 50.0  # an ordinary change
    before = all_frames(dev_s, name)
    d_m = gpu(new)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert p3d.lib().p3d_scene_set_shading_device(dev_s._h, 0, 3, d_m.data_ptr(), 0, 0, None, C.c_void_p(side.cuda_stream)) == 0  # P3D_OK
    side.synchronize()
    kept = mats.copy()
    kept[2] = new[2]
    assert_readback(dev_s, kept, lights, "two skipped, one written")
    # frames rendered with stats in between neither report the skips nor clear them
    now = assert_twin(dev_s, name, paths[name], kept, lights, "a twin given only the third change")
    assert frames_differ(now, before)
    assert dev_s.status() == INVALID
    msg = last_error()
    assert "p3d_scene_set_shading_device: 1 material(s) that would change whether they emit, 1 material(s) that would change whether they are transmissive" in msg, msg
    assert dev_s.status() == 0
    # the waiting form makes the same changes
    p3d.set_materials(dev_w, 0, new)
    assert_readback(dev_w, new, lights, "the waiting form")
    assert frames_differ(assert_twin(dev_w, name, paths[name], new, lights, "a twin given all three"), now)
    assert dev_w.status() == 0
    # ... and from then on the stream form may change those materials within their new predicates
    again = new.copy()
    again[0, EMIT], again[1, T] = (1, 3, 1), 0.25
    stream_update(dev_w, again)
    assert_readback(dev_w, again, lights, "within the new predicates")
    assert dev_w.status() == 0


# 7. memos and neighbours
@pytest.mark.parametrize("form", ["waiting", "stream"])
def test_accumulators_refuse_passes_until_reset(form, paths):
    name = "cornell"
    hs = host(paths[name], 64)
    dev = BUILDS[name](hs)
    mats, lights = tables(hs)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=3, max_depth=8, seed=9)
    acc = dev.accumulator(cfg)
    ada = dev.adaptive(cfg, rel_error=0.05, min_samples=4)
    acc.render(2)
    ada.render(4)
    new_m, _ = seeded(mats, lights, 571)
    if form == "waiting":
        p3d.set_materials(dev, 0, new_m)
    else:
        stream_update(dev, new_m)
    for a, done in ((acc, 2), (ada, 4)):
        with pytest.raises(p3d.P3DError) as e:
            a.render(1)
        assert e.value.code == INVALID
        assert a.samples_done == done
        a.reset()
    _, fresh = twin(paths[name], BUILDS[name], new_m, res=64)
    f_acc = fresh.accumulator(cfg)
    got, want = acc.render(9), f_acc.render(9)
    assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()
    ada.render(4)
    assert dev.status() == 0


def test_closest_hits_are_unchanged_and_memoised_frames_follow(paths):
    name = "balls_low"
    hs = host(paths[name])
    dev = BUILDS[name](hs)
    mats, lights = tables(hs)
    o, d = camera_rays(hs.arrays(), 4096, seed=7)
    want = ("hit_id", "t")
    hits = dev.trace_closest_device(p3d.ACCEL_BVH, o, d, want=want, out=trace_outputs(4096))
    torch.cuda.synchronize()
    was = {k: hits[k].cpu().numpy().tobytes() for k in want}
    literal = configs(name)[:1]
    first = frames(dev, literal)
    assert_same_frames(frames(dev, literal), first, "the memoised frame")  # twice: schedules and row chains exist
    new_m, new_l = seeded(mats, lights, 572)
    for step, update in enumerate((lambda: (p3d.set_materials(dev, 0, new_m), p3d.set_lights(dev, 0, new_l)), lambda: stream_update(dev, mats, 0, lights, 0))):
        update()
        m, l = (new_m, new_l) if step == 0 else (mats, lights)
        _, fresh = twin(paths[name], BUILDS[name], m, 0, l, 0)
        now = frames(dev, literal)
        assert_same_frames(now, frames(fresh, literal), "a literal frame after update %d" % step)
        assert_same_frames(frames(dev, literal), now, "and once more")
        hits = dev.trace_closest_device(p3d.ACCEL_BVH, o, d, want=want, out=trace_outputs(4096))
        torch.cuda.synchronize()
        assert {k: hits[k].cpu().numpy().tobytes() for k in want} == was
    assert_same_frames(now, first, "the file's values again")
    assert dev.status() == 0


# 8. refusals with a device, nothing changed
def test_refusals_leave_the_scene_as_it_was(paths):
    name = "balls_low"
    hs = host(paths[name])
    dev = BUILDS[name](hs)
    mats, lights = tables(hs)
    n_m, n_l = len(mats), len(lights)
    new_m, new_l = seeded(mats, lights, 580)
    d_m, d_l = gpu(new_m), gpu(new_l)
    was = readback(dev)
    L = p3d.lib()
    dev_call = lambda fm, cm, pm, fl, cl, pl: L.p3d_scene_set_shading_device(dev._h, fm, cm, pm, fl, cl, pl, None)
    cases = [
        ("materials past the count", lambda: dev_call(1, n_m, d_m.data_ptr(), 0, 0, None), "end behind"),
        ("a first material that wraps", lambda: dev_call(0xffffffff, 2, d_m.data_ptr(), 0, 0, None), "end behind"),
        ("lights past the count", lambda: dev_call(0, 0, None, n_l, 1, d_l.data_ptr()), "end behind"),
        ("null d_materials with a count", lambda: dev_call(0, n_m, None, 0, 0, None), "null pointer"),
        ("null d_lights with a count", lambda: dev_call(0, 0, None, 0, n_l, None), "null pointer"),
        ("d_materials off by two bytes", lambda: dev_call(0, 1, d_m.data_ptr() + 2, 0, 0, None), "4-byte aligned"),
        ("d_lights off by one byte", lambda: dev_call(0, 0, None, 0, 1, d_l.data_ptr() + 1), "4-byte aligned"),
        # Host memory must be refused BEFORE any launch.  The pointers are checked in front of the ranges, so these calls also
        # name a range past the counts: were the pointer check to let them through, the range check would still refuse the
        # call, and no kernel would ever be given a host address or a buffer that is too short.
        ("host memory as d_materials", lambda: dev_call(1, n_m, new_m.ctypes.data, 0, 0, None), "is host memory"),
        ("host memory as d_lights", lambda: dev_call(0, 0, None, 1, n_l, new_l.ctypes.data), "is host memory"),
        ("materials that end behind their allocation", lambda: dev_call(0, 1 << 24, d_m.data_ptr(), 0, 0, None), "ends behind its allocation"),
        ("host materials past the count", lambda: L.p3d_scene_set_materials(dev._h, 1, n_m, new_m.ctypes.data), "end behind"),
        ("host lights past the count", lambda: L.p3d_scene_set_lights(dev._h, n_l, 1, new_l.ctypes.data), "end behind"),
        ("a null host array", lambda: L.p3d_scene_set_materials(dev._h, 0, 1, None), "null array"),
        ("a readback past the count", lambda: L.p3d_scene_lights(dev._h, 1, n_l, new_l.ctypes.data), "end behind"),
    ]
    for what, call, word in cases:
        assert call() == INVALID, what
        assert word in last_error(), "%s: %s" % (what, last_error())
        assert readback(dev) == was, what
    for what, word, call in [
        ("float64 materials", "materials: dtype", lambda: p3d.set_shading_device(dev, materials=d_m.double())),
        ("flat lights", "lights: shape", lambda: p3d.set_shading_device(dev, lights=d_l.view(-1))),
        ("lights of 6 columns", "lights: shape", lambda: p3d.set_shading_device(dev, lights=d_l[:, :6].contiguous())),
        ("CPU materials", "host memory", lambda: p3d.set_shading_device(dev, materials=d_m.cpu())),
        ("too many materials", "end behind", lambda: p3d.set_shading_device(dev, materials=torch.cat([d_m, d_m]))),
    ]:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == INVALID and word in str(e.value), "%s: %s" % (what, e.value)
        assert readback(dev) == was, what
    # the same call without a fault is accepted
    assert dev_call(0, n_m, d_m.data_ptr(), 0, n_l, d_l.data_ptr()) == 0
    assert_readback(dev, new_m, new_l, "the accepted call")
    assert dev.status() == 0

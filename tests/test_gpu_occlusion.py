"""Hemisphere occlusion at points in device memory (p3d_occlusion_device) and its rays (p3d_occlusion_rays_device) on the GPU.

The yardsticks are exact.  The written rays must be the host writer's bits (tests/test_occlusion_api.py holds that one to the
float64 rule).  Through P3D_ACCEL_NONE the count of every point equals samples minus the brute force over the CPU oracle's
per-object test on those rays, no case left out.  Through the BVH it equals the per-point sum of p3d_trace_any_device over
the written rays with the limit repeated per sample - on an uploaded tree, a device-built one and the deep tree of tri5k,
where the stack spills - for every team size; the bent normal lies within samples^2 * 2^-24 per component of the float64 sum
of the free written directions (samples - 1 float32 additions of partial sums no larger than samples) and repeats bit for
bit.  33 or 65 points, 1 to 70 samples."""
import ctypes as C

import numpy as np
import pytest
import torch

import device_query_contract as dq
from device_query_contract import BIG, CAPACITY, INVALID, UNSUPPORTED
from frame_checks import assert_bits, gpu
import intersect_reference as ref
from occlusion_checks import BEGIN, OFFSET, SEED, bent_bound, bent_from, choose_points, counts_from, drawn_limits, surface_points
import p3d_amd as p3d
from ray_query_checks import INF, N_MESH, World
import segment_reference as seg

pytestmark = pytest.mark.gpu

SAMPLES = 70
TEAMS = (1, 2, 4, 8, 16, 32, 64)
KW = dict(sample_begin=BEGIN, seed=SEED, point_offset=OFFSET)


class Case:
    """65 surface points of one World with their limits, on the host and the device"""

    def __init__(self, w, dev, limits_of, count=65):
        self.w, self.dev = w, dev
        p, nrm = surface_points(w, dev)
        assert len(p) >= count
        self.p, self.nrm, self.limits = p[:count], nrm[:count], limits_of(count)
        self.d_p, self.d_n, self.d_limits = gpu(self.p), gpu(self.nrm), gpu(self.limits)
        self._want = {}

    def want(self, n, samples, limited=True):
        """(counts, float64 bent, rays) of the first n points by trace_any_device over the written rays: computed once per shape"""
        key = (n, samples, limited)
        if key not in self._want:
            rays = p3d.occlusion_rays_device(self.dev, self.d_p[:n], self.d_n[:n], samples, **KW)
            # (no limit is a limit of +inf through the segment query; trace_any_device without t_max is the feeler with its restart)
            t_max = self.d_limits[:n].repeat_interleave(samples) if limited else torch.full((n * samples,), float("inf"), device="cuda")
            occ = self.dev.trace_any_device(p3d.ACCEL_BVH, rays["origin"], rays["direction"], t_max=t_max)["occluded"].cpu().numpy()
            self._want[key] = (counts_from(occ, samples), bent_from(occ, rays["direction"].cpu().numpy(), samples))
        return self._want[key]

    def ask(self, n, samples, accel=p3d.ACCEL_BVH, limited=True, want=("unoccluded", "bent"), **kw):
        opts = dict(KW, **kw)
        out = p3d.occlusion_device(self.dev, accel, self.d_p[:n], self.d_n[:n], samples, max_dist=self.d_limits[:n] if limited else None, want=want, **opts)
        return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    return World(ref.scene_paths(tmp_path_factory.mktemp("occlusion"))["mixed"], ("host", "device"))


@pytest.fixture(scope="module")
def cases(mixed, tri5k_path):
    mesh = World(tri5k_path, ("device",), seed=9, n=N_MESH, oracle=False)
    assert mesh.devs["device"].export_bvh()["bvh_max_depth"] > 16  # deeper than the stack's LDS window: the spill path runs
    return {"mixed, uploaded tree": Case(mixed, mixed.devs["host"], drawn_limits),
            "mixed, device-built tree": Case(mixed, mixed.devs["device"], drawn_limits),
            "tri5k, device-built tree": Case(mesh, mesh.devs["device"], lambda n: np.random.default_rng(22).uniform(0.05, 0.6, n).astype(np.float32))}


# ---- 1. the writer ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("samples", [1, 5, 64, 70])
@pytest.mark.parametrize("n", [1, 65])
def test_the_device_writer_is_the_host_writer(n, samples, cases):
    c = cases["mixed, uploaded tree"]
    got = p3d.occlusion_rays_device(c.dev, c.d_p[:n], c.d_n[:n], samples, bias=2e-4, **KW)
    o, d = p3d.occlusion_rays(c.p[:n], c.nrm[:n], samples, bias=2e-4, **KW)
    assert_bits(got["origin"].cpu().numpy(), o, "%d points, %d samples: origin" % (n, samples))
    assert_bits(got["direction"].cpu().numpy(), d, "%d points, %d samples: direction" % (n, samples))
    assert np.isfinite(d).all() and (d != d[0]).any() == (n * samples > 1)


# ---- 2. brute force against the oracle ----------------------------------------------------------------------------------------------

def test_brute_force_equals_the_oracle(mixed):
    w, dev, n = mixed, mixed.devs["host"], 33
    p, nrm, limits = choose_points(w, n, SAMPLES, drawn_limits)
    o, d = p3d.occlusion_rays(p, nrm, SAMPLES, **KW)
    tests = seg.per_object(w.sc.object_intercepts, len(w.objs), o, d)
    sets = {"NULL": None, "inf": np.full(n, INF), "draws": limits, "zero": np.zeros(n, np.float32), "NaN": np.full(n, np.nan, np.float32)}
    for what, lim in sets.items():
        per_ray = np.repeat(np.full(n, INF) if lim is None else lim, SAMPLES)
        want = counts_from(seg.brute_force(tests, per_ray), SAMPLES)
        got = p3d.occlusion_device(dev, p3d.ACCEL_NONE, gpu(p), gpu(nrm), SAMPLES, max_dist=None if lim is None else gpu(lim), **KW)["unoccluded"].cpu().numpy()
        print("limits %s: unoccluded %s" % (what, want.tolist()))
        assert got.dtype == np.int32 and (got == want).all(), "limits %s: points %s differ from the oracle's brute force" % (what, np.nonzero(got != want)[0].tolist())
        if what in ("zero", "NaN"):
            assert (want == SAMPLES).all()
        if what == "draws":
            assert ((want > 0) & (want < SAMPLES)).sum() >= 5, "too few points are partly occluded: the test shows nothing"
    assert dev.status() == 0


# ---- 3. through the BVH -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed, uploaded tree", "mixed, device-built tree", "tri5k, device-built tree"])
def test_through_the_bvh_equals_trace_any_over_the_written_rays(name, cases):
    c, n = cases[name], 65
    for limited in (True, False):
        counts, bent = c.want(n, SAMPLES, limited)
        got = c.ask(n, SAMPLES, limited=limited)
        what = "%s, %s" % (name, "limits" if limited else "no limit")
        print("%s: unoccluded %s" % (what, counts.tolist()))
        assert (got["unoccluded"] == counts).all(), "%s: points %s differ" % (what, np.nonzero(got["unoccluded"] != counts)[0].tolist())
        err = np.abs(got["bent"].astype(np.float64) - bent).max()
        print("%s: bent max |error| %.3g (bound %.3g)" % (what, err, bent_bound(SAMPLES)))
        assert err <= bent_bound(SAMPLES), what
        alone = c.ask(n, SAMPLES, limited=limited, want=())
        assert list(alone) == ["unoccluded"] and (alone["unoccluded"] == counts).all(), what + ": without d_bent"
        if limited:
            assert ((counts > 0) & (counts < SAMPLES)).sum() >= 5, what + ": too few points are partly occluded"
    assert c.dev.status() == 0


# ---- 4. team sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed, uploaded tree", "tri5k, device-built tree"])
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("samples", [5, 70])
def test_every_team_size_counts_the_same(samples, n, name, cases):
    c = cases[name]
    counts, bent = c.want(n, samples)
    for team in TEAMS + (0,):
        a, b = c.ask(n, samples, team=team), c.ask(n, samples, team=team)
        what = "%s, %d points, %d samples, team %d" % (name, n, samples, team)
        assert (a["unoccluded"] == counts).all() and (b["unoccluded"] == counts).all(), what
        assert_bits(a["bent"], b["bent"], what + ": bent of two runs")
        assert np.abs(a["bent"].astype(np.float64) - bent).max() <= bent_bound(samples), what
    assert c.dev.status() == 0


# ---- 5. progressive and split -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed, device-built tree", "tri5k, device-built tree"])
def test_progressive_samples_and_split_batches(name, cases):
    c, n = cases[name], 65
    counts, bent = c.want(n, SAMPLES)
    out = {"unoccluded": torch.full((n,), -9, dtype=torch.int32, device="cuda"), "bent": torch.full((n, 3), -9.0, device="cuda")}
    common = dict(max_dist=c.d_limits, seed=SEED, point_offset=OFFSET, want=("unoccluded", "bent"), out=out)
    p3d.occlusion_device(c.dev, p3d.ACCEL_BVH, c.d_p, c.d_n, 32, sample_begin=BEGIN, **common)
    back = p3d.occlusion_device(c.dev, p3d.ACCEL_BVH, c.d_p, c.d_n, SAMPLES - 32, sample_begin=BEGIN + 32, flags=p3d.OCCLUSION_ACCUMULATE, **common)
    assert back["unoccluded"] is out["unoccluded"] and (out["unoccluded"].cpu().numpy() == counts).all(), name + ": 32 + 38 samples"
    assert np.abs(out["bent"].cpu().numpy().astype(np.float64) - bent).max() <= bent_bound(SAMPLES), name + ": bent of 32 + 38 samples"
    for team in (8, 64):
        whole = c.ask(n, SAMPLES, team=team)
        for a, b in ((0, 1), (1, 40), (40, 65)):
            part = p3d.occlusion_device(c.dev, p3d.ACCEL_BVH, c.d_p[a:b], c.d_n[a:b], SAMPLES, max_dist=c.d_limits[a:b], sample_begin=BEGIN, seed=SEED,
                                        point_offset=OFFSET + a, team=team, want=("unoccluded", "bent"))
            assert (part["unoccluded"].cpu().numpy() == whole["unoccluded"][a:b]).all(), "%s: points %d..%d, team %d" % (name, a, b, team)
            assert_bits(part["bent"].cpu().numpy(), whole["bent"][a:b], "%s: bent of points %d..%d, team %d" % (name, a, b, team))
    assert c.dev.status() == 0


# ---- 6. a case a person can check ---------------------------------------------------------------------------------------------------

HEAD = ref.HEAD.replace("from 0 0 20", "from 0 6 20")
FLOOR = "box -5 -1 -5 5 0 5\n"
LID = "box -3 -0.5 2 3 3 2.5\nbox -3 -0.5 -2.5 3 3 -2\nbox 2 -0.5 -3 2.5 3 3\nbox -2.5 -0.5 -3 -2 3 3\nbox -3 2 -3 3 2.5 3\n"  # four walls 2 away and a ceiling at 2


def test_an_open_floor_and_a_closed_lid(tmp_path):
    """Two points on a floor, the normal straight up.  Open sky: every sample is free.  Inside a closed room: none is, without a
    limit; the nearest wall is 1.5 away from the second point and the ceiling 2 above both, so a limit of 1.25 frees them all."""
    point, up = gpu(np.array([[0, 0, 0], [0.5, 0, -0.5]], np.float32)), gpu(np.array([[0, 1, 0], [0, 1, 0]], np.float32))
    short = torch.full((2,), 1.25, device="cuda")
    for name, text, want in (("open", FLOOR + "s 40 -40 40 1\n", [64, 64]), ("closed", FLOOR + LID, [0, 0])):
        path = tmp_path / (name + ".p3f")
        path.write_text(HEAD + text)
        dev = p3d.DeviceScene(p3d.HostScene(str(path)), bvh="device")
        for accel in (p3d.ACCEL_BVH, p3d.ACCEL_NONE):
            got = p3d.occlusion_device(dev, accel, point, up, 64, seed=1)["unoccluded"].cpu().tolist()
            assert got == want, "%s, accel %d: %s" % (name, accel, got)
            assert p3d.occlusion_device(dev, accel, point, up, 64, max_dist=short, seed=1)["unoccluded"].cpu().tolist() == [64, 64], name
        assert dev.status() == 0


# ---- 7. streams ---------------------------------------------------------------------------------------------------------------------

def test_on_a_side_stream_and_behind_pose_device(tmp_path):
    """Points written by a torch kernel on a side stream with the query behind them on that stream; then a pose on the same
    stream carries the only occluder away, and the query behind it counts every sample free"""
    tris = np.array([[[-30000, 1, -30000], [30000, 1, -30000], [0, 1, 30000]], [[90, -9, -5], [91, -9, -5], [90, -8, -5]], [[-90, -9, -4], [-91, -9, -4], [-90, -8, -4]]], np.float32)
    path = tmp_path / "roof.p3f"
    path.write_text(HEAD + "".join("p 3\n" + "".join("%g %g %g\n" % tuple(v) for v in t) for t in tris))
    dev = p3d.DeviceScene(p3d.HostScene(str(path)), bvh="device")
    dev.set_rig([(0, 1, 0)], 1)
    n, samples = 65, 37
    base = gpu(np.random.default_rng(5).uniform(-0.2, 0.2, (n, 3)).astype(np.float32))
    up = gpu(np.tile(np.float32([0, 1, 0]), (n, 1)))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0

    def ask(pose=None):
        with torch.cuda.stream(side):
            wave = base
            for _ in range(200):  # some work in front of the points, so that they are still being produced when the call begins
                wave = torch.sin(wave * 1.5 + 0.25)
            pts = (base * torch.tensor([1.0, 0.0, 1.0], device="cuda") + 0.0 * wave).contiguous()
            if pose is not None:
                dev.pose_device(pose, stream=side)
            res = {accel: p3d.occlusion_device(dev, accel, pts, up, samples, seed=2, stream=side)["unoccluded"] for accel in (p3d.ACCEL_BVH, p3d.ACCEL_NONE)}
        side.synchronize()
        return {k: v.cpu().tolist() for k, v in res.items()}

    assert all(v == [0] * n for v in ask().values())
    below = gpu(np.float32([[1, 0, 0, 0, 0, 1, 0, -50, 0, 0, 1, 0]]))
    assert all(v == [samples] * n for v in ask(below).values())
    assert dev.status() == 0


# ---- 8. refusals on a device scene --------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(cases):
    c = cases["mixed, uploaded tree"]
    dev, n = c.dev, 33
    p, nrm = c.d_p[:n], c.d_n[:n]
    query = dq.occlusion(4, seed=1)
    out = dq.check_buffer_refusals(query, dev, {"d_point": p, "d_normal": nrm, "d_max_dist": c.d_limits[:n]}, n)
    rows = torch.full((n * 4, 3), 123.0, device="cuda")
    host = np.zeros((n, 3), np.float32)
    dq.assert_refused([
        ("the grid", UNSUPPORTED, "grid", lambda: query.call(dev, p3d.ACCEL_GRID, {"d_point": p, "d_normal": nrm}, query.optional, 0, out)),
        # the ray writer, which does not traverse: its own two
        ("rows too short", INVALID, "ends behind its allocation",
         lambda: p3d.occlusion_rays_device(dev, (p.data_ptr(), BIG), (nrm.data_ptr(), BIG), 4, out={"origin": (rows.data_ptr(), 4 * BIG), "direction": (rows.data_ptr(), 4 * BIG)})),
        ("host rows", INVALID, "host memory", lambda: p3d.occlusion_rays_device(dev, p, nrm, 4, out={"origin": (host.ctypes.data, 4 * n), "direction": rows})),
    ])
    L = p3d.lib()
    good = {"d_point": p, "d_normal": nrm, "d_unoccluded": out["unoccluded"], "d_bent": out["bent"]}
    for what, word, other, bufs in [("team = 3", "team", dq.occlusion(4, team=3), good), ("samples = 0", "samples", dq.occlusion(0), good),
                                    ("a flag bit", "unknown flag", dq.occlusion(4, flags=2), good), ("a NaN bias", "bias", dq.occlusion(4, bias=float("nan")), good),
                                    ("a misaligned count", "aligned", query, dict(good, d_unoccluded=out["unoccluded"].data_ptr() + 2))]:
        assert other.raw(dev, p3d.ACCEL_BVH, n, **bufs) == INVALID, what
        assert word in L.p3d_last_error().decode(), "%s: %s" % (what, L.p3d_last_error())
    del good["d_bent"]
    assert dq.occlusion(4, team=64).raw(dev, p3d.ACCEL_BVH, 0x10000000, **good) == CAPACITY
    wide = p3d.OcclusionParams(seed=1, samples=0x10000, sample_begin=0, point_offset=0, flags=0, bias=1e-4, team=0)
    assert L.p3d_occlusion_rays_device(dev._h, 0x10000, p.data_ptr(), nrm.data_ptr(), C.byref(wide), rows.data_ptr(), rows.data_ptr(), None) == CAPACITY
    dq.check_empty_batch(query, dev)
    dq.assert_untouched(dict(out, rows=rows))
    assert query.raw(dev, p3d.ACCEL_BVH, n, **good) == 0 and dev.status() == 0 and not bool((out["unoccluded"] == 77).any())

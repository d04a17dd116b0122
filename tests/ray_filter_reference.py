"""The yardstick of the filtered ray queries (include/p3d_filter.h: p3d_trace_any_filtered_device, p3d_trace_hits_filtered_device,
p3d_occlusion_filtered_device), stated differently from host/filter_rule.hpp and with no ray-object rule of its own:

    take the per-object (hit, t) tables of the UNFILTERED scene (segment_reference.per_object over the oracle's per-object test,
    or the float64 model's table), set the entries filter_reference.skipped names to "no hit", and hand the result to the
    existing brute forces and models: hits_reference.brute_hits / model_hits / all_hits_margin and
    segment_reference.brute_force / occluded_within.

A second, independent statement for filters that a whole batch shares: the scene WITHOUT the objects of a range, written out as
a file of its own (write_thinned), whose unfiltered answers with the indices mapped back (mapped_back) are the filtered ones.
Also here: the rays and the filters both suites use, so that what the CPU suite says about their margins is said about the rays
the GPU suite sends.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import numpy as np

import filter_reference as fr
import hits_reference as hr
import intersect_reference as ref
import segment_reference as seg

SEED = {"mixed": 610, "axis_aligned": 611, "mixed_planes": 612}  # the scenes of intersect_reference.scene_paths that are used
N_RAYS = 4099       # the largest batch of device_query_contract.BATCHES
RAY_SEED = 8        # ray_query_checks.World's: its rays are these (the GPU suite asserts it)
INF = np.float32(np.inf)


def scene_rays(objs, seed=RAY_SEED, n=N_RAYS):
    """The rays ray_query_checks.World attaches: intersect_reference.scene_rays, shuffled so that every prefix holds aimed and
    random rays -> float32 (o, d)"""
    o, d = ref.scene_rays(objs, seed, n)
    order = np.random.default_rng(seed + 100).permutation(len(o))
    return np.ascontiguousarray(o[order], np.float32), np.ascontiguousarray(d[order], np.float32)


class Case:
    """One scene without a device: the model's objects, the suite's rays, the model's table of them and seeded limits"""

    def __init__(self, path, seed, objs=None, rays=None):
        self.path, self.seed = path, seed
        self.objs = ref.load_objects(path) if objs is None else objs
        self.o, self.d = scene_rays(self.objs) if rays is None else rays
        self.n = len(self.o)
        self.table = ref._all(self.objs, self.o, self.d)
        self.limits = seg.draw_limits(self.objs, self.o, self.d, seed + 1, table=self.table)


def first_hits(table, width=fr.SKIP_MAX):
    """(n, width) the objects the model's unfiltered ray hits first, -1 behind them: what draw() aims three filters in four at"""
    return hr.model_hits(table, None, width)[1].astype(np.int32)


def draw(case, n_skip, ranged, n=None):
    """The filters of the first n rays of a case: filter_reference.draw round the unfiltered answers, seeded by the case"""
    n = case.n if n is None else n
    skip, skip_range = fr.draw(case.n, len(case.objs), n_skip, ranged, case.seed + 7 * n_skip + ranged, answers=first_hits(case.table))
    return (None if skip is None else np.ascontiguousarray(skip[:n])), (None if skip_range is None else np.ascontiguousarray(skip_range[:n]))


def mask_tests(tests, skip, skip_range):
    """per_object's (hit, t) with the named entries set to "no hit" (t is left: nothing reads the t of a miss)"""
    hit, t = tests
    return hit & ~fr.skipped(hit.shape[0], hit.shape[1], skip, skip_range), t


def mask_table(table, skip, skip_range):
    """intersect_reference._all's (hit, t, margin, cand) with the named entries set to a miss that no last bit can turn: no hit,
    t NaN, margin and t_cand infinite - a skipped object is not tested, so it decides nothing"""
    hit, t, margin, cand = table
    named = fr.skipped(hit.shape[0], hit.shape[1], skip, skip_range)
    return hit & ~named, np.where(named, np.nan, t), np.where(named, np.inf, margin), np.where(named, np.inf, cand)


def hits_margin(objs, o, d, t_max, masked):
    """hits_reference.all_hits_margin of the thinned table: the rays whose filtered hit list a last bit could change"""
    return hr.all_hits_margin(objs, o, d, t_max, masked)


def model_occluded(objs, o, d, t_max, masked):
    """segment_reference.occluded_within of the thinned table -> (occluded, margin)"""
    return seg.occluded_within(objs, o, d, t_max, table=masked)


# ---- the thinned scene as a scene of its own ---------------------------------------------------------------------------------------

def shared_ranges(n_objs):
    """A few (first, count) ranges for a whole batch: the head of the scene, a piece of its middle, and one that runs past its end"""
    return [(0, max(1, n_objs // 3)), (n_objs // 2, min(5, n_objs - n_objs // 2 - 1)), (n_objs - 2, 7)]


def kept(n_objs, first, count):
    """The objects a range leaves, ascending: index in the thinned scene -> index in the scene"""
    return np.array([j for j in range(n_objs) if not first <= j < first + count], np.int64)


def mapped_back(obj, keep):
    """Object indices of the thinned scene as the scene's; -1 stays"""
    obj = np.asarray(obj)
    return np.where(obj >= 0, keep[np.maximum(obj, 0)], -1).astype(obj.dtype)


def write_thinned(path, objs, keep):
    """The objects `keep` of the model's list as a .p3f file: the float32 values a loader read, written so that it reads them again"""
    line = lambda *vs: " ".join(repr(float(x)) for v in vs for x in np.asarray(v).reshape(-1))
    with open(str(path), "w") as f:
        f.write(ref.HEAD)
        for j in keep:
            ob = objs[int(j)]
            if ob["kind"] == ref.SPHERE:
                f.write("s %s\n" % line(ob["c"], ob["r"]))
            elif ob["kind"] == ref.TRIANGLE:
                f.write("p 3\n%s\n" % line(ob["p0"], ob["p1"], ob["p2"]))
            elif ob["kind"] == ref.BOX:
                f.write("box %s\n" % line(ob["mn"], ob["mx"]))
            else:
                f.write("pl %s\n" % line(ob["p0"], ob["p1"], ob["p2"]))
    return str(path)


# ---- the cube and a second body ------------------------------------------------------------------------------------------------------

CUBE_TRIANGLES = 12
BODY_CENTRE = np.array([5.0, 0.25, -0.5])  # the second closed body: a smaller cube well clear of the cube [-1, 1]^3
BODY_HALF = 0.75


def write_cube_and_body(path):
    """hits_reference's closed cube (objects 0 .. 11) and a second closed mesh next to it (objects 12 .. 23): total counts a
    triangle mesh's crossings (a sphere or a box would count once), so its parity says "inside" for each body"""
    hr.write_cube(path)
    tris = [[BODY_CENTRE + BODY_HALF * np.array(v, np.float64) for v in t] for q in hr._CUBE_QUADS for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])]
    with open(str(path), "a") as f:
        f.write(hr._triangles(tris))
    return str(path)


def body_rays(seed, n):
    """n rays with seeded unit directions from points strictly inside the second body, at least 10 % of its half-size from every
    face -> float32 (o, d)"""
    rng = np.random.default_rng(seed)
    o = (BODY_CENTRE + BODY_HALF * rng.uniform(-0.9, 0.9, (n, 3))).astype(np.float32)
    return o, ref.normalize32(ref._unit(rng, n).astype(np.float32))

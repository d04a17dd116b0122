"""What the hemisphere-occlusion tests share: surface points with normals on the scenes of ray_query_checks.World, the limits
drawn for them, and the yardsticks of a count and of a bent normal from the written rays.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import numpy as np

import intersect_reference as ref
import p3d_amd as p3d

SEED = 0x0CC1
BEGIN, OFFSET = 3, 7  # a sample_begin and a point_offset that are not zero


def surface_points(w, dev=None):
    """The closest hits of the World's rays that hit something, in ray order -> (points, normals) float32: the hit point, and
    object_normal there turned against the ray.  By the oracle's object loop on the CPU where the World has an oracle scene,
    otherwise by `dev`'s."""
    if w.sc is not None:
        hit, _, hp = w.sc.trace_closest(0, w.o, w.d)
        normal_of = w.sc.object_normal
    else:
        hit, hp = dev.trace_closest(p3d.ACCEL_NONE, w.o, w.d)
        normal_of = lambda j, p: dev.object_normal(j, p[None])[0]
    keep = np.nonzero(hit >= 0)[0]
    nrm = np.stack([normal_of(int(hit[k]), hp[k]) for k in keep]).astype(np.float32)
    against = (nrm * w.d[keep]).sum(1) > 0
    nrm[against] = -nrm[against]
    return np.ascontiguousarray(hp[keep]), np.ascontiguousarray(nrm)


def drawn_limits(n, seed=21):
    """One float32 limit per point, uniform in [0.3, 3]: the scenes are a few units across"""
    return np.random.default_rng(seed).uniform(0.3, 3.0, n).astype(np.float32)


def model_occluded(objs, origin, direction, limits, samples):
    """The float64 model's answer for the written rays -> (n, samples) bool (no margins: a choice of points, not a yardstick)"""
    hit, t = ref._all(objs, origin, direction)[:2]
    with np.errstate(invalid="ignore"):
        return (hit & (t < np.repeat(np.asarray(limits, np.float64), samples)[None, :])).any(0).reshape(-1, samples)


def choose_points(w, count, samples, limits_of, candidates=240):
    """`count` of the World's surface points, chosen on the CPU: those the float64 model sees partly occluded under their
    drawn limit come first (up to two thirds), the rest in ray order -> (points, normals, limits)"""
    p, nrm = surface_points(w)
    p, nrm = p[:candidates], nrm[:candidates]
    limits = limits_of(len(p))
    o, d = p3d.occlusion_rays(p, nrm, samples, sample_begin=BEGIN, seed=SEED, point_offset=0)
    free = (~model_occluded(w.objs, o, d, limits, samples)).sum(1)
    partly = np.nonzero((free > 0) & (free < samples))[0][: 2 * count // 3]
    rest = np.setdiff1d(np.arange(len(p)), partly)[: count - len(partly)]
    pick = np.sort(np.concatenate([partly, rest]))
    return np.ascontiguousarray(p[pick]), np.ascontiguousarray(nrm[pick]), np.ascontiguousarray(limits[pick])


def counts_from(occluded, samples):
    """unoccluded per point from the (n * samples,) answers of an any-hit over the written rays"""
    return samples - np.asarray(occluded, bool).reshape(-1, samples).sum(1)


def bent_from(occluded, direction, samples):
    """The float64 sum of the free written directions per point"""
    free = ~np.asarray(occluded, bool).reshape(-1, samples)
    return (np.asarray(direction, np.float64).reshape(-1, samples, 3) * free[:, :, None]).sum(1)


def bent_bound(samples):
    """samples - 1 float32 additions of partial sums no larger than samples"""
    return samples * samples * 2.0 ** -24

"""Shared by test_device_geometry_api.py and test_gpu_device_geometry.py: the indexed form of a triangle scene, and seeded
deformations whose float32 bits are the yardstick of both routes."""
import numpy as np


def indexed(prim_v):
    """(positions (V, 3) float32, indices (F, 3) int64) of the triangles prim_v (F, 9): np.unique over the vertices, so that
    positions[indices] returns prim_v bit for bit"""
    v = np.ascontiguousarray(prim_v, np.float32).reshape(-1, 3)
    bits = v.view(np.uint32)  # (-0 and +0 stay apart: the gather must return the input BITS)
    uniq, inverse = np.unique(bits, axis=0, return_inverse=True)
    return np.ascontiguousarray(uniq.view(np.float32)), inverse.reshape(-1, 3).astype(np.int64)


def smooth_field(positions, seed, reach):
    """`positions` (n, 3) displaced by a seeded sum of three sine waves per axis, |displacement| <= reach -> (n, 3) float32.
    Evaluated in float64 and rounded once."""
    rng = np.random.default_rng(seed)
    p = np.asarray(positions, np.float64)
    freq = rng.uniform(1.0, 4.0, (3, 3, 3))   # (wave, axis of the displacement, axis of the position)
    phase = rng.uniform(0, 2 * np.pi, (3, 3))
    d = sum(np.sin(p @ freq[w].T + phase[w]) for w in range(3)) / 3.0  # every component in [-1, 1]
    return (p + d * (reach / np.sqrt(3.0))).astype(np.float32)


def diagonal(arrays, objects=None):
    lo, hi = arrays["prim_bmin"], arrays["prim_bmax"]
    if objects is not None:
        lo, hi = lo[objects], hi[objects]
    return float(np.linalg.norm(hi.max(0).astype(np.float64) - lo.min(0).astype(np.float64)))


def deformed_mesh(arrays, seed, fraction=0.02):
    """The triangles of a scene of triangles only, every vertex displaced by at most `fraction` x the scene diagonal ->
    (positions, indices, soup): the deduplicated positions with their (F, 3) indices, and soup = positions[indices] (3F, 3):
    the same numbers in both forms"""
    pos, idx = indexed(arrays["prim_v"])
    pos = smooth_field(pos, seed, fraction * diagonal(arrays))
    return pos, idx, np.ascontiguousarray(pos[idx].reshape(-1, 3))


def moved_spheres(arrays, first, count, seed, reach=0.05):
    """(count, 4) float32: the spheres [first, first + count) with centres moved by at most reach x their diagonal and radii
    scaled by 0.8 .. 1.2"""
    rng = np.random.default_rng(seed)
    cr = np.array(arrays["prim_v"][first:first + count, :4], np.float32)
    d = rng.uniform(-1, 1, (count, 3)) * reach * diagonal(arrays, np.arange(first, first + count)) / np.sqrt(3.0)
    cr[:, :3] = (cr[:, :3].astype(np.float64) + d).astype(np.float32)
    cr[:, 3] = (cr[:, 3].astype(np.float64) * rng.uniform(0.8, 1.2, count)).astype(np.float32)
    return cr

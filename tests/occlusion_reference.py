"""The float64 statement of the rays of a hemisphere-occlusion query (host/occlusion_rule.hpp; p3d_occlusion_rays,
p3d_occlusion_rays_device and what p3d_occlusion_device casts): sample s of the point with stream index k draws r1 and r2 from
seed_stream(seed, k, s) - rng_reference.py's integers - and takes r1, r2, r2s = sqrt(r2) and sqrt(1 - r2) in numpy float32, as
the rule does; the tangent frame, the sine and cosine (libm's, in double) and the normalisation are float64.  The origin is
point + normal * bias in float32, the rule's own three operations.

A reference module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import math

import numpy as np

from rng_reference import next31, seed_stream

F = np.float32
TWO_PI_F = F(2) * F(3.141592653589793238462)  # 2 * kPIf: one float32 product


def draws(seed, index, sample):
    """(r1, r2, r2s, sqrt(1 - r2)) of one sample, float32"""
    state, inc = seed_stream(seed, index, sample)
    state, a = next31(state, inc)
    state, b = next31(state, inc)
    r1 = TWO_PI_F * (F(a) / F(2147483648.0))
    r2 = F(b) / F(2147483648.0)
    return r1, r2, np.sqrt(r2, dtype=F), np.sqrt(F(1) - r2, dtype=F)


def frame(normal):
    """(u, v, w) in float64 around the normal as given"""
    w = np.asarray(normal, np.float64)
    a = np.array([0.0, 1.0, 0.0]) if abs(w[0]) > 0.1 else np.array([1.0, 0.0, 0.0])
    u = np.cross(a, w)
    u = u / math.sqrt(u @ u)
    return u, np.cross(w, u), w


def directions(seed, index, normal, sample_begin, samples):
    """(samples, 3) float64: the directions of samples sample_begin .. sample_begin + samples - 1 of one point"""
    u, v, w = frame(normal)
    out = np.empty((samples, 3))
    for j in range(samples):
        r1, r2, r2s, cz = draws(seed, index, sample_begin + j)
        d = (u * math.cos(float(r1)) + v * math.sin(float(r1))) * float(r2s) + w * float(cz)
        out[j] = d / math.sqrt(d @ d)
    return out


def rays(points, normals, samples, sample_begin=0, seed=0, point_offset=0, bias=1e-4):
    """-> (origin float32 (n * samples, 3): point + normal * bias in float32; direction float64 (n * samples, 3)), row i * samples + j"""
    p, w = np.asarray(points, F), np.asarray(normals, F)
    origin = np.repeat(p + w * F(bias), samples, axis=0)
    direction = np.concatenate([directions(seed, point_offset + i, w[i], sample_begin, samples) for i in range(len(p))])
    return origin, direction

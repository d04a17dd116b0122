"""The RNG state arithmetic of csrc/device_core.hpp (Rng::seed_stream and the 31-bit draw) restated on Python integers.
tests/test_trace_path_api.py holds it to oracle.binding.rng_stream; tests/test_gpu_trace_path.py builds its states with it.

The *_v functions are the same arithmetic on numpy uint64 arrays, one stream per element (the float64 shading model draws a
whole frame's samples at once); tests/test_shading_reference.py holds them to the scalar functions.

A reference module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import numpy as np

M64 = (1 << 64) - 1
PCG_MUL = 6364136223846793005


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seed_stream(seed, pixel, sample):
    """-> (state, inc) of the stream of (pixel, sample), as csrc/device_core.hpp Rng::seed_stream"""
    k = mix64(seed ^ mix64((pixel << 32) | sample))
    inc = ((mix64(k) << 1) | 1) & M64
    return (k * PCG_MUL + inc) & M64, inc


def next31(state, inc):
    """-> (the state after the draw, the draw)"""
    xs, rot = (((state >> 18) ^ state) >> 27) & 0xffffffff, state >> 59
    return (state * PCG_MUL + inc) & M64, (((xs >> rot) | (xs << ((-rot) & 31))) & 0xffffffff) >> 1


# ---- the same, one stream per element: numpy uint64 arrays, whose arithmetic wraps at 2^64 as the C++ does -------------------------------

def _u64(x):
    return np.asarray(x).astype(np.uint64)


def mix64_v(z):
    z = _u64(z) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def seed_stream_v(seed, pixel, sample):
    """seed_stream for arrays of pixel and sample indices (broadcast against each other) -> (state, inc), uint64 arrays"""
    pixel, sample = np.broadcast_arrays(_u64(pixel), _u64(sample))
    k = mix64_v(np.uint64(seed & M64) ^ mix64_v((pixel << np.uint64(32)) | sample))
    inc = (mix64_v(k) << np.uint64(1)) | np.uint64(1)
    return k * np.uint64(PCG_MUL) + inc, inc


def next31_v(state, inc):
    """next31 for arrays of streams -> (the states after the draw, the draws as int64)"""
    xs = (((state >> np.uint64(18)) ^ state) >> np.uint64(27)) & np.uint64(0xffffffff)
    rot = state >> np.uint64(59)
    draw = (((xs >> rot) | (xs << ((np.uint64(32) - rot) & np.uint64(31)))) & np.uint64(0xffffffff)) >> np.uint64(1)
    return state * np.uint64(PCG_MUL) + inc, draw.astype(np.int64)

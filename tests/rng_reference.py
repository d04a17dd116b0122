"""The RNG state arithmetic of csrc/device_core.hpp (Rng::seed_stream and the 31-bit draw) restated on Python integers.
tests/test_trace_path_api.py holds it to oracle.binding.rng_stream; tests/test_gpu_trace_path.py builds its states with it.

A reference module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
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

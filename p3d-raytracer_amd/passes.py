"""The objects that work on frames of a DeviceScene: Accumulator, AdaptiveAccumulator, Denoiser, Temporal."""
import ctypes as C

import numpy as np

from ._abi import AdaptiveParams, Stats, _check, _Handle, _ptr, _stream, lib
from .config import denoise_params, temporal_params


def _frame_outputs(t, want_rgb8, stats, samples=None):
    """The outputs of a host-buffer frame call over tile `t` -> (the tuple the call returns: rgb, hit, [samples,] [rgb8,]
    Stats; the call's arguments for rgb, hit, rgb8 and stats).  `samples`: the sample-count plane of an adaptive pass, which
    the caller allocates and passes to the library itself."""
    rgb = np.zeros((t.h, t.w, 3), np.float32)
    hit = np.zeros((t.h, t.w), np.int32)
    rgb8 = np.zeros((t.h, t.w, 3), np.uint8) if want_rgb8 else None
    st = Stats()
    out = (rgb, hit) + (() if samples is None else (samples,)) + ((rgb8,) if want_rgb8 else ()) + (st,)
    return out, (rgb.ctypes.data, hit.ctypes.data, rgb8.ctypes.data if want_rgb8 else None, C.byref(st) if stats else None)


def _shape(a, shape, dtype, what, owner):
    """`a` as a contiguous array of `dtype`, or ValueError if its shape is not the one `owner` was made for"""
    a = np.ascontiguousarray(a, dtype)
    if a.shape != shape:
        raise ValueError("%s: shape %s, %s is for %s" % (what, a.shape, owner, shape))
    return a


class Accumulator(_Handle):
    """p3d_accum (include/p3d.h): one anti-aliased frame of a DeviceScene rendered in passes over its samples, the running
    sums kept on the device.  Every pass renders samples [samples_done, samples_done + n) of every pixel; rgb is the mean of
    the samples so far, hit_id the first sample's hit.  Close it (or let it go) before the scene."""
    _destroy = "p3d_accum_destroy"

    def __init__(self, scene, cfg, tile):
        self._L = scene._L
        self.scene = scene  # (keeps the scene alive while the accumulator is)
        self.cfg = cfg
        self.tile = tile
        self.total = int(cfg.spp_sqrt) ** 2
        h = C.c_void_p()
        _check(self._L.p3d_accum_create(scene._h, C.byref(cfg), C.byref(tile), C.byref(h)))
        self._h = h

    @property
    def samples_done(self):
        return int(self._L.p3d_accum_samples_done(self._h))

    def reset(self):
        """Back to 0 samples (also what lets an accumulator whose pass failed render again)."""
        _check(self._L.p3d_accum_reset(self._h))

    def render(self, n, want_rgb8=False, stats=True):
        """p3d_accum_render: the next n samples; returns numpy arrays, the same tuple as DeviceScene.render."""
        out, buffers = _frame_outputs(self.tile, want_rgb8, stats)
        _check(self._L.p3d_accum_render(self._h, int(n), *buffers))
        return out

    def render_device(self, n, d_rgb=0, d_hit=0, d_rgb8=0, stream=0, stats=None):
        """p3d_accum_render_device: raw HBM addresses and a hipStream_t (or a torch.cuda.Stream); without stats the pass
        is only enqueued - DeviceScene.status() reports what the device detected."""
        _check(self._L.p3d_accum_render_device(self._h, int(n), _ptr(d_rgb), _ptr(d_hit), _ptr(d_rgb8), _stream(stream),
                                               C.byref(stats) if stats is not None else None))


class AdaptiveAccumulator(_Handle):
    """p3d_adaptive (include/p3d.h): a progressive path-traced frame whose pixels stop taking samples once converged.
    Every pass renders samples [samples_done, samples_done + n) of the still-active pixels and writes every pixel: a
    pixel that stopped after k samples holds the bits a plain Accumulator holds after k.  Close it before the scene."""
    _destroy = "p3d_adaptive_destroy"

    def __init__(self, scene, cfg, tile, rel_error, min_samples=16, reserved=(0, 0)):
        self._L = scene._L
        self.scene = scene
        self.cfg = cfg
        self.tile = tile
        self.total = int(cfg.spp_sqrt) ** 2
        prm = AdaptiveParams(float(rel_error), int(min_samples), (C.c_uint32 * 2)(*reserved))
        h = C.c_void_p()
        _check(self._L.p3d_adaptive_create(scene._h, C.byref(cfg), C.byref(tile), C.byref(prm), C.byref(h)))
        self._h = h

    @property
    def samples_done(self):
        return int(self._L.p3d_adaptive_samples_done(self._h))

    @property
    def active_pixels(self):
        """Pixels the next pass renders (waits for the device)."""
        n = C.c_uint32()
        _check(self._L.p3d_adaptive_active_pixels(self._h, C.byref(n)))
        return int(n.value)

    def reset(self):
        """Back to 0 samples, every pixel active (also what lets an object whose pass failed render again)."""
        _check(self._L.p3d_adaptive_reset(self._h))

    def render(self, n, want_rgb8=False, stats=True):
        """p3d_adaptive_render: the next n samples of the active pixels -> (rgb, hit, samples, [rgb8,] stats)."""
        samples = np.zeros((self.tile.h, self.tile.w), np.uint32)
        out, (d_rgb, d_hit, d_rgb8, st) = _frame_outputs(self.tile, want_rgb8, stats, samples)
        _check(self._L.p3d_adaptive_render(self._h, int(n), d_rgb, d_hit, d_rgb8, samples.ctypes.data, st))
        return out

    def render_device(self, n, d_rgb=0, d_hit=0, d_rgb8=0, d_samples=0, stream=0, stats=None):
        """p3d_adaptive_render_device: raw HBM addresses and a hipStream_t (or a torch.cuda.Stream); without stats the
        pass is only enqueued - DeviceScene.status() reports what the device detected."""
        _check(self._L.p3d_adaptive_render_device(self._h, int(n), _ptr(d_rgb), _ptr(d_hit), _ptr(d_rgb8), _ptr(d_samples),
                                                  _stream(stream), C.byref(stats) if stats is not None else None))

    def read_state(self):
        """p3d_adaptive_read_state (waits for the device): {"sum": (h, w, 3) float32, "sum_y2": (h, w) float32,
        "samples": (h, w) uint32, "rel_err": (h, w) float32}."""
        t = self.tile
        out = {"sum": np.zeros((t.h, t.w, 3), np.float32), "sum_y2": np.zeros((t.h, t.w), np.float32),
               "samples": np.zeros((t.h, t.w), np.uint32), "rel_err": np.zeros((t.h, t.w), np.float32)}
        _check(self._L.p3d_adaptive_read_state(self._h, out["sum"].ctypes.data, out["sum_y2"].ctypes.data,
                                               out["samples"].ctypes.data, out["rel_err"].ctypes.data))
        return out

    def variance(self):
        """p3d_denoise_variance (waits for the device): per pixel the variance of its mean luminance, (h, w) float32 - the
        variance buffer of Denoiser.run; 0 where a pixel has fewer than 2 samples."""
        t = self.tile
        var = np.zeros((t.h, t.w), np.float32)
        _check(self._L.p3d_denoise_variance(self._h, var.ctypes.data))
        return var

    def variance_device(self, d_var, stream=0):
        """p3d_denoise_variance_device: the same into HBM (w*h float), enqueued on `stream` behind the pass."""
        _check(self._L.p3d_denoise_variance_device(self._h, _ptr(d_var), _stream(stream)))


class Denoiser(_Handle):
    """p3d_denoiser (include/p3d.h): the edge-avoiding a-trous filter for w x h images on one device.  Inputs are the
    linear rgb of a frame, its feature buffers (DeviceScene.render_features) and optionally a variance buffer
    (AdaptiveAccumulator.variance); the device form neither allocates nor waits."""
    _destroy = "p3d_denoiser_destroy"

    def __init__(self, device, w, h):
        self._L = lib()
        self.w, self.h = int(w), int(h)
        hd = C.c_void_p()
        _check(self._L.p3d_denoiser_create(int(device), self.w, self.h, C.byref(hd)))
        self._h = hd

    def run(self, rgb, normal_depth, albedo_cov, variance=None, params=None, want_rgb8=False):
        """p3d_denoise: -> rgb (h, w, 3) float32, and with want_rgb8 (rgb, rgb8)."""
        h, w = self.h, self.w
        rgb = _shape(rgb, (h, w, 3), np.float32, "rgb", "the denoiser")
        nd = _shape(normal_depth, (h, w, 4), np.float32, "normal_depth", "the denoiser")
        ac = _shape(albedo_cov, (h, w, 4), np.float32, "albedo_cov", "the denoiser")
        var = None if variance is None else _shape(variance, (h, w), np.float32, "variance", "the denoiser")
        prm = params if params is not None else denoise_params()
        out = np.zeros((h, w, 3), np.float32)
        out8 = np.zeros((h, w, 3), np.uint8) if want_rgb8 else None
        _check(self._L.p3d_denoise(self._h, C.byref(prm), rgb.ctypes.data, var.ctypes.data if var is not None else None,
                                   nd.ctypes.data, ac.ctypes.data, out.ctypes.data, out8.ctypes.data if want_rgb8 else None))
        return (out, out8) if want_rgb8 else out

    def run_device(self, d_rgb, d_normal_depth, d_albedo_cov, d_out_rgb=0, d_out_rgb8=0, d_var=0, params=None, stream=0):
        """p3d_denoise_device: raw HBM addresses and a hipStream_t (or a torch.cuda.Stream); enqueued, not waited for."""
        prm = params if params is not None else denoise_params()
        _check(self._L.p3d_denoise_device(self._h, C.byref(prm), _ptr(d_rgb), _ptr(d_var), _ptr(d_normal_depth), _ptr(d_albedo_cov),
                                          _ptr(d_out_rgb), _ptr(d_out_rgb8), _stream(stream)))


class Temporal(_Handle):
    """p3d_temporal (include/p3d.h): temporal accumulation of w x h frames on one device - every frame's colour blended with
    the previous frames' history reprojected into its view, plus a luminance variance for Denoiser.run.  Inputs per frame:
    the Camera the frame was rendered with (DeviceScene.camera), its linear rgb and its feature buffers
    (DeviceScene.render_features).  The device form neither allocates nor waits."""
    _destroy = "p3d_temporal_destroy"

    def __init__(self, device, w, h):
        self._L = lib()
        self.w, self.h = int(w), int(h)
        hd = C.c_void_p()
        _check(self._L.p3d_temporal_create(int(device), self.w, self.h, C.byref(hd)))
        self._h = hd

    @property
    def frames(self):
        """Frames accumulated since create / reset."""
        return int(self._L.p3d_temporal_frames(self._h))

    def reset(self):
        """Forget the history: the next frame starts it again."""
        _check(self._L.p3d_temporal_reset(self._h))

    def run(self, camera, rgb, normal_depth, albedo_cov, params=None):
        """p3d_temporal_accumulate -> (rgb (h, w, 3), var (h, w), history (h, w)), float32."""
        h, w = self.h, self.w
        rgb = _shape(rgb, (h, w, 3), np.float32, "rgb", "the object")
        nd = _shape(normal_depth, (h, w, 4), np.float32, "normal_depth", "the object")
        ac = _shape(albedo_cov, (h, w, 4), np.float32, "albedo_cov", "the object")
        prm = params if params is not None else temporal_params()
        out = np.zeros((h, w, 3), np.float32)
        var = np.zeros((h, w), np.float32)
        hist = np.zeros((h, w), np.float32)
        _check(self._L.p3d_temporal_accumulate(self._h, C.byref(prm), C.byref(camera), rgb.ctypes.data, nd.ctypes.data,
                                               ac.ctypes.data, out.ctypes.data, var.ctypes.data, hist.ctypes.data))
        return out, var, hist

    def run_device(self, camera, d_rgb, d_normal_depth, d_albedo_cov, d_out_rgb, d_out_var=0, d_out_history=0, params=None,
                   stream=0):
        """p3d_temporal_accumulate_device: raw HBM addresses and a hipStream_t (or a torch.cuda.Stream); enqueued, not waited
        for."""
        prm = params if params is not None else temporal_params()
        _check(self._L.p3d_temporal_accumulate_device(self._h, C.byref(prm), C.byref(camera), _ptr(d_rgb), _ptr(d_normal_depth),
                                                      _ptr(d_albedo_cov), _ptr(d_out_rgb), _ptr(d_out_var), _ptr(d_out_history),
                                                      _stream(stream)))

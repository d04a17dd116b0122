"""Configurations, filter parameters and cameras: the library's defaults, then the fields given."""
import ctypes as C

from ._abi import ACCEL_BVH, PATHTRACE, WHITTED, Camera, Config, DenoiseParams, TemporalParams, _check, lib

def default_config(**kw):
    c = Config()
    lib().p3d_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def denoise_params(**kw):
    """p3d_denoise_params_default, then the fields given (iterations, sigma_color, sigma_luma, sigma_normal, sigma_depth,
    sigma_albedo, gamma, reserved)."""
    p = DenoiseParams()
    lib().p3d_denoise_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_uint32 * 2)(*v) if k == "reserved" else v)
    return p


def temporal_params(**kw):
    """p3d_temporal_params_default, then the fields given (alpha, alpha_moments, max_history, depth_tolerance,
    normal_tolerance, variance_min_history, sigma_normal, sigma_depth, reserved)."""
    p = TemporalParams()
    lib().p3d_temporal_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_uint32 * 2)(*v) if k == "reserved" else v)
    return p


def _f3(v):
    v = [float(x) for x in v]
    if len(v) != 3:
        raise ValueError("a 3-vector is needed, got %r" % (v,))
    return (C.c_float * 3)(*v)


def look_at(from_, at, up, angle, res, aperture_ratio=0.0, focal_ratio=1.0):
    """p3d_camera_look_at: the Camera the .p3f loader builds for a `v` block with these values (camera.h:34-63);
    res = (res_x, res_y)."""
    cam = Camera()
    _check(lib().p3d_camera_look_at(_f3(from_), _f3(at), _f3(up), float(angle), int(res[0]), int(res[1]), float(aperture_ratio),
                                    float(focal_ratio), C.byref(cam)))
    return cam


def whitted_config(accel=ACCEL_BVH, max_depth=4, **kw):
    """SURVEY.md §8(d) Whitted configs: no AA / soft shadows / DOF, one ray per pixel."""
    base = dict(integrator=WHITTED, accel=accel, max_depth=max_depth, spp_sqrt=1, antialiasing=0,
                depth_of_field=0, soft_shadows=0)
    base.update(kw)
    return default_config(**base)


def pathtrace_config(accel=ACCEL_BVH, spp_sqrt=16, max_depth=20, dof=0, **kw):
    base = dict(integrator=PATHTRACE, accel=accel, max_depth=max_depth, spp_sqrt=spp_sqrt, antialiasing=1,
                depth_of_field=dof, sample_disk=1, soft_shadows=0)
    base.update(kw)
    return default_config(**base)

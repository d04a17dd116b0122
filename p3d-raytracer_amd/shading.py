"""The lights and materials of a live scene (include/p3d_shading.h): set from host arrays, read back, set from device tensors
on the caller's stream, and the same on a HostScene.  Functions of a DeviceScene or a HostScene, not members: the recorded
surface (tests/python_api_surface.json) holds both classes to their members of then.

Host arrays are float32 (n, 16) materials and (n, 8) lights, the layouts of p3d_material and p3d_light - what
HostScene.arrays()["materials"] holds, so it can be passed back unchanged - and (n, 6) lights, position then colour, as
arrays()["lights"] holds them."""
import numpy as np

from ._abi import P3DError, _check, _ptr, _stream
from ._device_args import _device_rows

MATERIAL_FLOATS, LIGHT_FLOATS = 16, 8  # sizeof(p3d_material) / 4, sizeof(p3d_light) / 4


def _material_rows(who, materials):
    """float32 (n, 16) rows of p3d_material, or P3DError"""
    m = np.ascontiguousarray(materials, np.float32)
    if m.ndim != 2 or m.shape[1] != MATERIAL_FLOATS:
        raise P3DError(-1, "%s: materials of shape %r, needed: (n, %d)" % (who, m.shape, MATERIAL_FLOATS))
    return m


def _light_rows(who, lights):
    """float32 (n, 8) rows of p3d_light from (n, 8) rows, or from (n, 6) rows of position then colour; or P3DError"""
    l = np.ascontiguousarray(lights, np.float32)
    if l.ndim == 2 and l.shape[1] == 6:
        full = np.zeros((len(l), LIGHT_FLOATS), np.float32)
        full[:, 0:3], full[:, 4:7] = l[:, 0:3], l[:, 3:6]
        return full
    if l.ndim != 2 or l.shape[1] != LIGHT_FLOATS:
        raise P3DError(-1, "%s: lights of shape %r, needed: (n, %d) or (n, 6)" % (who, l.shape, LIGHT_FLOATS))
    return l


def _first(who, first):
    first = int(first)
    if not 0 <= first < 1 << 32:
        raise P3DError(-1, "%s: first must be 0 .. 2^32 - 1, got %d" % (who, first))
    return first


def set_materials(scene, first, materials):
    """p3d_scene_set_materials: the (n, 16) rows replace materials first .. first + n - 1 of the DeviceScene `scene`.  Waits for
    the device.  Every fact the library derives from the records follows: the emitter list of the path tracer, the kernels of
    STACK_LITERAL frames, the Ks == 0 shortcut.  Accumulators of the scene refuse further passes until they are reset."""
    who = "set_materials"
    m = _material_rows(who, materials)
    _check(scene._L.p3d_scene_set_materials(scene._h, _first(who, first), len(m), m.ctypes.data if len(m) else None))


def set_lights(scene, first, lights):
    """p3d_scene_set_lights: the (n, 8) or (n, 6) rows replace lights first .. first + n - 1 of the DeviceScene `scene`.  Waits
    for the device.  A light is switched off by colour 0."""
    who = "set_lights"
    l = _light_rows(who, lights)
    _check(scene._L.p3d_scene_set_lights(scene._h, _first(who, first), len(l), l.ctypes.data if len(l) else None))


def _count(scene, entry):
    """How many records the scene has, from the library itself (the host scene a DeviceScene was made of may have changed
    since): an empty range is accepted exactly up to first == count, and answered without a wait"""
    lo, hi = 0, 1 << 32  # accepted at lo, refused at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if getattr(scene._L, entry)(scene._h, mid, 0, None) == 0:
            lo = mid
        else:
            hi = mid
    return lo


def _read(scene, who, entry, cols, first, n):
    first = _first(who, first)
    n = max(_count(scene, entry) - first, 0) if n is None else int(n)
    if n < 0:
        raise P3DError(-1, "%s: n must not be negative, got %d" % (who, n))
    out = np.zeros((n, cols), np.float32)
    _check(getattr(scene._L, entry)(scene._h, first, n, out.ctypes.data if n else None))
    return out


def scene_materials(scene, first=0, n=None):
    """p3d_scene_materials: materials first .. first + n - 1 (n None: to the last) as the device holds them -> float32 (n, 16).
    Waits for the device."""
    return _read(scene, "scene_materials", "p3d_scene_materials", MATERIAL_FLOATS, first, n)


def scene_lights(scene, first=0, n=None):
    """p3d_scene_lights: lights first .. first + n - 1 (n None: to the last) as the device holds them -> float32 (n, 8)"""
    return _read(scene, "scene_lights", "p3d_scene_lights", LIGHT_FLOATS, first, n)


def set_shading_device(scene, materials=None, first_material=0, lights=None, first_light=0, stream=0):
    """p3d_scene_set_shading_device: float32 (n, 16) materials and / or (n, 8) lights held in device memory (CUDA/HIP torch
    tensors, or raw (address, rows) pairs) replace the records from first_material / first_light on, by one kernel enqueued on
    `stream` without a wait: what is enqueued behind it on that stream sees them.  A material that would start or stop
    emitting, or start or stop being transmissive and reflective, keeps its record; scene.status() reports the counts
    (set_materials makes such a change).  Neither given: nothing is done."""
    who = "set_shading_device"
    d_m, n_m = _device_rows(materials, who + ": materials", MATERIAL_FLOATS, ("float32",), scene.device) if materials is not None else (None, 0)
    d_l, n_l = _device_rows(lights, who + ": lights", LIGHT_FLOATS, ("float32",), scene.device) if lights is not None else (None, 0)
    _check(scene._L.p3d_scene_set_shading_device(scene._h, _first(who, first_material), n_m, _ptr(d_m), _first(who, first_light), n_l, _ptr(d_l),
                                                 _stream(stream)))


def host_set_materials(hs, first, materials):
    """p3d_host_scene_set_materials: the same rows into the HostScene `hs`: a DeviceScene made of it afterwards is the twin of
    one given them through set_materials.  A host BVH and grid already built stay."""
    who = "host_set_materials"
    m = _material_rows(who, materials)
    _check(hs._L.p3d_host_scene_set_materials(hs._h, _first(who, first), len(m), m.ctypes.data if len(m) else None))


def host_set_lights(hs, first, lights):
    """p3d_host_scene_set_lights: the same for lights; after replicate_lights the indices are those of the replicated list"""
    who = "host_set_lights"
    l = _light_rows(who, lights)
    _check(hs._L.p3d_host_scene_set_lights(hs._h, _first(who, first), len(l), l.ctypes.data if len(l) else None))

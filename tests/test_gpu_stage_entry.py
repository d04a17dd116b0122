"""The LDS staging copy at the head of every render kernel (csrc/kernels.hpp: stage_issue / stage_scene).

A wave copies the staged range in batches of kStageBatch = 4 float4 per lane (256 float4 per wave): the loads of a batch
are all issued before its first LDS store, a load past the range reads the range's last float4 and is not stored.  What can
go wrong is a float4 that is not copied, copied to the wrong place or copied from past the range - any of which changes the
scene the frame is rendered from.  So: small frames (a handful of tiles, one wave each, every wave stages for itself) over
generated sphere scenes whose staged range has exactly the sizes at which the copy takes another path, each compared with
the oracle as tests/test_gpu_parity.py does (literal: hit IDs and every colour bit; per-pixel: bit-identical up to libm
pow, every counter equal).

Sizes of the range (float4), from the layout rules of capi_scene_layout.hpp / capi_frame_plan.hpp - a Whitted frame over the
BVH stages  2 * nodes + 3 * prims (BVH order) + prims (normals) + 4 * materials + 2 * lights,  the object loop
(ACCEL_NONE) 3 * prims (object order) more; node counts are odd, so a BVH frame's range is always EVEN and "one over a
multiple" can only be had exactly from an object-loop frame:
     24   under 64: lanes 24..63 copy nothing, three of the four loads of every lane are clamped
    144   not a multiple of 64: the third load is stored by 16 lanes only
    256   one whole batch, the loop behind it makes no trip
    257   (ACCEL_NONE) one over: the loop's single trip stores one float4
    258   (BVH) the least a BVH frame can be over
    512   two whole batches: the loop ends exactly at the range's end
    513   (ACCEL_NONE) / 514 (BVH) over that
   1664   26 KB, the largest range that is still staged (six batches and a half); one sphere more is not staged
The primitive, material and light counts below were picked on the CPU (HostScene descriptor -> the sum above); every test
asserts that the plan stages exactly that many float4.
"""
import pytest

from frame_checks import _pair, check_whitted
import p3d_amd as p3d
from variant_scenes import write_spheres

pytestmark = pytest.mark.gpu

LIMIT_F4 = 26 * 1024 // 16  # kLdsSceneLimitBytes (capi_frame_plan.hpp)
FRAMES = ((64, 64), (72, 40))


def layout_f4(path, accel):
    """The staged range by the layout rules, from the host-side descriptor alone."""
    d = p3d.HostScene(path).desc(bvh=True)
    d = d.contents if hasattr(d, "contents") else d
    bvh_frame = 2 * d.n_bvh_nodes + 3 * d.n_bvh_prim_index + d.n_prims + 4 * d.n_materials + 2 * d.n_lights
    return bvh_frame + (3 * d.n_prims if accel != p3d.ACCEL_BVH else 0)


#                  staged float4, accel, spheres, materials, lights
CASES = [(24, p3d.ACCEL_BVH, 3, 1, 1), (144, p3d.ACCEL_BVH, 18, 7, 1), (256, p3d.ACCEL_BVH, 37, 8, 1),
         (257, p3d.ACCEL_NONE, 27, 1, 1), (258, p3d.ACCEL_BVH, 37, 8, 2), (512, p3d.ACCEL_BVH, 74, 9, 1),
         (513, p3d.ACCEL_NONE, 53, 7, 2), (514, p3d.ACCEL_BVH, 74, 9, 2), (LIMIT_F4, p3d.ACCEL_BVH, 265, 9, 1)]


@pytest.mark.parametrize("want,accel,n,mats,lights", CASES, ids=["f4_%d" % c[0] for c in CASES])
def test_frames_over_a_staged_range_of_every_critical_size(want, accel, n, mats, lights, tmp_path):
    path = write_spheres(str(tmp_path / "spheres.p3f"), n, mats, lights)
    assert layout_f4(path, accel) == want
    for res in FRAMES:
        dev, sc = _pair(path, res=res, grid=False)
        cfg = p3d.whitted_config(accel=accel, max_depth=3)
        assert dev.staged_f4(cfg) == want  # the plan stages this scene, and exactly the range the layout rules give
        if accel == p3d.ACCEL_BVH:
            assert dev.staged_f4(p3d.whitted_config(accel=accel, max_depth=3, stack_mode=p3d.STACK_PER_PIXEL)) == want
        _, _, st = check_whitted(dev, sc, cfg)  # BVH: the literal frame, the kernels without counters, the per-pixel frame
        assert st.rays_primary == res[0] * res[1] and st.shaded_hits > 0  # (the camera looks at the lattice's centre: some ray hits)
        assert dev.status() == 0


def test_the_largest_staged_range_is_the_limit(tmp_path):
    """One sphere more than the 1664-float4 scene: over 26 KB, traversed from global memory (nothing staged)."""
    path = write_spheres(str(tmp_path / "spheres.p3f"), 266, 9, 1)
    assert layout_f4(path, p3d.ACCEL_BVH) == LIMIT_F4 + 4
    dev, sc = _pair(path, res=FRAMES[0], grid=False)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=3)
    assert dev.staged_f4(cfg) == 0
    check_whitted(dev, sc, cfg)

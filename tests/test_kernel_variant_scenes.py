"""The scenes of tests/test_gpu_kernel_variants.py without a GPU: the layout rule of csrc/capi_scene_layout.hpp on the host-side
descriptors puts each scene on the side of the 16 / 20 / 26 KB limits of plan_frame its cases claim, and the generated
sphere scene has the transmissive and reflective material its GHOSTS cases need."""
import p3d_amd as p3d
from variant_scenes import ACCEL_VALUES, scene_files, staged_bytes  # noqa: F401 (scene_files is a fixture)


def test_scene_sizes_are_what_the_cases_need(scene_files):
    size = lambda name, accel: staged_bytes(scene_files[name][0], accel, legacy=scene_files[name][1])
    assert size("pt_l2", p3d.ACCEL_NONE) > 16 * 1024  # (the path tracer stages the object-order geometry on every accel)
    assert size("path_glass", p3d.ACCEL_NONE) <= 16 * 1024
    # staged, and scene + one stack entry per lane over 20 KB: the spilling stack whatever the stack bound
    assert 20 * 1024 < size("spill_spheres", p3d.ACCEL_NONE) <= 26 * 1024 and size("spill_spheres", p3d.ACCEL_BVH) <= 20 * 1024
    assert size("balls_medium", p3d.ACCEL_BVH) <= 20 * 1024 and size("balls_medium", p3d.ACCEL_NONE) <= 19 * 1024
    assert size("balls_low", p3d.ACCEL_NONE) <= 19 * 1024
    for accel in ACCEL_VALUES:
        assert size("l2_ghosts", accel) > 26 * 1024 and size("tri5k", accel) > 26 * 1024


def test_stack_bounds_and_materials(scene_files):
    """(lights + 1) * (tree depth - 1) > 24 makes a staged Whitted BVH frame spill; a material with transmittance != 0 and
    reflection > 0 is what gives a scene zero-weight reflection rays."""
    for name, ghosts in (("balls_medium", False), ("spill_spheres", True), ("l2_ghosts", True)):
        hs = p3d.HostScene(scene_files[name][0], legacy_f11=scene_files[name][1])
        d = hs.desc(bvh=True)
        assert (d.n_lights + 1) * (d.bvh_max_depth - 1) > 24, name
        m = hs.arrays()["materials"]
        assert bool(((m[:, 9] != 0) & (m[:, 11] > 0)).any()) == ghosts, name

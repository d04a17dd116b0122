"""Every kernel that writes the u8 image (the Whitted megakernel, the fold of the per-level launches, the path tracer, the
adaptive resolve, the denoiser's last pass) ends with the same step: colour -> gamma -> u8.  The same floats must give the
same bytes whichever of them wrote the frame; test_rgb8_and_gamma anchors one of them to the oracle."""

import numpy as np
import pytest

from conftest import scene_path
from frame_checks import CORNELL, device_scene
import p3d_amd as p3d

pytestmark = pytest.mark.gpu

W, H, GAMMA = 64, 48, 2.2


def whitted(dev, **kw):
    rgb, _, rgb8, _ = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=2, gamma=GAMMA, **kw), want_rgb8=True)
    return rgb, rgb8


def pathtraced(dev, spp):
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=spp, max_depth=20, dof=0, seed=0x5EED, gamma=GAMMA)
    rgb, _, rgb8, _ = dev.render(cfg, want_rgb8=True)
    return rgb, rgb8


def adaptive(dev, spp):
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=spp, max_depth=20, dof=0, seed=0x5EED, gamma=GAMMA)
    ad = dev.adaptive(cfg, 0.0, min_samples=2)
    try:
        for n in (8, 8):
            rgb, _, _, rgb8, _ = ad.render(n, want_rgb8=True)
        assert ad.samples_done == spp * spp  # the last pass
    finally:
        ad.close()
    return rgb, rgb8


WRITERS = {
    "megakernel": lambda tri5k: whitted(device_scene(scene_path("balls_low.p3f"), (W, H), grid=False)),
    "megakernel_aa": lambda tri5k: whitted(device_scene(scene_path("balls_low.p3f"), (W, H), grid=False), antialiasing=1, spp_sqrt=2),
    "per_level_fold": lambda tri5k: whitted(device_scene(tri5k, (W, H), grid=False), chain_launch=p3d.CHAIN_PER_LEVEL),
    "path_tracer_one_lane": lambda tri5k: pathtraced(device_scene(CORNELL, (W, H), grid=False), 2),
    "path_tracer_four_lanes": lambda tri5k: pathtraced(device_scene(CORNELL, (W, H), grid=False), 4),
    "adaptive_resolve": lambda tri5k: adaptive(device_scene(CORNELL, (W, H), grid=False), 4),
}


@pytest.mark.parametrize("writer", list(WRITERS))
def test_every_writer_gives_the_bytes_the_denoiser_gives_for_the_same_floats(writer, tri5k_path):
    rgb, rgb8 = WRITERS[writer](tri5k_path)
    assert rgb.shape == (H, W, 3) and rgb8.shape == (H, W, 3) and rgb8.dtype == np.uint8
    assert rgb8.max() > rgb8.min()  # a picture, not a constant frame
    zeros = np.zeros((H, W, 4), np.float32)
    dn = p3d.Denoiser(0, W, H)
    try:
        out, out8 = dn.run(rgb, zeros, zeros, params=p3d.denoise_params(iterations=0, gamma=GAMMA), want_rgb8=True)
    finally:
        dn.close()
    assert np.array_equal(out.view(np.uint32), rgb.view(np.uint32))
    assert np.array_equal(out8, rgb8)

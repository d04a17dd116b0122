#!/usr/bin/env python3
"""What a wave of whitted_kernel spends before its first ray (profiles/entry/README.md).

  make -C p3d-raytracer_amd variant NAME=entry EXTRA=-DP3D_ENTRY_CLOCK
  P3D_LIB=$PWD/build/variants/libp3d_entry.so python profiles/tools/entry_clock.py \\
      tests/golden/scenes/balls_low.p3f 1024 4 [literal|per_pixel]

Every workgroup of the instrumented library stores two wall_clock64() differences (100 MHz): from its first
instruction to the point behind scene staging - or to the exit most waves of round 0 take - and to its end.  Prints,
for pass 1 (or the per-pixel launch) and for round 0 of the hand-off: waves, median / mean entry time, summed entry time
as a share of summed residency; round 0 separately for the waves that leave and the waves that stay."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import p3d_amd as p3d  # noqa: E402

scene, res, depth = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
mode = sys.argv[4] if len(sys.argv) > 4 else "literal"
hs = p3d.HostScene(scene)
hs.set_resolution(res, res)
dev = p3d.DeviceScene(hs, bvh=True)
cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=depth,
                         stack_mode=p3d.STACK_LITERAL if mode == "literal" else p3d.STACK_PER_PIXEL)
half = ((res + 7) // 8) ** 2 + (res * 16 + 63) // 64 + 64  # tiles + halo workgroups, rounded up generously
clock = torch.zeros(3 * 2 * half, dtype=torch.int64, device="cuda")
if not hasattr(dev._L, "p3d_debug_set_entry_clock"):
    sys.exit("P3D_LIB must point at a library built with -DP3D_ENTRY_CLOCK (make variant)")
assert dev._L.p3d_debug_set_entry_clock(C.c_void_p(clock.data_ptr()), C.c_uint32(half)) == 0
rgb = torch.empty(res * res * 3, dtype=torch.float32, device="cuda")
tile = dev.full_tile()
print("%s %dx%d depth %d %s" % (os.path.basename(scene), res, res, depth, mode))
for frame in range(5):  # the first launch records the tile costs, the later ones are scheduled: the last frame is reported
    clock.zero_()
    torch.cuda.synchronize()
    dev.render_device(cfg, tile, rgb.data_ptr())
    dev.join(host_wait=True)
    torch.cuda.synchronize()
t = clock.cpu().numpy().reshape(2, half, 3)


def report(name, rows):
    rows = rows[rows[:, 2] != 0]
    if not len(rows):
        return
    entry, total = rows[:, 0] * 0.01, rows[:, 1] * 0.01  # us
    print("%-28s %6d waves: entry median %.2f mean %.2f p90 %.2f us; residency median %.2f mean %.2f us; entry share of summed residency %.3f"
          % (name, len(rows), np.median(entry), entry.mean(), np.percentile(entry, 90), np.median(total), total.mean(),
             entry.sum() / total.sum()))


report("pass 1" if mode == "literal" else "per-pixel launch", t[0])
r0 = t[1]
report("round 0, all waves", r0)
report("round 0, leave at the ballot", r0[r0[:, 2] == 1])
report("round 0, stay", r0[r0[:, 2] == 2])
if (r0[:, 2] != 0).any():
    left = r0[r0[:, 2] == 1]
    print("round 0: waves that leave hold %.3f of the launch's summed residency" % (left[:, 1].sum() / r0[r0[:, 2] != 0][:, 1].sum()))

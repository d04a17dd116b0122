#!/usr/bin/env python3
"""The interpreter's cost of a call through the Python package: the host clock around back-to-back device-buffer calls.

    P3D_LIB=<one built libp3d.so> python profiles/python_package/call_clock.py <root of the tree whose package is measured>

balls_low at 64x64, Whitted depth 4 over the BVH.  Rows: 3 000 render_device calls without stats on one stream (literal and
per-pixel stacks), and 3 000 trace_closest_device calls with 64 rays into preallocated outputs (_device_query, the longest
Python path of a call); one synchronise behind each loop; microseconds per call, five loops per row.  Prints one JSON line.
Run it once per process, the packages to compare alternately, with the same P3D_LIB, so that only the Python differs."""
import json
import os
import statistics
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch  # noqa: E402
import p3d_amd as p3d  # noqa: E402

CALLS, LOOPS = 3000, 5
assert os.path.dirname(os.path.abspath(p3d.__file__)) == root
torch.cuda.init()
hs = p3d.HostScene(os.path.join(root, "tests", "golden", "scenes", "balls_low.p3f"))
hs.set_resolution(64, 64)
dev = p3d.DeviceScene(hs, bvh=True)
tile = dev.full_tile()
rgb = torch.empty(64 * 64 * 3, dtype=torch.float32, device="cuda")
hit = torch.empty(64 * 64, dtype=torch.int32, device="cuda")
stream = torch.cuda.Stream()
g = torch.Generator().manual_seed(1)
cam = dev.camera
origin = torch.tensor([list(cam.eye)] * 64, dtype=torch.float32).cuda()
direction = torch.nn.functional.normalize(torch.rand(64, 3, generator=g) - 0.5, dim=1).cuda()
out = {"hit_id": torch.empty(64, dtype=torch.int32, device="cuda"), "t": torch.empty(64, dtype=torch.float32, device="cuda")}


def clock(call):
    for _ in range(100):
        call()
    loops = []
    for _ in range(LOOPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        torch.cuda.synchronize()
        loops.append((time.perf_counter() - t0) / CALLS * 1e6)
    assert dev.status() == 0
    return {"us_per_call": statistics.median(loops), "loops": [round(x, 3) for x in loops]}


rows = {}
for name, mode in (("render_device literal", p3d.STACK_LITERAL), ("render_device per_pixel", p3d.STACK_PER_PIXEL)):
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, stack_mode=mode)
    rows[name] = clock(lambda: dev.render_device(cfg, tile, rgb.data_ptr(), hit.data_ptr(), 0, stream.cuda_stream))
rows["trace_closest_device 64 rays"] = clock(lambda: dev.trace_closest_device(p3d.ACCEL_BVH, origin, direction, stream=stream, out=out))
print(json.dumps({"package": root, "lib": p3d.LIB_PATH, "rows": rows}))

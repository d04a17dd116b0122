"""CPU tests of the product's HOST side (no GPU needed): the C-ABI library loads and exports
every symbol include/p3d.h declares; the .p3f loader, BVH builder and grid builder inside
libp3d.so produce bit-for-bit what the oracle's independent restatement produces."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENES, scene_path
from oracle import binding as ob
import p3d_amd as p3d

ALL_SCENES = sorted(f for f in os.listdir(SCENES) if f.endswith(".p3f"))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "p3d.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(p3d.EXPORTS), declared ^ set(p3d.EXPORTS)
    lib = p3d.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.p3d_abi_version() == 4  # round 4: p3d_stats.handoff_dense_retry
    # the test hooks are exported but live in a private header (csrc/p3d_debug.h), not in the drop-in boundary
    assert "p3d_debug" not in hdr and hasattr(lib, "p3d_debug_scene_limits")
    dbg = open(os.path.join(ROOT, "p3d-raytracer_amd", "csrc", "p3d_debug.h")).read()
    assert "p3d_debug_scene_limits" in dbg


def test_struct_layouts_match_the_header():
    assert C.sizeof(p3d.Prim) == 96 and C.sizeof(p3d.Material) == 64 and C.sizeof(p3d.Light) == 32
    assert C.sizeof(p3d.Camera) == 80 and C.sizeof(p3d.BvhNode) == 32
    assert C.sizeof(p3d.Config) == 80 and C.sizeof(p3d.Tile) == 24 and C.sizeof(p3d.Stats) == 21 * 8


def test_config_default_is_constants_h():
    c = p3d.default_config()
    assert (c.integrator, c.accel, c.max_depth, c.spp_sqrt) == (p3d.PATHTRACE, p3d.ACCEL_BVH, 20, 20)  # constants.h:6,12,36,44
    assert (c.antialiasing, c.depth_of_field, c.sample_disk, c.soft_shadows, c.sample_mode) == (1, 1, 1, 0, 0)
    assert (c.light_side, c.gamma) == (0.5, 1.0)
    assert c.stack_mode == p3d.STACK_LITERAL  # one hit_stack for the whole frame (bvh.cpp:86)
    assert c.debug_view == p3d.DEBUG_NONE     # TEST_INTERSECT false, DEPTH_MAP false (constants.h:18,33)


def test_no_gpu_means_loud_failure_not_fallback():
    if p3d.device_count() > 0:
        pytest.skip("a HIP device is present")
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    with pytest.raises(p3d.P3DError) as e:
        p3d.DeviceScene(hs)
    assert e.value.code == -2  # P3D_ERR_NO_DEVICE


@pytest.mark.parametrize("scene", ALL_SCENES)
@pytest.mark.parametrize("legacy", [False, True])
def test_loader_and_builders_match_oracle(scene, legacy):
    hs = p3d.HostScene(scene_path(scene), legacy_f11=legacy)
    sc = ob.Scene(scene_path(scene), legacy_f11=legacy)
    cnt = sc.counts()
    try:
        a = hs.arrays(bvh=True, grid=cnt["objects"] > 0)
    except p3d.P3DError:
        # objects before the first `f`: neither side can render (the reference would null-deref)
        assert any(sc.object(i)["material"] < 0 for i in range(cnt["objects"]))
        return
    assert (a["n_prims"], a["n_lights"], a["n_materials"]) == (cnt["objects"], cnt["lights"], cnt["materials"])
    for i in range(cnt["objects"]):
        o = sc.object(i)
        assert a["prim_type"][i] == o["type"] and a["prim_material"][i] == o["material"]
        assert (u32(a["prim_v"][i]) == u32(o["v"])).all()
        assert (u32(a["prim_bmin"][i]) == u32(o["bmin"])).all() and (u32(a["prim_bmax"][i]) == u32(o["bmax"])).all()
        if o["type"] == 1:
            assert (u32(a["prim_n"][i]) == u32(o["n"])).all()
    for i in range(cnt["materials"]):
        assert (u32(a["materials"][i][:15]) == u32(sc.material(i)[:15])).all()
    for i in range(cnt["lights"]):
        p, c = sc.light(i)
        assert (u32(a["lights"][i]) == u32(np.concatenate([p, c]))).all()
    if cnt["has_camera"]:
        cam = sc.camera()
        for k in ("eye", "u", "v", "n"):
            assert (u32(a["camera"][k]) == u32(cam[k])).all()
        for k in ("w", "h", "plane_dist", "focal_ratio", "aperture"):
            assert np.float32(a["camera"][k]).view(np.uint32) == np.float32(cam[k]).view(np.uint32)
    assert (u32(a["background"]) == u32(sc.background())).all()
    # BVH: same nodes in the same order, same permutation (bvh.cpp:89-196)
    o = sc.bvh_nodes()
    assert len(a["bvh_index"]) == len(o["index"])
    assert (u32(a["bvh_bmin"]) == u32(o["bmin"])).all() and (u32(a["bvh_bmax"]) == u32(o["bmax"])).all()
    assert (a["bvh_index"] == o["index"]).all() and (a["bvh_order"] == o["order"]).all()
    assert (((a["bvh_count_leaf"] >> 31) & 1) == o["leaf"]).all()
    leaf = o["leaf"] == 1
    assert ((a["bvh_count_leaf"][leaf] & 0x7fffffff) == o["n_objs"][leaf]).all()
    assert a["bvh_max_depth"] == sc.bvh_info()["max_depth"]
    if cnt["objects"] > 0:  # grid.cpp:3-68
        g = sc.grid()
        assert tuple(a["grid_n"]) == tuple(int(v) for v in g["n"])
        assert (u32(a["grid_bmin"]) == u32(g["bmin"])).all() and (u32(a["grid_bmax"]) == u32(g["bmax"])).all()
        assert (a["grid_cell_start"] == g["cell_start"]).all() and (a["grid_cell_items"] == g["cell_items"]).all()


def test_big_bvh_matches_oracle_and_reference_counts(tri100k_path):
    hs = p3d.HostScene(tri100k_path)
    a = hs.arrays(bvh=True)
    sc = ob.Scene(tri100k_path)
    o = sc.bvh_nodes()
    assert len(a["bvh_index"]) == 125701 and a["bvh_max_depth"] == 21
    assert (a["bvh_index"] == o["index"]).all() and (a["bvh_order"] == o["order"]).all()
    assert (u32(a["bvh_bmin"]) == u32(o["bmin"])).all() and (u32(a["bvh_bmax"]) == u32(o["bmax"])).all()


def test_camera_overrides_and_light_replication():
    hs = p3d.HostScene(scene_path("path_dof.p3f"))
    sc = ob.Scene(scene_path("path_dof.p3f"))
    for h in (hs, sc):
        h.set_resolution(640, 360)
        h.set_lens(4.0, 1.25)
    a = hs.arrays()
    cam = sc.camera()
    assert a["res"] == (640, 360)
    for k in ("w", "h", "aperture", "focal_ratio"):
        assert np.float32(a["camera"][k]).view(np.uint32) == np.float32(cam[k]).view(np.uint32)
    hs2 = p3d.HostScene(scene_path("balls_low.p3f"))
    sc2 = ob.Scene(scene_path("balls_low.p3f"))
    hs2.replicate_lights(4, 0.5)
    sc2.replicate_lights(4, 0.5)
    a2 = hs2.arrays()
    assert a2["n_lights"] == 3 * 16 == sc2.counts()["lights"]
    for i in range(a2["n_lights"]):
        p, c = sc2.light(i)
        assert (u32(a2["lights"][i]) == u32(np.concatenate([p, c]))).all()


def test_loader_error_paths():
    with pytest.raises(p3d.P3DError) as e:
        p3d.HostScene("/no/such/scene.p3f")
    assert e.value.code == -5
    hs = p3d.HostScene(scene_path("balls_medium.p3f"))   # 11-number `f`: shipped parser stops, 0 objects
    assert hs.arrays()["n_prims"] == 0 and hs.arrays()["n_lights"] == 3
    assert p3d.HostScene(scene_path("balls_medium.p3f"), legacy_f11=True).arrays()["n_prims"] == 93


def test_handoff_predecessor_successor_scans(tmp_path):
    """csrc/handoff.hpp: which unit's leftover a pixel starts on (handoff_pred) and whose start a changed leftover
    invalidates (handoff_succ) — bit scans over the touched words, cut at rows that start a halo chain — against a
    unit-by-unit walk over random patterns.  Host build of the same inline functions the kernels use; no GPU."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "handoff_scan_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "p3d-raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "handoff_scan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 100000


def test_scene_create_rejects_a_bvh_that_is_not_a_tree():
    """The descriptor's BVH is validated before anything touches a device (so this runs without one): a record with
    two parents - shared or overlapping child pairs - passes the bounds checks but is a DAG; the upload's relabelling
    walk would re-visit shared subtrees (Fibonacci-sized work for a chain of overlapping pairs).  Rejected, not hung."""
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    good = hs.desc(bvh=True, grid=False)
    L = p3d.lib()

    def create(mutate):
        d = p3d.SceneDesc.from_buffer_copy(bytes(good))
        nodes = (p3d.BvhNode * good.n_bvh_nodes)(*[good.bvh_nodes[i] for i in range(good.n_bvh_nodes)])
        d.bvh_nodes = nodes
        mutate(nodes)
        h = C.c_void_p()
        rc = L.p3d_scene_create(C.byref(d), 0, C.byref(h))
        if rc == 0:
            L.p3d_scene_destroy(h)
        return rc, L.p3d_last_error().decode()

    inner = [i for i in range(good.n_bvh_nodes) if not (good.bvh_nodes[i].count_leaf & 0x80000000)]
    a, b = inner[1], inner[2]

    def shared(n):
        n[a].index = n[b].index = max(n[a].index, n[b].index)

    def overlapping(n):
        n[b].index = n[a].index + 1

    for m in (shared, overlapping):
        rc, msg = create(m)
        assert rc == -1 and "more than one parent" in msg, (m.__name__, rc, msg)
    # a synthetic chain of 60 overlapping pairs (node k -> children k+1, k+2): 2^40-ish walk if it were accepted
    n_chain = 64
    d = p3d.SceneDesc.from_buffer_copy(bytes(good))
    nodes = (p3d.BvhNode * n_chain)()
    for k in range(n_chain):
        nodes[k].bmin[:] = [-1, -1, -1]
        nodes[k].bmax[:] = [1, 1, 1]
        if k + 2 < n_chain:
            nodes[k].index, nodes[k].count_leaf = k + 1, 0
        else:
            nodes[k].index, nodes[k].count_leaf = 0, 0x80000000 | 1
    d.bvh_nodes, d.n_bvh_nodes, d.bvh_max_depth = nodes, n_chain, n_chain
    h = C.c_void_p()
    assert L.p3d_scene_create(C.byref(d), 0, C.byref(h)) == -1 and "more than one parent" in L.p3d_last_error().decode()


def test_library_decodes_the_shipped_jpeg_faces_like_the_fixture(tmp_path):
    """Scene::LoadSkybox (scene.cpp:329-377) asks DevIL for the six JPEG faces; the library decodes them itself
    (host/jpeg_decode.cpp: baseline JPEG along the IJG library's default path).  DevIL's version is unpinned in the
    reference, so the bar is the decoder the fixtures were made with: tests/golden/skybox/decoded.json (PIL 12.2,
    libjpeg-turbo) - byte for byte, tolerance 0, on all six shipped faces."""
    import hashlib
    import json
    sky = os.path.join(ROOT, "tests", "golden", "skybox")
    want = json.load(open(os.path.join(sky, "decoded.json")))["faces"]
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    assert not hs.has_skybox()  # `env skybox` is relative to the working directory / the scene file: not there
    hs.load_skybox(sky)
    assert hs.has_skybox()
    for i, name in enumerate(p3d.SKYBOX_FACE_FILES):
        face = hs.skybox_face(i)  # bottom row first (IL_ORIGIN_LOWER_LEFT)
        assert face.shape == (2048, 2048, 3)
        assert hashlib.sha256(np.ascontiguousarray(face[::-1]).tobytes()).hexdigest() == want[name]["decoded_rgb_sha256"], name
    with pytest.raises(p3d.P3DError) as e:
        p3d.HostScene(scene_path("balls_low.p3f")).load_skybox(str(tmp_path))
    assert e.value.code == -5 and "right" in str(e.value)  # P3D_ERR_IO, names the face


def test_jpeg_decoder_matches_pil_on_other_baseline_files_and_refuses_the_rest(tmp_path):
    """Sampling factors 1x1 / 2x1 / 2x2, grey, sizes that are not whole MCUs, restart intervals: byte for byte what PIL
    decodes.  Progressive files and garbage are refused with a message, not decoded wrongly."""
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:61, 0:83]
    base = np.stack([(xx * 3 + yy) % 256, (yy * 5 + 40 * np.sin(xx / 7.0)) % 256, (xx * yy // 9) % 256], -1).astype(np.uint8)
    base[20:40, 30:60] = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    hs = p3d.HostScene(scene_path("balls_low.p3f"))

    def through_library(make):
        folder = tmp_path / ("sky%d" % through_library.n)
        through_library.n += 1
        folder.mkdir()
        for name in p3d.SKYBOX_FACE_FILES:
            make(str(folder / (name + ".jpg")))
        hs.load_skybox(str(folder))
        return hs.skybox_face(0)[::-1], np.asarray(Image.open(str(folder / "right.jpg")).convert("RGB"))
    through_library.n = 0

    cases = [dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, quality=35), dict(subsampling=0, quality=98)]
    for size in ((83, 61), (16, 16), (17, 9), (1, 1), (33, 2)):
        for kw in cases:
            img = Image.fromarray(base[:size[1], :size[0]])
            got, ref = through_library(lambda p: img.save(p, "JPEG", **kw))
            assert got.shape == ref.shape and (got == ref).all(), (size, kw, int(np.abs(got.astype(int) - ref).max()))
    grey = Image.fromarray(base[..., 0])
    got, ref = through_library(lambda p: grey.save(p, "JPEG", quality=80))
    assert (got == ref).all()
    try:  # restart markers (Pillow >= 10.2)
        img = Image.fromarray(base)
        got, ref = through_library(lambda p: img.save(p, "JPEG", subsampling=2, restart_marker_blocks=3))
        assert (got == ref).all()
    except TypeError:
        pass
    with pytest.raises(p3d.P3DError) as e:
        through_library(lambda p: Image.fromarray(base).save(p, "JPEG", progressive=True))
    assert "progressive" in str(e.value)
    with pytest.raises(p3d.P3DError):
        through_library(lambda p: open(p, "wb").write(b"\xff\xd8\xff\xe0 not a jpeg at all"))


def test_bench_counts_the_instructions_of_a_frame_of_the_profiled_stack_mode_only():
    """bench.py `roofline.timed_loop_frac` sums the VALU wave-instructions of every launch of ONE frame from the committed PMC
    summary.  A profiled literal run also times its per-pixel counterpart (and once each the counting instantiations): those
    must not be counted.  Checked on a synthetic summary with the kernel names rocprofv3 reports."""
    import sys
    sys.path.insert(0, ROOT)
    import bench

    def k(calls, valu):
        return {"calls": calls, "counters": {"SQ_INSTS_VALU": {"mean": valu}}}
    summary = {"dominant": {"calls": 100, "SQ_INSTS_VALU": 60.0},
               "kernels": {"whitted_kernel<2, true, false, false, false, 1, 1, false>": k(100, 60.0),   # pass 1
                           "whitted_kernel<2, true, false, false, false, 1, 3, false>": k(100, 7.0),    # round 0 over the tiles
                           "whitted_kernel<2, true, false, false, false, 1, 2, false>": k(200, 0.5),    # two work-list launches per frame
                           "handoff_check_entries_kernel<true, false, false>": k(100, 0.25),
                           "clear_kernel": k(110, 0.01),
                           "whitted_kernel<2, true, false, false, false, 1, 0, true>": k(101, 58.0),    # the per-pixel frames of the same run
                           "whitted_kernel<2, true, true, false, false, 1, 1, false>": k(1, 70.0),      # counting instantiation, once
                           "sched_build_kernel": k(2, 0.02), "__amd_rocclr_copyBuffer": k(100, 0.001)}}
    assert abs(bench.frame_valu_instructions(summary, True) - (60.0 + 7.0 + 2 * 0.5 + 0.25 + 0.011)) < 1e-9
    assert abs(bench.frame_valu_instructions(summary, False) - 58.0 * 1.01) < 1e-9


def test_bench_dump_outputs_types_and_fixed_sample(tmp_path):
    """bench.py --dump-outputs: float32 / float64 files; above the size limit every array keeps the same seeded sample of
    pixels, the same from run to run, with its pixel indices, and the files stay within the limit."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(1)
    h, w = 64, 48
    frame = {"rgb": rng.random((h, w, 3), dtype=np.float32), "hit": rng.integers(-1, 1 << 30, (h, w), dtype=np.int32),
             "rgb8": rng.integers(0, 256, (h, w, 3), dtype=np.uint8)}
    shapes = bench.dump_outputs(str(tmp_path / "whole"), frame)
    assert shapes == {"rgb": (h, w, 3), "hit": (h, w), "rgb8": (h, w, 3)}
    got = {k: np.load(str(tmp_path / "whole" / (k + ".npy"))) for k in shapes}
    assert got["rgb"].dtype == np.float32 and (got["rgb"] == frame["rgb"]).all()
    assert got["hit"].dtype == np.float64 and (got["hit"] == frame["hit"]).all()
    assert got["rgb8"].dtype == np.float32 and (got["rgb8"] == frame["rgb8"]).all()
    limit = 40000
    for run in ("a", "b"):
        shapes = bench.dump_outputs(str(tmp_path / run), frame, limit=limit)
        assert set(shapes) == {"rgb", "hit", "rgb8", "pixel_index"}
        assert sum(os.path.getsize(str(tmp_path / run / (k + ".npy"))) for k in shapes) <= limit
    idx = np.load(str(tmp_path / "a" / "pixel_index.npy"))
    assert idx.dtype == np.float64 and 0 < len(idx) < h * w and (np.diff(idx) > 0).all()
    assert (idx == np.load(str(tmp_path / "b" / "pixel_index.npy"))).all()
    flat = idx.astype(np.int64)
    for k in ("rgb", "hit", "rgb8"):
        a = np.load(str(tmp_path / "a" / (k + ".npy")))
        assert (a == np.load(str(tmp_path / "b" / (k + ".npy")))).all()
        assert (a == frame[k].reshape((h * w,) + frame[k].shape[2:])[flat]).all()

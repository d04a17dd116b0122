// p3d_render — the console front end.  Does what the reference's main() does when its GL
// window is off (main.cpp:1004-1019): ask for a scene, load it, render a frame, print the
// time, save the image — with the frame loop (main.cpp:747-820) running on the MI355X
// through include/p3d.h.  Options that are #defines in constants.h are flags here.
//
//   p3d_render [scene.p3f] [--whitted|--pathtrace] [--accel none|grid|bvh] [--depth N]
//              [--spp N(sqrt)] [--aa 0|1] [--dof 0|1] [--soft 0|1] [--tent] [--gamma G]
//              [--res W H] [--seed S] [--legacy-f11] [--device D]
//              [--out image.png|image.ppm]   default RT_Output.png, as saveImgFile writes it (main.cpp:674-689,851);
//                               PNG through zlib (8-bit RGB, no DevIL), a name ending in .ppm gives a binary PPM
//              [--stack literal|per_pixel]   p3d_config.stack_mode (default literal: the reference's one hit_stack)
//              [--device-bvh]   build a linear BVH on the GPU instead of the reference's tree on the host
//                               (p3d_scene_create_device_bvh: same closest hits, shadow feelers may differ)
//              [--device-grid]  build the uniform grid on the GPU after create (p3d_scene_build_grid: the host's grid to the
//                               bit, same image as without the flag); implies --device-bvh; for --accel grid
//              [--skybox DIR]   DIR/{right,left,top,bottom,front,back}.jpg (baseline JPEG, decoded by the library as
//                               Scene::LoadSkybox asks DevIL to; .ppm accepted too) -> SKYBOX true.  A scene's own
//                               `env <dir>` line does the same when the folder is found.
//              [--gpus N]       the frame's rows dealt to N GPUs of this node in 8-row stripes (one device scene each, this
//                               one process driving them), every GPU's part of the image brought to GPU 0 by ONE
//                               ncclGather over xGMI (RCCL, loaded at run time), de-interleaved on the host.  Same image
//                               as one GPU renders, bit for bit (P3D_STACK_LITERAL included: include/p3d.h, p3d_tile).
//              [--verify]       with --gpus: one more frame whose float RGB + hit IDs (16 B/px, what bench.py gathers) go
//                               through a second ncclGather; GPU 0 then renders the whole frame alone and the gathered
//                               frame is compared with it bit for bit - colours, hit IDs and the u8 image.  Prints the
//                               verdict; a mismatch is exit code 3.
//              [--passes K]     progressive: the frame's SPP*SPP samples in K passes of as-equal-as-possible size (p3d_accum,
//                               include/p3d.h); --out is rewritten after every pass and one line per pass gives the samples
//                               done and the pass time.  The last file is byte-identical to the one written without --passes.
//                               Needs --aa 1 and, for --whitted over the BVH, --stack per_pixel; not with --gpus.
//              [--adaptive REL] with --passes and --pathtrace: adaptive sampling (p3d_adaptive, include/p3d.h) - a pixel
//              [--min-spp M]    stops taking samples once its relative error is below REL and it has at least M samples
//                               (default 16, or SPP*SPP when smaller).  One line per pass gives the samples done, the pixels
//                               still active and the pass time; the passes end early once no pixel is active.
//              [--denoise FILE] --pathtrace --aa 1: the final frame (the one-shot frame, or the last of --passes) denoised
//              [--denoise-iter N]  with the edge-avoiding a-trous filter (p3d_denoise, include/p3d.h; N iterations, default 5,
//              [--feature-spp K]   at most 8) over feature buffers of the first K samples' primary rays (default 0 = min(16,
//                               SPP*SPP)); with --adaptive the filter uses the frame's variance.  FILE is PNG or PPM by
//                               extension, as --out; --out is written as without --denoise.  Not with --whitted or --gpus.
//              [--frames N]     N frames of a moving camera (one-shot renders): frame k turns the view k * DEG degrees about
//              [--orbit DEG]    the `up` axis through `at` (p3d_camera_look_at, p3d_scene_set_camera) and uses seed + k.  Frame k
//                               is written to <out>_%03d.<ext> (and <denoise>_%03d.<ext>), and one line per frame prints its
//                               from / at / up (%.9g).  Frame 0 is the scene's own view.  Not with --passes or --gpus.
//              [--temporal]     with --frames, --pathtrace and --denoise: every frame goes through the temporal accumulator
//                               (p3d_temporal, default parameters) and the variance-term filter at sigma_luma = 4 (SVGF's
//                               value: the temporal variance is per sample; DESIGN.md "Temporal reprojection").
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <zlib.h>

#include "p3d.h"

namespace {

int die(const char* what) {
  std::fprintf(stderr, "%s: %s\n", what, p3d_last_error());
  return 1;
}

// img_Data is stored bottom row first (main.cpp:818-820, y = 0 at the bottom); image files
// start with the top row, so rows are written in reverse.
bool save_ppm(const std::string& path, const std::vector<uint8_t>& rgb8, int w, int h) {
  std::ofstream f(path, std::ios::binary);
  if (!f) return false;
  f << "P6\n" << w << " " << h << "\n255\n";
  for (int y = h - 1; y >= 0; --y) f.write(reinterpret_cast<const char*>(&rgb8[(size_t)y * w * 3]), (std::streamsize)w * 3);
  return (bool)f;
}

// saveImgFile (main.cpp:674-689) without DevIL: 8-bit RGB PNG, one IDAT chunk, filter type 0 on every scanline.
bool save_png(const std::string& path, const std::vector<uint8_t>& rgb8, int w, int h) {
  std::vector<uint8_t> raw((size_t)h * (1 + (size_t)w * 3));
  for (int y = 0; y < h; ++y) {  // file rows are top-down, img_Data is bottom-up
    uint8_t* row = &raw[(size_t)y * (1 + (size_t)w * 3)];
    row[0] = 0;
    std::memcpy(row + 1, &rgb8[(size_t)(h - 1 - y) * w * 3], (size_t)w * 3);
  }
  uLongf zlen = compressBound((uLong)raw.size());
  std::vector<uint8_t> z(zlen);
  if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), 6) != Z_OK) return false;
  std::ofstream f(path, std::ios::binary);
  if (!f) return false;
  auto be32 = [](uint32_t v, uint8_t* p) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; };
  auto chunk = [&](const char type[4], const uint8_t* data, uint32_t n) {
    uint8_t len[4], crcb[4];
    be32(n, len);
    f.write(reinterpret_cast<const char*>(len), 4);
    f.write(type, 4);
    if (n) f.write(reinterpret_cast<const char*>(data), n);
    uLong crc = crc32(0L, reinterpret_cast<const Bytef*>(type), 4);
    if (n) crc = crc32(crc, data, n);
    be32((uint32_t)crc, crcb);
    f.write(reinterpret_cast<const char*>(crcb), 4);
  };
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  f.write(reinterpret_cast<const char*>(sig), 8);
  uint8_t ihdr[13];
  be32((uint32_t)w, ihdr); be32((uint32_t)h, ihdr + 4);
  ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;  // 8 bits, colour type 2 (RGB)
  chunk("IHDR", ihdr, 13);
  chunk("IDAT", z.data(), (uint32_t)zlen);
  chunk("IEND", nullptr, 0);
  return (bool)f;
}

// ---- --gpus N: one process, N devices, one RCCL gather per frame (ncclGather, rccl.h:745) ----
// RCCL is loaded with dlopen: a run without --gpus neither needs nor loads it.  Only the five entry points used here
// are declared (types as in rccl.h: ncclComm_t is an opaque pointer, ncclResult_t / ncclDataType_t are enums; ncclUint8 = 1).
struct Rccl {
  void* lib = nullptr;
  int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
  int (*CommDestroy)(void* comm) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Gather)(const void* send, void* recv, size_t count, int datatype, int root, void* comm, hipStream_t stream) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool load() {
    for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) { std::fprintf(stderr, "--gpus: cannot load librccl.so: %s\n", dlerror()); return false; }
    auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p) std::fprintf(stderr, "--gpus: librccl.so has no %s\n", n); return p; };
    CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
    GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
    Gather = (decltype(Gather))sym("ncclGather");
    GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
    return CommInitAll && CommDestroy && GroupStart && GroupEnd && Gather && GetErrorString;
  }
};
constexpr int kNcclUint8 = 1;  // rccl.h: ncclUint8
constexpr int kStripeRows = 8;

// Renders the frame on n GPUs into `img` (bottom row first, 3 bytes per pixel).  Returns 0, or 1 after printing why not.
int render_multi_gpu(const p3d_scene_desc* desc, bool device_bvh, bool device_grid, p3d_config cfg, int n, bool verify, std::vector<uint8_t>& img, double* secs) {
  const int W = desc->camera.res_x, H = desc->camera.res_y;
  int ndev = p3d_device_count();
  if (n > ndev) { std::fprintf(stderr, "--gpus %d: this node shows %d HIP device(s)\n", n, ndev); return 1; }
  if (H % (kStripeRows * n) != 0) { std::fprintf(stderr, "--gpus %d: the image height %d is not a multiple of %d rows\n", n, H, kStripeRows * n); return 1; }
  Rccl rccl;
  if (!rccl.load()) return 1;
  auto hip_ok = [](hipError_t e, const char* what) { if (e != hipSuccess) std::fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); return e == hipSuccess; };
  auto nccl_ok = [&](int r, const char* what) { if (r != 0) std::fprintf(stderr, "%s: %s\n", what, rccl.GetErrorString(r)); return r == 0; };
  std::vector<int> devs(n);
  for (int d = 0; d < n; ++d) devs[d] = d;
  std::vector<void*> comms(n, nullptr);
  if (!nccl_ok(rccl.CommInitAll(comms.data(), n, devs.data()), "ncclCommInitAll")) return 1;
  const size_t part = (size_t)3 * W * (H / n);  // bytes of one GPU's stripes
  std::vector<p3d_scene*> scenes(n, nullptr);
  std::vector<hipStream_t> streams(n, nullptr);
  std::vector<uint8_t*> d_part(n, nullptr);
  uint8_t* d_all = nullptr;
  cfg.collect_stats = 0;
  for (int d = 0; d < n; ++d) {
    const int rc = device_grid || (device_bvh && cfg.accel == P3D_ACCEL_BVH) ? p3d_scene_create_device_bvh(desc, d, &scenes[d], nullptr) : p3d_scene_create(desc, d, &scenes[d]);
    if (rc != P3D_OK) return die("scene_create");
    if (device_grid && p3d_scene_build_grid(scenes[d], nullptr) != P3D_OK) return die("scene_build_grid");
    if (!hip_ok(hipSetDevice(d), "hipSetDevice") || !hip_ok(hipStreamCreate(&streams[d]), "hipStreamCreate") ||
        !hip_ok(hipMalloc((void**)&d_part[d], part), "hipMalloc"))
      return 1;
    if (d == 0 && !hip_ok(hipMalloc((void**)&d_all, part * n), "hipMalloc")) return 1;
  }
  auto frame = [&]() {
    for (int d = 0; d < n; ++d) {  // every GPU renders its stripes: rows d*8 .. d*8+7, then every n-th stripe
      p3d_tile t{0, d * kStripeRows, W, H / n, kStripeRows, n};
      if (p3d_render_tile_device(scenes[d], &cfg, &t, nullptr, nullptr, d_part[d], streams[d], nullptr) != P3D_OK) return false;
    }
    if (!nccl_ok(rccl.GroupStart(), "ncclGroupStart")) return false;
    for (int d = 0; d < n; ++d)
      if (!nccl_ok(rccl.Gather(d_part[d], d == 0 ? d_all : nullptr, part, kNcclUint8, 0, comms[d], streams[d]), "ncclGather")) return false;
    if (!nccl_ok(rccl.GroupEnd(), "ncclGroupEnd")) return false;
    for (int d = 0; d < n; ++d)
      if (!hip_ok(hipSetDevice(d), "hipSetDevice") || !hip_ok(hipStreamSynchronize(streams[d]), "hipStreamSynchronize")) return false;
    return true;
  };
  if (!frame()) return 1;  // first frame: code objects loaded, tile schedules and halo chains recorded
  const auto t0 = std::chrono::high_resolution_clock::now();
  if (!frame()) return 1;
  *secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
  for (int d = 0; d < n; ++d)
    if (p3d_scene_status(scenes[d]) != P3D_OK) return die("render");
  std::vector<uint8_t> all(part * n);
  if (!hip_ok(hipSetDevice(0), "hipSetDevice") || !hip_ok(hipMemcpy(all.data(), d_all, all.size(), hipMemcpyDeviceToHost), "hipMemcpy")) return 1;
  // de-interleave: stripe k of GPU d holds frame rows (k * n + d) * 8 .. + 7
  const size_t row_bytes = (size_t)3 * W;
  for (int d = 0; d < n; ++d)
    for (int r = 0; r < H / n; ++r) {
      const int y = ((r / kStripeRows) * n + d) * kStripeRows + r % kStripeRows;
      std::memcpy(&img[(size_t)y * row_bytes], &all[(size_t)d * part + (size_t)r * row_bytes], row_bytes);
    }
  int verdict = 0;
  if (verify) {
    // One more frame, all outputs: every GPU renders float RGB + hit IDs (packed: 12 B/px of colour, then 4 B/px of IDs,
    // for its own rows) next to the u8 image; the packed buffers go to GPU 0 through a second gather.  Then GPU 0 renders
    // the whole frame alone and the de-interleaved gathered frame must equal it bit for bit (SURVEY.md 8(e) invariant).
    const size_t px_part = (size_t)W * (H / n), packed = px_part * 16;
    std::vector<uint8_t*> d_packed(n, nullptr);
    uint8_t* d_packed_all = nullptr;
    bool ok = true;
    for (int d = 0; d < n && ok; ++d) {
      ok = hip_ok(hipSetDevice(d), "hipSetDevice") && hip_ok(hipMalloc((void**)&d_packed[d], packed), "hipMalloc");
      if (ok && d == 0) ok = hip_ok(hipMalloc((void**)&d_packed_all, packed * n), "hipMalloc");
    }
    for (int d = 0; d < n && ok; ++d) {
      p3d_tile t{0, d * kStripeRows, W, H / n, kStripeRows, n};
      ok = p3d_render_tile_device(scenes[d], &cfg, &t, (float*)d_packed[d], (int32_t*)(d_packed[d] + px_part * 12), d_part[d], streams[d], nullptr) == P3D_OK;
      if (!ok) std::fprintf(stderr, "--verify render: %s\n", p3d_last_error());
    }
    if (ok) ok = nccl_ok(rccl.GroupStart(), "ncclGroupStart");
    for (int d = 0; d < n && ok; ++d)
      ok = nccl_ok(rccl.Gather(d_part[d], d == 0 ? d_all : nullptr, part, kNcclUint8, 0, comms[d], streams[d]), "ncclGather") &&
           nccl_ok(rccl.Gather(d_packed[d], d == 0 ? d_packed_all : nullptr, packed, kNcclUint8, 0, comms[d], streams[d]), "ncclGather");
    if (ok) ok = nccl_ok(rccl.GroupEnd(), "ncclGroupEnd");
    for (int d = 0; d < n && ok; ++d) ok = hip_ok(hipSetDevice(d), "hipSetDevice") && hip_ok(hipStreamSynchronize(streams[d]), "hipStreamSynchronize") && p3d_scene_status(scenes[d]) == P3D_OK;
    const size_t px = (size_t)W * H;
    std::vector<float> g_rgb(px * 3), one_rgb(px * 3);
    std::vector<int32_t> g_hit(px), one_hit(px);
    std::vector<uint8_t> g_u8(px * 3), one_u8(px * 3), raw(packed * n), raw8(part * n);
    if (ok) ok = hip_ok(hipSetDevice(0), "hipSetDevice") && hip_ok(hipMemcpy(raw.data(), d_packed_all, raw.size(), hipMemcpyDeviceToHost), "hipMemcpy") &&
                 hip_ok(hipMemcpy(raw8.data(), d_all, raw8.size(), hipMemcpyDeviceToHost), "hipMemcpy");
    for (int d = 0; d < n && ok; ++d)
      for (int r = 0; r < H / n; ++r) {
        const int y = ((r / kStripeRows) * n + d) * kStripeRows + r % kStripeRows;
        const uint8_t* base = &raw[(size_t)d * packed];
        std::memcpy(&g_rgb[(size_t)y * W * 3], base + (size_t)r * W * 12, (size_t)W * 12);
        std::memcpy(&g_hit[(size_t)y * W], base + px_part * 12 + (size_t)r * W * 4, (size_t)W * 4);
        std::memcpy(&g_u8[(size_t)y * row_bytes], &raw8[(size_t)d * part + (size_t)r * row_bytes], row_bytes);
      }
    if (ok) {  // the whole frame on GPU 0 alone, through the host-buffer call
      p3d_tile full{0, 0, W, H, 0, 1};
      ok = p3d_render_tile(scenes[0], &cfg, &full, one_rgb.data(), one_hit.data(), one_u8.data(), nullptr) == P3D_OK;
      if (!ok) std::fprintf(stderr, "--verify single-GPU frame: %s\n", p3d_last_error());
    }
    for (int d = 0; d < n; ++d) { (void)hipSetDevice(d); if (d_packed[d]) (void)hipFree(d_packed[d]); }
    (void)hipSetDevice(0);
    if (d_packed_all) (void)hipFree(d_packed_all);
    if (!ok) return 1;
    size_t bad_rgb = 0, bad_hit = 0, bad_u8 = 0;
    for (size_t i = 0; i < px * 3; ++i) {
      uint32_t a, b;
      std::memcpy(&a, &g_rgb[i], 4); std::memcpy(&b, &one_rgb[i], 4);
      bad_rgb += a != b;
      bad_u8 += g_u8[i] != one_u8[i];
    }
    for (size_t i = 0; i < px; ++i) bad_hit += g_hit[i] != one_hit[i];
    const bool same = bad_rgb == 0 && bad_hit == 0 && bad_u8 == 0 && g_u8 == img;
    std::printf("verify: frame gathered from %d GPU(s) vs the frame GPU 0 renders alone (float RGB, hit IDs, u8 image): %s", n, same ? "bit-identical\n" : "MISMATCH");
    if (!same) std::printf(" (%zu colour words, %zu hit IDs, %zu bytes differ%s)\n", bad_rgb, bad_hit, bad_u8, g_u8 == img ? "" : "; the timed frame's u8 image differs from the verify frame's");
    verdict = same ? 0 : 3;
  }
  for (int d = 0; d < n; ++d) {
    (void)hipSetDevice(d);
    (void)hipFree(d_part[d]);
    (void)hipStreamDestroy(streams[d]);
    p3d_scene_destroy(scenes[d]);
    (void)rccl.CommDestroy(comms[d]);
  }
  (void)hipSetDevice(0);
  (void)hipFree(d_all);
  return verdict;
}

bool save_image(const std::string& path, const std::vector<uint8_t>& rgb8, int w, int h) {
  const bool ppm = path.size() > 4 && path.compare(path.size() - 4, 4, ".ppm") == 0;
  return ppm ? save_ppm(path, rgb8, w, h) : save_png(path, rgb8, w, h);
}

// <base>_%03d<.ext>: the frame number before the extension (none: appended)
std::string frame_name(const std::string& path, long k) {
  char num[16];
  std::snprintf(num, sizeof(num), "_%03ld", k);
  const size_t slash = path.find_last_of('/'), dot = path.find_last_of('.');
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return path + num;
  return path.substr(0, dot) + num + path.substr(dot);
}

// --frames N --orbit DEG: frame k sees the scene from `from` turned k * DEG degrees about the `up` axis through `at` (Rodrigues'
// rotation in double, rounded to float once), rendered with seed + k; with --denoise every frame is filtered, with --temporal
// after the temporal accumulator.  Returns the exit code.
int render_frames(p3d_host_scene* hs, p3d_scene* scene, p3d_config cfg, long frames, double orbit, bool temporal, const std::string& out,
                  const std::string& denoise_out, long denoise_iter, long feature_spp, int device) {
  float from[3], at[3], up[3], angle, aperture_ratio, focal_ratio;
  if (p3d_host_scene_view(hs, from, at, up, &angle, &aperture_ratio, &focal_ratio) != P3D_OK) return die("view");
  p3d_camera cam0;
  if (p3d_scene_camera(scene, &cam0) != P3D_OK) return die("camera");
  const int W = cam0.res_x, H = cam0.res_y;
  const size_t px = (size_t)W * H;
  const bool denoise = !denoise_out.empty();
  std::vector<uint8_t> img(px * 3), den(denoise ? px * 3 : 0);
  std::vector<float> lin(denoise ? px * 3 : 0), nd(denoise ? px * 4 : 0), ac(denoise ? px * 4 : 0), trgb, tvar;
  p3d_denoiser* dn = nullptr;
  p3d_temporal* tp = nullptr;
  if (denoise && p3d_denoiser_create(device, W, H, &dn) != P3D_OK) return die("denoiser_create");
  if (temporal) {
    if (p3d_temporal_create(device, W, H, &tp) != P3D_OK) return die("temporal_create");
    trgb.resize(px * 3);
    tvar.resize(px);
  }
  p3d_denoise_params dprm;
  p3d_denoise_params_default(&dprm);
  if (denoise_iter >= 0) dprm.iterations = (uint32_t)denoise_iter;
  dprm.gamma = cfg.gamma;
  if (temporal) dprm.sigma_luma = 4.0f;  // the per-sample variance of the temporal moments, as SVGF's
  p3d_temporal_params tprm;
  p3d_temporal_params_default(&tprm);
  const p3d_tile tile{0, 0, W, H, 0, 1};
  const uint64_t seed0 = cfg.seed;
  double ax = up[0], ay = up[1], az = up[2];
  const double al = std::sqrt(ax * ax + ay * ay + az * az);
  if (!(al > 0)) { std::fprintf(stderr, "--orbit: the scene's up vector is zero\n"); return 1; }
  ax /= al; ay /= al; az /= al;
  for (long k = 0; k < frames; ++k) {
    float f[3] = {from[0], from[1], from[2]};
    if (k > 0) {  // v' = v cos + (a x v) sin + a (a.v)(1 - cos), v = from - at
      const double th = (double)k * orbit * 3.14159265358979323846 / 180.0, c = std::cos(th), s = std::sin(th);
      const double vx = (double)from[0] - at[0], vy = (double)from[1] - at[1], vz = (double)from[2] - at[2];
      const double dt = ax * vx + ay * vy + az * vz;
      const double rx = vx * c + (ay * vz - az * vy) * s + ax * dt * (1 - c);
      const double ry = vy * c + (az * vx - ax * vz) * s + ay * dt * (1 - c);
      const double rz = vz * c + (ax * vy - ay * vx) * s + az * dt * (1 - c);
      f[0] = (float)(at[0] + rx); f[1] = (float)(at[1] + ry); f[2] = (float)(at[2] + rz);
      p3d_camera cam;
      if (p3d_camera_look_at(f, at, up, angle, W, H, aperture_ratio, focal_ratio, &cam) != P3D_OK || p3d_scene_set_camera(scene, &cam) != P3D_OK)
        return die("set_camera");
    }
    std::printf("frame %ld: from %.9g %.9g %.9g at %.9g %.9g %.9g up %.9g %.9g %.9g\n", k, f[0], f[1], f[2], at[0], at[1], at[2], up[0], up[1], up[2]);
    cfg.seed = seed0 + (uint64_t)k;
    p3d_stats st{};
    const auto t0 = std::chrono::high_resolution_clock::now();
    if (p3d_render_tile(scene, &cfg, &tile, denoise ? lin.data() : nullptr, nullptr, img.data(), &st) != P3D_OK) return die("render");
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    if (!save_image(frame_name(out, k), img, W, H)) { std::printf("Error saving Image file\n"); return 1; }
    if (denoise) {
      if (p3d_render_features(scene, &cfg, &tile, feature_spp > 0 ? (uint32_t)feature_spp : 0u, nd.data(), ac.data()) != P3D_OK)
        return die("render_features");
      if (temporal) {
        p3d_camera cam;
        if (p3d_scene_camera(scene, &cam) != P3D_OK) return die("camera");
        if (const int t = p3d_temporal_accumulate(tp, &tprm, &cam, lin.data(), nd.data(), ac.data(), trgb.data(), tvar.data(), nullptr); t != P3D_OK) {
          if (t != P3D_ERR_UNSUPPORTED) return die("temporal");
          std::fprintf(stderr, "--temporal: %s\n", p3d_last_error());
          return 2;
        }
      }
      if (p3d_denoise(dn, &dprm, temporal ? trgb.data() : lin.data(), temporal ? tvar.data() : nullptr, nd.data(), ac.data(), nullptr, den.data()) != P3D_OK)
        return die("denoise");
      if (!save_image(frame_name(denoise_out, k), den, W, H)) { std::printf("Error saving Image file\n"); return 1; }
    }
    std::printf("frame %ld: %.3f ms (render call), seed %llu\n", k, ms, (unsigned long long)cfg.seed);
    std::fflush(stdout);
  }
  if (tp) p3d_temporal_destroy(tp);
  if (dn) p3d_denoiser_destroy(dn);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  p3d_config cfg;
  p3d_config_default(&cfg);
  std::string scene_path, skybox_dir, out = "RT_Output.png";  // main.cpp:851
  int res_w = 0, res_h = 0, device = 0, gpus = 0;
  long passes = 0;  // --passes K (0: one call renders the frame)
  float adaptive = -1.0f;  // --adaptive REL (< 0: off)
  long min_spp = 0;        // --min-spp M (0: the default)
  std::string denoise_out;   // --denoise FILE (empty: off)
  long denoise_iter = -1;    // --denoise-iter N (-1: the default)
  long feature_spp = -1;     // --feature-spp K (-1: the default)
  long frames = 0;           // --frames N (0: one frame, the usual output names)
  double orbit = 0.0;        // --orbit DEG (degrees per frame)
  bool orbit_set = false, temporal = false;
  bool device_bvh = false, device_grid = false, verify = false;
  uint32_t load_flags = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&](const char* name) -> const char* {
      if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", name); std::exit(2); }
      return argv[++i];
    };
    if (a == "--whitted") cfg.integrator = P3D_WHITTED;
    else if (a == "--pathtrace") cfg.integrator = P3D_PATHTRACE;
    else if (a == "--accel") {
      const std::string v = next("--accel");
      cfg.accel = v == "none" ? P3D_ACCEL_NONE : (v == "grid" ? P3D_ACCEL_GRID : P3D_ACCEL_BVH);
    } else if (a == "--depth") cfg.max_depth = std::atoi(next("--depth"));
    else if (a == "--spp") cfg.spp_sqrt = (uint32_t)std::atoi(next("--spp"));
    else if (a == "--aa") cfg.antialiasing = (uint32_t)std::atoi(next("--aa"));
    else if (a == "--dof") cfg.depth_of_field = (uint32_t)std::atoi(next("--dof"));
    else if (a == "--soft") cfg.soft_shadows = (uint32_t)std::atoi(next("--soft"));
    else if (a == "--tent") cfg.sample_mode = P3D_SAMPLE_TENT;
    else if (a == "--gamma") cfg.gamma = (float)std::atof(next("--gamma"));
    else if (a == "--seed") cfg.seed = std::strtoull(next("--seed"), nullptr, 0);
    else if (a == "--res") { res_w = std::atoi(next("--res")); res_h = std::atoi(next("--res")); }
    else if (a == "--legacy-f11") load_flags |= P3D_LOAD_LEGACY_F11;
    else if (a == "--out") out = next("--out");
    else if (a == "--skybox") skybox_dir = next("--skybox");
    else if (a == "--stack") cfg.stack_mode = std::string(next("--stack")) == "per_pixel" ? P3D_STACK_PER_PIXEL : P3D_STACK_LITERAL;
    else if (a == "--device") device = std::atoi(next("--device"));
    else if (a == "--device-bvh") device_bvh = true;
    else if (a == "--device-grid") device_grid = device_bvh = true;
    else if (a == "--gpus") gpus = std::atoi(next("--gpus"));
    else if (a == "--verify") verify = true;
    else if (a == "--passes") {
      const char* v = next("--passes");
      char* end = nullptr;
      passes = std::strtol(v, &end, 10);
      if (end == v || *end != 0 || passes < 1) { std::fprintf(stderr, "--passes needs a whole number of passes, at least 1 (got '%s')\n", v); return 2; }
    }
    else if (a == "--adaptive") {
      const char* v = next("--adaptive");
      char* end = nullptr;
      adaptive = std::strtof(v, &end);
      if (end == v || *end != 0 || !(adaptive >= 0.0f) || adaptive == HUGE_VALF) {
        std::fprintf(stderr, "--adaptive needs a relative error, a number >= 0 (got '%s')\n", v);
        return 2;
      }
    } else if (a == "--min-spp") {
      const char* v = next("--min-spp");
      char* end = nullptr;
      min_spp = std::strtol(v, &end, 10);
      if (end == v || *end != 0 || min_spp < 2) { std::fprintf(stderr, "--min-spp needs a whole number of samples, at least 2 (got '%s')\n", v); return 2; }
    }
    else if (a == "--denoise") denoise_out = next("--denoise");
    else if (a == "--frames") {
      const char* v = next("--frames");
      char* end = nullptr;
      frames = std::strtol(v, &end, 10);
      if (end == v || *end != 0 || frames < 1 || frames > 1000) { std::fprintf(stderr, "--frames needs a whole number from 1 to 1000 (got '%s')\n", v); return 2; }
    } else if (a == "--orbit") {
      const char* v = next("--orbit");
      char* end = nullptr;
      orbit = std::strtod(v, &end);
      if (end == v || *end != 0 || !std::isfinite(orbit)) { std::fprintf(stderr, "--orbit needs a finite number of degrees (got '%s')\n", v); return 2; }
      orbit_set = true;
    } else if (a == "--temporal") temporal = true;
    else if (a == "--denoise-iter" || a == "--feature-spp") {
      const char* v = next(a.c_str());
      char* end = nullptr;
      const long n = std::strtol(v, &end, 10);
      const long hi = a == "--denoise-iter" ? 8 : 1L << 20;
      if (end == v || *end != 0 || n < 0 || n > hi) {
        std::fprintf(stderr, "%s needs a whole number from 0 to %ld (got '%s')\n", a.c_str(), hi, v);
        return 2;
      }
      (a == "--denoise-iter" ? denoise_iter : feature_spp) = n;
    }
    else if (a[0] != '-') scene_path = a;
    else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
  }
  if (passes > 0) {
    if (gpus > 0) { std::fprintf(stderr, "--passes does not combine with --gpus (one frame's samples stay on one GPU)\n"); return 2; }
    const long total = cfg.antialiasing ? (long)cfg.spp_sqrt * (long)cfg.spp_sqrt : 1;
    if (cfg.antialiasing && passes > total) { std::fprintf(stderr, "--passes %ld: the frame has only %ld samples per pixel\n", passes, total); return 2; }
  }
  if (min_spp > 0 && adaptive < 0) { std::fprintf(stderr, "--min-spp goes with --adaptive\n"); return 2; }
  if (adaptive >= 0) {
    if (passes == 0) { std::fprintf(stderr, "--adaptive needs --passes K (the decisions are taken between passes)\n"); return 2; }
    if (cfg.integrator != P3D_PATHTRACE) { std::fprintf(stderr, "--adaptive is for --pathtrace (not --whitted)\n"); return 2; }
    if (gpus > 0) { std::fprintf(stderr, "--adaptive does not combine with --gpus\n"); return 2; }
    const long total = (long)cfg.spp_sqrt * (long)cfg.spp_sqrt;
    if (min_spp > total) { std::fprintf(stderr, "--min-spp %ld: the frame has only %ld samples per pixel\n", min_spp, total); return 2; }
    if (min_spp == 0) min_spp = std::max(2L, std::min(16L, total));
  }
  if ((denoise_iter >= 0 || feature_spp >= 0) && denoise_out.empty()) {
    std::fprintf(stderr, "%s goes with --denoise\n", denoise_iter >= 0 ? "--denoise-iter" : "--feature-spp");
    return 2;
  }
  if (!denoise_out.empty()) {
    if (cfg.integrator != P3D_PATHTRACE) { std::fprintf(stderr, "--denoise is for --pathtrace (not --whitted)\n"); return 2; }
    if (gpus > 0) { std::fprintf(stderr, "--denoise does not combine with --gpus\n"); return 2; }
    if (!cfg.antialiasing) { std::fprintf(stderr, "--denoise needs --aa 1 (a path-traced frame with samples to filter)\n"); return 2; }
    if (feature_spp > (long)cfg.spp_sqrt * (long)cfg.spp_sqrt) {
      std::fprintf(stderr, "--feature-spp %ld: the frame has only %ld samples per pixel\n", feature_spp, (long)cfg.spp_sqrt * (long)cfg.spp_sqrt);
      return 2;
    }
  }
  if (orbit_set && frames == 0) { std::fprintf(stderr, "--orbit goes with --frames\n"); return 2; }
  if (temporal) {
    if (frames == 0) { std::fprintf(stderr, "--temporal needs --frames N (it integrates a sequence)\n"); return 2; }
    if (denoise_out.empty()) { std::fprintf(stderr, "--temporal needs --denoise FILE (its output goes through the variance-term filter)\n"); return 2; }
  }
  if (frames > 0) {
    if (passes > 0) { std::fprintf(stderr, "--frames does not combine with --passes (every frame is one render call)\n"); return 2; }
    if (gpus > 0) { std::fprintf(stderr, "--frames does not combine with --gpus\n"); return 2; }
  }
  if (scene_path.empty()) {  // main.cpp:968-980: prompt for a name under P3D_Scenes/
    std::string name;
    std::cout << "Input the Scene Name: ";
    if (!(std::cin >> name)) return 2;
    scene_path = "P3D_Scenes/" + name;
  }

  p3d_host_scene* hs = nullptr;
  if (p3d_host_scene_load(scene_path.c_str(), load_flags, &hs) != P3D_OK) {
    std::printf("\nError opening P3F file.\n");
    return die("load");
  }
  if (res_w > 0 && p3d_host_scene_set_resolution(hs, res_w, res_h) != P3D_OK) return die("resolution");
  if (cfg.soft_shadows && !cfg.antialiasing &&  // main.cpp:725-745
      p3d_host_scene_replicate_lights(hs, cfg.spp_sqrt, cfg.light_side) != P3D_OK)
    return die("lights");

  const auto t_build0 = std::chrono::high_resolution_clock::now();
  const p3d_scene_desc* desc = nullptr;
  if (p3d_host_scene_desc(hs, cfg.accel == P3D_ACCEL_BVH && !device_bvh, cfg.accel == P3D_ACCEL_GRID && !device_grid, &desc) != P3D_OK) return die("flatten");
  const int W = desc->camera.res_x, H = desc->camera.res_y;
  std::printf("\nResolutionX = %d  ResolutionY= %d.\n", W, H);  // main.cpp:986
  if (gpus > 0) {  // several GPUs of this node (or one, through the same path): stripes + one RCCL gather
    if (!skybox_dir.empty()) { std::fprintf(stderr, "--gpus with --skybox is not wired up in this front end\n"); return 2; }
    std::vector<uint8_t> img((size_t)3 * W * H);
    double secs = 0;
    if (const int rc = render_multi_gpu(desc, device_bvh, device_grid, cfg, gpus, verify, img, &secs)) return rc;
    std::printf("Drawing finished!\n\nDone: %.2f (sec)\n", secs);
    std::printf("%d GPU(s): stripes of %d rows, one ncclGather of %zu bytes per GPU; second frame %.3f ms (render + gather)\n", gpus, kStripeRows,
                (size_t)3 * W * (H / gpus), secs * 1e3);
    const bool ppm = out.size() > 4 && out.compare(out.size() - 4, 4, ".ppm") == 0;
    if (!(ppm ? save_ppm(out, img, W, H) : save_png(out, img, W, H))) { std::printf("Error saving Image file\n"); return 1; }
    std::printf("Image file created\n");
    p3d_host_scene_destroy(hs);
    return 0;
  }
  p3d_scene* scene = nullptr;
  if (device_grid || (device_bvh && cfg.accel == P3D_ACCEL_BVH)) {  // (a device-built grid needs the scene kind that keeps its boxes on the GPU)
    float build_ms = 0;
    if (p3d_scene_create_device_bvh(desc, device, &scene, &build_ms) != P3D_OK) return die("scene_create_device_bvh");
    std::printf("BVH built on the GPU in %.2f ms\n", build_ms);
    if (device_grid) {
      if (p3d_scene_build_grid(scene, &build_ms) != P3D_OK) return die("scene_build_grid");
      std::printf("Grid built on the GPU in %.2f ms\n", build_ms);
    }
  } else if (p3d_scene_create(desc, device, &scene) != P3D_OK) {
    return die("scene_create");
  }
  if (skybox_dir.empty() && p3d_host_scene_has_skybox(hs)) {  // `env <dir>` in the scene file, faces found as PPMs: SKYBOX true (constants.h:30)
    if (p3d_host_scene_bind_device(hs, scene) != P3D_OK) return die("skybox");
    cfg.skybox = 1;
  }
  if (!skybox_dir.empty()) {  // Scene::LoadSkybox (scene.cpp:329-377) + SKYBOX true (constants.h:30)
    if (p3d_host_scene_load_skybox(hs, skybox_dir.c_str()) != P3D_OK) return die("skybox");
    if (p3d_host_scene_bind_device(hs, scene) != P3D_OK) return die("skybox");
    cfg.skybox = 1;
  }
  const auto t_build1 = std::chrono::high_resolution_clock::now();
  if (frames > 0) {
    const int rc = render_frames(hs, scene, cfg, frames, orbit, temporal, out, denoise_out, denoise_iter, feature_spp, device);
    p3d_scene_destroy(scene);
    p3d_host_scene_destroy(hs);
    return rc;
  }

  std::vector<uint8_t> img((size_t)3 * W * H);
  const bool denoise = !denoise_out.empty();
  std::vector<float> lin(denoise ? (size_t)3 * W * H : 0), var;  // --denoise: the final frame's linear rgb (and variance)
  p3d_tile tile{0, 0, W, H, 0, 1};
  p3d_stats st{};
  cfg.collect_stats = 1;
  const bool ppm = out.size() > 4 && out.compare(out.size() - 4, 4, ".ppm") == 0;
  const auto t0 = std::chrono::high_resolution_clock::now();
  if (passes > 0 && adaptive >= 0) {  // adaptive: converged pixels stop taking samples (p3d_adaptive)
    p3d_adaptive* ad = nullptr;
    const p3d_adaptive_params prm{adaptive, (uint32_t)min_spp, {0, 0}};
    if (const int rc = p3d_adaptive_create(scene, &cfg, &tile, &prm, &ad); rc != P3D_OK) {
      if (rc != P3D_ERR_UNSUPPORTED && rc != P3D_ERR_INVALID) return die("adaptive_create");
      std::fprintf(stderr, "--adaptive: %s\n", p3d_last_error());
      return 2;
    }
    const uint32_t total = cfg.spp_sqrt * cfg.spp_sqrt;
    for (long k = 0; k < passes; ++k) {
      const uint32_t n = (uint32_t)(total / passes) + ((long)(total % passes) > k ? 1u : 0u);
      p3d_stats ps{};
      uint32_t active = 0;
      const auto p0 = std::chrono::high_resolution_clock::now();
      if (p3d_adaptive_render(ad, n, denoise ? lin.data() : nullptr, nullptr, img.data(), nullptr, &ps) != P3D_OK) return die("render");
      if (p3d_adaptive_active_pixels(ad, &active) != P3D_OK) return die("adaptive_active_pixels");
      const double pass_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - p0).count();
      std::printf("pass %ld/%ld: %u of %u samples done, %u of %d pixels active, %.3f ms\n", k + 1, passes,
                  p3d_adaptive_samples_done(ad), total, active, W * H, pass_ms);
      std::fflush(stdout);
      st.rays_primary += ps.rays_primary; st.rays_shadow += ps.rays_shadow; st.rays_reflect += ps.rays_reflect;
      st.rays_refract += ps.rays_refract; st.rays_bounce += ps.rays_bounce; st.rays_light += ps.rays_light;
      st.kernel_ms += ps.kernel_ms;
      if (!(ppm ? save_ppm(out, img, W, H) : save_png(out, img, W, H))) {
        std::printf("Error saving Image file\n");
        return 1;
      }
      if (active == 0) break;  // every pixel has converged: later passes would change nothing
    }
    if (denoise) {
      var.resize((size_t)W * H);
      if (p3d_denoise_variance(ad, var.data()) != P3D_OK) return die("denoise_variance");
    }
    p3d_adaptive_destroy(ad);
  } else if (passes > 0) {  // progressive: the image refines pass by pass (p3d_accum), --out rewritten after every pass
    p3d_accum* acc = nullptr;
    if (const int rc = p3d_accum_create(scene, &cfg, &tile, &acc); rc != P3D_OK) {
      if (rc != P3D_ERR_UNSUPPORTED) return die("accum_create");
      std::fprintf(stderr, "--passes: %s\n", p3d_last_error());
      return 2;
    }
    const uint32_t total = cfg.spp_sqrt * cfg.spp_sqrt;
    for (long k = 0; k < passes; ++k) {
      const uint32_t n = (uint32_t)(total / passes) + ((long)(total % passes) > k ? 1u : 0u);
      p3d_stats ps{};
      const auto p0 = std::chrono::high_resolution_clock::now();
      if (p3d_accum_render(acc, n, denoise ? lin.data() : nullptr, nullptr, img.data(), &ps) != P3D_OK) return die("render");
      const double pass_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - p0).count();
      std::printf("pass %ld/%ld: %u of %u samples done, %.3f ms\n", k + 1, passes, p3d_accum_samples_done(acc), total, pass_ms);
      std::fflush(stdout);
      st.rays_primary += ps.rays_primary; st.rays_shadow += ps.rays_shadow; st.rays_reflect += ps.rays_reflect;
      st.rays_refract += ps.rays_refract; st.rays_bounce += ps.rays_bounce; st.rays_light += ps.rays_light;
      st.kernel_ms += ps.kernel_ms;
      if (!(ppm ? save_ppm(out, img, W, H) : save_png(out, img, W, H))) {
        std::printf("Error saving Image file\n");
        return 1;
      }
    }
    p3d_accum_destroy(acc);
  } else if (p3d_render_tile(scene, &cfg, &tile, denoise ? lin.data() : nullptr, nullptr, img.data(), &st) != P3D_OK) {
    return die("render");
  }
  const auto t1 = std::chrono::high_resolution_clock::now();
  std::printf("Drawing finished!\n");
  const double secs = std::chrono::duration<double>(t1 - t0).count();
  const uint64_t rays = st.rays_primary + st.rays_shadow + st.rays_reflect + st.rays_refract + st.rays_bounce + st.rays_light;
  std::printf("\nDone: %.2f (sec)\n", secs);  // main.cpp:1012
  std::printf("accel build + upload %.3f s; kernel %.3f ms; %llu rays; %.1f Mrays/s (kernel)\n",
              std::chrono::duration<double>(t_build1 - t_build0).count(), st.kernel_ms, (unsigned long long)rays,
              st.kernel_ms > 0 ? rays / (st.kernel_ms * 1e3) : 0.0);
  if (!(ppm ? save_ppm(out, img, W, H) : save_png(out, img, W, H))) {
    std::printf("Error saving Image file\n");
    return 1;
  }
  std::printf("Image file created\n");
  if (denoise) {  // the final frame through the a-trous filter, over the primary rays' feature buffers
    const auto d0 = std::chrono::high_resolution_clock::now();
    std::vector<float> nd((size_t)4 * W * H), ac((size_t)4 * W * H);
    if (p3d_render_features(scene, &cfg, &tile, feature_spp > 0 ? (uint32_t)feature_spp : 0u, nd.data(), ac.data()) != P3D_OK)
      return die("render_features");
    p3d_denoise_params prm;
    p3d_denoise_params_default(&prm);
    if (denoise_iter >= 0) prm.iterations = (uint32_t)denoise_iter;
    prm.gamma = cfg.gamma;
    p3d_denoiser* dn = nullptr;
    if (p3d_denoiser_create(device, W, H, &dn) != P3D_OK) return die("denoiser_create");
    std::vector<uint8_t> den((size_t)3 * W * H);
    if (p3d_denoise(dn, &prm, lin.data(), var.empty() ? nullptr : var.data(), nd.data(), ac.data(), nullptr, den.data()) != P3D_OK)
      return die("denoise");
    p3d_denoiser_destroy(dn);
    std::printf("denoised: %u iterations%s, features and filter %.3f ms\n", prm.iterations, var.empty() ? "" : " (adaptive variance)",
                std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - d0).count());
    const bool dppm = denoise_out.size() > 4 && denoise_out.compare(denoise_out.size() - 4, 4, ".ppm") == 0;
    if (!(dppm ? save_ppm(denoise_out, den, W, H) : save_png(denoise_out, den, W, H))) {
      std::printf("Error saving Image file\n");
      return 1;
    }
    std::printf("Denoised image file created\n");
  }
  p3d_scene_destroy(scene);
  p3d_host_scene_destroy(hs);
  return 0;
}

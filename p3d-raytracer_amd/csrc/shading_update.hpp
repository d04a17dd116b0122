// shading_update.hpp — the device half of p3d_scene_set_shading_device: material and light records from the CALLER's device
// memory into the scene's blob, and the rules both forms of the update share with assemble_blob (capi_scene_layout.hpp).
//
// One thread per material of the SCENE, not of the range: the Ks == 0 flag in the .w of a material's fourth float4 depends on
// every light's colour, so a change of one light can flip the flag of every material.  Every workgroup derives lights_plain
// itself, from the EFFECTIVE lights - light i is the caller's record if it lies in the range and the blob's otherwise - so no
// thread reads what another writes in the same launch: a material is read and written by its own thread alone, a blob light
// inside the range is written (by one thread) and read by none, one outside is read and never written.  No grid-wide order is
// needed.  A few hundred bytes per material, no reuse: the launch is the cost.
//
// The host cannot see the values and its facts must stay true (DESIGN.md "Shading updates"): a material whose new record
// would flip its own emissive predicate or its own transmissive-and-reflective predicate, against the record it replaces,
// keeps its four float4 but for the flag.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace p3d {
namespace shade {

constexpr uint32_t kThreads = 256;  // a workgroup: four waves
// The bit the kernel raises in the scene's status word when it skips a material (upd::kStatusRefitSkipped and
// upd::kStatusPoseSkipped are below it); the counts are in the scene's counter block
constexpr uint32_t kStatusShadingSkipped = 128u;

// ---- the rules, one spelling for assemble_blob's arithmetic on the host and on the device ----
__host__ __device__ inline bool plain(float c) { return c >= 0.0f && c <= 1e15f; }
__host__ __device__ inline bool light_plain(float r, float g, float b) { return plain(r) && plain(g) && plain(b); }
// The .w of a material's fourth float4 (assemble_blob): its specular term is provably an exact, finite zero
__host__ __device__ inline float pow_flag(bool lights_plain, float specular, float shine, float sr, float sg, float sb) {
  return (lights_plain && specular == 0.0f && shine >= 0.0f && shine < INFINITY && plain(sr) && plain(sg) && plain(sb)) ? 1.0f : 0.0f;
}
// A sphere of this material is in the emitter list: float32, added in assemble_blob's order
__host__ __device__ inline bool emissive(float e0, float e1, float e2) { return e0 + e1 + e2 > 0; }
// The material makes a LITERAL frame trace zero-weight reflections (create_impl)
__host__ __device__ inline bool ghost(float transmittance, float reflection) { return transmittance != 0 && reflection > 0; }

// mats: 4 float4 per material of the scene, lights: 2 per light.  new_mats: 16 floats per material of [first_mat, first_mat +
// n_new_mats), new_lights: 8 per light of [first_light, first_light + n_new_lights), read as scalar floats: the caller's memory
// is 4-byte aligned and no more.  The host has checked both ranges against n_mats and n_lights: no read of new_mats outside
// [0, 16 n_new_mats), none of new_lights outside [0, 8 n_new_lights), no access of mats or lights outside the scene's counts.
// counters[0]: materials skipped for the emissive predicate, counters[1]: for the transmissive-and-reflective one; the scene's
// own block, added to and never cleared here, one atomic per wave after a ballot; *status takes kStatusShadingSkipped with
// them.  The grid is ceil(n_mats / kThreads) workgroups, at least one (a scene without materials may have lights).
__global__ __launch_bounds__(kThreads) void set_shading(float4* mats, uint32_t n_mats, float4* lights, uint32_t n_lights, const float* new_mats,
                                                        uint32_t first_mat, uint32_t n_new_mats, const float* new_lights, uint32_t first_light,
                                                        uint32_t n_new_lights, uint32_t* counters, uint32_t* status) {
  __shared__ uint32_t wave_plain[kThreads / 64];
  const uint32_t tid = threadIdx.x;
  // lights_plain over the effective lights: a stride loop per thread (0 lights: plain; more lights than the workgroup has
  // threads: several trips), an AND over the wave, an AND over the workgroup's waves
  bool mine = true;
  for (uint32_t i = tid; i < n_lights; i += kThreads) {
    const uint32_t k = i - first_light;  // (wraps below the range: >= n_new_lights then, as first_light + n_new_lights <= n_lights)
    float r, g, b;
    if (i >= first_light && k < n_new_lights) {
      const float* l = new_lights + 8 * (size_t)k;
      r = l[4]; g = l[5]; b = l[6];
    } else {
      const float4 c = lights[2 * (size_t)i + 1];
      r = c.x; g = c.y; b = c.z;
    }
    mine = mine && light_plain(r, g, b);
  }
  const bool wave_all = __all(mine) != 0;
  if ((tid & 63u) == 0) wave_plain[tid >> 6] = wave_all ? 1u : 0u;
  __syncthreads();
  bool lights_plain = true;
  for (uint32_t w = 0; w < kThreads / 64; ++w) lights_plain = lights_plain && wave_plain[w] != 0u;

  // the material of this thread
  const uint32_t m = blockIdx.x * kThreads + tid;
  bool skip_emissive = false, skip_ghost = false;
  if (m < n_mats) {
    float4* rec = mats + 4 * (size_t)m;
    float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    const uint32_t k = m - first_mat;
    bool write_all = false;
    if (m >= first_mat && k < n_new_mats) {
      const float* f = new_mats + 16 * (size_t)k;
      const float4 n0 = make_float4(f[0], f[1], f[2], f[3]), n1 = make_float4(f[4], f[5], f[6], f[7]);
      const float4 n2 = make_float4(f[8], f[9], f[10], f[11]), n3 = make_float4(f[12], f[13], f[14], 0.f);
      skip_emissive = emissive(n3.x, n3.y, n3.z) != emissive(r3.x, r3.y, r3.z);
      skip_ghost = ghost(n2.y, n2.w) != ghost(r2.y, r2.w);
      if (!skip_emissive && !skip_ghost) {
        r0 = n0; r1 = n1; r2 = n2; r3 = n3;
        write_all = true;
      }
    }
    r3.w = pow_flag(lights_plain, r1.w, r2.x, r1.x, r1.y, r1.z);
    if (write_all) {
      rec[0] = r0;
      rec[1] = r1;
      rec[2] = r2;
    }
    rec[3] = r3;
  }
  const unsigned long long be = __ballot(skip_emissive), bg = __ballot(skip_ghost);
  if ((tid & 63u) == 0 && (be | bg)) {
    if (be) atomicAdd(&counters[0], (uint32_t)__popcll(be));
    if (bg) atomicAdd(&counters[1], (uint32_t)__popcll(bg));
    atomicOr(status, kStatusShadingSkipped);
  }

  // the lights of the range, by the grid's threads in a stride loop (there may be more of them than threads)
  const uint32_t threads = gridDim.x * kThreads;
  for (uint32_t k = blockIdx.x * kThreads + tid; k < n_new_lights; k += threads) {
    const float* l = new_lights + 8 * (size_t)k;
    float4* dst = lights + 2 * ((size_t)first_light + k);
    dst[0] = make_float4(l[0], l[1], l[2], 0.f);
    dst[1] = make_float4(l[4], l[5], l[6], 0.f);
  }
}

}  // namespace shade
}  // namespace p3d

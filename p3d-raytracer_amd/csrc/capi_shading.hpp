// capi_shading.hpp — the lights and materials of a live scene (include/p3d_shading.h): the waiting forms from host memory,
// the readbacks, and the stream form from device memory, whose kernel is shading_update.hpp's.  Every scene takes them: the
// accelerators do not depend on a material or a light.
#pragma once
#include "capi_update.hpp"

namespace {

static_assert(sizeof(p3d_material) == 4 * sizeof(float4) && sizeof(p3d_light) == 2 * sizeof(float4), "a material is four float4 of the blob, a light two");

// The waits of a call that reads or rewrites the tables: enqueued frames and stream updates read and write them
int shading_wait(p3d_scene* s) {
  P3D_HIP(hipSetDevice(s->device));
  if (int rc = p3d_scene_join(s, nullptr, 1)) return rc;
  P3D_HIP(hipDeviceSynchronize());
  return P3D_OK;
}

// What the waiting forms share: the device's tables as they are now (a stream form may have changed them: the host keeps no
// copy), `patch` applied to them, every derived fact worked out from the whole tables as assemble_blob and create_impl do,
// one upload each, and the memos of earlier frames dropped.  The device is idle from shading_wait on.
template <class Patch>
int rewrite_shading(p3d_scene* s, Patch&& patch) {
  if (int rc = shading_wait(s)) return rc;
  DevScene& v = s->dev;
  std::vector<float4> mats((size_t)4 * v.n_mats), lights((size_t)2 * v.n_lights);
  if (!mats.empty()) P3D_HIP(hipMemcpy(mats.data(), s->d_blob + s->off_mats, mats.size() * sizeof(float4), hipMemcpyDeviceToHost));
  if (!lights.empty()) P3D_HIP(hipMemcpy(lights.data(), s->d_blob + s->off_lights, lights.size() * sizeof(float4), hipMemcpyDeviceToHost));
  patch(mats, lights);
  bool lights_plain = true;
  for (uint32_t i = 0; i < v.n_lights; ++i) {
    const float4 c = lights[2 * (size_t)i + 1];
    lights_plain = lights_plain && shade::light_plain(c.x, c.y, c.z);
  }
  bool ghosts = false;
  for (uint32_t i = 0; i < v.n_mats; ++i) {
    const float4 r1 = mats[4 * (size_t)i + 1], r2 = mats[4 * (size_t)i + 2];
    mats[4 * (size_t)i + 3].w = shade::pow_flag(lights_plain, r1.w, r2.x, r1.x, r1.y, r1.z);
    ghosts = ghosts || shade::ghost(r2.y, r2.w);
  }
  std::vector<uint32_t> emitters;  // emissive spheres in object order
  for (uint32_t i = 0; i < v.n_objs; ++i) {
    const float4 e = mats[4 * (size_t)(s->obj_tm[i] >> 8) + 3];
    if (shade::emissive(e.x, e.y, e.z) && (s->obj_tm[i] & 0xffu) == P3D_PRIM_SPHERE) emitters.push_back(i);
  }
  if (emitters.size() > s->emitters_cap) {  // before anything changes: a list that does not fit leaves the scene as it was
    uint32_t* grown = nullptr;
    P3D_HIP(hipMalloc((void**)&grown, emitters.size() * 4));
    if (s->d_emitters) (void)hipFree(s->d_emitters);
    s->d_emitters = grown;
    s->emitters_cap = (uint32_t)emitters.size();
  }
  // from here on the scene changes
  hipError_t e = hipSuccess;
  if (!mats.empty()) e = hipMemcpy(s->d_blob + s->off_mats, mats.data(), mats.size() * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess && !lights.empty()) e = hipMemcpy(s->d_blob + s->off_lights, lights.data(), lights.size() * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess && !emitters.empty()) e = hipMemcpy(s->d_emitters, emitters.data(), emitters.size() * 4, hipMemcpyHostToDevice);
  v.emitters = s->d_emitters;
  v.n_emitters = (uint32_t)emitters.size();
  s->zero_weight_reflections = ghosts;
  // whatever happened, what earlier frames worked out for the old records is void
  ++s->geom_gen;
  drop_schedules(s);
  s->ho_chain_key.clear();
  if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("shading update: ") + hipGetErrorString(e));
  return P3D_OK;
}

// What the four host-memory calls refuse, in this order
int shading_range_refused(const p3d_scene* s, const std::string& pre, uint32_t first, uint32_t n, uint32_t count, const void* array, const char* noun) {
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  if ((uint64_t)first + n > count)
    return fail(P3D_ERR_INVALID, pre + noun + " " + std::to_string(first) + " .. " + std::to_string((uint64_t)first + n) + " end behind the scene's " + std::to_string(count));
  if (n && !array) return fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_scene_set_materials(p3d_scene* s, uint32_t first, uint32_t n, const p3d_material* materials) {
  if (int rc = shading_range_refused(s, "p3d_scene_set_materials: ", first, n, s ? s->dev.n_mats : 0u, materials, "materials")) return rc;
  if (n == 0) return P3D_OK;
  return rewrite_shading(s, [&](std::vector<float4>& mats, std::vector<float4>&) {
    for (uint32_t i = 0; i < n; ++i) {
      const p3d_material& m = materials[i];
      float4* rec = mats.data() + 4 * ((size_t)first + i);
      rec[0] = make_float4(m.diff_color[0], m.diff_color[1], m.diff_color[2], m.diffuse);
      rec[1] = make_float4(m.spec_color[0], m.spec_color[1], m.spec_color[2], m.specular);
      rec[2] = make_float4(m.shine, m.transmittance, m.refr_index, m.reflection);
      rec[3] = make_float4(m.emission[0], m.emission[1], m.emission[2], 0.f);
    }
  });
}

int p3d_scene_set_lights(p3d_scene* s, uint32_t first, uint32_t n, const p3d_light* lights_in) {
  if (int rc = shading_range_refused(s, "p3d_scene_set_lights: ", first, n, s ? s->dev.n_lights : 0u, lights_in, "lights")) return rc;
  if (n == 0) return P3D_OK;
  return rewrite_shading(s, [&](std::vector<float4>&, std::vector<float4>& lights) {
    for (uint32_t i = 0; i < n; ++i) {
      const p3d_light& l = lights_in[i];
      lights[2 * ((size_t)first + i)] = make_float4(l.position[0], l.position[1], l.position[2], 0.f);
      lights[2 * ((size_t)first + i) + 1] = make_float4(l.color[0], l.color[1], l.color[2], 0.f);
    }
  });
}

int p3d_scene_materials(p3d_scene* s, uint32_t first, uint32_t n, p3d_material* out) {
  if (int rc = shading_range_refused(s, "p3d_scene_materials: ", first, n, s ? s->dev.n_mats : 0u, out, "materials")) return rc;
  if (n == 0) return P3D_OK;
  if (int rc = shading_wait(s)) return rc;
  P3D_HIP(hipMemcpy(out, s->d_blob + s->off_mats + 4 * (size_t)first, (size_t)n * sizeof(p3d_material), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) out[i].reserved = 0.0f;  // (the blob keeps the Ks == 0 flag there)
  return P3D_OK;
}

int p3d_scene_lights(p3d_scene* s, uint32_t first, uint32_t n, p3d_light* out) {
  if (int rc = shading_range_refused(s, "p3d_scene_lights: ", first, n, s ? s->dev.n_lights : 0u, out, "lights")) return rc;
  if (n == 0) return P3D_OK;
  if (int rc = shading_wait(s)) return rc;
  P3D_HIP(hipMemcpy(out, s->d_blob + s->off_lights + 2 * (size_t)first, (size_t)n * sizeof(p3d_light), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) out[i].reserved0 = out[i].reserved1 = 0.0f;
  return P3D_OK;
}

int p3d_scene_set_shading_device(p3d_scene* s, uint32_t first_material, uint32_t n_materials, const void* d_materials, uint32_t first_light,
                                 uint32_t n_lights, const void* d_lights, void* hip_stream) {
  const std::string pre = "p3d_scene_set_shading_device: ";
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  const DevScene& v = s->dev;
  // pointers first, as p3d_scene_pose_device checks them: host memory is refused whatever else the call says
  if ((n_materials && !d_materials) || (n_lights && !d_lights)) return fail(P3D_ERR_INVALID, pre + "null pointer with a count");
  if (((uintptr_t)d_materials | (uintptr_t)d_lights) & 3u) return fail(P3D_ERR_INVALID, pre + "d_materials and d_lights must be 4-byte aligned");
  P3D_HIP(hipSetDevice(s->device));
  if (n_materials)
    if (int rc = device_buffer_usable(s, d_materials, (size_t)64 * n_materials, pre + "d_materials")) return rc;
  if (n_lights)
    if (int rc = device_buffer_usable(s, d_lights, (size_t)32 * n_lights, pre + "d_lights")) return rc;
  if ((uint64_t)first_material + n_materials > v.n_mats)
    return fail(P3D_ERR_INVALID, pre + "materials " + std::to_string(first_material) + " .. " + std::to_string((uint64_t)first_material + n_materials) +
                                     " end behind the scene's " + std::to_string(v.n_mats));
  if ((uint64_t)first_light + n_lights > v.n_lights)
    return fail(P3D_ERR_INVALID, pre + "lights " + std::to_string(first_light) + " .. " + std::to_string((uint64_t)first_light + n_lights) +
                                     " end behind the scene's " + std::to_string(v.n_lights));
  if (n_materials == 0 && n_lights == 0) return P3D_OK;
  if (!s->shading_skipped.p) {  // the scene's first such call: the counter block, zeroed before the kernel can add to it
    if (int rc = s->shading_skipped.ensure(2 * sizeof(uint32_t))) return rc;
    P3D_HIP(hipMemset(s->shading_skipped.p, 0, 2 * sizeof(uint32_t)));
    P3D_HIP(hipStreamSynchronize(nullptr));
  }
  hipStream_t st = (hipStream_t)hip_stream;
  if (int rc = wait_for_tail(s, st)) return rc;  // the previous frame's tail reads the records (p3d_scene_set_tail_stream)
  // from here on the scene changes
  const uint32_t grid = std::max(1u, (v.n_mats + shade::kThreads - 1) / shade::kThreads);
  hipLaunchKernelGGL(shade::set_shading, dim3(grid), dim3(shade::kThreads), 0, st, s->d_blob + s->off_mats, v.n_mats, s->d_blob + s->off_lights, v.n_lights,
                     (const float*)d_materials, first_material, n_materials, (const float*)d_lights, first_light, n_lights,
                     (uint32_t*)s->shading_skipped.p, s->d_status);
  const hipError_t e = hipGetLastError();
  // the old records' memos are void, as after finish_stream_refit; nothing here allocates, frees, waits or reads back
  ++s->geom_gen;
  void_schedules(s);
  s->ho_chain_key.clear();
  if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, pre + "update: " + hipGetErrorString(e));
  return P3D_OK;
}

}  // extern "C"

/*
 * p3d_radiance.h - part of the C-ABI of libp3d.so, included by p3d.h (include that; including this file alone works too).
 * Radiance along rays from device memory (Whitted and path-traced) and the rays of a camera: the entry points added to the boundary after p3d.h's own
 * list was closed.  Same conventions as p3d.h: int return codes (P3D_OK or a P3D_ERR_*), p3d_last_error for the message.
 */
#ifndef P3D_RADIANCE_H
#define P3D_RADIANCE_H

#include "p3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * WHAT A RAY SEES: the Whitted radiance along rays held in device memory - a fisheye or panoramic view, a stereo pair, a light
 * or reflection probe at a point, a batch of training rays, a pixel shaded again after a simulation step - without a copy of
 * the shading chain outside the library.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 *
 * rgb[i] is the colour rayTracing(ray i, max_depth, 1.0, 0, 0) returns (main.cpp:92-309, called as main.cpp:808-811 calls it
 * for a pixel): closest hit, one shadow feeler per light and Blinn-Phong, then the reflected or refracted ray, max_depth
 * levels deep, folded bottom-up with the clamp of every level.  The ray starts as a primary ray: ior_1 = 1, outside every
 * object, on an EMPTY hit_stack, which its own chain then carries from query to query, feelers included (bvh.cpp:86,322) -
 * what a pixel of a P3D_STACK_PER_PIXEL frame with antialiasing = 0, soft_shadows = 0 and debug_view = 0 does.  For a ray that
 * equals such a pixel's primary ray (p3d_camera_rays_device below gives them) rgb and hit_id are that frame's floats, bit for
 * bit, for every accel.  There is no pixel order among a caller's rays, hence no P3D_STACK_LITERAL form; no anti-aliasing,
 * soft shadows or lens sampling per ray; every ray of a call has the same depth and starts outside every medium.
 *   d_origin, d_direction : n*3 float32.  The direction is used as given, as in the other ray queries; the formulas of the
 *                           chain (reflection, refraction, the Blinn half vector) assume unit length.
 *   max_depth             : 0 .. P3D_RADIANCE_MAX_DEPTH; 0 is local shading alone.
 *   flags                 : 0, or P3D_RADIANCE_SKYBOX: a ray that leaves the scene returns the cubemap's texel
 *                           (Scene::GetSkyboxColor, scene.cpp:379-457) instead of the background colour, as p3d_config.skybox.
 *   d_rgb    : n*3 float32, required ; d_hit_id : n int32, the object of ray i's first closest hit or -1, may be NULL.
 * P3D_ACCEL_NONE, P3D_ACCEL_GRID and P3D_ACCEL_BVH are all taken.  The scene is traversed from global memory whatever its
 * size; the records of the levels live in the workgroup's LDS (max_depth x 1 KB per wave), so the call needs no scratch.
 *
 * Stream, buffers, tail join and spill area as p3d_trace_closest_device: one kernel on `hip_stream`, no wait, no allocation
 * once the spill area is large enough (its worst case is a frame's: (lights + 1) x the tree's depth entries per ray); behind
 * p3d_scene_refit_device or p3d_scene_pose_device on the same stream it sees the moved geometry.  Refused, nothing enqueued
 * and nothing written: P3D_ERR_INVALID for a null scene, an unknown accel or one the scene was created without, max_depth
 * outside 0 .. P3D_RADIANCE_MAX_DEPTH, an unknown flag, P3D_RADIANCE_SKYBOX on a scene without a cubemap (as p3d_skybox_color
 * refuses), with n > 0 a null d_origin, d_direction or d_rgb, a misaligned pointer, host memory, memory of another device or a
 * buffer too short; P3D_ERR_UNSUPPORTED for a grid over an empty scene; P3D_ERR_CAPACITY where n x the stack's worst case does
 * not fit the spill area's 32-bit offsets (split the batch).  n = 0 returns P3D_OK.
 */
#define P3D_RADIANCE_MAX_DEPTH 16u
#define P3D_RADIANCE_SKYBOX 1u
int p3d_trace_radiance_device(p3d_scene* scene, uint32_t accel, uint32_t n,
                              const float* d_origin, const float* d_direction, int32_t max_depth, uint32_t flags,
                              float* d_rgb /* n*3 */, int32_t* d_hit_id /* n, may be NULL */, void* hip_stream);
/*
 * The PRIMARY RAYS of a camera, in device memory: Camera::PrimaryRay (camera.h:65-82) of the centre (x + 0.5, y + 0.5) of every
 * pixel of `tile`, as the frame loop casts them without anti-aliasing (main.cpp:805-808) - the very floats the frame kernels
 * trace.  The starting point a caller distorts, offsets or subsamples before p3d_trace_radiance_device.
 *   camera : NULL = the scene's current camera; otherwise a camera of the scene's resolution (p3d_camera_look_at), which the
 *            scene does not keep.   tile : NULL = the whole frame; stripes as in p3d_render_tile.
 *   d_origin, d_direction : w*h*3 float32 each on the scene's device, 4-byte aligned, in the row order of p3d_render_tile's
 *            output for that tile (row 0 = image row y0).  The origin of every ray is the eye.
 * One kernel on `hip_stream`, no wait and no allocation.  Refused, nothing enqueued: P3D_ERR_INVALID for a null scene, a scene
 * without a camera, a camera of another resolution or with a non-finite field or w, h, plane_dist <= 0, a tile outside the
 * image, a null or misaligned buffer, host memory, memory of another device or a buffer too short; P3D_ERR_UNSUPPORTED for a
 * lens camera (aperture != 0): its rays (camera.h:84-115) need the sampler.
 */
int p3d_camera_rays_device(p3d_scene* scene, const p3d_camera* camera /* NULL: the scene's */,
                           const p3d_tile* tile /* NULL: the whole frame */, float* d_origin, float* d_direction,
                           void* hip_stream);

/*
 * WHAT A RAY SEES, PATH-TRACED: the estimate of Radiance (main.cpp:313-516) along rays held in device memory - emitters sampled
 * explicitly, diffuse inter-reflection, mirrors, glass that forks on its first two bounces, Russian roulette from the fifth -
 * for a fisheye view, an irradiance or reflection probe, a batch of training rays, a light-map texel.  Detected by the symbols.
 *
 * rgb[i] is the SUM, over s = sample_begin .. sample_begin + samples - 1 and added in that order, of what Radiance(ray i,
 * max_depth, ...) returns for ray i as a primary ray; every sample starts on a cleared stack, as a sample of a pixel does.
 * The sum starts from 0, with P3D_PATH_ACCUMULATE from what d_rgb[i] holds (the way a later pass of p3d_accum goes on from its
 * running sum).  Nothing is divided: the caller divides by the samples it asked for.  A ray that leaves the scene sees the
 * background colour, with P3D_RADIANCE_SKYBOX the cubemap's texel.  hit_id[i] is the object ray i hits first, or -1 (the ray
 * is the same in every sample; the call's first sample names it).  No debug view, no per-ray depth or seed, no adaptive stop;
 * every ray starts outside every medium.
 *   max_depth : 0 .. 1024, as in a path-traced frame (Russian roulette sets in at the fifth bounce).
 *   d_rng == NULL : sample s of ray i draws from the stream a frame seeds for (pixel, sample) = (i, s) with `seed`
 *                   (p3d_config.seed): the frame's rule with the ray index in the pixel's place.
 *   d_rng given   : n*2 uint64 {state, inc} on the scene's device, 8-byte aligned.  Ray i draws ALL its samples from the one
 *                   PCG stream at d_rng[2i], d_rng[2i+1]; the stream goes on from sample to sample and is written back when
 *                   the ray is done.  seed and sample_begin then only number the samples.
 *   flags : 0 or any of P3D_RADIANCE_SKYBOX, P3D_PATH_ACCUMULATE.
 * With the rays and states of p3d_camera_sample_rays_device below, one call per sample s (samples = 1, sample_begin = s,
 * P3D_PATH_ACCUMULATE into an rgb that starts at zero), then rgb / (spp_sqrt * spp_sqrt), is the path-traced frame of that
 * config in every bit, for every accel; the hit_id of the s = 0 call is the frame's.
 *
 * Stream, buffers, tail join and spill area as p3d_trace_closest_device: one kernel on `hip_stream`, no wait, no allocation
 * once the spill area is large enough (its worst case is one traversal's: the path tracer asks closest-hit queries only, which
 * leave the stack empty); behind p3d_scene_refit_device or p3d_scene_pose_device on the same stream it sees the moved geometry.
 * The pending branches of glass live in the workgroup's LDS (6 KB per wave), so the call needs no scratch.  Refused, nothing
 * enqueued and nothing written: P3D_ERR_INVALID for a null scene, an unknown accel or one the scene was created without,
 * max_depth outside 0 .. 1024, samples == 0, sample_begin + samples past 2^32, an unknown flag, P3D_RADIANCE_SKYBOX on a scene
 * without a cubemap, with n > 0 a null d_origin, d_direction or d_rgb, a misaligned pointer, host memory, memory of another
 * device or a buffer too short; P3D_ERR_UNSUPPORTED for a grid over an empty scene; P3D_ERR_CAPACITY where n x the tree's depth
 * does not fit the spill area's 32-bit offsets (split the batch).  n = 0 returns P3D_OK.
 */
#define P3D_PATH_ACCUMULATE 2u
int p3d_trace_path_device(p3d_scene* scene, uint32_t accel, uint32_t n,
                          const float* d_origin, const float* d_direction, int32_t max_depth,
                          uint32_t sample_begin, uint32_t samples, uint64_t seed,
                          uint64_t* d_rng /* n*2 {state, inc}, in/out, may be NULL */, uint32_t flags,
                          float* d_rgb /* n*3 */, int32_t* d_hit_id /* n, may be NULL */, void* hip_stream);
/*
 * The SAMPLE RAYS of a camera, in device memory: for every pixel (x, y) of `tile`, in the row order of p3d_render_tile's
 * output, sample `sample` of that pixel as the frame loop casts it (main.cpp:758-787) - the pixel's RNG stream of that sample,
 * seeded with cfg->seed as a frame seeds it, the jittered or tent-filtered position in cell (sample / spp_sqrt,
 * sample % spp_sqrt) and, with depth_of_field, the lens sample (square or sample_disk) - and, if d_rng is given, the state
 * {state, inc} of that stream AFTER those draws: what the sample's path goes on from (p3d_trace_path_device's d_rng).
 * Reads of cfg: antialiasing, spp_sqrt, sample_mode, depth_of_field, sample_disk, seed.  antialiasing = 0 gives the
 * pixel-centre rays of p3d_camera_rays_device and the freshly seeded state.  A lens camera is taken: with depth_of_field its
 * rays start on the lens (camera.h:84-115), without it they are the pinhole rays a frame traces then.
 *   d_origin, d_direction : w*h*3 float32 each ; d_rng : w*h*2 uint64, 8-byte aligned, may be NULL.
 * One kernel on `hip_stream`, no wait and no allocation.  Refused, nothing enqueued: what p3d_camera_rays_device refuses, but
 * for the lens camera; a null cfg, spp_sqrt == 0 or above 1024, sample >= spp_sqrt * spp_sqrt, an unknown sample_mode, a
 * misaligned d_rng, one in host memory or too short.  (depth_of_field through a camera whose aperture is 0 is not refused: the
 * frames take it too.)
 */
int p3d_camera_sample_rays_device(p3d_scene* scene, const p3d_camera* camera /* NULL: the scene's */,
                                  const p3d_tile* tile /* NULL: the whole frame */, const p3d_config* cfg,
                                  uint32_t sample, float* d_origin, float* d_direction,
                                  uint64_t* d_rng /* w*h*2, may be NULL */, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* P3D_RADIANCE_H */

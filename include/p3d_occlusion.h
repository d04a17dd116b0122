/*
 * p3d_occlusion.h - part of the C-ABI of libp3d.so, included by p3d.h (include that; including this file alone works too).
 * Hemisphere occlusion at points held in device memory.  Same conventions as p3d.h: int return codes (P3D_OK or a P3D_ERR_*),
 * p3d_last_error for the message.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#ifndef P3D_OCCLUSION_H
#define P3D_OCCLUSION_H

#include "p3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * HOW OPEN A SURFACE POINT IS: the share of the hemisphere above it that is free within a distance - ambient occlusion for a
 * preview, sky visibility and a bent normal for light probes and baking, an exposure term for particles and cloth, a
 * per-vertex feature for training code - in one kernel that reads a point and a normal and writes a count, instead of n x
 * samples rays built outside the library, traced with p3d_trace_any_device and reduced.
 *
 * The rays (host/occlusion_rule.hpp, one spelling for the host and the device).  Sample s of point i draws from the PCG stream
 * a frame seeds for (pixel, sample) = (point_offset + i, s) with `seed`, and is the cosine-weighted direction of the path
 * tracer's diffuse bounce (main.cpp:391-405) around w = normal[i] AS GIVEN - the library does not normalise it:
 *   r1 = 2 pi rand_float() ; r2 = rand_float() ; r2s = sqrtf(r2)
 *   u = normalized(cross(|w.x| > 0.1 ? (0,1,0) : (1,0,0), w)) ; v = cross(w, u)
 *   direction = normalized((u cos(r1) r2s + v sin(r1) r2s) + w sqrtf(1 - r2)) ; origin = point[i] + w * bias
 * in float32, with the sine and cosine of the path tracer.  A normal that is zero or not finite gives NaN rays; a NaN ray
 * hits nothing, so every sample of such a point counts as free.
 *
 * A ray is FREE when no object j has intercepts(object j, a fresh copy of the ray, t) && t < max_dist[i]: the segment query
 * of p3d_trace_any_device with d_t_max, word for word (strict; a zero or NaN limit leaves every ray free).  d_max_dist NULL is
 * a limit of +inf through that same query - not the reference's feeler with its restart.
 *   d_unoccluded[i] : the number of samples in [sample_begin, sample_begin + samples) whose ray is free.  The sampling is
 *                     cosine-weighted, so unoccluded / samples is the ambient-occlusion term as it stands.
 *   d_bent[i]       : the float32 sum of the free rays' directions, NOT normalised: the caller divides or normalises.
 * With P3D_OCCLUSION_ACCUMULATE both are added to what the outputs hold: a later call with the next sample_begin continues the
 * estimate.  point_offset numbers point 0 for the streams: a batch split into calls gives the rows of the whole.
 *
 * team: the lanes that share a point.  A point's samples lie on `team` neighbouring lanes of one wavefront (lane l takes
 * samples sample_begin + l, + team, ...): they share an origin, hence the top of the tree; the count is a ballot, the bent
 * normal a butterfly of fixed order over the team - no atomics, so the same call with the same team gives the same bits
 * every time.  The counts do not depend on team; the last bits of d_bent do (the order of the float32 additions).  0: the
 * smallest power of two >= min(samples, 64).
 *
 * P3D_ACCEL_NONE and P3D_ACCEL_BVH; P3D_ACCEL_GRID is P3D_ERR_UNSUPPORTED, as for the segment query.  Stream, buffers, tail
 * join and spill area as p3d_trace_any_device: one kernel on `hip_stream`, no wait, no allocation once the spill area is large
 * enough (n x team lanes x the tree's depth); behind p3d_scene_refit_device or p3d_scene_pose_device on the same stream it
 * sees the moved geometry.  Refused, nothing enqueued and nothing written: P3D_ERR_INVALID for a null scene or params, an
 * unknown accel or one the scene was created without, samples == 0, sample_begin + samples past 2^32, a team that is not 0 or
 * a power of two <= 64, an unknown flag, a bias that is not finite, with n > 0 a null d_point, d_normal or d_unoccluded, a
 * misaligned pointer, host memory, memory of another device or a buffer too short; P3D_ERR_CAPACITY where n x team lanes (or,
 * for the writers, n x samples rows) do not fit 32 bits, or the lanes x the tree's depth the spill area's 32-bit offsets
 * (split the batch).  n = 0 returns P3D_OK.
 */
#define P3D_OCCLUSION_ACCUMULATE 1u
typedef struct p3d_occlusion_params {
  uint64_t seed;
  uint32_t samples;        /* per point in this call, >= 1 */
  uint32_t sample_begin;   /* index of the first one: a later call continues the estimate */
  uint32_t point_offset;   /* index of point 0 for the streams: a split batch gives the rows of the whole */
  uint32_t flags;          /* P3D_OCCLUSION_ACCUMULATE: add to what the outputs hold */
  float    bias;           /* 1e-4f is offsetIntersection's */
  uint32_t team;           /* lanes per point: 0 = the library chooses, else a power of two <= 64 */
} p3d_occlusion_params;    /* 32 bytes */

int p3d_occlusion_device(p3d_scene* scene, uint32_t accel, uint32_t n, const float* d_point, const float* d_normal,
                         const float* d_max_dist /* n, or NULL: no limit */, const p3d_occlusion_params* params,
                         uint32_t* d_unoccluded /* n, required */, float* d_bent /* n*3, may be NULL */, void* hip_stream);
/*
 * The RAYS of the query above, written out: row i * samples + j of d_origin and d_direction is sample sample_begin + j of
 * point i.  What p3d_trace_any_device takes; the check of the fused kernel, and the two-call path it replaces.  One kernel
 * on `hip_stream`, no wait and no allocation; flags and team are checked and not used.
 */
int p3d_occlusion_rays_device(p3d_scene* scene, uint32_t n, const float* d_point, const float* d_normal,
                              const p3d_occlusion_params* params, float* d_origin, float* d_direction /* n*samples*3 each */,
                              void* hip_stream);
/* The same rays on host arrays, bit for bit: no scene and no device needed. */
int p3d_occlusion_rays(uint32_t n, const float* point, const float* normal, const p3d_occlusion_params* params,
                       float* origin, float* direction /* n*samples*3 each */);

#ifdef __cplusplus
}
#endif

#endif /* P3D_OCCLUSION_H */

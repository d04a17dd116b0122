/*
 * p3d_filter.h - part of the C-ABI of libp3d.so, included by p3d.h (include that; including this file alone works too).
 * Nearest-surface queries, sphere sweeps, ray queries and occlusion that leave objects out, per query.  Same conventions as p3d.h: int return codes
 * (P3D_OK or a P3D_ERR_*), p3d_last_error for the message.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#ifndef P3D_FILTER_H
#define P3D_FILTER_H

#include "p3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * QUERIES FROM INSIDE THE SCENE.  A cloth vertex that asks p3d_nearest_device for the nearest surface gets one of its own
 * triangles at distance 0; a particle that is a sphere of the scene, swept along its step, touches itself at T = 0; a vertex of
 * a rigid body finds its own body.  The filtered forms answer for the scene WITHOUT the objects a query names:
 *
 *     a filtered query  ==  the unfiltered query over the scene from which the objects of its filter are removed.
 *
 * A skipped object is never offered: it is not listed, is not the contact and tightens no bound.  Nothing else changes: the
 * per-object rule, the order (d2, object) / (T, object), the limits, the rows behind count, the no-answer values, and under
 * P3D_ACCEL_BVH the cull with its slack (the boxes are those of the whole scene) are p3d_nearest_k_device's and
 * p3d_sweep_sphere_device's.  Object indices keep their meaning: they are the scene's, not those of the thinned scene.
 *
 * Query i has two independent filters; either may be absent:
 *   the skip list  : row i of d_skip, n x n_skip int32 object indices, 0 <= n_skip <= P3D_FILTER_SKIP_MAX.  An entry < 0 or
 *                    >= the object count names nothing (pad a short row with -1); duplicates are allowed.  For a vertex's
 *                    incident triangles, a particle's own sphere.  n_skip = 0: no list, d_skip is not looked at.
 *   the skip range : row i of d_skip_range, n x 2 int32 (first, count).  Object j is skipped iff count > 0 and
 *                    first <= j < first + count, in exact integer arithmetic (no 32-bit overflow; first may be negative).
 *                    For a rigid body's own objects, as p3d_scene_set_rig describes bodies.  NULL: no range.
 * With n_skip = 0 and d_skip_range NULL the call IS the unfiltered call: the same kernel, every bit of every output.
 */
#define P3D_FILTER_SKIP_MAX 8u

/*
 * p3d_nearest_k_device with filters.  k = 1 is p3d_nearest_device's answer (with a count); every argument but the three of the
 * filter, every output, the stream, the tail join, the spill area and every refusal are p3d_nearest_k_device's (the grid and a
 * plane under the BVH: P3D_ERR_UNSUPPORTED; P3D_ERR_CAPACITY as there).  d_skip and d_skip_range are device buffers like the
 * others: 4-byte aligned, on the scene's device, n*n_skip and n*2 int32 long, or the call is refused with nothing enqueued.
 * Additionally P3D_ERR_INVALID: n_skip > P3D_FILTER_SKIP_MAX (whatever n); with n > 0, n_skip > 0 and a NULL d_skip.
 * d_count, d_object, d_dist and d_closest equal p3d_host_scene_nearest_k_filtered's, bit for bit, for both accels.
 */
int p3d_nearest_k_filtered_device(p3d_scene* scene, uint32_t accel, uint32_t n, uint32_t k, const float* d_point,
                                  const float* d_max_dist /* n, or NULL */, const int32_t* d_skip /* n*n_skip, or NULL */,
                                  uint32_t n_skip, const int32_t* d_skip_range /* n*2, or NULL */, int32_t* d_count /* n */,
                                  int32_t* d_object /* n*k */, float* d_dist /* n*k */, float* d_closest /* n*k*3 */,
                                  float* d_normal /* n*k*3; these three may be NULL */, void* hip_stream);
/*
 * p3d_sweep_sphere_device with filters: likewise (a scene with a box, the grid and a plane under the BVH are refused as there).
 * d_object, d_t, d_centre and d_contact equal p3d_host_scene_sweep_sphere_filtered's, bit for bit, for both accels.
 */
int p3d_sweep_sphere_filtered_device(p3d_scene* scene, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction,
                                     const float* d_radius /* n */, const float* d_t_max /* n, or NULL */,
                                     const int32_t* d_skip /* n*n_skip, or NULL */, uint32_t n_skip,
                                     const int32_t* d_skip_range /* n*2, or NULL */, int32_t* d_object /* n, required */,
                                     float* d_t, float* d_centre, float* d_contact, float* d_normal, void* hip_stream);
/*
 * RAY QUERIES FROM INSIDE THE SCENE.  A range sensor mounted inside a rigged body hits its own hull at t ~ 0; a visibility
 * segment from a cloth vertex to a light is blocked by the vertex's own triangles; a particle that is a sphere of the scene
 * gets occlusion 0 from its own shell; "am I inside that mesh?" (total & 1 of p3d_trace_hits_device) counts the asking body's
 * own triangles.  The SEGMENT FAMILY of the ray queries - p3d_trace_any_device with d_t_max, p3d_trace_hits_device and
 * p3d_occlusion_device - tests every object on a fresh copy of the ray and answers with a set over objects that does not
 * depend on the order of the visits, so for both accels it supports
 *
 *     a filtered query  ==  the unfiltered query over the scene from which the objects of its filter are removed
 *
 * holds exactly: a skipped object is not tested at all, under P3D_ACCEL_BVH the boxes are those of the whole scene (a filter
 * makes a walk no shorter), and object indices stay the scene's.  The filters, their buffers and their refusals are those
 * above; with n_skip = 0 and d_skip_range NULL each call IS its unfiltered call: the same kernel, every bit of every output.
 * p3d_trace_closest_device and the feeler (p3d_trace_any_device without d_t_max) take no filter: they hand ONE ray from test to
 * test and, under the BVH, restart after a dead end (Q1), so their answers are not sets over objects.  The filtered closest
 * hit is k = 1 of p3d_trace_hits_filtered_device.  There are no host forms, as there are none of the unfiltered ray queries.
 *
 * p3d_trace_any_filtered_device: the segment query of p3d_trace_any_device with filters - d_occluded[i] = 1 iff some object
 * that query i does not skip is hit at t < d_t_max[i].  d_t_max is REQUIRED with n > 0 (NULL: P3D_ERR_INVALID; pass +inf for a
 * half-line): the half-line without a limit is the reference's feeler, which has no thinned-scene meaning under the BVH.
 * P3D_ACCEL_GRID: P3D_ERR_UNSUPPORTED.  Everything else, every refusal included, as p3d_trace_any_device with d_t_max.
 */
int p3d_trace_any_filtered_device(p3d_scene* scene, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction,
                                  const float* d_t_max /* n, required */, const int32_t* d_skip /* n*n_skip, or NULL */,
                                  uint32_t n_skip, const int32_t* d_skip_range /* n*2, or NULL */, uint8_t* d_occluded /* n */,
                                  void* hip_stream);
/*
 * p3d_trace_hits_device with filters.  A skipped object is never offered: it is not listed, it is not counted in d_total and
 * it tightens no bound, so a full list is refilled from behind it.  0 <= k <= P3D_TRACE_HITS_K_MAX; k = 0 with d_total is the
 * parity without the asking body.  k = 1 is the filtered closest hit of the segment family: like p3d_trace_hits_device's k = 1
 * it is the minimum of the per-object tests under (t, index), which - filter or no filter - need not equal
 * p3d_trace_closest_device's answer (Q8, ties), nor P3D_ACCEL_NONE's in the last bits under the BVH.  Every other argument,
 * every output and every refusal are p3d_trace_hits_device's.
 */
int p3d_trace_hits_filtered_device(p3d_scene* scene, uint32_t accel, uint32_t n, uint32_t k, const float* d_origin,
                                   const float* d_direction, const float* d_t_max /* may be NULL */,
                                   const int32_t* d_skip /* n*n_skip, or NULL */, uint32_t n_skip,
                                   const int32_t* d_skip_range /* n*2, or NULL */, int32_t* d_count /* n */,
                                   int32_t* d_total /* n, may be NULL */, int32_t* d_object /* n*k */, float* d_t /* n*k */,
                                   float* d_hit_point /* n*k*3 */, float* d_normal /* n*k*3 */, void* hip_stream);
/*
 * p3d_occlusion_device with filters: ONE filter row per POINT (n rows), shared by all of the point's samples and by all lanes
 * of its team.  d_unoccluded and d_bent are those of p3d_occlusion_device over the thinned scene - with the same team the
 * same bits -, and they equal p3d_trace_any_filtered_device over p3d_occlusion_rays_device's rays (unchanged: the filter moves
 * no ray) with each point's row repeated per sample.  Every other argument and every refusal are p3d_occlusion_device's.
 */
int p3d_occlusion_filtered_device(p3d_scene* scene, uint32_t accel, uint32_t n, const float* d_point, const float* d_normal,
                                  const float* d_max_dist /* n, or NULL */, const p3d_occlusion_params* params,
                                  const int32_t* d_skip /* n*n_skip, or NULL */, uint32_t n_skip,
                                  const int32_t* d_skip_range /* n*2, or NULL */, uint32_t* d_unoccluded /* n */,
                                  float* d_bent /* n*3, or NULL */, void* hip_stream);
/*
 * The statements of these semantics on the CPU: p3d_host_scene_nearest_k and p3d_host_scene_sweep_sphere with the same filter
 * rule (host/filter_rule.hpp, one spelling for the host and the device), by brute force.  No device is needed.  Arguments,
 * outputs and refusals as the unfiltered host forms; additionally P3D_ERR_INVALID for n_skip > P3D_FILTER_SKIP_MAX, and for
 * n > 0 with n_skip > 0 and a NULL skip.
 */
int p3d_host_scene_nearest_k_filtered(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* points, const float* max_dist,
                                      const int32_t* skip /* n*n_skip, or NULL */, uint32_t n_skip,
                                      const int32_t* skip_range /* n*2, or NULL */, int32_t* count, int32_t* object, float* dist,
                                      float* closest);
int p3d_host_scene_sweep_sphere_filtered(const p3d_host_scene* hs, uint32_t n, const float* origin, const float* direction,
                                         const float* radius, const float* t_max, const int32_t* skip, uint32_t n_skip,
                                         const int32_t* skip_range, int32_t* object, float* t, float* centre, float* contact);

#ifdef __cplusplus
}
#endif

#endif /* P3D_FILTER_H */

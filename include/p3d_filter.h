/*
 * p3d_filter.h - part of the C-ABI of libp3d.so, included by p3d.h (include that; including this file alone works too).
 * Nearest-surface queries and sphere sweeps that leave objects out, per query.  Same conventions as p3d.h: int return codes
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

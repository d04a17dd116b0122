/*
 * p3d_segment.h - part of the C-ABI of libp3d.so, included by p3d.h (include that; including this file alone works too).
 * Nearest surfaces to a SEGMENT: capsule overlap and edge proximity against a live scene.  Same conventions as p3d.h: int
 * return codes (P3D_OK or a P3D_ERR_*), p3d_last_error for the message.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#ifndef P3D_SEGMENT_H
#define P3D_SEGMENT_H

#include "p3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A QUERY FOR A THING THAT HAS LENGTH: an edge of a cloth mesh (edge-edge proximity, the half of cloth contact that vertex
 * queries cannot see), the axis of a capsule ("what does this link overlap?" is "which objects lie within r of its axis?"), a
 * piece of rope or hair, the thick line between two particles.  Sampling points along the segment and asking
 * p3d_nearest_k_device for each costs several traversals, returns duplicates, misses a thin triangle between two samples and
 * never reports distance 0 for a segment that passes clean through a face.  This is the one query for it.
 *
 * Segment i runs from a_i to b_i (two n x 3 float32 buffers).  For every segment: the (at most) k objects whose SURFACE - a
 * sphere's shell inside and outside alike, the closed triangle, the plane, as p3d_nearest_device has it - comes nearest to ANY
 * point of the segment, within d_max_dist[i] (optional, per segment; for a capsule: its radius), in the order (d2, object
 * index): the total order, the gate, the rule for limits (only max_dist > 0 finds anything; a NaN: nothing) and the no-answer
 * values of p3d_nearest_k_device.  Row i k + j, j < d_count[i]:
 *   d_object     : the object
 *   d_dist       : sqrtf(d2)
 *   d_param      : s in [0, 1]: the point of the segment nearest to the object is x = a + (b - a) s
 *   d_on_segment : x, as the rule computed it
 *   d_closest    : q, the point of the object nearest to x; d2 = |x - q|^2 from the two as stored
 *   d_normal     : the object's normal at q, geometric and not turned, as p3d_nearest_device reports it
 * Rows j >= d_count[i]: -1, FLT_MAX, zeros.
 *
 * The per-object rule (host/nearest_segment_rule.hpp, float32, one spelling for the host and the device):
 *   a == b     : in all three coordinates: the point rule at a.  Every bit of p3d_nearest_k_filtered_device's answer there, with
 *                param = +0.0 and on_segment = a.
 *   crossing   : a segment that pierces a triangle, enters or leaves a sphere's shell or crosses a plane has distance 0 to it:
 *                x = q is the crossing nearest to a, and d2 is exactly +0.0.
 *   triangle   : otherwise the minimum over five candidates in a fixed order, the first winning a tie: the two endpoints
 *                against the triangle, then the edges A B, B C, C A as closest pairs of two segments.
 *   sphere     : outside, the foot of the centre on the segment against the shell; wholly inside, the endpoint farthest from
 *                the centre (a on a tie) against the shell.
 *   plane      : otherwise the endpoint of the smaller height, a on a tie.
 *   box        : NOT part of this query: a scene that holds a box is refused with P3D_ERR_UNSUPPORTED.  Segment against a box's
 *                faces is left for a later change.
 *
 * FILTERS are part of the query (an edge of a cloth belongs to the scene: its two incident triangles and their neighbours are
 * its skip list): d_skip, n_skip and d_skip_range are those of p3d_filter.h, their meaning and their refusals unchanged - a
 * filtered query is the unfiltered query over the scene without the named objects; object indices stay the scene's.  With
 * n_skip = 0 and a NULL d_skip_range the kernel that holds no filter code is launched.
 *
 * d_count, d_object, d_dist, d_param, d_on_segment and d_closest equal p3d_host_scene_nearest_segment_k's for the same
 * geometry, bit for bit, for both accels.
 *   P3D_ACCEL_NONE : every object.
 *   P3D_ACCEL_BVH  : the tree, a node keyed by a lower bound of the squared distance from the segment to its box (the gaps
 *                    between the segment's extent and the box, per axis) and dropped once that exceeds the k-th candidate's d2
 *                    (or the limit's square) times 1 + 2^-10.  A scene that holds a plane is refused with
 *                    P3D_ERR_UNSUPPORTED, as by p3d_nearest_device and for the same reason.
 *   P3D_ACCEL_GRID : P3D_ERR_UNSUPPORTED.
 * Everything else is p3d_nearest_k_filtered_device's: one kernel on `hip_stream`, no wait, no allocation once the spill area
 * is large enough; behind p3d_scene_refit_device or p3d_scene_pose_device on the same stream it sees the moved geometry.
 * Refused, nothing enqueued and nothing written: P3D_ERR_INVALID for a null scene, an unknown accel or one the scene was
 * created without, k == 0 or k > P3D_NEAREST_K_MAX, n_skip > P3D_FILTER_SKIP_MAX, with n > 0 a null d_a, d_b, d_count or
 * d_object or a null d_skip with n_skip > 0, a misaligned pointer, host memory, memory of another device or a buffer too
 * short; P3D_ERR_CAPACITY where n x the tree's depth does not fit the 32-bit offsets of the spill area (split the batch).
 * n = 0 returns P3D_OK.
 */
int p3d_nearest_segment_k_device(p3d_scene* scene, uint32_t accel, uint32_t n, uint32_t k, const float* d_a, const float* d_b,
                                 const float* d_max_dist /* n, or NULL */, const int32_t* d_skip /* n*n_skip, or NULL */,
                                 uint32_t n_skip, const int32_t* d_skip_range /* n*2, or NULL */, int32_t* d_count /* n */,
                                 int32_t* d_object /* n*k, required */, float* d_dist /* n*k */, float* d_param /* n*k */,
                                 float* d_on_segment /* n*k*3 */, float* d_closest /* n*k*3 */,
                                 float* d_normal /* n*k*3; these five may be NULL */, void* hip_stream);
/*
 * The statement of these semantics on the CPU: the rule on every object the segment's filter does not name, in object order,
 * by brute force.  No device is needed.  dist, param, on_segment and closest may be NULL.  P3D_ERR_INVALID: a null scene,
 * k == 0 or k > P3D_NEAREST_K_MAX, n_skip > P3D_FILTER_SKIP_MAX, with n > 0 a null a, b, count or object or a null skip with
 * n_skip > 0; P3D_ERR_UNSUPPORTED: the scene holds a box.
 */
int p3d_host_scene_nearest_segment_k(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* a, const float* b,
                                     const float* max_dist /* n, or NULL */, const int32_t* skip /* n*n_skip, or NULL */,
                                     uint32_t n_skip, const int32_t* skip_range /* n*2, or NULL */, int32_t* count, int32_t* object,
                                     float* dist, float* param, float* on_segment, float* closest);
/*
 * Host only, for the tests: the key of a BVH node under this query, out[i] = the rule's lower bound of the squared distance
 * from the segment a_i b_i to the box lo_i .. hi_i (n x 3 float32 each).  P3D_ERR_INVALID: a null array with n > 0.
 */
int p3d_debug_segment_box_d2(uint32_t n, const float* a, const float* b, const float* lo, const float* hi, float* out);

#ifdef __cplusplus
}
#endif

#endif /* P3D_SEGMENT_H */

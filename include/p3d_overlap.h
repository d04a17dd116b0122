/*
 * p3d_overlap.h - part of the C-ABI of libp3d.so, included by p3d.h (include that; including this file alone works too).
 * Overlap queries: the objects of a live scene that touch an axis-aligned box.  Same conventions as p3d.h: int return codes
 * (P3D_OK or a P3D_ERR_*), p3d_last_error for the message.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#ifndef P3D_OVERLAP_H
#define P3D_OVERLAP_H

#include "p3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Spheres and boxes count as solids: a query box wholly inside one overlaps it.  Triangles and planes have no inside. */
#define P3D_OVERLAP_SOLID 1u

/*
 * WHAT IS IN THIS REGION?  The broad phase of a rigid body (which objects touch my bounding box, leaving out my own), a
 * trigger volume, a selection rectangle extruded into a box, the occupancy of a voxel.  p3d_nearest_k_device at the box's
 * centre with the half diagonal as limit answers for the circumscribed ball, stops at 16 objects without saying how many
 * there are, and sampled points miss thin triangles.  This is the one query for it.
 *
 * Query i is the CLOSED axis-aligned box lo_i .. hi_i (two n x 3 float32 buffers).  For every box:
 *   d_total[i]       : the number of objects the box overlaps (required)
 *   d_object[i k + j]: for k >= 1 (required then), the min(total, k) LOWEST object indices among them, ascending; the rows
 *                      behind those hold -1.  0 <= k <= P3D_NEAREST_K_MAX; k == 0 is the count alone: d_object is neither
 *                      read nor written.
 * A box with lo > hi on some axis, or with a NaN, finds nothing: total = 0.
 *
 * "Overlaps" follows the surface convention of p3d_nearest_device: the closed triangle, a sphere's shell, a box's faces, the
 * plane.  flags: 0 or P3D_OVERLAP_SOLID, with which spheres and boxes count as solids.  Touching counts as overlap.
 *
 * The per-object rule (host/overlap_rule.hpp, float32, one spelling for the host and the device).  First, for every kind
 * but the plane, plain comparisons of the query box against the object's own box - the extent of a triangle's vertices, a
 * sphere's centre -+ radius, a box's min and max - and then:
 *   triangle : a separating-axis test over the triangle's normal and the nine products of an edge with a coordinate axis, in
 *              a fixed order; both shapes are projected onto each axis as intervals, and only a strictly positive gap
 *              separates.  A zero-area triangle's null axes separate nothing: it is what its remaining axes make of it.
 *   sphere   : the squared distance from the centre to the box <= r r; without SOLID also the squared distance to the
 *              farthest corner >= r r (the box is not wholly inside the shell).
 *   box      : without SOLID the query box must not lie strictly inside the open interior.
 *   plane    : the smallest and the largest height of the eight corners, min_h <= 0 <= max_h.
 * Every test is a positive one: a NaN is never an overlap.
 *
 * FILTERS: d_skip, n_skip and d_skip_range are those of p3d_filter.h, their meaning and their refusals unchanged (a body asks
 * with its own box and skips its own range); a skipped object is neither counted nor listed.  With n_skip = 0 and a NULL
 * d_skip_range the kernel that holds no filter code is launched.
 *
 * d_total and d_object equal p3d_host_scene_overlap_box's for the same geometry, bit for bit, for both accels.
 *   P3D_ACCEL_NONE : every object, planes included.
 *   P3D_ACCEL_BVH  : the tree, a node kept unless its box and the query box are apart on some axis, by comparisons alone:
 *                    the rule's first stage makes that exact, no slack is needed.  A scene that holds a plane is refused with
 *                    P3D_ERR_UNSUPPORTED, as by p3d_nearest_device and for the same reason.
 *   P3D_ACCEL_GRID : P3D_ERR_UNSUPPORTED.
 * One kernel on `hip_stream`, no wait, no allocation once the spill area is large enough; behind p3d_scene_refit_device or
 * p3d_scene_pose_device on the same stream it sees the moved geometry.
 * Refused, nothing enqueued and nothing written: P3D_ERR_INVALID for a null scene, an unknown accel or one the scene was
 * created without, k > P3D_NEAREST_K_MAX, a bit of flags other than P3D_OVERLAP_SOLID, n_skip > P3D_FILTER_SKIP_MAX, with
 * n > 0 a null d_lo, d_hi or d_total, a null d_object with k >= 1 or a null d_skip with n_skip > 0, a misaligned pointer, host
 * memory, memory of another device or a buffer too short; P3D_ERR_CAPACITY where n x the tree's depth does not fit the 32-bit
 * offsets of the spill area (split the batch).  n = 0 returns P3D_OK.
 */
int p3d_overlap_box_device(p3d_scene* scene, uint32_t accel, uint32_t n, uint32_t k, const float* d_lo, const float* d_hi,
                           const int32_t* d_skip /* n*n_skip, or NULL */, uint32_t n_skip, const int32_t* d_skip_range /* n*2, or NULL */,
                           uint32_t flags, int32_t* d_total /* n */, int32_t* d_object /* n*k; NULL with k == 0 */, void* hip_stream);
/*
 * The statement of these semantics on the CPU: the rule on every object the box's filter does not name, in object order, by
 * brute force.  No device is needed.  P3D_ERR_INVALID: a null scene, k > P3D_NEAREST_K_MAX, an unknown flag,
 * n_skip > P3D_FILTER_SKIP_MAX, with n > 0 a null lo, hi or total, a null object with k >= 1 or a null skip with n_skip > 0.
 */
int p3d_host_scene_overlap_box(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* lo, const float* hi,
                               const int32_t* skip /* n*n_skip, or NULL */, uint32_t n_skip, const int32_t* skip_range /* n*2, or NULL */,
                               uint32_t flags, int32_t* total, int32_t* object);

#ifdef __cplusplus
}
#endif

#endif /* P3D_OVERLAP_H */

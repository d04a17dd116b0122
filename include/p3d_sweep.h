/*
 * p3d_sweep.h - part of the C-ABI of libp3d.so, included by p3d.h (include that; including this file alone works too).
 * Sphere sweeps against a live scene: the first contact of a moving ball.  Same conventions as p3d.h: int return codes (P3D_OK
 * or a P3D_ERR_*), p3d_last_error for the message.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#ifndef P3D_SWEEP_H
#define P3D_SWEEP_H

#include "p3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * CONTINUOUS COLLISION DETECTION for a body with a thickness that moves between two steps: a particle, a cloth vertex, a
 * probe.  A ray query treats it as a point (a ball of radius r clips the edge of a triangle its centre line misses), a nearest
 * query sees only the end of the step (a fast ball tunnels through a thin wall).  This is the one query for both.
 *
 * Query i is an origin o, a direction d, a radius r >= 0 and, with d_t_max, a limit.  d is used AS GIVEN: it need not be unit,
 * and t is in units of d (pass the step's displacement and a limit of 1 for "within this step").  The ball's centre is
 * c(t) = o + t d.  For object j, dist_j(p) is the distance from p to j's SURFACE, exactly as p3d_nearest_device has it: a
 * sphere's shell inside and outside alike, the closed triangle, the plane.  The contact time is
 *     T_j = min { t in [0, t_max] : dist_j(c(t)) <= r }      (none if the set is empty; 0 when the ball touches at the start)
 * and the answer is the object with the smallest (T_j, object index): a total order.
 *
 * The per-object rule (host/sweep_rule.hpp, float32, one spelling for the host and the device):
 *   every kind : a start that overlaps (the nearest-surface rule's d2 <= r^2) is T = 0.
 *   triangle   : the face - the centre reaches the plane offset by r on the side it starts on - if the foot of c(t) on the plane
 *                lies in the closed triangle; otherwise the smallest root among the three edges (the ray against the cylinder
 *                of radius r about the edge, foot on the edge) and the three vertices (the ray against the sphere of radius r).
 *   sphere     : from outside the smaller root against radius R + r; from inside the shell the larger root against R - r.
 *   plane      : the signed height reaches +-r from the side it starts on, only when the centre moves towards the plane.
 *   box        : not swept (a rounded box, and its inside).  A scene that holds a box is refused with P3D_ERR_UNSUPPORTED.
 *
 * Outputs per query, d_object required, the others may be NULL:
 *   d_object  : the object, or -1
 *   d_t       : T; FLT_MAX where nothing is met
 *   d_centre  : c(T); zeros where nothing is met
 *   d_contact : the nearest-surface rule's closest point of that object at c(T): where the ball touches; zeros
 *   d_normal  : the object's normal at d_contact, geometric and not turned towards the ball, as p3d_nearest_device reports
 *               it; zeros
 * Nothing is found by: r NaN or negative; a limit that is NaN or <= 0; a NaN in o or d; a zero direction, unless the start
 * overlaps (T = 0).
 *
 * d_object, d_t, d_centre and d_contact equal p3d_host_scene_sweep_sphere's for the same geometry, bit for bit, for both accels.
 *   P3D_ACCEL_NONE : every object.
 *   P3D_ACCEL_BVH  : the tree, culled by the ray's entry into each node's box grown by r (times 1 + 2^-10, plus 1e-4): a node
 *                    entered later than the best T so far (times 1 + 2^-10) is dropped.  A scene that holds a plane is refused
 *                    with P3D_ERR_UNSUPPORTED, as by p3d_nearest_device and for the same reason.
 *   P3D_ACCEL_GRID : P3D_ERR_UNSUPPORTED.
 * Stream, buffers, tail join and spill area as p3d_nearest_device: one kernel on `hip_stream`, no wait, no allocation once the
 * spill area is large enough; behind p3d_scene_refit_device or p3d_scene_pose_device on the same stream it sees the moved
 * geometry.  Refused, nothing enqueued and nothing written: P3D_ERR_INVALID for a null scene, an unknown accel or one the scene
 * was created without, with n > 0 a null d_origin, d_direction, d_radius or d_object, a misaligned pointer, host memory, memory
 * of another device or a buffer too short; P3D_ERR_CAPACITY where n x the tree's depth does not fit the 32-bit offsets of the
 * spill area (split the batch).  n = 0 returns P3D_OK.
 */
int p3d_sweep_sphere_device(p3d_scene* scene, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction,
                            const float* d_radius /* n */, const float* d_t_max /* n, or NULL: no limit */,
                            int32_t* d_object /* n, required */, float* d_t /* n */, float* d_centre /* n*3 */,
                            float* d_contact /* n*3 */, float* d_normal /* n*3; these four may be NULL */, void* hip_stream);
/*
 * The statement of these semantics on the CPU: the rule on every object of a loaded host scene, by brute force.  No device is
 * needed.  t, centre and contact may be NULL.  P3D_ERR_INVALID: a null scene, a null origin, direction, radius or object with
 * n > 0; P3D_ERR_UNSUPPORTED: the scene holds a box.
 */
int p3d_host_scene_sweep_sphere(const p3d_host_scene* hs, uint32_t n, const float* origin, const float* direction,
                                const float* radius /* n */, const float* t_max /* n, or NULL */, int32_t* object,
                                float* t, float* centre, float* contact);

#ifdef __cplusplus
}
#endif

#endif /* P3D_SWEEP_H */

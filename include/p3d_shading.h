/*
 * p3d_shading.h - part of the C-ABI of libp3d.so, included by p3d.h (include that; including this file alone works too).
 * The lights and materials of a live scene, set from host memory or from device memory on the caller's stream.  Same
 * conventions as p3d.h: int return codes (P3D_OK or a P3D_ERR_*), p3d_last_error for the message.  Detected by the symbols
 * (P3D_ABI_VERSION is unchanged).
 */
#ifndef P3D_SHADING_H
#define P3D_SHADING_H

#include "p3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * WHAT A SCENE IS LIT BY AND MADE OF can change as its camera and its objects can: to dim or move a light, turn a mirror
 * into glass, recolour an object or switch an emitter on, without a new scene.  The accelerators do not depend on materials
 * or lights, so EVERY scene takes these calls: those with an uploaded tree or an uploaded grid, which refuse every geometry
 * update, included.  The counts are fixed at creation, and so is every object's material index.  A light is switched off by
 * giving it colour 0.  Values are taken as given, NaN and inf included, as p3d_scene_create takes them.
 *
 * What the library derives from the records follows them (DESIGN.md "Shading updates"): the flag that lets a kernel leave out
 * the pow of a material whose specular term is an exact zero (it depends on the material and on every light's colour), the
 * list of emissive spheres the path tracer samples (emission[0] + emission[1] + emission[2] > 0, in float32), the kernel
 * variants of P3D_STACK_LITERAL frames (some material with transmittance != 0 && reflection > 0), and the memos of earlier
 * frames: after a call that changed something, an accumulator or adaptive state of the scene refuses further passes until it
 * is reset, as after a geometry update.  p3d_temporal knows nothing of shading changes: it keeps reprojecting with the camera
 * alone; reset it, or accept that the history lags.
 *
 * THE WAITING FORMS: records in HOST memory replace materials / lights [first, first + n).  They join the tail stream and
 * wait for the device, write the records and work out every derived fact above from the scene's whole tables as they then
 * are: the emitter list may grow, shrink or become empty, a LITERAL frame may change its kernels.  first + n past the
 * scene's count: P3D_ERR_INVALID, nothing changed.  n == 0: P3D_OK, nothing done.
 */
int p3d_scene_set_materials(p3d_scene* scene, uint32_t first, uint32_t n, const p3d_material* materials);
int p3d_scene_set_lights(p3d_scene* scene, uint32_t first, uint32_t n, const p3d_light* lights);
/*
 * The records as the device holds them, the counterpart of p3d_scene_camera: they wait for the device (the tail stream and
 * whatever a stream form enqueued) and copy [first, first + n) back.  Reserved fields come back as 0.
 */
int p3d_scene_materials(p3d_scene* scene, uint32_t first, uint32_t n, p3d_material* out);
int p3d_scene_lights(p3d_scene* scene, uint32_t first, uint32_t n, p3d_light* out);
/*
 * THE STREAM FORM: d_materials is [n_materials, 16] float32 and d_lights [n_lights, 8] float32 in DEVICE memory - the two
 * structs' own layouts (the reserved floats are not read) - e.g. tensors a torch program has just written on `hip_stream`.
 * Either part may be empty, with a null pointer.  One kernel is enqueued on `hip_stream` behind the previous frame's tail;
 * the call does not wait, copies nothing back and allocates nothing after the scene's first such call.  A query or frame
 * enqueued behind it on the same stream sees the new records.
 *
 * The host never sees the values, so the kernel keeps what the host knows of them: a material whose new record would change
 * whether it emits, or whether it is transmissive and reflective, compared with the record it replaces, is SKIPPED - it keeps
 * its record (its pow flag still follows the new lights); the others are written.  The call itself returns P3D_OK; the next
 * p3d_scene_status returns P3D_ERR_INVALID with the two counts since the last check in p3d_last_error, and the one after
 * that P3D_OK.  The waiting form makes such a change.
 *
 * Refused, nothing enqueued: P3D_ERR_INVALID for a null scene, a range past the scene's count, a null pointer with a count,
 * a pointer that is not 4-byte aligned, host memory, memory of another device or a buffer too short.  Both counts 0:
 * P3D_OK, nothing done.
 */
int p3d_scene_set_shading_device(p3d_scene* scene, uint32_t first_material, uint32_t n_materials, const void* d_materials,
                                 uint32_t first_light, uint32_t n_lights, const void* d_lights, void* hip_stream);
/*
 * The same on a loaded host scene, so that p3d_host_scene_desc afterwards describes the changed scene (what a fresh
 * p3d_scene_create of it renders is what the calls above leave).  A host BVH and grid already built stay valid.  After
 * p3d_host_scene_replicate_lights the indices are those of the replicated list.
 */
struct p3d_host_scene; /* (p3d.h names it p3d_host_scene further down, behind the point where it includes this file) */
int p3d_host_scene_set_materials(struct p3d_host_scene* hs, uint32_t first, uint32_t n, const p3d_material* materials);
int p3d_host_scene_set_lights(struct p3d_host_scene* hs, uint32_t first, uint32_t n, const p3d_light* lights);

#ifdef __cplusplus
}
#endif

#endif /* P3D_SHADING_H */

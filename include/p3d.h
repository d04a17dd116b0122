/*
 * p3d.h — C-ABI of the MI355X-native per-pixel ray-trace hot path.
 *
 * This is the drop-in boundary.  The reference (fmbnicola/P3D-RayTracer) has no
 * FFI: the seam is the in-process call that renderScene() (Raytracing/main.cpp:694)
 * makes once per pixel sample,
 *     rayTracing(ray, MAX_DEPTH, 1.0, i, j)            main.cpp:795,811
 *     Radiance  (ray, MAX_DEPTH, 1.0, i, j, seed)      main.cpp:792
 * against process globals (Scene* scene, Grid grid, BVH bvh: main.cpp:67-69) and the
 * compile-time option set of constants.h:6-45.  A per-ray FFI is meaningless on a
 * GPU, so one call here replaces the whole pixel x sample loop body of
 * main.cpp:747-820 for a tile of the image: primary-ray generation
 * (camera.h:65-115), closest-hit / any-hit traversal (bvh.cpp:198-340,
 * grid.cpp:71-208, brute force main.cpp:116-124), the shape tests
 * (scene.cpp:47-94,116-137,149-186,215-227; boundingBox.cpp:44-98), Whitted
 * shading (main.cpp:92-309) or the path tracer (main.cpp:313-516), sample
 * averaging (main.cpp:800), gamma (main.cpp:814-815) and the u8 pack
 * (maths.h:81-86).
 *
 * Plain C types only: no C++ classes, no torch types.  All functions return 0 on
 * success and a negative p3d_status on failure; they never throw and never
 * exit().  There is NO CPU fallback behind this ABI: without a HIP device every
 * render/trace entry point fails with P3D_ERR_NO_DEVICE.
 */
#ifndef P3D_H
#define P3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_ABI_VERSION 4u /* round 4: p3d_stats.handoff_dense_retry; the test hooks left this header (csrc/p3d_debug.h) */

typedef enum p3d_status {
  P3D_OK = 0,
  P3D_ERR_INVALID = -1,     /* bad argument / inconsistent descriptor           */
  P3D_ERR_NO_DEVICE = -2,   /* no HIP device, or HIP runtime error (see last_error) */
  P3D_ERR_UNSUPPORTED = -3, /* option combination not implemented on the device  */
  P3D_ERR_CAPACITY = -4,    /* traversal stack / scene exceeds device limits     */
  P3D_ERR_IO = -5           /* .p3f file could not be opened                     */
} p3d_status;

/* Object kinds of scene.h:101-179 (Sphere, Triangle, aaBox, Plane). */
typedef enum p3d_prim_type {
  P3D_PRIM_SPHERE = 0,
  P3D_PRIM_TRIANGLE = 1,
  P3D_PRIM_BOX = 2,
  P3D_PRIM_PLANE = 3
} p3d_prim_type;

/* constants.h:41 — enum accel_struct {None, UGrid, Bvh}; same numeric values. */
typedef enum p3d_accel { P3D_ACCEL_NONE = 0, P3D_ACCEL_GRID = 1, P3D_ACCEL_BVH = 2 } p3d_accel;
/* constants.h:42 — enum sample_mode {jitter, tent}. */
typedef enum p3d_sample_mode { P3D_SAMPLE_JITTER = 0, P3D_SAMPLE_TENT = 1 } p3d_sample_mode;
/* constants.h:36 — PATHTRACING false/true. */
typedef enum p3d_integrator { P3D_WHITTED = 0, P3D_PATHTRACE = 1 } p3d_integrator;

/*
 * One scene object, in Scene::objects push order (scene.cpp:296-299).  The index
 * of a record in the array IS the hit ID reported by the renderer.
 *   sphere   : v[0..2] = center, v[3] = radius                   (scene.h:139-162)
 *   triangle : v[0..8] = P0,P1,P2 ; n = unit normal as the ctor computes it
 *              (scene.cpp:17-18) ; bmin/bmax = Min/Max -/+ EPSILON (scene.cpp:21-34)
 *   box      : v[0..2] = min, v[3..5] = max                      (scene.cpp:205-209)
 *   plane    : v[0..2] = PN (unit normal), v[3..5] = A            (scene.cpp:102-113)
 * bmin/bmax hold GetBoundingBox() for every kind (sphere: center -/+ r,
 * scene.cpp:194-198; plane: the default [-1,1]^3 box, scene.h:114).
 */
typedef struct p3d_prim {
  float v[9];
  uint32_t type;     /* p3d_prim_type */
  uint32_t material; /* index into p3d_scene_desc.materials */
  uint32_t reserved0;
  float n[3];
  uint32_t reserved1;
  float bmin[3];
  uint32_t reserved2;
  float bmax[3];
  uint32_t reserved3;
} p3d_prim; /* 96 bytes */

/* Material (scene.h:34-71).  reflection == specular: m_Refl = Ks (scene.h:42). */
typedef struct p3d_material {
  float diff_color[3];
  float diffuse;      /* Kd */
  float spec_color[3];
  float specular;     /* Ks */
  float shine;
  float transmittance; /* T */
  float refr_index;    /* ior */
  float reflection;    /* = Ks */
  float emission[3];
  float reserved;
} p3d_material; /* 64 bytes */

/* Light (scene.h:73-81). */
typedef struct p3d_light {
  float position[3];
  float reserved0;
  float color[3];
  float reserved1;
} p3d_light; /* 32 bytes */

/* Camera state after the constructor of camera.h:34-63 has run. */
typedef struct p3d_camera {
  float eye[3];
  float plane_dist;
  float u[3];
  float w;           /* view-window width  */
  float v[3];
  float h;           /* view-window height */
  float n[3];
  float focal_ratio;
  float aperture;    /* Aperture_ratio * (w / res_x), camera.h:59 */
  int32_t res_x;
  int32_t res_y;
  int32_t reserved;
} p3d_camera; /* 80 bytes */

/*
 * BVH node, 32 bytes, in the order BVH::build_recursive pushes them
 * (bvh.cpp:185-194): node 0 is the root and the two children of an inner node
 * are adjacent at [index, index+1].
 *   inner: count_leaf == 0,                 index = left child
 *   leaf : count_leaf = 0x80000000 | n_objs, index = first entry in bvh_prim_index
 */
typedef struct p3d_bvh_node {
  float bmin[3];
  uint32_t index;
  float bmax[3];
  uint32_t count_leaf;
} p3d_bvh_node;
#define P3D_BVH_LEAF 0x80000000u

/* Uniform grid as Grid::Build lays it out (grid.cpp:3-68): cell (ix,iy,iz) is
 * entry ix + nx*iy + nx*ny*iz; its objects are cell_items[cell_start[c] ..
 * cell_start[c+1]) in insertion (= object) order. */
typedef struct p3d_grid_desc {
  float bmin[3];
  int32_t nx;
  float bmax[3];
  int32_t ny;
  int32_t nz;
  uint32_t n_cells;          /* nx*ny*nz */
  uint32_t n_items;          /* cell_start[n_cells] */
  uint32_t reserved;
  const uint32_t* cell_start; /* n_cells + 1 entries */
  const uint32_t* cell_items; /* object indices */
} p3d_grid_desc;

/* Everything the device needs; all arrays are host memory owned by the caller
 * and are copied by p3d_scene_create. */
typedef struct p3d_scene_desc {
  uint32_t abi_version; /* P3D_ABI_VERSION */
  uint32_t n_prims;
  uint32_t n_materials;
  uint32_t n_lights;
  const p3d_prim* prims;
  const p3d_material* materials;
  const p3d_light* lights;
  p3d_camera camera;
  float background[3];       /* bclr, Scene::GetBackgroundColor (scene.h:189) */
  uint32_t n_bvh_nodes;      /* 0 = no BVH supplied */
  const p3d_bvh_node* bvh_nodes;
  const uint32_t* bvh_prim_index; /* permuted BVH::objs (bvh.cpp:84), object indices */
  uint32_t n_bvh_prim_index;
  uint32_t bvh_max_depth;    /* levels, root = 1 */
  uint32_t has_grid;
  uint32_t reserved;
  p3d_grid_desc grid;
} p3d_scene_desc;

/* Runtime form of the compile-time options of constants.h:6-45.  p3d_config_default()
 * fills in the reference's shipped values, except SKYBOX: it defaults to 0 (miss = bclr)
 * because the cubemap has to be supplied separately (p3d_scene_set_skybox). */
/* Order in which the 8x8-pixel tiles of a launch are handed to the GPU.  COST (default, 0):
 * tiles whose pixels spawn reflection / refraction chains go first, so the long-running
 * tiles do not end up alone at the end of the frame; the order comes from a small estimate
 * pass that is memoised per (scene, max_depth, accel, tile).  FRAME: image order. */
#define P3D_TILE_ORDER_COST 0u
#define P3D_TILE_ORDER_FRAME 1u

/*
 * What becomes of BVH::hit_stack (bvh.cpp:86), which the reference keeps as ONE member for the
 * whole frame: an any-hit query that returns `true` (bvh.cpp:322) leaves its entries behind, and
 * they are still there when the NEXT pixel's primary ray is traced (serial pixel loop,
 * main.cpp:747-751); that closest-hit query drains them (bvh.cpp:256-274), which can re-normalise
 * its ray copy once more (ray.h:16-18) and move the hit point by an ulp.
 *   LITERAL (default, 0): every pixel starts with exactly the entries the reference's serial loop
 *     would hand it (x fastest, rows ascending, samples of a pixel in order).  The GPU renders all
 *     pixels speculatively on an empty stack, keeps every pixel's leftover, and re-renders the
 *     pixels whose first closest hit changes under the predecessor's leftover, round by round
 *     until nothing changes (DESIGN.md "hit_stack hand-off").  Zero-weight reflection rays of
 *     transmissive materials (Kr = 1/2*(Rs+Rp) = 0, main.cpp:282,290-300) are traced for their
 *     effect on the stack, as the reference traces them.  Frames are bit-identical to the
 *     reference's order of execution.  Only Whitted + accel = Bvh have such a stack.
 *   PER_PIXEL (1): the stack is emptied at every primary sample and zero-weight rays are skipped:
 *     one launch, no hand-off; hit IDs as LITERAL, colours differ by a few 1e-5 on sphere scenes.
 */
#define P3D_STACK_LITERAL 0u
#define P3D_STACK_PER_PIXEL 1u

/*
 * How the chain of rayTracing calls of a pixel (main.cpp:247-300) is put on the GPU.  MEGAKERNEL: one lane follows its
 * pixel from the primary ray to the end of the chain.  PER_LEVEL: one launch per chain level; the surviving child rays
 * are compacted into a queue and put in order (origin cell, direction octant) between levels, so that every wave of a
 * reflection level starts with 64 live rays.  Only for Whitted frames without anti-aliasing over a BVH too big for LDS.
 * AUTO (default) = MEGAKERNEL: on the scenes measured the per-level launches issue 13 % fewer instructions but take
 * longer (100k triangles 2048x2048: 25.3 ms against 19.6 ms) — what keeps lanes idle there is the spread of traversal
 * lengths inside one query, not dead pixels.  Same queries in the same per-pixel order either way: the
 * frames are bit-identical.
 */
#define P3D_CHAIN_AUTO 0u
#define P3D_CHAIN_MEGAKERNEL 1u
#define P3D_CHAIN_PER_LEVEL 2u

/* p3d_config.handoff_records.  COMPACT (default): leftovers share a pool of 8 entries (64 bytes) per pixel of the tile on
 * average - most pixels leave nothing, a few leave up to lights x tree depth entries; a frame that needs more fails with
 * P3D_ERR_CAPACITY (the host-buffer call p3d_render_tile then renders it again with DENSE records by itself; after a
 * device-buffer call ask p3d_scene_status and repeat the call with DENSE).  DENSE: room for the worst case of every pixel
 * (2 x lights x tree depth x 8 bytes per pixel: 2.7 GB for the 100k-triangle frame at 2048 x 2048), cannot run out. */
#define P3D_HANDOFF_COMPACT 0u
#define P3D_HANDOFF_DENSE 1u

/* p3d_config.debug_view */
#define P3D_DEBUG_NONE 0u
#define P3D_DEBUG_TEST_INTERSECT 1u /* TEST_INTERSECT (constants.h:18): every hit is Color(1,0,0) (main.cpp:156, 359) */
#define P3D_DEBUG_DEPTH_MAP 2u      /* DEPTH_MAP (constants.h:33): rayTracing without an acceleration structure returns
                                       the grey value remap(5, 20, 1, 0, min_t), clamped (main.cpp:86-88, 127-139);
                                       ignored with a grid or BVH and by the path tracer, as in the reference */

typedef struct p3d_config {
  uint32_t integrator;    /* PATHTRACING        constants.h:36  */
  uint32_t accel;         /* acl_str            constants.h:44  */
  int32_t max_depth;      /* MAX_DEPTH          constants.h:6   */
  uint32_t spp_sqrt;      /* SPP (sqrt of spp)  constants.h:12  */
  uint32_t antialiasing;  /* ANTIALIASING       constants.h:24  */
  uint32_t depth_of_field;/* DEPTH_OF_FIELD     constants.h:27  */
  uint32_t sample_disk;   /* SAMPLE_DISK        constants.h:21  */
  uint32_t soft_shadows;  /* SOFT_SHADOWS       constants.h:9   */
  uint32_t sample_mode;   /* s_mode             constants.h:45  */
  float light_side;       /* LIGHT_SIDE         constants.h:15  */
  float gamma;            /* GAMMA              constants.h:38  */
  uint32_t collect_stats; /* 1: fill the test/ray counters of p3d_stats (slower kernel) */
  uint32_t skybox;        /* SKYBOX             constants.h:30: a miss returns the cubemap texel
                             (main.cpp:145,351) instead of bclr; needs p3d_scene_set_skybox */
  uint32_t tile_order;    /* P3D_TILE_ORDER_*: scheduling only, never changes a result */
  uint64_t seed;          /* replaces set_rand_seed(time*time), main.cpp:722:
                             every (pixel, sample) draws from its own stream */
  uint32_t stack_mode;    /* P3D_STACK_*: BVH::hit_stack across pixels (bvh.cpp:86) */
  uint32_t chain_launch;  /* P3D_CHAIN_*: how the reflect / refract chain is launched; never changes a result */
  uint32_t debug_view;    /* P3D_DEBUG_*: the reference's two debug switches (constants.h:18,33), 0 as shipped */
  uint32_t handoff_records; /* P3D_HANDOFF_*: storage of the per-pixel hit_stack leftovers under P3D_STACK_LITERAL; never changes a result */
} p3d_config;

/*
 * Region of the image a call renders.  Rows are numbered as the reference
 * numbers them: y = 0 is the BOTTOM image row (main.cpp:747, camera.h:71).
 * Local row r of the output buffers maps to image row
 *     y = y0 + (r / stripe_h) * stripe_h * stripe_stride + (r % stripe_h)
 * so that one rank of an N-rank job renders every N-th stripe of stripe_h rows
 * (stripe_stride = N, y0 = rank * stripe_h); stripe_stride = 1 (or stripe_h = 0)
 * is a plain rectangle.  Output buffers are w*h, local row 0 first.
 * Under P3D_STACK_LITERAL a tile that is not the whole frame still renders the pixels of the serial frame: for every
 * row whose predecessor in the frame lies outside the tile the call first finds, among the frame pixels in front of
 * that row, one whose result provably does not depend on the hit_stack it finds (no primitive of the scene nearer than
 * its own first hit, ray direction stable under re-normalisation) and renders the pixels from there to the row for
 * what they leave on the stack.  If no such pixel is found among the 16 nearest candidates the call FAILS with
 * P3D_ERR_CAPACITY (it never returns a frame that is only probably right); stripes and sub-rectangles of every rank
 * count are therefore bit-identical to the whole frame, or the caller is told.
 */
typedef struct p3d_tile {
  int32_t x0, y0, w, h;
  int32_t stripe_h;
  int32_t stripe_stride;
} p3d_tile;

/* Counters of one call.  A "ray" is one traversal query (closest-hit or
 * any-hit).  The test counters feed the algorithmic-bytes figure of DESIGN.md.
 * They count what the FINAL frame traced, query by query, as the reference's serial loop would: under
 * P3D_STACK_LITERAL a pixel that was rendered again counts once, with its last render, a pixel whose first closest hit
 * was only re-traced on its predecessor's leftover counts that query's tests as re-traced (the stale entries it
 * visits), and the zero-weight reflection rays are rays.  max_stack is the deepest stack of anything that was traced,
 * speculative passes included.  What the hand-off cost on top is in the handoff_* fields and handoff_ms. */
typedef struct p3d_stats {
  uint64_t rays_primary;
  uint64_t rays_shadow;
  uint64_t rays_reflect;
  uint64_t rays_refract;
  uint64_t rays_bounce;  /* path-tracer continuation rays */
  uint64_t rays_light;   /* path-tracer light-visibility rays */
  uint64_t node_tests;   /* AABB::intercepts calls on BVH nodes */
  uint64_t sphere_tests;
  uint64_t tri_tests;
  uint64_t box_tests;
  uint64_t plane_tests;
  uint64_t shaded_hits;
  uint64_t pixels;
  uint64_t max_stack;    /* deepest traversal stack seen (entries) */
  double kernel_ms;      /* HIP-event time of the kernel(s) of this call */
  /* P3D_STACK_LITERAL only: the hand-off of BVH::hit_stack from pixel to pixel */
  uint64_t handoff_checked;  /* pixels whose first closest hit was re-traced on the predecessor's leftover */
  uint64_t handoff_redone;   /* pixels rendered again because that hit changed */
  uint64_t handoff_rounds;   /* rounds until no leftover changed any more */
  double pass1_ms;           /* of kernel_ms: the speculative pass over all pixels (the launches of pass 1 alone) */
  double handoff_ms;         /* of kernel_ms: check, redo and fixed-point launches */
  uint64_t handoff_dense_retry; /* p3d_render_tile only: 1 = the COMPACT leftover pool was too small for this frame and the
                                   call rendered it a second time with P3D_HANDOFF_DENSE records (twice the time, and the
                                   dense records allocated: lights x tree depth entries per pixel) */
} p3d_stats;

/* Device-resident scene, one per HIP device.  A p3d_scene also owns per-launch scratch and the
 * memoised tile schedules, so calls on ONE scene must not overlap in time from several host
 * threads (as the reference's renderScene() is single-threaded); different scenes are independent. */
typedef struct p3d_scene p3d_scene;

/* ---- library ---- */
uint32_t p3d_abi_version(void);
const char* p3d_last_error(void);          /* thread-local message of the last failure */
int p3d_device_count(void);                /* >= 0, or negative p3d_status */
void p3d_config_default(p3d_config* cfg);  /* constants.h:6-45 as shipped */

/* ---- scene on the device ---- */
/* Uploads the flattened scene to HBM of HIP device `device` (arrays copied). */
int p3d_scene_create(const p3d_scene_desc* desc, int device, p3d_scene** out);
/*
 * Same, but the BVH is built ON the GPU (linear BVH: Morton codes of the bounding-box centres,
 * radix sort, Karras hierarchy, bottom-up refit) instead of being uploaded; the descriptor's bvh_*
 * arrays are ignored, prims[].bmin/bmax must hold GetBoundingBox().  NOT the reference's tree
 * (bvh.cpp:89-196): closest-hit queries find the same nearest intersection (exact-t ties aside),
 * but the any-hit quirk of bvh.cpp:329-334 depends on the tree shape, so Whitted shadow feelers
 * can differ from a scene created with the reference-exact tree.  For callers who want correct
 * closest hits without waiting for the host build.  *build_ms (may be NULL): GPU time of the build.
 */
int p3d_scene_create_device_bvh(const p3d_scene_desc* desc, int device, p3d_scene** out, float* build_ms);
void p3d_scene_destroy(p3d_scene* scene);

/*
 * Cubemap for miss shading = the skybox_img[6] array that Scene::LoadSkybox fills
 * (scene.cpp:329-377, scene.h:218-223).  The caller decodes the six images (the reference
 * uses DevIL for that; JPEG decoding is not part of this library) and hands over raw bytes:
 * bpp 3 (RGB) or 4 (RGBA), row 0 = BOTTOM image row (IL_ORIGIN_LOWER_LEFT, scene.cpp:344-345),
 * face order RIGHT, LEFT, TOP, BOTTOM, FRONT, BACK (enum CubeMap, scene.h:28).  The texel
 * lookup itself (Scene::GetSkyboxColor, scene.cpp:379-457) runs in the kernels.
 */
typedef struct p3d_skybox_face {
  const uint8_t* img;
  uint32_t res_x, res_y, bpp;
  uint32_t reserved;
} p3d_skybox_face;
typedef struct p3d_skybox_desc {
  p3d_skybox_face face[6];
} p3d_skybox_desc;
int p3d_scene_set_skybox(p3d_scene* scene, const p3d_skybox_desc* sky);

/* ---- the hot path ---- */
/*
 * Renders one tile.  Replaces the loop body main.cpp:753-820 for every pixel of
 * the tile.  Host-buffer form: synchronous; any output pointer may be NULL.
 *   rgb    : w*h*3 float, linear colour after sample averaging (main.cpp:800),
 *            BEFORE gamma
 *   hit_id : w*h int32, object index hit by the pixel's first primary ray, -1 = miss
 *   rgb8   : w*h*3 uint8, after gamma + u8fromfloat (main.cpp:814-820) = img_Data
 */
int p3d_render_tile(p3d_scene* scene, const p3d_config* cfg, const p3d_tile* tile,
                    float* rgb, int32_t* hit_id, uint8_t* rgb8, p3d_stats* stats);
/*
 * Device-buffer form: the output pointers are HBM addresses on the scene's
 * device; the kernel is enqueued on `hip_stream` (a hipStream_t, NULL = default
 * stream) and the call returns without synchronising unless `stats` is non-NULL
 * (then it waits for the kernel and fills kernel_ms and, with
 * cfg->collect_stats, the counters).
 * All launches on ONE scene share its scratch (level records, stack spill area, hit_stack hand-off records, work lists,
 * counters): enqueue them on one stream, or order the streams with events; two renders of the same scene in flight at
 * once on different streams would overwrite each other's records.  Different scenes are independent.
 */
int p3d_render_tile_device(p3d_scene* scene, const p3d_config* cfg, const p3d_tile* tile,
                           float* d_rgb, int32_t* d_hit_id, uint8_t* d_rgb8,
                           void* hip_stream, p3d_stats* stats);

/*
 * The launches behind pass 1 of a P3D_STACK_LITERAL frame - the hit_stack hand-off rounds: a chain of short launches that
 * depend on each other and carry a few per cent of the frame's work - can be given a stream of their own, so that what the
 * caller enqueues behind the frame on `hip_stream` (other scenes' frames) is not held up by them: with a tail stream set,
 * p3d_render_tile_device without `stats` enqueues clear + pass 1 on `hip_stream` and everything behind them on the tail stream
 * (ordered by an event).  The frame's outputs are complete when the TAIL stream has passed the call: p3d_scene_join makes
 * `hip_stream` wait for that (host_wait = 0) or the calling thread (host_wait != 0); the next call on the same scene waits by
 * itself.  NULL switches it off.  No counterpart in the reference (one frame at a time on one core); what `bench.py` uses to
 * keep the chip busy with several frames in flight.
 */
int p3d_scene_set_tail_stream(p3d_scene* scene, void* tail_hip_stream);
int p3d_scene_join(p3d_scene* scene, void* hip_stream, int host_wait);

/*
 * Moving the camera of a device scene between frames - what a display loop does when the viewer moves - without a new .p3f,
 * host scene, BVH or upload.  Detected by the symbols, like p3d_accum (P3D_ABI_VERSION is unchanged).
 *
 * p3d_camera_look_at runs the Camera constructor (camera.h:34-63) the .p3f loader runs for a `v` block - the same code, not a
 * copy: with a scene's own `v` values (from, at, up, angle, resolution, aperture, focal) it gives, byte for byte, the
 * p3d_camera p3d_host_scene_desc returns.  P3D_ERR_INVALID for a resolution <= 0.  Host only, no device needed.
 * p3d_host_scene_view returns the `v` block a host scene was loaded with (after p3d_host_scene_set_lens: the lens it set).
 *
 * p3d_scene_set_camera replaces the scene's camera; frames enqueued after it render the new view, bit for bit as a scene
 * created with that camera renders it.  It is a host call that WAITS: for the scene's tail stream (p3d_scene_join) and then for
 * the whole device (hipDeviceSynchronize), because enqueued frames read the scene's memos; it therefore cannot be captured into
 * a graph (and a graph captured before it keeps the camera it was captured with).  Then it forgets what was worked out for the
 * old view's primary rays: the tile-cost schedules and the hit_stack hand-off's row chains and halo pixels.  Refused with
 * P3D_ERR_INVALID: a scene created without a camera (res_x or res_y <= 0), a camera whose res_x / res_y differ from the scene's
 * (the resolution is fixed at create), a non-finite field, w, h or plane_dist <= 0.  Setting the camera the scene already has
 * changes nothing.  A p3d_accum or p3d_adaptive records the scene's camera at create and reset: a pass after the camera changed,
 * without a reset in between, is refused with P3D_ERR_INVALID and changes nothing.
 * p3d_scene_camera returns the scene's current camera (reserved = 0).
 */
int p3d_camera_look_at(const float from[3], const float at[3], const float up[3], float angle, int32_t res_x, int32_t res_y,
                       float aperture_ratio, float focal_ratio, p3d_camera* out);
int p3d_scene_set_camera(p3d_scene* scene, const p3d_camera* camera);
int p3d_scene_camera(p3d_scene* scene, p3d_camera* out);

/*
 * Moving the OBJECTS of a device scene between frames, without a new scene.  Detected by the symbols (P3D_ABI_VERSION is
 * unchanged).  Only for scenes of p3d_scene_create_device_bvh: the linear BVH is brought up to date on the device, in place.
 *
 * p3d_scene_update_prims replaces the `n` objects object[0..n) by prims[0..n) (whole p3d_prim records: geometry, normal and
 * box, as p3d_host_scene_desc hands them out after p3d_host_scene_set_geometry) and then
 *   P3D_UPDATE_REFIT   keeps the tree's topology and leaf order and recomputes every node box bottom-up: cheap, exact for the
 *                      tree it keeps, but the tree fits the scene less well the further objects have moved;
 *   P3D_UPDATE_REBUILD runs the whole build again in a workspace the scene keeps (no allocation per call): node and leaf
 *                      arrays are, bit for bit, those p3d_scene_create_device_bvh builds for the updated descriptor.
 *                      n = 0 is allowed: it re-sorts a tree that many refits have degraded.
 * Frames enqueued after the call see the new geometry.  Like p3d_scene_set_camera it is a host call that WAITS (tail stream,
 * then the whole device, then for its own launches) and cannot be captured into a graph.  It forgets the tile-cost schedules
 * and the hit_stack hand-off's row chains and halo pixels, refreshes the root box, and a p3d_accum or p3d_adaptive refuses
 * passes (P3D_ERR_INVALID, nothing changed) until it is reset.  p3d_temporal knows nothing of it: it reprojects with the camera
 * only, so the caller resets it or accepts ghosting on moved objects.  The first update of a scene allocates the builder's
 * state (about 150 bytes per object), which p3d_scene_destroy frees.
 * *update_ms (may be NULL): GPU time between two events around the staging copy and the launches.
 * A scene with a device-built grid (p3d_scene_build_grid, below) keeps it: in both modes the grid is rebuilt in full after the
 * BVH work, inside *update_ms.  If that rebuild fails the call returns its error (P3D_ERR_CAPACITY, P3D_ERR_NO_DEVICE): the
 * geometry and the BVH ARE updated, and the scene has no grid until p3d_scene_build_grid succeeds again.
 * Refused with P3D_ERR_INVALID, nothing changed: a scene of p3d_scene_create; a scene created with the host's grid in its
 * descriptor (it would go stale);
 * an object index out of range or repeated within the call; a record whose type or material differs from the object's
 * (emitter list and kernel selection stay valid); a non-finite or inverted bmin / bmax; an unknown mode; NULL arrays with n > 0.
 *
 * p3d_scene_export_bvh returns the scene's current device-built tree in the descriptor's format (p3d_bvh_node: children
 * adjacent and behind their parent, leaves as ranges of prim_index), relabelled on the host by a depth-first walk from the
 * root, left child first: exactly what p3d_scene_create accepts as bvh_nodes / bvh_prim_index / bvh_max_depth.  *n_nodes and
 * *n_prim_index hold the capacities of the arrays on entry and the sizes on return; with nodes == NULL only the sizes are
 * returned.  P3D_ERR_CAPACITY if an array is too small, P3D_ERR_INVALID for a scene of p3d_scene_create.  max_depth may be NULL.
 */
typedef enum p3d_update_mode { P3D_UPDATE_REFIT = 0, P3D_UPDATE_REBUILD = 1 } p3d_update_mode;
int p3d_scene_update_prims(p3d_scene* scene, uint32_t n, const uint32_t* object, const p3d_prim* prims,
                           uint32_t mode, float* update_ms);
int p3d_scene_export_bvh(p3d_scene* scene, p3d_bvh_node* nodes, uint32_t* n_nodes, uint32_t* prim_index,
                         uint32_t* n_prim_index, uint32_t* max_depth);

/*
 * The QUALITY of a device-built tree, and a refit that rebuilds by itself.  Detected by the symbols (P3D_ABI_VERSION and
 * p3d_update_mode are unchanged).  The same scenes as p3d_scene_update_prims.
 *
 * The cost is the surface-area estimate with traversal and intersection cost both 1, stated on the tree
 * p3d_scene_export_bvh returns (float32 boxes):
 *   A(node) = (dx dy + dy dz) + dz dx,  dx = (double)bmax[0] - (double)bmin[0], dy, dz alike: float64, left to right, no
 *             contraction
 *   sah     = (sum over inner nodes A(node) + sum over leaves count(leaf) A(leaf)) / A(root)
 * The root counts like any node.  A(root) == 0 (or not above 0), or no objects: sah = 0.  One object is one leaf: sah = 1.
 * The sum is taken on the device in an order that depends on the number of objects alone (no floating-point atomics): the
 * same tree gives the same bits, on every call and on every scene that holds it.  Against another summation order of the
 * same terms it differs by rounding only (relative n 2^-53).
 *
 * p3d_scene_bvh_cost measures the scene's current tree.  Like p3d_scene_export_bvh it is a host call that WAITS (tail stream,
 * then the whole device, then for its two short launches and 32 bytes read back).  It allocates the builder's state if the
 * scene has none; on a scene that was never updated it recovers the topology and runs the fit over the boxes the tree was
 * built from, which rewrites the node array with the same bits.  It changes no frame, schedule or generation counter.
 *
 * p3d_scene_set_auto_rebuild(ratio): 0 = off, the default: every call behaves, and launches, as without it.  With a ratio >= 1
 * (+inf allowed: measure, never rebuild) an update called with P3D_UPDATE_REFIT, through p3d_scene_update_prims or
 * p3d_scene_transform_prims, refits, measures the refitted tree, and if sah > ratio * sah_baseline (strict, float64) runs the
 * builder in the same call.  The result of such a promoted update is, bit for bit, that of the same update called with
 * P3D_UPDATE_REBUILD; the result of one that is not promoted is that of a plain REFIT.  A device-built grid is rebuilt once,
 * after the final tree, and *update_ms covers all of it.  P3D_UPDATE_REBUILD is unchanged except that, with the policy on, it
 * measures the new tree as the new baseline.
 * sah_baseline is the cost of the tree at the latest of: create, as long as no update has run since (recorded by the first
 * p3d_scene_bvh_cost; the same holds for any tree that no refit has touched since it was built); an update that ran the
 * builder with the policy on; the moment the policy was switched on (off -> a ratio; changing the ratio keeps it).  With the
 * policy off an update voids it (0 = none recorded), and so does switching the policy off.
 * p3d_scene_auto_rebuild returns the ratio.
 * Refused with P3D_ERR_INVALID, nothing changed: null arguments; a scene of p3d_scene_create; a ratio that is NaN, negative or
 * inside (0, 1).
 */
typedef struct p3d_bvh_cost {   /* 32 bytes */
  double sah;                   /* the scene's current tree */
  double sah_baseline;          /* the tree the policy compares against; 0 = none recorded */
  uint32_t n_inner, n_leaves;   /* of the exported tree */
  uint32_t refits_since_build;  /* updates that kept the topology since it was last built */
  uint32_t last_update_rebuilt; /* 1: the last update ran the builder (REBUILD, or a REFIT the policy promoted) */
} p3d_bvh_cost;
int p3d_scene_bvh_cost(p3d_scene* scene, p3d_bvh_cost* out);
int p3d_scene_set_auto_rebuild(p3d_scene* scene, float ratio);
int p3d_scene_auto_rebuild(p3d_scene* scene, float* ratio);

/*
 * Moving objects by TRANSFORMS, applied on the device.  Detected by the symbol (P3D_ABI_VERSION is unchanged).  The same
 * scenes as p3d_scene_update_prims, and the same call from the BVH work onwards; what differs is where the new geometry comes
 * from: the caller sends 64 bytes per transform and 16 bytes per range of objects, and a kernel moves the objects and does
 * what the host's constructors do (triangle normal, boxes).
 *
 * Rest pose.  Every object has a REST geometry: the nine floats it was created with or was last given by
 * p3d_scene_update_prims.  p3d_scene_transform_prims sets every object of ranges[i] = [first, first + count) to
 * xforms[ranges[i].xform](rest) - never to T(current): calling it every frame with that frame's absolute pose accumulates no
 * rounding.  Objects that no range names keep their current geometry.  The rest copy (48 bytes per object) is made by the
 * first call from the scene's geometry of that moment and freed by p3d_scene_destroy; from then on p3d_scene_update_prims
 * writes it too for the objects it replaces.
 *
 * Arithmetic: float32, left to right, no contraction (host/prim_rule.hpp, shared with the host's constructors).
 *   point    x' = ((m[0] x + m[1] y) + m[2] z) + m[3], y' from m[4..7], z' from m[8..11]
 *   triangle the three vertices as points; normal and box as the loader computes them from those vertices
 *   sphere   the centre as a point; radius' = radius * sphere_scale; box = centre -+ radius'
 *   box      min and max as points; accepted only if m[0], m[5], m[10] > 0 and the six off-diagonal entries are exactly 0
 * The result is, bit for bit, what p3d_host_scene_set_geometry + p3d_scene_update_prims give for the same numbers.  (The
 * identity returns the rest bits except that a coordinate -0 comes back as +0: 1 * -0 + 0 is +0.)
 *
 * Behaviour: modes, the device-grid rebuild inside *update_ms, the waits, the forgotten schedules and row chains, the root
 * box, and accumulators refusing passes until reset are those of p3d_scene_update_prims.  n_ranges = 0 is allowed.  The
 * staging for ranges and transforms grows when needed and is kept: a second call of the same size allocates nothing.
 * Overflow: finite inputs can still overflow.  An object whose new box would be non-finite or inverted is NOT written and
 * keeps its current geometry; the other objects are updated, the BVH and grid work runs, and the call returns
 * P3D_ERR_INVALID with the number of such objects in p3d_last_error.
 * Refused with P3D_ERR_INVALID, nothing changed: a null scene; a scene of p3d_scene_create; a scene with an uploaded grid;
 * NULL arrays with non-zero counts; an unknown mode; a range with count = 0, first + count > the object count,
 * xform >= n_xforms or reserved != 0; ranges that overlap (their order is free); a non-finite m or sphere_scale;
 * sphere_scale <= 0; reserved != 0 in a transform; a range that covers a plane; a range that covers a box with a transform
 * that is not positive-diagonal.
 */
typedef struct p3d_xform { /* 64 bytes */
  float m[12];             /* row-major 3x4 */
  float sphere_scale;      /* radius' = radius * sphere_scale; > 0 */
  uint32_t reserved[3];    /* must be 0 */
} p3d_xform;
typedef struct p3d_xform_range { /* objects [first, first + count) take xforms[xform] */
  uint32_t first, count, xform, reserved;
} p3d_xform_range;
int p3d_scene_transform_prims(p3d_scene* scene, uint32_t n_ranges, const p3d_xform_range* ranges, uint32_t n_xforms,
                              const p3d_xform* xforms, uint32_t mode, float* update_ms);

/*
 * New geometry for triangles and spheres FROM DEVICE MEMORY: a deforming mesh or a particle set that a GPU program keeps
 * (positions [V, 3] and indices [F, 3], or centres and radii [N, 4]) goes into the scene with one kernel and no host round
 * trip.  Detected by the symbol (P3D_ABI_VERSION and p3d_update_mode are unchanged).  The same scenes as
 * p3d_scene_update_prims, and the same call from the BVH work onwards.
 *
 * Every object of sources[i] = [first, first + count) gets its nine geometry floats from the buffers: triangle k of a source
 * takes the positions d_index[3k], d_index[3k + 1], d_index[3k + 2] of d_data (without d_index: 3k, 3k + 1, 3k + 2), sphere k
 * takes d_data[4k .. 4k + 3].  The kernel computes the triangle normal and box, or the sphere box, with the arithmetic of the
 * host's constructors (host/prim_rule.hpp) and writes what p3d_scene_update_prims writes - geometry, shading normal, box,
 * and the rest copy of p3d_scene_transform_prims if the scene has one (a deformed object rests where it is put).  Type,
 * material and index of an object stay.  The result is, bit for bit, what p3d_host_scene_set_geometry +
 * p3d_scene_update_prims give for the same numbers, with one exception: the normal of a zero-area triangle is NaN on both
 * routes and its bit pattern (sign, payload) is unspecified.  The bound host scene is not touched.
 *
 * Ordering.  Like every update the call WAITS before its kernel: for the scene's tail stream, then for the whole device.
 * Whatever any stream of this device had enqueued to fill the buffers before the call has therefore finished; that is why
 * there is no stream argument (a stream could only promise less).  The buffers are only read, and they may be freed or
 * overwritten once the call returns.  Modes, the auto-rebuild policy, the device-grid rebuild inside *update_ms, the
 * forgotten schedules and row chains, the root box and accumulators refusing passes until reset are those of
 * p3d_scene_update_prims; p3d_temporal knows nothing of it.  n_sources = 0 is allowed and behaves like
 * p3d_scene_update_prims with n = 0; a scene without objects returns P3D_OK.  The staging for the source table grows when
 * needed and is kept: a second call of the same size allocates nothing.
 *
 * Per-object failures, found by the kernel: a triangle with an index >= n_elems (checked before anything is read through
 * it: nothing outside [0, n_elems) of d_data or [0, 3 count) of d_index is ever read), and an object whose new box is
 * non-finite or inverted (a NaN or infinite position, a negative or NaN radius).  Such an object is NOT written and keeps its
 * current geometry; the others are updated, the BVH and grid work runs, and the call returns P3D_ERR_INVALID with the two
 * counts, separately, in p3d_last_error.
 * Refused with P3D_ERR_INVALID, nothing changed, before any launch: a null scene; a scene of p3d_scene_create; a scene with an
 * uploaded grid; an unknown mode; NULL sources with n_sources > 0; a source with count = 0, with first + count > the object
 * count, with a kind other than P3D_PRIM_TRIANGLE / P3D_PRIM_SPHERE, or that covers an object of another type; NULL d_data;
 * d_data or d_index not 4-byte aligned; d_index given for spheres; n_elems = 0; a soup with n_elems != 3 count; spheres with
 * n_elems != count; reserved != 0; sources that overlap (their order is free).  A d_data or d_index that the HIP runtime
 * identifies as host memory (registered or not), or as memory of another device, is refused too, and so is a buffer that
 * ends behind the allocation the runtime reports for it.  A pointer the runtime cannot answer for is let through.
 */
typedef struct p3d_geom_source {  /* 48 bytes */
  uint32_t first, count;     /* objects [first, first + count), all of type `kind` */
  uint32_t kind;             /* P3D_PRIM_TRIANGLE or P3D_PRIM_SPHERE */
  uint32_t n_elems;          /* triangles: number of positions in d_data; spheres: must equal count */
  const void* d_data;        /* DEVICE memory, float32, 4-byte aligned.  triangles: n_elems x 3 (x y z);
                                spheres: count x 4 (centre x y z, radius) */
  const uint32_t* d_index;   /* triangles only, DEVICE memory, count x 3: triangle k has positions d_index[3k..3k+2].
                                NULL = soup: triangle k has positions 3k, 3k+1, 3k+2, and n_elems must equal 3 * count.
                                Must be NULL for spheres. */
  uint64_t reserved[2];      /* must be 0 */
} p3d_geom_source;
int p3d_scene_update_geometry_device(p3d_scene* scene, uint32_t n_sources, const p3d_geom_source* sources,
                                     uint32_t mode, float* update_ms);

/*
 * The REFIT of p3d_scene_update_geometry_device ENQUEUED ON THE CALLER'S STREAM, without a wait: a simulation step that
 * produces positions on a stream hands them to the scene and asks rays of it (p3d_trace_*_device) or renders it, and the host
 * is never in the loop.  Detected by the symbol (P3D_ABI_VERSION and p3d_update_mode are unchanged).  `sources` are the
 * records of p3d_scene_update_geometry_device, with the same meaning.
 *
 * What it writes: object-order geometry, shading normal, box, and the rest copy if the scene has one; then the REFIT of the
 * kept topology - node records and leaf-order geometry.  All of it is, bit for bit, what
 * p3d_scene_update_geometry_device(..., P3D_UPDATE_REFIT, ...) leaves for the same buffers (boxes are exact min / max and
 * the keys are unique), with that call's one exception: the NaN normal of a zero-area triangle.  The tree's depth stands: a
 * refit keeps the topology.
 *
 * Stream.  Everything is enqueued on hip_stream (NULL = the default stream) under the scene's stream rules
 * (p3d_render_tile_device): keep one scene's work on one stream, or order the streams with events.  What the stream had
 * enqueued to produce the buffers runs first; frames and queries enqueued on that stream after the call see the new
 * geometry; the buffers may be reused once the stream has passed the call.  With a tail stream set, the launch first joins a
 * pending tail with hipStreamWaitEvent, as p3d_trace_*_device does.  The sources travel as kernel arguments - nothing of the
 * call has to outlive it - so there are at most 16 per call: more is P3D_ERR_CAPACITY (the waiting form stages any number).
 * Capturing the call into a graph is not supported.
 *
 * Which calls may wait.  The FIRST p3d_scene_refit_device of a scene allocates the two failure counters and, unless an
 * earlier update, grid build or cost query has made them, the builder's state and the tree's topology, as the waiting forms
 * do: it waits for the tail stream and the device.  So does the first call after a geometry update that failed with
 * P3D_ERR_NO_DEVICE (which voids the topology).  Every other call neither allocates, nor frees, nor waits for the device, nor
 * copies anything back.  There is no update_ms: time the stream.
 *
 * Per-object failures (an index >= n_elems; a new box that is non-finite or inverted) are found by the kernel as in the
 * waiting form: the object keeps its geometry, the others are updated, and THE CALL RETURNS P3D_OK.  The kernel counts the two
 * kinds in a block the scene owns and raises a flag: p3d_scene_status then returns P3D_ERR_INVALID with the two counts since
 * the last check in p3d_last_error, and clears both (with capacity flags pending too it returns P3D_ERR_CAPACITY and the
 * message carries both).  Render calls never report them: the check behind a call with `stats` leaves this flag pending.
 *
 * On return, without a wait: accumulators and adaptive frames refuse passes until reset, the hit_stack row chains are
 * forgotten, p3d_bvh_cost.refits_since_build is one more, last_update_rebuilt is 0 and sah_baseline is void, as after
 * a waiting REFIT with the policy off.  The memoised tile schedules are not freed (that would wait): each is recorded
 * again, in the memory it holds, by the next frame with its key.  The cached root box - it only cuts the ray bins of
 * P3D_CHAIN_PER_LEVEL, and never changes a result - goes stale; the next call on the scene that waits for the device anyway
 * (a waiting update, p3d_scene_status, p3d_scene_export_bvh, p3d_scene_bvh_cost, p3d_scene_set_auto_rebuild switching on,
 * p3d_scene_set_camera) brings it up to date, and a P3D_CHAIN_PER_LEVEL frame that still finds it stale first waits for
 * its stream and reads it back: THAT FRAME MAY WAIT.
 *
 * Refused, nothing enqueued and nothing changed: everything p3d_scene_update_geometry_device refuses before its launch, in
 * the same words (mode apart); P3D_ERR_UNSUPPORTED for a scene with a device-built grid (its rebuild reads sizes back) and
 * for a scene whose auto-rebuild ratio is not 0 (the policy needs the cost on the host): both take the waiting form.
 * n_sources = 0 returns P3D_OK and enqueues nothing.
 */
int p3d_scene_refit_device(p3d_scene* scene, uint32_t n_sources, const p3d_geom_source* sources, void* hip_stream);

/*
 * The REFIT of p3d_scene_transform_prims ENQUEUED ON THE CALLER'S STREAM, without a wait: a rigid-body or robot simulation
 * that produces one 3x4 pose per body per step in device memory hands the poses to the scene and asks rays of it or renders
 * it, and the host is never in the loop.  Detected by the symbols (P3D_ABI_VERSION and p3d_update_mode are unchanged).  The
 * same scenes as p3d_scene_transform_prims.  Which objects follow which body does not change from step to step, only the
 * matrices do: the ranges are given once, as a RIG, by a call that may wait; the pose call takes the matrices and a stream.
 *
 * p3d_scene_set_rig: objects [first, first + count) of ranges[i] follow transform slot ranges[i].xform of later poses, with
 * the meaning the records have in p3d_scene_transform_prims; objects that no range names are never touched.  n_xforms is the
 * number of slots every later pose must bring.  The call waits for the tail stream and the device, as every update does, and
 * makes what a pose needs and may not wait for: the rest copy, from the scene's geometry of this moment if the scene has none
 * (the rule of the first p3d_scene_transform_prims); the builder's state and the tree's topology; two failure counters; and
 * the rig on the device, one word per object (4 bytes per object, whatever the number of ranges).  A second call replaces the
 * rig; n_ranges = 0 removes it and frees the table.  The rig survives every geometry update, REBUILD included (objects keep
 * their types and indices).  Refused with P3D_ERR_INVALID, nothing changed: a null scene; a scene of p3d_scene_create; a
 * scene with an uploaded grid; NULL ranges with n_ranges > 0; n_ranges > 0 with n_xforms = 0; a range with count = 0, first +
 * count > the object count, xform >= n_xforms or reserved != 0; ranges that overlap (their order is free); a range that
 * covers a plane.  A box IS accepted: whether a matrix suits it is only known on the device (see below).
 * p3d_scene_rig: the ranges and slots of the current rig and the objects it covers; three zeros without one.
 *
 * p3d_scene_pose_device: every rigged object becomes d_xforms[its slot](rest), with radius' = radius * d_sphere_scale[its
 * slot] for a sphere, by the arithmetic of p3d_scene_transform_prims; then the REFIT of the kept topology.  What the call
 * leaves - object-order geometry, shading normals, boxes, node records, leaf-order geometry - is, bit for bit, what
 * p3d_scene_transform_prims(the rig's ranges, the same numbers, P3D_UPDATE_REFIT) leaves.  The rest copy is not written.
 * d_xforms: n_xforms x 12 float32 in DEVICE memory, row-major 3x4, one matrix per slot (a contiguous [K, 3, 4] tensor);
 * d_sphere_scale: n_xforms float32 in DEVICE memory, or NULL = 1 for every slot.  4-byte alignment is enough.
 *
 * Stream, and which calls may wait: as p3d_scene_refit_device.  Everything is enqueued on hip_stream (NULL = the default
 * stream); what the stream had enqueued to produce the matrices runs first, frames and queries enqueued on it afterwards see
 * the new pose, and the buffers may be reused once the stream has passed the call.  A pending tail stream is joined with
 * hipStreamWaitEvent.  On a rigged scene the call neither allocates, nor frees, nor waits for the device, nor copies anything
 * back, and returns while the stream may still be busy (the one exception: the first call after a geometry update that
 * failed with P3D_ERR_NO_DEVICE, which makes the topology again).  What it leaves on the host - accumulators refusing
 * passes, forgotten row chains, refits_since_build, the tile schedules recorded again in place, the stale root box and the
 * P3D_CHAIN_PER_LEVEL frame that may wait for it - is what p3d_scene_refit_device leaves.  Capturing the call into a graph is
 * not supported.
 *
 * Per-object skips, found by the kernel (the host cannot see the numbers: these are the checks the waiting form makes on the
 * host, made per object).  An object keeps its current geometry, and is counted in the first of two counters, if its
 * transform has a non-finite entry among the 12, if its sphere_scale is not finite and > 0 (whatever the object's type, as
 * the waiting form refuses such a transform whatever it moves), or if it is a box and the matrix is not positive-diagonal
 * (m[0], m[5], m[10] > 0 and the six off-diagonal entries exactly 0).  It keeps its geometry and is counted in the second
 * if its new box is non-finite or inverted (finite inputs can overflow).  The other objects are updated and THE CALL RETURNS
 * P3D_OK; p3d_scene_status then returns P3D_ERR_INVALID with the two counts since the last check in p3d_last_error and
 * clears both, exactly as for the skips of p3d_scene_refit_device (with capacity flags pending too it returns
 * P3D_ERR_CAPACITY and the message carries both; render calls never report them).
 *
 * Refused, nothing enqueued and nothing changed: P3D_ERR_INVALID for a null scene, a scene of p3d_scene_create, a scene with
 * an uploaded grid, a scene without a rig, n_xforms other than the rig's, NULL d_xforms, a pointer that is not 4-byte
 * aligned, and a buffer that the HIP runtime identifies as host memory or memory of another device or that ends behind its
 * allocation (48 n_xforms bytes, 4 n_xforms for the scales; a pointer the runtime cannot answer for is let through);
 * P3D_ERR_UNSUPPORTED for a scene with a device-built grid and for a scene whose auto-rebuild ratio is not 0: both take
 * p3d_scene_transform_prims.  A scene without objects returns P3D_OK.
 */
int p3d_scene_set_rig(p3d_scene* scene, uint32_t n_ranges, const p3d_xform_range* ranges /* HOST */, uint32_t n_xforms);
int p3d_scene_rig(p3d_scene* scene, uint32_t* n_ranges, uint32_t* n_xforms, uint32_t* n_posed_objects);
int p3d_scene_pose_device(p3d_scene* scene, uint32_t n_xforms,
                          const void* d_xforms,        /* DEVICE, float32, n_xforms x 12, row-major 3x4, 4-byte aligned */
                          const void* d_sphere_scale,  /* DEVICE, float32, n_xforms; NULL = 1 for every transform */
                          void* hip_stream);

/*
 * The uniform grid of a live scene, built on the device.  Detected by the symbols (P3D_ABI_VERSION is unchanged).  Only for
 * scenes of p3d_scene_create_device_bvh, which keep their objects' boxes on the device and accept updates.
 *
 * p3d_scene_build_grid builds, or builds again, the scene's grid from the current object boxes: bounds, cell counts,
 * cell_start and cell_items are, bit for bit, those of Grid::Build (grid.cpp:3-68; p3d_host_scene_desc with build_grid = 1)
 * for the same objects, every cell's list in ascending object index.  After it accel = P3D_ACCEL_GRID works on the scene in
 * every render, accumulate, adaptive, feature and query entry point, with the results of a scene created with the host's grid,
 * and p3d_scene_update_prims rebuilds the grid with every update.  Like an update it is a host call that WAITS (tail stream,
 * then the whole device, then for its own launches) and cannot be captured into a graph; it forgets the tile-cost schedules.
 * The first build allocates the builder's state (that of the first update, if none has run, and about 40 bytes per object
 * plus 16 bytes per cell item); the cell arrays and that state grow when a later build needs more, are kept otherwise - a
 * rebuild that fits allocates nothing - and are freed by p3d_scene_destroy.
 * *build_ms (may be NULL): GPU time between two events around the launches.
 * Refused with P3D_ERR_INVALID, nothing changed: a null scene; a scene of p3d_scene_create; a scene whose descriptor carried a
 * grid at create (it has the host's grid, and stays refused by updates).  P3D_ERR_UNSUPPORTED: a scene with no objects; a
 * scene created with a non-finite or inverted box.  P3D_ERR_CAPACITY: a cell count along an axis that does not fit an int;
 * more than 2^28 cells in all (a stated limit, not a measured one: 1 GiB of cell_start); more cell items than a uint32
 * counts; an allocation that fails.  After a failed build the scene has NO grid (accel = P3D_ACCEL_GRID is refused as for a
 * scene created without one); its BVH is untouched.
 *
 * p3d_scene_export_grid returns the device-built grid in the descriptor's format.  *n_cell_start and *n_cell_items hold the
 * capacities of the arrays on entry and the sizes (n_cells + 1, n_items) on return; `info` receives nx, ny, nz, bmin, bmax,
 * n_cells and n_items, its pointers are NULL.  With cell_start == NULL only `info` and the sizes are returned.
 * P3D_ERR_CAPACITY if an array is too small (nothing is written to the arrays), P3D_ERR_INVALID for a scene without a
 * device-built grid.
 */
int p3d_scene_build_grid(p3d_scene* scene, float* build_ms /* may be NULL */);
int p3d_scene_export_grid(p3d_scene* scene, p3d_grid_desc* info, uint32_t* cell_start, uint32_t* n_cell_start,
                          uint32_t* cell_items, uint32_t* n_cell_items);

/*
 * Progressive accumulation: one anti-aliased frame rendered in passes over its samples, the image shown (or the frame
 * stopped) after any of them - what the reference's drawModeEnabled display (main.cpp:45-48) does line by line, by sample
 * instead.  A caller detects these entry points by the symbols being present (P3D_ABI_VERSION is unchanged).
 *
 * p3d_accum_create copies `cfg` and `tile` and allocates, on the scene's device, w*h running sums (3 float) and w*h first
 * hits.  An accumulator belongs to its scene: destroy it before the scene.  Every pass renders samples [done, done + n) of
 * every pixel of the tile, adds them to the running sums in sample order and advances `done`:
 *   rgb    : sum / (float)done - after the last pass exactly sum / (float)(SPP*SPP), main.cpp:800
 *   rgb8   : gamma + u8fromfloat of that value
 *   hit_id : the first sample's primary hit, kept in the accumulator and written by every pass
 * Exactness: every (pixel, sample) draws from its own RNG stream and a pixel's samples are added one at a time in sample
 * order whatever the pass boundaries, so the pass that completes SPP*SPP samples writes the same bits as
 * p3d_render_tile(_device) of the same cfg / tile, and any two partitions of samples [0, m) give the same bits after m.
 * Summed over the passes of a frame, the rays_* / *_tests / shaded_hits counters equal the one-shot frame's; p3d_stats
 * describes one pass (pixels = w*h per pass).
 *
 * Accepted: cfg->antialiasing = 1; every PATHTRACE configuration; WHITTED with P3D_STACK_PER_PIXEL or accel != BVH.
 * Refused at create with P3D_ERR_UNSUPPORTED: antialiasing = 0 (no sample loop), and WHITTED + BVH + P3D_STACK_LITERAL
 * (the serial order hands the hit_stack from pixel p's last sample to pixel p+1's first: no split over samples keeps it).
 * A pass with n == 0 or done + n > SPP*SPP returns P3D_ERR_INVALID and changes nothing.  After a pass that returned an
 * error the accumulator refuses passes (P3D_ERR_INVALID) until p3d_accum_reset, which goes back to 0 samples.
 *
 * p3d_accum_render is the host-buffer form (synchronous).  p3d_accum_render_device enqueues the pass on `hip_stream`
 * under the scene's stream rules (p3d_render_tile_device): without `stats` it returns without waiting, and an error the
 * device detects shows in p3d_scene_status - after such an error, reset every accumulator of the scene rendered since
 * the last check.  Output pointers may be NULL.
 */
typedef struct p3d_accum p3d_accum;
int p3d_accum_create(p3d_scene* scene, const p3d_config* cfg, const p3d_tile* tile, p3d_accum** out);
void p3d_accum_destroy(p3d_accum* acc);
int p3d_accum_reset(p3d_accum* acc);
uint32_t p3d_accum_samples_done(const p3d_accum* acc);
int p3d_accum_render(p3d_accum* acc, uint32_t n, float* rgb, int32_t* hit_id, uint8_t* rgb8, p3d_stats* stats);
int p3d_accum_render_device(p3d_accum* acc, uint32_t n, float* d_rgb, int32_t* d_hit_id, uint8_t* d_rgb8,
                            void* hip_stream, p3d_stats* stats);

/*
 * Adaptive sampling: a progressive path-traced frame (p3d_accum above) whose pixels stop taking samples once they have
 * converged, so that later passes cost in proportion to the pixels still noisy.  Detected by its symbols, like p3d_accum.
 *
 * Passes.  A pass of n samples renders samples [done, done + n) of every ACTIVE pixel and then advances `done` by n, even
 * when no pixel is active.  The rules of p3d_accum for n, for failures and for reset hold unchanged: n == 0 or
 * done + n > SPP*SPP is P3D_ERR_INVALID and changes nothing; after a failed pass, passes are refused until
 * p3d_adaptive_reset (0 samples, every pixel active again).  Every pass writes EVERY pixel of the tile to each non-NULL
 * output:  rgb = sum / (float)samples_p,  rgb8 = gamma + u8fromfloat of that value,  hit_id = sample 0's primary hit,
 *          samples = samples_p, the samples in the pixel's sum (w*h uint32).
 * Exactness: a pixel that stopped after k samples holds exactly the bits a plain p3d_accum holds for it after k samples
 * (same RNG streams, same additions in sample order, same epilogue); a pixel that never stops holds the one-shot frame's.
 *
 * Decision, at the end of a pass only: a pixel becomes inactive for good when samples_p >= min_samples, the denominator
 * m + 1.0e-3f of rel_err_p is positive (rel_err_p has a clear sign bit) and rel_err_p < rel_error (strict: rel_error = 0
 * never stops a pixel).  The reference's radiance can be negative behind glass: a pixel whose mean luminance m is -1.0e-3f
 * or less has no relative error to speak of (rel_err_p is negative, -0, inf or NaN) and goes on taking samples.
 * Error metric, float32 on the device in this order, without contraction:
 *   per sample radiance L added to the sum:  y = 0.2126f*L.x + 0.7152f*L.y + 0.0722f*L.z;  S2 += y*y  (sample order)
 *   n = (float)samples_p;  Y = 0.2126f*S.x + 0.7152f*S.y + 0.0722f*S.z;  m = Y / n;
 *   v = fmaxf((S2 - Y*m) / (n - 1.0f), 0.0f);  rel_err = sqrtf(v / n) / (m + 1.0e-3f)
 *
 * Refused at create: P3D_ERR_UNSUPPORTED for integrator = WHITTED (its anti-aliased frames have few, cheap samples) and
 * antialiasing = 0; P3D_ERR_INVALID for a NaN or negative rel_error, min_samples outside [2, SPP*SPP], or non-zero
 * reserved fields.  One device only.
 * Stats describe one pass: pixels = the pixels rendered (the active ones); with collect_stats, rays_primary summed over
 * a frame's passes equals the sum over pixels of samples_p.
 *
 * p3d_adaptive_render is the host-buffer form (synchronous).  p3d_adaptive_render_device follows
 * p3d_accum_render_device's stream and error rules: without `stats` it returns without waiting for the device.
 * p3d_adaptive_active_pixels (the pixels the next pass renders) and p3d_adaptive_read_state (per pixel: the running sum,
 * 3 float; S2; samples_p; rel_err of the pixel's last pass) wait for the device.  Any output pointer may be NULL.
 */
typedef struct p3d_adaptive_params {
  float rel_error;       /* a pixel stops once its rel_err is < rel_error (see "Decision"); 0 = no pixel ever stops */
  uint32_t min_samples;  /* no pixel stops before this many samples; 2 <= min_samples <= SPP*SPP */
  uint32_t reserved[2];  /* must be 0 */
} p3d_adaptive_params;
typedef struct p3d_adaptive p3d_adaptive;
int p3d_adaptive_create(p3d_scene* scene, const p3d_config* cfg, const p3d_tile* tile, const p3d_adaptive_params* params,
                        p3d_adaptive** out);
void p3d_adaptive_destroy(p3d_adaptive* ad);
int p3d_adaptive_reset(p3d_adaptive* ad);
uint32_t p3d_adaptive_samples_done(const p3d_adaptive* ad);
int p3d_adaptive_active_pixels(p3d_adaptive* ad, uint32_t* n);
int p3d_adaptive_render(p3d_adaptive* ad, uint32_t n, float* rgb, int32_t* hit_id, uint8_t* rgb8, uint32_t* samples,
                        p3d_stats* stats);
int p3d_adaptive_render_device(p3d_adaptive* ad, uint32_t n, float* d_rgb, int32_t* d_hit_id, uint8_t* d_rgb8,
                               uint32_t* d_samples, void* hip_stream, p3d_stats* stats);
int p3d_adaptive_read_state(p3d_adaptive* ad, float* sum, float* sum_y2, uint32_t* samples, float* rel_err);

/*
 * Denoising: feature buffers (AOVs) of a tile's primary rays, and an edge-avoiding a-trous wavelet filter (Dammertz et al.
 * 2010; with a variance buffer, the luminance term of SVGF, Schied et al. 2017) that uses them - what a display loop runs
 * behind every pass of a progressive frame.  Detected by its symbols, like p3d_accum (P3D_ABI_VERSION is unchanged).
 *
 * p3d_render_features traces the primary rays of samples [0, K) of every pixel of the tile - the rays the integrators trace:
 * the (pixel, sample) RNG stream, the jitter / tent / lens sample of cfg, the closest-hit traversal of cfg->accel on an
 * empty stack - and writes two w*h*4 float buffers, each averaged over the samples whose primary ray hit something:
 *   normal_depth : (n.x, n.y, n.z, t)  n = the shading normal turned against the ray (main.cpp:366-368), the mean NOT
 *                  renormalised (shorter than 1 on silhouettes); t = the traversal's closest-hit distance (p3d_trace_closest)
 *   albedo_cov   : (diff_color, coverage)  coverage = the fraction of the K samples that hit; 0 = every component 0
 * K = samples; 0 means min(16, SPP*SPP).  antialiasing = 0 has only the pixel-centre ray: K <= 1.  Either integrator,
 * every accel.  P3D_ERR_INVALID for K > the frame's samples; P3D_ERR_UNSUPPORTED for a striped tile (stripe_stride > 1).
 * The device form enqueues one launch on `hip_stream` under the scene's stream rules (p3d_render_tile_device) and
 * returns without waiting; its buffers must be 16-byte aligned.
 */
int p3d_render_features(p3d_scene* scene, const p3d_config* cfg, const p3d_tile* tile, uint32_t samples, float* normal_depth,
                        float* albedo_cov);
int p3d_render_features_device(p3d_scene* scene, const p3d_config* cfg, const p3d_tile* tile, uint32_t samples,
                               float* d_normal_depth, float* d_albedo_cov, void* hip_stream);

/*
 * The filter.  Iteration i = 0 .. iterations-1 has step s = 2^i; pixel p takes the taps q = p + s*(dx, dy), dx, dy in
 * {-2 .. 2}, that lie in the w x h image, each with weight
 *   h   = k[dx] k[dy],  k = (1/16, 1/4, 3/8, 1/4, 1/16)
 *   w_g = 1 if cov_p == 0 and cov_q == 0;  0 if exactly one of them is 0;  otherwise
 *         max(0, n_p.n_q)^sigma_normal * exp(-|t_p - t_q| / (sigma_depth * s * t_p)) * exp(-|a_p - a_q|^2 / sigma_albedo^2)
 *         (a term whose sigma is 0 is left out)
 *   w_c = exp(-|Y_p - Y_q| / (sigma_luma * sqrt(v_p) + 1e-4))   with a variance buffer;  Y = 0.2126 R + 0.7152 G + 0.0722 B
 *         exp(-|c_p - c_q|^2 * 4^i / sigma_color^2)              without one
 *   w   = w_g * w_c, and 1 for the centre tap
 *   c'_p = sum(h w c_q) / sum(h w),   v'_p = sum((h w)^2 v_q) / sum(h w)^2   (the next iteration filters c', v')
 * in float32 (expf / powf / sqrtf, no contraction).  The last iteration writes out_rgb (w*h*3 float) and out_rgb8
 * (gamma + u8fromfloat, the render calls' epilogue); either may be NULL, not both.  iterations = 0 copies the input: out_rgb
 * is rgb, bit for bit, and out_rgb8 the rgb8 a render call writes for that rgb.
 * Inputs: rgb w*h*3 float (linear, before gamma), var w*h float (NULL: the colour-distance term), normal_depth and
 * albedo_cov as p3d_render_features writes them (required).  The outputs must not overlap the inputs.
 * P3D_ERR_INVALID: iterations > 8, a NaN or negative sigma, sigma_color <= 0 without variance or sigma_luma <= 0 with it,
 * gamma NaN or <= 0, non-zero reserved fields, null inputs.  p3d_denoise_params_default fills the defaults DESIGN.md
 * chose on the Cornell box (5 iterations, sigma_color 4, sigma_luma 64, sigma_normal 128, sigma_depth 1, sigma_albedo 0.1;
 * gamma 1 as p3d_config_default).
 *
 * A denoiser is made for one image size on one device: p3d_denoiser_create allocates the two float4 images the iterations
 * ping-pong between, so p3d_denoise_device neither allocates nor waits: it enqueues one launch per iteration on `hip_stream`
 * (behind a pass on that stream, or into a captured graph).  Its scratch is shared by its calls: enqueue the calls of one
 * denoiser on one stream.  Device buffers are HBM addresses on the denoiser's device; the feature buffers 16-byte aligned.
 * p3d_denoise is the host-buffer form (synchronous).
 */
typedef struct p3d_denoise_params {
  uint32_t iterations;  /* 0 .. 8 */
  float sigma_color;    /* colour distance, without a variance buffer (> 0) */
  float sigma_luma;     /* luminance distance in standard deviations, with a variance buffer (> 0) */
  float sigma_normal;   /* exponent of the normal term (0: off) */
  float sigma_depth;    /* relative depth difference per unit of step (0: off) */
  float sigma_albedo;   /* albedo distance (0: off) */
  float gamma;          /* GAMMA of the rgb8 output, as p3d_config.gamma */
  uint32_t reserved[2]; /* must be 0 */
} p3d_denoise_params;
void p3d_denoise_params_default(p3d_denoise_params* params);
typedef struct p3d_denoiser p3d_denoiser;
int p3d_denoiser_create(int device, int32_t w, int32_t h, p3d_denoiser** out);
void p3d_denoiser_destroy(p3d_denoiser* dn);
int p3d_denoise(p3d_denoiser* dn, const p3d_denoise_params* params, const float* rgb, const float* var, const float* normal_depth,
                const float* albedo_cov, float* out_rgb, uint8_t* out_rgb8);
int p3d_denoise_device(p3d_denoiser* dn, const p3d_denoise_params* params, const float* d_rgb, const float* d_var,
                       const float* d_normal_depth, const float* d_albedo_cov, float* d_out_rgb, uint8_t* d_out_rgb8,
                       void* hip_stream);
/*
 * The variance buffer of an adaptive frame: per pixel the variance of its mean luminance, v / n in the variables of the
 * "Error metric" above (float32, that order); 0 for a pixel with fewer than 2 samples.  Reads the adaptive state and
 * changes nothing.  Host form: waits for the device, writes w*h float.  Device form: one launch on `hip_stream`, enqueued
 * behind the pass it describes.
 */
int p3d_denoise_variance(p3d_adaptive* ad, float* var);
int p3d_denoise_variance_device(p3d_adaptive* ad, float* d_var, void* hip_stream);

/*
 * Temporal accumulation: the frames of a moving camera integrated over time - SVGF's history (Schied et al. 2017), the piece
 * that makes a 1-spp path-traced frame watchable while the view moves.  Every pixel takes the previous frames' integrated colour
 * wherever the same surface is still visible, and a luminance variance from temporal moments that goes into p3d_denoise's
 * luminance term: (out_rgb, out_var) are the (rgb, var) of p3d_denoise / p3d_denoise_device.  Detected by its symbols.
 *
 * Inputs per frame: rgb (w*h*3 float, linear colour, from any render call or pass), normal_depth and albedo_cov as
 * p3d_render_features writes them for that frame and camera, and `camera` - the camera the frame was rendered with
 * (p3d_scene_camera).  The object keeps the previous frame's camera.  Per pixel p = (x, y) (y = 0 the bottom row):
 *   point     d = the direction of primary_ray(camera, x + 0.5, y + 0.5) (float32, the render kernels' pixel-centre ray);
 *             cov_p > 0: X = eye + t_p d;  cov_p == 0 (a miss): the point at infinity in direction d
 *   project   into the previous camera (eye', u', v', n', w', h', plane_dist'): e = X - eye' (a miss: e = d);
 *             a = e.u', b = e.v', c = e.n'; c >= 0: behind the previous camera, no history; otherwise
 *             px' = (a (-plane_dist' / c) / w' + 0.5) res_x - 0.5,  py' = (b (-plane_dist' / c) / h' + 0.5) res_y - 0.5;
 *             a previous camera identical to `camera` (every field, bit for bit) maps every pixel onto itself: px' = x, py' = y
 *   taps      the four pixels q around (px', py') with bilinear weights; q is valid when it lies in the image, cov_p > 0 and
 *             cov'_q > 0 or both are 0, and for hits |t'_q - |X - eye'|| <= depth_tolerance |X - eye'| and
 *             n_p.n'_q >= normal_tolerance |n_p| |n'_q| (the features' normals, not renormalised)
 *   history   W = the sum of the valid taps' weights.  W < 1e-3 (or the first frame since create / reset): n = 1, the colour
 *             is c_p and the moments (Y, Y^2).  Otherwise c_hist, (m1, m2)_hist and n_prev are the weight-normalised sums over
 *             the valid taps, n = min(n_prev + 1, max_history), a = max(alpha, 1/n), am = max(alpha_moments, 1/n):
 *             c = (1 - a) c_hist + a c_p,  m1 = (1 - am) m1_hist + am Y,  m2 = (1 - am) m2_hist + am Y^2,
 *             Y = 0.2126 R + 0.7152 G + 0.0722 B of c_p (the denoiser's luminance)
 *   variance  n >= variance_min_history: var = max(0, m2 - m1^2).  Otherwise the same expression over moments averaged across
 *             the 7x7 neighbourhood in the current frame (taps in the image) with the weights w_g of p3d_denoise at step 1
 *             (sigma_normal, sigma_depth; the albedo term off) and 1 for the centre
 * The state between frames - c, n, m1, m2, the coverage and normal_depth - is kept in float32; the projection and the blend
 * are evaluated in float64 from those values and rounded once, the spatial weights in float32 (expf / powf), no contraction.
 * n is rounded to float32 before it is used.  tests/temporal_reference.py is the float64 statement the kernels are checked
 * against.  Outputs: out_rgb w*h*3 float, required; out_var w*h float and out_history w*h float (n), either may be NULL.
 * The outputs must not overlap the inputs.
 *
 * Refused: P3D_ERR_UNSUPPORTED for a camera with aperture != 0 (the pinhole reprojection is not exact for a lens);
 * P3D_ERR_INVALID for a camera whose resolution is not w x h or with a non-finite field or w, h, plane_dist <= 0, for alpha or
 * alpha_moments outside [0, 1], max_history < 1, depth_tolerance <= 0, normal_tolerance outside [-1, 1], a negative or NaN
 * sigma, non-zero reserved fields and null inputs.  A refused call changes nothing.
 *
 * An object is made for one image size (whole images only) on one device, like p3d_denoiser: p3d_temporal_create allocates
 * two sets of three float4 images (96 bytes per pixel) that the frames ping-pong between, so p3d_temporal_accumulate_device
 * neither allocates nor waits: it enqueues one launch (two with out_var) on `hip_stream`, behind a pass or inside a captured
 * graph.  Enqueue the calls of one object on one stream.  p3d_temporal_accumulate is the host-buffer form (synchronous).
 * p3d_temporal_reset forgets the history: the next frame is a first frame.  p3d_temporal_frames counts the frames since
 * create / reset.  p3d_temporal_params_default fills the defaults DESIGN.md chose (alpha 0.2, alpha_moments 0.2,
 * max_history 32, depth_tolerance 0.1, normal_tolerance 0.9, variance_min_history 4, sigma_normal 128, sigma_depth 1).
 */
typedef struct p3d_temporal_params {
  float alpha;             /* floor of the new frame's colour weight (SVGF: 0.2); 0 = a plain running mean */
  float alpha_moments;     /* the same for the luminance moments (SVGF: 0.2) */
  float max_history;       /* cap on the history length n (>= 1) */
  float depth_tolerance;   /* relative depth test of a reprojected tap (> 0) */
  float normal_tolerance;  /* minimum cosine between the two normals (-1 .. 1) */
  uint32_t variance_min_history; /* below this n the variance comes from a 7x7 spatial estimate (SVGF: 4) */
  float sigma_normal, sigma_depth; /* weights of that spatial estimate, as p3d_denoise_params */
  uint32_t reserved[2];    /* must be 0 */
} p3d_temporal_params;
typedef struct p3d_temporal p3d_temporal;
void p3d_temporal_params_default(p3d_temporal_params* params);
int p3d_temporal_create(int device, int32_t w, int32_t h, p3d_temporal** out);
void p3d_temporal_destroy(p3d_temporal* tp);
int p3d_temporal_reset(p3d_temporal* tp);
uint32_t p3d_temporal_frames(const p3d_temporal* tp);
int p3d_temporal_accumulate(p3d_temporal* tp, const p3d_temporal_params* params, const p3d_camera* camera, const float* rgb,
                            const float* normal_depth, const float* albedo_cov, float* out_rgb, float* out_var, float* out_history);
int p3d_temporal_accumulate_device(p3d_temporal* tp, const p3d_temporal_params* params, const p3d_camera* camera,
                                   const float* d_rgb, const float* d_normal_depth, const float* d_albedo_cov, float* d_out_rgb,
                                   float* d_out_var, float* d_out_history, void* hip_stream);

/*
 * Errors a kernel detects while it runs (a hit_stack leftover that outgrew its record, a work list of the hit_stack
 * hand-off that overflowed or did not run empty within its round bound, a row of a stripe or sub-rectangle whose
 * incoming hit_stack could not be established, a sample hand-out loop that reached its trip bound and would write pixels
 * with samples missing) raise a flag on the device.  The host-buffer
 * call and every call with `stats` turn it into P3D_ERR_CAPACITY themselves; after device-buffer calls without
 * `stats` ask here: waits for the scene's device, returns P3D_OK or P3D_ERR_CAPACITY and clears the flag.  Once
 * p3d_scene_refit_device or p3d_scene_pose_device has been used on the scene, the objects their kernels skipped show here
 * too, as P3D_ERR_INVALID (see there).
 */
int p3d_scene_status(p3d_scene* scene);
/*
 * Batched traversal queries — device counterparts of BVH::intersect_bvh
 * (bvh.cpp:198), Grid::Traverse (grid.cpp:71) and the brute-force loop
 * (main.cpp:116-124) for closest hit, and of BVH::bool_intersect_bvh
 * (bvh.cpp:278), Grid::Traverse(ray) (grid.cpp:154) and main.cpp:208-216 for any
 * hit.  Every ray starts with an empty traversal stack.  Host buffers:
 *   origin, direction : n*3 float (direction used as given, not normalised)
 *   hit_id : n int32 (-1 = miss) ; t : n float, the traversal's tmin / min_t (bvh.cpp:246, grid.cpp:100,
 *   main.cpp:120), FLT_MAX on a miss (may be NULL) ; hit_point : n*3 float (may be NULL)
 *   occluded : n uint8
 */
int p3d_trace_closest(p3d_scene* scene, uint32_t accel, uint32_t n, const float* origin,
                      const float* direction, int32_t* hit_id, float* t, float* hit_point);
int p3d_trace_any(p3d_scene* scene, uint32_t accel, uint32_t n, const float* origin,
                  const float* direction, uint8_t* occluded);
/*
 * The same queries over DEVICE buffers on the caller's stream, and an any-hit with a distance limit.  Detected by the symbols
 * (P3D_ABI_VERSION is unchanged).  For programs that keep their rays where they keep the positions they hand to
 * p3d_scene_update_geometry_device: no copy, and no wait.
 *
 * Buffers.  Every pointer is an address on the scene's device; the float and int32 buffers must be 4-byte aligned.
 *   d_origin, d_direction : n*3 float32 (direction used as given, not normalised, as in the host forms)
 *   d_t_max               : n float32, or NULL = no limit
 *   d_hit_id : n int32, required ; d_t : n float32 ; d_hit_point, d_normal : n*3 float32 - these three may be NULL
 *   d_occluded : n uint8, required
 * t and t_max are DISTANCES only for unit directions: a sphere test measures t along the normalised direction, the other kinds
 * in units of the direction as given (Q8), and the limit is compared with whatever the test reports.
 *
 * Stream.  The kernel is enqueued on `hip_stream` (a hipStream_t, NULL = the default stream) under the scene's stream rules
 * (p3d_render_tile_device: the launches on one scene share its stack spill area).  The call does not wait, neither before nor
 * after the launch: what the stream had enqueued to produce the rays runs first, and the outputs are complete when the
 * stream has passed the call.  Over a tree deeper than the 16-entry LDS window the call may have to grow the scene's spill
 * area; freeing the old one waits for the device, as it does in a render call; a second call of the same n allocates nothing.
 * With a tail stream set (p3d_scene_set_tail_stream) the launch first joins the previous frame's tail, as the next render
 * call on the scene does.
 *
 * p3d_trace_closest_device is the traversal of p3d_trace_closest.  With d_t_max = NULL every output equals the host form's, bit
 * for bit: d_t is FLT_MAX and d_hit_point zero on a miss.  With d_t_max a hit is kept only if t < t_max[i] (strict; a NaN limit
 * keeps nothing); otherwise the ray reports a miss.  The limit filters the traversal's nearest hit, it does not shorten the
 * traversal.  d_normal is Object::getNormal of the hit object at d_hit_point - what p3d_object_normal(hit_id, hit_point)
 * returns, bit for bit; it is NOT turned against the ray, and zero on a miss.
 *
 * p3d_trace_any_device with d_t_max = NULL is p3d_trace_any, bit for bit, for every accel: the reference's shadow feeler, which
 * has no distance limit (main.cpp:192-217) - an object BEHIND the point the feeler was sent to shadows it.
 * With d_t_max it is the SEGMENT query, which no traversal of the reference answers ("can A see B"):
 *   occluded[i] = 1 iff some object j has Object::intercepts(object j, a fresh copy of ray i, t) true and t < t_max[i].
 * Every primitive is tested on a copy of the caller's ray, so a sphere test's normalisation cannot change what a later test
 * sees, and the answer does not depend on the order of the visits.  A NaN t_max, and t_max <= 0, leave every ray free.
 *   P3D_ACCEL_NONE : a loop over all objects.
 *   P3D_ACCEL_BVH  : a stack traversal that skips a child whose box the ray misses or enters behind t_max, takes the nearer
 *                    child first and, at a dead end, pops the next entry - not the feeler's restart from the bottom of the stack
 *                    (bvh.cpp:329-338), which can miss an occluder.  Boxes are culled with the ray as given, as the closest-hit
 *                    traversal prunes; for unit directions it answers as P3D_ACCEL_NONE does wherever the decision is not a
 *                    matter of the last bits.  Planes are lost by the BVH as everywhere (Q12).
 *   P3D_ACCEL_GRID : P3D_ERR_UNSUPPORTED.  The reference's grid feeler runs the brute-force loop as well (Q6), so
 *                    P3D_ACCEL_NONE gives the answer a grid segment query would.
 *
 * Refused with P3D_ERR_INVALID, nothing enqueued: a null scene; an unknown accel, or one the scene was created without (and
 * P3D_ERR_UNSUPPORTED for a grid over an empty scene, as in the host forms); with n > 0, a null d_origin, d_direction,
 * d_hit_id or d_occluded; a misaligned pointer; a pointer that the HIP runtime identifies as host memory (registered or not)
 * or as memory of another device, or whose buffer ends behind the allocation the runtime reports for it (a pointer the
 * runtime cannot answer for is let through).  n = 0 returns P3D_OK.  P3D_ERR_CAPACITY: n x the tree's depth does not fit the
 * 32-bit offsets of the spill area (split the batch), as in the host forms.
 */
int p3d_trace_closest_device(p3d_scene* scene, uint32_t accel, uint32_t n,
                             const float* d_origin, const float* d_direction, const float* d_t_max /* may be NULL */,
                             int32_t* d_hit_id, float* d_t, float* d_hit_point, float* d_normal, void* hip_stream);
int p3d_trace_any_device(p3d_scene* scene, uint32_t accel, uint32_t n,
                         const float* d_origin, const float* d_direction, const float* d_t_max /* may be NULL */,
                         uint8_t* d_occluded, void* hip_stream);
/*
 * The HITS IN ORDER along a ray, and the count of all of them: what lies behind the first surface - entry and exit, thickness,
 * picking through a surface, and the sign of a point against a closed triangle mesh (the parity of the crossings).  The
 * ray-side twin of p3d_nearest_k_device.  Detected by the symbol (P3D_ABI_VERSION is unchanged).
 *
 * For ray i let limit = +inf where d_t_max is NULL, else t_max[i]; a NaN limit, and a limit <= 0, keep nothing.
 *   H(i) = the objects j for which Object::intercepts(object j, a fresh copy of ray i, t) is true and t < limit
 * - the per-object predicate of the segment query of p3d_trace_any_device, exactly.  A NaN t is never in.  Every test runs on a
 * copy of the caller's ray, so a sphere's normalisation reaches no other test; t is in the units the test reports (Q8), as in
 * p3d_trace_closest_device.  H(i) is ordered by (t, object index): the smaller t first, equal t to the smaller index - a total
 * order, so the answer is a function of the set and not of the order of the visits.
 *   count[i] = min(|H(i)|, k)
 *   row i*k + j, j < count[i] : the j-th element of H(i) - object: its index ; t: the t its test reported ; hit_point: o + d*t on
 *       the copy of the ray its test ran on (a sphere has normalised d), spelt as the closest-hit query spells it: a lone
 *       object reports the bits p3d_trace_closest_device reports for it ; normal: Object::getNormal at that point, NOT turned
 *       against the ray - the bits of p3d_object_normal(object, hit_point)
 *   row i*k + j, j >= count[i] : -1, FLT_MAX, zeros, zeros
 *   total[i] = |H(i)|, the number of objects hit in front of the limit, whatever k is (only where d_total is not NULL)
 * total counts OBJECTS, not crossings of a surface.  A sphere or a box reports ONE t, whether the ray starts inside or outside
 * it: a ray through a sphere adds 1, not 2.  A closed triangle mesh is one object per triangle: there total is the number of
 * crossings, and total & 1 says "the origin is inside" for a ray that grazes no edge or vertex (such a ray may count a
 * crossing twice or not at all: send another direction).
 * A smaller k gives a prefix of a larger one; count == k with d_total == NULL says that there may be more.
 *
 * k = 1 with d_t_max = NULL over P3D_ACCEL_NONE gives the minimum of the per-object tests under (t, index).  That is NOT in
 * general p3d_trace_closest_device's answer: its traversals hand ONE ray from test to test, so that a sphere's normalisation
 * reaches the tests after it (Q8), and break ties by the order of the visits.  Where no sphere re-normalises the ray (unit
 * directions, or no spheres) and no two objects tie, the two agree.
 *
 * Buffers (addresses on the scene's device, 4-byte aligned; sizes are taken in 64 bits):
 *   d_origin, d_direction : n*3 float32 (direction used as given) ; d_t_max : n float32, or NULL = no limit
 *   d_count : n int32 ; d_total : n int32, or NULL ; d_object : n*k int32 ; d_t : n*k float32 ; d_hit_point, d_normal : n*k*3 float32
 * 0 <= k <= P3D_TRACE_HITS_K_MAX.  k == 0 is the pure count: d_total is required, and d_count, d_object, d_t, d_hit_point and
 * d_normal are ignored (they may be NULL) - no list is kept.  With k >= 1 d_count and d_object are required and d_t,
 * d_hit_point and d_normal may be NULL.
 *
 *   P3D_ACCEL_NONE : a loop over all objects.
 *   P3D_ACCEL_BVH  : the segment query's traversal, which does not stop at a hit.  While fewer than k hits are listed, and
 *                    always when d_total is given, a child is skipped only if the ray misses its box or enters it behind the
 *                    limit; with d_total == NULL and a full list, behind the k-th listed t.  So asking for total costs the
 *                    whole segment, and a small k without it ends early.  Boxes are culled with the ray as given; for unit
 *                    directions it answers as P3D_ACCEL_NONE does wherever no decision is a matter of the last bits.  Planes
 *                    are lost by the BVH as everywhere (Q12), and not refused.
 *   P3D_ACCEL_GRID : P3D_ERR_UNSUPPORTED.
 *
 * Stream, buffers, tail join and spill area as p3d_trace_closest_device: one kernel on `hip_stream`, no wait, no allocation
 * once the spill area is large enough; behind p3d_scene_refit_device or p3d_scene_pose_device on the same stream it sees the
 * moved geometry.  Refused as p3d_nearest_k_device, nothing enqueued and nothing written: P3D_ERR_INVALID for a null scene, an
 * unknown accel or P3D_ACCEL_BVH on a scene without one, k > P3D_TRACE_HITS_K_MAX, with n > 0 a missing required pointer, a
 * misaligned pointer, host memory, memory of another device or a buffer too short; P3D_ERR_CAPACITY where n x the tree's depth
 * does not fit the spill area's 32-bit offsets.  n = 0 returns P3D_OK.
 */
#define P3D_TRACE_HITS_K_MAX 16u
int p3d_trace_hits_device(p3d_scene* scene, uint32_t accel, uint32_t n, uint32_t k,
                          const float* d_origin, const float* d_direction, const float* d_t_max /* may be NULL */,
                          int32_t* d_count /* n */, int32_t* d_total /* n, may be NULL */,
                          int32_t* d_object /* n*k */, float* d_t /* n*k */,
                          float* d_hit_point /* n*k*3 */, float* d_normal /* n*k*3 */, void* hip_stream);
/*
 * WHAT A RAY SEES - the Whitted radiance along rays held in device memory, p3d_trace_radiance_device, and the primary rays of
 * a camera, p3d_camera_rays_device - is declared in p3d_radiance.h, which this header includes: the entry points added after
 * the list of this file was closed.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#include "p3d_radiance.h"
/*
 * HOW OPEN A SURFACE POINT IS - the free share of the hemisphere above points held in device memory, p3d_occlusion_device, and
 * its rays written out, p3d_occlusion_rays_device and p3d_occlusion_rays - is declared in p3d_occlusion.h, which this header
 * includes likewise.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#include "p3d_occlusion.h"
/*
 * WHAT A SCENE IS LIT BY AND MADE OF - the lights and materials of a live scene, set from host memory
 * (p3d_scene_set_materials, p3d_scene_set_lights), read back (p3d_scene_materials, p3d_scene_lights) or set from device memory
 * on the caller's stream (p3d_scene_set_shading_device), and the same on a host scene - is declared in p3d_shading.h, which
 * this header includes likewise.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#include "p3d_shading.h"
/*
 * NEAREST-SURFACE queries: which object's surface is nearest to a point, how far away it is, and where on it - the contact
 * and proximity query of a particle or cloth step, and a distance field around a deforming mesh.  Detected by the symbols
 * (P3D_ABI_VERSION is unchanged).
 *
 * The per-object rule (host/nearest_rule.hpp, float32, one spelling for the host and the device): the closest point q on the
 * object's SURFACE and d2 = |p - q|^2 taken from q as stored.
 *   triangle : the closest point of the closed triangle - the face, an edge or a vertex
 *   sphere   : q = c + (p - c) * (r / |p - c|), inside and outside alike (the surface, not the solid); p == c: q = c + (r, 0, 0)
 *   box      : outside, the clamp of p to the box; inside or on it, p moved onto the nearest face (ties: the lowest axis, then
 *              the min face)
 *   plane    : q = p - ((p - A).N) N
 * The answer is the object with the smallest d2, equal d2 going to the smallest object index.  With a limit an object counts
 * only if max_dist > 0 and d2 < max_dist * max_dist (the float32 product): a zero, negative or NaN limit finds nothing.
 *   object : n int32, -1 = nothing ; dist : n float32, sqrtf(d2), FLT_MAX for nothing ; closest : n*3 float32, q, zero for nothing
 * p3d_host_scene_nearest (host side, below) is the statement of these semantics, on the CPU.
 *
 * p3d_nearest_device answers the question for n points in DEVICE memory with one kernel on the caller's stream, under
 * the buffer and stream rules of p3d_trace_closest_device: no copy, no wait, no allocation once the spill area is large
 * enough, and with a tail stream set the launch first joins the previous frame's tail.  Behind p3d_scene_refit_device or
 * p3d_scene_pose_device on the same stream it sees the moved geometry.
 *   d_point    : n*3 float32 ; d_max_dist : n float32, or NULL = no limit
 *   d_object   : n int32, required ; d_dist : n float32 ; d_closest, d_normal : n*3 float32 - these three may be NULL
 * d_object, d_dist and d_closest equal p3d_host_scene_nearest's for the same geometry, bit for bit, for both accels.
 * d_normal is Object::getNormal of the found object at d_closest - what p3d_object_normal(object, closest) returns, bit for
 * bit; it is not turned towards the point, and zero where nothing was found.
 *   P3D_ACCEL_NONE : a loop over all objects, planes included.
 *   P3D_ACCEL_BVH  : a stack traversal, uploaded and device-built trees alike, that visits the child whose box is nearer
 *                    first and drops a node only if its box lies farther than the shrinking search radius, with a slack of
 *                    2^-10 on the squared distance (the box distance and an object's d2 are rounded along different paths).
 *                    A scene that holds a plane is refused with P3D_ERR_UNSUPPORTED: a plane's box is the [-1,1]^3 default
 *                    (Q12), so the tree cannot find it.
 *   P3D_ACCEL_GRID : P3D_ERR_UNSUPPORTED.
 * Refused with P3D_ERR_INVALID, nothing enqueued, as p3d_trace_closest_device refuses: a null scene; an unknown accel, or
 * P3D_ACCEL_BVH on a scene created without one; with n > 0, a null d_point or d_object; a misaligned pointer; host memory,
 * memory of another device, or a buffer that ends behind its allocation.  n = 0 returns P3D_OK; an empty scene answers -1
 * everywhere.  P3D_ERR_CAPACITY: n x the tree's depth does not fit the 32-bit offsets of the spill area (split the batch).
 */
int p3d_nearest_device(p3d_scene* scene, uint32_t accel, uint32_t n, const float* d_point, const float* d_max_dist /* may be NULL */,
                       int32_t* d_object /* int32, required */, float* d_dist, float* d_closest, float* d_normal /* optional */,
                       void* hip_stream);
/*
 * THE K NEAREST SURFACES within a radius: for every point the (at most) k objects nearest to it, in order, each with its
 * distance, closest point and normal - what a contact solver needs where a point touches several surfaces at once (a cloth
 * vertex in a corner, a particle in a crease).  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 *
 * The per-object rule and the limit are those of p3d_nearest_device.  Let radius2 be +inf without a limit and the float32
 * product max_dist * max_dist with one (a zero, negative or NaN limit finds nothing), and S(i) the objects with d2 < radius2
 * for point i, ordered by (d2, object index): the smaller d2 first, equal d2 to the smaller index.  Then
 *   count[i] = min(|S(i)|, k), and row i*k + j holds for j < count[i] the j-th object of S(i):
 *     object : its index ; dist : sqrtf(d2) ; closest : the rule's q ; normal (device form) : Object::getNormal of that object
 *     at q - the bits of p3d_object_normal(object, closest), not turned towards the point
 *   and for j >= count[i]: -1, FLT_MAX, zeros and zeros.
 * count[i] == k means "there may be more": ask with a larger k or a smaller radius.  The size of S(i) is deliberately not
 * reported: counting it would forbid the search to cull against its k-th entry.  With k = 1 object, dist, closest and normal
 * equal p3d_nearest_device's / p3d_host_scene_nearest's bit for bit, and count is object >= 0.  The first k' rows of a point's
 * answer are its answer for k' < k.
 * p3d_host_scene_nearest_k (host side, below) is the statement of these semantics, on the CPU.
 *
 * p3d_nearest_k_device answers for n points in DEVICE memory with one kernel on the caller's stream, under the buffer, stream,
 * tail-join and spill-area rules of p3d_nearest_device: no copy, no wait, no allocation once the spill area is large enough.
 * Behind p3d_scene_refit_device or p3d_scene_pose_device on the same stream it sees the moved geometry.
 *   d_point  : n*3 float32 ; d_max_dist : n float32, or NULL = no limit
 *   d_count  : n int32, required ; d_object : n*k int32, required
 *   d_dist   : n*k float32 ; d_closest, d_normal : n*k*3 float32 - these three may be NULL
 * d_count, d_object, d_dist and d_closest equal p3d_host_scene_nearest_k's for the same geometry, bit for bit, for both accels.
 *   P3D_ACCEL_NONE : a loop over all objects, planes included.
 *   P3D_ACCEL_BVH  : the traversal of p3d_nearest_device, uploaded and device-built trees alike, with a sorted candidate list
 *                    per point (in LDS, sized for the k of the call).  A node is dropped only if its box lies farther than the
 *                    search bound - radius2 while fewer than k candidates are listed, the k-th candidate's d2 afterwards -
 *                    with the same slack of 2^-10.  A scene that holds a plane is refused with P3D_ERR_UNSUPPORTED.
 *   P3D_ACCEL_GRID : P3D_ERR_UNSUPPORTED.
 * Refused with P3D_ERR_INVALID, nothing enqueued and nothing written, as p3d_nearest_device refuses: a null scene; an unknown
 * accel, or P3D_ACCEL_BVH on a scene created without one; k == 0 or k > P3D_NEAREST_K_MAX; with n > 0, a null d_point, d_count
 * or d_object; a misaligned pointer; host memory, memory of another device, or a buffer that ends behind its allocation (n, n*k
 * and n*k*3 elements, computed in 64 bits).  n = 0 returns P3D_OK, whatever the pointers, once k is valid; an empty scene
 * answers count 0 everywhere.  P3D_ERR_CAPACITY: n x the tree's depth does not fit the 32-bit offsets of the spill area (split
 * the batch).
 */
#define P3D_NEAREST_K_MAX 16u
int p3d_nearest_k_device(p3d_scene* scene, uint32_t accel, uint32_t n, uint32_t k,
                         const float* d_point, const float* d_max_dist /* may be NULL */,
                         int32_t* d_count /* n, required */, int32_t* d_object /* n*k, required */,
                         float* d_dist /* n*k */, float* d_closest /* n*k*3 */, float* d_normal /* n*k*3 */, /* may be NULL */
                         void* hip_stream);
/*
 * Per-object queries — device counterparts of the virtual Object::intercepts(Ray&, float&)
 * (scene.cpp:47-94,116-137,149-186,215-227) and Object::getNormal(Vector) (scene.cpp:41-44,
 * 139-142,188-192,229-267) for object `object` (index in Scene::objects) and n rays / points.
 *   direction : n*3 float, IN and OUT — Sphere::intercepts normalises the ray in place
 *               (scene.cpp:156, ray.h:16-18); the other kinds leave it as it was
 *   hit : n uint8 ; t : n float (written where hit, as the reference writes its out-parameter)
 */
int p3d_object_intercepts(p3d_scene* scene, uint32_t object, uint32_t n, const float* origin,
                          float* direction, uint8_t* hit, float* t);
int p3d_object_normal(p3d_scene* scene, uint32_t object, uint32_t n, const float* point, float* normal);
/* Scene::GetSkyboxColor (scene.cpp:379-457) for n ray directions: rgb n*3 float.  Needs p3d_scene_set_skybox. */
int p3d_skybox_color(p3d_scene* scene, uint32_t n, const float* direction, float* rgb);

/* ---- host side: .p3f loader and acceleration-structure builders ---- */
/*
 * Host scene = Scene::load_p3f (scene.cpp:472-628) + the accel builds that
 * renderScene() does first (main.cpp:701-720): BVH::build (bvh.cpp:89-196) and
 * Grid::Build (grid.cpp:3-68).  These run on the host (as they do in the
 * reference) and produce the flat p3d_scene_desc that p3d_scene_create uploads.
 */
typedef struct p3d_host_scene p3d_host_scene;

#define P3D_LOAD_LEGACY_F11 1u /* accept the older 11-number `f` line (no emission);
                                  the shipped parser breaks on it */

int p3d_host_scene_load(const char* p3f_path, uint32_t flags, p3d_host_scene** out);
void p3d_host_scene_destroy(p3d_host_scene* hs);
/* Re-runs the Camera constructor (camera.h:34-63) with another resolution —
 * what editing the `resolution` line of the .p3f would do.  rx,ry <= 0 keeps. */
int p3d_host_scene_set_resolution(p3d_host_scene* hs, int32_t res_x, int32_t res_y);
/* Same for the `aperture` / `focal` entries of the `v` block. */
int p3d_host_scene_set_lens(p3d_host_scene* hs, float aperture_ratio, float focal_ratio);
/*
 * Replaces the nine geometry floats of the objects object[0..n): v + 9 i means what p3d_prim.v means for the object's kind
 * (sphere: centre and radius, triangle: three vertices, box: min and max).  The objects are constructed again by the
 * constructors the .p3f loader runs (the same code), so the triangle normal, Min / Max -/+ EPSILON and the sphere box come out
 * as a scene file with these numbers would give them; material and index stay.  Planes are refused (P3D_ERR_INVALID), as are
 * an index out of range and NULL arrays with n > 0; nothing is changed then.  Drops the host BVH and grid - the next
 * p3d_host_scene_desc builds them again - and invalidates the flattened arrays.  Host only, no device needed.
 */
int p3d_host_scene_set_geometry(p3d_host_scene* hs, uint32_t n, const uint32_t* object, const float* v /* n x 9 */);
/*
 * The nearest-surface query of p3d_nearest_device (see there for the rule, the tie and the limit), stated as a brute force
 * over the host scene's objects: the yardstick the device forms are held to bit for bit.  points : n*3 float32; max_dist :
 * n float32 or NULL; object : n int32, required; dist : n float32 and closest : n*3 float32 may be NULL.  Host only, no
 * device needed.
 */
int p3d_host_scene_nearest(p3d_host_scene* hs, uint32_t n, const float* points, const float* max_dist /* may be NULL */,
                           int32_t* object, float* dist, float* closest);
/*
 * The k-nearest query of p3d_nearest_k_device (see there for the order, the limit and the rows), stated as a brute force over
 * the host scene's objects with the candidate list of host/nearest_rule.hpp: the yardstick the device form is held to bit for
 * bit.  points : n*3 float32; max_dist : n float32 or NULL; count : n int32 and object : n*k int32, required; dist : n*k
 * float32 and closest : n*k*3 float32 may be NULL.  P3D_ERR_INVALID: a null scene, k == 0 or k > P3D_NEAREST_K_MAX, a null
 * required array with n > 0.  Host only, no device needed.
 */
int p3d_host_scene_nearest_k(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* points,
                             const float* max_dist /* may be NULL */,
                             int32_t* count /* n, required */, int32_t* object /* n*k, required */,
                             float* dist /* n*k */, float* closest /* n*k*3 */);   /* the last two may be NULL */
/* Replaces every light by SPP x SPP jittered copies (main.cpp:725-745); used for
 * SOFT_SHADOWS without ANTIALIASING. */
int p3d_host_scene_replicate_lights(p3d_host_scene* hs, uint32_t spp_sqrt, float light_side);
/* Builds (once) the requested structures and returns the descriptor; the
 * pointer stays valid until the host scene is destroyed or modified. */
int p3d_host_scene_desc(p3d_host_scene* hs, int build_bvh, int build_grid,
                        const p3d_scene_desc** out);
/* Points the query methods of the host classes (C++: Object::intercepts / getNormal, BVH::intersect_bvh /
 * bool_intersect_bvh, Grid::Traverse, Scene::GetSkyboxColor — p3d-raytracer_amd/host/scene_model.hpp) at the
 * device scene created from this host scene's descriptor, and uploads the cubemap the loader read for an `env`
 * line (p3d_host_scene_has_skybox) to it.  NULL unbinds.
 * The forwards exist so that code written against the reference's classes compiles and gives the reference's
 * answers; each call is a kernel launch for ONE ray (about 10 us).  Anything that asks more than a handful of
 * questions should ask them in one batch: p3d_trace_closest / p3d_trace_any / p3d_object_intercepts /
 * p3d_object_normal / p3d_skybox_color take n rays per call, and so do the array overloads of BVH::intersect_bvh /
 * BVH::bool_intersect_bvh on the host class (accel_build.hpp). */
int p3d_host_scene_bind_device(p3d_host_scene* hs, p3d_scene* scene);
/* 1 if a cubemap is loaded: the `.p3f` had an `env <dir>` line (scene.cpp:605-610) and the folder was found (relative to
 * the working directory, as in the reference, or next to the scene file), or p3d_host_scene_load_skybox was called. */
int p3d_host_scene_has_skybox(p3d_host_scene* hs);
/* The `v` block as loaded (from, at, up, angle; the aperture / focal ratios, as p3d_host_scene_set_lens left them): the
 * arguments of p3d_camera_look_at that rebuild the scene's camera.  P3D_ERR_INVALID without a `v` block. */
int p3d_host_scene_view(p3d_host_scene* hs, float from[3], float at[3], float up[3], float* angle, float* aperture_ratio,
                        float* focal_ratio);
/* Scene::LoadSkybox (scene.cpp:329-377): <sky_dir>/{right,left,top,bottom,front,back}.jpg, decoded by the library
 * (baseline JPEG - sequential DCT, Huffman, 8 bit, grey or YCbCr with 1x1 / 2x1 / 2x2 luma sampling - following the IJG
 * library's default path: the six shipped faces come out byte for byte as PIL's libjpeg-turbo decodes them; DevIL's own
 * version is unpinned in the reference).  A face that is not there as .jpg is read from a binary .ppm of that name.
 * P3D_ERR_IO names the face that could not be read (the reference exit(0)s, scene.cpp:354-357).  The faces go to the
 * device scene with p3d_host_scene_bind_device. */
int p3d_host_scene_load_skybox(p3d_host_scene* hs, const char* sky_dir);
/* Scene::skybox_img[face] (scene.h:218-223; RIGHT 0, LEFT 1, TOP 2, BOTTOM 3, FRONT 4, BACK 5): the decoded RGB bytes,
 * bottom row first (IL_ORIGIN_LOWER_LEFT, scene.cpp:344-345), owned by the host scene. */
int p3d_host_scene_skybox_face(p3d_host_scene* hs, int face, const uint8_t** img, uint32_t* res_x, uint32_t* res_y);

#ifdef __cplusplus
}
#endif
/*
 * WHEN A MOVING BALL FIRST TOUCHES THE SCENE - the sphere sweep of balls held in device memory, p3d_sweep_sphere_device, and its
 * statement on the CPU, p3d_host_scene_sweep_sphere - is declared in p3d_sweep.h, which this header includes here, behind the
 * host scene's type.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#include "p3d_sweep.h"
/*
 * QUERIES THAT LEAVE OBJECTS OUT, PER QUERY - p3d_nearest_k_filtered_device and p3d_sweep_sphere_filtered_device, for a cloth
 * vertex, a particle or a body that is itself part of the scene, and their statements on the CPU - are declared in p3d_filter.h,
 * which this header includes here.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#include "p3d_filter.h"
/*
 * NEAREST SURFACES TO A SEGMENT - capsule overlap and edge proximity: the k objects nearest to any point of each segment held in
 * device memory, p3d_nearest_segment_k_device, with the filters of p3d_filter.h, and its statement on the CPU - are declared in
 * p3d_segment.h, which this header includes here.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#include "p3d_segment.h"
/*
 * WHAT IS IN THIS REGION - overlap queries: the objects that touch each axis-aligned box held in device memory, their number
 * and the lowest k of them, p3d_overlap_box_device, with the filters of p3d_filter.h, and its statement on the CPU - are
 * declared in p3d_overlap.h, which this header includes here.  Detected by the symbols (P3D_ABI_VERSION is unchanged).
 */
#include "p3d_overlap.h"
#endif /* P3D_H */

// capi_scene_layout.hpp — the host-only half of scene creation, no call of the HIP runtime (float4 is only the storage type):
// descriptor validation, the BVH relabelling into child-pair slots, the assembly of the float4 blob
#pragma once
#include "capi_common.hpp"

namespace {

// Every index a kernel may follow is checked here, before any device call (DESIGN.md "Scene layout").
int validate_scene_desc(const p3d_scene_desc* d) {
  if (d->abi_version != P3D_ABI_VERSION) return fail(P3D_ERR_INVALID, "p3d_scene_create: ABI version mismatch");
  if ((d->n_prims && !d->prims) || (d->n_materials && !d->materials) || (d->n_lights && !d->lights))
    return fail(P3D_ERR_INVALID, "p3d_scene_create: null array with non-zero count");
  for (uint32_t i = 0; i < d->n_prims; ++i) {
    if (d->prims[i].material >= d->n_materials) return fail(P3D_ERR_INVALID, "p3d_scene_create: material index out of range");
    if (d->prims[i].type > P3D_PRIM_PLANE) return fail(P3D_ERR_INVALID, "p3d_scene_create: unknown primitive type");
  }
  if (d->n_bvh_nodes) {  // every index a lane may follow is checked here, not in the kernel
    if (!d->bvh_nodes || (d->n_bvh_prim_index && !d->bvh_prim_index) || d->n_bvh_prim_index != d->n_prims)
      return fail(P3D_ERR_INVALID, "p3d_scene_create: inconsistent BVH arrays");
    std::vector<uint8_t> has_parent(d->n_bvh_nodes, 0);  // a TREE: every record is the child of at most one inner node
    for (uint32_t i = 0; i < d->n_bvh_nodes; ++i) {
      const p3d_bvh_node& n = d->bvh_nodes[i];
      if (n.index > 0x0fffffffu) return fail(P3D_ERR_CAPACITY, "p3d_scene_create: BVH index exceeds 2^28");
      if (n.count_leaf & P3D_BVH_LEAF) {
        const uint64_t cnt = n.count_leaf & ~P3D_BVH_LEAF;
        if (cnt > 7) return fail(P3D_ERR_CAPACITY, "p3d_scene_create: BVH leaf with more than 7 objects (the reference's Threshold is 2)");
        if ((uint64_t)n.index + cnt > d->n_bvh_prim_index) return fail(P3D_ERR_INVALID, "p3d_scene_create: BVH leaf range out of bounds");
      } else if ((uint64_t)n.index + 1 >= d->n_bvh_nodes || n.index <= i) {
        return fail(P3D_ERR_INVALID, "p3d_scene_create: BVH child index out of bounds");
      } else {
        // (children lie behind their parent, so index 0 is nobody's child; a record with two parents - shared or
        // overlapping child pairs - would make the relabelling walk of layout_bvh, and every traversal, visit a DAG)
        if (has_parent[n.index] || has_parent[n.index + 1]) return fail(P3D_ERR_INVALID, "p3d_scene_create: BVH record with more than one parent (not a tree)");
        has_parent[n.index] = has_parent[n.index + 1] = 1;
      }
    }
    for (uint32_t i = 0; i < d->n_bvh_prim_index; ++i)
      if (d->bvh_prim_index[i] >= d->n_prims) return fail(P3D_ERR_INVALID, "p3d_scene_create: BVH object index out of bounds");
    if (d->bvh_max_depth == 0 || d->bvh_max_depth > 4096) return fail(P3D_ERR_INVALID, "p3d_scene_create: bad bvh_max_depth");
  }
  if (d->has_grid) {
    const p3d_grid_desc& g = d->grid;
    if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0 || (uint64_t)g.nx * g.ny * g.nz != g.n_cells || !g.cell_start ||
        (g.n_items && !g.cell_items) || g.cell_start[g.n_cells] != g.n_items)
      return fail(P3D_ERR_INVALID, "p3d_scene_create: inconsistent grid arrays");
    for (uint32_t c = 0; c < g.n_cells; ++c)
      if (g.cell_start[c] > g.cell_start[c + 1]) return fail(P3D_ERR_INVALID, "p3d_scene_create: grid cell_start not monotone");
    for (uint32_t i = 0; i < g.n_items; ++i)
      if (g.cell_items[i] >= d->n_prims) return fail(P3D_ERR_INVALID, "p3d_scene_create: grid object index out of bounds");
  }
  return P3D_OK;
}

// The float4 blob of a scene as it is uploaded: nodes | bgeom | normals | mats | lights | ogeom, offsets in float4s
struct SceneLayout {
  std::vector<float4> blob;
  uint32_t off_nodes = 0, off_bgeom = 0, off_ogeom = 0, off_normals = 0, off_mats = 0, off_lights = 0;
  uint32_t n_nodes = 0;     // node records uploaded (0 for a tree the device builds)
  uint32_t real_depth = 0;  // depth of the uploaded tree as its node array really is
  bool odd_boxes = false;   // some uploaded box is not finite with min <= max
  std::vector<uint32_t> emitters;  // emissive spheres in object order
};

// ---- node records: relabelled, never reordered as far as a ray can tell ----
// A traversal only ever follows descriptors, so where a record lies is free; what the reference's order fixes is
// which child is visited first, and that is untouched.  Layout: one 32-byte pad, the root, then the CHILD PAIRS (64 B,
// 64-byte aligned: one visit = one half line; in the reference's numbering a pair starts at an odd node index,
// i.e. it straddled two 64-byte sectors, every second one two 128-byte lines).  Pairs are laid out two to a 128-byte
// line as "dominoes": a pair and the child pair of its bigger (by box area: likelier) child share a line, so that
// about every second step down the tree stays in the line it is in; the root shares its line with its own child pair.
// Pairs without a child pair (both children leaves: half of all pairs) follow behind, two to a line.
// The descriptor must have passed validate_scene_desc (children lie behind their parent: the walks terminate).
int layout_bvh(const p3d_scene_desc* d, SceneLayout& L) {
  std::vector<float4>& blob = L.blob;
  blob.push_back(make_float4(0, 0, 0, 0));
  blob.push_back(make_float4(0, 0, 0, 0));
  L.off_nodes = (uint32_t)blob.size();
  if (!d->n_bvh_nodes) return P3D_OK;
  const p3d_bvh_node* N = d->bvh_nodes;
  auto inner = [&](uint32_t i) { return !(N[i].count_leaf & P3D_BVH_LEAF); };
  auto area = [&](uint32_t i) {
    const double x = (double)N[i].bmax[0] - N[i].bmin[0], y = (double)N[i].bmax[1] - N[i].bmin[1], z = (double)N[i].bmax[2] - N[i].bmin[2];
    const double a = x * y + y * z + z * x;
    return a == a ? a : 0.0;
  };
  std::vector<uint32_t> slot_of(d->n_bvh_nodes, 0xffffffffu);  // inner node -> slot of its child pair
  std::vector<uint32_t> singles, heads;
  uint32_t next_slot = 0;
  if (inner(0)) {
    slot_of[0] = next_slot++;
    for (int k = 1; k >= 0; --k) if (inner(N[0].index + k)) heads.push_back(N[0].index + k);  // left subtree first
  }
  while (!heads.empty()) {
    const uint32_t h = heads.back();
    heads.pop_back();
    const uint32_t l = N[h].index, r = l + 1;
    const bool li = inner(l), ri = inner(r);
    if (!li && !ri) { singles.push_back(h); continue; }
    const uint32_t second = (li && ri) ? (area(r) > area(l) ? r : l) : (li ? l : r);
    slot_of[h] = next_slot++;       // an odd slot: the first half of a line
    slot_of[second] = next_slot++;  // ... and the pair most rays take next in its second half
    for (int k = 1; k >= 0; --k) if (inner(N[second].index + k)) heads.push_back(N[second].index + k);
    const uint32_t other = second == l ? r : l;
    if (inner(other)) heads.push_back(other);
  }
  for (uint32_t h : singles) slot_of[h] = next_slot++;
  L.n_nodes = 1 + 2 * next_slot;
  if (L.n_nodes > 0x0fffffffu) return fail(P3D_ERR_CAPACITY, "p3d_scene_create: BVH index exceeds 2^28");
  blob.resize(blob.size() + (size_t)2 * L.n_nodes, make_float4(0, 0, 0, 0));
  auto put = [&](uint32_t at, uint32_t old) {
    const p3d_bvh_node& n = N[old];
    const uint32_t desc = inner(old) ? 1u + 2u * slot_of[old] : (kDescLeaf | ((n.count_leaf & 7u) << 28) | n.index);
    float descf;
    std::memcpy(&descf, &desc, 4);
    blob[L.off_nodes + 2 * (size_t)at] = make_float4(n.bmin[0], n.bmin[1], n.bmin[2], descf);
    blob[L.off_nodes + 2 * (size_t)at + 1] = make_float4(n.bmax[0], n.bmax[1], n.bmax[2], 0.f);
    for (int k = 0; k < 3; ++k)  // the slab fast paths assume finite boxes with min <= max (device_core.hpp); only uploaded records matter
      if (!(std::fabs(n.bmin[k]) < INFINITY) || !(std::fabs(n.bmax[k]) < INFINITY) || !(n.bmin[k] <= n.bmax[k])) L.odd_boxes = true;
  };
  put(0, 0);
  for (uint32_t i = 0; i < d->n_bvh_nodes; ++i)
    if (slot_of[i] != 0xffffffffu) {  // (records no descriptor leads to are not uploaded)
      put(1 + 2 * slot_of[i], N[i].index);
      put(2 + 2 * slot_of[i], N[i].index + 1);
    }
  // The node-stack capacity (LDS + spill) is derived from the tree depth: never trust the caller's
  // number below what the node array really contains.
  std::vector<uint32_t> level(d->n_bvh_nodes, 0);
  level[0] = L.real_depth = 1;
  for (uint32_t i = 0; i < d->n_bvh_nodes; ++i) {
    if (level[i] == 0) continue;  // unreachable record
    L.real_depth = std::max(L.real_depth, level[i]);
    if (inner(i)) level[N[i].index] = level[N[i].index + 1] = level[i] + 1;
  }
  return P3D_OK;
}

// Everything behind the uploaded node records.  lbvh_nodes / lbvh_slots: room for the tree and the BVH-ordered geometry
// that lbvh::build fills in on the device (0 for an uploaded tree).
void assemble_blob(const p3d_scene_desc* d, uint32_t lbvh_nodes, uint32_t lbvh_slots, SceneLayout& L) {
  std::vector<float4>& blob = L.blob;
  auto geom_of = [&](uint32_t obj, float4 dst[3]) {
    const p3d_prim& p = d->prims[obj];
    dst[0] = make_float4(p.v[0], p.v[1], p.v[2], p.v[3]);
    dst[1] = make_float4(p.v[4], p.v[5], p.v[6], p.v[7]);
    const uint32_t tm = p.type | (p.material << 8);
    float tmf, objf;
    std::memcpy(&tmf, &tm, 4);
    std::memcpy(&objf, &obj, 4);
    dst[2] = make_float4(p.v[8], tmf, objf, 0.f);
  };
  blob.resize(blob.size() + (size_t)2 * lbvh_nodes, make_float4(0, 0, 0, 0));  // filled in by lbvh::build
  L.off_bgeom = (uint32_t)blob.size();
  blob.resize(blob.size() + (size_t)3 * lbvh_slots, make_float4(0, 0, 0, 0));
  for (uint32_t i = 0; i < d->n_bvh_prim_index; ++i) {
    float4 g[3];
    geom_of(d->bvh_prim_index[i], g);
    blob.insert(blob.end(), g, g + 3);
  }
  L.off_normals = (uint32_t)blob.size();
  for (uint32_t i = 0; i < d->n_prims; ++i) blob.push_back(make_float4(d->prims[i].n[0], d->prims[i].n[1], d->prims[i].n[2], 0.f));
  L.off_mats = (uint32_t)blob.size();
  auto plain = [](float c) { return c >= 0.0f && c <= 1e15f; };
  bool lights_plain = true;
  for (uint32_t i = 0; i < d->n_lights; ++i)
    lights_plain = lights_plain && plain(d->lights[i].color[0]) && plain(d->lights[i].color[1]) && plain(d->lights[i].color[2]);
  for (uint32_t i = 0; i < d->n_materials; ++i) {
    const p3d_material& m = d->materials[i];
    blob.push_back(make_float4(m.diff_color[0], m.diff_color[1], m.diff_color[2], m.diffuse));
    blob.push_back(make_float4(m.spec_color[0], m.spec_color[1], m.spec_color[2], m.specular));
    blob.push_back(make_float4(m.shine, m.transmittance, m.refr_index, m.reflection));
    // .w: the material's specular term is provably multiplied by an exact zero - Ks == 0 - and provably finite and
    // non-negative whatever the geometry (0 <= shine < inf, specular colour and every light colour in [0, 1e15]): the kernels
    // then leave the pow(H.N, shine) of main.cpp:224 out for Blinn cosines <= 1 (whitted_level.inc), same bits
    blob.push_back(make_float4(m.emission[0], m.emission[1], m.emission[2], (lights_plain && m.specular == 0.0f && m.shine >= 0.0f && m.shine < INFINITY &&
                                                                              plain(m.spec_color[0]) && plain(m.spec_color[1]) && plain(m.spec_color[2])) ? 1.0f : 0.0f));
  }
  L.off_lights = (uint32_t)blob.size();
  for (uint32_t i = 0; i < d->n_lights; ++i) {
    const p3d_light& l = d->lights[i];
    blob.push_back(make_float4(l.position[0], l.position[1], l.position[2], 0.f));
    blob.push_back(make_float4(l.color[0], l.color[1], l.color[2], 0.f));
  }
  // object-order geometry last: the kernels that walk the BVH read the BVH-ordered copy only, and an LDS-staged launch of
  // theirs leaves this array out (stage range, plan_frame)
  L.off_ogeom = (uint32_t)blob.size();
  for (uint32_t i = 0; i < d->n_prims; ++i) {
    float4 g[3];
    geom_of(i, g);
    blob.insert(blob.end(), g, g + 3);
  }
  if (blob.empty()) blob.push_back(make_float4(0, 0, 0, 0));
  // emissive spheres in object order: the light loop of Radiance (main.cpp:407-415)
  for (uint32_t i = 0; i < d->n_prims; ++i) {
    const p3d_material& m = d->materials[d->prims[i].material];
    if (m.emission[0] + m.emission[1] + m.emission[2] > 0 && d->prims[i].type == P3D_PRIM_SPHERE) L.emitters.push_back(i);
  }
}

}  // namespace

// grid_build.hpp — the uniform grid built ON the device (p3d_scene_build_grid, and again by every p3d_scene_update_prims of
// a scene that has one), from the per-object boxes a live scene keeps there (lbvh::Workspace::boxes).
//
// The result is Grid::Build's (host/accel_build.cpp, grid.cpp:3-68) to the bit: same bounds, same cell counts, same CSR
// arrays with every cell's objects in ascending object index (the host's insertion order).  The frame arithmetic is the
// host's own (host/grid_rule.hpp).  Steps, all on the null stream:
//   1. box_bounds    min of bmin / max of bmax over all objects: wave shuffle, LDS, one set of integer atomics per block
//      (24-byte read-back: the host grows the bounds, derives nx, ny, nz and checks the limits)
//   2. object_spans  per object the box of cells it overlaps and its volume
//   3. exclusive sum of the volumes (hipCUB): first[j] = number of (object, cell) pairs in front of object j
//      (8-byte read-back: the pair total sizes the arrays)
//   4. emit_pairs    one lane per PAIR - not per object: two floor triangles of balls_low own half of its pairs each -,
//                    which finds its object by binary search in first[]; writes (cell, object), pairs in object order
//   5. stable radix sort of the pairs by cell, over the bits a cell index needs (hipCUB): a cell's objects stay in pair
//      order, which is object order, whatever order the waves ran in; the sorted objects ARE cell_items
//   6. run_ends      the last pair of every run of equal cells writes its end into cell_start[cell + 1] (no atomics)
//   7. inclusive max-scan of cell_start[1 ..] (hipCUB): an empty cell inherits the end of the last cell in front of it
// Nothing here depends on arrival order: integer min / max, integer sums, a stable sort, one writer per word.
#pragma once

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <cstring>

#include "../host/grid_rule.hpp"
#include "lbvh.hpp"

namespace p3d {
namespace grid_build {

constexpr int kThreads = lbvh::kThreads;
constexpr uint64_t kMaxCells = 1ull << 28;  // include/p3d.h: 1 GiB of cell_start

struct Dims {
  float p0[3], p1[3];
  int n[3];
};

// boxes: [2 * i] = {bmin, -}, [2 * i + 1] = {bmax, -}.  bounds[0..2] = min of bmin, [3..5] = max of bmax (ordered uints)
__global__ void __launch_bounds__(kThreads) box_bounds(const float4* boxes, uint32_t n, uint32_t* out) {
  __shared__ uint32_t part[kThreads / 64][6];
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  uint32_t v[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  if (i < n) {
    const float4 lo = boxes[2 * i], hi = boxes[2 * i + 1];
    v[0] = lbvh::f2o(lo.x); v[1] = lbvh::f2o(lo.y); v[2] = lbvh::f2o(lo.z);
    v[3] = lbvh::f2o(hi.x); v[4] = lbvh::f2o(hi.y); v[5] = lbvh::f2o(hi.z);
  }
  for (int off = 32; off >= 1; off >>= 1)
    for (int k = 0; k < 3; ++k) {
      v[k] = min(v[k], (uint32_t)__shfl_xor((int)v[k], off, 64));
      v[3 + k] = max(v[3 + k], (uint32_t)__shfl_xor((int)v[3 + k], off, 64));
    }
  const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  if (lane == 0)
    for (int k = 0; k < 6; ++k) part[wave][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 6) {
    const uint32_t k = threadIdx.x;
    uint32_t r = part[0][k];
    for (int w = 1; w < kThreads / 64; ++w) r = k < 3 ? min(r, part[w][k]) : max(r, part[w][k]);
    if (k < 3) atomicMin(&out[k], r);
    else atomicMax(&out[k], r);
  }
}

// spans: [2 * j] = first cell (x, y, z) of object j, [2 * j + 1] = cells per axis.  volume[j] = their product; volume[n] = 0
__global__ void object_spans(const float4* boxes, uint32_t n, Dims d, int4* spans, unsigned long long* volume) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j > n) return;
  if (j == n) { volume[n] = 0; return; }
  const float4 lo = boxes[2 * j], hi = boxes[2 * j + 1];
  const float bl[3] = {lo.x, lo.y, lo.z}, bh[3] = {hi.x, hi.y, hi.z};
  int c0[3], cn[3];
  for (int k = 0; k < 3; ++k) {
    // (the int clamp changes no value Grid::Build can index with: it keeps a NaN quotient, which the host cannot survive, inside the arrays)
    const int a = min(max(grid_axis_cell(bl[k], d.p0[k], d.p1[k], d.n[k]), 0), d.n[k] - 1);
    const int b = min(max(grid_axis_cell(bh[k], d.p0[k], d.p1[k], d.n[k]), 0), d.n[k] - 1);
    c0[k] = a;
    cn[k] = b >= a ? b - a + 1 : 0;  // (the host's loops run no trip then)
  }
  spans[2 * j] = make_int4(c0[0], c0[1], c0[2], 0);
  spans[2 * j + 1] = make_int4(cn[0], cn[1], cn[2], 0);
  volume[j] = (unsigned long long)cn[0] * (unsigned long long)cn[1] * (unsigned long long)cn[2];
}

// Pair p belongs to the object j with first[j] <= p < first[j + 1] (first[n] = total); its cell is the (p - first[j])-th of
// the object's span, x fastest.
__global__ void emit_pairs(const unsigned long long* first, const int4* spans, uint32_t n, uint32_t total, int nx, int ny,
                           uint32_t* cell, uint32_t* object) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= total) return;
  uint32_t lo = 0, hi = n;  // the first j in (lo, hi] with first[j] > p, minus one: objects without cells are skipped
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= p) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t j = lo - 1;  // first[0] = 0 <= p: lo >= 1
  const int4 c0 = spans[2 * j], cn = spans[2 * j + 1];
  const uint32_t l = (uint32_t)(p - first[j]);
  const uint32_t ix = (uint32_t)c0.x + l % (uint32_t)cn.x;
  const uint32_t iy = (uint32_t)c0.y + (l / (uint32_t)cn.x) % (uint32_t)cn.y;
  const uint32_t iz = (uint32_t)c0.z + l / ((uint32_t)cn.x * (uint32_t)cn.y);
  cell[p] = ix + (uint32_t)nx * iy + (uint32_t)nx * (uint32_t)ny * iz;
  object[p] = j;
}

// sorted: the pairs' cells in ascending order.  cell_start (n_cells + 1 words, zeroed): [c + 1] = end of cell c's run
__global__ void run_ends(const uint32_t* sorted, uint32_t total, uint32_t n_cells, uint32_t* cell_start) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const uint32_t c = sorted[i];
  if (c < n_cells && (i + 1 == total || sorted[i + 1] != c)) cell_start[c + 1] = (uint32_t)(i + 1);
}

// What a scene keeps between builds.  Everything but `temp` is sized by the object count (fixed for a scene) or by the pair
// capacity, which only grows.
struct Workspace {
  uint32_t n = 0;
  uint32_t* bounds = nullptr;          // 6
  int4* spans = nullptr;               // 2 n
  unsigned long long* first = nullptr; // n + 1: volumes, then their exclusive sum in place
  uint32_t *cell = nullptr, *sorted = nullptr, *object = nullptr;  // pair_cap each
  uint64_t pair_cap = 0;
  void* temp = nullptr;
  size_t temp_bytes = 0;

  hipError_t alloc(uint32_t n_objs) {
    n = n_objs;
    P3D_LBVH_HIP(hipMalloc((void**)&bounds, 6 * sizeof(uint32_t)));
    P3D_LBVH_HIP(hipMalloc((void**)&spans, (size_t)2 * n * sizeof(int4)));
    P3D_LBVH_HIP(hipMalloc((void**)&first, ((size_t)n + 1) * sizeof(unsigned long long)));
    return hipSuccess;
  }
  hipError_t ensure_pairs(uint64_t total) {
    if (total <= pair_cap) return hipSuccess;
    for (uint32_t** p : {&cell, &sorted, &object}) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
    pair_cap = 0;
    for (uint32_t** p : {&cell, &sorted, &object}) P3D_LBVH_HIP(hipMalloc((void**)p, (size_t)total * sizeof(uint32_t)));
    pair_cap = total;
    return hipSuccess;
  }
  hipError_t ensure_temp(size_t need) {
    if (need <= temp_bytes && temp) return hipSuccess;
    if (temp) (void)hipFree(temp);
    temp = nullptr;
    temp_bytes = 0;
    P3D_LBVH_HIP(hipMalloc(&temp, need ? need : 16));
    temp_bytes = need ? need : 16;
    return hipSuccess;
  }
  void release() {
    for (void* p : {(void*)bounds, (void*)spans, (void*)first, (void*)cell, (void*)sorted, (void*)object, temp})
      if (p) (void)hipFree(p);
    *this = Workspace{};
  }
};

// Step 1, and the read-back of its six words as floats: lo = min of bmin, hi = max of bmax
inline hipError_t box_union(Workspace& w, const float4* d_boxes, float lo[3], float hi[3]) {
  P3D_LBVH_HIP(hipMemsetAsync(w.bounds, 0xff, 3 * sizeof(uint32_t), 0));
  P3D_LBVH_HIP(hipMemsetAsync(w.bounds + 3, 0, 3 * sizeof(uint32_t), 0));
  hipLaunchKernelGGL(box_bounds, dim3((w.n + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, d_boxes, w.n, w.bounds);
  P3D_LBVH_HIP(hipGetLastError());
  uint32_t h[6];
  P3D_LBVH_HIP(hipMemcpy(h, w.bounds, sizeof(h), hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; ++k) {
    auto back = [](uint32_t o) {
      const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
      float f;
      std::memcpy(&f, &u, 4);
      return f;
    };
    lo[k] = back(h[k]);
    hi[k] = back(h[3 + k]);
  }
  return hipSuccess;
}

// Steps 2 and 3, and the read-back of the pair total
inline hipError_t count_pairs(Workspace& w, const float4* d_boxes, const Dims& d, uint64_t* total) {
  hipLaunchKernelGGL(object_spans, dim3((w.n + 1 + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, d_boxes, w.n, d, w.spans, w.first);
  P3D_LBVH_HIP(hipGetLastError());
  size_t need = 0;
  P3D_LBVH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, w.first, w.first, (int)(w.n + 1)));
  P3D_LBVH_HIP(w.ensure_temp(need));
  P3D_LBVH_HIP(hipcub::DeviceScan::ExclusiveSum(w.temp, need, w.first, w.first, (int)(w.n + 1)));
  unsigned long long t = 0;
  P3D_LBVH_HIP(hipMemcpy(&t, w.first + w.n, sizeof(t), hipMemcpyDeviceToHost));
  *total = t;
  return hipSuccess;
}

// Steps 4 to 7: d_cell_start has n_cells + 1 words, d_cell_items and the workspace's pair arrays `total` or more
inline hipError_t enqueue_cells(Workspace& w, const Dims& d, uint32_t n_cells, uint32_t total, uint32_t* d_cell_start, uint32_t* d_cell_items) {
  P3D_LBVH_HIP(hipMemsetAsync(d_cell_start, 0, ((size_t)n_cells + 1) * sizeof(uint32_t), 0));
  if (total) {
    int bits = 1;
    while (bits < 32 && (1ull << bits) < n_cells) ++bits;
    size_t need_sort = 0, need_scan = 0;
    P3D_LBVH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, w.cell, w.sorted, w.object, d_cell_items, total, 0, bits));
    P3D_LBVH_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, need_scan, d_cell_start + 1, d_cell_start + 1, hipcub::Max(), (int)n_cells));
    P3D_LBVH_HIP(w.ensure_temp(need_sort > need_scan ? need_sort : need_scan));
    const uint32_t blocks = (uint32_t)(((uint64_t)total + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(emit_pairs, dim3(blocks), dim3(kThreads), 0, 0, w.first, w.spans, w.n, total, d.n[0], d.n[1], w.cell, w.object);
    P3D_LBVH_HIP(hipGetLastError());
    P3D_LBVH_HIP(hipcub::DeviceRadixSort::SortPairs(w.temp, need_sort, w.cell, w.sorted, w.object, d_cell_items, total, 0, bits));
    hipLaunchKernelGGL(run_ends, dim3(blocks), dim3(kThreads), 0, 0, w.sorted, total, n_cells, d_cell_start);
    P3D_LBVH_HIP(hipGetLastError());
    P3D_LBVH_HIP(hipcub::DeviceScan::InclusiveScan(w.temp, need_scan, d_cell_start + 1, d_cell_start + 1, hipcub::Max(), (int)n_cells));
  }
  return hipGetLastError();
}

}  // namespace grid_build
}  // namespace p3d

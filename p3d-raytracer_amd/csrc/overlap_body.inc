// overlap_body.inc — the body of overlap_box_device_kernel, included into each of the kernels of that name (overlap_query.hpp):
// `P` is the kernel's OverlapParams, `filters` its source of filters (queries.hpp FilterParams or NoFilterSource).  Text and
// not a function, as nearest_k_body.inc: the unfiltered kernel holds no trace of a filter.
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  OverlapSearch s;
  s.list = query_list_base(smem, P.stack);
  s.count = 0; s.k = P.k; s.total = 0; s.flags = P.flags;
  s.gate = P.k ? INT32_MAX : -1;
  if (i >= P.n) return;
  const QueryBox box{{P.lo[3 * i], P.lo[3 * i + 1], P.lo[3 * i + 2]}, {P.hi[3 * i], P.hi[3 * i + 1], P.hi[3 * i + 2]}};
  const auto filter = filters.load(i, P.sc.n_objs);
  if (overlap_query_open(box.lo, box.hi) && P.sc.n_objs > 0) {
    if (ACCEL == P3D_ACCEL_BVH) bvh_overlap_box(P.sc, st, box, s, filter);
    else brute_overlap_box(P.sc, box, s, filter);
  }
  P.total[i] = (int32_t)s.total;
  for (uint32_t e = 0; e < P.k; ++e) P.object[(size_t)i * P.k + e] = e < s.count ? (int32_t)s.list[e * kBlock] : -1;

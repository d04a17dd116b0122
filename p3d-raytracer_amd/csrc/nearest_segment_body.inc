// nearest_segment_body.inc — the body of nearest_segment_k_device_kernel, included into each of the kernels of that name
// (nearest_segment_query.hpp): `P` is the kernel's NearestSegmentParams, `filters` its source of filters (queries.hpp FilterParams
// or NoFilterSource).  Text and not a function, as nearest_k_body.inc: the unfiltered kernel holds no trace of a filter.
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  NearestKSearch s;
  s.list.base = query_list_base(smem, P.stack);
  s.count = 0; s.k = P.k;
  if (i >= P.n) return;
  const QuerySegment seg{{P.a[3 * i], P.a[3 * i + 1], P.a[3 * i + 2]}, {P.b[3 * i], P.b[3 * i + 1], P.b[3 * i + 2]}};
  const bool open = nearest_k_open(P.max_dist != nullptr, P.max_dist ? P.max_dist[i] : 0.0f, s.gate);
  const auto filter = filters.load(i, P.sc.n_objs);
  if (open && P.sc.n_objs > 0) {
    if (ACCEL == P3D_ACCEL_BVH) bvh_nearest_segment_k(P.sc, st, seg, s, filter);
    else brute_nearest_segment_k(P.sc, seg, s, filter);
  }
  P.count[i] = (int32_t)s.count;
  const float4* geom = ACCEL == P3D_ACCEL_BVH ? P.sc.bgeom : P.sc.ogeom;
  for (uint32_t e = 0; e < P.k; ++e) {
    const size_t row = (size_t)i * P.k + e;
    const bool found = e < s.count;
    int32_t object = -1;
    float dist = FLT_MAX, param = FLT_MAX;
    F3 x = f3(0, 0, 0), q = f3(0, 0, 0), nrm = f3(0, 0, 0);
    if (found) {
      const Geom g = load_geom(geom, s.list.slot(e));
      const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
      float on[3], c[3];
      segment_nearest(geom_type(g), v, seg.a, seg.b, param, on, c);
      object = s.list.object(e);
      dist = sqrtf(s.list.d2(e));
      x = f3(on[0], on[1], on[2]);
      q = f3(c[0], c[1], c[2]);
      if (P.normal) nrm = get_normal(g, P.sc.normals, q);
    }
    P.object[row] = object;
    if (P.dist) P.dist[row] = dist;
    if (P.param) P.param[row] = param;
    if (P.on_segment) store_f3(P.on_segment, row, x);
    if (P.closest) store_f3(P.closest, row, q);
    if (P.normal) store_f3(P.normal, row, nrm);
  }

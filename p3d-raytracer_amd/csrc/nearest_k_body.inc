// nearest_k_body.inc — the body of nearest_k_device_kernel, included into each of the kernels of that name (nearest_query.hpp): `P` is the kernel's NearestKParams, `filters` its source
// of filters (queries.hpp FilterParams or NoFilterSource).  The lane's filter is loaded once, behind the bounds check and in front
// of the search.  Text and not a function: the unfiltered kernel then is, instruction for instruction, the kernel it was before
// there were filters - as an inlined function taking P by reference it was not (DESIGN.md "Filtered queries").
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  NearestKSearch s;
  s.list.base = query_list_base(smem, P.stack);
  s.count = 0; s.k = P.k;
  if (i >= P.n) return;
  const float p[3] = {P.point[3 * i], P.point[3 * i + 1], P.point[3 * i + 2]};
  const bool open = nearest_k_open(P.max_dist != nullptr, P.max_dist ? P.max_dist[i] : 0.0f, s.gate);
  const auto filter = filters.load(i, P.sc.n_objs);
  if (open && P.sc.n_objs > 0) {
    if (ACCEL == P3D_ACCEL_BVH) bvh_nearest_k(P.sc, st, p, s, filter);
    else brute_nearest_k(P.sc, p, s, filter);
  }
  if (P.count) P.count[i] = (int32_t)s.count;
  const float4* geom = ACCEL == P3D_ACCEL_BVH ? P.sc.bgeom : P.sc.ogeom;
  for (uint32_t e = 0; e < P.k; ++e) {
    const size_t row = (size_t)i * P.k + e;
    const bool found = e < s.count;
    int32_t object = -1;
    float dist = FLT_MAX;
    F3 q = f3(0, 0, 0), nrm = f3(0, 0, 0);
    if (found) {
      const Geom g = load_geom(geom, s.list.slot(e));
      const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
      float c[3];
      nearest_point(geom_type(g), v, p, c);
      object = s.list.object(e);
      dist = sqrtf(s.list.d2(e));
      q = f3(c[0], c[1], c[2]);
      if (P.normal) nrm = get_normal(g, P.sc.normals, q);
    }
    P.object[row] = object;
    if (P.dist) P.dist[row] = dist;
    if (P.closest) store_f3(P.closest, row, q);
    if (P.normal) store_f3(P.normal, row, nrm);
  }
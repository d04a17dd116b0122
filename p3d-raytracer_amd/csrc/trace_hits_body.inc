// trace_hits_body.inc — the body of trace_hits_kernel, included into each of the kernels of that name (hit_list_query.hpp): `P` is
// the kernel's TraceHitsParams, `filters` its source of filters (queries.hpp FilterParams or NoFilterSource).  Text and not a
// function, as nearest_k_body.inc: the unfiltered kernel holds no trace of a filter.
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  HitListSearch s;
  s.list.base = query_list_base(smem, P.stack);
  s.k = P.k; s.want_total = P.total != nullptr;
  if (i >= P.n) return;
  Counters<false> ct;
  RayS ray;
  ray_set(ray, f3(P.origin[3 * i], P.origin[3 * i + 1], P.origin[3 * i + 2]),
          f3(P.direction[3 * i], P.direction[3 * i + 1], P.direction[3 * i + 2]));
  const auto filter = filters.load(i, P.sc.n_objs);
  if (hit_list_open(P.t_max, i, s) && P.sc.n_objs > 0) {
    if (ACCEL == P3D_ACCEL_BVH) bvh_segment_hits(P.sc, st, ray, s, filter, ct);
    else brute_segment_hits(P.sc, ray, s, filter, ct);
  }
  if (P.total) P.total[i] = (int32_t)s.total;
  if (P.k == 0) return;
  P.count[i] = (int32_t)s.count;
  const float4* geom = ACCEL == P3D_ACCEL_BVH ? P.sc.bgeom : P.sc.ogeom;
  for (uint32_t e = 0; e < P.k; ++e) {
    const size_t row = (size_t)i * P.k + e;
    int32_t object = -1;
    float t = FLT_MAX;
    F3 hp = f3(0, 0, 0), nrm = f3(0, 0, 0);
    if (e < s.count) {
      object = s.list.object(e);
      t = s.list.d2(e);
      if (P.hit_point || P.normal) {
        const Geom g = load_geom(geom, s.list.slot(e));
        RayS r = ray;
        float again;
        intercepts(g, r, again, ct);  // (for the ray it leaves behind: a sphere has normalised it, Q8)
        hp = r.o + r.d * t;
        if (P.normal) nrm = get_normal(g, P.sc.normals, hp);
      }
    }
    P.object[row] = object;
    if (P.t) P.t[row] = t;
    if (P.hit_point) store_f3(P.hit_point, row, hp);
    if (P.normal) store_f3(P.normal, row, nrm);
  }

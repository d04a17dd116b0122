// ray_query_body.inc — the body of ray_query_kernel, included into each of the kernels of that name (ray_query.hpp): `P` is the
// kernel's RayQueryParams, `filters` its source of filters (queries.hpp FilterParams or NoFilterSource).  Text and not a
// function, as nearest_k_body.inc: the unfiltered kernel holds no trace of a filter.
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  if (i >= P.n) return;
  Counters<false> ct;
  RayS ray;
  ray_set(ray, f3(P.origin[3 * i], P.origin[3 * i + 1], P.origin[3 * i + 2]),
          f3(P.direction[3 * i], P.direction[3 * i + 1], P.direction[3 * i + 2]));
  const float* t_max = EXTRAS ? P.t_max : nullptr;
  if (ANY) {
    bool occluded;
    if (!t_max) occluded = any_hit<ACCEL, true, true>(P.sc, st, ray, ct);  // (the feeler knows no filter: the host refuses a filtered call without t_max)
    else {
      const auto filter = filters.load(i, P.sc.n_objs);
      if (ACCEL == P3D_ACCEL_BVH) occluded = bvh_segment_any(P.sc, st, ray, t_max[i], filter, ct);
      else occluded = brute_segment_any(P.sc, ray, t_max[i], filter, ct);
    }
    P.occluded[i] = occluded ? 1 : 0;
  } else {
    F3 hp = f3(0, 0, 0);
    Geom g;
    float t = FLT_MAX;
    int obj = closest_hit<ACCEL, true, true>(P.sc, st, ray, hp, g, ct, nullptr, &t);
    if (t_max && obj >= 0 && !(t < t_max[i])) obj = -1;
    P.hit_id[i] = obj;
    if (P.t) P.t[i] = obj < 0 ? FLT_MAX : t;
    if (obj < 0) hp = f3(0, 0, 0);
    if (P.hit_point) store_f3(P.hit_point, i, hp);
    if (EXTRAS && P.normal) store_f3(P.normal, i, obj < 0 ? f3(0, 0, 0) : get_normal(g, P.sc.normals, hp));
  }

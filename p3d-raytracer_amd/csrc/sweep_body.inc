// sweep_body.inc — the body of sweep_sphere_device_kernel, included into each of the kernels of that name (sweep_query.hpp): `P` is the kernel's SweepParams, `filters` its source
// of filters (queries.hpp FilterParams or NoFilterSource).  The lane's filter is loaded once, behind the bounds check and in front
// of the search.  Text and not a function: the unfiltered kernel then is, instruction for instruction, the kernel it was before
// there were filters - as an inlined function taking P by reference it was not (DESIGN.md "Filtered queries").
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  if (i >= P.n) return;
  const size_t row = i;  // (3 * row in 64 bits)
  const float o[3] = {P.origin[3 * row], P.origin[3 * row + 1], P.origin[3 * row + 2]};
  const float d[3] = {P.direction[3 * row], P.direction[3 * row + 1], P.direction[3 * row + 2]};
  SweepRay s;
  sweep_ray(o, d, P.radius[i], P.t_max != nullptr, P.t_max ? P.t_max[i] : 0.0f, s);
  SweepBest best{s.limit, kSweepNoObject, 0u};
  const auto filter = filters.load(i, P.sc.n_objs);
  if (s.ok && P.sc.n_objs > 0) {
    if (ACCEL == P3D_ACCEL_BVH) bvh_sweep(P.sc, st, s, best, filter);
    else brute_sweep(P.sc, s, best, filter);
  }
  const bool found = best.object != kSweepNoObject;
  int32_t object = -1;
  float t = FLT_MAX;
  F3 c = f3(0, 0, 0), q = f3(0, 0, 0), nrm = f3(0, 0, 0);
  if (found) {
    const Geom g = load_geom(ACCEL == P3D_ACCEL_BVH ? P.sc.bgeom : P.sc.ogeom, best.slot);
    const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
    float cc[3], qq[3];
    sweep_centre(s, best.t, cc);
    nearest_point(geom_type(g), v, cc, qq);
    object = best.object;
    t = best.t;
    c = f3(cc[0], cc[1], cc[2]);
    q = f3(qq[0], qq[1], qq[2]);
    if (P.normal) nrm = get_normal(g, P.sc.normals, q);
  }
  P.object[i] = object;
  if (P.t) P.t[i] = t;
  if (P.centre) store_f3(P.centre, row, c);
  if (P.contact) store_f3(P.contact, row, q);
  if (P.normal) store_f3(P.normal, row, nrm);
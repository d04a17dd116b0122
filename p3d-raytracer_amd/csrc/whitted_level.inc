// whitted_level.inc — ONE level of the reflect / refract chain of rayTracing (main.cpp:92-309): closest hit, shadow
// feelers + Blinn-Phong, and the child ray (reflection, or refraction of a transmissive material).  Included by the chain
// loop of whitted_sample.inc (megakernels: the whole chain in one lane) and by wf_level_kernel (wavefront launches: one
// level per launch).  Not a header of its own.
// In scope: P, sc, st, ct, rng, ray, depth, ior_1, inside, level, ghost, GHOST (zero-weight reflection rays are put aside), si, sj, SPP, gid, n_deferred, cold (ColdState), COLD, VOTE, the
// macro P3D_FIRST_HIT(obj) (what the includer does with the object the pixel's first primary ray hit); with
// LIT != 0 also unit_touched, unit_ch0, H (the hand-off records: H.first / H.first_sample of `unit` are written here) and unit.
// Leaves: chain_ended (true: chain_result is the colour this chain ends with); otherwise col / weight = this level's record
// and child_o / child_d / child_ior / child_inside = the ray that continues the chain (origin and direction only: the
// reciprocals of a RayS are worked out where the ray is traced, not carried to it).
            F3 col = f3(0, 0, 0);
            bool have_child = false;
            float weight = 0.0f;
            F3 child_o = f3(0, 0, 0), child_d = f3(0, 0, 0);
            bool child_inside = inside;
            float child_ior = ior_1;
            bool chain_ended = true;
            do {
              PT_REGION(1)
              F3 Pn;
              Geom g;
              bool root_passed = false;
              Counters<STATS> ct_before;
              if (STATS && LIT != 0 && level == 0 && !ghost && !unit_touched) ct_before = ct;
              float hit_t = FLT_MAX;
              const int obj = closest_hit<ACCEL, SPILL, VOTE>(sc, st, ray, Pn, g, ct, LIT != 0 ? &root_passed : nullptr,
                                                        ACCEL == P3D_ACCEL_NONE ? &hit_t : nullptr);
              PT_REGION(2)
              if (level == 0 && !ghost) {
                if (si == 0 && sj == 0) P3D_FIRST_HIT(obj);
                if (LIT != 0 && root_passed && !unit_touched) {  // what the hand-off check compares (handoff.hpp)
                  if (STATS)  // the tests of this query on their own (handoff.hpp: uch0)
                    for (int k = 0; k < kCh0Counters; ++k) unit_ch0[k] = ct.get(kNodeTests + k) - ct_before.get(kNodeTests + k);
                  unit_touched = true;  // (the record goes to memory here: nothing of it has to live through the chain)
#ifndef P3D_ABL_NO_RECORDS
                  H.first[unit] = obj < 0 ? make_float4(0.f, 0.f, 0.f, __int_as_float(-1)) : make_float4(Pn.x, Pn.y, Pn.z, __int_as_float(obj));
                  if (AA) H.first_sample[unit] = (uint32_t)(si * SPP + sj);
#endif
                }
              }
              if (ACCEL == P3D_ACCEL_NONE && P.debug_view == P3D_DEBUG_DEPTH_MAP) {  // main.cpp:127-139, hit or not
                const float grey = 1.f + (hit_t - 5.f) * (0.f - 1.f) / (20.f - 5.f);  // remap(5, 20, 1, 0, min_t), main.cpp:86-88
                chain_result = clamp01(f3(grey, grey, grey));
                break;
              }
              if (obj < 0) {  // main.cpp:144-147
                chain_result = miss_color(P.sc, P.skybox != 0, ray.d);
                break;
              }
              if (P.debug_view == P3D_DEBUG_TEST_INTERSECT) {  // main.cpp:156
                chain_result = f3(1, 0, 0);
                break;
              }
              PT_REGION(9)
              ct.add(kShadedHits);
              const uint32_t m = geom_material(g);  // material rows are re-read where used, not carried
              const F3 intercept = offset_intersection(Pn, get_normal(g, sc.normals, Pn));  // main.cpp:165
              F3 norm = get_normal(g, sc.normals, intercept);                               // main.cpp:167
              cold.set_pn(Pn);
              cold.clear_sums();  // diff, spec of main.cpp:170
              PT_REGION(10)
              const bool dead_spec_mat = sc.mats[4 * m + 3].w != 0.0f;  // (read once per shading point, not per light: the feelers' stack traffic keeps the compiler from hoisting it)
              if (!inside) {  // main.cpp:172-227
                for (uint32_t li = 0; li < sc.n_lights; ++li) {
                  // the light index is wave-uniform: read through the scalar cache (s_load), not LDS
                  const float4 l0 = P.sc.lights[2 * li];
                  F3 lpos = xyz(l0);
                  if (AA && P.soft_shadows) {  // main.cpp:180-186 (g++ draws y first)
                    const float jy = rng.rand_float();
                    const float jx = rng.rand_float();
                    lpos = f3(l0.x + P.light_side * (si + jx) / SPP, l0.y + P.light_side * (sj + jy) / SPP, l0.z);
                  }
                  PT_REGION(3)
                  const F3 l_dir = normalized(lpos - intercept);
                  RayS feeler;
                  ray_set(feeler, intercept, l_dir);
                  ct.add(kRaysShadow);
                  PT_REGION(4)
                  const bool shadowed = any_hit<ACCEL, SPILL, VOTE>(sc, st, feeler, ct);
                  PT_REGION(5)
                  F3 l_dir_now = l_dir;
                  if (COLD) {  // the light direction is worked out again rather than kept in registers through the traversal
                    F3 at = intercept;  // (same operands, same operations: same bits; the barrier keeps the compiler from merging the two)
                    asm volatile("" : "+v"(at.x), "+v"(at.y), "+v"(at.z));
                    l_dir_now = normalized(xyz(P.sc.lights[2 * li]) - at);
                  }
                  const F3 blinn = normalized((l_dir_now + get_direction(ray) * -1.0f) / 2);
                  if (!shadowed) {  // main.cpp:222-225: max() and pow() evaluate in double
                    const float4 l1 = P.sc.lights[2 * li + 1];
                    const float4 m0 = sc.mats[4 * m], m1 = sc.mats[4 * m + 1];
                    const float shine = sc.mats[4 * m + 2].x;
                    const float nl = dot(norm, l_dir_now);
                    const float bn = dot(blinn, norm);
                    const float kd = (0.0f > nl) ? 0.0f : nl;
                    const float kb = (0.0f > bn) ? 0.0f : bn;
                    // (a material whose specular term is multiplied by Ks == 0 in main.cpp:232 and cannot be anything but a finite
                    // non-negative number - flagged at upload, capi_scene_layout.hpp - does not need its value: for 0 <= kb <= 1 the power is in
                    // [0, 1], the product a finite number >= +0, and leaving it out of a sum of such numbers changes no bit of
                    // diff * Kd + spec * 0.  A NaN cosine fails kb <= 1 and takes the full path.)
                    const bool dead_spec = dead_spec_mat && kb <= 1.0f;
                    const float pw = dead_spec ? 0.0f : (float)pow_spec((double)kb, (double)shine);
                    cold.add((xyz(l1) * xyz(m0)) * kd, (xyz(l1) * xyz(m1)) * pw);
                  }
                }
              }
              PT_REGION(6)
              const float4 m2 = sc.mats[4 * m + 2];
              const float mKd = sc.mats[4 * m].w, mKs = sc.mats[4 * m + 1].w;
              col = cold.diff() * mKd + cold.spec() * mKs;  // main.cpp:232
              if (depth <= 0) {
                chain_result = clamp01(col);
                break;
              }
              norm = !inside ? norm : norm * -1.0f;  // main.cpp:238
              const F3 v = get_direction(ray) * -1.0f;
              const F3 vn = norm * dot(v, norm);
              F3 vt = vn - v;
              if (m2.y == 0) {          // opaque: Kr = Ks (main.cpp:250)
                if (m2.w > 0) {         // reflective (main.cpp:290-300)
                  // g++ evaluates the right operand of `+` first; both calls re-normalise ray.d
                  const F3 b = get_direction(ray);
                  const F3 a = norm * dot(get_direction(ray) * -1.0f, norm) * 2;
                  child_o = intercept;
                  child_d = a + b;
                  weight = mKs;
                  have_child = true;
                  ct.add(kRaysReflect);
                }
              } else {                  // transmissive (main.cpp:252-283): Kr = 1/2*(Rs+Rp) == 0 (Q3)
                const float n = !inside ? ior_1 / m2.z : ior_1 / 1;
                const float sinOt = n * length(vt);
                const float insqrt = (float)(1 - (double)sinOt * (double)sinOt);  // 1 - pow(sinOt,2) in double
                if (insqrt >= 0) {
                  const float cosOt = sqrtf(insqrt);
                  F3 refractDir = normalized(vt) * sinOt + norm * (-cosOt);
                  refractDir = normalized(refractDir);
                  child_o = offset_intersection(cold.pn(), refractDir);  // main.cpp:267
                  child_d = refractDir;
                  child_ior = !inside ? m2.z : 1.0f;
                  child_inside = !inside;
                  weight = 1.0f;  // (1 - Kr) with Kr == 0
                  have_child = true;
                  ct.add(kRaysRefract);
                }
                if (GHOST && m2.w > 0) {  // the zero-weight reflection ray (main.cpp:290-300), traced after this subtree
                  const F3 b = get_direction(ray);
                  const F3 a = norm * dot(get_direction(ray) * -1.0f, norm) * 2;
                  const F3 rd = a + b;
                  P.deferred[(size_t)(2 * n_deferred) * P.level_stride + gid] =
                      make_float4(intercept.x, intercept.y, intercept.z, __int_as_float((depth - 1) | (inside ? 0x40000000 : 0)));
                  P.deferred[(size_t)(2 * n_deferred + 1) * P.level_stride + gid] = make_float4(rd.x, rd.y, rd.z, ior_1);
                  ++n_deferred;
                  ct.add(kRaysReflect);
                }
              }
              if (!have_child) {
                chain_result = clamp01(col);
                break;
              }
              chain_ended = false;
            } while (0);

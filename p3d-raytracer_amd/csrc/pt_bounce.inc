// pt_bounce.inc — one bounce of the path tracer: the body of Radiance (main.cpp:313-516) from the closest hit to the ray of the
// next bounce, included verbatim inside the persistent bounce loop of pt_body.inc (the frame kernels) and of path_query_kernel
// (path_query.hpp: rays from device memory).  One spelling, so that a sample of a query and a sample of a frame are the same
// operations in the same order.  `continue` goes round the includer's loop.  Not a header of its own.
// In scope: ACCEL, LDS, SUB, PT_STACK, MAXD, P (sc, skybox, debug_view), sc, st, ct, ray, rng, T, L, depth, alive, first_ray,
// first_hit, pend (base, stride, n), and for SUB == 4 shared and px.
        // ---- one bounce: the body of Radiance ----
        PT_REGION(2)
        F3 Pn;
        Geom g;
        const int obj = closest_hit<ACCEL, PT_STACK, !LDS, true>(sc, st, ray, Pn, g, ct);
        PT_REGION(3)
        if (first_ray) {
          first_hit = obj;
          if (SUB == 4) shared.first_hit[px] = obj;
          first_ray = false;
        }
        if (obj < 0 || depth == 0) {  // main.cpp:350-355: the background acts as an environment light
          L = L + T * miss_color(P.sc, P.skybox != 0, ray.d);
          alive = false;
          continue;
        }
        if (P.debug_view == P3D_DEBUG_TEST_INTERSECT) {  // main.cpp:359
          L = L + T * f3(1, 0, 0);
          alive = false;
          continue;
        }
        ct.add(kShadedHits);
        const uint32_t m = geom_material(g);
        const float4 m0 = sc.mats[4 * m], m1 = sc.mats[4 * m + 1], m2 = sc.mats[4 * m + 2], m3 = sc.mats[4 * m + 3];
        const F3 E = xyz(m3);
        const F3 norm = get_normal(g, sc.normals, Pn);                         // main.cpp:366
        const F3 norml = (dot(norm, ray.d) < 0) ? norm : norm * -1.0f;         // main.cpp:368
        const F3 intercept_out = offset_intersection(Pn, norm);
        const F3 intercept_in = offset_intersection(Pn, norm * -1.0f);
        F3 f = xyz(m0);
        const float p = max3_ref(f.x, f.y, f.z);
        if (--depth <= MAXD - 5) {  // Russian roulette, main.cpp:382-388
          if (rng.rand_float() < p) {
            f = f * (1 / p);
          } else {
            L = L + T * E;
            alive = false;
            continue;
          }
        }
        if (m0.w == 1.0f) {  // ideal diffuse, main.cpp:391-480
          PT_REGION(4)
          const float r1 = 2 * kPIf * rng.rand_float();
          const float r2 = rng.rand_float();
          const float r2s = sqrtf(r2);
          const F3 w = norml;
          const F3 u = normalized(cross(gt_0p1(fabsf(w.x)) ? f3(0, 1, 0) : f3(1, 0, 0), w));
          const F3 v = cross(w, u);
          double s1, c1;
          det_sincos((double)r1, s1, c1);
          const F3 d = normalized((u * (float)c1 * r2s + v * (float)s1 * r2s) + w * sqrtf(1 - r2));
          F3 e = f3(0, 0, 0);
          for (uint32_t k = 0; k < sc.n_emitters; ++k) {  // explicit light sampling, main.cpp:407-477
            const uint32_t lobj = sc.emitters[k];
            const Geom lg = load_geom(sc.ogeom, lobj);
            const F3 center = f3(lg.a.x, lg.a.y, lg.a.z);
            const float rad = lg.a.w;
            const F3 sw = center - intercept_out;
            const F3 su = normalized(cross(gt_0p1(fabsf(sw.x)) ? f3(0, 1, 0) : f3(1, 0, 0), sw));
            const F3 sv = cross(sw, su);
            const F3 ic = intercept_out - center;
            const double cos_a_max = sqrt(1 - ((double)rad * (double)rad) / (double)dot(ic, ic));
            const double eps1 = rng.erand48();
            const double eps2 = rng.erand48();
            const double cos_a = 1 - eps1 + eps1 * cos_a_max;
            const double sin_a = sqrt(1 - cos_a * cos_a);
            const double phi = (double)(2 * kPIf) * eps2;
            double sphi, cphi;
            det_sincos(phi, sphi, cphi);
            const F3 l = normalized((su * (float)cphi * (float)sin_a + sv * (float)sphi * (float)sin_a) + sw * (float)cos_a);
            RayS feeler;
            ray_set(feeler, intercept_out, l);
            ct.add(kRaysLight);
            // what main.cpp:472-475 multiplies when the sample is visible, worked out before the traversal: two floats live
            // through it instead of l, norml and a double (same operands, same operations: same bits)
            const float omega_f = (float)((double)(2 * kPIf) * (1 - cos_a_max));
            const float l_dot_n = dot(l, norml);
            F3 hp2;
            Geom g2;
            PT_REGION(5)
            const int hit2 = closest_hit<ACCEL, PT_STACK, !LDS, true>(sc, st, feeler, hp2, g2, ct);
            PT_REGION(6)
            if (hit2 >= 0 && hit2 == (int)lobj) {  // main.cpp:472-475
              const F3 emi = xyz(sc.mats[4 * geom_material(load_geom(sc.ogeom, lobj)) + 3]);
              e = e + f * (emi * l_dot_n * omega_f) * (1 / kPIf);
            }
          }
          L = L + T * (E + e);
          T = T * f;
          ray_set(ray, intercept_out, d);
          ct.add(kRaysBounce);
          continue;
        }
        if (m1.w == 1.0f) {  // mirror, main.cpp:481-484
          PT_REGION(7)
          L = L + T * E;
          T = T * f;
          ray_set(ray, intercept_out, ray.d - norm * (2 * dot(norm, ray.d)));
          ct.add(kRaysBounce);
          continue;
        }
        // dielectric, main.cpp:486-515
        PT_REGION(8)
        const F3 refl_d = ray.d - norm * 2 * dot(norm, ray.d);
        const bool into = dot(norm, norml) > 0;
        const double nc = 1.0, nt = (double)m2.z;
        const double nnt = into ? nc / nt : nt / nc;
        const double ddn = (double)dot(ray.d, norml);
        const double cos2t = 1 - nnt * nnt * (1 - ddn * ddn);
        L = L + T * E;
        T = T * f;
        if (cos2t < 0) {  // total internal reflection
          ray_set(ray, intercept_out, refl_d);
          ct.add(kRaysBounce);
          continue;
        }
        const F3 tdir = normalized(ray.d * (float)nnt - norm * (float)((into ? 1 : -1) * (ddn * nnt + sqrt(cos2t))));
        const double a = nt - nc, b = nt + nc;
        const double R0 = (a * a) / (b * b);
        const double cc = 1 - (into ? -ddn : (double)dot(tdir, norm));
        const double Re = R0 + (1 - R0) * cc * cc * cc * cc * cc;
        const double Tr = 1 - Re;
        const double Pp = 0.25 + 0.5 * Re;
        const double RP = Re / Pp, TP = Tr / (1 - Pp);
        if (depth <= MAXD - 2) {  // main.cpp:509-511: choose one
          if (rng.erand48() < Pp) {
            T = T * (float)RP;
            ray_set(ray, intercept_out, refl_d);
          } else {
            T = T * (float)TP;
            ray_set(ray, intercept_out, tdir);
          }
          ct.add(kRaysBounce);
        } else {  // first two bounces trace both; g++ evaluates the transmission operand first
          {  // at most two levels fork (depth > MAX_DEPTH-2), so two pending entries suffice
            const F3 Tr_ = T * (float)Re;
            pend.base[(size_t)(pend.n * 3 + 0) * pend.stride] = make_float4(intercept_out.x, intercept_out.y, intercept_out.z, refl_d.x);
            pend.base[(size_t)(pend.n * 3 + 1) * pend.stride] = make_float4(refl_d.y, refl_d.z, Tr_.x, Tr_.y);
            pend.base[(size_t)(pend.n * 3 + 2) * pend.stride] = make_float4(Tr_.z, __int_as_float(depth), 0, 0);
            ++pend.n;
          }
          T = T * (float)Tr;
          ray_set(ray, intercept_in, tdir);
          ct.add(kRaysBounce, 2);
        }

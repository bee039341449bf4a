// rtc_trace_body.inc — the body of the one-kernel path's kernel (rtc_device.hpp rtc_trace_kernel / rtc_trace_kernel_uv), included
// inside both so that the kernels scenes without a UV pattern run keep their names and their code.  Template parameters and the
// constants COUNT, FEAT, KOPS, LEAN, AREA, UV come from the including kernel.
  RTC_LDS_STACK(lds_stack);
  int* stack = lds_stack + threadIdx.x;
  const int stride = RTC_BLOCK;
  Counters C = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned n_primary = 0, n_shadow = 0, n_reflect = 0, n_refract = 0, n_container = 0;
  const WorkMap wm = make_workmap(pm, cam);
#ifdef RTC_DIAG
  if (threadIdx.x < 64) s_diag[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long diag_t0_ = 0;
  const unsigned long long diag_k0 = __builtin_amdgcn_s_memtime();
#endif

  const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t q = 0;
  const bool have = id < wm.n_work && work_to_slot(wm, id, q);

  if (have) {
    Ray ray = slot_ray(pm, cam, q);

    Pending pend[LEAN ? 1 : RTC_MAX_FUEL];
    int np = 0;
    double acc_r = 0.0, acc_g = 0.0, acc_b = 0.0;
    double weight = 1.0;
    int fuel = fuel0;
    int kind = 0;
    bool first = true;
    unsigned long long dg = 0ull;  // hit-tree digest (counting variant with pm.digest set)
    const double L = (double)S.n_lights;

    for (;;) {
      if (kind == 0) n_primary++; else if (kind == 1) n_reflect++; else n_refract++;
      DIAG_LOOP(4);
      DIAG_T0();
      Trav T;
      reset_closest(T, MODE_CLOSEST);
      traverse<FEAT, KOPS, MODE_CLOSEST>(S, ray, T, C, stack, stride);
      nan_commit(T, C);
      DIAG_REGION(0);
      bool did_hit = T.best_prim != 0x7fffffff;
      if (COUNT && pm.digest) {
        unsigned long long tb = 0ull;
        if (did_hit) __builtin_memcpy(&tb, &T.best_t, 8);
        dg += rtc_hit_hash(rtc_hit_hash_base(tb, did_hit ? T.best_prim : -1, did_hit ? T.best_k : 0), fuel0 - fuel, kind);
      }
      if (first) {
        first = false;
        if (hit_t) {
          hit_t[q] = did_hit ? T.best_t : 0.0;
          hit_prim[q] = did_hit ? T.best_prim : -1;
          hit_k[q] = did_hit ? T.best_k : 0;
        }
      }
      if (did_hit) {
        const DPrim P = S.prims[T.best_prim];
        const double* M = S.mat + 8 * P.mat;
        const double ambient = M[0], diffuse = M[1], specular = M[2], shininess = M[3], reflective = M[4], transparency = M[5];
        State st;
        double hu, hv;
        hit_uv(S, P, ray, hu, hv);
        prepare_state(S, P, ray, T.best_t, hu, hv, st);

        // n1 / n2 / reflectance are only consumed when the surface is transparent (src/world.rs:70-78, :110)
        double n1 = 1.0, n2 = 1.0;
        if (transparency != 0.0 && fuel > 0) {
          n_container++;
          Trav K = T;  // keeps the hit key (thi = best_t, best_prim, best_klast)
          K.mode = MODE_CONTAINERS;
          K.tlo = -DINF; K.thi = T.best_t;
          K.c1_prim = -1; K.c2_prim = -1; K.c1_t = 0.0; K.c2_t = 0.0;
          traverse<FEAT, KOPS, MODE_CONTAINERS>(S, ray, K, C, stack, stride);
          if (K.c1_prim >= 0) n1 = S.mat[8 * S.prims[K.c1_prim].mat + 6];
          if (K.c2_prim >= 0) n2 = S.mat[8 * S.prims[K.c2_prim].mat + 6];
          DIAG_REGION(1);
        }

        // Pattern::color_at(material_inv * over_point) — identical for every light (src/shape.rs:437)
        double cr, cg, cb;
        {
          const double* mi = S.xf_matinv + 16 * P.xform;
          double x = mi[0] * st.px + mi[1] * st.py + mi[2] * st.pz + mi[3] * 1.0;
          double y = mi[4] * st.px + mi[5] * st.py + mi[6] * st.pz + mi[7] * 1.0;
          double z = mi[8] * st.px + mi[9] * st.py + mi[10] * st.pz + mi[11] * 1.0;
          double w = mi[12] * st.px + mi[13] * st.py + mi[14] * st.pz + mi[15] * 1.0;
          const DPat& root = S.pats[S.mat_pattern[P.mat]];
          if (LEAN || root.tag == 1) { cr = root.color[0]; cg = root.color[1]; cb = root.color[2]; }
          else if constexpr (UV) pattern_color_uv(S, S.mat_pattern[P.mat], x, y, z, w, cr, cg, cb);
          else pattern_color(S, S.mat_pattern[P.mat], x, y, z, w, cr, cg, cb);
        }

        const bool blend = !LEAN && reflective > 0.0 && transparency > 0.0;  // (LEAN: DScene.no_glass_mirror)
        double R = 0.0;
        if (blend) R = blend_reflectance(st, n1, n2, fuel, cr, cg, cb);

        DIAG_REGION(2);
        // World::shade_hit (src/world.rs:50-82): per light, shadow test + Phong (src/shape.rs:429-462)
        double sr = 0.0, sg = 0.0, sb = 0.0;
        if constexpr (AREA) {
          shade_lights_area<FEAT, KOPS, false, true>(S, st.px, st.py, st.pz, st.nx, st.ny, st.nz, st.ex, st.ey, st.ez, cr, cg, cb, ambient, diffuse, specular,
                                                     shininess, C, stack, stride, n_shadow, LdsScene{}, sr, sg, sb);
        } else
        for (int l = 0; l < S.n_lights; l++) {
          DIAG_LOOP(5);
          const double* LG = S.lights + 6 * l;
          double vx = LG[3] - st.px, vy = LG[4] - st.py, vz = LG[5] - st.pz;
          n_shadow++;
          if (light_is_behind(S, vx, vy, vz, st.nx, st.ny, st.nz)) {  // ambient term only, in the expression of the general case
            const double lr = (cr * LG[0]) * ambient, lg = (cg * LG[1]) * ambient, lb = (cb * LG[2]) * ambient;
            sr += (lr + 0.0) + 0.0; sg += (lg + 0.0) + 0.0; sb += (lb + 0.0) + 0.0;
            continue;
          }
          double distance = sqrt(vx * vx + vy * vy + vz * vz);
          Ray sray;
          sray.ox = st.px; sray.oy = st.py; sray.oz = st.pz;
          sray.dx = vx / distance; sray.dy = vy / distance; sray.dz = vz / distance;
          Trav Sh;
          reset_closest(Sh, S.all_cast_shadow ? MODE_SHADOW_ANY : MODE_SHADOW_CLOSEST);
          if (S.all_cast_shadow) Sh.thi = distance;
          Sh.light = l; Sh.c1_t = distance;
          DIAG_T0();
          traverse<FEAT, KOPS>(S, sray, Sh, C, stack, stride);
          nan_commit(Sh, C);
          DIAG_REGION(3);
          bool shadowed;
          if (S.all_cast_shadow) shadowed = Sh.shadowed != 0;
          else shadowed = (Sh.best_prim != 0x7fffffff) && (S.prims[Sh.best_prim].flags & 1u) && (Sh.best_t < distance);

          double er = cr * LG[0], eg = cg * LG[1], eb = cb * LG[2];  // effective_color
          double lr = er * ambient, lg = eg * ambient, lb = eb * ambient;
          // light vector: (light.origin - point).normalize() — same numbers as the shadow ray direction
          double ldn = sray.dx * st.nx + sray.dy * st.ny + sray.dz * st.nz;
          double dr = 0.0, dg = 0.0, db = 0.0, pr = 0.0, pg = 0.0, pb = 0.0;
          if (!shadowed && ldn >= 0.0) {
            dr = er * diffuse * ldn; dg = eg * diffuse * ldn; db = eb * diffuse * ldn;
            // reflect = (-light).reflect(normal)
            double mlx = -sray.dx, mly = -sray.dy, mlz = -sray.dz;
            double d2 = 2.0 * (mlx * st.nx + mly * st.ny + mlz * st.nz);
            double rfx = mlx - st.nx * d2, rfy = mly - st.ny * d2, rfz = mlz - st.nz * d2;
            double rde = rfx * st.ex + rfy * st.ey + rfz * st.ez;
            if (rde > 0.0) {
              double f = specular_factor(rde, shininess, specular);
              pr = LG[0] * specular * f; pg = LG[1] * specular * f; pb = LG[2] * specular * f;
            }
          }
          sr += (lr + dr) + pr; sg += (lg + dg) + pg; sb += (lb + db) + pb;
        }
        acc_r += weight * sr; acc_g += weight * sg; acc_b += weight * sb;
        DIAG_T0();

        // reflected_color / refracted_color (src/world.rs:84-132), once per light in the reference -> factor L
        if (fuel > 0) {
          bool do_refl = reflective != 0.0;
          bool do_refr = transparency != 0.0;
          double wr = weight * L * reflective, wt = weight * L * transparency;
          if (blend) {
            wr *= R;
            wt *= (1.0 - R);
          }
          double tdx = 0.0, tdy = 0.0, tdz = 0.0;
          if (do_refr) {
            double n_ratio = n1 / n2;
            double cos_i = st.ex * st.nx + st.ey * st.ny + st.ez * st.nz;
            double sin2_t = (n_ratio * n_ratio) * (1.0 - cos_i * cos_i);
            if (sin2_t > 1.0) do_refr = false;
            else {
              double cos_t = sqrt(1.0 - sin2_t);
              double kk = n_ratio * cos_i - cos_t;
              tdx = st.nx * kk - st.ex * n_ratio; tdy = st.ny * kk - st.ey * n_ratio; tdz = st.nz * kk - st.ez * n_ratio;
            }
          }
          // depth-first: the reflection ray (if any) is traced next; only a refraction ray that has to wait is stacked
          if (!LEAN && do_refr && do_refl) {
            Pending& p = pend[np++];
            p.ox = st.ux; p.oy = st.uy; p.oz = st.uz; p.dx = tdx; p.dy = tdy; p.dz = tdz;
            p.weight = wt; p.fuel = fuel - 1; p.kind = 2;
          }
          if (do_refl) {
            ray.ox = st.px; ray.oy = st.py; ray.oz = st.pz; ray.dx = st.rx; ray.dy = st.ry; ray.dz = st.rz;
            weight = wr; fuel = fuel - 1; kind = 1;
            continue;
          }
          if (do_refr) {
            ray.ox = st.ux; ray.oy = st.uy; ray.oz = st.uz; ray.dx = tdx; ray.dy = tdy; ray.dz = tdz;
            weight = wt; fuel = fuel - 1; kind = 2;
            continue;
          }
        }
      }
      DIAG_REGION(5);
      if (np == 0) {
        rgb[3 * q + 0] = acc_r;
        rgb[3 * q + 1] = acc_g;
        rgb[3 * q + 2] = acc_b;
        if (COUNT && pm.digest) pm.digest[q] = dg;
        break;
      }
      const Pending& p = pend[--np];
      ray.ox = p.ox; ray.oy = p.oy; ray.oz = p.oz; ray.dx = p.dx; ray.dy = p.dy; ray.dz = p.dz;
      weight = p.weight; fuel = p.fuel; kind = p.kind;
    }
  }

#ifdef RTC_DIAG
  atomicAdd(&s_diag[14], __builtin_amdgcn_s_memtime() - diag_k0);
  atomicAdd(&s_diag[15], 1ull);
  __syncthreads();
  if (threadIdx.x < 64 && s_diag[threadIdx.x]) atomicAdd(&stats->diag[threadIdx.x], s_diag[threadIdx.x]);
#endif
  if (COUNT || true) {
    // nan_ts must always be published (error reporting); the rest only in the counting variant
    if (C.nan_ts) atomicAdd(&stats->nan_ts, (unsigned long long)C.nan_ts);
  }
  if (COUNT) {
    atomicAdd(&stats->rays_primary, (unsigned long long)n_primary);
    atomicAdd(&stats->rays_shadow, (unsigned long long)n_shadow);
    atomicAdd(&stats->rays_reflect, (unsigned long long)n_reflect);
    atomicAdd(&stats->rays_refract, (unsigned long long)n_refract);
    atomicAdd(&stats->rays_container, (unsigned long long)n_container);
    atomicAdd(&stats->accel_nodes, (unsigned long long)C.accel_nodes);
    atomicAdd(&stats->group_tests, (unsigned long long)C.group_tests);
    atomicAdd(&stats->tri_tests, (unsigned long long)C.tri_tests);
    atomicAdd(&stats->analytic_tests, (unsigned long long)C.analytic_tests);
    atomicAdd(&stats->knodes, (unsigned long long)C.knodes);
    atomicAdd(&stats->kplanes, (unsigned long long)C.kplanes);
    atomicAdd(&stats->light_cells, (unsigned long long)C.light_cells);
    atomicAdd(&stats->kgroups, (unsigned long long)C.kgroups);
  }

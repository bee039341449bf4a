// wf_shade_body.inc — the body of the wavefront path's shading kernel (rtc_kernels.hip wf_shade / wf_shade_uv), included inside both
// so that the kernels scenes without a UV pattern run keep their names and their code.  COUNT, PAT and UV come from the including
// kernel.
  // per wave and class: its count, then its base index in the queue (double-buffered by iteration parity: no barrier needed before
  // the next iteration writes).  Classes keep like with like inside a block's span of the queues, so that most 64-item chunks of the
  // next traversal launch hold one kind of ray: shade records on planes / on other primitives; reflected rays off planes (mirror
  // images of their coherent parents) / off other primitives / refracted rays.
  __shared__ unsigned s_rec2[2][2][16], s_child2[2][3][16];
  unsigned parity = 0;
  const WorkMap wm = make_workmap(pm, cam);
  const unsigned count = wf_count(W, level, n0);
  const size_t cap = W.cap;
  const double L = (double)S.n_lights;
  const int fuel = fuel0 - level;
  unsigned n_reflect = 0, n_refract = 0;
  int32_t* ch = W.child + (size_t)level * 2 * cap;
  double* nq = W.rq[(level + 1) & 1];
  const int lane = RTC_LANE_ID;
  const int wave = (int)(threadIdx.x / (RTC_WF_SHADE_BLOCK >= 64 ? 64 : 1));
  const int n_waves = RTC_WF_SHADE_BLOCK >= 64 ? RTC_WF_SHADE_BLOCK / 64 : 1;
  for (unsigned base = blockIdx.x * RTC_WF_SHADE_BLOCK; base < count; base += gridDim.x * RTC_WF_SHADE_BLOCK) {  // block-uniform bound: barriers inside
    const unsigned i = base + threadIdx.x;
    int prim = -1;
    if (i < count) prim = W.h_prim[i];
    const bool hit = prim >= 0;
    State st;
    double cr = 0.0, cg = 0.0, cbl = 0.0, weight = 1.0, n1 = 1.0, n2 = 1.0;
    int mat = 0, geom = 0;
    double reflective = 0.0, transparency = 0.0;
    if (hit) {
      Ray ray;
      if (level == 0) {
        uint64_t q = 0;
        (void)work_to_slot(wm, i, q);
        ray = slot_ray(pm, cam, q);
      } else {
        ray = wf_load_ray(W, level, i, weight);
      }
      const DPrim P = S.prims[prim];
      mat = P.mat;
      geom = P.geom;
      const double* M = S.mat + 8 * P.mat;
      reflective = M[4]; transparency = M[5];
      double hu, hv;
      hit_uv(S, P, ray, hu, hv);
      prepare_state(S, P, ray, W.h_t[i], hu, hv, st);
      if (transparency != 0.0 && fuel > 0) { n1 = W.h_n12[i]; n2 = W.h_n12[cap + i]; }  // stored under the same condition
      // Pattern::color_at(material_inv * over_point) — identical for every light (src/shape.rs:437)
      const double* mi = S.xf_matinv + 16 * P.xform;
      double x = mi[0] * st.px + mi[1] * st.py + mi[2] * st.pz + mi[3] * 1.0;
      double y = mi[4] * st.px + mi[5] * st.py + mi[6] * st.pz + mi[7] * 1.0;
      double z = mi[8] * st.px + mi[9] * st.py + mi[10] * st.pz + mi[11] * 1.0;
      double w = mi[12] * st.px + mi[13] * st.py + mi[14] * st.pz + mi[15] * 1.0;
      const DPat& root = S.pats[S.mat_pattern[P.mat]];
      if (!PAT || root.tag == 1) { cr = root.color[0]; cg = root.color[1]; cbl = root.color[2]; }
      else if constexpr (UV) pattern_color_uv(S, S.mat_pattern[P.mat], x, y, z, w, cr, cg, cbl);
      else pattern_color(S, S.mat_pattern[P.mat], x, y, z, w, cr, cg, cbl);
    }
    const bool blend = hit && reflective > 0.0 && transparency > 0.0;
    double R = 0.0;
    if (blend) R = blend_reflectance(st, n1, n2, fuel, cr, cg, cbl);  // (a NaN reflectance: the record's colour becomes NaN)
    // reflected_color / refracted_color (src/world.rs:84-132), once per light in the reference -> factor L
    bool do_refl = false, do_refr = false;
    double wr = 0.0, wt = 0.0, tdx = 0.0, tdy = 0.0, tdz = 0.0;
    if (hit && fuel > 0) {
      do_refl = reflective != 0.0;
      do_refr = transparency != 0.0;
      wr = weight * L * reflective; wt = weight * L * transparency;
      if (blend) {
        wr *= R;
        wt *= (1.0 - R);
      }
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
    }
    // queue space: shade records and child rays (a wave's reflected rays first, then its refracted ones); one pair of
    // atomics per block and iteration
    const unsigned long long lt = (1ull << lane) - 1ull;
    const bool on_plane = hit && geom == 1;
    const unsigned long long m_rec0 = __ballot(hit && on_plane ? 1 : 0), m_rec1 = __ballot(hit && !on_plane ? 1 : 0);
    const unsigned long long m_c0 = __ballot(do_refl && on_plane ? 1 : 0), m_c1 = __ballot(do_refl && !on_plane ? 1 : 0), m_c2 = __ballot(do_refr ? 1 : 0);
    unsigned (*s_rec)[16] = s_rec2[parity];
    unsigned (*s_child)[16] = s_child2[parity];
    parity ^= 1u;
    if (lane == 0) {
      s_rec[0][wave] = (unsigned)__popcll(m_rec0); s_rec[1][wave] = (unsigned)__popcll(m_rec1);
      s_child[0][wave] = (unsigned)__popcll(m_c0); s_child[1][wave] = (unsigned)__popcll(m_c1); s_child[2][wave] = (unsigned)__popcll(m_c2);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned tr = 0, tc = 0;
      for (int w = 0; w < n_waves; w++) { tr += s_rec[0][w] + s_rec[1][w]; tc += s_child[0][w] + s_child[1][w] + s_child[2][w]; }
      unsigned br = tr ? atomicAdd(&W.counts[RTC_WF_SHADE_COUNT + level], tr) : 0u;
      unsigned bc = tc ? atomicAdd(&W.counts[level + 1], tc) : 0u;
      if ((unsigned long long)br + tr > W.cap || (unsigned long long)bc + tc > W.cap) { W.counts[RTC_WF_OVERFLOW] = 1u; stats->wf_overflow = 1ull; }
      for (int k = 0; k < 2; k++)
        for (int w = 0; w < n_waves; w++) { unsigned r = s_rec[k][w]; s_rec[k][w] = br; br += r; }
      for (int k = 0; k < 3; k++)
        for (int w = 0; w < n_waves; w++) { unsigned c = s_child[k][w]; s_child[k][w] = bc; bc += c; }
    }
    __syncthreads();
    const unsigned s = on_plane ? s_rec[0][wave] + (unsigned)__popcll(m_rec0 & lt) : s_rec[1][wave] + (unsigned)__popcll(m_rec1 & lt);
    const unsigned jr = on_plane ? s_child[0][wave] + (unsigned)__popcll(m_c0 & lt) : s_child[1][wave] + (unsigned)__popcll(m_c1 & lt);
    const unsigned jt = s_child[2][wave] + (unsigned)__popcll(m_c2 & lt);
    if (hit && s < W.cap) {
      double* r = W.sr;
      r[s] = st.px; r[cap + s] = st.py; r[2 * cap + s] = st.pz;
      r[3 * cap + s] = st.nx; r[4 * cap + s] = st.ny; r[5 * cap + s] = st.nz;
      r[6 * cap + s] = cr; r[7 * cap + s] = cg; r[8 * cap + s] = cbl;
      W.sr_mat[s] = mat;
      W.sr_node[s] = (int32_t)i;
    }
    if (do_refl && jr < W.cap) {
      nq[jr] = st.px; nq[cap + jr] = st.py; nq[2 * cap + jr] = st.pz; nq[3 * cap + jr] = st.rx; nq[4 * cap + jr] = st.ry; nq[5 * cap + jr] = st.rz;
      nq[6 * cap + jr] = wr;
      ch[i] = (int32_t)jr;
      n_reflect++;
    }
    if (do_refr && jt < W.cap) {
      nq[jt] = st.ux; nq[cap + jt] = st.uy; nq[2 * cap + jt] = st.uz; nq[3 * cap + jt] = tdx; nq[4 * cap + jt] = tdy; nq[5 * cap + jt] = tdz;
      nq[6 * cap + jt] = wt;
      ch[cap + i] = (int32_t)jt;
      n_refract++;
    }
  }
  if (COUNT) {
    atomicAdd(&stats->rays_reflect, (unsigned long long)n_reflect);
    atomicAdd(&stats->rays_refract, (unsigned long long)n_refract);
  }

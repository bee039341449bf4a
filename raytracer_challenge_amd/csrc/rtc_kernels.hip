// rtc_kernels.hip — hand-written HIP for gfx950 (MI355X): the kernels of the hot path that do not depend on the scene's kernel
// variant (wf_shade, wf_gather, the quantiser) and the host-callable launchers.  The ray kernels (rtc_trace_kernel, wf_ts) are
// templates in rtc_device.hpp, instantiated per row of RTC_VARIANTS by rtc_feat.hip (one translation unit per row, and one more per
// general row and extension, built in parallel); the launchers here pick a scene's row (rtc_variant; rtc_general_row for a scene with a
// background or a bump table) and call through its RtcVariantOps.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../include/rtc.h"
#include "rtc_device.hpp"

#ifdef RTC_EMU
#include "rtc_feat.hip"  // the CPU emulator (tests/cpu_emu) compiles everything as one translation unit
constexpr int RTC_VARIANTS_BUILT = 6;  // ... with variants 0..5 only: it has no entry point that creates an area-light, UV or spot scene
#else
constexpr int RTC_VARIANTS_BUILT = RTC_N_VARIANTS;
#endif
// the launchers of variant v (rtc_feat.hip), one record per row of RTC_VARIANTS (all null for a row that is not built)
template <int... V>
static const RtcVariantOps& rtc_ops(int v, std::integer_sequence<int, V...>) {
  static const RtcVariantOps ops[RTC_N_VARIANTS] = {rtc_variant_ops<V>()...};
  return ops[v];
}
static const RtcVariantOps& rtc_ops(int v) { return rtc_ops(v, std::make_integer_sequence<int, RTC_VARIANTS_BUILT>{}); }
// kernel variant that renders a scene on a device path (rtc_pick_variant)
static int rtc_variant(const DScene& S, bool wavefront) {
  return rtc_pick_variant(rtc_scene_feat(S), S.n_kops > 0, S.has_area != 0, S.has_uv != 0, S.has_spot != 0, wavefront);
}

#ifndef RTC_WF_SHADE_WAVES
#define RTC_WF_SHADE_WAVES 4  // <= 128 VGPRs: two 512-thread blocks per CU, so one block's wait for its queue atomics is covered by the other
#endif
namespace {
// What a PIPE build of wf_shade reads of a ray one iteration ahead: the ray's hit, and of levels > 0 the ray itself.
struct WfShadeIn {
  int prim;  // -1: a miss, tile padding, or past the level's end
  Ray ray;
  double weight, t;
};
// (w: a linear work id of the level, top + bottom = count of them; wf_index gives its place in the two-ended queue)
__device__ __forceinline__ int wf_shade_fetch_prim(const DWave& W, const WfParts& parts, unsigned long long w, unsigned count) {
  return w < count ? W.h_prim[wf_index(parts, W.cap, (unsigned)w)] : -1;
}
// Every lane loads, without a branch: values that arrive under a branch are merged with the other path's by register copies, for which
// the compiler waits right there -- in front of the barrier the loads are meant to cross.  A lane without a hit reads the element of
// its wave's first lane instead of its own (or element 0 past the level's end): one address for all of them, in a line the wave's hits
// fetch anyway, so a miss's ray still costs no bandwidth (71 % of level 3 on the headline scene are misses).  (A wave whose work ids
// span the queue's two parts has its first lane's element at the far end: one more line for that one wave of the level.)
template <bool LV0>
__device__ __forceinline__ WfShadeIn wf_shade_prefetch(const DWave& W, const WfParts& parts, int level, unsigned long long w, int lane, unsigned count, int prim) {
  const unsigned long long first = w - (unsigned)lane;
  const unsigned j = prim >= 0 ? wf_index(parts, W.cap, (unsigned)w) : (first < count ? wf_index(parts, W.cap, (unsigned)first) : 0u);
  WfShadeIn in = {prim, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 1.0, 0.0};
  if (!LV0) in.ray = wf_load_ray(W, level, j, in.weight);  // (level 0: the camera's ray, computed where it is used)
  in.t = W.h_t[j];
  return in;
}
#ifndef RTC_EMU
// lane l's value + the values of lanes l - 1 ... down to the start of its row of 16 lanes (DPP row shifts, zeros shifted in)
__device__ __forceinline__ unsigned wf_row_scan16(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // row_shr:8
  return v;
}
#endif
}  // namespace
// PAT = false: every pattern of the scene is a Plain colour (DScene.all_plain): no pattern-tree walk and none of its 672 B of scratch per lane.
// UV: scenes with a texture-mapped pattern (DScene.has_uv): the pattern walk with the RTC_PAT_UV branch (pattern_color_uv).
// PIPE: the loop is software-pipelined: h_prim of the NEXT iteration is requested before this one's evaluation, the ray and h_t of its
// hits before this one's barrier, so they travel while the block reserves queue space and stores; and wave 0 scans the 40 class
// counters with one lane each, where thread 0 of the other builds walks them.  25 more VGPRs (97 -> 122): the PAT builds, at 127
// with 672 B of scratch (UV: 896 B), keep the plain loop -- the wave scan alone cost them 16 B more scratch per lane.
// LV0 (PIPE builds): the launch is level 0's, a compile-time fact there so that no branch surrounds the prefetch.
// NP: scenes with a bump record (include/rtc.h rtc_bump): prepare_state's NP build, so rows 3..5 of the shade record and the child rays
// carry the shading normal.  Four builds (COUNT x UV, PAT = true, no PIPE); only they take a DSceneNp.
template <bool COUNT, bool PAT = true, bool UV = false, bool PIPE = false, bool LV0 = false, bool NP = false>
__global__ void __launch_bounds__(RTC_WF_SHADE_BLOCK, RTC_WF_SHADE_WAVES) wf_shade(std::conditional_t<NP, DSceneNp, DScene> S, DCamera cam, DPixelMap pm, DWave W, int level, unsigned n0, int fuel0, DStats* __restrict__ stats) {
  // per class and wave: its count, then its base index in the queue (double-buffered by iteration parity: no barrier needed before
  // the next iteration writes).  Classes keep like with like inside a block's span of the queues, so that most 64-item chunks of the
  // next traversal launch hold one kind of ray: shade records on planes / on other primitives [0..15]; reflected rays off planes
  // (mirror images of their coherent parents) / off other primitives / refracted rays [16..39].  Entry = 8 * class + wave.
  // A block iteration makes four reservations, one per end of the two queues (DWave): records on planes at the near end, the other
  // records at the far end; rays reflected off planes at the near end, rays reflected off other primitives and then the refracted rays
  // at the far end.  end_of[class]: its reservation.
  constexpr int end_of[5] = {0, 1, 2, 3, 3};
  constexpr int n_waves = RTC_WF_SHADE_BLOCK >= 64 ? RTC_WF_SHADE_BLOCK / 64 : 1;
  static_assert(n_waves <= 8, "wf_shade: eight counters per class");
  __shared__ unsigned s_cnt2[2][40];
  unsigned parity = 0;
  const WorkMap wm = make_workmap(pm, cam);
  const bool level0 = PIPE ? LV0 : level == 0;
  const WfParts parts = level0 ? WfParts{0u, n0} : wf_count(W, level, n0);
  const unsigned count = parts.top + parts.bottom;
  const size_t cap = W.cap;
  const double L = (double)S.n_lights;
  const int fuel = fuel0 - level;
  unsigned n_reflect = 0, n_refract = 0;
  int32_t* ch = W.child + (size_t)level * 2 * cap;
  double* nq = W.rq[(level + 1) & 1];
  const int lane = RTC_LANE_ID;
  const int wave = (int)(threadIdx.x / (RTC_WF_SHADE_BLOCK >= 64 ? 64 : 1));
  const unsigned long long step = (unsigned long long)gridDim.x * RTC_WF_SHADE_BLOCK;
  WfShadeIn nx = {-1, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 1.0, 0.0};
  int nx_prim = -1;
  if (PIPE) {
    const unsigned long long w0 = (unsigned long long)blockIdx.x * RTC_WF_SHADE_BLOCK + threadIdx.x;
    nx = wf_shade_prefetch<LV0>(W, parts, level, w0, lane, count, wf_shade_fetch_prim(W, parts, w0, count));
  }
  for (unsigned long long base = (unsigned long long)blockIdx.x * RTC_WF_SHADE_BLOCK; base < count; base += step) {  // block-uniform bound: barriers inside
    const unsigned i = wf_index(parts, W.cap, (unsigned)base + threadIdx.x);  // (the ray's place in the queue; only a hit uses it)
    const WfShadeIn in = nx;
    const int prim = PIPE ? in.prim : wf_shade_fetch_prim(W, parts, base + threadIdx.x, count);
    if (PIPE) nx_prim = wf_shade_fetch_prim(W, parts, base + step + threadIdx.x, count);
    const bool hit = prim >= 0;
    State st;
    double cr = 0.0, cg = 0.0, cbl = 0.0, weight = 1.0, n1 = 1.0, n2 = 1.0;
    int mat = 0, shading_row = 0, geom = 0;
    double reflective = 0.0, transparency = 0.0;
    // mat >= 0: the record carries its colour (rows 6..8): the root pattern is not Plain, or blend_reflectance() made the colour the
    // NaN it computed (whose bits no table knows).  mat < 0, material ~mat: the colour is the material's constant and the shadow role
    // reads it with the Phong terms from the material's shading row (DScene.mat): sr_mat = RTC_SR_PLAIN | that row, rows 6..8 stay
    // unwritten.  (One register for both facts: the PAT builds have none to spare.)
    if (hit) {
      Ray ray;
      if (level0) {
        uint64_t q = 0;
        (void)work_to_slot(wm, i, q);
        ray = slot_ray(pm, cam, q);
      } else if (PIPE) {
        ray = in.ray;
        weight = in.weight;
      } else {
        ray = wf_load_ray(W, level, i, weight);
      }
      const DPrim P = S.prims[prim];
      geom = P.geom;
      const double* M = S.mat + 8 * P.mat;
      reflective = M[4]; transparency = M[5];
      mat = ~P.mat;
      if (PIPE) shading_row = (int)M[7];  // (the other builds read it where they store it: they have no register to spare)
      double hu, hv;
      hit_uv(S, P, ray, hu, hv);
      if constexpr (NP) prepare_state<true>(S, P, ray, W.h_t[i], hu, hv, st, &S.bump);
      else prepare_state(S, P, ray, PIPE ? in.t : W.h_t[i], hu, hv, st);
      if (transparency != 0.0 && fuel > 0) { n1 = W.h_n12[i]; n2 = W.h_n12[cap + i]; }  // stored under the same condition
      if constexpr (PAT) {
        if (S.pats[S.mat_pattern[P.mat]].tag != 1) {
          pattern_at<UV>(S, P, st, cr, cg, cbl);
          mat = P.mat;
        }
      }
    }
    const bool blend = hit && reflective > 0.0 && transparency > 0.0;
    double R = 0.0;
    if (blend) {
      R = blend_reflectance(st, n1, n2, fuel, cr, cg, cbl);  // (a NaN reflectance: the record's colour becomes that NaN)
      if (R != R && mat < 0) mat = ~mat;
    }
    // reflected_color / refracted_color (src/world.rs:84-132), once per light in the reference -> factor L
    ChildRays spawn = {false, false, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (hit && fuel > 0) spawn = child_rays(st, n1, n2, weight, L, reflective, transparency, blend, R);
    // queue space: shade records and child rays (a wave's reflected rays first, then its refracted ones); one pair of
    // atomics per block and iteration, after the evaluation
    const unsigned long long lt = (1ull << lane) - 1ull;
    const bool on_plane = hit && geom == 1;
    const unsigned long long m_rec0 = __ballot(hit && on_plane ? 1 : 0), m_rec1 = __ballot(hit && !on_plane ? 1 : 0);
    const unsigned long long m_c0 = __ballot(spawn.refl && on_plane ? 1 : 0), m_c1 = __ballot(spawn.refl && !on_plane ? 1 : 0), m_c2 = __ballot(spawn.refr ? 1 : 0);
    unsigned* s_cnt = s_cnt2[parity];
    parity ^= 1u;
    if (lane == 0) {
      s_cnt[wave] = (unsigned)__popcll(m_rec0); s_cnt[8 + wave] = (unsigned)__popcll(m_rec1);
      s_cnt[16 + wave] = (unsigned)__popcll(m_c0); s_cnt[24 + wave] = (unsigned)__popcll(m_c1); s_cnt[32 + wave] = (unsigned)__popcll(m_c2);
    }
    if (PIPE) nx = wf_shade_prefetch<LV0>(W, parts, level, base + step + threadIdx.x, lane, count, nx_prim);  // in flight across the reservation and the stores
    __syncthreads();
#ifndef RTC_EMU
    if (PIPE && n_waves == 8 && wave == 0) {
      // one lane per counter: lanes 0..15 the record classes (one DPP row), 16..39 the child classes (a row and a half); the totals of
      // the four reservations in one atomic instruction (lanes 0..3), so the block waits for one round trip
      const unsigned c = lane < 40 ? s_cnt[lane] : 0u;
      const unsigned in_row = wf_row_scan16(c);
      const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)in_row, 7), r01 = (unsigned)__builtin_amdgcn_readlane((int)in_row, 15);
      const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)in_row, 23), k01 = (unsigned)__builtin_amdgcn_readlane((int)in_row, 31);
      const unsigned k2 = (unsigned)__builtin_amdgcn_readlane((int)in_row, 39);
      const unsigned t_rn = r0, t_rf = r01 - r0, t_cn = k0, t_cf = k01 - k0 + k2;
      const unsigned total = lane == 0 ? t_rn : lane == 1 ? t_rf : lane == 2 ? t_cn : t_cf;
      unsigned first = 0u;
      if (lane < 4 && total) {
        const int row = lane == 0 ? RTC_WF_SHADE_COUNT + level : lane == 1 ? RTC_WF_SHADE_TOP_COUNT + level : lane == 2 ? level + 1 : RTC_WF_TOP_COUNT + level + 1;
        const unsigned old = atomicAdd(&W.counts[row], total);
        const bool fits = (unsigned long long)old + total <= W.cap;
        if (!fits) { W.counts[RTC_WF_OVERFLOW] = 1u; stats->wf_overflow = 1ull; }
        first = (lane & 1) ? (fits ? W.cap - old - total : W.cap) : old;
      }
      const unsigned b_rn = (unsigned)__builtin_amdgcn_readlane((int)first, 0), b_rf = (unsigned)__builtin_amdgcn_readlane((int)first, 1);
      const unsigned b_cn = (unsigned)__builtin_amdgcn_readlane((int)first, 2), b_cf = (unsigned)__builtin_amdgcn_readlane((int)first, 3);
      if (lane < 40) {
        const unsigned ex = in_row - c;  // the counters in front of this one in its row
        s_cnt[lane] = lane < 8 ? b_rn + ex : lane < 16 ? b_rf + ex - r0 : lane < 24 ? b_cn + ex : lane < 32 ? b_cf + ex - k0 : b_cf + k01 - k0 + ex;
      }
    }
    if (!PIPE || n_waves != 8)
#endif
    if (threadIdx.x == 0) {
      unsigned t[4] = {0u, 0u, 0u, 0u}, b[4];
      for (int k = 0; k < 5; k++)
        for (int w = 0; w < n_waves; w++) t[end_of[k]] += s_cnt[8 * k + w];
      const int row[4] = {RTC_WF_SHADE_COUNT + level, RTC_WF_SHADE_TOP_COUNT + level, level + 1, RTC_WF_TOP_COUNT + level + 1};
      for (int e = 0; e < 4; e++) {
        const unsigned old = t[e] ? atomicAdd(&W.counts[row[e]], t[e]) : 0u;
        const bool fits = (unsigned long long)old + t[e] <= W.cap;
        if (!fits) { W.counts[RTC_WF_OVERFLOW] = 1u; stats->wf_overflow = 1ull; }
        b[e] = (e & 1) ? (fits ? W.cap - old - t[e] : W.cap) : old;
      }
      for (int k = 0; k < 5; k++)
        for (int w = 0; w < n_waves; w++) { const unsigned r = s_cnt[8 * k + w]; s_cnt[8 * k + w] = b[end_of[k]]; b[end_of[k]] += r; }
    }
    __syncthreads();
    const unsigned s = on_plane ? s_cnt[wave] + (unsigned)__popcll(m_rec0 & lt) : s_cnt[8 + wave] + (unsigned)__popcll(m_rec1 & lt);
    const unsigned jr = on_plane ? s_cnt[16 + wave] + (unsigned)__popcll(m_c0 & lt) : s_cnt[24 + wave] + (unsigned)__popcll(m_c1 & lt);
    const unsigned jt = s_cnt[32 + wave] + (unsigned)__popcll(m_c2 & lt);
    if (hit && s < W.cap) {
      double* r = W.sr;
      r[s] = st.px; r[cap + s] = st.py; r[2 * cap + s] = st.pz;
      r[3 * cap + s] = st.nx; r[4 * cap + s] = st.ny; r[5 * cap + s] = st.nz;
      if (mat >= 0) {
        r[6 * cap + s] = cr; r[7 * cap + s] = cg; r[8 * cap + s] = cbl;
        W.sr_mat[s] = mat;
      } else {
        if (!PIPE) shading_row = (int)S.mat[8 * ~mat + 7];
        W.sr_mat[s] = RTC_SR_PLAIN | shading_row;
      }
      W.sr_node[s] = (int32_t)i;
    }
    if (spawn.refl && jr < W.cap) {
      nq[jr] = st.px; nq[cap + jr] = st.py; nq[2 * cap + jr] = st.pz; nq[3 * cap + jr] = st.rx; nq[4 * cap + jr] = st.ry; nq[5 * cap + jr] = st.rz;
      nq[6 * cap + jr] = spawn.wr;
      ch[i] = (int32_t)jr;
      n_reflect++;
    }
    if (spawn.refr && jt < W.cap) {
      nq[jt] = st.ux; nq[cap + jt] = st.uy; nq[2 * cap + jt] = st.uz; nq[3 * cap + jt] = spawn.tdx; nq[4 * cap + jt] = spawn.tdy; nq[5 * cap + jt] = spawn.tdz;
      nq[6 * cap + jt] = spawn.wt;
      ch[cap + i] = (int32_t)jt;
      n_refract++;
    }
  }
  if (COUNT) {
    atomicAdd(&stats->rays_reflect, (unsigned long long)n_reflect);
    atomicAdd(&stats->rays_refract, (unsigned long long)n_refract);
  }
}

// Pixel = the contributions of its ray tree added in the order the one-kernel path adds them (a ray, then its reflected
// subtree, then its refracted subtree: rtc_trace_kernel's depth-first loop), so both paths produce the same bits and a
// pixel's value does not depend on what else was rendered with it.  One lane per level-0 work id walks the child links.
__global__ void __launch_bounds__(256) wf_gather(DCamera cam, DPixelMap pm, DWave W, unsigned n0, double* __restrict__ rgb) {
  const WorkMap wm = make_workmap(pm, cam);
  const size_t cap = W.cap;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n0; i += gridDim.x * blockDim.x) {
    uint64_t q;
    if (!work_to_slot(wm, i, q)) continue;
    double r = 0.0, g = 0.0, b = 0.0;
    int wait_idx[RTC_MAX_FUEL + 1];  // refracted children waiting for their turn; entry k belongs to level wait_lvl[k]
    int wait_lvl[RTC_MAX_FUEL + 1];
    int sp = 0, lvl = 0, idx = (int)i;
    const bool digest = W.dig != nullptr && pm.digest != nullptr;  // parity channel: the same walk sums the rays' hit hashes
    unsigned long long dg = 0ull;
    int kind = 0;
    for (;;) {
      const double* cb = W.contrib + (size_t)lvl * 3 * cap;
      const int32_t* ch = W.child + (size_t)lvl * 2 * cap;
      const int a = ch[idx], c = ch[cap + idx];
      if (a != RTC_WF_MISS) { r += cb[idx]; g += cb[cap + idx]; b += cb[2 * cap + idx]; }  // a miss wrote no contribution
      if (digest) dg += rtc_hit_hash(W.dig[(size_t)lvl * cap + idx], lvl, kind);
      if (c >= 0) { wait_idx[sp] = c; wait_lvl[sp] = lvl + 1; sp++; }
      if (a >= 0) { idx = a; lvl++; kind = 1; continue; }
      if (sp == 0) break;
      sp--;
      idx = wait_idx[sp]; lvl = wait_lvl[sp]; kind = 2;
    }
    rgb[3 * q + 0] = r; rgb[3 * q + 1] = g; rgb[3 * q + 2] = b;
    if (digest) pm.digest[q] = dg;
  }
}


// LDS-resident scene (rtc_device.hpp, LdsScene): bytes of dynamic LDS a block of the LDSC traversal kernel needs, or 0 when the
// scene does not qualify (program not in the kernel arguments, tables + stacks beyond a CU's 160 KB) or `enabled` is false (RTC_WF_LDS=0
// when the scene was created; the emulator, which has no LDSC build).
unsigned rtc_wavefront_lds_bytes(const DScene& S, bool enabled) {
#ifdef RTC_EMU
  enabled = false;
#endif
  return rtc_pick_lds_bytes(RTC_VARIANTS[rtc_variant(S, true)], enabled, rtc_lds_table_bytes(S), S.bvh_stack);
}
// wf_shade build of one level of a frame (the emulator has no UV builds: no entry point of it creates a UV scene)
static RtcWfShadeBuild rtc_scene_shade_build(const DScene& S, bool count, bool level0) {
#ifdef RTC_EMU
  const bool uv = false;
#else
  const bool uv = S.has_uv != 0;
#endif
  return rtc_pick_wf_shade_build(count, uv, S.all_plain != 0, level0);
}

// The dispatch of a launch of scene S, read-only (rtc.h rtc_scene_kernel_info): the same functions the launchers below call.
// lds_bytes: rtc_wavefront_lds_bytes of the scene; big_scene: rtc_big_scene of its device bytes; device: the scene's.
void rtc_kernel_info_fill(const DScene& S, bool wavefront, bool count, bool big_scene, unsigned lds_bytes, int device, rtc_kernel_info* out) {
  const int v = rtc_variant(S, wavefront);
  out->variant = v;
  out->n_kops = S.n_kops; out->n_kplanes = S.n_kplanes; out->n_kaux = 0;
  for (int i = 0; i < S.n_kops; i++) if ((S.kops[i].op == OP_BVH || S.kops[i].op == OP_MESH) && S.kops[i].pad[0] >= 0) out->n_kaux++;
  out->has_recs = S.has_recs; out->all_plain = S.all_plain; out->no_glass_mirror = S.no_glass_mirror;
  out->big_scene = big_scene ? 1 : 0;
  out->n_bvh_nodes = S.n_bvh; out->n_recs = S.n_recs; out->n_mesh_tris = S.n_mtri; out->has_mesh = S.has_mesh; out->bvh_stack = S.bvh_stack;
  out->lds_bytes = wavefront ? lds_bytes : 0u;
  out->lds_refused = 0;
#ifndef RTC_EMU
  // (the one choice that is made at launch time: a device that refuses the LDS size gets the memory build, rtc_launch_wavefront)
  if (wavefront && lds_bytes && rtc_ops(v).wf_ts_lds_refused && rtc_ops(v).wf_ts_lds_refused(device)) out->lds_refused = 1;
#endif
  out->trace_build = out->wf_ts_build = out->wf_shade_build0 = out->wf_shade_build = -1;
  if (wavefront) {
    out->wf_ts_build = rtc_pick_wf_ts_build(count, lds_bytes != 0);
    out->wf_shade_build0 = rtc_scene_shade_build(S, count, true);
    out->wf_shade_build = rtc_scene_shade_build(S, count, false);
  } else {
    out->trace_build = rtc_pick_trace_build(RTC_VARIANTS[v], count, big_scene, S.all_plain != 0, S.no_glass_mirror != 0);
  }
}
// ... and of a scene with a background or a bump table on the one-kernel path (rtc.h rtc_scene_background_info / rtc_scene_bump_info):
// the number of the general row rtc_launch_trace takes, 6 more for a bumped scene with a background.
int rtc_ext_trace_build(const DScene& S, const RtcSceneExt& X) {
  return X.bump ? rtc_pick_np_build(S.has_area != 0, S.has_uv != 0, S.has_spot != 0, X.bg != nullptr) : rtc_pick_bg_build(S.has_area != 0, S.has_uv != 0, S.has_spot != 0);
}
bool rtc_scene_is_big(unsigned long long scene_bytes) { return rtc_big_scene(scene_bytes); }

#ifndef RTC_EMU

// Grid of the wavefront traversal kernel: as many one-wave blocks as the chip holds at once (the kernel hands out chunks
// itself), from the occupancy the runtime reports for this scene's variant and LDS stack size.
unsigned rtc_wavefront_grid(const DScene& S, int n_cu) {
  return (unsigned)std::max(1, n_cu * rtc_ops(rtc_variant(S, true)).wf_ts_blocks_per_cu(rtc_stack_bytes(S)));
}
// ... and of its LDS-resident build: one block per CU, `spare` CUs left out (rtc_pick_wf_ts_lds_grid; spare 0: every CU)
unsigned rtc_wavefront_lds_grid(int n_cu, int spare) { return rtc_pick_wf_ts_lds_grid(n_cu, spare); }
int rtc_wavefront_spare_cus_default(int n_cu) { return rtc_wf_spare_cus_default(n_cu); }
#endif

// work ids of a launch (tile padding included): the minimum DWave.cap
uint64_t rtc_wavefront_work(const DCamera& cam, const DPixelMap& pm) {
  if (pm.mode == 2 && cam.hsize >= 8 && pm.n % cam.hsize == 0) return (uint64_t)((cam.hsize + 7) / 8) * ((pm.n / cam.hsize + 7) / 8) * 64;
  return pm.n;
}

// One frame through the wavefront kernels.  The caller zeroed W.counts (RTC_WF_COUNTS entries) on the stream and sized the
// arrays for W.cap >= the work ids of the launch and fuel + 1 levels; `blocks` / `shade_blocks` = grid sizes of the traversal /
// shading kernels; `lds` = the scene's rtc_wavefront_lds_bytes (0: tables in memory) and `lds_blocks` = the grid of the LDSC traversal build
// (rtc_wavefront_lds_grid; read only when lds != 0), always given together.
// `X`: the scene's background and bump table, each of which may be null.  With a background, wf_background (rtc_background.hip) runs once
// per level, behind that level's trace role.  With a bump table, every level is shaded by wf_shade's NP build (COUNT x UV), whatever
// build the scene takes without.
// The overload without these three is all a caller without LDSC builds can ask for: tables in memory, no background, no bumps.
#ifndef RTC_EMU
void rtc_launch_wf_background(const DScene& S, const DCamera& cam, const DPixelMap& pm, const DWave& W, int level, unsigned n0, const DBackground& bg, unsigned blocks,
                              hipStream_t stream);
#endif
void rtc_launch_wavefront(const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, const DWave& W, double* rgb, double* hit_t, int* hit_prim, int* hit_k,
                          DStats* stats, bool count, hipStream_t stream, unsigned blocks, unsigned shade_blocks, unsigned lds, unsigned lds_blocks, const RtcSceneExt& X) {
  if (pm.n == 0) return;
  const RtcVariantOps& ops = rtc_ops(rtc_variant(S, true));
  const RtcFrame F = {S, cam, pm, hit_t, hit_prim, hit_k, stats, stream, count};
  const unsigned n0 = (unsigned)rtc_wavefront_work(cam, pm);
  const dim3 sgrid(std::max(1u, shade_blocks)), sblock(RTC_WF_SHADE_BLOCK);
  // one level's shading: a build of wf_shade and the scene argument it takes
  auto shade = [&](auto kernel, const auto& scene, int level) { hipLaunchKernelGGL(kernel, sgrid, sblock, 0, stream, scene, cam, pm, W, level, n0, fuel, stats); };
#ifndef RTC_EMU
  DSceneNp N;  // (the NP builds' scene: assembled once per frame, for a scene with a bump table only)
  if (X.bump) N = rtc_widen_scene(S, X);
#endif
  // trace_0; shade_0; [shadow_0 + trace_1]; shade_1; ... [shadow_{fuel-1} + trace_fuel]; shade_fuel; shadow_fuel; sums
  for (int level = 0; level <= fuel + 1; level++) {
    const int tl = level <= fuel ? level : -1, sl = level - 1;
#ifndef RTC_EMU
    // (a device that refuses the LDS size — the opt-in is per device — runs the kernel that reads the tables from memory)
    if (!lds || !ops.launch_wf_ts_lds(F, RtcLevel{W, tl, sl, n0, level, fuel - level, std::max(1u, lds_blocks), lds}))
#endif
    ops.launch_wf_ts(F, RtcLevel{W, tl, sl, n0, level, fuel - level, blocks, 0u});
    if (level > fuel) break;
#ifndef RTC_EMU
    if (X.bg) rtc_launch_wf_background(S, cam, pm, W, level, n0, *X.bg, 4u * std::max(1u, shade_blocks), stream);
    if (X.bump) {
      switch (rtc_pick_wf_shade_np_build(count, S.has_uv != 0)) {
        case RTC_SH_NP_COUNT_UV: shade(wf_shade<true, true, true, false, false, true>, N, level); break;
        case RTC_SH_NP_UV: shade(wf_shade<false, true, true, false, false, true>, N, level); break;
        case RTC_SH_NP_COUNT: shade(wf_shade<true, true, false, false, false, true>, N, level); break;
        case RTC_SH_NP: shade(wf_shade<false, true, false, false, false, true>, N, level); break;
      }
      continue;
    }
#endif
    switch (rtc_scene_shade_build(S, count, level == 0)) {
#ifndef RTC_EMU
      case RTC_SH_COUNT_UV: shade(wf_shade<true, true, true>, S, level); break;
      case RTC_SH_UV: shade(wf_shade<false, true, true>, S, level); break;
#else
      case RTC_SH_COUNT_UV: case RTC_SH_UV: break;  // (never picked here: rtc_scene_shade_build)
#endif
      case RTC_SH_COUNT: shade(wf_shade<true>, S, level); break;
      case RTC_SH_PIPE_LV0: shade(wf_shade<false, false, false, true, true>, S, level); break;
      case RTC_SH_PIPE: shade(wf_shade<false, false, false, true, false>, S, level); break;
      case RTC_SH_PAT: shade(wf_shade<false>, S, level); break;
    }
  }
  hipLaunchKernelGGL(wf_gather, dim3(std::max(1u, std::min(blocks, (n0 + 255u) / 256u))), dim3(256), 0, stream, cam, pm, W, n0, rgb);
}
void rtc_launch_wavefront(const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, const DWave& W, double* rgb, double* hit_t, int* hit_prim, int* hit_k,
                          DStats* stats, bool count, hipStream_t stream, unsigned blocks, unsigned shade_blocks) {
  rtc_launch_wavefront(S, cam, pm, fuel, W, rgb, hit_t, hit_prim, hit_k, stats, count, stream, blocks, shade_blocks, 0u, 0u, RtcSceneExt{nullptr, nullptr});
}

// ---- host-callable launcher (C++ linkage, used by rtc_scene.cpp) ------------------------------------------
// grid of the element-wise kernels below (grid-stride loops over n elements)
static dim3 rtc_elementwise_grid(unsigned long long n) { return dim3((unsigned)std::min<unsigned long long>((n + 255) / 256, 8192)); }
// Color::clamp (src/color.rs:42-46) over a flat array of channel values.
__global__ void __launch_bounds__(256) rtc_quantize_kernel(const double* __restrict__ rgb, unsigned char* __restrict__ out, unsigned long long n) {
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    double x = rgb[i];
    double c = (x != x) ? 1.0 : (x < 1.0 ? x : 1.0);  // x.min(1.0): NaN -> 1.0
    c = c > 0.0 ? c : 0.0;                            // .max(0.0)
    double r = round(c * 255.0);                      // half away from zero
    out[i] = (unsigned char)(r <= 0.0 ? 0.0 : (r >= 255.0 ? 255.0 : r));
  }
}
// The kernels' SoA primary-hit rows -> the C ABI's 16-byte records (include/rtc.h rtc_hit), so that the host copy is one transfer.
__global__ void __launch_bounds__(256) rtc_pack_hits_kernel(const double* __restrict__ t, const int* __restrict__ prim, const int* __restrict__ k, DHit* __restrict__ out, unsigned long long n) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    DHit h;
    h.t = t[i]; h.prim = prim[i]; h.k = k[i];
    out[i] = h;
  }
}
void rtc_launch_pack_hits(const double* t, const int* prim, const int* k, DHit* out, unsigned long long n, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(rtc_pack_hits_kernel, rtc_elementwise_grid(n), dim3(256), 0, stream, t, prim, k, out, n);
}
void rtc_launch_quantize(const double* rgb, unsigned char* out, unsigned long long n, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(rtc_quantize_kernel, rtc_elementwise_grid(n), dim3(256), 0, stream, rgb, out, n);
}


// Multi-GPU gather, last step: image row k + n j  <-  row j of replica k's dense tile in the slab.
// (bands of `band` rows: image row y is row ((y / band) / n) * band + y % band of replica (y / band) % n's tile)
// T = double, or unsigned char for quantised tiles (rtc_render_multi_rgb8: every replica quantises its own rows, so 3 bytes per pixel
// cross xGMI, not 24).
template <typename T>
__global__ void __launch_bounds__(256) rtc_deinterleave_kernel(const T* __restrict__ slab, T* __restrict__ image, unsigned rowlen, unsigned vsize, unsigned n, unsigned max_rows,
                                                               unsigned band) {
  const unsigned long long total = (unsigned long long)vsize * rowlen;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned y = (unsigned)(i / rowlen), x = (unsigned)(i % rowlen);
    const unsigned b = y / band;
    image[i] = slab[((unsigned long long)(b % n) * max_rows + (b / n) * band + y % band) * rowlen + x];
  }
}
template <typename T>
static void launch_deinterleave(const T* slab, T* image, unsigned rowlen, unsigned vsize, unsigned n, unsigned max_rows, unsigned band, hipStream_t stream) {
  const unsigned long long total = (unsigned long long)vsize * rowlen;
  if (total == 0) return;
  hipLaunchKernelGGL(rtc_deinterleave_kernel<T>, rtc_elementwise_grid(total), dim3(256), 0, stream, slab, image, rowlen, vsize, n, max_rows, band ? band : 1u);
}
void rtc_launch_deinterleave8(const unsigned char* slab, unsigned char* image, unsigned rowlen, unsigned vsize, unsigned n, unsigned max_rows, unsigned band, hipStream_t stream) {
  launch_deinterleave(slab, image, rowlen, vsize, n, max_rows, band, stream);
}
void rtc_launch_deinterleave(const double* slab, double* image, unsigned rowlen, unsigned vsize, unsigned n, unsigned max_rows, unsigned band, hipStream_t stream) {
  launch_deinterleave(slab, image, rowlen, vsize, n, max_rows, band, stream);
}

// One-kernel path: one lane per work id (tile padding included).  big_scene: the accelerator does not fit the L2s.  X: the scene's
// background and bump table (each may be null): a scene with either takes that extension of its general row (rtc_general_row).
// (A caller without extended builds -- the emulator -- leaves X out, as it takes the short rtc_launch_wavefront.)
void rtc_launch_trace(const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, double* rgb, double* hit_t, int* hit_prim, int* hit_k,
                      DStats* stats, bool count, hipStream_t stream, bool big_scene, const RtcSceneExt& X = RtcSceneExt{nullptr, nullptr}) {
  if (pm.n == 0) return;
  const unsigned grid = (unsigned)((rtc_wavefront_work(cam, pm) + RTC_BLOCK - 1) / RTC_BLOCK);
  const RtcFrame F = {S, cam, pm, hit_t, hit_prim, hit_k, stats, stream, count};
  const RtcExt e = rtc_ext_of(X);
  if (e == RTC_EXT_NONE) rtc_ops(rtc_variant(S, false)).launch_trace(F, big_scene, grid, fuel, rgb);
  else rtc_ops(rtc_general_row(S.has_area != 0, S.has_uv != 0, S.has_spot != 0)).launch_trace_ext[e](F, X, grid, fuel, rgb);
}

// rtc_kernels.hip — hand-written HIP for gfx950 (MI355X): the kernels of the hot path that do not depend on the scene's feature
// level (wf_shade, wf_gather, the quantiser) and the host-callable launchers.  The ray kernels (rtc_trace_kernel, wf_ts) are
// templates in rtc_device.hpp, instantiated per feature level by rtc_feat.hip (one translation unit per level, built in parallel).
#include <cstdio>
#include <cstdlib>

#include "rtc_device.hpp"

#define RTC_VARIANT_DECL(N)                                                                                                                                   \
  void rtc_launch_trace_v##N(bool count, int waves, unsigned grid, hipStream_t stream, const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, double* rgb, \
                             double* hit_t, int* hit_prim, int* hit_k, DStats* stats);                                                                       \
  void rtc_launch_wf_ts_v##N(bool count, unsigned grid, hipStream_t stream, const DScene& S, const DCamera& cam, const DPixelMap& pm, const DWave& W, int tl, \
                             int sl, unsigned n0, int slot, int fuel_left, double* hit_t, int* hit_prim, int* hit_k, DStats* stats);                         \
  int rtc_wf_ts_blocks_per_cu_v##N(unsigned lds_bytes);                                                                                                        \
  bool rtc_launch_wf_ts_lds_v##N(bool count, unsigned grid, unsigned lds_bytes, hipStream_t stream, const DScene& S, const DCamera& cam, const DPixelMap& pm,   \
                                 const DWave& W, int tl, int sl, unsigned n0, int slot, int fuel_left, double* hit_t, int* hit_prim, int* hit_k, DStats* stats);
RTC_VARIANT_DECL(0) RTC_VARIANT_DECL(1) RTC_VARIANT_DECL(2) RTC_VARIANT_DECL(3) RTC_VARIANT_DECL(4) RTC_VARIANT_DECL(5)
#ifndef RTC_EMU
RTC_VARIANT_DECL(6) RTC_VARIANT_DECL(7)  // area-light scenes (the CPU emulator has no entry point that creates one)
#define RTC_AREA_CASES(call)   \
  case 6: call(6); break;      \
  case 7: call(7); break;
// one-kernel path of scenes with a UV pattern (8; 9 with an area light): the wavefront path keeps the traversal variant and runs the
// UV build of wf_shade
void rtc_launch_trace_v8(bool count, int waves, unsigned grid, hipStream_t stream, const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, double* rgb,
                         double* hit_t, int* hit_prim, int* hit_k, DStats* stats);
void rtc_launch_trace_v9(bool count, int waves, unsigned grid, hipStream_t stream, const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, double* rgb,
                         double* hit_t, int* hit_prim, int* hit_k, DStats* stats);
#define RTC_UV_CASES(call)     \
  case 8: call(8); break;      \
  case 9: call(9); break;
#else
#define RTC_AREA_CASES(call)
#define RTC_UV_CASES(call)
#endif
#undef RTC_VARIANT_DECL
#ifdef RTC_EMU
// the CPU emulator (tests/cpu_emu) compiles everything as one translation unit
#define RTC_VARIANT 0
#include "rtc_feat.hip"
#undef RTC_VARIANT
#define RTC_VARIANT 1
#include "rtc_feat.hip"
#undef RTC_VARIANT
#define RTC_VARIANT 2
#include "rtc_feat.hip"
#undef RTC_VARIANT
#define RTC_VARIANT 3
#include "rtc_feat.hip"
#undef RTC_VARIANT
#define RTC_VARIANT 4
#include "rtc_feat.hip"
#undef RTC_VARIANT
#define RTC_VARIANT 5
#include "rtc_feat.hip"
#undef RTC_VARIANT
#endif

// kernel variant a scene needs (rtc_feat.hip): its feature level (rtc_device.hpp, visit_prim) and where its program lives
static int rtc_variant(const DScene& S) {
  const int feat = S.has_csg ? 3 : (S.has_groups == 2 ? 2 : (S.has_groups ? 1 : 0));
  // scenes with an area light: the AREA builds of the kernel-argument variants 0 / 1, or of the most general one (4) for the rest
  if (S.has_area) return (feat <= 1 && S.n_kops > 0) ? 7 : 6;
  if (feat <= 1 && S.n_kops > 0) return feat;
  if (feat == 2 && S.n_kops > 0) return 5;
  return feat <= 1 ? 2 : feat + 1;
}

#ifndef RTC_WF_SHADE_WAVES
#define RTC_WF_SHADE_WAVES 4  // <= 128 VGPRs: two 512-thread blocks per CU, so one block's wait for its queue atomics is covered by the other
#endif
// PAT = false: every pattern of the scene is a Plain colour (DScene.all_plain): no pattern-tree walk and none of its 672 B of scratch per lane.
// UV: scenes with a texture-mapped pattern (DScene.has_uv): the pattern walk with the RTC_PAT_UV branch (pattern_color_uv).
template <bool COUNT, bool PAT = true>
__global__ void __launch_bounds__(RTC_WF_SHADE_BLOCK, RTC_WF_SHADE_WAVES) wf_shade(DScene S, DCamera cam, DPixelMap pm, DWave W, int level, unsigned n0, int fuel0, DStats* __restrict__ stats) {
  constexpr bool UV = false;
#include "wf_shade_body.inc"
}
template <bool COUNT>
__global__ void __launch_bounds__(RTC_WF_SHADE_BLOCK, RTC_WF_SHADE_WAVES) wf_shade_uv(DScene S, DCamera cam, DPixelMap pm, DWave W, int level, unsigned n0, int fuel0, DStats* __restrict__ stats) {
  constexpr bool PAT = true, UV = true;
#include "wf_shade_body.inc"
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


static void launch_wf_ts(int v, bool count, unsigned grid, hipStream_t stream, const DScene& S, const DCamera& cam, const DPixelMap& pm, const DWave& W, int tl, int sl,
                         unsigned n0, int slot, int fuel_left, double* hit_t, int* hit_prim, int* hit_k, DStats* stats) {
  switch (v) {
    case 0: rtc_launch_wf_ts_v0(count, grid, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats); break;
    case 1: rtc_launch_wf_ts_v1(count, grid, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats); break;
    case 2: rtc_launch_wf_ts_v2(count, grid, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats); break;
    case 3: rtc_launch_wf_ts_v3(count, grid, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats); break;
    case 5: rtc_launch_wf_ts_v5(count, grid, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats); break;
#define RTC_CALL(N) rtc_launch_wf_ts_v##N(count, grid, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats)
    RTC_AREA_CASES(RTC_CALL)
#undef RTC_CALL
    default: rtc_launch_wf_ts_v4(count, grid, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats); break;
  }
}

#ifndef RTC_EMU
// LDS-resident scene (rtc_device.hpp, LdsScene): bytes of dynamic LDS a block of the LDSC traversal kernel needs, or 0 when the
// scene does not qualify (program not in the kernel arguments, tables + stacks beyond a CU's 160 KB) or RTC_WF_LDS=0.
unsigned rtc_wavefront_lds_bytes(const DScene& S) {
  static const bool off = [] { const char* e = std::getenv("RTC_WF_LDS"); return e && e[0] == '0'; }();
  if (off || (rtc_variant(S) > 1 && rtc_variant(S) != 5)) return 0;
  const unsigned long long need = rtc_lds_table_bytes(S) + (unsigned long long)RTC_LDS_BLOCK * (unsigned)S.bvh_stack * sizeof(int);
  return need <= 158ull * 1024 ? (unsigned)need : 0u;
}
static bool launch_wf_ts_lds(int v, bool count, unsigned grid, unsigned lds, hipStream_t stream, const DScene& S, const DCamera& cam, const DPixelMap& pm, const DWave& W, int tl,
                             int sl, unsigned n0, int slot, int fuel_left, double* hit_t, int* hit_prim, int* hit_k, DStats* stats) {
  if (v == 0) return rtc_launch_wf_ts_lds_v0(count, grid, lds, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats);
  if (v == 5) return rtc_launch_wf_ts_lds_v5(count, grid, lds, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats);
  return rtc_launch_wf_ts_lds_v1(count, grid, lds, stream, S, cam, pm, W, tl, sl, n0, slot, fuel_left, hit_t, hit_prim, hit_k, stats);
}

// Grid of the wavefront traversal kernel: as many one-wave blocks as the chip holds at once (the kernel hands out chunks
// itself), from the occupancy the runtime reports for this scene's variant and LDS stack size.
unsigned rtc_wavefront_grid(const DScene& S, int n_cu) {
  const unsigned lds = rtc_stack_bytes(S);
  int per_cu = 8;
  switch (rtc_variant(S)) {
    case 0: per_cu = rtc_wf_ts_blocks_per_cu_v0(lds); break;
    case 1: per_cu = rtc_wf_ts_blocks_per_cu_v1(lds); break;
    case 2: per_cu = rtc_wf_ts_blocks_per_cu_v2(lds); break;
    case 3: per_cu = rtc_wf_ts_blocks_per_cu_v3(lds); break;
    case 5: per_cu = rtc_wf_ts_blocks_per_cu_v5(lds); break;
#define RTC_CALL(N) per_cu = rtc_wf_ts_blocks_per_cu_v##N(lds)
    RTC_AREA_CASES(RTC_CALL)
#undef RTC_CALL
    default: per_cu = rtc_wf_ts_blocks_per_cu_v4(lds); break;
  }
  return (unsigned)std::max(1, n_cu * per_cu);
}
#endif

// work ids of a launch (tile padding included): the minimum DWave.cap
uint64_t rtc_wavefront_work(const DCamera& cam, const DPixelMap& pm) {
  if (pm.mode == 2 && cam.hsize >= 8 && pm.n % cam.hsize == 0) return (uint64_t)((cam.hsize + 7) / 8) * ((pm.n / cam.hsize + 7) / 8) * 64;
  return pm.n;
}

// One frame through the wavefront kernels.  The caller zeroed W.counts (RTC_WF_COUNTS entries) on the stream and sized the
// arrays for W.cap >= the work ids of the launch and fuel + 1 levels; `blocks` / `shade_blocks` = grid sizes of the traversal /
// shading kernels.
void rtc_launch_wavefront(const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, const DWave& W, double* rgb, double* hit_t, int* hit_prim, int* hit_k,
                          DStats* stats, bool count, hipStream_t stream, unsigned blocks, unsigned shade_blocks) {
  if (pm.n == 0) return;
  const int v = rtc_variant(S);
  const unsigned n0 = (unsigned)rtc_wavefront_work(cam, pm);
#ifndef RTC_EMU
  const unsigned lds = rtc_wavefront_lds_bytes(S);
  const unsigned lds_blocks = std::max(1u, shade_blocks / 2u);  // one block per CU (the shading grid is two per CU)
#endif
  const dim3 sgrid(std::max(1u, shade_blocks)), sblock(RTC_WF_SHADE_BLOCK);
  // trace_0; shade_0; [shadow_0 + trace_1]; shade_1; ... [shadow_{fuel-1} + trace_fuel]; shade_fuel; shadow_fuel; sums
  for (int level = 0; level <= fuel + 1; level++) {
    const int tl = level <= fuel ? level : -1, sl = level - 1;
#ifndef RTC_EMU
    // (a device that refuses the LDS size — the opt-in is per device — runs the kernel that reads the tables from memory)
    if (!lds || !launch_wf_ts_lds(v, count, lds_blocks, lds, stream, S, cam, pm, W, tl, sl, n0, level, fuel - level, hit_t, hit_prim, hit_k, stats))
#endif
    launch_wf_ts(v, count, blocks, stream, S, cam, pm, W, tl, sl, n0, level, fuel - level, hit_t, hit_prim, hit_k, stats);
    if (level <= fuel) {
#ifndef RTC_EMU
      if (S.has_uv) {
        if (count) hipLaunchKernelGGL((wf_shade_uv<true>), sgrid, sblock, 0, stream, S, cam, pm, W, level, n0, fuel, stats);
        else hipLaunchKernelGGL((wf_shade_uv<false>), sgrid, sblock, 0, stream, S, cam, pm, W, level, n0, fuel, stats);
        continue;
      }
#endif
      if (count) hipLaunchKernelGGL((wf_shade<true>), sgrid, sblock, 0, stream, S, cam, pm, W, level, n0, fuel, stats);
      else if (S.all_plain) hipLaunchKernelGGL((wf_shade<false, false>), sgrid, sblock, 0, stream, S, cam, pm, W, level, n0, fuel, stats);
      else hipLaunchKernelGGL((wf_shade<false>), sgrid, sblock, 0, stream, S, cam, pm, W, level, n0, fuel, stats);
    }
  }
  hipLaunchKernelGGL(wf_gather, dim3(std::max(1u, std::min(blocks, (n0 + 255u) / 256u))), dim3(256), 0, stream, cam, pm, W, n0, rgb);
}

// ---- host-callable launcher (C++ linkage, used by rtc_scene.cpp) ------------------------------------------
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
  unsigned long long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(rtc_pack_hits_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, t, prim, k, out, n);
}
void rtc_launch_quantize(const double* rgb, unsigned char* out, unsigned long long n, hipStream_t stream) {
  if (n == 0) return;
  unsigned long long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(rtc_quantize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, rgb, out, n);
}


// Multi-GPU gather, last step: image row k + n j  <-  row j of replica k's dense tile in the slab.
// (bands of `band` rows: image row y is row ((y / band) / n) * band + y % band of replica (y / band) % n's tile)
__global__ void __launch_bounds__(256) rtc_deinterleave_kernel(const double* __restrict__ slab, double* __restrict__ image, unsigned rowlen, unsigned vsize, unsigned n,
                                                               unsigned max_rows, unsigned band) {
  const unsigned long long total = (unsigned long long)vsize * rowlen;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned y = (unsigned)(i / rowlen), x = (unsigned)(i % rowlen);
    const unsigned b = y / band;
    image[i] = slab[((unsigned long long)(b % n) * max_rows + (b / n) * band + y % band) * rowlen + x];
  }
}
// The same for quantised tiles (rtc_render_multi_rgb8: every replica quantises its own rows, so 3 bytes per pixel cross xGMI, not 24).
__global__ void __launch_bounds__(256) rtc_deinterleave8_kernel(const unsigned char* __restrict__ slab, unsigned char* __restrict__ image, unsigned rowlen, unsigned vsize,
                                                                unsigned n, unsigned max_rows, unsigned band) {
  const unsigned long long total = (unsigned long long)vsize * rowlen;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned y = (unsigned)(i / rowlen), x = (unsigned)(i % rowlen);
    const unsigned b = y / band;
    image[i] = slab[((unsigned long long)(b % n) * max_rows + (b / n) * band + y % band) * rowlen + x];
  }
}
void rtc_launch_deinterleave8(const unsigned char* slab, unsigned char* image, unsigned rowlen, unsigned vsize, unsigned n, unsigned max_rows, unsigned band, hipStream_t stream) {
  const unsigned long long total = (unsigned long long)vsize * rowlen;
  if (total == 0) return;
  unsigned long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(rtc_deinterleave8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, slab, image, rowlen, vsize, n, max_rows, band ? band : 1u);
}
void rtc_launch_deinterleave(const double* slab, double* image, unsigned rowlen, unsigned vsize, unsigned n, unsigned max_rows, unsigned band, hipStream_t stream) {
  const unsigned long long total = (unsigned long long)vsize * rowlen;
  if (total == 0) return;
  unsigned long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(rtc_deinterleave_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, slab, image, rowlen, vsize, n, max_rows, band ? band : 1u);
}

// One-kernel path: one lane per work id (tile padding included).  big_scene: the accelerator does not fit the L2s.
void rtc_launch_trace(const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, double* rgb, double* hit_t, int* hit_prim, int* hit_k,
                      DStats* stats, bool count, hipStream_t stream, bool big_scene) {
  if (pm.n == 0) return;
  const unsigned grid = (unsigned)((rtc_wavefront_work(cam, pm) + RTC_BLOCK - 1) / RTC_BLOCK);
  const int waves = big_scene ? 3 : 0;
  switch (S.has_uv ? (S.has_area ? 9 : 8) : rtc_variant(S)) {
    case 0: rtc_launch_trace_v0(count, waves, grid, stream, S, cam, pm, fuel, rgb, hit_t, hit_prim, hit_k, stats); break;
    case 1: rtc_launch_trace_v1(count, waves, grid, stream, S, cam, pm, fuel, rgb, hit_t, hit_prim, hit_k, stats); break;
    case 2: rtc_launch_trace_v2(count, waves, grid, stream, S, cam, pm, fuel, rgb, hit_t, hit_prim, hit_k, stats); break;
    case 3: rtc_launch_trace_v3(count, waves, grid, stream, S, cam, pm, fuel, rgb, hit_t, hit_prim, hit_k, stats); break;
    case 5: rtc_launch_trace_v5(count, waves, grid, stream, S, cam, pm, fuel, rgb, hit_t, hit_prim, hit_k, stats); break;
#define RTC_CALL(N) rtc_launch_trace_v##N(count, waves, grid, stream, S, cam, pm, fuel, rgb, hit_t, hit_prim, hit_k, stats)
    RTC_AREA_CASES(RTC_CALL)
    RTC_UV_CASES(RTC_CALL)
#undef RTC_CALL
    default: rtc_launch_trace_v4(count, waves, grid, stream, S, cam, pm, fuel, rgb, hit_t, hit_prim, hit_k, stats); break;
  }
}

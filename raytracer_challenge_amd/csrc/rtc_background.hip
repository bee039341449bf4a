// rtc_background.hip — everything a scene's background (include/rtc.h rtc_background) adds to the device: hand-written HIP for gfx950.
//   without -DRTC_BG_BUILD: wf_background (the wavefront path's kernel for the rays of a level that hit nothing), the kernel behind
//     rtc_background_colors, and the launchers rtc_kernels.hip and rtc_scene.cpp call;
//   with -DRTC_BG_BUILD=<b>: the one-kernel path's BG instantiations of row b of RTC_BG_BUILDS (rtc_device.hpp), plain and counting --
//     one object each, built in parallel like the rows of RTC_VARIANTS (each instantiation is tens of thousands of instructions).
// Scenes without a background launch nothing of this file.
#include "rtc_device.hpp"

#ifdef RTC_BG_BUILD

template <>
void rtc_launch_trace_bg_build<RTC_BG_BUILD>(const RtcFrame& F, const DBackground& bg, unsigned grid, int fuel, double* rgb) {
  constexpr RtcVariant R = RTC_BG_BUILDS[RTC_BG_BUILD];
  DSceneBg S;
  static_cast<DScene&>(S) = F.S;
  S.bg = bg;
  if (F.count)
    hipLaunchKernelGGL((rtc_trace_kernel<true, R.feat, R.kops, 0, false, R.area, R.uv, R.spot, true>), dim3(grid), dim3(RTC_BLOCK), rtc_stack_bytes(F.S), F.stream, S, F.cam, F.pm, fuel,
                       rgb, F.hit_t, F.hit_prim, F.hit_k, F.stats);
  else
    hipLaunchKernelGGL((rtc_trace_kernel<false, R.feat, R.kops, 0, false, R.area, R.uv, R.spot, true>), dim3(grid), dim3(RTC_BLOCK), rtc_stack_bytes(F.S), F.stream, S, F.cam, F.pm, fuel,
                       rgb, F.hit_t, F.hit_prim, F.hit_k, F.stats);
}

#else

uint64_t rtc_wavefront_work(const DCamera& cam, const DPixelMap& pm);  // rtc_kernels.hip

// Wavefront path: once per level of a background scene, after the trace role of wf_ts for that level and before the shading kernel
// that overwrites the level's ray queue.  Ray i of the level whose link says RTC_WF_MISS gets contrib[level][*][i] = weight * B and
// the link -1 ("no children, contribution written"): wf_gather then adds it in the one-kernel path's order, unchanged.  The direction
// and the weight come from where wf_ts took the ray: slot_ray and 1.0 at level 0, the queue's rows 3..6 below that.
// One lane per ray, grid-stride: the link row and the queue rows are SoA, so a wave's reads are whole lines, and only the missing lanes'
// queue lines are touched at all (a wave of hits reads 256 B of links and nothing else).  The misses of a wave are not compacted: a Plain
// root costs a missing lane three loads and three stores, and a pattern walk runs once per missing lane whatever lane it sits in
// (DESIGN.md section 15).
// UV: scenes with DScene.has_uv (the pattern walk with the RTC_PAT_UV branch).
template <bool UV>
__global__ void __launch_bounds__(256) wf_background(DScene S, DCamera cam, DPixelMap pm, DWave W, int level, unsigned n0, DBackground bg) {
  const WorkMap wm = make_workmap(pm, cam);
  const WfParts parts = wf_count(W, level, n0);
  const unsigned count = parts.top + parts.bottom;
  const size_t cap = W.cap;
  int32_t* ch = W.child + (size_t)level * 2 * cap;
  double* cb = W.contrib + (size_t)level * 3 * cap;
  const double* rq = W.rq[level & 1];
  for (unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; w < count; w += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned i = wf_index(parts, W.cap, (unsigned)w);
    double dx, dy, dz, weight = 1.0;
    if (level == 0) {
      uint64_t q = 0;
      if (!work_to_slot(wm, i, q)) continue;  // tile padding: wf_trace_ray never wrote this id's link
      if (ch[i] != RTC_WF_MISS) continue;
      const Ray r = slot_ray(pm, cam, q);
      dx = r.dx; dy = r.dy; dz = r.dz;
    } else {
      if (ch[i] != RTC_WF_MISS) continue;
      dx = rq[3 * cap + i]; dy = rq[4 * cap + i]; dz = rq[5 * cap + i];
      weight = rq[6 * cap + i];
    }
    double r, g, b;
    background_color<UV>(S, bg, dx, dy, dz, r, g, b);
    cb[i] = weight * r; cb[cap + i] = weight * g; cb[2 * cap + i] = weight * b;
    ch[i] = -1;
  }
}

void rtc_launch_wf_background(const DScene& S, const DCamera& cam, const DPixelMap& pm, const DWave& W, int level, unsigned n0, const DBackground& bg, unsigned blocks,
                              hipStream_t stream) {
  // (the level's ray count lives in device memory: the grid covers the queue's capacity at most, a block past the count leaves at once)
  const unsigned long long most = level == 0 ? n0 : W.cap;
  const dim3 grid((unsigned)std::max<unsigned long long>(1ull, std::min<unsigned long long>((most + 255ull) / 256ull, (unsigned long long)std::max(1u, blocks)))), block(256);
  if (S.has_uv) hipLaunchKernelGGL(wf_background<true>, grid, block, 0, stream, S, cam, pm, W, level, n0, bg);
  else hipLaunchKernelGGL(wf_background<false>, grid, block, 0, stream, S, cam, pm, W, level, n0, bg);
}

// The rule alone (rtc.h rtc_background_colors): rgb[i] = the background's colour for direction dirs[i], n x {x, y, z} each.
template <bool UV>
__global__ void __launch_bounds__(256) rtc_background_colors_kernel(DScene S, DBackground bg, const double* __restrict__ dirs, unsigned long long n, double* __restrict__ rgb) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    double r, g, b;
    background_color<UV>(S, bg, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], r, g, b);
    rgb[3 * i] = r; rgb[3 * i + 1] = g; rgb[3 * i + 2] = b;
  }
}
void rtc_launch_background_colors(const DScene& S, const DBackground& bg, const double* dirs, unsigned long long n, double* rgb, hipStream_t stream) {
  if (n == 0) return;
  const dim3 grid((unsigned)std::min<unsigned long long>((n + 255ull) / 256ull, 8192ull)), block(256);
  if (S.has_uv) hipLaunchKernelGGL(rtc_background_colors_kernel<true>, grid, block, 0, stream, S, bg, dirs, n, rgb);
  else hipLaunchKernelGGL(rtc_background_colors_kernel<false>, grid, block, 0, stream, S, bg, dirs, n, rgb);
}

// One-kernel path of a background scene: one lane per work id (tile padding included), as rtc_launch_trace.
void rtc_launch_trace_bg(const DScene& S, const DBackground& bg, const DCamera& cam, const DPixelMap& pm, int fuel, double* rgb, double* hit_t, int* hit_prim, int* hit_k,
                         DStats* stats, bool count, hipStream_t stream) {
  if (pm.n == 0) return;
  const unsigned grid = (unsigned)((rtc_wavefront_work(cam, pm) + RTC_BLOCK - 1) / RTC_BLOCK);
  const RtcFrame F = {S, cam, pm, hit_t, hit_prim, hit_k, stats, stream, count};
  switch (rtc_pick_bg_build(S.has_area != 0, S.has_uv != 0, S.has_spot != 0)) {
    case 0: return rtc_launch_trace_bg_build<0>(F, bg, grid, fuel, rgb);
    case 1: return rtc_launch_trace_bg_build<1>(F, bg, grid, fuel, rgb);
    case 2: return rtc_launch_trace_bg_build<2>(F, bg, grid, fuel, rgb);
    case 3: return rtc_launch_trace_bg_build<3>(F, bg, grid, fuel, rgb);
    case 4: return rtc_launch_trace_bg_build<4>(F, bg, grid, fuel, rgb);
    case 5: return rtc_launch_trace_bg_build<5>(F, bg, grid, fuel, rgb);
  }
}
// What a launch of a background scene takes (rtc.h rtc_scene_background_info): the same selection the launchers above make.
int rtc_background_trace_build(const DScene& S) { return rtc_pick_bg_build(S.has_area != 0, S.has_uv != 0, S.has_spot != 0); }

#endif

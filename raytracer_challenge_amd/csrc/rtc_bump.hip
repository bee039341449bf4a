// rtc_bump.hip — what normal perturbation (include/rtc.h rtc_bump) adds to the device beside wf_shade's NP builds (rtc_kernels.hip):
// hand-written HIP for gfx950.
//   without -DRTC_NP_BUILD: the kernel behind rtc_bump_normals and the launchers rtc_scene.cpp calls;
//   with -DRTC_NP_BUILD=<b>: the one-kernel path's NP instantiations of row b of RTC_NP_BUILDS (rtc_device.hpp), plain and counting --
//     one object each, built in parallel like the rows of RTC_VARIANTS (each instantiation is tens of thousands of instructions).
// Scenes without a bump record launch nothing of this file.
#include "rtc_device.hpp"

#ifdef RTC_NP_BUILD

template <>
void rtc_launch_trace_np_build<RTC_NP_BUILD>(const RtcFrame& F, const DSceneNp& S, unsigned grid, int fuel, double* rgb) {
  constexpr RtcVariant R = RTC_NP_BUILDS[RTC_NP_BUILD];
  constexpr bool BG = rtc_np_build_bg(RTC_NP_BUILD);
  if (F.count)
    hipLaunchKernelGGL((rtc_trace_kernel<true, R.feat, R.kops, 0, false, R.area, R.uv, R.spot, BG, true>), dim3(grid), dim3(RTC_BLOCK), rtc_stack_bytes(F.S), F.stream, S, F.cam, F.pm,
                       fuel, rgb, F.hit_t, F.hit_prim, F.hit_k, F.stats);
  else
    hipLaunchKernelGGL((rtc_trace_kernel<false, R.feat, R.kops, 0, false, R.area, R.uv, R.spot, BG, true>), dim3(grid), dim3(RTC_BLOCK), rtc_stack_bytes(F.S), F.stream, S, F.cam, F.pm,
                       fuel, rgb, F.hit_t, F.hit_prim, F.hit_k, F.stats);
}

#else

uint64_t rtc_wavefront_work(const DCamera& cam, const DPixelMap& pm);  // rtc_kernels.hip

// The rule alone (rtc.h rtc_bump_normals): out[i] = the shading normal (steps 1-4) of a hit at points[i] on primitive prims[i] whose
// geometric normal is normals[i]; a primitive whose material has no record gets its normal back.
// One lane per item, grid-stride.  The inputs and the output are SoA (three rows of n doubles each; the host entry transposes), so a
// wave reads and writes whole lines; the primitive, its matrix and its record are gathers, 16 + 96 + 24 bytes per lane.
__global__ void __launch_bounds__(256) rtc_bump_normals_kernel(DScene S, DBumpTable bt, const int32_t* __restrict__ prims, const double* __restrict__ points,
                                                               const double* __restrict__ normals, unsigned long long n, double* __restrict__ out) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const double nn[3] = {normals[i], normals[n + i], normals[2 * n + i]};
    double o[3] = {nn[0], nn[1], nn[2]};
    const int32_t prim = prims[i];
    if (prim >= 0 && prim < S.n_prims) {  // (the host entry refuses anything else; a lane never reads outside the tables)
      const DPrim P = S.prims[prim];
      const int32_t b = bt.mat_bump[P.mat];
      if (b >= 0) {
        const DBump B = bt.recs[b];
        rtc_bump_normal_at(B.kind, B.octaves, B.amplitude, B.frequency, S.xf_matinv + 16 * P.xform, points[i], points[n + i], points[2 * n + i], nn, o);
      }
    }
    out[i] = o[0]; out[n + i] = o[1]; out[2 * n + i] = o[2];
  }
}
void rtc_launch_bump_normals(const DScene& S, const DBumpTable& bt, const int32_t* prims, const double* points, const double* normals, unsigned long long n, double* out,
                             hipStream_t stream) {
  if (n == 0) return;
  const dim3 grid((unsigned)std::min<unsigned long long>((n + 255ull) / 256ull, 8192ull)), block(256);
  hipLaunchKernelGGL(rtc_bump_normals_kernel, grid, block, 0, stream, S, bt, prims, points, normals, n, out);
}

// What a launch of a bumped scene takes on the one-kernel path (rtc.h rtc_scene_bump_info): the selection the launcher below makes.
int rtc_bump_trace_build(const DScene& S, bool has_bg) { return rtc_pick_np_build(S.has_area != 0, S.has_uv != 0, S.has_spot != 0, has_bg); }

// One-kernel path of a bumped scene: one lane per work id (tile padding included), as rtc_launch_trace.  bg: the scene's background or NULL.
void rtc_launch_trace_np(const DScene& S, const DBumpTable& bt, const DBackground* bg, const DCamera& cam, const DPixelMap& pm, int fuel, double* rgb, double* hit_t,
                         int* hit_prim, int* hit_k, DStats* stats, bool count, hipStream_t stream) {
  if (pm.n == 0) return;
  const unsigned grid = (unsigned)((rtc_wavefront_work(cam, pm) + RTC_BLOCK - 1) / RTC_BLOCK);
  const RtcFrame F = {S, cam, pm, hit_t, hit_prim, hit_k, stats, stream, count};
  DSceneNp N;
  static_cast<DScene&>(N) = S;
  N.bg = bg ? *bg : DBackground{0, 0};
  N.bump = bt;
  switch (rtc_bump_trace_build(S, bg != nullptr)) {
    case 0: return rtc_launch_trace_np_build<0>(F, N, grid, fuel, rgb);
    case 1: return rtc_launch_trace_np_build<1>(F, N, grid, fuel, rgb);
    case 2: return rtc_launch_trace_np_build<2>(F, N, grid, fuel, rgb);
    case 3: return rtc_launch_trace_np_build<3>(F, N, grid, fuel, rgb);
    case 4: return rtc_launch_trace_np_build<4>(F, N, grid, fuel, rgb);
    case 5: return rtc_launch_trace_np_build<5>(F, N, grid, fuel, rgb);
    case 6: return rtc_launch_trace_np_build<6>(F, N, grid, fuel, rgb);
    case 7: return rtc_launch_trace_np_build<7>(F, N, grid, fuel, rgb);
    case 8: return rtc_launch_trace_np_build<8>(F, N, grid, fuel, rgb);
    case 9: return rtc_launch_trace_np_build<9>(F, N, grid, fuel, rgb);
    case 10: return rtc_launch_trace_np_build<10>(F, N, grid, fuel, rgb);
    case 11: return rtc_launch_trace_np_build<11>(F, N, grid, fuel, rgb);
  }
}

#endif

// rtc_feat.hip — the ray kernels of ONE kernel variant: a row of RTC_VARIANTS (rtc_device.hpp), compiled once per row with
// -DRTC_VARIANT=<row>, in parallel: each instantiation of the traversal is tens of thousands of instructions and most of the
// library's build time.  Exports one symbol, rtc_variant_ops<RTC_VARIANT>(): the variant's launchers, for rtc_kernels.hip.
// With -DRTC_EXT=<e> as well (general rows only; RtcExt): the one-kernel path's builds of that row for scenes with a background, a bump
// record or both, an object of their own that exports rtc_launch_trace_ext<RTC_VARIANT, RTC_EXT> and nothing else.
// (The CPU emulator includes this file in rtc_kernels.hip's translation unit and instantiates the rows it uses from there.)
#include "rtc_device.hpp"
#ifndef RTC_EMU
#include <atomic>
#endif

namespace {

// (S: F.S, or its widened form for a kernel that takes one)
template <typename K, typename SceneT>
void launch_trace_kernel(K kernel, const SceneT& S, const RtcFrame& F, unsigned grid, int fuel, double* rgb) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(RTC_BLOCK), rtc_stack_bytes(F.S), F.stream, S, F.cam, F.pm, fuel, rgb, F.hit_t, F.hit_prim, F.hit_k, F.stats);
}
template <typename K>
void launch_wf_ts_kernel(K kernel, unsigned block, unsigned lds_bytes, const RtcFrame& F, const RtcLevel& L) {
  hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(block), lds_bytes, F.stream, F.S, F.cam, F.pm, L.W, L.tl, L.sl, L.n0, L.slot, L.fuel_left, F.hit_t, F.hit_prim, F.hit_k, F.stats);
}

// One-kernel path.  UV-pattern and area-light scenes: one build per counting mode (no 3-wave or lean build).
template <int V>
void launch_trace(const RtcFrame& F, bool big_scene, unsigned grid, int fuel, double* rgb) {
  constexpr RtcVariant R = RTC_VARIANTS[V];
  switch (rtc_pick_trace_build(R, F.count, big_scene, F.S.all_plain != 0, F.S.no_glass_mirror != 0)) {
    case RTC_TB_3WAVE:  // (instantiated for the rows that can be told to take it only)
      if constexpr (rtc_v_trace_3wave(R)) launch_trace_kernel(rtc_trace_kernel<false, R.feat, R.kops, 3>, F.S, F, grid, fuel, rgb);
      return;
    case RTC_TB_LEAN:
      if constexpr (rtc_v_trace_lean(R)) launch_trace_kernel(rtc_trace_kernel<false, R.feat, R.kops, 0, true>, F.S, F, grid, fuel, rgb);
      return;
    case RTC_TB_COUNT: return launch_trace_kernel(rtc_trace_kernel<true, R.feat, R.kops, 0, false, R.area, R.uv, R.spot>, F.S, F, grid, fuel, rgb);
    case RTC_TB_DEFAULT: return launch_trace_kernel(rtc_trace_kernel<false, R.feat, R.kops, 0, false, R.area, R.uv, R.spot>, F.S, F, grid, fuel, rgb);
  }
}

template <int V>
void launch_wf_ts(const RtcFrame& F, const RtcLevel& L) {
  constexpr RtcVariant R = RTC_VARIANTS[V];
  if (rtc_pick_wf_ts_build(F.count, false) == RTC_TS_MEM_COUNT) launch_wf_ts_kernel(wf_ts<true, R.feat, R.kops, false, R.area, R.spot>, RTC_BLOCK, rtc_stack_bytes(F.S), F, L);
  else launch_wf_ts_kernel(wf_ts<false, R.feat, R.kops, false, R.area, R.spot>, RTC_BLOCK, rtc_stack_bytes(F.S), F, L);
}

#ifndef RTC_EMU
// Per device (rtc_multi renders on several from one process), one bit each: the dynamic-LDS attribute of this variant's LDSC kernels was
// raised / was refused.
template <int V>
struct WfLdsState {
  static inline std::atomic<unsigned long long> raised{0ull}, refused{0ull};
};
template <int V>
bool wf_ts_lds_refused(int dev) { return dev >= 0 && dev < 64 && ((WfLdsState<V>::refused.load(std::memory_order_acquire) >> dev) & 1ull) != 0; }

// The same kernel with the scene's accelerator nodes and intersection records copied into LDS by every block (variants with a
// kernel-argument program only: those are the small scenes); one block of RTC_LDS_BLOCK threads per CU, L.lds_bytes of dynamic LDS.
// Returns false when this device refuses the dynamic LDS size (nothing was launched: the caller takes the kernel that reads the tables from memory).
template <int V>
bool launch_wf_ts_lds(const RtcFrame& F, const RtcLevel& L) {
  constexpr RtcVariant R = RTC_VARIANTS[V];
  // More than 64 KB of dynamic LDS has to be asked for, and the attribute belongs to the function object of the CURRENT device:
  // one bit per device in WfLdsState.
  std::atomic<unsigned long long>&raised = WfLdsState<V>::raised, &refused = WfLdsState<V>::refused;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  const unsigned long long bit = 1ull << dev;
  if (refused.load(std::memory_order_acquire) & bit) return false;
  if (!(raised.load(std::memory_order_acquire) & bit)) {
    // (static LDS of the kernel — the RTC_DIAG build has some — comes out of the same 160 KB)
    hipFuncAttributes fa;
    const int st = hipFuncGetAttributes(&fa, (const void*)wf_ts<false, R.feat, R.kops, true>) == hipSuccess ? (int)fa.sharedSizeBytes : 0;
    const hipError_t e1 = hipFuncSetAttribute((const void*)wf_ts<true, R.feat, R.kops, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - st);
    const hipError_t e2 = hipFuncSetAttribute((const void*)wf_ts<false, R.feat, R.kops, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - st);
    if (e1 != hipSuccess || e2 != hipSuccess) {
      (void)hipGetLastError();
      refused.fetch_or(bit, std::memory_order_acq_rel);
      return false;
    }
    raised.fetch_or(bit, std::memory_order_acq_rel);
  }
  if (rtc_pick_wf_ts_build(F.count, true) == RTC_TS_LDS_COUNT) launch_wf_ts_kernel(wf_ts<true, R.feat, R.kops, true>, RTC_LDS_BLOCK, L.lds_bytes, F, L);
  else launch_wf_ts_kernel(wf_ts<false, R.feat, R.kops, true>, RTC_LDS_BLOCK, L.lds_bytes, F, L);
  return true;
}

// resident waves per CU of this variant's traversal kernel (the persistent grid of the wavefront path)
template <int V>
int wf_ts_blocks_per_cu(unsigned lds_bytes) {
  constexpr RtcVariant R = RTC_VARIANTS[V];
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, wf_ts<false, R.feat, R.kops, false, R.area, R.spot>, RTC_BLOCK, lds_bytes) != hipSuccess || nb <= 0) nb = 8;
  return nb;
}
#endif

}  // namespace

template <int V>
RtcVariantOps rtc_variant_ops() {
  constexpr RtcVariant R = RTC_VARIANTS[V];
  RtcVariantOps ops = {launch_trace<V>, nullptr, nullptr, nullptr, nullptr, {nullptr, nullptr, nullptr, nullptr}};
  if constexpr (rtc_v_wavefront(R)) ops.launch_wf_ts = launch_wf_ts<V>;
#ifndef RTC_EMU
  if constexpr (rtc_v_general(R)) {
    ops.launch_trace_ext[RTC_EXT_BG] = rtc_launch_trace_ext<V, RTC_EXT_BG>;
    ops.launch_trace_ext[RTC_EXT_NP] = rtc_launch_trace_ext<V, RTC_EXT_NP>;
    ops.launch_trace_ext[RTC_EXT_NP_BG] = rtc_launch_trace_ext<V, RTC_EXT_NP_BG>;
  }
  if constexpr (rtc_v_lds(R)) { ops.launch_wf_ts_lds = launch_wf_ts_lds<V>; ops.wf_ts_lds_refused = wf_ts_lds_refused<V>; }
  if constexpr (rtc_v_wavefront(R)) ops.wf_ts_blocks_per_cu = wf_ts_blocks_per_cu<V>;
#endif
  return ops;
}

#ifndef RTC_EMU
#ifndef RTC_VARIANT
#error "compile with -DRTC_VARIANT=<a row of RTC_VARIANTS>"
#endif
#ifdef RTC_EXT
// (Defined in the extension's object alone: the row's own object, which takes its address, must not see a body to instantiate.)
template <int V, int E>
void rtc_launch_trace_ext(const RtcFrame& F, const RtcSceneExt& X, unsigned grid, int fuel, double* rgb) {
  constexpr RtcVariant R = RTC_VARIANTS[V];
  static_assert(rtc_v_general(R) && E > RTC_EXT_NONE && E < RTC_N_EXT, "an extension of a general row");
  const DSceneNp S = rtc_widen_scene(F.S, X);
  if (F.count) launch_trace_kernel(rtc_trace_kernel<true, R.feat, R.kops, 0, false, R.area, R.uv, R.spot, rtc_ext_bg(E), rtc_ext_np(E)>, S, F, grid, fuel, rgb);
  else launch_trace_kernel(rtc_trace_kernel<false, R.feat, R.kops, 0, false, R.area, R.uv, R.spot, rtc_ext_bg(E), rtc_ext_np(E)>, S, F, grid, fuel, rgb);
}
template void rtc_launch_trace_ext<RTC_VARIANT, RTC_EXT>(const RtcFrame&, const RtcSceneExt&, unsigned, int, double*);
#else
template RtcVariantOps rtc_variant_ops<RTC_VARIANT>();
#endif
#endif

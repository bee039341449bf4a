// rtc_background.hip — the small kernels a scene's background (include/rtc.h rtc_background) adds to the device, hand-written HIP for
// gfx950: wf_background (the wavefront path's kernel for the rays of a level that hit nothing), the kernel behind rtc_background_colors,
// and their launchers, which rtc_kernels.hip and rtc_scene.cpp call.  (The one-kernel path's BG builds: rtc_feat.hip, RtcExt.)
// Scenes without a background launch nothing of this file.
#include "rtc_device.hpp"

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

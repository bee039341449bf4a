// rtc_filter.hip — the reconstruction filters (include/rtc.h rtc_filter) on gfx950: rtc_resolve_filtered gathers, per output pixel, the
// weighted samples of the (2W + 1)^2 pixels of its window (filter_weights.h's rule) out of a chunk's sample colours.  One thread per
// output pixel, four accumulators; a block owns a TX x TY tile of output pixels (blockDim = (TX, TY), one-dimensional grid of tiles,
// row-major).  Two branches, the same loop (rtc_filter_pixel) and the same bits:
//   LDS: the block first stages the tile and its W-pixel halo -- every sample's (fx, fy) and colour, 40 B -- so that a colour is read
//        from memory once per tile instead of once per output pixel (25 times for a radius-2 window) and the position hash runs once
//        per sample; planes of doubles per k, neighbouring pixels in neighbouring doubles: the 32 lanes of a half-wave read 256
//        consecutive bytes (a ds_read_b64 each) when the tile is 32 wide, two runs of 128 bytes when it is 16 wide.
//   memory: a thread reads its window's colours where the trace left them and hashes each position itself.  Taken when no tile's patch
//        fits the 160 KB of a CU (16 x 16 samples per pixel never do) and for W = 0, where no sample is shared.
// The kernel only WRITES its destination: a chunk that is rendered again after a wavefront queue overflow resolves to the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "filter_weights.h"

namespace {
constexpr unsigned RTC_FILTER_LDS_MAX = 160u * 1024u;  // one CU's
// doubles of one plane of a tile's patch: odd, so that the 5 N planes a staging thread writes to do not fall on one bank
unsigned patch_plane(unsigned tx, unsigned ty, unsigned W) { return ((tx + 2 * W) * (ty + 2 * W)) | 1u; }
unsigned patch_bytes(unsigned tx, unsigned ty, unsigned W, unsigned N) { return 5u * N * patch_plane(tx, ty, W) * (unsigned)sizeof(double); }
}  // namespace

// samples: the colours of the image rows row0 .. row1 - 1 (pixel-major, k inner); dst: the rows out0 .. out1 - 1, which lie inside them
// together with as much of their windows as the image has (the launcher's caller traces the halo).
template <bool LDS>
__global__ void __launch_bounds__(256) rtc_resolve_filtered(rtc_filter f, rtc_sampling sp, unsigned long long hsize, unsigned long long row0, unsigned long long row1,
                                                            unsigned long long out0, unsigned long long out1, unsigned W, const double* __restrict__ samples,
                                                            double* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) double patch[];
  const unsigned N = sp.side * sp.side;
  const unsigned TX = blockDim.x, TY = blockDim.y;
  const unsigned long long tiles_x = (hsize + TX - 1) / TX;
  const unsigned long long tx0 = (blockIdx.x % tiles_x) * TX, ty0 = out0 + (blockIdx.x / tiles_x) * TY;
  const unsigned long long x = tx0 + threadIdx.x, y = ty0 + threadIdx.y;
  const bool live = x < hsize && y < out1;
  uint64_t qx0 = 0, qx1 = 0, qy0 = 0, qy1 = 0;
  if (live) {
    rtc_filter_span(x, W, 0, hsize, &qx0, &qx1);
    rtc_filter_span(y, W, row0, row1 - row0, &qy0, &qy1);
  }
  double out[3];
  if (LDS) {
    // the patch: the windows of the tile's corner pixels, clipped like every window
    const unsigned long long xe = std::min<unsigned long long>(tx0 + TX, hsize) - 1, ye = std::min<unsigned long long>(ty0 + TY, out1) - 1;
    uint64_t px0, px1, py0, py1, unused;
    rtc_filter_span(tx0, W, 0, hsize, &px0, &unused);
    rtc_filter_span(xe, W, 0, hsize, &unused, &px1);
    rtc_filter_span(ty0, W, row0, row1 - row0, &py0, &unused);
    rtc_filter_span(ye, W, row0, row1 - row0, &unused, &py1);
    const unsigned pitch = TX + 2 * W, plane = ((TX + 2 * W) * (TY + 2 * W)) | 1u;
    const unsigned pw = (unsigned)(px1 - px0 + 1), ph = (unsigned)(py1 - py0 + 1), row_samples = pw * N;
    // a patch row's samples are contiguous in memory: consecutive threads take consecutive samples of it
    for (unsigned id = threadIdx.y * TX + threadIdx.x; id < ph * row_samples; id += TX * TY) {
      const unsigned ly = id / row_samples, j = id % row_samples, lx = j / N, k = j % N;
      const unsigned long long qx = px0 + lx, qy = py0 + ly;
      const double* c = samples + 3 * (((qy - row0) * hsize + qx) * (unsigned long long)N + k);
      double fx, fy;
      rtc_sample_offset(sp, qy * hsize + qx, k, &fx, &fy);
      double* o = patch + (size_t)k * plane + ly * pitch + lx;
      const size_t step = (size_t)N * plane;
      o[0] = fx; o[step] = fy; o[2 * step] = c[0]; o[3 * step] = c[1]; o[4 * step] = c[2];
    }
    __syncthreads();
    if (!live) return;
    const rtc_filter_patch_src src{patch, px0, py0, pitch, plane, N};
    rtc_filter_pixel(f, N, x, y, qx0, qx1, qy0, qy1, src, out);
  } else {
    if (!live) return;
    const rtc_filter_mem_src src{samples, hsize, row0, N, sp};
    rtc_filter_pixel(f, N, x, y, qx0, qx1, qy0, qy1, src, out);
  }
  double* o = dst + 3 * ((y - out0) * hsize + x);
  o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

// ---- host-callable launcher (C++ linkage, used by rtc_scene.cpp) ------------------------------------------------------------------
// Queues the filter of the output rows out0 .. out1 - 1 over `samples` = the rows row0 .. row1 - 1.  Returns the dynamic LDS bytes of
// the launch: > 0 = the LDS branch with that patch, 0 = the memory branch; *tile (optional) = TX << 16 | TY.
// Tile choice: of the shapes below, the one whose patch fits a CU's LDS and keeps the most waves resident per CU (16 fill the SIMDs'
// f64 pipes: more do not count), the larger tile -- less halo per pixel -- at equal counts.  RTC_FILTER_LDS=0 forces the memory branch.
unsigned rtc_launch_resolve_filtered(const rtc_filter& f, const rtc_sampling& sp, unsigned long long hsize, unsigned long long row0, unsigned long long row1,
                                     unsigned long long out0, unsigned long long out1, const double* samples, double* dst, hipStream_t stream, unsigned* tile) {
  if (tile) *tile = 0;
  if (out1 <= out0 || hsize == 0) return 0;
  const unsigned W = rtc_filter_window(f.radius), N = sp.side * sp.side;
  static const unsigned shapes[6][2] = {{32, 8}, {16, 16}, {32, 4}, {16, 8}, {32, 2}, {8, 8}};
  unsigned tx = 16, ty = 16, lds = 0, best = 0;
  const char* e = std::getenv("RTC_FILTER_LDS");
  if (W > 0 && !(e && std::atoi(e) == 0)) {
    for (const auto& s : shapes) {
      // (5 N planes of at most 38 x 22 | 1 doubles: the product stays far below 2^32 for N <= 256)
      const unsigned bytes = patch_bytes(s[0], s[1], W, N);
      if (bytes > RTC_FILTER_LDS_MAX) continue;
      const unsigned waves = std::min(16u, (RTC_FILTER_LDS_MAX / bytes) * (s[0] * s[1] / 64u));
      if (waves > best) { best = waves; tx = s[0]; ty = s[1]; lds = bytes; }
    }
  }
  if (lds > 64u * 1024u) {
    // More than 64 KB of dynamic LDS has to be asked for, per device (rtc_feat.hip launch_wf_ts_lds): one bit per device, raised / refused.
    static std::atomic<unsigned long long> raised{0ull}, refused{0ull};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) lds = 0;
    else {
      const unsigned long long bit = 1ull << dev;
      if (refused.load(std::memory_order_acquire) & bit) lds = 0;
      else if (!(raised.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute((const void*)rtc_resolve_filtered<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RTC_FILTER_LDS_MAX) != hipSuccess) {
          (void)hipGetLastError();
          refused.fetch_or(bit, std::memory_order_acq_rel);
          lds = 0;
        } else raised.fetch_or(bit, std::memory_order_acq_rel);
      }
    }
    if (lds == 0) { tx = 16; ty = 16; }  // refused: the memory branch (same bits)
  }
  const unsigned long long tiles = ((hsize + tx - 1) / tx) * ((out1 - out0 + ty - 1) / ty);
  if (tile) *tile = tx << 16 | ty;
  if (lds) hipLaunchKernelGGL(rtc_resolve_filtered<true>, dim3((unsigned)tiles), dim3(tx, ty), lds, stream, f, sp, hsize, row0, row1, out0, out1, W, samples, dst);
  else hipLaunchKernelGGL(rtc_resolve_filtered<false>, dim3((unsigned)tiles), dim3(tx, ty), 0, stream, f, sp, hsize, row0, row1, out0, out1, W, samples, dst);
  return lds;
}

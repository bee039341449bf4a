// rtc_adaptive.hip — adaptive sampling (include/rtc.h rtc_adaptive) on gfx950: which pixels of a frame differ from a neighbour
// (adaptive_contrast.h's rule), their image indices compacted into an ASCENDING list, and the scatter of the refined pixels' means
// back into the frame.  The list's order is arithmetic: flags -> ballot masks and per-block counts, an exclusive scan of the counts,
// positions = block base + earlier waves' popcounts + mbcnt.  No atomic decides a position, no block waits for another.
// Every kernel here takes one-dimensional blocks of RTC_ADAPT_BLOCK threads: lane = threadIdx.x % 64 (wave64), wave = threadIdx.x / 64.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "adaptive_contrast.h"

namespace {
constexpr unsigned RTC_ADAPT_BLOCK = 256;
constexpr unsigned RTC_ADAPT_WAVES = RTC_ADAPT_BLOCK / 64;
}  // namespace

// One thread per pixel (block b: pixels 256 b ..; threads past the frame flag nothing): wave_mask[4 b + w] = the ballot of wave w's 64
// flags, block_count[b] = the block's number of refined pixels.
__global__ void __launch_bounds__(RTC_ADAPT_BLOCK) rtc_contrast_flags(const double* __restrict__ frame, unsigned long long hsize, unsigned long long vsize, double threshold,
                                                                      unsigned neighbours, unsigned long long* __restrict__ wave_mask,
                                                                      unsigned long long* __restrict__ block_count) {
  __shared__ unsigned wave_n[RTC_ADAPT_WAVES];
  const unsigned long long i = (unsigned long long)blockIdx.x * RTC_ADAPT_BLOCK + threadIdx.x;
  const bool flag = i < hsize * vsize && rtc_contrast_refined(frame, hsize, vsize, i, threshold, neighbours);
  const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
  const unsigned w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    wave_mask[(unsigned long long)blockIdx.x * RTC_ADAPT_WAVES + w] = m;
    wave_n[w] = (unsigned)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = (unsigned long long)(wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3]);
}

// One level of the scan: tile b = v[256 b .. 256 b + 255] (entries past m count as 0) becomes its own exclusive prefix sums,
// totals[b] = the tile's sum.  The host scans `totals` the same way, level after level until one tile holds everything, then adds
// the bases back down (rtc_scan_add_base).
__global__ void __launch_bounds__(RTC_ADAPT_BLOCK) rtc_scan_tiles(unsigned long long* __restrict__ v, unsigned long long m, unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long buf[2][RTC_ADAPT_BLOCK];
  const unsigned t = threadIdx.x;
  const unsigned long long i = (unsigned long long)blockIdx.x * RTC_ADAPT_BLOCK + t;
  const unsigned long long own = i < m ? v[i] : 0ull;
  buf[0][t] = own;
  __syncthreads();
  unsigned cur = 0;
  for (unsigned off = 1; off < RTC_ADAPT_BLOCK; off <<= 1) {
    const unsigned long long y = buf[cur][t] + (t >= off ? buf[cur][t - off] : 0ull);
    buf[cur ^ 1u][t] = y;
    __syncthreads();
    cur ^= 1u;
  }
  const unsigned long long inclusive = buf[cur][t];
  if (i < m) v[i] = inclusive - own;
  if (t == RTC_ADAPT_BLOCK - 1) totals[blockIdx.x] = inclusive;
}

// v[i] += base[i / 256]: the finished prefix of tile i / 256 (one level up) onto the tile's own prefixes.
__global__ void __launch_bounds__(RTC_ADAPT_BLOCK) rtc_scan_add_base(unsigned long long* __restrict__ v, unsigned long long m, const unsigned long long* __restrict__ base) {
  const unsigned long long i = (unsigned long long)blockIdx.x * RTC_ADAPT_BLOCK + threadIdx.x;
  if (i < m) v[i] += base[blockIdx.x];
}

// One thread per pixel, the flag kernel's layout: a flagged pixel i goes to out[block_base[b] + refined pixels of the block's earlier
// waves + flagged lanes below its own].  Writes exactly the positions 0 .. total - 1, each once, in ascending pixel order.
__global__ void __launch_bounds__(RTC_ADAPT_BLOCK) rtc_contrast_scatter(const unsigned long long* __restrict__ wave_mask, const unsigned long long* __restrict__ block_base,
                                                                        unsigned long long* __restrict__ out) {
  const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned long long* bm = wave_mask + (unsigned long long)blockIdx.x * RTC_ADAPT_WAVES;
  const unsigned long long m = bm[w];
  unsigned long long pos = block_base[blockIdx.x];
  for (unsigned u = 0; u < w; u++) pos += (unsigned long long)__popcll(bm[u]);
  if ((m >> lane) & 1ull) {
    const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    out[pos + below] = (unsigned long long)blockIdx.x * RTC_ADAPT_BLOCK + threadIdx.x;
  }
}

// rtc_resolve_samples (rtc_camera.hip) with a scattered destination: one thread per (list slot, channel), the k-ordered mean of the
// slot's N ray colours WRITTEN to pixel indices[slot] of the frame (never accumulated: a chunk that is rendered again resolves to the
// same bits; a list holds a pixel once, so no two threads write one value).
__global__ void __launch_bounds__(RTC_ADAPT_BLOCK) rtc_resolve_samples_scatter(const double* __restrict__ ray_rgb, unsigned N, unsigned long long n_slots,
                                                                               const unsigned long long* __restrict__ indices, double* __restrict__ frame) {
  const unsigned long long total = n_slots * 3;
  for (unsigned long long id = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long slot = id / 3;
    const unsigned ch = (unsigned)(id % 3);
    const double* c = ray_rgb + 3 * slot * N + ch;
    double sum = c[0];
    for (unsigned k = 1; k < N; k++) sum = sum + c[3ull * k];
    frame[3 * indices[slot] + ch] = sum / (double)N;
  }
}

// ---- host-callable launchers (C++ linkage, used by rtc_scene.cpp) --------------------------------------------------------------
// Blocks of the flag / scatter kernels for a frame of n pixels, and of one scan level over m entries.
unsigned long long rtc_contrast_blocks(unsigned long long n) { return (n + RTC_ADAPT_BLOCK - 1) / RTC_ADAPT_BLOCK; }

// The exclusive scan of v[0 .. n - 1] in place, for any caller with a table of counts (the compaction below, rtc_shutter.hip's counting
// sort): `levels` = rtc_scan_work_words(n) device words for the tile sums of every level above v, *total = the sum of all of v (one
// device word).  Returns the number of kernels queued.
unsigned long long rtc_scan_work_words(unsigned long long n) {
  unsigned long long m = n, words = 0;
  do { m = rtc_contrast_blocks(m); words += m; } while (m > 1);
  return words;
}
unsigned rtc_launch_scan(unsigned long long* v, unsigned long long n, unsigned long long* levels, unsigned long long* total, hipStream_t stream) {
  unsigned long long* level[18];
  unsigned long long size[17];
  int top = 0;
  level[0] = v; size[0] = n;
  level[1] = levels;
  do { size[top + 1] = rtc_contrast_blocks(size[top]); level[top + 2] = level[top + 1] + size[top + 1]; top++; } while (size[top] > 1);  // 256^8 entries before 16 levels
  unsigned launches = 0;
  // up: level k's tiles scanned in place, their sums = level k + 1; the last level is one word, the total (`total` may be that word's copy)
  for (int k = 0; k < top; k++, launches++)
    hipLaunchKernelGGL(rtc_scan_tiles, dim3((unsigned)size[k + 1]), dim3(RTC_ADAPT_BLOCK), 0, stream, level[k], size[k], k + 1 == top ? total : level[k + 1]);
  // down: level top - 1 is one tile and complete; every level below adds its tile's finished prefix
  for (int k = top - 2; k >= 0; k--, launches++)
    hipLaunchKernelGGL(rtc_scan_add_base, dim3((unsigned)size[k + 1]), dim3(RTC_ADAPT_BLOCK), 0, stream, level[k], size[k], level[k + 1]);
  return launches;
}

// Device words (8 bytes each) rtc_launch_contrast_compact needs in `work` for a frame of n pixels: the wave masks, then the scan's levels.
unsigned long long rtc_contrast_work_words(unsigned long long n) {
  const unsigned long long m = rtc_contrast_blocks(n);
  return m * RTC_ADAPT_WAVES + m + rtc_scan_work_words(m);
}

// Queues the whole detect-and-compact step for the n = hsize * vsize pixels of `frame`: list[0 .. *count - 1] = the refined pixels'
// indices, ascending (list: room for n); count: one device word.  Returns the number of kernels queued.
unsigned rtc_launch_contrast_compact(const double* frame, unsigned long long hsize, unsigned long long vsize, double threshold, unsigned neighbours,
                                     unsigned long long* work, unsigned long long* list, unsigned long long* count, hipStream_t stream) {
  const unsigned long long n = hsize * vsize, nb = rtc_contrast_blocks(n);
  unsigned long long* mask = work;
  unsigned long long* block_count = work + nb * RTC_ADAPT_WAVES;
  hipLaunchKernelGGL(rtc_contrast_flags, dim3((unsigned)nb), dim3(RTC_ADAPT_BLOCK), 0, stream, frame, hsize, vsize, threshold, neighbours, mask, block_count);
  const unsigned scans = rtc_launch_scan(block_count, nb, block_count + nb, count, stream);
  hipLaunchKernelGGL(rtc_contrast_scatter, dim3((unsigned)nb), dim3(RTC_ADAPT_BLOCK), 0, stream, mask, block_count, list);
  return 2 + scans;
}

void rtc_launch_resolve_samples_scatter(const double* ray_rgb, unsigned n_samples, unsigned long long n_slots, const unsigned long long* indices, double* frame,
                                        hipStream_t stream) {
  if (n_slots == 0) return;
  const unsigned grid = (unsigned)std::min<unsigned long long>((n_slots * 3 + RTC_ADAPT_BLOCK - 1) / RTC_ADAPT_BLOCK, 1u << 20);
  hipLaunchKernelGGL(rtc_resolve_samples_scatter, dim3(grid), dim3(RTC_ADAPT_BLOCK), 0, stream, ray_rgb, n_samples, n_slots, indices, frame);
}

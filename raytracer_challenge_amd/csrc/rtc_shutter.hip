// rtc_shutter.hip — the shutter (include/rtc.h rtc_shutter) on gfx950: every sample of a chunk of pixels is dealt to one of K poses
// (shutter_pose.h's rule) and the sample ids are sorted by pose with a counting sort whose order is arithmetic: per wave a ballot per
// distinct pose gives the lanes' ranks and the wave's counts, the blocks' counts go to a POSE-MAJOR table, ONE exclusive scan of that table
// (rtc_adaptive.hip's scan kernels) yields every (pose, block)'s base, positions = base + earlier waves' counts + rank.  No atomic decides a
// position, no block waits for another; the list is ascending within a pose by construction.  Then one small generator launch per pose
// writes that pose's rays (camera_sampling.h's function, its camera in the kernel arguments) into its run of the pose-major ray buffer,
// the scenes' ray kernels trace the runs as explicit rays, and the resolve gathers each pixel's N colours back in k order.
// Every kernel of the dealing takes one-dimensional blocks of RTC_SHUTTER_BLOCK threads: lane = threadIdx.x % 64 (wave64), wave = threadIdx.x / 64.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "camera_sampling.h"
#include "shutter_pose.h"

// rtc_adaptive.hip
unsigned long long rtc_scan_work_words(unsigned long long n);
unsigned rtc_launch_scan(unsigned long long* v, unsigned long long n, unsigned long long* levels, unsigned long long* total, hipStream_t stream);

namespace {
constexpr unsigned RTC_SHUTTER_BLOCK = 256;
constexpr unsigned RTC_SHUTTER_WAVES = RTC_SHUTTER_BLOCK / 64;
dim3 shutter_grid(unsigned long long n) { return dim3((unsigned)std::min<unsigned long long>((n + RTC_SHUTTER_BLOCK - 1) / RTC_SHUTTER_BLOCK, 1u << 20)); }

// What the counting and the placing kernel share, so that they cannot disagree: the pose of this thread's sample id (block b: ids
// 256 b ..; threads past the chunk's M samples are in no pose), its rank among its wave's lanes of that pose, and the wave's count of every
// pose present in it, left in cnt (the block's RTC_SHUTTER_WAVES x RTC_SHUTTER_MAX_POSES table, zeroed here; poses stay below K <= 64).
// The loop is wave-uniform: one turn per distinct pose, the pose read from the lowest remaining lane.  Ends with the block in step.
__device__ __forceinline__ unsigned shutter_wave_ranks(const rtc_shutter& sh, const rtc_sampling& sp, unsigned K, const DPixelMap& pm, const DCamera& cam,
                                                       unsigned long long slot_first, unsigned N, unsigned M, unsigned (*cnt)[RTC_SHUTTER_MAX_POSES], unsigned* pose_out,
                                                       bool* valid_out) {
  const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned long long id = (unsigned long long)blockIdx.x * RTC_SHUTTER_BLOCK + threadIdx.x;
  const bool valid = id < M;
  unsigned pose = 0;
  if (valid) pose = rtc_shutter_pose(sh, sp, K, rtc_slot_pixel(pm, cam, slot_first + id / N), (unsigned)(id % N));
  cnt[w][lane] = 0;  // (RTC_SHUTTER_MAX_POSES == 64: a lane per pose)
  __syncthreads();
  unsigned rank = 0;
  unsigned long long rem = __builtin_amdgcn_ballot_w64(valid);
  while (rem) {
    const unsigned first = (unsigned)__builtin_ctzll(rem);
    const unsigned p = (unsigned)__builtin_amdgcn_readlane((int)pose, (int)first);
    const bool mine = valid && pose == p;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
    if (mine) rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (lane == first) cnt[w][p] = (unsigned)__popcll(m);
    rem &= ~m;
  }
  __syncthreads();
  *pose_out = pose;
  *valid_out = valid;
  return rank;
}
}  // namespace

static_assert(RTC_SHUTTER_MAX_POSES == 64, "the dealing kernels keep one LDS word per pose and lane");

// One thread per sample id of the chunk: count[p * n_blocks + b] = samples of block b dealt to pose p (pose-major, n_blocks = gridDim.x).
__global__ void __launch_bounds__(RTC_SHUTTER_BLOCK) rtc_shutter_count(rtc_shutter sh, rtc_sampling sp, unsigned K, DPixelMap pm, DCamera cam, unsigned long long slot_first,
                                                                       unsigned N, unsigned M, unsigned long long* __restrict__ count) {
  __shared__ unsigned cnt[RTC_SHUTTER_WAVES][RTC_SHUTTER_MAX_POSES];
  unsigned pose;
  bool valid;
  (void)shutter_wave_ranks(sh, sp, K, pm, cam, slot_first, N, M, cnt, &pose, &valid);
  const unsigned t = threadIdx.x;
  if (t < K) count[(unsigned long long)t * gridDim.x + blockIdx.x] = (unsigned long long)(cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t]);
}

// The counting kernel's layout, after the scan turned count into base: sample id goes to position base[p][b] + its pose's count in the
// block's earlier waves + its rank; order[pos] = id, where[id] = pos.  Writes exactly the positions 0 .. M - 1, each once.  Block 0 also
// writes offsets[p] = base[p][0], where pose p's run starts (offsets[K], the total, is the scan's).
__global__ void __launch_bounds__(RTC_SHUTTER_BLOCK) rtc_shutter_place(rtc_shutter sh, rtc_sampling sp, unsigned K, DPixelMap pm, DCamera cam, unsigned long long slot_first,
                                                                       unsigned N, unsigned M, const unsigned long long* __restrict__ base, unsigned* __restrict__ order,
                                                                       unsigned* __restrict__ where, unsigned long long* __restrict__ offsets) {
  __shared__ unsigned cnt[RTC_SHUTTER_WAVES][RTC_SHUTTER_MAX_POSES];
  unsigned pose;
  bool valid;
  const unsigned rank = shutter_wave_ranks(sh, sp, K, pm, cam, slot_first, N, M, cnt, &pose, &valid);
  const unsigned w = threadIdx.x >> 6;
  if (valid) {
    unsigned long long pos = base[(unsigned long long)pose * gridDim.x + blockIdx.x] + rank;
    for (unsigned u = 0; u < w; u++) pos += cnt[u][pose];
    const unsigned id = blockIdx.x * RTC_SHUTTER_BLOCK + threadIdx.x;
    if (pos < M) {  // (always, unless the table was not this chunk's: nothing is written outside the lists)
      order[pos] = id;
      where[id] = (unsigned)pos;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < K) offsets[threadIdx.x] = base[(unsigned long long)threadIdx.x * gridDim.x];
}

// One thread per position j of one pose's run [off, off + len) of the pose-major list: ray j = sample order[j] % N of the pixel of output
// slot slot_first + order[j] / N, through THIS pose's camera.  A wave writes 64 consecutive rays.  M: the chunk's samples; an id at
// or beyond it (never, after a dealing of this chunk) names no slot and is skipped.
__global__ void __launch_bounds__(RTC_SHUTTER_BLOCK) rtc_shutter_gen_rays(DCamera cam, DPixelMap pm, rtc_sampling sp, unsigned long long slot_first,
                                                                          const unsigned* __restrict__ order, unsigned off, unsigned len, unsigned N, unsigned M,
                                                                          double* __restrict__ rays) {
  for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < len; t += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long j = (unsigned long long)off + t;
    const unsigned id = order[j];
    if (id >= M) continue;
    double r[6];
    rtc_sample_ray(cam, sp, rtc_slot_pixel(pm, cam, slot_first + id / N), id % N, r);
    double* o = rays + 6 * j;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4]; o[5] = r[5];
  }
}

// rtc_resolve_samples (rtc_camera.hip) over the pose-major colours: one thread per (pixel slot, channel), sample k's colour found through
// where[], summed in k order, WRITTEN to the destination (never accumulated: a chunk that was traced again resolves to the same bits).
// A position outside the chunk's n_slots * N colours (never, after a dealing of this chunk) is held to the last one: no read leaves the buffer.
__global__ void __launch_bounds__(RTC_SHUTTER_BLOCK) rtc_shutter_resolve(const double* __restrict__ ray_rgb, const unsigned* __restrict__ where, unsigned N,
                                                                         unsigned long long n_slots, double* __restrict__ dst) {
  const unsigned long long total = n_slots * 3;
  const unsigned last = (unsigned)(n_slots * N - 1);
  for (unsigned long long id = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long slot = id / 3;
    const unsigned ch = (unsigned)(id % 3);
    const unsigned* wh = where + slot * N;
    double sum = ray_rgb[3ull * min(wh[0], last) + ch];
    for (unsigned k = 1; k < N; k++) sum = sum + ray_rgb[3ull * min(wh[k], last) + ch];
    dst[id] = sum / (double)N;
  }
}

// ---- host-callable launchers (C++ linkage, used by rtc_scene.cpp) --------------------------------------------------------------
// Blocks of the counting / placing kernels for a chunk of m samples.
unsigned long long rtc_shutter_blocks(unsigned long long m) { return (m + RTC_SHUTTER_BLOCK - 1) / RTC_SHUTTER_BLOCK; }

// Device words (8 bytes each) rtc_launch_shutter_deal needs in `work` for a chunk of m samples, whatever K: the pose-major table, the
// scan's levels above it, the K + 1 offsets.
unsigned long long rtc_shutter_work_words(unsigned long long m) {
  const unsigned long long table = RTC_SHUTTER_MAX_POSES * rtc_shutter_blocks(m);
  return table + rtc_scan_work_words(table) + RTC_SHUTTER_MAX_POSES + 1;
}

// Where the K + 1 offsets of a dealt chunk of m samples are in `work`.
unsigned long long* rtc_shutter_offsets(unsigned long long* work, unsigned long long m) { return work + rtc_shutter_work_words(m) - (RTC_SHUTTER_MAX_POSES + 1); }

// Queues the dealing of the m (1 .. 2^31) samples of the output slots slot_first .. of `pm`: order[0 .. m - 1] = the sample ids pose-major,
// where[id] = an id's position, rtc_shutter_offsets(work, m)[0 .. K] = the runs' starts and the total.  Returns the number of kernels queued.
unsigned rtc_launch_shutter_deal(const rtc_shutter& sh, const rtc_sampling& sp, unsigned K, const DPixelMap& pm, const DCamera& cam, unsigned long long slot_first,
                                 unsigned long long m, unsigned long long* work, unsigned* order, unsigned* where, hipStream_t stream) {
  const unsigned N = sp.side * sp.side;
  const unsigned long long nb = rtc_shutter_blocks(m), table = (unsigned long long)K * nb;
  unsigned long long* levels = work + RTC_SHUTTER_MAX_POSES * nb;
  unsigned long long* offsets = rtc_shutter_offsets(work, m);
  hipLaunchKernelGGL(rtc_shutter_count, dim3((unsigned)nb), dim3(RTC_SHUTTER_BLOCK), 0, stream, sh, sp, K, pm, cam, slot_first, N, (unsigned)m, work);
  const unsigned scans = rtc_launch_scan(work, table, levels, offsets + K, stream);
  hipLaunchKernelGGL(rtc_shutter_place, dim3((unsigned)nb), dim3(RTC_SHUTTER_BLOCK), 0, stream, sh, sp, K, pm, cam, slot_first, N, (unsigned)m, work, order, where, offsets);
  return 2 + scans;
}

void rtc_launch_shutter_gen_rays(const DCamera& cam, const DPixelMap& pm, const rtc_sampling& sp, unsigned long long slot_first, const unsigned* order, unsigned off, unsigned len,
                                 unsigned m, double* rays, hipStream_t stream) {
  if (len == 0) return;
  hipLaunchKernelGGL(rtc_shutter_gen_rays, shutter_grid(len), dim3(RTC_SHUTTER_BLOCK), 0, stream, cam, pm, sp, slot_first, order, off, len, sp.side * sp.side, m, rays);
}

void rtc_launch_shutter_resolve(const double* ray_rgb, const unsigned* where, unsigned n_samples, unsigned long long n_slots, double* dst, hipStream_t stream) {
  if (n_slots == 0) return;
  hipLaunchKernelGGL(rtc_shutter_resolve, shutter_grid(n_slots * 3), dim3(RTC_SHUTTER_BLOCK), 0, stream, ray_rgb, where, n_samples, n_slots, dst);
}

// rtc_camera.hip — the sampled camera (include/rtc.h rtc_sampling) on gfx950: rtc_gen_rays writes every pixel's sample rays into a
// ray buffer the existing kernels trace as explicit rays (DPixelMap mode 3), rtc_resolve_samples averages the rays' colours into the
// pixel.  The ray kernels themselves are untouched: every kernel variant renders sampled frames.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "camera_sampling.h"

namespace {
constexpr unsigned RTC_CAMERA_BLOCK = 256;
dim3 camera_grid(unsigned long long n) { return dim3((unsigned)std::min<unsigned long long>((n + RTC_CAMERA_BLOCK - 1) / RTC_CAMERA_BLOCK, 1u << 20)); }
}  // namespace

// One thread per (pixel slot, k): ray slot * N + k of `rays` (pm.rays' layout) = sample k of the pixel of output slot slot_first + slot
// of the launch `pm` (mode 1 or 2).  A wave writes 64 consecutive rays: 3 KB, contiguous.
__global__ void __launch_bounds__(RTC_CAMERA_BLOCK) rtc_gen_rays(DCamera cam, DPixelMap pm, rtc_sampling sp, unsigned long long slot_first, unsigned long long n_slots,
                                                                 double* __restrict__ rays) {
  const unsigned N = sp.side * sp.side;
  const unsigned long long total = n_slots * N;
  for (unsigned long long id = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long slot = id / N;
    const unsigned k = (unsigned)(id % N);
    double r[6];
    rtc_sample_ray(cam, sp, rtc_slot_pixel(pm, cam, slot_first + slot), k, r);
    double* o = rays + 6 * id;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4]; o[5] = r[5];
  }
}

// One thread per (pixel slot, channel): (((c_0 + c_1) + c_2) + ... + c_{N-1}) / N over the slot's N ray colours, WRITTEN to the
// destination (never accumulated: a chunk that is rendered again after a queue overflow resolves to the same bits).
__global__ void __launch_bounds__(RTC_CAMERA_BLOCK) rtc_resolve_samples(const double* __restrict__ ray_rgb, unsigned N, unsigned long long n_slots, double* __restrict__ dst) {
  const unsigned long long total = n_slots * 3;
  for (unsigned long long id = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long slot = id / 3;
    const unsigned ch = (unsigned)(id % 3);
    const double* c = ray_rgb + 3 * slot * N + ch;
    double sum = c[0];
    for (unsigned k = 1; k < N; k++) sum = sum + c[3ull * k];
    dst[id] = sum / (double)N;
  }
}

// ---- host-callable launchers (C++ linkage, used by rtc_scene.cpp) --------------------------------------------------------------
void rtc_launch_gen_rays(const DCamera& cam, const DPixelMap& pm, const rtc_sampling& sp, unsigned long long slot_first, unsigned long long n_slots, double* rays,
                         hipStream_t stream) {
  if (n_slots == 0) return;
  hipLaunchKernelGGL(rtc_gen_rays, camera_grid(n_slots * sp.side * sp.side), dim3(RTC_CAMERA_BLOCK), 0, stream, cam, pm, sp, slot_first, n_slots, rays);
}
void rtc_launch_resolve_samples(const double* ray_rgb, unsigned n_samples, unsigned long long n_slots, double* dst, hipStream_t stream) {
  if (n_slots == 0) return;
  hipLaunchKernelGGL(rtc_resolve_samples, camera_grid(n_slots * 3), dim3(RTC_CAMERA_BLOCK), 0, stream, ray_rgb, n_samples, n_slots, dst);
}

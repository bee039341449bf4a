// shutter_pose.h — the shutter's rule (include/rtc.h rtc_shutter): which of K poses sample k of image pixel i is traced in.  ONE function,
// compiled for the device (rtc_shutter.hip's counting and placing kernels) and for the host (rtc_shutter_deal without a scene), so the
// two cannot drift.  Integer arithmetic except for the one product u * K of the hashed draw, which is one f64 operation on both sides.
#pragma once
#include "../../include/rtc.h"
#include "device_scene.h"

// Pose of a draw u in [0, 1): floor(u * K), held to K - 1 (u * K may round up to K).
static inline RTC_HD uint32_t rtc_shutter_draw_pose_of(double u, uint32_t K) {
  const double t = u * (double)K;
  const uint32_t s = (uint32_t)t;
  return s < K ? s : K - 1u;
}

// Pose (0 .. K - 1) of sample k (0 .. side * side - 1) of image pixel i.  K >= 1; without RTC_SHUTTER_HASHED also K <= side * side.
static inline RTC_HD uint32_t rtc_shutter_pose(const rtc_shutter& sh, const rtc_sampling& sp, uint32_t K, uint64_t i, uint32_t k) {
  if (!(sh.flags & RTC_SHUTTER_HASHED)) {
    // sequential: the pixel's samples in K runs of floor(N / K) or ceil(N / K)
    const uint32_t N = sp.side * sp.side;
    return (uint32_t)(((uint64_t)k * K) / N);
  }
  // camera_sampling.h's h: nothing of the launch, chunk, device or path; draw 4 follows the lens's 2 and 3
  const unsigned long long h = rtc_splitmix64(rtc_splitmix64(rtc_splitmix64((unsigned long long)sp.seed) ^ (unsigned long long)i) ^ (unsigned long long)k);
  return rtc_shutter_draw_pose_of(rtc_area_jitter(h, 4u), K);
}

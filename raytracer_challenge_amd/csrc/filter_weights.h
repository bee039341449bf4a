// filter_weights.h — the reconstruction filters' rule (include/rtc.h rtc_filter): ONE weight function and ONE pixel loop, compiled for
// the device (rtc_filter.hip's gather kernel, both of its branches) and for the host (rtc_filter_frame without a scene), so they cannot
// drift; -ffp-contract=off holds on both.  Every step is one f64 operation.  Only exp of the Gaussian comes from different libraries
// on the two sides.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/rtc.h"
#include "device_scene.h"

// Sub-pixel position (fx, fy) of sample k of image pixel i: the first lines of rtc_sample_ray (camera_sampling.h), restated.  Factored out
// of rtc_sample_ray it changed the generator kernel's code (scripts/kernel_isa_diff.py: rtc_gen_rays DIFF), so that function stays as it
// is and tests/test_filter_cpu.py pins the two against each other through rtc_camera_rays.
static inline RTC_HD void rtc_sample_offset(const rtc_sampling& sp, uint64_t i, uint32_t k, double* fx, double* fy) {
  const uint32_t n = sp.side;
  const uint32_t sx = k % n, sy = k / n;
  const unsigned long long h = rtc_splitmix64(rtc_splitmix64(rtc_splitmix64((unsigned long long)sp.seed) ^ (unsigned long long)i) ^ (unsigned long long)k);
  double jx = 0.5, jy = 0.5;
  if (sp.flags & RTC_SAMPLE_JITTER) { jx = rtc_area_jitter(h, 0u); jy = rtc_area_jitter(h, 1u); }
  *fx = ((double)sx + jx) / (double)n;
  *fy = ((double)sy + jy) / (double)n;
}

// W: how many pixels beyond its own an output pixel's window reaches, per side and axis.
static inline RTC_HD uint32_t rtc_filter_window(double radius) { return (uint32_t)ceil(radius - 0.5); }

// The pixels lo .. hi (inclusive) of an axis of `size` pixels that lie within W of pixel c and inside [first, first + size).
static inline RTC_HD void rtc_filter_span(uint64_t c, uint32_t W, uint64_t first, uint64_t size, uint64_t* lo, uint64_t* hi) {
  *lo = c >= first + W ? c - W : first;
  *hi = c + W < first + size ? c + W : first + size - 1;
}

// f of one axis: d = the sample's distance from the output pixel's centre, in pixels.
static inline RTC_HD double rtc_filter_f(const rtc_filter& f, double d) {
  const double a = fabs(d), r = f.radius;
  if (!(a < r)) return 0.0;
  if (f.kind == RTC_FILTER_BOX) return 1.0;
  if (f.kind == RTC_FILTER_TENT) return 1.0 - a / r;
  if (f.kind == RTC_FILTER_GAUSSIAN) return exp(-f.alpha * a * a) - exp(-f.alpha * r * r);
  const double t = (a + a) / r;  // Mitchell-Netravali, B = C = 1/3, support stretched from 2 to r
  if (t < 1.0) return ((((7.0 * t - 12.0) * t) * t) + 16.0 / 3.0) / 6.0;
  return ((((-7.0 / 3.0) * t + 12.0) * t - 20.0) * t + 32.0 / 3.0) / 6.0;
}

// Where rtc_filter_pixel takes sample k of image pixel (qx, qy) from: its sub-pixel position and its colour.
// From memory: `rgb` holds the samples of the image rows row0 .. (pixel-major, k inner, rows of hsize pixels); the position is hashed anew.
struct rtc_filter_mem_src {
  const double* rgb;
  uint64_t hsize, row0;
  uint32_t N;
  rtc_sampling sp;
  RTC_HD void offset(uint64_t qx, uint64_t qy, uint32_t k, double* fx, double* fy) const { rtc_sample_offset(sp, qy * hsize + qx, k, fx, fy); }
  RTC_HD void colour(uint64_t qx, uint64_t qy, uint32_t k, double c[3]) const {
    const double* p = rgb + 3 * (((qy - row0) * hsize + qx) * (uint64_t)N + k);
    c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
  }
};
// From a staged patch of pixels (rtc_filter.hip's LDS branch): five planes per k -- fx, fy, r, g, b -- of `plane` doubles each, a
// patch pixel at (qy - y0) * pitch + (qx - x0): the lanes of a wave read neighbouring doubles.
struct rtc_filter_patch_src {
  const double* v;
  uint64_t x0, y0;
  uint32_t pitch, plane, N;
  RTC_HD const double* at(uint64_t qx, uint64_t qy, uint32_t k, uint32_t p) const {
    return v + (size_t)(p * N + k) * plane + (uint32_t)(qy - y0) * pitch + (uint32_t)(qx - x0);
  }
  RTC_HD void offset(uint64_t qx, uint64_t qy, uint32_t k, double* fx, double* fy) const { *fx = *at(qx, qy, k, 0); *fy = *at(qx, qy, k, 1); }
  RTC_HD void colour(uint64_t qx, uint64_t qy, uint32_t k, double c[3]) const { c[0] = *at(qx, qy, k, 2); c[1] = *at(qx, qy, k, 3); c[2] = *at(qx, qy, k, 4); }
};

// Output pixel (x, y) over the window pixels qx0 .. qx1, qy0 .. qy1 (inclusive; rtc_filter_span's), N samples each.
// A sample whose f(dx) is 0.0 has w = 0.0 * f(dy) == 0.0 whatever the finite f(dy) is, and is skipped before f(dy) is evaluated.
template <class Src>
static inline RTC_HD void rtc_filter_pixel(const rtc_filter& f, uint32_t N, uint64_t x, uint64_t y, uint64_t qx0, uint64_t qx1, uint64_t qy0, uint64_t qy1,
                                           const Src& src, double out[3]) {
  double num0 = 0.0, num1 = 0.0, num2 = 0.0, den = 0.0;
  for (uint64_t qy = qy0; qy <= qy1; qy++) {
    const double oy = (double)((int64_t)qy - (int64_t)y);
    for (uint64_t qx = qx0; qx <= qx1; qx++) {
      const double ox = (double)((int64_t)qx - (int64_t)x);
      for (uint32_t k = 0; k < N; k++) {
        double fx, fy;
        src.offset(qx, qy, k, &fx, &fy);
        const double wx = rtc_filter_f(f, ox + (fx - 0.5));
        if (wx == 0.0) continue;
        const double w = wx * rtc_filter_f(f, oy + (fy - 0.5));
        if (w == 0.0) continue;
        double c[3];
        src.colour(qx, qy, k, c);
        num0 = num0 + w * c[0];
        num1 = num1 + w * c[1];
        num2 = num2 + w * c[2];
        den = den + w;
      }
    }
  }
  out[0] = num0 / den; out[1] = num1 / den; out[2] = num2 / den;
}

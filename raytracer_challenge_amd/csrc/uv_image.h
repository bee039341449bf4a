// uv_image.h — the bilinear image-texture lookup (include/rtc.h RTC_UV_IMAGE_LINEAR, _LINEAR_WRAP_U, _LINEAR_WRAP): ONE function,
// compiled for the device (uv_lookup, rtc_device.hpp) and for the host (rtc_texture_sample), so the two cannot drift;
// -ffp-contract=off holds on both.  f64 +, -, *, floor, comparisons and i32 arithmetic: nothing here rounds differently on the two
// sides.
#pragma once
#include <math.h>

#include "device_scene.h"
#include "noise3.h"

// One axis at coordinate a over n texels: the two texel indices and the weight t of the second, in [0, 1].
//   clamped:  texel centres where the nearest rule samples them, a = i / (n - 1); indices clamped to the edge.
//   periodic: n texels per period, centres at (i + 0.5) / n; indices wrap.
// A NaN t (a NaN or infinite a) is 0, and as_i32 saturates: i0 and i1 are in [0, n) whatever a is.
static inline RTC_HD void rtc_uv_axis(double a, int n, bool periodic, int& i0, int& i1, double& t) {
  if (!periodic) {
    const double x = a * (double)(n - 1);
    const double f = floor(x);
    t = x - f;
    i0 = as_i32(f);
    i1 = as_i32(f + 1.0);
    i0 = i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0);
    i1 = i1 < 0 ? 0 : (i1 > n - 1 ? n - 1 : i1);
  } else {
    const double x = a * (double)n - 0.5;
    const double f = floor(x);
    t = x - f;
    i0 = ((as_i32(f) % n) + n) % n;
    i1 = (i0 + 1 == n) ? 0 : i0 + 1;
  }
  if (t != t) t = 0.0;
}

// The record rule of kinds 3..5 at (u, v) on a w x h texture (tex: h rows of w {r, g, b}, row 0 at the top).
// All twelve texel loads are issued before the first arithmetic that depends on one: the four gathers are independent random reads
// and overlap instead of queueing behind each other.  Where the second column follows the first, the two texels of a row are six
// consecutive doubles (48 contiguous, 8-byte-aligned bytes) and are read as one run per row.
static inline RTC_HD void rtc_uv_image_linear(const double* tex, int w, int h, int kind, double u, double v, double rgb[3]) {
  int x0, x1, y0, y1;
  double tx, ty;
  rtc_uv_axis(u, w, kind >= 4, x0, x1, tx);         // RTC_UV_IMAGE_LINEAR_WRAP_U, _LINEAR_WRAP: u periodic
  rtc_uv_axis(1.0 - v, h, kind == 5, y0, y1, ty);   // RTC_UV_IMAGE_LINEAR_WRAP: v periodic too
  const double* r0 = tex + 3 * ((long long)y0 * w);
  const double* r1 = tex + 3 * ((long long)y1 * w);
  double c[12];  // (x0,y0) (x1,y0) (x0,y1) (x1,y1)
  if (x1 == x0 + 1) {
    const double* a = r0 + 3 * x0;
    const double* b = r1 + 3 * x0;
    for (int k = 0; k < 6; k++) c[k] = a[k];
    for (int k = 0; k < 6; k++) c[6 + k] = b[k];
  } else {
    const double *a0 = r0 + 3 * x0, *a1 = r0 + 3 * x1, *b0 = r1 + 3 * x0, *b1 = r1 + 3 * x1;
    for (int k = 0; k < 3; k++) { c[k] = a0[k]; c[3 + k] = a1[k]; c[6 + k] = b0[k]; c[9 + k] = b1[k]; }
  }
  for (int k = 0; k < 3; k++) {
    const double top = c[k] + (c[3 + k] - c[k]) * tx;
    const double bot = c[6 + k] + (c[9 + k] - c[6 + k]) * tx;
    rgb[k] = top + (bot - top) * ty;
  }
}

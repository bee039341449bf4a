// adaptive_contrast.h — adaptive sampling's contrast rule (include/rtc.h rtc_adaptive): ONE function, compiled for the device
// (rtc_adaptive.hip's flag kernel) and for the host (rtc_contrast_pixels without a scene), so the two cannot drift; -ffp-contract=off
// holds on both.  Comparisons, subtractions and fabs only: nothing here rounds differently on the two sides.
#pragma once
#include <math.h>
#include <stdint.h>

#include "device_scene.h"

// What a viewer sees of a channel after Color::clamp; NaN passes through (both comparisons are false).
static inline RTC_HD double rtc_contrast_q(double c) { return c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c); }

// d of two pixels: the maximum over the three channels of |q(a) - q(b)|, taken by d = (e > d) ? e : d from the first channel on: a
// NaN first channel stays NaN, a NaN in a later channel is skipped.
static inline RTC_HD double rtc_contrast_d(const double* a, const double* b) {
  double d = fabs(rtc_contrast_q(a[0]) - rtc_contrast_q(b[0]));
  for (int c = 1; c < 3; c++) {
    const double e = fabs(rtc_contrast_q(a[c]) - rtc_contrast_q(b[c]));
    d = (e > d) ? e : d;
  }
  return d;
}

// Is pixel i of the hsize x vsize frame (rows of {r, g, b}) refined: does some neighbour inside the image have !(d <= threshold)?
// neighbours = 4: (x +- 1, y), (x, y +- 1); 8: the diagonals too.
static inline RTC_HD bool rtc_contrast_refined(const double* frame, uint64_t hsize, uint64_t vsize, uint64_t i, double threshold, uint32_t neighbours) {
  const uint64_t x = i % hsize, y = i / hsize;
  const double* p = frame + 3 * i;
  bool refined = false;
  for (int dy = -1; dy <= 1; dy++) {
    for (int dx = -1; dx <= 1; dx++) {
      if ((dx == 0 && dy == 0) || (neighbours != 8 && dx != 0 && dy != 0)) continue;
      if ((dx < 0 && x == 0) || (dx > 0 && x + 1 == hsize) || (dy < 0 && y == 0) || (dy > 0 && y + 1 == vsize)) continue;
      const uint64_t r = (uint64_t)((int64_t)i + (int64_t)dy * (int64_t)hsize + (int64_t)dx);
      refined = refined || !(rtc_contrast_d(p, frame + 3 * r) <= threshold);
    }
  }
  return refined;
}

// background_point.h — where a ray that hits nothing looks up the scene's background (include/rtc.h rtc_background): ONE function,
// compiled for the device (rtc_trace_kernel's BG build and wf_background, rtc_device.hpp / rtc_background.hip) and for the host
// (rtc_background_point), so the two cannot drift; -ffp-contract=off holds on both.  Comparisons, fabs and three correctly rounded
// divisions: nothing here rounds differently on the two sides.
#pragma once
#include <math.h>

#include "device_scene.h"

// f64::max as Rust defines it (a NaN operand is skipped): what the CUBE uv map's face choice uses (rtc_device.hpp rmax).
static inline RTC_HD double rtc_bg_max(double a, double b) { return (a != a) ? b : ((b != b) ? a : (a > b ? a : b)); }

// projection 0 (RTC_BG_DIRECTION): the direction as it is.  1 (RTC_BG_CUBE): the direction scaled onto the unit cube's surface, where
// RTC_UVMAP_CUBE expects its point: c = max(|dx|, |dy|, |dz|), three divisions.  The zero vector gives 0 / 0 = NaN three times.
static inline RTC_HD void rtc_background_point_at(int projection, double dx, double dy, double dz, double p[3]) {
  if (projection == 1) {
    const double c = rtc_bg_max(rtc_bg_max(fabs(dx), fabs(dy)), fabs(dz));
    p[0] = dx / c; p[1] = dy / c; p[2] = dz / c;
    return;
  }
  p[0] = dx; p[1] = dy; p[2] = dz;
}

// spot_factor.h — a spot light's cone factor (include/rtc.h rtc_light_cone): ONE function, compiled for the device (shade_lights_area's
// SPOT build, rtc_device.hpp) and for the host (rtc_spot_factor, scene creation), so the two cannot drift; -ffp-contract=off holds on
// both.  Additions, multiplications, one division, comparisons -- and the correctly rounded sqrt and / of the host's restatement of the
// shadow ray: nothing here rounds differently on the two sides.
#pragma once
#include <math.h>

#include "device_scene.h"

// c: the cosine between the cone's unit axis a and the direction from the light to the shading point, -d of the shadow ray (d points
// from the point to the light).
static inline RTC_HD double rtc_spot_cos(double dx, double dy, double dz, double ax, double ay, double az) { return ((-dx) * ax + (-dy) * ay) + (-dz) * az; }

// f of c: 1 inside the inner cone, 0 outside the outer one, smoothstep between; the tests in this order, so cos_inner == cos_outer is a
// hard edge and never divides by zero.  A NaN c fails both tests and comes back as NaN.
static inline RTC_HD double rtc_spot_f(double c, double cos_inner, double cos_outer) {
  if (c >= cos_inner) return 1.0;
  if (c <= cos_outer) return 0.0;
  const double t = (c - cos_outer) / (cos_inner - cos_outer);
  return (t * t) * (3.0 - 2.0 * t);
}

// The unit axis a scene keeps: Vector::normalize's order.
static inline RTC_HD void rtc_spot_axis(const double axis[3], double a[3]) {
  const double m = sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
  a[0] = axis[0] / m; a[1] = axis[1] / m; a[2] = axis[2] / m;
}

// The whole rule for a light (sample) at l and a shading point o (the over_point), with the scene's unit axis: the direction is
// shadow_ray()'s (rtc_device.hpp), restated for the host.
static inline RTC_HD double rtc_spot_factor_at(const double a[3], double cos_inner, double cos_outer, const double l[3], const double o[3]) {
  const double vx = l[0] - o[0], vy = l[1] - o[1], vz = l[2] - o[2];
  const double dist = sqrt(vx * vx + vy * vy + vz * vz);
  return rtc_spot_f(rtc_spot_cos(vx / dist, vy / dist, vz / dist, a[0], a[1], a[2]), cos_inner, cos_outer);
}

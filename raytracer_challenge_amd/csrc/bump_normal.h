// bump_normal.h — the shading normal of a hit on a material with a bump record (include/rtc.h rtc_bump, steps 1-4): ONE function,
// compiled for the device (prepare_state's NP build and the kernel behind rtc_bump_normals, rtc_device.hpp / rtc_bump.hip) and for the
// host (rtc_bump_normal), so the two cannot drift; -ffp-contract=off holds on both.  The noise is noise3.h's; beside it there are f64
// +, -, *, /, sqrt and floor, all correctly rounded on both sides: nothing here rounds differently on the two.
#pragma once
#include <math.h>

#include "device_scene.h"
#include "noise3.h"

// kind / octaves / a / f: the record.  m: the primitive's material_inv, row-major, rows 0..2 read.  (x, y, z): the hit point.
// n: the unit world normal before the inside flip.  out: the shading normal, before the flip too.
static inline RTC_HD void rtc_bump_normal_at(int kind, unsigned octaves, double a, double f, const double* m, double x, double y, double z, const double n[3],
                                             double out[3]) {
  // 1. material space (pattern_at's rows), then the record's frequency
  const double qx = m[0] * x + m[1] * y + m[2] * z + m[3] * 1.0;
  const double qy = m[4] * x + m[5] * y + m[6] * z + m[7] * 1.0;
  const double qz = m[8] * x + m[9] * y + m[10] * z + m[11] * 1.0;
  const double sx = qx * f, sy = qy * f, sz = qz * f;
  // 2. the slope d, in material space
  double dx, dy, dz;
  if (kind == 0) {  // RTC_BUMP_SIMPLEX: jitter_3d's three offsets
    dx = simplex3(sx, sy, sz);
    dy = simplex3(sx, sy, sz + 1.0);
    dz = simplex3(sx, sy, sz + 2.0);
  } else if (kind == 1) {  // RTC_BUMP_FRACTAL
    dx = fractal3(sx, sy, sz, octaves);
    dy = fractal3(sx, sy, sz + 1.0, octaves);
    dz = fractal3(sx, sy, sz + 2.0, octaves);
  } else {  // RTC_BUMP_RIPPLE: rings about the y axis, a triangle wave as the slope
    const double r = sqrt(sx * sx + sz * sz);
    if (r == 0.0) {
      dx = 0.0; dy = 0.0; dz = 0.0;
    } else {
      const double g = 2.0 * (r - floor(r));
      const double w = (g < 1.0) ? 1.0 - 2.0 * g : 2.0 * g - 3.0;
      dx = (sx / r) * w; dy = 0.0; dz = (sz / r) * w;
    }
  }
  // 3. to world space as a gradient goes: by the transpose of the 3x3
  const double gx = (m[0] * dx + m[4] * dy) + m[8] * dz;
  const double gy = (m[1] * dx + m[5] * dy) + m[9] * dz;
  const double gz = (m[2] * dx + m[6] * dy) + m[10] * dz;
  // 4. v = n + a g; an unmoved normal keeps its bits
  const double vx = n[0] + a * gx, vy = n[1] + a * gy, vz = n[2] + a * gz;
  if (vx == n[0] && vy == n[1] && vz == n[2]) { out[0] = n[0]; out[1] = n[1]; out[2] = n[2]; return; }
  const double mag = sqrt(vx * vx + vy * vy + vz * vz);
  out[0] = vx / mag; out[1] = vy / mag; out[2] = vz / mag;
}

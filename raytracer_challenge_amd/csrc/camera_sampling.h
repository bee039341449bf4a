// camera_sampling.h — the sampled camera's rule (include/rtc.h rtc_sampling): ONE function, compiled for the device (rtc_camera.hip's
// generator kernel) and for the host (rtc_camera_rays without a scene), so the two cannot drift; -ffp-contract=off holds on both.
// Every step is one f64 operation.  Only cos / sin of the thin lens come from different libraries on the two sides.
#pragma once
#include <math.h>

#include "../../include/rtc.h"
#include "device_scene.h"

// Image pixel of output slot q of a launch over an index list (mode 1) or bands / interleaved rows (mode 2): rtc_device.hpp slot_ray's
// arithmetic.
static inline RTC_HD uint64_t rtc_slot_pixel(const DPixelMap& pm, const DCamera& cam, uint64_t q) {
  if (pm.mode == 1) return pm.indices[q];
  const uint64_t j = q / cam.hsize, band = pm.band ? pm.band : 1u;
  return (((uint64_t)pm.row_first + (j / band) * pm.row_step) * band + j % band) * cam.hsize + (q % cam.hsize);
}

// Ray of sample k (0 .. side * side - 1) of image pixel i: out = {o, d}.
static inline RTC_HD void rtc_sample_ray(const DCamera& cam, const rtc_sampling& sp, uint64_t i, uint32_t k, double out[6]) {
  const uint32_t n = sp.side;
  const uint64_t x = i % cam.hsize, y = i / cam.hsize;
  const uint32_t sx = k % n, sy = k / n;
  // nothing of the launch, chunk, device or path: any partition of the image draws the same bits
  const unsigned long long h = rtc_splitmix64(rtc_splitmix64(rtc_splitmix64((unsigned long long)sp.seed) ^ (unsigned long long)i) ^ (unsigned long long)k);
  double jx = 0.5, jy = 0.5;
  if (sp.flags & RTC_SAMPLE_JITTER) { jx = rtc_area_jitter(h, 0u); jy = rtc_area_jitter(h, 1u); }  // stratified: one sample per cell
  const double fx = ((double)sx + jx) / (double)n;
  const double fy = ((double)sy + jy) / (double)n;
  const double xoffset = ((double)x + fx) * cam.pixel_size;
  const double yoffset = ((double)y + fy) * cam.pixel_size;
  const double world_x = cam.half_width - xoffset;
  const double world_y = cam.half_height - yoffset;
  const double* m = cam.inv;
  double ox, oy, oz, px, py, pz;
  if (!(sp.lens_radius > 0.0)) {
    // pinhole: Camera::ray_at_pixel (src/camera.rs:39-55) from here on, as rtc_device.hpp camera_ray has it
    px = m[0] * world_x + m[1] * world_y + m[2] * -1.0 + m[3] * 1.0;
    py = m[4] * world_x + m[5] * world_y + m[6] * -1.0 + m[7] * 1.0;
    pz = m[8] * world_x + m[9] * world_y + m[10] * -1.0 + m[11] * 1.0;
    ox = m[3]; oy = m[7]; oz = m[11];
  } else {
    // thin lens: a point of the lens disc (concentric map of two draws) towards the pixel's point of the plane at depth F
    const double R = sp.lens_radius, F = sp.focal_distance;
    const double a = 2.0 * rtc_area_jitter(h, 2u) - 1.0, b = 2.0 * rtc_area_jitter(h, 3u) - 1.0;
    double lx = 0.0, ly = 0.0;
    if (!(a == 0.0 && b == 0.0)) {
      double r, phi;
      if (fabs(a) > fabs(b)) { r = a; phi = (M_PI / 4.0) * (b / a); }
      else { r = b; phi = M_PI / 2.0 - (M_PI / 4.0) * (a / b); }
      lx = (R * r) * cos(phi);
      ly = (R * r) * sin(phi);
    }
    ox = m[0] * lx + m[1] * ly + m[2] * 0.0 + m[3] * 1.0;
    oy = m[4] * lx + m[5] * ly + m[6] * 0.0 + m[7] * 1.0;
    oz = m[8] * lx + m[9] * ly + m[10] * 0.0 + m[11] * 1.0;
    const double tx = world_x * F, ty = world_y * F, tz = -F;
    px = m[0] * tx + m[1] * ty + m[2] * tz + m[3] * 1.0;
    py = m[4] * tx + m[5] * ty + m[6] * tz + m[7] * 1.0;
    pz = m[8] * tx + m[9] * ty + m[10] * tz + m[11] * 1.0;
  }
  const double dx = px - ox, dy = py - oy, dz = pz - oz;
  const double mag = sqrt(dx * dx + dy * dy + dz * dz);
  out[0] = ox; out[1] = oy; out[2] = oz;
  out[3] = dx / mag; out[4] = dy / mag; out[5] = dz / mag;
}

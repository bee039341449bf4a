// noise3.h — the reference's noise (src/noise.rs): ONE copy of simplex3 / fractal3 and their helpers, compiled for the device (the
// pattern walk's jitters and the bump rule, rtc_device.hpp) and for the host (rtc_bump_normal, rtc_scene.cpp), so the two cannot drift;
// -ffp-contract=off holds on both.  Integer arithmetic, comparisons, f64 +, -, * and one division: nothing here rounds differently on
// the two sides.  The device functions keep the names, the linkage names and the code they had inside rtc_device.hpp
// (profiles/bump_isa_diff.txt).
#pragma once
#include "device_scene.h"

#if defined(__HIPCC__) || defined(RTC_EMU)
#define RTC_NOISE_FI RTC_HD __forceinline__
#define RTC_NOISE_NI inline RTC_HD __noinline__
#else
#define RTC_NOISE_FI static inline
#define RTC_NOISE_NI static inline
#endif

#define RTC_NOISE_PERM                                                                                                                  \
  {151, 160, 137, 91,  90,  15,  131, 13,  201, 95,  96,  53,  194, 233, 7,   225, 140, 36,  103, 30,  69,  142, 8,   99,  37,  240, \
   21,  10,  23,  190, 6,   148, 247, 120, 234, 75,  0,   26,  197, 62,  94,  252, 219, 203, 117, 35,  11,  32,  57,  177, 33,  88,  \
   237, 149, 56,  87,  174, 20,  125, 136, 171, 168, 68,  175, 74,  165, 71,  134, 139, 48,  27,  166, 77,  146, 158, 231, 83,  111, \
   229, 122, 60,  211, 133, 230, 220, 105, 92,  41,  55,  46,  245, 40,  244, 102, 143, 54,  65,  25,  63,  161, 1,   216, 80,  73,  \
   209, 76,  132, 187, 208, 89,  18,  169, 200, 196, 135, 130, 116, 188, 159, 86,  164, 100, 109, 198, 173, 186, 3,   64,  52,  217, \
   226, 250, 124, 123, 5,   202, 38,  147, 118, 126, 255, 82,  85,  212, 207, 206, 59,  227, 47,  16,  58,  17,  182, 189, 28,  42,  \
   223, 183, 170, 213, 119, 248, 152, 2,   44,  154, 163, 70,  221, 153, 101, 155, 167, 43,  172, 9,   129, 22,  39,  253, 19,  98,  \
   108, 110, 79,  113, 224, 232, 178, 185, 112, 104, 218, 246, 97,  228, 251, 34,  242, 193, 238, 210, 144, 12,  191, 179, 162, 241, \
   81,  51,  145, 235, 249, 14,  239, 107, 49,  192, 214, 31,  181, 199, 106, 157, 184, 84,  204, 176, 115, 121, 50,  45,  127, 4,   \
   150, 254, 138, 236, 205, 93,  222, 114, 67,  29,  24,  72,  243, 141, 128, 195, 78,  66,  215, 61,  156, 180}

// ---- noise (src/noise.rs) ------------------------------------------------------------------------------
#if defined(__HIPCC__) || defined(RTC_EMU)
__device__ const unsigned char PERM[256] = RTC_NOISE_PERM;
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
static const unsigned char PERM_HOST[256] = RTC_NOISE_PERM;  // the host's copy of the same 256 numbers
#endif

RTC_NOISE_FI unsigned nhash(unsigned i) {  // :90-92, table period 256
#if defined(__HIP_DEVICE_COMPILE__)
  return PERM[i & 255u];
#else
  return PERM_HOST[i & 255u];
#endif
}

RTC_NOISE_FI int as_i32(double x) {  // Rust `as i32`: saturating, NaN -> 0
  if (x != x) return 0;
  if (x >= 2147483647.0) return 2147483647;
  if (x <= -2147483648.0) return (int)0x80000000;
  return (int)x;
}
RTC_NOISE_FI int wadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
RTC_NOISE_FI int fast_floor(double x) { return x > 0.0 ? as_i32(x) : (int)((unsigned)as_i32(x) - 1u); }  // :116-122
RTC_NOISE_FI unsigned modulus256(int x) { int a = x % 256; return a < 0 ? (unsigned)(a + 256) : (unsigned)a; }  // :124-131

RTC_NOISE_FI double ngrad(unsigned h, double x, double y, double z) {  // :94-114
  switch (h & 0xF) {
    case 0x0: return x + y;
    case 0x1: return -x + y;
    case 0x2: return x - y;
    case 0x3: return -x - y;
    case 0x4: return x + z;
    case 0x5: return -x + z;
    case 0x6: return x - z;
    case 0x7: return -x - z;
    case 0x8: return y + z;
    case 0x9: return -y + z;
    case 0xA: return y - z;
    case 0xB: return -y - z;
    case 0xC: return y + x;
    case 0xD: return -y + z;
    case 0xE: return y - x;
    default: return -y - z;
  }
}

RTC_NOISE_NI double simplex3(double x, double y, double z) {  // :134-219
  const double F3 = 1.0 / 3.0, G3 = 1.0 / 6.0;
  double s = (x + y + z) * F3;
  int i = fast_floor(x + s), j = fast_floor(y + s), k = fast_floor(z + s);
  double t = (double)wadd(wadd(i, j), k) * G3;
  double x0 = x - ((double)i - t), y0 = y - ((double)j - t), z0 = z - ((double)k - t);
  int i1, j1, k1, i2, j2, k2;
  if (x0 >= y0) {
    if (y0 >= z0) { i1 = 1; j1 = 0; k1 = 0; i2 = 1; j2 = 1; k2 = 0; }
    else if (x0 >= z0) { i1 = 1; j1 = 0; k1 = 0; i2 = 1; j2 = 0; k2 = 1; }
    else { i1 = 0; j1 = 0; k1 = 1; i2 = 1; j2 = 0; k2 = 1; }
  } else {
    if (y0 < z0) { i1 = 0; j1 = 0; k1 = 1; i2 = 0; j2 = 1; k2 = 1; }
    else if (x0 < z0) { i1 = 0; j1 = 1; k1 = 0; i2 = 0; j2 = 1; k2 = 1; }
    else { i1 = 0; j1 = 1; k1 = 0; i2 = 1; j2 = 1; k2 = 0; }
  }
  double x1 = x0 - (double)i1 + G3, y1 = y0 - (double)j1 + G3, z1 = z0 - (double)k1 + G3;
  double x2 = x0 - (double)i2 + 2.0 * G3, y2 = y0 - (double)j2 + 2.0 * G3, z2 = z0 - (double)k2 + 2.0 * G3;
  double x3 = x0 - 1.0 + 3.0 * G3, y3 = y0 - 1.0 + 3.0 * G3, z3 = z0 - 1.0 + 3.0 * G3;
  unsigned ii = modulus256(i), jj = modulus256(j), kk = modulus256(k);
  unsigned gi0 = nhash(ii + nhash(jj + nhash(kk)));
  unsigned gi1 = nhash(ii + i1 + nhash(jj + j1 + nhash(kk + k1)));
  unsigned gi2 = nhash(ii + i2 + nhash(jj + j2 + nhash(kk + k2)));
  unsigned gi3 = nhash(ii + 1 + nhash(jj + 1 + nhash(kk + 1)));
  double n0, n1, n2, n3;
  double t0 = 0.6 - x0 * x0 - y0 * y0 - z0 * z0;
  if (t0 < 0.0) n0 = 0.0; else { t0 *= t0; n0 = t0 * t0 * ngrad(gi0, x0, y0, z0); }
  double t1 = 0.6 - x1 * x1 - y1 * y1 - z1 * z1;
  if (t1 < 0.0) n1 = 0.0; else { t1 *= t1; n1 = t1 * t1 * ngrad(gi1, x1, y1, z1); }
  double t2 = 0.6 - x2 * x2 - y2 * y2 - z2 * z2;
  if (t2 < 0.0) n2 = 0.0; else { t2 *= t2; n2 = t2 * t2 * ngrad(gi2, x2, y2, z2); }
  double t3 = 0.6 - x3 * x3 - y3 * y3 - z3 * z3;
  if (t3 < 0.0) n3 = 0.0; else { t3 *= t3; n3 = t3 * t3 * ngrad(gi3, x3, y3, z3); }
  return 32.0 * (n0 + n1 + n2 + n3);
}

RTC_NOISE_FI double fractal3(double x, double y, double z, unsigned octaves) {  // :221-237
  double output = 0.0, denom = 0.0, frequency = 1.0, amplitude = 1.0;
  for (unsigned o = 0; o < octaves; o++) {
    output += amplitude * simplex3(x * frequency, y * frequency, z * frequency);
    denom += amplitude;
    frequency *= 2.0;
    amplitude *= 0.5;
  }
  return output / denom;
}

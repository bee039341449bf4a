// =============================================================================
// oracle/rt_oracle.hpp — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// CPU restatement (C++17, f64, no FMA contraction: build with -ffp-contract=off)
// of the reference's per-pixel `Image::par_render -> World::color_at` path and
// of the scene-construction semantics that feed it.  Every function cites the
// reference file:line it follows (paths relative to the reference crate root).
//
// Who may use this file: tests/, __graft_entry__.smoke() and the cpu_baseline
// leg of bench.py — as the checker / reported baseline only.  Nothing under
// raytracer_challenge_amd/ includes, links or loads anything from oracle/.
//
// Parity pin: oracle/known_answers.cpp ports the reference's own unit-test
// values and tests/golden/*.json holds sampled pixels of the
// reference's committed renders; tests/test_oracle_*.py check both.
// Unpinned by any reference fixture: Noise::Fractal and JitterKind::Color
// ("parity unpinned" — restated from src/noise.rs:221-237, src/material.rs:209-217).
// =============================================================================
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <fstream>
#include <sstream>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#if defined(ORC_EXT) && !defined(ORC_EXT_MUTANT)
#define ORC_EXT_MUTANT 0
#endif

namespace orc {

// src/config.rs:1-2
constexpr double EPSILON = 0.00001;
constexpr int FUEL = 5;
constexpr double INF = std::numeric_limits<double>::infinity();

// src/approx.rs:19-23
inline bool approx(double a, double b) { return std::fabs(a - b) < EPSILON; }

// Rust f64::max / f64::min: a NaN operand is ignored (IEEE maxNum/minNum).
inline double rmax(double a, double b) {
  if (a != a) return b;
  if (b != b) return a;
  return a > b ? a : b;
}
inline double rmin(double a, double b) {
  if (a != a) return b;
  if (b != b) return a;
  return a < b ? a : b;
}
// Rust `x as i32`: saturating, NaN -> 0.
inline int32_t as_i32(double x) {
  if (x != x) return 0;
  if (x >= 2147483647.0) return INT32_MAX;
  if (x <= -2147483648.0) return INT32_MIN;
  return (int32_t)x;
}
inline int32_t wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
inline int32_t wrap_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

// ---------------------------------------------------------------- linalg/vector.rs
struct Vector {
  double x, y, z, w;
  static Vector point(double x, double y, double z) { return {x, y, z, 1.0}; }   // :16-18
  static Vector vector(double x, double y, double z) { return {x, y, z, 0.0}; }  // :20-22
  double magnitude() const { return std::sqrt(x * x + y * y + z * z); }          // :24-26
  Vector normalize() const {                                                     // :28-37
    double m = magnitude();
    return {x / m, y / m, z / m, 0.0};
  }
  double dot(const Vector& o) const { return x * o.x + y * o.y + z * o.z; }  // :39-41
  Vector cross(const Vector& o) const {                                      // :43-49
    return vector(y * o.z - z * o.y, z * o.x - x * o.z, x * o.y - y * o.x);
  }
  Vector operator+(const Vector& o) const { return {x + o.x, y + o.y, z + o.z, w + o.w}; }  // :92-103
  Vector operator-(const Vector& o) const { return {x - o.x, y - o.y, z - o.z, w - o.w}; }  // :105-116
  Vector operator-() const { return {-x, -y, -z, -w}; }                                    // :118-129
  Vector operator*(double s) const { return {x * s, y * s, z * s, w * s}; }                // :131-142
  Vector operator/(double s) const { return {x / s, y / s, z / s, w / s}; }                // :144-155
  Vector reflect(const Vector& n) const { return *this - n * (2.0 * dot(n)); }             // :75-77
};

// ---------------------------------------------------------------- linalg/matrix.rs
struct Matrix {
  double m[4][4];
  static Matrix from16(const double* a) {
    Matrix r;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) r.m[i][j] = a[i * 4 + j];
    return r;
  }
  static Matrix id() {  // :19-28
    Matrix r{};
    for (int i = 0; i < 4; i++) r.m[i][i] = 1.0;
    return r;
  }
  static Matrix translation(double x, double y, double z) {  // :30-40
    Matrix r = id();
    r.m[0][3] = x; r.m[1][3] = y; r.m[2][3] = z;
    return r;
  }
  static Matrix scaling(double x, double y, double z) {  // :42-52
    Matrix r = id();
    r.m[0][0] = x; r.m[1][1] = y; r.m[2][2] = z;
    return r;
  }
  static Matrix rotation_x(double a) {  // :54-64
    Matrix r = id();
    r.m[1][1] = std::cos(a); r.m[1][2] = -std::sin(a);
    r.m[2][1] = std::sin(a); r.m[2][2] = std::cos(a);
    return r;
  }
  static Matrix rotation_y(double a) {  // :66-76
    Matrix r = id();
    r.m[0][0] = std::cos(a); r.m[0][2] = std::sin(a);
    r.m[2][0] = -std::sin(a); r.m[2][2] = std::cos(a);
    return r;
  }
  static Matrix rotation_z(double a) {  // :78-88
    Matrix r = id();
    r.m[0][0] = std::cos(a); r.m[0][1] = -std::sin(a);
    r.m[1][0] = std::sin(a); r.m[1][1] = std::cos(a);
    return r;
  }
  static Matrix shearing(double xy, double xz, double yx, double yz, double zx, double zy) {  // :90-100
    Matrix r = id();
    r.m[0][1] = xy; r.m[0][2] = xz;
    r.m[1][0] = yx; r.m[1][2] = yz;
    r.m[2][0] = zx; r.m[2][1] = zy;
    return r;
  }
  Matrix transpose() const {  // :126-136
    Matrix r;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) r.m[j][i] = m[i][j];
    return r;
  }
  // :138-160 / :162-207 — 2x2 sub-determinant (s*, c*) cofactor expansion.
  double determinant() const {
    double s0 = m[0][0] * m[1][1] - m[1][0] * m[0][1];
    double s1 = m[0][0] * m[1][2] - m[1][0] * m[0][2];
    double s2 = m[0][0] * m[1][3] - m[1][0] * m[0][3];
    double s3 = m[0][1] * m[1][2] - m[1][1] * m[0][2];
    double s4 = m[0][1] * m[1][3] - m[1][1] * m[0][3];
    double s5 = m[0][2] * m[1][3] - m[1][2] * m[0][3];
    double c5 = m[2][2] * m[3][3] - m[3][2] * m[2][3];
    double c4 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
    double c3 = m[2][1] * m[3][2] - m[3][1] * m[2][2];
    double c2 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
    double c1 = m[2][0] * m[3][2] - m[3][0] * m[2][2];
    double c0 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
    return s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
  }
  bool inverse(Matrix* out) const {  // :162-207; false where the reference asserts det != 0
    double s0 = m[0][0] * m[1][1] - m[1][0] * m[0][1];
    double s1 = m[0][0] * m[1][2] - m[1][0] * m[0][2];
    double s2 = m[0][0] * m[1][3] - m[1][0] * m[0][3];
    double s3 = m[0][1] * m[1][2] - m[1][1] * m[0][2];
    double s4 = m[0][1] * m[1][3] - m[1][1] * m[0][3];
    double s5 = m[0][2] * m[1][3] - m[1][2] * m[0][3];
    double c5 = m[2][2] * m[3][3] - m[3][2] * m[2][3];
    double c4 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
    double c3 = m[2][1] * m[3][2] - m[3][1] * m[2][2];
    double c2 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
    double c1 = m[2][0] * m[3][2] - m[3][0] * m[2][2];
    double c0 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
    double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    if (!(det != 0.0)) return false;
    Matrix r;
    r.m[0][0] = (m[1][1] * c5 - m[1][2] * c4 + m[1][3] * c3) / det;
    r.m[0][2] = (m[3][1] * s5 - m[3][2] * s4 + m[3][3] * s3) / det;
    r.m[1][1] = (m[0][0] * c5 - m[0][2] * c2 + m[0][3] * c1) / det;
    r.m[1][3] = (m[2][0] * s5 - m[2][2] * s2 + m[2][3] * s1) / det;
    r.m[2][0] = (m[1][0] * c4 - m[1][1] * c2 + m[1][3] * c0) / det;
    r.m[2][2] = (m[3][0] * s4 - m[3][1] * s2 + m[3][3] * s0) / det;
    r.m[3][1] = (m[0][0] * c3 - m[0][1] * c1 + m[0][2] * c0) / det;
    r.m[3][3] = (m[2][0] * s3 - m[2][1] * s1 + m[2][2] * s0) / det;
    r.m[0][1] = (-m[0][1] * c5 + m[0][2] * c4 - m[0][3] * c3) / det;
    r.m[0][3] = (-m[2][1] * s5 + m[2][2] * s4 - m[2][3] * s3) / det;
    r.m[1][0] = (-m[1][0] * c5 + m[1][2] * c2 - m[1][3] * c1) / det;
    r.m[1][2] = (-m[3][0] * s5 + m[3][2] * s2 - m[3][3] * s1) / det;
    r.m[2][1] = (-m[0][0] * c4 + m[0][1] * c2 - m[0][3] * c0) / det;
    r.m[2][3] = (-m[2][0] * s4 + m[2][1] * s2 - m[2][3] * s0) / det;
    r.m[3][0] = (-m[1][0] * c3 + m[1][1] * c1 - m[1][2] * c0) / det;
    r.m[3][2] = (-m[3][0] * s3 + m[3][1] * s1 - m[3][2] * s0) / det;
    *out = r;
    return true;
  }
  Matrix inverse_or_die() const {
    Matrix r;
    if (!inverse(&r)) {
      std::fprintf(stderr, "oracle: singular matrix (reference asserts det != 0, src/linalg/matrix.rs:181)\n");
      std::abort();
    }
    return r;
  }
  Matrix operator*(const Matrix& o) const {  // :239-259
    Matrix r;
    for (int row = 0; row < 4; row++)
      for (int col = 0; col < 4; col++) {
        double value = 0.0;
        for (int i = 0; i < 4; i++) value += m[row][i] * o.m[i][col];
        r.m[row][col] = value;
      }
    return r;
  }
  Vector operator*(const Vector& v) const {  // :261-284
    return {m[0][0] * v.x + m[0][1] * v.y + m[0][2] * v.z + m[0][3] * v.w,
            m[1][0] * v.x + m[1][1] * v.y + m[1][2] * v.z + m[1][3] * v.w,
            m[2][0] * v.x + m[2][1] * v.y + m[2][2] * v.z + m[2][3] * v.w,
            m[3][0] * v.x + m[3][1] * v.y + m[3][2] * v.z + m[3][3] * v.w};
  }
};

// ---------------------------------------------------------------- color.rs
struct Color {
  double r, g, b;
  static Color black() { return {0.0, 0.0, 0.0}; }
  static Color white() { return {1.0, 1.0, 1.0}; }
  Color operator+(const Color& o) const { return {r + o.r, g + o.g, b + o.b}; }  // :70-80
  Color operator-(const Color& o) const { return {r - o.r, g - o.g, b - o.b}; }  // :88-98
  Color operator*(double s) const { return {r * s, g * s, b * s}; }              // :100-110
  Color operator*(const Color& o) const { return {r * o.r, g * o.g, b * o.b}; }  // :112-122
  Color avg(const Color& o) const { return (*this + o) * 0.5; }                  // :48-50
  // :42-46 — `(x.min(1).max(0) * 255).round() as u8` (round = half away from zero)
  static uint8_t clamp1(double x) {
    double c = rmax(rmin(x, 1.0), 0.0) * 255.0;
    double rr = std::round(c);
    if (rr != rr) return 0;
    if (rr <= 0.0) return 0;
    if (rr >= 255.0) return 255;
    return (uint8_t)rr;
  }
};

// ---------------------------------------------------------------- ray.rs / light.rs
struct Ray {
  Vector origin, direction;
  Vector position(double t) const { return origin + direction * t; }          // ray.rs:10-12
  Ray transform(const Matrix& mm) const { return {mm * origin, mm * direction}; }  // ray.rs:14-19
};
struct PointLight {  // light.rs:5-8
  Color intensity;
  Vector origin;
};

// ---------------------------------------------------------------- noise.rs
// Ken Perlin's reference permutation (src/noise.rs:56-84 holds it twice, 512 entries).
static const uint8_t PERM[256] = {
    151, 160, 137, 91,  90,  15,  131, 13,  201, 95,  96,  53,  194, 233, 7,   225, 140, 36,  103, 30,
    69,  142, 8,   99,  37,  240, 21,  10,  23,  190, 6,   148, 247, 120, 234, 75,  0,   26,  197, 62,
    94,  252, 219, 203, 117, 35,  11,  32,  57,  177, 33,  88,  237, 149, 56,  87,  174, 20,  125, 136,
    171, 168, 68,  175, 74,  165, 71,  134, 139, 48,  27,  166, 77,  146, 158, 231, 83,  111, 229, 122,
    60,  211, 133, 230, 220, 105, 92,  41,  55,  46,  245, 40,  244, 102, 143, 54,  65,  25,  63,  161,
    1,   216, 80,  73,  209, 76,  132, 187, 208, 89,  18,  169, 200, 196, 135, 130, 116, 188, 159, 86,
    164, 100, 109, 198, 173, 186, 3,   64,  52,  217, 226, 250, 124, 123, 5,   202, 38,  147, 118, 126,
    255, 82,  85,  212, 207, 206, 59,  227, 47,  16,  58,  17,  182, 189, 28,  42,  223, 183, 170, 213,
    119, 248, 152, 2,   44,  154, 163, 70,  221, 153, 101, 155, 167, 43,  172, 9,   129, 22,  39,  253,
    19,  98,  108, 110, 79,  113, 224, 232, 178, 185, 112, 104, 218, 246, 97,  228, 251, 34,  242, 193,
    238, 210, 144, 12,  191, 179, 162, 241, 81,  51,  145, 235, 249, 14,  239, 107, 49,  192, 214, 31,
    181, 199, 106, 157, 184, 84,  204, 176, 115, 121, 50,  45,  127, 4,   150, 254, 138, 236, 205, 93,
    222, 114, 67,  29,  24,  72,  243, 141, 128, 195, 78,  66,  215, 61,  156, 180};
inline size_t nhash(size_t i) { return PERM[i & 255]; }  // noise.rs:90-92 (table is periodic with 256)

inline double ngrad(size_t h, double x, double y, double z) {  // noise.rs:94-114
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
inline int32_t fast_floor(double x) {  // noise.rs:116-122
  return x > 0.0 ? as_i32(x) : wrap_sub(as_i32(x), 1);
}
inline size_t modulus(int32_t x, int32_t mm) {  // noise.rs:124-131
  int32_t a = x % mm;
  return a < 0 ? (size_t)(a + mm) : (size_t)a;
}
inline double simplex(double x, double y, double z) {  // noise.rs:134-219
  const double F3 = 1.0 / 3.0, G3 = 1.0 / 6.0;
  double s = (x + y + z) * F3;
  int32_t i = fast_floor(x + s), j = fast_floor(y + s), k = fast_floor(z + s);
  double t = (double)wrap_add(wrap_add(i, j), k) * G3;
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
  size_t ii = modulus(i, 256), jj = modulus(j, 256), kk = modulus(k, 256);
  size_t gi0 = nhash(ii + nhash(jj + nhash(kk)));
  size_t gi1 = nhash(ii + i1 + nhash(jj + j1 + nhash(kk + k1)));
  size_t gi2 = nhash(ii + i2 + nhash(jj + j2 + nhash(kk + k2)));
  size_t gi3 = nhash(ii + 1 + nhash(jj + 1 + nhash(kk + 1)));
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
inline double fractal(double x, double y, double z, size_t octaves) {  // noise.rs:221-237
  double output = 0.0, denom = 0.0, frequency = 1.0, amplitude = 1.0;
  const double lacunarity = 2.0, persistence = 0.5;
  for (size_t o = 0; o < octaves; o++) {
    output += amplitude * simplex(x * frequency, y * frequency, z * frequency);
    denom += amplitude;
    frequency *= lacunarity;
    amplitude *= persistence;
  }
  return output / denom;
}
struct Noise {  // noise.rs:4-7
  enum Kind { Simplex = 0, Fractal = 1 } kind = Simplex;
  double scale = 1.0;
  size_t octaves = 1;
  void jitter_3d(double x, double y, double z, double* ox, double* oy, double* oz) const {  // :31-52
    double nx, ny, nz;
    if (kind == Simplex) {
      nx = simplex(x, y, z) * scale;
      ny = simplex(x, y, z + 1.0) * scale;
      nz = simplex(x, y, z + 2.0) * scale;
    } else {
      nx = fractal(x, y, z, octaves) * scale;
      ny = fractal(x, y, z + 1.0, octaves) * scale;
      nz = fractal(x, y, z + 2.0, octaves) * scale;
    }
    *ox = x + nx; *oy = y + ny; *oz = z + nz;
  }
};

// ---------------------------------------------------------------- material.rs
enum JitterKind { JitterColor = 0, JitterPoint = 1 };
enum MixtureKind { Blend = 0, Checkers = 1, RingGradient = 2, Ring = 3, Gradient = 4, Stripes = 5 };

struct Pattern;
using PatternPtr = std::shared_ptr<const Pattern>;  // Box<Pattern>; trees are immutable so clones may share
struct Pattern {                                    // material.rs:60-65
  enum Tag {
    Debug = 0, Plain = 1, Jitter = 2, Mixture = 3,
#ifdef ORC_EXT
    UV = 4,  // include/rtc.h RTC_PAT_UV (rt_oracle_ext.hpp)
#endif
  } tag = Plain;
  Color color{1, 1, 1};
  JitterKind jkind = JitterPoint;
  Noise noise;
  MixtureKind mkind = Blend;
  Matrix transform_inv = Matrix::id();
  PatternPtr left, right;  // Jitter uses `left` as its child
#ifdef ORC_EXT
  std::shared_ptr<const struct UvNode> uv;  // UV: the map and its records; transform_inv as a Mixture's
  Color uv_color_at(Vector point) const;    // rt_oracle_ext.hpp
#endif

  static PatternPtr debug() { auto p = std::make_shared<Pattern>(); p->tag = Debug; return p; }
  static PatternPtr plain(Color c) { auto p = std::make_shared<Pattern>(); p->tag = Plain; p->color = c; return p; }
  static PatternPtr jitter(JitterKind k, Noise n, PatternPtr child) {  // :114-128
    auto p = std::make_shared<Pattern>();
    p->tag = Jitter; p->jkind = k; p->noise = n; p->left = std::move(child);
    return p;
  }
  static PatternPtr mixture(MixtureKind k, const Matrix& transform, PatternPtr l, PatternPtr r) {  // :130-137
    auto p = std::make_shared<Pattern>();
    p->tag = Mixture; p->mkind = k; p->transform_inv = transform.inverse_or_die();
    p->left = std::move(l); p->right = std::move(r);
    return p;
  }

  Color color_at(Vector point) const {  // :164-187
    switch (tag) {
      case Debug: return {point.x, point.y, point.z};
      case Plain: return color;
      case Jitter: {  // :206-224
        if (jkind == JitterColor) {
          Color c = left->color_at(point);
          double nr, ng, nb;
          noise.jitter_3d(c.r, c.g, c.b, &nr, &ng, &nb);
          return {nr, ng, nb};
        } else {
          double nx, ny, nz;
          noise.jitter_3d(point.x, point.y, point.z, &nx, &ny, &nz);
          return left->color_at(Vector::point(nx, ny, nz));
        }
      }
#ifdef ORC_EXT
      case UV: return uv_color_at(point);
#endif
      default: {
        Vector p = transform_inv * point;
        return mix(p);
      }
    }
  }
  Color mix(Vector point) const {  // :250-302
    switch (mkind) {
      case Blend: {
        Color l = left->color_at(point), r = right->color_at(point);
        return l.avg(r);
      }
      case Checkers: {
        int32_t x = as_i32(std::floor(point.x)), y = as_i32(std::floor(point.y)), z = as_i32(std::floor(point.z));
        return (wrap_add(wrap_add(x, y), z) % 2 == 0) ? left->color_at(point) : right->color_at(point);
      }
      case RingGradient: {
        double distance = (point - Vector::point(0.0, 0.0, 0.0)).magnitude();
        double fraction = distance - std::floor(distance);
        Color l = left->color_at(point), r = right->color_at(point);
        return l + ((r - l) * fraction);
      }
      case Ring:
        return (as_i32(std::floor(std::sqrt(point.x * point.x + point.z * point.z))) % 2 == 0)
                   ? left->color_at(point) : right->color_at(point);
      case Gradient: {
        double fraction = point.x - std::floor(point.x);
        Color l = left->color_at(point), r = right->color_at(point);
        return l + ((r - l) * fraction);
      }
      default:  // Stripes
        return (as_i32(std::floor(point.x)) % 2 == 0) ? left->color_at(point) : right->color_at(point);
    }
  }
};

struct Material {  // material.rs:19-43
  PatternPtr pattern = Pattern::plain(Color::white());
  double ambient = 0.1, diffuse = 0.9, specular = 0.9, shininess = 200.0;
  double reflective = 0.0, transparency = 0.0, refractive_index = 1.0;
#ifdef ORC_EXT
  std::shared_ptr<const struct BumpRecord> bump;  // include/rtc.h rtc_bump (rt_oracle_ext.hpp); null: no record
#endif
};

// ---------------------------------------------------------------- bounding_box.rs
// shape.rs:635-653
inline void intersect_cube_axis(double origin, double direction, double mn, double mx, double* tmin, double* tmax) {
  double t_min_numerator = mn - origin, t_max_numerator = mx - origin;
  double a, b;
  if (std::fabs(direction) >= EPSILON) {
    a = t_min_numerator / direction;
    b = t_max_numerator / direction;
  } else {
    a = t_min_numerator * INF;
    b = t_max_numerator * INF;
  }
  if (a > b) { *tmin = b; *tmax = a; } else { *tmin = a; *tmax = b; }
}

struct BoundingBox {
  Vector min, max;
  static BoundingBox empty() {  // :19-24
    return {Vector::point(INF, INF, INF), Vector::point(-INF, -INF, -INF)};
  }
  BoundingBox insert(const Vector& p) const {  // :30-43
    return {Vector::point(rmin(min.x, p.x), rmin(min.y, p.y), rmin(min.z, p.z)),
            Vector::point(rmax(max.x, p.x), rmax(max.y, p.y), rmax(max.z, p.z))};
  }
  BoundingBox unite(const BoundingBox& o) const { return insert(o.min).insert(o.max); }  // :45-47
  bool contains(const Vector& p) const {                                                 // :49-56
    return min.x <= p.x && p.x <= max.x && min.y <= p.y && p.y <= max.y && min.z <= p.z && p.z <= max.z;
  }
  bool encloses(const BoundingBox& o) const { return contains(o.min) && contains(o.max); }  // :58-60
  BoundingBox transform(const Matrix& mm) const {                                          // :62-78
    Vector p[8] = {min,
                   Vector::point(min.x, min.y, max.z),
                   Vector::point(min.x, max.y, min.z),
                   Vector::point(min.x, max.y, max.z),
                   Vector::point(max.x, min.y, min.z),
                   Vector::point(max.x, min.y, max.z),
                   Vector::point(max.x, max.y, min.z),
                   max};
    BoundingBox b = empty();
    for (auto& q : p) b = b.insert(mm * q);
    return b;
  }
  bool intersects(const Ray& ray) const {  // :80-92
    double xa, xb, ya, yb, za, zb;
    intersect_cube_axis(ray.origin.x, ray.direction.x, min.x, max.x, &xa, &xb);
    intersect_cube_axis(ray.origin.y, ray.direction.y, min.y, max.y, &ya, &yb);
    intersect_cube_axis(ray.origin.z, ray.direction.z, min.z, max.z, &za, &zb);
    double t_min = rmax(rmax(xa, ya), za);
    double t_max = rmin(rmin(xb, yb), zb);
    return t_min <= t_max;
  }
};

// ---------------------------------------------------------------- shape.rs
struct Shape;
struct Intersection {  // intersection.rs:42-47
  double t;
  const Shape* shape;
  bool has_uv;
  double u, v;
  int push_idx;  // bookkeeping only (position within the shape's own pushes); not in the reference
};
using Intersections = std::vector<Intersection>;

enum GeometryKind { Sphere = 0, Plane = 1, Cube = 2, Cylinder = 3, Cone = 4, Triangle = 5, SmoothTriangle = 6 };

struct Geometry {  // shape.rs:466-498
  GeometryKind kind = Sphere;
  double min = -INF, max = INF;
  bool closed = false;
  Vector p1{}, p2{}, p3{}, e1{}, e2{}, n{}, n1{}, n2{}, n3{};

  BoundingBox bbox() const {  // :948-996
    switch (kind) {
      case Sphere:
      case Cube: return {Vector::point(-1, -1, -1), Vector::point(1, 1, 1)};
      case Plane: return {Vector::point(-INF, 0.0, -INF), Vector::point(INF, 0.0, INF)};
      case Cylinder:
        if (closed) return {Vector::point(-1.0, min, -1.0), Vector::point(1.0, max, 1.0)};
        return {Vector::point(-1.0, -INF, -1.0), Vector::point(1.0, INF, 1.0)};
      case Cone:
        if (closed) {
          double limit = rmax(std::fabs(min), std::fabs(max));
          return {Vector::point(-limit, min, -limit), Vector::point(limit, max, limit)};
        }
        return {Vector::point(-INF, -INF, -INF), Vector::point(INF, INF, INF)};
      default: return BoundingBox::empty().insert(p1).insert(p2).insert(p3);
    }
  }
};

static std::atomic<size_t> g_next_id{0};  // shape.rs:18-28 (thread-local there; identity only)

struct Shape {  // shape.rs:297-306
  Matrix transform_inv, transform_inv_tsp;
  BoundingBox bbox;
  Matrix material_inv;
  Material material;
  Geometry geometry;
  bool casts_shadow = true;
  size_t id = 0;

  static Shape make(const Matrix& transform, const Material& material, bool casts_shadow, const Geometry& g) {  // :335-347
    Matrix inv = transform.inverse_or_die();
    Shape s;
    s.transform_inv = inv;
    s.transform_inv_tsp = inv.transpose();
    s.bbox = g.bbox().transform(transform);
    s.material_inv = inv;
    s.material = material;
    s.geometry = g;
    s.casts_shadow = casts_shadow;
    s.id = g_next_id++;
    return s;
  }
  static Geometry triangle_geometry(Vector p1, Vector p2, Vector p3) {  // :369-385
    Geometry g;
    g.kind = Triangle;
    g.p1 = p1; g.p2 = p2; g.p3 = p3;
    g.e1 = p2 - p1; g.e2 = p3 - p1;
    g.n = g.e2.cross(g.e1).normalize();
    return g;
  }
  static Geometry smooth_triangle_geometry(Vector p1, Vector p2, Vector p3, Vector n1, Vector n2, Vector n3) {  // :387-412
    Geometry g;
    g.kind = SmoothTriangle;
    g.p1 = p1; g.p2 = p2; g.p3 = p3;
    g.e1 = p2 - p1; g.e2 = p3 - p1;
    g.n1 = n1; g.n2 = n2; g.n3 = n3;
    return g;
  }

  void push(Intersections& xs, double t, int& k, bool has_uv = false, double u = 0, double v = 0) const {
    xs.push_back({t, this, has_uv, u, v, k++});
  }

  // :414-417 + Geometry::intersect :862-885
  void intersect(const Ray& world_ray, Intersections& xs) const {
    Ray ray = world_ray.transform(transform_inv);
    int k = 0;
    const Vector& o = ray.origin;
    const Vector& d = ray.direction;
    switch (geometry.kind) {
      case Sphere: {  // :592-619
        Vector sphere_to_ray = o - Vector::point(0.0, 0.0, 0.0);
        double a = d.dot(d);
        double b = 2.0 * d.dot(sphere_to_ray);
        double c = sphere_to_ray.dot(sphere_to_ray) - 1.0;
        double disc = b * b - 4.0 * a * c;
        if (disc < 0.0) return;
        double t0 = (-b - std::sqrt(disc)) / (2.0 * a);
        double t1 = (-b + std::sqrt(disc)) / (2.0 * a);
        push(xs, t0, k);
        push(xs, t1, k);
        return;
      }
      case Plane: {  // :621-633
        if (approx(d.y, 0.0)) return;
        push(xs, -o.y / d.y, k);
        return;
      }
      case Cube: {  // :655-679
        double xa, xb, ya, yb, za, zb;
        intersect_cube_axis(o.x, d.x, -1.0, 1.0, &xa, &xb);
        intersect_cube_axis(o.y, d.y, -1.0, 1.0, &ya, &yb);
        intersect_cube_axis(o.z, d.z, -1.0, 1.0, &za, &zb);
        double t_min = rmax(rmax(xa, ya), za);
        double t_max = rmin(rmin(xb, yb), zb);
        if (t_min <= t_max) {
          push(xs, t_min, k);
          push(xs, t_max, k);
        }
        return;
      }
      case Cylinder: {  // :724-768
        double mn = geometry.min, mx = geometry.max;
        double a = d.x * d.x + d.z * d.z;
        if (!approx(a, 0.0)) {
          double b = 2.0 * o.x * d.x + 2.0 * o.z * d.z;
          double c = o.x * o.x + o.z * o.z - 1.0;
          double disc = b * b - 4.0 * a * c;
          if (disc >= 0.0) {
            double t0 = (-b - std::sqrt(disc)) / (2.0 * a);
            double y0 = o.y + t0 * d.y;
            if (mn < y0 && y0 < mx) push(xs, t0, k);
            double t1 = (-b + std::sqrt(disc)) / (2.0 * a);
            double y1 = o.y + t1 * d.y;
            if (mn < y1 && y1 < mx) push(xs, t1, k);
          }
        }
        intersect_cap(ray, mn, mx, 1.0, 1.0, xs, k);
        return;
      }
      case Cone: {  // :770-822
        double mn = geometry.min, mx = geometry.max;
        double a = d.x * d.x - d.y * d.y + d.z * d.z;
        double b = 2.0 * o.x * d.x - 2.0 * o.y * d.y + 2.0 * o.z * d.z;
        if (!approx(a, 0.0) || !approx(b, 0.0)) {
          double c = o.x * o.x - o.y * o.y + o.z * o.z;
          if (!approx(a, 0.0)) {
            double disc = b * b - 4.0 * a * c;
            if (disc >= 0.0) {
              double t0 = (-b - std::sqrt(disc)) / (2.0 * a);
              double y0 = o.y + t0 * d.y;
              if (mn < y0 && y0 < mx) push(xs, t0, k);
              double t1 = (-b + std::sqrt(disc)) / (2.0 * a);
              double y1 = o.y + t1 * d.y;
              if (mn < y1 && y1 < mx) push(xs, t1, k);
            }
          } else {
            push(xs, -c / (2.0 * b), k);
          }
        }
        intersect_cap(ray, mn, mx, mn, mx, xs, k);
        return;
      }
      default: {  // Triangle / SmoothTriangle :824-860
        const Vector &p1 = geometry.p1, &e1 = geometry.e1, &e2 = geometry.e2;
        Vector dir_cross_e2 = d.cross(e2);
        double det = e1.dot(dir_cross_e2);
        if (std::fabs(det) < EPSILON) return;
        double f = 1.0 / det;
        Vector p1_to_origin = o - p1;
        double u = f * p1_to_origin.dot(dir_cross_e2);
        if (u < 0.0 || u > 1.0) return;
        Vector origin_cross_e1 = p1_to_origin.cross(e1);
        double v = f * d.dot(origin_cross_e1);
        if (v < 0.0 || u + v > 1.0) return;
        push(xs, f * e2.dot(origin_cross_e1), k, true, u, v);
        return;
      }
    }
  }
  // :681-722
  void intersect_cap(const Ray& ray, double mn, double mx, double min_radius, double max_radius, Intersections& xs,
                     int& k) const {
    if (!geometry.closed || approx(ray.direction.y, 0.0)) return;
    auto hits_cap = [&](double t, double radius) {
      double x = ray.origin.x + t * ray.direction.x;
      double z = ray.origin.z + t * ray.direction.z;
      return (x * x + z * z) <= radius * radius;
    };
    double t = (mn - ray.origin.y) / ray.direction.y;
    if (hits_cap(t, min_radius)) push(xs, t, k);
    t = (mx - ray.origin.y) / ray.direction.y;
    if (hits_cap(t, max_radius)) push(xs, t, k);
  }

  Vector local_normal(const Vector& p, bool has_uv, double u, double v) const {  // :887-946
    const Geometry& g = geometry;
    switch (g.kind) {
      case Sphere: return Vector::vector(p.x, p.y, p.z);
      case Plane: return Vector::vector(0.0, 1.0, 0.0);
      case Cube: {
        double xa = std::fabs(p.x), ya = std::fabs(p.y), za = std::fabs(p.z);
        double mx = rmax(rmax(xa, ya), za);
        if (mx == xa) return Vector::vector(p.x, 0.0, 0.0);
        if (mx == ya) return Vector::vector(0.0, p.y, 0.0);
        return Vector::vector(0.0, 0.0, p.z);
      }
      case Cylinder: {
        double dist = p.x * p.x + p.z * p.z;
        if (dist < 1.0 && p.y >= g.max - EPSILON) return Vector::vector(0.0, 1.0, 0.0);
        if (dist < 1.0 && p.y <= g.min + EPSILON) return Vector::vector(0.0, -1.0, 0.0);
        return Vector::vector(p.x, 0.0, p.z);
      }
      case Cone: {
        double dist = p.x * p.x + p.z * p.z;
        if (dist < 1.0 && p.y >= g.max - EPSILON) return Vector::vector(0.0, 1.0, 0.0);
        if (dist < 1.0 && p.y <= g.min + EPSILON) return Vector::vector(0.0, -1.0, 0.0);
        double y = std::sqrt(dist);
        if (p.y > 0.0) y = -y;
        return Vector::vector(p.x, y, p.z);
      }
      case Triangle: return g.n;
      default:
        if (!has_uv) {
          std::fprintf(stderr, "oracle: smooth triangle normal without u,v (reference unwraps, src/shape.rs:940)\n");
          std::abort();
        }
        return g.n2 * u + g.n3 * v + g.n1 * (1.0 - u - v);
    }
  }
  Vector normal(const Vector& point, bool has_uv, double u, double v) const {  // :419-427
    Vector shape_point = transform_inv * point;
    Vector shape_normal = local_normal(shape_point, has_uv, u, v);
    Vector world_normal = transform_inv_tsp * shape_normal;
    world_normal.w = 0.0;
    return world_normal.normalize();
  }
  Color lighting(const PointLight& light, const Vector& point, const Vector& eye, const Vector& normal,
                 bool shadowed) const {  // :429-462
    Color color = material.pattern->color_at(material_inv * point);
    Color effective_color = color * light.intensity;
    Color intensity = light.intensity;
    Vector lightv = (light.origin - point).normalize();
    Color ambient = effective_color * material.ambient;
    Color diffuse = Color::black(), specular = Color::black();
    double light_dot_normal = lightv.dot(normal);
    if (!shadowed && light_dot_normal >= 0.0) {
      diffuse = effective_color * material.diffuse * light_dot_normal;
      Vector reflect = (-lightv).reflect(normal);
      double reflect_dot_eye = reflect.dot(eye);
      if (reflect_dot_eye > 0.0) specular = intensity * material.specular * std::pow(reflect_dot_eye, material.shininess);
    }
    return ambient + diffuse + specular;
  }
};

enum GroupKind { Union = 0, GIntersection = 1, Difference = 2, Aggregation = 3 };  // shape.rs:161-166
inline bool allows_intersection(GroupKind k, bool left_hit, bool in_left, bool in_right) {  // :168-178
  switch (k) {
    case Union: return (left_hit && !in_right) || (!left_hit && !in_left);
    case GIntersection: return (left_hit && in_right) || (!left_hit && in_left);
    case Difference: return (left_hit && !in_right) || (!left_hit && in_left);
    default: return true;
  }
}

struct Element;
using ElementPtr = std::unique_ptr<Element>;
inline void sort_intersections(Intersections& xs, bool* nan_seen);

struct Element {  // shape.rs:31-34 (Composite(Group) | Primitive(Shape)); Group :181-185
  bool is_group = false;
  Shape shape;  // Primitive
  GroupKind kind = Aggregation;
  BoundingBox gbbox = BoundingBox::empty();
  std::vector<ElementPtr> children;

  static ElementPtr primitive(Shape s) {
    auto e = std::make_unique<Element>();
    e->is_group = false;
    e->shape = std::move(s);
    return e;
  }
  BoundingBox bbox() const { return is_group ? gbbox : shape.bbox; }  // :146-151
  bool includes(const Shape* s) const {                               // :153-158, :226-228
    if (!is_group) return shape.id == s->id;
    for (auto& c : children)
      if (c->includes(s)) return true;
    return false;
  }
  void propagate_inverses(const Matrix& transform, const Matrix& inv, const Matrix& inv_tsp,
                          const Material* material) {  // :47-72
    if (is_group) {
      for (auto& c : children) c->propagate_inverses(transform, inv, inv_tsp, material);
      gbbox = gbbox.transform(transform);
    } else {
      shape.transform_inv = shape.transform_inv * inv;
      shape.transform_inv_tsp = inv_tsp * shape.transform_inv_tsp;
      if (material) {
        shape.material = *material;
        shape.material_inv = inv;
      } else {
        shape.material_inv = shape.material_inv * inv;
      }
    }
  }
  static ElementPtr composite(const Matrix& transform, const Material* material, GroupKind kind,
                              std::vector<ElementPtr> children) {  // :74-101
    if (kind != Aggregation && children.size() != 2) {
      std::fprintf(stderr, "oracle: CSG group needs exactly 2 children (src/shape.rs:82)\n");
      std::abort();
    }
    Matrix inv = transform.inverse_or_die();
    Matrix inv_tsp = inv.transpose();
    BoundingBox b = BoundingBox::empty();
    for (auto& c : children) b = b.unite(c->bbox());
    auto e = std::make_unique<Element>();
    e->is_group = true;
    e->kind = kind;
    e->gbbox = b;
    e->children = std::move(children);
    e->propagate_inverses(transform, inv, inv_tsp, material);
    return e;
  }
  void filter_by_group(Intersections& xs) const {  // :230-246
    bool in_left = false, in_right = false;
    Intersections kept;
    for (auto& i : xs) {
      bool left_hit = children[0]->includes(i.shape);
      bool keep = allows_intersection(kind, left_hit, in_left, in_right);
      if (left_hit) in_left = !in_left; else in_right = !in_right;
      if (keep) kept.push_back(i);
    }
    xs.swap(kept);
  }
  void intersect(const Ray& ray, Intersections& xs, bool* nan_seen) const {  // :139-144, :248-269
    if (!is_group) {
      shape.intersect(ray, xs);
      return;
    }
    if (gbbox.intersects(ray)) {
      if (kind == Aggregation) {
        for (auto& c : children) c->intersect(ray, xs, nan_seen);
      } else {
        Intersections tmp;
        for (auto& c : children) c->intersect(ray, tmp, nan_seen);
        sort_intersections(tmp, nan_seen);
        filter_by_group(tmp);
        xs.insert(xs.end(), tmp.begin(), tmp.end());
      }
    }
  }
};

// ---------------------------------------------------------------- intersection.rs
// :123-125 — stable sort by t; the reference panics on NaN (`partial_cmp().unwrap()`).
inline void sort_intersections(Intersections& xs, bool* nan_seen) {
  if (xs.size() > 1)  // a 0/1-element slice never calls the comparator
    for (auto& i : xs)
      if (i.t != i.t) { if (nan_seen) *nan_seen = true; }
  std::stable_sort(xs.begin(), xs.end(), [](const Intersection& a, const Intersection& b) { return a.t < b.t; });
}
inline const Intersection* hit(const Intersections& xs) {  // :127-132
  for (auto& i : xs)
    if (i.t >= 0.0) return &i;
  return nullptr;
}
inline double schlick(const Vector& eye, const Vector& normal, double n1, double n2) {  // :24-39
  double cosv = eye.dot(normal);
  if (n1 > n2) {
    double n = n1 / n2;
    double sin2_t = n * n * (1.0 - cosv * cosv);
    if (sin2_t > 1.0) return 1.0;
    cosv = std::sqrt(1.0 - sin2_t);
  }
  double q = (n1 - n2) / (n1 + n2);
  double r0 = q * q;
  double x = 1.0 - cosv;
  double x5 = x * ((x * x) * (x * x));  // powi(5) as compiler-rt __powidf2 evaluates it
  return r0 + (1.0 - r0) * x5;
}
struct State {  // :9-22
  double t;
  const Shape* shape;
  Vector point, over_point, under_point, eye, normal, reflect;
  bool inside;
  double n1, n2, reflectance;
#ifdef ORC_EXT
  Vector geo_normal;  // the flipped geometric normal (`normal` is the shading normal ns where the material has a bump record)
#endif
};
#ifdef ORC_EXT
// include/rtc.h rtc_bump (rt_oracle_ext.hpp): steps 1-4, the unit shading normal before the flip; steps 5-7 on the state.
inline Vector bump_shading_normal(const Shape& shape, const Vector& point, const Vector& n);
inline void bump_state(State& st, Vector ns);
#endif
inline State prepare_state(const Intersection& self, const Ray& ray, const Intersections& xs) {  // :50-121
  State st;
  st.t = self.t;
  st.shape = self.shape;
  st.point = ray.position(self.t);
  st.eye = -ray.direction;
  st.normal = self.shape->normal(st.point, self.has_uv, self.u, self.v);
#ifdef ORC_EXT
  const bool bumped = self.shape->material.bump != nullptr;  // a material without a record takes every step as the reference does
  Vector ns = st.normal;
  if (bumped) ns = bump_shading_normal(*self.shape, st.point, st.normal);
#endif
  st.inside = false;
  if (st.normal.dot(st.eye) < 0.0) {
    st.normal = -st.normal;
    st.inside = true;
  }
  st.over_point = st.point + (st.normal * EPSILON);
  st.under_point = st.point - (st.normal * EPSILON);
#ifdef ORC_EXT
  st.geo_normal = st.normal;
  if (bumped) bump_state(st, ns);  // the flip was decided on the geometric normal, over / under_point are made from it; normal = +-ns
#endif
  st.reflect = ray.direction.reflect(st.normal);

  std::vector<const Shape*> shapes;  // the HashSet mirrors membership of this Vec
  double n1 = 1.0, n2 = 1.0;
  for (auto& i : xs) {
    bool same = (self.t == i.t) && (self.shape->id == i.shape->id);  // :135-139
    if (same) n1 = shapes.empty() ? 1.0 : shapes.back()->material.refractive_index;
    auto it = std::find_if(shapes.begin(), shapes.end(), [&](const Shape* s) { return s->id == i.shape->id; });
    if (it != shapes.end()) {
      std::vector<const Shape*> kept;
      for (auto* s : shapes)
        if (s->id != i.shape->id) kept.push_back(s);
      shapes.swap(kept);
    } else {
      shapes.push_back(i.shape);
    }
    if (same) n2 = shapes.empty() ? 1.0 : shapes.back()->material.refractive_index;
  }
  st.n1 = n1;
  st.n2 = n2;
#if defined(ORC_EXT) && ORC_EXT_MUTANT == 11   // schlick (here) and the refracted direction (refracted_color) from the geometric normal
  st.reflectance = schlick(st.eye, st.geo_normal, n1, n2);
#else
  st.reflectance = schlick(st.eye, st.normal, n1, n2);
#endif
  return st;
}

// ---------------------------------------------------------------- world.rs
struct Counters {
  // calls by recursion depth (0 = primary).  The reference re-traces each reflection/refraction
  // subtree once per light (world.rs:58-79), so a ray at depth d is traced L^d times: unique rays =
  // calls[d] / L^d.
  static constexpr int MAXD = 24;
  uint64_t color_at[MAXD] = {0};
  uint64_t shadow[MAXD] = {0};
  uint64_t prim_tests = 0;
  // The de-duplicated ray tree (TEST CHANNEL, as the digest): every ray once, by class and depth -- the copies the reference re-traces
  // for a light other than the first (Ctx::repeat > 0) are left out.  u_shadow[d]: the is_shadowed calls made for a hit at depth d;
  // u_container[d]: the hits at depth d whose n1 / n2 reach a result (World::color_at).  For a plain world of L lights
  // (u_primary + u_reflect + u_refract)[d] * L^d == color_at[d] and u_shadow[d] * L^d == shadow[d].
  uint64_t u_primary[MAXD] = {0}, u_reflect[MAXD] = {0}, u_refract[MAXD] = {0}, u_shadow[MAXD] = {0}, u_container[MAXD] = {0};
  void add(const Counters& o) {
    for (int i = 0; i < MAXD; i++) {
      color_at[i] += o.color_at[i]; shadow[i] += o.shadow[i];
      u_primary[i] += o.u_primary[i]; u_reflect[i] += o.u_reflect[i]; u_refract[i] += o.u_refract[i];
      u_shadow[i] += o.u_shadow[i]; u_container[i] += o.u_container[i];
    }
    prim_tests += o.prim_tests;
  }
};

struct World {  // :12-15
  std::vector<PointLight> lights;
  std::vector<ElementPtr> elements;
#ifdef ORC_EXT
  // Area lights, light cones and the background (include/rtc.h; not in the reference), rt_oracle_ext.hpp.  Null for a world
  // that has none of them: such a world takes every step below as liboracle.so takes it.
  std::shared_ptr<struct WorldExt> ext;
#endif

  static World default_world() {  // :152-183
    World w;
    w.lights.push_back({Color::white(), Vector::point(-10.0, 10.0, -10.0)});
    Material m1;
    m1.pattern = Pattern::plain({0.8, 1.0, 0.6});
    m1.diffuse = 0.7;
    m1.specular = 0.2;
    Geometry g;
    g.kind = Sphere;
    w.elements.push_back(Element::primitive(Shape::make(Matrix::id(), m1, true, g)));
    w.elements.push_back(Element::primitive(Shape::make(Matrix::scaling(0.5, 0.5, 0.5), Material(), true, g)));
    return w;
  }

  // Hit-tree digest (TEST CHANNEL, not a reference concept): the wrapping 64-bit sum, over every ray of the pixel's ray tree
  // counted ONCE — the reference traces a reflected / refracted subtree once per light (world.rs:58-79); only the first light's
  // copy is summed — of a hash of the ray's nearest hit (t bits, primitive sequence number, push index; a miss: 0, -1, 0), its
  // depth and its kind (0 primary, 1 reflected, 2 refracted).  The hash is the one the device states in csrc/device_scene.h
  // (rtc_hit_hash_base / rtc_hit_hash), restated here; the hits are each side's own.
  static uint64_t mix64(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }
  static uint64_t hit_hash(uint64_t t_bits, int32_t prim, int32_t push, int depth, int kind) {
    uint64_t base = mix64(t_bits) ^ ((((uint64_t)(uint32_t)prim << 32) | (uint64_t)(uint32_t)push) * 0x9E3779B97F4A7C15ull);
    return mix64(base ^ ((uint64_t)(((unsigned)depth << 8) | (unsigned)kind) + 1ull) * 0xD6E8FEB86659FD93ull);
  }
  struct Ctx {
    Intersections xs;
    bool nan_seen = false;
    Counters* counters = nullptr;
    int fuel0 = FUEL;
    // digest channel
    uint64_t* digest = nullptr;                                    // this pixel's accumulator (nullptr = off)
    const std::vector<std::pair<size_t, int32_t>>* id2seq = nullptr;  // shape id -> DFS sequence number (sorted)
    int repeat = 0;      // > 0: inside a subtree the reference re-traces for a light other than the first
    int next_kind = 0;   // kind of the ray the next color_at call traces
  };
#ifdef ORC_EXT
  Color shade_hit_ext(const State& st, int fuel, Ctx& c) const;
  Color miss_color_ext(const Ray& ray, int fuel, const Ctx& c) const;
#endif

  void intersect(const Ray& ray, Ctx& c) const {  // :18-24
    c.xs.clear();
    for (auto& e : elements) e->intersect(ray, c.xs, &c.nan_seen);
  }
  bool is_shadowed(const PointLight& light, const Vector& point, Ctx& c, int depth = 0) const {  // :26-48
    if (c.counters && depth < Counters::MAXD) {
      c.counters->shadow[depth]++;
      if (c.repeat == 0) c.counters->u_shadow[depth]++;
    }
    Vector v = light.origin - point;
    double distance = v.magnitude();
    Ray ray{point, v.normalize()};
    intersect(ray, c);
    sort_intersections(c.xs, &c.nan_seen);
    const Intersection* h = hit(c.xs);
    return h ? (h->shape->casts_shadow && h->t < distance) : false;
  }
  Color shade_hit(const State& st, int fuel, Ctx& c) const {  // :50-82
#ifdef ORC_EXT
    if (ext) return shade_hit_ext(st, fuel, c);
#endif
    Color color = Color::black();
    int depth = c.fuel0 - fuel;
    bool first_light = true;
    for (auto& light : lights) {
      bool shadowed = is_shadowed(light, st.over_point, c, depth < 0 ? 0 : depth);
      Color surface = st.shape->lighting(light, st.over_point, st.eye, st.normal, shadowed);
      if (!first_light) c.repeat++;   // (digest channel only: marks the re-traced copies)
      Color reflected = reflected_color(st, fuel, c);
      Color refracted = refracted_color(st, fuel, c);
      if (!first_light) c.repeat--;
      first_light = false;
      Color extra = (st.shape->material.reflective > 0.0 && st.shape->material.transparency > 0.0)
                        ? reflected * st.reflectance + refracted * (1.0 - st.reflectance)
                        : reflected + refracted;
      color = color + (surface + extra);
    }
    return color;
  }
  Color reflected_color(const State& st, int fuel, Ctx& c) const {  // :84-102
    if (fuel <= 0 || st.shape->material.reflective == 0.0) return Color::black();
    Ray r{st.over_point, st.reflect};
    c.next_kind = 1;
    return color_at(r, fuel - 1, c) * st.shape->material.reflective;
  }
  Color refracted_color(const State& st, int fuel, Ctx& c) const {  // :104-132
    if (fuel <= 0 || st.shape->material.transparency == 0.0) return Color::black();
    double n_ratio = st.n1 / st.n2;
#if defined(ORC_EXT) && ORC_EXT_MUTANT == 11
    double cos_i = st.eye.dot(st.geo_normal);
#else
    double cos_i = st.eye.dot(st.normal);
#endif
    double sin2_t = (n_ratio * n_ratio) * (1.0 - cos_i * cos_i);
    if (sin2_t > 1.0) return Color::black();
    double cos_t = std::sqrt(1.0 - sin2_t);
#if defined(ORC_EXT) && ORC_EXT_MUTANT == 11
    Vector direction = st.geo_normal * (n_ratio * cos_i - cos_t) - st.eye * n_ratio;
#else
    Vector direction = st.normal * (n_ratio * cos_i - cos_t) - st.eye * n_ratio;
#endif
    Ray r{st.under_point, direction};
    c.next_kind = 2;
    return color_at(r, fuel - 1, c) * st.shape->material.transparency;
  }
  // :134-149.  `first` (optional) receives the nearest-hit record of THIS call.
  Color color_at(const Ray& ray, int fuel, Ctx& c, Intersection* first = nullptr, bool* did_hit = nullptr) const {
    int depth = c.fuel0 - fuel;
    const bool counted = c.counters && depth >= 0 && depth < Counters::MAXD;
    if (counted) {
      c.counters->color_at[depth]++;
      if (c.repeat == 0) (c.next_kind == 0 ? c.counters->u_primary : c.next_kind == 1 ? c.counters->u_reflect : c.counters->u_refract)[depth]++;
    }
    intersect(ray, c);
    sort_intersections(c.xs, &c.nan_seen);
    const Intersection* h = hit(c.xs);
    if (did_hit) *did_hit = (h != nullptr);
    if (c.digest && c.repeat == 0) {
      uint64_t tb = 0;
      int32_t seq = -1, push = 0;
      if (h) {
        std::memcpy(&tb, &h->t, 8);
        auto it = std::lower_bound(c.id2seq->begin(), c.id2seq->end(), std::make_pair(h->shape->id, (int32_t)INT32_MIN));
        seq = (it != c.id2seq->end() && it->first == h->shape->id) ? it->second : -2;
        push = h->push_idx;
      }
      *c.digest += hit_hash(tb, seq, push, depth, c.next_kind);
    }
    if (h) {
      Intersection self = *h;
      if (first) *first = self;
      State st = prepare_state(self, ray, c.xs);
      // n1 / n2 reach a result only through schlick's blend and refracted_color (:70-78, :110): a transparent material, fuel left, and
      // a light to run shade_hit's loop for
      if (counted && c.repeat == 0 && self.shape->material.transparency != 0.0 && fuel > 0 && !lights.empty()) c.counters->u_container[depth]++;
      return shade_hit(st, fuel, c);
    }
#ifdef ORC_EXT
    if (ext) return miss_color_ext(ray, fuel, c);
#endif
    return Color::black();
  }

  // DFS numbering of primitives (world.elements order, children in order): the sequence number the
  // parity channel reports.  Not a reference concept; insertion order of intersections follows it.
  void number_shapes(std::vector<const Shape*>& out) const {
    struct R {
      static void go(const Element* e, std::vector<const Shape*>& o) {
        if (e->is_group) for (auto& c : e->children) go(c.get(), o);
        else o.push_back(&e->shape);
      }
    };
    for (auto& e : elements) R::go(e.get(), out);
  }
};

// ---------------------------------------------------------------- camera.rs
struct Camera {
  size_t hsize, vsize;
  double field_of_view;
  Matrix transform_inv;
  double pixel_size, half_width, half_height;
  static Camera make(size_t hsize, size_t vsize, double fov, const Matrix& transform) {  // :16-37
    Camera c;
    double half_view = std::tan(fov / 2.0);
    double aspect = (double)hsize / (double)vsize;
    if (aspect >= 1.0) { c.half_width = half_view; c.half_height = half_view / aspect; }
    else { c.half_width = half_view * aspect; c.half_height = half_view; }
    c.pixel_size = (c.half_width * 2.0) / (double)hsize;
    c.hsize = hsize; c.vsize = vsize; c.field_of_view = fov;
    c.transform_inv = transform.inverse_or_die();
    return c;
  }
  Ray ray_at_pixel(size_t x, size_t y) const {  // :39-55
    double xoffset = ((double)x + 0.5) * pixel_size;
    double yoffset = ((double)y + 0.5) * pixel_size;
    double world_x = half_width - xoffset;
    double world_y = half_height - yoffset;
    Vector pixel = transform_inv * Vector::point(world_x, world_y, -1.0);
    Vector origin = Vector::point(transform_inv.m[0][3], transform_inv.m[1][3], transform_inv.m[2][3]);
    Vector direction = (pixel - origin).normalize();
    return {origin, direction};
  }
  static Matrix view_transform(Vector from, Vector to, Vector up) {  // Camera::transform :57-73
    Vector forward = (to - from).normalize();
    Vector upn = up.normalize();
    Vector left = forward.cross(upn);
    Vector true_up = left.cross(forward);
    Matrix o = Matrix::id();
    o.m[0][0] = left.x; o.m[0][1] = left.y; o.m[0][2] = left.z;
    o.m[1][0] = true_up.x; o.m[1][1] = true_up.y; o.m[1][2] = true_up.z;
    o.m[2][0] = -forward.x; o.m[2][1] = -forward.y; o.m[2][2] = -forward.z;
    return o * Matrix::translation(-from.x, -from.y, -from.z);
  }
};

// ---------------------------------------------------------------- image.rs
struct HitRecord {  // parity channel: nearest hit of the primary ray
  double t;
  int32_t prim;  // DFS sequence number, -1 = miss
  int32_t push_idx;
};

struct RenderResult {
  bool nan_seen = false;
  Counters counters;
  double seconds = 0.0;
};

// image.rs:65-81 over an arbitrary list of pixel indices (i -> x = i % hsize, y = i / hsize), on
// `threads` std::threads with dynamic chunking (stands in for rayon's work-stealing par_iter).
inline RenderResult render_pixels(const Camera& cam, const World& world, int fuel, const uint64_t* indices, size_t n,
                                  double* rgb, HitRecord* hits, unsigned threads, uint64_t* digest = nullptr) {
  std::vector<const Shape*> order;
  world.number_shapes(order);
  std::vector<std::pair<size_t, int32_t>> id2seq;
  id2seq.reserve(order.size());
  for (size_t k = 0; k < order.size(); k++) id2seq.push_back({order[k]->id, (int32_t)k});
  std::sort(id2seq.begin(), id2seq.end());
  auto seq_of = [&](const Shape* s) -> int32_t {
    auto it = std::lower_bound(id2seq.begin(), id2seq.end(), std::make_pair(s->id, (int32_t)INT32_MIN));
    return (it != id2seq.end() && it->first == s->id) ? it->second : -2;
  };
  if (threads == 0) threads = std::max(1u, std::thread::hardware_concurrency());
  std::atomic<size_t> next{0};
  const size_t chunk = 256;
  std::vector<Counters> per(threads);
  std::atomic<bool> nan_any{false};
  auto worker = [&](unsigned tid) {
    World::Ctx c;
    c.counters = &per[tid];
    c.fuel0 = fuel;
    for (;;) {
      size_t b = next.fetch_add(chunk);
      if (b >= n) break;
      size_t e = std::min(n, b + chunk);
      for (size_t q = b; q < e; q++) {
        uint64_t i = indices ? indices[q] : (uint64_t)q;
        size_t x = (size_t)(i % cam.hsize), y = (size_t)(i / cam.hsize);
        Ray ray = cam.ray_at_pixel(x, y);
        World::Ctx fresh;  // `&mut vec![]` per pixel (image.rs:72)
        fresh.counters = c.counters;
        fresh.fuel0 = fuel;
        if (digest) { digest[q] = 0; fresh.digest = &digest[q]; fresh.id2seq = &id2seq; fresh.next_kind = 0; }
        Intersection first{};
        bool did = false;
        Color col = world.color_at(ray, fuel, fresh, &first, &did);
        if (fresh.nan_seen) nan_any = true;
        if (rgb) { rgb[3 * q + 0] = col.r; rgb[3 * q + 1] = col.g; rgb[3 * q + 2] = col.b; }
        if (hits) {
          if (did) hits[q] = {first.t, seq_of(first.shape), first.push_idx};
          else hits[q] = {0.0, -1, 0};
        }
      }
    }
  };
  auto t0 = std::chrono::steady_clock::now();
  if (threads == 1) worker(0);
  else {
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; t++) pool.emplace_back(worker, t);
    for (auto& th : pool) th.join();
  }
  RenderResult rr;
  rr.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (auto& p : per) rr.counters.add(p);
  rr.nan_seen = nan_any;
  return rr;
}

// image.rs:93-112 — P3 writer: header, <=5 pixels per line, newline at each row start.
inline std::string ppm(size_t hsize, size_t vsize, const double* rgb) {
  std::string out = "P3\n" + std::to_string(hsize) + " " + std::to_string(vsize) + "\n255";
  size_t j = 0;
  for (size_t i = 0; i < hsize * vsize; i++) {
    unsigned r = Color::clamp1(rgb[3 * i]), g = Color::clamp1(rgb[3 * i + 1]), b = Color::clamp1(rgb[3 * i + 2]);
    std::string px = std::to_string(r) + " " + std::to_string(g) + " " + std::to_string(b);
    if (i % hsize == 0 || j % 5 == 0) { out += "\n" + px; j = 1; }
    else { out += " " + px; j += 1; }
  }
  out += "\n";
  return out;
}

// ---------------------------------------------------------------- obj.rs
// Loader with the reference's line grammar (obj.rs:54-149) and assembly rules (:186-258).
struct ObjResult {
  ElementPtr element;
  std::vector<std::pair<uint32_t, std::string>> ignored;
  size_t triangles = 0;
  std::string error;
};

namespace objdetail {
inline bool space1(const char*& p) {  // nom space1: one or more ' ' or '\t'
  const char* q = p;
  while (*q == ' ' || *q == '\t') q++;
  if (q == p) return false;
  p = q;
  return true;
}
// nom number::complete::double — recognise [+-]? (digits[.digits?] | .digits) ([eE][+-]?digits)? then parse.
inline bool parse_double(const char*& p, double* out) {
  const char* q = p;
  if (*q == '+' || *q == '-') q++;
  const char* ds = q;
  while (*q >= '0' && *q <= '9') q++;
  bool int_digits = q > ds;
  bool frac_digits = false;
  if (*q == '.') {
    const char* f = q + 1;
    while (*f >= '0' && *f <= '9') f++;
    frac_digits = f > q + 1;
    if (int_digits || frac_digits) q = f;
  }
  if (!int_digits && !frac_digits) return false;
  if (*q == 'e' || *q == 'E') {
    const char* e = q + 1;
    if (*e == '+' || *e == '-') e++;
    const char* es = e;
    while (*e >= '0' && *e <= '9') e++;
    if (e > es) q = e;
  }
  std::string tok(p, q);
  *out = std::strtod(tok.c_str(), nullptr);
  p = q;
  return true;
}
inline bool parse_usize(const char*& p, size_t* out) {  // digit1 + parse::<usize>
  const char* q = p;
  size_t v = 0;
  while (*q >= '0' && *q <= '9') { v = v * 10 + (size_t)(*q - '0'); q++; }
  if (q == p) return false;
  *out = v;
  p = q;
  return true;
}
struct VN { size_t v; bool has_n; size_t n; };
inline bool parse_face_item(const char*& p, VN* out) {  // :92-112
  const char* q = p;
  size_t v;
  if (!parse_usize(q, &v)) return false;
  const char* after_v = q;
  if (*q == '/') {  // triplet: v '/' anything-up-to '/' n
    const char* r = q + 1;
    while (*r && *r != '/') r++;
    if (*r == '/') {
      r++;
      size_t n;
      if (parse_usize(r, &n)) {
        *out = {v, true, n};
        p = r;
        return true;
      }
    }
  }
  *out = {v, false, 0};
  p = after_v;
  return true;
}
}  // namespace objdetail

inline ObjResult parse_obj_stream(std::istream& in, const Matrix& transform, const Material& material) {
  using namespace objdetail;
  ObjResult res;
  std::vector<Vector> vertices, normals;
  // HashMap<String, Vec<Element>> in the reference (:196); iteration order there is arbitrary
  // (SURVEY Q13).  Here: first-seen order, "Default" first.
  std::vector<std::pair<std::string, std::vector<ElementPtr>>> groups;
  groups.emplace_back(std::string("Default"), std::vector<ElementPtr>());
  size_t cur = 0;
  Geometry dummy;
  std::string line;
  uint32_t n = 1;
  auto ignore = [&](const std::string& l) { res.ignored.push_back({n, l}); };
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    const char* p = line.c_str();
    bool done = false;
    // parse_vertex (:54-70)
    if (!done && p[0] == 'v') {
      const char* q = p + 1;
      double x, y, z;
      if (space1(q) && parse_double(q, &x) && space1(q) && parse_double(q, &y) && space1(q) && parse_double(q, &z)) {
        vertices.push_back(Vector::point(x, y, z));
        done = true;
      }
    }
    // parse_normal (:72-88)
    if (!done && p[0] == 'v' && p[1] == 'n') {
      const char* q = p + 2;
      double x, y, z;
      if (space1(q) && parse_double(q, &x) && space1(q) && parse_double(q, &y) && space1(q) && parse_double(q, &z)) {
        normals.push_back(Vector::vector(x, y, z));
        done = true;
      }
    }
    // parse_faces (:125-136) + triangulate (:114-123)
    if (!done && p[0] == 'f') {
      const char* q = p + 1;
      if (space1(q)) {
        std::vector<VN> idx;
        VN it;
        const char* r = q;
        if (parse_face_item(r, &it)) {
          idx.push_back(it);
          for (;;) {
            const char* s = r;
            if (!space1(s)) break;
            if (!parse_face_item(s, &it)) break;
            idx.push_back(it);
            r = s;
          }
        }
        if (idx.empty()) {
          res.error = "line " + std::to_string(n) + ": face with no indices (reference underflows, src/obj.rs:118)";
          return res;
        }
        for (size_t i = 1; i + 1 < idx.size(); i++) {
          VN a = idx[0], b = idx[i], c = idx[i + 1];
          auto vtx = [&](size_t k, Vector* o) { if (k < 1 || k > vertices.size()) return false; *o = vertices[k - 1]; return true; };
          auto nrm = [&](size_t k, Vector* o) { if (k < 1 || k > normals.size()) return false; *o = normals[k - 1]; return true; };
          Vector p1, p2, p3;
          if (!vtx(a.v, &p1) || !vtx(b.v, &p2) || !vtx(c.v, &p3)) {
            res.error = "line " + std::to_string(n) + ": vertex index out of range (src/obj.rs:209-214)";
            return res;
          }
          Geometry g;
          if (a.has_n && b.has_n && c.has_n) {
            Vector n1, n2, n3;
            if (!nrm(a.n, &n1) || !nrm(b.n, &n2) || !nrm(c.n, &n3)) {
              res.error = "line " + std::to_string(n) + ": normal index out of range (src/obj.rs:212-214)";
              return res;
            }
            g = Shape::smooth_triangle_geometry(p1, p2, p3, n1, n2, n3);
          } else {
            g = Shape::triangle_geometry(p1, p2, p3);
          }
          groups[cur].second.push_back(Element::primitive(Shape::make(Matrix::id(), Material(), true, g)));
          res.triangles++;
        }
        done = true;
      }
    }
    // parse_group (:138-149)
    if (!done && p[0] == 'g') {
      const char* q = p + 1;
      if (space1(q)) {
        const char* s = q;
        while ((*s >= '0' && *s <= '9') || (*s >= 'a' && *s <= 'z') || (*s >= 'A' && *s <= 'Z')) s++;
        if (s > q) {
          std::string name(q, s);
          size_t k = 0;
          for (; k < groups.size(); k++)
            if (groups[k].first == name) break;
          if (k == groups.size()) groups.emplace_back(name, std::vector<ElementPtr>());
          cur = k;
          done = true;
        }
      }
    }
    if (!done) ignore(line);
    n++;
  }
  std::vector<ElementPtr> elements;
  for (auto& g : groups)
    if (!g.second.empty())
      elements.push_back(Element::composite(transform, &material, Aggregation, std::move(g.second)));
  if (elements.size() == 1) res.element = std::move(elements[0]);
  else res.element = Element::composite(Matrix::id(), nullptr, Aggregation, std::move(elements));
  return res;
}
inline ObjResult parse_obj_file(const std::string& path, const Matrix& transform, const Material& material) {
  std::ifstream f(path);
  if (!f) {
    ObjResult r;
    r.error = "cannot open " + path;
    return r;
  }
  return parse_obj_stream(f, transform, material);
}

}  // namespace orc

#ifdef ORC_EXT
#include "rt_oracle_ext.hpp"  // liboracle_ext.so only: the extensions' bodies
#endif

// tests/cpu_emu/threads_tsan.cpp — TEST INFRASTRUCTURE.
// The product's HOST build (rtw_capi.cpp, host_scene.hpp, scene_build.hpp, bvh_build.hpp) driven from several threads at once under
// ThreadSanitizer: `make tsan` compiles this program and the emulator library with -fsanitize=thread into _build_tsan/.
//
//   threads_tsan <teapot_low.obj> [n_threads]     every thread builds its own worlds through rtw.h and has each flattened and built by
//                                                 rtw_render with an index list of length 0 (the whole host path runs, no kernel does);
//                                                 then the main thread alone renders every world and compares its frame with the one it
//                                                 rendered before any thread started: "same bits: <world>" per world and thread
//   threads_tsan --racy                           two threads increment one unguarded int: the run ThreadSanitizer must report
//
// The emulated kernels are never run on two threads: the shim's gridDim / blockIdx / threadIdx are globals and __shared__ arrays are
// function statics, so concurrent emulated renders race by construction of the emulator, not of the product.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/rtw.h"

namespace {

const double ID[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
struct M { double m[16]; };
M translation(double x, double y, double z) { M r; std::memcpy(r.m, ID, sizeof(ID)); r.m[3] = x; r.m[7] = y; r.m[11] = z; return r; }
M scaling(double x, double y, double z) { M r; std::memcpy(r.m, ID, sizeof(ID)); r.m[0] = x; r.m[5] = y; r.m[10] = z; return r; }
M rotation_y(double a) { M r; std::memcpy(r.m, ID, sizeof(ID)); r.m[0] = std::cos(a); r.m[2] = std::sin(a); r.m[8] = -std::sin(a); r.m[10] = std::cos(a); return r; }
M rotation_x(double a) { M r; std::memcpy(r.m, ID, sizeof(ID)); r.m[5] = std::cos(a); r.m[6] = -std::sin(a); r.m[9] = std::sin(a); r.m[10] = std::cos(a); return r; }
M operator*(const M& a, const M& b) {
  M r;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s += a.m[4 * i + k] * b.m[4 * k + j];
      r.m[4 * i + j] = s;
    }
  return r;
}

[[noreturn]] void die(const char* what) {
  std::fprintf(stderr, "threads_tsan: %s: %s\n", what, rtw_last_error());
  std::exit(2);
}
template <class T> T* must(T* p, const char* what) { if (!p) die(what); return p; }
void must0(int rc, const char* what) { if (rc != 0) die(what); }

rtw_material material(const rtw_pattern* p, double reflective = 0.0, double transparency = 0.0) {
  return rtw_material{0.1, 0.7, 0.3, 200.0, reflective, transparency, 1.5, p};
}

// A view from (0.5, 1.2, -5.5) towards the origin, written out: the inverse of a translation, no matrix inversion of our own involved.
rtw_camera camera(uint64_t h, uint64_t v) {
  rtw_camera c{};
  c.hsize = h; c.vsize = v; c.field_of_view = 1.1;
  const M t = rotation_x(-0.15) * translation(-0.5, -1.2, 5.5);
  std::memcpy(c.transform, t.m, sizeof(t.m));
  return c;
}

void lights(rtw_world* w) {
  const double i0[3] = {1.0, 1.0, 1.0}, o0[3] = {-4.0, 6.5, -5.0}, i1[3] = {0.3, 0.3, 0.45}, o1[3] = {5.0, 4.0, -3.0};
  must0(rtw_world_add_light(w, i0, o0), "add_light");
  must0(rtw_world_add_light(w, i1, o1), "add_light");
}

void add_floor(rtw_world* w, const rtw_pattern* p) {
  const rtw_material m = material(p, 0.2);
  must0(rtw_world_add_element(w, must(rtw_shape(RTW_PLANE, ID, &m, 1, nullptr, 0), "plane")), "add_element");
}

// Patterns (checkers of a stripe mixture and a jittered ring), a CSG difference, an aggregation group of eight shapes (an analytic BVH).
rtw_world* small_world() {
  rtw_world* w = must(rtw_world_create(), "world");
  lights(w);
  rtw_pattern* a = must(rtw_pattern_plain(0.9, 0.2, 0.1), "plain");
  rtw_pattern* b = must(rtw_pattern_plain(0.1, 0.3, 0.9), "plain");
  rtw_pattern* stripes = must(rtw_pattern_mixture(RTW_STRIPES, scaling(0.25, 0.25, 0.25).m, a, b), "stripes");
  rtw_pattern* ring = must(rtw_pattern_mixture(RTW_RING, scaling(0.2, 0.2, 0.2).m, b, a), "ring");
  rtw_pattern* jit = must(rtw_pattern_jitter(RTW_JITTER_POINT, RTW_NOISE_SIMPLEX, 0.3, 1, ring), "jitter");
  rtw_pattern* checks = must(rtw_pattern_mixture(RTW_CHECKERS, scaling(0.7, 0.7, 0.7).m, stripes, jit), "checkers");
  add_floor(w, checks);
  const rtw_material ma = material(a, 0.3), mb = material(b, 0.1, 0.6), mc = material(checks);
  rtw_element* carve[2] = {must(rtw_shape(RTW_CUBE, ID, &ma, 1, nullptr, 0), "cube"), must(rtw_shape(RTW_SPHERE, scaling(1.3, 1.3, 1.3).m, &mb, 1, nullptr, 0), "sphere")};
  must0(rtw_world_add_element(w, must(rtw_composite((translation(0.0, 0.5, -1.0) * rotation_y(0.5) * scaling(0.5, 0.5, 0.5)).m, nullptr, RTW_DIFFERENCE, carve, 2), "difference")),
        "add_element");
  std::vector<rtw_element*> kids;
  for (int i = 0; i < 8; i++) {
    const double ang = 0.785398 * i + 0.3;
    const M t = translation(1.9 * std::cos(ang), 0.6 + 0.3 * (i % 3), 1.4 * std::sin(ang)) * scaling(0.5, 0.5, 0.5);
    const double cyl[3] = {-0.8, 0.9, 1.0};
    kids.push_back(i % 4 == 3 ? must(rtw_shape(RTW_CYLINDER, t.m, &mc, 1, cyl, 3), "cylinder") : must(rtw_shape(RTW_SPHERE, t.m, i % 2 ? &ma : &mb, 1, nullptr, 0), "sphere"));
  }
  must0(rtw_world_add_element(w, must(rtw_composite((translation(0.0, 0.05, 0.1) * rotation_y(0.2)).m, nullptr, RTW_AGGREGATION, kids.data(), kids.size()), "group")), "add_element");
  for (rtw_pattern* p : {checks, jit, ring, stripes, b, a}) rtw_pattern_release(p);
  return w;
}

rtw_world* mesh_world(const std::string& obj, const M& t, uint64_t want_tris) {
  rtw_world* w = must(rtw_world_create(), "world");
  lights(w);
  rtw_pattern* grey = must(rtw_pattern_plain(0.6, 0.6, 0.55), "plain");
  rtw_pattern* blue = must(rtw_pattern_plain(0.3, 0.7, 0.9), "plain");
  add_floor(w, grey);
  const rtw_material m = material(blue, 0.2);
  uint64_t ignored = 0, tris = 0;
  rtw_element* e = must(rtw_parse_obj(obj.c_str(), t.m, &m, &ignored, &tris), "parse_obj");
  if (want_tris && tris != want_tris) { std::fprintf(stderr, "threads_tsan: %s holds %llu triangles, not %llu\n", obj.c_str(), (unsigned long long)tris, (unsigned long long)want_tris); std::exit(2); }
  must0(rtw_world_add_element(w, e), "add_element");
  rtw_pattern_release(blue);
  rtw_pattern_release(grey);
  return w;
}

// (n + 1)^2 vertices, 2 n^2 flat triangles in one group.  n = 256: 131 072 triangles -- halves far above the BVH builder's
// kParMin = 16384, and with the floor 131 073 primitives, past scene_build.hpp parallel_for's 2 * 65536: both thread pools start.
constexpr int GRID = 256;
std::string write_grid() {
  const char* dir = std::getenv("TMPDIR");
  std::string path = std::string(dir && *dir ? dir : "/tmp") + "/threads_tsan_grid_XXXXXX";
  const int fd = mkstemp(&path[0]);
  if (fd < 0) { std::perror("mkstemp"); std::exit(2); }
  FILE* f = fdopen(fd, "w");
  std::fprintf(f, "g Grid\n");
  for (int j = 0; j <= GRID; j++)
    for (int i = 0; i <= GRID; i++) {
      const double x = -1.0 + 2.0 * i / GRID, z = -1.0 + 2.0 * j / GRID;
      std::fprintf(f, "v %.17g %.17g %.17g\n", x, 0.25 * std::sin(3.0 * x + 0.5) * std::cos(2.5 * z) + 0.002 * ((i * 31 + j * 17) % 7), z);
    }
  for (int j = 0; j < GRID; j++)
    for (int i = 0; i < GRID; i++) {
      const int a = j * (GRID + 1) + i + 1;
      std::fprintf(f, "f %d %d %d\nf %d %d %d\n", a, a + GRID + 1, a + 1, a + 1, a + GRID + 1, a + GRID + 2);
    }
  std::fclose(f);
  return path;
}

struct Kind {
  const char* name;
  uint64_t h, v;
  int fuel;
};
const Kind KINDS[3] = {{"small", 24, 16, 5}, {"teapot", 16, 10, 3}, {"grid131072", 12, 8, 2}};

struct Paths { std::string teapot, grid; };

rtw_world* make(int kind, const Paths& p) {
  if (kind == 0) return small_world();
  if (kind == 1) return mesh_world(p.teapot, translation(0.2, 0.0, 0.3) * rotation_y(0.5) * rotation_x(-1.5707963267948966) * scaling(0.12, 0.12, 0.12), 0);
  return mesh_world(p.grid, translation(0.0, 0.7, 0.4) * rotation_x(-0.5) * scaling(1.8, 1.0, 1.4), 2ull * GRID * GRID);
}

struct Frame {
  std::vector<double> rgb;
  std::vector<rtw_hit> hits;
  bool same(const Frame& o) const {
    return rgb.size() == o.rgb.size() && hits.size() == o.hits.size() && std::memcmp(rgb.data(), o.rgb.data(), rgb.size() * sizeof(double)) == 0 &&
           std::memcmp(hits.data(), o.hits.data(), hits.size() * sizeof(rtw_hit)) == 0;
  }
};

Frame render(rtw_world* w, const Kind& k) {
  const rtw_camera c = camera(k.h, k.v);
  Frame f;
  f.rgb.assign(3 * k.h * k.v, -1.0);
  f.hits.resize(k.h * k.v);
  std::memset(f.hits.data(), 0xCD, f.hits.size() * sizeof(rtw_hit));   // (padding bytes included: the frames are compared as bytes)
  must0(rtw_render(w, &c, k.fuel, nullptr, k.h * k.v, f.rgb.data(), f.hits.data()), "rtw_render");
  return f;
}

// The whole host path of a world, no kernel: flatten, build_arrays, the BVHs and light grids.
void build_only(rtw_world* w, const Kind& k) {
  const rtw_camera c = camera(k.h, k.v);
  const uint64_t none = 0;
  must0(rtw_render(w, &c, k.fuel, &none, 0, nullptr, nullptr), "rtw_render (no pixels)");
}

int racy() {
  int shared = 0;   // deliberately unguarded
  auto bump = [&shared] { for (int i = 0; i < 100000; i++) shared = shared + 1; };
  std::thread a(bump), b(bump);
  a.join();
  b.join();
  std::printf("racy: %d\n", shared);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "--racy") == 0) return racy();
  if (argc < 2) { std::fprintf(stderr, "usage: threads_tsan <teapot_low.obj> [n_threads] | --racy\n"); return 2; }
  const int n_threads = argc >= 3 ? std::atoi(argv[2]) : 4;
  Paths paths{argv[1], write_grid()};

  // the frames to hold everything to: rendered before any thread exists
  Frame ref[3];
  for (int k = 0; k < 3; k++) {
    rtw_world* w = make(k, paths);
    ref[k] = render(w, KINDS[k]);
    rtw_world_release(w);
    double top = 0.0;
    for (double x : ref[k].rgb) top = std::fmax(top, x);
    if (!(top > 0.1)) { std::fprintf(stderr, "threads_tsan: the %s frame is black\n", KINDS[k].name); return 2; }
  }

  // every thread: its own three worlds, started at another kind each, so that builds of all sizes overlap
  std::vector<std::vector<rtw_world*>> worlds(n_threads, std::vector<rtw_world*>(3, nullptr));
  std::vector<std::thread> pool;
  for (int t = 0; t < n_threads; t++)
    pool.emplace_back([t, &worlds, &paths] {
      for (int j = 0; j < 3; j++) {
        const int k = (t + j) % 3;
        worlds[t][k] = make(k, paths);
        build_only(worlds[t][k], KINDS[k]);
      }
    });
  for (std::thread& th : pool) th.join();

  int bad = 0;
  for (int t = 0; t < n_threads; t++)
    for (int k = 0; k < 3; k++) {
      const bool same = render(worlds[t][k], KINDS[k]).same(ref[k]);   // (the scene built on thread t: rtw_render builds nothing now)
      std::printf("%s: %s (thread %d)\n", same ? "same bits" : "OTHER BITS", KINDS[k].name, t);
      bad += !same;
      rtw_world_release(worlds[t][k]);
    }
  unlink(paths.grid.c_str());
  return bad ? 1 : 0;
}

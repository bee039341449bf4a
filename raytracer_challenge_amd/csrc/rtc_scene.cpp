// rtc_scene.cpp — the rtc.h C ABI: validates a flattened scene, builds the traversal program + accelerator,
// uploads SoA buffers to HBM and launches the trace kernels.  There is no CPU execution path in this file:
// every entry point that computes pixels needs a HIP device and fails with RTC_ERR_DEVICE otherwise.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rtc.h"
#include "adaptive_contrast.h"
#include "background_point.h"
#include "bump_normal.h"
#include "camera_sampling.h"
#include "device_scene.h"
#include "filter_weights.h"
#include "scene_build.hpp"
#include "shutter_pose.h"
#include "spot_factor.h"
#include "uv_image.h"

void rtc_launch_trace(const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, double* rgb, double* hit_t, int* hit_prim, int* hit_k,
                      DStats* stats, bool count, hipStream_t stream, bool big_scene, const RtcSceneExt& X);
void rtc_launch_quantize(const double* rgb, unsigned char* out, unsigned long long n, hipStream_t stream);
void rtc_launch_pack_hits(const double* t, const int* prim, const int* k, DHit* out, unsigned long long n, hipStream_t stream);
void rtc_launch_deinterleave(const double* slab, double* image, unsigned rowlen, unsigned vsize, unsigned n, unsigned max_rows, unsigned band, hipStream_t stream);
void rtc_launch_deinterleave8(const unsigned char* slab, unsigned char* image, unsigned rowlen, unsigned vsize, unsigned n, unsigned max_rows, unsigned band, hipStream_t stream);
void rtc_launch_wavefront(const DScene& S, const DCamera& cam, const DPixelMap& pm, int fuel, const DWave& W, double* rgb, double* hit_t, int* hit_prim, int* hit_k,
                          DStats* stats, bool count, hipStream_t stream, unsigned blocks, unsigned shade_blocks, unsigned lds, unsigned lds_blocks, const RtcSceneExt& X);
void rtc_launch_bump_normals(const DScene& S, const DBumpTable& bt, const int32_t* prims, const double* points, const double* normals, unsigned long long n, double* out,
                             hipStream_t stream);
void rtc_launch_background_colors(const DScene& S, const DBackground& bg, const double* dirs, unsigned long long n, double* rgb, hipStream_t stream);
int rtc_ext_trace_build(const DScene& S, const RtcSceneExt& X);
void rtc_kernel_info_fill(const DScene& S, bool wavefront, bool count, bool big_scene, unsigned lds_bytes, int device, rtc_kernel_info* out);
bool rtc_scene_is_big(unsigned long long scene_bytes);
uint64_t rtc_wavefront_work(const DCamera& cam, const DPixelMap& pm);
unsigned rtc_wavefront_grid(const DScene& S, int n_cu);
unsigned rtc_wavefront_lds_grid(int n_cu, int spare);
int rtc_wavefront_spare_cus_default(int n_cu);
unsigned rtc_wavefront_lds_bytes(const DScene& S, bool enabled);
void rtc_launch_gen_rays(const DCamera& cam, const DPixelMap& pm, const rtc_sampling& sp, unsigned long long slot_first, unsigned long long n_slots, double* rays,
                         hipStream_t stream);
void rtc_launch_resolve_samples(const double* ray_rgb, unsigned n_samples, unsigned long long n_slots, double* dst, hipStream_t stream);
unsigned long long rtc_contrast_blocks(unsigned long long n);
unsigned long long rtc_contrast_work_words(unsigned long long n);
unsigned long long rtc_scan_work_words(unsigned long long n);
unsigned rtc_launch_scan(unsigned long long* v, unsigned long long n, unsigned long long* levels, unsigned long long* total, hipStream_t stream);
int rtc_cull_probe_doubles(int kind);
void rtc_launch_cull_probe(int kind, const double* records, unsigned long long n, unsigned char* out, hipStream_t stream);
unsigned rtc_launch_contrast_compact(const double* frame, unsigned long long hsize, unsigned long long vsize, double threshold, unsigned neighbours,
                                     unsigned long long* work, unsigned long long* list, unsigned long long* count, hipStream_t stream);
void rtc_launch_resolve_samples_scatter(const double* ray_rgb, unsigned n_samples, unsigned long long n_slots, const unsigned long long* indices, double* frame,
                                        hipStream_t stream);
unsigned rtc_launch_resolve_filtered(const rtc_filter& f, const rtc_sampling& sp, unsigned long long hsize, unsigned long long row0, unsigned long long row1,
                                     unsigned long long out0, unsigned long long out1, const double* samples, double* dst, hipStream_t stream, unsigned* tile);
unsigned long long rtc_shutter_work_words(unsigned long long m);
unsigned long long* rtc_shutter_offsets(unsigned long long* work, unsigned long long m);
unsigned rtc_launch_shutter_deal(const rtc_shutter& sh, const rtc_sampling& sp, unsigned K, const DPixelMap& pm, const DCamera& cam, unsigned long long slot_first,
                                 unsigned long long m, unsigned long long* work, unsigned* order, unsigned* where, hipStream_t stream);
void rtc_launch_shutter_gen_rays(const DCamera& cam, const DPixelMap& pm, const rtc_sampling& sp, unsigned long long slot_first, const unsigned* order, unsigned off, unsigned len,
                                 unsigned m, double* rays, hipStream_t stream);
void rtc_launch_shutter_resolve(const double* ray_rgb, const unsigned* where, unsigned n_samples, unsigned long long n_slots, double* dst, hipStream_t stream);
int32_t rtc_bvh_build_device(const std::vector<bvh::Item>& items, std::vector<DBvhNode>& n2, std::vector<uint32_t>& order, uint32_t base, int leaf_max, double* frame);
int32_t rtc_bvh_build_device_keys(const std::vector<bvh::Item>& items, std::vector<DBvhNode>& n2, std::vector<uint32_t>& order, uint32_t base, int leaf_max, double* frame,
                                  std::vector<unsigned long long>* keys);

static thread_local std::string g_rtc_err;
static int rtc_fail(int code, const std::string& m) {
  g_rtc_err = m;
  return code;
}
#define HIP_OK(expr)                                                                                     \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return rtc_fail(RTC_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct rtc_scene {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t marker[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool marker_recorded[8] = {false, false, false, false, false, false, false, false};
  std::vector<void*> allocs;
  uint64_t bytes = 0;
  DScene d{};
  bool has_bg = false;  // the scene has a background (rtc_scene_create_ext3): its launches take the BG builds (rtc_feat.hip RtcExt; rtc_background.hip)
  DBackground bg{0, 0};
  bool bg_plain = false;  // its root is a Plain colour: no pattern walk
  bool has_bump = false;  // the scene has bump records (rtc_scene_create_ext4): its launches take the NP builds (rtc_feat.hip RtcExt, wf_shade's)
  uint32_t n_bumps = 0;
  DBumpTable bump{nullptr, nullptr};
  RtcSceneExt ext() const { return RtcSceneExt{has_bg ? &bg : nullptr, has_bump ? &bump : nullptr}; }  // what the launchers take of the two
  DStats* d_stats = nullptr;
  // scratch output buffers (grown on demand)
  double* d_rgb = nullptr;
  double* d_hit_t = nullptr;
  int* d_hit_prim = nullptr;
  int* d_hit_k = nullptr;
  DHit* d_hits = nullptr;   // packed {t, prim, push} records for the copy to the host (rtc_hit layout)
  unsigned long long* d_digest = nullptr;    // hit-tree digests of a parity launch (per output slot)
  unsigned long long* d_wave_dig = nullptr;  //   and, wavefront path, the per-level hit hashes they are summed from
  uint64_t cap_digest = 0, cap_wave_dig = 0;
  uint8_t* d_rgb8 = nullptr;
  uint64_t cap_hits = 0, cap_rgb8 = 0;
  uint64_t* d_idx = nullptr;
  double* d_rays = nullptr;
  uint64_t cap_px = 0, cap_idx = 0, cap_rays = 0;
  // sampled camera (run_sampled): the sample rays of one chunk of pixels and their colours, reused chunk after chunk on the stream
  double* d_srays = nullptr;
  double* d_srgb = nullptr;
  uint64_t cap_srays = 0, cap_srgb = 0;
  hipEvent_t evs0 = nullptr, evs1 = nullptr;  // around a chunk's generator, traces and resolve
  // adaptive sampling (run_adaptive, rtc_contrast_pixels): the refined pixels' list (one slot per pixel of the largest frame so far),
  // the wave masks and scan levels of the compaction, the list's length
  unsigned long long* d_alist = nullptr;
  unsigned long long* d_awork = nullptr;
  unsigned long long* d_acount = nullptr;
  uint64_t cap_alist = 0;
  // the shutter (run_shutter, rtc_shutter_deal; this scene as scenes[0]): per sample of the largest chunk so far the pose-major list of
  // sample ids and each id's position in it; the pose-major count table, its scan levels and the offsets
  unsigned* d_shorder = nullptr;
  unsigned* d_shwhere = nullptr;
  unsigned long long* d_shwork = nullptr;
  uint64_t cap_shutter = 0;
  int kernel_version = 0;  // 0: measured choice between the one-kernel (1) and the wavefront (4) path, per launch signature
  uint64_t tune_sig = 0;
  double tune_ms[2] = {-1.0, -1.0};
  int tune_n[2] = {0, 0};
  int tune_choice = 0;
  // what the scene is made of, for the first-launch path guess (pick_path)
  uint32_t n_analytic = 0;      // bounded analytic primitives (the world BVH's leaves)
  uint32_t n_bouncing = 0;      // primitives whose material reflects or refracts
  uint32_t n_prims_total = 0;
  bool last_wavefront = false;  // path of the most recent launch (for stats read back after an asynchronous launch)
  int last_fuel = 0;
  DCsgHit* csg_slab = nullptr;  // CSG subtrees beyond the per-lane buffer: csg_max_hits rows per thread of the largest launch so far
  uint64_t csg_slab_threads = 0;
  bool wave_alloc_failed = false;  // the device refused the queues once: launches stay on the one-kernel path
  // wavefront path (RTC_KERNEL=4): queues and per-level arrays, grown on demand
  DWave wave{};
  void* wave_mem = nullptr;
  uint64_t wave_cap = 0;
  int wave_levels = 0;
  unsigned wave_blocks = 0, shade_blocks = 0;
  unsigned lds_bytes = 0;     // dynamic LDS of the wavefront traversal kernel (0: tables in memory; RTC_WF_LDS=0 at creation pins that)
  int n_cu = 1;               // CUs of the scene's device: the grid of the LDS-resident traversal build, less the spare ones (lds_grid below)
  int spare_cus = 0;          // CUs an unsynchronised launch of that build leaves to other scenes' kernels (RTC_WF_SPARE_CUS at creation, else the default)
  bool counted = false;       // the scene is in its device's count of live scenes (g_live_scenes)
  unsigned wave_eighths = 9;  // queue capacity per level, in eighths of the launch's level-0 work ids
  int bvh_depth = 0;
  int built_on_device = 0;  // mesh accelerators of this scene whose tree came from bvh_device.hip
  uint32_t n_bvh_nodes = 0, n_mesh_tris = 0;

  template <class T>
  int upload(const std::vector<T>& v, const T** out) {
    *out = nullptr;
    if (v.empty()) return RTC_OK;
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, v.size() * sizeof(T)));
    allocs.push_back(p);
    bytes += v.size() * sizeof(T);
    HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)p;
    return RTC_OK;
  }
};

namespace {

// Grows the device scratch buffers that share the capacity `*cap` to `need` elements; nothing happens (no wait either) when the
// capacity suffices.  Otherwise every buffer is freed and nulled and the capacity zeroed before the first hipMalloc, so that a failed
// allocation leaves a consistent scene.  `wait`: a stream whose queued work may still use the buffers, waited for before they are
// freed (the buffers a chunked launch reuses on the stream, the wavefront digests, the CSG slab).  The others pass none: they are
// written and read within one synchronous call, and hipFree (hipFree(nullptr) is a no-op) waits for the device anyway.
struct GrowBuf { void** p; uint64_t bytes; };
int grow(uint64_t* cap, uint64_t need, std::initializer_list<GrowBuf> bufs, hipStream_t wait = nullptr) {
  if (need <= *cap) return RTC_OK;
  if (wait) HIP_OK(hipStreamSynchronize(wait));
  for (const GrowBuf& b : bufs) { (void)hipFree(*b.p); *b.p = nullptr; }
  *cap = 0;
  for (const GrowBuf& b : bufs) HIP_OK(hipMalloc(b.p, b.bytes));
  *cap = need;
  return RTC_OK;
}

int ensure_px(rtc_scene* s, uint64_t n, bool hits) {
  int rc = grow(&s->cap_px, n, {{(void**)&s->d_rgb, n * 3 * sizeof(double)}, {(void**)&s->d_hit_t, n * sizeof(double)},
                                {(void**)&s->d_hit_prim, n * sizeof(int)}, {(void**)&s->d_hit_k, n * sizeof(int)}});
  if (rc == RTC_OK && hits) rc = grow(&s->cap_hits, n, {{(void**)&s->d_hits, n * sizeof(DHit)}});
  return rc;
}
// the quantised pixels of a launch whose caller wants bytes (render_to_host): n x 3
int ensure_rgb8(rtc_scene* s, uint64_t n) { return grow(&s->cap_rgb8, 3 * n, {{(void**)&s->d_rgb8, 3 * n}}); }
// d_rays for n explicit rays (or as many doubles of another kind): n x 6
int ensure_rays(rtc_scene* s, uint64_t n) { return grow(&s->cap_rays, n, {{(void**)&s->d_rays, n * 6 * sizeof(double)}}); }

// ---- device -> host for the caller's output buffers (Image::par_render returns host pixels, src/image.rs:76-80) ----------------
// Measured on the GPU box (scripts/d2h_probe.hip, profiles/r3_d2h_probe.txt): a pageable hipMemcpy runs at PCIe speed (52-56 GB/s,
// 1.0 ms per 50 MB) when the destination's pages exist and at 2.4 ms per 50 MB into a freshly allocated buffer (Vec / calloc /
// numpy.empty: the runtime pins the range, which faults its pages in in bulk).  What made round 2's rtc_render 13x slower than its
// kernels was everything around that copy: three temporary vectors and a scalar host loop for the hit records, and a host sync
// between the kernels and the first copy.  So: (1) hit records are packed on the device into the caller's layout; (2) one copy per
// output array, straight into the caller's memory, queued on the scene's stream behind the kernels.
// Touching the destination's pages from host threads while the device renders was measured too and is OFF by default
// (RTC_PRETOUCH_THREADS=n turns it on): 3.5 ms per 50 MB with 8 threads writing one byte per page (page faults of one address space
// serialise in the kernel) — and 22 ms when the page was read first (zero page mapped, then a second, copy-on-write fault).
void pretouch_pages(void* p, size_t bytes, std::vector<std::thread>* pool) {
  if (!p || bytes < (4u << 20)) return;
  static const int T = [] { const char* e = std::getenv("RTC_PRETOUCH_THREADS"); int t = e ? std::atoi(e) : 0; return t < 0 ? 0 : (t > 32 ? 32 : t); }();
  if (T == 0) return;
  char* base = (char*)p;
  const size_t per = ((bytes / (size_t)T) + 4095) & ~(size_t)4095;
  for (int t = 0; t < T; t++) {
    const size_t b = std::min(bytes, per * (size_t)t), e = std::min(bytes, per * (size_t)(t + 1));
    if (e > b) pool->emplace_back([base, b, e] { for (size_t o = b; o < e; o += 4096) { volatile char* q = base + o; *q = 0; } });
  }
}
void join_all(std::vector<std::thread>* pool) {
  for (auto& t : *pool) t.join();
  pool->clear();
}

// Sizes the wavefront arrays for `n_work` level-0 work ids and fuel + 1 levels: every level may hold up to wave_eighths / 8 x
// n_work rays (1.125 x to start with: a level larger than the frame's work ids needs most hits to spawn two rays).  A level that
// needs more sets the overflow flag; a synchronous launch then doubles the factor and renders again while the arrays stay
// under RTC_WF_MAX_BYTES (default 24 GiB), else falls back to the one-kernel path.
uint64_t wave_cap(uint64_t n_work, unsigned eighths) { return std::max<uint64_t>((n_work * eighths + 7) / 8, 4096); }
uint64_t wave_bytes(uint64_t cap, int lv) { return dwave_bytes(cap, lv); }
uint64_t wave_budget() {
  const char* e = std::getenv("RTC_WF_MAX_BYTES");
  return e ? std::strtoull(e, nullptr, 10) : (24ull << 30);
}
int ensure_wave(rtc_scene* s, uint64_t n_work, int fuel) {
  const int levels = fuel + 1;
  uint64_t cap = wave_cap(n_work, s->wave_eighths);
  if (cap > 0x7fffff00ull || wave_bytes(cap, levels) > wave_budget()) return rtc_fail(RTC_ERR_UNSUPPORTED, "launch too large for the wavefront path");
  if (cap <= s->wave_cap && levels <= s->wave_levels) return RTC_OK;
  cap = std::max(cap, s->wave_cap);
  const int lv = std::max(levels, s->wave_levels);
  HIP_OK(hipStreamSynchronize(s->stream));
  if (s->wave_mem) (void)hipFree(s->wave_mem);
  s->wave_mem = nullptr; s->wave_cap = 0; s->wave_levels = 0;
  {
    // other owners of the device's memory (a host framework's allocator, other scenes) are not in the budget: ask the device
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && wave_bytes(cap, lv) > (uint64_t)free_b)
      return rtc_fail(RTC_ERR_UNSUPPORTED, "the wavefront queues do not fit the device's free memory");
    const hipError_t e = std::getenv("RTC_WF_FAIL_ALLOC") ? hipErrorOutOfMemory : hipMalloc(&s->wave_mem, wave_bytes(cap, lv));  // env: test hook
    if (e != hipSuccess) {
      (void)hipGetLastError();  // clear the sticky error: the launch continues on the one-kernel path
      s->wave_mem = nullptr;
      if (e == hipErrorOutOfMemory) return rtc_fail(RTC_ERR_UNSUPPORTED, "hipMalloc of the wavefront queues: out of memory");
      return rtc_fail(RTC_ERR_DEVICE, std::string("hipMalloc of the wavefront queues: ") + hipGetErrorString(e));
    }
  }
  dwave_carve(&s->wave, s->wave_mem, cap, lv);
  s->wave_cap = cap;
  s->wave_levels = lv;
  return RTC_OK;
}

void to_dcam(const rtc_camera& c, DCamera* d) {
  d->hsize = c.hsize; d->vsize = c.vsize;
  d->half_width = c.half_width; d->half_height = c.half_height; d->pixel_size = c.pixel_size;
  std::memcpy(d->inv, c.transform_inv, sizeof(d->inv));
}

// Signature of a launch for the path choice below: everything the ray counts of a frame depend on besides the scene.
uint64_t launch_signature(const DCamera& cam, const DPixelMap& pm, int fuel) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; } };
  mix(&cam, sizeof(cam));
  mix(&pm.n, sizeof(pm.n)); mix(&pm.mode, sizeof(pm.mode)); mix(&pm.row_first, sizeof(pm.row_first)); mix(&pm.row_step, sizeof(pm.row_step)); mix(&pm.band, sizeof(pm.band));
  mix(&fuel, sizeof(fuel));
  return h ? h : 1;
}

// Which path renders a launch (RTC_KERNEL unset).  The one-kernel path wins where rays are cheap (planes + one gated mesh:
// the teapot scenes, 0.85 vs 1.5 ms), the wavefront path where a ray walks a BVH of analytic primitives and the ray trees
// are deep (config 2: 2.3 vs 4.2 ms); which one depends on scene, camera and fuel, so the choice is measured where it can be:
// for a given launch signature the first four SYNCHRONOUS launches alternate between the paths, starting with the guess below (the
// smaller of a path's two times counts), and every later launch — synchronous or not — takes the faster.  Until a signature is
// measured, and for a caller that renders one frame per scene (the reference's only call pattern, src/bin/*.rs), the guess decides:
// first_guess() — wavefront iff the scene has an analytic BVH worth walking (>= 32 bounded analytic primitives), a tenth of its
// primitives reflect or refract, the frame is large enough to fill per-level launches and fuel allows bounces; else one kernel,
// which also never allocates ray queues.  (Calibrated on the nine reference scenes and the five BASELINE configs:
// profiles/r3_path_choice.txt.)  A wavefront launch whose queues overflowed is rendered again by the one-kernel path and never chosen for
// that signature, so an unsynchronised wavefront launch only ever repeats a launch that is known to fit.
int first_guess(const rtc_scene* s, uint64_t n_work, int fuel) {
  if (const char* e = std::getenv("RTC_FIRST_GUESS")) { const int v = std::atoi(e); if (v == 1 || v == 4) return v; }
  const bool deep = fuel >= 2 && (uint64_t)s->n_bouncing * 10u >= (uint64_t)s->n_prims_total && s->n_bouncing > 0;
  return (s->n_analytic >= 32 && deep && n_work >= (256u << 10)) ? 4 : 1;
}
int pick_path(rtc_scene* s, uint64_t sig, uint64_t n_work, int fuel, bool will_sync, bool pixel_list) {
  if (sig != s->tune_sig) { s->tune_sig = sig; s->tune_ms[0] = s->tune_ms[1] = -1.0; s->tune_n[0] = s->tune_n[1] = 0; s->tune_choice = 0; }
  if (pixel_list) return 1;  // index lists and explicit rays: small, irregular launches
  if (s->tune_choice) return s->tune_choice;
  const int guess = first_guess(s, n_work, fuel);
  if (!will_sync) return guess;
  // two samples per path, alternating, the smaller one counts: a path's first launch pays for code loading and scratch
  const int other = guess == 4 ? 1 : 4;
  const int ng = s->tune_n[guess == 4 ? 1 : 0], no = s->tune_n[other == 4 ? 1 : 0];
  return ng <= no ? guess : other;
}
// The wavefront path is no candidate for the current signature any more (its queues were refused or overflowed): the choice is made.
void drop_wavefront(rtc_scene* s) { s->tune_ms[1] = 1e30; s->tune_n[1] = 2; s->tune_choice = 1; }
// One sample of pick_path's measurement: `ms` of a launch of the current signature on the one-kernel or the wavefront path.
void record_sample(rtc_scene* s, bool wavefront, double ms) {
  const int k = wavefront ? 1 : 0;
  s->tune_ms[k] = s->tune_n[k] ? std::min(s->tune_ms[k], ms) : ms;
  s->tune_n[k]++;
  if (s->tune_n[0] >= 2 && s->tune_n[1] >= 2) s->tune_choice = s->tune_ms[1] < s->tune_ms[0] ? 4 : 1;
}

// Scenes alive per device (up at the end of scene_create, down in rtc_scene_destroy): a scene's stream can overlap another's kernels
// only where another scene exists.  (A device index beyond the table is never counted: its scenes launch as lone ones do.)
constexpr int RTC_LIVE_DEVICES = 64;
std::atomic<int> g_live_scenes[RTC_LIVE_DEVICES];
int live_scenes(int device) { return device >= 0 && device < RTC_LIVE_DEVICES ? g_live_scenes[device].load(std::memory_order_relaxed) : 0; }

// Grid of the LDS-resident traversal build for a launch of scene s ("Spare CUs").  The persistent 768-thread blocks fill
// their CUs, so while they run no block of another stream's wf_shade or wf_gather fits anywhere.  An UNSYNCHRONISED launch of a scene
// that has company on its device therefore leaves spare_cus CUs out of its grid: pipelined frames of other scenes shade there.  Every
// other launch takes all n_cu: a synchronous one (rtc_render, the tuning and counting launches) has the host waiting for this frame
// alone, and a lone scene has no other stream that could use the room.
unsigned lds_grid(const rtc_scene* s, bool will_sync) {
  const bool spare = !will_sync && live_scenes(s->device) > 1;
  return rtc_wavefront_lds_grid(s->n_cu, spare ? s->spare_cus : 0);
}

// Sticky error state of the scene (DStats tail): read and cleared together.
int read_clear_sticky(rtc_scene* s, DStats* h) {
  HIP_OK(hipMemcpy(h, s->d_stats, sizeof(*h), hipMemcpyDeviceToHost));
  if (h->nan_ts || h->guard || h->wf_overflow)
    HIP_OK(hipMemset((char*)s->d_stats + RTC_STATS_LAUNCH_BYTES, 0, sizeof(DStats) - RTC_STATS_LAUNCH_BYTES));
  return RTC_OK;
}

// rtc_stats of the scene's most recent launch from its device counters `h` (read after the stream went idle).
int fill_stats(rtc_scene* s, const DStats& h, uint64_t pixels, rtc_stats* stats) {
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
  std::memset(stats, 0, sizeof(*stats));
  stats->pixels = pixels;
  stats->rays_primary = h.rays_primary; stats->rays_shadow = h.rays_shadow; stats->rays_reflect = h.rays_reflect; stats->rays_refract = h.rays_refract;
  stats->rays_container = h.rays_container; stats->accel_nodes = h.accel_nodes; stats->group_tests = h.group_tests; stats->tri_tests = h.tri_tests;
  stats->analytic_tests = h.analytic_tests; stats->nan_ts = h.nan_ts;
  stats->accel_nodes_kernarg = h.knodes; stats->analytic_tests_kernarg = h.kplanes; stats->light_grid_cells = h.light_cells;
  stats->group_tests_uniform = h.kgroups;
  stats->kernel_ms = ms;
  stats->n_launches = s->last_wavefront ? 2u * (uint32_t)s->last_fuel + 4u + (s->has_bg ? (uint32_t)s->last_fuel + 1u : 0u) : 1u;  // (wf_background: one per level)
  return RTC_OK;
}

// `after` (optional): queued behind the kernels of EVERY attempt of this launch, before the host waits (the copies of a host-pixel
// render); a launch that is rendered again (queue overflow -> larger queues / the other path) calls it again.
typedef std::function<int()> AfterLaunch;
int run(rtc_scene* s, const DCamera& cam, DPixelMap pm, int fuel, double* d_rgb, bool want_hits, rtc_stats* stats, bool count, bool sync, int force = 0,
        const AfterLaunch* after = nullptr) {
  if (fuel < 0) fuel = 0;  // fuel <= 0 spawns nothing (src/world.rs:90,110)
  if (fuel > RTC_MAX_FUEL) return rtc_fail(RTC_ERR_UNSUPPORTED, "fuel exceeds RTC_MAX_FUEL (16): the reference recurses without a limit, the device keeps its pending rays per lane");
  // World::shade_hit calls reflected_color / refracted_color inside its loop over the lights (src/world.rs:58-79): a world without
  // lights traces no secondary ray at all (and shades every hit black)
  if (s->d.n_lights == 0) fuel = 0;
  HIP_OK(hipSetDevice(s->device));
  // only the per-launch counters are zeroed: the error fields behind them accumulate until somebody reads them
  HIP_OK(hipMemsetAsync(s->d_stats, 0, RTC_STATS_LAUNCH_BYTES, s->stream));
  HIP_OK(hipEventRecord(s->ev0, s->stream));
  const bool will_sync = sync || stats != nullptr;
  const bool tuned = force == 0 && s->kernel_version == 0;
  int path = force ? force : s->kernel_version;
  if (tuned) path = pick_path(s, launch_signature(cam, pm, fuel), rtc_wavefront_work(cam, pm), fuel, will_sync, pm.mode != 2);
  if (path == 4 && s->wave_alloc_failed && force == 0) path = 1;
  const bool wavefront = path == 4 && pm.n > 0;
  if (s->d.csg_max_hits > RTC_CSG_MAX_HITS) {
    // threads of the launch that walk CSG sub-programs: the one-kernel grid covers every work id, the wavefront traversal grid is persistent
    const uint64_t threads = wavefront ? (uint64_t)s->wave_blocks * 64ull : ((rtc_wavefront_work(cam, pm) + 63) / 64) * 64;
    if (threads > s->csg_slab_threads) {
      const uint64_t bytes = threads * (uint64_t)s->d.csg_max_hits * sizeof(DCsgHit);
      const char* e = std::getenv("RTC_CSG_MAX_BYTES");
      if (bytes > (e ? std::strtoull(e, nullptr, 10) : (16ull << 30)))
        return rtc_fail(RTC_ERR_UNSUPPORTED, "the CSG intersection slab of this launch exceeds RTC_CSG_MAX_BYTES: render fewer pixels per call");
      const int rc = grow(&s->csg_slab_threads, threads, {{(void**)&s->csg_slab, bytes}}, s->stream);
      if (rc != RTC_OK) return rc;
    }
    s->d.csg_slab = s->csg_slab;
  }
  if (wavefront) {
    int rc = ensure_wave(s, rtc_wavefront_work(cam, pm), fuel);
    if (rc == RTC_ERR_UNSUPPORTED && force == 0) {
      // does not fit the memory budget / the device's free memory: this launch shape stays on the one-kernel path (same bits)
      if (tuned) drop_wavefront(s);
      else s->wave_alloc_failed = true;
      return run(s, cam, pm, fuel, d_rgb, want_hits, stats, count, sync, 1, after);
    }
    if (rc != RTC_OK) return rc;
    s->wave.dig = nullptr;
    if (pm.digest && count) {  // parity launch: (levels) x cap hit hashes beside the queues
      const uint64_t need = (uint64_t)s->wave_cap * (uint64_t)(fuel + 1);
      rc = grow(&s->cap_wave_dig, need, {{(void**)&s->d_wave_dig, need * sizeof(unsigned long long)}}, s->stream);
      if (rc != RTC_OK) return rc;
      s->wave.dig = s->d_wave_dig;
    }
    HIP_OK(hipMemsetAsync(s->wave.counts, 0, RTC_WF_COUNTS * sizeof(uint32_t), s->stream));
    HIP_OK(hipEventRecord(s->ev0, s->stream));
    rtc_launch_wavefront(s->d, cam, pm, fuel, s->wave, d_rgb, want_hits ? s->d_hit_t : nullptr, s->d_hit_prim, s->d_hit_k, s->d_stats, count, s->stream, s->wave_blocks, s->shade_blocks, s->lds_bytes,
                         lds_grid(s, will_sync), s->ext());
  } else {
    rtc_launch_trace(s->d, cam, pm, fuel, d_rgb, want_hits ? s->d_hit_t : nullptr, s->d_hit_prim, s->d_hit_k, s->d_stats, count, s->stream, rtc_scene_is_big(s->bytes), s->ext());
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(s->ev1, s->stream));
  s->last_wavefront = wavefront;
  s->last_fuel = fuel;
  if (after) { int rca = (*after)(); if (rca != RTC_OK) return rca; }
  if (!sync && !stats) return RTC_OK;
  HIP_OK(hipStreamSynchronize(s->stream));
  DStats h;
  int rcs = read_clear_sticky(s, &h);
  if (rcs != RTC_OK) return rcs;
  if (wavefront) {
    if (std::getenv("RTC_WF_DUMP_COUNTS")) {  // debug aid: rays and shade records per level of this frame
      uint32_t c[64], top[64];  // (the near ends' counts; the far ends': rays, records)
      HIP_OK(hipMemcpy(c, s->wave.counts, sizeof(c), hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(top, s->wave.counts + RTC_WF_TOP_COUNT, sizeof(top), hipMemcpyDeviceToHost));
      std::fprintf(stderr, "[rtc-wf] level: rays far + near / shade records far + near:");
      for (int l = 0; l <= fuel; l++)
        std::fprintf(stderr, " %d: %u + %u / %u + %u;", l, top[l], l ? c[l] : (unsigned)rtc_wavefront_work(cam, pm), top[32 + l], c[RTC_WF_SHADE_COUNT + l]);
      std::fprintf(stderr, "\n");
    }
    uint32_t overflow = 0;
    HIP_OK(hipMemcpy(&overflow, s->wave.counts + RTC_WF_OVERFLOW, sizeof(overflow), hipMemcpyDeviceToHost));
    if (overflow) {  // a level outgrew its queue: larger queues if they fit the budget, else the one-kernel path (always fits)
      const uint64_t n_work = rtc_wavefront_work(cam, pm);
      if (s->wave_eighths < 512 && wave_bytes(wave_cap(n_work, 2 * s->wave_eighths), fuel + 1) <= wave_budget() && wave_cap(n_work, 2 * s->wave_eighths) <= 0x7fffff00ull) {
        s->wave_eighths *= 2;
        const int rc2 = run(s, cam, pm, fuel, d_rgb, want_hits, stats, count, true, 4, after);
        if (rc2 != RTC_ERR_UNSUPPORTED) return rc2;  // (the larger queues were refused by the device: fall through)
      }
      if (tuned) drop_wavefront(s);
      return run(s, cam, pm, fuel, d_rgb, want_hits, stats, count, true, 1, after);
    }
  }
  if (tuned && !count && pm.mode == 2 && !s->tune_choice) {
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    record_sample(s, wavefront, ms);
  }
  if (stats) {
    int rcf = fill_stats(s, h, pm.n, stats);
    if (rcf != RTC_OK) return rcf;
  }
  if (std::getenv("RTC_DIAG_DUMP")) {  // RTC_DIAG builds: raw region / utilisation counters for scripts/diag_report.py
    std::fprintf(stderr, "[rtc-diag]");
    for (int i = 0; i < 64; i++) std::fprintf(stderr, " %llu", (unsigned long long)h.diag[i]);
    std::fprintf(stderr, "\n");
  }
  if (h.guard) return rtc_fail(RTC_ERR_DEVICE, "traversal guard tripped (mask " + std::to_string(h.guard) + "): an index left its array; no pixel since the last check is trustworthy");
  if (h.nan_ts) return rtc_fail(RTC_ERR_NAN, "a NaN intersection t reached a sort of two or more intersections (the reference panics in Intersection::sort, src/intersection.rs:124)");
  return RTC_OK;
}

// The pixel map of a host-side launch over pixels first .. first + n - 1 or the n listed indices (uploaded to the scene's index buffer).
// (`total`: the frame's pixel count, the bound of a listed index)
int make_pixel_map(rtc_scene* s, uint64_t hsize, uint64_t total, const uint64_t* pixel_indices, uint64_t first, uint64_t n, DPixelMap* pm, std::vector<uint64_t>* range_idx) {
  *pm = DPixelMap{};
  pm->n = n;
  // A contiguous range is expressed through the two pixel maps the kernels are validated with on hardware: whole rows ->
  // interleaved-row map with step 1; anything else -> an explicit index list.
  if (!pixel_indices) {
    if (first % hsize == 0 && n % hsize == 0) {
      pm->mode = 2; pm->row_first = (uint32_t)(first / hsize); pm->row_step = 1;
    } else {
      range_idx->resize(n);
      for (uint64_t i = 0; i < n; i++) (*range_idx)[i] = first + i;
      pixel_indices = range_idx->data();
    }
  }
  if (pixel_indices) {
    for (uint64_t i = 0; i < n; i++)
      if (pixel_indices[i] >= total) return rtc_fail(RTC_ERR_INVALID, "pixel index exceeds the image");
    const int rc = grow(&s->cap_idx, n, {{(void**)&s->d_idx, n * sizeof(uint64_t)}});
    if (rc != RTC_OK) return rc;
    HIP_OK(hipMemcpy(s->d_idx, pixel_indices, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    pm->mode = 1; pm->indices = s->d_idx;
  }
  return RTC_OK;
}
int make_pixel_map(rtc_scene* s, const rtc_camera* cam, const uint64_t* pixel_indices, uint64_t first, uint64_t n, DPixelMap* pm, std::vector<uint64_t>* range_idx) {
  return make_pixel_map(s, cam->hsize, cam->hsize * cam->vsize, pixel_indices, first, n, pm, range_idx);
}
// The pixel map of the n pixels of whole rows from row_first on.
DPixelMap rows_map(uint64_t n, uint32_t row_first = 0) {
  DPixelMap pm{};
  pm.n = n; pm.mode = 2; pm.row_first = row_first; pm.row_step = 1;
  return pm;
}

// ---- the sampled camera (include/rtc.h rtc_sampling; kernels in rtc_camera.hip) ---------------------------------------------------
int check_sampling(const rtc_sampling* sp) {
  if (!sp) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (sp->side == 0) return rtc_fail(RTC_ERR_INVALID, "sampling: side must be >= 1");
  if (sp->flags & ~(uint32_t)RTC_SAMPLE_JITTER) return rtc_fail(RTC_ERR_INVALID, "sampling: unknown flag bits");
  if (!std::isfinite(sp->lens_radius) || sp->lens_radius < 0.0) return rtc_fail(RTC_ERR_INVALID, "sampling: lens_radius must be finite and >= 0");
  if (sp->lens_radius > 0.0 && (!std::isfinite(sp->focal_distance) || sp->focal_distance <= 0.0))
    return rtc_fail(RTC_ERR_INVALID, "sampling: focal_distance must be finite and > 0 when lens_radius > 0");
  if (sp->side > RTC_SAMPLES_MAX_SIDE) return rtc_fail(RTC_ERR_UNSUPPORTED, "sampling: side exceeds RTC_SAMPLES_MAX_SIDE (16)");
  return RTC_OK;
}

// Rays per chunk of a sampled launch.  RTC_SAMPLED_MAX_RAYS (read at each call; tests force many chunks with it); default 2^22: a
// 201 MB ray buffer, and wavefront queues of the size a 4 MP frame's are (profiles/sampled_camera_probe.txt).
uint64_t sampled_max_rays() {
  const char* e = std::getenv("RTC_SAMPLED_MAX_RAYS");
  const uint64_t v = e ? std::strtoull(e, nullptr, 10) : 0;
  return v ? v : (1ull << 22);
}

int ensure_sampled(rtc_scene* s, uint64_t n_rays, bool colours) {
  int rc = grow(&s->cap_srays, n_rays, {{(void**)&s->d_srays, n_rays * 6 * sizeof(double)}}, s->stream);
  if (rc == RTC_OK && colours) rc = grow(&s->cap_srgb, n_rays, {{(void**)&s->d_srgb, n_rays * 3 * sizeof(double)}}, s->stream);
  return rc;
}

// Pixels per chunk of a sampled launch over n pixels with N rays each: as many as RTC_SAMPLED_MAX_RAYS allows, in whole `unit`s (a row
// of the frame, or one pixel of a list), never fewer than one unit.
int sampled_chunk_px(uint64_t n, uint64_t unit, uint64_t N, uint64_t* chunk_px) {
  *chunk_px = std::min<uint64_t>(n / unit, std::max<uint64_t>(1, sampled_max_rays() / (unit * N))) * unit;
  if (*chunk_px * N > 0x7fffff00ull) return rtc_fail(RTC_ERR_UNSUPPORTED, "one row of this sampled launch exceeds 2^31 rays");
  return RTC_OK;
}

// launch_signature of a sampled launch: the pixel set's, and the sampling
uint64_t sampled_signature(const DCamera& cam, const DPixelMap& pm, const rtc_sampling& sp, int fuel) {
  uint64_t h = launch_signature(cam, pm, fuel) ^ 0x73616d706c656473ull;
  auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; } };
  mix(&sp.side, sizeof(sp.side)); mix(&sp.flags, sizeof(sp.flags)); mix(&sp.seed, sizeof(sp.seed));
  mix(&sp.lens_radius, sizeof(sp.lens_radius)); mix(&sp.focal_distance, sizeof(sp.focal_distance));
  return h ? h : 1;
}

void add_stats(rtc_stats* a, const rtc_stats& b) {
  a->rays_primary += b.rays_primary; a->rays_shadow += b.rays_shadow; a->rays_reflect += b.rays_reflect; a->rays_refract += b.rays_refract;
  a->rays_container += b.rays_container; a->accel_nodes += b.accel_nodes; a->group_tests += b.group_tests; a->tri_tests += b.tri_tests;
  a->analytic_tests += b.analytic_tests; a->nan_ts += b.nan_ts; a->n_launches += b.n_launches;
  a->accel_nodes_kernarg += b.accel_nodes_kernarg; a->analytic_tests_kernarg += b.analytic_tests_kernarg;
  a->light_grid_cells += b.light_grid_cells; a->group_tests_uniform += b.group_tests_uniform;
  a->kernel_ms += b.kernel_ms;
}

// What the chunked launches (run_sampled, run_filtered) do alike.  All on the scene's stream, so the ray buffer d_srays and the per-ray
// colours d_srgb are reused chunk after chunk; a synchronous launch reads every chunk's state back (a chunk whose wavefront queues
// overflowed is rendered again by run() before its rays are overwritten; the resolves only write).
//   begin(): the path of the call.  A tuned call goes through pick_path ONCE -- the signature is the whole launch's, the guess counts
//     the rays of a chunk, the measurement is the sum of the chunks' trace times -- and every chunk takes that path; an untuned call
//     leaves force at 0 (run() decides: the scene's pinned path, the one-kernel path for lists) unless the caller sets it.
//   chunk(): `generate` fills d_srays with the chunk's n_rays rays, run() traces them as explicit rays into d_srgb, `resolve` queues the
//     caller's kernel behind them as run()'s hook (again behind every attempt run() makes); `after` follows the last chunk's resolve.
//     Queues that the device refuses and a fallback of run()'s own after an overflow move the rest of the call to the one-kernel path
//     (same bits) and drop the wavefront candidate.  With stats: the chunk's counters, its launches + 2, the span evs0 .. evs1.
//   end(): one sample of pick_path's measurement, as run() takes it, when the call kept its path; the pixel count of the stats.
struct ChunkDriver {
  rtc_scene* s;
  int fuel;
  rtc_stats* stats;
  bool count, sync;
  const AfterLaunch* after;
  const char* resolve_name;  // of the caller's resolve kernel, for an error's text
  bool tuned = false;
  int force = 0, first_path = 0;
  double trace_ms = 0.0;

  bool will_sync() const { return sync || stats != nullptr; }
  void begin(bool tune, uint64_t signature, uint64_t chunk_rays) {
    tuned = tune;
    if (tuned) {
      force = pick_path(s, signature, chunk_rays, fuel, will_sync(), false);
      if (force == 4 && s->wave_alloc_failed) force = 1;
    }
    first_path = force;
    if (stats) std::memset(stats, 0, sizeof(*stats));
  }
  int chunk(uint64_t n_rays, bool last, const std::function<void()>& generate, const std::function<void()>& resolve) {
    if (stats) HIP_OK(hipEventRecord(s->evs0, s->stream));
    generate();
    HIP_OK(hipGetLastError());
    DCamera ray_cam{};
    ray_cam.hsize = 1; ray_cam.vsize = 1;
    DPixelMap rm{};
    rm.n = n_rays; rm.mode = 3; rm.rays = s->d_srays;
    const AfterLaunch hook = [&]() -> int {
      resolve();
      hipError_t e = hipGetLastError();
      if (e == hipSuccess && stats) e = hipEventRecord(s->evs1, s->stream);
      if (e != hipSuccess) return rtc_fail(RTC_ERR_DEVICE, std::string(resolve_name) + ": " + hipGetErrorString(e));
      return (last && after) ? (*after)() : RTC_OK;
    };
    rtc_stats st;
    int rc = run(s, ray_cam, rm, fuel, s->d_srgb, false, stats ? &st : nullptr, count, sync, force, &hook);
    if (rc == RTC_ERR_UNSUPPORTED && force == 4) {  // the queues were refused: this shape stays on the one-kernel path (same bits)
      if (tuned) drop_wavefront(s);
      force = 1;
      rc = run(s, ray_cam, rm, fuel, s->d_srgb, false, stats ? &st : nullptr, count, sync, force, &hook);
    }
    if (rc != RTC_OK) return rc;
    if (force == 4 && will_sync() && !s->last_wavefront) {  // run() rendered the chunk again on the one-kernel path after an overflow
      if (tuned) drop_wavefront(s);
      force = 1;
    }
    if (will_sync()) {
      float ms = 0.f;
      HIP_OK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
      trace_ms += ms;
    }
    if (stats) {
      float ms = 0.f;
      HIP_OK(hipEventElapsedTime(&ms, s->evs0, s->evs1));
      st.n_launches += 2u;
      st.kernel_ms = ms;
      add_stats(stats, st);
    }
    return RTC_OK;
  }
  void end(uint64_t pixels) {
    if (tuned && will_sync() && !count && !s->tune_choice && force == first_path) record_sample(s, force == 4, trace_ms);
    if (stats) stats->pixels = pixels;
  }
};
// debug aid (RTC_SAMPLED_TIMING): the three parts of the chunk that chunk() just ran with stats, by the events around them
int chunk_parts_ms(rtc_scene* s, float* generator, float* traces, float* resolve) {
  HIP_OK(hipEventElapsedTime(generator, s->evs0, s->ev0));
  HIP_OK(hipEventElapsedTime(traces, s->ev0, s->ev1));
  HIP_OK(hipEventElapsedTime(resolve, s->ev1, s->evs1));
  return RTC_OK;
}

// run() for a sampled camera: the pixel set `pm` (mode 1 or 2) is cut into chunks of whole rows (mode 2) or slices of the list (mode 1)
// of at most RTC_SAMPLED_MAX_RAYS rays, never fewer than one row / pixel; per chunk (ChunkDriver) rtc_gen_rays fills the scene's ray
// buffer, run() traces it, rtc_resolve_samples writes the pixels' means to their slots of d_rgb.
// Path: whole-row launches are tuned -- the shape is the whole launch's (camera, sampling, rows, fuel) --; lists are left to run(),
// which keeps them on the one-kernel path.  `after`: behind the last chunk's resolve (see run()).
// `scatter` (run_adaptive's refine pass; pm is a device-resident list): d_rgb is the whole FRAME and a slot's mean goes to its pixel
// of it (rtc_resolve_samples_scatter); such a list may be millions of rays, 64 consecutive of which belong to four neighbouring
// pixels, so its chunks take the scene's first guess over a chunk's rays (nothing is measured: the list changes with every frame).
int run_sampled(rtc_scene* s, const DCamera& cam, const DPixelMap& pm, const rtc_sampling& sp, int fuel, double* d_rgb, rtc_stats* stats, bool count, bool sync,
                const AfterLaunch* after = nullptr, bool scatter = false) {
  if (fuel < 0) fuel = 0;
  HIP_OK(hipSetDevice(s->device));
  const uint64_t N = (uint64_t)sp.side * sp.side;
  const bool rows = pm.mode == 2;
  uint64_t chunk_px = 0;
  int rc = sampled_chunk_px(pm.n, rows ? cam.hsize : 1, N, &chunk_px);
  if (rc == RTC_OK) rc = ensure_sampled(s, chunk_px * N, true);
  if (rc != RTC_OK) return rc;
  ChunkDriver drv{s, fuel, stats, count, sync, after, "rtc_resolve_samples"};
  drv.begin(rows && s->kernel_version == 0, sampled_signature(cam, pm, sp, s->d.n_lights == 0 ? 0 : fuel), chunk_px * N);
  if (!drv.tuned && scatter && s->kernel_version == 0) drv.force = s->wave_alloc_failed ? 1 : first_guess(s, chunk_px * N, fuel);
  for (uint64_t p0 = 0; p0 < pm.n; p0 += chunk_px) {
    const uint64_t np = std::min(chunk_px, pm.n - p0);
    rc = drv.chunk(np * N, p0 + np == pm.n, [&] { rtc_launch_gen_rays(cam, pm, sp, p0, np, s->d_srays, s->stream); }, [&] {
      if (scatter) rtc_launch_resolve_samples_scatter(s->d_srgb, (unsigned)N, np, (const unsigned long long*)pm.indices + p0, d_rgb, s->stream);
      else rtc_launch_resolve_samples(s->d_srgb, (unsigned)N, np, d_rgb + 3 * p0, s->stream);
    });
    if (rc != RTC_OK) return rc;
    if (stats && std::getenv("RTC_SAMPLED_TIMING")) {  // debug aid (scripts/sampled_camera_probe.py)
      float g = 0.f, t = 0.f, r = 0.f;
      rc = chunk_parts_ms(s, &g, &t, &r);
      if (rc != RTC_OK) return rc;
      std::fprintf(stderr, "[rtc-sampled] chunk of %llu rays: generator %.3f ms, traces %.3f ms, resolve %.3f ms\n", (unsigned long long)(np * N), g, t, r);
    }
  }
  drv.end(pm.n);
  return RTC_OK;
}

// ---- adaptive sampling (include/rtc.h rtc_adaptive; kernels in rtc_adaptive.hip, the rule in adaptive_contrast.h) -------------------
int check_adaptive(const rtc_adaptive* ad) {
  if (!ad) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_sampling(&ad->base);
  if (rc == RTC_OK) rc = check_sampling(&ad->fine);
  if (rc != RTC_OK) return rc;
  if (std::isnan(ad->threshold)) return rtc_fail(RTC_ERR_INVALID, "adaptive: threshold is NaN");
  if (ad->neighbours != 4 && ad->neighbours != 8) return rtc_fail(RTC_ERR_INVALID, "adaptive: neighbours must be 4 or 8");
  return RTC_OK;
}
int check_contrast_frame(uint64_t hsize, uint64_t vsize) {
  if (hsize == 0 || vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty frame");
  if (hsize >= (1ull << 39) || vsize >= (1ull << 39) || hsize * vsize >= (1ull << 39)) return rtc_fail(RTC_ERR_UNSUPPORTED, "adaptive: frames of 2^39 pixels or more");
  return RTC_OK;
}

// The compaction's buffers for a frame of n pixels, grown like d_srays.
int ensure_adaptive(rtc_scene* s, uint64_t n) {
  if (!s->d_acount) HIP_OK(hipMalloc((void**)&s->d_acount, sizeof(unsigned long long)));
  return grow(&s->cap_alist, n, {{(void**)&s->d_alist, n * sizeof(unsigned long long)},
                                 {(void**)&s->d_awork, rtc_contrast_work_words(n) * sizeof(unsigned long long)}}, s->stream);  // (monotonic in n)
}

// Detect and compact over the frame in d_frame (hsize x vsize), on the stream; then the ONE read-back the host needs: the list's length.
int contrast_compact(rtc_scene* s, const double* d_frame, uint64_t hsize, uint64_t vsize, double threshold, uint32_t neighbours, uint64_t* n_refined,
                     unsigned* n_kernels, bool timed) {
  int rc = ensure_adaptive(s, hsize * vsize);
  if (rc != RTC_OK) return rc;
  if (timed) HIP_OK(hipEventRecord(s->evs0, s->stream));
  *n_kernels = rtc_launch_contrast_compact(d_frame, hsize, vsize, threshold, neighbours, s->d_awork, s->d_alist, s->d_acount, s->stream);
  HIP_OK(hipGetLastError());
  if (timed) HIP_OK(hipEventRecord(s->evs1, s->stream));
  unsigned long long c = 0;
  HIP_OK(hipMemcpyAsync(&c, s->d_acount, sizeof(c), hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  if (c > hsize * vsize) return rtc_fail(RTC_ERR_DEVICE, "adaptive: the compaction counted more pixels than the frame has");
  *n_refined = c;
  return RTC_OK;
}

// The whole frame of `cam` into s->d_rgb (ensure_px'ed by the caller) under the rule `ad`: base pass, detect and compact, count
// read-back, refine pass over the device-resident list with the scatter resolve.  `mask` / `n_refined`: optional host outputs.
// `after`: queued behind the last kernel that writes the frame (see run()).
int run_adaptive(rtc_scene* s, const DCamera& cam, const rtc_adaptive& ad, int fuel, rtc_stats* stats, uint8_t* mask, uint64_t* n_refined, const AfterLaunch* after) {
  const uint64_t n = cam.hsize * cam.vsize;
  const bool count = stats != nullptr;
  const DPixelMap rows = rows_map(n);
  rtc_stats st_base, st_fine;
  std::memset(&st_fine, 0, sizeof(st_fine));
  // 1. base: one centre sample per pixel IS rtc_render's frame (include/rtc.h rtc_sampling), so it takes rtc_render's launch
  const bool plain = ad.base.side == 1 && !(ad.base.flags & RTC_SAMPLE_JITTER) && !(ad.base.lens_radius > 0.0);
  int rc = plain ? run(s, cam, rows, fuel, s->d_rgb, false, stats ? &st_base : nullptr, count, true)
                 : run_sampled(s, cam, rows, ad.base, fuel, s->d_rgb, stats ? &st_base : nullptr, count, true);
  if (rc != RTC_OK) return rc;
  // 2. + 3. the refined pixels' list and its length
  uint64_t refined = 0;
  unsigned n_kernels = 0;
  rc = contrast_compact(s, s->d_rgb, cam.hsize, cam.vsize, ad.threshold, ad.neighbours, &refined, &n_kernels, stats != nullptr);
  if (rc != RTC_OK) return rc;
  float detect_ms = 0.f;
  if (stats) HIP_OK(hipEventElapsedTime(&detect_ms, s->evs0, s->evs1));
  if (stats && std::getenv("RTC_SAMPLED_TIMING"))  // debug aid (scripts/adaptive_probe.py)
    std::fprintf(stderr, "[rtc-adaptive] detect + compact %.3f ms (%u kernels): %llu of %llu pixels refined\n", detect_ms, n_kernels, (unsigned long long)refined, (unsigned long long)n);
  if (n_refined) *n_refined = refined;
  if (mask) {  // from the list: the stream is idle, the pass below only reads it
    std::vector<unsigned long long> list(refined);
    if (refined) HIP_OK(hipMemcpy(list.data(), s->d_alist, refined * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::memset(mask, 0, n);
    for (unsigned long long i : list) if (i < n) mask[i] = 1;
  }
  // 4. refine: run_sampled's chunks over the list, each mean written to its pixel of the frame
  if (refined) {
    DPixelMap lm{};
    lm.n = refined; lm.mode = 1; lm.indices = (const uint64_t*)s->d_alist;
    rc = run_sampled(s, cam, lm, ad.fine, fuel, s->d_rgb, stats ? &st_fine : nullptr, count, true, after, true);
    if (rc != RTC_OK) return rc;
  } else if (after) {
    rc = (*after)();
    if (rc != RTC_OK) return rc;
    HIP_OK(hipStreamSynchronize(s->stream));
  }
  if (stats) {
    *stats = st_base;
    add_stats(stats, st_fine);
    stats->pixels = n;
    stats->n_launches += n_kernels;
    stats->kernel_ms += detect_ms;
  }
  return RTC_OK;
}

// ---- the shutter (include/rtc.h rtc_shutter; kernels in rtc_shutter.hip, the rule in shutter_pose.h) ---------------------------------
// The shutter's own numbers, with the sampling they deal: no device is looked at.
int check_shutter(const rtc_shutter* sh, uint32_t n_poses, const rtc_sampling* sp) {
  if (!sh) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (n_poses == 0) return rtc_fail(RTC_ERR_INVALID, "shutter: n_poses must be >= 1");
  if (sh->flags & ~(uint32_t)RTC_SHUTTER_HASHED) return rtc_fail(RTC_ERR_INVALID, "shutter: unknown flag bits");
  if (n_poses > RTC_SHUTTER_MAX_POSES) return rtc_fail(RTC_ERR_UNSUPPORTED, "shutter: n_poses exceeds RTC_SHUTTER_MAX_POSES (64)");
  const int rc = check_sampling(sp);
  if (rc != RTC_OK) return rc;
  if (!(sh->flags & RTC_SHUTTER_HASHED) && n_poses > sp->side * sp->side)
    return rtc_fail(RTC_ERR_INVALID, "shutter: more poses than samples per pixel without RTC_SHUTTER_HASHED (some poses would never be sampled)");
  return RTC_OK;
}

// The poses' arrays: entries, one frame size, one device.
int check_poses(rtc_scene* const* scenes, const rtc_camera* cameras, uint32_t n_poses) {
  if (!scenes || !cameras) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (cameras[0].hsize == 0 || cameras[0].vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  for (uint32_t p = 1; p < n_poses; p++)
    if (cameras[p].hsize != cameras[0].hsize || cameras[p].vsize != cameras[0].vsize) return rtc_fail(RTC_ERR_INVALID, "shutter: the cameras' hsize or vsize differ");
  for (uint32_t p = 0; p < n_poses; p++)
    if (!scenes[p]) return rtc_fail(RTC_ERR_INVALID, "shutter: a NULL scene among the poses");
  for (uint32_t p = 1; p < n_poses; p++)
    if (scenes[p]->device != scenes[0]->device) return rtc_fail(RTC_ERR_INVALID, "shutter: the poses' scenes are on different devices");
  return RTC_OK;
}

// The dealing's buffers for a chunk of m samples, grown like d_srays.
int ensure_shutter(rtc_scene* s, uint64_t m) {
  return grow(&s->cap_shutter, m, {{(void**)&s->d_shorder, m * sizeof(unsigned)}, {(void**)&s->d_shwhere, m * sizeof(unsigned)},
                                   {(void**)&s->d_shwork, rtc_shutter_work_words(m) * sizeof(unsigned long long)}}, s->stream);
}

// Deal the m samples of the output slots slot_first .. of `pm` on s's stream (ensure_shutter'ed for m), then the ONE read-back the host
// needs: offsets[0 .. K], checked before anybody launches over them.  `timed`: evs0 / evs1 around the kernels.
int shutter_deal(rtc_scene* s, const rtc_shutter& sh, const rtc_sampling& sp, uint32_t K, const DPixelMap& pm, const DCamera& cam, uint64_t slot_first, uint64_t m,
                 unsigned long long* offsets, unsigned* n_kernels, bool timed) {
  if (timed) HIP_OK(hipEventRecord(s->evs0, s->stream));
  *n_kernels = rtc_launch_shutter_deal(sh, sp, K, pm, cam, slot_first, m, s->d_shwork, s->d_shorder, s->d_shwhere, s->stream);
  HIP_OK(hipGetLastError());
  if (timed) HIP_OK(hipEventRecord(s->evs1, s->stream));
  HIP_OK(hipMemcpyAsync(offsets, rtc_shutter_offsets(s->d_shwork, m), (K + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  bool ok = offsets[0] == 0 && offsets[K] == m;
  for (uint32_t p = 0; p < K && ok; p++) ok = offsets[p] <= offsets[p + 1];
  if (!ok) return rtc_fail(RTC_ERR_DEVICE, "shutter: the dealing's offsets do not partition the chunk's samples");
  return RTC_OK;
}

// run_sampled over K poses: the pixel set `pm` (mode 1 or 2; a list lives in scenes[0]'s index buffer) in run_sampled's chunks; the
// buffers and the shutter's own kernels are scenes[0]'s, on its stream.  Per chunk: deal and read the offsets back (shutter_deal); per
// pose with a non-empty run its generator, then run() of ITS scene over the run's rays -- synchronously, so a run whose wavefront queues
// overflowed is traced again before anything else touches its colours, and so that the trace is over before scenes[0]'s stream goes
// on; a trace on another scene's stream waits for the generator through an event --; then the resolve.
// Path of a run: a pinned scene's own; otherwise that scene's first guess over the run's rays (nothing is measured: the runs change
// with the seed), the one-kernel path after a refusal of the queues.  `after`: behind the last chunk's resolve (see run()).
int run_shutter(rtc_scene* const* scenes, const DCamera* cams, uint32_t K, const rtc_shutter& sh, const DPixelMap& pm, const rtc_sampling& sp, int fuel, double* d_rgb,
                rtc_stats* stats, const AfterLaunch* after) {
  rtc_scene* s = scenes[0];
  if (fuel < 0) fuel = 0;
  HIP_OK(hipSetDevice(s->device));
  const uint64_t N = (uint64_t)sp.side * sp.side;
  uint64_t chunk_px = 0;
  int rc = sampled_chunk_px(pm.n, pm.mode == 2 ? cams[0].hsize : 1, N, &chunk_px);
  if (rc == RTC_OK) rc = ensure_sampled(s, chunk_px * N, true);
  if (rc == RTC_OK) rc = ensure_shutter(s, chunk_px * N);
  if (rc != RTC_OK) return rc;
  const bool count = stats != nullptr;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  DCamera ray_cam{};
  ray_cam.hsize = 1; ray_cam.vsize = 1;
  unsigned long long offsets[RTC_SHUTTER_MAX_POSES + 1];
  for (uint64_t p0 = 0; p0 < pm.n; p0 += chunk_px) {
    const uint64_t np = std::min(chunk_px, pm.n - p0);
    const bool last = p0 + np == pm.n;
    unsigned n_kernels = 0;
    rc = shutter_deal(s, sh, sp, K, pm, cams[0], p0, np * N, offsets, &n_kernels, stats != nullptr);
    if (rc != RTC_OK) return rc;
    float ms = 0.f, deal_ms = 0.f;
    double gen_ms = 0.0, trace_ms = 0.0;
    if (stats) {
      HIP_OK(hipEventElapsedTime(&deal_ms, s->evs0, s->evs1));
      stats->kernel_ms += deal_ms;
      stats->n_launches += n_kernels;
    }
    for (uint32_t p = 0; p < K; p++) {
      const uint64_t off = offsets[p], len = offsets[p + 1] - off;
      if (len == 0) continue;  // an empty run launches nothing
      rtc_scene* t = scenes[p];
      if (stats) HIP_OK(hipEventRecord(s->evs0, s->stream));
      rtc_launch_shutter_gen_rays(cams[p], pm, sp, p0, s->d_shorder, (unsigned)off, (unsigned)len, (unsigned)(np * N), s->d_srays, s->stream);
      HIP_OK(hipGetLastError());
      HIP_OK(hipEventRecord(s->evs1, s->stream));
      if (t->stream != s->stream) HIP_OK(hipStreamWaitEvent(t->stream, s->evs1, 0));
      DPixelMap rm{};
      rm.n = len; rm.mode = 3; rm.rays = s->d_srays + 6 * off;
      int force = 0;
      if (t->kernel_version == 0) force = t->wave_alloc_failed ? 1 : first_guess(t, len, fuel);
      rtc_stats st;
      rc = run(t, ray_cam, rm, fuel, s->d_srgb + 3 * off, false, stats ? &st : nullptr, count, true, force);
      if (rc == RTC_ERR_UNSUPPORTED && force == 4) {  // the queues were refused: the one-kernel path (same bits)
        rc = run(t, ray_cam, rm, fuel, s->d_srgb + 3 * off, false, stats ? &st : nullptr, count, true, 1);
      }
      if (rc != RTC_OK) return rc;
      // (run() waited for t's stream: whatever scenes[0]'s stream does next comes after the trace)
      if (stats) {
        HIP_OK(hipEventElapsedTime(&ms, s->evs0, s->evs1));
        add_stats(stats, st);
        stats->kernel_ms += ms;
        stats->n_launches += 1u;
        gen_ms += ms; trace_ms += st.kernel_ms;
      }
    }
    if (stats) HIP_OK(hipEventRecord(s->evs0, s->stream));
    rtc_launch_shutter_resolve(s->d_srgb, s->d_shwhere, (unsigned)N, np, d_rgb + 3 * p0, s->stream);
    HIP_OK(hipGetLastError());
    if (stats) HIP_OK(hipEventRecord(s->evs1, s->stream));
    if (last && after) { rc = (*after)(); if (rc != RTC_OK) return rc; }
    if (stats || last) HIP_OK(hipStreamSynchronize(s->stream));
    if (stats) {
      HIP_OK(hipEventElapsedTime(&ms, s->evs0, s->evs1));
      if (std::getenv("RTC_SAMPLED_TIMING"))  // debug aid (scripts/shutter_probe.py)
        std::fprintf(stderr, "[rtc-shutter] chunk of %llu rays: dealing %.3f ms (%u kernels), generators %.3f ms, traces %.3f ms, resolve %.3f ms\n",
                     (unsigned long long)(np * N), deal_ms, n_kernels, gen_ms, trace_ms, ms);
      stats->kernel_ms += ms;
      stats->n_launches += 1u;
    }
  }
  if (stats) stats->pixels = pm.n;
  return RTC_OK;
}

// ---- reconstruction filters (include/rtc.h rtc_filter; kernel in rtc_filter.hip, the rule in filter_weights.h) ------------------------
int check_filter(const rtc_filter* f) {
  if (!f) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (f->kind < RTC_FILTER_BOX || f->kind > RTC_FILTER_MITCHELL) return rtc_fail(RTC_ERR_INVALID, "filter: unknown kind");
  if (!std::isfinite(f->radius) || f->radius < 0.5) return rtc_fail(RTC_ERR_INVALID, "filter: radius must be finite and >= 0.5");
  if (f->kind == RTC_FILTER_GAUSSIAN && (!std::isfinite(f->alpha) || f->alpha <= 0.0)) return rtc_fail(RTC_ERR_INVALID, "filter: a Gaussian's alpha must be finite and > 0");
  if (f->radius > RTC_FILTER_MAX_RADIUS) return rtc_fail(RTC_ERR_UNSUPPORTED, "filter: radius exceeds RTC_FILTER_MAX_RADIUS (3)");
  return RTC_OK;
}

// sampled_signature of a filtered launch (pm = its output rows): and the filter
uint64_t filtered_signature(const DCamera& cam, const DPixelMap& pm, const rtc_sampling& sp, const rtc_filter& f, int fuel) {
  uint64_t h = sampled_signature(cam, pm, sp, fuel) ^ 0x66696c7465726564ull;
  auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; } };
  mix(&f.kind, sizeof(f.kind)); mix(&f.radius, sizeof(f.radius)); mix(&f.alpha, sizeof(f.alpha));
  return h ? h : 1;
}

// run_sampled for whole rows with a reconstruction filter: pm (mode 2, row_step 1, no bands) names the OUTPUT rows [a, b); they are cut
// into chunks of whole rows, a chunk [a', b') traces the image rows [max(0, a' - W), min(vsize, b' + W)) -- rtc_gen_rays, run() over
// explicit rays (ChunkDriver) -- and rtc_resolve_filtered, the hook behind run()'s kernels, writes the chunk's own rows of d_rgb and
// nothing else, so a chunk that run() renders again resolves to the same bits.  RTC_SAMPLED_MAX_RAYS bounds a chunk's TRACED rays, halo
// included, never below one output row and its halo.  The halo rows are traced again by the neighbouring chunk: the two buffers stay
// reusable.
// Path: always tuned (unless the scene's path is pinned); the shape also holds the filter (and pm the row range), the guess counts a
// chunk's traced rays.  `after`: behind the last chunk's filter kernel (see run()).
int run_filtered(rtc_scene* s, const DCamera& cam, const DPixelMap& pm, const rtc_sampling& sp, const rtc_filter& f, int fuel, double* d_rgb, rtc_stats* stats,
                 bool count, bool sync, const AfterLaunch* after = nullptr) {
  if (fuel < 0) fuel = 0;
  HIP_OK(hipSetDevice(s->device));
  const uint64_t N = (uint64_t)sp.side * sp.side, W = rtc_filter_window(f.radius);
  const uint64_t a = pm.row_first, b = a + pm.n / cam.hsize;
  const uint64_t row_rays = cam.hsize * N, fit = sampled_max_rays() / row_rays;
  const uint64_t chunk_rows = std::min<uint64_t>(b - a, fit > 2 * W + 1 ? fit - 2 * W : 1);
  const uint64_t traced_rows = std::min<uint64_t>(chunk_rows + 2 * W, cam.vsize);
  if (traced_rows * row_rays > 0x7fffff00ull) return rtc_fail(RTC_ERR_UNSUPPORTED, "one row of this filtered launch and its halo exceed 2^31 rays");
  int rc = ensure_sampled(s, traced_rows * row_rays, true);
  if (rc != RTC_OK) return rc;
  ChunkDriver drv{s, fuel, stats, count, sync, after, "rtc_resolve_filtered"};
  drv.begin(s->kernel_version == 0, filtered_signature(cam, pm, sp, f, s->d.n_lights == 0 ? 0 : fuel), traced_rows * row_rays);
  for (uint64_t c0 = a; c0 < b; c0 += chunk_rows) {
    const uint64_t c1 = std::min(c0 + chunk_rows, b);
    const uint64_t t0 = c0 > W ? c0 - W : 0, t1 = std::min<uint64_t>(c1 + W, cam.vsize);
    const DPixelMap tm = rows_map((t1 - t0) * cam.hsize, (uint32_t)t0);
    unsigned lds = 0, tile = 0;
    rc = drv.chunk(tm.n * N, c1 == b, [&] { rtc_launch_gen_rays(cam, tm, sp, 0, tm.n, s->d_srays, s->stream); }, [&] {
      lds = rtc_launch_resolve_filtered(f, sp, cam.hsize, t0, t1, c0, c1, s->d_srgb, d_rgb + 3 * (c0 - a) * cam.hsize, s->stream, &tile);
    });
    if (rc != RTC_OK) return rc;
    if (stats && std::getenv("RTC_SAMPLED_TIMING")) {  // debug aid (scripts/filter_probe.py)
      float g = 0.f, t = 0.f, r = 0.f;
      rc = chunk_parts_ms(s, &g, &t, &r);
      if (rc != RTC_OK) return rc;
      std::fprintf(stderr, "[rtc-filtered] chunk of %llu rays for %llu rows: generator %.3f ms, traces %.3f ms, filter %.3f ms (%s, tile %ux%u, %u B of LDS)\n",
                   (unsigned long long)(tm.n * N), (unsigned long long)(c1 - c0), g, t, r, lds ? "LDS" : "memory", tile >> 16, tile & 0xffffu, lds);
    }
  }
  drv.end(pm.n);
  return RTC_OK;
}

// One launch whose results go to the caller's host buffers: rgb (n x 3 doubles) or rgb8 (n x 3 bytes, Color::clamp on the device),
// and optionally the primary-hit records, all of the n pixels the launch leaves in the scene's buffers (ensure_px, ensure_rgb8).  The
// destination's pages are touched by host threads while the device renders, the copies are queued behind the kernels (see
// pretouch_pages above).  `body`: the launch itself -- run(), run_sampled(), run_adaptive(), run_filtered() or run_shutter() into
// s->d_rgb, synchronous, with the hook it is handed as their `after`.
int render_to_host(rtc_scene* s, uint64_t n, double* rgb, uint8_t* rgb8, rtc_hit* hits, const std::function<int(const AfterLaunch*)>& body) {
  static_assert(sizeof(DHit) == sizeof(rtc_hit) && offsetof(DHit, prim) == offsetof(rtc_hit, prim) && offsetof(DHit, k) == offsetof(rtc_hit, push_idx), "hit layout");
  std::vector<std::thread> pool;
  bool touched = false;
  const AfterLaunch after = [&]() -> int {
    if (!touched) {  // (a launch that is rendered again finds the pages present)
      touched = true;
      if (rgb) pretouch_pages(rgb, n * 3 * sizeof(double), &pool);
      if (rgb8) pretouch_pages(rgb8, n * 3, &pool);
      if (hits) pretouch_pages(hits, n * sizeof(rtc_hit), &pool);
    }
    if (rgb8) rtc_launch_quantize(s->d_rgb, s->d_rgb8, n * 3, s->stream);
    if (hits) rtc_launch_pack_hits(s->d_hit_t, s->d_hit_prim, s->d_hit_k, s->d_hits, n, s->stream);
    hipError_t e = hipGetLastError();
    join_all(&pool);
    if (e == hipSuccess && rgb) e = hipMemcpyAsync(rgb, s->d_rgb, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && rgb8) e = hipMemcpyAsync(rgb8, s->d_rgb8, n * 3, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && hits) e = hipMemcpyAsync(hits, s->d_hits, n * sizeof(rtc_hit), hipMemcpyDeviceToHost, s->stream);
    if (e != hipSuccess) return rtc_fail(RTC_ERR_DEVICE, std::string("copy to the host: ") + hipGetErrorString(e));
    return RTC_OK;
  };
  const int rc = body(&after);
  join_all(&pool);  // (an error before the hook ran its join)
  return rc;
}

// What the entry points with host pixels need on the device before their launch: the scene's device current, its pixel buffers for n
// pixels (`hits`: the packed hit records too; `rgb8`: the quantised pixels too).
int prepare_output(rtc_scene* s, uint64_t n, bool hits, bool rgb8) {
  HIP_OK(hipSetDevice(s->device));
  int rc = ensure_px(s, n, hits);
  if (rc == RTC_OK && rgb8) rc = ensure_rgb8(s, n);
  return rc;
}
// "empty camera" and, for a range (no index list), "pixel range exceeds the image"
int check_pixel_range(const rtc_camera* cam, const uint64_t* pixel_indices, uint64_t first, uint64_t n) {
  if (cam->hsize == 0 || cam->vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  if (!pixel_indices && first + n > cam->hsize * cam->vsize) return rtc_fail(RTC_ERR_INVALID, "pixel range exceeds the image");
  return RTC_OK;
}


}  // namespace

extern "C" {

const char* rtc_last_error(void) { return g_rtc_err.c_str(); }

int rtc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"

namespace {
// What a creation call was given, in the one form scene_create takes (scene_inputs fills it for all twelve rtc_*_create* entry points).
struct SceneInputs {
  rtc_scene_desc desc{};             // the caller's descriptor; without its lights once they were converted into `lights`
  bool ex = false;                   // the lights are lx[0 .. n_lx) for build_arrays_ex (desc.lights must be empty); else desc.lights
  const rtc_light_ex* lx = nullptr;
  uint32_t n_lx = 0;
  std::vector<rtc_light_ex> lights;  // desc->lights as point lights of an rtc_light_ex list: cones sit on lights of that form
  rtb::UvInput uv;                   // rtc_scene_create_ext: the UV pattern records and textures
  rtb::ConeInput cones;              // rtc_scene_create_ext2: the light cones (with ex == true only)
  bool has_bg = false;               // rtc_scene_create_ext3: the background
  rtc_background bg{};
  rtb::BumpInput bumps;              // rtc_scene_create_ext4: the bump records
};

// Fills `in` from a creation call's arguments and makes every check that needs no device, in this order: the descriptor, the bump
// records, the background, the cones.  `*out` (the caller's handle) is cleared first, so every failure leaves it NULL.
// Lights: `ext` with a light list, or `always_ex` (rtc_scene_create_ex: even an empty list), takes build_arrays_ex; cones on
// desc->lights convert those into such a list; everything else stays with desc->lights and build_arrays.
template <class Handle>
int scene_inputs(const rtc_scene_desc* desc, const rtc_scene_ext* ext, bool always_ex, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg,
                 const rtc_bump* bumps, uint32_t n_bumps, Handle** out, SceneInputs* in) {
  if (out) *out = nullptr;
  if (!desc) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  in->desc = *desc;
  std::string why;
  if (n_bumps > 0) {
    in->bumps = rtb::BumpInput{bumps, n_bumps};
    if (const int rc = rtb::validate_bumps(in->bumps, desc->n_materials, &why)) return rtc_fail(rc, why);
  }
  if (bg) {
    if (const int rc = rtb::validate_background(*bg, desc->n_pattern_nodes, &why)) return rtc_fail(rc, why);
    in->has_bg = true;
    in->bg = *bg;
  }
  if (ext) in->uv = rtb::UvInput{ext->uv_patterns, ext->n_uv_patterns, ext->textures, ext->n_textures};
  const bool ext_lights = ext && ext->n_lights > 0;
  in->ex = ext_lights || always_ex;
  if (in->ex) { in->lx = ext->lights; in->n_lx = ext->n_lights; }
  if (n_cones == 0) return RTC_OK;
  in->cones = rtb::ConeInput{cones, n_cones};
  if (const int rc = rtb::validate_cones(in->cones, ext_lights ? ext->n_lights : desc->n_lights, &why)) return rtc_fail(rc, why);
  if (ext_lights) return RTC_OK;
  if (desc->n_lights > 0 && !desc->lights) return rtc_fail(RTC_ERR_INVALID, "lights is NULL");
  in->lights.resize(desc->n_lights);
  for (uint32_t i = 0; i < desc->n_lights; i++) {
    rtc_light_ex x{};
    x.kind = RTC_LIGHT_POINT;
    std::memcpy(x.intensity, desc->lights[i].intensity, sizeof(x.intensity));
    std::memcpy(x.corner, desc->lights[i].origin, sizeof(x.corner));
    in->lights[i] = x;
  }
  in->desc.n_lights = 0; in->desc.lights = nullptr;
  in->ex = true; in->lx = in->lights.data(); in->n_lx = desc->n_lights;
  return RTC_OK;
}

// rtc_scene_create_ex / rtc_multi_create_ex: the light list alone, as an ext that holds nothing else
template <class Handle>
int scene_inputs_ex(const rtc_scene_desc* desc, const rtc_light_ex* lights, uint32_t n_lights, Handle** out, SceneInputs* in) {
  rtc_scene_ext ext{};
  ext.lights = lights; ext.n_lights = n_lights;
  return scene_inputs(desc, &ext, true, nullptr, 0, nullptr, nullptr, 0, out, in);
}

// One scene on one device from normalised inputs: its own checks (the handle, the device), then the host build (build_arrays or
// build_arrays_ex, which validate the descriptor and the lights), the upload and the per-scene launch parameters.
int scene_create(const SceneInputs& in, int device, rtc_scene** out) {
  if (!out) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  *out = nullptr;
  const rtc_scene_desc* desc = &in.desc;
  const rtb::BumpInput& bumps = in.bumps;
  const rtc_background* bg = in.has_bg ? &in.bg : nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rtc_fail(RTC_ERR_DEVICE, "no HIP device available (this library has no CPU path)");
  if (device < 0 || device >= ndev) return rtc_fail(RTC_ERR_DEVICE, "device index out of range");
  HIP_OK(hipSetDevice(device));
  rtb::HostArrays H;
  H.has_bg = (bg || bumps.n) ? 1 : 0;  // (bump records too: the NP builds read the program from memory, like the BG builds)
  std::string err;
  // Mesh accelerators of at least 100 000 triangles are built on the device (LBVH over extent-aware bisection keys, bvh_device.hip)
  // instead of by the host's binned SAH: same pixels (the accelerator is results-neutral), a quarter of the build time, frames
  // within 8 % of the SAH tree's (config 5: 11.8 vs 10.9 ms; profiles/r3_device_bvh_build.txt).  RTC_DEVICE_BVH=0: always the host
  // build; =1: the device build from 4 096 triangles up (RTC_DEVICE_BVH_MIN overrides either threshold).
  const char* dbe = std::getenv("RTC_DEVICE_BVH");
  const bool device_bvh = !(dbe && dbe[0] == '0');
  const size_t device_min = (dbe && dbe[0] == '1') ? 4096 : 100000;
  int rc = in.ex ? rtb::build_arrays_ex(*desc, in.lx, in.n_lx, &H, &err, device_bvh ? rtc_bvh_build_device : nullptr, device_min, in.uv, in.cones)
                 : rtb::build_arrays(*desc, &H, &err, device_bvh ? rtc_bvh_build_device : nullptr, device_min, in.uv);
  if (rc != RTC_OK) return rtc_fail(rc, err);
  const bool timing = std::getenv("RTC_TIMING") != nullptr;
  const auto t_up0 = std::chrono::steady_clock::now();

  // (every early return below releases what was created so far: streams, events, uploaded tables)
  struct SceneDeleter { void operator()(rtc_scene* p) const { rtc_scene_destroy(p); } };
  std::unique_ptr<rtc_scene, SceneDeleter> s(new rtc_scene());
  s->device = device;
  if (bg) { s->has_bg = true; s->bg = DBackground{bg->pattern, bg->projection}; s->bg_plain = desc->pattern_nodes[bg->pattern].tag == RTC_PAT_PLAIN; }
  HIP_OK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  HIP_OK(hipEventCreate(&s->ev0));
  HIP_OK(hipEventCreate(&s->ev1));
  HIP_OK(hipEventCreate(&s->evs0));
  HIP_OK(hipEventCreate(&s->evs1));
  for (auto& m : s->marker) HIP_OK(hipEventCreate(&m));

  DScene& d = s->d;
#define UP(field)                                                       \
  do {                                                                  \
    int rc_ = s->upload(H.field, &d.field);                             \
    if (rc_ != RTC_OK) return rc_;                                      \
  } while (0)
  UP(ops); UP(group_box); UP(group_parent); UP(bvh); UP(mtri); UP(mtri_prim); {
    int rc_ = s->upload(H.items, &d.item_prim);
    if (rc_ != RTC_OK) return rc_;
    d.quirk_prim = d.item_prim;
    d.qitem = d.item_prim;
  }
  UP(qgrids); UP(qcell); UP(bvh_frame); UP(csg); UP(prims); UP(pisect); UP(xf_inv); UP(xf_matinv); UP(limits);
  UP(tri_geo); UP(tri_nrm); UP(mat); UP(mat_pattern); UP(pats); UP(lights);
#undef UP
  if (bumps.n) {  // the bump table: a record index per material, -1 without one
    std::vector<int32_t> mat_bump(desc->n_materials, -1);
    std::vector<DBump> recs(bumps.n);
    for (uint32_t k = 0; k < bumps.n; k++) {
      const rtc_bump& b = bumps.bumps[k];
      mat_bump[b.material] = (int32_t)k;
      recs[k] = DBump{b.kind, b.octaves, b.amplitude, b.frequency};
    }
    if (const int rc_ = s->upload(mat_bump, &s->bump.mat_bump)) return rc_;
    if (const int rc_ = s->upload(recs, &s->bump.recs)) return rc_;
    s->has_bump = true;
    s->n_bumps = bumps.n;
  }
  d.n_ops = (int32_t)H.ops.size();
  d.n_prims = (int32_t)H.prims.size();
  d.n_recs = H.recs_bg_only ? 0 : (int32_t)H.pisect.size();
  d.n_lights = H.n_lights;
  d.all_cast_shadow = H.all_cast_shadow;
  {
    DScene hv = H.view();
    d.bvh_stack = hv.bvh_stack;
    d.has_mesh = hv.has_mesh;
    d.has_csg = hv.has_csg;
    d.has_groups = hv.has_groups;
    d.has_recs = hv.has_recs;
    d.all_plain = hv.all_plain;
    d.no_glass_mirror = hv.no_glass_mirror;
    d.backface_skip = hv.backface_skip;
    d.light_grid_first = hv.light_grid_first;
    d.quirk_reach2 = hv.quirk_reach2;
    std::memcpy(d.abvh_frame, hv.abvh_frame, sizeof(d.abvh_frame));
    d.light_grid_n = hv.light_grid_n; d.light_grid_cell_off = hv.light_grid_cell_off;
    d.csg_max_hits = hv.csg_max_hits;
    d.csg_slab = nullptr;
    d.n_kops = hv.n_kops; d.n_kplanes = hv.n_kplanes;
    std::memcpy(d.kops, hv.kops, sizeof(d.kops));
    std::memcpy(d.kplanes, hv.kplanes, sizeof(d.kplanes));
    std::memcpy(d.kaux, hv.kaux, sizeof(d.kaux));
    d.kqgrid = hv.kqgrid;
    d.n_bvh = hv.n_bvh; d.n_items = hv.n_items; d.n_mtri = hv.n_mtri; d.n_quirk = hv.n_quirk;
    d.n_qitem = hv.n_qitem; d.n_qcell = hv.n_qcell; d.n_groups = hv.n_groups; d.n_qgrids = hv.n_qgrids;
    d.has_area = hv.has_area;
    d.has_uv = hv.has_uv;
    d.has_spot = hv.has_spot;
  }
  s->n_prims_total = desc->n_prims;
  for (uint32_t i = 0; i < desc->n_prims; i++) {
    const rtc_prim& P = desc->prims[i];
    if (P.geometry != RTC_PLANE && P.geometry != RTC_TRIANGLE && P.geometry != RTC_SMOOTH_TRIANGLE) s->n_analytic++;
    if (P.material >= 0 && (uint32_t)P.material < desc->n_materials) {
      const rtc_material& M = desc->materials[P.material];
      if (M.reflective != 0.0 || M.transparency != 0.0) s->n_bouncing++;
    }
  }
  s->bvh_depth = H.bvh_depth;
  s->built_on_device = H.built_on_device;
  s->n_bvh_nodes = (uint32_t)H.bvh.size();
  s->n_mesh_tris = (uint32_t)H.mtri_prim.size();
  if (std::getenv("RTC_VERIFY_UPLOAD")) {  // debug aid: read every table back and compare with the host copy
    auto verify = [&](const char* name, const void* dev, const void* host, size_t bytes) {
      if (!bytes) return true;
      std::vector<unsigned char> back(bytes);
      if (hipMemcpy(back.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
      if (std::memcmp(back.data(), host, bytes) != 0) { std::fprintf(stderr, "[rtc] upload mismatch in %s (%zu bytes)\n", name, bytes); return false; }
      return true;
    };
    bool ok = verify("items", d.item_prim, H.items.data(), H.items.size() * 4);
    ok = verify("qcell", d.qcell, H.qcell.data(), H.qcell.size() * 4) && ok;
    ok = verify("ops", d.ops, H.ops.data(), H.ops.size() * sizeof(DOp)) && ok;
    std::fprintf(stderr, "[rtc] upload verify: %s; n_items=%zu n_qcell=%zu n_prims=%zu\n", ok ? "ok" : "MISMATCH", H.items.size(), H.qcell.size(), H.prims.size());
  }
  if (timing) std::fprintf(stderr, "[rtc-timing] %-28s %.3f s (%.1f MB)\n", "upload", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_up0).count(), (double)s->bytes / 1e6);
  HIP_OK(hipMalloc((void**)&s->d_stats, sizeof(DStats)));
  HIP_OK(hipMemset(s->d_stats, 0, sizeof(DStats)));
  {
    // RTC_KERNEL pins a device path for A/B runs and for the parity tests: 1 = one kernel per frame, 4 = wavefront kernels (every
    // launch, pixel lists and explicit rays included); unset = measured choice per launch shape.
    const char* kv = std::getenv("RTC_KERNEL");
    const int kvi = kv ? std::atoi(kv) : 0;
    s->kernel_version = (kvi == 1 || kvi == 4) ? kvi : 0;
    // RTC_WF_LDS=0: the wavefront traversal reads this scene's tables from memory (A/B runs, the build tests); pinned here likewise
    const char* le = std::getenv("RTC_WF_LDS");
    s->lds_bytes = rtc_wavefront_lds_bytes(s->d, !(le && le[0] == '0'));
    // hipDeviceGetAttribute, not hipGetDeviceProperties: the property struct's layout differs between ROCm releases and
    // this library may run on the HIP runtime PyTorch loaded first.
    int n_cu = 0;
    HIP_OK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    // traversal kernel: a persistent grid of one-wave blocks, as many as the chip holds; shading kernel: two 512-thread blocks per CU
    s->wave_blocks = rtc_wavefront_grid(s->d, n_cu);
    if (const char* w = std::getenv("RTC_WF_BLOCKS_PER_CU")) s->wave_blocks = (unsigned)std::max(1, n_cu * std::atoi(w));
    s->shade_blocks = (unsigned)std::max(1, n_cu * 2);
    if (const char* w = std::getenv("RTC_WF_SHADE_BLOCKS_PER_CU")) s->shade_blocks = (unsigned)std::max(1, n_cu * std::atoi(w));
    // the LDS-resident traversal build: one block per CU, whatever the shading grid is; RTC_WF_SPARE_CUS=k: its unsynchronised launches
    // leave k CUs out while another scene is alive on the device (lds_grid), pinned here as the switches above are
    s->n_cu = std::max(1, n_cu);
    const char* sp = std::getenv("RTC_WF_SPARE_CUS");
    s->spare_cus = std::min(std::max(sp ? std::atoi(sp) : rtc_wavefront_spare_cus_default(s->n_cu), 0), s->n_cu - 1);
  }
  if (device >= 0 && device < RTC_LIVE_DEVICES) {
    g_live_scenes[device].fetch_add(1, std::memory_order_relaxed);
    s->counted = true;
  }
  *out = s.release();
  return RTC_OK;
}
}  // namespace

extern "C" {

// The six entry points differ in what they can be given; what they are not given is empty (include/rtc.h).
int rtc_scene_create(const rtc_scene_desc* desc, int device, rtc_scene** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, nullptr, false, nullptr, 0, nullptr, nullptr, 0, out, &in)) return rc;
  return scene_create(in, device, out);
}
int rtc_scene_create_ex(const rtc_scene_desc* desc, const rtc_light_ex* lights, uint32_t n_lights, int device, rtc_scene** out) {
  SceneInputs in;
  if (const int rc = scene_inputs_ex(desc, lights, n_lights, out, &in)) return rc;
  return scene_create(in, device, out);
}
int rtc_scene_create_ext(const rtc_scene_desc* desc, const rtc_scene_ext* ext, int device, rtc_scene** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, ext, false, nullptr, 0, nullptr, nullptr, 0, out, &in)) return rc;
  return scene_create(in, device, out);
}
int rtc_scene_create_ext2(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, int device, rtc_scene** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, ext, false, cones, n_cones, nullptr, nullptr, 0, out, &in)) return rc;
  return scene_create(in, device, out);
}
int rtc_scene_create_ext3(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg, int device,
                          rtc_scene** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, ext, false, cones, n_cones, bg, nullptr, 0, out, &in)) return rc;
  return scene_create(in, device, out);
}
int rtc_scene_create_ext4(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg,
                          const rtc_bump* bumps, uint32_t n_bumps, int device, rtc_scene** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, ext, false, cones, n_cones, bg, bumps, n_bumps, out, &in)) return rc;
  return scene_create(in, device, out);
}

int rtc_bump_normal(const rtc_bump* bump, const double material_inv[16], const double point[3], const double normal[3], double out[3]) {
  if (!bump || !material_inv || !point || !normal || !out) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (const char* why = rtb::bump_invalid(*bump)) return rtc_fail(RTC_ERR_INVALID, std::string("bump: ") + why);
  rtc_bump_normal_at(bump->kind, bump->octaves, bump->amplitude, bump->frequency, material_inv, point[0], point[1], point[2], normal, out);
  return RTC_OK;
}

int rtc_bump_normals(rtc_scene* s, const int32_t* prims, const double* points, const double* normals, uint64_t n, double* out) {
  if (!s || (n && (!prims || !points || !normals || !out))) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (n == 0) return RTC_OK;
  for (uint64_t i = 0; i < n; i++)
    if (prims[i] < 0 || prims[i] >= s->d.n_prims) return rtc_fail(RTC_ERR_INVALID, "bump_normals: primitive index out of range");
  if (!s->has_bump) {  // no record anywhere: every primitive gets its normal back
    std::memcpy(out, normals, n * 3 * sizeof(double));
    return RTC_OK;
  }
  HIP_OK(hipSetDevice(s->device));
  int rc = ensure_px(s, n, true);  // d_rgb: 3 rows of n doubles; d_hit_prim: n ints
  if (rc == RTC_OK) rc = ensure_rays(s, n);  // d_rays: 6 rows of n doubles (the points' rows, then the normals')
  if (rc != RTC_OK) return rc;
  std::vector<double> soa(6 * n);  // the kernel reads rows: a wave's loads are whole lines
  for (uint64_t i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) { soa[c * n + i] = points[3 * i + c]; soa[(3 + c) * n + i] = normals[3 * i + c]; }
  HIP_OK(hipMemcpyAsync(s->d_rays, soa.data(), 6 * n * sizeof(double), hipMemcpyHostToDevice, s->stream));
  HIP_OK(hipMemcpyAsync(s->d_hit_prim, prims, n * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
  rtc_launch_bump_normals(s->d, s->bump, s->d_hit_prim, s->d_rays, s->d_rays + 3 * n, n, s->d_rgb, s->stream);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(soa.data(), s->d_rgb, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  for (uint64_t i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) out[3 * i + c] = soa[c * n + i];
  return RTC_OK;
}

int rtc_scene_bump_info(const rtc_scene* s, rtc_bump_info* out) {
  if (!s || !out) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  out->trace_build = out->wf_shade_build = -1;
  if (!s->has_bump) return RTC_OK;
  out->has_bump = 1;
  out->n_bumps = s->n_bumps;
  out->trace_build = rtc_ext_trace_build(s->d, s->ext());
  out->trace_area = s->d.has_area || s->d.has_spot; out->trace_uv = s->d.has_uv; out->trace_spot = s->d.has_spot; out->trace_bg = s->has_bg ? 1 : 0;
  out->wf_shade_build = s->d.has_uv ? RTC_WF_NP_UV : RTC_WF_NP_PLAIN;
  return RTC_OK;
}

int rtc_background_point(int32_t projection, const double dir[3], double point[3]) {
  if (!dir || !point) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (projection != RTC_BG_DIRECTION && projection != RTC_BG_CUBE) return rtc_fail(RTC_ERR_INVALID, "background: unknown projection");
  rtc_background_point_at(projection, dir[0], dir[1], dir[2], point);
  return RTC_OK;
}

int rtc_background_colors(rtc_scene* s, const double* dirs, uint64_t n, double* rgb) {
  if (!s || (!dirs && n) || (!rgb && n)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (!s->has_bg) return rtc_fail(RTC_ERR_INVALID, "the scene has no background");
  if (n == 0) return RTC_OK;
  HIP_OK(hipSetDevice(s->device));
  int rc = ensure_px(s, n, false);  // d_rgb: n x 3 doubles
  if (rc == RTC_OK) rc = ensure_rays(s, (n + 1) / 2);  // d_rays holds 6 doubles per ray: n directions need half as many
  if (rc != RTC_OK) return rc;
  HIP_OK(hipMemcpyAsync(s->d_rays, dirs, n * 3 * sizeof(double), hipMemcpyHostToDevice, s->stream));
  rtc_launch_background_colors(s->d, s->bg, s->d_rays, n, s->d_rgb, s->stream);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(rgb, s->d_rgb, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  return RTC_OK;
}

int rtc_scene_background_info(const rtc_scene* s, rtc_background_info* out) {
  if (!s || !out) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  out->pattern = out->trace_build = out->wf_background_build = -1;
  out->projection = -1;
  if (!s->has_bg) return RTC_OK;
  out->has_background = 1;
  out->pattern = s->bg.pattern; out->projection = s->bg.projection;
  out->trace_build = rtc_ext_trace_build(s->d, RtcSceneExt{&s->bg, nullptr});  // (of the background alone: a bumped scene's is rtc_scene_bump_info's)
  out->trace_area = s->d.has_area || s->d.has_spot; out->trace_uv = s->d.has_uv; out->trace_spot = s->d.has_spot;
  out->wf_background_build = s->d.has_uv ? RTC_WF_BG_UV : RTC_WF_BG_PLAIN;
  out->plain_root = s->bg_plain ? 1 : 0;
  return RTC_OK;
}

int rtc_spot_factor(const rtc_light_cone* cone, const double light_pos[3], const double point[3], double* f) {
  if (!cone || !light_pos || !point || !f) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (const char* why = rth::cone_invalid(cone->axis, cone->cos_inner, cone->cos_outer)) return rtc_fail(RTC_ERR_INVALID, std::string("cone: ") + why);
  double a[3];
  rtc_spot_axis(cone->axis, a);
  *f = rtc_spot_factor_at(a, cone->cos_inner, cone->cos_outer, light_pos, point);
  return RTC_OK;
}

int rtc_texture_sample(const rtc_texture* tex, int32_t kind, double u, double v, double rgb[3]) {
  if (!tex || !rgb) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (kind < RTC_UV_IMAGE || kind > RTC_UV_IMAGE_LINEAR_WRAP) return rtc_fail(RTC_ERR_INVALID, "kind is not an image kind (RTC_UV_IMAGE .. RTC_UV_IMAGE_LINEAR_WRAP)");
  if (tex->width == 0 || tex->height == 0) return rtc_fail(RTC_ERR_INVALID, "texture of width or height 0");
  if (tex->width > RTC_TEXTURE_MAX_SIDE || tex->height > RTC_TEXTURE_MAX_SIDE) return rtc_fail(RTC_ERR_INVALID, "a texture side above RTC_TEXTURE_MAX_SIDE");
  if (!tex->rgb) return rtc_fail(RTC_ERR_INVALID, "texture rgb is NULL");
  const int w = (int)tex->width, h = (int)tex->height;
  if (kind == RTC_UV_IMAGE) {  // uv_lookup's nearest texel (rtc_device.hpp), restated
    int xi = as_i32(round(u * (double)(w - 1))), yi = as_i32(round((1.0 - v) * (double)(h - 1)));
    xi = xi < 0 ? 0 : (xi > w - 1 ? w - 1 : xi);
    yi = yi < 0 ? 0 : (yi > h - 1 ? h - 1 : yi);
    std::memcpy(rgb, tex->rgb + 3 * ((int64_t)yi * w + xi), 3 * sizeof(double));
  } else {
    rtc_uv_image_linear(tex->rgb, w, h, kind, u, v, rgb);
  }
  return RTC_OK;
}

void rtc_scene_destroy(rtc_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (void* p : s->allocs) (void)hipFree(p);
  if (s->d_stats) (void)hipFree(s->d_stats);
  (void)hipFree(s->d_rgb); (void)hipFree(s->d_hit_t); (void)hipFree(s->d_hit_prim); (void)hipFree(s->d_hit_k);
  (void)hipFree(s->d_hits); (void)hipFree(s->d_rgb8); (void)hipFree(s->d_digest); (void)hipFree(s->d_wave_dig);
  if (s->wave_mem) (void)hipFree(s->wave_mem);
  (void)hipFree(s->csg_slab);
  if (s->d_idx) (void)hipFree(s->d_idx);
  if (s->d_rays) (void)hipFree(s->d_rays);
  (void)hipFree(s->d_srays); (void)hipFree(s->d_srgb);
  (void)hipFree(s->d_alist); (void)hipFree(s->d_awork); (void)hipFree(s->d_acount);
  (void)hipFree(s->d_shorder); (void)hipFree(s->d_shwhere); (void)hipFree(s->d_shwork);
  if (s->evs0) (void)hipEventDestroy(s->evs0);
  if (s->evs1) (void)hipEventDestroy(s->evs1);
  for (auto& m : s->marker) if (m) (void)hipEventDestroy(m);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  if (s->counted) g_live_scenes[s->device].fetch_sub(1, std::memory_order_relaxed);
  delete s;
}

uint64_t rtc_scene_device_bytes(const rtc_scene* s) { return s ? s->bytes : 0; }

int rtc_render(rtc_scene* s, const rtc_camera* cam, int32_t fuel, const uint64_t* pixel_indices, uint64_t first, uint64_t n, double* rgb, rtc_hit* hits,
               rtc_stats* stats) {
  if (!s || !cam || (!rgb && n)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_pixel_range(cam, pixel_indices, first, n);
  if (rc != RTC_OK) return rc;
  if (n == 0) { if (stats) std::memset(stats, 0, sizeof(*stats)); return RTC_OK; }
  rc = prepare_output(s, n, hits != nullptr, false);
  if (rc != RTC_OK) return rc;
  DPixelMap pm{};
  std::vector<uint64_t> range_idx;
  rc = make_pixel_map(s, cam, pixel_indices, first, n, &pm, &range_idx);
  if (rc != RTC_OK) return rc;
  DCamera dc;
  to_dcam(*cam, &dc);
  return render_to_host(s, n, rgb, nullptr, hits, [&](const AfterLaunch* after) { return run(s, dc, pm, fuel, s->d_rgb, hits != nullptr, stats, stats != nullptr, true, 0, after); });
}

int rtc_render_hit_digest(rtc_scene* s, const rtc_camera* cam, int32_t fuel, const uint64_t* pixel_indices, uint64_t first, uint64_t n, uint64_t* digest) {
  if (!s || !cam || (!digest && n)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_pixel_range(cam, pixel_indices, first, n);
  if (rc != RTC_OK) return rc;
  if (n == 0) return RTC_OK;
  rc = prepare_output(s, n, false, false);
  if (rc == RTC_OK) rc = grow(&s->cap_digest, n, {{(void**)&s->d_digest, n * sizeof(unsigned long long)}});
  if (rc != RTC_OK) return rc;
  DPixelMap pm{};
  std::vector<uint64_t> range_idx;
  rc = make_pixel_map(s, cam, pixel_indices, first, n, &pm, &range_idx);
  if (rc != RTC_OK) return rc;
  pm.digest = s->d_digest;
  DCamera dc;
  to_dcam(*cam, &dc);
  rtc_stats st;
  rc = run(s, dc, pm, fuel, s->d_rgb, false, &st, true, true);   // the counting variants carry the digest code
  if (rc != RTC_OK) return rc;
  HIP_OK(hipMemcpy(digest, s->d_digest, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return RTC_OK;
}

int rtc_render_rgb8(rtc_scene* s, const rtc_camera* cam, int32_t fuel, uint8_t* rgb8, rtc_stats* stats) {
  if (!s || !cam || !rgb8) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (cam->hsize == 0 || cam->vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  const uint64_t n = cam->hsize * cam->vsize;
  const int rc = prepare_output(s, n, false, true);
  if (rc != RTC_OK) return rc;
  const DPixelMap pm = rows_map(n);
  DCamera dc;
  to_dcam(*cam, &dc);
  return render_to_host(s, n, nullptr, rgb8, nullptr, [&](const AfterLaunch* after) { return run(s, dc, pm, fuel, s->d_rgb, false, stats, stats != nullptr, true, 0, after); });
}

// Rows of the image owned by part `first` of `step` when bands of `band` rows are dealt out round-robin (the last band of the image
// may be short).
static uint64_t band_rows_owned(uint64_t vsize, uint32_t band, uint32_t first, uint32_t step) {
  const uint64_t n_bands = (vsize + band - 1) / band;
  if (first >= n_bands) return 0;
  const uint64_t mine = (n_bands - first + step - 1) / step;
  uint64_t rows = mine * band;
  const uint64_t last = first + (mine - 1) * (uint64_t)step;  // my last band; short only if it is the image's last
  if (last == n_bands - 1) rows -= n_bands * band - vsize;
  return rows;
}

int rtc_render_bands_device(rtc_scene* s, const rtc_camera* cam, int32_t fuel, uint32_t band_rows, uint32_t band_first, uint32_t band_step, uint32_t n_rows,
                            double* rgb_dev, rtc_stats* stats, int count_stats, int sync) {
  if (!s || !cam || (!rgb_dev && n_rows)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (band_step == 0 || band_rows == 0) return rtc_fail(RTC_ERR_INVALID, "band_rows and band_step must be >= 1");
  if (n_rows) {
    // the launch covers the first n_rows rows of this part's dense tile: whole bands, then possibly part of one
    const uint64_t j = n_rows - 1, last_row = ((uint64_t)band_first + (j / band_rows) * band_step) * band_rows + j % band_rows;
    if (last_row >= cam->vsize) return rtc_fail(RTC_ERR_INVALID, "rows exceed the image");
  }
  DPixelMap pm{};
  pm.n = (uint64_t)n_rows * cam->hsize;
  pm.mode = 2; pm.row_first = band_first; pm.row_step = band_step; pm.band = band_rows;
  if (pm.n == 0) { if (stats) std::memset(stats, 0, sizeof(*stats)); return RTC_OK; }
  DCamera dc;
  to_dcam(*cam, &dc);
  return run(s, dc, pm, fuel, rgb_dev, false, stats, count_stats != 0, sync != 0);
}

int rtc_render_rows_device(rtc_scene* s, const rtc_camera* cam, int32_t fuel, uint32_t row_first, uint32_t row_step, uint32_t n_rows, double* rgb_dev,
                           rtc_stats* stats, int count_stats, int sync) {
  return rtc_render_bands_device(s, cam, fuel, 1, row_first, row_step, n_rows, rgb_dev, stats, count_stats, sync);
}

uint64_t rtc_band_rows_owned(uint64_t vsize, uint32_t band_rows, uint32_t band_first, uint32_t band_step) {
  if (band_rows == 0 || band_step == 0) return 0;
  return band_rows_owned(vsize, band_rows, band_first, band_step);
}

int rtc_trace_rays(rtc_scene* s, const double* rays, uint64_t n, int32_t fuel, double* rgb, rtc_hit* hits, rtc_stats* stats) {
  if (!s || (!rays && n) || (!rgb && n)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (n == 0) return RTC_OK;
  int rc = prepare_output(s, n, hits != nullptr, false);
  if (rc == RTC_OK) rc = ensure_rays(s, n);
  if (rc != RTC_OK) return rc;
  HIP_OK(hipMemcpyAsync(s->d_rays, rays, n * 6 * sizeof(double), hipMemcpyHostToDevice, s->stream));
  DPixelMap pm{};
  pm.n = n; pm.mode = 3; pm.rays = s->d_rays;
  DCamera dc{};
  dc.hsize = 1; dc.vsize = 1;
  return render_to_host(s, n, rgb, nullptr, hits, [&](const AfterLaunch* after) { return run(s, dc, pm, fuel, s->d_rgb, hits != nullptr, stats, stats != nullptr, true, 0, after); });
}

// ---- the sampled camera's entry points (include/rtc.h) ---------------------------------------------------------------------------
int rtc_render_sampled(rtc_scene* s, const rtc_camera* cam, const rtc_sampling* sp, int32_t fuel, const uint64_t* pixel_indices, uint64_t first, uint64_t n,
                       double* rgb, rtc_stats* stats) {
  if (!s || !cam || !sp || (!rgb && n)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_sampling(sp);
  if (rc == RTC_OK) rc = check_pixel_range(cam, pixel_indices, first, n);
  if (rc != RTC_OK) return rc;
  if (n == 0) { if (stats) std::memset(stats, 0, sizeof(*stats)); return RTC_OK; }
  rc = prepare_output(s, n, false, false);
  if (rc != RTC_OK) return rc;
  DPixelMap pm{};
  std::vector<uint64_t> range_idx;
  rc = make_pixel_map(s, cam, pixel_indices, first, n, &pm, &range_idx);
  if (rc != RTC_OK) return rc;
  DCamera dc;
  to_dcam(*cam, &dc);
  return render_to_host(s, n, rgb, nullptr, nullptr, [&](const AfterLaunch* after) { return run_sampled(s, dc, pm, *sp, fuel, s->d_rgb, stats, stats != nullptr, true, after); });
}

int rtc_render_sampled_rgb8(rtc_scene* s, const rtc_camera* cam, const rtc_sampling* sp, int32_t fuel, uint8_t* rgb8, rtc_stats* stats) {
  if (!s || !cam || !sp || !rgb8) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_sampling(sp);
  if (rc != RTC_OK) return rc;
  if (cam->hsize == 0 || cam->vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  const uint64_t n = cam->hsize * cam->vsize;
  rc = prepare_output(s, n, false, true);
  if (rc != RTC_OK) return rc;
  const DPixelMap pm = rows_map(n);
  DCamera dc;
  to_dcam(*cam, &dc);
  return render_to_host(s, n, nullptr, rgb8, nullptr, [&](const AfterLaunch* after) { return run_sampled(s, dc, pm, *sp, fuel, s->d_rgb, stats, stats != nullptr, true, after); });
}


int rtc_render_sampled_bands_device(rtc_scene* s, const rtc_camera* cam, const rtc_sampling* sp, int32_t fuel, uint32_t band_rows, uint32_t band_first,
                                    uint32_t band_step, uint32_t n_rows, double* rgb_dev, rtc_stats* stats, int count_stats, int sync) {
  if (!s || !cam || !sp || (!rgb_dev && n_rows)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_sampling(sp);
  if (rc != RTC_OK) return rc;
  if (band_step == 0 || band_rows == 0) return rtc_fail(RTC_ERR_INVALID, "band_rows and band_step must be >= 1");
  if (cam->hsize == 0 || cam->vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  if (n_rows) {
    const uint64_t j = n_rows - 1, last_row = ((uint64_t)band_first + (j / band_rows) * band_step) * band_rows + j % band_rows;
    if (last_row >= cam->vsize) return rtc_fail(RTC_ERR_INVALID, "rows exceed the image");
  }
  DPixelMap pm{};
  pm.n = (uint64_t)n_rows * cam->hsize;
  pm.mode = 2; pm.row_first = band_first; pm.row_step = band_step; pm.band = band_rows;
  if (pm.n == 0) { if (stats) std::memset(stats, 0, sizeof(*stats)); return RTC_OK; }
  DCamera dc;
  to_dcam(*cam, &dc);
  return run_sampled(s, dc, pm, *sp, fuel, rgb_dev, stats, count_stats != 0, sync != 0);
}

int rtc_camera_rays(rtc_scene* s, const rtc_camera* cam, const rtc_sampling* sp, const uint64_t* pixel_indices, uint64_t first, uint64_t n, double* rays) {
  if (!cam || !sp || (!rays && n)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_sampling(sp);
  if (rc != RTC_OK) return rc;
  if (cam->hsize == 0 || cam->vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  const uint64_t total = cam->hsize * cam->vsize;
  if (!pixel_indices && (first > total || n > total - first)) return rtc_fail(RTC_ERR_INVALID, "pixel range exceeds the image");
  if (n == 0) return RTC_OK;
  const uint64_t N = (uint64_t)sp->side * sp->side;
  DCamera dc;
  to_dcam(*cam, &dc);
  if (!s) {  // the same function on the host
    for (uint64_t j = 0; j < n; j++) {
      const uint64_t i = pixel_indices ? pixel_indices[j] : first + j;
      if (i >= total) return rtc_fail(RTC_ERR_INVALID, "pixel index exceeds the image");
      for (uint64_t k = 0; k < N; k++) rtc_sample_ray(dc, *sp, i, (uint32_t)k, rays + 6 * (j * N + k));
    }
    return RTC_OK;
  }
  HIP_OK(hipSetDevice(s->device));
  DPixelMap pm{};
  std::vector<uint64_t> range_idx;
  rc = make_pixel_map(s, cam, pixel_indices, first, n, &pm, &range_idx);
  if (rc != RTC_OK) return rc;
  rc = ensure_sampled(s, n * N, false);
  if (rc != RTC_OK) return rc;
  rtc_launch_gen_rays(dc, pm, *sp, 0, n, s->d_srays, s->stream);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(rays, s->d_srays, n * N * 6 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  return RTC_OK;
}

// ---- adaptive sampling's entry points (include/rtc.h) -------------------------------------------------------------------------------
static int render_adaptive(rtc_scene* s, const rtc_camera* cam, const rtc_adaptive* ad, int32_t fuel, double* rgb, uint8_t* rgb8, uint8_t* mask, uint64_t* n_refined,
                           rtc_stats* stats) {
  int rc = check_adaptive(ad);  // (the rule first: it is checked without a device)
  if (rc != RTC_OK) return rc;
  if (!s || !cam || (!rgb && !rgb8)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (cam->hsize == 0 || cam->vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  rc = check_contrast_frame(cam->hsize, cam->vsize);
  if (rc != RTC_OK) return rc;
  const uint64_t n = cam->hsize * cam->vsize;
  rc = prepare_output(s, n, false, rgb8 != nullptr);
  if (rc != RTC_OK) return rc;
  DCamera dc;
  to_dcam(*cam, &dc);
  return render_to_host(s, n, rgb, rgb8, nullptr, [&](const AfterLaunch* after) { return run_adaptive(s, dc, *ad, fuel, stats, mask, n_refined, after); });
}


int rtc_render_adaptive(rtc_scene* s, const rtc_camera* cam, const rtc_adaptive* ad, int32_t fuel, double* rgb, uint8_t* mask, uint64_t* n_refined, rtc_stats* stats) {
  return render_adaptive(s, cam, ad, fuel, rgb, nullptr, mask, n_refined, stats);
}

int rtc_render_adaptive_rgb8(rtc_scene* s, const rtc_camera* cam, const rtc_adaptive* ad, int32_t fuel, uint8_t* rgb8, uint8_t* mask, uint64_t* n_refined,
                             rtc_stats* stats) {
  return render_adaptive(s, cam, ad, fuel, nullptr, rgb8, mask, n_refined, stats);
}

int rtc_contrast_pixels(rtc_scene* s, uint64_t hsize, uint64_t vsize, const double* rgb, double threshold, uint32_t neighbours, uint64_t* indices, uint64_t* n) {
  if (!rgb || !indices || !n) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (std::isnan(threshold)) return rtc_fail(RTC_ERR_INVALID, "adaptive: threshold is NaN");
  if (neighbours != 4 && neighbours != 8) return rtc_fail(RTC_ERR_INVALID, "adaptive: neighbours must be 4 or 8");
  int rc = check_contrast_frame(hsize, vsize);
  if (rc != RTC_OK) return rc;
  const uint64_t total = hsize * vsize;
  if (!s) {  // the same function on the host
    uint64_t k = 0;
    for (uint64_t i = 0; i < total; i++)
      if (rtc_contrast_refined(rgb, hsize, vsize, i, threshold, neighbours)) indices[k++] = i;
    *n = k;
    return RTC_OK;
  }
  HIP_OK(hipSetDevice(s->device));
  rc = ensure_px(s, total, false);
  if (rc != RTC_OK) return rc;
  HIP_OK(hipMemcpyAsync(s->d_rgb, rgb, total * 3 * sizeof(double), hipMemcpyHostToDevice, s->stream));
  uint64_t refined = 0;
  unsigned n_kernels = 0;
  rc = contrast_compact(s, s->d_rgb, hsize, vsize, threshold, neighbours, &refined, &n_kernels, false);
  if (rc != RTC_OK) return rc;
  if (refined) HIP_OK(hipMemcpy(indices, s->d_alist, refined * sizeof(uint64_t), hipMemcpyDeviceToHost));
  *n = refined;
  return RTC_OK;
}

// ---- the shutter's entry points (include/rtc.h) ---------------------------------------------------------------------------------------
static int render_shutter(rtc_scene* const* scenes, const rtc_camera* cameras, uint32_t n_poses, const rtc_shutter* sh, const rtc_sampling* sp, int32_t fuel,
                          const uint64_t* pixel_indices, uint64_t first, uint64_t n, bool whole, double* rgb, uint8_t* rgb8, rtc_stats* stats) {
  int rc = check_shutter(sh, n_poses, sp);  // (the rule first: it is checked without a device)
  if (rc == RTC_OK) rc = check_poses(scenes, cameras, n_poses);
  if (rc != RTC_OK) return rc;
  const uint64_t total = cameras[0].hsize * cameras[0].vsize;
  if (whole) n = total;
  if ((!rgb && !rgb8) && n) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (!pixel_indices && (first > total || n > total - first)) return rtc_fail(RTC_ERR_INVALID, "pixel range exceeds the image");
  if (n == 0) { if (stats) std::memset(stats, 0, sizeof(*stats)); return RTC_OK; }
  rtc_scene* s = scenes[0];
  rc = prepare_output(s, n, false, rgb8 != nullptr);
  if (rc != RTC_OK) return rc;
  DPixelMap pm{};
  std::vector<uint64_t> range_idx;
  rc = make_pixel_map(s, &cameras[0], pixel_indices, first, n, &pm, &range_idx);
  if (rc != RTC_OK) return rc;
  std::vector<DCamera> cams(n_poses);
  for (uint32_t p = 0; p < n_poses; p++) to_dcam(cameras[p], &cams[p]);
  return render_to_host(s, n, rgb, rgb8, nullptr, [&](const AfterLaunch* after) { return run_shutter(scenes, cams.data(), n_poses, *sh, pm, *sp, fuel, s->d_rgb, stats, after); });
}


int rtc_render_shutter(rtc_scene* const* scenes, const rtc_camera* cameras, uint32_t n_poses, const rtc_shutter* sh, const rtc_sampling* sp, int32_t fuel,
                       const uint64_t* pixel_indices, uint64_t first, uint64_t n, double* rgb, rtc_stats* stats) {
  return render_shutter(scenes, cameras, n_poses, sh, sp, fuel, pixel_indices, first, n, false, rgb, nullptr, stats);
}

int rtc_render_shutter_rgb8(rtc_scene* const* scenes, const rtc_camera* cameras, uint32_t n_poses, const rtc_shutter* sh, const rtc_sampling* sp, int32_t fuel,
                            uint8_t* rgb8, rtc_stats* stats) {
  if (!rgb8) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  return render_shutter(scenes, cameras, n_poses, sh, sp, fuel, nullptr, 0, 0, true, nullptr, rgb8, stats);
}

int rtc_shutter_deal(rtc_scene* s, uint64_t hsize, uint32_t n_poses, const rtc_shutter* sh, const rtc_sampling* sp, const uint64_t* pixel_indices, uint64_t first,
                     uint64_t n, uint32_t* order, uint64_t* offsets) {
  int rc = check_shutter(sh, n_poses, sp);
  if (rc != RTC_OK) return rc;
  if (!offsets || (!order && n)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (hsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty frame");
  const uint64_t N = (uint64_t)sp->side * sp->side;
  if (n > 0x7fffff00ull / N) return rtc_fail(RTC_ERR_UNSUPPORTED, "shutter: a dealing of 2^31 samples or more");
  if (!pixel_indices && first > ~0ull - n) return rtc_fail(RTC_ERR_INVALID, "pixel range exceeds the image");
  const uint64_t m = n * N;
  if (n == 0) { for (uint32_t p = 0; p <= n_poses; p++) offsets[p] = 0; return RTC_OK; }
  if (!s) {  // the same rule on the host: count, prefix sums, place in id order (stable)
    std::vector<uint32_t> pose(m);
    std::vector<uint64_t> next(n_poses + 1, 0);
    for (uint64_t j = 0; j < n; j++) {
      const uint64_t i = pixel_indices ? pixel_indices[j] : first + j;
      for (uint64_t k = 0; k < N; k++) next[(pose[j * N + k] = rtc_shutter_pose(*sh, *sp, n_poses, i, (uint32_t)k)) + 1]++;
    }
    for (uint32_t p = 0; p < n_poses; p++) next[p + 1] += next[p];
    for (uint32_t p = 0; p <= n_poses; p++) offsets[p] = next[p];
    for (uint64_t id = 0; id < m; id++) order[next[pose[id]]++] = (uint32_t)id;
    return RTC_OK;
  }
  HIP_OK(hipSetDevice(s->device));
  DPixelMap pm{};
  std::vector<uint64_t> range_idx;
  rc = make_pixel_map(s, hsize, ~0ull, pixel_indices, first, n, &pm, &range_idx);
  if (rc == RTC_OK) rc = ensure_shutter(s, m);
  if (rc != RTC_OK) return rc;
  DCamera dc{};
  dc.hsize = hsize; dc.vsize = 1;  // (of the camera only hsize enters a slot's pixel)
  unsigned long long offs[RTC_SHUTTER_MAX_POSES + 1];
  unsigned n_kernels = 0;
  rc = shutter_deal(s, *sh, *sp, n_poses, pm, dc, 0, m, offs, &n_kernels, false);
  if (rc != RTC_OK) return rc;
  for (uint32_t p = 0; p <= n_poses; p++) offsets[p] = offs[p];
  HIP_OK(hipMemcpy(order, s->d_shorder, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTC_OK;
}

uint32_t rtc_shutter_draw_pose(double u, uint32_t n_poses) { return n_poses ? rtc_shutter_draw_pose_of(u, n_poses) : 0u; }

// ---- the reconstruction filters' entry points (include/rtc.h) ------------------------------------------------------------------------
static int render_filtered(rtc_scene* s, const rtc_camera* cam, const rtc_sampling* sp, const rtc_filter* f, int32_t fuel, uint64_t row_first, uint64_t n_rows,
                           double* rgb, uint8_t* rgb8, rtc_stats* stats) {
  if (!s || !cam || !sp || !f || (!rgb && !rgb8)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_sampling(sp);
  if (rc == RTC_OK) rc = check_filter(f);
  if (rc != RTC_OK) return rc;
  if (cam->hsize == 0 || cam->vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  if (n_rows == 0 || row_first >= cam->vsize || n_rows > cam->vsize - row_first) return rtc_fail(RTC_ERR_INVALID, "filtered: the row range is empty or leaves the image");
  if (cam->vsize > 0xffffffffull) return rtc_fail(RTC_ERR_UNSUPPORTED, "filtered: frames of 2^32 rows or more");
  const uint64_t n = n_rows * cam->hsize;
  rc = prepare_output(s, n, false, rgb8 != nullptr);
  if (rc != RTC_OK) return rc;
  const DPixelMap pm = rows_map(n, (uint32_t)row_first);
  DCamera dc;
  to_dcam(*cam, &dc);
  return render_to_host(s, n, rgb, rgb8, nullptr, [&](const AfterLaunch* after) { return run_filtered(s, dc, pm, *sp, *f, fuel, s->d_rgb, stats, stats != nullptr, true, after); });
}


int rtc_render_filtered(rtc_scene* s, const rtc_camera* cam, const rtc_sampling* sp, const rtc_filter* f, int32_t fuel, uint32_t row_first, uint32_t n_rows, double* rgb,
                        rtc_stats* stats) {
  return render_filtered(s, cam, sp, f, fuel, row_first, n_rows, rgb, nullptr, stats);
}

int rtc_render_filtered_rgb8(rtc_scene* s, const rtc_camera* cam, const rtc_sampling* sp, const rtc_filter* f, int32_t fuel, uint8_t* rgb8, rtc_stats* stats) {
  return render_filtered(s, cam, sp, f, fuel, 0, cam ? cam->vsize : 0, nullptr, rgb8, stats);
}

int rtc_filter_frame(rtc_scene* s, uint64_t hsize, uint64_t vsize, const rtc_sampling* sp, const rtc_filter* f, const double* sample_rgb, double* rgb) {
  if (!sp || !f || !sample_rgb || !rgb) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  int rc = check_sampling(sp);
  if (rc == RTC_OK) rc = check_filter(f);
  if (rc != RTC_OK) return rc;
  if (hsize == 0 || vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty frame");
  const uint64_t N = (uint64_t)sp->side * sp->side;
  if (hsize > 0x7fffff00ull || vsize > 0x7fffff00ull || hsize * vsize > 0x7fffff00ull / N) return rtc_fail(RTC_ERR_UNSUPPORTED, "filter: frames of 2^31 samples or more");
  const uint64_t total = hsize * vsize;
  if (!s) {  // the same function on the host
    const uint32_t W = rtc_filter_window(f->radius);
    const rtc_filter_mem_src src{sample_rgb, hsize, 0, (uint32_t)N, *sp};
    for (uint64_t i = 0; i < total; i++) {
      const uint64_t x = i % hsize, y = i / hsize;
      uint64_t qx0, qx1, qy0, qy1;
      rtc_filter_span(x, W, 0, hsize, &qx0, &qx1);
      rtc_filter_span(y, W, 0, vsize, &qy0, &qy1);
      rtc_filter_pixel(*f, (uint32_t)N, x, y, qx0, qx1, qy0, qy1, src, rgb + 3 * i);
    }
    return RTC_OK;
  }
  HIP_OK(hipSetDevice(s->device));
  rc = ensure_px(s, total, false);
  if (rc == RTC_OK) rc = ensure_sampled(s, total * N, true);
  if (rc != RTC_OK) return rc;
  HIP_OK(hipMemcpyAsync(s->d_srgb, sample_rgb, total * N * 3 * sizeof(double), hipMemcpyHostToDevice, s->stream));
  (void)rtc_launch_resolve_filtered(*f, *sp, hsize, 0, vsize, 0, vsize, s->d_srgb, s->d_rgb, s->stream, nullptr);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(rgb, s->d_rgb, total * 3 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  return RTC_OK;
}

int rtc_quantize_device(rtc_scene* s, const double* rgb_dev, uint64_t n_values, uint8_t* out_dev, int sync) {
  if (!s || (n_values && (!rgb_dev || !out_dev))) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  HIP_OK(hipSetDevice(s->device));
  rtc_launch_quantize(rgb_dev, out_dev, n_values, s->stream);
  HIP_OK(hipGetLastError());
  if (sync) HIP_OK(hipStreamSynchronize(s->stream));
  return RTC_OK;
}

int rtc_quantize(rtc_scene* s, const double* rgb, uint64_t n_values, uint8_t* out) {
  if (!s || (n_values && (!rgb || !out))) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (n_values == 0) return RTC_OK;
  HIP_OK(hipSetDevice(s->device));
  double* d_in = nullptr;
  uint8_t* d_out = nullptr;
  HIP_OK(hipMalloc((void**)&d_in, n_values * sizeof(double)));
  if (hipMalloc((void**)&d_out, n_values) != hipSuccess) { (void)hipFree(d_in); return rtc_fail(RTC_ERR_DEVICE, "hipMalloc failed"); }
  int rc = RTC_OK;
  if (hipMemcpy(d_in, rgb, n_values * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = rtc_fail(RTC_ERR_DEVICE, "H2D copy failed");
  if (rc == RTC_OK) rc = rtc_quantize_device(s, d_in, n_values, d_out, 1);
  if (rc == RTC_OK && hipMemcpy(out, d_out, n_values, hipMemcpyDeviceToHost) != hipSuccess) rc = rtc_fail(RTC_ERR_DEVICE, "D2H copy failed");
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return rc;
}

uint64_t rtc_ppm(uint64_t hsize, uint64_t vsize, const uint8_t* rgb8, char* out, uint64_t cap) {
  // two passes: size, then fill (src/image.rs:93-112)
  auto digits = [](unsigned v) { return v >= 100 ? 3u : (v >= 10 ? 2u : 1u); };
  std::string head = "P3\n" + std::to_string(hsize) + " " + std::to_string(vsize) + "\n255";
  uint64_t size = head.size() + 1;  // + trailing newline
  const uint64_t n = hsize * vsize;
  for (uint64_t i = 0; i < n; i++) size += 1 + digits(rgb8[3 * i]) + 1 + digits(rgb8[3 * i + 1]) + 1 + digits(rgb8[3 * i + 2]);
  if (!out || cap < size + 1) return size;
  char* p = out;
  std::memcpy(p, head.data(), head.size());
  p += head.size();
  auto put = [&](unsigned v) {
    if (v >= 100) *p++ = (char)('0' + v / 100);
    if (v >= 10) *p++ = (char)('0' + (v / 10) % 10);
    *p++ = (char)('0' + v % 10);
  };
  uint64_t j = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (i % hsize == 0 || j % 5 == 0) { *p++ = '\n'; j = 1; } else { *p++ = ' '; j += 1; }
    put(rgb8[3 * i]); *p++ = ' '; put(rgb8[3 * i + 1]); *p++ = ' '; put(rgb8[3 * i + 2]);
  }
  *p++ = '\n';
  *p = 0;
  return (uint64_t)(p - out);
}

// Error state of every launch since the last check (or the last synchronous render, which reports and clears it too):
// asynchronous launches (sync == 0, stats == NULL) do not read it back themselves.
int rtc_scene_check(rtc_scene* s) {
  if (!s) return rtc_fail(RTC_ERR_INVALID, "NULL scene");
  HIP_OK(hipSetDevice(s->device));
  HIP_OK(hipStreamSynchronize(s->stream));
  DStats h;
  int rc = read_clear_sticky(s, &h);
  if (rc != RTC_OK) return rc;
  if (h.guard) return rtc_fail(RTC_ERR_DEVICE, "traversal guard tripped (mask " + std::to_string(h.guard) + ")");
  if (h.nan_ts) return rtc_fail(RTC_ERR_NAN, "a NaN intersection t reached a sort of two or more intersections (the reference panics in Intersection::sort, src/intersection.rs:124)");
  if (h.wf_overflow) return rtc_fail(RTC_ERR_UNSUPPORTED, "a wavefront ray queue overflowed in an unsynchronised launch: render this launch synchronously (falls back by itself)");
  return RTC_OK;
}

// Stream markers.  Every event is created with the scene and lives as long as it; a marker that was never recorded is an
// error, not an undefined wait (hipEventSynchronize / hipEventElapsedTime on a never-recorded event).
static int marker_slot(rtc_scene* s, int slot, bool need_recorded) {
  if (!s) return rtc_fail(RTC_ERR_INVALID, "NULL scene");
  if (slot < 0 || slot >= 8) return rtc_fail(RTC_ERR_INVALID, "marker slot out of range (0..7)");
  if (need_recorded && !s->marker_recorded[slot]) return rtc_fail(RTC_ERR_INVALID, "marker slot " + std::to_string(slot) + " was never recorded");
  return RTC_OK;
}
int rtc_scene_record(rtc_scene* s, int slot) {
  int rc = marker_slot(s, slot, false);
  if (rc != RTC_OK) return rc;
  HIP_OK(hipSetDevice(s->device));
  HIP_OK(hipEventRecord(s->marker[slot], s->stream));
  s->marker_recorded[slot] = true;
  return RTC_OK;
}
int rtc_scene_wait(rtc_scene* s, int slot) {
  int rc = marker_slot(s, slot, true);
  if (rc != RTC_OK) return rc;
  HIP_OK(hipSetDevice(s->device));
  HIP_OK(hipEventSynchronize(s->marker[slot]));
  return RTC_OK;
}
int rtc_scene_elapsed_ms(rtc_scene* s, int from, int to, double* ms) {
  int rc = marker_slot(s, from, true);
  if (rc == RTC_OK) rc = marker_slot(s, to, true);
  if (rc != RTC_OK) return rc;
  if (!ms) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  HIP_OK(hipSetDevice(s->device));
  HIP_OK(hipEventSynchronize(s->marker[to]));  // both must have completed for hipEventElapsedTime
  float f = 0.f;
  HIP_OK(hipEventElapsedTime(&f, s->marker[from], s->marker[to]));
  *ms = f;
  return RTC_OK;
}

int rtc_scene_sync(rtc_scene* s) {
  if (!s) return rtc_fail(RTC_ERR_INVALID, "NULL scene");
  HIP_OK(hipSetDevice(s->device));
  HIP_OK(hipStreamSynchronize(s->stream));
  return RTC_OK;
}

// ---- N GPUs of one process (include/rtc.h) ---------------------------------------------------------------------
struct rtc_multi {
  std::vector<rtc_scene*> scenes;   // one replica per listed device
  std::vector<double*> tiles;       // replica k's dense rows k, k + n, ... on ITS device
  std::vector<uint64_t> tile_cap;
  std::vector<hipEvent_t> done;     // replica k's tile is complete (recorded on its stream)
  std::vector<hipEvent_t> copied;   // the first device has pulled replica k's tile (recorded on the first replica's stream): the
  std::vector<char> copied_valid;   //   replica's next frame waits for it before it overwrites the tile
  double* slab = nullptr;           // first device: n x max_rows x hsize x 3
  double* image = nullptr;          // first device: vsize x hsize x 3
  uint64_t slab_cap = 0, image_cap = 0;
  // rtc_render_multi_rgb8: the same buffers for quantised pixels (a replica quantises its tile on its own device)
  std::vector<uint8_t*> tiles8;
  std::vector<uint64_t> tile8_cap;
  uint8_t* slab8 = nullptr;
  uint8_t* image8 = nullptr;
  uint64_t slab8_cap = 0, image8_cap = 0;
  uint32_t band = 8;                // rows per band of the partition (rtc_multi_set_band_rows)
};

namespace {

// `sp`: every replica renders its tile through run_sampled (with stats: synchronously, one replica after the other -- a sampled
// launch's counters are summed over its chunks by the host).
int render_multi(rtc_multi* m, const rtc_camera* cam, int32_t fuel, double* rgb_dev_out, double* rgb_host, rtc_stats* stats, bool sync, uint8_t* rgb8_host = nullptr,
                 const rtc_sampling* sp = nullptr) {
  const bool q8 = rgb8_host != nullptr;
  if (!m || !cam) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (cam->hsize == 0 || cam->vsize == 0) return rtc_fail(RTC_ERR_INVALID, "empty camera");
  const uint32_t n = (uint32_t)m->scenes.size();
  const uint64_t H = cam->hsize, V = cam->vsize, rowlen = H * 3;
  if (rowlen > 0xffffffffull || V > 0xffffffffull) return rtc_fail(RTC_ERR_INVALID, "image too large");
  const uint32_t B = m->band;
  const uint64_t max_rows = (((V + B - 1) / B + n - 1) / n) * B;
  rtc_scene* s0 = m->scenes[0];
  DCamera dc;
  to_dcam(*cam, &dc);
  // buffers: a tile per replica on its own device; slab and image on the first device
  for (uint32_t k = 0; k < n; k++) {
    rtc_scene* s = m->scenes[k];
    if (max_rows * rowlen > m->tile_cap[k]) {
      HIP_OK(hipSetDevice(s->device));
      HIP_OK(hipStreamSynchronize(s->stream));
      (void)hipFree(m->tiles[k]);
      m->tiles[k] = nullptr; m->tile_cap[k] = 0;
      HIP_OK(hipMalloc((void**)&m->tiles[k], max_rows * rowlen * sizeof(double)));
      m->tile_cap[k] = max_rows * rowlen;
    }
    if (q8 && max_rows * rowlen > m->tile8_cap[k]) {
      HIP_OK(hipSetDevice(s->device));
      HIP_OK(hipStreamSynchronize(s->stream));
      (void)hipFree(m->tiles8[k]);
      m->tiles8[k] = nullptr; m->tile8_cap[k] = 0;
      HIP_OK(hipMalloc((void**)&m->tiles8[k], max_rows * rowlen));
      m->tile8_cap[k] = max_rows * rowlen;
    }
  }
  HIP_OK(hipSetDevice(s0->device));
  if (q8) {
    if ((uint64_t)n * max_rows * rowlen > m->slab8_cap) {
      HIP_OK(hipStreamSynchronize(s0->stream));
      (void)hipFree(m->slab8);
      m->slab8 = nullptr; m->slab8_cap = 0;
      HIP_OK(hipMalloc((void**)&m->slab8, (uint64_t)n * max_rows * rowlen));
      m->slab8_cap = (uint64_t)n * max_rows * rowlen;
    }
    if (V * rowlen > m->image8_cap) {
      HIP_OK(hipStreamSynchronize(s0->stream));
      (void)hipFree(m->image8);
      m->image8 = nullptr; m->image8_cap = 0;
      HIP_OK(hipMalloc((void**)&m->image8, V * rowlen));
      m->image8_cap = V * rowlen;
    }
  }
  if (!q8 && (uint64_t)n * max_rows * rowlen > m->slab_cap) {
    HIP_OK(hipStreamSynchronize(s0->stream));
    (void)hipFree(m->slab);
    m->slab = nullptr; m->slab_cap = 0;
    HIP_OK(hipMalloc((void**)&m->slab, (uint64_t)n * max_rows * rowlen * sizeof(double)));
    m->slab_cap = (uint64_t)n * max_rows * rowlen;
  }
  if (!q8 && !rgb_dev_out && V * rowlen > m->image_cap) {
    HIP_OK(hipStreamSynchronize(s0->stream));
    (void)hipFree(m->image);
    m->image = nullptr; m->image_cap = 0;
    HIP_OK(hipMalloc((void**)&m->image, V * rowlen * sizeof(double)));
    m->image_cap = V * rowlen;
  }
  double* image = rgb_dev_out ? rgb_dev_out : m->image;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  std::vector<rtc_stats> sampled_stats(sp && stats ? n : 0);
  // every replica traces its interleaved rows on its own device and stream; nothing is exchanged while tracing
  for (uint32_t k = 0; k < n; k++) {
    rtc_scene* s = m->scenes[k];
    DPixelMap pm{};
    const uint64_t rows = band_rows_owned(V, B, k, n);
    pm.n = rows * H; pm.mode = 2; pm.row_first = k; pm.row_step = n; pm.band = B;
    if (pm.n == 0) continue;
    if (m->copied_valid[k]) {  // frames queued back to back: the previous frame's gather still reads this tile
      HIP_OK(hipSetDevice(s->device));
      HIP_OK(hipStreamWaitEvent(s->stream, m->copied[k], 0));
    }
    // asynchronous on the replica's own stream (the counting variant when stats are wanted: they are read back after the gather)
    int rc = sp ? run_sampled(s, dc, pm, *sp, fuel, m->tiles[k], stats ? &sampled_stats[k] : nullptr, stats != nullptr, false)
                : run(s, dc, pm, fuel, m->tiles[k], false, nullptr, stats != nullptr, false);
    if (rc != RTC_OK) return rc;
    HIP_OK(hipSetDevice(s->device));
    if (q8) {  // Color::clamp on the replica's own device, behind its trace kernels
      rtc_launch_quantize(m->tiles[k], m->tiles8[k], rows * rowlen, s->stream);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(m->done[k], s->stream));
  }
  // gather: the first device's stream waits for each tile and pulls it over xGMI into its slot of the slab, then one
  // de-interleave pass writes the image (row k + n j  <-  slab[k][j])
  HIP_OK(hipSetDevice(s0->device));
  for (uint32_t k = 0; k < n; k++) {
    const uint64_t rows = band_rows_owned(V, B, k, n);
    if (rows == 0) continue;
    rtc_scene* s = m->scenes[k];
    HIP_OK(hipStreamWaitEvent(s0->stream, m->done[k], 0));
    void* dst = q8 ? (void*)(m->slab8 + (uint64_t)k * max_rows * rowlen) : (void*)(m->slab + (uint64_t)k * max_rows * rowlen);
    const void* src = q8 ? (const void*)m->tiles8[k] : (const void*)m->tiles[k];
    const uint64_t bytes = rows * rowlen * (q8 ? 1 : sizeof(double));
    if (s->device == s0->device) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s0->stream));
    else HIP_OK(hipMemcpyPeerAsync(dst, s0->device, src, s->device, bytes, s0->stream));
    HIP_OK(hipEventRecord(m->copied[k], s0->stream));
    m->copied_valid[k] = 1;
  }
  if (q8) rtc_launch_deinterleave8(m->slab8, m->image8, (unsigned)rowlen, (unsigned)V, n, (unsigned)max_rows, B, s0->stream);
  else rtc_launch_deinterleave(m->slab, image, (unsigned)rowlen, (unsigned)V, n, (unsigned)max_rows, B, s0->stream);
  HIP_OK(hipGetLastError());
  {  // the caller's pages, while the devices render (see pretouch_pages)
    std::vector<std::thread> pool;
    if (q8) pretouch_pages(rgb8_host, V * rowlen, &pool);
    if (rgb_host) pretouch_pages(rgb_host, V * rowlen * sizeof(double), &pool);
    join_all(&pool);
  }
  if (q8) HIP_OK(hipMemcpyAsync(rgb8_host, m->image8, V * rowlen, hipMemcpyDeviceToHost, s0->stream));
  if (rgb_host) HIP_OK(hipMemcpyAsync(rgb_host, image, V * rowlen * sizeof(double), hipMemcpyDeviceToHost, s0->stream));
  if (!sync && !rgb_host && !q8 && !stats) return RTC_OK;
  HIP_OK(hipStreamSynchronize(s0->stream));
  for (uint32_t k = 0; k < n; k++) {
    rtc_scene* s = m->scenes[k];
    const uint64_t rows = band_rows_owned(V, B, k, n);
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipStreamSynchronize(s->stream));
    DStats h;
    int rc = read_clear_sticky(s, &h);   // counters of the replica's launch + error state of every launch since the last check
    if (rc != RTC_OK) return rc;
    if (h.guard) return rtc_fail(RTC_ERR_DEVICE, "traversal guard tripped (mask " + std::to_string(h.guard) + ")");
    if (h.nan_ts) return rtc_fail(RTC_ERR_NAN, "a NaN intersection t reached a sort of two or more intersections (the reference panics in Intersection::sort, src/intersection.rs:124)");
    if (h.wf_overflow) {  // an unsynchronised wavefront launch overflowed its queues: once more, synchronously (falls back by itself)
      DPixelMap pm{};
      pm.n = rows * H; pm.mode = 2; pm.row_first = k; pm.row_step = n; pm.band = B;
      rc = sp ? run_sampled(s, dc, pm, *sp, fuel, m->tiles[k], nullptr, false, true) : run(s, dc, pm, fuel, m->tiles[k], false, nullptr, false, true);
      if (rc != RTC_OK) return rc;
      return render_multi(m, cam, fuel, rgb_dev_out, rgb_host, stats, true, rgb8_host, sp);
    }
    if (stats && rows) {
      rtc_stats st;
      if (sp) st = sampled_stats[k];
      else rc = fill_stats(s, h, rows * H, &st);
      if (rc != RTC_OK) return rc;
      stats->pixels += st.pixels; stats->rays_primary += st.rays_primary; stats->rays_shadow += st.rays_shadow; stats->rays_reflect += st.rays_reflect;
      stats->rays_refract += st.rays_refract; stats->rays_container += st.rays_container; stats->accel_nodes += st.accel_nodes; stats->group_tests += st.group_tests;
      stats->tri_tests += st.tri_tests; stats->analytic_tests += st.analytic_tests; stats->nan_ts += st.nan_ts; stats->n_launches += st.n_launches;
      stats->accel_nodes_kernarg += st.accel_nodes_kernarg; stats->analytic_tests_kernarg += st.analytic_tests_kernarg;
      stats->light_grid_cells += st.light_grid_cells; stats->group_tests_uniform += st.group_tests_uniform;
      stats->kernel_ms = std::max(stats->kernel_ms, st.kernel_ms);  // replicas run side by side: the slowest one
    }
  }
  return RTC_OK;
}

// One replica of the scene per listed device, each created from the same normalised inputs.
int multi_create(const SceneInputs& in, const int* devices, int n_devices, rtc_multi** out) {
  if (!devices || !out || n_devices <= 0) return rtc_fail(RTC_ERR_INVALID, "NULL argument / no devices");
  *out = nullptr;
  std::unique_ptr<rtc_multi> m(new rtc_multi());
  for (int k = 0; k < n_devices; k++) {
    rtc_scene* s = nullptr;
    int rc = scene_create(in, devices[k], &s);
    if (rc != RTC_OK) { rtc_multi_destroy(m.release()); return rc; }
    m->scenes.push_back(s);
    m->tiles.push_back(nullptr);
    m->tile_cap.push_back(0);
    m->tiles8.push_back(nullptr);
    m->tile8_cap.push_back(0);
    hipEvent_t e = nullptr;
    if (hipSetDevice(devices[k]) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      rtc_multi_destroy(m.release());
      return rtc_fail(RTC_ERR_DEVICE, "hipEventCreate failed");
    }
    m->done.push_back(e);
    hipEvent_t c = nullptr;
    if (hipSetDevice(devices[0]) != hipSuccess || hipEventCreateWithFlags(&c, hipEventDisableTiming) != hipSuccess) {
      rtc_multi_destroy(m.release());
      return rtc_fail(RTC_ERR_DEVICE, "hipEventCreate failed");
    }
    m->copied.push_back(c);
    m->copied_valid.push_back(0);
  }
  // direct xGMI copies into the first device where the platform allows them (hipMemcpyPeerAsync stages through the host otherwise)
  (void)hipSetDevice(devices[0]);
  for (int k = 1; k < n_devices; k++) {
    int can = 0;
    if (devices[k] != devices[0] && hipDeviceCanAccessPeer(&can, devices[0], devices[k]) == hipSuccess && can) {
      if (hipDeviceEnablePeerAccess(devices[k], 0) != hipSuccess) (void)hipGetLastError();  // already enabled: fine
    }
  }
  *out = m.release();
  return RTC_OK;
}
}  // namespace

// (as the six rtc_scene_create* above)
int rtc_multi_create(const rtc_scene_desc* desc, const int* devices, int n_devices, rtc_multi** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, nullptr, false, nullptr, 0, nullptr, nullptr, 0, out, &in)) return rc;
  return multi_create(in, devices, n_devices, out);
}
int rtc_multi_create_ex(const rtc_scene_desc* desc, const rtc_light_ex* lights, uint32_t n_lights, const int* devices, int n_devices, rtc_multi** out) {
  SceneInputs in;
  if (const int rc = scene_inputs_ex(desc, lights, n_lights, out, &in)) return rc;
  return multi_create(in, devices, n_devices, out);
}
int rtc_multi_create_ext(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const int* devices, int n_devices, rtc_multi** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, ext, false, nullptr, 0, nullptr, nullptr, 0, out, &in)) return rc;
  return multi_create(in, devices, n_devices, out);
}
int rtc_multi_create_ext2(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const int* devices, int n_devices,
                          rtc_multi** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, ext, false, cones, n_cones, nullptr, nullptr, 0, out, &in)) return rc;
  return multi_create(in, devices, n_devices, out);
}
int rtc_multi_create_ext3(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg, const int* devices,
                          int n_devices, rtc_multi** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, ext, false, cones, n_cones, bg, nullptr, 0, out, &in)) return rc;
  return multi_create(in, devices, n_devices, out);
}
int rtc_multi_create_ext4(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg,
                          const rtc_bump* bumps, uint32_t n_bumps, const int* devices, int n_devices, rtc_multi** out) {
  SceneInputs in;
  if (const int rc = scene_inputs(desc, ext, false, cones, n_cones, bg, bumps, n_bumps, out, &in)) return rc;
  return multi_create(in, devices, n_devices, out);
}

void rtc_multi_destroy(rtc_multi* m) {
  if (!m) return;
  for (size_t k = 0; k < m->scenes.size(); k++) {
    rtc_scene* s = m->scenes[k];
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (k < m->tiles.size()) (void)hipFree(m->tiles[k]);
    if (k < m->tiles8.size()) (void)hipFree(m->tiles8[k]);
    if (k < m->done.size() && m->done[k]) (void)hipEventDestroy(m->done[k]);
  }
  for (hipEvent_t c : m->copied) if (c) (void)hipEventDestroy(c);
  if (!m->scenes.empty()) {
    (void)hipSetDevice(m->scenes[0]->device);
    (void)hipFree(m->slab);
    (void)hipFree(m->image);
    (void)hipFree(m->slab8);
    (void)hipFree(m->image8);
  }
  for (rtc_scene* s : m->scenes) rtc_scene_destroy(s);
  delete m;
}

int rtc_multi_device_count(const rtc_multi* m) { return m ? (int)m->scenes.size() : 0; }

int rtc_multi_set_band_rows(rtc_multi* m, uint32_t band_rows) {
  if (!m || band_rows == 0) return rtc_fail(RTC_ERR_INVALID, "NULL argument / band_rows must be >= 1");
  for (rtc_scene* s : m->scenes) {  // queued frames still use the old layout of tiles and slab
    HIP_OK(hipSetDevice(s->device));
    HIP_OK(hipStreamSynchronize(s->stream));
  }
  m->band = band_rows;
  return RTC_OK;
}

int rtc_render_multi(rtc_multi* m, const rtc_camera* cam, int32_t fuel, double* rgb, rtc_stats* stats) {
  if (!rgb) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  return render_multi(m, cam, fuel, nullptr, rgb, stats, true);
}

int rtc_render_multi_sampled(rtc_multi* m, const rtc_camera* cam, const rtc_sampling* sp, int32_t fuel, double* rgb, rtc_stats* stats) {
  if (!rgb || !sp) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  const int rc = check_sampling(sp);
  if (rc != RTC_OK) return rc;
  return render_multi(m, cam, fuel, nullptr, rgb, stats, true, nullptr, sp);
}

int rtc_render_multi_rgb8(rtc_multi* m, const rtc_camera* cam, int32_t fuel, uint8_t* rgb8, rtc_stats* stats) {
  if (!rgb8) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  return render_multi(m, cam, fuel, nullptr, nullptr, stats, true, rgb8);
}

int rtc_render_multi_device(rtc_multi* m, const rtc_camera* cam, int32_t fuel, double* rgb_dev, int sync) {
  if (!rgb_dev) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  return render_multi(m, cam, fuel, rgb_dev, nullptr, nullptr, sync != 0);
}

int rtc_multi_sync(rtc_multi* m) {
  if (!m) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  for (rtc_scene* s : m->scenes) {
    int rc = rtc_scene_check(s);
    if (rc != RTC_OK) return rc;
  }
  return RTC_OK;
}

// Accelerator facts for reports (not part of the reference-facing surface).
void rtc_scene_path_info(const rtc_scene* s, int32_t* choice, double* one_kernel_ms, double* wavefront_ms) {
  if (choice) *choice = s ? (s->kernel_version ? s->kernel_version : s->tune_choice) : 0;
  if (one_kernel_ms) *one_kernel_ms = s ? s->tune_ms[0] : -1.0;
  if (wavefront_ms) *wavefront_ms = s ? s->tune_ms[1] : -1.0;
}

int rtc_scene_bvh_built_on_device(const rtc_scene* s) { return s ? s->built_on_device : 0; }

// Test hooks: a builder's raw tree, no scene (include/rtc.h).
int rtc_bvh_build_raw(const double* boxes, uint32_t n, int32_t leaf_max, uint32_t base, int32_t where, void* nodes, uint32_t nodes_cap, uint32_t* n_nodes, uint32_t* order,
                      uint32_t order_cap, uint64_t* keys, uint32_t keys_cap, int32_t* root, double* frame, int32_t* depth, int32_t* stack_need) {
  std::string err;
  const int rc = rtb::bvh_build_raw(boxes, n, leaf_max, base, where, rtc_bvh_build_device_keys, nodes, nodes_cap, n_nodes, order, order_cap, keys, keys_cap, root, frame, depth,
                                    stack_need, &err);
  return rc > 0 ? rtc_fail(rc, err) : rc;
}
int rtc_bvh_collapse_raw(const void* nodes, uint32_t n_nodes, int32_t root, int32_t* depth, int32_t* stack_need) {
  std::string err;
  const int rc = rtb::bvh_collapse_raw(nodes, n_nodes, root, depth, stack_need, &err);
  return rc > 0 ? rtc_fail(rc, err) : rc;
}
int rtc_light_grid_build_raw(const int32_t* geometry, const double* limits, const double* transform_inv, const double* tris, uint32_t n_prims, const double* light, int32_t n,
                             int32_t max_list, int32_t tight, uint32_t* cells, uint32_t cells_cap, int32_t* items, uint32_t items_cap, uint32_t* n_items) {
  std::string err;
  const int rc = rtb::light_grid_build_raw(geometry, limits, transform_inv, tris, n_prims, light, n, max_list, tight, cells, cells_cap, items, items_cap, n_items, &err);
  return rc > 0 ? rtc_fail(rc, err) : rc;
}

// Test hook: the shared scan (rtc_adaptive.hip rtc_launch_scan) alone on the caller's words, in buffers of its own (include/rtc.h).
int rtc_scan_raw(rtc_scene* s, uint64_t* values, uint64_t n, uint64_t* total) {
  if (!total || (!values && n)) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  *total = 0;
  if (n == 0) return RTC_OK;
  if (!s) {  // the same sums on the host
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) { const uint64_t v = values[i]; values[i] = sum; sum += v; }
    *total = sum;
    return RTC_OK;
  }
  if (n >= (1ull << 39)) return rtc_fail(RTC_ERR_UNSUPPORTED, "scan: 2^39 words or more");
  HIP_OK(hipSetDevice(s->device));
  const uint64_t words = n + rtc_scan_work_words(n) + 1;  // the values, the levels above them, the total
  unsigned long long* d = nullptr;
  HIP_OK(hipMalloc((void**)&d, words * sizeof(unsigned long long)));
  hipError_t e = hipMemcpyAsync(d, values, n * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) {
    (void)rtc_launch_scan(d, n, d + n, d + words - 1, s->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(values, d, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream);
  unsigned long long sum = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&sum, d + words - 1, sizeof(sum), hipMemcpyDeviceToHost, s->stream);
  const hipError_t e_sync = hipStreamSynchronize(s->stream);  // (before the buffer goes, whatever happened)
  (void)hipFree(d);
  HIP_OK(e);
  HIP_OK(e_sync);
  *total = sum;
  return RTC_OK;
}

// Test hook: one culling predicate of rtc_device.hpp on the caller's records (rtc_probe.hip), in buffers of its own (include/rtc.h).
int rtc_cull_probe_raw(rtc_scene* s, int32_t kind, const double* records, uint64_t n, uint8_t* answers) {
  const int stride = rtc_cull_probe_doubles(kind);
  if (stride == 0) return rtc_fail(RTC_ERR_INVALID, "cull probe: no such predicate");
  if (n == 0) return RTC_OK;
  if (!records || !answers || !s) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (n >= (1ull << 32)) return rtc_fail(RTC_ERR_UNSUPPORTED, "cull probe: 2^32 records or more");
  HIP_OK(hipSetDevice(s->device));
  const uint64_t rec_bytes = n * (uint64_t)stride * sizeof(double);
  unsigned char* d = nullptr;  // the records, then the answers
  HIP_OK(hipMalloc((void**)&d, rec_bytes + n));
  hipError_t e = hipMemcpyAsync(d, records, rec_bytes, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) {
    rtc_launch_cull_probe(kind, (const double*)d, n, d + rec_bytes, s->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(answers, d + rec_bytes, n, hipMemcpyDeviceToHost, s->stream);
  const hipError_t e_sync = hipStreamSynchronize(s->stream);  // (before the buffer goes, whatever happened)
  (void)hipFree(d);
  HIP_OK(e);
  HIP_OK(e_sync);
  return RTC_OK;
}

uint32_t rtc_scene_wavefront_lds_bytes(const rtc_scene* s) { return s ? s->lds_bytes : 0u; }

int rtc_scene_wavefront_ts_grid(const rtc_scene* s, int32_t sync, uint32_t* grid, uint32_t* n_cu, uint32_t* spare_cus, uint32_t* live) {
  if (!s) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (grid) *grid = s->lds_bytes ? lds_grid(s, sync != 0) : s->wave_blocks;  // (what run() hands rtc_launch_wavefront)
  if (n_cu) *n_cu = (uint32_t)s->n_cu;
  if (spare_cus) *spare_cus = (uint32_t)s->spare_cus;
  if (live) *live = (uint32_t)live_scenes(s->device);
  return RTC_OK;
}

int rtc_scene_kernel_info(const rtc_scene* s, int32_t path, int32_t count, rtc_kernel_info* out) {
  if (!s || !out) return rtc_fail(RTC_ERR_INVALID, "NULL argument");
  if (path != 1 && path != 4) return rtc_fail(RTC_ERR_INVALID, "path must be 1 (one kernel) or 4 (wavefront)");
  rtc_kernel_info_fill(s->d, path == 4, count != 0, rtc_scene_is_big(s->bytes), s->lds_bytes, s->device, out);
  return RTC_OK;
}

void rtc_scene_accel_info(const rtc_scene* s, uint32_t* n_ops, uint32_t* n_bvh_nodes, uint32_t* n_mesh_tris, uint32_t* bvh_depth) {
  if (n_ops) *n_ops = s ? (uint32_t)s->d.n_ops : 0;
  if (n_bvh_nodes) *n_bvh_nodes = s ? s->n_bvh_nodes : 0;
  if (n_mesh_tris) *n_mesh_tris = s ? s->n_mesh_tris : 0;
  if (bvh_depth) *bvh_depth = s ? (uint32_t)s->bvh_depth : 0;
}

}  // extern "C"

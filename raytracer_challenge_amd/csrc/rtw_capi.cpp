// rtw_capi.cpp — include/rtw.h for the product: C handles over the host mirror (host_scene.hpp).  A world is
// flattened once (first render after the last edit), uploaded through rtc_scene_create, and every render goes
// to the HIP kernels through the rtc.h entry points.  Nothing here can compute a pixel on the CPU.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>

#include "../../include/rtc.h"
#include "../../include/rtw.h"
#include "host_scene.hpp"

using namespace rth;

// Weak: the CPU emulator of the kernels (tests/cpu_emu) links this file without the _ex entry point; a world with an area light then
// fails to render with a message instead of the whole library failing to load.
extern "C" int rtc_scene_create_ex(const rtc_scene_desc*, const rtc_light_ex*, uint32_t, int, rtc_scene**) __attribute__((weak));
// (the same for texture-mapped patterns)
extern "C" int rtc_scene_create_ext(const rtc_scene_desc*, const rtc_scene_ext*, int, rtc_scene**) __attribute__((weak));
// (and for light cones)
extern "C" int rtc_scene_create_ext2(const rtc_scene_desc*, const rtc_scene_ext*, const rtc_light_cone*, uint32_t, int, rtc_scene**) __attribute__((weak));

// (and for a background)
extern "C" int rtc_scene_create_ext3(const rtc_scene_desc*, const rtc_scene_ext*, const rtc_light_cone*, uint32_t, const rtc_background*, int, rtc_scene**) __attribute__((weak));

// (and for bump records)
extern "C" int rtc_scene_create_ext4(const rtc_scene_desc*, const rtc_scene_ext*, const rtc_light_cone*, uint32_t, const rtc_background*, const rtc_bump*, uint32_t, int,
                                     rtc_scene**) __attribute__((weak));

struct rtw_pattern { PatRef p; };
struct rtw_texture { TexRef t; };
struct rtw_element { std::unique_ptr<Elem> e; };
struct rtw_world {
  WorldH w;
  rtc_scene* scene = nullptr;  // cached flatten+upload; dropped on edit
  int device = 0;
  std::unique_ptr<Flat> flat;  // rtw_world_flatten_desc: the arrays behind the descriptor it handed out
  std::vector<rtc_light_ex> lights_ex;  // every light in order (point and area) once an area light was added; empty otherwise
  std::vector<rtc_light_cone> cones;    // rtw_world_set_light_cone: at most one per light, `light` = the light's place in the order
  PatRef background;                    // rtw_world_set_background: the pattern a ray that hits nothing sees (null: none)
  int32_t background_projection = RTC_BG_DIRECTION;
  size_t n_lights() const { return lights_ex.empty() ? w.lights.size() : lights_ex.size(); }
  ~rtw_world() { if (scene) rtc_scene_destroy(scene); }
};

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return 1; }

static Mat to_mat(const rtw_material* m) {
  Mat r;
  if (!m) return r;
  r.ambient = m->ambient; r.diffuse = m->diffuse; r.specular = m->specular; r.shininess = m->shininess;
  r.reflective = m->reflective; r.transparency = m->transparency; r.refractive_index = m->refractive_index;
  if (m->pattern) r.pattern = m->pattern->p;
  return r;
}

static int ensure_scene(rtw_world* w) {
  if (w->scene) return 0;
  const bool timing = std::getenv("RTC_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
  int rc;
  {
    Flat f;
    Flattener fl(f);
    if (!fl.run(w->w)) return fail("flatten: " + f.error);
    rtc_scene_desc d = f.desc();
    if (timing) std::fprintf(stderr, "[rtc-timing] %-28s %.3f s\n", "flatten (host mirror -> desc)", since(t0));
    const auto t1 = std::chrono::steady_clock::now();
    // The lowest entry point that takes everything the world has (the emulator library exports rtc_scene_create alone): bump records
    // need _ext4, a background _ext3, light cones _ext2, texture-mapped patterns _ext, an area light's list _ex; whatever else the
    // world has goes along.
    const int level = !f.bumps.empty() ? 4 : w->background ? 3 : !w->cones.empty() ? 2 : !f.uv_pats.empty() ? 1 : 0;
    const bool light_list = !w->lights_ex.empty();
    if (level == 4 && !rtc_scene_create_ext4) return fail("a bump (rtw_element_set_bump) needs rtc_scene_create_ext4 (librtc_amd.so)");
    if (level == 3 && !rtc_scene_create_ext3) return fail("a background needs rtc_scene_create_ext3 (librtc_amd.so)");
    if (level == 2 && !rtc_scene_create_ext2) return fail("light cones need rtc_scene_create_ext2 (librtc_amd.so)");
    if (level == 1 && !rtc_scene_create_ext) return fail("texture-mapped patterns need rtc_scene_create_ext (librtc_amd.so)");
    if (level == 0 && light_list && !rtc_scene_create_ex) return fail("area lights need rtc_scene_create_ex (librtc_amd.so)");
    rtc_background bg{0, w->background_projection};
    if (w->background) { bg.pattern = fl.root_pattern(w->background); d = f.desc(); }  // (its pattern tree joins the node array, which grew)
    rtc_scene_ext x{};
    if (light_list) {  // the light list replaces the descriptor's point lights
      d.n_lights = 0; d.lights = nullptr;
      x.n_lights = (uint32_t)w->lights_ex.size(); x.lights = w->lights_ex.data();
    }
    x.n_uv_patterns = (uint32_t)f.uv_pats.size(); x.uv_patterns = f.uv_pats.data();
    x.n_textures = (uint32_t)f.textures.size(); x.textures = f.textures.data();
    const rtc_light_cone* cones = w->cones.empty() ? nullptr : w->cones.data();
    const uint32_t n_cones = (uint32_t)w->cones.size();
    if (level == 4) rc = rtc_scene_create_ext4(&d, &x, cones, n_cones, w->background ? &bg : nullptr, f.bumps.data(), (uint32_t)f.bumps.size(), w->device, &w->scene);
    else if (level == 3) rc = rtc_scene_create_ext3(&d, &x, cones, n_cones, &bg, w->device, &w->scene);
    else if (level == 2) rc = rtc_scene_create_ext2(&d, &x, cones, n_cones, w->device, &w->scene);
    else if (level == 1) rc = rtc_scene_create_ext(&d, &x, w->device, &w->scene);
    else if (light_list) rc = rtc_scene_create_ex(&d, x.lights, x.n_lights, w->device, &w->scene);
    else rc = rtc_scene_create(&d, w->device, &w->scene);
    if (timing) std::fprintf(stderr, "[rtc-timing] %-28s %.3f s\n", "rtc_scene_create (all of it)", since(t1));
  }
  if (timing) std::fprintf(stderr, "[rtc-timing] %-28s %.3f s\n", "flatten + create + frees", since(t0));
  if (rc != RTC_OK) return fail(std::string("rtc_scene_create: ") + rtc_last_error());
  return 0;
}

extern "C" {

const char* rtw_last_error(void) { return g_err.c_str(); }
#ifndef RTW_BACKEND_NAME
#define RTW_BACKEND_NAME "hip"
#endif
const char* rtw_backend(void) { return RTW_BACKEND_NAME; }

rtw_pattern* rtw_pattern_debug(void) {
  auto p = std::make_shared<Pat>();
  p->tag = RTC_PAT_DEBUG;
  return new rtw_pattern{p};
}
rtw_pattern* rtw_pattern_plain(double r, double g, double b) {
  auto p = std::make_shared<Pat>();
  p->tag = RTC_PAT_PLAIN;
  p->color[0] = r; p->color[1] = g; p->color[2] = b;
  return new rtw_pattern{p};
}
rtw_pattern* rtw_pattern_jitter(int jk, int nk, double scale, uint64_t octaves, const rtw_pattern* child) {
  if (!child) { fail("jitter: child is NULL"); return nullptr; }
  auto p = std::make_shared<Pat>();
  p->tag = RTC_PAT_JITTER; p->kind = jk; p->noise_kind = nk; p->scale = scale; p->octaves = (uint32_t)octaves; p->left = child->p;
  if (p->frame_depth() > RTC_MAX_PATTERN_DEPTH) { fail("pattern keeps more than RTC_MAX_PATTERN_DEPTH colour frames on one path (blends / gradients / colour jitters nested deeper than 8)"); return nullptr; }
  return new rtw_pattern{p};
}
rtw_pattern* rtw_pattern_mixture(int mk, const double t[16], const rtw_pattern* l, const rtw_pattern* r) {
  if (!l || !r) { fail("mixture: child is NULL"); return nullptr; }
  auto p = std::make_shared<Pat>();
  p->tag = RTC_PAT_MIXTURE; p->kind = mk; p->left = l->p; p->right = r->p;
  if (!M4::from(t).invert(&p->transform_inv)) { fail("mixture: singular transform (src/linalg/matrix.rs:181)"); return nullptr; }
  if (p->frame_depth() > RTC_MAX_PATTERN_DEPTH) { fail("pattern keeps more than RTC_MAX_PATTERN_DEPTH colour frames on one path (blends / gradients / colour jitters nested deeper than 8)"); return nullptr; }
  return new rtw_pattern{p};
}
void rtw_pattern_release(rtw_pattern* p) { delete p; }

rtw_texture* rtw_texture_create(uint32_t width, uint32_t height, const double* rgb) {
  if (width == 0 || height == 0) { fail("texture: width and height must be at least 1"); return nullptr; }
  if (width > RTC_TEXTURE_MAX_SIDE || height > RTC_TEXTURE_MAX_SIDE) { fail("texture: a side above RTC_TEXTURE_MAX_SIDE (16384)"); return nullptr; }
  if (!rgb) { fail("texture: rgb is NULL"); return nullptr; }
  auto t = std::make_shared<Tex>();
  t->w = width; t->h = height;
  t->rgb.assign(rgb, rgb + (size_t)3 * width * height);
  return new rtw_texture{t};
}
void rtw_texture_release(rtw_texture* t) { delete t; }
rtw_pattern* rtw_pattern_uv(int map_kind, const double t[16], const rtw_uv_pattern* faces, size_t n_faces) {
  if (map_kind < RTC_UVMAP_PLANAR || map_kind > RTC_UVMAP_CUBE) { fail("uv: map kind out of range (planar, spherical, cylindrical, cube)"); return nullptr; }
  if (!t) { fail("uv: transform is NULL"); return nullptr; }
  const size_t want = map_kind == RTC_UVMAP_CUBE ? 6 : 1;
  if (!faces || n_faces != want) { fail(map_kind == RTC_UVMAP_CUBE ? "uv: a cube map takes 6 faces" : "uv: this map takes 1 face"); return nullptr; }
  auto p = std::make_shared<Pat>();
  p->tag = RTC_PAT_UV; p->kind = map_kind;
  for (size_t k = 0; k < n_faces; k++) {
    const rtw_uv_pattern& in = faces[k];
    UvFace f;
    f.kind = in.kind; f.width = in.width; f.height = in.height;
    if (in.kind < RTC_UV_CHECKERS || in.kind > RTC_UV_IMAGE_LINEAR_WRAP) { fail("uv: face kind out of range (checkers, align_check, image, image_linear, image_linear_wrap_u, image_linear_wrap)"); return nullptr; }
    if (in.kind == RTC_UV_CHECKERS && !(std::isfinite(in.width) && in.width > 0.0 && std::isfinite(in.height) && in.height > 0.0)) {
      fail("uv: checkers width and height must be finite and > 0");
      return nullptr;
    }
    if (in.kind >= RTC_UV_IMAGE) {  // nearest or bilinear
      if (!in.texture) { fail(in.kind == RTC_UV_IMAGE ? "uv: image face without a texture" : "uv: face kind image_linear* without a texture"); return nullptr; }
      f.texture = in.texture->t;
    }
    for (int c = 0; c < f.n_children(); c++) {
      if (!in.child[c]) { fail("uv: child is NULL"); return nullptr; }
      f.child[c] = in.child[c]->p;
    }
    p->faces.push_back(f);
  }
  if (!M4::from(t).invert(&p->transform_inv)) { fail("uv: singular transform"); return nullptr; }
  if (p->frame_depth() > RTC_MAX_PATTERN_DEPTH) { fail("pattern keeps more than RTC_MAX_PATTERN_DEPTH colour frames on one path (blends / gradients / colour jitters nested deeper than 8)"); return nullptr; }
  return new rtw_pattern{p};
}

rtw_element* rtw_shape(int geometry, const double t[16], const rtw_material* material, int casts_shadow, const double* p, size_t np) {
  Geo g;
  switch (geometry) {
    case RTW_SPHERE: g.kind = RTC_SPHERE; break;
    case RTW_PLANE: g.kind = RTC_PLANE; break;
    case RTW_CUBE: g.kind = RTC_CUBE; break;
    case RTW_CYLINDER:
    case RTW_CONE:
      if (np != 3) { fail("cylinder/cone: params = {min,max,closed}"); return nullptr; }
      g.kind = geometry == RTW_CYLINDER ? RTC_CYLINDER : RTC_CONE;
      g.lo = p[0]; g.hi = p[1]; g.closed = p[2] != 0.0;
      break;
    case RTW_TRIANGLE:
      if (np != 9) { fail("triangle: 9 params"); return nullptr; }
      g = Geo::triangle(p, nullptr);
      break;
    case RTW_SMOOTH_TRIANGLE:
      if (np != 18) { fail("smooth triangle: 18 params"); return nullptr; }
      g = Geo::triangle(p, p + 9);
      break;
    default: fail("unknown geometry"); return nullptr;
  }
  std::string err;
  auto e = Elem::shape(M4::from(t), to_mat(material), casts_shadow != 0, g, &err);
  if (!e) { fail(err); return nullptr; }
  return new rtw_element{std::move(e)};
}

rtw_element* rtw_composite(const double t[16], const rtw_material* material, int kind, rtw_element** children, size_t n) {
  std::vector<std::unique_ptr<Elem>> kids;
  for (size_t i = 0; i < n; i++) {
    if (!children[i] || !children[i]->e) { fail("composite: NULL/consumed child"); return nullptr; }
  }
  for (size_t i = 0; i < n; i++) {
    kids.push_back(std::move(children[i]->e));
    delete children[i];
  }
  Mat m = to_mat(material);
  std::string err;
  auto e = Elem::group(M4::from(t), material ? &m : nullptr, kind, std::move(kids), &err);
  if (!e) { fail(err); return nullptr; }
  return new rtw_element{std::move(e)};
}

rtw_element* rtw_parse_obj(const char* path, const double t[16], const rtw_material* material, uint64_t* n_ignored, uint64_t* n_triangles) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { fail(std::string("cannot open ") + path); return nullptr; }
  std::stringstream ss;
  ss << f.rdbuf();
  M4 tr = M4::from(t), tmp;
  if (!tr.invert(&tmp)) { fail("parse_obj: singular transform"); return nullptr; }
  ObjOut o = parse_obj_text(ss.str(), tr, to_mat(material));
  if (!o.error.empty() || !o.root) { fail(o.error.empty() ? "parse_obj: no geometry" : o.error); return nullptr; }
  if (n_ignored) *n_ignored = o.ignored;
  if (n_triangles) *n_triangles = o.triangles;
  return new rtw_element{std::move(o.root)};
}
int rtw_element_set_bump(rtw_element* e, int32_t kind, uint32_t octaves, double amplitude, double frequency) {
  if (!e || !e->e) return fail("set_bump: NULL/consumed element");
  rtc_bump b{};
  b.kind = kind; b.octaves = octaves; b.amplitude = amplitude; b.frequency = frequency;
  if (kind != RTC_BUMP_SIMPLEX && kind != RTC_BUMP_FRACTAL && kind != RTC_BUMP_RIPPLE) return fail("set_bump: unknown kind of bump");
  if (!std::isfinite(amplitude)) return fail("set_bump: the bump's amplitude is not finite");
  if (!(std::isfinite(frequency) && frequency > 0.0)) return fail("set_bump: the bump's frequency must be finite and > 0");
  if (kind == RTC_BUMP_FRACTAL && (octaves == 0 || octaves > RTC_BUMP_MAX_OCTAVES)) return fail("set_bump: a fractal bump takes 1 .. RTC_BUMP_MAX_OCTAVES (64) octaves");
  e->e->set_bump(kind, kind == RTC_BUMP_FRACTAL ? octaves : 0u, amplitude, frequency);
  return 0;
}
void rtw_element_release(rtw_element* e) { delete e; }

rtw_world* rtw_world_create(void) { return new rtw_world(); }
int rtw_world_add_light(rtw_world* w, const double i[3], const double o[3]) {
  Light l;
  std::memcpy(l.intensity, i, sizeof(l.intensity));
  std::memcpy(l.origin, o, sizeof(l.origin));
  w->w.lights.push_back(l);
  if (!w->lights_ex.empty()) {
    rtc_light_ex x{};
    x.kind = RTC_LIGHT_POINT;
    std::memcpy(x.intensity, i, sizeof(x.intensity));
    std::memcpy(x.corner, o, sizeof(x.corner));
    w->lights_ex.push_back(x);
  }
  if (w->scene) { rtc_scene_destroy(w->scene); w->scene = nullptr; }
  return 0;
}
int rtw_world_add_area_light(rtw_world* w, const double i[3], const double corner[3], const double uvec[3], uint32_t usteps, const double vvec[3], uint32_t vsteps,
                             int jitter) {
  if (w->lights_ex.empty()) {  // the point lights added so far, in order
    for (const Light& p : w->w.lights) {
      rtc_light_ex x{};
      x.kind = RTC_LIGHT_POINT;
      std::memcpy(x.intensity, p.intensity, sizeof(x.intensity));
      std::memcpy(x.corner, p.origin, sizeof(x.corner));
      w->lights_ex.push_back(x);
    }
  }
  rtc_light_ex x{};
  x.kind = RTC_LIGHT_AREA;
  x.usteps = usteps; x.vsteps = vsteps;
  x.flags = jitter ? RTC_LIGHT_JITTER : 0u;
  std::memcpy(x.intensity, i, sizeof(x.intensity));
  std::memcpy(x.corner, corner, sizeof(x.corner));
  std::memcpy(x.uvec, uvec, sizeof(x.uvec));
  std::memcpy(x.vvec, vvec, sizeof(x.vvec));
  w->lights_ex.push_back(x);
  if (w->scene) { rtc_scene_destroy(w->scene); w->scene = nullptr; }
  return 0;
}
int rtw_world_set_light_cone(rtw_world* w, uint32_t light, const double axis[3], double cos_inner, double cos_outer) {
  if (!w || !axis) return fail("set_light_cone: NULL argument");
  if ((size_t)light >= w->n_lights()) return fail("set_light_cone: the world has no light " + std::to_string(light) + " yet");
  for (const rtc_light_cone& c : w->cones) if (c.light == light) return fail("set_light_cone: light " + std::to_string(light) + " already has a cone");
  if (const char* why = cone_invalid(axis, cos_inner, cos_outer)) return fail(std::string("set_light_cone: ") + why);
  rtc_light_cone c{};
  c.light = light;
  std::memcpy(c.axis, axis, sizeof(c.axis));
  c.cos_inner = cos_inner; c.cos_outer = cos_outer;
  w->cones.push_back(c);
  if (w->scene) { rtc_scene_destroy(w->scene); w->scene = nullptr; }
  return 0;
}
int rtw_world_set_background(rtw_world* w, const rtw_pattern* pattern, int32_t projection) {
  if (!w || !pattern || !pattern->p) return fail("set_background: NULL argument");
  if (projection != RTC_BG_DIRECTION && projection != RTC_BG_CUBE) return fail("set_background: unknown projection of the background");
  w->background = pattern->p;
  w->background_projection = projection;
  if (w->scene) { rtc_scene_destroy(w->scene); w->scene = nullptr; }
  return 0;
}
int rtw_world_add_element(rtw_world* w, rtw_element* e) {
  if (!e || !e->e) return fail("add_element: NULL/consumed element");
  w->w.elements.push_back(std::move(e->e));
  delete e;
  if (w->scene) { rtc_scene_destroy(w->scene); w->scene = nullptr; }
  return 0;
}
uint64_t rtw_world_primitive_count(const rtw_world* w) {
  uint64_t n = 0;
  for (auto& e : w->w.elements) n += e->count_prims();
  return n;
}
void rtw_world_release(rtw_world* w) { delete w; }

int rtw_render(rtw_world* w, const rtw_camera* cam, int fuel, const uint64_t* idx, uint64_t n, double* rgb, rtw_hit* hits) {
  if (ensure_scene(w)) return 1;
  rtc_camera c;
  if (!make_camera(cam->hsize, cam->vsize, cam->field_of_view, M4::from(cam->transform), &c)) return fail("camera: singular transform");
  static_assert(sizeof(rtw_hit) == sizeof(rtc_hit), "hit layout");
  int rc = rtc_render(w->scene, &c, fuel, idx, 0, n, rgb, (rtc_hit*)hits, nullptr);
  if (rc != RTC_OK) return fail(std::string("rtc_render: ") + rtc_last_error());
  return 0;
}

int rtw_color_at(rtw_world* w, const double* rays, uint64_t n, int fuel, double* rgb, rtw_hit* hits) {
  if (ensure_scene(w)) return 1;
  int rc = rtc_trace_rays(w->scene, rays, n, fuel, rgb, (rtc_hit*)hits, nullptr);
  if (rc != RTC_OK) return fail(std::string("rtc_trace_rays: ") + rtc_last_error());
  return 0;
}

// ---- product-only helpers for the Python harness / bench (not in rtw.h) ------------------------------------
// The flattened + uploaded scene behind a world (created on first use).
rtc_scene* rtw_world_scene(rtw_world* w, int device) {
  if (w->scene && w->device != device) { rtc_scene_destroy(w->scene); w->scene = nullptr; }
  w->device = device;
  if (ensure_scene(w)) return nullptr;
  return w->scene;
}
// Camera::new -> rtc_camera.
int rtw_make_camera(const rtw_camera* cam, rtc_camera* out) {
  if (!make_camera(cam->hsize, cam->vsize, cam->field_of_view, M4::from(cam->transform), out)) return fail("camera: singular transform");
  return 0;
}
// Flatten only (no device): sizes of the arrays a Rust shim would hand to rtc_scene_create.  Works without a GPU.
// A world with an area light has no such descriptor: its lights are an rtc_light_ex list for rtc_scene_create_ex, which these two
// helpers do not hand out, and a descriptor without them would render a different scene.  Both refuse such a world.
static int refuse_area(const rtw_world* w) {
  return w->lights_ex.empty() ? 0 : fail("flatten: the world has area lights; its lights are an rtc_light_ex list for rtc_scene_create_ex, not desc->lights");
}
// ... a world with a light cone, which only rtc_scene_create_ext2 takes ...
static int refuse_cones(const rtw_world* w) {
  return w->cones.empty() ? 0 : fail("flatten: the world has light cones; they go to rtc_scene_create_ext2, not into a descriptor");
}
// ... a world with a background, which only rtc_scene_create_ext3 takes ...
static int refuse_background(const rtw_world* w) {
  return !w->background ? 0 : fail("flatten: the world has a background; it goes to rtc_scene_create_ext3, not into a descriptor");
}
// ... a world with a bump on some shape, whose records only rtc_scene_create_ext4 takes ...
static int refuse_bumps(const rtw_world* w) {
  for (auto& e : w->w.elements)
    if (e->has_bump()) return fail("flatten: the world has a bump on a shape; bump records go to rtc_scene_create_ext4, not into a descriptor");
  return 0;
}
// ... and a world with a texture-mapped pattern, whose records and textures only rtc_scene_create_ext takes.
static int refuse_uv(const Flat& f) {
  return f.uv_pats.empty() ? 0 : fail("flatten: the world has texture-mapped patterns; their records and textures go to rtc_scene_create_ext, not into a descriptor");
}
int rtw_world_flatten_counts(rtw_world* w, uint32_t counts[8]) {
  if (refuse_area(w) || refuse_cones(w) || refuse_background(w) || refuse_bumps(w)) return 1;
  Flat f;
  Flattener fl(f);
  if (!fl.run(w->w)) return fail("flatten: " + f.error);
  if (refuse_uv(f)) return 1;
  rtc_scene_desc d = f.desc();
  counts[0] = d.n_nodes; counts[1] = d.n_prims; counts[2] = d.n_xforms; counts[3] = d.n_limits;
  counts[4] = d.n_tris; counts[5] = d.n_materials; counts[6] = d.n_pattern_nodes; counts[7] = d.n_lights;
  return 0;
}

// Flatten only (no device): the descriptor a Rust shim would hand to rtc_scene_create; its arrays live in the world handle until
// the next call / the world's release.  Works without a GPU (tests compare it with a foreign flattener's output).
int rtw_world_flatten_desc(rtw_world* w, rtc_scene_desc* out) {
  if (refuse_area(w) || refuse_cones(w) || refuse_background(w) || refuse_bumps(w)) return 1;
  w->flat.reset(new Flat());
  Flattener fl(*w->flat);
  if (!fl.run(w->w)) return fail("flatten: " + w->flat->error);
  if (refuse_uv(*w->flat)) return 1;
  *out = w->flat->desc();
  return 0;
}

}  // extern "C"

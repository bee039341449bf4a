// oracle/oracle_ext_capi.cpp — TEST INFRASTRUCTURE.  liboracle_ext.so: everything liboracle.so exports (oracle_capi.cpp, compiled
// here with ORC_EXT set, so that rt_oracle.hpp's hooks and rt_oracle_ext.hpp come in), plus include/rtw.h's extension entry points
// with the product library's limits, plus a few probes of the single rules (orc_ext_*).  Never loaded by the product package.
#define ORC_EXT 1
#include "oracle_capi.cpp"

#include "../include/rtc.h"

struct rtw_texture { std::shared_ptr<const Texture> t; };

static WorldExt& ext_of(rtw_world* w) {
  if (!w->w.ext) w->w.ext = std::make_shared<WorldExt>();
  return *w->w.ext;
}
template <class T>
static void put(std::vector<std::shared_ptr<const T>>& v, size_t k, std::shared_ptr<const T> x) {
  if (v.size() <= k) v.resize(k + 1);
  v[k] = std::move(x);
}

extern "C" {

rtw_texture* rtw_texture_create(uint32_t width, uint32_t height, const double* rgb) {
  if (width == 0 || height == 0) { fail("texture: width and height must be at least 1"); return nullptr; }
  if (width > RTC_TEXTURE_MAX_SIDE || height > RTC_TEXTURE_MAX_SIDE) { fail("texture: a side above RTC_TEXTURE_MAX_SIDE (16384)"); return nullptr; }
  if (!rgb) { fail("texture: rgb is NULL"); return nullptr; }
  auto t = std::make_shared<Texture>();
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
  Matrix m = Matrix::from16(t), inv;
  if (!m.inverse(&inv)) { fail("uv: singular transform (src/linalg/matrix.rs:181)"); return nullptr; }
  auto node = std::make_shared<UvNode>();
  node->map = (UvMap)map_kind;
  for (size_t k = 0; k < n_faces; k++) {
    const rtw_uv_pattern& in = faces[k];
    if (in.kind < RTC_UV_CHECKERS || in.kind > RTC_UV_IMAGE) { fail("uv: face kind out of range (checkers, align_check, image)"); return nullptr; }
    UvRecord r;
    r.kind = (UvKind)in.kind; r.width = in.width; r.height = in.height;
    if (in.kind == RTC_UV_CHECKERS && !(std::isfinite(in.width) && in.width > 0.0 && std::isfinite(in.height) && in.height > 0.0)) {
      fail("uv: checkers width and height must be finite and > 0");
      return nullptr;
    }
    if (in.kind == RTC_UV_IMAGE) {
      if (!in.texture) { fail("uv: image face without a texture"); return nullptr; }
      r.texture = in.texture->t;
    }
    const int nc = in.kind == RTC_UV_CHECKERS ? 2 : (in.kind == RTC_UV_ALIGN_CHECK ? 5 : 0);
    for (int c = 0; c < nc; c++) {
      if (!in.child[c]) { fail("uv: child is NULL"); return nullptr; }
      r.child[c] = in.child[c]->p;
    }
    node->records.push_back(std::move(r));
  }
  auto p = std::make_shared<Pattern>();
  p->tag = Pattern::UV;
  p->transform_inv = inv;
  p->uv = node;
  return new rtw_pattern{p};
}

int rtw_world_add_area_light(rtw_world* w, const double i[3], const double corner[3], const double uvec[3], uint32_t usteps, const double vvec[3], uint32_t vsteps,
                             int jitter) {
  if (!w || !i || !corner || !uvec || !vvec) return fail("add_area_light: NULL argument");
  if (usteps == 0 || vsteps == 0) return fail("add_area_light: usteps and vsteps must be at least 1");
  if (usteps > RTC_AREA_MAX_STEPS || vsteps > RTC_AREA_MAX_STEPS) return fail("add_area_light: more than RTC_AREA_MAX_STEPS (16) steps along a side");
  auto a = std::make_shared<AreaLight>();
  a->corner = Vector::point(corner[0], corner[1], corner[2]);
  a->uvec = Vector::vector(uvec[0], uvec[1], uvec[2]);
  a->vvec = Vector::vector(vvec[0], vvec[1], vvec[2]);
  a->usteps = usteps; a->vsteps = vsteps; a->jitter = jitter != 0;
  put<AreaLight>(ext_of(w).area, w->w.lights.size(), a);
  w->w.lights.push_back({{i[0], i[1], i[2]}, a->corner});
  return 0;
}

int rtw_world_set_light_cone(rtw_world* w, uint32_t light, const double axis[3], double cos_inner, double cos_outer) {
  if (!w || !axis) return fail("set_light_cone: NULL argument");
  if ((size_t)light >= w->w.lights.size()) return fail("set_light_cone: the world has no light " + std::to_string(light) + " yet");
  if (w->w.ext && w->w.ext->cone_of(light)) return fail("set_light_cone: light " + std::to_string(light) + " already has a cone");
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(axis[k])) return fail("set_light_cone: the axis is not finite");
  const double m = std::sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
  if (!(m > 0.0) || !std::isfinite(m)) return fail("set_light_cone: the axis is zero or its length is not finite");
  if (!std::isfinite(cos_inner) || !std::isfinite(cos_outer) || cos_inner < -1.0 || cos_inner > 1.0 || cos_outer < -1.0 || cos_outer > 1.0)
    return fail("set_light_cone: the cosines must be finite and within [-1, 1]");
  if (cos_outer > cos_inner) return fail("set_light_cone: cos_outer above cos_inner");
  put<LightCone>(ext_of(w).cone, light, std::make_shared<LightCone>(LightCone::make(axis, cos_inner, cos_outer)));
  return 0;
}

int rtw_world_set_background(rtw_world* w, const rtw_pattern* pattern, int32_t projection) {
  if (!w || !pattern || !pattern->p) return fail("set_background: NULL argument");
  if (projection != RTC_BG_DIRECTION && projection != RTC_BG_CUBE) return fail("set_background: unknown projection of the background");
  WorldExt& x = ext_of(w);
  x.background = pattern->p;
  x.projection = projection;
  return 0;
}

// include/rtw.h: the record on the material of every primitive of the element (a shape, a whole group, an OBJ element); a second call
// replaces the first; a group built with a material afterwards replaces its children's materials (Element::propagate_inverses), the
// record with the rest.  The limits are rtc_scene_create_ext4's.
static const char* bump_limits(int32_t kind, uint32_t octaves, double amplitude, double frequency) {
  if (kind < RTC_BUMP_SIMPLEX || kind > RTC_BUMP_RIPPLE) return "bump: unknown kind (simplex, fractal, ripple)";
  if (!std::isfinite(amplitude)) return "bump: the amplitude is not finite";
  if (!std::isfinite(frequency) || !(frequency > 0.0)) return "bump: the frequency must be finite and > 0";
  if (kind == RTC_BUMP_FRACTAL && (octaves == 0 || octaves > RTC_BUMP_MAX_OCTAVES)) return "bump: fractal octaves must be within 1..RTC_BUMP_MAX_OCTAVES (64)";
  return nullptr;
}
static void put_bump(Element& e, const std::shared_ptr<const BumpRecord>& b) {
  if (!e.is_group) { e.shape.material.bump = b; return; }
  for (auto& c : e.children) put_bump(*c, b);
}
int rtw_element_set_bump(rtw_element* e, int32_t kind, uint32_t octaves, double amplitude, double frequency) {
  if (!e || !e->e) return fail("set_bump: NULL/consumed element");
  if (const char* why = bump_limits(kind, octaves, amplitude, frequency)) return fail(why);
  auto b = std::make_shared<BumpRecord>();
  b->kind = kind; b->octaves = octaves; b->amplitude = amplitude; b->frequency = frequency;
  put_bump(*e->e, b);
  return 0;
}

// ---- probes of the single rules ---------------------------------------------------------------------------------------------------
// The usteps * vsteps sample positions (k order) of an area light that is number light_index of its list, for a shading point `over`.
void orc_ext_sample_positions(const double corner[3], const double uvec[3], uint32_t usteps, const double vvec[3], uint32_t vsteps, int jitter,
                              uint64_t light_index, const double over[3], double* out) {
  AreaLight a;
  a.corner = Vector::point(corner[0], corner[1], corner[2]);
  a.uvec = Vector::vector(uvec[0], uvec[1], uvec[2]);
  a.vvec = Vector::vector(vvec[0], vvec[1], vvec[2]);
  a.usteps = usteps; a.vsteps = vsteps; a.jitter = jitter != 0;
  std::vector<Vector> s;
  area_samples(a, light_index, Vector::point(over[0], over[1], over[2]), s);
  for (size_t k = 0; k < s.size(); k++) { out[3 * k] = s[k].x; out[3 * k + 1] = s[k].y; out[3 * k + 2] = s[k].z; }
}
// The cone factor f (the axis is normalised here, as at scene creation).
double orc_ext_spot_factor(const double axis[3], double cos_inner, double cos_outer, const double light_pos[3], const double point[3]) {
  return spot_factor(LightCone::make(axis, cos_inner, cos_outer), Vector::point(light_pos[0], light_pos[1], light_pos[2]),
                     Vector::point(point[0], point[1], point[2]));
}
// A pattern's colour at n points (x, y, z; w = 1); tie (optional): the tie flag of each evaluation.
void orc_ext_pattern_colors(const rtw_pattern* p, const double* points, uint64_t n, double* rgb, uint8_t* tie) {
  for (uint64_t q = 0; q < n; q++) {
    g_tie = false;
    Color c = p->p->color_at(Vector::point(points[3 * q], points[3 * q + 1], points[3 * q + 2]));
    rgb[3 * q] = c.r; rgb[3 * q + 1] = c.g; rgb[3 * q + 2] = c.b;
    if (tie) tie[q] = g_tie ? 1 : 0;
  }
}
// Steps 1-4 of rtc_bump: the unit shading normal before the inside flip, for a record, a material_inv (16, row-major), a hit point and
// the unit normal.
int orc_ext_bump_normal(int32_t kind, uint32_t octaves, double amplitude, double frequency, const double material_inv[16], const double point[3],
                        const double normal[3], double out[3]) {
  if (!material_inv || !point || !normal || !out) return fail("bump_normal: NULL argument");
  if (const char* why = bump_limits(kind, octaves, amplitude, frequency)) return fail(why);
  BumpRecord b;
  b.kind = kind; b.octaves = octaves; b.amplitude = amplitude; b.frequency = frequency;
  bump_normal(b, Matrix::from16(material_inv), Vector::point(point[0], point[1], point[2]), Vector::vector(normal[0], normal[1], normal[2]), out);
  return 0;
}
// rtc_bump_normals' counterpart: item q is a primitive (its place in the depth-first numbering), a point and a unit normal; out is steps
// 1-4 with the record and the material_inv that primitive holds in THIS world, or the normal itself where its material has no record.
int orc_ext_world_bump_normals(const rtw_world* w, const int32_t* prims, const double* points, const double* normals, uint64_t n, double* out) {
  if (!w || !prims || !points || !normals || !out) return fail("world_bump_normals: NULL argument");
  std::vector<const Shape*> order;
  w->w.number_shapes(order);
  for (uint64_t q = 0; q < n; q++) {
    if (prims[q] < 0 || (size_t)prims[q] >= order.size()) return fail("world_bump_normals: primitive out of range");
    const Shape& s = *order[(size_t)prims[q]];
    const double *X = points + 3 * q, *nn = normals + 3 * q;
    if (!s.material.bump) { out[3 * q] = nn[0]; out[3 * q + 1] = nn[1]; out[3 * q + 2] = nn[2]; continue; }
    bump_normal(*s.material.bump, s.material_inv, Vector::point(X[0], X[1], X[2]), Vector::vector(nn[0], nn[1], nn[2]), out + 3 * q);
  }
  return 0;
}
// normal . eye of the state of each listed pixel's (idx == NULL: every pixel's) primary hit -- the shading normal after the flip against
// the eye vector; NaN for a pixel that hits nothing.  Negative where a bump turns the shading normal away from the viewer.
int orc_ext_pixel_normal_dot_eye(rtw_world* w, const rtw_camera* cam, const uint64_t* idx, uint64_t n, double* out) {
  Matrix m = Matrix::from16(cam->transform), inv;
  if (!m.inverse(&inv)) return fail("camera: singular transform");
  Camera c = Camera::make((size_t)cam->hsize, (size_t)cam->vsize, cam->field_of_view, m);
  World::Ctx ctx;
  for (uint64_t q = 0; q < n; q++) {
    uint64_t i = idx ? idx[q] : q;
    Ray ray = c.ray_at_pixel((size_t)(i % c.hsize), (size_t)(i / c.hsize));
    w->w.intersect(ray, ctx);
    sort_intersections(ctx.xs, &ctx.nan_seen);
    const Intersection* h = hit(ctx.xs);
    out[q] = std::nan("");
    if (h) {
      Intersection self = *h;
      State st = prepare_state(self, ray, ctx.xs);
      out[q] = st.normal.dot(st.eye);
    }
  }
  return 0;
}
// Where a ray of direction dir looks the background up.
int orc_ext_background_point(int32_t projection, const double dir[3], double point[3]) {
  if (projection != RTC_BG_DIRECTION && projection != RTC_BG_CUBE) return fail("background_point: unknown projection");
  Vector p = background_point(projection, Vector::vector(dir[0], dir[1], dir[2]));
  point[0] = p.x; point[1] = p.y; point[2] = p.z;
  return 0;
}
// The tie flag of each listed pixel's (idx == NULL: every pixel's) ray tree, and of each ray's.  A pass of their own: the flag is a
// property of the inputs, not a result.
int orc_ext_pixel_ties(rtw_world* w, const rtw_camera* cam, int fuel, const uint64_t* idx, uint64_t n, uint8_t* tie) {
  Matrix m = Matrix::from16(cam->transform), inv;
  if (!m.inverse(&inv)) return fail("camera: singular transform");
  Camera c = Camera::make((size_t)cam->hsize, (size_t)cam->vsize, cam->field_of_view, m);
  unsigned threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::atomic<uint64_t> next{0};
  auto worker = [&]() {
    for (;;) {
      uint64_t q = next.fetch_add(1);
      if (q >= n) break;
      uint64_t i = idx ? idx[q] : q;
      World::Ctx ctx;
      ctx.fuel0 = fuel;
      g_tie = false;
      w->w.color_at(c.ray_at_pixel((size_t)(i % c.hsize), (size_t)(i / c.hsize)), fuel, ctx);
      tie[q] = g_tie ? 1 : 0;
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < threads; t++) pool.emplace_back(worker);
  for (auto& th : pool) th.join();
  return 0;
}
int orc_ext_ray_ties(rtw_world* w, const double* rays, uint64_t n, int fuel, uint8_t* tie) {
  for (uint64_t q = 0; q < n; q++) {
    const double* r = rays + 6 * q;
    World::Ctx ctx;
    ctx.fuel0 = fuel;
    g_tie = false;
    w->w.color_at(Ray{Vector::point(r[0], r[1], r[2]), Vector::vector(r[3], r[4], r[5])}, fuel, ctx);
    tie[q] = g_tie ? 1 : 0;
  }
  return 0;
}

}  // extern "C"

/* rtw.h — C handles over the host-side mirror of the reference's scene API.
 *
 * The reference's hot path sits behind safe Rust types (`World`, `Element`, `Shape`, `Material`,
 * `Pattern`, `Camera`, `Image::par_render`).  This header exposes a C++ mirror of those
 * types through opaque handles so that non-Rust hosts (this repo's Python harness, tests, bench) can
 * build the same scenes.  It is implemented twice, with identical symbols:
 *
 *   raytracer_challenge_amd/csrc  -> librtc_amd.so   the product: flatten once -> HIP kernels (rtc.h)
 *   oracle/                       -> liboracle.so    test infrastructure: literal CPU restatement
 *
 * A Rust host does NOT need this layer: it binds rtc.h directly.
 *
 * Each entry point names the reference item it mirrors (paths relative to the reference crate).
 */
#ifndef RTW_H
#define RTW_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtw_pattern rtw_pattern; /* src/material.rs:60-65  Pattern (immutable, ref-counted) */
typedef struct rtw_element rtw_element; /* src/shape.rs:31-34     Element (owned until consumed)   */
typedef struct rtw_world rtw_world;     /* src/world.rs:12-15     World                            */

/* src/material.rs:19-28 Material.  `pattern` is borrowed; NULL = Pattern::plain(white) (:32). */
typedef struct rtw_material {
  double ambient, diffuse, specular, shininess, reflective, transparency, refractive_index;
  const rtw_pattern* pattern;
} rtw_material;

/* src/camera.rs:16-37 Camera::new(hsize, vsize, field_of_view, transform); row-major 4x4. */
typedef struct rtw_camera {
  uint64_t hsize, vsize;
  double field_of_view;
  double transform[16];
} rtw_camera;

/* Parity channel: nearest hit of a traced ray.  prim = DFS sequence number of the primitive in
 * world.elements order (-1 = miss); push_idx = position among that primitive's own pushes
 * (src/shape.rs:608-619, :667-678, :746-767).  t is the reference's Intersection.t, bit-exact. */
typedef struct rtw_hit {
  double t;
  int32_t prim;
  int32_t push_idx;
} rtw_hit;

enum { RTW_SPHERE = 0, RTW_PLANE = 1, RTW_CUBE = 2, RTW_CYLINDER = 3, RTW_CONE = 4, RTW_TRIANGLE = 5, RTW_SMOOTH_TRIANGLE = 6 };
enum { RTW_UNION = 0, RTW_INTERSECTION = 1, RTW_DIFFERENCE = 2, RTW_AGGREGATION = 3 }; /* src/shape.rs:161-166 */
enum { RTW_JITTER_COLOR = 0, RTW_JITTER_POINT = 1 };                                    /* src/material.rs:190-193 */
enum { RTW_BLEND = 0, RTW_CHECKERS = 1, RTW_RING_GRADIENT = 2, RTW_RING = 3, RTW_GRADIENT = 4, RTW_STRIPES = 5 }; /* :227-234 */
enum { RTW_NOISE_SIMPLEX = 0, RTW_NOISE_FRACTAL = 1 };                                  /* src/noise.rs:4-7 */

/* 0 = ok; non-zero = failure, message in rtw_last_error() (never unwinds across the boundary). */
const char* rtw_last_error(void);
/* "hip" for the product library, "oracle-cpu" for the oracle. */
const char* rtw_backend(void);

/* Patterns (src/material.rs:110-162).  Children are borrowed (shared), results are new handles. */
rtw_pattern* rtw_pattern_debug(void);
rtw_pattern* rtw_pattern_plain(double r, double g, double b);
rtw_pattern* rtw_pattern_jitter(int jitter_kind, int noise_kind, double scale, uint64_t octaves, const rtw_pattern* child);
rtw_pattern* rtw_pattern_mixture(int mixture_kind, const double transform[16], const rtw_pattern* left, const rtw_pattern* right);
void rtw_pattern_release(rtw_pattern*);

/* Texture mapping (include/rtc.h RTC_PAT_UV; the book's bonus chapter, not in the reference).  Product library only: the oracle
 * restates the reference, which has none, and rendering such a world needs rtc_scene_create_ext.
 * rtw_texture_create copies h rows of w {r, g, b} (row 0 at the top); textures are immutable and ref-counted like patterns.
 * rtw_pattern_uv: map_kind = RTC_UVMAP_*, transform as rtw_pattern_mixture's; n_faces = 1, or 6 for a cube map (left, front, right,
 * back, up, down).  A face is one rtc_uv_pattern: kind RTC_UV_*, width / height (checkers), texture (image) and the children its
 * kind reads (checkers: child[0], child[1]; align check: main, ul, ur, bl, br), all borrowed.  The bilinear image kinds
 * RTC_UV_IMAGE_LINEAR, _LINEAR_WRAP_U and _LINEAR_WRAP take a texture as RTC_UV_IMAGE does and read no child. */
typedef struct rtw_texture rtw_texture;
typedef struct rtw_uv_pattern {
  int kind;
  double width, height;
  const rtw_texture* texture;
  const rtw_pattern* child[5];
} rtw_uv_pattern;
rtw_texture* rtw_texture_create(uint32_t width, uint32_t height, const double* rgb);
void rtw_texture_release(rtw_texture*);
rtw_pattern* rtw_pattern_uv(int map_kind, const double transform[16], const rtw_uv_pattern* faces, size_t n_faces);

/* Element::{sphere,plane,cube,cylinder,cone,triangle,smooth_triangle} (src/shape.rs:103-137).
 * params: cylinder/cone = {min, max, closed(0/1)}; triangle = p1,p2,p3 (9); smooth = p1,p2,p3,n1,n2,n3 (18). */
rtw_element* rtw_shape(int geometry, const double transform[16], const rtw_material* material, int casts_shadow,
                       const double* params, size_t n_params);
/* Element::composite(transform, Option<Material>, kind, children) (src/shape.rs:74-101).  Consumes children. */
rtw_element* rtw_composite(const double transform[16], const rtw_material* material_or_null, int kind,
                           rtw_element** children, size_t n_children);
/* ObjParser::new(path).parse_obj(transform, material) (src/obj.rs:186-258).  n_ignored may be NULL. */
rtw_element* rtw_parse_obj(const char* path, const double transform[16], const rtw_material* material,
                           uint64_t* n_ignored, uint64_t* n_triangles);
/* Normal perturbation (include/rtc.h rtc_bump; not in the reference): every primitive of the element, a shape or a whole group, gets
 * the bump record {kind (RTC_BUMP_*), octaves (fractal only), amplitude, frequency} on its material; a second call replaces the first.
 * A group built with a material afterwards replaces its children's materials, bumps included, as ever.  Two shapes that share a
 * material but not the bump flatten to two material rows.  Fails for numbers rtc_scene_create_ext4 would refuse.  Product library (rendering
 * such a world needs rtc_scene_create_ext4) and the tests' extended oracle; the reference restatement liboracle.so has no such entry. */
int rtw_element_set_bump(rtw_element*, int32_t kind, uint32_t octaves, double amplitude, double frequency);
void rtw_element_release(rtw_element*);

rtw_world* rtw_world_create(void);
int rtw_world_add_light(rtw_world*, const double intensity[3], const double origin[3]); /* src/light.rs:5-8 */
/* An area light (include/rtc.h rtc_light_ex; not in the reference): usteps x vsteps samples over the rectangle corner + [0, uvec] x
 * [0, vvec], jittered when jitter != 0.  Lights keep the order they were added in, point and area alike.  Product library only (the
 * oracle restates the reference, which has none); rendering such a world needs rtc_scene_create_ex. */
int rtw_world_add_area_light(rtw_world*, const double intensity[3], const double corner[3], const double uvec[3], uint32_t usteps,
                             const double vvec[3], uint32_t vsteps, int jitter);
/* A cone on the light added as number `light` (include/rtc.h rtc_light_cone; not in the reference): the light, point or area, becomes a
 * spot light pointing along `axis` (any length), full inside the half-angle of cosine cos_inner, dark outside cos_outer's.  Fails for
 * an index no light has yet, a second cone on one light and numbers rtc_scene_create_ext2 would refuse.  Product library only;
 * rendering such a world needs rtc_scene_create_ext2. */
int rtw_world_set_light_cone(rtw_world*, uint32_t light, const double axis[3], double cos_inner, double cos_outer);
/* The world's background (include/rtc.h rtc_background; not in the reference, where a ray that leaves the scene is black): a ray that
 * hits nothing sees `pattern` (borrowed, any kind) at the point `projection` (RTC_BG_DIRECTION / RTC_BG_CUBE) makes of its direction.
 * A second call replaces the first.  Fails for a NULL pattern and an unknown projection.  Product library only; rendering such a
 * world needs rtc_scene_create_ext3. */
int rtw_world_set_background(rtw_world*, const rtw_pattern* pattern, int32_t projection);
int rtw_world_add_element(rtw_world*, rtw_element*);                                    /* consumes */
uint64_t rtw_world_primitive_count(const rtw_world*);
void rtw_world_release(rtw_world*);

/* Image::par_render(&camera, &world) (src/image.rs:65-81) with `fuel` a runtime argument
 * (src/config.rs:2 hard-codes 5).  pixel_indices == NULL renders i = 0..hsize*vsize-1; otherwise the n
 * listed row-major indices.  rgb: n*3 doubles; hits: n records or NULL. */
int rtw_render(rtw_world*, const rtw_camera*, int fuel, const uint64_t* pixel_indices, uint64_t n, double* rgb,
               rtw_hit* hits);
/* World::color_at(ray, fuel, ..) (src/world.rs:134-149) for n rays given as {ox,oy,oz,dx,dy,dz}. */
int rtw_color_at(rtw_world*, const double* rays, uint64_t n, int fuel, double* rgb, rtw_hit* hits);

#ifdef __cplusplus
}
#endif
#endif

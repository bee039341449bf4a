/* rtc.h — the drop-in boundary of the hot path: `Image::par_render(&Camera, &World) -> Image`
 * (reference src/image.rs:65-81) and everything it calls (src/world.rs:18-149, src/intersection.rs:24-139,
 * src/shape.rs:139-158/225-269/414-462/592-946, src/bounding_box.rs:80-92, src/material.rs:164-302,
 * src/noise.rs:31-237, src/camera.rs:39-55), executed by hand-written HIP kernels on gfx950.
 *
 * The reference has no FFI of its own: the path sits behind one safe-Rust function.  A Rust
 * maintainer replaces the body of `par_render` with: flatten `&World` into an `rtc_scene_desc` (plain arrays,
 * field-wise copies — the Rust types are not #[repr(C)]), `rtc_scene_create`, `rtc_render`, copy the returned
 * doubles into `Vec<Color>`.  INTEGRATION.md shows that shim.  Every record below names the reference item it
 * carries.  All floating point is IEEE f64; matrices are row-major 4x4 exactly as `Matrix.data`.
 *
 * Ownership: `rtc_scene_create` copies everything it needs (the caller may free the arrays on return) and owns
 * all device memory; the caller owns output buffers.  Errors: status code + `rtc_last_error()`; nothing unwinds.
 * Threading: calls are blocking; distinct scenes may be used from distinct threads; one HIP stream per scene.
 *   - "Distinct": an object and everything a call on it touches belong to one thread at a time.  An `rtc_scene` is one object; an
 *     `rtc_multi` with all its replicas is one object of its caller; the K scenes handed to one rtc_render_shutter call belong to that
 *     caller for the length of the call.  Two threads on one scene at once are undefined.  Scene creation and destruction count as calls:
 *     any number of threads may create, render and destroy scenes of their own at the same time, on one device or several.
 *   - A scene rendered from a thread beside others gives the frame, hit records, digests and counters it gives alone, bit for bit
 *     (tests/test_threads_gpu.py); company changes only how many CUs an unsynchronised wavefront launch takes (rtc_scene_wavefront_ts_grid).
 *   - `rtc_last_error()` (and rtw.h's `rtw_last_error()`) is per thread: it returns the text of the calling thread's own most recent
 *     failed call, valid until that thread's next failing call.  A successful call leaves it unchanged; no call clears it.
 *   - Handles are not tied to a thread: a scene may be created on one thread, used on another and destroyed on a third, one at a time.
 *     Every entry point selects the scene's device itself.
 *   - Environment variables are read with getenv, never written: RTC_KERNEL, RTC_WF_*, RTC_NO_KOPS, RTC_KOPS_GROUPS, RTC_DEVICE_BVH*,
 *     RTC_LIGHT_GRID*, RTC_BUILD_THREADS and the other build switches when a scene is created; RTC_SAMPLED_MAX_RAYS, RTC_FILTER_LDS,
 *     RTC_FIRST_GUESS, RTC_WF_MAX_BYTES and RTC_CSG_MAX_BYTES at each launch.  A host that changes them does so before it starts threads.
 *   - Scene creation may start a few host threads of its own inside the call (large meshes); they are joined before it returns.
 * There is no CPU fallback: without a HIP device every entry point that computes returns RTC_ERR_DEVICE.
 */
#ifndef RTC_H
#define RTC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtc_scene rtc_scene;

enum {
  RTC_OK = 0,
  RTC_ERR_INVALID = 1,     /* malformed description (index out of range, cyclic pattern nodes, ...)    */
  RTC_ERR_UNSUPPORTED = 2, /* valid in the reference, beyond a device limit: CSG groups nested deeper than 32; a
                              pattern with more than RTC_MAX_PATTERN_DEPTH colour frames on one path (below); a launch
                              whose CSG intersection slab would exceed RTC_CSG_MAX_BYTES (16 GiB: a subtree with more
                              than 32 possible intersections gets that many rows per thread); a material whose
                              refractive_index is not in (1e-70, 1e70); more than 64 lights (an area light is one); an area
                              light with more than 16 steps along a side; a texture side above 16384 or more than 2^26
                              texels in one scene; fuel above 16; a sampled camera with more than 16 samples along a side */
  RTC_ERR_DEVICE = 3,      /* HIP failure / no device                                                   */
  RTC_ERR_NAN = 4          /* a NaN intersection t reached a sort the reference's comparator would run on: a list
                              of two or more entries of one World::intersect or CSG child list; the reference
                              panics there (src/intersection.rs:123-125).  A single NaN entry is legal: a slice
                              of one is never compared, the ray then has no hit                          */
};

/* Geometry (src/shape.rs:466-498). */
enum { RTC_SPHERE = 0, RTC_PLANE = 1, RTC_CUBE = 2, RTC_CYLINDER = 3, RTC_CONE = 4, RTC_TRIANGLE = 5, RTC_SMOOTH_TRIANGLE = 6 };
enum { RTC_FLAG_CASTS_SHADOW = 1u, RTC_FLAG_CLOSED = 2u };

/* Shape (src/shape.rs:297-306), one per primitive, in DFS order over world.elements (children in order).
 * The index of a record is the primitive's sequence number: intersection ties resolve by it exactly as the
 * reference's stable sort resolves them by insertion order (src/intersection.rs:123-125). */
typedef struct rtc_prim {
  int32_t geometry; /* RTC_SPHERE.. */
  uint32_t flags;   /* RTC_FLAG_* : Shape.casts_shadow, Cylinder/Cone.closed */
  int32_t material; /* index into materials (Shape.material) */
  int32_t xform;    /* index into xforms (Shape.transform_inv / material_inv; shared by a whole OBJ group) */
  int32_t data;     /* cylinder/cone: index into limits; triangles: index into tri_*; else -1 */
} rtc_prim;

/* Shape.transform_inv and Shape.material_inv after Element::propagate_inverses (src/shape.rs:47-72).
 * Shape.transform_inv_tsp is not passed: it is bitwise transpose(transform_inv). */
typedef struct rtc_xform {
  double transform_inv[16];
  double material_inv[16];
} rtc_xform;

/* Material (src/material.rs:19-28); `pattern` = index of the root rtc_pattern_node. */
typedef struct rtc_material {
  double ambient, diffuse, specular, shininess, reflective, transparency, refractive_index;
  int32_t pattern;
  int32_t _pad;
} rtc_material;

/* Pattern (src/material.rs:60-65) as a node array. */
enum { RTC_PAT_DEBUG = 0, RTC_PAT_PLAIN = 1, RTC_PAT_JITTER = 2, RTC_PAT_MIXTURE = 3 };
enum { RTC_JITTER_COLOR = 0, RTC_JITTER_POINT = 1 };
enum { RTC_MIX_BLEND = 0, RTC_MIX_CHECKERS = 1, RTC_MIX_RING_GRADIENT = 2, RTC_MIX_RING = 3, RTC_MIX_GRADIENT = 4, RTC_MIX_STRIPES = 5 };
enum { RTC_NOISE_SIMPLEX = 0, RTC_NOISE_FRACTAL = 1 };
/* Pattern trees may be of any depth (the reference's Box tree is unbounded); the device's walk keeps a frame only at nodes that
 * need both children's colours (Blend, RingGradient, Gradient) or post-process a child's colour (colour jitter): at most this many
 * of THOSE on one root-to-leaf path, else RTC_ERR_UNSUPPORTED.  Checkers, rings, stripes and point jitters nest freely. */
#define RTC_MAX_PATTERN_DEPTH 8
typedef struct rtc_pattern_node {
  int32_t tag;        /* RTC_PAT_* */
  int32_t kind;       /* RTC_JITTER_* or RTC_MIX_* */
  int32_t noise_kind; /* RTC_NOISE_* (jitter) */
  uint32_t octaves;   /* Noise::Fractal.octaves */
  int32_t left;       /* child node (jitter: the wrapped pattern), -1 if none */
  int32_t right;
  double scale;             /* Noise scale */
  double color[3];          /* Plain */
  double transform_inv[16]; /* Mixture.transform_inv */
} rtc_pattern_node;

/* PointLight (src/light.rs:5-8). */
typedef struct rtc_light {
  double intensity[3];
  double origin[3];
} rtc_light;

/* Either kind of light, for rtc_scene_create_ex / rtc_multi_create_ex.  The reference knows point lights only; the area light is
 * the rectangular light of the book's first bonus chapter ("Rendering soft shadows"), defined here as follows.
 *   RTC_LIGHT_POINT: intensity, corner = the origin; the other fields are ignored.  Exactly an rtc_light.
 *   RTC_LIGHT_AREA:  N = usteps * vsteps samples.  Cells uc = uvec / usteps, vc = vvec / vsteps (componentwise, f64).  Sample
 *     k = v * usteps + u (v outer, u inner) lies at p_k = (corner + uc * (u + ju)) + vc * (v + jv), componentwise, one rounding per
 *     operation.  Without RTC_LIGHT_JITTER ju = jv = 0.5 (the cell centres); with it they come from rtc_area_jitter
 *     (csrc/device_scene.h): h = m(m(m(m(light) ^ bits(x)) ^ bits(y)) ^ bits(z)) over the light's index in the list and the
 *     shading point's over_point (x, y, z) -- the shadow rays' origin --, ju = (m(h ^ 2k) >> 11) * 2^-53,
 *     jv = (m(h ^ (2k + 1)) >> 11) * 2^-53, m = SplitMix64's finaliser.  Deterministic: no state, nothing of the pixel or launch.
 *     Each sample adds exactly the reference's point-light term (World::is_shadowed + Shape::lighting, src/world.rs:26-82,
 *     src/shape.rs:429-462) for a light at p_k of intensity intensity / N (one f64 division), the N terms in k order: for the
 *     surface colour an area light is N point lights.  The reflected and refracted colour of a hit is added once per LIGHT
 *     (src/world.rs:58-79), and an area light is one light: once, not once per sample.
 * Limits: usteps == 0 or vsteps == 0 is RTC_ERR_INVALID; usteps > 16 or vsteps > 16 is RTC_ERR_UNSUPPORTED.  An area light counts as
 * one of the 64 lights a scene may have.  rtc_stats.rays_shadow counts one ray per sample. */
enum { RTC_LIGHT_POINT = 0, RTC_LIGHT_AREA = 1 };
enum { RTC_LIGHT_JITTER = 1u };
#define RTC_AREA_MAX_STEPS 16
typedef struct rtc_light_ex {
  int32_t kind;     /* RTC_LIGHT_* */
  uint32_t usteps, vsteps;
  uint32_t flags;   /* RTC_LIGHT_JITTER */
  double intensity[3];
  double corner[3]; /* point lights: the origin */
  double uvec[3];
  double vvec[3];
} rtc_light_ex;

/* Texture mapping (the book's third bonus chapter, "Texture mapping"; not in the reference), for rtc_scene_create_ext /
 * rtc_multi_create_ext.  A pattern node of tag RTC_PAT_UV maps its point to (u, v) and hands that to one rtc_uv_pattern record:
 *   kind          = the map: RTC_UVMAP_PLANAR, _SPHERICAL, _CYLINDRICAL or _CUBE;
 *   transform_inv = applied to the 4-vector point first, exactly as a Mixture applies it (the same four rows, w included);
 *   left          = index of the node's first rtc_uv_pattern record.  A cube map uses six consecutive records, in the book's
 *                   cube_map order: left, front, right, back, up, down.
 *   Every other field is ignored.
 * A UV node keeps no colour frame: like Checkers it selects a child or yields a colour, nests freely and does not count against
 * RTC_MAX_PATTERN_DEPTH (the frames of its children do).  Children are evaluated at the UV node's transformed point, as Mixture
 * children are.
 * Every step below is one f64 operation on the transformed point (x, y, z); floor and round are C's (round: half away from zero),
 * as_i32 = Rust's saturating `as i32` (NaN -> 0), wadd = wrapping i32 addition, PI = M_PI, m1(a) = a - floor(a),
 * m2(a) = a - 2.0 * floor(a * 0.5).
 *   PLANAR:      u = m1(x), v = m1(z).
 *   SPHERICAL:   theta = atan2(x, z), r = sqrt(x*x + y*y + z*z), phi = acos(y / r), u = 1.0 - (theta / (2.0*PI) + 0.5),
 *                v = 1.0 - phi / PI.
 *   CYLINDRICAL: u as SPHERICAL, v = m1(y).
 *   CUBE:        c = max(|x|, |y|, |z|) (a NaN operand is skipped, as Rust's f64::max does); the first test that holds picks the
 *                face: c == x right, c == -x left, c == y up, c == -y down, c == z front, otherwise (NaN included) back.  Then
 *                front (m2(x+1)/2, m2(y+1)/2), back (m2(1-x)/2, m2(y+1)/2), left (m2(z+1)/2, m2(y+1)/2),
 *                right (m2(1-z)/2, m2(y+1)/2), up (m2(x+1)/2, m2(1-z)/2), down (m2(x+1)/2, m2(z+1)/2).
 * The records (child[] entries are pattern-node indices; fields a kind does not use are ignored):
 *   RTC_UV_CHECKERS:    wadd(as_i32(floor(u * width)), as_i32(floor(v * height))) % 2 == 0 selects child[0], else child[1].
 *   RTC_UV_ALIGN_CHECK: children main, ul, ur, bl, br.  v > 0.8: u < 0.2 gives ul, u > 0.8 ur; else v < 0.2: u < 0.2 gives bl,
 *                       u > 0.8 br; anything else (NaN included) gives main.
 *   RTC_UV_IMAGE:       the texel of textures[texture] (w x h) at column xi = clamp(as_i32(round(u * (double)(w-1))), 0, w-1), row
 *                       yi = clamp(as_i32(round((1.0 - v) * (double)(h-1))), 0, h-1); row 0 is the top row.  No filtering; every
 *                       lookup stays in bounds (NaN and +-inf included).
 *   RTC_UV_IMAGE_LINEAR, RTC_UV_IMAGE_LINEAR_WRAP_U, RTC_UV_IMAGE_LINEAR_WRAP: the bilinear blend of four texels of textures[texture]
 *     (csrc/uv_image.h, one function for device and host).  They read `texture` exactly as RTC_UV_IMAGE does, have no children and
 *     ignore width / height / child[].  _LINEAR clamps both axes (cube-map faces, decals), _LINEAR_WRAP_U takes u as periodic and
 *     clamps v (spherical maps), _LINEAR_WRAP takes both as periodic (planar and cylindrical maps).
 *     Per axis, with n = the texture's size along it and a = the coordinate (columns: a = u; rows: a = 1.0 - v, row 0 at the top):
 *       clamped axis, texel centres where RTC_UV_IMAGE samples them (a = i / (n-1)):
 *         x = a * (double)(n - 1), f = floor(x), t = x - f, i0 = clamp(as_i32(f), 0, n-1), i1 = clamp(as_i32(f + 1.0), 0, n-1);
 *       periodic axis, n texels per period with centres at (i + 0.5) / n:
 *         x = a * (double)n - 0.5, f = floor(x), t = x - f, i0 = emod(as_i32(f), n) with emod(k, n) = ((k % n) + n) % n in i32,
 *         i1 = (i0 + 1 == n) ? 0 : i0 + 1;
 *       either: a NaN t (a NaN or infinite a) becomes 0.0.  So t is in [0, 1], and every lookup stays in bounds, NaN and +-inf included.
 *     Colour, per channel, with c[col][row] the four texels and tx, ty the two axes' t:
 *       top = c[x0][y0] + (c[x1][y0] - c[x0][y0]) * tx, bot = c[x0][y1] + (c[x1][y1] - c[x0][y1]) * tx, out = top + (bot - top) * ty
 *     -- the lerp of the Gradient mixture.  Four equal texels give that texel's bits whatever tx and ty are; a clamped axis at an
 *     integer x gives RTC_UV_IMAGE's texel.
 *     Not covered: mip-mapping and any minification filter, a per-record wrap choice beyond these three kinds, mirrored wrap,
 *     filtering of RTC_UV_CHECKERS, height-map bumps (rtc_bump).
 * Textures are `height` rows of `width` f64 RGB triples, copied at scene creation; one texture may back any number of records and
 * is uploaded once per device.
 * Limits: RTC_ERR_INVALID for a UV node without records (always so in a plain rtc_scene_create descriptor), a cube map whose
 * left + 6 exceeds the record count, an unknown map or record kind, a child or texture index out of range, a checkers width or
 * height that is not finite and > 0, a texture of width or height 0 or with NULL rgb, a cycle through UV children;
 * RTC_ERR_UNSUPPORTED for a texture side above RTC_TEXTURE_MAX_SIDE or more than RTC_TEXTURE_MAX_TEXELS texels in one scene. */
enum { RTC_PAT_UV = 4 };
enum { RTC_UVMAP_PLANAR = 0, RTC_UVMAP_SPHERICAL = 1, RTC_UVMAP_CYLINDRICAL = 2, RTC_UVMAP_CUBE = 3 };
enum { RTC_UV_CHECKERS = 0, RTC_UV_ALIGN_CHECK = 1, RTC_UV_IMAGE = 2 };
enum { RTC_UV_IMAGE_LINEAR = 3,         /* bilinear, both axes clamped            (cube-map faces, decals)        */
       RTC_UV_IMAGE_LINEAR_WRAP_U = 4,  /* bilinear, u periodic, v clamped        (spherical maps)                */
       RTC_UV_IMAGE_LINEAR_WRAP = 5 };  /* bilinear, both axes periodic           (planar, cylindrical maps)      */
#define RTC_TEXTURE_MAX_SIDE 16384
#define RTC_TEXTURE_MAX_TEXELS (1ull << 26)
typedef struct rtc_uv_pattern {
  int32_t kind;          /* RTC_UV_* */
  int32_t texture;       /* RTC_UV_IMAGE*: index into the ext's textures */
  double width, height;  /* RTC_UV_CHECKERS: squares along u and v */
  int32_t child[5];      /* CHECKERS: the two colours; ALIGN_CHECK: main, ul, ur, bl, br */
  int32_t _pad;
} rtc_uv_pattern;
typedef struct rtc_texture {
  uint32_t width, height;
  const double* rgb;     /* height rows of width {r, g, b}, row 0 at the top */
} rtc_texture;
/* What rtc_scene_create_ext adds to a descriptor.  n_lights == 0: the lights are desc->lights (rtc_scene_create's rule); otherwise
 * `lights` replace them under rtc_scene_create_ex's rule (desc->n_lights must be 0). */
typedef struct rtc_scene_ext {
  uint32_t n_lights;
  const rtc_light_ex* lights;
  uint32_t n_uv_patterns;
  const rtc_uv_pattern* uv_patterns;
  uint32_t n_textures;
  const rtc_texture* textures;
} rtc_scene_ext;

/* Spot lights (not in the reference; the light kind the book's readers build next): a cone with a smooth edge on one light of the
 * scene's list, point or area, for rtc_scene_create_ext2 / rtc_multi_create_ext2.  `light` indexes the scene's light list, `axis` is
 * the direction the light points in (any length), cos_inner / cos_outer are the cosines of the two half-angles: inside the inner cone
 * the light is full, outside the outer one it is dark.  Cosines, not angles: no cos of any maths library enters the rule.  Every step is
 * one f64 operation, in the order written here (csrc/spot_factor.h, one function for device and host).
 *   At scene creation: m = sqrt((ax*ax + ay*ay) + az*az), a = axis / m componentwise (Vector::normalize's order).
 *   For a sample at p_k (rtc_light_ex; a point light: its origin) and a shading point o = the over_point, the shadow rays' origin:
 *     d  = the shadow ray's direction (World::is_shadowed, src/world.rs:139-143): v = p_k - o, dist = sqrt(vx*vx + vy*vy + vz*vz),
 *          d = v / dist componentwise;
 *     c  = ((-dx)*ax + (-dy)*ay) + (-dz)*az;
 *     f  = 1.0 if c >= cos_inner; else 0.0 if c <= cos_outer; else t = (c - cos_outer) / (cos_inner - cos_outer),
 *          f = (t * t) * (3.0 - 2.0 * t).  The tests run in that order: cos_inner == cos_outer is a hard edge and never divides by
 *          zero.  A NaN c fails both tests: t and f are NaN and poison the sample.
 *     f == 0.0: the sample adds nothing, no shadow ray is traced and rtc_stats.rays_shadow does not count it.
 *     Otherwise the sample is exactly the reference's point-light term for a light at p_k of intensity I[ch] * f, one multiplication per
 *     channel; I is the light's intensity, of an area light already divided by N.  x * 1.0 is exact: a sample inside the inner cone
 *     has an ordinary light's bits, and so has every sample of an open cone, cos_inner = cos_outer = -1 (|c| <= 1 holds whenever the
 *     axis has one non-zero component; for a general axis c can fall one rounding below -1 where d is exactly opposite to it).
 *     The one-kernel path's shortcut for a light behind the surface (ambient term only) uses the scaled intensity as well.
 *   A light with a cone is still ONE light: L = n_lights and the once-per-light reflected and refracted colour do not change, whatever
 *   f is.  A point light with a cone keeps its light grid.
 * Limits: RTC_ERR_INVALID for a `light` index out of range, two cones on one light, an axis that is zero or not finite (or whose length
 * is, in f64), cosines not finite or outside [-1, 1], cos_outer > cos_inner, n_cones > 0 with NULL cones.
 * Not covered: distance attenuation, textured (gobo) lights, more than one cone per light. */
typedef struct rtc_light_cone {
  uint32_t light;     /* index into the scene's light list */
  uint32_t _pad;
  double axis[3];     /* where the light points; normalised at scene creation */
  double cos_inner;   /* cosine of the half-angle inside which the light is full */
  double cos_outer;   /* cosine of the half-angle outside which it is dark; <= cos_inner */
} rtc_light_cone;

/* The scene's background (not in the reference, where a ray that leaves the scene is Color::BLACK): what a ray that hits nothing sees --
 * a pattern, a UV map or a skybox --, for rtc_scene_create_ext3 / rtc_multi_create_ext3.  A background belongs to the world, not to its
 * geometry: no dome is intersected, no bound grows.
 *   `pattern` is the index of a root node in the scene's pattern-node array.  It may be any tag, RTC_PAT_UV included.
 *   `projection` is one of:
 *     RTC_BG_DIRECTION: the point is (dx, dy, dz, 1.0), the ray's direction as it is, with no normalisation.
 *     RTC_BG_CUBE:      c = max(|dx|, |dy|, |dz|), with the NaN-skipping max that the CUBE uv map uses.  The point is
 *                       (dx / c, dy / c, dz / c, 1.0), three divisions.  The direction lands on the unit cube's surface, where
 *                       RTC_UVMAP_CUBE expects its point.  This is a skybox.
 *     (csrc/background_point.h, one function for device and host.)
 *   For a ray of the ray tree, camera ray or child ray, whose closest-hit pass finds nothing:
 *     B = the pattern's colour at that point.  Root-level transform_inv matrices apply as ever, and w = 1.0, so translations count.
 *     The ray contributes weight * B[ch] per channel, one multiplication each.
 *     `weight` is the path weight the ray already carries: 1.0 at level 0, and child_rays()' wr / wt below that (the reflective or
 *     transparency factors down the path, each times L = n_lights, as for a hit's surface colour).
 *     The contribution is added at the place in the one-kernel path's depth-first order where a hit's surface colour would have been
 *     added.  Both device paths give the same bits.
 *   A background traces no ray and changes no hit; changes no hit-tree digest; is not a light: no ambient term, no factor per light of
 *   its own, and shadow rays never see it; changes none of rtc_stats' counters (n_launches counts the wavefront path's extra kernel,
 *   one per level).  A scene without lights still shows its background to the camera rays (fuel is 0 there, as ever).
 *   A scene without a background is exactly today's scene: the same kernels, the same builds, the same kernel arguments.
 * Which kernels: on the wavefront path every existing kernel runs as it does without the background, and wf_background
 * (csrc/rtc_background.hip) runs once per level behind that level's closest-hit pass.  On the one-kernel path a background scene takes
 * the BG build of the general kernel that reads the program from memory (feature level 3) with the scene's own area / uv / spot flags:
 * there is no LEAN, 3-wave or kernel-argument one-kernel build for background scenes.  rtc_scene_kernel_info describes the scene as it
 * would run without its background (on path 4 that is what runs); rtc_scene_background_info says what the background adds or replaces.
 * Limits: RTC_ERR_INVALID for a pattern index out of range, an unknown projection, or a NULL where a background is announced
 * (rtc_background_point, rtc_background_colors, rtc_scene_background_info); checked before anything else, a device included.  The
 * pattern tree's own limits apply as they do for a material: RTC_MAX_PATTERN_DEPTH, UV records, textures.
 * Not covered: importance-sampled environment lighting; a background that only the camera sees; a per-channel or per-level tint;
 * mip-mapped (minified) texture lookups -- a skybox magnifies, and RTC_UV_IMAGE_LINEAR covers that. */
enum { RTC_BG_DIRECTION = 0, RTC_BG_CUBE = 1 };
typedef struct rtc_background {
  int32_t pattern;     /* index of a root rtc_pattern_node */
  int32_t projection;  /* RTC_BG_* */
} rtc_background;

/* Normal perturbation (the book's "next steps"; not in the reference, whose surfaces are as smooth as their geometry): bump records for
 * rtc_scene_create_ext4 / rtc_multi_create_ext4.  A record belongs to a material; at most one record per material.  A hit on a
 * primitive whose material has a record is shaded with a perturbed normal ns in place of the geometric normal.  The inputs are
 *   X, the hit point ray.position(t);  n, the unit world normal of Shape::normal BEFORE the inside flip;  m, the primitive's
 *   material_inv;  a = amplitude, f = frequency.
 * Every step is one f64 operation in the order written (csrc/bump_normal.h, one function for device and host, -ffp-contract=off).
 *   1. q = rows 0..2 of m applied to (X, 1.0), each row as m[0]*x + m[1]*y + m[2]*z + m[3]*1.0 left to right (as for a pattern's
 *      point); s = q * f componentwise.
 *   2. d by kind:
 *        RTC_BUMP_SIMPLEX: d = (simplex(sx,sy,sz), simplex(sx,sy,sz+1.0), simplex(sx,sy,sz+2.0)): the offsets of a point jitter.
 *        RTC_BUMP_FRACTAL: the same with fractal(.., octaves).
 *        RTC_BUMP_RIPPLE:  rings about the material-space y axis with a triangle wave as the slope (no libm function enters):
 *          r = sqrt(sx*sx + sz*sz);  r == 0.0: d = (0, 0, 0);  otherwise g = 2.0 * (r - floor(r)),
 *          w = (g < 1.0) ? 1.0 - 2.0*g : 2.0*g - 3.0,  d = ((sx / r) * w, 0.0, (sz / r) * w).
 *   3. To world space the way a gradient transforms, by the transpose of the 3x3:
 *        gx = (m[0]*dx + m[4]*dy) + m[8]*dz;  gy = (m[1]*dx + m[5]*dy) + m[9]*dz;  gz = (m[2]*dx + m[6]*dy) + m[10]*dz.
 *   4. v = n + a * g componentwise.  vx == nx && vy == ny && vz == nz: ns = n, with its bits and no renormalisation (amplitude 0 is
 *      exactly the scene without the record).  Otherwise mag = sqrt(vx*vx + vy*vy + vz*vz), ns = v / mag.
 *   5. Where prepare_state flips the geometric normal (n . eye < 0), ns is negated too: the bumps are one field on the surface, seen
 *      from either side.
 *   6. over_point and under_point keep using the flipped GEOMETRIC normal: their bits, the shadow rays' origins and the pattern colour
 *      do not move.
 *   7. The state's normal is ns, and reflect = direction - ns * (2 * direction.dot(ns)) by the usual expression.  Everything that reads
 *      the state's normal reads ns: the Phong terms, the light-behind-the-surface test, schlick, the blend of a glass mirror, and the
 *      reflected and refracted rays.  Both device paths give the same bits.
 * A scene without a record is exactly today's scene: the same kernels, the same builds, the same kernel arguments.
 * Which kernels: on the one-kernel path a bumped scene takes the NP build of the general kernel that reads the program from memory
 * (feature level 3) with the scene's own area / uv / spot / background flags (rtc_bump_info.trace_build numbers them); there is no
 * LEAN, 3-wave or kernel-argument build for it.  On the wavefront path wf_shade's NP build (COUNT x UV) shades every level; wf_ts,
 * wf_gather and wf_background run as they do without.  rtc_scene_kernel_info describes the scene as it would run without its records;
 * rtc_scene_bump_info says what they replace.
 * Limits: RTC_ERR_INVALID for a material index out of range, two records on one material, an unknown kind, an amplitude that is not
 * finite, a frequency that is not finite or <= 0, FRACTAL with octaves == 0 or above RTC_BUMP_MAX_OCTAVES, and n_bumps > 0 with NULL
 * bumps; checked before anything else, a device included.  (A pattern node's octaves have no limit beyond their 32 bits; a record's are
 * capped because every hit pays three noise evaluations per octave, and octave 54 and later add less than one ulp of the sum.)
 * Not covered: a shading normal that faces away from the eye or below the geometric surface is not clamped, so a reflected ray may
 * re-enter its own surface; height maps taken from patterns or images (the filtered lookups they need exist now,
 * RTC_UV_IMAGE_LINEAR*; the bump kind that reads them does not); a transform of the record's own; distance-dependent amplitude. */
enum { RTC_BUMP_SIMPLEX = 0, RTC_BUMP_FRACTAL = 1, RTC_BUMP_RIPPLE = 2 };
#define RTC_BUMP_MAX_OCTAVES 64
typedef struct rtc_bump {
  uint32_t material;   /* index into desc->materials; at most one record per material */
  int32_t  kind;       /* RTC_BUMP_* */
  uint32_t octaves;    /* FRACTAL only */
  uint32_t _pad;
  double amplitude;    /* a */
  double frequency;    /* f */
} rtc_bump;

/* The sampled camera (not in the reference, whose Camera::ray_at_pixel sends one ray through each pixel centre from a pinhole): n x n
 * samples per pixel (anti-aliasing, box filter) and an optional thin lens (depth of field), for the rtc_render_sampled* entry points
 * and rtc_camera_rays.  Pixel i has x = i % hsize, y = i / hsize; sample k of its N = n * n has sx = k % n, sy = k / n.  Every step is
 * one f64 operation; m = SplitMix64's finaliser (rtc_splitmix64, csrc/device_scene.h), rtc_area_jitter as for rtc_light_ex.
 *   h = m(m(m(seed) ^ i) ^ k), draw(j) = rtc_area_jitter(h, j) = (m(h ^ j) >> 11) * 2^-53.  Nothing of the launch, chunk, device or
 *     device path enters: any partition of the image gives the same bits.
 *   Sub-pixel position: without RTC_SAMPLE_JITTER jx = jy = 0.5; with it jx = draw(0), jy = draw(1) (stratified: one sample per cell).
 *     fx = ((double)sx + jx) / (double)n, fy likewise; xoffset = ((double)x + fx) * pixel_size, yoffset likewise;
 *     world_x = half_width - xoffset, world_y = half_height - yoffset.
 *   lens_radius R == 0 (pinhole): the rest is Camera::ray_at_pixel's (src/camera.rs:46-54) on world_x, world_y.  side = 1 without
 *     jitter is therefore exactly rtc_render's ray (0.5 / 1.0 = 0.5).
 *   R > 0 (thin lens): a = 2.0 * draw(2) - 1.0, b = 2.0 * draw(3) - 1.0 (hashed whether or not RTC_SAMPLE_JITTER is set); concentric
 *     map: a == 0 && b == 0 gives lx = ly = 0; else if fabs(a) > fabs(b): r = a, phi = (M_PI / 4.0) * (b / a); else r = b,
 *     phi = M_PI / 2.0 - (M_PI / 4.0) * (a / b); lx = (R * r) * cos(phi), ly = (R * r) * sin(phi).  Origin = rows 0-2 of transform_inv
 *     applied to (lx, ly, 0, 1), target = the same rows applied to (world_x * F, world_y * F, -F, 1), F = focal_distance, each row as
 *     m[0]*px + m[1]*py + m[2]*pz + m[3]*1.0 left to right; direction = (target - origin) normalised as ray_at_pixel normalises.
 *   Pixel colour: (((c_0 + c_1) + c_2) + ... + c_{N-1}) / (double)N per channel, c_k = World::color_at(ray_k, fuel).
 * Limits: RTC_ERR_INVALID for side == 0, unknown flag bits, R negative or not finite, R > 0 with F not finite or <= 0, NULL
 * arguments; RTC_ERR_UNSUPPORTED for side > RTC_SAMPLES_MAX_SIDE. */
enum { RTC_SAMPLE_JITTER = 1u };
#define RTC_SAMPLES_MAX_SIDE 16
typedef struct rtc_sampling {
  uint32_t side;          /* n: n x n samples per pixel, N = n*n */
  uint32_t flags;         /* RTC_SAMPLE_JITTER */
  uint64_t seed;
  double lens_radius;     /* R; 0 = pinhole */
  double focal_distance;  /* F, camera-space depth that is in focus; read only when R > 0 */
} rtc_sampling;

/* Adaptive sampling (not in the reference): render the frame once with `base`, find the pixels that differ from a neighbour, render
 * those again with `fine`; for rtc_render_adaptive* and, the contrast rule alone, rtc_contrast_pixels.  Pixel i has x = i % hsize,
 * y = i / hsize; every step is one f64 operation or comparison (csrc/adaptive_contrast.h, one function for device and host).
 *   Base frame: B[i] = rtc_render_sampled's pixel i with `base`, for every pixel of the frame.
 *   Contrast: q(c) = c < 0 ? 0 : (c > 1 ? 1 : c) per channel value -- what a viewer sees after Color::clamp; NaN passes through.  The
 *     neighbours of p = (x, y) are (x-1, y), (x+1, y), (x, y-1), (x, y+1) and, with neighbours == 8, the four diagonals; only those inside
 *     the image count.  For a neighbour r: d = fabs(q(B[p][0]) - q(B[r][0])), then for c = 1, 2: e = fabs(q(B[p][c]) - q(B[r][c])),
 *     d = (e > d) ? e : d -- so a NaN in the first channel stays (d is NaN), a NaN in a later channel is skipped.
 *   p is REFINED iff some neighbour has !(d <= threshold).  d is symmetric in p and r: both sides of an edge refine.  A NaN d refines at
 *     any threshold; threshold = +inf refines nothing else; a negative threshold refines every pixel that has a neighbour (every pixel
 *     of a frame larger than 1x1); a 1x1 frame refines nothing.
 *   Result: a refined pixel is exactly rtc_render_sampled's pixel with `fine` (the base sample is not blended in), any other pixel is
 *     B[i]: every pixel of the result is, bit for bit, a pixel of one of two rtc_render_sampled frames.
 * Limits: `base` and `fine` as rtc_sampling's; RTC_ERR_INVALID for a NaN threshold, neighbours other than 4 or 8, NULL arguments;
 * RTC_ERR_UNSUPPORTED for a frame of 2^39 pixels or more.
 * Not covered: bands, rtc_render_multi and several devices (a band's edge rows need neighbours another device owns); a measured device
 * path for the refined list; filters other than the box mean; refining the refined pixels again. */
typedef struct rtc_adaptive {
  rtc_sampling base;      /* first pass: every pixel */
  rtc_sampling fine;      /* second pass: the refined pixels */
  double threshold;
  uint32_t neighbours;    /* 4 or 8 */
  uint32_t _pad;
} rtc_adaptive;

/* Pixel reconstruction filters (not in the reference) for the sampled camera: a pixel is the weighted mean of the samples of every
 * pixel within `radius` of its centre, for the rtc_render_filtered* entry points and, the filter step alone, rtc_filter_frame.  `radius`
 * is in pixels, measured from the pixel centre per axis; the filter is separable.  Every step is one f64 operation, in the order written
 * here (csrc/filter_weights.h, one function for device and host); only exp of the Gaussian comes from different libraries on the two sides.
 *   Sample position: sample k of image pixel q = (qx, qy) sits at the sub-pixel position (fx, fy) of rtc_sampling above (same hash, same
 *     jx / jy; 0.5 without RTC_SAMPLE_JITTER).  The lens draws do not enter.
 *   Window: W = (uint32_t)ceil(radius - 0.5).  The window of output pixel p = (x, y) is the pixels q with |qx - x| <= W and |qy - y| <= W;
 *     only those inside the image count.
 *   Weight of sample (q, k) for p: dx = (double)((int64_t)qx - (int64_t)x) + (fx - 0.5), dy likewise; w = f(dx) * f(dy).  In f,
 *     a = fabs(d) and r = radius; f = 0.0 unless a < r, else
 *       BOX       1.0
 *       TENT      1.0 - a / r
 *       GAUSSIAN  exp(-alpha * a * a) - exp(-alpha * r * r), each product left to right
 *       MITCHELL  (B = C = 1/3; alpha is ignored) t = (a + a) / r;
 *                 t < 1.0:  ((((7.0 * t - 12.0) * t) * t) + 16.0 / 3.0) / 6.0
 *                 else:     ((((-7.0 / 3.0) * t + 12.0) * t - 20.0) * t + 32.0 / 3.0) / 6.0
 *   Pixel value: num[c] = 0.0, den = 0.0; loop qy ascending (outer), qx ascending, k ascending (inner); a sample with w == 0.0 is skipped
 *     (a NaN or infinite colour outside the support cannot reach the pixel); otherwise num[c] = num[c] + w * colour_k(q)[c] and
 *     den = den + w.  The pixel is num[c] / den; a zero den gives what IEEE gives.
 *   Identity: BOX with radius 0.5 has W = 0 and every weight 1.0, den is N exactly, and the pixel is rtc_render_sampled's bit for bit --
 *     unless a jitter draw is exactly 0 (probability 2^-53 per draw): that sample sits on the pixel's edge, a == r, and is skipped.
 * Limits: RTC_ERR_INVALID for NULL arguments, an unknown kind, radius not finite or < 0.5, GAUSSIAN with alpha not finite or <= 0, a row
 * range outside the image or empty; RTC_ERR_UNSUPPORTED for radius > RTC_FILTER_MAX_RADIUS.  rtc_sampling's own limits apply as ever.
 * Not covered: pixel lists; bands, rtc_render_multi and several devices; filtering rtc_render_adaptive's refine pass; filters given as
 * tables; a radial (non-separable) support. */
enum { RTC_FILTER_BOX = 0, RTC_FILTER_TENT = 1, RTC_FILTER_GAUSSIAN = 2, RTC_FILTER_MITCHELL = 3 };
#define RTC_FILTER_MAX_RADIUS 3.0
typedef struct rtc_filter {
  int32_t kind;           /* RTC_FILTER_* */
  uint32_t _pad;
  double radius;          /* r, in pixels from the pixel centre, per axis */
  double alpha;           /* GAUSSIAN's falloff; read by no other kind */
} rtc_filter;

/* The shutter (not in the reference, whose frame sees one scene from one camera): motion blur over K poses of the scene and the camera,
 * the accumulation-buffer way, for the rtc_render_shutter* entry points and, the dealing alone, rtc_shutter_deal.  The caller supplies K
 * poses; pose p of K has scenes[p] and cameras[p] (the pointers may repeat: a moving camera over a static scene passes one scene K
 * times).  Every sample of every pixel is dealt to ONE pose and traced there; the pixel stays the mean of its N samples (a box shutter).
 * All cameras share hsize and vsize; transform_inv, half_width, half_height and pixel_size may differ from pose to pose.
 *   Pixel i, sample k of N = side * side, h = m(m(m(seed) ^ i) ^ k) and rtc_area_jitter are rtc_sampling's above.
 *   Pose s of sample (i, k) (csrc/shutter_pose.h, one function for device and host):
 *     without RTC_SHUTTER_HASHED: s = (uint32_t)(((uint64_t)k * K) / N) -- sequential: the pixel's samples in K runs of floor(N / K) or
 *       ceil(N / K); K > N is refused, some poses would never be sampled.
 *     with RTC_SHUTTER_HASHED: u = rtc_area_jitter(h, 4u), the draw after the lens's two; t = u * (double)K; s = (uint32_t)t, held to
 *       K - 1.  Hashed whether or not RTC_SAMPLE_JITTER is set, as the lens draws are.  Nothing of the launch, chunk, device or device
 *       path enters.
 *   Ray of sample (i, k): rtc_sampling's ray of (i, k) through cameras[s], unchanged, lens included.
 *   Colour: c_k = World::color_at(that ray, fuel) in scenes[s].
 *   Pixel colour: (((c_0 + c_1) + c_2) + ... + c_{N-1}) / (double)N per channel, k ascending: rtc_render_sampled's sum.
 *   Identities: K = 1 is rtc_render_sampled bit for bit; so are K equal poses under either flag -- the same pointers repeated, or equal
 *     scenes created twice.
 * Limits: RTC_ERR_INVALID for K == 0, NULL arrays or entries, unknown flag bits, cameras whose hsize or vsize differ, scenes on different
 * devices, K > N without RTC_SHUTTER_HASHED, and everything rtc_sampling refuses; RTC_ERR_UNSUPPORTED for K > RTC_SHUTTER_MAX_POSES.  The
 * shutter's own numbers are checked before anything else, a device included.
 * Not covered: bands, rtc_render_rows_device and rtc_multi; adaptive and filtered renders; hit records and digests; a time stratified
 * jointly with the sub-pixel cell; interpolated transforms inside one scene; shutters other than the box. */
enum { RTC_SHUTTER_HASHED = 1u };
#define RTC_SHUTTER_MAX_POSES 64
typedef struct rtc_shutter {
  uint32_t flags;         /* RTC_SHUTTER_HASHED */
  uint32_t _pad;
} rtc_shutter;

/* The Element tree (src/shape.rs:31-34, :181-185) in DFS pre-order.  A group node carries the world-space
 * bounding box the reference computed for it (Element::composite + propagate_inverses; NaN/inf included,
 * SURVEY Q9) and `skip` = index of the first node after its subtree.  The device evaluates
 * BoundingBox::intersects (src/bounding_box.rs:80-92) on exactly these numbers. */
enum { RTC_NODE_PRIM = -1, RTC_NODE_UNION = 0, RTC_NODE_INTERSECTION = 1, RTC_NODE_DIFFERENCE = 2, RTC_NODE_AGGREGATION = 3 };
typedef struct rtc_node {
  int32_t kind; /* RTC_NODE_* */
  int32_t ref;  /* RTC_NODE_PRIM: primitive index; groups: unused */
  int32_t skip; /* groups: one past the subtree; primitives: own index + 1 */
  int32_t _pad;
  double bbox_min[3]; /* groups only */
  double bbox_max[3];
} rtc_node;

typedef struct rtc_scene_desc {
  uint32_t n_nodes;  const rtc_node* nodes;
  uint32_t n_prims;  const rtc_prim* prims;
  uint32_t n_xforms; const rtc_xform* xforms;
  uint32_t n_limits; const double* limits;          /* n x {min, max}              (Geometry::Cylinder/Cone) */
  uint32_t n_tris;   const double* tri_p1e1e2;      /* n x {p1, e1, e2} xyz        (src/shape.rs:369-412)    */
                     const double* tri_normals;     /* n x {n1, n2, n3} xyz; flat triangles: {n, -, -}       */
  uint32_t n_materials;     const rtc_material* materials;
  uint32_t n_pattern_nodes; const rtc_pattern_node* pattern_nodes;
  uint32_t n_lights;        const rtc_light* lights;
} rtc_scene_desc;

/* Camera (src/camera.rs:5-13) with its derived fields as Camera::new computes them (:16-37). */
typedef struct rtc_camera {
  uint64_t hsize, vsize;
  double half_width, half_height, pixel_size;
  double transform_inv[16];
} rtc_camera;

/* Parity channel: the nearest hit of a primary ray (t bit-exact; prim = sequence number or -1). */
typedef struct rtc_hit {
  double t;
  int32_t prim;
  int32_t push_idx;
} rtc_hit;

/* Work counters of one render call (deterministic for a given scene + accelerator).  The *_kernarg counters say how many of
 * the nodes / tests read their record from the kernel arguments (scalar loads): those move no bytes through the memory
 * system and are excluded from bench.py's algorithmic-byte figure. */
typedef struct rtc_stats {
  uint64_t pixels;
  uint64_t rays_primary, rays_shadow, rays_reflect, rays_refract; /* unique rays, SURVEY.md §8d */
  uint64_t rays_container;   /* hits whose n1 / n2 (src/intersection.rs:70-103) reach a result: the material has
                                transparency != 0.0, World::shade_hit gets fuel > 0 and the world has a light (src/world.rs:70-78,
                                :110) -- one extra pass over the hit's ray each; not counted as rays                            */
  uint64_t accel_nodes;      /* accelerator BVH nodes visited (4-wide nodes, 128 B each)                  */
  uint64_t group_tests;      /* reference group boxes tested (BoundingBox::intersects; 48 B each)         */
  uint64_t tri_tests;        /* triangles tested (72 B each)                                              */
  uint64_t analytic_tests;   /* analytic primitives tested (one 128-B intersection record each)           */
  uint64_t nan_ts;           /* passes with a NaN t in a list of >= 2 since the last check (-> RTC_ERR_NAN) */
  double kernel_ms;          /* device time of the trace kernel(s), HIP events on the scene's stream */
  uint32_t n_launches;
  uint32_t _pad;
  uint64_t accel_nodes_kernarg;    /* of accel_nodes: root nodes read from the kernel arguments           */
  uint64_t analytic_tests_kernarg; /* of analytic_tests: plane records read from the kernel arguments     */
  uint64_t light_grid_cells;       /* light-grid cells looked up by shadow rays, each instead of a BVH walk (8 B of
                                      offsets + 4 B per candidate)                                         */
  uint64_t group_tests_uniform;    /* of group_tests: gates of whole meshes named by a kernel-argument program: every lane of
                                      the wave reads the SAME box (scalar loads of one address), so like the other
                                      *_kernarg records they move no bytes through the vector memory system */
} rtc_stats;

const char* rtc_last_error(void);
/* Number of HIP devices visible (0 = none; never initialises a context). */
int rtc_device_count(void);

/* Flatten-once upload: validates, builds the results-neutral accelerator (BVH over each group's bounded
 * primitive children) and copies SoA buffers to HBM on `device`. */
int rtc_scene_create(const rtc_scene_desc* desc, int device, rtc_scene** out);
/* Same, with the scene's lights given as n rtc_light_ex records (point and area lights in any order; the order is the scene's light
 * order) in place of desc->lights: desc->n_lights must be 0 (RTC_ERR_INVALID otherwise).  A scene whose list holds point lights only
 * is exactly the rtc_scene_create scene (same kernels, same bits); one with an area light renders with kernel instantiations of its
 * own on both device paths.  Every render entry point takes either. */
int rtc_scene_create_ex(const rtc_scene_desc* desc, const rtc_light_ex* lights, uint32_t n_lights, int device, rtc_scene** out);
/* Same, with the extensions of rtc_scene_ext: lights (rtc_scene_create_ex's rule when ext->n_lights > 0), UV pattern records and
 * textures for RTC_PAT_UV nodes.  An ext of NULL, or one with lights only, is exactly rtc_scene_create / rtc_scene_create_ex (same
 * kernels, same bits); a scene with a UV node renders with kernel instantiations of its own on both device paths.  Every render
 * entry point takes the result. */
int rtc_scene_create_ext(const rtc_scene_desc* desc, const rtc_scene_ext* ext, int device, rtc_scene** out);
/* Same, with n_cones light cones (rtc_light_cone above; `light` indexes ext->lights, or desc->lights when ext is NULL or has none).
 * Zero cones is exactly rtc_scene_create_ext (same kernels, same bits); a scene with a cone renders with kernel instantiations of its
 * own on both device paths, whether or not it has an area light.  The cones' own numbers are checked before anything else, a device
 * included.  Every render entry point takes the result. */
int rtc_scene_create_ext2(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, int device, rtc_scene** out);
/* Same, with a background (rtc_background above).  bg == NULL is exactly rtc_scene_create_ext2 (same kernels, same bits).  The
 * background's own numbers are checked before anything else, a device included.  Every render entry point takes the result. */
int rtc_scene_create_ext3(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg, int device,
                          rtc_scene** out);
/* The projection rule alone: point = where a ray of direction dir looks the background up.  Host-only: no device needed (like
 * rtc_spot_factor).  RTC_ERR_INVALID for NULL arguments or an unknown projection. */
int rtc_background_point(int32_t projection, const double dir[3], double point[3]);
/* The whole rule on the device for n directions (dirs: n x {x, y, z}, rgb: n x 3, both host): rgb[i] = B of a ray with direction
 * dirs[i] -- to a background what rtc_camera_rays is to the camera.  RTC_ERR_INVALID for a scene without a background. */
int rtc_background_colors(rtc_scene*, const double* dirs, uint64_t n, double* rgb);
/* Test hook, read-only: what a launch of this scene takes for its background.  has_background == 0: pattern, projection and the
 * builds are -1.  trace_build: path 1, the general kernel (feature level 3, program read from memory) whose BG instantiation of
 * rtc_trace_kernel replaces the build rtc_scene_kernel_info reports, numbered by the scene's flags -- 0 none, 1 area lights, 2 UV patterns,
 * 3 area + UV, 4 light cones, 5 cones + UV (a cone always comes with the area code path) -- which trace_area / trace_uv / trace_spot
 * repeat; wf_background_build: path 4, RTC_WF_BG_*. */
enum { RTC_WF_BG_PLAIN = 0, RTC_WF_BG_UV = 1 };
typedef struct rtc_background_info {
  int32_t has_background;
  int32_t pattern, projection;
  int32_t plain_root;           /* the root is a Plain colour: no pattern walk, no projection */
  int32_t trace_build;          /* path 1: 0..5 by the scene's flags, as above (feature level 3, program read from memory) */
  int32_t trace_area, trace_uv, trace_spot;  /* ... and its flags */
  int32_t wf_background_build;  /* path 4: RTC_WF_BG_PLAIN (pattern_color) or RTC_WF_BG_UV (pattern_color_uv, scenes with a UV node) */
  int32_t _pad;
} rtc_background_info;
int rtc_scene_background_info(const rtc_scene*, rtc_background_info* out);
/* Same, with n_bumps bump records (rtc_bump above).  n_bumps == 0 is exactly rtc_scene_create_ext3 (same kernels, same bits).  The
 * records' own numbers are checked before anything else, a device included.  Every render entry point takes the result. */
int rtc_scene_create_ext4(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg,
                          const rtc_bump* bumps, uint32_t n_bumps, int device, rtc_scene** out);
/* Steps 1-4 of the rule alone: out = the shading normal of a hit at `point` whose unit normal is `normal`, on a primitive whose
 * material_inv is the row-major 4x4 `material_inv`; bump->material is not read.  Host-only: no device needed (like rtc_spot_factor).
 * RTC_ERR_INVALID for NULL arguments and for a record rtc_scene_create_ext4 would refuse. */
int rtc_bump_normal(const rtc_bump* bump, const double material_inv[16], const double point[3], const double normal[3], double out[3]);
/* The same steps on the device for n items (prims: n primitive indices; points, normals, out: n x {x, y, z}; all host): the record and
 * the matrix come from the scene's tables by primitive index, and a primitive whose material has no record gets its normal back -- to
 * a bump what rtc_background_colors is to the background.  RTC_ERR_INVALID for a primitive index out of range. */
int rtc_bump_normals(rtc_scene*, const int32_t* prims, const double* points, const double* normals, uint64_t n, double* out);
/* Test hook, read-only: what a launch of this scene takes for its bump records.  has_bump == 0: the builds are -1.  trace_build: path 1,
 * the general kernel whose NP instantiation of rtc_trace_kernel replaces the build rtc_scene_kernel_info (or rtc_scene_background_info)
 * reports: rtc_background_info.trace_build's 0..5 by the scene's area / uv / spot flags, and 6 more (6..11) for a scene that has a
 * background too; trace_area / trace_uv / trace_spot / trace_bg repeat the flags; wf_shade_build: path 4, RTC_WF_NP_*, for every level. */
enum { RTC_WF_NP_PLAIN = 0, RTC_WF_NP_UV = 1 };
typedef struct rtc_bump_info {
  int32_t has_bump;
  uint32_t n_bumps;
  int32_t trace_build;          /* path 1: 0..5 by the scene's flags, + 6 with a background (feature level 3, program read from memory) */
  int32_t trace_area, trace_uv, trace_spot, trace_bg;  /* ... and its flags */
  int32_t wf_shade_build;       /* path 4: RTC_WF_NP_PLAIN or RTC_WF_NP_UV (scenes with a UV node); each has its counting form */
} rtc_bump_info;
int rtc_scene_bump_info(const rtc_scene*, rtc_bump_info* out);
/* The cone factor f alone, for a light (or sample) at light_pos and a shading point `point`; `cone->light` is not read.  Host-only: no
 * device needed (like rtc_ppm).  RTC_ERR_INVALID for NULL arguments and for a cone rtc_scene_create_ext2 would refuse. */
int rtc_spot_factor(const rtc_light_cone* cone, const double light_pos[3], const double point[3], double* f);
/* One image record's colour at (u, v), on the host: rgb = the texel rule of `kind` (RTC_UV_IMAGE, or RTC_UV_IMAGE_LINEAR* through
 * csrc/uv_image.h, the function the kernels compile) on `tex`.  Host-only: no device needed (like rtc_spot_factor).  RTC_ERR_INVALID for
 * NULL arguments, a kind outside RTC_UV_IMAGE .. RTC_UV_IMAGE_LINEAR_WRAP, and a texture rtc_scene_create_ext would refuse (a side of 0
 * or above RTC_TEXTURE_MAX_SIDE, NULL rgb). */
int rtc_texture_sample(const rtc_texture* tex, int32_t kind, double u, double v, double rgb[3]);
void rtc_scene_destroy(rtc_scene*);
/* Size in bytes of the scene's device buffers (accelerator and texels included). */
uint64_t rtc_scene_device_bytes(const rtc_scene*);

/* Image::par_render for pixels i = first .. first+n-1 (row-major: x = i % hsize, y = i / hsize) or, when
 * pixel_indices != NULL, for the n listed indices.  rgb: n*3 doubles (host).  hits, stats: optional. */
int rtc_render(rtc_scene*, const rtc_camera*, int32_t fuel, const uint64_t* pixel_indices, uint64_t first, uint64_t n,
               double* rgb, rtc_hit* hits, rtc_stats* stats);

/* Parity channel beyond the primary hit ("hit indices bit-exact" for the whole ray tree): per pixel, the wrapping 64-bit sum over
 * every ray of its de-duplicated ray tree — the primary ray and every reflected / refracted ray World::color_at spawns, each
 * once (the reference traces them once per light, src/world.rs:58-79) — of hash(t bits, primitive sequence number, push index of
 * the ray's nearest hit; ray depth; ray kind), a miss hashing as (0, -1, 0).  The hash is defined in csrc/device_scene.h
 * (rtc_hit_hash_base / rtc_hit_hash) and restated by the oracle; equal digests mean every closest hit of the pixel's ray tree
 * agrees bit for bit.  Pixels as in rtc_render; digest: n values (host).  Runs the counting kernel variants. */
int rtc_render_hit_digest(rtc_scene*, const rtc_camera*, int32_t fuel, const uint64_t* pixel_indices, uint64_t first, uint64_t n, uint64_t* digest);

/* The whole frame, quantised on the device (Color::clamp, src/color.rs:42-46 — what Image::ppm writes): hsize*vsize*3 bytes
 * (host), row-major; 3 bytes per pixel cross PCIe instead of 24. */
int rtc_render_rgb8(rtc_scene*, const rtc_camera*, int32_t fuel, uint8_t* rgb8, rtc_stats* stats);

/* Host buffers handed to rtc_render / rtc_render_rgb8 / rtc_render_multi* / rtc_trace_rays are written by the device copy
 * directly (one copy per array, queued behind the kernels; hit records are packed on the device); on an error return their
 * contents are unspecified.  RTC_PRETOUCH_THREADS=n (default 0: measured slower than the copy's own page handling) lets n host
 * threads write one byte to each destination page while the device renders. */

/* Same, output left in device memory (rgb_dev: n*3 doubles on the scene's device), for the rows
 * row_first, row_first+row_step, ... (n_rows of them) — the tile-interleaved multi-GPU partition.
 * Asynchronous on the scene's stream unless `sync` != 0.  count_stats != 0 uses the counting kernel variant. */
int rtc_render_rows_device(rtc_scene*, const rtc_camera*, int32_t fuel, uint32_t row_first, uint32_t row_step, uint32_t n_rows,
                           double* rgb_dev, rtc_stats* stats, int count_stats, int sync);

/* The partition the multi-device entries use ("8-row strips"): the image is cut into bands of band_rows rows
 * (the last one may be short) and part band_first of band_step owns bands band_first, band_first + band_step, ...; its dense
 * tile holds them in order.  A wave of the trace kernels is an 8x8 pixel tile of the DENSE tile, so band_rows = 8 keeps it an 8x8
 * tile of the image too (band_rows = 1 is rtc_render_rows_device: at 8 parts one wave's pixels then span 64 image rows).
 * Renders the first n_rows rows of that dense tile (rtc_band_rows_owned() = all of them). */
int rtc_render_bands_device(rtc_scene*, const rtc_camera*, int32_t fuel, uint32_t band_rows, uint32_t band_first, uint32_t band_step,
                            uint32_t n_rows, double* rgb_dev, rtc_stats* stats, int count_stats, int sync);
uint64_t rtc_band_rows_owned(uint64_t vsize, uint32_t band_rows, uint32_t band_first, uint32_t band_step);

/* ---- N GPUs of one process ----------------------------------------------------------------------------------------
 * For the caller of Image::par_render (src/image.rs:65-81) that owns several devices.  An rtc_multi holds one replica of the
 * scene per listed device (a device may be listed more than once — two replicas on one GPU — which is how a one-GPU box
 * exercises the whole path).  rtc_render_multi: replica k traces the bands k, k + n, ... of the image (8 rows each unless
 * rtc_multi_set_band_rows says otherwise; see rtc_render_bands_device) on its own device and stream (no
 * exchange while tracing: pixels are independent, src/image.rs:68-73); the dense tiles are pulled to the FIRST listed device over
 * xGMI (peer copies behind per-replica events), de-interleaved there, and the whole image (hsize*vsize*3 doubles, row-major) is
 * copied to `rgb` (host).  Same pixels, bit for bit, as rtc_render on one device.  stats (optional): counters summed over the
 * replicas (counting kernel variants), kernel_ms = the slowest replica.
 * One process per GPU + RCCL (bench.py, raytracer_challenge_amd/parallel.py) is the other way to use N GPUs; both partition alike. */
typedef struct rtc_multi rtc_multi;
int rtc_multi_create(const rtc_scene_desc* desc, const int* devices, int n_devices, rtc_multi** out);
/* Same with the lights of rtc_scene_create_ex. */
int rtc_multi_create_ex(const rtc_scene_desc* desc, const rtc_light_ex* lights, uint32_t n_lights, const int* devices, int n_devices, rtc_multi** out);
/* Same with the extensions of rtc_scene_create_ext (every replica uploads its own copy of the texels). */
int rtc_multi_create_ext(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const int* devices, int n_devices, rtc_multi** out);
/* Same with the light cones of rtc_scene_create_ext2. */
int rtc_multi_create_ext2(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const int* devices, int n_devices,
                          rtc_multi** out);
/* Same with the background of rtc_scene_create_ext3. */
int rtc_multi_create_ext4(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg,
                          const rtc_bump* bumps, uint32_t n_bumps, const int* devices, int n_devices, rtc_multi** out);  /* with the bump records of rtc_scene_create_ext4 */
int rtc_multi_create_ext3(const rtc_scene_desc* desc, const rtc_scene_ext* ext, const rtc_light_cone* cones, uint32_t n_cones, const rtc_background* bg, const int* devices,
                          int n_devices, rtc_multi** out);
void rtc_multi_destroy(rtc_multi*);
int rtc_multi_device_count(const rtc_multi*);
/* Rows per band of the partition (default 8; 1 = single rows interleaved).  Waits for queued frames. */
int rtc_multi_set_band_rows(rtc_multi*, uint32_t band_rows);
int rtc_render_multi(rtc_multi*, const rtc_camera*, int32_t fuel, double* rgb, rtc_stats* stats);
/* Same, quantised (Color::clamp, src/color.rs:42-46 — what Image::ppm writes): every replica quantises its own rows on its own
 * device, so 3 bytes per pixel cross xGMI instead of 24.  rgb8: hsize*vsize*3 bytes (host), row-major. */
int rtc_render_multi_rgb8(rtc_multi*, const rtc_camera*, int32_t fuel, uint8_t* rgb8, rtc_stats* stats);
/* Same, image left on the first listed device (rgb_dev: hsize*vsize*3 doubles there).  Asynchronous unless sync != 0: queue
 * several frames, then rtc_multi_sync() waits for all replicas and returns (and clears) their error state. */
int rtc_render_multi_device(rtc_multi*, const rtc_camera*, int32_t fuel, double* rgb_dev, int sync);
int rtc_multi_sync(rtc_multi*);

/* World::color_at(ray, fuel) for n rays {ox,oy,oz,dx,dy,dz} (host arrays). */
int rtc_trace_rays(rtc_scene*, const double* rays, uint64_t n, int32_t fuel, double* rgb, rtc_hit* hits, rtc_stats* stats);

/* ---- the sampled camera (rtc_sampling above) ------------------------------------------------------------------------------------
 * rtc_render / rtc_render_rgb8 / rtc_render_bands_device / rtc_render_multi with n x n samples per pixel and an optional thin lens.
 * A device kernel generates the sample rays of a chunk of pixels (at most RTC_SAMPLED_MAX_RAYS rays, an environment variable read at
 * each call, default 2^22; never fewer than one row or one pixel), the scene's ray kernels trace them as explicit rays -- every scene
 * kind, both device paths --, a second kernel averages them into the pixel; chunk after chunk on the scene's stream.  Only pixels
 * leave the device.  Whole-row launches choose their device path as rtc_scene_path_info describes (the launch shape includes the
 * sampling; the guess counts a chunk's rays); pixel lists stay on the one-kernel path.  rtc_stats: pixels = the pixel count,
 * rays_primary = pixels * N, counters summed over the chunks, kernel_ms = generator + traces + resolve.  No hit records or digests:
 * a pixel has N primary hits.  side = 1 without jitter or lens gives rtc_render's pixels bit for bit. */
int rtc_render_sampled(rtc_scene*, const rtc_camera*, const rtc_sampling*, int32_t fuel, const uint64_t* pixel_indices, uint64_t first, uint64_t n,
                       double* rgb, rtc_stats* stats);
int rtc_render_sampled_rgb8(rtc_scene*, const rtc_camera*, const rtc_sampling*, int32_t fuel, uint8_t* rgb8, rtc_stats* stats);
int rtc_render_sampled_bands_device(rtc_scene*, const rtc_camera*, const rtc_sampling*, int32_t fuel, uint32_t band_rows, uint32_t band_first,
                                    uint32_t band_step, uint32_t n_rows, double* rgb_dev, rtc_stats* stats, int count_stats, int sync);
int rtc_render_multi_sampled(rtc_multi*, const rtc_camera*, const rtc_sampling*, int32_t fuel, double* rgb, rtc_stats* stats);
/* The sample rays themselves: n*N rows {o, d}, pixel-major, k inner (host array).  scene != NULL: generated by the device kernel and
 * copied back; scene == NULL: evaluated on the host by the same function, no device needed (like rtc_ppm). */
int rtc_camera_rays(rtc_scene*, const rtc_camera*, const rtc_sampling*, const uint64_t* pixel_indices, uint64_t first, uint64_t n, double* rays);

/* ---- adaptive sampling (rtc_adaptive above) ---------------------------------------------------------------------------------------
 * The whole frame (the rule needs neighbours), on one device.  On the scene's stream: the base pass into the frame buffer (`base` of
 * side 1 without jitter or lens goes the way rtc_render goes: row launch, measured path choice; the bits are the same), three small
 * kernels that flag the refined pixels and compact their indices into an ascending device list (ballot masks, a scan of per-block counts,
 * a scatter: no atomic orders it), then rtc_render_sampled's chunks over that list with `fine`, whose resolve writes each mean to
 * its pixel of the frame.  The host must know the list's length to size the chunks: ONE 8-byte read-back between the passes is the
 * synchronisation this feature adds (the base pass itself ends as a synchronous rtc_render does).  A list of 0 pixels skips the second pass.
 * Device path of the second pass: RTC_KERNEL pins as ever; otherwise the scene's first guess (rtc_scene_path_info) over the rays of
 * a chunk -- the list's length changes with every frame, so nothing is measured.
 * rgb: hsize*vsize*3 doubles (host).  mask (optional): hsize*vsize bytes (host), 1 = refined.  n_refined (optional): the list's length.
 * rtc_stats: pixels = the frame's, rays_primary = pixels * Nb + n_refined * Nf, counters summed over both passes, kernel_ms = both
 * passes and the kernels between them. */
int rtc_render_adaptive(rtc_scene*, const rtc_camera*, const rtc_adaptive*, int32_t fuel, double* rgb, uint8_t* mask, uint64_t* n_refined, rtc_stats* stats);
/* Same, quantised on the device (Color::clamp): rgb8 = hsize*vsize*3 bytes (host). */
int rtc_render_adaptive_rgb8(rtc_scene*, const rtc_camera*, const rtc_adaptive*, int32_t fuel, uint8_t* rgb8, uint8_t* mask, uint64_t* n_refined, rtc_stats* stats);
/* The contrast rule alone on a host frame (rgb: hsize*vsize*3 doubles): indices[0 .. *n - 1] = the refined pixels' image indices in
 * ascending order (indices: room for hsize*vsize values, host).  scene != NULL: the frame is uploaded, the device kernels flag and
 * compact, the list is copied back; scene == NULL: evaluated on the host by the same function, no device needed (like rtc_camera_rays). */
int rtc_contrast_pixels(rtc_scene*, uint64_t hsize, uint64_t vsize, const double* rgb, double threshold, uint32_t neighbours, uint64_t* indices, uint64_t* n);

/* ---- pixel reconstruction filters (rtc_filter above) ------------------------------------------------------------------------------
 * rtc_render_sampled's whole-row launches with a filter wider than the pixel, on one device.  Renders the rows [row_first, row_first +
 * n_rows) of the image (rgb: n_rows*hsize*3 doubles, host), filtered over the whole image's neighbours: the output rows are cut into
 * chunks of whole rows; a chunk of rows [a, b) traces the rows [max(0, a - W), min(vsize, b + W)) -- generator, the scene's ray kernels
 * over explicit rays, then a gather kernel (csrc/rtc_filter.hip) that writes the chunk's own rows and nothing else.  The W halo rows of a
 * chunk are traced again by its neighbour: the price of two reusable buffers; the samples do not depend on the chunk, so any split of the
 * frame into row ranges, and any RTC_SAMPLED_MAX_RAYS (which bounds the TRACED rays of a chunk, halo included; never less than one output
 * row and its halo), gives the whole frame's bits.  Device path as for rtc_render_sampled's row launches (the launch shape includes the
 * filter and the row range; the guess counts a chunk's traced rays).  rtc_stats: pixels = the output pixels, rays_primary = the rays
 * actually traced (halo rows counted each time), counters summed, kernel_ms = generator + traces + filter kernel. */
int rtc_render_filtered(rtc_scene*, const rtc_camera*, const rtc_sampling*, const rtc_filter*, int32_t fuel, uint32_t row_first, uint32_t n_rows,
                        double* rgb, rtc_stats* stats);
/* The whole frame, quantised on the device (Color::clamp): rgb8 = hsize*vsize*3 bytes (host). */
int rtc_render_filtered_rgb8(rtc_scene*, const rtc_camera*, const rtc_sampling*, const rtc_filter*, int32_t fuel, uint8_t* rgb8, rtc_stats* stats);
/* The filter step alone on the caller's sample colours: sample_rgb = hsize*vsize*N*3 doubles, pixel-major, k inner (rtc_trace_rays'
 * colours of rtc_camera_rays' rays); rgb = hsize*vsize*3 doubles (both host).  scene != NULL: the colours are uploaded, the device
 * kernel filters, the frame is copied back; scene == NULL: evaluated on the host by the same function, no device needed (like
 * rtc_contrast_pixels).  Of `sampling` only side, flags and seed are read (its lens is validated). */
int rtc_filter_frame(rtc_scene*, uint64_t hsize, uint64_t vsize, const rtc_sampling*, const rtc_filter*, const double* sample_rgb, double* rgb);

/* ---- the shutter (rtc_shutter above) -------------------------------------------------------------------------------------------------
 * rtc_render_sampled over n_poses poses: pixels as in rtc_render (a range or a list, of the cameras' common frame).  On one device, in
 * rtc_render_sampled's chunks (RTC_SAMPLED_MAX_RAYS as there; the buffers are scenes[0]'s).  Per chunk, on scenes[0]'s stream: two small
 * kernels and a scan (csrc/rtc_shutter.hip) deal the chunk's samples to the poses and sort their ids by pose -- ballots, ranks within the
 * wave, a pose-major table of per-block counts, ONE exclusive scan: no atomic orders the list, it is ascending within a pose --; the host
 * must know the runs to launch over them: ONE read-back of the n_poses + 1 offsets is the synchronisation this feature adds per chunk.
 * Then, per pose with a non-empty run, a generator kernel writes the run's rays through that pose's camera and that pose's scene traces
 * them as explicit rays (every scene kind, both device paths; ordered against scenes[0]'s stream by an event before, and by the end of
 * the synchronous trace after); a last kernel gathers each pixel's N colours back in k order and WRITES their mean.  Only pixels leave the device.
 * Device path of a run: RTC_KERNEL pins as ever; otherwise its scene's first guess (rtc_scene_path_info) over the run's rays -- the runs
 * change with the seed, so nothing is measured.  rtc_stats: pixels = n, rays_primary = n * N, counters summed over poses and chunks,
 * kernel_ms = dealing + generators + traces + resolve, n_launches counts those kernels too.  No hit records or digests. */
int rtc_render_shutter(rtc_scene* const* scenes, const rtc_camera* cameras, uint32_t n_poses, const rtc_shutter*, const rtc_sampling*,
                       int32_t fuel, const uint64_t* pixel_indices, uint64_t first, uint64_t n, double* rgb, rtc_stats* stats);
/* The whole frame, quantised on the device (Color::clamp): rgb8 = hsize*vsize*3 bytes (host). */
int rtc_render_shutter_rgb8(rtc_scene* const* scenes, const rtc_camera* cameras, uint32_t n_poses, const rtc_shutter*, const rtc_sampling*,
                            int32_t fuel, uint8_t* rgb8, rtc_stats* stats);
/* The dealing alone, for pixels as in rtc_render_shutter (of a frame hsize wide; one chunk: n * N below 2^31): order[0 .. n*N-1] = the
 * sample ids (slot * N + k, slot = the pixel's place in the range or list) pose-major, ascending within a pose; offsets[0 .. n_poses] =
 * where each pose's run starts (offsets[n_poses] = n*N).  scene != NULL: the device kernels above, copied back; scene == NULL: the same
 * rule on the host (a stable counting sort), no device needed -- like rtc_contrast_pixels. */
int rtc_shutter_deal(rtc_scene* scene, uint64_t hsize, uint32_t n_poses, const rtc_shutter*, const rtc_sampling*,
                     const uint64_t* pixel_indices, uint64_t first, uint64_t n, uint32_t* order, uint64_t* offsets);
/* Test hook: the pose of a hashed draw u in [0, 1) among n_poses (>= 1) -- (uint32_t)(u * (double)n_poses), held to n_poses - 1.  Host only. */
uint32_t rtc_shutter_draw_pose(double u, uint32_t n_poses);

/* ---- the step after the path: Color::clamp and Image::ppm ---------------------------------
 * Color::clamp (src/color.rs:42-46): u8 = round(min(max(c, 0), 1) * 255), round half away from zero, NaN -> 255 (Rust's
 * f64::min returns the non-NaN operand).  n_values = 3 * pixels.  Device pointers, on the scene's stream. */
int rtc_quantize_device(rtc_scene*, const double* rgb_dev, uint64_t n_values, uint8_t* out_dev, int sync);
/* Same through host buffers (upload, quantise on device, download). */
int rtc_quantize(rtc_scene*, const double* rgb, uint64_t n_values, uint8_t* out);
/* Image::ppm (src/image.rs:93-112) from quantised pixels: "P3\n{w} {h}\n255", <= 5 pixels per line, a new line at each
 * row start, trailing newline.  Host-only formatting (no device needed).  Returns the byte count (excluding the NUL);
 * writes only if cap is large enough. */
uint64_t rtc_ppm(uint64_t hsize, uint64_t vsize, const uint8_t* rgb8, char* out, uint64_t cap);

/* Waits for the stream and returns (and clears) the error state accumulated by EVERY launch since the last check or the last
 * synchronous render: RTC_ERR_NAN / RTC_ERR_DEVICE / RTC_ERR_UNSUPPORTED (a wavefront queue overflowed in an unsynchronised
 * launch).  Asynchronous launches (sync == 0, stats == NULL) do not report it themselves. */
int rtc_scene_check(rtc_scene*);
/* Stream markers for pipelined hosts: record marker `slot` (0..7) behind everything queued so far on the scene's stream;
 * wait for it on the host; device time between two recorded markers in ms.  RTC_ERR_INVALID for a slot outside 0..7 and for
 * waiting on / measuring a slot that was never recorded. */
int rtc_scene_record(rtc_scene*, int slot);
int rtc_scene_wait(rtc_scene*, int slot);
int rtc_scene_elapsed_ms(rtc_scene*, int slot_from, int slot_to, double* ms);

/* Blocks until the scene's stream is idle. */
int rtc_scene_sync(rtc_scene*);

/* Accelerator facts for reports: traversal-program length, BVH node count (4-wide nodes, 128 B each), triangles packed
 * into mesh BVH leaves, deepest BVH (levels of 4-wide nodes).  Any pointer may be NULL. */
void rtc_scene_accel_info(const rtc_scene*, uint32_t* n_ops, uint32_t* n_bvh_nodes, uint32_t* n_mesh_tris, uint32_t* bvh_depth);

/* Number of this scene's mesh accelerators whose binary tree was built on the device: a linear BVH — items sorted by the cell
 * of a longest-side-first bisection of their bounds, Karras' radix tree, csrc/bvh_device.hip — instead of the host's binned-SAH
 * build.  Default: meshes of at least 100 000 triangles (a quarter of the build time, frames within 8 % of the SAH tree's);
 * RTC_DEVICE_BVH=0: never; =1: from 4 096 triangles (RTC_DEVICE_BVH_MIN overrides the threshold).  The accelerator is
 * results-neutral: pixels and hit records do not depend on it. */
int rtc_scene_bvh_built_on_device(const rtc_scene*);

/* Test hook: ONE run of a binary-tree builder on the caller's boxes, handed back raw; no scene is involved and nothing about how scenes
 * are built depends on it.  boxes = n records of 6 doubles (lo[3], hi[3]: an item's bounds); leaf_max = items per leaf (both builders
 * clamp it to 1..8); base = index of the first item in the leaf references; where = 0: the host's binned-SAH builder (no device needed,
 * like rtc_ppm), 1: the device's linear-BVH builder (csrc/bvh_device.hip).  Outputs, each with its capacity in records: nodes = the 64-byte
 * node records verbatim (both children's boxes as f32 relative to frame[0..2], rounded outward; child references >= 0: node index,
 * < 0: leaf, items [first, first + count) with first = (~ref) >> 3, count = ((~ref) & 7) + 1); order = the items in leaf order (n entries);
 * keys = the n sorted 63-bit keys of the device builder (where = 1 only; NULL or capacity 0: not wanted); frame[4] = the tree's centre and
 * inf-norm radius; *depth and *stack_need = levels of 4-wide nodes and worst-case traversal stack entries of that tree after the 4-wide
 * collapse (-1 each if the tree cannot be walked).  *n_nodes receives the number of node records in every case where a tree was built.
 * Returns RTC_OK; -1, the builder's own answer, when the device builder declines (n < 2, n <= leaf_max, an unbounded item, no device);
 * RTC_ERR_INVALID for NULL arguments, n == 0, another `where`, or a capacity that is too small (nothing is written to that buffer). */
int rtc_bvh_build_raw(const double* boxes, uint32_t n, int32_t leaf_max, uint32_t base, int32_t where, void* nodes, uint32_t nodes_cap, uint32_t* n_nodes,
                      uint32_t* order, uint32_t order_cap, uint64_t* keys, uint32_t keys_cap, int32_t* root, double* frame, int32_t* depth, int32_t* stack_need);
/* The 4-wide collapse alone on the caller's node records (the layout above): *depth and *stack_need as above.  Host only.  RTC_ERR_INVALID
 * for NULL arguments, a root or child reference outside the array, or a node that is reached twice. */
int rtc_bvh_collapse_raw(const void* nodes, uint32_t n_nodes, int32_t root, int32_t* depth, int32_t* stack_need);

/* Test hook: ONE light-grid build on the caller's primitives and one light position, handed back raw, through the
 * function a scene's build calls; host only, no device, no scene.  Primitive k is geometry[k] (RTC_SPHERE..; no planes), limits[2k..2k+1]
 * (cylinder / cone {min, max}, finite; others: ignored), transform_inv + 16 k (world -> object, row major, as rtc_xform) and, for triangles,
 * tris + 9 k ({p1, e1, e2}; tris may be NULL when there is no triangle).  n = cells per face edge (2..512); max_list = the longest list
 * a cell may hold (at least 8; a scene takes its traversal stack's depth); tight = 0: the rectangle lists of RTC_LIGHT_GRID_TIGHT=0.
 * Outputs: cells[6 n n + 1] = per cell (face, v, u) the index of its first item, the last entry = *n_items; items = *n_items pairs
 * {leaf reference = ~(k << 3), f32 bits of the lower bound of the primitive's distance from the light}, per cell sorted by (distance,
 * k); a cell with more than max_list candidates holds the one reference 0x7fffffff (its rays walk the BVH).  *n_items is written
 * whenever a grid was built.  Returns RTC_OK; -1 when the build declines (over its work budget, or most cells over-full);
 * RTC_ERR_INVALID for NULL arguments, n out of range, a primitive without bounds, or a capacity that is too small. */
int rtc_light_grid_build_raw(const int32_t* geometry, const double* limits, const double* transform_inv, const double* tris, uint32_t n_prims, const double* light, int32_t n,
                             int32_t max_list, int32_t tight, uint32_t* cells, uint32_t cells_cap, int32_t* items, uint32_t items_cap, uint32_t* n_items);

/* Test hook, not part of the rendering surface: the exclusive scan that orders the work lists of adaptive sampling (the compaction's block
 * counts) and of the shutter (the dealing's pose-major count table), alone, on the caller's words.  values[0 .. n - 1] are replaced by their
 * exclusive prefix sums (values[i] = the sum of the former values[0 .. i - 1], modulo 2^64) and *total receives the sum of all n.  With a
 * scene the device's scan runs on that scene's device and stream (csrc/rtc_adaptive.hip rtc_launch_scan: tiles of 256 entries, one
 * level per factor of 256 in n, so 1 level up to 256 entries, 2 up to 65 536, 3 up to 2^24, ...) in device buffers of the call's own
 * (n + the levels' words + 1, freed before it returns; nothing of the scene is touched); with scene == NULL the same sums are formed in a
 * plain loop on the host, no device needed.  n == 0 sets *total = 0 and reads nothing.  RTC_ERR_INVALID for a NULL `total`, or NULL
 * `values` with n > 0; RTC_ERR_UNSUPPORTED for n >= 2^39 with a scene (the limit of the frames the compaction accepts). */
int rtc_scan_raw(rtc_scene* scene, uint64_t* values, uint64_t n, uint64_t* total);

/* Test hook, not part of the rendering surface: ONE culling predicate of the ray kernels (csrc/rtc_device.hpp; DESIGN.md 4, "culling only")
 * on n caller-supplied records, one uint8_t answer (0 / 1) per record.  No scene geometry is involved: the scene only names the device and
 * the stream, and the records and answers travel in device buffers of the call's own, freed before it returns (csrc/rtc_probe.hip; the
 * CPU emulator runs the same functions in a host loop and ignores the scene).  A record is an array of doubles:
 *   RTC_CULL_SLAB   (18) fr[4] = a BVH's centre and radius, ray o[3] d[3] in the BVH's space, tlo, thi, box lo[3] hi[3] (f32 values, relative
 *                        to the centre, within the radius of it): make_frame + t_interval32 + slab32c, 1 = the box is taken
 *   RTC_CULL_POINT  (17) fr[4], ray, t_hit, box: make_frame_point + point_in_box, 1 = the hit point counts as inside the box
 *   RTC_CULL_GATE   (12) box lo[3] hi[3] (f64), ray: group_box_hit, 1 = the ray passes the group's box
 *   RTC_CULL_PLANE   (3) oy, dy, mode (0 closest, 1 any-hit shadow, 2 closest shadow, 3 containers): plane_behind where the kernels ask it, that is
 *                        after the reference's |dy| < EPSILON rule has let the ray through; 1 = the plane is skipped as behind the origin
 *   RTC_CULL_BEHIND  (9) point[3], light[3], unit normal[3], in a scene with backface_skip = 1: light_is_behind, 1 = the shadow ray is skipped
 * n == 0 reads and writes nothing.  RTC_ERR_INVALID for another kind, NULL records or answers with n > 0, or a NULL scene where a
 * device is needed (librtc_amd.so); RTC_ERR_UNSUPPORTED for n >= 2^32 on the device. */
enum { RTC_CULL_SLAB = 0, RTC_CULL_POINT = 1, RTC_CULL_GATE = 2, RTC_CULL_PLANE = 3, RTC_CULL_BEHIND = 4 };
int rtc_cull_probe_raw(rtc_scene* scene, int32_t kind, const double* records, uint64_t n, uint8_t* answers);

/* Dynamic LDS (bytes per block) the wavefront traversal kernel uses for this scene: > 0 = the scene's accelerator nodes, intersection
 * records and mesh triangles are copied into every CU's LDS and walks read them there (small scenes: the tables and the traversal
 * stacks fit 160 KB); 0 = they are read from memory.  bench.py's byte accounting counts LDS-resident records as 0 bytes. */
uint32_t rtc_scene_wavefront_lds_bytes(const rtc_scene*);

/* Read-only: the grid (blocks) of the wavefront traversal kernel in a launch of this scene made now.  sync != 0: a launch the host
 * waits for (rtc_render, any launch with a stats pointer or sync set); 0: an unsynchronised one (rtc_render_rows_device / _bands_device
 * with sync = 0 and no stats).  A scene whose tables live in LDS (rtc_scene_wavefront_lds_bytes > 0) runs one persistent 768-thread
 * block per CU, which fills the CU: *grid = the device's CU count.  Such a block leaves no room for the kernels of other streams, so an
 * UNSYNCHRONISED launch of such a scene, while at least one other scene is alive on the same device, leaves *spare_cus CUs out:
 * *grid = n_cu - spare_cus, and the shading and gather kernels of the other scenes' frames run there meanwhile ("Spare
 * CUs").  Every grid renders the same bits.  The environment variable RTC_WF_SPARE_CUS=k, read when a scene is created and clamped
 * to 0 .. n_cu - 1, replaces the built-in number for that scene; 0 turns the rule off.  A scene whose tables are read from memory
 * (lds_bytes == 0) reports the grid of that build (one-wave blocks, as many as the device holds), which no switch changes.  (A device
 * that refused the LDS size, rtc_kernel_info.lds_refused, runs that build too, whatever is reported here.)  *n_cu: CUs of the scene's
 * device; *spare_cus: the scene's number, whether or not it applies now; *live: scenes alive on the device, this one included.  Any
 * out pointer may be NULL.  RTC_ERR_INVALID for a NULL scene. */
int rtc_scene_wavefront_ts_grid(const rtc_scene*, int32_t sync, uint32_t* grid, uint32_t* n_cu, uint32_t* spare_cus, uint32_t* live);

/* Test hook: which build of each ray kernel a launch of this scene takes, read-only.  The ray kernels are compiled in several builds
 * (DESIGN.md "Kernel builds"); the launchers and this query call the same selection functions, so what is reported is what runs -- with one exception, decided
 * at launch time: a device that refuses the dynamic LDS size runs wf_ts's memory build (lds_refused below tells).
 * path = 1: the one-kernel path (trace_build is set, the wf_* fields are -1); 4: the wavefront path (the reverse); count != 0: a launch
 * with counters (a stats pointer, rtc_render_hit_digest).  RTC_NO_KOPS (set: the program is read from memory), RTC_KOPS_GROUPS=0
 * (programs with per-primitive gates are read from memory) and RTC_WF_LDS=0 (tables are read from memory) are read when a scene is
 * created and hold for that scene, as RTC_KERNEL does.  Returns RTC_ERR_INVALID for a NULL argument or another path. */
enum { RTC_TRACE_DEFAULT = 0, RTC_TRACE_COUNT = 1, RTC_TRACE_LEAN = 2, RTC_TRACE_3WAVE = 3 };
enum { RTC_WF_TS_MEM = 0, RTC_WF_TS_MEM_COUNT = 1, RTC_WF_TS_LDS = 2, RTC_WF_TS_LDS_COUNT = 3 };
enum { RTC_SHADE_COUNT = 0, RTC_SHADE_COUNT_UV = 1, RTC_SHADE_UV = 2, RTC_SHADE_PIPE_LV0 = 3, RTC_SHADE_PIPE = 4, RTC_SHADE_PAT = 5 };
typedef struct rtc_kernel_info {
  int32_t variant;          /* row of the variant table (csrc/rtc_device.hpp RTC_VARIANTS) */
  int32_t n_kops;           /* ops of the program in the kernel arguments (0: the program is read from memory) */
  int32_t n_kplanes;        /* plane records in the kernel arguments */
  int32_t n_kaux;           /* accelerator roots in the kernel arguments */
  int32_t has_recs;         /* some op reads the intersection-record table */
  int32_t all_plain;        /* every material's root pattern is a Plain colour */
  int32_t no_glass_mirror;  /* no material both reflects and refracts */
  int32_t big_scene;        /* the scene's tables exceed 32 MiB */
  uint32_t lds_bytes;       /* path 4: dynamic LDS of the traversal kernel, 0 = tables in memory */
  int32_t trace_build;      /* path 1: RTC_TRACE_* */
  int32_t wf_ts_build;      /* path 4: RTC_WF_TS_* */
  int32_t wf_shade_build0;  /* path 4: RTC_SHADE_* of level 0 */
  int32_t wf_shade_build;   /* path 4: RTC_SHADE_* of the levels above */
  /* what the LDS size is computed from: 112 B per accelerator node, 128 B per intersection record if has_recs, 76 B per mesh
   * triangle (rounded up to 16) if has_mesh, and 4 * bvh_stack bytes of traversal stack for each of the block's 768 threads */
  int32_t n_bvh_nodes, n_recs, n_mesh_tris, has_mesh, bvh_stack;
  int32_t lds_refused;      /* path 4, lds_bytes > 0: the scene's device has refused that much dynamic LDS in an earlier launch, so
                               its launches run the RTC_WF_TS_MEM* build instead of the one reported (0 before any launch) */
} rtc_kernel_info;
int rtc_scene_kernel_info(const rtc_scene*, int32_t path, int32_t count, rtc_kernel_info* out);

/* Which device path renders whole-row launches of this scene (both give bit-identical pixels and hits):
 *   1  one kernel: a lane walks its pixel's whole ray tree (rtc_trace_kernel);
 *   4  wavefront: per bounce level a closest-hit + shadow kernel and a shading kernel over ray queues (wf_* kernels).
 * RTC_KERNEL=1|4 pins a path for every launch of scenes created afterwards (pixel lists and explicit rays included: the parity
 * tests run both).  With the environment variable RTC_KERNEL unset the library measures: for one launch shape (camera, rows, fuel) the first
 * four SYNCHRONOUS launches alternate between the paths (the smaller of a path's two device times counts: a first launch
 * pays for code loading and scratch), every later launch of that shape takes the faster.  Until a shape is measured — a caller
 * that renders one frame per scene, asynchronous launches — a guess from the scene decides: wavefront iff it has >= 32 bounded
 * analytic primitives, >= 10 % of its primitives reflect or refract, fuel >= 2 and the launch has >= 256 K pixels (the one-kernel
 * path needs no ray queues).  Whole-row launches of the sampled camera (rtc_render_sampled*) are launch shapes too -- camera, sampling,
 * rows and fuel; the guess counts the rays of a chunk, the measurement sums the chunks' device times --; their pixel lists stay on
 * the one-kernel path.  Reports the state for
 * the most recent launch shape: *choice = 0 while undecided, else 1 or 4; the measured device times in ms (< 0 = not yet
 * measured).  Any pointer may be NULL. */
void rtc_scene_path_info(const rtc_scene*, int32_t* choice, double* one_kernel_ms, double* wavefront_ms);

#ifdef __cplusplus
}
#endif
#endif

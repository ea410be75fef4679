/*
 * pt.h -- C-ABI of the MI355X-native path tracer (libptamd.so).
 *
 * Drop-in boundary for CulDeVu/CUDAPathTracer's render call.  Plain C types,
 * plain pointers and sizes; no torch, no HIP types in any signature.
 *
 * Two halves:
 *   1. Host surface (plain C++ behind C entry points), the reference's callers of the path:
 *        pt_scene_*      <- modelLoader.h:43-47 globals + loadOBJ (modelLoader.h:125-210)
 *                           via tinyobj::LoadObj (tiny_obj_loader.cc:638-884)
 *        pt_scene_build_bvh <- buildBVH (BVH.h:443-474) + depth guard (kernel.cu:627-631)
 *        pt_camera_ray / pt_morton_* <- camera.h:36-97
 *        pt_view / pt_view_look_at / pt_view_set_fov / pt_camera_ray_view  (no counterpart) an oriented camera: a
 *                           view places the pt_camera in the world (look-at, film extent); every entry point that
 *                           takes a camera has a *_view twin, and a NULL view is the reference camera
 *        pt_write_ppm    <- kernel.cu:763-778 + color.h:59-71
 *   2. Render (hand-written gfx950 HIP kernels):
 *        pt_create       <- the uploads of kernel.cu:637-700 (scene, camera, BVH to device)
 *        pt_render       <- setupCurand (kernel.cu:527-533, :639) + setupImgBuffer (:520-526, :662)
 *                           + the NUM_SAMPLES-1 launches of drawPixel (kernel.cu:535-553, :709-736)
 *        pt_accum_*      <- the progressive loop's state between launches (kernel.cu:527-553, 702-737)
 *        pt_noise_* / pt_accum_add_until  (no counterpart in the reference) per-pixel noise estimates of an
 *                           accumulator from batch means, and a loop that adds passes until the image converged
 *        pt_accum_freeze / pt_noise_freeze / pt_accum_add_adaptive  (no counterpart) adaptive sampling: converged
 *                           pixels are frozen and the passes sample only the rest
 *        pt_session_*    (no counterpart) the whole progressive state -- accumulator, frozen-at counts, estimator -- in
 *                           one file: an adaptive render resumes in another process as if it had never stopped
 *        pt_render_features / pt_denoise  (no counterpart in the reference) per-pixel first-hit feature
 *                           buffers and an edge-avoiding a-trous filter: a preview from a few samples per pixel
 *        pt_noise_variance / pt_denoise_guided  (no counterpart) the estimator's variance map and an a-trous filter
 *                           guided by it, which leaves converged pixels alone: its result converges to the render
 *        pt_project_view / pt_temporal_*  (no counterpart) temporal reprojection: a history of the image that follows
 *                           a moving camera through the feature buffers, and the variance map of what it holds
 *        pt_destroy      <- cudaFree (kernel.cu:782-783)
 *        pt_last_error   <- checkError (kernel.cu:37-42), but returned instead of printed
 *
 * Errors: every int-returning entry point returns PT_OK (0) or a negative PT_E* code and
 * records a message for pt_last_error() (thread-local).  Nothing calls exit().
 * Ownership: the caller owns every array it passes; pt_create copies what it needs and keeps
 * no pointer into caller memory.  A pt_ctx is used by one host thread at a time.
 */
#ifndef PT_PT_H
#define PT_PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 6

/* ---- status codes */
#define PT_OK 0
#define PT_E_INVALID (-1)    /* bad argument                                              */
#define PT_E_IO (-2)         /* cannot open / read / write a file                          */
#define PT_E_SCENE (-3)      /* scene unusable (fewer than 2 triangles, bad indices, ...)  */
#define PT_E_BVH_DEPTH (-4)  /* BVH depth >= 64 (kernel.cu:627-631 "BVH depth is too big") */
#define PT_E_HIP (-5)        /* HIP runtime error (message names the call)                 */
#define PT_E_NODEV (-6)      /* no gfx950 device / device index out of range               */
#define PT_E_OOM (-7)

/* ---- POD mirrors of the reference layouts (static_assert'ed in the implementation) */
typedef struct { float x, y, z; } pt_vec3;                                      /* vec3.h:4-7, 12 B       */
typedef struct { int32_t v0, v1, v2; pt_vec3 norm; int32_t mat; } pt_triangle; /* modelLoader.h:14-19, 28 B */
typedef struct { double albedo[3]; double emission[3]; } pt_material;          /* modelLoader.h:21-25, 48 B */
typedef struct { pt_vec3 lo, hi; uint32_t left, right; } pt_bvh_node;          /* BVH.h:111-115, 32 B    */
typedef struct {                                                                /* camera.h:26-34, 32 B   */
    pt_vec3 pos;
    float dist_from_film;
    float focal_length;
    float radius;
    int32_t pxl_width, pxl_height;
} pt_camera;

#define PT_BVH_LEAF_FLAG 0x80000000u   /* limits.h:6 */
#define PT_MAX_BVH_DEPTH 64            /* kernel.cu:35 */
#define PT_LIGHT_SPHERE 0x80000000u    /* lights[] entry: PT_LIGHT_SPHERE | sphere index    */

/* sphere.h:7-12 (64 B).  The reference has the struct but no intersection code (its include is
 * commented out, kernel.cu:21); the semantics here are this build's:
 * hit ids num_tris + i, closest root with 0 < t < MAX_FLOAT, normal (p - pos) / rad, material
 * {diffuse, emission}; emissive spheres are area lights of area 4*3.14159*rad^2. */
typedef struct { pt_vec3 pos; float rad; double diffuse[3]; double emission[3]; } pt_sphere;

/* Read-only view of a scene: sceneDesc (modelLoader.h:29-41) + BVH_array (BVH.h:116-121).
 *
 * The arrays may be pt_scene_view's or the caller's own, BVH included.  pt_create checks, on the host and before it
 * looks for a device, what the device walks rely on, and refuses anything else with PT_E_SCENE (the message names the
 * node or triangle):
 *   - the nodes are a binary tree, root = node 0, that reaches every triangle exactly once (any node order: a child
 *     may have a smaller index than its parent); every index of tris, lights and the tree is in range;
 *   - every box coordinate is finite;
 *   - every child node's box lies within its parent's (lo >= lo and hi <= hi per axis, compared as floats);
 *   - the three vertices of every triangle lie within the box of the node whose leaf it is;
 *   - bvh_depth >= the tree's true depth (a leaf counts 1, a node 1 + its deeper child): every traversal stack is
 *     sized from the field.  A larger value changes no result.  A true depth >= PT_MAX_BVH_DEPTH is PT_E_BVH_DEPTH.
 * pt_scene_build_bvh's trees meet all of it.  Boxes may be looser than the vertices (the scene's extent, by which
 * far origins and cameras are told, is that of the triangles' vertices and the spheres, not of the boxes).  Hits at equal distance go to the
 * triangle met first in left-first depth-first order of this tree, as in the reference's trace().  norm, lights and
 * total_light_area are used as given. */
typedef struct {
    uint32_t num_verts, num_tris, num_mats, num_lights;
    const pt_vec3* verts;
    const pt_triangle* tris;
    const pt_material* mats;
    const uint32_t* lights;
    float total_light_area;
    const pt_bvh_node* bvh;    /* node 0 = root (pt_scene_build_bvh: breadth-first) */
    uint32_t bvh_size;         /* = num_tris - 1 (0 for a scene of spheres only) */
    int32_t bvh_depth;         /* BVH_node::depth of the root (BVH.h:322, :346), or more */
    const pt_sphere* spheres;  /* sphere primitives (hit ids num_tris + i)      */
    uint32_t num_spheres;
} pt_scene;

/* ======================================================================= host surface */
typedef struct pt_host_scene pt_host_scene;

/* Empty scene (the reference's global vectors, modelLoader.h:43-47, as an object). */
pt_host_scene* pt_scene_new(void);
void pt_scene_free(pt_host_scene* s);

/* loadOBJ(filename, origin, scale, flipNormals) -- modelLoader.h:125-210.  Appends to the
 * scene exactly as the reference appends to its globals.  mtl_basepath: the directory
 * prefix tinyobj prepends to `mtllib` names (the reference hard-codes "models/",
 * modelLoader.h:132); NULL means "models/".  A tinyobj warning/error (e.g. a missing .mtl,
 * which makes tinyobj stop reading the OBJ at the mtllib line) does not fail the call, as in
 * the reference: it is returned through pt_scene_last_warning(). */
int pt_scene_load_obj(pt_host_scene* s, const char* obj_path, const char* mtl_basepath,
                      pt_vec3 origin, float scale, int flip_normals);
const char* pt_scene_last_warning(const pt_host_scene* s);

/* buildBVH() -- BVH.h:443-474, byte-identical node array.  Fails with PT_E_SCENE for
 * fewer than 2 triangles (decision d5) and PT_E_BVH_DEPTH when depth >= 64. */
int pt_scene_build_bvh(pt_host_scene* s);

/* Append a sphere primitive (sphere.h); an emissive one (emission[0] != 0, the triangle rule of
 * modelLoader.h:188) joins the light list and totalLightArea.  rad must be finite and > 0. */
int pt_scene_add_sphere(pt_host_scene* scene, const pt_sphere* sphere);

/* Borrow a view of the scene arrays (valid until the next mutation or pt_scene_free). */
int pt_scene_view(const pt_host_scene* s, pt_scene* out);

/* camera.h:57-75 Morton maps and camera.h:77-97 cameraRay.  `lens` = 0: no lens draws
 * (exactly zero lens offset); otherwise (u1,u2) are the lens draws. */
uint32_t pt_morton_pxl_to_i(uint32_t x, uint32_t y);
void pt_morton_i_to_pxl(uint32_t idx, uint32_t* x, uint32_t* y);
void pt_camera_ray(const pt_camera* cam, uint32_t idx, int lens, float u1, float u2,
                   pt_vec3* origin, pt_vec3* dir);

/* ------------------------------------------------- the oriented camera (no counterpart in the reference)
 * pt_camera mirrors the reference's struct: it looks down -z with +y up, and its film is the unit square whatever
 * the image's shape (pxlToFilm, camera.h: no aspect correction).  A pt_view places that camera in the world: an
 * orthonormal basis and the film's extent.  Every entry point that takes a camera has a *_view twin with
 * `const pt_view* view` after `cam`; view = NULL is the reference camera, today's code and today's bits (the plain
 * entry points are calls of their twins with NULL).
 *
 * The ray of pixel (px, py) of a W x H camera (W = pxl_width, H = pxl_height), all f32, every operation rounded on
 * its own, no contraction, IEEE division and square root; `lens` as everywhere: radius != 0 or Morton index 0:
 *   f   = ((float)px/(float)W - 0.5f) * film_w,  ((float)py/(float)H - 0.5f) * film_h,  dist
 *   f   = (f * -focal) / dist
 *   lo  = lens ? (r*cos(theta), r*sin(theta), 0) with r = radius*sqrt(u1), theta = (float)(2*3.14159*(double)u2),
 *                as pt_camera_ray  :  (0, 0, 0)
 *   c   = f - lo
 *   w_k = (right[k]*c.x + up[k]*c.y) + back[k]*c.z           k = 0, 1, 2
 *   d   = w / sqrt((w.x*w.x + w.y*w.y) + w.z*w.z)             (the normalisation pt_camera_ray uses)
 *   o_k = lens ? (right[k]*lo.x + up[k]*lo.y) + pos[k]  :  (0 + pos[k])
 * An identity view (right = +x, up = +y, back = +z, film 1 x 1) is NOT promised to equal the NULL view in the sign
 * of a zero component: (-0)*1 + c.y*0 is +0 when c.y > 0, where the reference camera keeps -0.  Compare an oriented
 * render against this arithmetic, never against the reference camera.
 *
 * A view is valid when all 11 floats are finite, film_w > 0 and film_h > 0, and, in double, each of |r.r - 1|,
 * |u.u - 1|, |b.b - 1|, |r.u|, |r.b|, |u.b| is <= 1e-3 (a condition, not a measurement; left-handed bases -- mirrors
 * -- are allowed).  Every entry point that takes a view returns PT_E_INVALID for an invalid one.
 *
 * Host helpers (no device; computed in double from the float inputs, rounded to float once at the end):
 *   pt_view_look_at  back = (pos - target)/|pos - target|, right = cross(up, back)/|cross(up, back)|,
 *                    up' = cross(back, right), film 1 x 1.  PT_E_INVALID: pos == target, up parallel to back (or
 *                    zero: |cross(up, back)| <= 1e-12 |up|), a non-finite input, a null out.  pos (0,1,3), target (0,1,0), up (0,1,0) -- the
 *                    reference camera's pose -- gives the identity.
 *   pt_view_set_fov  film_h = 2*dist_from_film*tan(vfov/2), film_w = film_h*width/height (square pixels); the
 *                    basis is left alone.  PT_E_INVALID: vfov_deg outside (0, 180), width or height <= 0, a
 *                    dist_from_film that is not finite and > 0, a result that is not finite and > 0 as a float.
 *   pt_view_validate the condition above (PT_OK or PT_E_INVALID with the reason in pt_last_error).
 *   pt_camera_ray_view  the arithmetic above on the host, as pt_camera_ray is for the reference camera (which a
 *                    NULL view gives); the view is not validated. */
typedef struct {
    float right[3], up[3], back[3];  /* world-space images of camera +x, +y, +z; the camera looks along -back */
    float film_w, film_h;            /* film extent in the reference's film units; 1, 1 = the reference's unit square */
} pt_view;                           /* 44 B, static_assert'ed */
int pt_view_look_at(pt_vec3 pos, pt_vec3 target, pt_vec3 up, pt_view* out);
int pt_view_set_fov(pt_view* v, const pt_camera* cam, float vfov_deg, int width, int height);
int pt_view_validate(const pt_view* v);
void pt_camera_ray_view(const pt_camera* cam, const pt_view* view /* NULL = pt_camera_ray */, uint32_t idx, int lens,
                        float u1, float u2, pt_vec3* origin, pt_vec3* dir);

/* kernel.cu:763-778: "P3 W H 255\n" then "%d %d %d " for rows y = 0..H-1 and x = W-1..0,
 * c = (int)(pow(c/(c+1), (float)(1/2.2)) * 255).  rgb is the scanline mean buffer written by
 * pt_render (pixel (x,y) at rgb[(y*W + x)*3]); the f64 variant takes the reference's own
 * double accumulator type. */
int pt_write_ppm(const char* path, const float* rgb, int width, int height);
/* Same for a buffer in either pixel order (PT_ORDER_MORTON: the reference's imgBuffer_host
 * indexing, kernel.cu:771; square power-of-two sizes only). */
int pt_write_ppm_order(const char* path, const float* rgb, int width, int height, int pixel_order);
int pt_write_ppm_f64(const char* path, const double* rgb, int width, int height);
/* PPM tone map of one value: (int)(pow(c/(c+1), (double)(float)(1/2.2)) * 255). */
int pt_tonemap_u8(double c);

/* The PPM text of kernel.cu:763-778 from already tone-mapped codes codes[(y*W+x)*3+k] (the
 * values pt_tonemap_u8 / pt_tonemap produce), and a PFM float dump of the fp32 mean image
 * (lossless; rows bottom-up, little-endian, per the PFM format). */
int pt_write_ppm_codes(const char* path, const int32_t* codes, int width, int height);
int pt_write_pfm(const char* path, const float* rgb, int width, int height);

/* ============================================================================ render */
typedef struct pt_ctx pt_ctx;

#define PT_INTEGRATOR_UNIDIR 0   /* radianceAlongSingleStep2, kernel.cu:417-515 (north star) */
#define PT_INTEGRATOR_HEAD 1     /* radianceAlongSingleStep,  kernel.cu:217-415 (HEAD :549)  */

/* pt_params.flags */
#define PT_FLAG_REFERENCE_TRAVERSAL 0x1u  /* left-first stack walk with no distance culling,
                                             the exact node/triangle sequence of kernel.cu:112-161 */
#define PT_FLAG_NO_DEAD_PATH_SKIP 0x2u    /* trace every bounce even after the path weight is 0   */
#define PT_FLAG_NO_PRIMARY_CACHE 0x4u     /* re-trace the (sample-invariant) camera ray per sample  */
#define PT_FLAG_COUNT 0x8u                /* fill node/triangle test counters (slower variant)     */
#define PT_FLAG_REFERENCE_BVH 0x10u       /* culled walk on the reference BVH only (no SAH BVH)     */
#define PT_FLAG_TRI_COUNTS 0x20u          /* with PT_FLAG_COUNT: also the per-triangle test counts of
                                             kernel.cu:133 (read back with pt_tri_counts; one atomic
                                             per triangle test)                                      */
#define PT_FLAG_JITTER 0x40u               /* sub-pixel jitter: every sample's camera ray goes through its own
                                             point of the pixel's footprint (box filter); see below    */
#define PT_FLAG_JITTER_TENT 0x80u          /* with PT_FLAG_JITTER only: the point is drawn from the tent of
                                             half-width 1 pixel about the footprint's centre             */

/* ------------------------------------------------- sub-pixel jitter (no counterpart in the reference)
 * Without PT_FLAG_JITTER every camera ray goes through its pixel's lower corner (px/W, py/H), as the reference's do:
 * a pinhole render is not anti-aliased however many samples it takes.  With it every sample draws a point of the
 * film first.  All f32, every operation rounded on its own, no contraction, IEEE division and square root:
 *
 *   per sample, before anything else of the sample:  ua = curand_uniform, ub = curand_uniform
 *   box :  jx = ua                      jy = ub
 *   tent:  t(u) = u < 0.5f ? sqrt(2.0f*u) - 1.0f : 1.0f - sqrt(2.0f - 2.0f*u)        (PT_FLAG_JITTER_TENT)
 *          jx = 0.5f + t(ua)            jy = 0.5f + t(ub)
 *   sx = (float)px + jx                 sy = (float)py + jy
 *
 * and the ray is the unjittered one with sx, sy in the places of (float)px, (float)py:
 *   NULL view (pt_camera_ray's arithmetic):
 *     film = (sx/(float)W - 0.5f, sy/(float)H - 0.5f, dist)
 *     film = (film * -focal)/dist
 *     o    = lo + pos
 *     d    = normalized(film - lo)
 *   with a view: the block under "the oriented camera" above, f = ((sx/(float)W - 0.5f) * film_w, ...), unchanged
 *   otherwise.
 * The tent is sampled by inverting its CDF (filter importance sampling): each sample still belongs to exactly one
 * pixel and has weight 1, so pixels stay independent -- frozen pixels, per-pixel counts and "a pixel with n samples
 * holds the n-sample value" hold as before.
 *
 * Draw order of a sample: ua, ub; then the lens pair u1, u2 if the pixel is a lens pixel (radius != 0 or Morton index
 * 0, unchanged); then the integrator's draws.  Without the flag nothing is drawn and nothing is added: the code and
 * the bits are what they were.  PT_FLAG_JITTER_TENT without PT_FLAG_JITTER is PT_E_INVALID from every entry point
 * that validates params.
 *
 * Consequences:
 *   - A jittered pixel has no sample-invariant camera ray, so the primary-hit memo, the memo the chunks of a split
 *     pixel share and the tile kernel's memo are off, as if PT_FLAG_NO_PRIMARY_CACHE were set (that flag stays legal
 *     and changes nothing).  pt_stats.rays_reference keeps its meaning.
 *   - pt_render_features*: with PT_FLAG_JITTER in params->flags the feature ray goes through the footprint's centre,
 *     jx = jy = 0.5f in the arithmetic above, box and tent alike, so the guide buffers sit under the image they guide
 *     and not half a pixel off.  Without the flag the ray is the corner ray, as before (no other flag is looked at).
 *   - Everything that takes pt_params takes the two flags: pt_render*, _device, _async; pt_render_group / _multi;
 *     pt_accum_create*; pt_accum_save / _load and pt_session_save / _load through the stored params (the file
 *     formats do not change); all of these with a view as well.
 *
 * Host helpers (no device; the host's copies of the device functions, as pt_camera_ray_view is):
 *   pt_jitter_offset      (jx, jy) of the draws (ua, ub) for `flags` (only the two jitter bits are looked at):
 *                         (0, 0) without PT_FLAG_JITTER; PT_E_INVALID for PT_FLAG_JITTER_TENT alone or a null out.
 *   pt_camera_ray_jitter  the ray of pixel `idx` (Morton) through (px + jx, py + jy); jx = jy = 0 is
 *                         pt_camera_ray_view exactly (with a NULL view, the signs of zeros included). */
int pt_jitter_offset(uint32_t flags, float ua, float ub, float* jx, float* jy);
void pt_camera_ray_jitter(const pt_camera* cam, const pt_view* view /* NULL ok */, uint32_t idx, float jx, float jy,
                          int lens, float u1, float u2, pt_vec3* origin, pt_vec3* dir);

typedef struct {
    int32_t width, height;   /* image size (IMAGE_WIDTH/HEIGHT, kernel.cu:28-29)                    */
    int32_t spp;             /* samples per pixel = the reference's NUM_SAMPLES - 1 (kernel.cu:709) */
    int32_t bounces;         /* NUM_BOUNCES (kernel.cu:33), integrator 0 only, 1..64                 */
    int32_t integrator;      /* PT_INTEGRATOR_*                                                     */
    uint32_t flags;          /* PT_FLAG_*                                                           */
    uint64_t seed;           /* curand_init seed (kernel.cu:532 uses 1234)                          */
    int32_t shard_index;     /* this renderer's shard in [0, shard_count)                           */
    int32_t shard_count;     /* image tiles (tile_w x tile_h) are dealt round-robin: tile t -> shard
                                t % count, tiles numbered row-major                                 */
    int32_t pixel_order;     /* PT_ORDER_*: how the output buffer is indexed                        */
    int32_t tile_w, tile_h;  /* shard tile size in pixels: 0 = 8; multiples of 8 up to 256           */
} pt_params;

/* pt_params.pixel_order.  SCANLINE: pixel (x,y) at out[(y*W + x)*3 + k].  MORTON: at
 * out[mortonPxltoI(x,y)*3 + k] -- the reference's own imgBuff indexing (drawPixel writes
 * imgBuff[idx] with idx the Morton index, kernel.cu:543,552; the PPM loop reads
 * imgBuffer_host[cam.mortonPxltoI(x,y)], kernel.cu:771), defined only where the reference's is:
 * square power-of-two images (others: PT_E_INVALID). */
#define PT_ORDER_SCANLINE 0
#define PT_ORDER_MORTON 1

/* Empty shards.  shard_count need not fit the image: a shard with shard_index >= the number of tiles (an 8-GPU job
 * on a small preview image) is legal wherever a shard is taken, and owns no pixel.  Nothing is launched for it:
 *   pt_render                  an all-zero image; stats samples, rays_traced, rays_reference, rays_nominal, work_units
 *                              and split_pixels are 0, seconds and kernel_ms the (finite) time of the empty render
 *   pt_render_device, pt_render_features_device, pt_noise_map_device, pt_noise_variance_device, d_out of pt_accum_add
 *                              the buffer is left untouched (the host variants return their "outside the shard" value
 *                              for every pixel)
 *   pt_accum_add(spp)          succeeds with zero stats; pt_accum_samples still advances by spp (no pixel is frozen);
 *                              pt_accum_read and pt_accum_counts give zeros
 *   pt_accum_freeze            a no-op whatever the mask; pt_accum_active gives *n_out = 0
 *   pt_accum_save / _load      the header (which alone names the shard) plus W*H all-zero records
 *   pt_noise_update            pixels = converged = 0 and every bin 0; samples and batches advance as usual
 *   pt_noise_freeze            *newly_frozen = *active = 0
 *   pt_accum_add_until         stops with stopped_converged = 1 after exactly min_batches passes: 0 >= ceil(quantile * 0)
 *   pt_accum_add_adaptive      no pixel is active: no pass, stopped_converged = 1, active = samples_total = 0,
 *                              pt_accum_samples unchanged
 *   pt_session_save            the header (flags without PT_SESSION_COUNTS: no pixel can be frozen; frozen pixels 0) plus
 *                              all-zero sections: A, and C when an estimator is saved
 *   pt_session_load            loads such a file back as such an accumulator (and estimator)
 * and the next render on the context is unaffected. */

typedef struct {
    double seconds;            /* device time of the whole render (hipEvent pair around every
                                  launch: RNG seeding, integration, split-pixel finalisation)     */
    double kernel_ms;          /* device time of the integration kernel alone, in ms (its own
                                  hipEvent pair)                                                  */
    uint64_t samples;          /* pixel samples computed                                         */
    uint64_t rays_traced;      /* trace() calls actually executed on the device                   */
    uint64_t rays_reference;   /* trace() calls the reference integrator performs for the same
                                  samples (differs from rays_traced by the primary-ray cache and
                                  the dead-path skip)                                             */
    uint64_t rays_nominal;     /* pixels*spp*(bounces+1) over THIS render's pixels (its shard; the
                                  whole image for pt_render_group): the kernel.cu:757 formula, in
                                  64-bit                                                          */
    uint64_t node_tests;       /* node records fetched (PT_FLAG_COUNT only)                       */
    uint64_t tri_tests;        /* triangle records tested (PT_FLAG_COUNT only)                    */
    uint64_t walk_lane_slots;  /* PT_FLAG_COUNT, wavefront kernel: 64 x BVH-walk iterations; with
                                  node_tests gives the SIMD lane utilisation of the walk          */
    uint64_t leaf_steps;       /* PT_FLAG_COUNT: walk steps that tested a triangle                */
    uint64_t shade_lane_slots; /* PT_FLAG_COUNT, wavefront kernel: 64 x shading passes            */
    uint64_t accel_fallbacks;  /* rays taking the exact reference-BVH walk: outside the fast-path
                                  preconditions, or the BVH4 winner failed the reference-parent
                                  check                                                          */
    uint64_t walk_cycles;      /* PT_FLAG_COUNT, wavefront kernel: wave-clock cycles spent in walk
                                  phases, summed over waves                                     */
    uint64_t shade_cycles;     /* same for shading (+ refill) phases                              */
    uint64_t spill_entries;    /* PT_FLAG_COUNT, BVH4 walk: stack entries pushed beyond the 16-entry
                                  per-lane LDS ring into the lane's HBM spill column (the reference's
                                  fixed stack[64] of kernel.cu:114 has no such tier)              */
    uint64_t lds_node_tests;   /* PT_FLAG_COUNT, wavefront kernel: the node_tests served by the copy
                                  of the BVH4's top nodes in LDS (no vector-memory fetch)         */
    uint64_t work_units;       /* wavefront kernel: work units of this render (whole pixels + sample
                                  chunks of split pixels); 0 for the tile kernel                  */
    uint64_t split_pixels;     /* wavefront kernel: pixel slots split into sample chunks          */
} pt_stats;

/* Host-only diagnostic: builds the render path's private acceleration structure for `scene`
 * exactly as pt_create does (SAH BVH collapsed to BVH4) and returns an FNV-1a digest
 * of it, its BVH4 node count and depth.  Used to check that the parallel host build is
 * deterministic. */
int pt_accel_digest(const pt_scene* scene, uint64_t* digest, uint32_t* num_nodes4, int32_t* depth4);

/* Upload a scene to HIP device `device` (ordinal among visible devices). */
pt_ctx* pt_create(const pt_scene* scene, int device, int* err);

/* Render into a HOST buffer out_rgb[W*H*3] (fp32 mean radiance, in params->pixel_order).  Pixels
 * outside this shard are written as 0.  Blocking.  The image leaves the device through a pinned
 * staging buffer owned by the context (one DMA, then a parallel host copy into out_rgb). */
int pt_render(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, float* out_rgb, pt_stats* stats);
/* The same through an oriented camera (pt_view above; NULL = pt_render).  So for every *_view entry point below. */
int pt_render_view(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, const pt_view* view, float* out_rgb,
                   pt_stats* stats);

/* Same into a DEVICE buffer d_out[W*H*3] on `stream` (a hipStream_t, NULL = default stream).
 * Only this shard's pixels are written; the caller zero-fills the buffer (a multi-GPU job
 * then sums the shards with one RCCL reduce).  Blocking (it waits for its own events). */
int pt_render_device(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, float* d_out,
                     void* stream, pt_stats* stats);
int pt_render_device_view(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, const pt_view* view, float* d_out,
                          void* stream, pt_stats* stats);

/* pt_render_device in two halves: _async enqueues the whole render on `stream` and returns at once (up
 * to 2 renders in flight per context, each with its own work buffers: two renders on two streams may run
 * concurrently -- the next frame's blocks start while this one's last waves drain); pt_render_wait waits
 * for the OLDEST render in flight and returns its stats.  Frames queued back to back leave the GPU no
 * idle gap between them (the bench's frame loop).  pt_render_device = _async + wait, and refuses to run
 * while renders are in flight, as do pt_trace* and pt_tri_counts. */
int pt_render_device_async(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, float* d_out, void* stream);
int pt_render_device_view_async(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, const pt_view* view,
                                float* d_out, void* stream);
int pt_render_wait(pt_ctx* ctx, pt_stats* stats);

/* ------------------------------------------------- resumable accumulation (progressive rendering)
 * The reference renders progressively: one drawPixel launch per sample (kernel.cu:702-737), the
 * whole render state in two device buffers between launches -- randState_device, the per-pixel
 * XORWOW state (setupCurand, kernel.cu:527-533), and imgBuffer_device, the per-pixel f64 running
 * mean m*(n-1)/n + L/n (kernel.cu:535-553).  An accumulator keeps exactly that state (48 B per
 * pixel: 24 B XORWOW after the pixel's last finished sample, 24 B f64 mean) on the context's device,
 * and pt_accum_add runs the NEXT spp samples of every pixel on top of it -- a pass of the wavefront
 * kernels that continues each pixel's stream and mean.  A render built up in passes equals the
 * one-shot pt_render of the same total in every bit; the state can be written to a file and loaded
 * into another process.  The reference's loop, kernel.cu:709-736, is
 *     for (i = 1; i < NUM_SAMPLES; ++i) pt_accum_add(acc, 1, NULL, NULL, NULL);
 *
 * pt_accum_create fixes everything in `params` except spp (ignored) and the camera, validates them
 * as pt_render_device_async does, and allocates the state with 0 samples done.  Accumulation runs on
 * the wavefront kernels only: both integrators, flags drawn from 0, PT_FLAG_NO_DEAD_PATH_SKIP,
 * PT_FLAG_NO_PRIMARY_CACHE, PT_FLAG_JITTER and PT_FLAG_JITTER_TENT.  Whatever would take another kernel is refused here with PT_E_INVALID
 * (never a silent fall-back): PT_FLAG_REFERENCE_TRAVERSAL, PT_FLAG_REFERENCE_BVH, PT_FLAG_COUNT, a
 * camera farther than 64 scene extents from the origin, integrator 1 with PT_HEAD_WF=0, a
 * non-default PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES.  An accumulator belongs to one context (one
 * shard: shard_index / shard_count are fixed params; a multi-GPU job keeps one accumulator per
 * shard and reduces d_out as for pt_render_device) and is destroyed before it.
 *
 * pt_accum_add renders samples N+1 .. N+spp of every pixel of the shard (N = pt_accum_samples).
 * Blocking; refuses to run while asynchronous renders are in flight.  d_out: a DEVICE buffer
 * W*H*3 on `stream` or NULL; if given, this shard's pixels receive the fp32 mean after N+spp
 * samples (params->pixel_order), other pixels are untouched.  `stats` describes this pass alone
 * (the primary-hit memo is re-traced once per pixel per pass, so rays_traced summed over passes may
 * exceed a one-shot render's; samples and rays_reference do not).  spp = 0: a no-op.  A total
 * beyond 2^30 - 1 samples is PT_E_INVALID.  If a pass fails, the state is undefined: destroy it.
 *
 * pt_accum_read copies to HOST buffers (either may be NULL), both W*H*3 in params->pixel_order,
 * pixels outside the shard 0: out_rgb the fp32 mean as pt_render returns it, out_mean the f64
 * running mean itself (the reference's imgBuffer; pt_write_ppm_f64 takes it).
 *
 * Checkpoint file (pt_accum_save / pt_accum_load / pt_accum_file_info), little-endian:
 *   offset  0  char[8]   magic "PTACCUM\0"
 *           8  uint32    format version (1)
 *          12  uint32    header size in bytes (128)
 *          16  pt_params 56 B as laid out above (seed at +24; spp = 0; 4 bytes of zero padding last)
 *          72  pt_camera 32 B
 *         104  int64     samples done
 *         112  uint64    FNV-1a digest of the scene arrays the context was created from (verts, tris,
 *                        mats, lights, total_light_area, bvh, spheres, in that order)
 *         120  uint32    num_tris
 *         124  uint32    num_spheres
 *         128  W*H records in scanline order (pixel (x,y) at y*W + x), 48 B each: six uint32
 *              (XORWOW v0..v4, d) and three f64 (the mean r, g, b); pixels outside the shard all zero.
 * pt_accum_load fails with PT_E_IO for an unreadable or truncated file, PT_E_INVALID for a wrong
 * magic, version, header size or a file longer than its records, PT_E_SCENE when the digest or the
 * counts differ from the context's scene.  pt_accum_file_info is host-only: it reads and validates
 * the header and the file's size; any out pointer may be NULL. */
typedef struct pt_accum pt_accum;
pt_accum* pt_accum_create(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, int* err);
/* With an oriented camera: the accumulator keeps its view for life, as it keeps its camera.  pt_accum_view reads it
 * back: *has_view = 1 and *out the view, or *has_view = 0 (either pointer may be NULL).  pt_accum_save refuses an
 * accumulator with a view (PT_E_INVALID: format version 1's 32-byte camera has no room; pt_session_save holds it). */
pt_accum* pt_accum_create_view(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, const pt_view* view, int* err);
int pt_accum_view(const pt_accum* acc, pt_view* out, int* has_view);
int pt_accum_add(pt_accum* acc, int32_t spp, float* d_out, void* stream, pt_stats* stats);
int64_t pt_accum_samples(const pt_accum* acc);
int pt_accum_read(pt_accum* acc, float* out_rgb, double* out_mean);
int pt_accum_save(pt_accum* acc, const char* path);
pt_accum* pt_accum_load(pt_ctx* ctx, const char* path, int* err);
int pt_accum_file_info(const char* path, pt_params* params, pt_camera* cam, int64_t* samples, uint64_t* scene_digest);
void pt_accum_destroy(pt_accum* acc);

/* --------------------------------------------- per-pixel noise estimates and a convergence stop
 * An accumulator can add samples forever; a pt_noise attached to it says how noisy the image still is.
 * The f64 mean before and after a pass gives the mean of that pass's samples, and the spread of those
 * pass means (batch means) is an unbiased estimate of the variance of the pixel mean -- with no change
 * to any render kernel: pt_accum_add behaves exactly as without an estimator.
 *
 * pt_noise_create attaches an estimator to `acc` (at most one live estimator per accumulator; it is
 * destroyed before the accumulator).  Its window starts at the accumulator's state at that moment:
 * prev = the current mean, n_start = n0 = pt_accum_samples, batches = 0, window weight W = 0 -- so a
 * resumed or half-finished accumulator gets one too.  It holds 40 B per work slot on the accumulator's
 * device (f64 planes prev[3], mu, m2 in the accumulator's slot order) plus a 4-B slot -> pixel index.
 *
 * The arithmetic (all f64, every operation rounded on its own, no contraction, IEEE division; integers
 * convert to double exactly; max(a, b) is `b > a ? b : a`):
 *   update  pt_noise_update at n1 = pt_accum_samples folds when n1 > n0 (n0: the sample count at the last
 *           fold, or n_start).  With s = n1 - n0 and m1 the accumulator's mean, per pixel:
 *             b[k] = (m1[k]*n1 - prev[k]*n0) / s            k = r, g, b: the mean of the pass's samples
 *             y    = (0.2126*b[0] + 0.7152*b[1]) + 0.0722*b[2]
 *             Wn   = W + s;   d = y - mu;   mu' = mu + d*(s/Wn);   m2' = m2 + (s*d)*(y - mu');   prev = m1
 *           then W = Wn, n0 = n1, batches += 1.  When n1 == n0 nothing is folded; the summary is recomputed
 *           with the given parameters (ask again with another tol).
 *   error   batches >= 2:  var = m2 / ((batches-1) * W);  den = max(y_floor, mu);  rel2 = var / (den*den)
 *           -- the squared relative standard error of the mean luminance over the window (no square root).
 *           batches < 2:   rel2 = +inf for every pixel of the shard.
 *   summary a pixel is converged iff rel2 <= (double)tol*(double)tol (NaN and inf are not).  hist[] bins
 *           r = (float)rel2, tested in this order: r != r -> 63; !(r > 0) -> 0; inf -> 63; otherwise
 *           clamp(((bits >> 23) & 255) - 127 + 48, 1, 62).  Work slots outside the image are not pixels.
 *           All counts are integers: the summary does not depend on the reduction order.
 *   map     (float)rel2 at the pixel's index in the accumulator's pixel_order.  pt_noise_map (host buffer,
 *           W*H) writes pixels outside the shard as 0; pt_noise_map_device (device buffer on `stream`)
 *           leaves them untouched.  pt_noise_read returns mu and m2 the same way (host, W*H each, pixels
 *           outside the shard 0; either pointer may be NULL).
 * Every call blocks.  PT_E_INVALID: null arguments, tol or y_floor not finite or <= 0, asynchronous
 * renders in flight, a second estimator on one accumulator.
 *
 * pt_accum_add_until is a host loop over the two steps: while pt_accum_samples < max_samples it calls
 * pt_accum_add(min(pass_spp, max_samples - samples), d_out, stream) and then pt_noise_update, and stops
 * with stopped_converged = 1 as soon as batches >= min_batches and
 * converged >= (uint64_t)ceil((double)quantile * (double)pixels); otherwise at max_samples with
 * stopped_converged = 0.  `passes` counts the passes it ran and `last` is the summary of its last
 * update (with no pass to run: one update, which only re-summarises when nothing is unfolded).
 * PT_E_INVALID: pass_spp < 1, quantile outside (0, 1], min_batches < 2, max_samples < 0 or beyond the
 * accumulator's 2^30 - 1, an estimator of another accumulator.  Whatever it returns, the accumulator's
 * image is the plain render's at that sample count. */
typedef struct pt_noise pt_noise;
typedef struct {
    float tol;      /* a pixel is converged when its relative standard error is <= tol; > 0, finite */
    float y_floor;  /* luminance below which the error is taken relative to y_floor; > 0, finite    */
} pt_noise_params;
void pt_noise_defaults(pt_noise_params* p);   /* {0.05f, 0.01f}: design choices, not measurements */
typedef struct {
    int64_t samples;      /* pt_accum_samples at this update                       */
    int32_t batches;      /* passes folded so far                                  */
    uint64_t pixels;      /* pixels of this shard                                  */
    uint64_t converged;   /* of those, pixels with rel2 <= tol*tol                 */
    uint64_t hist[64];    /* pixels per power-of-two bin of (float)rel2, see above */
} pt_noise_summary;

pt_noise* pt_noise_create(pt_accum* acc, int* err);
int pt_noise_update(pt_noise* noise, const pt_noise_params* np, void* stream, pt_noise_summary* out);
int pt_noise_read(pt_noise* noise, double* mu, double* m2);
int pt_noise_map(pt_noise* noise, const pt_noise_params* np, float* rel2 /* host */);
int pt_noise_map_device(pt_noise* noise, const pt_noise_params* np, float* d_rel2, void* stream);
void pt_noise_destroy(pt_noise* noise);

typedef struct {
    int32_t pass_spp;       /* samples per pass, >= 1                                     */
    int32_t max_samples;    /* stop at this total (pt_accum_samples) at the latest        */
    int32_t min_batches;    /* >= 2: no stop before this many folded passes               */
    float quantile;         /* in (0, 1]: the fraction of the pixels that must converge   */
    pt_noise_params noise;
} pt_converge_params;
typedef struct {
    int32_t passes;             /* passes this call ran                  */
    int32_t stopped_converged;  /* 1: the quantile converged; 0: the cap */
    pt_noise_summary last;
} pt_converge_result;
int pt_accum_add_until(pt_accum* acc, pt_noise* noise, const pt_converge_params* cp, float* d_out, void* stream,
                       pt_converge_result* result);

/* ------------------------------------------------- adaptive sampling: freeze converged pixels
 * pt_accum_add_until stops all or nothing; until then every pass samples every pixel.  A pixel of an
 * accumulator can instead be FROZEN: it is never sampled again, and pt_accum_add renders the others only.
 * Pixels are independent (each has its own XORWOW stream, seeded by its Morton index), so a pixel with n
 * samples holds exactly the f64 mean a plain render has after n samples, in every bit, whatever was frozen
 * around it and whenever.  Freezing is permanent (no unfreeze): every ACTIVE (not frozen) pixel therefore
 * has exactly pt_accum_samples samples, which stays the largest count in the image, and a frozen pixel has
 * the count it was frozen at.
 * Stopping a pixel on its own estimated error biases the image slightly (a pixel whose samples happened to
 * agree stops early), as with every adaptive sampler; nothing here corrects for it.
 *
 * pt_accum_freeze  mask: HOST buffer, W*H bytes in params->pixel_order; non-zero freezes the pixel at the
 *                  current count, zero changes nothing (it never unfreezes); pixels outside the shard are
 *                  ignored.  Legal at 0 samples: such a pixel stays at mean 0 with count 0.  Blocking.
 * pt_accum_counts  out: HOST buffer, W*H uint32 in pixel_order: each pixel's sample count, 0 outside the shard.
 * pt_accum_active  the active pixels' scanline ids y*W + x in work order: pt_shard_pixels' order with the
 *                  frozen pixels removed.  out = NULL: only *n_out; cap < *n_out is PT_E_INVALID.  The list
 *                  is the one the passes use, built on the device (an ordered compaction of the frozen
 *                  flags, rebuilt only when the frozen set changed); this call reads it back.
 * pt_accum_add     on an accumulator that never had a pixel frozen: unchanged, the same launches.  Once a
 *                  pixel is frozen: spp more samples of the active pixels only, each one whole-pixel work
 *                  unit; stats->samples = active * spp; d_out receives the active pixels' new means and
 *                  frozen pixels keep what the buffer held.  With no active pixel: a no-op (zero stats,
 *                  pt_accum_samples unchanged).
 * pt_accum_read    unchanged: every pixel's mean, at its own count.
 * pt_accum_save    with unequal counts PT_E_INVALID: format version 1 holds a single sample count (a session file,
 *                  pt_session_save below, holds them all).
 *
 * The estimator with per-pixel counts.  Once the accumulator has a frozen pixel, each pixel q carries its
 * own window weight W_q and batch count b_q (two uint32 planes, allocated then, both starting from the
 * scalar W and batches, which described every pixel until that moment).  With n_q the pixel's count (the
 * count it was frozen at, or n1 = pt_accum_samples for an active pixel) and n0 the scalar count at the
 * last fold, pt_noise_update at n1 > n0 folds pixel q iff n_q > n0:
 *             s    = n_q - n0
 *             b[k] = (m1[k]*n_q - prev[k]*n0) / s
 *             y    = (0.2126*b[0] + 0.7152*b[1]) + 0.0722*b[2]
 *             Wn   = W_q + s;   d = y - mu;   mu' = mu + d*(s/Wn);   m2' = m2 + (s*d)*(y - mu');   prev = m1
 *           then W_q = Wn, b_q += 1; afterwards n0 = n1 and the scalars W, batches advance as before (they
 *           remain the active pixels' values; the summary's `batches` is the scalar).
 *   error   b_q >= 2:  var = m2 / ((b_q-1) * W_q);  den = max(y_floor, mu);  rel2 = var / (den*den);
 *           b_q < 2:   rel2 = +inf.
 * For an active pixel this is the arithmetic above bit for bit; a frozen pixel's state stops at its last
 * fold (a pixel frozen between two passes that one update folds together folds once more, with its own
 * shorter s).  Summary, histogram, map and pt_noise_read are as before, over all pixels of the shard.  An
 * estimator of an accumulator without frozen pixels runs the scalar sweep, unchanged.
 *
 * pt_noise_freeze freezes every active pixel with rel2 <= (double)tol*(double)tol at the current count, in
 * one sweep on the device (the error map never reaches the host); *newly_frozen and *active (the pixels
 * still active afterwards) come back.  Blocking; PT_E_INVALID as for pt_noise_update.
 *
 * pt_accum_add_adaptive (argument checks as pt_accum_add_until): while pt_accum_samples < max_samples and
 * a pixel is active it calls pt_accum_add(min(pass_spp, max_samples - samples)), pt_noise_update and, once
 * batches >= min_batches, pt_noise_freeze; it stops with stopped_converged = 1 when (batches >=
 * min_batches and) that update's converged >= (uint64_t)ceil((double)quantile * (double)pixels), or when
 * no pixel is active; otherwise at max_samples with stopped_converged = 0.  `last` is the summary of the
 * last update (taken before that pass's freeze), `active` the pixels still active, `samples_total` the sum
 * of the per-pixel counts (what the loop and everything before it sampled in this shard).  With no pass to
 * run: one update, as pt_accum_add_until. */
typedef struct {
    int32_t passes;             /* passes this call ran                              */
    int32_t stopped_converged;  /* 1: the quantile converged or nothing is active    */
    pt_noise_summary last;
    uint64_t active;            /* pixels still sampled                              */
    uint64_t samples_total;     /* sum of the per-pixel sample counts                */
} pt_adaptive_result;
int pt_accum_freeze(pt_accum* acc, const uint8_t* mask);
int pt_accum_counts(pt_accum* acc, uint32_t* out);
int pt_accum_active(pt_accum* acc, uint32_t* out, uint32_t cap, uint64_t* n_out);
int pt_noise_freeze(pt_noise* noise, const pt_noise_params* np, void* stream, uint64_t* newly_frozen, uint64_t* active);
int pt_accum_add_adaptive(pt_accum* acc, pt_noise* noise, const pt_converge_params* cp, float* d_out, void* stream,
                          pt_adaptive_result* result);

/* ------------------------------------------------- session files: checkpoint and resume adaptive renders
 * The checkpoint file of pt_accum_save (format version 1) holds the accumulator alone, at a single sample count.  A
 * SESSION FILE holds the whole progressive state of one shard: the accumulator, the per-pixel frozen-at counts of
 * adaptive sampling and, optionally, the attached noise estimator with its window -- so an adaptive or until-error
 * render that is saved, destroyed and loaded again (in another process, on another context of the same scene)
 * continues exactly as if it had never stopped: every later image, count, active list, estimator state, summary,
 * error map and variance map agrees in every byte.  pt_accum_save / _load / _file_info and format version 1 are
 * unchanged, including their refusals.
 *
 * Session file (pt_session_save / pt_session_load / pt_session_file_info), little-endian; the magic is format 1's,
 * so a reader of format 1 answers "format version 2, this build reads 1":
 *   offset  0  char[8]   magic "PTACCUM\0"
 *           8  uint32    format version (2)
 *          12  uint32    header size in bytes (192)
 *          16  pt_params 56 B (seed at +24; spp = 0; 4 bytes of zero padding last)      \
 *          72  pt_camera 32 B                                                            |
 *         104  int64     samples done (pt_accum_samples: the active pixels' count)      |  exactly format 1's
 *         112  uint64    FNV-1a digest of the scene arrays, as in format 1              |  fields
 *         120  uint32    num_tris                                                        |
 *         124  uint32    num_spheres                                                    /
 *         128  uint32    flags: PT_SESSION_COUNTS 0x1 (a pixel was ever frozen: section B), PT_SESSION_NOISE 0x2 (an
 *                        estimator: section C), PT_SESSION_NOISE_PER_PIXEL 0x4 (its W_q / b_q planes carry the state:
 *                        section D; only with 0x2); every other bit 0
 *         132  uint32    0
 *         136  int64     noise n0       the sample count at the estimator's last fold   \
 *         144  f64       noise W        its window weight                               |  0 without PT_SESSION_NOISE
 *         152  int32     noise batches  the passes it has folded                        /
 *         156  uint32    0
 *         160  uint64    frozen pixels of this shard (0 without PT_SESSION_COUNTS)
 *         168  24 bytes of zero
 *         192  the sections, in this order, each W*H entries in scanline order (pixel (x,y) at y*W + x), pixels
 *              outside the shard all zero:
 *                A  always                       48 B  format 1's record: six uint32 (XORWOW v0..v4, d) and three f64
 *                                                      (the mean r, g, b); all zero at 0 samples
 *                B  PT_SESSION_COUNTS             4 B  uint32: 0xffffffff = the pixel is active (its count is `samples`),
 *                                                      else the count the pixel was frozen at
 *                C  PT_SESSION_NOISE             40 B  five f64: the estimator's prev r, g, b, mu, m2
 *                D  PT_SESSION_NOISE_PER_PIXEL    8 B  two uint32: W_q, b_q
 * An accumulator with a view (pt_accum_create_view) is written as FORMAT VERSION 3, recognised by its version and
 * header size together (no flag bit says so); one without a view is written as version 2, byte for byte as before:
 *           8  uint32    format version (3)
 *          12  uint32    header size in bytes (256)
 *          16  ...       bytes 16..191 exactly version 2's fields
 *         192  pt_view   44 B: right, up, back, film_w, film_h
 *         236  20 bytes of zero
 *         256  the sections, as above
 * pt_session_load and pt_session_file_info read both versions; a stored view that is not valid (pt_view above), a
 * non-zero byte in 236..255, version 3 with another header size than 256 and version 2 with another than 192 are
 * PT_E_INVALID.  pt_session_file_view reads the view of a file (validated as pt_session_file_info validates the
 * file): *has_view = 1 and *out the view for version 3, *has_view = 0 for version 2; either pointer may be NULL.
 * With no pixel ever frozen and no estimator (flags 0), section A is byte for byte the records pt_accum_save writes
 * for the same accumulator.
 *
 * pt_session_save writes `acc` and, when `noise` is not NULL, its estimator.  Blocking.  The sections are laid out
 * on the device (pt_session.hip: one pack kernel over the state planes) and leave it in one copy through a pinned
 * staging buffer, which grows on demand inside the context and is freed by pt_destroy.  PT_E_INVALID: a null acc or
 * path, a `noise` that is not acc's live estimator, asynchronous renders in flight; PT_E_IO: the file cannot be
 * written.  Legal at any moment between two calls: between pt_accum_add and pt_noise_update the estimator's n0 and
 * prev are saved as they stand, and the next update after a load folds what the uninterrupted run would fold;
 * legal at 0 samples, with or without pixels frozen at 0.  Section D is written when the estimator's per-pixel
 * planes are live (after its first call on an accumulator with a frozen pixel); before that the scalars W and batches
 * describe every pixel, as they do after the load.
 *
 * pt_session_load creates the accumulator on `ctx` (*acc_out; every fixed parameter and the camera come from the
 * file) and, when the file has an estimator and noise_out is not NULL, an estimator attached to it (*noise_out) with
 * batches, W, n0, the five f64 planes and the W_q / b_q planes as saved: it continues the saved window, it does not
 * open a fresh one.  *has_noise (may be NULL) says whether the file has an estimator.  With noise_out = NULL the
 * estimator's sections are skipped and pt_noise_create on the accumulator opens a fresh window as always.  After a
 * load with PT_SESSION_COUNTS the accumulator is in the state pt_accum_freeze leaves: the active list is rebuilt on
 * first use.  Destroy the estimator before the accumulator, as any other.  On failure both outputs are NULL and
 * nothing stays allocated:
 *   PT_E_IO       an unreadable or truncated file
 *   PT_E_INVALID  null ctx, path or acc_out; asynchronous renders in flight; a wrong magic, version or header size;
 *                 unknown flag bits; 0x4 without 0x2; 0x4 without 0x1 (the per-pixel planes exist only beside frozen
 *                 pixels: pt_session_save never writes one without the other); noise batches < 0; noise n0 outside
 *                 0..samples; a noise W outside 0..samples (NaN included); a file longer than its sections; a section-B word of a pixel of the shard that
 *                 is neither 0xffffffff nor <= samples; a header `frozen pixels` that disagrees with section B (both
 *                 counted on the device while the sections are unpacked); parameters pt_accum_create refuses
 *   PT_E_SCENE    the digest or the counts differ from the context's scene
 *
 * A refusal of the file's parameters by pt_accum_create's validation comes back under pt_session_load's name.
 *
 * pt_session_file_info is host-only: it reads and validates the header and the file's size (every check above that
 * does not need the sections or a context).
 *
 * The staging (device and pinned host, each the size of the largest session saved or loaded on the context so far:
 * 100 B per pixel of the image with all four sections, 207 MB at 1920x1080) is kept for the next call and never
 * shrinks; pt_destroy frees it, like the denoiser's scratch.
 * Measurement hook: with PT_TIMING set in the environment, pt_session_save / _load and pt_accum_save / _load print
 * the host wall time of each of their stages (state <-> host buffer, file write / read) to stderr, as pt_create
 * prints its phases; unset, nothing is printed and nothing else changes. */
#define PT_SESSION_COUNTS 0x1u
#define PT_SESSION_NOISE 0x2u
#define PT_SESSION_NOISE_PER_PIXEL 0x4u
typedef struct {
    pt_params params;         /* spp = 0 */
    pt_camera cam;
    int64_t samples;
    uint64_t scene_digest;
    uint32_t flags;           /* PT_SESSION_* */
    int32_t noise_batches;
    int64_t noise_n0;
    double noise_W;
    uint64_t frozen_pixels;
} pt_session_info;            /* 136 B */
int pt_session_save(pt_accum* acc, pt_noise* noise /* NULL: no estimator section */, const char* path);
int pt_session_load(pt_ctx* ctx, const char* path, pt_accum** acc_out, pt_noise** noise_out /* may be NULL */, int* has_noise);
int pt_session_file_info(const char* path, pt_session_info* info);
int pt_session_file_view(const char* path, pt_view* out, int* has_view);

/* ------------------------------------------------- the variance map of the image's mean
 * What the variance-guided denoiser (pt_denoise_guided, below) takes: per pixel q the estimated variance of the
 * mean luminance of ALL of the pixel's n_q samples, in f64 with every operation rounded on its own as above:
 *   b_q >= 2:  v = m2 / ((double)(b_q - 1) * (double)n_q);  the map holds (float)v
 *   b_q <  2:  the map holds +inf.
 * n_q is the pixel's sample count: pt_accum_samples for an active pixel, the count it was frozen at for a frozen
 * one.  b_q and m2 are the scalar batches and the pixel's m2, or the per-pixel values once the accumulator has a
 * frozen pixel.  This is the window variance m2 / ((b-1) * W) scaled by W / n: the variance of the mean of all n
 * samples if they are independent, so an estimator attached late (or after a resume) does not overstate the noise
 * of the image; it equals the window variance when the window started at 0 samples.
 * Indexing is pt_noise_map's: the accumulator's pixel_order; pt_noise_variance (host buffer, W*H) writes pixels
 * outside the shard as 0, pt_noise_variance_device (device buffer on `stream`) leaves them untouched.  Both block
 * and fold nothing: they read the state as of the last pt_noise_update.  PT_E_INVALID: null arguments,
 * asynchronous renders in flight. */
int pt_noise_variance(pt_noise* noise, float* var /* host, W*H */);
int pt_noise_variance_device(pt_noise* noise, float* d_var, void* stream);

/* The reference's trace() (kernel.cu:112-161) for n rays given as rays[6n] = {o.xyz, d.xyz}
 * (host buffers): tri_out[i] = winning ORIGINAL triangle index or -1, t_out[i] = its closestT
 * (MAX_FLOAT = 1e5 on a miss).  flags: 0 = the render path's walk, PT_FLAG_REFERENCE_BVH = the
 * reference's own stack walk on its BVH.  Bit-identical to the reference for both, for every ray
 * with finite components and a non-zero direction.  Blocking.
 * With flags = 0 the walk is chosen per ray: the BVH4 walk for a regular ray inside the Markstein
 * ranges (origin coordinates 0 or in [2^-50, 2^20], direction components 0 or in [2^-100, 2^45],
 * and a scene whose coordinates all are 0 or in [2^-50, 2^20]); the exact culled walk on the
 * reference BVH for a regular ray outside them; and the reference's own stack walk -- slower, it
 * culls nothing -- for a ray that is not regular.  Regular: max |o_k| <= 64 * the scene's extent
 * (its largest absolute coordinate) and d.x*d.x + d.y*d.y + d.z*d.z <= 1 + 2^-10 in float, i.e. an
 * origin no farther out than a plain render's camera may be for the render path's own walk, and a
 * direction no longer than a normalised one. */
int pt_trace(pt_ctx* ctx, uint32_t n, const float* rays, int32_t* tri_out, float* t_out, uint32_t flags);

/* trace() as above, plus diagnostics (either may be NULL):
 *   tri_counts[num_tris]: every triangle test of the walk ADDED to tri_counts[original id] --
 *     the reference's test[k] += 1 (kernel.cu:133); with PT_FLAG_REFERENCE_BVH exactly the
 *     reference's counts for these rays, otherwise the tests the render path's walk performed;
 *   spill_entries: BVH4 stack entries pushed past the per-lane LDS ring into HBM. */
int pt_trace_counts(pt_ctx* ctx, uint32_t n, const float* rays, int32_t* tri_out, float* t_out, uint32_t flags,
                    uint32_t* tri_counts, uint64_t* spill_entries);

/* Per-triangle test counts (n = num_tris entries, by original triangle id) of the ctx's last
 * pt_render / pt_render_device with PT_FLAG_COUNT | PT_FLAG_TRI_COUNTS: the reference's bvhIntersection buffer
 * (kernel.cu:694-697, written to out.csv at :742-750).  With PT_FLAG_REFERENCE_TRAVERSAL |
 * PT_FLAG_NO_PRIMARY_CACHE | PT_FLAG_NO_DEAD_PATH_SKIP the render performs exactly the reference's
 * trace() calls, so these are the reference's counts (without its racy increments and with the
 * last triangle's slot, which the reference's numTris-1 buffer lacks). */
int pt_tri_counts(pt_ctx* ctx, uint32_t* counts, uint32_t n);

/* ------------------------------------------------------------------ ray queries on device buffers
 * A caller's own rays, in DEVICE memory on a stream: the closest hit, and "is anything between these two
 * points?".  Rays are d_rays[6n] = {o.xyz, d.xyz} as pt_trace's.  All three calls block: they wait for their
 * own work on `stream` (NULL = the default stream), as every _device call does.  No device memory is allocated
 * per call: the walks' spill columns grow inside the context as they do for renders.
 *
 * pt_trace_device: pt_trace exactly -- d_tri[i], d_t[i] = (tri, t) of the reference's trace() for every ray with
 * finite components and a non-zero direction, spheres included (ids num_tris + i), t = 1e5 and tri = -1 on a
 * miss.  flags: 0 or PT_FLAG_REFERENCE_BVH, as pt_trace's; with 0 each ray takes the walk pt_trace gives it.
 *
 * pt_occluded*: is the segment of ray i up to tmax[i] blocked?  A definition, not a measurement:
 *     occ[i] = (tri_i >= 0 && t_i < tmax_i) ? 1 : 0          (an f32 compare)
 * with (tri_i, t_i) what pt_trace returns for ray i.  A NaN, zero or negative tmax gives 0; +inf or anything
 * above 1e5 means "any hit"; tmax = NULL means 1e5 for every ray.  The closest hit is not computed: the walk is
 * bounded at tmax and ends at the first hit the reference would also have tested (a first hit it would not have
 * tested sends the ray to the exact walk, whose closest hit is compared); rays outside the fast walk's ranges
 * take their exact walks and compare at the end; spheres are tested only if no triangle decided.  flags must be
 * 0.  Every entry below n is written as a 0 or 1 byte.  pt_occluded: host buffers, staged through a device
 * buffer the context keeps, grows on demand and frees in pt_destroy.
 *
 * Order of the checks, for all three: a null context is PT_E_INVALID; then n == 0 is PT_OK and nothing else is
 * looked at or touched (entries at index n and beyond are never written for any n); then PT_E_INVALID for
 * unknown flag bits, a null buffer (d_tmax / tmax may be NULL) or asynchronous renders in flight; then
 * PT_E_BVH_DEPTH as pt_trace returns it.
 * PT_QUERY_BLOCKS in the environment (read on every call) forces the persistent grid to 1..default blocks; no
 * bit of any answer depends on it. */
int pt_trace_device(pt_ctx* ctx, uint32_t n, const float* d_rays, int32_t* d_tri, float* d_t, uint32_t flags, void* stream);
int pt_occluded_device(pt_ctx* ctx, uint32_t n, const float* d_rays, const float* d_tmax /* n floats, or NULL */,
                       uint8_t* d_occ, uint32_t flags, void* stream);
int pt_occluded(pt_ctx* ctx, uint32_t n, const float* rays, const float* tmax /* or NULL */, uint8_t* occ, uint32_t flags);

/* ------------------------------------------------------------------ renders along caller-supplied rays
 * The integrators run down a ray buffer instead of a camera: any projection (orthographic, fisheye, panorama),
 * irradiance probes, light baking.  No pt_camera and no pt_view is taken.
 *
 * rays holds width * height * 6 floats, {o.xyz, d.xyz} per pixel as pt_trace's, indexed like the image: the ray of
 * pixel (x, y) sits at its index in params->pixel_order (y * width + x, or the Morton index).  Device buffers must
 * be 8-byte aligned.  d_out / out_rgb behave as pt_render_device's / pt_render's: the device call writes only this
 * shard's pixels, the host call writes the others as 0; both block.  The host call stages the rays through a
 * device buffer the context keeps, grows on demand and frees in pt_destroy.
 *
 * Arithmetic (a definition): pixel (x, y) is
 *     rng = curand_init(seed, morton(x, y), 0)
 *     for n = 1..spp:  L = integrator(o, d, rng);  m = m*(n-1)/n + L/n
 * the reference's loop with the camera ray replaced.  No lens draws happen anywhere -- Morton index 0 is not a lens
 * pixel here -- so the integrator's own draws are a sample's only draws.  Rays built with
 * pt_camera_ray(cam, idx, lens = 0, ...) from a radius == 0 camera give pt_render's image in every bit for every
 * pixel except Morton index 0, which in pt_render consumes the reference's two quirk lens draws per sample.  A ray
 * is the same for every sample, so the primary-hit memo works as for a pinhole pixel (PT_FLAG_NO_PRIMARY_CACHE
 * turns it off).  pt_stats keeps its meanings; rays_reference counts the trace() calls of the loop above.
 *
 * Ray classes.  Every one of the width * height rays (not only the shard's) is classified before a render, by the
 * kernel pt_rays_classify_device makes public:
 *     invalid    a non-finite component, or a direction of exactly (0, 0, 0)
 *     regular    max |o_k| <= 64 * the scene's extent and d.x*d.x + d.y*d.y + d.z*d.z <= 1 + 2^-10 in float
 *                (pt_trace's rule)
 *     irregular  every other valid ray
 * A buffer with an invalid ray is refused: PT_E_INVALID, the message names the lowest such pixel, nothing is
 * written.  A buffer with at least one irregular ray sends THE WHOLE RENDER to the tile kernel with the reference's
 * own stack walk, which is exact for every valid ray but much slower -- as a plain render with its camera beyond 64
 * scene extents does; stats->work_units == 0 shows that it happened.  Otherwise the render takes the wavefront
 * kernels, a regular ray outside the Markstein ranges (see pt_trace) taking the exact culled walk per lane.
 * first_invalid is the lowest index of an invalid ray, 0xffffffff when there is none.  pt_rays_classify_device
 * blocks; n == 0 gives all zeros; it is refused while asynchronous renders are in flight.
 *
 * flags: 0, PT_FLAG_NO_DEAD_PATH_SKIP, PT_FLAG_NO_PRIMARY_CACHE, PT_FLAG_REFERENCE_TRAVERSAL and
 * PT_FLAG_REFERENCE_BVH (the last two select the tile kernel, with the reference's walk).  PT_E_INVALID:
 * PT_FLAG_COUNT, PT_FLAG_TRI_COUNTS, PT_FLAG_JITTER, PT_FLAG_JITTER_TENT (there is no film to jitter on), unknown
 * bits.  Both integrators; PT_HEAD_WF=0 puts integrator 1 on the tile kernel.  Shard fields, tile sizes, Morton
 * order, empty shards and split units work as in pt_render_device; every shard of a multi-GPU job is given the whole
 * buffer.  spp == 0 or an empty shard launches no render (invalid rays are still refused first).  Both calls are
 * refused while asynchronous renders are in flight, and there is no asynchronous variant: the classes must reach
 * the host before the launch.  Only the default PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES have kernels: a context created
 * with other values is refused (PT_E_INVALID) where the render would take the wavefront kernels.
 *
 * Accumulators (with noise estimates, the convergence stop and adaptive sampling), masked pixels and feature buffers
 * over a ray buffer: pt_accum_create_rays* and pt_render_features_rays*, below the denoisers.
 *
 * Out of scope: sessions and checkpoints over a ray buffer; pt_render_group / pt_render_multi; temporal reprojection
 * for ray renders; anti-aliasing and depth of field for custom projections (the one per-sample ray source is the
 * cosine hemisphere of pt_render_irradiance*, below); passes from the command line (pt_cli --rays renders one
 * shot). */
typedef struct { uint64_t regular, irregular, invalid; uint32_t first_invalid; uint32_t pad; } pt_ray_classes;
int pt_render_rays_device(pt_ctx* ctx, const pt_params* params, const float* d_rays, float* d_out, void* stream,
                          pt_stats* stats);
int pt_render_rays(pt_ctx* ctx, const pt_params* params, const float* rays /* host */, float* out_rgb /* host */,
                   pt_stats* stats);
int pt_rays_classify_device(pt_ctx* ctx, uint32_t n, const float* d_rays, void* stream, pt_ray_classes* out /* host */);

/* ------------------------------------------------------------------ irradiance renders at caller-supplied points
 * A ray render sends every sample of a pixel down one fixed ray.  An irradiance render gives every sample a fresh
 * direction over the hemisphere of a surface point: lightmap texels, surface probes, light baking.
 *
 * A point buffer holds width * height * 6 floats, {p.xyz, n.xyz} per pixel (position, unit normal), indexed exactly
 * like a ray buffer (params->pixel_order) and 8-byte aligned on the device.  Pixel (x, y) is
 *     rng = curand_init(seed, morton(x, y), 0)
 *     for s = 1..spp:
 *         u1 = uniform(rng); u2 = uniform(rng)
 *         d  = cosineWeightedRay(n, u1, u2)      (kernel.cu:78-99: the device function the bounces already use)
 *         L  = integrator(p, d, rng)
 *         m  = m*(s-1)/s + L/s                   (kernel.cu:551-552)
 * A sample's draws are those of a lens pixel: a pair first, then the integrator's own (integrator 1: 9 draws per
 * sample).  No pixel has a sample-invariant ray, so there is no primary-hit memo of any kind:
 * PT_FLAG_NO_PRIMARY_CACHE is legal and changes nothing, neither the image nor rays_traced.
 *
 * What m is: the cosine-weighted mean of the incoming radiance over n's hemisphere, E / pi for the irradiance E.  A
 * Lambertian texel's outgoing radiance is its albedo times m.
 *
 * p is used as given: the caller lifts it off the surface (the helpers of cudapathtracer_amd.rays take a `lift`
 * along the normal).  The self-hit rule is the integrator's: it zeroes a path whose first hit is nearer than 0.002
 * (closestT -= 0.001; if (closestT < 0.001)), so a point lying in a surface it can see is black along those
 * directions.
 *
 * Point classes.  Every one of the width * height points is classified before a render, by the kernel
 * pt_points_classify_device makes public, into the same pt_ray_classes; all arithmetic is float32:
 *     invalid    a non-finite component, or (n.x*n.x + n.y*n.y) + n.z*n.z outside [1 - 2^-10, 1 + 2^-10] (a normal
 *                far from unit length bends the distribution, a tiny one underflows the tangent: both are refused)
 *     regular    max |p_k| <= 64 * the scene's extent
 *     irregular  every other valid point
 * An invalid point refuses the render (PT_E_INVALID, the lowest such pixel is named, nothing is written).  A single
 * irregular point sends THE WHOLE RENDER to the tile kernel with the reference's walk, as for ray buffers;
 * stats->work_units == 0 shows it.  The direction handed to the walk is normalized(...) in float32, so it is always
 * within pt_trace's length rule.
 *
 * Flags, shard fields, tile sizes, pixel order, empty shards, spp == 0, blocking behaviour, the refusal while
 * asynchronous renders are in flight and the refusal of non-default PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES are
 * pt_render_rays*'s.  The host call stages the points through the context's ray staging buffer.  pt_stats keeps its
 * meanings; rays_reference counts the trace() calls of the loop above.
 *
 * Accumulators over a point buffer (passes, noise estimates, the convergence stop, adaptive sampling, masked texels):
 * pt_accum_create_points*, below the ray accumulators.
 *
 * Out of scope: feature buffers, checkpoints and sessions over a point buffer; pt_render_group / pt_render_multi;
 * other distributions (uniform sphere, cones); passes from the command line (pt_cli --irradiance renders one shot). */
int pt_render_irradiance_device(pt_ctx* ctx, const pt_params* params, const float* d_points, float* d_out, void* stream,
                                pt_stats* stats);
int pt_render_irradiance(pt_ctx* ctx, const pt_params* params, const float* points /* host */, float* out_rgb /* host */,
                         pt_stats* stats);
int pt_points_classify_device(pt_ctx* ctx, uint32_t n, const float* d_points, void* stream, pt_ray_classes* out /* host */);

/* Output step on the GPU (kernel.cu:763-778, color.h:59-71): codes = pt_tonemap_u8(rgb) per
 * channel, identical to the host function (threshold table bisected with the host's libm at
 * pt_create).  _device: device pointers on `stream`, blocking; negative inputs (which the
 * integrator never produces) are written as INT32_MAX for the caller to redo on the host.
 * pt_tonemap: host buffers, negatives handled. */
int pt_tonemap_device(pt_ctx* ctx, const float* d_rgb, int width, int height, int32_t* d_codes, void* stream);
int pt_tonemap(pt_ctx* ctx, const float* rgb, int width, int height, int32_t* codes);

/* ------------------------------------------- primary-hit feature buffers and the preview denoiser
 * What a progressive renderer shows after 1, 2 or 4 samples per pixel is mostly noise.  Two additions
 * turn it into a preview: the per-pixel features of the camera ray's first hit, and a feature-guided,
 * edge-avoiding a-trous filter over the fp32 mean image (hand-written gfx950 kernels, pt_denoise.hip).
 *
 * pt_render_features*: one pt_feature per pixel.  Uses width, height, pixel_order, shard_index,
 * shard_count, tile_w and tile_h of `params` (validated as pt_render_device validates them, including the
 * refusal while asynchronous renders are in flight) and ignores spp, bounces, integrator, seed and flags.
 * The ray of pixel (x, y) is pt_camera_ray(cam, pt_morton_pxl_to_i(x, y), lens = 0, ...) -- a thin-lens
 * camera still gets its pinhole ray, the features are the sharp ones -- traced by the render path's own
 * walk (what pt_trace(flags = 0) runs: the reference's trace() bit for bit, for a camera at any finite
 * position -- one farther than 64 scene extents from the origin gets the slower walk pt_trace gives a
 * ray from there); hit ids as pt_trace's (the
 * original triangle index, num_tris + i for sphere i).  A scene with num_tris + num_spheres >= 2^30 is
 * PT_E_INVALID (the id shares its word with PT_FEATURE_EMISSIVE).  Records are indexed like the image
 * (params->pixel_order).  _device: d_feat is a device buffer of W*H records, 16-byte aligned (PT_E_INVALID
 * otherwise); only this shard's pixels are written, all others are left untouched.
 * Host variant: pixels outside the shard are all zero bytes with prim = -1.  Both block.
 *
 * pt_denoise*: filters the whole width x height image `in` (W*H*3 fp32, as pt_render returns it) guided
 * by `feat`, both and `out` in `pixel_order`; out may equal in.  Blocking; the scratch (64 B per pixel)
 * grows on demand inside the context and is freed by pt_destroy.  Refused while asynchronous renders are
 * in flight.  PT_E_INVALID: null pointers, sizes <= 0, iterations outside 0..8, normal_power_log2
 * outside 0..7, a non-finite or <= 0 sigma_depth, unknown flags, Morton order on a non-square or
 * non-power-of-two image.
 *
 * The filter's arithmetic (all f32, every operation rounded on its own, no contraction, IEEE division;
 * max(a, b) below is `b > a ? b : a`, so a NaN second operand gives the first):
 *   pass-through: pixel p with prim < 0 or prim & PT_FEATURE_EMISSIVE keeps its input bit for bit and
 *     contributes to no neighbour.  iterations = 0: every pixel keeps its input bit for bit.
 *   demodulation: a_p[k] = max(1e-3f, albedo[k]) (1 with PT_DENOISE_NO_DEMODULATE), c_p[k] = in_p[k] / a_p[k],
 *     s_p = sigma_depth * depth_p.
 *   iteration it = 0 .. iterations-1, step = 1 << it, h = {1/16, 1/4, 3/8, 1/4, 1/16}; for j = -2..2
 *     (outer), i = -2..2 (inner), q = (x + i*step, y + j*step), skipped when outside the image or
 *     pass-through:
 *       dn = max(0, (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z);  wn = dn squared normal_power_log2 times
 *       e  = (n_p.x*(P_q.x-P_p.x) + n_p.y*(P_q.y-P_p.y)) + n_p.z*(P_q.z-P_p.z)
 *       r  = e / s_p;  wz = 1 / (1 + r*r);  w = ((h[j]*h[i]) * wn) * wz
 *       sigma_color > 0: dc = ((D0*D0 + D1*D1) + D2*D2) over D = c_q - c_p, sc = sigma_color / (float)(1 << it),
 *                        w = w * (1 / (1 + dc / (sc*sc)))
 *       acc[k] = acc[k] + w*c_q[k];  wsum = wsum + w
 *     c'_p[k] = acc[k] / wsum if wsum > 0, else c_p[k] (also when wsum is NaN).  Every pixel of iteration
 *     it reads the image of iteration it - 1.
 *   output: out_p[k] = c_p[k] * a_p[k].
 * The edge-stopping weights are rational on purpose (no exp): a numpy restatement agrees in every bit. */
#define PT_FEATURE_EMISSIVE 0x40000000   /* OR'ed into prim when the hit material has emission[0] != 0 */
typedef struct {            /* 48 B, static_assert'ed */
    float albedo[3];        /* (float) of mats[mat].albedo / sphere diffuse; 0 on a miss          */
    float depth;            /* trace()'s closestT of the camera ray; 1e5 (MAX_FLOAT) on a miss     */
    float normal[3];        /* tris[id].norm, or (position - pos)/rad for a sphere; 0 on a miss    */
    int32_t prim;           /* -1 miss (test prim < 0 first); else hit id [| PT_FEATURE_EMISSIVE]  */
    float position[3];      /* o + d*depth, each component (o + (d*depth)) in f32; 0 on a miss     */
    float reserved;         /* written as 0 */
} pt_feature;

#define PT_DENOISE_NO_DEMODULATE 0x1u
typedef struct {
    int32_t iterations;         /* 0..8; iteration i samples at a spacing of 2^i pixels             */
    int32_t normal_power_log2;  /* 0..7: normal weight = max(0, n_p.n_q) squared this many times    */
    float sigma_depth;          /* > 0, finite                                                      */
    float sigma_color;          /* <= 0: colour term off                                            */
    uint32_t flags;             /* PT_DENOISE_NO_DEMODULATE 0x1                                     */
} pt_denoise_params;
void pt_denoise_defaults(pt_denoise_params* p);   /* {5, 5, 0.02f, 0.0f, 0} */

int pt_render_features_device(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, pt_feature* d_feat, void* stream);
int pt_render_features(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, pt_feature* feat /* host */);
/* With a view the ray is pt_camera_ray_view(cam, view, ..., lens = 0, ...): the oriented pinhole ray. */
/* With PT_FLAG_JITTER in params->flags: pt_camera_ray_jitter(cam, view, ..., 0.5f, 0.5f, lens = 0, ...), the ray
 * through the centre of the pixel's footprint (params->flags is otherwise ignored here). */
int pt_render_features_view_device(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, const pt_view* view,
                                   pt_feature* d_feat, void* stream);
int pt_render_features_view(pt_ctx* ctx, const pt_params* params, const pt_camera* cam, const pt_view* view,
                            pt_feature* feat /* host */);
int pt_denoise_device(pt_ctx* ctx, const pt_denoise_params* dp, int width, int height, int pixel_order,
                      const float* d_in, const pt_feature* d_feat, float* d_out, void* stream);
int pt_denoise(pt_ctx* ctx, const pt_denoise_params* dp, int width, int height, int pixel_order,
               const float* in, const pt_feature* feat, float* out /* host */);

/* ------------------------------------------------- the variance-guided denoiser
 * pt_denoise is guided by geometry alone: it smooths a pixel as hard after 128 samples as after 4, so its bias
 * is fixed and past some sample count it makes the image worse.  pt_denoise_guided adds a weight
 * on the luminance difference, measured against the pixel's own estimated noise: where the estimate says the
 * pixel has converged the filter leaves it alone, and the result converges to the render.
 *
 * `var` is W*H fp32 in pixel_order: the variance of each pixel's mean luminance, as pt_noise_variance returns
 * it; any caller-made array is allowed.  Everything else is pt_denoise's (out may equal in; blocking; refused
 * while asynchronous renders are in flight; the scratch is 72 B per pixel here, pt_denoise's stays 64 B).
 * PT_E_INVALID: as pt_denoise, plus a null var and a sigma_luma that is not finite or <= 0.
 *
 * The arithmetic is pt_denoise's (all f32, every operation rounded on its own, no contraction, IEEE division,
 * max(a, b) as `b > a ? b : a`) with these additions:
 *   prepass:   A_p = (0.2126f*a_p[0] + 0.7152f*a_p[1]) + 0.0722f*a_p[2]   (1 with PT_DENOISE_NO_DEMODULATE)
 *              t = var_p / (A_p*A_p);   v_p = (var_p >= 0 && t < 1e30f) ? t : 1e30f
 *     NaN, negative, infinite and overflowing inputs all become the "unknown" value 1e30.  Demodulating the
 *     variance of the luminance by the luminance of the albedo is an approximation (the channels are divided
 *     by different albedos); it is exact for a grey albedo.
 *   each iteration, before the taps (c: that iteration's input):
 *              l_p = (0.2126f*c_p[0] + 0.7152f*c_p[1]) + 0.0722f*c_p[2]
 *     the prefiltered variance, always at a spacing of 1 pixel: g = {1/4, 1/2, 1/4}; for j = -1..1 (outer),
 *     i = -1..1 (inner), q = (x + i, y + j), skipped when outside the image or pass-through:
 *              va = va + (g[j]*g[i])*v_q;   vw = vw + (g[j]*g[i])
 *              vbar_p = va / vw;   den_p = (sigma_luma*sigma_luma)*vbar_p + 1e-20f
 *   each tap, after w has all of pt_denoise's factors (the sigma_color one included when it is on):
 *              dl = l_q - l_p;   w = w * (1 / (1 + (dl*dl)/den_p))
 *              acc[k] = acc[k] + w*c_q[k];   wsum = wsum + w;   vacc = vacc + (w*w)*v_q
 *   result:    wsum > 0:  c'_p[k] = acc[k] / wsum,  v'_p = vacc / (wsum*wsum);  otherwise both are kept.
 *     Pass-through pixels keep everything; iterations = 0 returns the input bit for bit.
 * With var unknown everywhere (+inf, say), (dl*dl)/den_p vanishes against 1 and the output equals pt_denoise's
 * in every bit: this holds whenever dl*dl < 2^-25 * sigma_luma^2 * 1e30, which any real image satisfies, and the
 * weight of a pixel's own tap does not underflow when squared, which normals of unit length ensure (v' stays
 * above 1e30/25 then). */
typedef struct {
    pt_denoise_params base;
    float sigma_luma;           /* > 0, finite: luminance differences count in units of sigma_luma standard errors */
} pt_denoise_guided_params;     /* 24 B */
void pt_denoise_guided_defaults(pt_denoise_guided_params* p);   /* base = pt_denoise_defaults, sigma_luma = 2.0f: a design choice */
int pt_denoise_guided_device(pt_ctx* ctx, const pt_denoise_guided_params* gp, int width, int height, int pixel_order,
                             const float* d_in, const pt_feature* d_feat, const float* d_var, float* d_out, void* stream);
int pt_denoise_guided(pt_ctx* ctx, const pt_denoise_guided_params* gp, int width, int height, int pixel_order,
                      const float* in, const pt_feature* feat, const float* var, float* out /* host */);

/* ----------------------------------------------- accumulators and feature buffers over caller-supplied rays
 * The progressive and the denoising layers over a ray buffer (see "renders along caller-supplied rays" above for the
 * buffer, its indexing and the ray classes): long bakes and probes in passes with a convergence stop and adaptive
 * sampling, and guide records for a panorama or fisheye preview.
 *
 * RAY ACCUMULATORS.  rays holds width * height * 6 floats indexed in params->pixel_order, as for pt_render_rays*; a
 * device buffer must be 8-byte aligned.  Ownership: the accumulator keeps its rays for life, as a camera accumulator
 * keeps its camera -- create copies the whole buffer into device memory it owns (24 B per pixel, freed by
 * pt_accum_destroy), so the caller's buffer may be freed or overwritten once create has returned.
 *
 * Arithmetic (a definition): pixel (x, y) after n samples holds the f64 mean of
 *     rng = curand_init(seed, morton(x, y), 0)
 *     for k = 1..n:  L = integrator(o, d, rng);  m = m*(k-1)/k + L/k
 * with no lens draws anywhere (Morton index 0 is no lens pixel), so pt_accum_add in any split of passes equals
 * pt_render_rays of the same total in every bit.
 *
 * Order of the checks at create: a null argument; asynchronous renders in flight; the flags; the parameters (as
 * pt_render_rays_device validates them); the kernels (below); the device buffer's alignment; then all width *
 * height rays (not only the shard's) are classified, once, on the accumulator's own copy.  Every refusal is
 * PT_E_INVALID with *err set and NULL returned:
 *     flags      only 0, PT_FLAG_NO_DEAD_PATH_SKIP and PT_FLAG_NO_PRIMARY_CACHE -- the flags pt_render_rays and
 *                pt_accum_create both take; the jitter, counting and reference flags and unknown bits are refused
 *     kernels    a context with a non-default PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES, or integrator 1 with PT_HEAD_WF=0,
 *                as pt_accum_create refuses them
 *     invalid    a buffer with an invalid ray, the message naming the lowest such pixel as pt_render_rays does
 *     irregular  a buffer with an irregular ray: accumulation runs on the wavefront kernels only and there is never a
 *                silent fall-back; the message gives the count and says that pt_render_rays takes such a buffer
 * Everything else works unchanged on a ray accumulator: pt_accum_add, _samples, _read, _freeze, _counts, _active,
 * _add_until, _add_adaptive, pt_noise_* (pt_noise_variance*, pt_noise_freeze included) and pt_accum_destroy.  Shards,
 * tile sizes, Morton order, empty shards and split units behave as documented for camera accumulators.  Once a pixel
 * is frozen, passes run over the active list with a set-up kernel that reads each unit's direction from the buffer.
 * pt_accum_view reports has_view = 0; pt_accum_has_rays is 1 for a ray accumulator, 0 for any other and for NULL.
 *
 * MASKED PIXELS (a lightmap texel that belongs to no chart, a fisheye's corners): pt_accum_freeze at 0 samples is the
 * mask.  Such a pixel stays at mean 0 and count 0 and is never sampled.  Its ray must still be valid and regular: the
 * caller pads it with any such ray.
 *
 * pt_accum_save and pt_session_save refuse a ray accumulator with PT_E_INVALID: both formats hold a camera, not a ray
 * buffer.
 *
 * RAY FEATURES.  One pt_feature per pixel for the buffer's ray as given: no normalisation, no 0 + o.  Of params the
 * fields pt_render_features* uses are used; flags is ignored, and nothing jitters.  Each ray takes the walk
 * pt_trace(flags = 0) gives it -- regular or irregular, inside or outside the Markstein ranges -- so an irregular
 * ray is legal here.  depth is trace()'s closestT along the given d: for a direction that is not of unit length it is
 * in units of |d|.  position = o + d * depth, per component in f32.  The other fields are pt_render_features'.
 * Order of the checks: a null argument; asynchronous renders in flight; the parameters; the scene's size (30 id
 * bits); _device: d_feat's 16-byte alignment; d_rays' 8-byte alignment; then an invalid ray anywhere in the buffer
 * (not only in the shard) refuses the call (PT_E_INVALID, the lowest pixel named) with nothing written.  _device
 * writes only this shard's pixels; the host variant writes the rest as zero bytes with prim = -1.  Both block.
 * pt_denoise* and pt_denoise_guided* take these records as they stand.
 *
 * Out of scope: see the list under pt_render_rays. */
pt_accum* pt_accum_create_rays_device(pt_ctx* ctx, const pt_params* params, const float* d_rays, void* stream, int* err);
pt_accum* pt_accum_create_rays(pt_ctx* ctx, const pt_params* params, const float* rays /* host */, int* err);
int pt_accum_has_rays(const pt_accum* acc);   /* 1 / 0; 0 for NULL */
int pt_render_features_rays_device(pt_ctx* ctx, const pt_params* params, const float* d_rays, pt_feature* d_feat, void* stream);
int pt_render_features_rays(pt_ctx* ctx, const pt_params* params, const float* rays /* host */, pt_feature* feat /* host */);

/* ------------------------------------------------------------- accumulators over caller-supplied points
 * The progressive layer over a point buffer (see "irradiance renders at caller-supplied points" above for the buffer,
 * its indexing, the arithmetic of a sample and the point classes): a lightmap or probe bake in passes, with a preview
 * after each, noise estimates, a convergence stop, adaptive sampling and masked texels.
 *
 * points holds width * height * 6 floats, {p.xyz, n.xyz} per pixel, indexed in params->pixel_order as for
 * pt_render_irradiance*; a device buffer must be 8-byte aligned.  Ownership is the ray accumulator's: create copies
 * the whole buffer into device memory the accumulator owns (24 B per pixel, freed by pt_accum_destroy), so the
 * caller's buffer may be freed or overwritten once create has returned.
 *
 * Arithmetic (a definition): pixel (x, y) after n samples holds the f64 mean of pt_render_irradiance's loop,
 *     rng = curand_init(seed, morton(x, y), 0)
 *     for k = 1..n:  u1 = uniform(rng); u2 = uniform(rng);  d = cosineWeightedRay(n, u1, u2)
 *                    L = integrator(p, d, rng);  m = m*(k-1)/k + L/k
 * so pt_accum_add in any split of passes equals pt_render_irradiance of the same total in every bit, and a pixel
 * frozen at k samples holds the k-sample value whatever is frozen around it.  Every unit of a pass is a lens unit: its
 * ray is formed per sample, there is no primary-hit memo, and a split unit's replay skips the pair of every earlier
 * sample.  rays_reference of a pass counts the loop's trace() calls for that pass's samples; summed over the passes it
 * is the one-shot render's.
 *
 * Order of the checks at create, pt_accum_create_rays': a null argument; asynchronous renders in flight; the flags; the
 * parameters; the kernels; the device buffer's alignment; then all width * height points (not only the shard's) are
 * classified, once, on the accumulator's own copy.  Every refusal is PT_E_INVALID with *err set and NULL returned:
 *     flags      only 0, PT_FLAG_NO_DEAD_PATH_SKIP and PT_FLAG_NO_PRIMARY_CACHE (legal, and it changes nothing, as in
 *                the one-shot render); the jitter, counting and reference flags and unknown bits are refused
 *     kernels    a context with a non-default PT_WF_MIN_WAVES / PT_HEAD_MIN_WAVES, or integrator 1 with PT_HEAD_WF=0
 *     invalid    a buffer with an invalid point, the message naming the lowest such pixel as pt_render_irradiance does
 *     irregular  a buffer with an irregular point (beyond 64 scene extents): accumulation runs on the wavefront
 *                kernels only and there is never a silent fall-back; the message gives the count and says that
 *                pt_render_irradiance takes such a buffer
 * Everything else works unchanged on a point accumulator: pt_accum_add, _samples, _read, _freeze, _counts, _active,
 * _add_until, _add_adaptive, pt_noise_* (pt_noise_variance*, pt_noise_freeze included) and pt_accum_destroy.  Shards,
 * tile sizes, Morton order, empty shards and split units behave as documented for camera accumulators.  Once a pixel
 * is frozen, passes run over the active list with a set-up kernel that marks every unit a lens unit.
 * pt_accum_view reports has_view = 0.  pt_accum_has_points is 1 for a point accumulator, 0 for any other and for NULL;
 * pt_accum_has_rays is 0 for a point accumulator.
 *
 * MASKED TEXELS (a lightmap texel that belongs to no chart): pt_accum_freeze at 0 samples is the mask, as for ray
 * accumulators.  Such a texel stays at mean 0 and count 0 and is never sampled.  Its point must still be valid and
 * regular: the caller pads it (cudapathtracer_amd.rays.chart_points pads with the origin and the normal +y).
 *
 * pt_accum_save and pt_session_save refuse a point accumulator with PT_E_INVALID: both formats hold a camera, not a
 * point buffer.
 *
 * Out of scope: sessions and checkpoints over a point buffer; feature buffers over points; pt_render_group /
 * pt_render_multi; passes from the command line (pt_cli --irradiance renders one shot). */
pt_accum* pt_accum_create_points_device(pt_ctx* ctx, const pt_params* params, const float* d_points, void* stream, int* err);
pt_accum* pt_accum_create_points(pt_ctx* ctx, const pt_params* params, const float* points /* host */, int* err);
int pt_accum_has_points(const pt_accum* acc);   /* 1 / 0; 0 for NULL */

/* ------------------------------------------------- temporal reprojection: keep the samples when the camera moves
 * An accumulator keeps its camera and view for life, so a moving camera starts from 1-spp noise every frame.  Every
 * material here is Lambertian (albedo plus emission), so the radiance leaving a surface point does not depend on where
 * the camera stands: last frame's colour at the same world point is a valid sample of this frame's pixel.  A
 * pt_temporal is the temporal stage of an SVGF-style preview pipeline: it reprojects its history through the previous
 * push's camera, accumulates the new frame into it and returns, beside the image, a per-pixel variance of the result
 * that pt_denoise_guided takes as it stands (hand-written gfx950 kernel, pt_temporal.hip; no render kernel is touched).
 *
 * pt_project_view: the inverse of the pinhole camera (lens = 0).  The continuous pixel coordinates (sx, sy) at which
 * the pinhole ray of cam / view passes through the world point P: the corner ray of pixel px gives sx ~ px, the ray
 * through the footprint's centre (the feature ray under PT_FLAG_JITTER) px + 0.5.  All f32, every operation rounded
 * on its own, no contraction, IEEE division; W = pxl_width, H = pxl_height:
 *   q   = P - pos                                           (componentwise)
 *   c.x = (right[0]*q.x + right[1]*q.y) + right[2]*q.z      c.y, c.z likewise with up, back
 *   front = c.z < 0
 *   gx  = (c.x * dist) / c.z            gy = (c.y * dist) / c.z
 *   sx  = (gx / film_w + 0.5f) * (float)W                   sy = (gy / film_h + 0.5f) * (float)H
 * A NULL view projects as right = +x, up = +y, back = +z, film 1 x 1 (the sign-of-zero caveat of the forward camera
 * does not arise: a zero of either sign gives the same sx).  Returns 1 when `front` holds, 0 when not (*sx, *sy are
 * then unspecified), PT_E_INVALID for a null cam, sx or sy.  The view is not validated, as in pt_camera_ray_view.  The
 * kernel runs the same function (one definition, host/project_view.h).
 *
 * pt_temporal_create: a history for width x height images in `pixel_order` on the context's device, destroyed before
 * the context; several may live on one context.  It holds two sets of planes, read one and write the other, all in
 * scanline order, 56 B per pixel and set: G0 = {P.xyz, prim}, G1 = {n.xyz, depth}, C = {r, g, b, n} (16 B each) and
 * M = {m1, m2} (8 B); and the camera, the view and `off` of its previous push.  PT_E_INVALID: a null ctx or params,
 * max_history < 1, a normal_min that is not finite or outside [-1, 1], a plane_tol that is not finite or <= 0, flags
 * != 0, a size outside 1..65535, an unknown pixel order, Morton order on a non-square or non-power-of-two image,
 * asynchronous renders in flight.
 *
 * pt_temporal_push*: takes whole images, as pt_denoise does: `in` W*H*3 fp32, `feat` W*H records of the same frame
 * (pt_render_features* through the same cam, view and PT_FLAG_JITTER; _device: 16-byte aligned), `out` W*H*3 and
 * `var` W*H (may be NULL), all in pixel_order; out may equal in.  Blocking; refused while asynchronous renders are in
 * flight.  In `flags` only PT_FLAG_JITTER is looked at: this frame's features were taken through the footprint's
 * centre, off = 0.5f; otherwise off = 0.0f.  PT_E_INVALID: null arguments; an invalid view; a cam whose pxl_width /
 * pxl_height differ from the object's or whose dist_from_film or focal_length is not finite and > 0; a d_feat that
 * is not 16-byte aligned.  The host variant stages through device buffers the object keeps.
 *
 * The arithmetic per pixel p of the new frame, with its feature record F_p and input colour in_p (all f32, every
 * operation rounded on its own, no contraction, IEEE division; max(a, b) is `b > a ? b : a`); prev cam, prev view and
 * off_prev are the previous push's:
 *   lum(c) = (0.2126f*c[0] + 0.7152f*c[1]) + 0.0722f*c[2]
 *   reset  := first push since create / reset, or prim_p < 0, or pt_project_view(prev cam, prev view, position_p)
 *             says not front
 *   fx = sx - off_prev;  fy = sy - off_prev
 *   snap:  r = floorf(fx + 0.5f);  if (fabsf(fx - r) <= 0.015625f) fx = r;      likewise fy
 *   reset |= !(fx > -1.0f && fx < (float)W) || !(fy > -1.0f && fy < (float)H)   (NaN resets)
 *   x0 = (int)floorf(fx);  tx = fx - (float)x0;   y0, ty likewise
 *   taps in this order: (x0,y0) w = (1-tx)*(1-ty); (x0+1,y0) w = tx*(1-ty); (x0,y0+1) w = (1-tx)*ty;
 *                       (x0+1,y0+1) w = tx*ty
 *   a tap q counts iff it is inside the image, its stored prim_q >= 0, its stored n_q > 0,
 *       (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z >= normal_min, and
 *       fabsf((n_p.x*(P_q.x-P_p.x) + n_p.y*(P_q.y-P_p.y)) + n_p.z*(P_q.z-P_p.z)) <= plane_tol * depth_p
 *   for counting taps:  ws += w;  hc[k] += w*C_q[k];  hn += w*n_q;  h1 += w*m1_q;  h2 += w*m2_q
 *   ws > 0 and not reset:  hc[k] /= ws; hn /= ws; h1 /= ws; h2 /= ws     else: all 0  (hn = 0)
 *   n' = min(hn + 1.0f, (float)max_history);   a = 1.0f / n'
 *   out[k] = hc[k] + (in_p[k] - hc[k]) * a
 *   l = lum(in_p);  m1' = h1 + (l - h1)*a;  m2' = h2 + (l*l - h2)*a
 *   var_p = n' < 2.0f ? +inf : max(0.0f, m2' - m1'*m1') / (n' - 1.0f)
 *   store G0, G1 from F_p, C = {out, n'}, M = {m1', m2'} into the write planes;  then swap
 * n' is the history length: below max_history the output is the running mean of the reprojected samples, from there
 * on an exponential average.  +inf is pt_noise_variance's "unknown" value and pt_denoise_guided treats it as such.  A
 * pixel with prim_p < 0 (a miss) stores n' = 1 and its prim, so next frame it is nobody's history; emissive pixels are
 * ordinary pixels here.  The snap is a condition, not a measurement: a still camera re-projects a pixel onto itself
 * only up to about 1e-3 pixel, from the rounding of position = o + d*depth; 1/64 pixel is far above that and far below
 * any real motion, and with it a still camera reads exactly one tap with weight 1.  Inputs are expected to be free of
 * NaN.  Out of scope: moving geometry, lens (depth-of-field) reprojection -- the features and the history are the
 * pinhole's --, per-shard histories (push the reduced image, as with pt_denoise).
 *
 * pt_temporal_length: the history length n' of every pixel as of the last push (host, W*H, pixel_order; all 0 before
 * the first push).  pt_temporal_frames: the pushes since create / reset (0 for a null object).  pt_temporal_reset: the
 * next push is a first push again. */
typedef struct pt_temporal pt_temporal;
typedef struct {
    int32_t max_history;   /* >= 1: the history length is capped here (then an exponential average) */
    float normal_min;      /* a tap is consistent when n_p.n_q >= normal_min; finite, in [-1, 1]     */
    float plane_tol;       /* ... and |n_p.(P_q - P_p)| <= plane_tol * depth_p; finite, > 0          */
    uint32_t flags;        /* 0 */
} pt_temporal_params;
int pt_project_view(const pt_camera* cam, const pt_view* view /* NULL ok */, pt_vec3 P, float* sx, float* sy);
void pt_temporal_defaults(pt_temporal_params* p);   /* {32, 0.9f, 0.02f, 0}: design choices, not measurements */
pt_temporal* pt_temporal_create(pt_ctx* ctx, const pt_temporal_params* tp, int width, int height, int pixel_order, int* err);
int pt_temporal_push_device(pt_temporal* t, const pt_camera* cam, const pt_view* view /* NULL ok */, uint32_t flags,
                            const float* d_in, const pt_feature* d_feat, float* d_out, float* d_var /* NULL ok */, void* stream);
int pt_temporal_push(pt_temporal* t, const pt_camera* cam, const pt_view* view /* NULL ok */, uint32_t flags,
                     const float* in, const pt_feature* feat, float* out, float* var /* NULL ok */);
int pt_temporal_length(pt_temporal* t, float* n_out /* host, W*H, pixel_order */);
int pt_temporal_frames(const pt_temporal* t);
int pt_temporal_reset(pt_temporal* t);
void pt_temporal_destroy(pt_temporal* t);

/* ------------------------------------------------- lightmap finishing: the gutter fill and the lightmapped view
 * A bake over a UV chart (pt_render_irradiance*, pt_accum_create_points*) leaves 0 in every texel of no chart.  A
 * lightmap is sampled bilinearly, so along every chart border the sampler would mix covered texels with those zeros: a
 * dark seam.  pt_lightmap_dilate* is the dilation pass that ends a bake; pt_lightmap_shade* shows a bake on the
 * geometry from any view, one lookup per pixel of a feature buffer (hand-written gfx950 kernels, pt_lightmap.hip; no
 * render kernel is touched).  All four block, and are refused while asynchronous renders are in flight.
 *
 * pt_lightmap_dilate*: in and out are width * height * 3 fp32 in scanline order (a lightmap is a texture: Morton order
 * is not offered), covered is width * height bytes, non-zero = covered (rays.chart_points' `covered`), src (may be
 * NULL) width * height int32.  The rule is in integers, so every implementation of it agrees exactly:
 *   a covered texel keeps its input bit for bit, and src is its own index y*W + x;
 *   an uncovered texel (x, y) looks at the covered texels (x+i, y+j) with |i| <= radius, |j| <= radius, inside the
 *     image (no wrap-around), and takes the one with the smallest i*i + j*j, ties to the smaller j, then to the
 *     smaller i: out is that texel's input bit for bit, src is (y+j)*W + (x+i);
 *   if there is none, out is the texel's own input bit for bit and src is -1.
 * Only covered texels are ever read as sources and they never change, so out may equal in (the same result);
 * radius = 0 is a copy.  PT_E_INVALID, naming the argument: a null ctx, in, covered or out; a width or height outside
 * 1..65535, or more than 2^31 - 1 texels; a radius outside 0..16; _device: an in, out or src that is not 4-byte
 * aligned.  The host variant stages through device buffers of its own.
 *
 * pt_lightmap_shade*: one output (3 fp32) per feature record, in the records' own order -- any pt_render_features*
 * buffer works (view, jitter and rays variants included), so no pixel order appears here.  tri_uv[6*t ..] holds the
 * chart coordinates ua, ub, uc (x then y each) of v0, v1, v2 of ORIGINAL triangle t, the id a feature's prim carries;
 * a NaN in its first float means "this triangle has no chart" (num_tris rows; may be NULL for a scene without
 * triangles).  map is map_w * map_h * 3 fp32 in scanline order.  A record gets `fill` when prim < 0, or prim &
 * PT_FEATURE_EMISSIVE, or prim >= num_tris (a sphere), or its triangle has no chart, or det below is 0 or not finite,
 * or s or t below is not finite.  For every other record, all in f32, every operation rounded on its own, no
 * contraction, IEEE division; clamp(v, lo, hi) is `v < lo ? lo : (v > hi ? hi : v)`, so a NaN stays one; v0, v1, v2
 * are the scene's f32 vertices of triangle prim:
 *   e1 = v1 - v0;  e2 = v2 - v0;  g = position - v0                               (componentwise)
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 *   d11 = dot(e1,e1);  d12 = dot(e1,e2);  d22 = dot(e2,e2);  g1 = dot(g,e1);  g2 = dot(g,e2)
 *   det = d11*d22 - d12*d12
 *   b1 = clamp((d22*g1 - d12*g2) / det, 0, 1);   b2 = clamp((d11*g2 - d12*g1) / det, 0, 1)
 *   u = (ua.x + b1*(ub.x - ua.x)) + b2*(uc.x - ua.x);   v likewise with .y
 *   s = u*(float)map_w - 0.5f;  t = v*(float)map_h - 0.5f        (not finite: fill);  then s = clamp(s, -1, (float)map_w),
 *                                                                 t = clamp(t, -1, (float)map_h)
 *   x0 = floorf(s);  fx = s - x0;  texel columns (int)x0 and (int)x0 + 1, each clamped to [0, map_w - 1];  rows likewise
 *   per channel, L00 = map(column 0, row 0 of the four), L10 the next column, L01 the next row:
 *     top = L00 + fx*(L10 - L00);  bot = L01 + fx*(L11 - L01);  val = top + fy*(bot - top)
 *   out = albedo * val                                            (val alone with PT_LIGHTMAP_NO_ALBEDO)
 * The lerp form is deliberate: a constant lightmap is reproduced exactly.  Every material here is Lambertian, so a
 * texel's outgoing radiance is its albedo times the baked E/pi; emitters get `fill` (composite them from a 0-bounce
 * render).  The triangles' vertices are read from the context's own original-order records (v0, e1, e2: the same f32
 * subtractions), nothing is uploaded.  PT_E_INVALID, naming the argument: a null ctx or params, unknown flags, a map_w
 * or map_h outside 1..65535, a null map, a null tri_uv (unless the scene has no triangles), a null feat or out (unless
 * n = 0); _device: a d_feat that is not 16-byte aligned, a d_tri_uv, d_map or d_out that is not 4-byte aligned.
 * n = 0 is PT_OK and touches nothing. */
#define PT_LIGHTMAP_NO_ALBEDO 0x1u
typedef struct {
    float fill[3];     /* the colour of a record without a lightmap value (copied bit for bit) */
    uint32_t flags;    /* PT_LIGHTMAP_NO_ALBEDO 0x1 */
} pt_lightmap_params;   /* 16 B */
int pt_lightmap_dilate_device(pt_ctx* ctx, int width, int height, int radius, const float* d_in, const uint8_t* d_covered,
                              float* d_out, int32_t* d_src /* or NULL */, void* stream);
int pt_lightmap_dilate(pt_ctx* ctx, int width, int height, int radius, const float* in, const uint8_t* covered, float* out,
                       int32_t* src /* or NULL */);
int pt_lightmap_shade_device(pt_ctx* ctx, const pt_lightmap_params* lp, uint32_t n, const pt_feature* d_feat,
                             const float* d_tri_uv /* num_tris*6 */, const float* d_map, int map_w, int map_h,
                             float* d_out /* n*3 */, void* stream);
int pt_lightmap_shade(pt_ctx* ctx, const pt_lightmap_params* lp, uint32_t n, const pt_feature* feat, const float* tri_uv,
                      const float* map, int map_w, int map_h, float* out);

/* ----------------------------------------------------------- one process, N GPUs
 * A group of contexts on distinct devices with one RCCL communicator per device
 * (ncclCommInitAll).  pt_render_group renders shard i of N on context i -- image tiles dealt
 * round-robin, tile t -> context t % N (params' shard fields are ignored) -- concurrently, one
 * host thread and HIP stream per device, each into a zero-filled fp32 framebuffer, then ONE
 * ncclReduce(sum, root = ctxs[0]'s device) over xGMI and one copy of the image to out_rgb:
 * bit-identical to a single-GPU pt_render (every pixel is its shard's value plus zeros).  Stats
 * are summed over the shards; `seconds` is the job's wall time (renders + reduce + copy).
 * Replaces the reference's launch loop (kernel.cu:709-736) and its D2H copy (:760).
 * The group does not own the contexts; destroy it before them. */
/* The pixels shard `shard_index` of `shard_count` renders (tile_w x tile_h tiles, 0 = 8, dealt tile t ->
 * shard t % count): their scanline ids y*W + x, in the order the shard's work slots take them (8x8
 * blocks, Morton order within a block).  out = NULL: only *n_out.  Host-only; the kernels use the same
 * mapping function. */
int pt_shard_pixels(int width, int height, int shard_index, int shard_count, int tile_w, int tile_h, uint32_t* out,
                    uint32_t cap, uint32_t* n_out);

typedef struct pt_group pt_group;
pt_group* pt_group_create(pt_ctx* const* ctxs, int n, int* err);
int pt_group_size(const pt_group* group);
int pt_render_group(pt_group* group, const pt_params* params, const pt_camera* cam, float* out_rgb, pt_stats* stats);
int pt_render_group_view(pt_group* group, const pt_params* params, const pt_camera* cam, const pt_view* view,
                         float* out_rgb, pt_stats* stats);
void pt_group_destroy(pt_group* group);
/* create + render + destroy */
int pt_render_multi(pt_ctx* const* ctxs, int n, const pt_params* params, const pt_camera* cam, float* out_rgb,
                    pt_stats* stats);
int pt_render_multi_view(pt_ctx* const* ctxs, int n, const pt_params* params, const pt_camera* cam, const pt_view* view,
                         float* out_rgb, pt_stats* stats);

void pt_destroy(pt_ctx* ctx);
const char* pt_last_error(void);
int pt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif

// scene.cpp -- the reference's scene globals and loadOBJ (modelLoader.h:43-47, 125-210),
// camera maps (camera.h:36-97) and the PPM writer (kernel.cu:763-778, color.h:59-71).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <thread>

#include "host_internal.h"
#include "project_view.h"

namespace pt {

namespace {
thread_local std::string g_error;

inline pt_vec3 v3(float x, float y, float z) { pt_vec3 r; r.x = x; r.y = y; r.z = z; return r; }
inline pt_vec3 vsub(pt_vec3 a, pt_vec3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline pt_vec3 vcross(pt_vec3 a, pt_vec3 b)
{
    return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
inline float vlen(pt_vec3 v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }
inline pt_vec3 vunit(pt_vec3 v)
{
    float len = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return v3(v.x / len, v.y / len, v.z / len);
}

// (int)x on the reference's x86 targets: truncation, "integer indefinite" INT_MIN for NaN
// and out-of-range values (cvttsd2si).  Made explicit so no C++ UB is involved.
inline int trunc_to_int(double x)
{
    if (!(x > -2147483649.0 && x < 2147483648.0)) return INT32_MIN;
    return static_cast<int>(x);
}
}  // namespace

int fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

void clear_error() { g_error.clear(); }

const char* last_error_cstr() { return g_error.c_str(); }

int validate_jitter_flags(const char* who, uint32_t flags)
{
    if ((flags & PT_FLAG_JITTER_TENT) && !(flags & PT_FLAG_JITTER))
        return fail(PT_E_INVALID, "%s: flags 0x%x: PT_FLAG_JITTER_TENT needs PT_FLAG_JITTER (the tent is a kind of jitter)", who, flags);
    return PT_OK;
}

// The condition of pt.h: 11 finite floats, a film > 0, an orthonormal basis to 1e-3 (in double).
int validate_view(const char* who, const pt_view* v)
{
    const float* f = v->right;   // (right, up, back, film_w, film_h: 11 consecutive floats)
    for (int k = 0; k < 11; ++k)
        if (!std::isfinite(f[k])) return fail(PT_E_INVALID, "%s: view: a component is not finite", who);
    if (!(v->film_w > 0.0f) || !(v->film_h > 0.0f))
        return fail(PT_E_INVALID, "%s: view: film %g x %g must be > 0", who, (double)v->film_w, (double)v->film_h);
    auto dotd = [](const float* a, const float* b) {
        return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
    };
    const double e[6] = {dotd(v->right, v->right) - 1.0, dotd(v->up, v->up) - 1.0, dotd(v->back, v->back) - 1.0,
                         dotd(v->right, v->up), dotd(v->right, v->back), dotd(v->up, v->back)};
    static const char* const names[6] = {"right.right - 1", "up.up - 1", "back.back - 1", "right.up", "right.back", "up.back"};
    for (int k = 0; k < 6; ++k)
        if (!(std::fabs(e[k]) <= 1e-3))
            return fail(PT_E_INVALID, "%s: view: the basis is not orthonormal (%s = %g, limit 1e-3)", who, names[k], e[k]);
    return PT_OK;
}

}  // namespace pt

using namespace pt;

extern "C" {

const char* pt_last_error(void) { return pt::last_error_cstr(); }
int pt_abi_version(void) { return PT_ABI_VERSION; }

pt_host_scene* pt_scene_new(void) { return new (std::nothrow) pt_host_scene(); }

void pt_scene_free(pt_host_scene* s) { delete s; }

const char* pt_scene_last_warning(const pt_host_scene* s) { return s ? s->s.warning.c_str() : ""; }

int pt_scene_load_obj(pt_host_scene* hs, const char* obj_path, const char* mtl_basepath, pt_vec3 origin,
                      float scale, int flip_normals)
{
    if (!hs || !obj_path) return fail(PT_E_INVALID, "pt_scene_load_obj: null argument");
    HostScene& s = hs->s;
    ObjResult r = read_obj(obj_path, mtl_basepath ? mtl_basepath : "models/");
    s.warning = r.message;
    if (r.fatal) return fail(r.message.rfind("Cannot open", 0) == 0 ? PT_E_IO : PT_E_SCENE, "%s", r.message.c_str());
    // materials are appended twice; triangles index the second copy (modelLoader.h:138-159)
    auto to_mat = [](const ObjMaterial& m) {
        pt_material d;
        for (int c = 0; c < 3; ++c) {
            d.albedo[c] = static_cast<double>(m.diffuse[c]);
            d.emission[c] = static_cast<double>(m.emission[c]);
        }
        return d;
    };
    for (const ObjMaterial& m : r.materials) s.mats.push_back(to_mat(m));
    const uint32_t mat_base = static_cast<uint32_t>(s.mats.size());
    for (const ObjMaterial& m : r.materials) s.mats.push_back(to_mat(m));

    for (const ObjShape& sh : r.shapes) {
        const int32_t vbase = static_cast<int32_t>(s.verts.size());
        const size_t nv = sh.positions.size() / 3;
        for (size_t i = 0; i < nv; ++i) {                                       // :165-172
            s.verts.push_back(v3(sh.positions[3 * i + 0] * scale + origin.x,
                                 sh.positions[3 * i + 1] * scale + origin.y,
                                 sh.positions[3 * i + 2] * scale + origin.z));
        }
        const size_t nt = sh.indices.size() / 3;
        for (size_t i = 0; i < nt; ++i) {                                       // :175-205
            pt_triangle t;
            t.v0 = static_cast<int32_t>(sh.indices[3 * i + 0]) + vbase;
            t.v1 = static_cast<int32_t>(sh.indices[3 * i + 1]) + vbase;
            t.v2 = static_cast<int32_t>(sh.indices[3 * i + 2]) + vbase;
            const pt_vec3 a = s.verts[t.v0], b = s.verts[t.v1], c = s.verts[t.v2];
            // every triangle of a shape takes the shape's first material id (:186)
            t.mat = static_cast<int32_t>(static_cast<uint32_t>(sh.material_ids[0]) + mat_base);
            if (t.mat < 0 || static_cast<size_t>(t.mat) >= s.mats.size())
                return fail(PT_E_SCENE, "%s: triangle uses material %d but only %zu materials are loaded "
                            "(face without usemtl and no mtllib?)", obj_path, t.mat, s.mats.size());
            if (s.mats[t.mat].emission[0] != 0) {                               // :188-196
                s.lights.push_back(static_cast<uint32_t>(s.tris.size()));
                float area = vlen(vcross(vsub(b, a), vsub(c, a))) / 2;
                s.total_light_area += area;
            }
            t.norm = vunit(vcross(vsub(b, a), vsub(c, a)));                     // :198-200
            if (flip_normals) t.norm = v3(t.norm.x * -1, t.norm.y * -1, t.norm.z * -1);
            s.tris.push_back(t);
        }
    }
    s.bvh.clear();
    s.bvh_depth = 0;
    return PT_OK;
}

int pt_scene_add_sphere(pt_host_scene* hs, const pt_sphere* sp)
{
    if (!hs || !sp) return fail(PT_E_INVALID, "pt_scene_add_sphere: null argument");
    if (!(sp->rad > 0.0f) || !std::isfinite(sp->rad) || !std::isfinite(sp->pos.x) || !std::isfinite(sp->pos.y) ||
        !std::isfinite(sp->pos.z))
        return fail(PT_E_INVALID, "pt_scene_add_sphere: radius must be > 0 and the sphere finite");
    HostScene& s = hs->s;
    if (sp->emission[0] != 0) {
        s.lights.push_back(PT_LIGHT_SPHERE | static_cast<uint32_t>(s.spheres.size()));
        s.total_light_area += sphere_area(sp->rad);
    }
    s.spheres.push_back(*sp);
    return PT_OK;
}

int pt_scene_build_bvh(pt_host_scene* hs)
{
    if (!hs) return fail(PT_E_INVALID, "pt_scene_build_bvh: null scene");
    HostScene& s = hs->s;
    if (s.tris.empty() && !s.spheres.empty()) {   // spheres only: no triangle BVH (config C1)
        s.bvh.clear();
        s.bvh_depth = 0;
        return PT_OK;
    }
    int rc = build_bvh(s.verts, s.tris, &s.bvh, &s.bvh_depth);
    if (rc != PT_OK) return rc;
    if (s.bvh_depth >= PT_MAX_BVH_DEPTH)                                        // kernel.cu:627-631
        return fail(PT_E_BVH_DEPTH, "Critical Error: BVH depth is too big (%d >= %d)", s.bvh_depth, PT_MAX_BVH_DEPTH);
    return PT_OK;
}

int pt_scene_view(const pt_host_scene* hs, pt_scene* out)
{
    if (!hs || !out) return fail(PT_E_INVALID, "pt_scene_view: null argument");
    const HostScene& s = hs->s;
    out->num_verts = static_cast<uint32_t>(s.verts.size());
    out->num_tris = static_cast<uint32_t>(s.tris.size());
    out->num_mats = static_cast<uint32_t>(s.mats.size());
    out->num_lights = static_cast<uint32_t>(s.lights.size());
    out->verts = s.verts.data();
    out->tris = s.tris.data();
    out->mats = s.mats.data();
    out->lights = s.lights.data();
    out->total_light_area = s.total_light_area;
    out->bvh = s.bvh.data();
    out->bvh_size = static_cast<uint32_t>(s.bvh.size());
    out->bvh_depth = s.bvh_depth;
    out->spheres = s.spheres.data();
    out->num_spheres = static_cast<uint32_t>(s.spheres.size());
    return PT_OK;
}

// camera.h:66-75
uint32_t pt_morton_pxl_to_i(uint32_t x, uint32_t y)
{
    uint32_t r = 0;
    for (int b = 0; b < 16; ++b) {
        r |= ((x >> b) & 1u) << (2 * b);
        r |= ((y >> b) & 1u) << (2 * b + 1);
    }
    return r;
}

// camera.h:57-65 (outputs are uint16_t in the reference)
void pt_morton_i_to_pxl(uint32_t idx, uint32_t* x, uint32_t* y)
{
    uint32_t xx = 0, yy = 0;
    for (int b = 0; b < 16; ++b) {
        xx |= ((idx >> (2 * b)) & 1u) << b;
        yy |= ((idx >> (2 * b + 1)) & 1u) << b;
    }
    if (x) *x = xx & 0xffffu;
    if (y) *y = yy & 0xffffu;
}

// camera.h:77-97; the lens angle goes through the same deterministic sin/cos as the kernels.
void pt_camera_ray(const pt_camera* cam, uint32_t idx, int lens, float u1, float u2, pt_vec3* origin, pt_vec3* dir)
{
    uint32_t px, py;
    pt_morton_i_to_pxl(idx, &px, &py);
    pt_vec3 film = v3(static_cast<float>(px) / static_cast<float>(cam->pxl_width) - 0.5f,
                      static_cast<float>(py) / static_cast<float>(cam->pxl_height) - 0.5f, 0.0f);
    pt_vec3 o = v3(0.0f, 0.0f, 0.0f);
    if (lens) {
        float r = cam->radius * sqrtf(u1);
        float theta = static_cast<float>(2 * 3.14159 * static_cast<double>(u2));
        float sn, cs;
        pt::sincos_det(theta, &sn, &cs);
        o = v3(r * cs, r * sn, 0.0f);
    }
    film.z = cam->dist_from_film;
    const float k = -cam->focal_length;
    film = v3(film.x * k / cam->dist_from_film, film.y * k / cam->dist_from_film, film.z * k / cam->dist_from_film);
    *origin = v3(o.x + cam->pos.x, o.y + cam->pos.y, o.z + cam->pos.z);
    *dir = vunit(vsub(film, o));
}

// ---- the oriented camera (pt_view, pt.h): no counterpart in the reference
int pt_view_validate(const pt_view* v)
{
    pt::clear_error();
    if (!v) return pt::fail(PT_E_INVALID, "pt_view_validate: null view");
    return pt::validate_view("pt_view_validate", v);
}

int pt_view_look_at(pt_vec3 pos, pt_vec3 target, pt_vec3 up, pt_view* out)
{
    pt::clear_error();
    if (!out) return pt::fail(PT_E_INVALID, "pt_view_look_at: null view");
    for (const float c : {pos.x, pos.y, pos.z, target.x, target.y, target.z, up.x, up.y, up.z})
        if (!std::isfinite(c)) return pt::fail(PT_E_INVALID, "pt_view_look_at: a component is not finite");
    // all in double from the float inputs, rounded to float once at the end
    const double b[3] = {(double)pos.x - (double)target.x, (double)pos.y - (double)target.y, (double)pos.z - (double)target.z};
    const double bl = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    if (!(bl > 0.0)) return pt::fail(PT_E_INVALID, "pt_view_look_at: the position is the target");
    const double back[3] = {b[0] / bl, b[1] / bl, b[2] / bl};
    const double u[3] = {(double)up.x, (double)up.y, (double)up.z};
    const double r[3] = {u[1] * back[2] - u[2] * back[1], u[2] * back[0] - u[0] * back[2], u[0] * back[1] - u[1] * back[0]};
    const double rl = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    const double ul = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    // (parallel: the cross product vanishes against |up|, to double rounding)
    if (!(rl > 1e-12 * ul)) return pt::fail(PT_E_INVALID, "pt_view_look_at: up is parallel to the viewing direction (or zero)");
    const double right[3] = {r[0] / rl, r[1] / rl, r[2] / rl};
    const double up2[3] = {back[1] * right[2] - back[2] * right[1], back[2] * right[0] - back[0] * right[2],
                           back[0] * right[1] - back[1] * right[0]};
    for (int k = 0; k < 3; ++k) {
        out->right[k] = (float)right[k];
        out->up[k] = (float)up2[k];
        out->back[k] = (float)back[k];
    }
    out->film_w = 1.0f;
    out->film_h = 1.0f;
    return PT_OK;
}

int pt_view_set_fov(pt_view* v, const pt_camera* cam, float vfov_deg, int width, int height)
{
    pt::clear_error();
    if (!v || !cam) return pt::fail(PT_E_INVALID, "pt_view_set_fov: null argument");
    if (!(vfov_deg > 0.0f && vfov_deg < 180.0f)) return pt::fail(PT_E_INVALID, "pt_view_set_fov: vfov %g outside (0, 180) degrees", (double)vfov_deg);
    if (width <= 0 || height <= 0) return pt::fail(PT_E_INVALID, "pt_view_set_fov: image size %dx%d", width, height);
    if (!(cam->dist_from_film > 0.0f) || !std::isfinite(cam->dist_from_film))
        return pt::fail(PT_E_INVALID, "pt_view_set_fov: dist_from_film %g must be finite and > 0", (double)cam->dist_from_film);
    const double half = ((double)vfov_deg * 3.14159265358979323846) / 360.0;
    const double fh = (2.0 * (double)cam->dist_from_film) * tan(half);
    const double fw = (fh * (double)width) / (double)height;
    const float film_w = (float)fw, film_h = (float)fh;
    if (!(film_w > 0.0f) || !(film_h > 0.0f) || !std::isfinite(film_w) || !std::isfinite(film_h))
        return pt::fail(PT_E_INVALID, "pt_view_set_fov: film %g x %g is not finite and > 0", fw, fh);
    v->film_w = film_w;
    v->film_h = film_h;
    return PT_OK;
}

// The arithmetic of pt.h, one rounded f32 operation at a time (this TU is compiled without contraction).
void pt_camera_ray_view(const pt_camera* cam, const pt_view* view, uint32_t idx, int lens, float u1, float u2, pt_vec3* origin,
                        pt_vec3* dir)
{
    if (!view) { pt_camera_ray(cam, idx, lens, u1, u2, origin, dir); return; }
    uint32_t px, py;
    pt_morton_i_to_pxl(idx, &px, &py);
    pt_vec3 film = v3((static_cast<float>(px) / static_cast<float>(cam->pxl_width) - 0.5f) * view->film_w,
                      (static_cast<float>(py) / static_cast<float>(cam->pxl_height) - 0.5f) * view->film_h, cam->dist_from_film);
    pt_vec3 lo = v3(0.0f, 0.0f, 0.0f);
    if (lens) {
        float r = cam->radius * sqrtf(u1);
        float theta = static_cast<float>(2 * 3.14159 * static_cast<double>(u2));
        float sn, cs;
        pt::sincos_det(theta, &sn, &cs);
        lo = v3(r * cs, r * sn, 0.0f);
    }
    const float k = -cam->focal_length;
    film = v3(film.x * k / cam->dist_from_film, film.y * k / cam->dist_from_film, film.z * k / cam->dist_from_film);
    const pt_vec3 c = vsub(film, lo);
    const float* R = view->right;
    const float* U = view->up;
    const float* B = view->back;
    const pt_vec3 w = v3((R[0] * c.x + U[0] * c.y) + B[0] * c.z, (R[1] * c.x + U[1] * c.y) + B[1] * c.z,
                         (R[2] * c.x + U[2] * c.y) + B[2] * c.z);
    *dir = vunit(w);
    if (lens)
        *origin = v3((R[0] * lo.x + U[0] * lo.y) + cam->pos.x, (R[1] * lo.x + U[1] * lo.y) + cam->pos.y,
                     (R[2] * lo.x + U[2] * lo.y) + cam->pos.z);
    else
        *origin = v3(0.0f + cam->pos.x, 0.0f + cam->pos.y, 0.0f + cam->pos.z);
}

// ---- sub-pixel jitter (PT_FLAG_JITTER, pt.h): the host's copies of the device functions
static float jitter_tent(float u)
{
    return (u < 0.5f) ? sqrtf(2.0f * u) - 1.0f : 1.0f - sqrtf(2.0f - 2.0f * u);
}

int pt_jitter_offset(uint32_t flags, float ua, float ub, float* jx, float* jy)
{
    pt::clear_error();
    if (!jx || !jy) return pt::fail(PT_E_INVALID, "pt_jitter_offset: null argument");
    if (int rc = pt::validate_jitter_flags("pt_jitter_offset", flags)) return rc;
    if (!(flags & PT_FLAG_JITTER)) { *jx = 0.0f; *jy = 0.0f; }
    else if (flags & PT_FLAG_JITTER_TENT) { *jx = 0.5f + jitter_tent(ua); *jy = 0.5f + jitter_tent(ub); }
    else { *jx = ua; *jy = ub; }
    return PT_OK;
}

// pt_camera_ray / pt_camera_ray_view with (px + jx, py + jy) in the places of (px, py), one rounded f32 operation at a
// time; zero offsets give their bits ((float)px + 0.0f is (float)px).
void pt_camera_ray_jitter(const pt_camera* cam, const pt_view* view, uint32_t idx, float jx, float jy, int lens, float u1, float u2,
                          pt_vec3* origin, pt_vec3* dir)
{
    uint32_t px, py;
    pt_morton_i_to_pxl(idx, &px, &py);
    const float sx = static_cast<float>(px) + jx, sy = static_cast<float>(py) + jy;
    pt_vec3 film = v3(sx / static_cast<float>(cam->pxl_width) - 0.5f, sy / static_cast<float>(cam->pxl_height) - 0.5f,
                      cam->dist_from_film);
    if (view) film = v3(film.x * view->film_w, film.y * view->film_h, film.z);
    pt_vec3 lo = v3(0.0f, 0.0f, 0.0f);
    if (lens) {
        float r = cam->radius * sqrtf(u1);
        float theta = static_cast<float>(2 * 3.14159 * static_cast<double>(u2));
        float sn, cs;
        pt::sincos_det(theta, &sn, &cs);
        lo = v3(r * cs, r * sn, 0.0f);
    }
    const float k = -cam->focal_length;
    film = v3(film.x * k / cam->dist_from_film, film.y * k / cam->dist_from_film, film.z * k / cam->dist_from_film);
    const pt_vec3 c = vsub(film, lo);
    if (!view) {
        *origin = v3(lo.x + cam->pos.x, lo.y + cam->pos.y, lo.z + cam->pos.z);
        *dir = vunit(c);
        return;
    }
    const float* R = view->right;
    const float* U = view->up;
    const float* B = view->back;
    const pt_vec3 w = v3((R[0] * c.x + U[0] * c.y) + B[0] * c.z, (R[1] * c.x + U[1] * c.y) + B[1] * c.z,
                         (R[2] * c.x + U[2] * c.y) + B[2] * c.z);
    *dir = vunit(w);
    if (lens)
        *origin = v3((R[0] * lo.x + U[0] * lo.y) + cam->pos.x, (R[1] * lo.x + U[1] * lo.y) + cam->pos.y,
                     (R[2] * lo.x + U[2] * lo.y) + cam->pos.z);
    else
        *origin = v3(0.0f + cam->pos.x, 0.0f + cam->pos.y, 0.0f + cam->pos.z);
}

// ---- the inverse of the pinhole camera (pt.h): the host's copy of what the temporal kernel runs (project_view.h)
int pt_project_view(const pt_camera* cam, const pt_view* view, pt_vec3 P, float* sx, float* sy)
{
    pt::clear_error();
    if (!cam || !sx || !sy) return pt::fail(PT_E_INVALID, "pt_project_view: null argument");
    const pt_view v = view ? *view : pt::identity_view();
    return pt::project_view(*cam, v, P.x, P.y, P.z, sx, sy) ? 1 : 0;
}

// kernel.cu:771 -> color.h:59-62 normalized, color.h:68-71 gammaCorrect(c, 1/2.2), (int)(c*255)
int pt_tonemap_u8(double c)
{
    double n = c / (c + 1);
    double g = pow(n, static_cast<double>(static_cast<float>(1 / 2.2)));
    return trunc_to_int(g * 255);
}

}  // extern "C"

namespace {
template <typename T>
int write_ppm_any(const char* path, const T* rgb, int w, int h, int order = PT_ORDER_SCANLINE)
{
    if (!path || !rgb || w <= 0 || h <= 0) return fail(PT_E_INVALID, "pt_write_ppm: bad arguments");
    if (order != PT_ORDER_SCANLINE && order != PT_ORDER_MORTON) return fail(PT_E_INVALID, "pt_write_ppm: pixel order %d", order);
    if (order == PT_ORDER_MORTON && !pt::morton_size_ok(w, h))
        return fail(PT_E_INVALID, "pt_write_ppm: Morton order needs a square power-of-two image (%dx%d)", w, h);
    FILE* fp = fopen(path, "w");
    if (!fp) return fail(PT_E_IO, "pt_write_ppm: cannot open %s", path);
    fprintf(fp, "P3 %d %d 255\n", w, h);
    for (int y = 0; y < h; ++y) {
        for (int x = w - 1; x >= 0; --x) {                                     // mirrored, kernel.cu:766
            const size_t idx = order == PT_ORDER_MORTON ? pt_morton_pxl_to_i((uint32_t)x, (uint32_t)y)   // kernel.cu:771
                                                        : static_cast<size_t>(y) * w + x;
            const T* p = rgb + idx * 3;
            fprintf(fp, "%d %d %d ", pt_tonemap_u8(static_cast<double>(p[0])), pt_tonemap_u8(static_cast<double>(p[1])),
                    pt_tonemap_u8(static_cast<double>(p[2])));
        }
    }
    if (fclose(fp) != 0) return fail(PT_E_IO, "pt_write_ppm: write failed for %s", path);
    return PT_OK;
}
}  // namespace

extern "C" int pt_write_ppm(const char* path, const float* rgb, int width, int height)
{
    return write_ppm_any(path, rgb, width, height);
}

extern "C" int pt_write_ppm_order(const char* path, const float* rgb, int width, int height, int pixel_order)
{
    return write_ppm_any(path, rgb, width, height, pixel_order);
}

// The reference's PPM text (kernel.cu:763-778) from tone-mapped codes (pt_tonemap / GPU).
extern "C" int pt_write_ppm_codes(const char* path, const int32_t* codes, int w, int h)
{
    if (!path || !codes || w <= 0 || h <= 0) return fail(PT_E_INVALID, "pt_write_ppm_codes: bad arguments");
    FILE* fp = fopen(path, "w");
    if (!fp) return fail(PT_E_IO, "pt_write_ppm_codes: cannot open %s", path);
    fprintf(fp, "P3 %d %d 255\n", w, h);
    for (int y = 0; y < h; ++y)
        for (int x = w - 1; x >= 0; --x) {                                         // mirrored, kernel.cu:766
            const int32_t* p = codes + (static_cast<size_t>(y) * w + x) * 3;
            fprintf(fp, "%d %d %d ", p[0], p[1], p[2]);
        }
    if (fclose(fp) != 0) return fail(PT_E_IO, "pt_write_ppm_codes: write failed for %s", path);
    return PT_OK;
}

// Portable float map of the fp32 mean image (little-endian, scale -1, rows bottom-up per the
// PFM convention): the lossless dump for parity checks.
extern "C" int pt_write_pfm(const char* path, const float* rgb, int w, int h)
{
    if (!path || !rgb || w <= 0 || h <= 0) return fail(PT_E_INVALID, "pt_write_pfm: bad arguments");
    FILE* fp = fopen(path, "wb");
    if (!fp) return fail(PT_E_IO, "pt_write_pfm: cannot open %s", path);
    fprintf(fp, "PF\n%d %d\n-1.0\n", w, h);
    bool ok = true;
    for (int y = h - 1; y >= 0 && ok; --y)
        ok = fwrite(rgb + static_cast<size_t>(y) * w * 3, sizeof(float), static_cast<size_t>(w) * 3, fp) ==
             static_cast<size_t>(w) * 3;
    if (fclose(fp) != 0 || !ok) return fail(PT_E_IO, "pt_write_pfm: write failed for %s", path);
    return PT_OK;
}

namespace pt {
// the sizes for which the reference's Morton framebuffer (idx < W*H, camera.h:57-75) covers the
// image one-to-one: square powers of two
bool morton_size_ok(int w, int h)
{
    return w > 0 && w == h && (w & (w - 1)) == 0 && w <= 65536;
}

unsigned host_threads()
{
    for (const char* var : {"PT_HOST_THREADS", "OMP_NUM_THREADS"}) {
        if (const char* e = getenv(var)) {
            const int v = atoi(e);
            if (v > 0) return static_cast<unsigned>(v < 64 ? v : 64);
        }
    }
    const unsigned hw = std::thread::hardware_concurrency();
    return hw == 0 ? 1u : (hw < 16 ? hw : 16u);
}

// Tone-map thresholds for the GPU output step: t[k] (k = 1..255) = the smallest non-negative
// float c with pt_tonemap_u8(c) >= k.  The map is monotone in c (c/(c+1), pow, *255 and the
// truncation all are), so for finite c >= 0 the code is the number of thresholds <= c, exactly
// as this host's libm computes it.  t[0] = 0.  Returns false if a bisection finds the map
// non-monotone at a boundary (then the device step must not be used).
bool tonemap_thresholds(float t[256])
{
    t[0] = 0.0f;
    bool ok = true;
    for (int k = 1; k < 256; ++k) {
        uint32_t lo = 0, hi = 0x7f7fffffu;   // [0, FLT_MAX]; f(FLT_MAX) = 255
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            float c;
            memcpy(&c, &mid, 4);
            if (pt_tonemap_u8(static_cast<double>(c)) >= k) hi = mid; else lo = mid + 1;
        }
        memcpy(&t[k], &lo, 4);
        if (pt_tonemap_u8(static_cast<double>(t[k])) < k) ok = false;
        if (lo > 0) {
            float below;
            const uint32_t b = lo - 1;
            memcpy(&below, &b, 4);
            if (pt_tonemap_u8(static_cast<double>(below)) >= k) ok = false;
        }
        if (k > 1 && t[k] < t[k - 1]) ok = false;
    }
    return ok;
}
}  // namespace pt

extern "C" int pt_write_ppm_f64(const char* path, const double* rgb, int width, int height)
{
    return write_ppm_any(path, rgb, width, height);
}

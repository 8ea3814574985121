// rt_host.cpp — host side of the C ABI: cameras, scene vocabulary, BVH builders, flattening.
//
// The reference builds its world out of ~1.5K single-object device allocations, each constructed by
// a <<<1,1>>> placement-new kernel so that vtables are device-valid (utilities/cuda_utilities/
// cuda_utils.cuh:9-23; SphereHittable.cuh:134-154).  Here the same vocabulary produces three flat
// host arrays (nodes 32 B, primitives 32 B, materials 32 B) that one hipMemcpy each puts in HBM.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rt06.h"
#include "rt_internal.hpp"
#include "rt_math.hpp"

// ---------------------------------------------------------------------------------------------
// error reporting
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

int rt_fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
extern "C" const char* rt_last_error(void) { return g_last_error.c_str(); }
#ifndef RT06_SRC_SHA256
#define RT06_SRC_SHA256 "unstamped"
#endif
// the documented defaults of the denoiser (rt06.h); host only
extern "C" int rt_denoise_params_default(rt_denoise_params* out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_denoise_params_default: null out");
    out->iterations = 5;
    out->sigma_depth = 0.05f;
    out->sigma_lum = 4.0f;
    out->demodulate = 1;
    return RT_OK;
}

extern "C" const char* rt_version(void) { return "rt06-amd 0.3 (gfx950) src " RT06_SRC_SHA256; }
extern "C" const char* rt_source_hash(void) { return RT06_SRC_SHA256; }

// ---------------------------------------------------------------------------------------------
// cameras — rt_engine/shaders/cu_Cameras.cuh ctors (:16-25, :40-52, :73-85)
// ---------------------------------------------------------------------------------------------
static void camera_basis(const float lookfrom[3], const float lookat[3], const float up[3], float vfov, float aspect,
                         bool prescale, rt_camera* c) {
    float theta = radians(vfov);
    float vh = tanf(theta * 0.5f);
    float vw = vh * aspect;
    f3 w = normalize(ld3(lookat) - ld3(lookfrom));
    f3 u = normalize(cross(ld3(up), w));
    if (prescale) u = u * vw;
    f3 v = normalize(cross(w, u));
    if (prescale) v = v * vh;
    std::memset(c, 0, sizeof(*c));
    st3(c->o, ld3(lookfrom)); st3(c->u, u); st3(c->v, v); st3(c->w, w);
    c->viewport_width = vw; c->viewport_height = vh;
    c->t0 = 0.0f; c->t1 = 1.0f;
}
extern "C" int rt_camera_pinhole(const float lookfrom[3], const float lookat[3], const float up[3], float vfov,
                                 float aspect, rt_camera* out) {
    if (!lookfrom || !lookat || !up || !out) return rt_fail(RT_ERR_INVALID, "rt_camera_pinhole: null argument");
    camera_basis(lookfrom, lookat, up, vfov, aspect, true, out);
    out->type = RT_CAM_PINHOLE;
    return RT_OK;
}
extern "C" int rt_camera_defocus(const float lookfrom[3], const float lookat[3], const float up[3], float vfov,
                                 float aspect, float aperture, float focus_dist, rt_camera* out) {
    if (!lookfrom || !lookat || !up || !out) return rt_fail(RT_ERR_INVALID, "rt_camera_defocus: null argument");
    camera_basis(lookfrom, lookat, up, vfov, aspect, false, out);
    out->type = RT_CAM_DEFOCUS;
    out->lens_radius = aperture * 0.5f;
    out->focus_dist = focus_dist;
    return RT_OK;
}
extern "C" int rt_camera_motion(const float lookfrom[3], const float lookat[3], const float up[3], float vfov,
                                float aspect, float time0, float time1, rt_camera* out) {
    if (!lookfrom || !lookat || !up || !out) return rt_fail(RT_ERR_INVALID, "rt_camera_motion: null argument");
    camera_basis(lookfrom, lookat, up, vfov, aspect, true, out);
    out->type = RT_CAM_MOTION;
    out->t0 = time0; out->t1 = time1;
    return RT_OK;
}

// the lens cameras (rt06.h): what a record of type 16 to 19 must satisfy; the three reference types pass as they always did
int rt_camera_check(const char* who, const rt_camera* c) {
    if (c->type <= RT_CAM_MOTION) return RT_OK;
    if (c->type < RT_CAM_PERSPECTIVE || c->type > RT_CAM_PANORAMA) return rt_fail(RT_ERR_INVALID, "%s: unknown camera type %u", who, c->type);
    const struct { const char* name; const float* p; int n; } fields[] = {
        {"o", c->o, 3}, {"u", c->u, 3}, {"v", c->v, 3}, {"w", c->w, 3}, {"viewport_width", &c->viewport_width, 1}, {"viewport_height", &c->viewport_height, 1},
        {"lens_radius", &c->lens_radius, 1}, {"focus_dist", &c->focus_dist, 1}, {"t0", &c->t0, 1}, {"t1", &c->t1, 1}};
    for (const auto& f : fields)
        for (int k = 0; k < f.n; k++)
            if (!std::isfinite(f.p[k])) return rt_fail(RT_ERR_INVALID, "%s: camera field %s is not finite", who, f.name);
    const float a = c->viewport_width, b = c->viewport_height;
    if (!(a > 0.0f)) return rt_fail(RT_ERR_INVALID, "%s: camera field viewport_width (the projection's first parameter) must be > 0, is %g", who, (double)a);
    if (!(b > 0.0f)) return rt_fail(RT_ERR_INVALID, "%s: camera field viewport_height (the projection's second parameter) must be > 0, is %g", who, (double)b);
    if (c->lens_radius < 0.0f) return rt_fail(RT_ERR_INVALID, "%s: camera field lens_radius must be >= 0, is %g", who, (double)c->lens_radius);
    if (c->lens_radius > 0.0f && !(c->focus_dist > 0.0f))
        return rt_fail(RT_ERR_INVALID, "%s: camera field focus_dist must be > 0 where there is a lens, is %g", who, (double)c->focus_dist);
    const double pi = 3.14159265358979323846;
    if (c->type == RT_CAM_FISHEYE && std::sqrt((double)a * a + (double)b * b) >= pi)
        return rt_fail(RT_ERR_INVALID, "%s: camera fields viewport_width, viewport_height: a fisheye's corner angle sqrt(a^2 + b^2) = %g must stay below pi", who,
                       std::sqrt((double)a * a + (double)b * b));
    // pi and pi / 2 as fp32 holds them: what radians(360) / 2 and radians(180) / 2 give
    if (c->type == RT_CAM_PANORAMA && a > 0x1.921fb6p+1f) return rt_fail(RT_ERR_INVALID, "%s: camera field viewport_width: a panorama's half horizontal span must be <= pi, is %g", who, (double)a);
    if (c->type == RT_CAM_PANORAMA && b > 0x1.921fb6p+0f) return rt_fail(RT_ERR_INVALID, "%s: camera field viewport_height: a panorama's half vertical span must be <= pi / 2, is %g", who, (double)b);
    return RT_OK;
}
// one body for the four constructors: rt_camera_defocus's basis, then the projection's (a, b), the lens and the shutter; *out is written only when the record is valid
static int lens_camera(const char* who, uint32_t type, const float lookfrom[3], const float lookat[3], const float up[3], float vfov, float aspect, bool own_ab, float a,
                       float b, float aperture, float focus_dist, float time0, float time1, rt_camera* out) {
    if (!lookfrom || !lookat || !up || !out) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    rt_camera c;
    camera_basis(lookfrom, lookat, up, vfov, aspect, false, &c);
    c.type = type;
    if (own_ab) { c.viewport_width = a; c.viewport_height = b; }
    c.lens_radius = aperture * 0.5f;
    c.focus_dist = focus_dist;
    c.t0 = time0; c.t1 = time1;
    if (const int rc = rt_camera_check(who, &c)) return rc;
    *out = c;
    return RT_OK;
}
extern "C" int rt_camera_perspective(const float lookfrom[3], const float lookat[3], const float up[3], float vfov, float aspect, float aperture, float focus_dist,
                                     float time0, float time1, rt_camera* out) {
    return lens_camera("rt_camera_perspective", RT_CAM_PERSPECTIVE, lookfrom, lookat, up, vfov, aspect, false, 0.0f, 0.0f, aperture, focus_dist, time0, time1, out);
}
extern "C" int rt_camera_orthographic(const float lookfrom[3], const float lookat[3], const float up[3], float height, float aspect, float aperture, float focus_dist,
                                      float time0, float time1, rt_camera* out) {
    const float b = height * 0.5f;
    return lens_camera("rt_camera_orthographic", RT_CAM_ORTHOGRAPHIC, lookfrom, lookat, up, 90.0f, 1.0f, true, b * aspect, b, aperture, focus_dist, time0, time1, out);
}
extern "C" int rt_camera_fisheye(const float lookfrom[3], const float lookat[3], const float up[3], float fov, float aspect, float aperture, float focus_dist,
                                 float time0, float time1, rt_camera* out) {
    const float b = radians(fov) * 0.5f;
    return lens_camera("rt_camera_fisheye", RT_CAM_FISHEYE, lookfrom, lookat, up, 90.0f, 1.0f, true, b * aspect, b, aperture, focus_dist, time0, time1, out);
}
extern "C" int rt_camera_panorama(const float lookfrom[3], const float lookat[3], const float up[3], float hspan_degrees, float vspan_degrees, float aperture,
                                  float focus_dist, float time0, float time1, rt_camera* out) {
    return lens_camera("rt_camera_panorama", RT_CAM_PANORAMA, lookfrom, lookat, up, 90.0f, 1.0f, true, radians(hspan_degrees) * 0.5f, radians(vspan_degrees) * 0.5f,
                       aperture, focus_dist, time0, time1, out);
}

// ---------------------------------------------------------------------------------------------
// aabb — rt_engine/geometry/aabb.cuh (host-side members used by the builders)
// ---------------------------------------------------------------------------------------------
struct Box {
    f3 mn, mx;
};
static Box box_empty() { return Box{mk3(1e9f), mk3(-1e9f)}; }                                  // aabb.cuh:17
static Box box_union(const Box& a, const Box& b) { return Box{glm_min(a.mn, b.mn), glm_max(a.mx, b.mx)}; }  // :19,:24
static int box_longest_axis(const Box& b) {                                                    // :46-53
    f3 s = b.mx - b.mn;
    s = mk3(fabsf(s.x), fabsf(s.y), fabsf(s.z));
    if (s.x > s.y) return s.x > s.z ? 0 : 2;
    return s.y > s.z ? 1 : 2;
}
static float box_surface_area(const Box& b) {                                                  // :55-64
    f3 s = b.mx - b.mn;
    if (s.x < 0 || s.y < 0 || s.z < 0) return 0.0f;
    float cost = 0.0f;
    cost += s.x * s.y; cost += s.x * s.z; cost += s.y * s.z;
    return 2.0f * cost;
}
static f3 box_centroid(const Box& b) { return (b.mx + b.mn) * 0.5f; }                          // :66-68
static float axis_of(f3 a, int ax) { return ax == 0 ? a.x : (ax == 1 ? a.y : a.z); }

// getSphereBounds / getMovingSphereBounds, SphereHittable.cu:52-54, 85-89
// Host probe: the aabb helpers the builders are made of (aabb.cuh:19,24,46-68,78-88), over arrays — checked against fixtures
// generated from the reference's own aabb.cuh (tests/golden/ref_aabbmisc_*).  boxes n*12 (a.min a.max b.min b.max) ->
// out n*20 [longest axis, surface area, centroid 3, union min 3 max 3, a += b min 3 max 3, a.min < b.min per axis 3]
extern "C" int rt_probe_aabb_misc(size_t n, const float* boxes, float* out) {
    if (!boxes || !out) return rt_fail(RT_ERR_INVALID, "rt_probe_aabb_misc: null argument");
    for (size_t i = 0; i < n; i++) {
        const Box a{ld3(boxes + 12 * i), ld3(boxes + 12 * i + 3)}, b{ld3(boxes + 12 * i + 6), ld3(boxes + 12 * i + 9)};
        float* o = out + 20 * i;
        o[0] = (float)box_longest_axis(a);
        o[1] = box_surface_area(a);
        st3(o + 2, box_centroid(a));
        const Box u = box_union(a, b);
        st3(o + 5, u.mn); st3(o + 8, u.mx);
        Box acc = a;
        acc = box_union(acc, b);
        st3(o + 11, acc.mn); st3(o + 14, acc.mx);
        o[17] = a.mn.x < b.mn.x ? 1.0f : 0.0f; o[18] = a.mn.y < b.mn.y ? 1.0f : 0.0f; o[19] = a.mn.z < b.mn.z ? 1.0f : 0.0f;
    }
    return RT_OK;
}

static Box prim_bounds(const rt_prim& p) {
    f3 r = mk3(p.radius);
    Box b0{ld3(p.c0) - r, ld3(p.c0) + r};
    if (!(p.mat & RT_PRIM_MOVING)) return b0;
    Box b1{ld3(p.c1) - r, ld3(p.c1) + r};
    return box_union(b0, b1);
}

// ---------------------------------------------------------------------------------------------
// rt_scene
// ---------------------------------------------------------------------------------------------
struct rt_scene {
    std::vector<rt_prim> prims;
    std::vector<rt_quad> quads;           // the parallelograms, then the n_tris triangles (rt_quad::kind), whatever the order of the calls
    uint32_t n_tris = 0;
    std::vector<rt_tri_normals> tri_vn;   // vertex normals: one record per triangle, in the triangles' order (nine zeros = flat); moves with them
    uint32_t n_smooth = 0;                // how many of those records are not flat: 0 = the scene has no table
    std::vector<rt_tri_uvs> tri_uv;       // texture coordinates: parallel to tri_vn; a triangle without any holds the identity (0,0), (1,0), (0,1)
    uint32_t background = 0;
    float background_color[3] = {0.0f, 0.0f, 0.0f};
    std::vector<float> env;               // environment map (background == 2): env_w x env_h texels of 3 floats, row 0 at the top
    uint32_t env_w = 0, env_h = 0;
    float env_u0 = 0.0f;                  // its rotation about y as a shift of u, in [0, 1)
    uint32_t traversal = RT_TRAVERSAL_STACK;
    std::vector<rt_material> mats;
    std::vector<rt_perlin> perlin;        // 0 or 1 table set (RT_MAT_LAMBERTIAN_NOISE)
    std::vector<uint8_t> image;           // RGB8 (RT_MAT_LAMBERTIAN_IMAGE)
    uint32_t image_w = 0, image_h = 0;
    // the texture table: entry 0 = `image` above under image_modes[0]; entries 1.. = more_images; `table` and `table_texels` are what
    // rt_scene_textures last handed out
    struct Image { uint32_t w = 0, h = 0; std::vector<uint8_t> rgb; };
    std::vector<Image> more_images;
    std::vector<uint32_t> image_wrap = {RT_WRAP_CLAMP}, image_filter = {RT_FILTER_NEAREST};   // one per entry, entry 0 included
    mutable std::vector<rt_texture> table;
    mutable std::vector<uint8_t> table_texels;
    std::vector<rt_normal_map> nmaps;    // normal maps: a record per material, grown on demand (a material behind its end has none)
    mutable std::vector<rt_normal_map> nmap_table;   // what rt_scene_normal_maps last handed out
    std::vector<rt_microfacet> mfacs;    // microfacet surfaces: likewise
    mutable std::vector<rt_microfacet> mfac_table;
    std::vector<rt_interior> interiors;  // solid glass: likewise
    mutable std::vector<rt_interior> interior_table;
    std::vector<rt_cutout> cutouts;      // alpha cutouts: likewise
    mutable std::vector<rt_cutout> cutout_table;
    std::vector<rt_bvh_node> nodes;     // world nodes (BVH or bvh_node tree)
    std::vector<rt_bvh_node> tree_nodes;  // bvh_node objects created by rt_scene_add_bvh_node
    uint32_t kind = RT_WORLD_LIST;
    int32_t root = 0;
    uint32_t max_stack = 0;
    Box bounds = box_empty();
    bool world_set = false;
};

extern "C" int rt_scene_create(rt_scene** out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_scene_create: null out");
    *out = new rt_scene();
    return RT_OK;
}
extern "C" void rt_scene_destroy(rt_scene* s) { delete s; }

extern "C" int rt_scene_add_material(rt_scene* s, uint32_t type, const float albedo[3], float param,
                                     const float albedo2[3], int32_t* out_id) {
    if (!s || !albedo) return rt_fail(RT_ERR_INVALID, "rt_scene_add_material: null argument");
    if (type > RT_MAT_LAMBERTIAN_IMAGE) return rt_fail(RT_ERR_INVALID, "rt_scene_add_material: unknown material type %u", type);
    if (type == RT_MAT_ISOTROPIC && !(param > 0.0f)) return rt_fail(RT_ERR_INVALID, "rt_scene_add_material: a constant medium needs a density > 0");
    if (type == RT_MAT_LAMBERTIAN_IMAGE && albedo2 && !rt_image_index_ok(albedo2[0]))   // §25: albedo2[0] names the image (param means nothing for this type)
        return rt_fail(RT_ERR_INVALID, "rt_scene_add_material: an image texture's albedo2[0] is its image index: an integer in [0, %u), not %g", RT_MAX_IMAGES, (double)albedo2[0]);
    rt_material m;
    std::memset(&m, 0, sizeof(m));
    st3(m.albedo, ld3(albedo));
    m.param = param;
    if (albedo2) st3(m.albedo2, ld3(albedo2));
    m.type = type;
    s->mats.push_back(m);
    if (out_id) *out_id = (int32_t)s->mats.size() - 1;
    return RT_OK;
}

static int add_prim(rt_scene* s, const float c0[3], const float c1[3], float radius, int32_t mat, bool moving, int32_t* out_prim) {
    if (!s || !c0 || !c1) return rt_fail(RT_ERR_INVALID, "add sphere: null argument");
    if (mat < 0 || (size_t)mat >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "add sphere: material index %d out of range", mat);
    rt_prim p;
    st3(p.c0, ld3(c0)); st3(p.c1, ld3(c1));
    p.radius = radius;
    p.mat = (uint32_t)mat | (moving ? RT_PRIM_MOVING : 0u);
    s->prims.push_back(p);
    s->world_set = false;
    if (out_prim) *out_prim = (int32_t)s->prims.size() - 1;
    return RT_OK;
}
extern "C" int rt_scene_add_sphere(rt_scene* s, const float center[3], float radius, int32_t mat, int32_t* out_prim) {
    return add_prim(s, center, center, radius, mat, false, out_prim);
}
extern "C" int rt_scene_add_moving_sphere(rt_scene* s, const float c0[3], const float c1[3], float radius, int32_t mat,
                                          int32_t* out_prim) {
    return add_prim(s, c0, c1, radius, mat, true, out_prim);
}
extern "C" int rt_scene_prim_bounds(const rt_scene* s, int32_t prim, float out_min[3], float out_max[3]) {
    if (!s || prim < 0 || (size_t)prim >= s->prims.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_prim_bounds: bad primitive %d", prim);
    Box b = prim_bounds(s->prims[prim]);
    st3(out_min, b.mn); st3(out_max, b.mx);
    return RT_OK;
}

// ---- quads (not in the reference; "Ray Tracing: The Next Week" quad(Q,u,v)) -------------------------
static void quad_finalize(rt_quad& q) {
    f3 n = cross(ld3(q.u), ld3(q.v));
    f3 normal = normalize(n);
    st3(q.normal, normal);
    q.D = dot(normal, ld3(q.Q));
    st3(q.w, n / dot(n, n));
    q.pad1 = q.pad2 = 0.0f;
}
static Box box_of_points(f3 a, f3 b) { return Box{glm_min(a, b), glm_max(a, b)}; }
// bbox = box(Q, Q+u+v) U box(Q+u, Q+v), every axis padded to at least 0.0001 (the book's aabb::pad_to_minimums)
static Box quad_bounds(const rt_quad& q) {
    f3 Q = ld3(q.Q), u = ld3(q.u), v = ld3(q.v);
    Box b = box_union(box_of_points(Q, Q + u + v), box_of_points(Q + u, Q + v));
    const float delta = 0.0001f;
    if (b.mx.x - b.mn.x < delta) { b.mn.x -= delta / 2; b.mx.x += delta / 2; }
    if (b.mx.y - b.mn.y < delta) { b.mn.y -= delta / 2; b.mx.y += delta / 2; }
    if (b.mx.z - b.mn.z < delta) { b.mn.z -= delta / 2; b.mx.z += delta / 2; }
    return b;
}
// a triangle (rt_quad::kind == RT_QUAD_TRIANGLE): the box of its vertices Q, Q + u, Q + v, padded like a quad's
static Box tri_bounds(const rt_quad& q) {
    f3 Q = ld3(q.Q), u = ld3(q.u), v = ld3(q.v);
    Box b = box_union(box_of_points(Q, Q + u), box_of_points(Q + v, Q + v));
    const float delta = 0.0001f;
    if (b.mx.x - b.mn.x < delta) { b.mn.x -= delta / 2; b.mx.x += delta / 2; }
    if (b.mx.y - b.mn.y < delta) { b.mn.y -= delta / 2; b.mx.y += delta / 2; }
    if (b.mx.z - b.mn.z < delta) { b.mn.z -= delta / 2; b.mx.z += delta / 2; }
    return b;
}
static Box quad_record_bounds(const rt_quad& q) { return q.kind == RT_QUAD_TRIANGLE ? tri_bounds(q) : quad_bounds(q); }
extern "C" int rt_scene_add_quad(rt_scene* s, const float Q[3], const float u[3], const float v[3], int32_t mat, int32_t* out_quad) {
    if (!s || !Q || !u || !v) return rt_fail(RT_ERR_INVALID, "rt_scene_add_quad: null argument");
    if (mat < 0 || (size_t)mat >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_add_quad: material index %d out of range", mat);
    rt_quad q;
    std::memset(&q, 0, sizeof(q));
    st3(q.Q, ld3(Q)); st3(q.u, ld3(u)); st3(q.v, ld3(v));
    q.mat = (uint32_t)mat;
    quad_finalize(q);
    const size_t at = s->quads.size() - s->n_tris;   // in front of the triangles
    s->quads.insert(s->quads.begin() + at, q);
    s->world_set = false;
    if (out_quad) *out_quad = (int32_t)at;
    return RT_OK;
}

// ---- triangles and meshes (not in the reference; the `tri` of "Ray Tracing: The Next Week": a quad with another interior test) ----
// the record of triangle (a, b, c), or false for a degenerate face: dot(n, n) of n = cross(b - a, c - a) not finite and > 0
static const rt_tri_uvs RT_TRI_UVS_IDENTITY = {{0.0f, 0.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}};   // §22: under it a triangle's texture coordinates are its planar ones
static bool tri_record(f3 a, f3 b, f3 c, uint32_t mat, rt_quad& q) {
    std::memset(&q, 0, sizeof(q));
    st3(q.Q, a); st3(q.u, b - a); st3(q.v, c - a);
    q.mat = mat;
    q.kind = RT_QUAD_TRIANGLE;
    const f3 n = cross(ld3(q.u), ld3(q.v));
    const float nn = dot(n, n);
    if (!(std::isfinite(nn) && nn > 0.0f)) return false;
    quad_finalize(q);
    return true;
}
extern "C" int rt_scene_add_triangle(rt_scene* s, const float a[3], const float b[3], const float c[3], int32_t mat, int32_t* out_quad) {
    if (!s || !a || !b || !c) return rt_fail(RT_ERR_INVALID, "rt_scene_add_triangle: null argument");
    if (mat < 0 || (size_t)mat >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_add_triangle: material index %d out of range", mat);
    rt_quad q;
    if (!tri_record(ld3(a), ld3(b), ld3(c), (uint32_t)mat, q))
        return rt_fail(RT_ERR_INVALID, "rt_scene_add_triangle: degenerate triangle (the squared length of cross(b - a, c - a) is not finite and > 0)");
    s->quads.push_back(q);
    s->tri_vn.push_back(rt_tri_normals{});
    s->tri_uv.push_back(RT_TRI_UVS_IDENTITY);
    s->n_tris++;
    s->world_set = false;
    if (out_quad) *out_quad = (int32_t)s->quads.size() - 1;
    return RT_OK;
}
// a vertex normal as the scene keeps it: finite, of non-zero length, normalised (x / sqrt(dot(x, x)) per component); false otherwise
static bool unit_normal(f3 x, float out[3]) {
    const float l2 = dot(x, x);
    if (!(std::isfinite(l2) && l2 > 0.0f)) return false;
    st3(out, x / sqrtf(l2));
    return std::isfinite(out[0]) && std::isfinite(out[1]) && std::isfinite(out[2]) && !(out[0] == 0.0f && out[1] == 0.0f && out[2] == 0.0f);
}
extern "C" int rt_scene_add_triangle_smooth(rt_scene* s, const float a[3], const float b[3], const float c[3], const float na[3], const float nb[3], const float nc[3],
                                            int32_t mat, int32_t* out_quad) {
    if (!s || !a || !b || !c || !na || !nb || !nc) return rt_fail(RT_ERR_INVALID, "rt_scene_add_triangle_smooth: null argument");
    rt_tri_normals vn;
    if (!unit_normal(ld3(na), vn.n0) || !unit_normal(ld3(nb), vn.n1) || !unit_normal(ld3(nc), vn.n2))
        return rt_fail(RT_ERR_INVALID, "rt_scene_add_triangle_smooth: a vertex normal is not finite or has zero length");
    if (const int rc = rt_scene_add_triangle(s, a, b, c, mat, out_quad)) return rc;
    s->tri_vn.back() = vn;
    s->n_smooth++;
    return RT_OK;
}
extern "C" int rt_scene_add_triangle_uv(rt_scene* s, const float a[3], const float b[3], const float c[3], const float na[3], const float nb[3], const float nc[3],
                                        const float ta[2], const float tb[2], const float tc[2], int32_t mat, int32_t* out_quad) {
    if (!s || !a || !b || !c || !ta || !tb || !tc) return rt_fail(RT_ERR_INVALID, "rt_scene_add_triangle_uv: null argument");
    if ((na == nullptr) != (nb == nullptr) || (na == nullptr) != (nc == nullptr)) return rt_fail(RT_ERR_INVALID, "rt_scene_add_triangle_uv: three vertex normals or none");
    const rt_tri_uvs uv = {{ta[0], ta[1]}, {tb[0], tb[1]}, {tc[0], tc[1]}};
    for (int k = 0; k < 6; k++)
        if (!std::isfinite(uv.t0[k])) return rt_fail(RT_ERR_INVALID, "rt_scene_add_triangle_uv: a texture coordinate is not finite");
    if (const int rc = na ? rt_scene_add_triangle_smooth(s, a, b, c, na, nb, nc, mat, out_quad) : rt_scene_add_triangle(s, a, b, c, mat, out_quad)) return rc;
    s->tri_uv.back() = uv;
    return RT_OK;
}
extern "C" int rt_scene_texture_coords(const rt_scene* s, const rt_tri_uvs** out, uint32_t* out_n) {
    if (!s || !out || !out_n) return rt_fail(RT_ERR_INVALID, "rt_scene_texture_coords: null argument");
    bool any = false;
    for (const rt_tri_uvs& r : s->tri_uv)
        if (!(r.t0[0] == 0.0f && r.t0[1] == 0.0f && r.t1[0] == 1.0f && r.t1[1] == 0.0f && r.t2[0] == 0.0f && r.t2[1] == 1.0f)) { any = true; break; }
    *out = any ? s->tri_uv.data() : nullptr;
    *out_n = any ? (uint32_t)s->tri_uv.size() : 0u;
    return RT_OK;
}
extern "C" int rt_scene_vertex_normals(const rt_scene* s, const rt_tri_normals** out, uint32_t* out_n) {
    if (!s || !out || !out_n) return rt_fail(RT_ERR_INVALID, "rt_scene_vertex_normals: null argument");
    *out = s->n_smooth ? s->tri_vn.data() : nullptr;
    *out_n = s->n_smooth ? (uint32_t)s->tri_vn.size() : 0u;
    return RT_OK;
}
extern "C" int rt_scene_set_background(rt_scene* s, uint32_t mode, const float color[3]) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_background: null scene");
    if (mode > 1) return rt_fail(RT_ERR_INVALID, "rt_scene_set_background: unknown mode %u", mode);
    s->background = mode;
    if (color) st3(s->background_color, ld3(color));
    s->env.clear(); s->env_w = s->env_h = 0u; s->env_u0 = 0.0f;   // the gradient and the constant colour drop an environment map
    return RT_OK;
}
// what rt_scene_set_environment and rt_renderer_environment refuse of an image; null = nothing
const char* rt_environment_image_refusal(uint32_t width, uint32_t height, const float* rgb) {
    if (width == 0u || height == 0u) return "a dimension is zero";
    if ((uint64_t)width * height > (uint64_t)RT_ENV_MAX_TEXELS) return "more than 2^25 texels";
    if (!rgb) return "null image";
    for (size_t i = 0; i < (size_t)width * height * 3u; i++) {
        if (!std::isfinite(rgb[i])) return "a texel that is not finite";
        if (rgb[i] < 0.0f) return "a negative texel";
    }
    return nullptr;
}
// The sampling distribution of an environment map, built in double and stored as fp32: see rt_environment_distribution in rt06.h.
const char* rt_environment_distribution_refusal(uint32_t width, uint32_t height, const float* rgb, float* rowc, float* rowy, float* colc, float* density) {
    const size_t W = width, H = height;
    const double pi = 3.14159265358979323846;
    for (size_t j = 0; j <= H; j++) rowy[j] = j == 0 ? 1.0f : j == H ? -1.0f : (float)std::cos(pi * (double)j / (double)H);
    double total = 0.0;
    for (size_t j = 0; j < H; j++) {
        const double h = (double)rowy[j] - (double)rowy[j + 1];
        double row = 0.0;
        for (size_t i = 0; i < W; i++) {
            const float* t = rgb + (j * W + i) * 3u;
            row += ((0.2126 * (double)t[0] + 0.7152 * (double)t[1]) + 0.0722 * (double)t[2]) * h;
            colc[j * W + i] = (float)row;
        }
        total += row;
        rowc[j] = (float)total;
    }
    const double A = (double)rowc[H - 1];
    if (!(A > 0.0)) return "the map is all black: nothing to sample";
    if (!std::isfinite(rowc[H - 1])) return "the map's radiance times solid angle does not sum to a finite fp32 number";
    for (size_t j = 0; j < H; j++) {   // from the stored values: what the binary searches really draw
        const double omega = (2.0 * pi / (double)W) * ((double)rowy[j] - (double)rowy[j + 1]);
        const double Pj = ((double)rowc[j] - (j ? (double)rowc[j - 1] : 0.0)) / A;
        const double R = (double)colc[j * W + W - 1];
        for (size_t i = 0; i < W; i++) {
            const double Pi = R > 0.0 ? ((double)colc[j * W + i] - (i ? (double)colc[j * W + i - 1] : 0.0)) / R : 0.0;
            density[j * W + i] = (Pj > 0.0 && Pi > 0.0) ? (float)((Pj * Pi) / omega) : 0.0f;
        }
    }
    return nullptr;
}
extern "C" int rt_environment_distribution(uint32_t width, uint32_t height, const float* rgb, float* rowc, float* rowy, float* colc, float* density) {
    if (const char* why = rt_environment_image_refusal(width, height, rgb)) return rt_fail(RT_ERR_INVALID, "rt_environment_distribution: %s", why);
    if (!rowc || !rowy || !colc || !density) return rt_fail(RT_ERR_INVALID, "rt_environment_distribution: null argument");
    if (const char* why = rt_environment_distribution_refusal(width, height, rgb, rowc, rowy, colc, density)) return rt_fail(RT_ERR_INVALID, "rt_environment_distribution: %s", why);
    return RT_OK;
}

extern "C" int rt_scene_set_environment(rt_scene* s, uint32_t width, uint32_t height, const float* rgb, float rotate_y_degrees) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_environment: null scene");
    if (const char* why = rt_environment_image_refusal(width, height, rgb)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_environment: %s", why);
    if (!std::isfinite(rotate_y_degrees)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_environment: the rotation is not finite");
    const double turns = (double)rotate_y_degrees / 360.0;
    float u0 = (float)(turns - std::floor(turns));   // frac: in [0, 1] after the rounding to fp32
    if (!(u0 < 1.0f)) u0 = 0.0f;
    s->env.assign(rgb, rgb + (size_t)width * height * 3u);
    s->env_w = width; s->env_h = height; s->env_u0 = u0;
    s->background = 2u;
    return RT_OK;
}
extern "C" int rt_scene_environment(const rt_scene* s, uint32_t* out_w, uint32_t* out_h, const float** out_rgb, float* out_u0) {
    if (!s || !out_w || !out_h || !out_rgb || !out_u0) return rt_fail(RT_ERR_INVALID, "rt_scene_environment: null argument");
    *out_w = s->env_w; *out_h = s->env_h; *out_u0 = s->env_u0;
    *out_rgb = s->env.empty() ? nullptr : s->env.data();
    return RT_OK;
}

extern "C" int rt_scene_set_traversal(rt_scene* s, uint32_t mode) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_traversal: null scene");
    if (mode > RT_TRAVERSAL_WIDE4) return rt_fail(RT_ERR_INVALID, "rt_scene_set_traversal: unknown mode %u", mode);
    s->traversal = mode;
    return RT_OK;
}

// ---- BVH_Handle::Factory (rt_engine/geometry/BVH.cu:156-384) --------------------------------
namespace {
struct Item {
    Box b;
    bool is_quad;
    rt_prim p;
    rt_quad q;
    rt_tri_normals vn;   // of a triangle: its vertex normals travel with it
    rt_tri_uvs uv;       // ... and its texture coordinates (§22)
};
struct Builder {
    std::vector<Item> arr;
    std::vector<rt_bvh_node>& nodes;
    explicit Builder(std::vector<rt_bvh_node>& n) : nodes(n) {}

    int32_t push(const Box& b, int32_t l, int32_t r) {
        rt_bvh_node n;
        st3(n.min, b.mn); st3(n.max, b.mx);
        n.left = l; n.right = r;
        nodes.push_back(n);
        return (int32_t)nodes.size() - 1;
    }
    Box partition_bounds(int start, int end) const {  // _get_partition_bounds, BVH.cu:306-312
        Box b = box_empty();
        for (int i = start; i < end; i++) b = box_union(b, arr[i].b);
        return b;
    }
    // The reference sorts with std::sort (unstable) on bounds.min[axis] only (BVH.cu:195-199,
    // aabb.cuh:78-88), so equal keys land in an STL-specific order.  A stable sort pins that order.
    void sort_axis(int start, int end, int axis) {
        std::stable_sort(arr.begin() + start, arr.begin() + end,
                         [axis](const Item& a, const Item& b) { return axis_of(a.b.mn, axis) < axis_of(b.b.mn, axis); });
    }
    int32_t rec1(int start, int end) {  // _build_bvh_rec1, BVH.cu:180-210
        Box bounds = partition_bounds(start, end);
        int axis = box_longest_axis(bounds);
        if (end - start == 1) return push(bounds, -1, start);
        sort_axis(start, end, axis);
        int mid = (start + end) / 2;
        int32_t l = rec1(start, mid);
        int32_t r = rec1(mid, end);
        return push(bounds, l, r);
    }
    void find_optimal_split(int start, int end, const Box& bounds, int& best_axis, float& best_split) const {  // BVH.cu:241-279
        const int split_points = 16;
        float best_cost = RT_MISS_DIST;
        best_axis = 0; best_split = 0.0f;
        for (int axis = 0; axis < 3; axis++)
            for (int split = 0; split < split_points; split++) {
                float pos = ((float)split + 1.0f) / ((float)split_points + 1.0f);
                pos = mix(axis_of(bounds.mn, axis), axis_of(bounds.mx, axis), pos);
                Box lb = box_empty(), rb = box_empty();
                int lc = 0, rc = 0;
                for (int i = start; i < end; i++) {
                    const Box& b = arr[i].b;
                    if (axis_of(box_centroid(b), axis) < pos) { lb = box_union(lb, b); lc++; }
                    else { rb = box_union(rb, b); rc++; }
                }
                float cost = box_surface_area(lb) * (float)lc + box_surface_area(rb) * (float)rc;
                if (cost < best_cost) { best_cost = cost; best_axis = axis; best_split = pos; }
            }
    }
    int partition_by_split(int start, int end, int axis, float split_pos) {  // BVH.cu:281-304
        int i = start, j = end;
        while (i < j) {
            if (axis_of(box_centroid(arr[i].b), axis) < split_pos) i++;
            else std::swap(arr[i], arr[--j]);
        }
        return i;
    }
    // _build_bvh_rec2, BVH.cu:212-239.  When the chosen plane leaves one side empty the reference
    // recurses on an empty range forever; this falls back to rec1's median split for that range.
    int32_t rec2(int start, int end) {
        Box bounds = partition_bounds(start, end);
        if (end - start == 1) return push(bounds, -1, start);
        int axis; float split;
        find_optimal_split(start, end, bounds, axis, split);
        int mid = partition_by_split(start, end, axis, split);
        if (mid == start || mid == end) {
            sort_axis(start, end, box_longest_axis(bounds));
            mid = (start + end) / 2;
        }
        int32_t l = rec2(start, mid);
        int32_t r = rec2(mid, end);
        return push(bounds, l, r);
    }
    // BuildBVH_BottomUp + _find_optimal_merge + _merge_nodes, BVH.cu:315-384
    int32_t bottom_up() {
        struct BN { Box b; int count; int32_t idx; };
        std::vector<BN> bn;
        for (size_t i = 0; i < arr.size(); i++) bn.push_back(BN{arr[i].b, 1, push(arr[i].b, -1, (int32_t)i)});
        while (bn.size() > 1) {
            float best_cost = RT_MISS_DIST;
            size_t ba = 0, bb = 1;
            for (size_t a = 0; a < bn.size(); a++)
                for (size_t b = a + 1; b < bn.size(); b++) {
                    Box nb = box_union(bn[a].b, bn[b].b);
                    float cost = box_surface_area(nb) * (float)(bn[a].count + bn[b].count);
                    if (cost < best_cost) { ba = a; bb = b; best_cost = cost; }
                }
            BN merged{box_union(bn[ba].b, bn[bb].b), bn[ba].count + bn[bb].count, 0};
            merged.idx = push(merged.b, bn[ba].idx, bn[bb].idx);
            bn.erase(bn.begin() + bb);
            bn.erase(bn.begin() + ba);
            bn.push_back(merged);
        }
        return bn[0].idx;
    }
};

uint32_t leaf_depth(const std::vector<rt_bvh_node>& nodes, int32_t idx) {
    if (nodes[idx].left == -1) return 0;
    return 1 + std::max(leaf_depth(nodes, nodes[idx].left), leaf_depth(nodes, nodes[idx].right));
}
}  // namespace

static int build_bvh(rt_scene* s, int builder) {
    if (!s) return rt_fail(RT_ERR_INVALID, "build_bvh: null scene");
    if (s->prims.empty() && s->quads.empty()) return rt_fail(RT_ERR_INVALID, "build_bvh: scene has no primitives");
    s->nodes.clear();
    Builder B(s->nodes);
    B.arr.reserve(s->prims.size() + s->quads.size());
    const size_t n_plain = s->quads.size() - s->n_tris;
    for (const rt_prim& p : s->prims) B.arr.push_back(Item{prim_bounds(p), false, p, rt_quad{}, rt_tri_normals{}, rt_tri_uvs{}});
    for (size_t i = 0; i < s->quads.size(); i++) B.arr.push_back(Item{quad_record_bounds(s->quads[i]), true, rt_prim{}, s->quads[i], i >= n_plain ? s->tri_vn[i - n_plain] : rt_tri_normals{}, i >= n_plain ? s->tri_uv[i - n_plain] : rt_tri_uvs{}});
    int32_t root;
    if (builder == 0) root = B.rec1(0, (int)B.arr.size());
    else if (builder == 1) root = B.rec2(0, (int)B.arr.size());
    else root = B.bottom_up();
    // hittables[] = arr order (BVH.cu:174-177), kept per kind: spheres first, then quads, then triangles; leaf indices are remapped
    {
        std::vector<int32_t> unified(B.arr.size());
        const size_t ns = s->prims.size();
        size_t si = 0, qi = 0, ti = s->quads.size() - s->n_tris;
        for (size_t i = 0; i < B.arr.size(); i++) {
            if (B.arr[i].is_quad) {
                size_t& at = B.arr[i].q.kind == RT_QUAD_TRIANGLE ? ti : qi;
                if (B.arr[i].q.kind == RT_QUAD_TRIANGLE) { s->tri_vn[at - n_plain] = B.arr[i].vn; s->tri_uv[at - n_plain] = B.arr[i].uv; }
                s->quads[at] = B.arr[i].q; unified[i] = (int32_t)(ns + at); at++;
            }
            else { s->prims[si] = B.arr[i].p; unified[i] = (int32_t)si; si++; }
        }
        for (rt_bvh_node& n : s->nodes)
            if (n.left == -1) n.right = unified[n.right];
    }
    s->kind = RT_WORLD_BVH;
    s->root = root;
    s->max_stack = leaf_depth(s->nodes, root) + 1;
    s->bounds = Box{ld3(s->nodes[root].min), ld3(s->nodes[root].max)};
    s->world_set = true;
    // The reference's traversal stack holds 32 entries and is never checked (BVH.cu:17,27-35).
    if (s->max_stack > RT_MAX_STACK)
        return rt_fail(RT_ERR_STACK, "BVH needs a traversal stack of %u entries; the limit is %d (BVH.cu:17)", s->max_stack, RT_MAX_STACK);
    return RT_OK;
}
extern "C" int rt_scene_build_bvh_topdown(rt_scene* s) { return build_bvh(s, 0); }
extern "C" int rt_scene_build_bvh_sah(rt_scene* s) { return build_bvh(s, 1); }
extern "C" int rt_scene_build_bvh_bottomup(rt_scene* s) { return build_bvh(s, 2); }

extern "C" int rt_scene_set_world_list(rt_scene* s) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_world_list: null scene");
    if (s->prims.empty() && s->quads.empty()) return rt_fail(RT_ERR_INVALID, "rt_scene_set_world_list: scene has no primitives");
    s->nodes.clear();
    s->kind = RT_WORLD_LIST;
    s->root = 0;
    s->max_stack = 0;
    Box b = box_empty();
    for (const rt_prim& p : s->prims) b = box_union(b, prim_bounds(p));  // world_bounds += handle.getBounds(), Scenes.cu:61
    for (const rt_quad& q : s->quads) b = box_union(b, quad_record_bounds(q));
    s->bounds = b;
    s->world_set = true;
    return RT_OK;
}

static bool ref_valid(const rt_scene* s, int32_t ref) {
    if (ref >= 0) return (size_t)ref < s->tree_nodes.size();
    return (size_t)(-ref - 1) < s->prims.size();
}
static Box ref_bounds(const rt_scene* s, int32_t ref) {
    if (ref >= 0) return Box{ld3(s->tree_nodes[ref].min), ld3(s->tree_nodes[ref].max)};
    return prim_bounds(s->prims[-ref - 1]);
}
extern "C" int rt_scene_add_bvh_node(rt_scene* s, int32_t left_ref, int32_t right_ref, const float bmin[3],
                                     const float bmax[3], int32_t* out_ref) {
    if (!s || !out_ref) return rt_fail(RT_ERR_INVALID, "rt_scene_add_bvh_node: null argument");
    if (!ref_valid(s, left_ref) || !ref_valid(s, right_ref)) return rt_fail(RT_ERR_INVALID, "rt_scene_add_bvh_node: bad child reference");
    Box b = (bmin && bmax) ? Box{ld3(bmin), ld3(bmax)} : box_union(ref_bounds(s, left_ref), ref_bounds(s, right_ref));
    rt_bvh_node n;
    st3(n.min, b.mn); st3(n.max, b.mx);
    n.left = left_ref; n.right = right_ref;
    s->tree_nodes.push_back(n);
    *out_ref = (int32_t)s->tree_nodes.size() - 1;
    return RT_OK;
}
static uint32_t tree_depth(const rt_scene* s, int32_t ref, uint32_t guard) {
    if (ref < 0 || guard > 100000) return 0;
    return 1 + std::max(tree_depth(s, s->tree_nodes[ref].left, guard + 1), tree_depth(s, s->tree_nodes[ref].right, guard + 1));
}
extern "C" int rt_scene_set_world_node_tree(rt_scene* s, int32_t root_ref) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_world_node_tree: null scene");
    if (!ref_valid(s, root_ref)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_world_node_tree: bad root reference");
    if (!s->quads.empty()) return rt_fail(RT_ERR_INVALID, "rt_scene_set_world_node_tree: bvh_node trees take spheres only");
    s->nodes = s->tree_nodes;
    s->kind = RT_WORLD_NODE_TREE;
    s->root = root_ref;
    // iterative twin of the recursion pushes right then left: one pending sibling per level + 1
    s->max_stack = tree_depth(s, root_ref, 0) + 1;
    s->bounds = ref_bounds(s, root_ref);
    s->world_set = true;
    if (s->max_stack > RT_MAX_STACK)
        return rt_fail(RT_ERR_STACK, "bvh_node tree needs a traversal stack of %u entries; the limit is %d", s->max_stack, RT_MAX_STACK);
    return RT_OK;
}

extern "C" int rt_scene_get_flat(const rt_scene* s, rt_world_flat* out) {
    if (!s || !out) return rt_fail(RT_ERR_INVALID, "rt_scene_get_flat: null argument");
    if (!s->world_set) return rt_fail(RT_ERR_INVALID, "rt_scene_get_flat: no world built (call a build_bvh / set_world function first)");
    std::memset(out, 0, sizeof(*out));
    out->kind = s->kind;
    out->root = s->root;
    out->n_nodes = (uint32_t)s->nodes.size();
    out->n_prims = (uint32_t)s->prims.size();
    out->n_materials = (uint32_t)s->mats.size();
    out->max_stack = s->max_stack;
    st3(out->bounds_min, s->bounds.mn); st3(out->bounds_max, s->bounds.mx);
    out->nodes = s->nodes.empty() ? nullptr : s->nodes.data();
    out->prims = s->prims.empty() ? nullptr : s->prims.data();
    out->materials = s->mats.data();
    out->quads = s->quads.empty() ? nullptr : s->quads.data();
    out->n_quads = (uint32_t)s->quads.size();
    out->background = s->background;
    st3(out->background_color, ld3(s->background_color));
    out->perlin = s->perlin.empty() ? nullptr : s->perlin.data();
    out->image = s->image.empty() ? nullptr : s->image.data();
    out->image_width = s->image_w;
    out->image_height = s->image_h;
    out->traversal = s->kind == RT_WORLD_BVH ? s->traversal : (uint32_t)RT_TRAVERSAL_STACK;
    return RT_OK;
}

// perlin::perlin() ("The Next Week"): randvec[i] = unit_vector(vec3::random(-1, 1)); perm = identity shuffled by
// `for i = n-1 .. 1: swap(p[i], p[random_int(0, i)])`, three times.  Uniforms: the build's sequential host stream, id 0x9E81.
// The lights of light sampling, for both entry points below: what every mode refuses (traversal, constant medium), then the quads whose
// material is a diffuse light, in quad-index order, each with the area of its parallelogram — sqrt(dot(n, n)) of n = cross(u, v), fp32, in that order — and,
// with_spheres, the static spheres with radius > 0 whose material is a diffuse light, in primitive order, area = (12.566371f * r) * r.  `none` and `many`
// are the caller's words for an empty list and for one past RT_MAX_LIGHTS.  out_kind may be null.
static_assert(RT_MAX_LIGHTS == 16, "the refusal messages below say 16");
// The kinds of a flat world's quads: parallelograms, then triangles.  Every consumer of a caller's rt_world_flat runs this on the host
// before a kernel turns "quad index >= count of parallelograms" into "triangle".
extern "C" int rt_world_triangles(const rt_world_flat* w, uint32_t* out_n) {
    if (!w || !out_n) return rt_fail(RT_ERR_INVALID, "rt_world_triangles: null argument");
    *out_n = 0;
    if (w->n_quads && !w->quads) return rt_fail(RT_ERR_INVALID, "rt_world_triangles: world array is null");
    uint32_t n = 0;
    for (uint32_t i = 0; i < w->n_quads; i++) {
        const uint32_t kind = w->quads[i].kind;
        if (kind > RT_QUAD_TRIANGLE) return rt_fail(RT_ERR_INVALID, "quad %u: unknown kind %u (RT_QUAD_PARALLELOGRAM 0, RT_QUAD_TRIANGLE 1)", i, kind);
        if (kind == RT_QUAD_TRIANGLE) n++;
        else if (n) return rt_fail(RT_ERR_INVALID, "quad %u: a parallelogram behind a triangle (the triangles follow the parallelograms in a flat world)", i);
    }
    *out_n = n;
    return RT_OK;
}
// with_triangles: behind those, the triangles whose material is a diffuse light, in quad-index order, area = 0.5f * sqrtf(dot(n, n)).  `cap`
// is where `many` is said: RT_MAX_LIGHTS, or RT_MAX_LIGHTS_MESH for the table with triangles.
static int world_lights(const rt_world_flat* w, bool with_spheres, const char* none, const char* many, uint32_t* out_kind, uint32_t* out_index, float* out_area,
                        uint32_t* out_n, bool with_triangles = false, uint32_t cap = RT_MAX_LIGHTS) {
    if (w->traversal != RT_TRAVERSAL_STACK)
        return rt_fail(RT_ERR_INVALID, "light sampling: the world has a queue or wide4 traversal (RT_TRAVERSAL_QUEUE, RT_TRAVERSAL_WIDE4); the light-sampling kernels walk the tree with the stack");
    for (uint32_t i = 0; i < w->n_materials; i++)
        if (w->materials[i].type == RT_MAT_ISOTROPIC)
            return rt_fail(RT_ERR_INVALID, "light sampling: the world has a constant medium (RT_MAT_ISOTROPIC), whose hit test draws from the path's RNG stream");
    uint32_t n = 0, n_tris = 0;
    if (int rc = rt_world_triangles(w, &n_tris)) return rc;
    for (uint32_t i = 0; i < w->n_quads; i++) {
        const rt_quad& q = w->quads[i];
        if (q.mat >= w->n_materials) return rt_fail(RT_ERR_INVALID, "quad %u: material index out of range", i);
        if (w->materials[q.mat].type != RT_MAT_DIFFUSE_LIGHT || q.kind == RT_QUAD_TRIANGLE) continue;   // a triangle light emits when hit and is not sampled (§18)
        if (n == cap) return rt_fail(RT_ERR_INVALID, "%s", many);
        const f3 nrm = cross(mk3(q.u[0], q.u[1], q.u[2]), mk3(q.v[0], q.v[1], q.v[2]));
        if (out_kind) out_kind[n] = RT_LIGHT_QUAD;
        out_index[n] = i;
        out_area[n] = sqrtf(dot(nrm, nrm));
        n++;
    }
    for (uint32_t i = 0; with_spheres && i < w->n_prims; i++) {
        const rt_prim& pr = w->prims[i];
        const uint32_t mat = pr.mat & ~RT_PRIM_MOVING;
        if (mat >= w->n_materials) return rt_fail(RT_ERR_INVALID, "primitive %u: material index out of range", i);
        if (w->materials[mat].type != RT_MAT_DIFFUSE_LIGHT || (pr.mat & RT_PRIM_MOVING) || !(pr.radius > 0.0f)) continue;
        if (n == cap) return rt_fail(RT_ERR_INVALID, "%s", many);
        if (out_kind) out_kind[n] = RT_LIGHT_SPHERE;
        out_index[n] = i;
        out_area[n] = (12.566371f * pr.radius) * pr.radius;
        n++;
    }
    for (uint32_t i = w->n_quads - n_tris; with_triangles && i < w->n_quads; i++) {
        const rt_quad& q = w->quads[i];
        if (w->materials[q.mat].type != RT_MAT_DIFFUSE_LIGHT) continue;   // q.mat was checked above
        if (n == cap) return rt_fail(RT_ERR_INVALID, "%s", many);
        const f3 nrm = cross(mk3(q.u[0], q.u[1], q.u[2]), mk3(q.v[0], q.v[1], q.v[2]));
        if (out_kind) out_kind[n] = RT_LIGHT_TRIANGLE;
        out_index[n] = i;
        out_area[n] = 0.5f * sqrtf(dot(nrm, nrm));
        n++;
    }
    if (n == 0) return rt_fail(RT_ERR_INVALID, "%s", none);
    *out_n = n;
    return RT_OK;
}

extern "C" int rt_world_quad_lights(const rt_world_flat* w, uint32_t out_quad[RT_MAX_LIGHTS], float out_area[RT_MAX_LIGHTS], uint32_t* out_n) {
    if (!w || !out_quad || !out_area || !out_n) return rt_fail(RT_ERR_INVALID, "rt_world_quad_lights: null argument");
    *out_n = 0;
    if ((w->n_quads && !w->quads) || (w->n_materials && !w->materials)) return rt_fail(RT_ERR_INVALID, "rt_world_quad_lights: world array is null");
    return world_lights(w, false, "light sampling: the world has no quad light (a quad whose material is RT_MAT_DIFFUSE_LIGHT); sphere lights emit but are not sampled",
                        "light sampling: the world has more than 16 quad lights", nullptr, out_quad, out_area, out_n);
}

// The lights of either mode.  RT_LIGHT_SAMPLING_QUADS: rt_world_quad_lights' list and refusals.  RT_LIGHT_SAMPLING_ALL: the same quads in the same order,
// then the sphere lights; a moving sphere is not in the table and keeps emitting when hit.
extern "C" int rt_world_lights(const rt_world_flat* w, uint32_t mode, uint32_t out_kind[RT_MAX_LIGHTS], uint32_t out_index[RT_MAX_LIGHTS], float out_area[RT_MAX_LIGHTS],
                               uint32_t* out_n) {
    if (!w || !out_kind || !out_index || !out_area || !out_n) return rt_fail(RT_ERR_INVALID, "rt_world_lights: null argument");
    *out_n = 0;
    if (mode != RT_LIGHT_SAMPLING_QUADS && mode != RT_LIGHT_SAMPLING_ALL)
        return rt_fail(RT_ERR_INVALID, "rt_world_lights: mode must be RT_LIGHT_SAMPLING_QUADS (1) or RT_LIGHT_SAMPLING_ALL (2)");
    if (mode == RT_LIGHT_SAMPLING_QUADS) {
        for (uint32_t i = 0; i < RT_MAX_LIGHTS; i++) out_kind[i] = RT_LIGHT_QUAD;
        return rt_world_quad_lights(w, out_index, out_area, out_n);
    }
    if ((w->n_quads && !w->quads) || (w->n_materials && !w->materials) || (w->n_prims && !w->prims)) return rt_fail(RT_ERR_INVALID, "rt_world_lights: world array is null");
    return world_lights(w, true, "light sampling: the world has no light to sample (a quad or a static sphere of radius > 0 whose material is RT_MAT_DIFFUSE_LIGHT)",
                        "light sampling: the world has more than 16 lights (quads and static spheres whose material is RT_MAT_DIFFUSE_LIGHT)", out_kind, out_index, out_area, out_n);
}

// The light tree of mode RT_LIGHT_SAMPLING_TREE: mode 4's lights (cap RT_MAX_LIGHTS_TREE) permuted into the leaf order of a median-split
// bounding-volume tree over their padded boxes, the running sum of their areas, and the nodes in preorder, 8 floats each: min.xyz, skip, max.xyz, leaf.
static_assert(RT_MAX_LIGHTS_TREE == 4096, "the refusal message below says 4096");
namespace {
struct LightTree { std::vector<uint32_t> kind, index; std::vector<float> area, cdf, nodes; };
struct LightTreeBuilder {
    std::vector<f3> bmin, bmax, cen;   // per light, in mode 4's order
    std::vector<uint32_t> order;       // the permutation under construction: a node's range [a, b) of it
    std::vector<float> nodes;
    static float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
    void build(uint32_t a, uint32_t b, f3& out_min, f3& out_max) {
        const size_t at = nodes.size();
        nodes.resize(at + 8);
        uint32_t leaf = 0xffffffffu;
        if (b - a == 1u) {
            out_min = bmin[order[a]]; out_max = bmax[order[a]];
            leaf = a;   // leaves are met in range order: the light's position in the permuted table
        } else {
            f3 cmin = cen[order[a]], cmax = cmin;
            for (uint32_t i = a + 1u; i < b; i++) { cmin = glm_min(cmin, cen[order[i]]); cmax = glm_max(cmax, cen[order[i]]); }
            const f3 e = cmax - cmin;
            const float ext[3] = {e.x, e.y, e.z};
            int axis = 0;
            if (ext[1] > ext[axis]) axis = 1;
            if (ext[2] > ext[axis]) axis = 2;
            std::stable_sort(order.begin() + a, order.begin() + b, [&](uint32_t p, uint32_t q) {
                const float cp = axis == 0 ? cen[p].x : axis == 1 ? cen[p].y : cen[p].z, cq = axis == 0 ? cen[q].x : axis == 1 ? cen[q].y : cen[q].z;
                return cp < cq;
            });
            const uint32_t mid = a + (b - a) / 2u;
            f3 lmin, lmax, rmin, rmax;
            build(a, mid, lmin, lmax);
            build(mid, b, rmin, rmax);
            out_min = glm_min(lmin, rmin); out_max = glm_max(lmax, rmax);
        }
        float* nd = nodes.data() + at;
        nd[0] = out_min.x; nd[1] = out_min.y; nd[2] = out_min.z; nd[3] = bits((uint32_t)(nodes.size() / 8));
        nd[4] = out_max.x; nd[5] = out_max.y; nd[6] = out_max.z; nd[7] = bits(leaf);
    }
};
}  // namespace
static int world_light_tree(const rt_world_flat* w, const char* who, LightTree& out) {
    if ((w->n_quads && !w->quads) || (w->n_materials && !w->materials) || (w->n_prims && !w->prims)) return rt_fail(RT_ERR_INVALID, "%s: world array is null", who);
    std::vector<uint32_t> kind(RT_MAX_LIGHTS_TREE), index(RT_MAX_LIGHTS_TREE);
    std::vector<float> area(RT_MAX_LIGHTS_TREE);
    uint32_t n = 0;
    if (int rc = world_lights(w, true, "light sampling: the world has no light to sample (a quad, a triangle or a static sphere of radius > 0 whose material is RT_MAT_DIFFUSE_LIGHT)",
                              "light sampling: the world has more than 4096 lights (quads, triangles and static spheres whose material is RT_MAT_DIFFUSE_LIGHT)", kind.data(), index.data(),
                              area.data(), &n, true, RT_MAX_LIGHTS_TREE))
        return rc;
    float M = 0.0f;
    for (int k = 0; k < 3; k++) M = glm_max(M, glm_max(fabsf(w->bounds_min[k]), fabsf(w->bounds_max[k])));
    const float pad = RT_LIGHT_TREE_PAD * M;
    LightTreeBuilder tb;
    tb.bmin.resize(n); tb.bmax.resize(n); tb.cen.resize(n); tb.order.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        f3 lo, hi;
        float p = pad;
        if (kind[i] == RT_LIGHT_SPHERE) {
            const rt_prim& pr = w->prims[index[i]];
            const f3 c = mk3(pr.c0[0], pr.c0[1], pr.c0[2]);
            lo = c - mk3(pr.radius); hi = c + mk3(pr.radius);
            p = pad + (RT_LIGHT_TREE_PAD_SPHERE * (M * M)) / pr.radius;
        } else {
            const rt_quad& q = w->quads[index[i]];
            const f3 Q = mk3(q.Q[0], q.Q[1], q.Q[2]), u = mk3(q.u[0], q.u[1], q.u[2]), v = mk3(q.v[0], q.v[1], q.v[2]);
            const f3 qu = Q + u, qv = Q + v;
            lo = glm_min(glm_min(Q, qu), qv); hi = glm_max(glm_max(Q, qu), qv);
            if (kind[i] == RT_LIGHT_QUAD) { const f3 quv = qu + v; lo = glm_min(lo, quv); hi = glm_max(hi, quv); }
        }
        tb.bmin[i] = lo - mk3(p); tb.bmax[i] = hi + mk3(p);
        tb.cen[i] = (tb.bmin[i] + tb.bmax[i]) * 0.5f;
        tb.order[i] = i;
    }
    tb.nodes.reserve((size_t)(2u * n - 1u) * 8u);
    f3 rmin, rmax;
    tb.build(0u, n, rmin, rmax);
    out.kind.resize(n); out.index.resize(n); out.area.resize(n); out.cdf.resize(n);
    float c = 0.0f;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t o = tb.order[i];
        out.kind[i] = kind[o]; out.index[i] = index[o]; out.area[i] = area[o];
        const float c1 = c + area[o];
        if (c1 == c)
            return rt_fail(RT_ERR_INVALID, "light sampling: the area of a light (kind %u, index %u: %g) is lost in the fp32 running sum of the areas (%g); it could never be drawn", kind[o], index[o],
                           (double)area[o], (double)c);
        out.cdf[i] = c = c1;
    }
    out.nodes.swap(tb.nodes);
    return RT_OK;
}

extern "C" int rt_world_light_tree(const rt_world_flat* w, uint32_t capacity, float* out_nodes, uint32_t* out_n_nodes, float* out_cdf) {
    if (!w || !out_nodes || !out_n_nodes || !out_cdf) return rt_fail(RT_ERR_INVALID, "rt_world_light_tree: null argument");
    *out_n_nodes = 0;
    LightTree t;
    if (int rc = world_light_tree(w, "rt_world_light_tree", t)) return rc;
    const uint32_t n = (uint32_t)t.kind.size();
    if (n > capacity) return rt_fail(RT_ERR_INVALID, "rt_world_light_tree: the table has %u lights, the caller's arrays hold %u", n, capacity);
    std::memcpy(out_nodes, t.nodes.data(), t.nodes.size() * sizeof(float));
    std::memcpy(out_cdf, t.cdf.data(), n * sizeof(float));
    *out_n_nodes = 2u * n - 1u;
    return RT_OK;
}

// The light table of any mode, into the caller's arrays of `capacity` entries.  Modes 1 and 2: rt_world_lights' own answer, through arrays of its size.  Mode
// RT_LIGHT_SAMPLING_MESH: mode 2's list, then the triangle lights.
static_assert(RT_MAX_LIGHTS_MESH == 64, "the refusal message below says 64");
extern "C" int rt_world_light_table(const rt_world_flat* w, uint32_t mode, uint32_t capacity, uint32_t* out_kind, uint32_t* out_index, float* out_area, uint32_t* out_n) {
    if (!w || !out_kind || !out_index || !out_area || !out_n) return rt_fail(RT_ERR_INVALID, "rt_world_light_table: null argument");
    *out_n = 0;
    if (mode != RT_LIGHT_SAMPLING_QUADS && mode != RT_LIGHT_SAMPLING_ALL && mode != RT_LIGHT_SAMPLING_MESH && mode != RT_LIGHT_SAMPLING_TREE)
        return rt_fail(RT_ERR_INVALID, "rt_world_light_table: mode must be RT_LIGHT_SAMPLING_QUADS (1), RT_LIGHT_SAMPLING_ALL (2), RT_LIGHT_SAMPLING_MESH (4) or RT_LIGHT_SAMPLING_TREE (16)");
    if (mode == RT_LIGHT_SAMPLING_TREE) {   // §20: mode 4's lights in the tree's leaf order
        LightTree t;
        if (int rc = world_light_tree(w, "rt_world_light_table", t)) return rc;
        const uint32_t n_t = (uint32_t)t.kind.size();
        if (n_t > capacity) return rt_fail(RT_ERR_INVALID, "rt_world_light_table: the table has %u lights, the caller's arrays hold %u", n_t, capacity);
        for (uint32_t i = 0; i < n_t; i++) { out_kind[i] = t.kind[i]; out_index[i] = t.index[i]; out_area[i] = t.area[i]; }
        *out_n = n_t;
        return RT_OK;
    }
    uint32_t kind[RT_MAX_LIGHTS_MESH], index[RT_MAX_LIGHTS_MESH], n = 0;
    float area[RT_MAX_LIGHTS_MESH];
    if (mode != RT_LIGHT_SAMPLING_MESH) {
        if (int rc = rt_world_lights(w, mode, kind, index, area, &n)) return rc;
    } else {
        if ((w->n_quads && !w->quads) || (w->n_materials && !w->materials) || (w->n_prims && !w->prims)) return rt_fail(RT_ERR_INVALID, "rt_world_light_table: world array is null");
        if (int rc = world_lights(w, true, "light sampling: the world has no light to sample (a quad, a triangle or a static sphere of radius > 0 whose material is RT_MAT_DIFFUSE_LIGHT)",
                                  "light sampling: the world has more than 64 lights (quads, triangles and static spheres whose material is RT_MAT_DIFFUSE_LIGHT)", kind, index, area, &n,
                                  true, RT_MAX_LIGHTS_MESH))
            return rc;
    }
    if (n > capacity) return rt_fail(RT_ERR_INVALID, "rt_world_light_table: the table has %u lights, the caller's arrays hold %u", n, capacity);
    for (uint32_t i = 0; i < n; i++) { out_kind[i] = kind[i]; out_index[i] = index[i]; out_area[i] = area[i]; }
    *out_n = n;
    return RT_OK;
}

extern "C" int rt_scene_set_perlin(rt_scene* s, uint64_t seed) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_perlin: null scene");
    Rng g;
    g.init(seed, 0u, 0u, 0x9E81u);
    s->perlin.assign(1, rt_perlin());
    rt_perlin& t = s->perlin[0];
    for (int i = 0; i < 256; i++) {
        f3 v;
        v.x = g.next() * 2.0f - 1.0f;
        v.y = g.next() * 2.0f - 1.0f;
        v.z = g.next() * 2.0f - 1.0f;
        if (near_zero(v)) v = mk3(1.0f, 0.0f, 0.0f);
        st3(t.randvec[i], normalize(v));
    }
    for (int k = 0; k < 3; k++) {
        for (int i = 0; i < 256; i++) t.perm[k][i] = i;
        for (int i = 255; i > 0; i--) {
            int target = (int)(g.next() * (float)(i + 1));   // random_int(0, i); the uniform is in (0, 1]
            if (target > i) target = i;
            int32_t tmp = t.perm[k][i]; t.perm[k][i] = t.perm[k][target]; t.perm[k][target] = tmp;
        }
    }
    return RT_OK;
}

extern "C" int rt_scene_set_image(rt_scene* s, uint32_t width, uint32_t height, const uint8_t* rgb) {
    if (!s || !rgb) return rt_fail(RT_ERR_INVALID, "rt_scene_set_image: null argument");
    if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 26)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_image: bad size %u x %u", width, height);
    uint64_t total = (uint64_t)width * height;   // §25: the scene's table, this image as its entry 0, stays one a renderer takes
    for (const rt_scene::Image& im : s->more_images) total += (uint64_t)im.w * im.h;
    if (total > (uint64_t)RT_MAX_TABLE_TEXELS) return rt_fail(RT_ERR_INVALID, "rt_scene_set_image: with the images added, more than RT_MAX_TABLE_TEXELS (2^28) texels in all");
    s->image.assign(rgb, rgb + (size_t)width * height * 3);
    s->image_w = width;
    s->image_h = height;
    return RT_OK;
}

// ---- the texture table ----
bool rt_image_index_ok(float param) { return param >= 0.0f && param < (float)RT_MAX_IMAGES && param == (float)(uint32_t)param; }
static const char* sampling_refusal(uint32_t wrap, uint32_t filter) {
    if (wrap > RT_WRAP_REPEAT) return "unknown wrap mode (RT_WRAP_CLAMP or RT_WRAP_REPEAT)";
    if (filter > RT_FILTER_BILINEAR) return "unknown filter (RT_FILTER_NEAREST or RT_FILTER_BILINEAR)";
    return nullptr;
}
const char* rt_texture_table_refusal(const rt_texture* records, uint32_t n, const uint8_t* texels, uint64_t* out_texels) {
    if (!records || n == 0u) return "a table and its count go together";
    if (n > RT_MAX_IMAGES) return "more than RT_MAX_IMAGES (256) entries";
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const rt_texture& t = records[i];
        if ((t.width == 0u) != (t.height == 0u)) return "an entry with one dimension zero (an empty entry is 0 x 0)";
        if ((uint64_t)t.width * t.height > (1ull << 26)) return "an entry of more than 2^26 texels";
        if (const char* why = sampling_refusal(t.wrap, t.filter)) return why;
        if ((uint64_t)t.first != at) return "the entries' texels do not sit back to back (first = the sum of the sizes before)";
        at += (uint64_t)t.width * t.height;
        if (at > (uint64_t)RT_MAX_TABLE_TEXELS) return "more than RT_MAX_TABLE_TEXELS (2^28) texels in all";
    }
    if (at != 0u && !texels) return "null texels";
    if (out_texels) *out_texels = at;
    return nullptr;
}
extern "C" int rt_scene_add_image(rt_scene* s, uint32_t width, uint32_t height, const uint8_t* rgb, uint32_t wrap, uint32_t filter, uint32_t* out_index) {
    if (!s || !rgb) return rt_fail(RT_ERR_INVALID, "rt_scene_add_image: null argument");
    if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 26)) return rt_fail(RT_ERR_INVALID, "rt_scene_add_image: bad size %u x %u", width, height);
    if (const char* why = sampling_refusal(wrap, filter)) return rt_fail(RT_ERR_INVALID, "rt_scene_add_image: %s", why);
    if (1u + s->more_images.size() >= RT_MAX_IMAGES) return rt_fail(RT_ERR_INVALID, "rt_scene_add_image: a scene holds at most RT_MAX_IMAGES (%u) images, entry 0 included", RT_MAX_IMAGES);
    uint64_t total = (uint64_t)s->image_w * s->image_h + (uint64_t)width * height;
    for (const rt_scene::Image& im : s->more_images) total += (uint64_t)im.w * im.h;
    if (total > (uint64_t)RT_MAX_TABLE_TEXELS) return rt_fail(RT_ERR_INVALID, "rt_scene_add_image: more than RT_MAX_TABLE_TEXELS (2^28) texels in all");
    rt_scene::Image im;
    im.w = width; im.h = height;
    im.rgb.assign(rgb, rgb + (size_t)width * height * 3);
    s->more_images.push_back(std::move(im));
    s->image_wrap.push_back(wrap); s->image_filter.push_back(filter);
    if (out_index) *out_index = (uint32_t)s->more_images.size();
    return RT_OK;
}
extern "C" int rt_scene_image_sampling(rt_scene* s, uint32_t index, uint32_t wrap, uint32_t filter) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_image_sampling: null scene");
    if (index > s->more_images.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_image_sampling: the scene has no image %u", index);
    if (const char* why = sampling_refusal(wrap, filter)) return rt_fail(RT_ERR_INVALID, "rt_scene_image_sampling: %s", why);
    s->image_wrap[index] = wrap; s->image_filter[index] = filter;
    return RT_OK;
}
extern "C" int rt_scene_textures(const rt_scene* s, const rt_texture** out_records, uint32_t* out_n, const uint8_t** out_texels) {
    if (!s || !out_records || !out_n || !out_texels) return rt_fail(RT_ERR_INVALID, "rt_scene_textures: null argument");
    s->table.clear(); s->table_texels.clear();
    *out_records = nullptr; *out_n = 0u; *out_texels = nullptr;
    if (s->image.empty() && s->more_images.empty() && s->image_wrap[0] == RT_WRAP_CLAMP && s->image_filter[0] == RT_FILTER_NEAREST) return RT_OK;
    uint32_t at = 0u;
    auto entry = [&](uint32_t w, uint32_t h, const std::vector<uint8_t>& rgb) {
        const size_t k = s->table.size();
        s->table.push_back(rt_texture{w, h, s->image_wrap[k], s->image_filter[k], at});
        s->table_texels.insert(s->table_texels.end(), rgb.begin(), rgb.end());
        at += w * h;
    };
    entry(s->image_w, s->image_h, s->image);
    for (const rt_scene::Image& im : s->more_images) entry(im.w, im.h, im.rgb);
    *out_records = s->table.data(); *out_n = (uint32_t)s->table.size();
    *out_texels = s->table_texels.empty() ? nullptr : s->table_texels.data();
    return RT_OK;
}

// ---- normal maps ----
extern "C" int rt_scene_set_normal_map(rt_scene* s, uint32_t material, uint32_t image, float strength) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_normal_map: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_set_normal_map: the scene has no material %u", material);
    const uint32_t type = s->mats[material].type;
    if (type == RT_MAT_DIELECTRIC || type == RT_MAT_DIFFUSE_LIGHT || type == RT_MAT_ISOTROPIC)
        return rt_fail(RT_ERR_INVALID, "rt_scene_set_normal_map: material %u is a dielectric, a light or a medium; Lambertian (plain, checker, noise, image) and metal materials take a normal map", material);
    if (image >= RT_MAX_IMAGES) return rt_fail(RT_ERR_INVALID, "rt_scene_set_normal_map: an image index lies in [0, %u), not %u", RT_MAX_IMAGES, image);
    if (!(std::isfinite(strength) && strength >= 0.0f)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_normal_map: a strength must be finite and >= 0");
    if (s->nmaps.size() <= material) s->nmaps.resize((size_t)material + 1u, rt_normal_map{0u, 0u, 0.0f, 0u});
    s->nmaps[material] = rt_normal_map{1u, image, strength, 0u};
    return RT_OK;
}
extern "C" int rt_scene_clear_normal_map(rt_scene* s, uint32_t material) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_clear_normal_map: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_clear_normal_map: the scene has no material %u", material);
    if (material < s->nmaps.size()) s->nmaps[material] = rt_normal_map{0u, 0u, 0.0f, 0u};
    return RT_OK;
}
extern "C" int rt_scene_normal_maps(const rt_scene* s, const rt_normal_map** out, uint32_t* out_n) {
    if (!s || !out || !out_n) return rt_fail(RT_ERR_INVALID, "rt_scene_normal_maps: null argument");
    *out = nullptr; *out_n = 0u;
    s->nmap_table.clear();
    bool any = false;
    for (const rt_normal_map& m : s->nmaps) any = any || m.on != 0u;
    if (!any) return RT_OK;
    s->nmap_table = s->nmaps;
    s->nmap_table.resize(s->mats.size(), rt_normal_map{0u, 0u, 0.0f, 0u});
    *out = s->nmap_table.data(); *out_n = (uint32_t)s->nmap_table.size();
    return RT_OK;
}

// ---- microfacet surfaces ----
extern "C" int rt_scene_set_microfacet(rt_scene* s, uint32_t material, float roughness, float specular) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_microfacet: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_set_microfacet: the scene has no material %u", material);
    const uint32_t type = s->mats[material].type;
    if (type == RT_MAT_DIELECTRIC || type == RT_MAT_DIFFUSE_LIGHT || type == RT_MAT_ISOTROPIC)
        return rt_fail(RT_ERR_INVALID, "rt_scene_set_microfacet: material %u is a dielectric, a light or a medium; a metal becomes a rough conductor, and Lambertian (plain, checker, noise, image) materials take a coat", material);
    if (!(std::isfinite(roughness) && roughness >= 0.0f && roughness <= 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_microfacet: a roughness must be finite and in [0, 1]");
    if (!(std::isfinite(specular) && specular >= 0.0f && specular <= 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_microfacet: a specular must be finite and in [0, 1]");
    if (s->mfacs.size() <= material) s->mfacs.resize((size_t)material + 1u, rt_microfacet{RT_MICROFACET_OFF, 0u, 0.0f, 0.0f});
    rt_microfacet& m = s->mfacs[material];
    if (m.on != RT_MICROFACET_MAPPED) m = rt_microfacet{RT_MICROFACET_CONSTANT, 0u, 0.0f, 0.0f};
    m.roughness = roughness; m.specular = specular;
    return RT_OK;
}
extern "C" int rt_scene_set_roughness_map(rt_scene* s, uint32_t material, uint32_t image) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_roughness_map: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_set_roughness_map: the scene has no material %u", material);
    if (material >= s->mfacs.size() || s->mfacs[material].on == RT_MICROFACET_OFF)
        return rt_fail(RT_ERR_INVALID, "rt_scene_set_roughness_map: material %u has no microfacet record; give it one with rt_scene_set_microfacet first", material);
    if (image >= RT_MAX_IMAGES) return rt_fail(RT_ERR_INVALID, "rt_scene_set_roughness_map: an image index lies in [0, %u), not %u", RT_MAX_IMAGES, image);
    const uint32_t on = s->mfacs[material].on;   // §30: a glass record stays a glass record
    s->mfacs[material].on = (on == RT_MICROFACET_GLASS || on == RT_MICROFACET_GLASS_MAPPED) ? RT_MICROFACET_GLASS_MAPPED : RT_MICROFACET_MAPPED;
    s->mfacs[material].image = image;
    return RT_OK;
}
// rough glass: a record kind of its own, on dielectrics alone
extern "C" int rt_scene_set_rough_glass(rt_scene* s, uint32_t material, float roughness) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_rough_glass: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_set_rough_glass: the scene has no material %u", material);
    if (s->mats[material].type != RT_MAT_DIELECTRIC)
        return rt_fail(RT_ERR_INVALID, "rt_scene_set_rough_glass: material %u is no dielectric; metals and Lambertian materials take their record from rt_scene_set_microfacet", material);
    if (!(std::isfinite(roughness) && roughness >= 0.0f && roughness <= 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_rough_glass: a roughness must be finite and in [0, 1]");
    if (s->mfacs.size() <= material) s->mfacs.resize((size_t)material + 1u, rt_microfacet{RT_MICROFACET_OFF, 0u, 0.0f, 0.0f});
    rt_microfacet& m = s->mfacs[material];
    if (m.on != RT_MICROFACET_GLASS_MAPPED) m = rt_microfacet{RT_MICROFACET_GLASS, 0u, 0.0f, 0.0f};
    m.roughness = roughness; m.specular = 0.0f;
    return RT_OK;
}
extern "C" int rt_scene_clear_microfacet(rt_scene* s, uint32_t material) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_clear_microfacet: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_clear_microfacet: the scene has no material %u", material);
    if (material < s->mfacs.size()) s->mfacs[material] = rt_microfacet{RT_MICROFACET_OFF, 0u, 0.0f, 0.0f};
    return RT_OK;
}
extern "C" int rt_scene_microfacets(const rt_scene* s, const rt_microfacet** out, uint32_t* out_n) {
    if (!s || !out || !out_n) return rt_fail(RT_ERR_INVALID, "rt_scene_microfacets: null argument");
    *out = nullptr; *out_n = 0u;
    s->mfac_table.clear();
    bool any = false;
    for (const rt_microfacet& m : s->mfacs) any = any || m.on != RT_MICROFACET_OFF;
    if (!any) return RT_OK;
    s->mfac_table = s->mfacs;
    s->mfac_table.resize(s->mats.size(), rt_microfacet{RT_MICROFACET_OFF, 0u, 0.0f, 0.0f});
    *out = s->mfac_table.data(); *out_n = (uint32_t)s->mfac_table.size();
    return RT_OK;
}

// ---- solid glass ----
extern "C" int rt_scene_set_interior(rt_scene* s, uint32_t material, const float sigma[3]) {
    if (!s || !sigma) return rt_fail(RT_ERR_INVALID, "rt_scene_set_interior: null argument");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_set_interior: the scene has no material %u", material);
    if (s->mats[material].type != RT_MAT_DIELECTRIC) return rt_fail(RT_ERR_INVALID, "rt_scene_set_interior: material %u is no dielectric; only glass has an inside to absorb in", material);
    for (int c = 0; c < 3; c++)
        if (!(std::isfinite(sigma[c]) && sigma[c] >= 0.0f)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_interior: an absorption coefficient must be finite and >= 0");
    if (material < s->cutouts.size() && s->cutouts[material].on != RT_CUTOUT_OFF)   // §34
        return rt_fail(RT_ERR_INVALID, "rt_scene_set_interior: material %u has a cutout record, and a holed solid has no inside (rt_scene_clear_cutout first)", material);
    if (s->interiors.size() <= material) s->interiors.resize((size_t)material + 1u, rt_interior{RT_INTERIOR_OFF, {0.0f, 0.0f, 0.0f}});
    s->interiors[material] = rt_interior{RT_INTERIOR_SOLID, {sigma[0] + 0.0f, sigma[1] + 0.0f, sigma[2] + 0.0f}};   // (-0 is stored as 0)
    return RT_OK;
}
extern "C" int rt_scene_clear_interior(rt_scene* s, uint32_t material) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_clear_interior: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_clear_interior: the scene has no material %u", material);
    if (material < s->interiors.size()) s->interiors[material] = rt_interior{RT_INTERIOR_OFF, {0.0f, 0.0f, 0.0f}};
    return RT_OK;
}
extern "C" int rt_scene_interiors(const rt_scene* s, const rt_interior** out, uint32_t* out_n) {
    if (!s || !out || !out_n) return rt_fail(RT_ERR_INVALID, "rt_scene_interiors: null argument");
    *out = nullptr; *out_n = 0u;
    s->interior_table.clear();
    bool any = false;
    for (const rt_interior& m : s->interiors) any = any || m.on != RT_INTERIOR_OFF;
    if (!any) return RT_OK;
    s->interior_table = s->interiors;
    s->interior_table.resize(s->mats.size(), rt_interior{RT_INTERIOR_OFF, {0.0f, 0.0f, 0.0f}});
    *out = s->interior_table.data(); *out_n = (uint32_t)s->interior_table.size();
    return RT_OK;
}

// ---- alpha cutouts ----
extern "C" int rt_scene_set_cutout(rt_scene* s, uint32_t material, uint32_t image, float cutoff) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_set_cutout: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_set_cutout: the scene has no material %u", material);
    if (s->mats[material].type == RT_MAT_DIFFUSE_LIGHT)
        return rt_fail(RT_ERR_INVALID, "rt_scene_set_cutout: material %u is a light, and the light tables take a light's whole area as emitting", material);
    if (s->mats[material].type == RT_MAT_ISOTROPIC) return rt_fail(RT_ERR_INVALID, "rt_scene_set_cutout: material %u is a medium, which has no surface to cut", material);
    if (material < s->interiors.size() && s->interiors[material].on != RT_INTERIOR_OFF)
        return rt_fail(RT_ERR_INVALID, "rt_scene_set_cutout: material %u has an interior record, and a holed solid has no inside (rt_scene_clear_interior first)", material);
    if (image >= RT_MAX_IMAGES) return rt_fail(RT_ERR_INVALID, "rt_scene_set_cutout: an image index lies in [0, %u)", RT_MAX_IMAGES);
    if (!(std::isfinite(cutoff) && cutoff >= 0.0f && cutoff <= 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_scene_set_cutout: a cutoff must be finite and in [0, 1]");
    if (s->cutouts.size() <= material) s->cutouts.resize((size_t)material + 1u, rt_cutout{RT_CUTOUT_OFF, 0u, 0.0f, 0u});
    s->cutouts[material] = rt_cutout{RT_CUTOUT_MASKED, image, cutoff + 0.0f, 0u};   // (-0 is stored as 0)
    return RT_OK;
}
extern "C" int rt_scene_clear_cutout(rt_scene* s, uint32_t material) {
    if (!s) return rt_fail(RT_ERR_INVALID, "rt_scene_clear_cutout: null scene");
    if (material >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_clear_cutout: the scene has no material %u", material);
    if (material < s->cutouts.size()) s->cutouts[material] = rt_cutout{RT_CUTOUT_OFF, 0u, 0.0f, 0u};
    return RT_OK;
}
extern "C" int rt_scene_cutouts(const rt_scene* s, const rt_cutout** out, uint32_t* out_n) {
    if (!s || !out || !out_n) return rt_fail(RT_ERR_INVALID, "rt_scene_cutouts: null argument");
    *out = nullptr; *out_n = 0u;
    s->cutout_table.clear();
    bool any = false;
    for (const rt_cutout& m : s->cutouts) any = any || m.on != RT_CUTOUT_OFF;
    if (!any) return RT_OK;
    s->cutout_table = s->cutouts;
    s->cutout_table.resize(s->mats.size(), rt_cutout{RT_CUTOUT_OFF, 0u, 0.0f, 0u});
    *out = s->cutout_table.data(); *out_n = (uint32_t)s->cutout_table.size();
    return RT_OK;
}

extern "C" int rt_host_uniforms(uint64_t seed, uint32_t first, uint32_t n, float* out) {
    if (!out && n) return rt_fail(RT_ERR_INVALID, "rt_host_uniforms: null out");
    Rng g;
    g.init(seed, 0u, 0u, RT_STREAM_SCENE);
    for (uint32_t i = 0; i < first; i++) (void)g.next();  // a sequential stream: skip to `first`
    for (uint32_t i = 0; i < n; i++) out[i] = g.next();
    return RT_OK;
}

// ---- prefab scenes ---------------------------------------------------------------------------
static void add(rt_scene* s, f3 c0, f3 c1, float r, bool moving, uint32_t type, f3 albedo, float param) {
    float a[3], p0[3], p1[3];
    st3(a, albedo); st3(p0, c0); st3(p1, c1);
    int32_t mat = 0;
    rt_scene_add_material(s, type, a, param, nullptr, &mat);
    add_prim(s, p0, p1, r, mat, moving, nullptr);
}

// SceneBook2BVH::Factory::_populate_world (Scenes.cu:219-270) when moving; the disabled SceneBook1
// variant (Scenes.cu:57-115) with static Lambertians otherwise (its centre1 draw is still consumed so
// both scenes share one layout, as google_testing/test.cpp:41-51 does).  Uniforms: the build's host
// stream (RT_STREAM_SCENE) in place of cuHostRND(512, 1984).
static rt_scene* book_scene(uint64_t seed, bool moving) {
    rt_scene* s = new rt_scene();
    Rng g;
    g.init(seed, 0u, 0u, RT_STREAM_SCENE);
    add(s, mk3(0, -1000, 0), mk3(0, -1000, 0), 1000.0f, false, RT_MAT_LAMBERTIAN, mk3(0.5f), 0.0f);
    for (int a = -11; a < 11; a++)
        for (int b = -11; b < 11; b++) {
            float choose_mat = g.next();
            float cx = (float)a + g.next();
            float cz = (float)b + g.next();
            f3 center = mk3(cx, 0.2f, cz);
            if (choose_mat < 0.8f) {
                float r0 = g.next(), r1 = g.next(), r2 = g.next(), r3 = g.next(), r4 = g.next(), r5 = g.next();
                f3 albedo = mk3(r0 * r1, r2 * r3, r4 * r5);
                float rc = g.next();
                f3 center1 = center + mk3(0, rc * 0.5f, 0);
                add(s, center, moving ? center1 : center, 0.2f, moving, RT_MAT_LAMBERTIAN, albedo, 0.0f);
            } else if (choose_mat < 0.95f) {
                float r0 = g.next(), r1 = g.next(), r2 = g.next(), r3 = g.next();
                f3 albedo = mk3(0.5f * (1.0f + r0), 0.5f * (1.0f + r1), 0.5f * (1.0f + r2));
                add(s, center, center, 0.2f, false, RT_MAT_METAL, albedo, 0.5f * r3);
            } else {
                add(s, center, center, 0.2f, false, RT_MAT_DIELECTRIC, mk3(1.0f), 1.5f);
            }
        }
    add(s, mk3(0, 1, 0), mk3(0, 1, 0), 1.0f, false, RT_MAT_DIELECTRIC, mk3(1.0f), 1.5f);
    add(s, mk3(-4, 1, 0), mk3(-4, 1, 0), 1.0f, false, RT_MAT_LAMBERTIAN, mk3(0.4f, 0.2f, 0.1f), 0.0f);
    add(s, mk3(4, 1, 0), mk3(4, 1, 0), 1.0f, false, RT_MAT_METAL, mk3(0.7f, 0.6f, 0.5f), 0.0f);
    return s;
}
extern "C" int rt_scene_book1_final(uint64_t seed, rt_scene** out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_scene_book1_final: null out");
    rt_scene* s = book_scene(seed, false);
    int rc = rt_scene_build_bvh_topdown(s);  // Scenes.cu:297-299
    if (rc != RT_OK) { delete s; return rc; }
    *out = s;
    return RT_OK;
}
extern "C" int rt_scene_book2_moving(uint64_t seed, rt_scene** out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_scene_book2_moving: null out");
    rt_scene* s = book_scene(seed, true);
    int rc = rt_scene_build_bvh_topdown(s);
    if (rc != RT_OK) { delete s; return rc; }
    *out = s;
    return RT_OK;
}
// Book-1 three-spheres scene (BASELINE.json config 1; layout from SURVEY.md §8d) as a HittableList.
extern "C" int rt_scene_three_spheres(rt_scene** out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_scene_three_spheres: null out");
    rt_scene* s = new rt_scene();
    add(s, mk3(0, -100.5f, -1), mk3(0, -100.5f, -1), 100.0f, false, RT_MAT_LAMBERTIAN, mk3(0.8f, 0.8f, 0.0f), 0.0f);
    add(s, mk3(0, 0, -1.2f), mk3(0, 0, -1.2f), 0.5f, false, RT_MAT_LAMBERTIAN, mk3(0.1f, 0.2f, 0.5f), 0.0f);
    add(s, mk3(-1, 0, -1), mk3(-1, 0, -1), 0.5f, false, RT_MAT_DIELECTRIC, mk3(1.0f), 1.5f);
    add(s, mk3(-1, 0, -1), mk3(-1, 0, -1), 0.4f, false, RT_MAT_DIELECTRIC, mk3(1.0f), 1.0f / 1.5f);
    add(s, mk3(1, 0, -1), mk3(1, 0, -1), 0.5f, false, RT_MAT_METAL, mk3(0.8f, 0.6f, 0.2f), 1.0f);
    int rc = rt_scene_set_world_list(s);
    if (rc != RT_OK) { delete s; return rc; }
    *out = s;
    return RT_OK;
}

// ---- Cornell box of "Ray Tracing: The Next Week" (BASELINE.json configs[3]) ------------------------------
static void cornell_quad(rt_scene* s, f3 Q, f3 u, f3 v, int32_t mat) {
    float a[3], b[3], c[3];
    st3(a, Q); st3(b, u); st3(c, v);
    rt_scene_add_quad(s, a, b, c, mat, nullptr);
}
static f3 rot_y(f3 p, float c, float sn) { return mk3(c * p.x + sn * p.z, p.y, -sn * p.x + c * p.z); }
// box(a,b) of the book as 6 quads, rotated about y and translated on the host (the book uses rotate_y / translate instances)
static void cornell_box(rt_scene* s, f3 a, f3 b, float degrees, f3 offset, int32_t mat) {
    f3 mn = glm_min(a, b), mx = glm_max(a, b);
    f3 dx = mk3(mx.x - mn.x, 0, 0), dy = mk3(0, mx.y - mn.y, 0), dz = mk3(0, 0, mx.z - mn.z);
    float rad = radians(degrees), c = cosf(rad), sn = sinf(rad);
    f3 Qs[6] = {mk3(mn.x, mn.y, mx.z), mk3(mx.x, mn.y, mx.z), mk3(mx.x, mn.y, mn.z), mk3(mn.x, mn.y, mn.z), mk3(mn.x, mx.y, mx.z), mk3(mn.x, mn.y, mn.z)};
    f3 us[6] = {dx, -dz, -dx, dz, dx, dx};
    f3 vs[6] = {dy, dy, dy, dy, -dz, dz};
    for (int k = 0; k < 6; k++) cornell_quad(s, rot_y(Qs[k], c, sn) + offset, rot_y(us[k], c, sn), rot_y(vs[k], c, sn), mat);
}
extern "C" int rt_scene_add_box(rt_scene* s, const float a[3], const float b[3], int32_t mat, float rotate_y_degrees,
                                const float translate[3], int32_t* out_first_quad) {
    if (!s || !a || !b) return rt_fail(RT_ERR_INVALID, "rt_scene_add_box: null argument");
    if (mat < 0 || (size_t)mat >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "rt_scene_add_box: material %d out of range", mat);
    if (out_first_quad) *out_first_quad = (int32_t)(s->quads.size() - s->n_tris);
    cornell_box(s, ld3(a), ld3(b), rotate_y_degrees, translate ? ld3(translate) : mk3(0.0f), mat);
    return RT_OK;
}

// An indexed mesh as triangles: every vertex p -> rot_y(p * scale) + translate (cornell_box's order and arithmetic), then tri_record per face.
// normals (rt_scene_add_mesh_smooth; null for the flat mesh): rot_y of each, then unit_normal; a face takes normal_indices' three, or its vertex indices.
// uvs (rt_scene_add_mesh_uv; null otherwise): as given, finite; a face takes uv_indices' three, or its vertex indices; without them every face gets the identity.
static int add_mesh(const char* who, rt_scene* s, uint32_t n_vertices, const float* xyz, uint32_t n_normals, const float* normals, uint32_t n_uvs, const float* uvs,
                    uint32_t n_triangles, const uint32_t* indices, const uint32_t* normal_indices, const uint32_t* uv_indices, int32_t mat, float scale, float rotate_y_degrees, const float translate[3], int32_t* out_first, uint32_t* out_added) {
    if (!s || (n_vertices && !xyz) || (n_triangles && !indices)) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    if (mat < 0 || (size_t)mat >= s->mats.size()) return rt_fail(RT_ERR_INVALID, "%s: material %d out of range", who, mat);
    if (!std::isfinite(scale) || !std::isfinite(rotate_y_degrees)) return rt_fail(RT_ERR_INVALID, "%s: scale and rotation must be finite", who);
    for (size_t i = 0; i < (size_t)n_triangles * 3u; i++)
        if (indices[i] >= n_vertices)
            return rt_fail(RT_ERR_INVALID, "%s: face %zu: vertex index %u out of range (%u vertices)", who, i / 3u, indices[i], n_vertices);
    const uint32_t* nidx = normal_indices ? normal_indices : indices;
    if (normals)
        for (size_t i = 0; i < (size_t)n_triangles * 3u; i++)
            if (nidx[i] >= n_normals)
                return rt_fail(RT_ERR_INVALID, "%s: face %zu: normal index %u out of range (%u normals)", who, i / 3u, nidx[i], n_normals);
    const uint32_t* tidx = uv_indices ? uv_indices : indices;
    if (uvs) {
        for (size_t i = 0; i < (size_t)n_triangles * 3u; i++)
            if (tidx[i] >= n_uvs)
                return rt_fail(RT_ERR_INVALID, "%s: face %zu: texture coordinate index %u out of range (%u texture coordinates)", who, i / 3u, tidx[i], n_uvs);
        for (size_t i = 0; i < (size_t)n_uvs * 2u; i++)
            if (!std::isfinite(uvs[i])) return rt_fail(RT_ERR_INVALID, "%s: texture coordinate %zu is not finite", who, i / 2u);
    }
    const float rad = radians(rotate_y_degrees), c = cosf(rad), sn = sinf(rad);
    const f3 offset = translate ? ld3(translate) : mk3(0.0f);
    std::vector<f3> pts(n_vertices);
    for (uint32_t i = 0; i < n_vertices; i++) pts[i] = rot_y(ld3(xyz + 3 * (size_t)i) * scale, c, sn) + offset;
    std::vector<float> unit((size_t)(normals ? n_normals : 0u) * 3u);
    for (uint32_t i = 0; normals && i < n_normals; i++)
        if (!unit_normal(rot_y(ld3(normals + 3 * (size_t)i), c, sn), &unit[3 * (size_t)i]))
            return rt_fail(RT_ERR_INVALID, "%s: normal %u is not finite or has zero length", who, i);
    std::vector<rt_quad> tris;
    std::vector<rt_tri_normals> vns;
    std::vector<rt_tri_uvs> tuv;
    tris.reserve(n_triangles);
    for (uint32_t f = 0; f < n_triangles; f++) {
        rt_quad q;
        if (!tri_record(pts[indices[3 * (size_t)f]], pts[indices[3 * (size_t)f + 1]], pts[indices[3 * (size_t)f + 2]], (uint32_t)mat, q)) continue;
        tris.push_back(q);
        rt_tri_normals vn{};
        if (normals) {
            std::memcpy(vn.n0, &unit[3 * (size_t)nidx[3 * (size_t)f]], 12); std::memcpy(vn.n1, &unit[3 * (size_t)nidx[3 * (size_t)f + 1]], 12);
            std::memcpy(vn.n2, &unit[3 * (size_t)nidx[3 * (size_t)f + 2]], 12);
        }
        vns.push_back(vn);
        rt_tri_uvs uv = RT_TRI_UVS_IDENTITY;
        if (uvs) {
            std::memcpy(uv.t0, &uvs[2 * (size_t)tidx[3 * (size_t)f]], 8); std::memcpy(uv.t1, &uvs[2 * (size_t)tidx[3 * (size_t)f + 1]], 8);
            std::memcpy(uv.t2, &uvs[2 * (size_t)tidx[3 * (size_t)f + 2]], 8);
        }
        tuv.push_back(uv);
    }
    if (out_first) *out_first = (int32_t)s->quads.size();
    if (out_added) *out_added = (uint32_t)tris.size();
    s->quads.insert(s->quads.end(), tris.begin(), tris.end());
    s->tri_vn.insert(s->tri_vn.end(), vns.begin(), vns.end());
    s->tri_uv.insert(s->tri_uv.end(), tuv.begin(), tuv.end());
    s->n_tris += (uint32_t)tris.size();
    if (normals) s->n_smooth += (uint32_t)tris.size();
    if (!tris.empty()) s->world_set = false;
    return RT_OK;
}
extern "C" int rt_scene_add_mesh(rt_scene* s, uint32_t n_vertices, const float* xyz, uint32_t n_triangles, const uint32_t* indices, int32_t mat, float scale,
                                 float rotate_y_degrees, const float translate[3], int32_t* out_first, uint32_t* out_added) {
    return add_mesh("rt_scene_add_mesh", s, n_vertices, xyz, 0u, nullptr, 0u, nullptr, n_triangles, indices, nullptr, nullptr, mat, scale, rotate_y_degrees, translate, out_first, out_added);
}
extern "C" int rt_scene_add_mesh_smooth(rt_scene* s, uint32_t n_vertices, const float* xyz, uint32_t n_normals, const float* normals, uint32_t n_triangles,
                                        const uint32_t* indices, const uint32_t* normal_indices, int32_t mat, float scale, float rotate_y_degrees, const float translate[3],
                                        int32_t* out_first, uint32_t* out_added) {
    if (!normals) return rt_fail(RT_ERR_INVALID, "rt_scene_add_mesh_smooth: null normals (rt_scene_add_mesh adds a flat mesh)");
    return add_mesh("rt_scene_add_mesh_smooth", s, n_vertices, xyz, n_normals, normals, 0u, nullptr, n_triangles, indices, normal_indices, nullptr, mat, scale, rotate_y_degrees, translate, out_first, out_added);
}
extern "C" int rt_scene_add_mesh_uv(rt_scene* s, uint32_t n_vertices, const float* xyz, uint32_t n_normals, const float* normals, uint32_t n_uvs, const float* uvs,
                                    uint32_t n_triangles, const uint32_t* indices, const uint32_t* normal_indices, const uint32_t* uv_indices, int32_t mat, float scale,
                                    float rotate_y_degrees, const float translate[3], int32_t* out_first, uint32_t* out_added) {
    if (!uvs) return rt_fail(RT_ERR_INVALID, "rt_scene_add_mesh_uv: null texture coordinates (rt_scene_add_mesh and rt_scene_add_mesh_smooth add a mesh without)");
    return add_mesh("rt_scene_add_mesh_uv", s, n_vertices, xyz, normals ? n_normals : 0u, normals, n_uvs, uvs, n_triangles, indices, normal_indices, uv_indices, mat, scale, rotate_y_degrees, translate,
                    out_first, out_added);
}

// The image the book loads from earthmap.jpg is not redistributable here: a synthetic 256 x 128 "planet" (integer
// arithmetic only, so that the oracle generates the same bytes): oceans, land masses, polar caps.
static void synthetic_earth(std::vector<uint8_t>& img, uint32_t& w, uint32_t& h) {
    w = 256; h = 128;
    img.resize((size_t)w * h * 3);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            uint32_t f = (x * x / 64u + y * y / 32u + x * y / 128u + 3u * x) % 64u;
            bool land = f < 26u, ice = y < 9u || y > 118u;
            uint8_t* px = &img[((size_t)y * w + x) * 3];
            if (ice) { px[0] = 235; px[1] = 240; px[2] = 245; }
            else if (land) { px[0] = (uint8_t)(60u + 2u * f); px[1] = (uint8_t)(120u + f); px[2] = 50; }
            else { px[0] = 25; px[1] = (uint8_t)(60u + f / 2u); px[2] = (uint8_t)(140u + f); }
        }
}

// final_scene() of "Ray Tracing: The Next Week" (BASELINE.json configs[4]; nothing of it exists in the reference):
// 400 ground boxes of random height (2400 quads), an area light, a moving sphere, glass, metal, a glass ball filled with a
// blue medium, a thin global fog, an image-textured sphere, a marble sphere and a rotated, translated cluster of 1000 small
// spheres, under ONE median-split BVH.  Uniforms: the host stream of rt_host_uniforms(seed), one per box, three per sphere.
extern "C" int rt_scene_book2_final(uint64_t seed, rt_scene** out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_scene_book2_final: null out");
    rt_scene* s = new rt_scene();
    Rng g;
    g.init(seed, 0u, 0u, RT_STREAM_SCENE);
    auto material = [&](uint32_t type, f3 albedo, float param) {
        float a[3]; st3(a, albedo);
        int32_t id = 0;
        rt_scene_add_material(s, type, a, param, nullptr, &id);
        return id;
    };
    auto sphere = [&](f3 c, float r, int32_t mat) { float p[3]; st3(p, c); add_prim(s, p, p, r, mat, false, nullptr); };
    const int32_t ground = material(RT_MAT_LAMBERTIAN, mk3(0.48f, 0.83f, 0.53f), 0.0f);
    for (int i = 0; i < 20; i++)
        for (int j = 0; j < 20; j++) {
            const float w = 100.0f;
            float x0 = -1000.0f + (float)i * w, z0 = -1000.0f + (float)j * w, y0 = 0.0f;
            float x1 = x0 + w, y1 = 1.0f + 100.0f * g.next(), z1 = z0 + w;
            cornell_box(s, mk3(x0, y0, z0), mk3(x1, y1, z1), 0.0f, mk3(0.0f), ground);
        }
    cornell_quad(s, mk3(123, 554, 147), mk3(300, 0, 0), mk3(0, 0, 265), material(RT_MAT_DIFFUSE_LIGHT, mk3(7.0f), 0.0f));
    {
        float c0[3] = {400, 400, 200}, c1[3] = {430, 400, 200};
        add_prim(s, c0, c1, 50.0f, material(RT_MAT_LAMBERTIAN, mk3(0.7f, 0.3f, 0.1f), 0.0f), true, nullptr);
    }
    const int32_t glass = material(RT_MAT_DIELECTRIC, mk3(1.0f), 1.5f);
    sphere(mk3(260, 150, 45), 50.0f, glass);
    sphere(mk3(0, 150, 145), 50.0f, material(RT_MAT_METAL, mk3(0.8f, 0.8f, 0.9f), 1.0f));
    sphere(mk3(360, 150, 145), 70.0f, glass);
    sphere(mk3(360, 150, 145), 70.0f, material(RT_MAT_ISOTROPIC, mk3(0.2f, 0.4f, 0.9f), 0.2f));
    sphere(mk3(0, 0, 0), 5000.0f, material(RT_MAT_ISOTROPIC, mk3(1.0f), 0.0001f));
    {
        uint32_t w = 0, h = 0;
        synthetic_earth(s->image, w, h);
        s->image_w = w; s->image_h = h;
    }
    sphere(mk3(400, 200, 400), 100.0f, material(RT_MAT_LAMBERTIAN_IMAGE, mk3(1.0f), 0.0f));
    rt_scene_set_perlin(s, seed);
    sphere(mk3(220, 280, 300), 80.0f, material(RT_MAT_LAMBERTIAN_NOISE, mk3(0.5f), 0.2f));
    const int32_t white = material(RT_MAT_LAMBERTIAN, mk3(0.73f), 0.0f);
    const float rad = radians(15.0f), c = cosf(rad), sn = sinf(rad);
    for (int j = 0; j < 1000; j++) {
        f3 ctr;
        ctr.x = 165.0f * g.next(); ctr.y = 165.0f * g.next(); ctr.z = 165.0f * g.next();
        sphere(rot_y(ctr, c, sn) + mk3(-100, 270, 395), 10.0f, white);   // translate(rotate_y(.., 15), (-100, 270, 395))
    }
    const float black[3] = {0.0f, 0.0f, 0.0f};
    rt_scene_set_background(s, 1, black);
    int rc = rt_scene_build_bvh_topdown(s);
    if (rc != RT_OK) { delete s; return rc; }
    *out = s;
    return RT_OK;
}

extern "C" int rt_scene_cornell_box(rt_scene** out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_scene_cornell_box: null out");
    rt_scene* s = new rt_scene();
    const float red[3] = {0.65f, 0.05f, 0.05f}, white[3] = {0.73f, 0.73f, 0.73f}, green[3] = {0.12f, 0.45f, 0.15f}, light[3] = {15.0f, 15.0f, 15.0f};
    int32_t m_red, m_white, m_green, m_light;
    rt_scene_add_material(s, RT_MAT_LAMBERTIAN, red, 0.0f, nullptr, &m_red);
    rt_scene_add_material(s, RT_MAT_LAMBERTIAN, white, 0.0f, nullptr, &m_white);
    rt_scene_add_material(s, RT_MAT_LAMBERTIAN, green, 0.0f, nullptr, &m_green);
    rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, light, 0.0f, nullptr, &m_light);
    cornell_quad(s, mk3(555, 0, 0), mk3(0, 555, 0), mk3(0, 0, 555), m_green);
    cornell_quad(s, mk3(0, 0, 0), mk3(0, 555, 0), mk3(0, 0, 555), m_red);
    cornell_quad(s, mk3(343, 554, 332), mk3(-130, 0, 0), mk3(0, 0, -105), m_light);
    cornell_quad(s, mk3(0, 0, 0), mk3(555, 0, 0), mk3(0, 0, 555), m_white);
    cornell_quad(s, mk3(555, 555, 555), mk3(-555, 0, 0), mk3(0, 0, -555), m_white);
    cornell_quad(s, mk3(0, 0, 555), mk3(555, 0, 0), mk3(0, 555, 0), m_white);
    cornell_box(s, mk3(0, 0, 0), mk3(165, 330, 165), 15.0f, mk3(265, 0, 295), m_white);
    cornell_box(s, mk3(0, 0, 0), mk3(165, 165, 165), -18.0f, mk3(130, 0, 65), m_white);
    const float black[3] = {0.0f, 0.0f, 0.0f};
    rt_scene_set_background(s, 1, black);
    int rc = rt_scene_build_bvh_topdown(s);
    if (rc != RT_OK) { delete s; return rc; }
    *out = s;
    return RT_OK;
}

// The Cornell box lit by a lamp: no ceiling quad light, a sphere light of radius 40 at (278, 470, 278) emitting (40, 40, 40), the two boxes as they are.
extern "C" int rt_scene_cornell_lamp(rt_scene** out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_scene_cornell_lamp: null out");
    rt_scene* s = new rt_scene();
    const float red[3] = {0.65f, 0.05f, 0.05f}, white[3] = {0.73f, 0.73f, 0.73f}, green[3] = {0.12f, 0.45f, 0.15f}, light[3] = {40.0f, 40.0f, 40.0f};
    int32_t m_red, m_white, m_green, m_light;
    rt_scene_add_material(s, RT_MAT_LAMBERTIAN, red, 0.0f, nullptr, &m_red);
    rt_scene_add_material(s, RT_MAT_LAMBERTIAN, white, 0.0f, nullptr, &m_white);
    rt_scene_add_material(s, RT_MAT_LAMBERTIAN, green, 0.0f, nullptr, &m_green);
    rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, light, 0.0f, nullptr, &m_light);
    cornell_quad(s, mk3(555, 0, 0), mk3(0, 555, 0), mk3(0, 0, 555), m_green);
    cornell_quad(s, mk3(0, 0, 0), mk3(0, 555, 0), mk3(0, 0, 555), m_red);
    cornell_quad(s, mk3(0, 0, 0), mk3(555, 0, 0), mk3(0, 0, 555), m_white);
    cornell_quad(s, mk3(555, 555, 555), mk3(-555, 0, 0), mk3(0, 0, -555), m_white);
    cornell_quad(s, mk3(0, 0, 555), mk3(555, 0, 0), mk3(0, 555, 0), m_white);
    cornell_box(s, mk3(0, 0, 0), mk3(165, 330, 165), 15.0f, mk3(265, 0, 295), m_white);
    cornell_box(s, mk3(0, 0, 0), mk3(165, 165, 165), -18.0f, mk3(130, 0, 65), m_white);
    const float lamp_at[3] = {278.0f, 470.0f, 278.0f};
    rt_scene_add_sphere(s, lamp_at, 40.0f, m_light, nullptr);
    const float black[3] = {0.0f, 0.0f, 0.0f};
    rt_scene_set_background(s, 1, black);
    int rc = rt_scene_build_bvh_topdown(s);
    if (rc != RT_OK) { delete s; return rc; }
    *out = s;
    return RT_OK;
}

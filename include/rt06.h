/*
 * rt06.h — C ABI of the MI355X-native path-tracer hot path.
 *
 * This is the drop-in boundary for the per-pixel sample loop of
 * SuperCat908809/Ray-Tracing-v06.  The reference has no FFI layer; the boundary
 * the hot path sits behind is its C++ class `Renderer`
 * (main/src/Renderer.h:38-46) plus the scene vocabulary that produces the
 * `world` argument.  Each entry point below names the reference interface it
 * replaces.  The reference-shaped C++ classes in include/rt06/ (Renderer,
 * SphereHandle, BVH_Handle::Factory, cameras, materials, scenes) are thin
 * header-only wrappers over exactly these functions.
 *
 * Conventions
 *  - plain pointers and sizes only; every function returns an int status
 *    (0 = RT_OK) and never throws; rt_last_error() returns the message of the
 *    last failure on the calling thread.  The reference's CUDA_ASSERT is a
 *    no-op in Release (utilities/cuda_utilities/cuError.h:25-29); this ABI is
 *    never silent.
 *  - all floating point is IEEE fp32; vectors are float[3] (x,y,z).
 *  - the framebuffer is row-major float RGBA, 16 B per pixel, alpha = 1,
 *    row 0 = BOTTOM row of the image, values sqrt-gamma in [0,1]
 *    (Renderer.cu:206-216).
 *  - objects are not thread-safe; distinct objects are independent.
 */
#ifndef RT06_H
#define RT06_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERR_INVALID 1   /* bad argument / malformed scene                */
#define RT_ERR_HIP 2       /* a HIP runtime call failed                     */
#define RT_ERR_NO_DEVICE 3 /* no usable gfx950 device                       */
#define RT_ERR_STACK 4     /* BVH deeper than the traversal stack allows    */

/* ------------------------------------------------------------------ */
/* GPU-linear scene records (what hittable_list / bvh_node / BVH flatten to) */
/* ------------------------------------------------------------------ */

/* == BVH::Node, rt_engine/geometry/BVH.cuh:16-25 (32 B, same field order).
 * RT_WORLD_BVH      : left == -1  -> leaf, right = primitive index;
 *                     otherwise left/right are child node indices.
 * RT_WORLD_NODE_TREE: (== bvh_node, rt_engine/geometry/bvh_node.cuh:9-25)
 *                     left/right are child references: r >= 0 is a node
 *                     index, r < 0 is primitive index (-r - 1).            */
typedef struct rt_bvh_node {
    float   min[3];
    float   max[3];
    int32_t left;
    int32_t right;
} rt_bvh_node;

#define RT_PRIM_MOVING 0x80000000u
/* Sphere (SphereHittable.cuh:35-52) / MovingSphere (:70-87) + its material
 * binding (SphereHittable{sphere*,mat*}, :56-67), 32 B.
 * mat = material index, bit 31 set for a MovingSphere (c1 is then used).   */
typedef struct rt_prim {
    float    c0[3];
    float    radius;
    float    c1[3];
    uint32_t mat;
} rt_prim;

/* ---- beyond the reference (the reference has no quads, no emission, no background colour:
 * only the commented `accum_radiance` placeholders of Renderer.cu:142,152,157,163,179).  Semantics follow
 * "Ray Tracing: The Next Week" (quad(Q,u,v), diffuse_light, camera background) in the reference's conventions.
 * PARITY UNPINNED: checked GPU against the build's own CPU oracle only. ---- */
/* quad(Q,u,v,mat): plane point Q, edge vectors u and v; normal/D/w are the cached plane quantities
 * (n = cross(u,v), normal = unit(n), D = dot(normal,Q), w = n/dot(n,n)), filled by rt_scene_add_quad.  80 B.
 * kind: RT_QUAD_PARALLELOGRAM (0, what every quad was: the interior is 0 <= alpha, beta <= 1) or RT_QUAD_TRIANGLE (1, the book's `tri`: the
 * same plane and coordinates, the interior is alpha >= 0, beta >= 0, alpha + beta <= 1 — the triangle Q, Q + u, Q + v).  In a flat world the
 * triangles FOLLOW the parallelograms: a kind above 1, or a kind-1 record in front of a kind-0 one, is refused before any kernel reads it.   */
#define RT_QUAD_PARALLELOGRAM 0u
#define RT_QUAD_TRIANGLE 1u
typedef struct rt_quad {
    float    Q[3];      float D;
    float    u[3];      uint32_t mat;
    float    v[3];      uint32_t kind;
    float    normal[3]; float pad1;
    float    w[3];      float pad2;
} rt_quad;

enum {
    RT_MAT_LAMBERTIAN = 0,         /* LambertianAbstract  cu_materials.cuh:44-65  param unused          */
    RT_MAT_METAL = 1,              /* MetalAbstract       cu_materials.cuh:68-96  param = fuzz          */
    RT_MAT_DIELECTRIC = 2,         /* DielectricAbstract  cu_materials.cuh:106-144 param = ior          */
    RT_MAT_LAMBERTIAN_CHECKER = 3, /* LambertianTexture   cu_materials.cuh:16-41  albedo/albedo2 = even/odd colour, param = 1/scale */
    RT_MAT_DIFFUSE_LIGHT = 4,      /* diffuse_light of "The Next Week" (not in the reference): emits albedo, never scatters    */
    RT_MAT_ISOTROPIC = 5,          /* isotropic phase function of "The Next Week" (not in the reference): a SPHERE with this
                                    * material is a constant_medium bounded by it; albedo = colour, param = density          */
    RT_MAT_LAMBERTIAN_NOISE = 6,   /* lambertian(noise_texture(scale)) of "The Next Week" (not in the reference): colour =
                                    * albedo * (1 + sin(param * p.z + 10 * turb(p, 7))) over the world's Perlin tables        */
    RT_MAT_LAMBERTIAN_IMAGE = 7    /* lambertian(image_texture) of "The Next Week": colour = the world's RGB8 image at (u, v) — on a sphere
                                    * sphere::get_sphere_uv of the normal, on a quad the planar coordinates (alpha, beta) of quad::hit;
                                    * albedo2[0] = which image of the texture table (rt_scene_add_image), 0 = the world's own; param unused */
};
typedef struct rt_material {
    float    albedo[3];
    float    param;
    float    albedo2[3];
    uint32_t type;
} rt_material;

enum {
    RT_WORLD_BVH = 0,       /* flat index-linked BVH          (BVH.cu:54-106)           */
    RT_WORLD_LIST = 1,      /* HittableList                   (HittableList.cuh:21-34)  */
    RT_WORLD_NODE_TREE = 2  /* pointer-recursive bvh_node     (bvh_node.cuh:19-24)      */
};
/* The `const Hittable* d_world_ptr` argument of Renderer::MakeRenderer,
 * resolved to flat host arrays.  Borrowed during rt_renderer_create only.   */
/* Perlin noise tables of "The Next Week" (perlin::randvec, perm_x/y/z), generated by rt_scene_set_perlin; 6144 B */
typedef struct rt_perlin {
    float   randvec[256][3];
    int32_t perm[3][256];
} rt_perlin;

typedef struct rt_world_flat {
    uint32_t kind;         /* RT_WORLD_*                                              */
    int32_t  root;         /* root node index (BVH: last node; NODE_TREE: child ref)  */
    uint32_t n_nodes;
    uint32_t n_prims;
    uint32_t n_materials;
    uint32_t max_stack;    /* traversal-stack bound derived from the tree at build time */
    float    bounds_min[3];/* world bounds (HittableList pre-test, HittableList.cuh:22) */
    float    bounds_max[3];
    const rt_bvh_node* nodes;
    const rt_prim*     prims;
    const rt_material* materials;
    /* extension (see rt_quad): a primitive index i >= n_prims means quad i - n_prims; the triangles are the last of the quads */
    const rt_quad*     quads;
    uint32_t n_quads;
    uint32_t background;         /* 0: the reference's sky gradient (Renderer.cu:150-151); 1: background_color; 2: the renderer's environment map (rt_renderer_environment) */
    float    background_color[3];
    uint32_t image_width;        /* RT_MAT_LAMBERTIAN_IMAGE: one RGB8 image per world, row 0 = top (as stb_image loads it) */
    const rt_perlin* perlin;     /* RT_MAT_LAMBERTIAN_NOISE: the world's noise tables, or NULL                            */
    const uint8_t*   image;      /* image_width * image_height * 3 bytes, or NULL                                         */
    uint32_t image_height;
    uint32_t traversal;          /* RT_WORLD_BVH only: RT_TRAVERSAL_STACK (0, the live path), RT_TRAVERSAL_QUEUE (1) or RT_TRAVERSAL_WIDE4 (2) */
} rt_world_flat;                 /* 128 B */

/* How BVH::ClosestIntersection walks the tree (rt_scene_set_traversal).
 * STACK: the reference's live depth-first walk, near child first (BVH.cu:54-106, `_USE_PRIO_QUEUE false`) — every streaming kernel.
 * QUEUE: the distance-sorted queue the reference carries but disables (BVH.cu:17-49, :80-86): best-first over the whole frontier,
 *        with its off-by-one (`distances[head]` written after `head++`, :37-39) FIXED.  Capacity 32 (_PRIO_QUEUE_ELEM_COUNT) is
 *        checked: an overflow is RT_ERR_STACK at the next synchronising call, never silent.  Renders on the streaming kernel
 *        (variant 0 / 2: its queue mode — a lane walks its whole trace with the queue when the trace begins; the framebuffer is
 *        the oracle's bit for bit) and on the baseline kernel (variant 1); the stack-walking variants 3-5 refuse it.  On the
 *        Book-1 final scene it saves 0.6 % of the box tests and costs 4.8 % more leaf tests (instrumented oracle); its frontier
 *        is one sorted list per ray, so it cannot share the wave-level hot loop: 1.29 against 5.6 Gsamples/s (EXPERIMENTS.md E2).
 * WIDE4: a 4-wide walk of the SAME binary tree (not in the reference, whose nodes are binary, BVH.cuh:16-25): a visit looks
 *        two levels down — up to four grandchild boxes, tested against rec.distance, nearest first, pushed far-to-near, culling at push time
 *        only (BVH.cu:87-96's rule generalised); the intermediate children's boxes are not tested.  Its 32 entries (at most 3 * ceil(depth / 2) + 1
 *        are needed) are checked like the queue's: RT_ERR_STACK at the next synchronising call.  Oracle twin: orc_world.traversal == 2.  Renders where the queue renders (streaming kernel's
 *        lane-walk mode bit-identical to the oracle, baseline kernel); measured next to the binary walk in EXPERIMENTS.md E3.               */
enum { RT_TRAVERSAL_STACK = 0, RT_TRAVERSAL_QUEUE = 1, RT_TRAVERSAL_WIDE4 = 2 };

enum {
    RT_CAM_PINHOLE = 0,  /* PinholeCamera     cu_Cameras.cuh:12-31 */
    RT_CAM_DEFOCUS = 1,  /* DefocusBlurCamera cu_Cameras.cuh:34-65 */
    RT_CAM_MOTION = 2,   /* MotionBlurCamera  cu_Cameras.cuh:68-90 */
    /* the lens cameras (below; not in the reference): 3 to 15 and 20 and above stay "unknown camera type" */
    RT_CAM_PERSPECTIVE = 16,
    RT_CAM_ORTHOGRAPHIC = 17,
    RT_CAM_FISHEYE = 18,
    RT_CAM_PANORAMA = 19
};
/* Camera POD, passed by value to the kernel like LaunchParams::cam
 * (Renderer.cu:99-108,117).  For PINHOLE/MOTION u,v are pre-scaled by the
 * viewport; for DEFOCUS and the lens cameras they are unit vectors and
 * viewport_* are separate.                                                  */
typedef struct rt_camera {
    uint32_t type;
    float o[3], u[3], v[3], w[3];
    float viewport_width, viewport_height;
    float lens_radius, focus_dist;
    float t0, t1;
} rt_camera;

const char* rt_last_error(void);

/* ------------------------------------------------------------------ */
/* cameras — constructors of cu_Cameras.cuh:16-28, 40-52, 73-85        */
/* ------------------------------------------------------------------ */
int rt_camera_pinhole(const float lookfrom[3], const float lookat[3], const float up[3],
                      float vfov, float aspect, rt_camera* out);
int rt_camera_defocus(const float lookfrom[3], const float lookat[3], const float up[3],
                      float vfov, float aspect, float aperture, float focus_dist, rt_camera* out);
int rt_camera_motion(const float lookfrom[3], const float lookat[3], const float up[3],
                     float vfov, float aspect, float time0, float time1, rt_camera* out);

/* ------------------------------------------------------------------ */
/* lens cameras — a projection, an optional thin lens and an optional shutter on one record.  Not in the reference, whose three
 * types exclude each other (DefocusBlurCamera has no time, MotionBlurCamera no lens).  The record keeps its 76 bytes:
 *   o, u, v, w                       the UNIT basis of DefocusBlurCamera's constructor (w = towards lookat, u = normalize(cross(up, w)), v = cross(w, u))
 *   viewport_width, viewport_height  the projection's two parameters (a, b), below
 *   lens_radius, focus_dist          the lens; lens_radius == 0: no lens and no lens draw
 *   t0, t1                           the shutter; t0 == t1: every ray has time t0 and there is no time draw
 * (a, b):  PERSPECTIVE   tan(vfov / 2) * aspect, tan(vfov / 2)              (what DEFOCUS stores)
 *          ORTHOGRAPHIC  half width, half height of the view window in world units
 *          FISHEYE       equidistant; b = radians(fov) / 2 across the image's height, a = b * aspect; sqrt(a^2 + b^2) < pi (the frame's corner stays
 *                        short of the back pole); no circular mask, every pixel of the rectangle has a ray
 *          PANORAMA      equirectangular; half horizontal and half vertical span in radians, 0 < a <= pi, 0 < b <= pi / 2; full: (pi, pi / 2)
 * THE RULE (lens_camera_draw / lens_camera_ray, csrc/rt_device_funcs.hpp), in fp32, every operation rounded on its own (no contraction), + - * / sqrt,
 * comparisons and the library's rt_sinf only; cos x = sin(x + 0x1.921fb6p+0f), where sin is rt_sinf throughout.  (s, t) = the jittered NDC point of a sample.  Vector expressions are
 * per component; a sum of three terms is (first + second) + third.
 *   draws, in this order: the pixel jitter (InUnit<2>); the lens point (la, lb) (InUnit<2>) iff lens_radius > 0; one uniform x iff t0 != t1.
 *   time = t0 * (1 - x) + t1 * x, or t0.
 *   off  = (u * la + v * lb) * lens_radius                                   (with a lens)
 *   PERSPECTIVE without a lens:  ray.o = o,        ray.d = (w + (u * a) * s) + (v * b) * t
 *   PERSPECTIVE with a lens:     ray.o = o + off,  ray.d = ((w * focus_dist + ((u * a) * focus_dist) * s) + ((v * b) * focus_dist) * t) - off
 *                                (DefocusBlurCamera::sample_ray's own order, cu_Cameras.cuh:54-64)
 *   the others:  (o0, d0) from the projection;  ray.o = o0 + off, ray.d = d0 * focus_dist - off  with a lens;  ray.o = o0, ray.d = d0  without
 *   ORTHOGRAPHIC  o0 = (o + (u * a) * s) + (v * b) * t,  d0 = w
 *   FISHEYE       x = a * s, y = b * t, th = sqrt(x * x + y * y);  th == 0: d0 = w;  else k = sin(th) / th,
 *                 d0 = (w * cos th + u * (x * k)) + v * (y * k)
 *   PANORAMA      ph = a * s, lm = b * t, cl = cos lm;  d0 = (w * (cl * cos ph) + u * (cl * sin(ph))) + v * sin(lm)
 * Directions are not normalised, as the reference's are not.  Two equivalences, bit for bit in rays and draws: a DEFOCUS record with type = 16 and
 * t0 = t1 = 0 is that DEFOCUS camera; a PINHOLE (also t0 = t1 = 0) or MOTION record with type = 16, viewport_* = 1, lens_radius = 0 is that camera.
 * Orientation of a panorama: looking along +x with +y up, u is -z, and a full panorama sees an unrotated environment map texel for texel (the frame's
 * row 0 is the bottom, the map's row 0 the top).
 * The constructors take aperture = 2 * lens_radius like rt_camera_defocus; orthographic: the window's full height and its aspect; fisheye: the angle across
 * the image's height in degrees and the aspect; panorama: the full spans in degrees.  They and, for these four types, rt_renderer_create / _set_camera and
 * the rt_multi_renderer twins validate: every field finite, a, b > 0, lens_radius >= 0, focus_dist > 0 where there is a lens, the bounds above.  A refused
 * call changes nothing and names the field.
 * Rendered by every streaming variant (0, 2 to 6) — their primary rays come from primary_rays_lens_kernel — with feature buffers, refinement, run-ahead, light
 * sampling and rt_multi_renderer.  Refused by the baseline kernel (variant 1, and worlds only it renders), rt_probe_radiance, rt_probe_camera(_tape). */
/* ------------------------------------------------------------------ */
int rt_camera_perspective(const float lookfrom[3], const float lookat[3], const float up[3], float vfov, float aspect,
                          float aperture, float focus_dist, float time0, float time1, rt_camera* out);
int rt_camera_orthographic(const float lookfrom[3], const float lookat[3], const float up[3], float height, float aspect,
                           float aperture, float focus_dist, float time0, float time1, rt_camera* out);
int rt_camera_fisheye(const float lookfrom[3], const float lookat[3], const float up[3], float fov, float aspect,
                      float aperture, float focus_dist, float time0, float time1, rt_camera* out);
int rt_camera_panorama(const float lookfrom[3], const float lookat[3], const float up[3], float hspan_degrees, float vspan_degrees,
                       float aperture, float focus_dist, float time0, float time1, rt_camera* out);
/* HOST (no GPU): the camera's rule on given cases, any of the seven types (the old three through camera_sample_ray): st n*2, uniforms from `tape` as
 * rt_probe_camera_tape takes them (case i draws tape[offsets[2i] ..] for offsets[2i+1] uniforms) -> ray n*7 (o, d, time), uniforms consumed n.  The
 * pixel jitter is the caller's: (s, t) is given.                                                                                                    */
int rt_camera_rays_batch(const rt_camera* cam, size_t n, const float* st, const uint32_t* tape, size_t tape_len,
                         const uint32_t* offsets, float* out_rays, uint32_t* out_draws);

/* ------------------------------------------------------------------ */
/* scene construction — host side, replaces SphereHandle / newOnDevice /
 * BVH_Handle::Factory / HittableList / bvh_node / SceneBook2BVH::Factory  */
/* ------------------------------------------------------------------ */
typedef struct rt_scene rt_scene;

int rt_scene_create(rt_scene** out);
void rt_scene_destroy(rt_scene* s);

/* newOnDevice<LambertianAbstract<G>>(albedo) etc. (Scenes.cu:222,235,242,248).
 * Returns the material index in *out_id.                                    */
int rt_scene_add_material(rt_scene* s, uint32_t type, const float albedo[3], float param,
                          const float albedo2[3], int32_t* out_id);
/* SphereHandle::MakeSphere / MakeMovingSphere (SphereHittable.cuh:134-154).
 * Returns the primitive index; bounds as getSphereBounds/getMovingSphereBounds
 * (SphereHittable.cu:52-54, 85-89).                                          */
int rt_scene_add_sphere(rt_scene* s, const float center[3], float radius, int32_t mat, int32_t* out_prim);
int rt_scene_add_moving_sphere(rt_scene* s, const float c0[3], const float c1[3], float radius,
                               int32_t mat, int32_t* out_prim);
int rt_scene_prim_bounds(const rt_scene* s, int32_t prim, float out_min[3], float out_max[3]);
/* quad(Q,u,v,mat) of "The Next Week"; returns the quad index (worlds: BVH builders and HittableList, where the
 * quads follow the spheres; bvh_node trees take spheres only).                                            */
int rt_scene_add_quad(rt_scene* s, const float Q[3], const float u[3], const float v[3], int32_t mat, int32_t* out_quad);
/* tri(Q,u,v,mat) of "The Next Week" (a quad whose interior test is alpha >= 0 && beta >= 0 && alpha + beta <= 1; nothing of it is in the
 * reference) from its vertices: Q = a, u = b - a, v = c - a, kind RT_QUAD_TRIANGLE; normal, D and w as rt_scene_add_quad fills them.  Bounds:
 * the box of the three vertices, every axis padded to 1e-4 as a quad's.  RT_ERR_INVALID when dot(n, n) of n = cross(u, v) is not finite and
 * > 0 (a degenerate face).  The scene keeps its triangles behind its parallelograms, whatever the order of the calls: *out_quad is the
 * record's index among the scene's quads at the time of the call (a parallelogram added later moves it up by one).                     */
int rt_scene_add_triangle(rt_scene* s, const float a[3], const float b[3], const float c[3], int32_t mat, int32_t* out_quad);
/* An indexed triangle mesh (the book has none; not in the reference): n_vertices points xyz[3 * i ..], n_triangles faces indices[3 * f ..].
 * Every vertex is scaled, rotated about y and translated on the host — p' = rot_y(p * scale, degrees) + translate, rt_scene_add_box's order
 * and arithmetic (translate NULL = none) — and each face goes through rt_scene_add_triangle.  An index >= n_vertices, a scale that is not
 * finite, or a bad material fails the whole call and leaves the scene unchanged.  Degenerate faces are skipped and counted out:
 * *out_added = faces added, *out_first = index of the first of them among the scene's quads (either may be NULL).                       */
int rt_scene_add_mesh(rt_scene* s, uint32_t n_vertices, const float* xyz, uint32_t n_triangles, const uint32_t* indices, int32_t mat,
                      float scale, float rotate_y_degrees, const float translate[3], int32_t* out_first, uint32_t* out_added);
/* ---- smooth shading (not in the reference): per-vertex normals for triangles.  A triangle record Q, u, v has the vertices a = Q, b = Q + u,
 * c = Q + v; it MAY carry three normals n0, n1, n2, one per vertex in that order.  sizeof(rt_quad) and sizeof(rt_world_flat) are what they were: the normals
 * travel BESIDE the flat world, one 36-byte record per triangle of the flat world in the flat world's triangle order; nine zeros = a flat triangle.
 * The rule, at a hit on such a triangle, after the flat normal f (the record's normal, negated if dot(ray.d, normal) > 0) is formed as ever:
 *   planar = hit_p - Q;  alpha = dot(w, cross(planar, v));  beta = dot(w, cross(u, planar));         (image_value_quad's three lines)
 *   g = (n0 * ((1 - alpha) - beta) + n1 * alpha) + n2 * beta;   l2 = dot(g, g);   !(l2 > 0): keep f   (an all-zero record, cancellation, NaN)
 *   s = g / sqrt(l2);   dot(s, f) < 0: s = -s   (the side of the face the ray sees);   !(dot(ray.d, s) < 0): keep f   (the normal faces AGAINST the ray, always)
 *   normal = s.   Only fp32 + - * / sqrt and comparisons, each rounded on its own.  Everything after it reads `normal` as it did.  Nothing is done about
 * scattered rays that dip under the geometric surface (the shading-normal terminator); a dielectric triangle keeps behaving as on a quad.               */
typedef struct rt_tri_normals { float n0[3], n1[3], n2[3]; } rt_tri_normals;   /* 36 B */
/* rt_scene_add_triangle with a normal per vertex: each must be finite and of non-zero length (RT_ERR_INVALID otherwise, scene unchanged) and is normalised here */
int rt_scene_add_triangle_smooth(rt_scene* s, const float a[3], const float b[3], const float c[3], const float na[3], const float nb[3], const float nc[3],
                                 int32_t mat, int32_t* out_quad);
/* rt_scene_add_mesh with n_normals normals (3 floats each) and, per face, three indices into them (normal_indices; NULL = the vertex indices).  The normals are
 * rotated about y with rt_scene_add_mesh's arithmetic, neither scaled nor translated, and normalised on the host.  A normal that is not finite or has zero length,
 * or a normal index out of range, fails the whole call and leaves the scene unchanged.  Degenerate faces are skipped and counted out as ever.                 */
int rt_scene_add_mesh_smooth(rt_scene* s, uint32_t n_vertices, const float* xyz, uint32_t n_normals, const float* normals, uint32_t n_triangles,
                             const uint32_t* indices, const uint32_t* normal_indices, int32_t mat, float scale, float rotate_y_degrees, const float translate[3],
                             int32_t* out_first, uint32_t* out_added);
/* One record per triangle of the flat world, in its triangle order (record i belongs to quad n_quads - n_triangles + i), carried through everything that permutes
 * triangles: the three BVH builders, the list, a parallelogram added later.  *out_n = 0 (and *out = NULL) when no triangle of the scene has normals.  The
 * pointer stays valid until the scene is modified or destroyed.                                                                                               */
int rt_scene_vertex_normals(const rt_scene* s, const rt_tri_normals** out, uint32_t* out_n);
/* HOST (no GPU): the rule above on n hits — triangle tris[i] (Q, u, v, normal, w read), record vn[i], ray rays[6 i ..] = (o, d), hit distance t[i] ->
 * out_normal[3 i ..], out_interpolated[i] = 1 where the normal is the interpolated one, 0 where it is the flat one.  The function the kernels call.          */
int rt_shading_normal_batch(size_t n, const rt_quad* tris, const rt_tri_normals* vn, const float* rays, const float* t, float* out_normal, uint32_t* out_interpolated);
/* ---- texture coordinates (not in the reference): a (u, v) per vertex of a triangle, in the order a = Q, b = Q + u, c = Q + v.  Like the normals they
 * travel BESIDE the flat world, one 24-byte record per triangle in the flat world's triangle order; sizeof(rt_quad) and sizeof(rt_world_flat) are what they were.
 * The rule changes one thing: the albedo of an RT_MAT_LAMBERTIAN_IMAGE hit on a triangle (parallelograms and spheres look the image up as ever):
 *   planar = hit_p - Q;  alpha = dot(w, cross(planar, v));  beta = dot(w, cross(u, planar));         (image_value_quad's three lines)
 *   tu = (t0.u * ((1 - alpha) - beta) + t1.u * alpha) + t2.u * beta;   tv = (t0.v * ((1 - alpha) - beta) + t1.v * alpha) + t2.v * beta
 *   albedo = the image's texel at (tu, tv): clamp to [0, 1], flip v, nearest texel, 1/255 — the lookup every image hit makes.
 * Only fp32 + - *, each rounded on its own.  There is NO sentinel: a triangle without coordinates carries the identity record (0,0), (1,0), (0,1), under which
 * tu = alpha and tv = beta up to the sign of a zero, so the texel is the one the planar lookup picks and "identity table" == "no table" bit for bit.
 * The image, its wrap mode and its filter are the texture table's (below at rt_scene_add_image): the clamp and the nearest texel named above are
 * the defaults.  No coordinates on parallelograms.                                                                                                           */
typedef struct rt_tri_uvs { float t0[2], t1[2], t2[2]; } rt_tri_uvs;   /* 24 B */
/* rt_scene_add_triangle with a texture coordinate per vertex (ta, tb, tc: two floats each, finite; RT_ERR_INVALID otherwise, scene unchanged) and, optionally,
 * a normal per vertex as rt_scene_add_triangle_smooth takes them (na = nb = nc = NULL: a flat triangle)                                                     */
int rt_scene_add_triangle_uv(rt_scene* s, const float a[3], const float b[3], const float c[3], const float na[3], const float nb[3], const float nc[3],
                             const float ta[2], const float tb[2], const float tc[2], int32_t mat, int32_t* out_quad);
/* rt_scene_add_mesh_smooth (normals = NULL with n_normals = 0: a flat mesh) with n_uvs texture coordinates (2 floats each) and, per face, three indices into them
 * (uv_indices; NULL = the vertex indices).  The coordinates are neither rotated, scaled nor translated.  One that is not finite, or an index out of range, fails
 * the whole call and leaves the scene unchanged.                                                                                                                */
int rt_scene_add_mesh_uv(rt_scene* s, uint32_t n_vertices, const float* xyz, uint32_t n_normals, const float* normals, uint32_t n_uvs, const float* uvs,
                         uint32_t n_triangles, const uint32_t* indices, const uint32_t* normal_indices, const uint32_t* uv_indices, int32_t mat, float scale,
                         float rotate_y_degrees, const float translate[3], int32_t* out_first, uint32_t* out_added);
/* One record per triangle of the flat world, in its triangle order, carried through everything that permutes triangles as the normals are.  *out_n = 0 (and
 * *out = NULL) when every record is the identity.  The pointer stays valid until the scene is modified or destroyed.                                         */
int rt_scene_texture_coords(const rt_scene* s, const rt_tri_uvs** out, uint32_t* out_n);
/* HOST (no GPU): the rule above on n hits — triangle tris[i] (Q, u, v, w read), record uv[i], ray rays[6 i ..] = (o, d), hit distance t[i] -> out_uv[2 i ..] =
 * (tu, tv) BEFORE the clamp.  The function the kernels call.                                                                                                 */
int rt_tri_uv_batch(size_t n, const rt_quad* tris, const rt_tri_uvs* uv, const float* rays, const float* t, float* out_uv);
/* camera::background of "The Next Week": mode 0 = the reference's sky gradient, 1 = constant colour       */
int rt_scene_set_background(rt_scene* s, uint32_t mode, const float color[3]);
/* ---- environment maps (not in the reference): a width x height image of fp32 RGB radiance, row 0 at the top, values finite and >= 0 (they may be
 * far above 1), plus a rotation about y, u0 in [0, 1).  At a miss (no hit), with d = the ray's direction:
 *   n     = normalize(d)                                   (the normalize of the sky gradient)
 *   cy    = clamp(-n.y, -1, 1);  theta = acos cy;  phi = atan2 (-n.z, n.x) + pi_f        (the library's own rt_acosf and rt_atan2f, shared with the CPU oracle)
 *   u     = phi / two_pi_f + u0;  if (u >= 1) u = u - 1;   v = theta / pi_f                  (the constants of the image texture's sphere map)
 *   texel : clamp u, v to [0, 1] as !(x > 0) ? 0 : (x > 1 ? 1 : x) (a NaN lands on 0); v = 1 - v; i = (int)(u * W), j = (int)(v * H), capped at W - 1, H - 1
 *   sky   = that texel's (r, g, b) as stored;   rad = atten * sky + accum_rad                (as for the constant background)
 * Only fp32 + - * / sqrt, comparisons and those two functions, each rounded on its own, no FMA.  With u0 = 0 a direction sees the texel that an image-textured
 * sphere around the viewer shows at normal n.  A miss at the last allowed bounce collects the map as it collects the constant background.  The map is NOT sampled
 * as a light: the light-sampling modes never put it in their tables.  Nearest texel, one map, rotation about y only.
 * rt_scene_set_environment copies the image (3 floats per texel), sets background mode 2 and stores u0 = frac(rotate_y_degrees / 360).  RT_ERR_INVALID, scene
 * unchanged: a texel that is not finite or is negative, a zero dimension, width * height > 2^25, a rotation that is not finite.                                  */
#define RT_ENV_MAX_TEXELS (1u << 25)
int rt_scene_set_environment(rt_scene* s, uint32_t width, uint32_t height, const float* rgb, float rotate_y_degrees);
/* What rt_scene_set_environment stored (*out_w = *out_h = 0, *out_rgb = NULL when the scene has none; rt_scene_set_background drops it).  The pointer stays valid
 * until the scene's environment or background is set again or the scene is destroyed.                                                                            */
int rt_scene_environment(const rt_scene* s, uint32_t* out_w, uint32_t* out_h, const float** out_rgb, float* out_u0);
/* HOST (no GPU): the rule above on n directions dirs[3 i ..] -> out_rgb[3 i ..], out_texel[i] = j * width + i.  The function the kernels call.                   */
int rt_environment_batch(size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* dirs, float* out_rgb, uint32_t* out_texel);
/* ---- environment light sampling: the distribution mode RT_LIGHT_SAMPLING_ENV draws directions from, in proportion to radiance times solid angle.
 * HOST (no GPU).  Built in double, stored as fp32; image row j (0 = the top) is the band n.y in [rowy[j + 1], rowy[j]]:
 *   rowy[j]    = fp32(cos(pi j / H)), rowy[0] = 1 and rowy[H] = -1 exactly;   h_j = rowy[j] - rowy[j + 1] (of the fp32 values);   omega_j = (2 pi / W) h_j
 *   w_ji       = ((0.2126 r + 0.7152 g) + 0.0722 b) h_j
 *   colc[j][i] = fp32(sum over k <= i of w_jk);   rowc[j] = fp32(sum over l <= j of row l's whole sum): running sums in double, rounded when stored
 *   A = rowc[H - 1], R_j = colc[j][W - 1]
 *   density[j][i] = fp32(P_j P_i|j / omega_j), P_j = (rowc[j] - rowc[j - 1]) / A, P_i|j = (colc[j][i] - colc[j][i - 1]) / R_j: differences of the STORED values,
 *                   taken in double, the predecessor of index 0 being 0; P_i|j = 0 in a row with R_j = 0; density 0 where either factor is 0
 * so the density is that of what the binary searches below really draw: a texel whose weight is lost in a running sum has density 0 and is never drawn (the cosine
 * half of the estimator still reaches it).  RT_ERR_INVALID: what rt_scene_set_environment refuses of an image; a null array; A = 0 (an all-black map: nothing to
 * sample); A not finite.  Sizes: rowc[H], rowy[H + 1], colc[H W], density[H W].                                                                                  */
int rt_environment_distribution(uint32_t width, uint32_t height, const float* rgb, float* rowc, float* rowy, float* colc, float* density);
/* The rule, with x1, x2, a, b uniforms in (0, 1]:
 *   x = x1 * A;   if (!(x < A)) x = the float just below A (bit pattern - 1);      j = the smallest row with rowc[j] > x        (binary search)
 *   x = x2 * R_j; if (!(x < R_j)) x = the float just below R_j;                    i = the smallest column with colc[j][i] > x
 *   u = ((float)i + a) / (float)W;   y = rowy[j + 1] + (rowy[j] - rowy[j + 1]) * b;   s2 = 1 - y * y;   s = sqrt(s2 > 0 ? s2 : 0)
 *   t = u - u0; if (t < 0) t = t + 1;   psi = t * two_pi_f - pi_f;   d = (s * sin(psi + half_pi_f), y, -(s * sin psi))          (the library's own rt_sinf)
 * d is unit only up to rounding and is not renormalised.  The density of ANY direction is density[the texel the lookup above puts it in], so a drawn direction
 * that rounding put across a border has its neighbour's.  Only fp32 + - * / sqrt, comparisons, that sine and the lookup, each rounded on its own, no FMA.
 * HOST (no GPU): the rule on n quadruples uniforms[4 i ..] -> out_dir[3 i ..], out_texel[i] = j * width + i as drawn, out_density[i] = the density of out_dir.
 * The functions the kernels call.  Refused as rt_environment_distribution refuses, and for a uniform outside (0, 1] or u0 outside [0, 1).                        */
int rt_environment_sample_batch(size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* uniforms, float* out_dir, uint32_t* out_texel,
                                float* out_density);
/* selects RT_TRAVERSAL_STACK / RT_TRAVERSAL_QUEUE / RT_TRAVERSAL_WIDE4 for the BVH world of this scene (see the enum) */
int rt_scene_set_traversal(rt_scene* s, uint32_t mode);
/* perlin::perlin() of "The Next Week": 256 random unit vectors + three Fisher-Yates permutations, drawn from the
 * build's host stream (rt_host_uniforms, stream id 0x9E81) with this seed                                  */
int rt_scene_set_perlin(rt_scene* s, uint64_t seed);
/* the image of image_texture (the book loads earthmap.jpg; any RGB8 array here), copied                     */
int rt_scene_set_image(rt_scene* s, uint32_t width, uint32_t height, const uint8_t* rgb);
/* ---- the texture table (not in the reference): several RGB8 images per world, each with a wrap mode and a filter.  Entry 0 is the world's image
 * of rt_scene_set_image; rt_scene_add_image appends entries 1, 2, ...  An RT_MAT_LAMBERTIAN_IMAGE material names its entry in rt_material.albedo2[0], as an
 * integer-valued float (0 from every adder before this, so every world means what it meant; not in param, where callers have been free to write anything for
 * this type).  rt_scene_add_material refuses an index that is negative, not an integer or >= RT_MAX_IMAGES.  This is a change at the edge for callers that
 * passed an albedo2 for an image material: any value was accepted and ignored before; now it must be an image index (renderer creation checks it too), and
 * "every world means what it meant" holds for the callers that left albedo2 at zero or NULL, as every adder of this library does.  The device's 16-byte
 * material record carries albedo2[0] in its fourth lane for this type, where it carried param, which nothing read.  The table travels BESIDE the flat world, as the texture coordinates
 * do: sizeof(rt_world_flat) is what it was and rt_world_flat.image stays entry 0's texels.
 * The rule, for entry (W, H, wrap, filter, texels) at the (u, v) a hit has before any clamp (sphere map, planar coordinates or the rule of rt_tri_uvs):
 *   wrap    : REPEAT: x = x - floor(x) (the result may be exactly 1; an infinite x gives NaN).  Then, under both modes, x = !(x > 0) ? 0 : (x > 1 ? 1 : x), so a
 *             coordinate that is not a number becomes 0: column 0 and, after the flip, the bottom row.  Then v = 1 - v.
 *   nearest : i = (int)(u * W), j = (int)(v * H), capped at W - 1, H - 1;  c = the texel's bytes * 0x1.010102p-8f             (image_texel's choice and constant)
 *   bilinear: x = u * W - 0.5;  x0 = floor(x);  fx = x - x0;  columns x0 and x0 + 1, under CLAMP each clamped into [0, W - 1], under REPEAT -1 -> W - 1 and W -> 0;
 *             the same in y;  the four texels converted as in nearest;  per channel c = lerp(lerp(c00, c10, fx), lerp(c01, c11, fx), fy),
 *             lerp(a, b, t) = a + (b - a) * t — this form: a constant image is exactly constant, and fx = 0 returns the texel itself
 * Only fp32 + - * /, comparisons, float/int conversion and floor, each rounded on its own, no FMA.  CLAMP with NEAREST gives the bits image_texel gives for every
 * coordinate that is a number.  No mirror wrap, no mip maps, no filtering of the environment map, images on Lambertian image materials only.                    */
enum { RT_WRAP_CLAMP = 0, RT_WRAP_REPEAT = 1 };
enum { RT_FILTER_NEAREST = 0, RT_FILTER_BILINEAR = 1 };
#define RT_MAX_IMAGES 256u
#define RT_MAX_TABLE_TEXELS (1u << 28)   /* of all the images of one table together */
/* One entry of the table on the host: `first` = the index of its first texel in the table's texel array (3 bytes per texel, rows from the top, images back to back
 * in the entries' order).  width = height = 0: an empty entry (entry 0 of a scene without rt_scene_set_image); a material may not use it.                         */
typedef struct rt_texture { uint32_t width, height, wrap, filter, first; } rt_texture;   /* 20 B */
/* Appends an image (copied) and returns its index (1, 2, ...) in *out_index.  RT_ERR_INVALID, scene unchanged: what rt_scene_set_image refuses, an unknown wrap
 * or filter, a 257th image (RT_MAX_IMAGES counts entry 0), more than RT_MAX_TABLE_TEXELS texels in all.                                                          */
int rt_scene_add_image(rt_scene* s, uint32_t width, uint32_t height, const uint8_t* rgb, uint32_t wrap, uint32_t filter, uint32_t* out_index);
/* The modes of any entry, 0 included (entry 0 may get its modes before or after, or without, its image).                                                       */
int rt_scene_image_sampling(rt_scene* s, uint32_t index, uint32_t wrap, uint32_t filter);
/* The table on the host: *out_n entries (1 + the images added; 0 and NULL pointers for a scene without any image and with default modes) and all texels.  The
 * pointers stay valid until an image or a mode of the scene is set or the scene is destroyed.                                                                  */
int rt_scene_textures(const rt_scene* s, const rt_texture** out_records, uint32_t* out_n, const uint8_t** out_texels);
/* HOST (no GPU): the rule above — out_rgb[3 i ..] = entry index[i] of the table at (u[i], v[i]).  The function the kernels call.  RT_ERR_INVALID: a table
 * rt_renderer_textures would refuse, an index without an entry.                                                                                                 */
int rt_texture_lookup_batch(const rt_texture* records, uint32_t n, const uint8_t* texels, const uint32_t* index, const float* u, const float* v, size_t count,
                            float* out_rgb);
/* HOST (no GPU): noise_texture::value of "The Next Week" as the kernels compute it (RT_MAT_LAMBERTIAN_NOISE: albedo * (1 + sin(scale * z + 10 * turb(p, 7))), fp32,
 * one fixed evaluation order, the library's own sine) — out_rgb[3 i ..] = the marble of `perlin` (rt_scene_set_perlin's tables) with the material's albedo and
 * param (`scale`) at points[3 i ..].  The function the kernels call.  RT_ERR_INVALID: a null argument, whatever n.                                         */
int rt_noise_value_batch(const rt_perlin* perlin, const float albedo[3], float scale, const float* points, size_t n, float* out_rgb);
/* ---- normal maps (not in the reference): an entry of the texture table read as a tangent-space normal map (OpenGL convention: red = +u, green = +v,
 * blue = along the normal; byte 128 is zero) that bends the normal a hit is shaded with.  A map is attached PER MATERIAL, in a table beside the flat world: one
 * 16-byte record per material; rt_material and rt_world_flat are what they were.  Lambertian, checker, noise, image and metal materials take one.
 * Tangents, unnormalised, the directions in which the lookup's u and v grow before the image flip:
 *   sphere, n = its normal: dPdu = (n.z, 0, -n.x), dPdv = (0, 1, 0)          parallelogram, triangle without coordinates: the record's u and v
 *   triangle with coordinates t0, t1, t2: (du1, dv1) = t1 - t0, (du2, dv2) = t2 - t0, det = du1 dv2 - du2 dv1; !(det > 0 || det < 0): no frame, the normal stays;
 *     dPdu = u dv2 - v dv1, dPdv = v du1 - u du2, both negated when det < 0
 * The rule, with c = the entry's texture value at the hit's (u, v) (its own wrap and filter), N = the flat or smooth normal as the shade phase has it:
 *   m = (c - C0) * K per component, C0 = 128.0f * 0x1.010102p-8f, K = fp32(255 / 127);   m.x *= strength; m.y *= strength;   m.x == 0 && m.y == 0: N stays
 *   T = dPdu - N dot(N, dPdu);  tt = dot(T, T);  !(tt > 0): N stays (a sphere's poles);  T = T / sqrt(tt);  B = cross(N, T), negated when dot(B, dPdv) < 0
 *   g = (T m.x + B m.y) + N m.z;  l2 = dot(g, g);  !(l2 > 0): N stays;  s = g / sqrt(l2)
 *   s replaces N only when dot(ray.d, s) is not zero and has the sign of dot(ray.d, N): every hit keeps the facing the rest of the shade phase assumes.
 * Only fp32 + - * / sqrt and comparisons, each rounded on its own, no FMA.  A flat map (bytes 128, 128, z) and strength 0 leave every normal's bits alone, under
 * both filters.  No maps on glass, lights or media; no parallax, displacement, mip maps, terminator correction, object-space maps or tangents from a file.   */
typedef struct rt_normal_map { uint32_t on, image; float strength; uint32_t pad; } rt_normal_map;   /* 16 B, one per material */
/* Attaches entry `image` of the scene's texture table to `material` as its normal map.  RT_ERR_INVALID, scene unchanged: no such material; a dielectric, a light or
 * an isotropic material; image >= RT_MAX_IMAGES; a strength that is not finite or is negative.  The entry itself is checked where a table is given to a renderer. */
int rt_scene_set_normal_map(rt_scene* s, uint32_t material, uint32_t image, float strength);
int rt_scene_clear_normal_map(rt_scene* s, uint32_t material);
/* One record per material of the scene (*out = NULL, *out_n = 0 while no material has a map).  Materials are never permuted: the table is the same under every
 * builder.  The pointer stays valid until the scene is modified or destroyed.                                                                                */
int rt_scene_normal_maps(const rt_scene* s, const rt_normal_map** out, uint32_t* out_n);
/* Where case i takes its tangents from (rt_normal_map_batch): a sphere's normal in a[3 i ..]; a record's u and v in a[], b[]; the same with the triangle's
 * coordinates t0, t1, t2 in tri_uv[6 i ..]; or dPdu and dPdv as given in a[], b[]                                                                           */
enum { RT_NMAP_SURFACE_SPHERE = 0, RT_NMAP_SURFACE_PLANAR = 1, RT_NMAP_SURFACE_TRI_UV = 2, RT_NMAP_SURFACE_GIVEN = 3 };
/* Which way a case left the rule: the normal was replaced, or it stays because the decoded x and y are zero, the coordinates span no area (det), the tangent has
 * no part across the normal (tt), the bent normal has no length (l2), or it would see the ray from the other side                                           */
enum { RT_NMAP_REPLACED = 1, RT_NMAP_FLAT = 2, RT_NMAP_NO_TANGENT = 3, RT_NMAP_NO_LENGTH = 4, RT_NMAP_FACING = 5, RT_NMAP_NO_FRAME = 6 };
/* HOST (no GPU): the two functions the kernels call, on `count` cases — the table as rt_texture_lookup_batch takes it; per case its surface (above), a, b, tri_uv
 * (NULL when no case is RT_NMAP_SURFACE_TRI_UV), the normal N, the ray's direction, the lookup's (u, v), the entry and the strength (finite, >= 0) ->
 * out_normal[3 i ..] (N where it stays), out_path[i] = RT_NMAP_*: the normal was replaced exactly where out_path[i] == RT_NMAP_REPLACED.  RT_ERR_INVALID: a table
 * rt_renderer_textures would refuse, an index without an entry, an unknown surface, a bad strength, a null argument.                                         */
int rt_normal_map_batch(const rt_texture* records, uint32_t n, const uint8_t* texels, size_t count, const uint32_t* surface, const float* a, const float* b,
                        const float* tri_uv, const float* normal, const float* ray_d, const float* u, const float* v, const uint32_t* index, const float* strength,
                        float* out_normal, uint32_t* out_path);
/* ---- microfacet surfaces (not in the reference): a GGX lobe with visible-normal sampling, attached PER MATERIAL in a table beside the flat world,
 * one 16-byte record per material, as a normal map is.  On RT_MAT_METAL the record makes a rough conductor: albedo is F0, the record's roughness replaces the fuzz
 * (which is not read), specular is ignored.  On Lambertian, checker, noise and image materials it lays a glossy dielectric coat of scalar F0 = specular over the
 * base, which stays what it was.  on == RT_MICROFACET_MAPPED multiplies the roughness by the green channel of entry `image` of the texture table at the hit's (u, v).
 * The rule, with N = the shading normal the shade phase holds (after a normal map), d = the ray's direction, r = the roughness, G = the hit's generator:
 *   1  v = -d / sqrt(dot(d, d));  co = dot(N, v);  !(co > 0): RT_MFAC_BACKSIDE, the hit is shaded as if its material had no record (a sphere seen from inside)
 *   2  a = max(r r, 0x1p-10f)
 *   3  s = N.z >= 0 ? 1 : -1;  k = -1 / (s + N.z);  b = (N.x N.y) k;  T = (1 + ((s N.x) N.x) k, s b, -(s N.x));  B = (b, s + (N.y N.y) k, -N.y)
 *   4  h = normalize((a dot(T, v), a dot(B, v), co))
 *   5  l2 = h.x h.x + h.y h.y;  T1 = l2 > 0 ? (-h.y, h.x, 0) / sqrt(l2) : (1, 0, 0);  T2 = cross(h, T1)
 *   6  (t1, t2) = a point of the unit disc, drawn as the lens's is (a rejection loop: the number of uniforms varies);  q = 0.5 (1 + h.z);
 *      t2 = (1 - q) sqrt(max(0, 1 - t1 t1)) + q t2;  nh = (T1 t1 + T2 t2) + h sqrt(max(0, (1 - t1 t1) - t2 t2))
 *   7  m = normalize((a nh.x, a nh.y, max(0, nh.z)));  M = (T m.x + B m.y) + N m.z;  ch = dot(v, M);  x = 1 - min(max(ch, 0), 1);  k5 = ((x x) (x x)) x
 *   8  conductor: F = F0 + (1 - F0) k5 per channel, and the hit is specular.  coat: F = f0 + (1 - f0) k5, one uniform u, specular exactly when u < F; otherwise
 *      RT_MFAC_BASE: the base material's scatter runs verbatim, with the draws, albedo, light-sampling half and weights it would have had without a record
 *   9  w = M (2 ch) - v;  ci = dot(N, w);  !(ci > 0): RT_MFAC_ABSORBED, as a metal's ray below the surface;
 *      G = 2 / (1 + sqrt(1 + ((a a) max(0, 1 - ci ci)) / (ci ci)));  RT_MFAC_SPECULAR: the direction is w, the throughput is multiplied by F G (conductor) or by
 *      G alone (coat: the toss already paid F); no light-sampling weight applies.
 * normalize(x) = x (1 / sqrt(dot(x, x))); max(x, c) = x > c ? x : c and min(x, c) = x < c ? x : c, so a NaN takes c.  Only fp32 + - * / sqrt and comparisons, each
 * rounded on its own, no FMA.  A material without a record changes no bit of any frame; roughness 0 is no special case.  Not done: anisotropy, the height-
 * correlated masking term, multiple-scattering compensation, sampling the lobe towards lights, metallic maps.  Rough refraction has kinds of its own, below. */
typedef struct rt_microfacet { uint32_t on, image; float roughness, specular; } rt_microfacet;   /* 16 B, one per material */
enum { RT_MICROFACET_OFF = 0, RT_MICROFACET_CONSTANT = 1, RT_MICROFACET_MAPPED = 2 };
/* Gives `material` a constant-roughness record.  RT_ERR_INVALID, scene unchanged: no such material; a dielectric, a light or an isotropic material; a roughness
 * or a specular that is not finite or lies outside [0, 1].  A record that is already mapped keeps its map.                                                   */
int rt_scene_set_microfacet(rt_scene* s, uint32_t material, float roughness, float specular);
/* Makes the record of `material` a mapped one: its roughness is multiplied by the green channel of entry `image` of the scene's texture table.  RT_ERR_INVALID:
 * no such material, a material without a record (rt_scene_set_microfacet first), image >= RT_MAX_IMAGES.  The entry is checked where a renderer launches.      */
int rt_scene_set_roughness_map(rt_scene* s, uint32_t material, uint32_t image);
int rt_scene_clear_microfacet(rt_scene* s, uint32_t material);
/* One record per material of the scene (*out = NULL, *out_n = 0 while no material has one), as rt_scene_normal_maps hands its table out                      */
int rt_scene_microfacets(const rt_scene* s, const rt_microfacet** out, uint32_t* out_n);
/* Which way a case left the rule (above) */
enum { RT_MFAC_SPECULAR = 1, RT_MFAC_BASE = 2, RT_MFAC_ABSORBED = 3, RT_MFAC_BACKSIDE = 4 };
/* HOST (no GPU): the function the kernels call, on `count` cases — per case N, d, the roughness (finite, in [0, 1]; no map: the product is the caller's), F0 in
 * f0[3 i ..] (a coat reads f0[3 i] alone), coat[i] != 0 for a coat, and its uniforms: the words tape[offsets[2 i] ..] of which there are offsets[2 i + 1], each k
 * in [1, 2^24] standing for the uniform k 2^-24 (past its end a tape serves 2^23 + 1, which every rejection loop accepts) -> out_dir[3 i ..] (w; zero unless the
 * case is specular), out_weight[3 i ..] (F G or G three times; zero unless specular), out_path[i] = RT_MFAC_*, out_draws[i] = uniforms consumed.
 * RT_ERR_INVALID: a null argument, a tape range outside the tape, a roughness out of range.                                                                    */
int rt_microfacet_batch(size_t count, const float* normal, const float* ray_d, const float* roughness, const float* f0, const uint32_t* coat, const uint32_t* tape,
                        size_t tape_len, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws);
/* ---- rough glass (not in the reference): the same lobe on RT_MAT_DIELECTRIC, reflecting or refracting about a micro-normal.  Record kinds of its
 * own in the same table: on == RT_MICROFACET_GLASS, a constant roughness, and RT_MICROFACET_GLASS_MAPPED, the roughness scaled by the green channel of entry
 * `image` as RT_MICROFACET_MAPPED scales it; specular is stored as 0 and not read.  The rule, with N = the normal the shade phase holds, d = the ray's direction,
 * r = the roughness, ior = the material's index of refraction, G = the hit's generator:
 *   1  back = dot(d, N) > 0;  n = back ? -N : N;  eta = back ? ior : 1 / ior                       (the smooth dielectric's own expressions)
 *   2  v = -d / sqrt(dot(d, d));  co = dot(n, v);  !(co > 0): RT_MFAC_BASE, the smooth dielectric runs verbatim, with its draws
 *   3  M = steps 2 to 7 of the rule above with n for N (the same draws), up to and including M;  ch = dot(v, M)
 *   4  x = 1 - min(max(ch, 0), 1);  r0 = (1 - eta) / (1 + eta);  r0 = r0 r0;  F = r0 + (1 - r0) (((x x) (x x)) x)     (the library's Schlick term, with the ratio)
 *   5  k = 1 - (eta eta) (1 - ch ch);  !(k >= 0): the reflection is total and no uniform is drawn;  otherwise one uniform u, and the hit reflects exactly when F > u
 *   6  reflect:  w = M (2 ch) - v;  ci = dot(n, w);  !(ci > 0): RT_MFAC_ABSORBED;  otherwise RT_MFAC_SPECULAR
 *   7  transmit: w = (-v) eta - M (eta (-ch) + sqrt(k))   (refract(-v, M, eta));  ci = -dot(n, w);  !(ci > 0): RT_MFAC_ABSORBED;  otherwise RT_MFAC_TRANSMITTED
 *      either way the direction is w and the throughput is multiplied by the material's albedo times G = 2 / (1 + sqrt(1 + ((a a) max(0, 1 - ci ci)) / (ci ci))):
 *      the toss paid F or 1 - F, the visible-normal draw paid the masking of v and the Jacobians.  No eta^2 radiance scaling, as the book's glass applies none.
 * The same arithmetic rules as above.  On parallelograms and triangles the shading normal always faces the ray, so such glass is always entered, as smooth glass on
 * them is.  Not done: tinted transmission, normal maps on glass, the eta^2 scaling.                                                                              */
enum { RT_MICROFACET_GLASS = 4, RT_MICROFACET_GLASS_MAPPED = 6 };
enum { RT_MFAC_TRANSMITTED = 5 };
/* Gives `material`, an RT_MAT_DIELECTRIC, a rough-glass record of constant roughness.  RT_ERR_INVALID, scene unchanged: no such material; any other type of
 * material; a roughness that is not finite or lies outside [0, 1].  A record that is already mapped keeps its map.  rt_scene_set_roughness_map on a material
 * with a glass record makes it RT_MICROFACET_GLASS_MAPPED; rt_scene_clear_microfacet clears it.                                                               */
int rt_scene_set_rough_glass(rt_scene* s, uint32_t material, float roughness);
/* HOST (no GPU): the rule on `count` cases, as rt_microfacet_batch runs its own — per case N, d, the roughness (finite, in [0, 1]), the index of refraction and
 * a tape -> out_dir[3 i ..] (w; zero unless specular or transmitted), out_weight[i] (G; zero likewise), out_path[i] = RT_MFAC_*, out_draws[i].               */
int rt_rough_glass_batch(size_t count, const float* normal, const float* ray_d, const float* roughness, const float* ior, const uint32_t* tape, size_t tape_len,
                         const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws);
/* ---- solid glass (not in the reference): a dielectric whose material has an interior record knows inside from outside on parallelograms and
 * triangles too, and absorbs along the way through it.  One record per material beside the flat world, as the microfacet records are; rt_material and
 * rt_world_flat keep their sizes.  sigma = the absorption coefficient per unit length and channel.  The rule (interior_hit), for a hit at parameter t of the ray
 * (o, d) on a dielectric of index ior whose material has a record:
 *   1  back = dot(d, Ng) > 0, Ng = the stored normal normalize(cross(u, v)) of a parallelogram or triangle before any turning (set_face_normal's own comparison,
 *      kept), or — on a sphere — the outward normal (hit - centre) / radius, as ever: a negative radius keeps meaning what it means.  The shading normal n stays what
 *      the shade phase holds by then, the flat or the interpolated normal, facing against the ray.  eta = back ? ior : 1 / ior.  The Schlick toss, reflect, refract
 *      and the rough-glass rule's steps 2 to 7 take (n, eta) as they take them without a record.
 *   2  only when back:  len = sqrt(dot(d, d));  dist = t len;  T_c = rt_expf of -(sigma_c dist) per channel;  albedo = albedo T, before the smooth or the rough rule
 *      touches it (a rough hit's factor is (albedo T) G).  Charged at every back hit, whether it reflects totally, reflects or refracts: the segment that ended there
 *      was inside.
 *   3  a dielectric without a record, and every other material, is untouched, draw for draw.
 * rt_expf, in rt_math.hpp: fp32 + - * /, floor and integer bit operations in one fixed order, no FMA; of +-0 it is 1 exactly, x <= -87 or NaN gives 0, results of x <= 0 lie
 * in [0, 1].  The winding is trusted: a closed mesh must be wound outward (mesh_io.orient_outward).  Known limit: a segment inside the glass that ends on another
 * object is not charged; overlapping or nested solids are undefined.  Not done: the eta^2 scaling, normal maps on glass.                                        */
typedef struct rt_interior { uint32_t on; float sigma[3]; } rt_interior;   /* 16 B, one per material */
enum { RT_INTERIOR_OFF = 0, RT_INTERIOR_SOLID = 1 };
/* Gives `material`, an RT_MAT_DIELECTRIC, an interior record.  RT_ERR_INVALID, scene unchanged: no such material; any other type of material; a sigma that is not
 * finite or is negative.  rt_scene_clear_interior takes it away (no record is no error).  rt_scene_interiors: *out = one record per material (the scene's own
 * memory, valid until the next call on the scene), *out_n = their number — or NULL, 0 while no material has a record.                                         */
int rt_scene_set_interior(rt_scene* s, uint32_t material, const float sigma[3]);
int rt_scene_clear_interior(rt_scene* s, uint32_t material);
int rt_scene_interiors(const rt_scene* s, const rt_interior** out, uint32_t* out_n);
/* HOST (no GPU): the rule on `count` cases — per case Ng (3), n (3; the outward normal of a sphere), d (3), t, ior, sigma (3) and sphere[i] != 0 when the hit is on
 * a sphere (back is then taken on n) -> out_back[i] (0 / 1), out_eta[i], out_T[3 i ..] (ones unless back).                                                    */
int rt_interior_batch(size_t count, const float* Ng, const float* n, const float* d, const float* t, const float* ior, const float* sigma, const uint32_t* sphere,
                      uint32_t* out_back, float* out_eta, float* out_T);
/* HOST: out[i] = rt_expf of x[i]                                                                                                                                  */
int rt_expf_batch(size_t count, const float* x, float* out);
/* ---- alpha cutouts (not in the reference): an image mask decides where a parallelogram or triangle is there — leaves, fences, grilles, decals.
 * One record per material beside the flat world, as the interior records are; rt_material and rt_world_flat keep their sizes.  image = an entry of the scene's
 * texture table, cutoff in [0, 1].  The rule (cutout_keeps), in the leaf phase, for a candidate hit at parameter t of the ray (o, d) that has passed the
 * surface's own test against the closest hit so far, on a material whose record is on:
 *   1  hit_p = o + d t
 *   2  (u, v) = tri_uv of the triangle's rt_tri_uvs record while the renderer has texture coordinates, the planar coordinates (quad_uv) otherwise and on a
 *      parallelogram: the functions the shade phase uses for the same surface
 *   3  c = texture_value(entry[image], u, v), the texture table's rule with the entry's own wrap and filter
 *   4  the hit is kept iff !(c.green < cutoff): a NaN keeps it.  A candidate turned down leaves the closest hit as it was, and the ray goes on to what lies behind.
 * The shade phase recomputes hit_p, (u, v) and the texel from the same t with the same functions, so a mask made from the alpha of the material's own map_Kd
 * agrees with its colour texel for texel.  Deterministic: nothing is drawn, and the order in which a sample consumes its random numbers is untouched.  Known
 * limits: spheres ignore the record (a sphere test yields one root, and looking through a hole at the sphere's own back needs the second); no stochastic
 * opacity; the feature pass knows the rule in mode RT_AOV_FULL alone (modes RT_AOV_PLAIN and RT_AOV_TEXTURED refuse a renderer with a table).                */
typedef struct rt_cutout { uint32_t on; uint32_t image; float cutoff; uint32_t reserved; } rt_cutout;   /* 16 B, one per material */
enum { RT_CUTOUT_OFF = 0, RT_CUTOUT_MASKED = 1 };
/* Gives `material` a cutout record.  RT_ERR_INVALID, scene unchanged: no such material; an RT_MAT_DIFFUSE_LIGHT (the light tables take a light's whole area as
 * emitting) or an RT_MAT_ISOTROPIC; a material that has an interior record (a holed solid has no inside — and rt_scene_set_interior refuses a material that
 * has a cutout); an image index outside [0, RT_MAX_IMAGES); a cutoff that is not finite or lies outside [0, 1].  rt_scene_clear_cutout takes it away (no
 * record is no error).  rt_scene_cutouts: *out = one record per material (the scene's own memory, valid until the next call on the scene), *out_n = their
 * number — or NULL, 0 while no material has a record.                                                                                                       */
int rt_scene_set_cutout(rt_scene* s, uint32_t material, uint32_t image, float cutoff);
int rt_scene_clear_cutout(rt_scene* s, uint32_t material);
int rt_scene_cutouts(const rt_scene* s, const rt_cutout** out, uint32_t* out_n);
/* HOST (no GPU): the rule on `count` cases — the texture table as rt_texture_lookup_batch takes it; per case its surface quads[i] (Q, u, v, w are read), the
 * triangle's coordinates uv[i] (uv = NULL: the planar coordinates for every case), the ray rays[6 i ..] (o, d), t[i] and material[i], an index into the
 * n_records records -> out_keep[i] (0 / 1), out_uv[2 i ..] and out_value[i] = c.green (zeros where the record is off: no lookup is made).                      */
int rt_cutout_batch(const rt_texture* textures, uint32_t n_textures, const uint8_t* texels, size_t count, const rt_quad* quads, const rt_tri_uvs* uv, const float* rays,
                    const float* t, const rt_cutout* records, uint32_t n_records, const uint32_t* material, uint32_t* out_keep, float* out_uv, float* out_value);

/* BVH_Handle::Factory::BuildBVH_TopDown -> _build_bvh_rec1 (BVH.cu:166-210):
 * median split on the longest axis, leaf size 1, post-order numbering, root =
 * last node.  Reorders the primitives (hittables[] = sorted order, :174-177). */
int rt_scene_build_bvh_topdown(rt_scene* s);
/* _build_bvh_rec2 + _find_optimal_split + _partition_by_split (BVH.cu:212-304) */
int rt_scene_build_bvh_sah(rt_scene* s);
/* BuildBVH_BottomUp (BVH.cu:315-384), O(n^3) agglomerative                    */
int rt_scene_build_bvh_bottomup(rt_scene* s);
/* HittableList(objects, count, bounds) (HittableList.cuh:19)                  */
int rt_scene_set_world_list(rt_scene* s);
/* bvh_node(left,right,bounds) (bvh_node.cuh:17).  Child refs: >= 0 node
 * returned earlier, < 0 primitive (-prim - 1).  bounds may be NULL = union of
 * the children's bounds.                                                      */
int rt_scene_add_bvh_node(rt_scene* s, int32_t left_ref, int32_t right_ref,
                          const float bmin[3], const float bmax[3], int32_t* out_ref);
int rt_scene_set_world_node_tree(rt_scene* s, int32_t root_ref);

/* SceneBook2BVH::getWorldPtr (Scenes.h:72) resolved to flat arrays.  Pointers
 * stay valid until the scene is modified or destroyed.                        */
int rt_scene_get_flat(const rt_scene* s, rt_world_flat* out);

/* HOST (no GPU): how many of a flat world's quads are triangles (they are its last *out_n quads) — after the validation every consumer of a
 * flat world runs: RT_ERR_INVALID for a kind above RT_QUAD_TRIANGLE or a triangle in front of a parallelogram.  Not in the reference.       */
int rt_world_triangles(const rt_world_flat* world, uint32_t* out_n);

/* cuHostRND::next (utilities/cuda_utilities/cuHostRND.h:9-32, cuHostRND.cpp:57-65): the host uniform
 * stream scene factories draw from.  Uniforms first .. first+n-1 of the library's counter-based host
 * stream for `seed` (each in (0,1]); stateless, so no generator object is needed.                      */
int rt_host_uniforms(uint64_t seed, uint32_t first, uint32_t n, float* out);

/* Prefab scenes.  The reference draws its layout from cuRAND's host XORWOW
 * stream (cuHostRND, seed 1984), which cannot be reproduced without cuRAND;
 * these use the library's own counter-based host stream with the reference's
 * draw pattern (Scenes.cu:229-252; test.cpp:36-62).
 *  book1_final   : 488 static spheres + BVH   (disabled SceneBook1, Scenes.cu:57-115)
 *  book2_moving  : moving Lambertians + BVH   (live SceneBook2BVH, Scenes.cu:219-270)
 *  three_spheres : Book-1 three-spheres scene as a HittableList (config 1)    */
int rt_scene_book1_final(uint64_t seed, rt_scene** out);
int rt_scene_book2_moving(uint64_t seed, rt_scene** out);
int rt_scene_three_spheres(rt_scene** out);
/* BASELINE.json configs[3]: the Cornell box of "The Next Week" (5 walls, light, two rotated boxes = 18 quads),
 * black background, median-split BVH.  Not in the reference (no quads / emission there).                  */
int rt_scene_cornell_box(rt_scene** out);
/* The Cornell box lit by a lamp: the same walls and boxes without the ceiling quad light, and a sphere light of radius 40 at
 * (278, 470, 278) emitting (40, 40, 40) — the small-emitter world of RT_LIGHT_SAMPLING_ALL.  Host only.                  */
int rt_scene_cornell_lamp(rt_scene** out);
/* box(a, b, mat) of "The Next Week" as 6 quads, rotated about y and translated on the host (the book wraps instances) */
int rt_scene_add_box(rt_scene* s, const float a[3], const float b[3], int32_t mat, float rotate_y_degrees,
                     const float translate[3], int32_t* out_first_quad);
/* BASELINE.json configs[4]: final_scene() of "The Next Week" — 2401 quads, 1008 spheres, two constant media, a marble
 * and an image texture (a synthetic planet stands in for earthmap.jpg), black background, median-split BVH.  Not in the
 * reference.  Camera of the book: lookfrom (478,278,-600), lookat (278,278,0), vfov 40, time 0..1.               */
int rt_scene_book2_final(uint64_t seed, rt_scene** out);

/* ------------------------------------------------------------------ */
/* Renderer — main/src/Renderer.h:38-46                                */
/* ------------------------------------------------------------------ */
typedef struct rt_renderer rt_renderer;

typedef struct rt_render_config {
    uint32_t width, height;       /* Renderer::MakeRenderer args 1-2 */
    uint32_t samples_per_pixel;   /* arg 3 */
    uint32_t max_depth;           /* arg 4 */
    uint64_t seed;                /* reference hard-codes 1984 (Renderer.cu:51) */
    int32_t  device;              /* HIP device ordinal */
    /* tile sharding across the GPUs of one node: this renderer owns the 8x8
     * pixel tiles t with t % world_size == rank (row-major tile order).      */
    uint32_t rank, world_size;
    uint32_t variant;             /* 0 = default (3 where the world allows it, else 2, else 1); 1 baseline wave-per-pixel kernel,
                                     2 streaming kernel with verbatim box tests (IEEE divisions), 3 = 2 + exact division without
                                     dividing (BVH worlds with box coordinates in [2^-40, 2^40)), 4 = 3 + filtered predicates
                                     (experimental, reference features only), 5 = 3 with rays exchanged between tracer and
                                     shader waves of a workgroup through LDS rings (render_kernel_xchg; LDS-resident BVH worlds
                                     of the reference's feature set; measured slower than 3, kept as an opt-in: EXPERIMENTS.md),
                                     6 = 3 in TOLERANCE MODE (opt-in, never chosen by 0): the box tests' plane parameters are
                                     (b - o) * RN(1/d) instead of aabb.cuh:30-31's quotients — inside BASELINE.json's |delta| < 1e-3,
                                     NOT bit-exact by construction (measured: 0 differing pixels on BASELINE configs[1..2] at full
                                     size, dominant kernel 1.24-1.26x faster); LDS-resident RT_WORLD_BVH worlds of the reference's own
                                     feature set only — worlds with quads / lights / media are refused (a quad's edges are its box's
                                     edges: the Cornell box at 5000 spp left the tolerance in one pixel, EXPERIMENTS.md E4).
                                     Same image bits for 2..5; worlds beyond the LDS take the global-memory form of 2 / 3
                                     (rt_renderer_kernel_info).                                                                */
} rt_render_config;

/* Renderer::MakeRenderer (Renderer.cu:31-67).  Copies the flat world; allocates the
 * device framebuffer.  `cam` is the camera of the first launch: the reference keeps
 * a POINTER to the caller's camera and reads it at every Render() (Renderer.cu:117),
 * which a C caller restates with rt_renderer_set_camera before a render (the C++
 * mirror does it inside Render()).  No RNG-state array is needed (counter-based
 * RNG), so init_random_states (Renderer.cu:22-29) has no twin.                  */
int rt_renderer_create(const rt_render_config* cfg, const rt_camera* cam,
                       const rt_world_flat* world, rt_renderer** out);
void rt_renderer_destroy(rt_renderer* r);

/* `params.cam = *m.cam;` of Renderer::Render (Renderer.cu:117): the camera of every launch from now on (render, render_async,
 * refine*).  Validated as in rt_renderer_create (NULL, an unknown type, a bad lens-camera field, a lens camera on the baseline kernel: RT_ERR_INVALID, renderer unchanged).  The camera travels
 * BY VALUE in the kernel arguments, so a launch that is already enqueued keeps the camera it was given.  A camera whose bytes differ
 * from the current one discards the refinement state (samples accumulated -> 0); the same bytes keep it.  The world, the per-pass
 * buffers and the streams are untouched: this is what an animation loop calls instead of destroy + create.                          */
int rt_renderer_set_camera(rt_renderer* r, const rt_camera* cam);
/* Renderer::Render (Renderer.cu:111-137): blocking; launches on the
 * renderer's own stream and waits.                                          */
int rt_renderer_render(rt_renderer* r);
/* Same launch on a caller-provided hipStream_t, no host synchronisation.
 * d_out = device buffer for this rank's shard (rt_renderer_shard_floats
 * floats) or NULL to use the renderer's own framebuffer.
 * What it promises: `d_out` (or the framebuffer) is written by work in the stream's order, behind everything enqueued on `hip_stream` before the
 * call, and is complete for everything enqueued behind it.  Nothing else the caller owns is read or written.  A renderer with two frame slots
 * (rt_renderer_run_ahead_info) generates and traces the frame on a stream of its own, which does not wait for `hip_stream`, and only resolves into
 * `d_out` in the stream's order: calls enqueued back to back overlap each frame's tail with the next frame's start.  The frame's bits are the same.  */
int rt_renderer_render_async(rt_renderer* r, void* hip_stream, float* d_out);
/* Frame slots (run-ahead).  out[0] = slots: 2 when a render is ONE pass of a streaming kernel (variant >= 2) over an RT_WORLD_BVH world, a second set of per-pass buffers fits the
 * budget of rt_renderer_pass_info beside the first, the device gave it, and RT06_RUN_AHEAD is not 0; else 1, and every call runs on the caller's stream
 * alone.  out[1] = render_async calls that ran ahead, out[2] = those of them that found the call before them still unfinished when they were enqueued
 * (so that frames really were in flight together), out[3] = bytes of the second set (the same as the first: 60 B per sample index of a pass).
 * rt_renderer_render, refine steps, the feature pass and the denoiser never run ahead: they order behind every queued render.  Nor does a
 * render_async enqueued while the last call of ANOTHER renderer on the same device is unfinished: two frames in flight on a device is what pays.  */
int rt_renderer_run_ahead_info(rt_renderer* r, uint64_t out[4]);
/* HIP-event time of the last render launch(es) in ms (cudaTimer twin,
 * Renderer.cu:127-136).  Synchronises on the events.                        */
int rt_renderer_last_kernel_ms(rt_renderer* r, float* out_ms);
/* Per-kernel HIP-event times (ms) of one of the last 32 render calls (renders_back = 0: the most recent), measured on the
 * stream the kernels ran on: out[0] = primary_rays_kernel, out[1] = the dominant kernel (render_kernel_stream /
 * render_kernel_xchg), out[2] = resolve_kernel — each SUMMED over the passes of that call (rt_renderer_pass_info).
 * Synchronises on that call's end.  Streaming variants (>= 2) only.  A call that ran ahead (rt_renderer_run_ahead_info) shares the GPU
 * with its neighbours: its three numbers are durations of kernels that ran beside another frame's, and its resolve is timed from behind
 * the wait for its tracer.                                                                                                  */
int rt_renderer_kernel_times(rt_renderer* r, uint32_t renders_back, float out_ms[3]);
/* How a render is cut into passes: out[0] = passes per render, out[1] = samples per pixel per pass, out[2] = HBM bytes per
 * sample index of a pass (12 B radiance + 48 B primary-ray record), out[3] = bytes of the per-pass buffers this renderer
 * holds (sample buffer + primary rays + running sums).  A pass is sized by a budget over ALL of those buffers: 120 GiB by
 * default but at most 45 % of the HBM that is free when the renderer is created (RT06_PASS_BUDGET_BYTES to change it, RT06_PASS_SPP to
 * force the samples per pixel per pass: tests); if the device cannot provide the buffers the passes are halved until it can.           */
int rt_renderer_pass_info(rt_renderer* r, uint64_t out[4]);
/* Which kernel the renderer resolved to: out[0] = variant actually used (1..6), out[1] = 1 when the scene image is
 * LDS-resident (0: baseline kernel, or a world too large for the LDS, served from global memory / L2 with 32-bit
 * references), out[2] = workgroup size, out[3] = workgroups per CU.                                              */
int rt_renderer_kernel_info(rt_renderer* r, uint32_t out[4]);
/* Which instantiation the NEXT launch runs (a diagnostic: it changes no launch).  out[0] = the kernel: RT_KERNEL_BASELINE (variant 1),
 * RT_KERNEL_STREAM (render_kernel_stream) or RT_KERNEL_XCHG (render_kernel_xchg, variant 5); for RT_KERNEL_STREAM out[1..8] are the template
 * arguments read back from the key the kernel table is indexed with: exact, filter, world (RT_WORLD_*; 3 = the BVH walked by the queue / wide4
 * traversal), ext, big, wide, tol, and nee = 1 while light sampling is on.  The other two kernels have no such arguments: zeros.               */
#define RT_KERNEL_BASELINE 0
#define RT_KERNEL_STREAM 1
#define RT_KERNEL_XCHG 2
int rt_renderer_kernel_form(rt_renderer* r, uint32_t out[9]);
/* *out = 1 when the NEXT launch runs an instantiation of the streaming kernel's triangle family: the same nine arguments as above, plus the book's `tri`
 * interior test for the quads of kind RT_QUAD_TRIANGLE.  A world without triangles never does (it keeps the kernels it had); a world with triangles does
 * on every streaming variant but under the queue / wide4 traversal, whose lane walks — like the baseline kernel — read the kind from the flat record.
 * That holds for light-sampling modes 0 to 4.  Mode RT_LIGHT_SAMPLING_TREE has kernels in the triangle family only, so while it is on the answer is 1 for
 * a world without triangles too (all its quads are plain ones: a valid world of that family).                                                           */
int rt_renderer_kernel_triangles(rt_renderer* r, uint32_t* out);
/* *out = 1 when the NEXT launch runs an instantiation of the light-tree family (mode RT_LIGHT_SAMPLING_TREE is on): rt_renderer_kernel_form's nine fields,
 * with nee = 1, plus the tree walk and the choice by area.  A query of its own, so that the nine fields stay what they are.                              */
int rt_renderer_kernel_light_tree(rt_renderer* r, uint32_t* out);
/* *out = 1 when the NEXT launch runs an instantiation of the environment-sampling family (mode RT_LIGHT_SAMPLING_ENV is on): the nine fields with nee = 1 and
 * ext = 2, plus the draw from the map; rt_renderer_kernel_triangles answers 1 too, as under the light tree.  A query of its own, for the same reason.        */
int rt_renderer_kernel_env_light(rt_renderer* r, uint32_t* out);
/* *out = 1 when the next launch runs an instantiation of the normal-map family, as rt_renderer_kernel_env_light answers for its own */
int rt_renderer_kernel_normal_map(rt_renderer* r, uint32_t* out);
/* *out = 1 when the next launch runs an instantiation of the microfacet family: a microfacet table is on — or an interior table (§32), with or
 * without a microfacet table, since the solid-glass forms are microfacet forms that read one more table.  rt_renderer_kernel_normal_map answers 0 then, whether
 * or not a normal-map table is on too: the microfacet forms read both tables.                                                                                 */
int rt_renderer_kernel_microfacet(rt_renderer* r, uint32_t* out);
/* *out = 1 when the NEXT launch runs a form of the solid-glass family: an interior table is on (rt_renderer_kernel_microfacet says what else).  */
int rt_renderer_kernel_interior(rt_renderer* r, uint32_t* out);
/* *out = 1 when the NEXT launch runs a form of the cutout family: a cutout table is on.  Its forms are solid-glass and microfacet forms that
 * read one more table, so rt_renderer_kernel_interior and rt_renderer_kernel_microfacet answer 1 then too; rt_renderer_kernel_form keeps its nine fields.    */
int rt_renderer_kernel_cutout(rt_renderer* r, uint32_t* out);
/* Renderer::DownloadRenderbuffer (Renderer.cu:94-96): width*height*4 floats,
 * row-major, row 0 = bottom.  Only valid for world_size == 1.               */
int rt_renderer_download(rt_renderer* r, float* host_rgba, size_t n_floats);
/* Number of floats in this rank's compact shard (n_local_tiles * 64 * 4);
 * identical on every rank.                                                  */
int rt_renderer_shard_floats(const rt_renderer* r, size_t* out);
/* Rank-0 side of the frame-end gather: `d_gathered` holds world_size shards
 * back to back (rank-major); writes the row-major width*height*4 image.     */
int rt_renderer_assemble(rt_renderer* r, const float* d_gathered, float* d_image, void* hip_stream);

/* ------------------------------------------------------------------ */
/* Progressive refinement (not in the reference's path tracer; what its  */
/* viewer, openglApp.cpp, would need of one): a frame that can be shown  */
/* after a few samples and improved while the camera rests.            */
/* ------------------------------------------------------------------ */
/* Adds samples [done, done + n_samples) of every pixel to the renderer's accumulation and writes the frame for done + n_samples
 * samples.  After ANY sequence of calls the framebuffer has the bits of ONE render at samples_per_pixel = done: the RNG stream is a
 * function of (seed, pixel, sample index) and the per-pixel sums continue in sample order.  Blocking / on a caller's stream with an
 * optional shard buffer, like render / render_async (calls on different streams are the caller's to order).  A step larger than one
 * pass (rt_renderer_refine_info out[1]) is cut into passes as Render() cuts a frame; cfg.samples_per_pixel sizes those passes and is
 * Render()'s count only — refinement may go past it, up to 2^31 samples.  The accumulation (16 B per local pixel, allocated at the
 * first call) is separate from Render()'s buffers: a Render() between two steps disturbs neither.  RT_ERR_INVALID: n_samples == 0,
 * done + n_samples > 2^31, or a renderer on the baseline kernel (variant 1), which has no sample buffer.  The state is discarded by
 * rt_renderer_refine_reset and by rt_renderer_set_camera with a different camera.                                                    */
int rt_renderer_refine(rt_renderer* r, uint32_t n_samples);
int rt_renderer_refine_async(rt_renderer* r, void* hip_stream, float* d_out, uint32_t n_samples);
int rt_renderer_refine_reset(rt_renderer* r);
/* out[0] = samples accumulated, out[1] = samples per pixel one internal pass can take, out[2] = bytes held for refinement */
int rt_renderer_refine_info(rt_renderer* r, uint64_t out[3]);
/* per-pixel accumulation, row-major like download: (sum R, sum G, sum B, sum Y^2), UNscaled; world_size == 1 only.  The sums are
 * fp32, in sample order; Y = (0.2126f*R + 0.7152f*G) + 0.0722f*B of each SAMPLE, every operation rounded on its own.              */
int rt_renderer_refine_download_sums(rt_renderer* r, float* host, size_t n_floats);
/* relative RMS standard error of the frame's mean luminance after the samples so far (needs >= 2): per pixel, fp32, every operation
 * rounded on its own, n = (float)done:  m = ((0.2126f*Sr + 0.7152f*Sg) + 0.0722f*Sb) / n,  v = max(0, Q / n - m*m) / (float)(done - 1);
 * the figure is sqrt(mean(v)) / mean(m), both means in fp64 over the pixels of the image (a shard: its own pixels, padding left out),
 * reduced in a fixed order, so it repeats bit for bit.  A frame whose mean luminance is 0 gives +inf.  A pixel whose m or v is not
 * finite (the reference's arithmetic yields a NaN sample about once per 6e8) is left out of both means.                             */
int rt_renderer_refine_noise(rt_renderer* r, double* out);

/* ------------------------------------------------------------------ */
/* Feature buffers and denoiser (not in the reference): what a refined   */
/* frame looks AT — first-hit normal, depth, albedo — and an edge-aware */
/* filter guided by them, so that a frame of 8 to 32 samples can be shown. */
/* ------------------------------------------------------------------ */
/* Turns the feature buffers on: from now on every refine pass is followed by a feature pass over the pass's OWN primary rays (jitter,
 * lens point and shutter time included), one bounce through the world's own traversal.  Per local pixel two float4 (32 B, allocated
 * here): (sum Nx, sum Ny, sum Nz, sum t) and (sum Ar, sum Ag, sum Ab, hits).  A hit adds the trace's normal, its distance (in units of
 * the ray direction's length, as the reference's records hold it), the first-hit albedo and 1; a miss adds albedo (1,1,1) only.
 * Albedo: Lambertian and metal: the material's; checker: the texture value at the hit point; dielectric and diffuse light: (1,1,1).
 * The sums are fp32, IN SAMPLE ORDER per pixel: after any sequence of refine steps they have the bits of one step of the same total.
 * max_samples == 0: every refined sample is covered; otherwise samples with index >= max_samples skip the feature pass.  The colour
 * path is untouched: frame and colour sums have the same bits with the buffers on or off.  Discards the refinement state, like
 * rt_renderer_refine_reset; afterwards the buffers share its lifecycle (reset, set_camera with other bytes: discarded; set_camera with
 * the same bytes, a Render() between steps: kept).  A sharded renderer accumulates its shard.  RT_ERR_INVALID: a renderer on the
 * baseline kernel (variant 1); a world with a constant medium (its first "hit" draws from the RNG), a noise or an image texture
 * (rt_renderer_aov_enable_mode with RT_AOV_TEXTURED takes the last two, with RT_AOV_FULL all three).                                    */
int rt_renderer_aov_enable(rt_renderer* r, uint32_t max_samples);
/* The same with a mode.  RT_AOV_PLAIN is rt_renderer_aov_enable, refusals and messages included.  RT_AOV_TEXTURED also covers the two textured Lambertians; every
 * other material, the normal, the distance and the hit count are as above:
 *   RT_MAT_LAMBERTIAN_NOISE: the marble at the hit point — rt_noise_value_batch's rule with the material's albedo and param;
 *   RT_MAT_LAMBERTIAN_IMAGE: the texel the colour path shades that hit with: (u, v) of the hit — the sphere map of the outward normal, the planar coordinates on a
 *   parallelogram, rt_tri_uvs' rule on a triangle while the renderer has texture coordinates (the planar coordinates otherwise) — looked up in the material's entry
 *   (albedo2[0]) of the renderer's texture table, or, without a table, in the world's image.
 * Tables given or taken away later (rt_renderer_textures, _texture_coords, _shading_normals) are followed: they restart the refinement anyway.  A launch whose
 * materials name an entry the renderer does not have is refused before any kernel runs, as without features.  Enabling in either mode restarts the refinement;
 * switching the mode is an enable.  RT_ERR_INVALID: variant 1; a constant medium (the message names RT_MAT_ISOTROPIC); an unknown mode.
 * RT_AOV_FULL is RT_AOV_TEXTURED on every world that mode takes, bit for bit, and also follows alpha cutouts and constant media: per sample, in
 * sample order, the feature trace IS the colour path's first trace.
 *   Cutouts (lists and stack-walked BVHs, the walks a table is accepted on): a parallelogram or triangle that passes its test, on a material whose rt_cutout
 *   record is on, is put to the rule of rt_scene_set_cutout at its own (u, v) — rt_tri_uvs' rule while the renderer has texture coordinates, the planar coordinates
 *   otherwise; a candidate turned down leaves the closest hit as it was and the walk goes on as after a failed test.  rt_renderer_cutouts accepts and removes a
 *   table while buffers of this mode are on, and restarts colour and features together.
 *   Media: the trace draws from the sample's own RNG, continued from where the camera's draws left it, so a medium's free path is the one the colour path drew,
 *   in traversal order.  A first hit inside a medium adds the normal as the trace returns it, (1, 0, 0) — a constant, so that pixels deep in fog agree in the
 *   filter's normal weight —, its distance, 1, and the isotropic material's albedo.
 *   Vertex normals and normal maps apply as in RT_AOV_TEXTURED; a miss adds albedo (1, 1, 1) only.
 * RT_ERR_INVALID in mode RT_AOV_FULL: variant 1; an unknown mode.  At a launch: a cutout, normal-map or image record that names an entry the texture table lacks. */
#define RT_AOV_PLAIN    0u
#define RT_AOV_TEXTURED 1u
#define RT_AOV_FULL     2u
int rt_renderer_aov_enable_mode(rt_renderer* r, uint32_t max_samples, uint32_t mode);
/* *out_mode = the mode of the last successful enable; RT_AOV_PLAIN before any */
int rt_renderer_aov_mode(rt_renderer* r, uint32_t* out_mode);
/* out[0] = 1 when enabled, out[1] = samples per pixel the buffers cover, out[2] = bytes held */
int rt_renderer_aov_info(rt_renderer* r, uint64_t out[3]);
/* width*height*8 floats, row-major like download, the two float4 of a pixel back to back, UNscaled; world_size == 1 only */
int rt_renderer_aov_download(rt_renderer* r, float* host, size_t n_floats);

/* A variance-guided a-trous wavelet filter of the refined frame.  With n colour samples and na feature samples per pixel:
 *   c = mean colour (as the frame takes it), A = max(sum A / na, 1e-3), N = sum N / na, Z = sum t / na,
 *   I = c / A per channel (demodulate = 1) or c,  v = the variance of the mean luminance of rt_renderer_refine_noise, divided by
 *   max(Y(A), 1e-3)^2 when demodulating;  Y(r,g,b) = (0.2126f*r + 0.7152f*g) + 0.0722f*b.
 * Iteration i = 0 .. iterations-1, step = 1 << i, 5x5 taps h = (1/16, 1/4, 3/8, 1/4, 1/16) at distance step, row-major tap order
 * (dy, then dx, from -2 to 2), sequential fp32 sums, taps outside the image left out; the centre weighs h(0)^2; another tap
 *   w = ((h(dx)*h(dy) * wn) * wz) * wl,   wn = max(0, dot(Np, Nq)) squared five times,
 *   wz = 1 / (1 + dz*dz),  dz = |Zp - Zq| / ((sigma_depth * (float)step) * min(Zp, Zq) + 1e-6f),
 *   wl = 1 / (1 + dl*dl),  dl = |Y(Ip) - Y(Iq)| / (sigma_lum * sqrt(max(vp, 0)) + 1e-6f);
 *   I' = sum(w*Iq) / sum(w),  v' = sum(w*w*vq) / (sum(w))^2.  A tap whose I or v is not finite is left out; a centre that is not
 * finite is copied through.  Output: clamp, sqrt-gamma, alpha 1 of I * A (demodulate = 1) or of I — the framebuffer's layout and
 * conventions, in a buffer of its own: the refined frame is never overwritten.  Only fp32 + - * / sqrt and comparisons, each rounded
 * on its own: numpy float32 restates it bit for bit.  RT_ERR_INVALID: no feature buffers or fewer than 2 accumulated samples, a
 * renderer that holds a shard, iterations outside 1..8, a sigma that is not finite and > 0.                                          */
typedef struct rt_denoise_params {
    uint32_t iterations;   /* default 5 (1..8): the last step is 1 << (iterations - 1) pixels */
    float sigma_depth;     /* default 0.05: the relative depth difference per pixel of step at which wz = 1/2 */
    float sigma_lum;       /* default 4: luminance difference in standard deviations of the centre's mean, see wl */
    uint32_t demodulate;   /* default 1: filter the illumination c / A instead of the colour */
} rt_denoise_params;
int rt_denoise_params_default(rt_denoise_params* out);   /* host only */
int rt_renderer_denoise(rt_renderer* r, const rt_denoise_params* params);   /* blocking, on the renderer's own stream */
/* The same on a caller's hipStream_t, no host synchronisation.  Ordering the library takes care of, whichever streams are used: the filter
 * starts behind the last refine step and behind the previous filter (they share buffers), and the next refine step starts behind the filter
 * (it overwrites the sums the filter reads).  The caller's part: rt_renderer_refine_reset, rt_renderer_set_camera and rt_renderer_aov_enable
 * are host-side state changes and touch no buffer, so they need no ordering; the HOST calls themselves must not race (one thread at a time
 * per renderer, as everywhere in this interface); rt_renderer_denoise_download waits for the last filter.                                */
int rt_renderer_denoise_async(rt_renderer* r, void* hip_stream, const rt_denoise_params* params);
/* the denoised frame: width*height*4 floats like rt_renderer_download; waits for the last denoise call */
int rt_renderer_denoise_download(rt_renderer* r, float* host_rgba, size_t n_floats);

/* ------------------------------------------------------------------ */
/* Light sampling (not in the reference; "Ray Tracing: The Rest of Your */
/* Life"): opt-in next-event estimation for worlds lit by quad lights.  */
/* ------------------------------------------------------------------ */
/* A light is a quad of kind RT_QUAD_PARALLELOGRAM whose material is RT_MAT_DIFFUSE_LIGHT (a triangle with a light material emits when hit and is
 * not sampled, like a moving sphere light); they are taken in quad-index order, 1 <= n_l <= RT_MAX_LIGHTS, each with
 * area = sqrt(dot(n, n)), n = cross(u, v), in fp32.  With sampling on, a hit on RT_MAT_LAMBERTIAN or RT_MAT_LAMBERTIAN_CHECKER that does
 * not end the path draws, in this order: c; if c < 0.5f a light — i = min((uint32_t)(next * (float)n_l), n_l - 1) when n_l > 1 (no draw
 * otherwise), then a, then b, and d = ((Q_i + u_i * a) + v_i * b) - hit_p, not normalised; otherwise d = normal + on_unit as without
 * sampling (near_zero(d) fails the scatter).  Then, from hit_p before the 0.001 offset:  len2 = dot(d, d), len = sqrt(len2),
 * cosn = dot(normal, d) / len, sp = cosn > 0 ? cosn * 0.318309886f : 0;  per light j the library's own quad test on the ray (hit_p, d)
 * over a fresh trace's interval gives t or a miss:  pl_j = ((t * t) * len2) / ((fabs(dot(d, normal_j)) / len) * area_j) or 0;
 * pl = (sum of pl_j in index order) / (float)n_l;  pdf = 0.5f * sp + 0.5f * pl.  sp == 0 or a pdf that is not > 0 ends the path like a
 * failed scatter (what was accumulated is kept); otherwise atten = atten * (albedo * (sp / pdf)) and the ray goes on along d.  Every
 * operation is rounded on its own.  Emission is untouched (two-sided, added when a path hits a light); sphere lights emit but are not
 * sampled; every other material scatters and draws as without sampling.  Off (the default), every launch is exactly what it was.
 * Enabling or disabling takes effect from the next launch and, when it changes anything, discards the refinement and feature-buffer
 * state as rt_renderer_set_camera with other bytes does.  RT_ERR_INVALID, with the cause in rt_last_error: no quad light; more than
 * RT_MAX_LIGHTS; a renderer on variant 1, 5 or 6; a world with a queue or wide4 traversal; a world with a constant medium.            */
#define RT_MAX_LIGHTS 16
/* on: RT_LIGHT_SAMPLING_OFF (0), RT_LIGHT_SAMPLING_QUADS (1, the estimator above), RT_LIGHT_SAMPLING_ALL (2, below), RT_LIGHT_SAMPLING_MESH (4, further
 * below), RT_LIGHT_SAMPLING_TREE (16, below that), RT_LIGHT_SAMPLING_ENV (32) or RT_LIGHT_SAMPLING_ENV_TREE (48, last below); every other value — 3 too, which is
 * no mode — is refused */
int rt_renderer_light_sampling_enable(rt_renderer* r, uint32_t on);
/* out[0] = the mode (RT_LIGHT_SAMPLING_OFF / _QUADS / _ALL / _MESH / _TREE / _ENV / _ENV_TREE), out[1] = n_l of that mode's table — off: of the quad lights, as
 * ever — (0 when the world cannot be light-sampled); mode RT_LIGHT_SAMPLING_ENV: the texels of the map, W H; mode RT_LIGHT_SAMPLING_ENV_TREE: n_l of mode 16's
 * table, which may be 0                                                                                                       */
int rt_renderer_light_sampling_info(rt_renderer* r, uint32_t out[2]);
/* HOST (no GPU): the light table of a world as rt_renderer_light_sampling_enable would take it — quad index and area of light i < *out_n —
 * or RT_ERR_INVALID with the world's own reason for refusal (no quad light, more than RT_MAX_LIGHTS, traversal, constant medium).     */
int rt_world_quad_lights(const rt_world_flat* w, uint32_t out_quad[RT_MAX_LIGHTS], float out_area[RT_MAX_LIGHTS], uint32_t* out_n);

/* Sphere lights too: mode RT_LIGHT_SAMPLING_ALL of rt_renderer_light_sampling_enable (opt-in beside mode 1, which stays what it is).
 * Lights of mode 2: first the quad lights exactly as mode 1 lists them, then the sphere lights in the order of the flat world's primitives —
 * a STATIC sphere with radius > 0 whose material is RT_MAT_DIFFUSE_LIGHT, area = (12.566371f * r) * r in fp32; a moving sphere with a light
 * material is not in the table and keeps emitting when hit.  1 <= n_l <= RT_MAX_LIGHTS over both kinds together.  The draw order is mode 1's:
 * c; if c < 0.5f the index i as above; for a quad a, b as above; for a sphere (centre C, radius r) u = the library's on-unit-sphere draw (its
 * rejection loop, as many uniforms as it takes) and d = ((C + u * r)) - hit_p, not normalised; otherwise the cosine half.  Densities: len2,
 * len, cosn, sp as above; a quad light j as above; a sphere light j, with oc = C - hit_p:  h = dot(d, oc), cr = cross(oc, d),
 * disc = (r * r) * len2 - dot(cr, cr);  !(disc > 0) gives pl_j = 0, and ends the path like a failed scatter if j is the light this hit drew its point
 * from (a point lost on the silhouette to rounding; its exact weight is nearly 0);  otherwise sq = sqrt(disc), cosl = (sq / r) / len, t1 = (h - sq) / len2,
 * t2 = (h + sq) / len2, pl_j = 0, and for each of t1, t2 (in this order) that is > 0:  pl_j = pl_j + ((t * t) * len2) / (cosl * area_j) —
 * the solid-angle density of an area-uniform point, summed over both crossings of the line through the sphere.  pl, pdf, the sp == 0 /
 * !(pdf > 0) rule, the weight and the new ray are mode 1's.  Refused as mode 1 is, with two messages of its own: no light to sample; more
 * than RT_MAX_LIGHTS lights.  A switch between any two different modes discards the refinement and feature-buffer state; a switch to the
 * mode a renderer is in keeps it.                                                                                                       */
#define RT_LIGHT_SAMPLING_OFF 0
#define RT_LIGHT_SAMPLING_QUADS 1
#define RT_LIGHT_SAMPLING_ALL 2
#define RT_LIGHT_QUAD 0
#define RT_LIGHT_SPHERE 1
/* HOST (no GPU): the light table of `mode` (RT_LIGHT_SAMPLING_QUADS: what rt_world_quad_lights gives; RT_LIGHT_SAMPLING_ALL: the combined list) —
 * kind (RT_LIGHT_QUAD: index is a quad index; RT_LIGHT_SPHERE: a primitive index), index and area of light i < *out_n — or RT_ERR_INVALID with
 * the world's own reason for refusal.                                                                                                    */
int rt_world_lights(const rt_world_flat* w, uint32_t mode, uint32_t out_kind[RT_MAX_LIGHTS], uint32_t out_index[RT_MAX_LIGHTS],
                    float out_area[RT_MAX_LIGHTS], uint32_t* out_n);

/* Triangle and mesh lights too: mode RT_LIGHT_SAMPLING_MESH of rt_renderer_light_sampling_enable (opt-in beside modes 1 and 2, which stay what they are;
 * in those a triangle with a light material emits when hit and is not sampled).  Lights of mode 4: first mode 2's list in mode 2's order (quad lights, then
 * static sphere lights), then every quad of kind RT_QUAD_TRIANGLE whose material is RT_MAT_DIFFUSE_LIGHT, in quad-index order — kind RT_LIGHT_TRIANGLE,
 * index = its quad index, area = 0.5f * sqrtf(dot(n, n)), n = cross(u, v), in fp32.  1 <= n_l <= RT_MAX_LIGHTS_MESH over the three kinds together (a cap,
 * not a tuning result: the density step is linear in n_l); RT_MAX_LIGHTS keeps governing modes 1 and 2.  The draw order is mode 1's: c; if c < 0.5f the
 * index i; a quad and a sphere as in mode 2; a triangle draws a = next, b = next, then  if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }  — the test is
 * one fp32 add, a sum of exactly 1 is not folded — and d = ((Q_i + u_i * a) + v_i * b) - hit_p, not normalised; it draws no on-unit vector.  Densities:
 * quad and sphere lights as in mode 2; a triangle light j: the library's own quad test with kind RT_QUAD_TRIANGLE on the ray (hit_p, d) over a fresh
 * trace's interval gives t or a miss:  pl_j = ((t * t) * len2) / ((fabs(dot(d, normal_j)) / len) * area_j) or 0 — 0 also for a drawn point that rounding
 * put just outside its own triangle: the direction is still taken, as mode 1 does at a quad's edge.  A closed emissive mesh needs nothing of its own: a ray
 * through it crosses two table entries and both contribute, as both crossings of a sphere do.  pl, pdf, the sp == 0 / !(pdf > 0) rule, the weight and the
 * new ray are mode 1's.  Refused as mode 2 is, with two messages of its own: no light to sample; more than RT_MAX_LIGHTS_MESH lights.                  */
#define RT_LIGHT_SAMPLING_MESH 4
#define RT_LIGHT_TRIANGLE 2
#define RT_MAX_LIGHTS_MESH 64
/* HOST (no GPU): the light table of `mode` into arrays of `capacity` entries.  RT_LIGHT_SAMPLING_QUADS and RT_LIGHT_SAMPLING_ALL: exactly what rt_world_lights
 * gives, refusals included (capacity >= their n_l).  RT_LIGHT_SAMPLING_MESH: the table above (RT_LIGHT_TRIANGLE: index is a quad index).  A table larger
 * than `capacity` is RT_ERR_INVALID.                                                                                                                     */
int rt_world_light_table(const rt_world_flat* w, uint32_t mode, uint32_t capacity, uint32_t* out_kind, uint32_t* out_index, float* out_area, uint32_t* out_n);

/* A light tree and a choice by area: mode RT_LIGHT_SAMPLING_TREE of rt_renderer_light_sampling_enable (opt-in beside modes 1, 2 and 4, which
 * stay what they are).  The lights are mode 4's, 1 <= n_l <= RT_MAX_LIGHTS_TREE (a cap, not a tuning result), PERMUTED into the leaf order of a bounding-volume
 * tree built on the host:  box of a light = the box of its vertices (quad: Q, Q + u, Q + v, (Q + u) + v; triangle: the first three; sphere: C - r, C + r),
 * widened on every side by pad = RT_LIGHT_TREE_PAD * M, M = the largest absolute coordinate of the world's bounds (a sphere by pad + (RT_LIGHT_TREE_PAD_SPHERE
 * * (M * M)) / r);  centroid = (bmin + bmax) * 0.5f;  a range of one light is a leaf, any other is split on the longest axis of its centroids' bounds (ties: the
 * lowest axis), stable-sorted by that coordinate (ties keep mode 4's order) and cut at a + (b - a) / 2.  Nodes are numbered in preorder, 2 n_l - 1 of them, each
 * (min.xyz, skip) (max.xyz, leaf): skip = the first node behind the subtree, leaf = the light's position in the permuted table or 0xffffffff.  c_j = the
 * sequential fp32 sum of the areas in table order, A = c_{n_l - 1}; a light with c_j == c_{j-1} is refused.
 * Draws: c; if c < 0.5f a light: with n_l > 1, x = next * A and i = the smallest j with c_j > x (none: n_l - 1), no draw with one light; the point by mode 4's
 * rule for the kind.  Density: len2, len, cosn, sp as ever; rd = 1.0f / d per component; the walk starts at node 0 and ends at node n_nodes; a node is ENTERED
 * when tmin <= tmax * RT_LIGHT_TREE_K && tmax > 0, with ta = (min - hit_p) * rd, tb = (max - hit_p) * rd, tmin = the largest of the per-axis smaller, tmax = the
 * smallest of the per-axis larger, every selection glm's `(y < x) ? y : x` / `(x < y) ? y : x` in x, y, z order (a NaN from 0 * inf is kept or dropped by its
 * position in those; a NaN tmin or tmax enters nothing); an inner node entered goes to the next node, a leaf entered adds its term and goes to skip, a node
 * not entered goes to skip.  The term of a leaf is mode 4's pl_j without the division by area_j; pl = (the sum in walk order) / A; pdf, the weight, the
 * sp == 0 / !(pdf > 0) rule and the new ray are mode 1's.  A drawn sphere light that the walk did not credit with disc > 0 fails the scatter.
 * Refused as mode 4 is, with messages of its own: no light to sample; more than RT_MAX_LIGHTS_TREE lights; a light whose area is lost in the running sum.  */
#define RT_LIGHT_SAMPLING_TREE 16
#define RT_MAX_LIGHTS_TREE 4096
#define RT_LIGHT_TREE_PAD 0x1p-10f
#define RT_LIGHT_TREE_PAD_SPHERE 0x1p-18f
#define RT_LIGHT_TREE_K 0x1.0001p+0f
/* HOST (no GPU): the tree of mode RT_LIGHT_SAMPLING_TREE over the table rt_world_light_table(w, RT_LIGHT_SAMPLING_TREE, ...) gives (which is the permuted one):
 * 8 floats per node — min.xyz, skip (bits), max.xyz, leaf (bits) — into out_nodes, 2 n_l - 1 into *out_n_nodes, c_j of every light into out_cdf.  `capacity`
 * counts lights: out_nodes holds 8 * (2 * capacity - 1) floats, out_cdf capacity.  Refused as the table is.                                                 */
int rt_world_light_tree(const rt_world_flat* w, uint32_t capacity, float* out_nodes, uint32_t* out_n_nodes, float* out_cdf);

/* The environment map as the light: mode RT_LIGHT_SAMPLING_ENV of rt_renderer_light_sampling_enable (opt-in beside modes 1, 2, 4 and 16, which
 * stay what they are).  It samples the MAP ONLY: the world's quad, sphere and triangle lights emit when hit and are not sampled, as a sphere light in mode 1.
 * At a Lambertian or checker hit that does not end the path:  c = next;  if c < 0.5f, x1, x2, a, b = next four times, in that order, and d = the rule of
 * rt_environment_sample_batch (no on-unit vector is drawn);  otherwise d = normal + on-unit vector, with its near-zero failure.  len2, len, cosn, sp as in the
 * estimator above;  pl = the density of d (no division by a light count);  pdf = 0.5f * sp + 0.5f * pl;  sp == 0 or !(pdf > 0) ends the path as a failed
 * scatter;  otherwise atten *= albedo * (sp / pdf) and the new ray is hit_p + d * 0.001f, d.  No shadow ray: the direction is followed, and a miss collects the
 * map as ever.  Every other material draws and scatters as with sampling off.
 * The distribution is built when the mode is first enabled and again when rt_renderer_environment replaces the map while the mode is on; the densities ride in
 * the fourth lane of the renderer's texel records, the tables in one more buffer of its own.  rt_renderer_light_sampling_info gives (32, W H).
 * RT_ERR_INVALID, each with a message of its own: a world whose background is not 2; a renderer without a map; an all-black map; a renderer on variant 1, 5 or 6;
 * a world with a queue or wide4 traversal; a world with a constant medium.  While the mode is on, rt_renderer_environment refuses NULL (switch sampling off
 * first) and an all-black map (the old map stays).                                                                                                       */
#define RT_LIGHT_SAMPLING_ENV 32

/* The map and the light tree together: mode RT_LIGHT_SAMPLING_ENV_TREE = 16 | 32 of rt_renderer_light_sampling_enable (opt-in beside modes 1 to
 * 32, which stay what they are).  A hit is sampled when its material is RT_MAT_LAMBERTIAN, RT_MAT_LAMBERTIAN_CHECKER or RT_MAT_LAMBERTIAN_IMAGE (whose albedo is
 * looked up behind the direction, as ever); RT_MAT_LAMBERTIAN_NOISE and every other material draw and scatter as with sampling off.  The table is mode 16's, and
 * n_l == 0 is accepted: the mode then behaves as the map alone.  Draws at a sampled hit:  c = next;  if c < 0.5f and n_l > 0, c2 = next: c2 < 0.5f is the map,
 * otherwise the table (n_l == 0: the map, no draw);  the map: x1, x2, a, b and the rule of mode 32;  the table: mode 16's choice and point;  c >= 0.5f:
 * d = normal + on-unit vector.  Density, whichever branch drew d:  pe = the map's density of d;  pl = mode 16's walk sum / A;  pm = 0.5f * pe + 0.5f * pl
 * (n_l == 0: pm = pe, pl is not computed);  pdf = 0.5f * sp + 0.5f * pm;  sp == 0 or !(pdf > 0) ends the path as a failed scatter, as does a drawn sphere light
 * the walk did not credit;  otherwise atten *= albedo * (sp / pdf) and the new ray is hit_p + d * 0.001f, d.  No shadow ray.
 * rt_renderer_light_sampling_info gives (48, n_l); rt_renderer_kernel_light_tree and rt_renderer_kernel_env_light both say 1.
 * RT_ERR_INVALID, each with a message of its own: a world whose background is not 2; a renderer without a map; an all-black map; a renderer on variant 1, 5 or 6;
 * a world with a queue or wide4 traversal; a world with a constant medium; more than RT_MAX_LIGHTS_TREE lights; a light whose area is lost in the running sum;
 * a table that does not fit beside an LDS-resident image.  While the mode is on, rt_renderer_environment behaves as in mode 32.                            */
#define RT_LIGHT_SAMPLING_ENV_TREE 48

/* Smooth shading (see rt_tri_normals): the renderer's table of vertex normals, one record per triangle of its world — n must equal rt_world_triangles of it —
 * or NULL, 0 to turn it off.  Copied.  Takes effect at the next launch and, like a light-sampling change, discards the refinement and feature-buffer state.  The
 * table lies in global memory behind the scene image (in every light-sampling mode) and is read once per shaded hit on a triangle; with it on, the feature
 * pass's first-hit normal is the shading normal by the same function (depth and albedo unchanged).  Validated on the host: every value finite; each record all
 * zero, or three normals of non-zero length.  RT_ERR_INVALID with a message of its own: the baseline kernel (variant 1), a queue or wide4 traversal, variants
 * 5 and 6, a wrong n, a bad record.                                                                                                                      */
int rt_renderer_shading_normals(rt_renderer* r, const rt_tri_normals* table, uint32_t n);
/* out[0] = 1 while a table is on, out[1] = how many of its records are not flat */
int rt_renderer_shading_normals_info(rt_renderer* r, uint32_t out[2]);
/* Texture coordinates (see rt_tri_uvs): the renderer's table, one record per triangle of its world — n must equal rt_world_triangles of it — or NULL, 0 to turn
 * it off.  Copied; every value finite.  Takes effect at the next launch; an unchanged table is a no-op that keeps the refinement, a change discards the refinement
 * and feature-buffer state.  The table lies in global memory behind the scene image and the vertex normals (either may be on without the other) and is read once
 * per image-textured hit on a triangle.  RT_ERR_INVALID with a message of its own: the baseline kernel (variant 1), a queue or wide4 traversal, variants 5 and 6,
 * a wrong n, a value that is not finite.                                                                                                                      */
int rt_renderer_texture_coords(rt_renderer* r, const rt_tri_uvs* table, uint32_t n);
/* out[0] = 1 while a table is on, out[1] = how many of its records are not the identity */
int rt_renderer_texture_coords_info(rt_renderer* r, uint32_t out[2]);
/* The environment map (see rt_scene_set_environment) of a renderer whose world has background mode 2: width x height texels of 3 floats, u0 in [0, 1); or
 * NULL, 0, 0 to turn it off.  Validated as rt_scene_set_environment validates; copied into a device buffer of the renderer's own, one 16-byte record per texel (the
 * images the kernels launch on carry two vec4 that point to it).  Takes effect at the next launch; an unchanged map is a no-op that keeps the refinement, a change
 * discards the refinement and feature-buffer state.  RT_ERR_INVALID with a message of its own: a world whose background is not 2, a bad image, a bad u0.
 * While a background-2 renderer has no map, rt_renderer_render, the refine calls and their async forms return RT_ERR_INVALID and launch nothing.                */
int rt_renderer_environment(rt_renderer* r, uint32_t width, uint32_t height, const float* rgb, float u0);
/* out[0] = 1 while a map is on, out[1] = width, out[2] = height, out[3] = the bits of u0 */
int rt_renderer_environment_info(rt_renderer* r, uint32_t out[4]);
/* The texture table (see rt_scene_add_image) of a renderer: n entries as rt_scene_textures gives them and their texels; or NULL, 0, NULL to turn it off.  Entries
 * must sit back to back (first = the sum of the sizes before), an entry is empty (0 x 0) or has both dimensions > 0, known modes, n <= RT_MAX_IMAGES.  Copied into
 * a device buffer of the renderer's own, one 4-byte record (r, g, b, 0) per texel; the images the kernels launch on carry the entries.  With a table on, entry 0
 * stands for the world's image: every image hit is looked up through the table.  Takes effect at the next launch; an unchanged table is a no-op that keeps the
 * refinement, a change discards the refinement and feature-buffer state.  RT_ERR_INVALID with a message of its own: a bad table; the baseline kernel (variant 1),
 * the ray exchange (5) and the tolerance mode (6), which read no table.
 * rt_renderer_render, the refine calls and their async forms return RT_ERR_INVALID and launch nothing while an image material of the world names an entry the
 * renderer does not have: any index above 0 without a table, an index past the table's end, an empty entry.                                                      */
int rt_renderer_textures(rt_renderer* r, const rt_texture* records, uint32_t n, const uint8_t* texels);
/* out[0] = 1 while a table is on, out[1] = how many entries it has */
int rt_renderer_textures_info(rt_renderer* r, uint32_t out[2]);
/* Normal maps (rt_scene_normal_maps): table = one record per material of the world, or NULL, 0 for off (the default).  While a table is on, plain
 * launches and those of light-sampling mode 48 run the NMAP form of the renderer's kernel (rt_renderer_kernel_normal_map), which bends the normal of every hit on
 * a material whose record says `on`, right after the flat or smooth normal is known; the feature pass in RT_AOV_TEXTURED mode accumulates the mapped normal.
 * Takes effect at the next launch; an unchanged table is a no-op that keeps the refinement, a change discards the refinement and feature-buffer state.
 * RT_ERR_INVALID with a message of its own: a count that is not the world's number of materials; a record on a dielectric, a light or a medium, with an image
 * index past RT_MAX_IMAGES or a strength that is not finite and >= 0; the baseline kernel (variant 1), the ray exchange (5) and the tolerance mode (6); a world
 * with a queue or wide4 traversal, or a bvh_node tree; light-sampling modes 1, 2, 4, 16 and 32 (rt_renderer_light_sampling_enable refuses them in turn while a
 * table is on); the plain feature pass (rt_renderer_aov_enable refuses in turn, and names the textured mode).
 * rt_renderer_render, the refine calls and their async forms return RT_ERR_INVALID and launch nothing while a record names an entry the renderer's texture
 * table (rt_renderer_textures) does not have — entry 0 included: normal maps are read through the table only.                                               */
int rt_renderer_normal_maps(rt_renderer* r, const rt_normal_map* table, uint32_t n);
/* out[0] = 1 while a table is on, out[1] = how many of its records are on */
int rt_renderer_normal_maps_info(rt_renderer* r, uint32_t out[2]);
/* Microfacet surfaces (rt_scene_microfacets): table = one record per material of the world, or NULL, 0 for off (the default).  While a table is on,
 * plain launches and those of light-sampling mode 48 run the MFAC form of the renderer's kernel (rt_renderer_kernel_microfacet), whether or not a normal-map table
 * is on; that form reads both.  A table without a mapped record needs no texture table.  The feature pass does not read the table and is what it was.
 * Takes effect at the next launch; an unchanged table is a no-op that keeps the refinement, a change discards the refinement and feature-buffer state.
 * RT_ERR_INVALID with a message of its own: a count that is not the world's number of materials; a record on a dielectric, a light or a medium, with an unknown
 * `on`, an image index past RT_MAX_IMAGES, or a roughness or specular that is not finite and in [0, 1]; kernel variants 1, 5 and 6; a world with a queue or wide4
 * traversal, or a bvh_node tree; light-sampling modes 1, 2, 4, 16 and 32 (rt_renderer_light_sampling_enable refuses them in turn while a table is on).
 * rt_renderer_render, the refine calls and their async forms return RT_ERR_INVALID and launch nothing while a mapped record names an entry the renderer's texture
 * table (rt_renderer_textures) does not have.  Rough glass (§30): on == RT_MICROFACET_GLASS and RT_MICROFACET_GLASS_MAPPED are accepted on dielectrics alone, with a
 * specular of 0, and refused in words of their own elsewhere; the mapped kind's entry is checked at launch like the other's.                                 */
int rt_renderer_microfacets(rt_renderer* r, const rt_microfacet* table, uint32_t n);
/* out[0] = 1 while a table is on, out[1] = how many of its records are on */
int rt_renderer_microfacets_info(rt_renderer* r, uint32_t out[2]);
/* Solid glass (rt_scene_interiors): table = one record per material of the world, or NULL, 0 for off (the default).  While a table is on, plain
 * launches and those of light-sampling mode 48 run the INTR form of the renderer's kernel (rt_renderer_kernel_interior), whether or not a microfacet, normal-map
 * or texture table is on; that form reads them all.  Takes effect at the next launch; an unchanged table is a no-op that keeps the refinement, a change discards
 * the refinement and feature-buffer state.  RT_ERR_INVALID, renderer and kernel unchanged: what rt_renderer_microfacets refuses a renderer for (variants 1, 5, 6;
 * queue and wide4 walks; bvh_node trees; light-sampling modes 1, 2, 4, 16, 32, which in turn refuse a renderer with a table), a count that is not the world's
 * number of materials, a record on a material that is no dielectric, an `on` other than 0 or 1, a sigma that is not finite or is negative.                    */
int rt_renderer_interiors(rt_renderer* r, const rt_interior* table, uint32_t n);
/* out[0] = 1 while a table is on, out[1] = how many of its records are on */
int rt_renderer_interiors_info(rt_renderer* r, uint32_t out[2]);
/* Alpha cutouts (rt_scene_cutouts): table = one record per material of the world, or NULL, 0 for off (the default).  While a table is on, plain
 * launches and those of light-sampling mode 48 run the CUT form of the renderer's kernel (rt_renderer_kernel_cutout), whether or not an interior, microfacet or
 * normal-map table is on; that form reads them all.  Takes effect at the next launch; an unchanged table is a no-op that keeps the refinement, a change discards
 * it.  RT_ERR_INVALID, renderer and kernel unchanged: what rt_renderer_interiors refuses a renderer for (variants 1, 5, 6; queue and wide4 walks; bvh_node
 * trees; light-sampling modes 1, 2, 4, 16, 32, which in turn refuse a renderer with a table), a renderer without a texture table, feature buffers that are on
 * in mode RT_AOV_PLAIN or RT_AOV_TEXTURED (which in turn refuse a renderer with a table: only mode RT_AOV_FULL knows the rule), a count that is not the world's number of
 * materials, a record on a light, a medium or a material whose interior record is on, an `on` other than 0 or 1, an image index outside [0, RT_MAX_IMAGES), a
 * cutoff that is not finite or outside [0, 1].  A record that names an entry the texture table does not hold is refused at the launch, before any kernel
 * runs: the tables come and go independently.                                                                                                                */
int rt_renderer_cutouts(rt_renderer* r, const rt_cutout* table, uint32_t n);
/* out[0] = 1 while a table is on, out[1] = how many of its records are on */
int rt_renderer_cutouts_info(rt_renderer* r, uint32_t out[2]);

/* ------------------------------------------------------------------ */
/* Multi-GPU renderer — the same three entry points (Renderer.h:38-46)  */
/* over the N GPUs of one node, driven by ONE host process.            */
/* ------------------------------------------------------------------ */
/* The reference is single-GPU.  Rank i = devices[i] (NULL: 0 .. n_gpus-1) renders the 8x8 tiles t with
 * t % n_gpus == i; ONE grouped RCCL exchange over xGMI (ncclSend from every rank, ncclRecv on rank 0) gathers the shards
 * on devices[0] at frame end and a de-interleave kernel assembles the row-major frame there.  cfg->device / rank /
 * world_size are ignored.  The image has the same bits for every n_gpus.  RCCL (librccl.so.1) is bound at first use.
 * RT06_MULTI_TRANSPORT=memcpy (tests, single-GPU boxes) replaces the RCCL exchange by hipMemcpyAsync on the ranks' own
 * streams and lifts the one-rank-per-device rule (devices may repeat; NULL = i % device count), so that the N > 1 branch
 * — shard offsets, stream ordering, assembly, download — runs on ONE GPU, where RCCL refuses two ranks.                 */
typedef struct rt_multi_renderer rt_multi_renderer;
int rt_multi_renderer_create(const rt_render_config* cfg, const rt_camera* cam, const rt_world_flat* world,
                             uint32_t n_gpus, const int32_t* devices, rt_multi_renderer** out);
void rt_multi_renderer_destroy(rt_multi_renderer* m);
/* Renderer::Render: blocking; renders all shards side by side, gathers, assembles.                                      */
int rt_multi_renderer_render(rt_multi_renderer* m);
/* rt_renderer_set_camera on every rank (validated first: an invalid camera changes no rank).                            */
int rt_multi_renderer_set_camera(rt_multi_renderer* m, const rt_camera* cam);
/* rt_renderer_refine on every rank, then the usual gather + assembly: the frame of rt_multi_renderer_download is the
 * refined one.  No noise figure here (each rank's rt_renderer_refine_noise covers its own pixels only).                 */
int rt_multi_renderer_refine(rt_multi_renderer* m, uint32_t n_samples);
/* rt_renderer_light_sampling_enable on every rank (the first rank refuses what any would, before any changes).          */
int rt_multi_renderer_light_sampling_enable(rt_multi_renderer* m, uint32_t on);
/* rt_renderer_shading_normals on every rank (the first rank refuses what any would, before any changes).                 */
int rt_multi_renderer_shading_normals(rt_multi_renderer* m, const rt_tri_normals* table, uint32_t n);
/* rt_renderer_texture_coords on every rank (refused before any rank changes).                                             */
int rt_multi_renderer_texture_coords(rt_multi_renderer* m, const rt_tri_uvs* table, uint32_t n);
/* rt_renderer_environment on every rank (refused before any rank changes).                                                */
int rt_multi_renderer_environment(rt_multi_renderer* m, uint32_t width, uint32_t height, const float* rgb, float u0);
/* rt_renderer_textures on every rank (refused before any rank changes).                                                   */
int rt_multi_renderer_textures(rt_multi_renderer* m, const rt_texture* records, uint32_t n, const uint8_t* texels);
/* rt_renderer_textures_info of the ranks (they hold the same table).                                                      */
int rt_multi_renderer_textures_info(rt_multi_renderer* m, uint32_t out[2]);
/* rt_renderer_normal_maps on every rank (refused before any rank changes), and rt_renderer_normal_maps_info of the ranks.    */
int rt_multi_renderer_normal_maps(rt_multi_renderer* m, const rt_normal_map* table, uint32_t n);
int rt_multi_renderer_normal_maps_info(rt_multi_renderer* m, uint32_t out[2]);
/* rt_renderer_microfacets on every rank (refused before any rank changes), and rt_renderer_microfacets_info of the ranks.    */
int rt_multi_renderer_microfacets(rt_multi_renderer* m, const rt_microfacet* table, uint32_t n);
int rt_multi_renderer_microfacets_info(rt_multi_renderer* m, uint32_t out[2]);
/* rt_renderer_interiors on every rank (refused before any rank changes).                                                                                        */
int rt_multi_renderer_interiors(rt_multi_renderer* m, const rt_interior* table, uint32_t n);
/* rt_renderer_cutouts on every rank (refused before any rank changes), and rt_renderer_cutouts_info of the ranks.                                             */
int rt_multi_renderer_cutouts(rt_multi_renderer* m, const rt_cutout* table, uint32_t n);
int rt_multi_renderer_cutouts_info(rt_multi_renderer* m, uint32_t out[2]);
/* Renderer::DownloadRenderbuffer: width*height*4 floats from devices[0].                                                */
int rt_multi_renderer_download(rt_multi_renderer* m, float* host_rgba, size_t n_floats);
/* ms of the last render: out[0] host wall-clock of Render(), out[1] slowest rank's kernels (HIP events),
 * out[2] exchange + assembly on devices[0] (HIP events)                                                                 */
int rt_multi_renderer_times(rt_multi_renderer* m, float out_ms[3]);
int rt_multi_renderer_gpus(const rt_multi_renderer* m, uint32_t* out);
/* HOST (no GPU): the shard layout every rank uses — out = {tiles_x, n_tiles, n_local_tiles, shard_floats} — and the global
 * pixel id of every shard position of one rank (n = n_local_tiles * 64 entries, 0xffffffff for padding).                */
int rt_shard_layout(uint32_t width, uint32_t height, uint32_t world_size, uint32_t out[4]);
int rt_shard_pixel_map(uint32_t width, uint32_t height, uint32_t world_size, uint32_t rank, uint32_t* out_gid, size_t n);

/* ------------------------------------------------------------------ */
/* Device probes: run ONE hot-path function over an array of inputs on  */
/* the GPU.  Used by the parity tests (per-function golden vectors) —   */
/* the twin of google_testing/test.cpp's host-vs-device differential.   */
/* All pointers are HOST pointers; the probes copy in/out themselves.   */
/* ------------------------------------------------------------------ */
/* aabb::intersects (aabb.cuh:30-44): boxes n*6 (min,max), rays n*6 (o,d),
 * max_dist n -> hit n (0/1), dist n (only written when hit, else left 0).   */
int rt_probe_aabb(int device, size_t n, const float* boxes, const float* rays, const float* max_dist,
                  int32_t* out_hit, float* out_dist);
/* _sphere_closest_intersection (SphereHittable.cuh:15-33): rays n*6,
 * spheres n*4 (c,r) -> t n                                                   */
int rt_probe_sphere(int device, size_t n, const float* rays, const float* spheres, float* out_t);
/* Hittable::ClosestIntersection on a whole world: rays n*7 (o,d,time) ->
 * hit n, t n, prim n, normal n*3                                             */
int rt_probe_trace(int device, const rt_world_flat* world, size_t n, const float* rays,
                   int32_t* out_hit, float* out_t, int32_t* out_prim, float* out_normal);
/* Hittable::ClosestIntersection on a whole world, then the smooth-shading rule on a triangle hit: rays n*7 (o,d,time), table = n_table records (n_table ==
 * rt_world_triangles of the world, or NULL, 0) -> hit n, normal n*3 (the flat normal where the rule keeps it; 0 on a miss), interpolated n (0/1)            */
int rt_probe_shading_normal(int device, const rt_world_flat* world, const rt_tri_normals* table, uint32_t n_table, size_t n, const float* rays,
                            int32_t* out_hit, float* out_normal, uint32_t* out_interpolated);
/* Hittable::ClosestIntersection on a whole world, then the texture-coordinate rule on a triangle hit: rays n*7 (o,d,time), table = n_table records (n_table ==
 * rt_world_triangles of the world, or NULL, 0 = no table: the planar coordinates on a triangle too) -> hit n, uv n*2: (tu, tv) before the clamp on a triangle,
 * the planar (alpha, beta) on a parallelogram, 0 on a sphere or a miss                                                                                        */
int rt_probe_tri_uv(int device, const rt_world_flat* world, const rt_tri_uvs* table, uint32_t n_table, size_t n, const float* rays, int32_t* out_hit, float* out_uv);
/* rt_environment_batch on the device, one lane per direction: the map as the renderer holds it (one 16-byte record per texel)                                  */
int rt_probe_environment(int device, size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* dirs, float* out_rgb, uint32_t* out_texel);
/* rt_texture_lookup_batch on the device, one lane per lookup: the table as the renderer holds it (one 4-byte record per texel, the entries as vec4)              */
int rt_probe_texture(int device, const rt_texture* records, uint32_t n, const uint8_t* texels, const uint32_t* index, const float* u, const float* v, size_t count,
                     float* out_rgb);
/* rt_normal_map_batch on the device, one lane per case: the table as the renderer holds it (one 4-byte record per texel, the entries as vec4)                  */
int rt_probe_normal_map(int device, const rt_texture* records, uint32_t n, const uint8_t* texels, size_t count, const uint32_t* surface, const float* a,
                        const float* b, const float* tri_uv, const float* normal, const float* ray_d, const float* u, const float* v, const uint32_t* index,
                        const float* strength, float* out_normal, uint32_t* out_path);
/* rt_microfacet_batch on the device, one lane per case                                                                                                        */
int rt_probe_microfacet(int device, size_t count, const float* normal, const float* ray_d, const float* roughness, const float* f0, const uint32_t* coat,
                        const uint32_t* tape, size_t tape_len, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws);
/* rt_rough_glass_batch on the device, one lane per case                                                                                                       */
int rt_probe_rough_glass(int device, size_t count, const float* normal, const float* ray_d, const float* roughness, const float* ior, const uint32_t* tape,
                         size_t tape_len, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws);
/* rt_interior_batch and rt_expf_batch on the device, one lane per case                                                                                           */
int rt_probe_interior(int device, size_t count, const float* Ng, const float* n, const float* d, const float* t, const float* ior, const float* sigma,
                      const uint32_t* sphere, uint32_t* out_back, float* out_eta, float* out_T);
int rt_probe_expf(int device, size_t count, const float* x, float* out);
/* rt_cutout_batch on the device, one lane per case: the table as the renderer holds it (one 4-byte record per texel, the entries as vec4)                      */
int rt_probe_cutout(int device, const rt_texture* textures, uint32_t n_textures, const uint8_t* texels, size_t count, const rt_quad* quads, const rt_tri_uvs* uv,
                    const float* rays, const float* t, const rt_cutout* records, uint32_t n_records, const uint32_t* material, uint32_t* out_keep, float* out_uv,
                    float* out_value);
/* rt_noise_value_batch on the device, one lane per point: the tables in global memory, as the renderer holds them                                              */
int rt_probe_noise_value(int device, const rt_perlin* perlin, const float albedo[3], float scale, const float* points, size_t n, float* out_rgb);
/* rt_environment_sample_batch on the device, one lane per quadruple: the records and the tables as the renderer holds them in mode RT_LIGHT_SAMPLING_ENV        */
int rt_probe_environment_sample(int device, size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* uniforms, float* out_dir,
                                uint32_t* out_texel, float* out_density);
/* SphereHittable / MovingSphereHittable::ClosestIntersection (SphereHittable.cu:56-66, :91-102): sphere
 * prims[i] (material ignored, RT_PRIM_MOVING kept) against ray i (o,d,time) with rec.distance preset[i]
 * -> hit n, rec.distance n, normal n*3 (0 when not hit)                      */
int rt_probe_sphere_hit(int device, size_t n, const rt_prim* prims, const float* rays, const float* preset,
                        int32_t* out_hit, float* out_dist, float* out_normal);
/* Material::Scatter (cu_materials.cuh:52,77,115,27): per case a material,
 * in-ray n*7, hit distance n, outward normal n*3, RNG key (pixel,sample) n*2
 * -> scattered n (0/1), out ray n*7, attenuation n*3, RNG blocks consumed n  */
int rt_probe_scatter(int device, uint64_t seed, size_t n, const rt_material* mats, const float* rays,
                     const float* dist, const float* normals, const uint32_t* keys,
                     int32_t* out_scattered, float* out_rays, float* out_atten, uint32_t* out_draws);
/* camera sample_ray (cu_Cameras.cuh:27,54,87): st n*2, keys n*2 -> ray n*7, RNG blocks consumed n */
int rt_probe_camera(int device, uint64_t seed, const rt_camera* cam, size_t n, const float* st,
                    const uint32_t* keys, float* out_rays, uint32_t* out_draws);
/* the same two on caller tapes of k in [1, 2^24] (u = k * 2^-24) instead of the generator: case i draws
 * tape[offsets[2i] ..] for offsets[2i+1] uniforms; a case that wants more gets k = 2^23 + 1 and reports
 * draws > its length                                                         */
int rt_probe_scatter_tape(int device, size_t n, const rt_material* mats, const float* rays, const float* dist,
                          const float* normals, const uint32_t* tape, size_t tape_len, const uint32_t* offsets,
                          int32_t* out_scattered, float* out_rays, float* out_atten, uint32_t* out_draws);
int rt_probe_camera_tape(int device, const rt_camera* cam, size_t n, const float* st, const uint32_t* tape,
                         size_t tape_len, const uint32_t* offsets, float* out_rays, uint32_t* out_draws);
/* the lens cameras' rule (types 16 to 19 only) on the device, one lane per case: what rt_camera_rays_batch computes on the host */
int rt_probe_camera_lens(int device, const rt_camera* cam, size_t n, const float* st, const uint32_t* tape,
                         size_t tape_len, const uint32_t* offsets, float* out_rays, uint32_t* out_draws);
/* one full sample (render_kernel body for one s + sample_world,
 * Renderer.cu:139-181,198-204): keys n*2 (pixel gid, sample) -> radiance n*3 */
int rt_probe_radiance(const rt_render_config* cfg, const rt_camera* cam, const rt_world_flat* world,
                      size_t n, const uint32_t* keys, float* out_radiance);
/* google_testing/test.cpp:112-135 `_sphere_index_ker`: brute-force nearest
 * sphere index per pixel, pinhole camera, NDC = x/(w-1)*2-1 (test.cpp:118-119) */
int rt_probe_sphere_index(int device, const rt_camera* cam, uint32_t width, uint32_t height,
                          size_t n_spheres, const float* spheres, int32_t* out_index);
/* raw uniforms of the counter-based RNG: keys n*2, n_draws each -> n*n_draws */
int rt_probe_rng(int device, uint64_t seed, size_t n, const uint32_t* keys, uint32_t n_draws, float* out);
/* the deterministic fp32 log / sin / acos / atan2 of the extension materials (fn = 0..3; b is the second atan2
 * argument, ignored otherwise): out[i] = f(a[i], b[i])                                                        */
int rt_probe_math(int device, int fn, size_t n, const float* a, const float* b, float* out);

/* The device math vocabulary (csrc/rt_math.hpp: GLM's dot / cross / normalize / reflect / refract / mix / min / max /
 * compMax / compMin / clamp+sqrt / radians and glm_utils.h's near_zero / length2 / linear_interpolate; fn = 0..15 in the
 * order of tests/golden/glm_*: dot cross normalize reflect refract mix3 mix1 min3 max3 compmax compmin clamp01_sqrt
 * near_zero length2 lerp radians) and fn 16 = Ray::at + isBackfacing (ray_data.cuh:14,44-46).  in = n * nin floats,
 * out = n * nout floats in the layout of those fixtures.  Run by the GPU tests on the reference-generated vectors.   */
int rt_probe_glm(int device, int fn, size_t n, const float* in, float* out);
/* HOST probe (no GPU): the aabb helpers of the BVH builders — longest_axis, surface_area, centeroid, union, +=,
 * box_{x,y,z}_compare (aabb.cuh:19,24,46-68,78-88): boxes n*12 (a.min a.max b.min b.max) -> out n*20.              */
int rt_probe_aabb_misc(size_t n, const float* boxes, float* out);

/* Verification probes for the fast exact division of the streaming kernel (csrc/rt_fastdiv.hpp).
 * rt_probe_aabb_regular: boxes n*6, rays n*6, max_dist n -> the "regular ray" classification n, and
 * hit/dist of the 5-instruction-division box test (only meaningful where regular == 1).             */
int rt_probe_aabb_regular(int device, size_t n, const float* boxes, const float* rays, const float* max_dist,
                          int32_t* out_regular, int32_t* out_hit, float* out_dist);
/* The filtered box-pair predicates of one inner-node visit (rt_fastdiv.hpp): boxes n*12 (left min,max,
 * right min,max), rays n*6, max_dist n -> out n*8 int32: [regular, uncertain, hit_left, hit_right, swap,
 * exact hit_left, exact hit_right, exact left_dist > right_dist].                                       */
int rt_probe_boxpair_filtered(int device, size_t n, const float* boxes, const float* rays, const float* max_dist, int32_t* out);
/* The box pair of the default hot loop (rt_fastdiv.hpp, CERTIFIED FAR PLANES: exact near parameters, far parameters as products with the
 * rounded reciprocal whose `tmin <= tmax` decisions are certified, exact redo otherwise) next to aabb::intersects (aabb.cuh:26-44) on both
 * boxes: same layout as above -> out n*8 int32: [regular, could not certify, hit_left, hit_right, left_dist > right_dist,
 * exact hit_left, exact hit_right, exact left_dist > right_dist].                                                                       */
int rt_probe_boxpair_certified(int device, size_t n, const float* boxes, const float* rays, const float* max_dist, int32_t* out);
/* The same pair as the hot loop takes it since E23: a far parameter is fma(plane, RN(1/d), RN(-o * RN(1/d))), and both `tmin <= tmax` and the sign
 * of tmax are certified under a margin with a per-ray additive term (rt_fastdiv.hpp, CERTIFIED FAR PLANES, ONE FMA EACH).  Same layout, same out. */
int rt_probe_boxpair_certified_fma(int device, size_t n, const float* boxes, const float* rays, const float* max_dist, int32_t* out);
/* Exhaustive self-test: for each of n_den divisor significands starting at first_den (0 .. 2^23-1) and
 * ALL 2^23 numerator significands, compare the 5-instruction quotient with IEEE n/d bit for bit.
 * num_exp / den_exp are the unbiased exponents given to numerator and divisor.  Returns the number of
 * mismatching pairs in *mismatches and one example in example[2] (numerator, divisor bits).          */
int rt_selftest_fastdiv(int device, uint32_t first_den, uint32_t n_den, int32_t num_exp, int32_t den_exp,
                        uint64_t* mismatches, uint32_t example[2]);

/* The same sweep for the 4-instruction quotient from a two-word reciprocal (fast_div_exact4, the one the default
 * kernel uses).                                                                                             */
int rt_selftest_fastdiv4(int device, uint32_t first_den, uint32_t n_den, int32_t num_exp, int32_t den_exp,
                         uint64_t* mismatches, uint32_t example[2]);
/* Exhaustive self-test of the 3-instruction reciprocal used for RN(1/d) of rays in the fast-division class: every fp32
 * x with 2^-40 <= |x| < 2^40 (1,342,177,280 values) against the IEEE division 1.0f / x, bit for bit.            */
int rt_selftest_fastrcp(int device, uint64_t* checked, uint64_t* mismatches, uint32_t* example);

/* library / device info */
int rt_device_count(int* out);
/* out = {compute units, peak engine clock in kHz, device memory in MiB, memory clock in kHz} (hipDeviceProp_t) */
int rt_device_info(int device, uint32_t out[4]);
const char* rt_version(void);
/* sha256 (hex) over the sources, Makefile and extra flags this library was built from (csrc/Makefile: SRC_HASH): committed
 * profiler summaries are stamped with it, so a stale binary cannot pass for the profiled one.                             */
const char* rt_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* RT06_H */

// rt_device_funcs.hpp — the hot-path functions as flat, non-virtual device code.
//
// The reference dispatches Hittable::ClosestIntersection and Material::Scatter through device
// vtables (rt_engine/geometry/hittable.cuh:18, rt_engine/shaders/material.cuh:24-28) and chases
// hittables[i] -> SphereHittable{vptr,sphere*,mat*} -> Sphere (3 dependent loads per leaf).  Here
// the world is three linear arrays and every call is a switch on a tag.  Arithmetic follows the
// reference expression by expression (rt_math.hpp) so the CPU oracle and the GPU agree bit for bit.
#pragma once
#include "rt06.h"
#include "rt_internal.hpp"
#include "rt_math.hpp"
#include <type_traits>

struct DeviceWorld {
    uint32_t kind;
    int32_t root;
    uint32_t n_nodes, n_prims, n_mats;
    f3 bmin, bmax;
    const rt_bvh_node* nodes;
    const rt_prim* prims;
    const rt_material* mats;
    // extension beyond the reference: quads (primitive index >= n_prims), constant background
    const rt_quad* quads;
    uint32_t n_quads;
    uint32_t background;
    f3 background_color;
    const rt_perlin* perlin;   // RT_MAT_LAMBERTIAN_NOISE tables (global memory), or null
    const uint8_t* image;      // RT_MAT_LAMBERTIAN_IMAGE RGB8 image, or null
    uint32_t image_w, image_h;
    uint32_t traversal;        // RT_TRAVERSAL_STACK / RT_TRAVERSAL_QUEUE (BVH worlds)
    uint32_t* error_flag;      // set to 1 when the distance-sorted queue overflows its 32 entries (checked by the host, never silent)
};

// RayPayload (ray_data.cuh:33-40) with Sphere::TraceRecord (SphereHittable.cuh:38-41) unpacked
struct HitRec {
    float distance;
    f3 normal;
    int32_t prim;
    uint32_t mat;
};

// aabb::intersects, rt_engine/geometry/aabb.cuh:30-44
RT_HD bool aabb_intersects(f3 box_min, f3 box_max, const Ray& ray, float ray_max_dist, float& dist) {
    f3 bmin = (box_min - ray.o) / ray.d;
    f3 bmax = (box_max - ray.o) / ray.d;
    f3 tmp_min = glm_min(bmin, bmax);
    bmax = glm_max(bmin, bmax);
    bmin = tmp_min;
    float tmin = comp_max(bmin);
    float tmax = comp_min(bmax);
    bool hit = tmin <= tmax && tmin < ray_max_dist && tmax > 0;
    if (hit) dist = tmin;
    return hit;
}

// _sphere_closest_intersection, rt_engine/geometry/SphereHittable.cuh:15-33
// `a` = dot(ray.d, ray.d) is a property of the ray: the streaming kernel computes it once per trace (same expression, same bits)
RT_HD float sphere_closest_intersection_a(const Ray& ray, float a, f3 center, float radius);
RT_HD float sphere_closest_intersection(const Ray& ray, f3 center, float radius) {
    return sphere_closest_intersection_a(ray, dot(ray.d, ray.d), center, radius);
}
RT_HD float sphere_closest_intersection_a(const Ray& ray, float a, f3 center, float radius) {
    f3 oc = ray.o - center;
    float hb = dot(ray.d, oc);
    float c = dot(oc, oc) - radius * radius;
    float d = hb * hb - a * c;
    if (d <= 0) return RT_MISS_DIST;
    d = sqrtf(d);
    float t = (-hb - d) / a;
    if (t < 0.0f) {
        t = (-hb + d) / a;
        if (t < 0.0f) return RT_MISS_DIST;
    }
    return t;
}

// SphereHittable::ClosestIntersection (SphereHittable.cu:56-66) /
// MovingSphereHittable::ClosestIntersection (:91-102)
// constant_medium::hit of "The Next Week" (extension, not in the reference): a sphere whose material is RT_MAT_ISOTROPIC
// IS a constant medium bounded by that sphere, density = the material's param.  Reference conventions: the ray interval
// is [0, rec.distance) instead of [t_min, t_max], a tangent ray misses (SphereHittable.cuh:22).  ONE uniform is drawn
// per test that finds a non-empty interval inside the boundary, in traversal order.  Returns the hit distance or
// RT_MISS_DIST.
RT_HD float medium_sphere_intersection(const Ray& ray, f3 center, float radius, float density, float max_dist, Rng& rng) {
    f3 oc = ray.o - center;
    float a = dot(ray.d, ray.d);
    float hb = dot(ray.d, oc);
    float c = dot(oc, oc) - radius * radius;
    float d = hb * hb - a * c;
    if (d <= 0) return RT_MISS_DIST;
    d = sqrtf(d);
    float t1 = (-hb - d) / a, t2 = (-hb + d) / a;
    float t_in = t1 < 0.0f ? 0.0f : t1;
    float t_out = t2 > max_dist ? max_dist : t2;
    if (!(t_in < t_out)) return RT_MISS_DIST;
    float ray_length = sqrtf(a);
    float distance_inside = (t_out - t_in) * ray_length;
    float hit_distance = (-1.0f / density) * rt_logf(rng.next());
    if (hit_distance > distance_inside) return RT_MISS_DIST;
    return t_in + hit_distance / ray_length;
}

RT_HD bool prim_closest_intersection(const rt_prim& p, int32_t idx, const Ray& ray, HitRec& rec, const rt_material* mats, Rng* rng) {
    f3 center = mk3(p.c0[0], p.c0[1], p.c0[2]);
    if (p.mat & RT_PRIM_MOVING) center = mix(center, mk3(p.c1[0], p.c1[1], p.c1[2]), ray.time);
    const rt_material& pm = mats[p.mat & ~RT_PRIM_MOVING];
    if (pm.type == RT_MAT_ISOTROPIC) {
        float tm = medium_sphere_intersection(ray, center, p.radius, pm.param, rec.distance, *rng);
        if (tm >= rec.distance) return false;
        rec.mat = p.mat & ~RT_PRIM_MOVING;
        rec.distance = tm;
        rec.prim = idx;
        rec.normal = mk3(1.0f, 0.0f, 0.0f);  // arbitrary, as in the book: an isotropic scatter ignores it
        return true;
    }
    float t = sphere_closest_intersection(ray, center, p.radius);
    if (t >= rec.distance) return false;
    rec.mat = p.mat & ~RT_PRIM_MOVING;
    rec.distance = t;
    rec.prim = idx;
    rec.normal = (ray_at(ray, rec.distance) - center) / p.radius;
    return true;
}

// quad::hit of "Ray Tracing: The Next Week" in the reference's conventions: t >= 0 accepted (no t_min: the origin is
// offset instead, Renderer.cu:175), `t >= rec.distance` rejects; the stored normal faces AGAINST the ray (two-sided).
// kind (rt_quad::kind): RT_QUAD_TRIANGLE is the book's `tri` — the same plane and coordinates, and alpha + beta > 1 rejects too (one fp32 add, rounded
// on its own; a sum of exactly 1 is inside).
RT_HD bool quad_closest_intersection(f3 Q, float D, f3 u, f3 v, f3 n, f3 w, uint32_t mat, int32_t unified, uint32_t kind, const Ray& ray, HitRec& rec) {
    float denom = dot(n, ray.d);
    if (fabsf(denom) < 1e-8f) return false;
    float t = (D - dot(n, ray.o)) / denom;
    if (t < 0.0f) return false;
    if (t >= rec.distance) return false;
    f3 planar = ray_at(ray, t) - Q;
    float alpha = dot(w, cross(planar, v));
    float beta = dot(w, cross(u, planar));
    if (!(alpha >= 0.0f && alpha <= 1.0f && beta >= 0.0f && beta <= 1.0f)) return false;
    if (kind == RT_QUAD_TRIANGLE && !(alpha + beta <= 1.0f)) return false;
    rec.mat = mat;
    rec.distance = t;
    rec.prim = unified;
    rec.normal = (dot(ray.d, n) > 0) ? -n : n;
    return true;
}

// Smooth shading (rt06.h: rt_tri_normals): the shading normal at hit_p on the triangle (Q, u, v, w) with the vertex normals n0, n1, n2, given
// the flat normal `normal` that already faces against the ray.  image_value_quad's planar coordinates, the interpolated normal g, and two ways back to the flat
// one: g has no direction (an all-zero record, cancellation, a NaN), or the interpolated normal does not face the ray — every hit keeps the invariant "the
// normal faces against the ray".  Returns whether `normal` was replaced.  Only + - * / sqrt and comparisons, each rounded on its own: the streaming kernels,
// the feature pass, the probe and rt_shading_normal_batch call this one function, and numpy float32 restates it bit for bit.
RT_HD bool shading_normal(f3 Q, f3 u, f3 v, f3 w, f3 n0, f3 n1, f3 n2, f3 ray_d, f3 hit_p, f3& normal) {
    f3 planar = hit_p - Q;
    float alpha = dot(w, cross(planar, v));
    float beta = dot(w, cross(u, planar));
    const f3 g = (n0 * ((1.0f - alpha) - beta) + n1 * alpha) + n2 * beta;
    const float l2 = dot(g, g);
    if (!(l2 > 0.0f)) return false;
    f3 s = g / sqrtf(l2);
    if (dot(s, normal) < 0.0f) s = -s;
    if (!(dot(ray_d, s) < 0.0f)) return false;
    normal = s;
    return true;
}
// the same on a hit of a world walk: rec.prim is the unified index of a triangle whose record in the table is vn (the caller has found it)
RT_HD bool shading_normal_flat(const rt_quad& q, const rt_tri_normals& vn, const Ray& ray, float t, f3& normal) {
    return shading_normal(ld3(q.Q), ld3(q.u), ld3(q.v), ld3(q.w), ld3(vn.n0), ld3(vn.n1), ld3(vn.n2), ray.d, ray_at(ray, t), normal);
}

// Declining a candidate: a walk may be given a Keep, asked about every parallelogram or triangle that has just passed its test — keep(q, idx,
// ray, t) with the record, its unified index and the candidate's distance.  One that is turned down leaves `rec` as it was before the test and counts as a failed
// test.  KeepAll, the default, is never asked: every caller but the feature pass's third mode compiles to the code it had.
struct KeepAll {};
template <class Keep = KeepAll>
__device__ inline bool any_prim_closest_intersection(const DeviceWorld& w, int32_t idx, const Ray& ray, HitRec& rec, Rng* rng, Keep keep = Keep()) {
    if ((uint32_t)idx >= w.n_prims) {
        const rt_quad& q = w.quads[(uint32_t)idx - w.n_prims];
        if constexpr (!std::is_same<Keep, KeepAll>::value) {
            const HitRec before = rec;
            if (!quad_closest_intersection(mk3(q.Q[0], q.Q[1], q.Q[2]), q.D, mk3(q.u[0], q.u[1], q.u[2]), mk3(q.v[0], q.v[1], q.v[2]),
                                           mk3(q.normal[0], q.normal[1], q.normal[2]), mk3(q.w[0], q.w[1], q.w[2]), q.mat, idx, q.kind, ray, rec)) return false;
            if (keep(q, idx, ray, rec.distance)) return true;
            rec = before;
            return false;
        } else
        return quad_closest_intersection(mk3(q.Q[0], q.Q[1], q.Q[2]), q.D, mk3(q.u[0], q.u[1], q.u[2]), mk3(q.v[0], q.v[1], q.v[2]),
                                         mk3(q.normal[0], q.normal[1], q.normal[2]), mk3(q.w[0], q.w[1], q.w[2]), q.mat, idx, q.kind, ray, rec);
    }
    return prim_closest_intersection(w.prims[idx], idx, ray, rec, w.mats, rng);
}

RT_HD bool node_box(const rt_bvh_node& n, const Ray& ray, float maxd, float& dist) {
    return aabb_intersects(mk3(n.min[0], n.min[1], n.min[2]), mk3(n.max[0], n.max[1], n.max[2]), ray, maxd, dist);
}

// Where a traversal keeps its RT_MAX_STACK entries.  OwnStack, the default: the local array `T stack[RT_MAX_STACK]` the traversals always
// declared — `Local` IS that array type, so every caller but the feature pass compiles to the code it had.  LaneStack: entry i of a lane at
// base[i * STRIDE], `base` being the lane's own column of a workgroup's LDS array (rt_aov_kernel.hpp): consecutive lanes, consecutive banks.
// Both are indexed alike, which is all the traversals below ask of `stack`.
template <class T>
struct OwnStack {
    typedef T Local[RT_MAX_STACK];
    __device__ static __forceinline__ void bind(Local&, OwnStack) {}
};
template <class T, int STRIDE>
struct LaneStack {
    typedef LaneStack Local;
    T* base;
    __device__ static __forceinline__ void bind(Local& l, LaneStack given) { l = given; }
    __device__ __forceinline__ T& operator[](int i) { return base[i * STRIDE]; }
};

// BVH::ClosestIntersection, rt_engine/geometry/BVH.cu:54-106 (the live, non-priority-queue branch):
// root box first; pop; leaf -> primitive; inner -> test BOTH child boxes, order near-first, push far
// then near iff dist < rec.distance; no re-check at pop.
template <class S = OwnStack<int32_t>, class Keep = KeepAll>
__device__ inline bool bvh_closest_intersection(const DeviceWorld& w, const Ray& ray, HitRec& rec, Rng* rng, S given = S(), Keep keep = Keep()) {
    typename S::Local stack;
    S::bind(stack, given);
    int head = 0;
    float root_dist;
    if (!node_box(w.nodes[w.root], ray, rec.distance, root_dist)) return false;
    stack[head++] = w.root;
    bool hit_any = false;
    while (head != 0) {
        int32_t idx = stack[--head];
        const rt_bvh_node& node = w.nodes[idx];
        int32_t left_idx = node.left, right_idx = node.right;
        if (left_idx == -1) {
            hit_any |= any_prim_closest_intersection(w, right_idx, ray, rec, rng, keep);
            continue;
        }
        float left_dist = RT_MISS_DIST, right_dist = RT_MISS_DIST;
        node_box(w.nodes[left_idx], ray, rec.distance, left_dist);
        node_box(w.nodes[right_idx], ray, rec.distance, right_dist);
        if (left_dist > right_dist) {
            int32_t ti = left_idx; left_idx = right_idx; right_idx = ti;
            float tf = left_dist; left_dist = right_dist; right_dist = tf;
        }
        if (right_dist < rec.distance) stack[head++] = right_idx;
        if (left_dist < rec.distance) stack[head++] = left_idx;
    }
    return hit_any;
}

// BVH::ClosestIntersection with the reference's disabled distance-sorted queue (BVH.cu:17-49 and the `#if _USE_PRIO_QUEUE`
// branch :80-86): each hit child box is enqueued with its entry distance, the queue stays sorted with the nearest entry on
// top, the nearest entry of the whole frontier is dequeued next.  The reference's enqueue writes `distances[head]` AFTER
// `head++` (:37-39: index and distance end up in different slots); fixed here and in the oracle — same slot, then the
// insertion sort as written.  Capacity _PRIO_QUEUE_ELEM_COUNT = 32, checked (the reference does not): overflow raises
// *w.error_flag and ends the walk.  Probes, baseline kernel and the streaming kernel's RT_WORLD_BVH_QUEUE mode (see RT_TRAVERSAL_QUEUE in rt06.h).
template <class SI = OwnStack<int32_t>, class SD = OwnStack<float>>
__device__ inline bool bvh_closest_intersection_queue(const DeviceWorld& w, const Ray& ray, HitRec& rec, Rng* rng, SI given_i = SI(), SD given_d = SD()) {
    typename SI::Local indices;
    typename SD::Local distances;
    SI::bind(indices, given_i);
    SD::bind(distances, given_d);
    int head = 0;
    float root_dist;
    if (!node_box(w.nodes[w.root], ray, rec.distance, root_dist)) return false;
    bool hit_any = false;
    auto enqueue = [&](int32_t idx, float dist) -> bool {
        if (head >= RT_MAX_STACK) { *w.error_flag = 1u; return false; }
        indices[head] = idx; distances[head] = dist; head++;
        for (int i = head - 1; i >= 1; i--) {
            if (distances[i] > distances[i - 1]) {
                float td = distances[i]; distances[i] = distances[i - 1]; distances[i - 1] = td;
                int32_t ti = indices[i]; indices[i] = indices[i - 1]; indices[i - 1] = ti;
            } else break;
        }
        return true;
    };
    enqueue(w.root, root_dist);
    while (head != 0) {
        const int32_t idx = indices[--head];
        const rt_bvh_node& node = w.nodes[idx];
        if (node.left == -1) {
            hit_any |= any_prim_closest_intersection(w, node.right, ray, rec, rng);
            continue;
        }
        float left_dist = RT_MISS_DIST, right_dist = RT_MISS_DIST;
        if (node_box(w.nodes[node.left], ray, rec.distance, left_dist) && !enqueue(node.left, left_dist)) return hit_any;
        if (node_box(w.nodes[node.right], ray, rec.distance, right_dist) && !enqueue(node.right, right_dist)) return hit_any;
    }
    return hit_any;
}

// A 4-wide walk of the same binary tree (RT_TRAVERSAL_WIDE4; SURVEY §8f rank 4 — the reference has binary nodes only, BVH.cuh:16-25): a visit
// looks two levels down — the children of the node's children, a leaf child standing for itself: up to four boxes —, tests each against
// rec.distance (BVH.cu:87-88), orders them nearest first (stable, a missed box keeps _MISS_DIST) and pushes them far-to-near iff
// dist < rec.distance (BVH.cu:95-96).  The oracle's bvh_closest_intersection_wide4, statement by statement.  Overflow of the 32 entries
// raises *w.error_flag and ends the walk (at most 3 * ceil(depth / 2) + 1 entries are ever needed).
template <class S = OwnStack<int32_t>>
__device__ inline bool bvh_closest_intersection_wide4(const DeviceWorld& w, const Ray& ray, HitRec& rec, Rng* rng, S given = S()) {
    typename S::Local stack;
    S::bind(stack, given);
    int head = 0;
    float root_dist;
    if (!node_box(w.nodes[w.root], ray, rec.distance, root_dist)) return false;
    stack[head++] = w.root;
    bool hit_any = false;
    while (head != 0) {
        const int32_t idx = stack[--head];
        const rt_bvh_node& node = w.nodes[idx];
        if (node.left == -1) {
            hit_any |= any_prim_closest_intersection(w, node.right, ray, rec, rng);
            continue;
        }
        int32_t cand[4];
        float dist[4];
        int n = 0;
        const int32_t kids[2] = {node.left, node.right};
        for (int k = 0; k < 2; k++) {
            const rt_bvh_node& c = w.nodes[kids[k]];
            if (c.left == -1) cand[n++] = kids[k];
            else { cand[n++] = c.left; cand[n++] = c.right; }
        }
        for (int i = 0; i < n; i++) {
            dist[i] = RT_MISS_DIST;
            node_box(w.nodes[cand[i]], ray, rec.distance, dist[i]);
        }
        for (int i = 1; i < n; i++)
            for (int j = i; j >= 1 && dist[j - 1] > dist[j]; j--) {
                const float td = dist[j]; dist[j] = dist[j - 1]; dist[j - 1] = td;
                const int32_t ti = cand[j]; cand[j] = cand[j - 1]; cand[j - 1] = ti;
            }
        if (head + n > RT_MAX_STACK) { *w.error_flag = 1u; return hit_any; }
        for (int i = n - 1; i >= 0; i--)
            if (dist[i] < rec.distance) stack[head++] = cand[i];
    }
    return hit_any;
}

// HittableList::ClosestIntersection, rt_engine/geometry/HittableList.cuh:21-34
template <class Keep = KeepAll>
__device__ inline bool list_closest_intersection(const DeviceWorld& w, const Ray& ray, HitRec& rec, Rng* rng, Keep keep = Keep()) {
    float d;
    if (!aabb_intersects(w.bmin, w.bmax, ray, rec.distance, d)) return false;
    bool hit_any = false;
    for (uint32_t i = 0; i < w.n_prims + w.n_quads; i++)
        if (any_prim_closest_intersection(w, (int32_t)i, ray, rec, rng, keep)) hit_any = true;
    return hit_any;
}

// bvh_node::ClosestIntersection, rt_engine/geometry/bvh_node.cuh:19-24, made iterative: the recursion
// "own box, then left subtree, then right subtree" is a pre-order walk, i.e. pop / test / push right /
// push left with the box test at visit time against the current rec.distance.
template <class S = OwnStack<int32_t>>
__device__ inline bool tree_closest_intersection(const DeviceWorld& w, const Ray& ray, HitRec& rec, Rng* rng, S given = S()) {
    typename S::Local stack;
    S::bind(stack, given);
    int head = 0;
    stack[head++] = w.root;
    bool hit_any = false;
    while (head != 0) {
        int32_t ref = stack[--head];
        if (ref < 0) {
            int32_t pi = -ref - 1;
            hit_any |= prim_closest_intersection(w.prims[pi], pi, ray, rec, w.mats, rng);
            continue;
        }
        const rt_bvh_node& n = w.nodes[ref];
        float d;
        if (!node_box(n, ray, rec.distance, d)) continue;
        stack[head++] = n.right;
        stack[head++] = n.left;
    }
    return hit_any;
}

// rng: drawn from by constant media only (one uniform per test that enters the boundary)
__device__ inline bool world_closest_intersection(const DeviceWorld& w, const Ray& ray, HitRec& rec, Rng* rng) {
    if (w.kind == RT_WORLD_BVH)
        return w.traversal == RT_TRAVERSAL_QUEUE ? bvh_closest_intersection_queue(w, ray, rec, rng)
             : w.traversal == RT_TRAVERSAL_WIDE4 ? bvh_closest_intersection_wide4(w, ray, rec, rng) : bvh_closest_intersection(w, ray, rec, rng);
    if (w.kind == RT_WORLD_LIST) return list_closest_intersection(w, ray, rec, rng);
    return tree_closest_intersection(w, ray, rec, rng);
}

// reflectance, rt_engine/shaders/cu_materials.cuh:99-104.  powf(1-cos,5) is evaluated as
// x2=x*x; x4=x2*x2; x5=x4*x on BOTH sides of the parity check: libm, OCML and CUDA powf differ in
// the last ulp, and that ulp decides `reflect_prob > rng.next()`.
RT_HD float reflectance(float cos_theta, float ior_ratio) {
    float r0 = (1 - ior_ratio) / (1 + ior_ratio);
    r0 = r0 * r0;
    float x = 1 - cos_theta;
    float x2 = x * x;
    float x4 = x2 * x2;
    float x5 = x4 * x;
    return r0 + (1 - r0) * x5;
}

// checker_texture::value, rt_engine/shaders/cu_Textures.cuh:31-39 (ivec3 truncates toward zero)
RT_HD f3 checker_value(f3 even, f3 odd, float inv_scale, f3 pos) {
    f3 sp = pos * inv_scale;
    int ix = (int)sp.x, iy = (int)sp.y, iz = (int)sp.z;
    int sum = 0;
    sum += ix; sum += iy; sum += iz;
    bool is_even = (sum % 2 == 0);
    return mk3(is_even ? even.x : odd.x, is_even ? even.y : odd.y, is_even ? even.z : odd.z);
}

// perlin::noise / perlin_interp / turb and noise_texture::value of "The Next Week" (extension, not in the reference), fp32
// in one fixed evaluation order; the sine is rt_sinf.
RT_HD float perlin_noise(const rt_perlin* t, f3 p) {
    float fx = floorf(p.x), fy = floorf(p.y), fz = floorf(p.z);
    float u = p.x - fx, v = p.y - fy, w = p.z - fz;
    int i = (int)fx, j = (int)fy, k = (int)fz;
    float uu = (u * u) * (3.0f - 2.0f * u), vv = (v * v) * (3.0f - 2.0f * v), ww = (w * w) * (3.0f - 2.0f * w);
    float accum = 0.0f;
    for (int di = 0; di < 2; di++)
        for (int dj = 0; dj < 2; dj++)
            for (int dk = 0; dk < 2; dk++) {
                int idx = t->perm[0][(i + di) & 255] ^ t->perm[1][(j + dj) & 255] ^ t->perm[2][(k + dk) & 255];
                const float* c = t->randvec[idx];
                float wx = u - (float)di, wy = v - (float)dj, wz = w - (float)dk;
                float d = c[0] * wx + c[1] * wy + c[2] * wz;
                float wi = di ? uu : 1.0f - uu, wj = dj ? vv : 1.0f - vv, wk = dk ? ww : 1.0f - ww;
                accum += ((wi * wj) * wk) * d;
            }
    return accum;
}
RT_HD float perlin_turb(const rt_perlin* t, f3 p, int depth) {
    float accum = 0.0f, weight = 1.0f;
    for (int i = 0; i < depth; i++) {
        accum += weight * perlin_noise(t, p);
        weight *= 0.5f;
        p = p * 2.0f;
    }
    return fabsf(accum);
}
RT_HD f3 noise_value(const rt_perlin* t, f3 albedo, float scale, f3 p) {
    return albedo * (1.0f + rt_sinf(scale * p.z + 10.0f * perlin_turb(t, p, 7)));
}
// sphere::get_sphere_uv + image_texture::value of "The Next Week" (extension): n = outward unit normal of the sphere
RT_HD f3 image_texel(const uint8_t* image, uint32_t width, uint32_t height, float u, float v);
RT_HD f3 image_value(const uint8_t* image, uint32_t width, uint32_t height, f3 n) {
    float cy = -n.y;
    cy = cy < -1.0f ? -1.0f : (cy > 1.0f ? 1.0f : cy);   // the normal is unit only up to rounding
    float theta = rt_acosf(cy);
    float phi = rt_atan2f(-n.z, n.x) + 0x1.921fb6p+1f;
    return image_texel(image, width, height, phi / 0x1.921fb6p+2f, theta / 0x1.921fb6p+1f);
}
// on a quad the texture coordinates are the planar coordinates (alpha, beta) of quad::hit, recomputed from the hit point
RT_HD f3 image_value_quad(const uint8_t* image, uint32_t width, uint32_t height, f3 Q, f3 u, f3 v, f3 w, f3 hit_p) {
    f3 planar = hit_p - Q;
    float alpha = dot(w, cross(planar, v));
    float beta = dot(w, cross(u, planar));
    return image_texel(image, width, height, alpha, beta);
}
// Texture coordinates (rt06.h: rt_tri_uvs): on a triangle the planar coordinates weigh the three vertices' (u, v), t0 at Q, t1 at Q + u, t2 at
// Q + v.  Only + - *, each rounded on its own, in this association.  Under the identity record (0,0), (1,0), (0,1) the products with 0 are zeros and those with
// 1 are exact, so tu = alpha and tv = beta up to the sign of a zero: the texel is image_value_quad's.  The streaming kernels, the probe and rt_tri_uv_batch call
// this one function, and numpy float32 restates it bit for bit.
RT_HD void tri_uv(f3 Q, f3 u, f3 v, f3 w, const float t0[2], const float t1[2], const float t2[2], f3 hit_p, float& tu, float& tv) {
    f3 planar = hit_p - Q;
    float alpha = dot(w, cross(planar, v));
    float beta = dot(w, cross(u, planar));
    const float gamma = (1.0f - alpha) - beta;
    tu = (t0[0] * gamma + t1[0] * alpha) + t2[0] * beta;
    tv = (t0[1] * gamma + t1[1] * alpha) + t2[1] * beta;
}
RT_HD f3 image_value_tri(const uint8_t* image, uint32_t width, uint32_t height, f3 Q, f3 u, f3 v, f3 w, const float t0[2], const float t1[2], const float t2[2], f3 hit_p) {
    float tu, tv;
    tri_uv(Q, u, v, w, t0, t1, t2, hit_p, tu, tv);
    return image_texel(image, width, height, tu, tv);
}
// image_texture::value(u, v) of "The Next Week": clamp, flip v to image coordinates, nearest texel, 1/255
RT_HD f3 image_texel(const uint8_t* image, uint32_t width, uint32_t height, float u, float v) {
    u = u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u);
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    v = 1.0f - v;   // flip to image coordinates
    int i = (int)(u * (float)width), j = (int)(v * (float)height);
    if (i > (int)width - 1) i = (int)width - 1;
    if (j > (int)height - 1) j = (int)height - 1;
    const uint8_t* px = image + ((size_t)j * width + (size_t)i) * 3u;
    return mk3((float)px[0] * 0x1.010102p-8f, (float)px[1] * 0x1.010102p-8f, (float)px[2] * 0x1.010102p-8f);
}

// The texture table (rt06.h: rt_scene_add_image): what image `rec` = (W, H, wrap | filter << 8, first texel) of the table shows at (u, v), the
// coordinates as image_value, image_value_quad and tri_uv compute them, before any clamp.  texels = one dword r | g << 8 | b << 16 per texel, all images back to
// back, rows from the top.  Only + - * /, comparisons, float/int conversion and floor, each rounded on its own; a coordinate that is not a number wraps to 0
// (column 0, the bottom row) on host and device alike.  Under clamp and nearest the texel and its bits are image_texel's for every coordinate that is a number.
// The streaming kernels, the probe and rt_texture_lookup_batch call this one function; numpy float32 restates it bit for bit.
RT_HD void sphere_uv(f3 n, float& u, float& v) {   // image_value's coordinates
    float cy = -n.y;
    cy = cy < -1.0f ? -1.0f : (cy > 1.0f ? 1.0f : cy);
    const float theta = rt_acosf(cy);
    const float phi = rt_atan2f(-n.z, n.x) + 0x1.921fb6p+1f;
    u = phi / 0x1.921fb6p+2f; v = theta / 0x1.921fb6p+1f;
}
RT_HD void quad_uv(f3 Q, f3 u, f3 v, f3 w, f3 hit_p, float& alpha, float& beta) {   // image_value_quad's coordinates
    const f3 planar = hit_p - Q;
    alpha = dot(w, cross(planar, v));
    beta = dot(w, cross(u, planar));
}
RT_HD float texture_wrap(float x, bool repeat) {
    const float frac = x - floorf(x);   // may be exactly 1 (a tiny negative x); infinity gives NaN
    x = repeat ? frac : x;              // selects, not branches: the shade phase has no scalars to spare for another level of divergence
    return !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x);
}
RT_HD f3 texture_texel(const uint32_t* texels, uint32_t at) {
    const uint32_t t = texels[at];   // one dword load
    return mk3((float)(t & 255u) * 0x1.010102p-8f, (float)((t >> 8) & 255u) * 0x1.010102p-8f, (float)((t >> 16) & 255u) * 0x1.010102p-8f);
}
RT_HD f3 texture_lerp(f3 a, f3 b, float t) { return a + (b - a) * t; }
// the rule's three parts: wrap and flip; the nearest texel of wrapped coordinates; the bilinear blend of them
RT_HD void texture_wrap_uv(uint4 rec, float& u, float& v) {
    const bool repeat = (rec.z & 255u) == RT_WRAP_REPEAT;
    u = texture_wrap(u, repeat);
    v = texture_wrap(v, repeat);
    v = 1.0f - v;   // flip to image coordinates
}
RT_HD f3 texture_nearest(const uint32_t* texels, uint4 rec, float u, float v) {
    const int W = (int)rec.x, H = (int)rec.y;
    int i = (int)(u * (float)W), j = (int)(v * (float)H);
    if (i > W - 1) i = W - 1;
    if (j > H - 1) j = H - 1;
    return texture_texel(texels, rec.w + (uint32_t)j * rec.x + (uint32_t)i);
}
RT_HD f3 texture_bilinear(const uint32_t* texels, uint4 rec, float u, float v) {
    const int W = (int)rec.x, H = (int)rec.y;
    const bool repeat = (rec.z & 255u) == RT_WRAP_REPEAT;
    const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;   // in [-1/2, W - 1/2]: texel centres sit on the integers
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    int i0 = (int)x0, j0 = (int)y0;
    int i1 = i0 + 1, j1 = j0 + 1;
    i0 = i0 < 0 ? (repeat ? W - 1 : 0) : i0;
    i1 = i1 > W - 1 ? (repeat ? 0 : W - 1) : i1;
    j0 = j0 < 0 ? (repeat ? H - 1 : 0) : j0;
    j1 = j1 > H - 1 ? (repeat ? 0 : H - 1) : j1;
    const uint32_t r0 = rec.w + (uint32_t)j0 * rec.x, r1 = rec.w + (uint32_t)j1 * rec.x;
    const f3 top = texture_lerp(texture_texel(texels, r0 + (uint32_t)i0), texture_texel(texels, r0 + (uint32_t)i1), fx);
    const f3 bottom = texture_lerp(texture_texel(texels, r1 + (uint32_t)i0), texture_texel(texels, r1 + (uint32_t)i1), fx);
    return texture_lerp(top, bottom, fy);
}
RT_HD f3 texture_value(const uint32_t* texels, uint4 rec, float u, float v) {
    texture_wrap_uv(rec, u, v);
    if (((rec.z >> 8) & 255u) != RT_FILTER_BILINEAR) return texture_nearest(texels, rec, u, v);
    return texture_bilinear(texels, rec, u, v);
}

// Alpha cutouts (rt06.h: rt_scene_set_cutout): whether a candidate hit at parameter t of `ray` on the parallelogram or triangle (Q, u, v, w) is
// there.  `entry` = the mask's entry of the texture table, `uvs` = the triangle's six texture coordinates (an rt_tri_uvs record) or nullptr for the planar
// coordinates.  The point, the coordinates and the texel are what the shade phase computes for the same t with the same functions — ray_at, tri_uv or quad_uv,
// texture_value — so a mask and a colour image over one surface agree texel for texel.  Kept iff !(green < cutoff): a NaN keeps the hit.  Nothing is drawn.
// The leaf phase of the CUT kernels, the probe and rt_cutout_batch call this one function, and numpy float32 restates it bit for bit.
RT_HD bool cutout_keeps(const uint32_t* texels, uint4 entry, float cutoff, f3 Q, f3 u, f3 v, f3 w, const float* uvs, const Ray& ray, float t, float& tu, float& tv, f3& c) {
    const f3 hit_p = ray_at(ray, t);
    if (uvs) {
        const float t0[2] = {uvs[0], uvs[1]}, t1[2] = {uvs[2], uvs[3]}, t2[2] = {uvs[4], uvs[5]};
        tri_uv(Q, u, v, w, t0, t1, t2, hit_p, tu, tv);
    } else {
        quad_uv(Q, u, v, w, hit_p, tu, tv);
    }
    c = texture_value(texels, entry, tu, tv);
    return !(c.y < cutoff);
}

// Normal maps (rt06.h: rt_scene_set_normal_map): a tangent-space map bends the normal the shade phase has.  Two functions: the directions in
// which a triangle's texture coordinates grow, and the rule.  The tangents are unnormalised and belong to the lookup's (u, v) before the image flip: on a sphere
// (n.z, 0, -n.x) and (0, 1, 0) (sphere_uv's phi = atan2(-z, x)), on a parallelogram and on a triangle without coordinates the record's u and v, on a triangle
// with coordinates t0, t1, t2 the two below.  Only + - * / sqrt and comparisons, each rounded on its own: the probe and rt_normal_map_batch call these
// functions, and numpy float32 restates them bit for bit.
RT_HD void normal_map_sphere_tangents(f3 n, f3& dPdu, f3& dPdv) {
    dPdu = mk3(n.z, 0.0f, -n.x);
    dPdv = mk3(0.0f, 1.0f, 0.0f);
}
// false: the coordinates span no area (det == 0, or a NaN), there is no frame and the normal stays
RT_HD bool normal_map_tri_tangents(f3 u, f3 v, const float t0[2], const float t1[2], const float t2[2], f3& dPdu, f3& dPdv) {
    const float du1 = t1[0] - t0[0], dv1 = t1[1] - t0[1];
    const float du2 = t2[0] - t0[0], dv2 = t2[1] - t0[1];
    const float det = du1 * dv2 - du2 * dv1;
    if (!(det > 0.0f || det < 0.0f)) return false;
    dPdu = u * dv2 - v * dv1;
    dPdv = v * du1 - u * du2;
    if (det < 0.0f) { dPdu = -dPdu; dPdv = -dPdv; }   // mirrored coordinates
    return true;
}
// c = texture_value of the map's entry at the hit's (u, v); `normal` = the flat or smooth normal, facing as the shade phase leaves it.  Decode (byte 128 is zero,
// 127 steps are one), scale x and y, Gram-Schmidt dPdu against the normal, a bitangent on dPdv's side, and the mapped normal only if it sees the ray from the
// side the normal sees it from.  Returns the path taken (rt06.h): RT_NMAP_REPLACED, or why the normal stays.
RT_HD uint32_t normal_map_apply(f3 c, float strength, f3 dPdu, f3 dPdv, f3 ray_d, f3& normal) {
    const float C0 = 128.0f * 0x1.010102p-8f;   // texture_texel's byte 128
    const float K = 255.0f / 127.0f;
    f3 m = (c - mk3(C0)) * K;
    m.x = m.x * strength;
    m.y = m.y * strength;
    if (m.x == 0.0f && m.y == 0.0f) return RT_NMAP_FLAT;
    const f3 N = normal;
    f3 T = dPdu - N * dot(N, dPdu);
    const float tt = dot(T, T);
    if (!(tt > 0.0f)) return RT_NMAP_NO_TANGENT;   // a sphere's poles, a degenerate u
    T = T / sqrtf(tt);
    f3 B = cross(N, T);
    if (dot(B, dPdv) < 0.0f) B = -B;
    const f3 g = (T * m.x + B * m.y) + N * m.z;
    const float l2 = dot(g, g);
    if (!(l2 > 0.0f)) return RT_NMAP_NO_LENGTH;
    const f3 s = g / sqrtf(l2);
    const float ds = dot(ray_d, s), dn = dot(ray_d, N);
    if (!((ds > 0.0f && dn > 0.0f) || (ds < 0.0f && dn < 0.0f))) return RT_NMAP_FACING;
    normal = s;
    return RT_NMAP_REPLACED;
}

// Microfacet surfaces (rt06.h: rt_scene_set_microfacet): a GGX lobe, its normals drawn from the distribution of those the viewer sees.  Two
// functions: the record's roughness under its map, and the rule, numbered as rt06.h numbers it.  Only + - * / sqrt and comparisons, each rounded on its own:
// the probe and rt_microfacet_batch call these functions, and numpy float32 restates them bit for bit.
RT_HD float mfac_max(float x, float c) { return x > c ? x : c; }   // a NaN takes c
RT_HD float mfac_min(float x, float c) { return x < c ? x : c; }
// c = texture_value of the record's entry at the hit's (u, v): the green channel scales the roughness
RT_HD float microfacet_roughness(float roughness, f3 c) { return roughness * c.y; }
// Steps 2 to 7 of the rule up to the micro-normal, shared with rough glass (§30): N = the normal on the viewer's side, v = the unit direction to the viewer,
// co = dot(N, v) > 0, r = the roughness.  Returns M, a normal of the distribution v sees, and a = the clamped width the masking term takes.
template <class G>
RT_HD f3 microfacet_visible_normal(f3 N, f3 v, float co, float r, G& g, float& a_out) {
    const float a = mfac_max(r * r, 0x1p-10f);                              // 2
    const float s = N.z >= 0.0f ? 1.0f : -1.0f;                             // 3
    const float k = -1.0f / (s + N.z);
    const float b = (N.x * N.y) * k;
    const float sx = s * N.x;
    const f3 T = mk3(1.0f + (sx * N.x) * k, s * b, -sx);
    const f3 B = mk3(b, s + (N.y * N.y) * k, -N.y);
    const f3 h = normalize(mk3(a * dot(T, v), a * dot(B, v), co));          // 4
    const float l2 = h.x * h.x + h.y * h.y;                                 // 5
    const f3 T1 = l2 > 0.0f ? mk3(-h.y, h.x, 0.0f) / sqrtf(l2) : mk3(1.0f, 0.0f, 0.0f);
    const f3 T2 = cross(h, T1);
    float t1, t2;                                                           // 6
    rng_in_unit2(g, t1, t2);
    const float q = 0.5f * (1.0f + h.z);
    const float t11 = t1 * t1;
    t2 = (1.0f - q) * sqrtf(mfac_max(1.0f - t11, 0.0f)) + q * t2;
    const f3 nh = (T1 * t1 + T2 * t2) + h * sqrtf(mfac_max((1.0f - t11) - t2 * t2, 0.0f));
    const f3 m = normalize(mk3(a * nh.x, a * nh.y, mfac_max(nh.z, 0.0f)));  // 7
    a_out = a;
    return (T * m.x + B * m.y) + N * m.z;
}
// the separable Smith term of a direction whose cosine to the normal is c > 0
RT_HD float microfacet_g1(float a, float c) {
    const float c2 = c * c;
    return 2.0f / (1.0f + sqrtf(1.0f + ((a * a) * mfac_max(1.0f - c2, 0.0f)) / c2));
}
// N = the shading normal, d = the ray's direction, r = the roughness, F0 = the conductor's albedo or — coat — the scalar specular three times; G: Rng, or the
// probes' tape.  Returns the way out (rt06.h): RT_MFAC_SPECULAR with the direction and the factor of the throughput, or why there is neither.
template <class G>
RT_HD uint32_t microfacet_scatter(f3 N, f3 d, float r, f3 F0, bool coat, G& g, f3& out_dir, f3& out_weight) {
    const f3 v = (-d) / sqrtf(dot(d, d));                                   // 1
    const float co = dot(N, v);
    if (!(co > 0.0f)) return RT_MFAC_BACKSIDE;
    float a;
    const f3 M = microfacet_visible_normal(N, v, co, r, g, a);              // 2 - 7
    const float ch = dot(v, M);
    const float x = 1.0f - mfac_min(mfac_max(ch, 0.0f), 1.0f);
    const float k5 = ((x * x) * (x * x)) * x;
    const f3 F = F0 + (mk3(1.0f) - F0) * k5;                                // 8
    if (coat && !(g.next() < F.x)) return RT_MFAC_BASE;
    const f3 w = M * (2.0f * ch) - v;                                       // 9
    const float ci = dot(N, w);
    if (!(ci > 0.0f)) return RT_MFAC_ABSORBED;
    const float Gm = microfacet_g1(a, ci);
    out_dir = w;
    out_weight = coat ? mk3(Gm) : F * Gm;
    return RT_MFAC_SPECULAR;
}

// Rough glass (rt06.h: rt_scene_set_rough_glass): the dielectric whose interface is a GGX height field.  The rule is rough_glass_scatter, numbered
// as rt06.h numbers it; its steps 2 to 7 are rough_glass_faced, which takes the facing (n, eta) as the smooth dielectric's own expressions leave it, so that the
// shade phase, which has just evaluated them, hands them on and no bit depends on who did.  Out: the direction and the scalar factor of the throughput.
template <class G>
RT_HD uint32_t rough_glass_faced(f3 n, float eta, f3 d, float r, G& g, f3& out_dir, float& out_weight) {
    const f3 v = (-d) / sqrtf(dot(d, d));                                   // 2
    const float co = dot(n, v);
    if (!(co > 0.0f)) return RT_MFAC_BASE;
    float a;
    const f3 M = microfacet_visible_normal(n, v, co, r, g, a);              // 3
    const float ch = dot(v, M);
    const float F = reflectance(mfac_min(mfac_max(ch, 0.0f), 1.0f), eta);   // 4
    const float k = 1.0f - eta * eta * (1.0f - ch * ch);                    // 5
    bool mirror = !(k >= 0.0f);
    if (!mirror) mirror = F > g.next();
    if (mirror) {                                                           // 6
        const f3 w = M * (2.0f * ch) - v;
        const float ci = dot(n, w);
        if (!(ci > 0.0f)) return RT_MFAC_ABSORBED;
        out_dir = w; out_weight = microfacet_g1(a, ci);
        return RT_MFAC_SPECULAR;
    }
    const f3 w = refract(-v, M, eta);                                       // 7
    const float ci = -dot(n, w);
    if (!(ci > 0.0f)) return RT_MFAC_ABSORBED;
    out_dir = w; out_weight = microfacet_g1(a, ci);
    return RT_MFAC_TRANSMITTED;
}
template <class G>
RT_HD uint32_t rough_glass_scatter(f3 N, f3 d, float r, float ior, G& g, f3& out_dir, float& out_weight) {
    const bool back = dot(d, N) > 0;                                        // 1
    const f3 n = back ? -N : N;
    const float eta = back ? ior : 1 / ior;
    return rough_glass_faced(n, eta, d, r, g, out_dir, out_weight);
}

// Solid glass (rt06.h: rt_scene_set_interior): a dielectric whose material has an interior record knows inside from outside on every kind of
// surface, and absorbs along the segment that ended inside it.  `back` is the facing as rt06.h's step 1 states it — dot(d, Ng) > 0 on the stored normal of a
// parallelogram or triangle, the smooth dielectric's own expression on a sphere's outward normal — handed in by who has just evaluated it, so that no bit depends
// on who did.  Out: eta as the smooth dielectric writes it, and T, the factor of the albedo (ones at a front hit).
RT_HD void interior_hit(bool back, f3 d, float t, float ior, f3 sigma, float& eta, f3& T) {
    eta = back ? ior : 1 / ior;                                             // 1
    T = mk3(1.0f);
    if (back) {                                                             // 2
        const float len = sqrtf(dot(d, d));
        const float dist = t * len;
        T = mk3(rt_expf(-(sigma.x * dist)), rt_expf(-(sigma.y * dist)), rt_expf(-(sigma.z * dist)));
    }
}

// Environment maps (rt06.h: rt_scene_set_environment): what a ray that leaves the world sees.  d = the ray's direction (any length), texels =
// width x height records (r, g, b, -), row 0 at the top, u0 in [0, 1) = the rotation about y.  image_value's map and constants, the rotation added to u, then
// image_texel's rule; the clamps are written so that a NaN coordinate lands on texel 0 on host and device alike.  Only + - * / sqrt, comparisons and the two rt_
// functions, each rounded on its own.  The streaming kernels, the probe and rt_environment_batch call this one function; numpy float32 restates it bit for bit.
RT_HD uint32_t environment_texel_index(uint32_t width, uint32_t height, float u0, f3 d) {
    const f3 n = normalize(d);
    float cy = -n.y;
    cy = cy < -1.0f ? -1.0f : (cy > 1.0f ? 1.0f : cy);
    const float theta = rt_acosf(cy);
    const float phi = rt_atan2f(-n.z, n.x) + 0x1.921fb6p+1f;
    float u = phi / 0x1.921fb6p+2f + u0;
    if (u >= 1.0f) u = u - 1.0f;
    float v = theta / 0x1.921fb6p+1f;
    u = !(u > 0.0f) ? 0.0f : (u > 1.0f ? 1.0f : u);
    v = !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v);
    v = 1.0f - v;   // flip to image coordinates
    int i = (int)(u * (float)width), j = (int)(v * (float)height);
    if (i > (int)width - 1) i = (int)width - 1;
    if (j > (int)height - 1) j = (int)height - 1;
    return (uint32_t)j * width + (uint32_t)i;
}
RT_HD f3 environment_value(const float4* texels, uint32_t width, uint32_t height, float u0, f3 d) {
    const float4 t = texels[environment_texel_index(width, height, u0, d)];   // one 16-byte load
    return mk3(t.x, t.y, t.z);
}

// Environment light sampling (rt06.h: RT_LIGHT_SAMPLING_ENV): a direction drawn from the map in proportion to radiance times solid angle, and the
// density of any direction.  dist = rt_environment_distribution's tables in one array: rowc[H], rowy[H + 1], colc[H * W]; x1, x2, a, b = uniforms in (0, 1].
// Two binary searches — the smallest row whose running sum passes x1 * A, the smallest column of it whose running sum passes x2 * R_j; a product that rounds up to
// the total takes the float just below it, so a search always ends on an entry whose sum rose — then a point uniform in the texel's (u, n.y) rectangle, which is
// uniform in solid angle.  Only + - * / sqrt, comparisons and rt_sinf, each rounded on its own; d is unit up to rounding and is not renormalised.  *out_texel =
// j * W + i as drawn.  The streaming kernels' ENVL forms, the probe and rt_environment_sample_batch call these two functions; numpy float32 restates them bit for bit.
RT_HD uint32_t environment_search(const float* c, uint32_t n, float x) {   // the smallest k with c[k] > x, or n - 1
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (c[mid] > x) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}
RT_HD f3 environment_sample(const float* dist, uint32_t width, uint32_t height, float u0, float x1, float x2, float a, float b, uint32_t* out_texel) {
    const float* rowc = dist;
    const float* rowy = dist + height;
    const float* colc = dist + 2u * height + 1u;
    const float A = rowc[height - 1u];
    float x = x1 * A;
    if (!(x < A)) x = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, A) - 1u);
    const uint32_t j = environment_search(rowc, height, x);
    const float* row = colc + (size_t)j * width;
    const float R = row[width - 1u];
    x = x2 * R;
    if (!(x < R)) x = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, R) - 1u);
    const uint32_t i = environment_search(row, width, x);
    const float u = ((float)i + a) / (float)width;
    const float y1 = rowy[j + 1u];
    const float y = y1 + (rowy[j] - y1) * b;
    const float s2 = 1.0f - y * y;
    const float s = sqrtf(s2 > 0.0f ? s2 : 0.0f);
    float t = u - u0;
    if (t < 0.0f) t = t + 1.0f;
    const float psi = t * 0x1.921fb6p+2f - 0x1.921fb6p+1f;
    if (out_texel) *out_texel = j * width + i;
    return mk3(s * rt_sinf(psi + 0x1.921fb6p+0f), y, -(s * rt_sinf(psi)));
}
// texels = the renderer's records (r, g, b, density): the density of d is that of the texel §23's lookup puts it in, even where rounding put a drawn d across a border
RT_HD float environment_density(const float4* texels, uint32_t width, uint32_t height, float u0, f3 d) {
    return texels[environment_texel_index(width, height, u0, d)].w;
}

// Material::Scatter — LambertianAbstract (cu_materials.cuh:52-64), MetalAbstract (:77-95),
// DielectricAbstract (:115-143), LambertianTexture (:27-40)
// `w`: the world's Perlin tables / image for the two textured extension materials (may be null otherwise)
// G: Rng, or the probes' tape of uniforms (rt_probes.hip), for the edges the generator's stream never reaches
template <class G>
RT_HD bool material_scatter(const rt_material& m, const Ray& in_ray, const HitRec& rec, G& rng, Ray& out, f3& attenuation,
                            const DeviceWorld* w = nullptr) {
    f3 normal = rec.normal;
    if (m.type == RT_MAT_DIFFUSE_LIGHT) return false;  // diffuse_light of "The Next Week": emits, never scatters
    const f3 albedo = mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
    const f3 albedo2 = mk3(m.albedo2[0], m.albedo2[1], m.albedo2[2]);
    if (m.type == RT_MAT_LAMBERTIAN || m.type == RT_MAT_LAMBERTIAN_CHECKER || m.type == RT_MAT_LAMBERTIAN_NOISE || m.type == RT_MAT_LAMBERTIAN_IMAGE) {
        f3 ray_dir = normal + rng_on_unit3(rng);
        if (near_zero(ray_dir)) return false;
        out.o = ray_at(in_ray, rec.distance); out.d = ray_dir; out.time = in_ray.time;
        if (m.type == RT_MAT_LAMBERTIAN) attenuation = albedo;
        else if (m.type == RT_MAT_LAMBERTIAN_CHECKER) attenuation = checker_value(albedo, albedo2, m.param, ray_at(in_ray, rec.distance));
        else if (m.type == RT_MAT_LAMBERTIAN_NOISE) attenuation = noise_value(w->perlin, albedo, m.param, ray_at(in_ray, rec.distance));
        else if (rec.prim >= 0 && (uint32_t)rec.prim >= w->n_prims) {
            const rt_quad& q = w->quads[(uint32_t)rec.prim - w->n_prims];
            attenuation = image_value_quad(w->image, w->image_w, w->image_h, mk3(q.Q[0], q.Q[1], q.Q[2]), mk3(q.u[0], q.u[1], q.u[2]), mk3(q.v[0], q.v[1], q.v[2]),
                                           mk3(q.w[0], q.w[1], q.w[2]), ray_at(in_ray, rec.distance));
        } else attenuation = image_value(w->image, w->image_w, w->image_h, normal);
        return true;
    }
    if (m.type == RT_MAT_ISOTROPIC) {  // isotropic phase function of "The Next Week": a uniformly random direction, always scatters
        out.o = ray_at(in_ray, rec.distance); out.d = rng_on_unit3(rng); out.time = in_ray.time;
        attenuation = albedo;
        return true;
    }
    if (m.type == RT_MAT_METAL) {
        f3 scatter_dir = reflect(in_ray.d, normal) + rng_on_unit3(rng) * m.param;
        if (dot(scatter_dir, normal) < 0 || near_zero(scatter_dir)) return false;
        out.o = ray_at(in_ray, rec.distance); out.d = scatter_dir; out.time = in_ray.time;
        attenuation = albedo;
        return true;
    }
    float ior = m.param;
    bool hit_backface = dot(in_ray.d, normal) > 0;  // isBackfacing, ray_data.cuh:44-46
    if (hit_backface) normal = -normal;
    float ior_ratio = hit_backface ? ior : 1 / ior;
    f3 unit_dir = normalize(in_ray.d);
    float cos_theta = fminf(dot(-unit_dir, normal), 1.0f);
    float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
    float reflect_prob = reflectance(cos_theta, ior_ratio);
    f3 scatter_dir;
    if (ior_ratio * sin_theta > 1.0f || reflect_prob > rng.next()) scatter_dir = reflect(unit_dir, normal);
    else scatter_dir = refract(unit_dir, normal, ior_ratio);
    out.o = ray_at(in_ray, rec.distance); out.d = scatter_dir; out.time = in_ray.time;
    attenuation = albedo;
    return true;
}

// sample_ray — PinholeCamera (cu_Cameras.cuh:27-30), DefocusBlurCamera (:54-64), MotionBlurCamera (:87-89), in two halves:
// camera_draw consumes the camera's uniforms (defocus: the lens point InUnit<2>; motion: one uniform -> time), camera_ray
// is the arithmetic.  The streaming path runs the first half in primary_rays_kernel and the second at regeneration.
template <class G>
RT_HD void camera_draw(const rt_camera& c, G& rng, float& a, float& b) {
    a = 0.0f; b = 0.0f;
    if (c.type == RT_CAM_DEFOCUS) rng_in_unit2(rng, a, b);                // a, b = lens point in the unit disc
    else if (c.type == RT_CAM_MOTION) a = mix(c.t0, c.t1, rng.next());  // a = ray time
}
RT_HD Ray camera_ray(const rt_camera& c, float s, float t, float a, float b) {
    Ray r;
    f3 o = mk3(c.o[0], c.o[1], c.o[2]), u = mk3(c.u[0], c.u[1], c.u[2]);
    f3 v = mk3(c.v[0], c.v[1], c.v[2]), w = mk3(c.w[0], c.w[1], c.w[2]);
    if (c.type == RT_CAM_DEFOCUS) {
        f3 offset = u * a + v * b;
        offset = offset * c.lens_radius;
        f3 forward = w * c.focus_dist;
        f3 hori = u * c.viewport_width * c.focus_dist;
        f3 vert = v * c.viewport_height * c.focus_dist;
        r.o = o + offset;
        r.d = forward + hori * s + vert * t - offset;
        r.time = 0.0f;
    } else {
        r.o = o;
        r.d = w + u * s + v * t;
        r.time = a;   // 0 for a pinhole camera
    }
    return r;
}
template <class G>
RT_HD Ray camera_sample_ray(const rt_camera& c, float s, float t, G& rng) {
    float a, b;
    camera_draw(c, rng, a, b);
    return camera_ray(c, s, t, a, b);
}

// The lens cameras (rt06.h: RT_CAM_PERSPECTIVE .. RT_CAM_PANORAMA): a projection, an optional thin lens and an optional shutter on ONE record.
// u, v, w are the unit basis, (viewport_width, viewport_height) = the projection's (a, b).  Like sample_ray above in two halves: lens_camera_draw consumes the
// uniforms (the lens point InUnit<2> iff lens_radius > 0, then one uniform -> time iff t0 != t1), lens_camera_ray is the arithmetic.  Only + - * / sqrt,
// comparisons and rt_sinf, each rounded on its own; cos x = rt_sinf(x + pi/2) as environment_sample writes it.  Directions are not normalised.
// proj = type - RT_CAM_PERSPECTIVE and lens = (lens_radius > 0) are arguments so that primary_rays_lens_kernel passes them as constants; the host and the probe
// pass what the record says.  PERSPECTIVE with a lens keeps DefocusBlurCamera's own expression order (camera_ray above), without one PinholeCamera's: a
// DEFOCUS record with type 16 and t0 = t1 = 0, and a PINHOLE / MOTION record with type 16, viewport 1 and no lens, give those cameras' rays bit for bit.
RT_HD bool lens_camera_has_lens(const rt_camera& c) { return c.lens_radius > 0.0f; }
RT_HD bool lens_camera_has_shutter(const rt_camera& c) { return c.t0 != c.t1; }
template <class G>
RT_HD void lens_camera_draw(const rt_camera& c, bool lens, bool shutter, G& rng, float& la, float& lb, float& time) {
    la = 0.0f; lb = 0.0f;
    if (lens) rng_in_unit2(rng, la, lb);
    time = shutter ? mix(c.t0, c.t1, rng.next()) : c.t0;
}
RT_HD Ray lens_camera_ray(const rt_camera& c, uint32_t proj, bool lens, float s, float t, float la, float lb, float time) {
    Ray r;
    const f3 o = mk3(c.o[0], c.o[1], c.o[2]), u = mk3(c.u[0], c.u[1], c.u[2]);
    const f3 v = mk3(c.v[0], c.v[1], c.v[2]), w = mk3(c.w[0], c.w[1], c.w[2]);
    const float a = c.viewport_width, b = c.viewport_height;
    const float half_pi = 0x1.921fb6p+0f;
    r.time = time;
    f3 offset = mk3(0.0f);
    if (lens) {
        offset = u * la + v * lb;
        offset = offset * c.lens_radius;
    }
    if (proj == 0u) {
        if (lens) {   // cu_Cameras.cuh:54-64, term for term
            const f3 forward = w * c.focus_dist;
            const f3 hori = u * a * c.focus_dist;
            const f3 vert = v * b * c.focus_dist;
            r.o = o + offset;
            r.d = forward + hori * s + vert * t - offset;
        } else {      // cu_Cameras.cuh:27-30 with u, v scaled here
            r.o = o;
            r.d = w + (u * a) * s + (v * b) * t;
        }
        return r;
    }
    f3 o0 = o, d0 = w;
    if (proj == RT_CAM_ORTHOGRAPHIC - RT_CAM_PERSPECTIVE) {
        o0 = o + (u * a) * s + (v * b) * t;
    } else if (proj == RT_CAM_FISHEYE - RT_CAM_PERSPECTIVE) {   // equidistant: the angle off the axis is the distance from the centre
        const float x = a * s, y = b * t;
        const float theta = sqrtf(x * x + y * y);
        if (theta != 0.0f) {
            const float k = rt_sinf(theta) / theta;
            d0 = w * rt_sinf(theta + half_pi) + u * (x * k) + v * (y * k);
        }
    } else {                                                     // equirectangular: longitude a s about v, latitude b t
        const float phi = a * s, lam = b * t;
        const float cl = rt_sinf(lam + half_pi);
        d0 = w * (cl * rt_sinf(phi + half_pi)) + u * (cl * rt_sinf(phi)) + v * rt_sinf(lam);
    }
    if (lens) {
        r.o = o0 + offset;
        r.d = d0 * c.focus_dist - offset;
    } else {
        r.o = o0;
        r.d = d0;
    }
    return r;
}
template <class G>
RT_HD Ray lens_camera_sample_ray(const rt_camera& c, float s, float t, G& rng) {
    const bool lens = lens_camera_has_lens(c);
    float la, lb, time;
    lens_camera_draw(c, lens, lens_camera_has_shutter(c), rng, la, lb, time);
    return lens_camera_ray(c, c.type - RT_CAM_PERSPECTIVE, lens, s, t, la, lb, time);
}

// sample_world, main/src/Renderer.cu:139-181.  The emission / background hooks are the reference's own commented
// placeholders (`accum_radiance`, Renderer.cu:142,152,157,163,179); with no emissive material and background 0 this
// is exactly the live function.
__device__ inline f3 sample_world(const DeviceWorld& w, Ray cur_ray, uint32_t max_depth, Rng& rng) {
    f3 accum_attenuation = mk3(1.0f);
    f3 accum_radiance = mk3(0.0f);
    for (uint32_t i = 0; i < max_depth; i++) {
        HitRec rec;
        rec.distance = RT_MISS_DIST; rec.normal = mk3(0.0f); rec.prim = -1; rec.mat = 0;
        if (!world_closest_intersection(w, cur_ray, rec, &rng)) {
            f3 sky;
            if (w.background == 1u) {
                sky = w.background_color;
            } else {
                float t = normalize(cur_ray.d).y * 0.5f + 0.5f;
                sky = linear_interpolate(mk3(0.1f, 0.2f, 0.4f), mk3(0.9f, 0.9f, 0.99f), t);
            }
            return accum_attenuation * sky + accum_radiance;
        }
        const rt_material& m = w.mats[rec.mat];
        if (m.type == RT_MAT_DIFFUSE_LIGHT) accum_radiance = accum_radiance + accum_attenuation * mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
        Ray scattered;
        f3 attenuation;
        if (!material_scatter(m, cur_ray, rec, rng, scattered, attenuation, &w)) return accum_radiance;
        accum_attenuation = accum_attenuation * attenuation;
        cur_ray = scattered;
        cur_ray.o = cur_ray.o + cur_ray.d * 0.001f;
    }
    return accum_radiance;
}

// pixel centre in NDC, Renderer.cu:188-192
RT_HD void pixel_ndc(uint32_t x, uint32_t y, uint32_t width, uint32_t height, float& psx, float& psy, float& ndcx, float& ndcy) {
    psx = 1.0f / (float)width;
    psy = 1.0f / (float)height;
    ndcx = ((float)x + 0.5f) * psx * 2.0f - 1.0f;
    ndcy = ((float)y + 0.5f) * psy * 2.0f - 1.0f;
}

// camera ray of one sample: jitter in a disc of half a pixel, then sample_ray (Renderer.cu:199-201).
// The RNG is keyed per (pixel, sample) — SURVEY.md Appendix A item 7.
RT_HD Ray primary_ray(const rt_camera& cam, uint32_t width, uint32_t height, uint32_t gid, Rng& rng) {
    uint32_t x = gid % width, y = gid / width;
    float psx, psy, ndcx, ndcy;
    pixel_ndc(x, y, width, height, psx, psy, ndcx, ndcy);
    float jx, jy;
    rng_in_unit2(rng, jx, jy);
    return camera_sample_ray(cam, ndcx + jx * psx, ndcy + jy * psy, rng);
}

__device__ inline f3 one_sample(const DeviceWorld& w, const rt_camera& cam, uint32_t width, uint32_t height,
                                uint32_t max_depth, uint64_t seed, uint32_t gid, uint32_t s) {
    Rng rng;
    rng.init(seed, gid, s, RT_STREAM_RENDER);
    Ray ray = primary_ray(cam, width, height, gid, rng);
    return sample_world(w, ray, max_depth, rng);
}

// ref_core_probe.cpp — golden-vector generator for the hot path's core (test infrastructure): spheres, the flat BVH and its
// builders, the three Scatters + LambertianTexture, the three cameras.
//
// Compiles the REFERENCE's own code from where it lies under /root/reference (never copied), with plain g++ -std=c++20 and
// NVIDIA's real <cuda_runtime.h> (as ref_path_probe.cpp):
//     main/src/rt_engine/geometry/SphereHittable.cuh, SphereHittable.cu   _sphere_closest_intersection, (Moving)SphereHittable,
//                                                                         getNormal, getSphereBounds / getMovingSphereBounds
//     main/src/rt_engine/geometry/BVH.cuh, BVH.cu                         BVH::ClosestIntersection, BVH_Handle::Factory
//     main/src/rt_engine/shaders/cu_materials.cuh                         Lambertian/Metal/Dielectric Abstract, LambertianTexture
//     main/src/rt_engine/shaders/cu_Cameras.cuh                           PinholeCamera, DefocusBlurCamera, MotionBlurCamera
//     main/src/utilities/cuda_utilities/cuRandom.cuh, utilities/glm_utils.h   cuRandom, glm::cuRandomInUnit / cuRandomOnUnit
// Three stand-ins (oracle/ref_shim/), none of which does arithmetic on a pinned value:
//   1. ref_shim/curand_kernel.h (first on -I): curand_uniform() served from a tape of k in [1, 2^24], u = k * 2^-24 — the values
//      the product's generator produces.  It counts draws and aborts on a tape overrun.  The random SOURCE is not part of the
//      contract (the product replaced cuRAND by design); which draws are taken, in what order, and their arithmetic are, and
//      those stay in the reference's cuRandom.cuh / glm_utils.h.
//   2. -DCUDA_UTILITIES_H -DCUDA_UTILITIES_CUH keep cuError.h (<format>) and cuda_utils.cuh (<<<1,1>>>) out; -include
//      ref_shim/prelude.h supplies CUDA_ASSERT, newOnDevice<T> as a host `new`, cuda_swap as the same three moves.
//   3. ref_shim/cuda_link_stubs.cpp: cudaMalloc / cudaMemcpy / cudaFree as malloc / memcpy / free, so BVH_Handle's arrays and its
//      BVH live in host memory and BVH::ClosestIntersection runs here.
// `private` is defined to `public` and `class` to `struct` around BVH.cuh / BVH.cu only, to read the Factory's node array and to
// call _build_bvh_rec2 (BuildBVH_TopDown is compiled with `#if 1` -> rec1): access, not arithmetic.
//
// Usage: oracle/_ref/core_probe <out_dir> <natural_tapes.u32>     (oracle/gen_golden.py)
// natural_tapes.u32: rows of [pixel, sample, k_0 .. k_{L-1}] — the product's own uniforms for (seed 1984, pixel, sample),
// L = NATURAL_LEN, written by gen_golden.py from the oracle's orc_rng_uniforms.
#include <curand_kernel.h>   // the stand-in: must precede glm_utils.h (its cuRandom helpers key on CURAND_KERNEL_H_)

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "rt_engine/ray_data.cuh"
#include "rt_engine/geometry/aabb.cuh"
#include "rt_engine/geometry/hittable.cuh"
#include "rt_engine/shaders/cu_materials.cuh"
#include "rt_engine/shaders/cu_Cameras.cuh"
#include "rt_engine/geometry/SphereHittable.cuh"
#include "rt_engine/geometry/SphereHittable.cu"
#define private public
#define class struct
#include "rt_engine/geometry/BVH.cuh"
#include "rt_engine/geometry/BVH.cu"
#undef class
#undef private

static const int NATURAL_LEN = 96;

static uint64_t g_state = 0xC0DEull;
static uint32_t next_u32() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
static float uni() { return (float)(next_u32() >> 8) * (1.0f / 16777216.0f); }
static float sym(float s) { return (uni() * 2.0f - 1.0f) * s; }
static float special(uint32_t k) {   // ref_path_probe.cpp's table
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float tab[] = {0.0f, -0.0f, inf, -inf, nan, 1e-38f, 1e-42f, -1e-42f, 3.402823466e+38F, -3.402823466e+38F, 1e20f, -1e20f, 1e-20f};
    return tab[k % (sizeof(tab) / sizeof(tab[0]))];
}
static glm::vec3 v3(float s) { return glm::vec3(sym(s), sym(s), sym(s)); }
static glm::vec3 axis_vec(int ax, float s) { glm::vec3 v(0.0f); v[ax] = s; return v; }

template <typename T> static void write_file(const std::string& path, const std::vector<T>& d) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::perror(path.c_str()); std::exit(1); }
    std::fwrite(d.data(), sizeof(T), d.size(), f);
    std::fclose(f);
    std::printf("%-44s %zu values\n", path.c_str(), d.size());
}
static void put(std::vector<float>& v, const glm::vec3& a) { v.push_back(a.x); v.push_back(a.y); v.push_back(a.z); }
static void put_ray(std::vector<float>& v, const Ray& r) { put(v, r.o); put(v, r.d); v.push_back(r.time); }

// ---------------------------------------------------------------------------------------------------------------------
// tapes
// ---------------------------------------------------------------------------------------------------------------------
struct Natural { uint32_t pixel, sample; std::vector<uint32_t> k; };
static std::vector<Natural> g_natural;
static size_t g_next_natural = 0;

static void load_natural(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::perror(path.c_str()); std::exit(1); }
    std::vector<uint32_t> row(2 + NATURAL_LEN);
    while (std::fread(row.data(), 4, row.size(), f) == row.size())
        g_natural.push_back({row[0], row[1], std::vector<uint32_t>(row.begin() + 2, row.end())});
    std::fclose(f);
    if (g_natural.empty()) { std::fprintf(stderr, "%s: no natural tapes\n", path.c_str()); std::exit(1); }
}

// A tape = an adversarial prefix (empty for a natural case) followed by the next natural tape of the pool.
struct Tape { std::vector<uint32_t> k; uint32_t pixel, sample, natural; };
static Tape make_tape(std::vector<uint32_t> prefix = {}) {
    const Natural& n = g_natural[g_next_natural++ % g_natural.size()];
    Tape t{prefix, n.pixel, n.sample, prefix.empty() ? 1u : 0u};
    t.k.insert(t.k.end(), n.k.begin(), n.k.end());
    return t;
}
// the consumed part of a tape: [offset, length, pixel, sample, natural] into idx, the k's into tape
struct TapeLog {
    std::vector<uint32_t> idx, tape;
    void begin(const Tape& t) { ref_tape::load(t.k.data(), t.k.size()); }
    uint32_t end(const Tape& t) {
        const uint32_t used = (uint32_t)ref_tape::pos;
        idx.push_back((uint32_t)tape.size()); idx.push_back(used); idx.push_back(t.pixel); idx.push_back(t.sample); idx.push_back(t.natural);
        tape.insert(tape.end(), t.k.begin(), t.k.begin() + used);
        ref_tape::load(nullptr, 0);
        return used;
    }
};
static const uint32_t K_ZERO = 1u << 23;   // u = 0.5  -> next<L>() * 2 - 1 = +0
static const uint32_t K_ONE = 1u << 24;    // u = 1    -> +1
static const uint32_t K_MIN = 1u;          // u = 2^-24 -> -1 + 2^-23

// ---------------------------------------------------------------------------------------------------------------------
// G5: _sphere_closest_intersection (SphereHittable.cuh:15-33), SphereHittable / MovingSphereHittable::ClosestIntersection and
// getNormal (SphereHittable.cu:43-102), getSphereBounds / getMovingSphereBounds
// in  [c0 3, c1 3, radius, moving, o 3, d 3, time, preset rec.distance]                                        16
// out [t of _sphere_closest_intersection at the ray's time, hit, rec.distance, normal 3 (0 on a miss), bounds min 3, max 3] 12
// ---------------------------------------------------------------------------------------------------------------------
static void gen_sphere(const std::string& dir) {
    const int N = 4096;
    std::vector<float> in, out;
    LambertianAbstract<Sphere> mat_s(glm::vec3(0.5f));
    LambertianAbstract<MovingSphere> mat_m(glm::vec3(0.5f));
    for (int k = 0; k < N; k++) {
        const int kind = k % 16;
        glm::vec3 c0 = v3(5.0f), c1 = c0;
        float r = 0.2f + uni() * 2.0f;
        bool moving = false;
        float time = 0.0f, preset = _MISS_DIST;
        glm::vec3 o = v3(12.0f), d = (c0 + v3(r * 1.3f)) - o;
        if (kind == 1) {   // tangent: hb * hb - a * c == 0 exactly (integer centre, power-of-two radius and direction scale)
            c0 = glm::vec3((float)((int)(next_u32() % 11) - 5), (float)((int)(next_u32() % 11) - 5), (float)((int)(next_u32() % 11) - 5));
            c1 = c0;
            r = std::ldexp(1.0f, (int)(next_u32() % 4) - 1);
            int ax = next_u32() % 3, bx = (ax + 1 + next_u32() % 2) % 3;
            float side = (next_u32() & 1) ? r : -r;
            o = c0 + axis_vec(ax, side) + axis_vec(bx, (float)((int)(next_u32() % 9) - 4));
            d = axis_vec(bx, ((next_u32() & 1) ? 1.0f : -1.0f) * std::ldexp(1.0f, (int)(next_u32() % 5) - 2));
        }
        if (kind == 2) o = c0 + v3(r * 0.5f);                                           // origin inside
        if (kind == 3) { int ax = next_u32() % 3; o = c0 + axis_vec(ax, (next_u32() & 1) ? r : -r); d = v3(1.0f); }   // origin on the sphere
        if (kind == 4) d = -d;                                                          // sphere behind the origin
        if (kind == 5) r = -r;                                                          // hollow glass: negative radius
        if (kind == 6) d = d * std::ldexp(1.0f, (int)(next_u32() % 40) - 20);           // unnormalised directions of any length
        if (kind == 7 || kind == 8 || kind == 9) {
            moving = true;
            c1 = c0 + v3(1.5f);
            time = kind == 7 ? 0.0f : (kind == 8 ? 1.0f : uni());
            glm::vec3 ct = glm::mix(c0, c1, time);
            d = (ct + v3(r * 1.2f)) - o;
        }
        if (kind == 10) {
            switch (next_u32() % 3) {
                case 0: o[next_u32() % 3] = special(next_u32()); break;
                case 1: d[next_u32() % 3] = special(next_u32()); break;
                default: c0[next_u32() % 3] = special(next_u32()); c1 = c0; break;
            }
        }
        if (kind == 11) preset = uni() * 20.0f;                                         // rec.distance already set by an earlier hit
        if (kind == 12) d[next_u32() % 3] = 0.0f;
        if (kind == 13) {   // axis-aligned hit on a pole: normal exactly +-e_axis
            c0 = glm::vec3((float)((int)(next_u32() % 11) - 5), (float)((int)(next_u32() % 11) - 5), (float)((int)(next_u32() % 11) - 5));
            c1 = c0;
            r = (float)(1 + next_u32() % 3);
            int ax = next_u32() % 3;
            float s = (next_u32() & 1) ? 1.0f : -1.0f;
            o = c0 + axis_vec(ax, s * 8.0f);
            d = axis_vec(ax, -s);
        }
        if (kind == 14) { moving = true; c1 = c0 + v3(3.0f); time = (float)(next_u32() % 3) * 0.5f; preset = uni() * 15.0f; }
        Ray ray(o, d, time);
        glm::vec3 ct = moving ? glm::mix(c0, c1, time) : c0;
        float t_raw = _sphere_closest_intersection(ray, ct, r);
        if (kind == 11 && (k & 32) && t_raw < _MISS_DIST) preset = t_raw;              // equal distance: `t >= rec.distance` rejects
        RayPayload rec;
        rec.distance = preset;
        bool hit;
        glm::vec3 normal(0.0f);
        aabb b;
        Sphere sp(c0, r);
        MovingSphere msp(c0, c1, r);
        if (moving) {
            MovingSphereHittable h(&msp, &mat_m);
            hit = h.ClosestIntersection(ray, rec);
            if (hit) normal = MovingSphere::getNormal(ray, rec);
            b = getMovingSphereBounds(msp);
        } else {
            SphereHittable h(&sp, &mat_s);
            hit = h.ClosestIntersection(ray, rec);
            if (hit) normal = Sphere::getNormal(ray, rec);
            b = getSphereBounds(sp);
        }
        put(in, c0); put(in, c1); in.push_back(r); in.push_back(moving ? 1.0f : 0.0f); put_ray(in, ray); in.push_back(preset);
        out.push_back(t_raw); out.push_back(hit ? 1.0f : 0.0f); out.push_back(rec.distance); put(out, normal); put(out, b.getMin()); put(out, b.getMax());
    }
    write_file(dir + "/ref_core_sphere_in.f32", in);
    write_file(dir + "/ref_core_sphere_out.f32", out);
}

// ---------------------------------------------------------------------------------------------------------------------
// G6: BVH_Handle::Factory (BVH.cu:156-384) and BVH::ClosestIntersection (BVH.cu:54-106) over real SphereHittable leaves
// ---------------------------------------------------------------------------------------------------------------------
// A recording Hittable around each leaf: delegates to the real SphereHittable, logs which leaves are reached and in what order.
static std::vector<int>* g_visits = nullptr;
static int g_hit_slot = -1;
struct Recorder : public Hittable {
    const Hittable* inner; int slot = -1;
    explicit Recorder(const Hittable* h) : inner(h) {}
    virtual bool ClosestIntersection(const Ray& ray, RayPayload& rec) const override {
        g_visits->push_back(slot);
        bool hit = inner->ClosestIntersection(ray, rec);
        if (hit) g_hit_slot = slot;
        return hit;
    }
};

struct SphereSet {
    std::vector<Sphere> sp; std::vector<MovingSphere> msp; std::vector<char> moving;
    std::vector<Hittable*> leaves; std::vector<Recorder> rec;
    LambertianAbstract<Sphere> mat_s{glm::vec3(0.5f)};
    LambertianAbstract<MovingSphere> mat_m{glm::vec3(0.5f)};
    size_t size() const { return moving.size(); }
    aabb bounds(size_t i) const { return moving[i] ? getMovingSphereBounds(msp[i]) : getSphereBounds(sp[i]); }
    void finish() {   // vectors are complete: take pointers
        for (size_t i = 0; i < size(); i++)
            leaves.push_back(moving[i] ? (Hittable*)new MovingSphereHittable(&msp[i], &mat_m) : (Hittable*)new SphereHittable(&sp[i], &mat_s));
        for (size_t i = 0; i < size(); i++) rec.emplace_back(leaves[i]);
    }
    ~SphereSet() { for (auto* h : leaves) delete h; }
    void put_spheres(std::vector<float>& v) const {   // [c0 3, c1 3, radius, moving]
        for (size_t i = 0; i < size(); i++) {
            glm::vec3 a = moving[i] ? msp[i].center0 : sp[i].center, b = moving[i] ? msp[i].center1 : sp[i].center;
            put(v, a); put(v, b); v.push_back(moving[i] ? msp[i].radius : sp[i].radius); v.push_back(moving[i] ? 1.0f : 0.0f);
        }
    }
    glm::vec3 centre(size_t i) const { return moving[i] ? msp[i].center0 : sp[i].center; }
    float radius(size_t i) const { return moving[i] ? msp[i].radius : sp[i].radius; }
};

static void put_node(std::vector<float>& v, const BVH::Node& n) {   // the layout of rt_bvh_node: min 3, max 3, left, right (int32 bits)
    put(v, n.bounds.getMin()); put(v, n.bounds.getMax());
    float l, r;
    std::memcpy(&l, &n.left_child_idx, 4); std::memcpy(&r, &n.right_child_hittable_idx, 4);
    v.push_back(l); v.push_back(r);
}

// rays through a set: [o 3, d 3, time]
static std::vector<Ray> make_rays(const SphereSet& s, int R) {
    std::vector<Ray> rays;
    for (int k = 0; k < R; k++) {
        size_t a = next_u32() % s.size();
        glm::vec3 o = v3(14.0f);
        if (k % 8 == 1) o = s.centre(a) + v3(s.radius(a) * 0.4f);                 // starts inside a sphere
        glm::vec3 d = (s.centre(next_u32() % s.size()) + v3(1.0f)) - o;
        if (k % 8 == 2) d[next_u32() % 3] = 0.0f;
        if (k % 8 == 3) d = d * std::ldexp(1.0f, (int)(next_u32() % 16) - 8);
        if (k % 8 == 4) d = v3(1.0f);
        if (k % 8 == 5) {   // along an axis through the point where a sphere touches its box plane: tangent (d == 0) and 0/0 slabs
            int ax = next_u32() % 3, bx = (ax + 1) % 3;
            o = s.centre(a) + axis_vec(ax, s.radius(a)) - axis_vec(bx, 20.0f);
            d = axis_vec(bx, 1.0f);
        }
        rays.push_back(Ray(o, d, (k % 8 == 6) ? uni() : (float)(k & 1)));
    }
    return rays;
}

// trace every ray through a BVH; out per ray: [hit, rec.distance, hittable slot, leaves reached, first 8 leaves]
static void trace_all(const BVH* bvh, const std::vector<Ray>& rays, std::vector<float>& rays_out, std::vector<float>& out) {
    for (const Ray& ray : rays) {
        std::vector<int> visits;
        g_visits = &visits;
        g_hit_slot = -1;
        RayPayload rec;   // rec.distance = _MISS_DIST: what sample_world starts every trace with (Renderer.cu:147)
        bool hit = bvh->ClosestIntersection(ray, rec);
        put_ray(rays_out, ray);
        out.push_back(hit ? 1.0f : 0.0f); out.push_back(rec.distance); out.push_back(hit ? (float)g_hit_slot : -1.0f);
        out.push_back((float)visits.size());
        for (int v = 0; v < 8; v++) out.push_back(v < (int)visits.size() ? (float)visits[v] : -1.0f);
    }
}

// _build_bvh_rec2 on an empty range recurses forever (a split plane that leaves one side empty): predict it with the
// reference's own _find_optimal_split / _partition_by_split on a copy before the real build
static bool rec2_terminates(std::vector<std::tuple<aabb, const Hittable*>> arr, int start, int end) {
    if (end - start <= 1) return end - start == 1;
    BVH_Handle::Factory f(arr);
    aabb bounds = f._get_partition_bounds(start, end);
    int axis; float split; int mid;
    f._find_optimal_split(start, end, bounds, axis, split);
    f._partition_by_split(start, end, axis, split, mid);
    if (mid == start || mid == end) return false;
    return rec2_terminates(arr, start, mid) && rec2_terminates(arr, mid, end);
}

static bool min_ties(const SphereSet& s) {   // std::sort is unstable: no two boxes may share bounds.min on any axis
    for (int ax = 0; ax < 3; ax++)
        for (size_t i = 0; i < s.size(); i++)
            for (size_t j = i + 1; j < s.size(); j++)
                if (s.bounds(i).getMin()[ax] == s.bounds(j).getMin()[ax]) return true;
    return false;
}

static void gen_bvh(const std::string& dir) {
    const int sizes[] = {1, 2, 3, 4, 5, 7, 8, 13, 16, 31, 33, 64};
    std::vector<float> spheres, nodes, rays, out;
    std::vector<int32_t> idx, order;   // idx rows: [sphere offset, n, builder, node offset, n nodes, root, ray offset, n rays]
    int n_sets = 0, skipped = 0;
    for (int rep = 0; rep < 4; rep++)
        for (int n : sizes) {
            SphereSet s;
            const float spread = 2.0f + 1.2f * std::cbrt((float)n) * (rep == 3 ? 0.5f : 2.0f);
            for (int i = 0; i < n; i++) {
                glm::vec3 c = v3(spread);
                float r = 0.2f + uni() * (rep == 3 ? 1.5f : 0.8f);
                bool mv = (rep == 2) && (i % 3 == 1);
                s.sp.emplace_back(c, r);
                s.msp.emplace_back(c, c + v3(0.7f), r);
                s.moving.push_back(mv ? 1 : 0);
            }
            if (min_ties(s)) { skipped++; continue; }
            s.finish();
            const int sphere_off = (int)(spheres.size() / 8);
            s.put_spheres(spheres);
            std::vector<Ray> rs = make_rays(s, 48);
            for (int builder = 0; builder < 3; builder++) {
                std::vector<std::tuple<aabb, const Hittable*>> arr;
                for (size_t i = 0; i < s.size(); i++) arr.emplace_back(s.bounds(i), &s.rec[i]);
                if (builder == 1 && !rec2_terminates(arr, 0, (int)arr.size())) { skipped++; continue; }
                BVH_Handle::Factory f(arr);
                if (builder == 0) f.BuildBVH_TopDown();
                else if (builder == 2) f.BuildBVH_BottomUp();
                else {   // BuildBVH_TopDown with the `#else` branch of BVH.cu:168-172
                    f.root_idx = f._build_bvh_rec2(0, (int)arr.size());
                    f.hittables.reserve(arr.size());
                    for (size_t i = 0; i < arr.size(); i++) f.hittables.push_back(std::get<1>(arr[i]));
                }
                for (size_t i = 0; i < f.hittables.size(); i++) {
                    Recorder* r = const_cast<Recorder*>(static_cast<const Recorder*>(f.hittables[i]));
                    r->slot = (int)i;
                    order.push_back((int32_t)(r - s.rec.data()));   // hittables[i] is sphere order[i] of the input set
                }
                idx.push_back(sphere_off); idx.push_back(n); idx.push_back(builder);
                idx.push_back((int32_t)(nodes.size() / 8)); idx.push_back((int32_t)f.bvh_nodes.size()); idx.push_back(f.root_idx);
                for (const BVH::Node& nd : f.bvh_nodes) put_node(nodes, nd);
                BVH_Handle* h = f.MakeHandle();
                idx.push_back((int32_t)(rays.size() / 7)); idx.push_back((int32_t)rs.size());
                trace_all(h->getBVHPtr(), rs, rays, out);
                delete h;
                n_sets++;
            }
        }
    std::printf("G6 builders: %d (set, builder) pairs, %d skipped (ties / rec2 empty range)\n", n_sets, skipped);
    write_file(dir + "/ref_core_bvh_spheres.f32", spheres);
    write_file(dir + "/ref_core_bvh_idx.i32", idx);
    write_file(dir + "/ref_core_bvh_order.i32", order);
    write_file(dir + "/ref_core_bvh_nodes.f32", nodes);
    write_file(dir + "/ref_core_bvh_rays.f32", rays);
    write_file(dir + "/ref_core_bvh_out.f32", out);
}

// Traversal on trees given by the fixture (not built): duplicate spheres, coincident boxes, rays tangent at the box planes.
// idx rows: [sphere offset, n, node offset, n nodes, root, ray offset, n rays]; hittables[i] = sphere i
static void gen_bvh_given(const std::string& dir) {
    std::vector<float> spheres, nodes, rays, out;
    std::vector<int32_t> idx;
    for (int sc = 0; sc < 48; sc++) {
        const int n = 2 + (int)(next_u32() % 9);
        SphereSet s;
        for (int i = 0; i < n; i++) {
            glm::vec3 c = v3(4.0f);
            float r = 0.3f + uni();
            if (i > 0 && (sc % 3 == 0) && (next_u32() % 2)) { size_t j = next_u32() % i; c = s.sp[j].center; r = s.sp[j].radius; }   // duplicate
            if (sc % 3 == 1) { c = glm::vec3((float)(i % 3) * 2.0f, (float)((i / 3) % 2) * 2.0f, 0.0f); r = 1.0f; }   // touching: shared box planes
            s.sp.emplace_back(c, r);
            s.msp.emplace_back(c, c, r);
            s.moving.push_back(0);
        }
        s.finish();
        // random topology; node box = union of the children, or (sc % 3 == 2) a coincident copy of one child's box
        struct Item { aabb b; int node; };
        std::vector<BVH::Node> nv;
        std::vector<Item> items;
        for (int i = 0; i < n; i++) {
            BVH::Node leaf; leaf.bounds = s.bounds(i); leaf.left_child_idx = _IS_LEAF_CODE; leaf.right_child_hittable_idx = i;
            nv.push_back(leaf);
            items.push_back({leaf.bounds, (int)nv.size() - 1});
        }
        while (items.size() > 1) {
            size_t i = next_u32() % items.size();
            Item a = items[i]; items.erase(items.begin() + i);
            size_t j = next_u32() % items.size();
            Item b = items[j]; items.erase(items.begin() + j);
            BVH::Node inner;
            inner.bounds = aabb(a.b, b.b);
            if (sc % 3 == 2 && (next_u32() % 2)) { nv[a.node].bounds = inner.bounds; nv[b.node].bounds = inner.bounds; }   // coincident boxes
            inner.left_child_idx = a.node; inner.right_child_hittable_idx = b.node;
            nv.push_back(inner);
            items.push_back({inner.bounds, (int)nv.size() - 1});
        }
        const int root = items[0].node;
        std::vector<const Hittable*> hs;
        for (int i = 0; i < n; i++) { s.rec[i].slot = i; hs.push_back(&s.rec[i]); }
        idx.push_back((int32_t)(spheres.size() / 8)); idx.push_back(n);
        s.put_spheres(spheres);
        idx.push_back((int32_t)(nodes.size() / 8)); idx.push_back((int32_t)nv.size()); idx.push_back(root);
        for (const BVH::Node& nd : nv) put_node(nodes, nd);
        BVH_Handle h(nv[root].bounds, root, nv, hs);
        std::vector<Ray> rs = make_rays(s, 64);
        idx.push_back((int32_t)(rays.size() / 7)); idx.push_back((int32_t)rs.size());
        trace_all(h.getBVHPtr(), rs, rays, out);
    }
    write_file(dir + "/ref_core_bvhgiven_spheres.f32", spheres);
    write_file(dir + "/ref_core_bvhgiven_idx.i32", idx);
    write_file(dir + "/ref_core_bvhgiven_nodes.f32", nodes);
    write_file(dir + "/ref_core_bvhgiven_rays.f32", rays);
    write_file(dir + "/ref_core_bvhgiven_out.f32", out);
}

// ---------------------------------------------------------------------------------------------------------------------
// G7: a ray hits a real Sphere / MovingSphere, then Material::Scatter (cu_materials.cuh:16-143)
// in  [c0 3, c1 3, radius, moving, type, albedo 3, param, albedo2 3, ray o 3, d 3, time]        23
//     type / albedo / param / albedo2 as rt_material: 0 Lambertian, 1 Metal (param fuzz), 2 Dielectric (param ior),
//     3 LambertianTexture (albedo = c1 = even, albedo2 = c2 = odd, param = 1.0f / scale as checker_texture keeps it)
// out [rec.distance, normal 3, scattered, out ray 7 (zeros when absorbed), attenuation 3 (zeros when absorbed), draws]   16
// ---------------------------------------------------------------------------------------------------------------------
struct ScatterCase { glm::vec3 c0, c1; float r; bool moving; int type; glm::vec3 albedo; float param_in; glm::vec3 albedo2; Ray ray; };

template <typename G>
static void run_scatter(const ScatterCase& c, const Tape& t, TapeLog& log, std::vector<float>& in, std::vector<float>& out) {
    Sphere sp(c.c0, c.r);
    MovingSphere msp(c.c0, c.c1, c.r);
    LambertianAbstract<G> lam(c.albedo);
    MetalAbstract<G> met(c.albedo, c.param_in);
    DielectricAbstract<G> die(c.albedo, c.param_in);
    LambertianTexture<G> tex(c.albedo, c.albedo2, c.param_in);
    const Material* m = c.type == 0 ? (const Material*)&lam : c.type == 1 ? (const Material*)&met : c.type == 2 ? (const Material*)&die : (const Material*)&tex;
    RayPayload rec;
    Ray o;
    glm::vec3 att;
    bool hit, sc;
    log.begin(t);
    if constexpr (std::is_same_v<G, Sphere>) { SphereHittable h(&sp, &lam); hit = h.ClosestIntersection(c.ray, rec); }
    else { MovingSphereHittable h(&msp, &lam); hit = h.ClosestIntersection(c.ray, rec); }
    if (!hit) { std::fprintf(stderr, "G7: a scatter case misses its sphere\n"); std::exit(1); }
    cuRandom rng(1984);
    o = Ray(glm::vec3(0.0f), glm::vec3(0.0f), 0.0f);
    att = glm::vec3(0.0f);
    sc = m->Scatter(c.ray, rec, rng, o, att);
    const uint32_t draws = log.end(t);
    put(in, c.c0); put(in, c.moving ? c.c1 : c.c0); in.push_back(c.r); in.push_back(c.moving ? 1.0f : 0.0f);
    in.push_back((float)c.type); put(in, c.albedo);
    in.push_back(c.type == 3 ? 1.0f / c.param_in : c.param_in);
    put(in, c.type == 3 ? c.albedo2 : glm::vec3(0.0f)); put_ray(in, c.ray);
    out.push_back(rec.distance); put(out, G::getNormal(c.ray, rec)); out.push_back(sc ? 1.0f : 0.0f); put_ray(out, o); put(out, att);
    out.push_back((float)draws);
}
static void run_scatter_any(const ScatterCase& c, const Tape& t, TapeLog& log, std::vector<float>& in, std::vector<float>& out) {
    if (c.moving) run_scatter<MovingSphere>(c, t, log, in, out);
    else run_scatter<Sphere>(c, t, log, in, out);
}

// The product's one documented deviation (rt_oracle.h): Schlick's (1 - cos)^5 is x^2^2 * x there, powf(x, 5) in the reference.
// Cases at u == reflect_prob are kept only where the two powers are the same float, so that they test the comparison, not libm.
// This selects cases; what is expected of them comes from the reference's Scatter.
static bool schlick_power_agrees(const Ray& ray, glm::vec3 outward) {
    const glm::vec3 facing = glm::dot(ray.d, outward) > 0 ? -outward : outward;
    const float c = std::min(glm::dot(-glm::normalize(ray.d), facing), 1.0f);
    const float x = 1 - c, sq = x * x;
    return powf(x, 5.0f) == sq * sq * x;
}

// a ray from outside (or, `inside`, from inside) that hits the sphere, found by rejection on the probe's own stream
static Ray aim(const glm::vec3& c, float r, bool inside, float time) {
    const float ar = std::fabs(r);
    for (;;) {
        glm::vec3 o = inside ? c + v3(ar * 0.55f) : c + v3(ar * 6.0f);
        glm::vec3 d = (c + v3(ar * 0.95f)) - o;
        if (next_u32() % 4 == 0) d = d * std::ldexp(1.0f, (int)(next_u32() % 8) - 4);
        Ray ray(o, d, time);
        if (_sphere_closest_intersection(ray, c, r) < _MISS_DIST) return ray;
    }
}

static void gen_scatter(const std::string& dir) {
    std::vector<float> in, out;
    TapeLog log;
    struct M { int type; float param; };
    const M mats[] = {{0, 0.0f}, {1, 0.0f}, {1, 0.3f}, {1, 1.0f}, {2, 1.5f}, {2, 1.0f / 1.5f}, {2, 1.333f}, {2, 2.4f}, {3, 0.32f}};
    // natural tapes: every material on static / moving spheres, front / back faces, hollow spheres
    for (int k = 0; k < 2304; k++) {
        const M& m = mats[k % 9];
        ScatterCase c;
        c.c0 = v3(3.0f); c.c1 = c.c0 + v3(1.0f);
        c.r = 0.3f + uni() * 1.5f;
        c.moving = (k / 9) % 4 == 1;
        const int geo = (k / 36) % 4;   // 0 outside, 1 inside (back face / TIR), 2 hollow (negative radius), 3 outside, grazing
        if (geo == 2) c.r = -c.r;
        float time = c.moving ? uni() : 0.0f;
        glm::vec3 ct = c.moving ? glm::mix(c.c0, c.c1, time) : c.c0;
        c.ray = aim(ct, c.r, geo == 1, time);
        if (geo == 3) {   // nearly tangent: Fresnel reflectance near 1, TIR from inside
            glm::vec3 o = ct + glm::vec3(std::fabs(c.r) * (0.999f - 0.01f * uni()), 0.0f, -4.0f);
            c.ray = Ray(o, glm::vec3(0.0f, 0.0f, 1.0f), time);
            if (_sphere_closest_intersection(c.ray, ct, c.r) >= _MISS_DIST) c.ray = aim(ct, c.r, false, time);
        }
        c.type = m.type; c.param_in = m.param;
        c.albedo = glm::vec3(uni(), uni(), uni()); c.albedo2 = glm::vec3(uni(), uni(), uni());
        run_scatter_any(c, make_tape(), log, in, out);
    }
    // adversarial tapes: edges of measure zero under the product's stream
    auto pole_case = [](int type, float param) {   // axis-aligned hit on the +z pole: normal exactly (0, 0, 1), in_ray.d = (0, 0, -1)
        ScatterCase c;
        c.c0 = glm::vec3(1.0f, -2.0f, 3.0f); c.c1 = c.c0; c.r = 2.0f; c.moving = false;
        c.type = type; c.param_in = param; c.albedo = glm::vec3(0.25f, 0.5f, 0.75f); c.albedo2 = glm::vec3(0.9f, 0.1f, 0.3f);
        c.ray = Ray(c.c0 + glm::vec3(0.0f, 0.0f, 6.0f), glm::vec3(0.0f, 0.0f, -1.0f), 0.0f);
        return c;
    };
    const uint32_t Z = K_ZERO, O = K_ONE;
    const std::vector<std::vector<uint32_t>> unit3_prefixes = {
        {Z, Z, Z},                                        // the zero vector: near_zero rejects (the product: l2 > 0)
        {O, Z, Z}, {Z, O, Z}, {Z, Z, O},                  // length2 == 1: rejected
        {K_MIN, Z, Z}, {Z, K_MIN, Z},                     // -1 + 2^-23: accepted
        {K_MIN, K_MIN, K_MIN}, {O, O, O}, {O, K_MIN, Z},  // outside the ball
        {Z + 1, Z, Z}, {Z, Z, Z - 1},                     // the smallest non-zero vectors: 2^-23 on one axis
        {Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z},   // 11 rejections
        {O, O, O, Z, Z, Z, K_MIN, K_MIN, Z, O, Z, Z, Z, O, Z, Z, Z, O, Z, Z, Z, O, O, O, O, O, O, O, O, O, Z, O, Z, K_MIN, K_MIN, K_MIN},   // 12
        {Z, Z, Z / 2},                                    // (0, 0, -0.5) -> unit (0, 0, -1)
    };
    for (const M& m : mats) {
        if (m.type == 2) continue;
        for (const auto& p : unit3_prefixes) {
            ScatterCase c = pole_case(m.type, m.param);
            run_scatter_any(c, make_tape(p), log, in, out);
            c = pole_case(m.type, m.param);
            c.c0 = glm::vec3(0.5f, 0.25f, -1.0f); c.c1 = c.c0; c.ray = aim(c.c0, c.r, false, 0.0f);
            run_scatter_any(c, make_tape(p), log, in, out);
        }
    }
    // Lambertian absorbed: normal (0,0,1) + unit (0,0,-1) == 0 -> near_zero; Metal fuzz 1: reflect = (0,0,1), + (0,0,-1) == 0
    for (const M& m : mats)
        if (m.type != 2) {
            ScatterCase c = pole_case(m.type, m.param);
            run_scatter_any(c, make_tape({Z, Z, Z / 2}), log, in, out);
            run_scatter_any(c, make_tape({Z, Z, Z, Z, Z, Z / 2}), log, in, out);
        }
    // Dielectric: u == reflect_prob exactly (strict `>` refracts), and its two neighbours on the 2^-24 grid.  reflect_prob is found
    // by asking the reference's own Scatter: with one-draw tapes, the smallest k in (2^23, 2^24] that refracts is reflect_prob * 2^24
    // (every float in [0.5, 1) lies on the 2^-24 grid).  A case that takes no draw is total internal reflection.  See
    // schlick_power_agrees for the cases left out.
    int exact = 0, tir = 0;
    for (int k = 0; (exact < 96 || tir < 16) && k < 400000; k++) {
        const float iors[] = {1.5f, 1.0f / 1.5f, 1.333f, 2.4f};
        ScatterCase c;
        c.c0 = glm::vec3(sym(2.0f), sym(2.0f), sym(2.0f)); c.c1 = c.c0; c.r = 0.5f + uni(); c.moving = false;
        c.type = 2; c.param_in = iors[k % 4]; c.albedo = glm::vec3(uni(), uni(), uni()); c.albedo2 = glm::vec3(0.0f);
        const bool inside = (k / 4) % 2;
        glm::vec3 o = c.c0 + glm::vec3(c.r * (inside ? 0.3f * uni() : 0.9f + 0.1f * uni()), c.r * sym(0.05f), inside ? 0.0f : -4.0f * c.r);
        c.ray = Ray(o, glm::vec3(inside ? 1.0f : sym(0.05f), sym(0.05f), inside ? sym(0.3f) : 1.0f), 0.0f);
        Sphere sp(c.c0, c.r);
        LambertianAbstract<Sphere> lam(glm::vec3(0.5f));
        DielectricAbstract<Sphere> die(c.albedo, c.param_in);
        SphereHittable h(&sp, &lam);
        RayPayload rec;
        if (!h.ClosestIntersection(c.ray, rec)) continue;
        // the scattered direction for u = kk * 2^-24, and the number of draws taken
        auto scatter_for = [&](uint32_t kk, size_t& draws) {
            const uint32_t tape[1] = {kk};
            ref_tape::load(tape, 1);
            cuRandom rng(1984);
            Ray out(glm::vec3(0.0f), glm::vec3(0.0f), 0.0f);
            glm::vec3 att(0.0f);
            die.Scatter(c.ray, rec, rng, out, att);
            draws = ref_tape::pos;
            ref_tape::load(nullptr, 0);
            return out.d;
        };
        size_t draws;
        const glm::vec3 refracted = scatter_for(K_ONE, draws);   // u = 1: `reflect_prob > 1` is false
        if (draws == 0) {
            if (tir < 16) { tir++; run_scatter_any(c, make_tape(), log, in, out); }
            continue;
        }
        if (exact >= 96 || !schlick_power_agrees(c.ray, Sphere::getNormal(c.ray, rec))) continue;
        if (scatter_for(K_ZERO, draws) == refracted) continue;   // reflect_prob <= 0.5: not on the grid
        uint32_t lo = K_ZERO, hi = K_ONE;   // lo reflects, hi refracts
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            (scatter_for(mid, draws) == refracted ? hi : lo) = mid;
        }
        for (uint32_t kk : {hi, hi - 1, hi + 1}) run_scatter_any(c, make_tape({kk}), log, in, out);
        exact++;
    }
    std::printf("G7: %d exact reflect_prob cases, %d TIR cases\n", exact, tir);
    if (exact < 96 || tir < 16) { std::fprintf(stderr, "G7: not enough edge cases found\n"); std::exit(1); }
    write_file(dir + "/ref_core_scatter_in.f32", in);
    write_file(dir + "/ref_core_scatter_out.f32", out);
    write_file(dir + "/ref_core_scatter_idx.u32", log.idx);
    write_file(dir + "/ref_core_scatter_tape.u32", log.tape);
}

// ---------------------------------------------------------------------------------------------------------------------
// G8: PinholeCamera / DefocusBlurCamera / MotionBlurCamera (cu_Cameras.cuh), built from constructor parameters
// cams  [type 0 pinhole / 1 defocus / 2 motion, lookfrom 3, lookat 3, up 3, vfov, aspect, aperture, focus_dist, t0, t1]   16
// state [o 3, u 3, v 3, w 3, viewport_width, viewport_height, lens_radius, focus_dist, t0, t1] — members the class has; 0 else  18
// in    [camera index, s, t]        out [ray o 3, d 3, time, draws]
// ---------------------------------------------------------------------------------------------------------------------
static void gen_camera(const std::string& dir) {
    struct P { int type; glm::vec3 from, at, up; float vfov, aspect, aperture, focus, t0, t1; };
    std::vector<P> ps = {
        {1, {13, 2, 3}, {0, 0, 0}, {0, 1, 0}, 20.0f, 16.0f / 9.0f, 0.1f, 10.0f, 0, 1},   // Book 1's final scene
        {1, {13, 2, 3}, {0, 0, 0}, {0, 1, 0}, 20.0f, 3.0f / 2.0f, 0.1f, 10.0f, 0, 1},
        {0, {13, 2, 3}, {0, 0, 0}, {0, 1, 0}, 20.0f, 16.0f / 9.0f, 0, 0, 0, 1},
        {2, {13, 2, 3}, {0, 0, 0}, {0, 1, 0}, 20.0f, 16.0f / 9.0f, 0, 0, 0.0f, 1.0f},    // Book 2's moving spheres
        {0, {0, 0, 0}, {0, 0, -1}, {0, 1, 0}, 90.0f, 1.0f, 0, 0, 0, 1},
        {0, {278, 278, -800}, {278, 278, 0}, {0, 1, 0}, 40.0f, 1.0f, 0, 0, 0, 1},        // Cornell box
        {1, {-2, 2, 1}, {0, 0, -1}, {0, 1, 0}, 90.0f, 2.0f, 2.0f, 3.4f, 0, 1},
        {1, {3, 3, 2}, {0, 0, -1}, {0, 1, 0}, 1.0f, 0.5f, 0.0f, 5.2f, 0, 1},
        {1, {478, 278, -600}, {278, 278, 0}, {0, 1, 0}, 170.0f, 1.25f, 0.7f, 1.0f, 0, 1},
        {2, {-2, 2, 1}, {0, 0, -1}, {0, 1, 0}, 40.0f, 2.0f, 0, 0, 0.25f, 0.75f},
        {2, {5, -1, 7}, {1, 2, -3}, {0, 0, 1}, 65.0f, 0.75f, 0, 0, 1.0f, 0.0f},
        {0, {5, -1, 7}, {1, 2, -3}, {0.3f, 1, 0.1f}, 120.0f, 1.0f / 3.0f, 0, 0, 0, 1},
    };
    std::vector<float> cams, state, in, out;
    TapeLog log;
    const uint32_t Z = K_ZERO, O = K_ONE;
    const std::vector<std::vector<uint32_t>> lens_prefixes = {
        {Z, Z}, {K_MIN, Z}, {Z, K_MIN}, {O, Z}, {Z, O}, {K_MIN, K_MIN}, {O, O}, {O, K_MIN}, {Z + 1, Z - 1},
        {O, O, O, O, O, O, O, O, O, O, O, O, O, O, O, O, O, O, O, O, O, O},              // 11 rejections, then the stream
        {O, Z, Z, O, K_MIN, Z, Z, K_MIN, O, O, K_MIN, K_MIN, O, K_MIN, K_MIN, O, O, Z, Z, O, K_MIN, Z, Z, K_MIN, Z + 7, Z - 3},
    };
    const std::vector<std::vector<uint32_t>> time_prefixes = {{O}, {K_MIN}, {Z}, {O - 1}, {1u << 22}, {3u << 22}};
    for (size_t ci = 0; ci < ps.size(); ci++) {
        const P& p = ps[ci];
        cams.push_back((float)p.type); put(cams, p.from); put(cams, p.at); put(cams, p.up);
        cams.push_back(p.vfov); cams.push_back(p.aspect); cams.push_back(p.aperture); cams.push_back(p.focus); cams.push_back(p.t0); cams.push_back(p.t1);
        PinholeCamera pin;
        DefocusBlurCamera def;
        MotionBlurCamera mot;
        if (p.type == 0) {
            pin = PinholeCamera(p.from, p.at, p.up, p.vfov, p.aspect);
            put(state, pin.o); put(state, pin.u); put(state, pin.v); put(state, pin.w);
            for (int z = 0; z < 6; z++) state.push_back(0.0f);
        } else if (p.type == 1) {
            def = DefocusBlurCamera(p.from, p.at, p.up, p.vfov, p.aspect, p.aperture, p.focus);
            put(state, def.o); put(state, def.u); put(state, def.v); put(state, def.w);
            state.push_back(def.viewport_width); state.push_back(def.viewport_height); state.push_back(def.lens_radius); state.push_back(def.focus_dist);
            state.push_back(0.0f); state.push_back(0.0f);
        } else {
            mot = MotionBlurCamera(p.from, p.at, p.up, p.vfov, p.aspect, p.t0, p.t1);
            put(state, mot.o); put(state, mot.u); put(state, mot.v); put(state, mot.w);
            for (int z = 0; z < 4; z++) state.push_back(0.0f);
            state.push_back(mot.t0); state.push_back(mot.t1);
        }
        auto sample = [&](float s, float t, const Tape& tape) {
            log.begin(tape);
            cuRandom rng(1984);
            Ray r = p.type == 0 ? pin.sample_ray(s, t) : p.type == 1 ? def.sample_ray(s, t, rng) : mot.sample_ray(s, t, rng);
            const uint32_t draws = log.end(tape);
            in.push_back((float)ci); in.push_back(s); in.push_back(t);
            put_ray(out, r); out.push_back((float)draws);
        };
        for (int k = 0; k < 160; k++) {
            float s = sym(1.0f), t = sym(1.0f);
            if (k % 16 == 1) { s = (float)((int)(next_u32() % 3) - 1); t = (float)((int)(next_u32() % 3) - 1); }   // corners, centre
            if (k % 16 == 2) { s = sym(1.0f) * 1e-30f; t = -0.0f; }
            sample(s, t, make_tape());
        }
        const auto& prefixes = p.type == 1 ? lens_prefixes : p.type == 2 ? time_prefixes : std::vector<std::vector<uint32_t>>{};
        for (const auto& pre : prefixes) sample(sym(1.0f), sym(1.0f), make_tape(pre));
    }
    write_file(dir + "/ref_core_camera_cams.f32", cams);
    write_file(dir + "/ref_core_camera_state.f32", state);
    write_file(dir + "/ref_core_camera_in.f32", in);
    write_file(dir + "/ref_core_camera_out.f32", out);
    write_file(dir + "/ref_core_camera_idx.u32", log.idx);
    write_file(dir + "/ref_core_camera_tape.u32", log.tape);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <out_dir> <natural_tapes.u32>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    load_natural(argv[2]);
    gen_sphere(dir);
    gen_bvh(dir);
    gen_bvh_given(dir);
    gen_scatter(dir);
    gen_camera(dir);
    return 0;
}

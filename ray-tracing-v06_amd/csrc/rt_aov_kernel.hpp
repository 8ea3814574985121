// rt_aov_kernel.hpp — first-hit feature buffers (AOVs) of a refined frame and the edge-aware filter they guide (rt06.h, "Feature buffers
// and denoiser").  Not in the reference.  Nothing here touches render_kernel_stream or the colour path.
#pragma once
#include <hip/hip_runtime.h>

#include "rt06.h"
#include "rt_device_funcs.hpp"
#include "rt_internal.hpp"
#include "rt_layout.hpp"
#include "rt_render_kernels.hpp"
#include "rt_stream_kernel.hpp"

// ---------------------------------------------------------------------------------------------
// Feature buffers.  After a refine pass has been resolved its 48-B primary-ray records (primary_rays_kernel) are still in place: the ray of
// sample (pixel, s) WITH its jitter, lens point and shutter time.  One lane per local pixel walks the pass's samples in sample order — the
// index arithmetic and the coalescing of add_pass_samples: 64 consecutive pixels per sample row — traces each ray ONE bounce through the
// verbatim traversal functions of rt_device_funcs.hpp (the flat world in global memory, so LDS-resident and global-memory renderers share it)
// and continues two fp32 sums per pixel:  aov[2L] = (sum Nx, sum Ny, sum Nz, sum t),  aov[2L + 1] = (sum Ar, sum Ag, sum Ab, hits).
// A hit adds the record's normal as the trace returns it, rec.distance, the first-hit albedo and 1; a miss adds albedo (1,1,1) only.
// The additions are those of ONE step of the same total, whatever the steps were (the contract of the colour accumulation).
// WALK picks the traversal on the host, so that a kernel holds ONE traversal stack: a LaneStack in the LDS (32 entries x 256 lanes x 4 B =
// 32 KiB per workgroup, twice that for the queue's distances), lane-interleaved.  Left to the compiler the stack became a 32-register vector
// whose divergent index is a chain of 32 compares and selects per access: no scratch, but 34 to 94 spilled scalar registers.
// ---------------------------------------------------------------------------------------------
#define RT_AOV_BLOCK 256u
#define RT_AOV_WALK_STACK 0   // RT_WORLD_BVH, BVH.cu:54-106
#define RT_AOV_WALK_LIST 1    // RT_WORLD_LIST
#define RT_AOV_WALK_TREE 2    // RT_WORLD_NODE_TREE
#define RT_AOV_WALK_QUEUE 3   // RT_WORLD_BVH with RT_TRAVERSAL_QUEUE
#define RT_AOV_WALK_WIDE4 4   // RT_WORLD_BVH with RT_TRAVERSAL_WIDE4

template <int WALK, class Keep = KeepAll>
__device__ __forceinline__ bool aov_first_hit(const DeviceWorld& w, const Ray& ray, HitRec& rec, int32_t* lds_i, float* lds_f, Rng* rng = nullptr, Keep keep = Keep()) {
    // modes 0 and 1, no RNG: only a constant medium draws during a trace, and they refuse a world with one; mode RT_AOV_FULL hands in the sample's own (§35),
    // and on the two walks a cutout table is accepted on, the cutout rule
    const LaneStack<int32_t, (int)RT_AOV_BLOCK> si = {lds_i + threadIdx.x};
    const LaneStack<float, (int)RT_AOV_BLOCK> sf = {lds_f + threadIdx.x};
    if (WALK == RT_AOV_WALK_LIST) return list_closest_intersection(w, ray, rec, rng, keep);
    if (WALK == RT_AOV_WALK_TREE) return tree_closest_intersection(w, ray, rec, rng, si);
    if (WALK == RT_AOV_WALK_QUEUE) return bvh_closest_intersection_queue(w, ray, rec, rng, si, sf);
    if (WALK == RT_AOV_WALK_WIDE4) return bvh_closest_intersection_wide4(w, ray, rec, rng, si);
    return bvh_closest_intersection(w, ray, rec, rng, si, keep);
}

// what the first hit looks like without its lighting: Lambertian / metal: albedo; checker: the texture value at the hit point (the shade
// phase's checker_value); dielectric, diffuse light (and a miss): (1,1,1)
__device__ __forceinline__ f3 aov_albedo(const rt_material& m, const Ray& ray, const HitRec& rec) {
    if (m.type == RT_MAT_LAMBERTIAN || m.type == RT_MAT_METAL) return mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
    if (m.type == RT_MAT_LAMBERTIAN_CHECKER)
        return checker_value(mk3(m.albedo[0], m.albedo[1], m.albedo[2]), mk3(m.albedo2[0], m.albedo2[1], m.albedo2[2]), m.param, ray_at(ray, rec.distance));
    return mk3(1.0f);
}
// Mode RT_AOV_TEXTURED: the two textured Lambertians too, restated from the leaf functions the shade phase calls (rt_stream_kernel.hpp, "(u, v) three
// ways"), on the flat world's records — the same floats the packed image holds.  Noise: noise_value at the hit point.  Image: (u, v) of the hit — sphere_uv of the
// OUTWARD normal (the trace returns a sphere's normal unflipped, as the shade phase computes it: a camera inside the sphere sees the same texel), quad_uv on a
// parallelogram, tri_uv with the tail's record on a triangle when a table of texture coordinates is on (uv_at != 0), quad_uv otherwise — then the material's entry
// of the tail's texture table (tex_at != 0; the entry is albedo2[0], the shade phase's fourth material lane) or the world's own image.  tail = the header behind the
// image the colour pass launches on: (-, uv_at, -, tex_at), wave-uniform.  A launch whose materials name an entry the renderer lacks is refused before any kernel.
__device__ __forceinline__ f3 aov_albedo_tex(const DeviceWorld& w, const uint4* tail, uint32_t uv_at, uint32_t tex_at, uint32_t first_tri, const rt_material& m,
                                             const Ray& ray, const HitRec& rec) {
    if (m.type == RT_MAT_LAMBERTIAN_NOISE) return noise_value(w.perlin, mk3(m.albedo[0], m.albedo[1], m.albedo[2]), m.param, ray_at(ray, rec.distance));
    if (m.type != RT_MAT_LAMBERTIAN_IMAGE) return aov_albedo(m, ray, rec);
    float tu, tv;
    if ((uint32_t)rec.prim >= w.n_prims) {
        const rt_quad& q = w.quads[(uint32_t)rec.prim - w.n_prims];
        const f3 hit_p = ray_at(ray, rec.distance);
        if (uv_at != 0u && (uint32_t)rec.prim >= first_tri) {
            const float* tr = reinterpret_cast<const float*>(tail + uv_at) + (size_t)((uint32_t)rec.prim - first_tri) * 6u;
            const float t0[2] = {tr[0], tr[1]}, t1[2] = {tr[2], tr[3]}, t2[2] = {tr[4], tr[5]};
            tri_uv(ld3(q.Q), ld3(q.u), ld3(q.v), ld3(q.w), t0, t1, t2, hit_p, tu, tv);
        } else
        quad_uv(ld3(q.Q), ld3(q.u), ld3(q.v), ld3(q.w), hit_p, tu, tv);
    } else {
        sphere_uv(rec.normal, tu, tv);
    }
    if (tex_at != 0u) return texture_table_value(tail + tex_at, (uint32_t)m.albedo2[0], tu, tv);
    return image_texel(w.image, w.image_w, w.image_h, tu, tv);
}

// Normal maps (aov_kernel_nmap): the first hit's normal is the mapped one, as the shade phase of an NMAP kernel forms it — the material's record of
// the table behind the texture table (tail + tex_at, whose header's fourth lane says where), (u, v) and the tangents by the kind of surface, then normal_map_apply
// on rec.normal, which is the flat or the smooth normal by now.
__device__ __forceinline__ void aov_normal_map(const DeviceWorld& w, const uint4* tail, uint32_t uv_at, uint32_t tex_at, uint32_t first_tri, const Ray& ray, HitRec& rec) {
    if (tex_at == 0u) return;
    const uint4* tt = tail + tex_at;
    const uint4 th = tt[0];
    const uint32_t nm_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)th.w);
    if (nm_at == 0u) return;
    const uint4 nr = tt[nm_at + rec.mat];
    if (nr.x == 0u) return;
    float tu, tv;
    f3 dPdu, dPdv;
    if ((uint32_t)rec.prim >= w.n_prims) {
        const rt_quad& q = w.quads[(uint32_t)rec.prim - w.n_prims];
        const f3 hit_p = ray_at(ray, rec.distance);
        if (uv_at != 0u && (uint32_t)rec.prim >= first_tri) {
            const float* tr = reinterpret_cast<const float*>(tail + uv_at) + (size_t)((uint32_t)rec.prim - first_tri) * 6u;
            const float t0[2] = {tr[0], tr[1]}, t1[2] = {tr[2], tr[3]}, t2[2] = {tr[4], tr[5]};
            tri_uv(ld3(q.Q), ld3(q.u), ld3(q.v), ld3(q.w), t0, t1, t2, hit_p, tu, tv);
            if (!normal_map_tri_tangents(ld3(q.u), ld3(q.v), t0, t1, t2, dPdu, dPdv)) return;
        } else {
            quad_uv(ld3(q.Q), ld3(q.u), ld3(q.v), ld3(q.w), hit_p, tu, tv);
            dPdu = ld3(q.u); dPdv = ld3(q.v);
        }
    } else {
        sphere_uv(rec.normal, tu, tv);
        normal_map_sphere_tangents(rec.normal, dPdu, dPdv);
    }
    const uint64_t texels = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.y) << 32;
    normal_map_apply(texture_value(reinterpret_cast<const uint32_t*>(texels), tt[1u + nr.y], tu, tv), __uint_as_float(nr.z), dPdu, dPdv, ray.d, rec.normal);
}

// Mode RT_AOV_FULL, the Keep of its list and stack walks: the leaf phase of the CUT kernels (rt_stream_kernel.hpp) on the flat world's records.  A
// parallelogram or triangle that has passed its test, on a material whose cutout record is on, is there iff cutout_keeps says so — the mask's entry of the texture
// table at the candidate's own (u, v): the triangle's record of the table of texture coordinates while there is one, the planar coordinates otherwise.
// cut_at = the sub-header's third lane, the vec4 from the tail's header to the records, 0 without a table (wave-uniform, like uv_at and tex_at).
struct AovCutoutKeep {
    const uint4* tail;
    uint32_t uv_at, tex_at, cut_at, first_tri;
    __device__ __forceinline__ bool operator()(const rt_quad& q, int32_t idx, const Ray& ray, float t) const {
        if (cut_at == 0u || tex_at == 0u) return true;   // (the host launches no record without its table entry)
        const uint4 cut_rec = tail[cut_at + q.mat];      // (on, image, cutoff bits, -)
        if (cut_rec.x == 0u) return true;
        const uint4* tt = tail + tex_at;
        const uint4 th = tt[0];
        const uint64_t texels = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.y) << 32;
        const float* tr = nullptr;
        if (uv_at != 0u && (uint32_t)idx >= first_tri) tr = reinterpret_cast<const float*>(tail + uv_at) + (size_t)((uint32_t)idx - first_tri) * 6u;
        float cut_u, cut_v;
        f3 cut_c;
        return cutout_keeps(reinterpret_cast<const uint32_t*>(texels), tt[1u + cut_rec.y], __uint_as_float(cut_rec.z), ld3(q.Q), ld3(q.u), ld3(q.v), ld3(q.w), tr, ray, t,
                            cut_u, cut_v, cut_c);
    }
};

// what the feature pass reads of a refine pass (a StreamParams would occupy scalar registers the traversal needs)
struct AovParams {
    TileMap tm;
    DeviceWorld world;
    uint32_t pass_first_s, pass_spp;   // as in StreamParams: the records of sample s_local of local pixel L are at (L >> 6) * pass_spp * 64 + s_local * 64 + (L & 63)
    uint32_t n_take;                   // how many of the pass's samples, from its first, are covered (max_samples may end inside a pass)
    const float4* prim_o;
    const float4* prim_d;
};

// SMOOTH (aov_kernel_smooth): a hit on a triangle — unified index >= first_tri — takes its normal through shading_normal() from the table's record
// TEX (aov_kernel_tex / aov_kernel_smooth_tex): the albedo is aov_albedo_tex's; tail = the header of the image's tail, first_tri as above
// NMAP (aov_kernel_nmap): TEX, and the normal goes through aov_normal_map behind the smooth rule; vn may be null (no table of vertex normals)
// FULL (aov_kernel_full): TEX, and the trace is the colour path's first trace — the lane's Rng starts from the sample's record in prim_rng, as
//      render_kernel_stream starts a sample, and goes to the walk, so that a constant medium draws what it drew there; with `cutouts` the list and stack walks put
//      their candidates to the cutout rule; a first hit inside a medium adds the trace's normal (1, 0, 0), its distance, 1 and the isotropic material's albedo
template <int WALK, bool SMOOTH, bool TEX = false, bool NMAP = false, bool FULL = false>
__device__ __forceinline__ void aov_body(const AovParams& p, float4* __restrict__ aov, int32_t* lds_i, float* lds_f, const rt_tri_normals* vn, uint32_t first_tri,
                                         const uint4* tail = nullptr, [[maybe_unused]] const uint4* prim_rng = nullptr, [[maybe_unused]] uint32_t cutouts = 0u) {
    const uint32_t L = blockIdx.x * RT_AOV_BLOCK + threadIdx.x;
    if (L >= p.tm.n_local_tiles * RT_TILE * RT_TILE) return;
    uint32_t gid;
    if (!local_pixel_to_gid(p.tm, L, gid)) return;   // padding pixels have no record (and read as zeros: the buffer is cleared at enable)
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.pass_first_s != 0u) { g = aov[2u * L]; a = aov[2u * L + 1u]; }
    size_t src = (size_t)(L >> 6) * p.pass_spp * 64u + (L & 63u);
    uint32_t uv_at = 0u, tex_at = 0u;
    if constexpr (TEX) {   // the tail header's second and fourth words: the same for every lane
        const uint4 th = tail[0];
        uv_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)th.y); tex_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)th.w);
    }
    [[maybe_unused]] AovCutoutKeep keep = {tail, uv_at, tex_at, 0u, first_tri};
    if constexpr (FULL && (WALK == RT_AOV_WALK_LIST || WALK == RT_AOV_WALK_STACK)) {
        if (cutouts) {   // only a tail with cutout records is known to have the sub-header (rt_launch_image.hpp): the header's first lane counts the vec4 to it
            const uint32_t sub_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)tail[0].x) >> 1;
            if (sub_at != 0u) keep.cut_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)tail[sub_at].z);
        }
    }
    for (uint32_t s = 0; s < p.n_take; s++) {
        const float4 o = p.prim_o[src], d = p.prim_d[src];
        Ray ray;
        ray.o = mk3(o.x, o.y, o.z); ray.d = mk3(d.x, d.y, d.z); ray.time = o.w;
        HitRec rec;
        rec.distance = RT_MISS_DIST; rec.normal = mk3(0.0f); rec.prim = -1; rec.mat = 0;   // as sample_world starts a trace
        f3 alb = mk3(1.0f);
        bool hit;
        if constexpr (FULL) {
            const uint4 rs = prim_rng[src];
            Rng rng;
            rng.s0 = rs.x; rng.s1 = rs.y; rng.s2 = rs.z; rng.s3 = rs.w; rng.draws = 0u;
            if constexpr (WALK == RT_AOV_WALK_LIST || WALK == RT_AOV_WALK_STACK) hit = aov_first_hit<WALK>(p.world, ray, rec, lds_i, lds_f, &rng, keep);
            else hit = aov_first_hit<WALK>(p.world, ray, rec, lds_i, lds_f, &rng);
        } else
        hit = aov_first_hit<WALK>(p.world, ray, rec, lds_i, lds_f);
        if (hit) {
            if (FULL && p.world.mats[rec.mat].type == RT_MAT_ISOTROPIC) { const rt_material& m = p.world.mats[rec.mat]; alb = mk3(m.albedo[0], m.albedo[1], m.albedo[2]); }
            else if constexpr (TEX) alb = aov_albedo_tex(p.world, tail, uv_at, tex_at, first_tri, p.world.mats[rec.mat], ray, rec);
            else alb = aov_albedo(p.world.mats[rec.mat], ray, rec);
            if (SMOOTH && (!NMAP || vn) && (uint32_t)rec.prim >= first_tri) shading_normal_flat(p.world.quads[(uint32_t)rec.prim - p.world.n_prims], vn[(uint32_t)rec.prim - first_tri], ray, rec.distance, rec.normal);
            if constexpr (NMAP) aov_normal_map(p.world, tail, uv_at, tex_at, first_tri, ray, rec);
            g.x += rec.normal.x; g.y += rec.normal.y; g.z += rec.normal.z; g.w += rec.distance;
            a.w += 1.0f;
        }
        a.x += alb.x; a.y += alb.y; a.z += alb.z;
        src += 64u;
    }
    aov[2u * L] = g;
    aov[2u * L + 1u] = a;
}
template <int WALK>
__global__ __launch_bounds__(RT_AOV_BLOCK) void aov_kernel(AovParams p, float4* __restrict__ aov) {
    __shared__ int32_t lds_i[WALK == RT_AOV_WALK_LIST ? 1u : RT_MAX_STACK * RT_AOV_BLOCK];
    __shared__ float lds_f[WALK == RT_AOV_WALK_QUEUE ? RT_MAX_STACK * RT_AOV_BLOCK : 1u];
    aov_body<WALK, false>(p, aov, lds_i, lds_f, nullptr, 0u);
}
// the same pass with a table of vertex normals on (lists and stack-walked BVHs: what rt_renderer_shading_normals accepts)
template <int WALK>
__global__ __launch_bounds__(RT_AOV_BLOCK) void aov_kernel_smooth(AovParams p, float4* __restrict__ aov, const rt_tri_normals* __restrict__ vn, uint32_t first_tri) {
    static_assert(WALK == RT_AOV_WALK_LIST || WALK == RT_AOV_WALK_STACK, "vertex normals: lists and stack-walked BVHs");
    __shared__ int32_t lds_i[WALK == RT_AOV_WALK_LIST ? 1u : RT_MAX_STACK * RT_AOV_BLOCK];
    __shared__ float lds_f[1u];
    aov_body<WALK, true>(p, aov, lds_i, lds_f, vn, first_tri);
}
// mode RT_AOV_TEXTURED: the same passes with aov_albedo_tex.  What they need beyond AovParams — the tail's header and the first triangle's unified index — are
// arguments of these kernels only (the Perlin tables and the world's own image are in AovParams' DeviceWorld already), so the plain forms' parameter block is as it was.
template <int WALK>
__global__ __launch_bounds__(RT_AOV_BLOCK) void aov_kernel_tex(AovParams p, float4* __restrict__ aov, const uint4* __restrict__ blob, uint32_t blob_vec4, uint32_t first_tri) {
    __shared__ int32_t lds_i[WALK == RT_AOV_WALK_LIST ? 1u : RT_MAX_STACK * RT_AOV_BLOCK];
    __shared__ float lds_f[WALK == RT_AOV_WALK_QUEUE ? RT_MAX_STACK * RT_AOV_BLOCK : 1u];
    aov_body<WALK, false, true>(p, aov, lds_i, lds_f, nullptr, first_tri, blob + blob_vec4);
}
template <int WALK>
__global__ __launch_bounds__(RT_AOV_BLOCK) void aov_kernel_smooth_tex(AovParams p, float4* __restrict__ aov, const rt_tri_normals* __restrict__ vn, const uint4* __restrict__ blob,
                                                                      uint32_t blob_vec4, uint32_t first_tri) {
    static_assert(WALK == RT_AOV_WALK_LIST || WALK == RT_AOV_WALK_STACK, "vertex normals: lists and stack-walked BVHs");
    __shared__ int32_t lds_i[WALK == RT_AOV_WALK_LIST ? 1u : RT_MAX_STACK * RT_AOV_BLOCK];
    __shared__ float lds_f[1u];
    aov_body<WALK, true, true>(p, aov, lds_i, lds_f, vn, first_tri, blob + blob_vec4);
}

// mode RT_AOV_TEXTURED of a renderer with a normal-map table: aov_kernel_smooth_tex with the mapped normal; vn = the table of vertex normals or null
template <int WALK>
__global__ __launch_bounds__(RT_AOV_BLOCK) void aov_kernel_nmap(AovParams p, float4* __restrict__ aov, const rt_tri_normals* __restrict__ vn, const uint4* __restrict__ blob,
                                                                uint32_t blob_vec4, uint32_t first_tri) {
    static_assert(WALK == RT_AOV_WALK_LIST || WALK == RT_AOV_WALK_STACK, "normal maps: lists and stack-walked BVHs");
    __shared__ int32_t lds_i[WALK == RT_AOV_WALK_LIST ? 1u : RT_MAX_STACK * RT_AOV_BLOCK];
    __shared__ float lds_f[1u];
    aov_body<WALK, true, true, true>(p, aov, lds_i, lds_f, vn, first_tri, blob + blob_vec4);
}

// mode RT_AOV_FULL: one family for the five walks.  Lists and stack-walked BVHs — what a cutout table, vertex normals and a normal map are accepted
// on — carry the cutout rule and aov_kernel_nmap's normals (vn may be null); the other three walks carry the RNG only.  prim_rng = the pass's RNG records
// (StreamParams::prim_rng), cutouts = whether the renderer has a cutout table: arguments of these kernels alone.
template <int WALK>
__global__ __launch_bounds__(RT_AOV_BLOCK) void aov_kernel_full(AovParams p, float4* __restrict__ aov, const uint4* __restrict__ prim_rng, const rt_tri_normals* __restrict__ vn,
                                                                const uint4* __restrict__ blob, uint32_t blob_vec4, uint32_t first_tri, uint32_t cutouts) {
    __shared__ int32_t lds_i[WALK == RT_AOV_WALK_LIST ? 1u : RT_MAX_STACK * RT_AOV_BLOCK];
    __shared__ float lds_f[WALK == RT_AOV_WALK_QUEUE ? RT_MAX_STACK * RT_AOV_BLOCK : 1u];
    constexpr bool FLAT = WALK == RT_AOV_WALK_LIST || WALK == RT_AOV_WALK_STACK;
    aov_body<WALK, FLAT, true, FLAT, true>(p, aov, lds_i, lds_f, vn, first_tri, blob + blob_vec4, prim_rng, cutouts);
}

// ---------------------------------------------------------------------------------------------
// Denoiser: a variance-guided a-trous wavelet filter over the refined frame, guided by the feature buffers.  fp32 + - * / sqrt, min / max as
// comparisons, every operation rounded on its own (the library is built without contraction and with correctly rounded / and sqrt), a
// fixed tap order: numpy float32 restates it bit for bit (tests/test_gpu_denoise.py).  Image space is row-major like the framebuffer
// (world_size == 1).  Per pixel: guide records g0 = (mean N, mean Z), g1 = (max(mean A, 1e-3), -) and a colour record (I, v): the
// illumination and the variance of its mean luminance.
// ---------------------------------------------------------------------------------------------
struct DenoiseParams {
    uint32_t width, height;
    float sigma_depth, sigma_lum;
    uint32_t demodulate;
};

__device__ __forceinline__ float dn_max(float a, float b) { return a < b ? b : a; }   // glm::max: a NaN in b is dropped, a NaN in a kept
__device__ __forceinline__ float dn_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float dn_luma(float r, float g, float b) {
    return __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, r), __fmul_rn(0.7152f, g)), __fmul_rn(0.0722f, b));
}
__device__ __forceinline__ bool dn_finite(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(c.w); }

// prepare: n colour samples in `acc` (sum R, sum G, sum B, sum Y^2), na feature samples in `aov`, both per LOCAL pixel
__global__ __launch_bounds__(256) void denoise_prepare_kernel(TileMap tm, DenoiseParams dp, const float4* __restrict__ acc, const float4* __restrict__ aov,
                                                              uint32_t n, uint32_t na, float4* __restrict__ g0, float4* __restrict__ g1, float4* __restrict__ col) {
    const uint32_t L = blockIdx.x * 256u + threadIdx.x;
    if (L >= tm.n_local_tiles * RT_TILE * RT_TILE) return;
    uint32_t gid;
    if (!local_pixel_to_gid(tm, L, gid)) return;
    const float4 s = acc[L], sn = aov[2u * L], sa = aov[2u * L + 1u];
    const float inv_n = 1.0f / (float)n, inv_na = 1.0f / (float)na;
    const float cr = __fmul_rn(s.x, inv_n), cg = __fmul_rn(s.y, inv_n), cb = __fmul_rn(s.z, inv_n);   // resolve_pixel's mean
    const float ar = dn_max(__fmul_rn(sa.x, inv_na), 1e-3f), ag = dn_max(__fmul_rn(sa.y, inv_na), 1e-3f), ab = dn_max(__fmul_rn(sa.z, inv_na), 1e-3f);
    float m, v;
    mean_luminance_variance(s, n, m, v);
    float ir = cr, ig = cg, ib = cb;
    if (dp.demodulate) {
        ir = __fdiv_rn(cr, ar); ig = __fdiv_rn(cg, ag); ib = __fdiv_rn(cb, ab);
        const float ya = dn_max(dn_luma(ar, ag, ab), 1e-3f);
        v = __fdiv_rn(v, __fmul_rn(ya, ya));
    }
    g0[gid] = make_float4(__fmul_rn(sn.x, inv_na), __fmul_rn(sn.y, inv_na), __fmul_rn(sn.z, inv_na), __fmul_rn(sn.w, inv_na));
    g1[gid] = make_float4(ar, ag, ab, 0.0f);
    col[gid] = make_float4(ir, ig, ib, v);
}

// B3-spline taps h = (1/16, 1/4, 3/8, 1/4, 1/16); every product h(dx) * h(dy) is exact in fp32
__device__ __forceinline__ float dn_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// One pixel of one iteration.  fetch(qx, qy, c, g) reads the colour and the first guide record of an in-image pixel (LDS tile or global).
//   centre: weight h(0)^2, no edge stopping; a centre that is not finite is copied through.
//   tap q:  w = ((h(dx) h(dy) * wn) * wz) * wl;  outside the image or not finite: left out.
//     wn = max(0, dot(Np, Nq)) squared five times
//     wz = 1 / (1 + dz * dz),  dz = |Zp - Zq| / ((sigma_depth * (float)step) * min(Zp, Zq) + 1e-6)
//     wl = 1 / (1 + dl * dl),  dl = |Y(Ip) - Y(Iq)| / (sigma_lum * sqrt(max(vp, 0)) + 1e-6)
//   I' = sum(w Iq) / sum(w),  v' = sum(w^2 vq) / (sum w)^2, sums sequential in row-major tap order (dy, then dx, from -2 to 2).
template <class Fetch>
__device__ __forceinline__ float4 denoise_filter_pixel(const DenoiseParams& dp, int x, int y, int step, Fetch fetch) {
    float4 cp, gp;
    fetch(x, y, cp, gp);
    if (!dn_finite(cp)) return cp;
    const float yp = dn_luma(cp.x, cp.y, cp.z);
    // sqrtf, not __fsqrt_rn: the build's correctly rounded square root (the intrinsic maps to the native, approximate one)
    const float den_l = __fadd_rn(__fmul_rn(dp.sigma_lum, sqrtf(dn_max(cp.w, 0.0f))), 1e-6f);
    const float sz = __fmul_rn(dp.sigma_depth, (float)step);
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step, qy = y + dy * step;
            float w;
            float4 cq = cp, gq;
            if (dx == 0 && dy == 0) {
                w = 0.140625f;
            } else {
                if ((uint32_t)qx >= dp.width || (uint32_t)qy >= dp.height) continue;
                fetch(qx, qy, cq, gq);
                if (!dn_finite(cq)) continue;
                float wn = dn_max(0.0f, __fadd_rn(__fadd_rn(__fmul_rn(gp.x, gq.x), __fmul_rn(gp.y, gq.y)), __fmul_rn(gp.z, gq.z)));
                wn = __fmul_rn(wn, wn); wn = __fmul_rn(wn, wn); wn = __fmul_rn(wn, wn); wn = __fmul_rn(wn, wn); wn = __fmul_rn(wn, wn);
                const float dz = __fdiv_rn(fabsf(__fsub_rn(gp.w, gq.w)), __fadd_rn(__fmul_rn(sz, dn_min(gp.w, gq.w)), 1e-6f));
                const float wz = __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(dz, dz)));
                const float dl = __fdiv_rn(fabsf(__fsub_rn(yp, dn_luma(cq.x, cq.y, cq.z))), den_l);
                const float wl = __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(dl, dl)));
                w = __fmul_rn(__fmul_rn(__fmul_rn(__fmul_rn(dn_h(dx), dn_h(dy)), wn), wz), wl);
            }
            sw = __fadd_rn(sw, w);
            sr = __fadd_rn(sr, __fmul_rn(w, cq.x)); sg = __fadd_rn(sg, __fmul_rn(w, cq.y)); sb = __fadd_rn(sb, __fmul_rn(w, cq.z));
            sv = __fadd_rn(sv, __fmul_rn(__fmul_rn(w, w), cq.w));
        }
    }
    return make_float4(__fdiv_rn(sr, sw), __fdiv_rn(sg, sw), __fdiv_rn(sb, sw), __fdiv_rn(sv, __fmul_rn(sw, sw)));
}

// Steps 1 and 2: the 25 taps of neighbouring pixels overlap almost entirely, so a workgroup stages its 16x16 tile plus a halo of 2 * STEP
// pixels in the LDS once — (16 + 4 STEP)^2 entries of 32 B: 12.5 KiB at step 1, 18 KiB at step 2 — and every tap is a ds_read_b128.
#define RT_DN_TILE 16
template <int STEP>
__global__ __launch_bounds__(RT_DN_TILE * RT_DN_TILE) void denoise_filter_tile_kernel(DenoiseParams dp, const float4* __restrict__ g0, const float4* __restrict__ in, float4* __restrict__ out) {
    constexpr int HALO = 2 * STEP, SIDE = RT_DN_TILE + 2 * HALO;
    __shared__ float4 t_col[SIDE * SIDE], t_g0[SIDE * SIDE];
    const int x0 = (int)blockIdx.x * RT_DN_TILE - HALO, y0 = (int)blockIdx.y * RT_DN_TILE - HALO;
    for (int e = (int)threadIdx.x; e < SIDE * SIDE; e += RT_DN_TILE * RT_DN_TILE) {
        const int qx = x0 + e % SIDE, qy = y0 + e / SIDE;
        const bool inside = (uint32_t)qx < dp.width && (uint32_t)qy < dp.height;   // an entry outside the image is never read back
        const size_t q = (size_t)qy * dp.width + (size_t)qx;
        t_col[e] = inside ? in[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        t_g0[e] = inside ? g0[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const int x = (int)blockIdx.x * RT_DN_TILE + (int)(threadIdx.x % RT_DN_TILE), y = (int)blockIdx.y * RT_DN_TILE + (int)(threadIdx.x / RT_DN_TILE);
    if ((uint32_t)x >= dp.width || (uint32_t)y >= dp.height) return;
    out[(size_t)y * dp.width + x] = denoise_filter_pixel(dp, x, y, STEP, [&](int qx, int qy, float4& c, float4& g) {
        const int e = (qy - y0) * SIDE + (qx - x0);
        c = t_col[e]; g = t_g0[e];
    });
}
// Steps >= 4: the taps of neighbouring pixels no longer overlap inside a tile a workgroup could stage (the halo alone would be 8 * step
// pixels wide), so each lane reads its 25 strided taps from global memory; a wave's 64 lanes still read 4 rows of 16 consecutive records.
__global__ __launch_bounds__(RT_DN_TILE * RT_DN_TILE) void denoise_filter_direct_kernel(DenoiseParams dp, int step, const float4* __restrict__ g0, const float4* __restrict__ in, float4* __restrict__ out) {
    const int x = (int)blockIdx.x * RT_DN_TILE + (int)(threadIdx.x % RT_DN_TILE), y = (int)blockIdx.y * RT_DN_TILE + (int)(threadIdx.x / RT_DN_TILE);
    if ((uint32_t)x >= dp.width || (uint32_t)y >= dp.height) return;
    out[(size_t)y * dp.width + x] = denoise_filter_pixel(dp, x, y, step, [&](int qx, int qy, float4& c, float4& g) {
        const size_t q = (size_t)qy * dp.width + (size_t)qx;
        c = in[q]; g = g0[q];
    });
}

// final: remodulate, clamp, sqrt-gamma, alpha = 1 (the framebuffer's conventions)
__global__ __launch_bounds__(256) void denoise_final_kernel(DenoiseParams dp, const float4* __restrict__ g1, const float4* __restrict__ col, float4* __restrict__ out) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= dp.width * dp.height) return;
    const float4 c = col[gid], a = g1[gid];
    f3 rad = mk3(c.x, c.y, c.z);
    if (dp.demodulate) rad = mk3(__fmul_rn(c.x, a.x), __fmul_rn(c.y, a.y), __fmul_rn(c.z, a.z));
    const f3 o = clamp01_sqrt(rad);
    out[gid] = make_float4(o.x, o.y, o.z, 1.0f);
}

// rt_stream_kernel.hpp — the production render path: a persistent, sample-streaming wavefront kernel
// with the whole BVH resident in LDS, plus the in-order resolve kernel.
//
// Reference shape (main/src/Renderer.cu:183-217): one thread per PIXEL, serial spp loop, 48 B of RNG
// state per pixel in global memory, two virtual calls per bounce, BVH nodes fetched from global memory
// by pointer.  MI355X shape:
//
//  * one work-item owns one pixel-SAMPLE.  The rank's samples of a pass form one linear index space
//    n = (block * pass_spp + s) * 64 + pixel-in-block (a block = the 64 pixels of an 8x8 tile), so the
//    64 lanes of a wavefront mostly hold one sample each of the 64 pixels of a tile (coherent primary
//    rays) and n is also the slot of the sample in the HBM sample buffer.  Waves are persistent: each pulls chunks of
//    `chunk` (<= 1024) consecutive sample indices from one global counter and hands them to its lanes with a
//    ballot + prefix popcount the moment a lane's path ends (sample regeneration), so path-length
//    divergence (1..50 bounces) does not idle lanes.
//  * the lane program is the reference's: primary ray, then trace / scatter per bounce with
//    BVH::ClosestIntersection's exact order of box tests, culling and pushes.  What is re-scheduled is
//    only WHICH lanes run WHICH phase together: the wave runs "inner node" steps while most lanes sit at
//    an inner node, services lanes that reached a leaf or finished a trace when enough have piled up
//    (wave ballots), and never lets one lane's long traversal hold 63 finished ones.
//  * the scene is staged once per workgroup into LDS (coalesced 16-B loads of one packed blob): 76-B
//    "wide" inner nodes that carry BOTH child boxes as (min, max, min) triples and both child references (so a visit
//    is one address and leaves need no node fetch at all; the triples turn the slab test's per-axis min/max into a
//    per-ray address offset), 16-B sphere records and 16-B (centre1, material) records.  The per-lane traversal stack
//    lives in LDS too, sized from the tree's depth.  Worlds that do not fit keep their records in global memory / L2
//    (BIG instantiation, 32-bit references).
//  * gfx950 issues fp32 add/mul/fma and simple integer ops in 2 cycles per wave, compares / selects / min / max in 4,
//    and scalar instructions are NOT hidden behind the vector issue (tools/bench_valu_issue.hip): the hot loop is
//    straight-line code built from the cheap class, one compare per phase test, exact division without dividing.
//  * the counter-based RNG keeps no state in memory; every sample writes its radiance (12 B) to an HBM
//    sample buffer laid out [pixel-block][sample][64 pixels], and `resolve_kernel` adds them IN SAMPLE
//    ORDER per pixel — the same order as the reference's `radiance +=` loop — so the framebuffer is
//    bit-identical to the CPU oracle's, and independent of scheduling and of the number of GPUs.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "rt06.h"
#include "rt_device_funcs.hpp"
#include "rt_fastdiv.hpp"
#include "rt_internal.hpp"
#include "rt_layout.hpp"
#include "rt_render_kernels.hpp"

#define RT_WORLD_BVH_QUEUE 3     // internal WORLD mode of render_kernel_stream: an RT_WORLD_BVH world walked by each lane on its own — the distance-sorted queue (RT_TRAVERSAL_QUEUE) or the 4-wide walk (RT_TRAVERSAL_WIDE4)
#define RT_CHUNK_MAX 768u        // sample indices a wave pulls per atomic (the host shrinks it for small frames / shards); 768 measured 0.35 ms ahead of 1024 and of 512 on config 2
// scheduling thresholds (lanes of 64); overridable per renderer for tuning (RT06_TUNE=keep,shade,leaf[,drop,floor])
#define RT_INNER_KEEP 36         // keep iterating inner-node steps while at least this many lanes want one (round 4, with the cheaper hot step: 36 / 52 / 4 is 0.3-1.2 % ahead of 40 / 56 / 4 on all four workloads)
#define RT_SHADE_MIN 52          // run the shade/regenerate phase once this many lanes wait for it
#define RT_LEAF_MIN 4            // run the leaf phase once this many lanes sit at a leaf (or nobody is at an inner node)
// ... and the node loop's exit relative to the lane count it was entered with (node_loop_keep).  0 / 64 is the fixed rule "fewer than inner_keep": the floor never
// lies below inner_keep, so the minimum is inner_keep whatever the entry count.
#define RT_INNER_DROP 0          // leave the node loop once this many of the lanes it was entered with have left their inner nodes ...
#define RT_INNER_FLOOR 64        // ... but never ask for fewer than this many lanes (nor for more than inner_keep)
// what variant 3's hot loop runs with (EXPERIMENTS.md E18: 36 / 52 / 4 / 16 / 8 is 2.2-4.3 % ahead of the fixed rule on all four workloads; the sweep is flat from
// drop 12 to 24 and floor 8 to 12, and loses half of the gain at floor 24)
#define RT_INNER_DROP_HOT 16
#define RT_INNER_FLOOR_HOT 8

// A primary-ray record is read exactly once: a non-temporal load, so that this 23 GB stream does not push the partially written lines of
// the sample buffer out of the L2 before their neighbours arrive.  Measured (config 2, round 3): HBM write traffic of the kernel
// 9.79 GB -> 6.63 GB for 5.76 GB of samples (1.70x -> 1.15x), same time (EXPERIMENTS.md).
typedef float rt_nt_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t rt_nt_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 rt_load_once(const float4* p) {
    const rt_nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const rt_nt_f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 rt_load_once(const uint4* p) {
    const rt_nt_u4 v = __builtin_nontemporal_load(reinterpret_cast<const rt_nt_u4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
#define RT_LOAD_ONCE(ptr) rt_load_once(ptr)
// The generator's stores and the resolve kernel's loads are streams too (written once / read once): non-temporal, -0.13 ms per config-2 frame
// (primary 4.03 -> 3.94 ms, resolve 0.99 -> 0.95 ms).
typedef float rt_nts_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t rt_nts_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void rt_store_stream(float4* p, float4 v) { rt_nts_f4 w = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(w, reinterpret_cast<rt_nts_f4*>(p)); }
__device__ __forceinline__ void rt_store_stream(uint4* p, uint4 v) { rt_nts_u4 w = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(w, reinterpret_cast<rt_nts_u4*>(p)); }
__device__ __forceinline__ float rt_load_stream(const float* p) { return __builtin_nontemporal_load(p); }

#define RT_SAMPLE_BYTES 12u
__device__ __forceinline__ void store_sample(float4* samples, uint32_t n, float x, float y, float z) {
    float* o = reinterpret_cast<float*>(samples) + (size_t)n * 3u;
    o[0] = x; o[1] = y; o[2] = z;
}
__device__ __forceinline__ f3 load_sample(const float4* samples, size_t n) {
    const float* q = reinterpret_cast<const float*>(samples) + n * 3u;
    return mk3(rt_load_stream(q), rt_load_stream(q + 1), rt_load_stream(q + 2));
}

struct StreamParams {
    uint32_t width, height, spp, max_depth;
    uint64_t seed;
    rt_camera cam;
    TileMap tm;
    PackedSceneRef scene;
    uint32_t pass_first_s;   // first sample index of this pass
    uint32_t pass_spp;       // samples per pixel in this pass
    uint32_t total;          // n_local_pixels * pass_spp
    uint32_t inner_keep, shade_min, leaf_min;
    uint32_t inner_drop, inner_floor;   // the node loop's exit, relative to its entry lane count: node_loop_keep()
    uint32_t chunk;          // sample indices per work-queue fetch
    float4* samples;         // [n_local_pixels/64][pass_spp][64] radiance, RT_SAMPLE_BYTES = 12 bytes per sample index n (one global_store_dwordx3;
                             // 16-byte slots were measured slower and MORE HBM write traffic: EXPERIMENTS.md)
    // primary rays of the pass, written by primary_rays_kernel and consumed by sample regeneration, indexed by n:
    float4* prim_o;          // (ray origin, ray time)
    float4* prim_d;          // (ray direction, -)
    uint4* prim_rng;         // the sample's RNG state after the camera's draws; all zero (never a valid state) marks a padding pixel
    uint32_t* work_counter;
    DeviceWorld world;       // WORLD == RT_WORLD_BVH_QUEUE only: the flat world as BVH::ClosestIntersection's queue walk reads it (BVH.cu:17-49, :80-86)
#ifdef RT_PHASE_TIMERS
    unsigned long long* phase_acc;  // development build only: [0..15] cycles per phase, [16..31] visits (summed over waves)
#endif
};

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The node loop runs on while at least this many lanes want an inner-node step, for a loop entered with `n_entry` such lanes: the loop is left once
// inner_drop of them have gone elsewhere, but the threshold stays within [inner_floor, inner_keep].  A wave that enters with few inner lanes late in a
// shade period then stays for more than the one step a fixed threshold gives it, and one that enters full leaves for a leaf round before it has thinned
// to the fixed threshold.  Scheduling only: which lane takes which step of which trace does not depend on it.  All operands are wave-uniform.
__device__ __forceinline__ uint32_t node_loop_keep(const StreamParams& p, uint32_t n_entry) {
    // (signed: all three are at most 64, and inner_floor >= 1 takes care of a negative difference.  An unsigned saturating difference, however it is spelt,
    // has no scalar instruction, and the compiler moves the whole chain to the vector unit for it)
    return (uint32_t)min((int)p.inner_keep, max((int)p.inner_floor, (int)n_entry - (int)p.inner_drop));
}

// pixel origin of the 8x8 tile that local 64-pixel block `blk` covers; false for a padding block
__device__ __forceinline__ bool block_origin(const TileMap& tm, uint32_t blk, uint32_t& x0, uint32_t& y0) {
    uint32_t gt = blk * tm.world_size + tm.rank;
    uint32_t ty = gt / tm.tiles_x;
    x0 = (gt - ty * tm.tiles_x) * RT_TILE;
    y0 = ty * RT_TILE;
    return gt < tm.n_tiles;
}

// A lane's status lives in `cur` alone (compares and selects are half-rate on gfx950; one register, one compare):
//   cur <  IRR                     at an inner node, ray in the fast-division class            } tracing
//   cur <  LEAF                    at an inner node (marked IRR: ray outside the class)        }  (cur < SHADE)
//   cur <  SHADE                   at a leaf: LEAF | code (code <= 0x7ffe)                     }
//   cur == SHADE                   trace finished, waiting for the shade phase
//   cur == NEED                    path finished, waiting for a new sample (render_kernel_xchg's tracers: an empty lane)
//   cur == OFF                     no samples left
//   cur == START                   got a new ray in this round; its trace begins at the end of the round
// 16-bit references: SHADE 0xffff (fits a stack entry: the sentinel at the bottom of the stack; leaf codes stop at 0x7ffe), NEED 0x20000,
// OFF 0x30000, START 0x40000; 32-bit references (WIDE): the top four values 0xfffffffc .. 0xffffffff.  "Tracing" is `cur < SHADE` either way.
template <bool WIDE>
struct LaneStatus {
    static constexpr uint32_t LEAF = WIDE ? RT_REF_LEAF_BIG : RT_REF_LEAF, IRR = WIDE ? RT_REF_IRR_BIG : RT_REF_IRR;
    static constexpr uint32_t SHADE = WIDE ? 0xfffffffcu : 0xffffu, NEED = WIDE ? 0xfffffffdu : 0x20000u;
    static constexpr uint32_t OFF = WIDE ? 0xfffffffeu : 0x30000u, START = WIDE ? 0xffffffffu : 0x40000u;
};

// The (near, far) plane pairs of both child boxes of wide node `idx` and its two child references.  kx/ky/kz: 0 where the
// ray direction component is >= 0 (near = box min) or the ray is outside the fast class, 4 where it is negative.
struct WideNodeData {
    float lnx, lny, lnz, lfx, lfy, lfz, rnx, rny, rnz, rfx, rfy, rfz;
    uint32_t left, right;
};
// BIG: nodes below n_top come from their LDS copy (`top`), the others from global memory — the global path is bound by
// the L1's tag lookups, which only the lanes that really go to memory consume.
template <bool BIG>
__device__ __forceinline__ WideNodeData fetch_wide_node(const char* nodes, const uint4* top, uint32_t n_top, uint32_t idx,
                                                        uint32_t kx, uint32_t ky, uint32_t kz) {
    WideNodeData n;
    if (BIG) {
        float4 a, b, c;
        uint4 r;
        if (idx < n_top) {
            const float4* q = reinterpret_cast<const float4*>(top + idx * (RT_NODE_DWORDS_BIG / 4u));
            a = q[0]; b = q[1]; c = q[2];
            r = reinterpret_cast<const uint4*>(q)[3];
        } else {
            const float4* q = reinterpret_cast<const float4*>(nodes + idx * (RT_NODE_DWORDS_BIG * 4u));
            a = q[0]; b = q[1]; c = q[2];
            r = reinterpret_cast<const uint4*>(q)[3];
        }
        const bool sx = kx != 0u, sy = ky != 0u, sz = kz != 0u;
        n.lnx = sx ? a.w : a.x; n.lfx = sx ? a.x : a.w;
        n.lny = sy ? b.x : a.y; n.lfy = sy ? a.y : b.x;
        n.lnz = sz ? b.y : a.z; n.lfz = sz ? a.z : b.y;
        n.rnx = sx ? c.y : b.z; n.rfx = sx ? b.z : c.y;
        n.rny = sy ? c.z : b.w; n.rfy = sy ? b.w : c.z;
        n.rnz = sz ? c.w : c.x; n.rfz = sz ? c.x : c.w;
        n.left = r.x; n.right = r.y;
    } else {
        // one 32-bit byte offset per access: (near, far) are consecutive dwords of the (min, max, min) triples
        const uint32_t nb = idx * RT_NODE_BYTES;
        const float* px = reinterpret_cast<const float*>(nodes + (nb + kx));
        const float* py = reinterpret_cast<const float*>(nodes + (nb + ky));
        const float* pz = reinterpret_cast<const float*>(nodes + (nb + kz));
        n.lnx = px[0]; n.lfx = px[1]; n.rnx = px[9]; n.rfx = px[10];
        n.lny = py[3]; n.lfy = py[4]; n.rny = py[12]; n.rfy = py[13];
        n.lnz = pz[6]; n.lfz = pz[7]; n.rnz = pz[15]; n.rfz = pz[16];
        const uint32_t refs = reinterpret_cast<const uint32_t*>(nodes + nb)[RT_NODE_REFS];
        n.left = refs & 0xffffu; n.right = refs >> 16;
    }
    return n;
}

// The tail's environment record: (W, H, u0 bits, -), (texels low, texels high, distribution low, distribution high), read wave-uniformly —
// every lane sees the same record, so it travels through scalars.  The miss branch keeps its own statement of the first six words; the ENVL forms read all eight here.
struct EnvRecord { uint32_t w, h; float u0; const float4* texels; const float* dist; };
__device__ __forceinline__ EnvRecord load_env_record(const uint4* er) {
    const uint4 e0 = er[0], e1 = er[1];
    EnvRecord r;
    r.w = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0.x); r.h = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0.y);
    r.u0 = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)e0.z));
    r.texels = reinterpret_cast<const float4*>((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)e1.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)e1.y) << 32);
    r.dist = reinterpret_cast<const float*>((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)e1.z) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)e1.w) << 32);
    return r;
}

// The tail's texture table at tt: (texels low, texels high, n, -), then one vec4 per image; entry `image` at (u, v) by texture_value.  Inlined:
// behind a __noinline__ call — the whole of it, or its bilinear part alone — most EXT 2 kernels take 4 to 20 bytes of scratch more (EXPERIMENTS.md E17).  The header is the same for every
// lane and goes through scalars; the entry is loaded per lane, since lanes may sit on different images.
__device__ __forceinline__ f3 texture_table_value(const uint4* tt, uint32_t image, float u, float v) {
    const uint4 th = tt[0];
    const uint64_t texels = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.y) << 32;
    return texture_value(reinterpret_cast<const uint32_t*>(texels), tt[1u + image], u, v);
}

// EXACT = true : box tests use aabb_intersects() verbatim (IEEE division, GLM min/max).
// EXACT = false: rays classified "regular" use the 4-instruction correctly-rounded division (two-word reciprocal) and
//                near/far plane selection by address (rt_fastdiv.hpp) — identical decisions, proven + exhaustively
//                verified; other rays carry marked references and are stepped by a verbatim loop.
// FILTER = true (variant 4, experimental): decide the two box tests of a visit from one-multiply plane
//                parameters with a safety margin (box_pair_filtered) and fall back to exact quotients only
//                for near-ties; sound and bit-identical, but not faster yet because ~1.5 % of visits are ties.
// WORLD: RT_WORLD_BVH (default), RT_WORLD_LIST (HittableList: bounds pre-test, then every sphere in order;
//        a reference is RT_REF_LEAF | primitive index and the "traversal" is the leaf phase alone) or
//        RT_WORLD_NODE_TREE (bvh_node: a node is tested against ITS OWN box when visited, then left, then right), or
//        RT_WORLD_BVH_QUEUE (the reference's disabled distance-sorted queue, BVH.cu:17-49: the frontier is one sorted list per ray, so
//        there is no wave-level hot loop to share — a lane walks its whole trace when the trace begins (bvh_closest_intersection_queue,
//        the function the probes and the baseline kernel run) and joins the others again at the shade phase; what the streaming kernel
//        adds for such a world is the in-order resolve, i.e. a framebuffer bit-identical to the oracle's, and the sample streaming).
// EXT >= 1: the scene uses features the reference does not have (quads, diffuse lights, a constant background, constant
//        media; EXT = 2 adds the two textured materials — Perlin marble and the image texture — whose code is large enough
//        to cost the other kernels registers):
//        leaf codes >= sphere_codes are quads, emitted radiance is accumulated along the path (the reference's
//        commented `accum_radiance`), the miss colour may be a constant.  A separate instantiation, so the
//        reference-feature kernels carry none of it.
// BIG: the records stay in global memory / L2 (the image does not fit the LDS); WIDE: 32-bit references (a BIG world with 2^14
//      inner nodes or 2^15 leaf codes or more) — a BIG world whose references fit 16 bits keeps the narrow encoding, which halves
//      the per-lane stacks and leaves that much more of the LDS for the top of the tree.
// TOL (variant 6, opt-in): the hot loop's plane parameters are (b - o) * RN(1/d) instead of the exact quotients — inside north_star's |delta| < 1e-3,
//      not bit-exact by construction (rt_fastdiv.hpp: slab_near_far_tolerant).  LDS-resident RT_WORLD_BVH worlds of the reference's feature set (EXT == 0) only.
// TRI: the world has triangles — quads at or past p.scene.n_plain_quads take the book's `tri` interior test in the leaf phase.  A family of its own:
//      measured in one instantiation with the quads, the extra compare and add cost the Cornell box 1.0 % (EXPERIMENTS.md E9), so worlds without triangles keep
//      the kernels they had, instruction for instruction.
// NEE (rt_renderer_light_sampling_enable, opt-in; EXT >= 1 only): a Lambertian / checker hit draws its next direction from the mixture of its own cosine
//      distribution and a distribution over the world's lights, and weighs the path by the ratio of the densities.  The light table —
//      a header (n_l, -, -, -), then (index, area, kind, -) per light, then — only where a kind says sphere — (Cx, Cy, Cz, r) per light — lies behind the
//      quads' shade records in the image the NEE launches are given, so it costs no kernel argument: the other instantiations neither see it nor pay for it.
//      A kind RT_LIGHT_TRIANGLE (mode RT_LIGHT_SAMPLING_MESH) exists only in a world with triangles, so only the TRI && NEE forms hold code for it.
// LTREE (mode RT_LIGHT_SAMPLING_TREE; NEE && TRI only, whether or not the world has a triangle): the light is drawn in proportion to its area — a
//      binary search over the cumulative areas in the entries' fourth lane, A in the header's second — and the density step walks a threaded bounding-volume tree
//      of the lights, two vec4 per node behind the table ((min.xyz, skip), (max.xyz, leaf)), instead of testing every light: no stack, no indexed private array.
// ENVL (mode RT_LIGHT_SAMPLING_ENV; EXT == 2 && NEE && TRI only, whether or not the world has a triangle): the light half draws its direction from
//      the environment map — environment_sample on the distribution the tail's environment record points to — and the light density is the map's own
//      (environment_density); the light table's pick, point, density loop and tree walk are compiled out.  No shadow ray: the direction is followed.
// NMAP (rt_renderer_normal_maps; EXT == 2 && TRI only, whether or not the world has a triangle): a hit on a material whose record of the tail's
//      normal-map table says `on` bends its normal by normal_map_apply, once, right after the flat or smooth normal is known; an image-textured hit shares its
//      (u, v) with the map.  The table lies behind the texture table, whose header's fourth lane says where; both words are read at the hit, through scalars.
// MFAC (rt_renderer_microfacets; NMAP only): a hit on a material whose record of the tail's microfacet table says `on` runs microfacet_scatter
//      before the scatter branches: a metal is a rough conductor, a Lambertian kind wears a coat whose toss comes before every draw of the base.  A specular or
//      absorbed hit takes none of the base's draws; a base or backside hit runs the code below as it stands.  The records lie last in the tail, where the bits
//      above bit 0 of the header's first lane say; that word is read at the hit, through a scalar, and vn_on keeps bit 0 alone.
//      Rough glass: a dielectric whose record is a glass one runs rough_glass_faced in the dielectric branch, from the facing that branch has
//      computed; reflected or transmitted, the albedo is scaled by the rule's weight; absorbed is a failed scatter; handed back, the smooth hit runs verbatim.
// INTR (rt_renderer_interiors; MFAC only): a dielectric hit whose material has an interior record takes its facing on a parallelogram or triangle
//      from the stored normal — the comparison set_face_normal makes, kept as q_back — and a back hit scales the albedo by interior_hit's transmittance before
//      the smooth or rough rule runs.  The tail's first lane then counts the vec4 to a sub-header (to the microfacet records or 0, to the interior records, -, -).
// CUT (rt_renderer_cutouts; INTR only): in the leaf phase a parallelogram or triangle that passes its test, on a material whose cutout record is
//      on, is taken only if cutout_keeps says so — the mask's texel at the candidate's own (u, v), the first texture lookup inside the traversal.  A candidate
//      turned down leaves rec_t and rec_code alone, and the lane goes on as after a failed test.  The records lie behind the interior records; the sub-header's
//      third lane says where, and its second lane is 0 when there is no interior table.  Spheres ignore the record.  Nothing is drawn.
// LTREE && ENVL (mode RT_LIGHT_SAMPLING_ENV_TREE): both at once.  The light half tosses once more between the map and mode 16's table (no toss
//      when the table is empty: n_l == 0 is the map alone), the light density is the mean of the map's and the walk's, and an image-textured Lambertian hit is
//      sampled as the diffuse hit it is — its albedo is looked up behind the direction, as ever.
template <bool EXACT, bool FILTER, int BLOCK, int WORLD = RT_WORLD_BVH, int EXT = 0, bool BIG = false, bool WIDE = BIG, bool TOL = false, bool NEE = false, bool TRI = false,
          bool LTREE = false, bool ENVL = false, bool CUT = false, bool INTR = false, bool MFAC = false, bool NMAP = false>
// (the second launch bound is hipcc's minimum of waves per SIMD — 6 for 768 threads, what two workgroups per CU are, and all the LDS admits: the register budget is
//  80, not the 64 of a full SIMD.  The default instantiation took 64 while it needed no more and takes 68 since E23, with no scratch; the occupancy the compiler
//  reports for it, 8 and now 7, is what its register count would admit, not what the launch gets.)
__global__ __launch_bounds__(BLOCK, BLOCK / 128) void render_kernel_stream(StreamParams p) {
    static_assert(!NMAP || (EXT == 2 && TRI), "normal maps: one family of the kernels that read the texture table, plain and with mode 48");
    static_assert(!MFAC || NMAP, "microfacet surfaces: a glossy asset wants its normal map in the same launch, and the roughness map shares the map's (u, v)");
    static_assert(!INTR || MFAC, "solid glass: one family, the microfacet forms once more, so that a frosted solid is entered and left in the same launch");
    static_assert(!CUT || INTR, "alpha cutouts: one family, the solid-glass forms once more, so that one launch serves an asset with every kind of record");
    static_assert(!NEE || (EXT >= 1 && WORLD != RT_WORLD_BVH_QUEUE), "light sampling: worlds with quads, walked by the stack or as a list");
    static_assert(!TRI || (EXT >= 1 && WORLD != RT_WORLD_BVH_QUEUE), "triangles: worlds with quads; a lane walk reads the kind from the flat record");
    static_assert(!LTREE || (NEE && TRI), "the light tree: one family, which knows all three kinds of light");
    static_assert(!ENVL || (EXT == 2 && NEE && TRI), "environment light sampling: one family of the kernels that look the map up, and one more with the light tree");
    constexpr bool ENVT = LTREE && ENVL;   // §26
    extern __shared__ uint4 lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = tid >> 6;

    // reference encoding and lane status codes (LaneStatus)
    using ref_t = typename std::conditional<WIDE, uint32_t, uint16_t>::type;
    using K = LaneStatus<WIDE>;
    static_assert(BIG || !WIDE, "an LDS-resident image always has 16-bit references");

    // ---- the scene: staged into the LDS with coalesced 16-B loads, or (BIG) left in global memory / L2 -------------
    const uint4* scene_base;
    if (BIG) {
        scene_base = p.scene.blob;
        for (uint32_t i = tid; i < p.scene.n_top * (RT_NODE_DWORDS_BIG / 4u); i += BLOCK) lds[i] = p.scene.blob[i];   // the top of the tree
        __syncthreads();
    } else {
        for (uint32_t i = tid; i < p.scene.blob_vec4; i += BLOCK) lds[i] = p.scene.blob[i];
        __syncthreads();
        scene_base = lds;
    }
    const char* nodes = reinterpret_cast<const char*>(scene_base);
    const float4* spheres = reinterpret_cast<const float4*>(scene_base + p.scene.off_spheres);
    const float4* extra = reinterpret_cast<const float4*>(scene_base + p.scene.off_extra);
    const float4* mats16 = reinterpret_cast<const float4*>(scene_base + p.scene.off_mats);
    const float4* quads = reinterpret_cast<const float4*>(scene_base + p.scene.off_quads);
    // per-lane traversal stack of references (16 bits, BIG: 32).  Entry k of this lane is stack[k * 64].
    ref_t* stack = reinterpret_cast<ref_t*>(lds + (BIG ? p.scene.n_top * (RT_NODE_DWORDS_BIG / 4u) : p.scene.blob_vec4)) + wave * 64u * p.scene.stack_cap + lane;

    // §21, TRI only: one vec4 behind the image the launch was given (behind its light table too) says whether vertex normals follow it — (on, -, -, -), then 36 B per
    // triangle, in global memory whatever the form of the image.  Wave-uniform; a world without a table pays this one scalar load and one scalar branch per shaded quad hit.
    uint32_t vn_on = 0u;
    if constexpr (TRI) vn_on = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].x);
    if constexpr (MFAC) vn_on &= 1u;   // §29: the bits above say where the microfacet records lie; the hit reads them
    // §22, TRI with image textures (EXT >= 2) only: the same header's .y = how many vec4 behind the header the texture coordinates start (24 B per triangle), 0 = none
    uint32_t uv_at = 0u;
    if constexpr (TRI && EXT >= 2) uv_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].y);
    // §23, EXT >= 2 only: the same header's .z = how many vec4 behind the header the environment record lies — (W, H, u0 bits, -), (pointer low, pointer high, -, -) —
    // 0 = none.  The renderer launches a background-2 world only with a record.
    uint32_t env_at = 0u;
    if constexpr (EXT >= 2) env_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].z);
    // §25, EXT >= 2 only: the same header's .w = how many vec4 behind the header the texture table lies — (texels low, texels high, n, -), then one vec4
    // (W, H, wrap | filter << 8, first texel) per image — 0 = none.  The renderer launches only when every image material's index has an entry.  That word is
    // NOT read here: a scalar kept live across the path loop cost every EXT 2 kernel spills (EXPERIMENTS.md E17); the image hit reads it where it needs it.
    const f3 root_min = mk3(p.scene.root_min[0], p.scene.root_min[1], p.scene.root_min[2]);
    const f3 root_max = mk3(p.scene.root_max[0], p.scene.root_max[1], p.scene.root_max[2]);

    // ---- per-lane path state ------------------------------------------------------------------------
    Ray ray;
    ray.o = mk3(0.0f); ray.d = mk3(0.0f); ray.time = 0.0f;
    f3 inv_d = mk3(0.0f);   // RN(1/d) of a regular ray (EXACT == false)
    f3 inv_lo = mk3(0.0f);  // its low word: inv_d + inv_lo ~= 1/d to 47 bits (fast_div_exact4, FAST_BVH only)
    f3 far_c = mk3(0.0f);   // RN(-o * inv_d): a far plane parameter is fma(plane, inv_d, far_c) (slab_far_fma, FAST_BVH only)
    float far_s_eps = 0.0f; // the per-ray term of that form's certificate margin (slab_fma_margin)
    bool regular = false;
    f3 atten = mk3(0.0f);
    f3 accum_rad = mk3(0.0f);  // EXT only: radiance emitted along the path so far
    Rng rng;
    rng.s0 = 1u; rng.s1 = 0u; rng.s2 = 0u; rng.s3 = 0u; rng.draws = 0u;   // every sample brings its own state (primary_rays_kernel)
    float ray_a = 0.0f;     // dot(ray.d, ray.d): the `a` of every sphere test of the trace (SphereHittable.cuh:17), computed once per ray
    float rec_t = RT_MISS_DIST;
    int32_t rec_code = -1;  // leaf code of the closest hit so far, -1 = none
    uint32_t cur = K::NEED;   // node reference being visited, or the lane's status (LaneStatus)
    ref_t* sp = stack + 64;   // next free entry of this lane's stack (entries are 64 apart; entry 0 is the sentinel)
    *stack = (ref_t)K::SHADE;
    uint32_t kx = 0, ky = 0, kz = 0;  // byte offset (0 / 4) of the (near, far) pair inside an axis triple, per ray
    // FAST_BVH: the default kernel (variant 3).  Inner references of rays outside the fast-division class are marked
    // with K::IRR (an LDS-resident tree has < 2^14 inner nodes) so that the hot loop needs no per-lane branch.
    constexpr bool FAST_BVH = !EXACT && !FILTER && WORLD == RT_WORLD_BVH;
    // The certified far planes as one fma each (E23): the kernels of the reference's feature set.  The form keeps four more registers alive per ray, and every
    // EXT kernel that was at its 80 registers answered them with scratch (EXPERIMENTS.md E23), so a quad-free world on an EXT kernel keeps the product form.
    constexpr bool FAR_FMA = FAST_BVH && !TOL && EXT == 0;
    bool irr_pending = false;         // wave-uniform: some lane is traversing with a ray outside the class
    uint32_t depth = 0;
    uint32_t out_idx = 0;   // == the sample index n: the sample buffer is laid out in index order

    // ---- wave-uniform work pool: sample indices [pool_next, pool_end) ----------------------------------
    // The FIRST chunk of a wave is its own (chunk number = the wave's number in the grid; the host starts the shared counter behind
    // them): 6144 waves asking one counter at once take ~70 us (one word serves ~88 returning atomics per us), which a 1/8 shard feels.
    // (readfirstlane: the wave's number is uniform, which the compiler cannot see in threadIdx.x >> 6 — the pool stays in scalar registers)
    uint32_t pool_next = min((blockIdx.x * (BLOCK / 64u) + (uint32_t)__builtin_amdgcn_readfirstlane((int)wave)) * p.chunk, p.total);
    uint32_t pool_end = min(pool_next + p.chunk, p.total);
    bool pool_dry = false;

/* entry 0 of every lane's stack holds K::SHADE: popping an empty stack IS "trace finished", no test needed */ \
#define RT_POP()                      \
    do {                              \
        sp -= 64;                     \
        cur = *sp;                    \
    } while (0)
#define RT_EMIT_DARK() RT_EMIT(EXT ? accum_rad.x : 0.0f, EXT ? accum_rad.y : 0.0f, EXT ? accum_rad.z : 0.0f)
#define RT_EMIT(rx, ry, rz)                                   \
    do {                                                      \
        store_sample(p.samples, out_idx, (rx), (ry), (rz));     \
        cur = K::NEED;                                    \
    } while (0)

#ifdef RT_PHASE_TIMERS
    unsigned long long pt_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, pt_last_ = __builtin_readcyclecounter();
    uint32_t pc_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#ifdef RT_TRACE_HIST
    uint32_t tr_steps_ = 0, tr_leafs_ = 0;   // per lane: inner-node steps / leaf tests of the current trace (histogram for tools/sched_model.py)
#endif
#define RT_PT(i) do { unsigned long long n_ = __builtin_readcyclecounter(); pt_[i] += n_ - pt_last_; pt_last_ = n_; pc_[i]++; } while (0)
#else
#define RT_PT(i)
#endif
    for (;;) {
        RT_PT(7);
        // ================= phase 1: inner-node steps (BVH.cu:76-97) ==================================
        if (FAST_BVH) {
            // Hot loop of the default kernel: lanes whose ray is in the fast-division class (all but a handful).  The
            // step is straight-line code; lanes outside the class carry K::IRR in their inner references, so they
            // fail `cur < K::IRR` here and are stepped by the verbatim loop below.
            bool at_inner = cur < K::IRR;
            const uint64_t m_entry = __ballot(at_inner);
            if (m_entry != 0ull) {
                uint32_t n_inner_lanes;
                // The loop is left relative to the lane count it was entered with (node_loop_keep); inner_keep >= 1 (host).  Once the queue is dry the
                // wave only drains its last paths: no reason to leave early.  The threshold is wave-uniform, worked out once per entry in scalar registers;
                // readfirstlane tells the compiler so (a scalar compare and branch instead of a vector compare and an exec-mask loop exit)
                const uint32_t keep_now = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pool_dry ? 1u : node_loop_keep(p, (uint32_t)__popcll(m_entry))));
                // Certified far planes (rt_fastdiv.hpp) pay where boxes have thickness.  The box of an axis-aligned quad is 1e-4 thick: the near and far
                // parameters of a ray that hits it agree to ~2e-7, inside the certificate's margin, so nearly every hit box would take the exact redo
                // (measured: Cornell box -6 %, Book-2 final scene -5 %).  Worlds with quads therefore keep the twelve exact quotients; the reference's
                // feature set has no quads (EXT == 0: decided at compile time), the EXT kernels decide per world (wave-uniform).
                const bool far_certified = EXT == 0 || p.scene.n_quads == 0u;
                do {
                    if (at_inner) {
                        const WideNodeData nd = fetch_wide_node<BIG>(nodes, lds, p.scene.n_top, cur, kx, ky, kz);
                        const uint32_t left_idx = nd.left, right_idx = nd.right;
                        float tl, tr;
                        bool hl, hr;
                        if (TOL) {
                            hl = slab_near_far_tolerant(nd.lnx, nd.lny, nd.lnz, nd.lfx, nd.lfy, nd.lfz, ray, inv_d, rec_t, tl);
                            hr = slab_near_far_tolerant(nd.rnx, nd.rny, nd.rnz, nd.rfx, nd.rfy, nd.rfz, ray, inv_d, rec_t, tr);
                        } else if (!far_certified) {   // a world with quads: all twelve parameters as exact quotients
                            hl = slab_near_far_regular(nd.lnx, nd.lny, nd.lnz, nd.lfx, nd.lfy, nd.lfz, ray, inv_d, inv_lo, rec_t, tl);
                            hr = slab_near_far_regular(nd.rnx, nd.rny, nd.rnz, nd.rfx, nd.rfy, nd.rfz, ray, inv_d, inv_lo, rec_t, tr);
                        } else {
                            // near parameters: exact quotients (tl, tr are compared with each other and with rec.distance); far parameters: one fma each
                            // (FAR_FMA) or products, with the `tmin <= tmax` decisions — and, of the fma form, the sign of tmax — certified (rt_fastdiv.hpp:
                            // CERTIFIED FAR PLANES) — or, rarely and for the whole wave, redone exactly from a second read of the node
                            tl = slab_near_exact(nd.lnx, nd.lny, nd.lnz, ray, inv_d, inv_lo);
                            tr = slab_near_exact(nd.rnx, nd.rny, nd.rnz, ray, inv_d, inv_lo);
                            float far_l, far_r;
                            bool unsure;
                            if (FAR_FMA) {
                                far_l = slab_far_fma(nd.lfx, nd.lfy, nd.lfz, inv_d, far_c);
                                far_r = slab_far_fma(nd.rfx, nd.rfy, nd.rfz, inv_d, far_c);
                                unsure = far_pair_uncertain_fma(tl, far_l, tr, far_r, far_s_eps);
                            } else {
                                far_l = slab_far_product(nd.lfx, nd.lfy, nd.lfz, ray, inv_d);
                                far_r = slab_far_product(nd.rfx, nd.rfy, nd.rfz, ray, inv_d);
                                unsure = far_pair_uncertain(tl, far_l, tr, far_r);
                            }
                            if (__ballot(unsure) != 0ull) {
#ifdef RT_PHASE_TIMERS
                                pc_[14]++;   // hot-loop steps that take the exact redo (wave level), and those of them that some lane asks for over the sign of tmax
                                if (FAR_FMA && __ballot(min(__float_as_uint(far_l), __float_as_uint(far_r)) <= __float_as_uint(far_s_eps)) != 0ull) pc_[15]++;
#endif
                                asm volatile("" ::: "memory");   // (a second read of the node: the common path need not keep six plane offsets alive)
                                const WideNodeData n2 = fetch_wide_node<BIG>(nodes, lds, p.scene.n_top, cur, kx, ky, kz);
                                far_l = slab_far_exact(n2.lfx, n2.lfy, n2.lfz, ray, inv_d, inv_lo);
                                far_r = slab_far_exact(n2.rfx, n2.rfy, n2.rfz, ray, inv_d, inv_lo);
                            }
                            hl = tl <= far_l && tl < rec_t && far_l > 0;
                            hr = tr <= far_r && tr < rec_t && far_r > 0;
                        }
                        // BVH.cu:87-96, see the generic loop below: with both boxes hit the far child is pushed and the near
                        // one continues; with one hit it continues; with none the stack is popped.  `left_dist > right_dist`
                        // (missed box = _MISS_DIST) is "right hit and (left missed or tl > tr)".
                        const bool go_right = hr && (!hl || tl > tr);
                        if (hl && hr) {
                            *sp = (ref_t)(go_right ? left_idx : right_idx);
                            sp += 64;
                        }
                        cur = go_right ? right_idx : left_idx;
                        if (!(hl || hr)) RT_POP();
#ifdef RT_TRACE_HIST
                        tr_steps_++;
#endif
                    }
                    at_inner = cur < K::IRR;
                    n_inner_lanes = (uint32_t)__popcll(__ballot(at_inner));
#ifdef RT_PHASE_TIMERS
                    pc_[6]++;
#endif
                } while (n_inner_lanes >= keep_now);
            }
            RT_PT(0);
            if (irr_pending) {   // wave-uniform, rare: rays with a zero / tiny / huge direction or origin component
                for (;;) {
                    const bool at_irr = (cur & (K::LEAF | K::IRR)) == K::IRR;
                    if (__ballot(at_irr) == 0ull) break;
                    if (at_irr) {
                        const WideNodeData nd = fetch_wide_node<BIG>(nodes, lds, p.scene.n_top, cur & (K::IRR - 1u), 0u, 0u, 0u);   // near = min, far = max
                        uint32_t left_idx = nd.left, right_idx = nd.right;
                        if (left_idx < K::LEAF) left_idx |= K::IRR;     // inner references stay marked all the way down
                        if (right_idx < K::LEAF) right_idx |= K::IRR;
                        float left_dist = RT_MISS_DIST, right_dist = RT_MISS_DIST;
                        const bool hl = aabb_intersects(mk3(nd.lnx, nd.lny, nd.lnz), mk3(nd.lfx, nd.lfy, nd.lfz), ray, rec_t, left_dist);
                        const bool hr = aabb_intersects(mk3(nd.rnx, nd.rny, nd.rnz), mk3(nd.rfx, nd.rfy, nd.rfz), ray, rec_t, right_dist);
                        const bool swap_lr = left_dist > right_dist;
                        if (hl && hr) {
                            *sp = (ref_t)(swap_lr ? left_idx : right_idx);
                            sp += 64;
                        }
                        cur = (swap_lr || !hl) ? right_idx : left_idx;
                        if (!(hl || hr)) RT_POP();
                    }
                }
                irr_pending = __ballot(!regular && (cur < K::SHADE)) != 0ull;
            }
            RT_PT(1);
        } else if (WORLD != RT_WORLD_BVH_QUEUE) {   // (a queue world's lanes are never "at a node": their trace ran when it began)
            bool at_inner = cur < K::LEAF;
            uint64_t m_inner = __ballot(at_inner);
            // the hot loop's exit rule (node_loop_keep); these kernels never stayed on a dry queue, and do not now
            const uint32_t keep_now = (uint32_t)__builtin_amdgcn_readfirstlane((int)node_loop_keep(p, (uint32_t)__popcll(m_inner)));
            while (m_inner != 0ull) {
                if (at_inner) {
                    // kx/ky/kz are 0 in these kernels: near == box min, far == box max
                    const WideNodeData nd = fetch_wide_node<BIG>(nodes, lds, p.scene.n_top, cur, 0u, 0u, 0u);
                    const float lnx = nd.lnx, lny = nd.lny, lnz = nd.lnz, lfx = nd.lfx, lfy = nd.lfy, lfz = nd.lfz;
                    const float rnx = nd.rnx, rny = nd.rny, rnz = nd.rnz, rfx = nd.rfx, rfy = nd.rfy, rfz = nd.rfz;
                    const uint32_t left_idx = nd.left, right_idx = nd.right;
                    if (WORLD == RT_WORLD_NODE_TREE) {
                        // bvh_node::ClosestIntersection (bvh_node.cuh:19-24): own box, then left subtree, then right
                        float d_own;
                        if (aabb_intersects(mk3(lnx, lny, lnz), mk3(lfx, lfy, lfz), ray, rec_t, d_own)) {
                            *sp = (ref_t)right_idx;
                            sp += 64;
                            cur = left_idx;
                        } else {
                            RT_POP();
                        }
                    } else {
                        const f3 lmin = mk3(lnx, lny, lnz), lmax = mk3(lfx, lfy, lfz), rmin = mk3(rnx, rny, rnz), rmax = mk3(rfx, rfy, rfz);
                        bool hl, hr, swap_lr;
                        if (EXACT || !regular) {
                            float left_dist = RT_MISS_DIST, right_dist = RT_MISS_DIST;
                            hl = aabb_intersects(lmin, lmax, ray, rec_t, left_dist);
                            hr = aabb_intersects(rmin, rmax, ray, rec_t, right_dist);
                            swap_lr = left_dist > right_dist;
                        } else {
                            BoxPairDecision dec = box_pair_filtered(lmin, lmax, rmin, rmax, ray, inv_d, rec_t);
                            hl = dec.hit_left; hr = dec.hit_right; swap_lr = dec.swap;
                            if (dec.uncertain) {
                                // a comparison too close to call (~1e-6 of visits): redo the visit with exact quotients.
                                // The node is re-read (volatile) so that the common path need not keep 12 box
                                // coordinates alive across the filter.
                                const volatile float* vn = reinterpret_cast<const volatile float*>(nodes + cur * RT_NODE_BYTES);   // FILTER kernels are LDS-resident
                                float left_dist = RT_MISS_DIST, right_dist = RT_MISS_DIST;
                                hl = aabb_intersects_regular(mk3(vn[0], vn[3], vn[6]), mk3(vn[1], vn[4], vn[7]), ray, inv_d, rec_t, left_dist);
                                hr = aabb_intersects_regular(mk3(vn[9], vn[12], vn[15]), mk3(vn[10], vn[13], vn[16]), ray, inv_d, rec_t, right_dist);
                                swap_lr = left_dist > right_dist;
                            }
                        }
                        // "assert that left is closer for next step" (BVH.cu:90-93), then push far / near iff
                        // dist < rec.distance (BVH.cu:95-96).  A hit box has dist = tmin < rec.distance by aabb.cuh:41 and
                        // a missed one keeps _MISS_DIST, so the push conditions ARE the hit flags: with both hit the far
                        // child is pushed and the near one (which would be popped straight away) stays in `cur`; with one
                        // hit it becomes `cur` (swap_lr is then exactly "the right one"); with none the stack is popped.
                        if (hl && hr) {
                            *sp = (ref_t)(swap_lr ? left_idx : right_idx);
                            sp += 64;
                        }
                        cur = (swap_lr || !hl) ? right_idx : left_idx;
                        if (!(hl || hr)) RT_POP();
                    }
                }
                at_inner = cur < K::LEAF;
                m_inner = __ballot(at_inner);
                if ((uint32_t)__popcll(m_inner) < keep_now) break;
            }
        }

        // ================= phase 2: leaves (BVH.cu:69-73 -> SphereHittable.cu:56-66 / :91-102) ========
        {
            bool at_leaf = WORLD != RT_WORLD_BVH_QUEUE && (cur - K::LEAF) < (K::SHADE - K::LEAF);
            uint64_t m_leaf = __ballot(at_leaf);
            if (m_leaf != 0ull && ((uint32_t)__popcll(m_leaf) >= p.leaf_min || __ballot(cur < K::LEAF) == 0ull)) {
                if (at_leaf) {
#ifdef RT_TRACE_HIST
                    tr_leafs_++;
#endif
                    uint32_t code = cur & (K::LEAF - 1u);   // BVH / tree: prim * 2 + is_moving;  list: unified primitive index
                    const uint32_t first_quad = (WORLD == RT_WORLD_LIST) ? p.scene.n_prims : p.scene.sphere_codes;
                    if (EXT && code >= first_quad) {
                        // quad::hit ("The Next Week"), reference conventions: see quad_closest_intersection()
                        const float4* qd = quads + (code - first_quad) * 4u;
                        float4 a0 = qd[0], a1 = qd[1], a2 = qd[2], a3 = qd[3];
                        // all four parts in ONE round trip: left alone, the compiler sinks the reads of (Q, D) below the tests that use the normal — three
                        // dependent round trips per quad test, which the global-memory form feels
                        asm volatile("" : : "v"(a0.x), "v"(a0.w));
                        HitRec tmp;
                        tmp.distance = rec_t; tmp.normal = mk3(0.0f); tmp.prim = -1; tmp.mat = 0;
                        // the triangles follow the parallelograms (§18): the quad's index says which interior test it takes
                        const uint32_t quad_kind = TRI && (code - first_quad) >= p.scene.n_plain_quads ? RT_QUAD_TRIANGLE : RT_QUAD_PARALLELOGRAM;
                        if (quad_closest_intersection(mk3(a0.x, a0.y, a0.z), a0.w, mk3(a1.x, a1.y, a1.z), mk3(a1.w, a2.x, a2.y),
                                                      mk3(a2.z, a2.w, a3.x), mk3(a3.y, a3.z, a3.w), 0u, 0, quad_kind, ray, tmp)) {
                            [[maybe_unused]] bool keep = true;
                            if constexpr (CUT) {
                                // §34: the cutout record of the candidate's material, (on, image, cutoff bits, -), read here alone; the offsets and the texture
                                // table's header are the same for every lane and are read through scalars where they are used, none of them kept across the loop
                                const uint32_t qi = code - first_quad;
                                const uint32_t cut_mat = __float_as_uint(quads[p.scene.n_quads * 4u + qi].w) & RT_MAT_INDEX_MASK;
                                uint4 cut_rec = make_uint4(0u, 0u, 0u, 0u);
                                const uint32_t sub_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].x) >> 1;
                                if (sub_at != 0u) {
                                    const uint32_t cut_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4 + sub_at].z);
                                    if (cut_at != 0u) cut_rec = p.scene.blob[p.scene.blob_vec4 + cut_at + cut_mat];
                                }
                                const uint32_t tex_here = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].w);
                                if (cut_rec.x != 0u && tex_here != 0u) {   // (the host launches no record without its table entry)
                                    const uint4* tt = p.scene.blob + p.scene.blob_vec4 + tex_here;
                                    const uint4 th = tt[0];
                                    const uint64_t texels = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.y) << 32;
                                    const uint32_t uv_here = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].y);
                                    const float* tr = nullptr;   // §22: a triangle under a table of texture coordinates weighs its vertices' (u, v), as the shade phase will
                                    if (uv_here != 0u && qi >= p.scene.n_plain_quads)
                                        tr = reinterpret_cast<const float*>(p.scene.blob + p.scene.blob_vec4 + uv_here) + (size_t)(qi - p.scene.n_plain_quads) * 6u;
                                    float cut_u, cut_v;
                                    f3 cut_c;
                                    keep = cutout_keeps(reinterpret_cast<const uint32_t*>(texels), tt[1u + cut_rec.y], __uint_as_float(cut_rec.z), mk3(a0.x, a0.y, a0.z),
                                                        mk3(a1.x, a1.y, a1.z), mk3(a1.w, a2.x, a2.y), mk3(a3.y, a3.z, a3.w), tr, ray, tmp.distance, cut_u, cut_v, cut_c);
                                }
                            }
                            if (!CUT || keep) {
                                rec_t = tmp.distance;
                                rec_code = (int32_t)(code - first_quad + p.scene.sphere_codes);   // the shade phase's code space
                            }
                        }
                        if (WORLD == RT_WORLD_LIST) {  // HittableList.cuh:26-30: every object, in order (the quads follow the spheres)
                            if (code + 1u < p.scene.n_prims + p.scene.n_quads) cur = K::LEAF | (code + 1u);
                            else cur = K::SHADE;
                        } else {
                            RT_POP();
                        }
                    } else {
                    uint32_t prim = (WORLD == RT_WORLD_LIST) ? code : code >> 1;
                    float4 sph = spheres[prim];
                    f3 center = mk3(sph.x, sph.y, sph.z);
                    uint32_t sph_matbits = 0u;  // EXT: a sphere with an isotropic material is a constant medium
                    if (WORLD == RT_WORLD_LIST) {
                        float4 ex = extra[prim];
                        const uint32_t moving = (__float_as_uint(ex.w) >> 28) & 1u;
                        code = prim * 2u + moving;
                        if (moving) center = mix(center, mk3(ex.x, ex.y, ex.z), ray.time);
                        sph_matbits = __float_as_uint(ex.w);
                    } else if (EXT || (code & 1u)) {
                        float4 ex = extra[prim];
                        if (code & 1u) center = mix(center, mk3(ex.x, ex.y, ex.z), ray.time);
                        sph_matbits = __float_as_uint(ex.w);
                    }
                    float t;
                    if (EXT && (sph_matbits >> 29) == RT_MAT_ISOTROPIC)
                        t = medium_sphere_intersection(ray, center, sph.w, mats16[sph_matbits & RT_MAT_INDEX_MASK].w, rec_t, rng);
                    else
                        t = sphere_closest_intersection_a(ray, ray_a, center, sph.w);
                    if (!(t >= rec_t)) {  // `if (t >= rec.distance) return false;`
                        rec_t = t;
                        rec_code = (int32_t)code;
                    }
                    if (WORLD == RT_WORLD_LIST) {  // HittableList.cuh:26-30: every object, in order
                        if (prim + 1u < p.scene.n_prims + (EXT ? p.scene.n_quads : 0u)) cur = K::LEAF | (prim + 1u);
                        else cur = K::SHADE;
                    } else {
                        RT_POP();
                    }
                    }
                }
            }
        }

        RT_PT(2);
        // ================= phase 3: shade finished traces, regenerate finished paths ==================
        // lanes that are not tracing wait for this phase (switched-off lanes count as waiting: near the end of the
        // pass that only makes the phase run a little earlier)
        uint64_t m_trav = __ballot((cur < K::SHADE));
        if (64u - (uint32_t)__popcll(m_trav) < p.shade_min && m_trav != 0ull) continue;

        bool start_trace = false;  // lanes that got a new ray this round begin their trace in ONE place below
        RT_PT(8);
        if (cur == K::SHADE) {  // sample_world's loop body after the trace (Renderer.cu:149-176)
#if defined(RT_PHASE_TIMERS) && defined(RT_TRACE_HIST)   // the histogram's atomics slow the kernel 40x: its own build flag
            atomicAdd(p.phase_acc + 32 + min(tr_steps_, 95u) * 16u + min(tr_leafs_, 15u), 1ull);
            tr_steps_ = 0; tr_leafs_ = 0;
#endif
            if (rec_code < 0) {
                f3 sky;
                if (EXT && p.scene.background == 1u) {
                    sky = mk3(p.scene.background_color[0], p.scene.background_color[1], p.scene.background_color[2]);
                } else {
                    bool from_map = false;
                    if constexpr (EXT >= 2) {
                        if (p.scene.background == 2u && env_at != 0u) {   // §23: the environment map; the record through scalars, the lookup per lane
                            const uint4* er = p.scene.blob + p.scene.blob_vec4 + env_at;
                            const uint4 e0 = er[0], e1 = er[1];
                            const uint32_t env_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0.x), env_h = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0.y);
                            const float env_u0 = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)e0.z));
                            const uint64_t env_p = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)e1.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)e1.y) << 32;
                            sky = environment_value(reinterpret_cast<const float4*>(env_p), env_w, env_h, env_u0, ray.d);
                            from_map = true;
                        }
                    }
                    if (!from_map) {
                    float t = normalize(ray.d).y * 0.5f + 0.5f;
                    sky = linear_interpolate(mk3(0.1f, 0.2f, 0.4f), mk3(0.9f, 0.9f, 0.99f), t);
                    }
                }
                f3 rad = atten * sky;
                if (EXT) rad = rad + accum_rad;
                RT_EMIT(rad.x, rad.y, rad.z);
            } else if (!EXT && depth + 1u >= p.max_depth) {
                RT_EMIT(0.0f, 0.0f, 0.0f);  // the scatter of the last allowed bounce cannot reach the sky: result is 0
            } else {
                // ---- what every material needs: hit point, outward normal, material record ----
                const f3 hit_p = ray_at(ray, rec_t);
                f3 normal;
                uint32_t mat_bits;
                [[maybe_unused]] bool q_back = false;   // §32, written and read under INTR alone: dot(d, Ng) > 0 on the stored normal of a parallelogram or triangle
                if (EXT && (uint32_t)rec_code >= p.scene.sphere_codes) {
                    const float4 qs = quads[p.scene.n_quads * 4u + ((uint32_t)rec_code - p.scene.sphere_codes)];   // the quad's shade record
                    normal = mk3(qs.x, qs.y, qs.z);
                    if constexpr (INTR) {   // §32: the same comparison, kept: the facing of a solid's parallelogram or triangle (it stands twice, as §30's smooth hit does)
                        q_back = dot(ray.d, normal) > 0;
                        if (q_back) normal = -normal;
                    } else {
                    if (dot(ray.d, normal) > 0) normal = -normal;  // the book's set_face_normal: a quad is two-sided
                    }
                    mat_bits = __float_as_uint(qs.w);
                    if constexpr (TRI) {
                        const uint32_t qi = (uint32_t)rec_code - p.scene.sphere_codes;
                        if (vn_on != 0u && qi >= p.scene.n_plain_quads) {   // §21: the shading normal of a triangle with vertex normals, or the flat one again
                            const float* vr = reinterpret_cast<const float*>(p.scene.blob + p.scene.blob_vec4 + 1u) + (size_t)(qi - p.scene.n_plain_quads) * 9u;
                            const f3 n0 = mk3(vr[0], vr[1], vr[2]), n1 = mk3(vr[3], vr[4], vr[5]), n2 = mk3(vr[6], vr[7], vr[8]);
                            const float4* qd = quads + qi * 4u;
                            const float4 a0 = qd[0], a1 = qd[1], a2 = qd[2], a3 = qd[3];
                            shading_normal(mk3(a0.x, a0.y, a0.z), mk3(a1.x, a1.y, a1.z), mk3(a1.w, a2.x, a2.y), mk3(a3.y, a3.z, a3.w), n0, n1, n2, ray.d, hit_p, normal);
                        }
                    }
                } else {
                    uint32_t prim = (uint32_t)rec_code >> 1;
                    float4 sph = spheres[prim];
                    float4 ex = extra[prim];
                    f3 center = mk3(sph.x, sph.y, sph.z);
                    if ((uint32_t)rec_code & 1u) center = mix(center, mk3(ex.x, ex.y, ex.z), ray.time);
                    normal = (hit_p - center) / sph.w;  // SphereHittable.cu:64 / :100
                    mat_bits = __float_as_uint(ex.w);
                }
                // §28: the normal map of the hit's material, if it has one: (u, v) and the tangents by the kind of surface, then the rule; the image lookup below
                // takes the same (u, v) — on a sphere the normal it would compute them from may just have been replaced
                float nm_tu = 0.0f, nm_tv = 0.0f;
                bool nm_uv = false;
                // §29: the microfacet record of the hit's material, (on, image, roughness bits, specular bits), zero where there is none; a mapped record's
                // roughness takes its map's green channel in the block below, which computes the (u, v) when either record needs them
                uint4 mf_rec = make_uint4(0u, 0u, 0u, 0u);
                float mf_rough = 0.0f;
                if constexpr (INTR) {   // §32: the lane counts the vec4 to the sub-header, whose first lane is what the MFAC forms read from the header itself
                    const uint32_t sub_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].x) >> 1;
                    uint32_t mf_at = 0u;
                    if (sub_at != 0u) mf_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4 + sub_at].x);
                    if (mf_at != 0u) mf_rec = p.scene.blob[p.scene.blob_vec4 + mf_at + (mat_bits & RT_MAT_INDEX_MASK)];
                    mf_rough = __uint_as_float(mf_rec.z);
                } else if constexpr (MFAC) {
                    const uint32_t mf_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].x) >> 1;
                    if (mf_at != 0u) mf_rec = p.scene.blob[p.scene.blob_vec4 + mf_at + (mat_bits & RT_MAT_INDEX_MASK)];
                    mf_rough = __uint_as_float(mf_rec.z);
                }
                if constexpr (NMAP) {
                    const uint32_t tex_here = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].w);
                    if (tex_here != 0u) {
                        const uint4* tt = p.scene.blob + p.scene.blob_vec4 + tex_here;
                        const uint4 th = tt[0];
                        const uint32_t nm_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)th.w);
                        const bool mf_mapped = MFAC && (mf_rec.x == RT_MICROFACET_MAPPED || mf_rec.x == RT_MICROFACET_GLASS_MAPPED);   // §30: a frosted surface under its map
                        if (nm_at != 0u || mf_mapped) {
                            uint4 nr = make_uint4(0u, 0u, 0u, 0u);
                            if (!MFAC || nm_at != 0u) nr = tt[nm_at + (mat_bits & RT_MAT_INDEX_MASK)];   // (on, image, strength bits, -): per lane, lanes sit on different materials
                            if (nr.x != 0u || mf_mapped) {
                                f3 dPdu, dPdv;
                                bool frame = true;
                                if ((uint32_t)rec_code >= p.scene.sphere_codes) {
                                    const uint32_t qi = (uint32_t)rec_code - p.scene.sphere_codes;
                                    const float4* qd = quads + qi * 4u;
                                    const float4 a0 = qd[0], a1 = qd[1], a2 = qd[2], a3 = qd[3];
                                    const f3 qu = mk3(a1.x, a1.y, a1.z), qv = mk3(a1.w, a2.x, a2.y);
                                    if (uv_at != 0u && qi >= p.scene.n_plain_quads) {
                                        const float* tr = reinterpret_cast<const float*>(p.scene.blob + p.scene.blob_vec4 + uv_at) + (size_t)(qi - p.scene.n_plain_quads) * 6u;
                                        const float t0[2] = {tr[0], tr[1]}, t1[2] = {tr[2], tr[3]}, t2[2] = {tr[4], tr[5]};
                                        tri_uv(mk3(a0.x, a0.y, a0.z), qu, qv, mk3(a3.y, a3.z, a3.w), t0, t1, t2, hit_p, nm_tu, nm_tv);
                                        frame = normal_map_tri_tangents(qu, qv, t0, t1, t2, dPdu, dPdv);
                                    } else {
                                        quad_uv(mk3(a0.x, a0.y, a0.z), qu, qv, mk3(a3.y, a3.z, a3.w), hit_p, nm_tu, nm_tv);
                                        dPdu = qu; dPdv = qv;
                                    }
                                } else {
                                    sphere_uv(normal, nm_tu, nm_tv);
                                    normal_map_sphere_tangents(normal, dPdu, dPdv);
                                }
                                nm_uv = true;
                                if (frame && (!MFAC || nr.x != 0u)) {
                                    const uint64_t texels = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.y) << 32;
                                    normal_map_apply(texture_value(reinterpret_cast<const uint32_t*>(texels), tt[1u + nr.y], nm_tu, nm_tv), __uint_as_float(nr.z), dPdu, dPdv, ray.d, normal);
                                }
                                if constexpr (MFAC) {
                                    if (mf_mapped) {   // §29: the roughness map, at the same (u, v)
                                        const uint64_t texels = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)th.y) << 32;
                                        mf_rough = microfacet_roughness(mf_rough, texture_value(reinterpret_cast<const uint32_t*>(texels), tt[1u + mf_rec.y], nm_tu, nm_tv));
                                    }
                                }
                            }
                        }
                    }
                }
                const uint32_t mtype = mat_bits >> 29;
                const float4 mrec = mats16[mat_bits & RT_MAT_INDEX_MASK];
                f3 albedo = mk3(mrec.x, mrec.y, mrec.z);
                const float mparam = mrec.w;

                // EXT: emitted radiance of a diffuse light is added before the scatter decision (accum_radiance of
                // Renderer.cu:157-163); a light never scatters; the last allowed bounce still collects emission.
                bool path_over = false;
                if (EXT) {
                    if (mtype == RT_MAT_DIFFUSE_LIGHT) { accum_rad = accum_rad + atten * albedo; path_over = true; }
                    if (depth + 1u >= p.max_depth) path_over = true;
                }
                RT_PT(9);
                // ---- Scatter (cu_materials.cuh:52-64 / 77-95 / 115-143 / 27-40); per-lane arithmetic is
                // ---- material_scatter()'s, expression by expression.
                const bool is_diel = (mtype == RT_MAT_DIELECTRIC);
                f3 unit_dir = mk3(0.0f);
                float ior_ratio = 0.0f, reflect_prob = 0.0f;
                bool must_reflect = false;
                if (is_diel && !path_over) {
                    if constexpr (INTR) {
                        // §32: the interior record of the hit's material, (on, sigma bits x 3), read here alone so that nothing of it lives across the phase.  With a
                        // record, a parallelogram or triangle takes its facing from the stored normal (q_back; the shading normal already faces the ray and stays),
                        // a sphere the expression it always took; a back hit ended a segment inside the glass and is charged for it before either rule below.
                        uint4 in_rec = make_uint4(0u, 0u, 0u, 0u);
                        const uint32_t sub_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].x) >> 1;
                        if (sub_at != 0u) {
                            const uint32_t in_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4 + sub_at].y);
                            if (in_at != 0u) in_rec = p.scene.blob[p.scene.blob_vec4 + in_at + (mat_bits & RT_MAT_INDEX_MASK)];
                        }
                        const bool solid = in_rec.x != 0u;
                        bool hit_backface;
                        if (solid && (uint32_t)rec_code >= p.scene.sphere_codes) hit_backface = q_back;
                        else {
                            hit_backface = dot(ray.d, normal) > 0;
                            if (hit_backface) normal = -normal;
                        }
                        if (solid) {
                            f3 in_T;
                            interior_hit(hit_backface, ray.d, rec_t, mparam, mk3(__uint_as_float(in_rec.y), __uint_as_float(in_rec.z), __uint_as_float(in_rec.w)), ior_ratio, in_T);
                            if (hit_backface) albedo = albedo * in_T;
                        } else ior_ratio = hit_backface ? mparam : 1 / mparam;
                    } else {
                    bool hit_backface = dot(ray.d, normal) > 0;
                    if (hit_backface) normal = -normal;
                    ior_ratio = hit_backface ? mparam : 1 / mparam;
                    }
                    unit_dir = normalize(ray.d);
                    float cos_theta = fminf(dot(-unit_dir, normal), 1.0f);
                    float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
                    reflect_prob = reflectance(cos_theta, ior_ratio);
                    must_reflect = ior_ratio * sin_theta > 1.0f;  // short-circuit: no uniform is drawn
                }
                RT_PT(10);
                f3 scatter_dir = mk3(0.0f);
                bool scattered_ok = !path_over;
                float nee_weight = 1.0f;   // NEE: cosine density / mixture density of the direction taken, at a Lambertian / checker hit
                bool nee_weighted = false;
                if (path_over) {
                    // nothing to sample: the path ends here with what it has collected
                } else if (is_diel) {
                    // §30: glass with a rough-glass record (the table admits no other kind on a dielectric) reflects or refracts about a micro-normal, from the
                    // facing the block above has just left in `normal` and ior_ratio — step 1 of the rule in its own expressions.  Specular or transmitted: the
                    // rule's direction, the albedo times its weight; absorbed: a failed scatter; base (a grazing or NaN cosine): the smooth hit, verbatim.
                    // (The smooth hit stands twice so that the forms without MFAC are the statements they were, to the compiler too.)
                    if constexpr (MFAC) {
                        bool gl_done = false;
                        if (mf_rec.x != 0u) {
                            float gl_weight = 0.0f;
                            const uint32_t way = rough_glass_faced(normal, ior_ratio, ray.d, mf_rough, rng, scatter_dir, gl_weight);
                            if (way == RT_MFAC_SPECULAR || way == RT_MFAC_TRANSMITTED) { albedo = albedo * gl_weight; gl_done = true; }
                            else if (way == RT_MFAC_ABSORBED) { scattered_ok = false; gl_done = true; }
                        }
                        if (!gl_done) {
                            if (must_reflect || reflect_prob > rng.next()) scatter_dir = reflect(unit_dir, normal);
                            else scatter_dir = refract(unit_dir, normal, ior_ratio);
                        }
                    } else {
                    if (must_reflect || reflect_prob > rng.next()) scatter_dir = reflect(unit_dir, normal);
                    else scatter_dir = refract(unit_dir, normal, ior_ratio);
                    }
                } else {
                    RT_PT(11);
                    // §29: a material with a microfacet record — a metal as a rough conductor with F0 = its albedo, the Lambertian kinds under a coat — before any
                    // draw of the base.  Specular: the direction and the factor of the throughput are the rule's; absorbed: a failed scatter.  Otherwise (the coat's
                    // toss fell to the base, or the surface is seen from behind) everything below runs as if there were no record.
                    bool mf_done = false;
                    if constexpr (MFAC) {
                        if (mf_rec.x != 0u) {
                            const bool coat = mtype != RT_MAT_METAL;
                            f3 mf_weight = mk3(0.0f);
                            const uint32_t way = microfacet_scatter(normal, ray.d, mf_rough, coat ? mk3(__uint_as_float(mf_rec.w)) : albedo, coat, rng, scatter_dir, mf_weight);
                            if (way == RT_MFAC_SPECULAR) { albedo = mf_weight; mf_done = true; }
                            else if (way == RT_MFAC_ABSORBED) { scattered_ok = false; mf_done = true; }
                        }
                    }
                    if (!(MFAC && mf_done)) {
                    // NEE: the first draw of a Lambertian / checker hit picks the half of the mixture; the light half draws no on-unit vector
                    const bool nee_mat = NEE && (mtype == RT_MAT_LAMBERTIAN || mtype == RT_MAT_LAMBERTIAN_CHECKER || (ENVT && mtype == RT_MAT_LAMBERTIAN_IMAGE));
                    const bool to_light = nee_mat && rng.next() < 0.5f;
                    bool to_env = ENVL;   // §26: which light the light half goes to — the map unless a second draw says the table; with an empty table no draw is made
                    if constexpr (ENVT) {
                        if (to_light && __float_as_uint((quads + p.scene.n_quads * 5u)[0].x) != 0u) to_env = rng.next() < 0.5f;
                    }
                    f3 on_unit = mk3(0.0f);
                    uint32_t nee_li = 0u, nee_quad = 0u;   // NEE, light half: the light drawn, and its quad index
                    bool to_sphere = false;                // ... or that it is a sphere light (§17), whose point is C + on_unit * r: the draw below serves it too
                    bool to_tri = false;                   // ... or a triangle light (§19, TRI only): a quad's two draws, folded into the triangle
                    if constexpr (!ENVL || LTREE)   // (§24: the map is the one light; its draws are made where the direction is)
                    if (NEE && to_light && !(ENVT && to_env)) {
                        const float4* lights = quads + p.scene.n_quads * 5u;
                        const uint32_t n_l = __float_as_uint(lights[0].x);
                        if constexpr (LTREE) {   // §20: the smallest j with c_j > x, x = next * A; none (x rounded up to A): the last light
                            if (n_l > 1u) {
                                const float x = rng.next() * lights[0].y;
                                uint32_t hi = n_l - 1u;
                                while (nee_li < hi) {
                                    const uint32_t mid = (nee_li + hi) >> 1;
                                    if (lights[1u + mid].w > x) hi = mid;
                                    else nee_li = mid + 1u;
                                }
                            }
                        } else
                        if (n_l > 1u) nee_li = min((uint32_t)(rng.next() * (float)n_l), n_l - 1u);
                        const float4 le = lights[1u + nee_li];
                        nee_quad = __float_as_uint(le.x);
                        if constexpr (TRI) {
                            to_sphere = __float_as_uint(le.z) == RT_LIGHT_SPHERE;
                            to_tri = __float_as_uint(le.z) == RT_LIGHT_TRIANGLE;
                        } else {
                            to_sphere = __float_as_uint(le.z) != 0u;
                        }
                        if (to_sphere) nee_li += n_l;      // where its (Cx, Cy, Cz, r) lies behind the entries
                    }
                    if (!NEE || !to_light || to_sphere) on_unit = rng_on_unit3(rng);
                    RT_PT(12);
                    if (EXT && mtype == RT_MAT_ISOTROPIC) {
                        scatter_dir = on_unit;   // isotropic phase function: any direction, never absorbed
                    } else if (mtype == RT_MAT_METAL) {
                        scatter_dir = reflect(ray.d, normal) + on_unit * mparam;
                        scattered_ok = !(dot(scatter_dir, normal) < 0 || near_zero(scatter_dir));
                    } else {
                        if constexpr (ENVL) {
                            if (to_light && to_env) {   // §24: four draws, then the rule; the record through scalars as the miss branch reads it
                                const EnvRecord er = load_env_record(p.scene.blob + p.scene.blob_vec4 + env_at);
                                const float x1 = rng.next();
                                const float x2 = rng.next();
                                const float ea = rng.next();
                                const float eb = rng.next();
                                scatter_dir = environment_sample(er.dist, er.w, er.h, er.u0, x1, x2, ea, eb, nullptr);
                            } else if (!LTREE || !to_light) {
                                scatter_dir = normal + on_unit;
                                scattered_ok = !near_zero(scatter_dir);
                            }
                        }
                        if (ENVL && !(ENVT && to_light && !to_env)) {
                            // (drawn above; §26: all but a light half that goes to the table, whose point is mode 16's below)
                        } else
                        if (NEE && to_light) {   // a point of light i, uniform over its area; the direction stays unnormalised
                            if (to_sphere) {
                                const float4 sc = (quads + p.scene.n_quads * 5u)[1u + nee_li];
                                scatter_dir = (mk3(sc.x, sc.y, sc.z) + on_unit * sc.w) - hit_p;
                            } else {
                            float la = rng.next();
                            float lb = rng.next();
                            if constexpr (TRI) {
                                if (to_tri && la + lb > 1.0f) { la = 1.0f - la; lb = 1.0f - lb; }   // one fp32 add decides; a sum of exactly 1 stays
                            }
                            const float4* qd = quads + nee_quad * 4u;
                            const float4 a0 = qd[0], a1 = qd[1], a2 = qd[2];
                            scatter_dir = ((mk3(a0.x, a0.y, a0.z) + mk3(a1.x, a1.y, a1.z) * la) + mk3(a1.w, a2.x, a2.y) * lb) - hit_p;
                            }
                        } else {
                        scatter_dir = normal + on_unit;
                        scattered_ok = !near_zero(scatter_dir);
                        }
                        if (NEE && nee_mat && scattered_ok) {
                            // densities of the direction under both halves, from hit_p before the offset: cosine, and per light the solid-angle density
                            // of its area where the ray (hit_p, d) meets it — quad::hit as the leaf phase runs it, on a fresh trace's interval
                            const f3 d = scatter_dir;
                            const float len2 = dot(d, d), len = sqrtf(len2), cosn = dot(normal, d) / len;
                            const float pdf_cos = cosn > 0 ? cosn * 0.318309886f : 0.0f;
                            float pdf_light = 0.0f;
                            float pdf_env = 0.0f;
                            if constexpr (ENVL) {   // §24: the density of the texel §23's lookup puts d in; no division by a light count
                                const EnvRecord er = load_env_record(p.scene.blob + p.scene.blob_vec4 + env_at);
                                pdf_env = environment_density(er.texels, er.w, er.h, er.u0, d);
                                if constexpr (!LTREE) pdf_light = pdf_env;
                            }
                            if constexpr (!ENVL || LTREE) {
                            const float4* lights = quads + p.scene.n_quads * 5u;
                            const uint32_t n_l = __float_as_uint(lights[0].x);
                            Ray lray;
                            lray.o = hit_p; lray.d = d; lray.time = ray.time;
                            if constexpr (LTREE) {
                                if (ENVT && n_l == 0u) pdf_light = pdf_env;   // §26: an empty table: the map alone, and no walk
                                else {
                                // §20: the threaded tree of the lights' padded boxes, in preorder; a leaf met adds mode 4's term without its division by area_j,
                                // in ascending table position — the linear loop's order with its zeros left out — and the sum is divided by A once
                                const float4* tnodes = lights + 1u + 2u * n_l;
                                const uint32_t n_nodes = 2u * n_l - 1u;
                                const f3 rd = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
                                bool own_met = !to_sphere;   // a drawn sphere whose leaf the walk credits with disc > 0
                                uint32_t i = 0u;
                                while (i < n_nodes) {
                                    const float4 b0 = tnodes[2u * i], b1 = tnodes[2u * i + 1u];
                                    const f3 ta = (mk3(b0.x, b0.y, b0.z) - hit_p) * rd, tb = (mk3(b1.x, b1.y, b1.z) - hit_p) * rd;
                                    const float tmin = comp_max(glm_min(ta, tb)), tmax = comp_min(glm_max(ta, tb));
                                    const uint32_t leaf = __float_as_uint(b1.w);
                                    if (!(tmin <= tmax * RT_LIGHT_TREE_K && tmax > 0)) { i = __float_as_uint(b0.w); continue; }
                                    if (leaf == 0xffffffffu) { i++; continue; }
                                    i = __float_as_uint(b0.w);
                                    const float4 lt = lights[1u + leaf];
                                    if (__float_as_uint(lt.z) == RT_LIGHT_SPHERE) {
                                        const float4 sc = lights[1u + n_l + leaf];
                                        const f3 oc = mk3(sc.x, sc.y, sc.z) - hit_p;
                                        const float h = dot(d, oc);
                                        const f3 cr = cross(oc, d);
                                        const float disc = (sc.w * sc.w) * len2 - dot(cr, cr);
                                        if (disc > 0) {
                                            if (nee_li == n_l + leaf) own_met = true;
                                            const float sq = sqrtf(disc);
                                            const float den = (sq / sc.w) / len;
                                            const float t1 = (h - sq) / len2, t2 = (h + sq) / len2;
                                            float pl_j = 0.0f;
                                            if (t1 > 0) pl_j = pl_j + ((t1 * t1) * len2) / den;
                                            if (t2 > 0) pl_j = pl_j + ((t2 * t2) * len2) / den;
                                            pdf_light = pdf_light + pl_j;
                                        }
                                    } else {
                                        const float4* qd = quads + __float_as_uint(lt.x) * 4u;
                                        const float4 a0 = qd[0], a1 = qd[1], a2 = qd[2], a3 = qd[3];
                                        const f3 ln = mk3(a2.z, a2.w, a3.x);
                                        HitRec tmp;
                                        tmp.distance = RT_MISS_DIST; tmp.normal = mk3(0.0f); tmp.prim = -1; tmp.mat = 0;
                                        if (quad_closest_intersection(mk3(a0.x, a0.y, a0.z), a0.w, mk3(a1.x, a1.y, a1.z), mk3(a1.w, a2.x, a2.y), ln, mk3(a3.y, a3.z, a3.w), 0u, 0,
                                                                      __float_as_uint(lt.z) == RT_LIGHT_TRIANGLE ? RT_QUAD_TRIANGLE : RT_QUAD_PARALLELOGRAM, lray, tmp))
                                            pdf_light = pdf_light + ((tmp.distance * tmp.distance) * len2) / (fabsf(dot(d, ln)) / len);
                                    }
                                }
                                if (!own_met) scattered_ok = false;   // §17's silhouette rule, for a walk that may not reach the leaf
                                pdf_light = pdf_light / lights[0].y;
                                if constexpr (ENVT) pdf_light = 0.5f * pdf_env + 0.5f * pdf_light;   // §26: pm, the light half's own mixture
                                }
                            } else {
                            for (uint32_t j = 0; j < n_l; j++) {
                                const float4 lt = lights[1u + j];
                                float pl_j = 0.0f;
                                if (TRI ? __float_as_uint(lt.z) == RT_LIGHT_SPHERE : __float_as_uint(lt.z) != 0u) {
                                    // a sphere light (§17): the area-uniform point's solid-angle density, summed over both crossings of the line through the
                                    // sphere; |n.d| = sqrt(disc) / r at both
                                    const float4 sc = lights[1u + n_l + j];
                                    const f3 oc = mk3(sc.x, sc.y, sc.z) - hit_p;
                                    const float h = dot(d, oc);
                                    const f3 cr = cross(oc, d);
                                    const float disc = (sc.w * sc.w) * len2 - dot(cr, cr);   // = h^2 - len2 (|oc|^2 - r^2), without the cancellation of numbers of size len2 |oc|^2
                                    if (!(disc > 0)) {
                                        if (to_sphere && nee_li == n_l + j) scattered_ok = false;   // the drawn point itself, lost on the silhouette: a failed scatter
                                    } else {
                                        const float sq = sqrtf(disc);
                                        const float den = ((sq / sc.w) / len) * lt.y;
                                        const float t1 = (h - sq) / len2, t2 = (h + sq) / len2;
                                        if (t1 > 0) pl_j = pl_j + ((t1 * t1) * len2) / den;
                                        if (t2 > 0) pl_j = pl_j + ((t2 * t2) * len2) / den;
                                    }
                                } else {
                                const float4* qd = quads + __float_as_uint(lt.x) * 4u;
                                const float4 a0 = qd[0], a1 = qd[1], a2 = qd[2], a3 = qd[3];
                                const f3 ln = mk3(a2.z, a2.w, a3.x);
                                HitRec tmp;
                                tmp.distance = RT_MISS_DIST; tmp.normal = mk3(0.0f); tmp.prim = -1; tmp.mat = 0;
                                if (quad_closest_intersection(mk3(a0.x, a0.y, a0.z), a0.w, mk3(a1.x, a1.y, a1.z), mk3(a1.w, a2.x, a2.y), ln, mk3(a3.y, a3.z, a3.w), 0u, 0,
                                                              TRI && __float_as_uint(lt.z) == RT_LIGHT_TRIANGLE ? RT_QUAD_TRIANGLE : RT_QUAD_PARALLELOGRAM, lray, tmp))   // §19: a triangle light's area (lt.y) is half its parallelogram's
                                    pl_j = ((tmp.distance * tmp.distance) * len2) / ((fabsf(dot(d, ln)) / len) * lt.y);
                                }
                                pdf_light = pdf_light + pl_j;
                            }
                            pdf_light = pdf_light / (float)n_l;
                            }
                            }
                            const float pdf = 0.5f * pdf_cos + 0.5f * pdf_light;
                            if (pdf_cos == 0.0f || !(pdf > 0)) scattered_ok = false;   // below the surface, or a density that is not a number: a failed scatter
                            else { nee_weight = pdf_cos / pdf; nee_weighted = true; }
                        }
                        if (mtype == RT_MAT_LAMBERTIAN_CHECKER) {
                            const rt_material& mg = p.scene.mats[mat_bits & RT_MAT_INDEX_MASK];
                            albedo = checker_value(albedo, mk3(mg.albedo2[0], mg.albedo2[1], mg.albedo2[2]), mparam, hit_p);
                        }
                        if (EXT >= 2 && mtype == RT_MAT_LAMBERTIAN_NOISE) albedo = noise_value(p.scene.perlin, albedo, mparam, hit_p);
                        if (EXT >= 2 && mtype == RT_MAT_LAMBERTIAN_IMAGE) {   // (u, v) three ways, then the world's image or — §25 — the material's entry of the texture table
                            float tu, tv;
                            if (NMAP && nm_uv) { tu = nm_tu; tv = nm_tv; }   // §28: the map's own (u, v)
                            else
                            if ((uint32_t)rec_code >= p.scene.sphere_codes) {   // on a quad: the planar coordinates of the hit
                                const uint32_t qi = (uint32_t)rec_code - p.scene.sphere_codes;
                                const float4* qd = quads + qi * 4u;
                                const float4 a0 = qd[0], a1 = qd[1], a2 = qd[2], a3 = qd[3];
                                if (TRI && uv_at != 0u && qi >= p.scene.n_plain_quads) {   // §22: a triangle under a table of texture coordinates weighs its vertices' (u, v)
                                    const float* tr = reinterpret_cast<const float*>(p.scene.blob + p.scene.blob_vec4 + uv_at) + (size_t)(qi - p.scene.n_plain_quads) * 6u;
                                    const float t0[2] = {tr[0], tr[1]}, t1[2] = {tr[2], tr[3]}, t2[2] = {tr[4], tr[5]};
                                    tri_uv(mk3(a0.x, a0.y, a0.z), mk3(a1.x, a1.y, a1.z), mk3(a1.w, a2.x, a2.y), mk3(a3.y, a3.z, a3.w), t0, t1, t2, hit_p, tu, tv);
                                } else
                                quad_uv(mk3(a0.x, a0.y, a0.z), mk3(a1.x, a1.y, a1.z), mk3(a1.w, a2.x, a2.y), mk3(a3.y, a3.z, a3.w), hit_p, tu, tv);
                            } else {
                                sphere_uv(normal, tu, tv);
                            }
                            const uint32_t tex_here = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.scene.blob[p.scene.blob_vec4].w);   // the tail header's fourth word: wave-uniform
                            if (tex_here != 0u) albedo = texture_table_value(p.scene.blob + p.scene.blob_vec4 + tex_here, (uint32_t)mparam, tu, tv);
                            else albedo = image_texel(p.scene.image, p.scene.image_w, p.scene.image_h, tu, tv);
                        }
                    }
                    }   // (§29: not a specular or absorbed microfacet hit)
                }
                RT_PT(13);
                if (!scattered_ok) {
                    RT_EMIT_DARK();
                } else {
                    if (NEE && nee_weighted) albedo = albedo * nee_weight;
                    atten = atten * albedo;
                    ray.o = hit_p;
                    ray.d = scatter_dir;  // time is inherited
                    ray.o = ray.o + ray.d * 0.001f;  // Renderer.cu:175
                    depth++;
                    start_trace = true;
                }
            }
        }

        RT_PT(3);
        // ---- hand new samples to the lanes that need one (wave-uniform loop).  The primary ray of sample index n
        // ---- (pixel jitter, camera sample, RNG state after those draws: Renderer.cu:199-201) was computed by
        // ---- primary_rays_kernel with every lane busy; here a lane only loads its 48-byte record.
        for (;;) {
            uint64_t m_need = __ballot(cur == K::NEED);
            if (m_need == 0ull) break;
            if (pool_next == pool_end) {
                if (pool_dry) break;
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(p.work_counter, p.chunk);
                base = __builtin_amdgcn_readfirstlane(base);
                if (base >= p.total) { pool_dry = true; break; }
                pool_next = base;
                pool_end = min(base + p.chunk, p.total);
            }
            uint32_t take = min(pool_end - pool_next, (uint32_t)__popcll(m_need));
            uint32_t rank = lane_rank(m_need);
            if (cur == K::NEED && rank < take) {
                const uint32_t n = pool_next + rank;
                // all three 16-byte parts of the record go out together: ONE global round trip (a padding pixel's two extra loads are wasted, rarely)
                const uint4 rs = RT_LOAD_ONCE(p.prim_rng + n);
                const float4 po = RT_LOAD_ONCE(p.prim_o + n), pd = RT_LOAD_ONCE(p.prim_d + n);
                asm volatile("" : : "v"(po.x), "v"(pd.x));   // keeps the compiler from sinking the two loads below the test (a second, dependent round trip)
                if ((rs.x | rs.y | rs.z | rs.w) != 0u) {
                    out_idx = n;
                    ray.o = mk3(po.x, po.y, po.z); ray.d = mk3(pd.x, pd.y, pd.z); ray.time = po.w;
                    rng.s0 = rs.x; rng.s1 = rs.y; rng.s2 = rs.z; rng.s3 = rs.w;
                    atten = mk3(1.0f);
                    if (EXT) accum_rad = mk3(0.0f);
                    depth = 0;
                    if (p.max_depth == 0u) {
                        RT_EMIT(0.0f, 0.0f, 0.0f);
                    } else {
                        start_trace = true;
                        cur = K::START;  // no longer K::NEED, so the loop does not hand it another sample
                    }
                }
                // a padding pixel (outside the image / past the last tile) consumes the index and the lane asks again
            }
            pool_next += take;
        }
        RT_PT(4);
        // BVH.cu:59-60 / HittableList.cuh:22: root (world) box first, against rec.distance (= _MISS_DIST for a fresh
        // payload); bvh_node.cuh:20 tests a node's own box when it is visited, so a tree starts at its root unconditionally.
        if (start_trace) {
            rec_t = RT_MISS_DIST;
            rec_code = -1;
            if (WORLD == RT_WORLD_BVH_QUEUE) {   // the whole trace, by this lane alone; leaf code as the shade phase wants it
                HitRec qrec;
                qrec.distance = RT_MISS_DIST; qrec.normal = mk3(0.0f); qrec.prim = -1; qrec.mat = 0;
                if (p.world.traversal == RT_TRAVERSAL_WIDE4 ? bvh_closest_intersection_wide4(p.world, ray, qrec, &rng)
                                                             : bvh_closest_intersection_queue(p.world, ray, qrec, &rng)) {
                    const uint32_t qp = (uint32_t)qrec.prim;
                    rec_t = qrec.distance;
                    rec_code = qp < p.scene.n_prims ? (int32_t)(qp * 2u + ((p.world.prims[qp].mat & RT_PRIM_MOVING) ? 1u : 0u))
                                                    : (int32_t)(p.scene.sphere_codes + (qp - p.scene.n_prims));
                }
                cur = K::SHADE;
            } else {
                ray_a = dot(ray.d, ray.d);
                if (!EXACT) {
                    regular = ray_is_regular(ray);
                    inv_d = mk3(rcp_exact_regular(ray.d.x), rcp_exact_regular(ray.d.y), rcp_exact_regular(ray.d.z));   // used by regular rays only
                    if (FAST_BVH && !TOL) inv_lo = mk3(rcp_low_word(ray.d.x, inv_d.x), rcp_low_word(ray.d.y, inv_d.y), rcp_low_word(ray.d.z, inv_d.z));
                    if (FAR_FMA) { far_c = slab_fma_offset(ray, inv_d); far_s_eps = slab_fma_margin(far_c); }
                    const uint32_t km = (regular && FAST_BVH) ? 4u : 0u;
                    kx = (__float_as_uint(ray.d.x) >> 29) & km;
                    ky = (__float_as_uint(ray.d.y) >> 29) & km;
                    kz = (__float_as_uint(ray.d.z) >> 29) & km;
                }
                float d_root;
                bool hit_root;
                if (WORLD == RT_WORLD_NODE_TREE) hit_root = true;
                else if (EXACT || !regular) hit_root = aabb_intersects(root_min, root_max, ray, rec_t, d_root);
                else hit_root = root_box_hit_certified(root_min, root_max, ray, inv_d);   // rec_t is _MISS_DIST here
                if (hit_root) {
                    cur = p.scene.root_ref;
                    if (FAST_BVH && !regular && cur < K::LEAF) cur |= K::IRR;
                    sp = stack + 64;
                } else {
                    cur = K::SHADE;
                }
            }
        }
        if (FAST_BVH && __ballot(start_trace && !regular) != 0ull) irr_pending = true;
        if (pool_dry && cur == K::NEED) cur = K::OFF;
        RT_PT(5);
        if (__ballot(cur != K::OFF) == 0ull) break;
    }
#ifdef RT_PHASE_TIMERS
    if (lane == 0)
        for (int i = 0; i < 16; i++) { atomicAdd(p.phase_acc + i, pt_[i]); atomicAdd(p.phase_acc + 16 + i, (unsigned long long)pc_[i]); }
#endif
#undef RT_PT
#undef RT_POP
#undef RT_EMIT
#undef RT_EMIT_DARK
}

// Primary rays of one pass: one thread per sample index n = (block * pass_spp + s) * 64 + pixel-in-block (the index space
// the streaming kernel consumes; blockIdx.y = block, so no integer division).  Renderer.cu:188-201: pixel centre in NDC,
// jitter in a disc of half a pixel (cuRandomInUnit<2>), camera sample_ray — with the per-sample counter-based RNG stream
// (Philox seed, then the sequential draws).  Done here, with every lane busy, instead of inside the persistent kernel where
// only the ~21 lanes of a wave whose path just ended would run it (it was 12 % of that kernel's time at one-third lane
// utilisation).  Writes 48 B per sample: (origin, time), (direction, -), RNG state after the camera's draws.
// The two rejection loops of a defocus camera (pixel jitter, lens point: glm_utils.h:84-90 twice) run as ONE loop whose
// iterations serve whichever of the two a lane is at — the same draws in the same order per lane, but the wave iterates
// max(tries_jitter + tries_lens) times instead of max(tries_jitter) + max(tries_lens).
__global__ __launch_bounds__(256) void primary_rays_kernel(StreamParams p, uint32_t first_blk) {
    const uint32_t blk = first_blk + blockIdx.y;
    const uint32_t rem = blockIdx.x * 256u + threadIdx.x;   // index inside the block's 64 * pass_spp samples
    if (rem >= 64u * p.pass_spp) return;
    const uint32_t n = blk * (64u * p.pass_spp) + rem;
    const uint32_t s_local = rem >> 6, pix = rem & 63u;
    uint32_t x0, y0;
    const bool ok = block_origin(p.tm, blk, x0, y0);
    const uint32_t x = x0 + (pix & 7u), y = y0 + (pix >> 3);
    if (!(ok && x < p.width && y < p.height)) {   // padding pixel: outside the image / past the last tile
        p.prim_rng[n] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    Rng rng;
    rng.init(p.seed, y * p.width + x, p.pass_first_s + s_local, RT_STREAM_RENDER);
    float psx, psy, ndcx, ndcy;
    pixel_ndc(x, y, p.width, p.height, psx, psy, ndcx, ndcy);
    float jx = 0.0f, jy = 0.0f, a = 0.0f, b = 0.0f;
    if (p.cam.type == RT_CAM_DEFOCUS) {
        uint32_t stage = 0;   // 0: pixel jitter (Renderer.cu:199), 1: lens point (cu_Cameras.cuh:55), 2: done
        do {
            const float u = rng.next_signed();
            const float v = rng.next_signed();
            if (length2(u, v) < 1.0f) {
                if (stage == 0u) { jx = u; jy = v; } else { a = u; b = v; }
                stage++;
            }
        } while (stage < 2u);
    } else {
        rng_in_unit2(rng, jx, jy);
        camera_draw(p.cam, rng, a, b);
    }
    const Ray ray = camera_ray(p.cam, ndcx + jx * psx, ndcy + jy * psy, a, b);
    rt_store_stream(p.prim_o + n, make_float4(ray.o.x, ray.o.y, ray.o.z, ray.time));
    rt_store_stream(p.prim_d + n, make_float4(ray.d.x, ray.d.y, ray.d.z, 0.0f));
    rt_store_stream(p.prim_rng + n, make_uint4(rng.s0, rng.s1, rng.s2, rng.s3));
}

// The same pass for a lens camera (rt06.h: types 16 to 19): primary_rays_kernel's index space, padding rule and three records, the ray from
// lens_camera_ray.  PROJ = type - RT_CAM_PERSPECTIVE, LENS = lens_radius > 0, SHUTTER = t0 != t1 are the host's reading of the camera at launch time, so each of
// the sixteen forms holds one projection and only the draws it makes.  With LENS the two rejection loops run as one, as in the DEFOCUS branch above.
template <uint32_t PROJ, bool LENS, bool SHUTTER>
__global__ __launch_bounds__(256) void primary_rays_lens_kernel(StreamParams p, uint32_t first_blk) {
    const uint32_t blk = first_blk + blockIdx.y;
    const uint32_t rem = blockIdx.x * 256u + threadIdx.x;   // index inside the block's 64 * pass_spp samples
    if (rem >= 64u * p.pass_spp) return;
    const uint32_t n = blk * (64u * p.pass_spp) + rem;
    const uint32_t s_local = rem >> 6, pix = rem & 63u;
    uint32_t x0, y0;
    const bool ok = block_origin(p.tm, blk, x0, y0);
    const uint32_t x = x0 + (pix & 7u), y = y0 + (pix >> 3);
    if (!(ok && x < p.width && y < p.height)) {   // padding pixel: outside the image / past the last tile
        p.prim_rng[n] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    Rng rng;
    rng.init(p.seed, y * p.width + x, p.pass_first_s + s_local, RT_STREAM_RENDER);
    float psx, psy, ndcx, ndcy;
    pixel_ndc(x, y, p.width, p.height, psx, psy, ndcx, ndcy);
    float jx = 0.0f, jy = 0.0f, la = 0.0f, lb = 0.0f;
    if (LENS) {
        uint32_t stage = 0;   // 0: pixel jitter, 1: lens point, 2: done
        do {
            const float u = rng.next_signed();
            const float v = rng.next_signed();
            if (length2(u, v) < 1.0f) {
                if (stage == 0u) { jx = u; jy = v; } else { la = u; lb = v; }
                stage++;
            }
        } while (stage < 2u);
    } else {
        rng_in_unit2(rng, jx, jy);
    }
    const float time = SHUTTER ? mix(p.cam.t0, p.cam.t1, rng.next()) : p.cam.t0;
    const Ray ray = lens_camera_ray(p.cam, PROJ, LENS, ndcx + jx * psx, ndcy + jy * psy, la, lb, time);
    rt_store_stream(p.prim_o + n, make_float4(ray.o.x, ray.o.y, ray.o.z, ray.time));
    rt_store_stream(p.prim_d + n, make_float4(ray.d.x, ray.d.y, ray.d.z, 0.0f));
    rt_store_stream(p.prim_rng + n, make_uint4(rng.s0, rng.s1, rng.s2, rng.s3));
}

// The two steps every resolve shares, so that a frame refined in steps and a frame rendered in one call cannot drift apart:
//   add_pass_samples: the samples of one pass added to a pixel's sum IN SAMPLE ORDER (Renderer.cu:198-204: `radiance += ...`);
//   resolve_pixel:    mean / clamp / sqrt-gamma / alpha over n_samples (Renderer.cu:206-216).
// WITH_Q (refinement): in the same loop, q += Y * Y with the sample's luminance Y = (0.2126 r + 0.7152 g) + 0.0722 b, every operation
// rounded on its own (the library is built without contraction; the _rn intrinsics say it again), so numpy float32 restates it bit for bit.
template <bool WITH_Q>
__device__ __forceinline__ f3 add_pass_samples(const StreamParams& p, uint32_t L, f3 radiance, float& q) {
    size_t src = (size_t)(L >> 6) * p.pass_spp * 64u + (L & 63u);   // 64 consecutive pixels per sample row: coalesced
    for (uint32_t s = 0; s < p.pass_spp; s++) {
        const f3 c = load_sample(p.samples, src);
        radiance = radiance + c;
        if (WITH_Q) {
            const float y = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, c.x), __fmul_rn(0.7152f, c.y)), __fmul_rn(0.0722f, c.z));
            q = __fadd_rn(q, __fmul_rn(y, y));
        }
        src += 64u;
    }
    return radiance;
}
__device__ __forceinline__ float4 resolve_pixel(f3 radiance, uint32_t n_samples) {
    radiance = radiance * (1.0f / (float)n_samples);
    const f3 col = clamp01_sqrt(radiance);
    return make_float4(col.x, col.y, col.z, 1.0f);
}

// Adds the samples of one pass to each pixel IN SAMPLE ORDER (Renderer.cu:198-204: `radiance += ...`),
// and on the last pass applies mean / clamp / sqrt-gamma / alpha (Renderer.cu:206-216).
__global__ __launch_bounds__(256) void resolve_kernel(StreamParams p, float4* __restrict__ running, float* __restrict__ out, uint32_t last_pass) {
    uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= p.tm.n_local_tiles * RT_TILE * RT_TILE) return;
    uint32_t gid;
    if (!local_pixel_to_gid(p.tm, L, gid)) return;
    f3 radiance = mk3(0.0f);
    if (p.pass_first_s != 0u) { const float4 r = running[L]; radiance = mk3(r.x, r.y, r.z); }
    float unused = 0.0f;
    radiance = add_pass_samples<false>(p, L, radiance, unused);
    if (last_pass) {
        reinterpret_cast<float4*>(out)[p.tm.direct ? gid : L] = resolve_pixel(radiance, p.spp);
    } else {
        running[L] = make_float4(radiance.x, radiance.y, radiance.z, 0.0f);
    }
}

// Progressive refinement (rt_renderer_refine): the pass holds samples [pass_first_s, pass_first_s + pass_spp) of every pixel; they are added to
// the renderer's accumulation `acc` = (sum R, sum G, sum B, sum Y^2) per local pixel, which continues the sum of every earlier refine call
// in sample order — the float additions are those of ONE render at samples_per_pixel = pass_first_s + pass_spp, whatever the steps were.
// On the last pass of a step the frame for `done_after` samples is written.  A pure HBM stream: 12 B per sample, 16 B + 16 B per pixel.
__global__ __launch_bounds__(256) void refine_resolve_kernel(StreamParams p, float4* __restrict__ acc, float* __restrict__ out, uint32_t last_pass, uint32_t done_after) {
    uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= p.tm.n_local_tiles * RT_TILE * RT_TILE) return;
    uint32_t gid;
    if (!local_pixel_to_gid(p.tm, L, gid)) return;
    f3 radiance = mk3(0.0f);
    float q = 0.0f;
    if (p.pass_first_s != 0u) { const float4 r = acc[L]; radiance = mk3(r.x, r.y, r.z); q = r.w; }
    radiance = add_pass_samples<true>(p, L, radiance, q);
    acc[L] = make_float4(radiance.x, radiance.y, radiance.z, q);
    if (last_pass) reinterpret_cast<float4*>(out)[p.tm.direct ? gid : L] = resolve_pixel(radiance, done_after);
}

// Noise figure of a refined frame (rt_renderer_refine_noise), stage 1: per pixel, in fp32 with individually rounded operations and IEEE
// division, n = samples so far:  m = ((0.2126 Sr + 0.7152 Sg) + 0.0722 Sb) / n  (mean luminance),  v = max(0, Q / n - m * m) / (n - 1)
// (variance of that mean).  The workgroup's sums of v and of m and its count of pixels are taken in fp64 in a FIXED order — lanes by
// __shfl_down, the four waves by thread 0 — and written as one partial (sum v, sum m, pixels) per workgroup.  No atomics: the figure
// repeats bit for bit.  Padding pixels of a shard contribute nothing, and neither does a pixel whose m or v is not finite: the reference's
// arithmetic makes a NaN sample about once per 6e8 ("NaN pixels"), and one such pixel must not turn a frame's figure into NaN.
#define RT_NOISE_BLOCK 256u
struct NoiseSums { double v, m, pixels; };
__device__ __forceinline__ void noise_block_sum(NoiseSums& a, double (*lds)[3]) {
    for (int off = 32; off > 0; off >>= 1) { a.v += __shfl_down(a.v, off); a.m += __shfl_down(a.m, off); a.pixels += __shfl_down(a.pixels, off); }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { lds[wave][0] = a.v; lds[wave][1] = a.m; lds[wave][2] = a.pixels; }
    __syncthreads();
    if (threadIdx.x == 0u)
        for (uint32_t w = 1; w < RT_NOISE_BLOCK / 64u; w++) { a.v += lds[w][0]; a.m += lds[w][1]; a.pixels += lds[w][2]; }
}
// m and v of one pixel's accumulation a = (sum R, sum G, sum B, sum Y^2) after n_done samples; the denoiser's prepare step (rt_aov_kernel.hpp) shares it
__device__ __forceinline__ void mean_luminance_variance(float4 a, uint32_t n_done, float& m, float& v) {
    const float n = (float)n_done, n1 = (float)(n_done - 1u);
    m = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(0.2126f, a.x), __fmul_rn(0.7152f, a.y)), __fmul_rn(0.0722f, a.z)), n);
    const float d = __fsub_rn(__fdiv_rn(a.w, n), __fmul_rn(m, m));
    v = __fdiv_rn(d < 0.0f ? 0.0f : d, n1);   // max(0, d) that KEEPS a NaN (inf - inf of an overflowed pixel): fmaxf would turn it into 0
}
__global__ __launch_bounds__(RT_NOISE_BLOCK) void refine_noise_kernel(TileMap tm, const float4* __restrict__ acc, uint32_t n_done, NoiseSums* __restrict__ partials) {
    __shared__ double lds[RT_NOISE_BLOCK / 64u][3];
    const uint32_t L = blockIdx.x * RT_NOISE_BLOCK + threadIdx.x;
    NoiseSums s = {0.0, 0.0, 0.0};
    uint32_t gid;
    if (L < tm.n_local_tiles * RT_TILE * RT_TILE && local_pixel_to_gid(tm, L, gid)) {
        float m, v;
        mean_luminance_variance(acc[L], n_done, m, v);
        if (isfinite(m) && isfinite(v)) { s.v = (double)v; s.m = (double)m; s.pixels = 1.0; }
    }
    noise_block_sum(s, lds);
    if (threadIdx.x == 0u) partials[blockIdx.x] = s;
}
// stage 2: ONE workgroup; thread t adds partials t, t + 256, ... in that order, then the same fixed-order workgroup sum
__global__ __launch_bounds__(RT_NOISE_BLOCK) void refine_noise_finish_kernel(const NoiseSums* __restrict__ partials, uint32_t n_partials, NoiseSums* __restrict__ out) {
    __shared__ double lds[RT_NOISE_BLOCK / 64u][3];
    NoiseSums s = {0.0, 0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < n_partials; i += RT_NOISE_BLOCK) { const NoiseSums q = partials[i]; s.v += q.v; s.m += q.m; s.pixels += q.pixels; }
    noise_block_sum(s, lds);
    if (threadIdx.x == 0u) out[0] = s;
}

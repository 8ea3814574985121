// rt_device.hip — the device half of the C ABI: Renderer (kernel selection, passes, launches, per-kernel timers), shard layout, assembly.
// Which streaming kernel a world gets: stream_kernel_key() and stream_kernel_for().  How much LDS it gets: stream_kernel_lds_bytes() (rt_runtime.hpp).
// Probes and self-tests: rt_probes.hip.  Multi-GPU driver: rt_multi.hip.
#include "rt_runtime.hpp"
#include "rt_render_kernels.hpp"
#include "rt_stream_kernel.hpp"
#include "rt_xchg_kernel.hpp"
#include "rt_aov_kernel.hpp"
#include "rt_launch_image.hpp"
static_assert(sizeof(rt_image::Vec4) == sizeof(uint4), "the unit of a launch image is uint4");

extern "C" int rt_device_info(int device, uint32_t out[4]) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_device_info: null out");
    int rc = select_device(device);
    if (rc != RT_OK) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    out[0] = (uint32_t)prop.multiProcessorCount;      // compute units
    out[1] = (uint32_t)prop.clockRate;                 // peak engine clock, kHz
    out[2] = (uint32_t)(prop.totalGlobalMem >> 20);   // HBM, MiB
    out[3] = (uint32_t)prop.memoryClockRate;           // kHz
    return RT_OK;
}

extern "C" int rt_shard_layout(uint32_t width, uint32_t height, uint32_t world_size, uint32_t out[4]) {
    if (!out || width == 0 || height == 0 || world_size == 0) return rt_fail(RT_ERR_INVALID, "rt_shard_layout: bad argument");
    const TileMap tm = make_tile_map(width, height, 0, world_size);
    out[0] = tm.tiles_x; out[1] = tm.n_tiles; out[2] = tm.n_local_tiles; out[3] = (uint32_t)n_local_pixels(tm) * 4u;
    return RT_OK;
}

extern "C" int rt_shard_pixel_map(uint32_t width, uint32_t height, uint32_t world_size, uint32_t rank, uint32_t* out_gid, size_t n) {
    if (!out_gid || width == 0 || height == 0 || world_size == 0 || rank >= world_size) return rt_fail(RT_ERR_INVALID, "rt_shard_pixel_map: bad argument");
    const TileMap tm = make_tile_map(width, height, rank, world_size);
    if (n != n_local_pixels(tm)) return rt_fail(RT_ERR_INVALID, "rt_shard_pixel_map: a shard has %u pixels", (uint32_t)n_local_pixels(tm));
    for (uint32_t L = 0; L < (uint32_t)n; L++) {   // the host statement of local_pixel_to_gid (csrc/rt_render_kernels.hpp)
        const uint32_t tl = L / (RT_TILE * RT_TILE), p = L % (RT_TILE * RT_TILE);
        const uint32_t gt = tl * world_size + rank;
        const uint32_t x = (gt % tm.tiles_x) * RT_TILE + (p % RT_TILE), y = (gt / tm.tiles_x) * RT_TILE + (p / RT_TILE);
        out_gid[L] = (gt < tm.n_tiles && x < width && y < height) ? y * width + x : 0xffffffffu;
    }
    return RT_OK;
}

extern "C" int rt_device_count(int* out) {
    if (!out) return rt_fail(RT_ERR_INVALID, "rt_device_count: null out");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return RT_OK;
}

// Kernel selection.  One instantiation, as a key: the template arguments of render_kernel_stream<exact, filter, RT_STREAM_BLOCK, world, ext, big, wide, tol>, or render_kernel_xchg<RT_XCHG_BLOCK>
constexpr uint32_t stream_key(bool exact, bool filter, int world, int ext = 0, bool big = false, bool wide = false, bool tol = false) {
    return (uint32_t)exact | (uint32_t)filter << 1 | (uint32_t)world << 2 | (uint32_t)ext << 4 | (uint32_t)big << 6 | (uint32_t)wide << 7 | (uint32_t)tol << 8;
}
constexpr uint32_t RT_KEY_XCHG = 1u << 9;
constexpr uint32_t RT_KEY_NEE = 1u << 10;   // light sampling (rt_renderer_light_sampling_enable): the NEE form of an EXT >= 1 stack-walk or list key
constexpr uint32_t RT_KEY_LTREE = 1u << 12; // the light tree (mode RT_LIGHT_SAMPLING_TREE): the LTREE form of a TRI && NEE key; reported by rt_renderer_kernel_light_tree
constexpr uint32_t RT_KEY_ENVL = 1u << 13;  // environment light sampling (mode RT_LIGHT_SAMPLING_ENV): the ENVL form of an EXT 2 TRI && NEE key; reported by rt_renderer_kernel_env_light
constexpr uint32_t RT_KEY_NMAP = 1u << 14;  // normal maps (rt_renderer_normal_maps): the NMAP form of an EXT 2 TRI key, plain or with mode 48; reported by rt_renderer_kernel_normal_map
constexpr uint32_t RT_KEY_MFAC = 1u << 15;  // microfacet surfaces (rt_renderer_microfacets): the MFAC form of an EXT 2 TRI key, plain or with mode 48, which reads the normal-map table too; reported by rt_renderer_kernel_microfacet
constexpr uint32_t RT_KEY_INTR = 1u << 16;  // solid glass (rt_renderer_interiors): the INTR form of an MFAC key, plain or with mode 48, which reads all three tables; reported by rt_renderer_kernel_interior
constexpr uint32_t RT_KEY_CUT = 1u << 17;   // alpha cutouts (rt_renderer_cutouts): the CUT form of an INTR key, plain or with mode 48, which reads all four tables; reported by rt_renderer_kernel_cutout
constexpr uint32_t RT_KEY_TRI = 1u << 11;   // the world has triangles: the TRI form of an EXT >= 1 stack-walk or list key, plain or NEE; not one of rt_renderer_kernel_form's fields
// The one decode of a key.  Field i of stream_key()'s seven, in its order: exact, filter, world, ext, big, wide, tol ...
constexpr uint32_t stream_key_field(uint32_t key, int i) {
    constexpr uint32_t shift[7] = {0, 1, 2, 4, 6, 7, 8}, mask[7] = {1, 1, 3, 3, 1, 1, 1};
    return key >> shift[i] & mask[i];
}
// ... the instantiation a key names: the nine low bits as above, then NEE, TRI, LTREE, ENVL, CUT, INTR and MFAC from their bits.  NMAP is on under RT_KEY_MFAC too:
// every MFAC form (so every INTR and CUT form) reads the normal-map table, and its key does not carry RT_KEY_NMAP (rt_renderer_kernel_normal_map says 0 of it).
template <uint32_t K> static const void* stream_kernel_of() {
    return reinterpret_cast<const void*>(&render_kernel_stream<
        stream_key_field(K, 0) != 0u, stream_key_field(K, 1) != 0u, RT_STREAM_BLOCK, (int)stream_key_field(K, 2), (int)stream_key_field(K, 3), stream_key_field(K, 4) != 0u,
        stream_key_field(K, 5) != 0u, stream_key_field(K, 6) != 0u, (K & RT_KEY_NEE) != 0u, (K & RT_KEY_TRI) != 0u, (K & RT_KEY_LTREE) != 0u, (K & RT_KEY_ENVL) != 0u,
        (K & RT_KEY_CUT) != 0u, (K & RT_KEY_INTR) != 0u, (K & RT_KEY_MFAC) != 0u, (K & (RT_KEY_NMAP | RT_KEY_MFAC)) != 0u>);
}
// ... and what rt_renderer_kernel_form reports: the seven fields, then NEE
static void stream_key_fields(uint32_t key, uint32_t out[8]) {
    for (int i = 0; i < 7; i++) out[i] = stream_key_field(key, i);
    out[7] = key & RT_KEY_NEE ? 1u : 0u;
}

// The kernel of a renderer: variant = the resolved one (2 verbatim box tests, 3 fast exact division, 4 filtered predicates, 5 ray exchange), tol = requested
// as variant 6.  rt_renderer::resolve_variant() has refused what has no kernel (3 and 4 on lists and trees, 4 to 6 beyond the LDS or the reference's feature set).
static uint32_t stream_kernel_key(uint32_t variant, bool tol, const DeviceScene& s) {
    if (variant == 5) return RT_KEY_XCHG;
    const bool exact = variant != 3;   // of the BVH kernels; lists and node trees have no box-pair test to speed up
    const int ext = s.textured ? 2 : 1;
    // the distance-sorted queue / the 4-wide walk: one instantiation per feature level, records in global memory, 32-bit references
    if (s.queue) return stream_key(true, false, RT_WORLD_BVH_QUEUE, s.textured || s.extended ? ext : 0, true, true);   // (a lane walk reads a quad's kind from the flat record: no TRI form)
    // triangles (§18): the TRI form of the list and stack-walk EXT families; a world with triangles has quads, so it is a list or a BVH and `extended`
    const uint32_t tri = s.n_triangles ? RT_KEY_TRI : 0u;
    if (s.big) {   // records in global memory; lists and BVHs in the EXT forms only
        if (s.dw.kind == RT_WORLD_LIST) return stream_key(true, false, RT_WORLD_LIST, ext, true, true) | tri;
        if (s.dw.kind == RT_WORLD_NODE_TREE) return stream_key(true, false, RT_WORLD_NODE_TREE, 0, true, true);
        return stream_key(exact, false, RT_WORLD_BVH, ext, true, s.wide) | tri;
    }
    if (s.extended) return (s.dw.kind == RT_WORLD_LIST ? stream_key(true, false, RT_WORLD_LIST, ext) : stream_key(exact, false, RT_WORLD_BVH, ext)) | tri;
    if (s.dw.kind != RT_WORLD_BVH) return stream_key(true, false, (int)s.dw.kind);
    if (tol) return stream_key(false, false, RT_WORLD_BVH, 0, false, false, true);
    return stream_key(variant == 2, variant == 4, RT_WORLD_BVH);
}

// The ray generator of a lens camera (types 16 to 19, validated by rt_camera_check): one of primary_rays_lens_kernel's sixteen forms, read off the record
typedef void (*PrimaryRaysLensKernel)(StreamParams, uint32_t);
static PrimaryRaysLensKernel primary_rays_lens_kernel_for(const rt_camera& c) {
#define RT_LENS_FORMS(proj) \
    primary_rays_lens_kernel<proj, false, false>, primary_rays_lens_kernel<proj, false, true>, primary_rays_lens_kernel<proj, true, false>, primary_rays_lens_kernel<proj, true, true>
    static const PrimaryRaysLensKernel forms[16] = {RT_LENS_FORMS(0u), RT_LENS_FORMS(1u), RT_LENS_FORMS(2u), RT_LENS_FORMS(3u)};
#undef RT_LENS_FORMS
    return forms[((c.type - RT_CAM_PERSPECTIVE) & 3u) * 4u + (lens_camera_has_lens(c) ? 2u : 0u) + (lens_camera_has_shutter(c) ? 1u : 0u)];
}

// Every shipped instantiation, once, in the order the code object has them (a key listed twice does not compile): the exchange kernel, the 26 plain keys, then
// the feature families, a line each: a family is a set of key bits over one of two shape lists.  stream_kernel_key() yields no other key, so the default is never taken.
// The sixteen EXT 1 and 2 list and stack-walk shapes (exact, world, ext, big, wide) ...
#define RT_SHAPES_16(S, bits) \
    S(true, RT_WORLD_LIST, 2, true, true, bits) S(true, RT_WORLD_LIST, 1, true, true, bits) \
    S(false, RT_WORLD_BVH, 2, true, true, bits) S(true, RT_WORLD_BVH, 2, true, true, bits) S(false, RT_WORLD_BVH, 1, true, true, bits) S(true, RT_WORLD_BVH, 1, true, true, bits) \
    S(false, RT_WORLD_BVH, 2, true, false, bits) S(true, RT_WORLD_BVH, 2, true, false, bits) S(false, RT_WORLD_BVH, 1, true, false, bits) S(true, RT_WORLD_BVH, 1, true, false, bits) \
    S(true, RT_WORLD_LIST, 2, false, false, bits) S(true, RT_WORLD_LIST, 1, false, false, bits) \
    S(false, RT_WORLD_BVH, 2, false, false, bits) S(true, RT_WORLD_BVH, 2, false, false, bits) S(false, RT_WORLD_BVH, 1, false, false, bits) S(true, RT_WORLD_BVH, 1, false, false, bits)
// ... and their eight EXT 2 members
#define RT_SHAPES_8(S, bits) \
    S(true, RT_WORLD_LIST, 2, true, true, bits) S(false, RT_WORLD_BVH, 2, true, true, bits) S(true, RT_WORLD_BVH, 2, true, true, bits) S(false, RT_WORLD_BVH, 2, true, false, bits) S(true, RT_WORLD_BVH, 2, true, false, bits) \
    S(true, RT_WORLD_LIST, 2, false, false, bits) S(false, RT_WORLD_BVH, 2, false, false, bits) S(true, RT_WORLD_BVH, 2, false, false, bits)
static const void* stream_kernel_for(uint32_t key) {
#define RT_CASE(key) case (key): return stream_kernel_of<(key)>();
#define RT_KERNEL(exact, filter, world, ext, big, wide, tol) RT_CASE(stream_key(exact, filter, world, ext, big, wide, tol))
#define RT_SHAPE(exact, world, ext, big, wide, bits) RT_CASE(stream_key(exact, false, world, ext, big, wide) | (bits))
#define RT_FAMILY_16(bits) RT_SHAPES_16(RT_SHAPE, bits)
#define RT_FAMILY_8(bits) RT_SHAPES_8(RT_SHAPE, bits)
    switch (key) {
        case RT_KEY_XCHG: return reinterpret_cast<const void*>(&render_kernel_xchg<RT_XCHG_BLOCK>);
        // the plain keys (arguments: exact, filter, world, ext, big, wide, tol)
        RT_KERNEL(true, false, RT_WORLD_BVH_QUEUE, 2, true, true, false) RT_KERNEL(true, false, RT_WORLD_BVH_QUEUE, 1, true, true, false) RT_KERNEL(true, false, RT_WORLD_BVH_QUEUE, 0, true, true, false)
        RT_KERNEL(true, false, RT_WORLD_LIST, 2, true, true, false) RT_KERNEL(true, false, RT_WORLD_LIST, 1, true, true, false) RT_KERNEL(true, false, RT_WORLD_NODE_TREE, 0, true, true, false)
        RT_KERNEL(false, false, RT_WORLD_BVH, 2, true, true, false) RT_KERNEL(true, false, RT_WORLD_BVH, 2, true, true, false) RT_KERNEL(false, false, RT_WORLD_BVH, 1, true, true, false) RT_KERNEL(true, false, RT_WORLD_BVH, 1, true, true, false)
        RT_KERNEL(false, false, RT_WORLD_BVH, 2, true, false, false) RT_KERNEL(true, false, RT_WORLD_BVH, 2, true, false, false) RT_KERNEL(false, false, RT_WORLD_BVH, 1, true, false, false) RT_KERNEL(true, false, RT_WORLD_BVH, 1, true, false, false)
        RT_KERNEL(true, false, RT_WORLD_LIST, 2, false, false, false) RT_KERNEL(true, false, RT_WORLD_LIST, 1, false, false, false)
        RT_KERNEL(false, false, RT_WORLD_BVH, 2, false, false, false) RT_KERNEL(true, false, RT_WORLD_BVH, 2, false, false, false) RT_KERNEL(false, false, RT_WORLD_BVH, 1, false, false, false) RT_KERNEL(true, false, RT_WORLD_BVH, 1, false, false, false)
        RT_KERNEL(true, false, RT_WORLD_LIST, 0, false, false, false) RT_KERNEL(true, false, RT_WORLD_NODE_TREE, 0, false, false, false)
        RT_KERNEL(false, false, RT_WORLD_BVH, 0, false, false, true) RT_KERNEL(true, false, RT_WORLD_BVH, 0, false, false, false) RT_KERNEL(false, true, RT_WORLD_BVH, 0, false, false, false) RT_KERNEL(false, false, RT_WORLD_BVH, 0, false, false, false)
        // the families.  Light sampling, triangles (§18), both, the light tree (§20); environment light sampling (§24), the map and the tree together (§26);
        // then the four material tables, each plain and under mode 48: normal maps (§28), microfacet surfaces (§29), solid glass (§32), alpha cutouts (§34)
        RT_FAMILY_16(RT_KEY_NEE)
        RT_FAMILY_16(RT_KEY_TRI)
        RT_FAMILY_16(RT_KEY_TRI | RT_KEY_NEE)
        RT_FAMILY_16(RT_KEY_TRI | RT_KEY_NEE | RT_KEY_LTREE)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_NEE | RT_KEY_ENVL)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_NEE | RT_KEY_LTREE | RT_KEY_ENVL)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_NMAP)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_NEE | RT_KEY_LTREE | RT_KEY_ENVL | RT_KEY_NMAP)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_MFAC)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_NEE | RT_KEY_LTREE | RT_KEY_ENVL | RT_KEY_MFAC)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_MFAC | RT_KEY_INTR)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_NEE | RT_KEY_LTREE | RT_KEY_ENVL | RT_KEY_MFAC | RT_KEY_INTR)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_MFAC | RT_KEY_INTR | RT_KEY_CUT)
        RT_FAMILY_8(RT_KEY_TRI | RT_KEY_NEE | RT_KEY_LTREE | RT_KEY_ENVL | RT_KEY_MFAC | RT_KEY_INTR | RT_KEY_CUT)
        default: return nullptr;
    }
#undef RT_FAMILY_8
#undef RT_FAMILY_16
#undef RT_SHAPE
#undef RT_KERNEL
#undef RT_CASE
}
#undef RT_SHAPES_8
#undef RT_SHAPES_16

// the feature pass's kernel: the world's own traversal, so that a kernel carries one traversal stack
static decltype(&aov_kernel<RT_AOV_WALK_STACK>) aov_kernel_for(const DeviceWorld& w) {
    if (w.kind == RT_WORLD_LIST) return &aov_kernel<RT_AOV_WALK_LIST>;
    if (w.kind == RT_WORLD_NODE_TREE) return &aov_kernel<RT_AOV_WALK_TREE>;
    if (w.traversal == RT_TRAVERSAL_QUEUE) return &aov_kernel<RT_AOV_WALK_QUEUE>;
    if (w.traversal == RT_TRAVERSAL_WIDE4) return &aov_kernel<RT_AOV_WALK_WIDE4>;
    return &aov_kernel<RT_AOV_WALK_STACK>;
}
// ... and its RT_AOV_TEXTURED form
static decltype(&aov_kernel_tex<RT_AOV_WALK_STACK>) aov_kernel_tex_for(const DeviceWorld& w) {
    if (w.kind == RT_WORLD_LIST) return &aov_kernel_tex<RT_AOV_WALK_LIST>;
    if (w.kind == RT_WORLD_NODE_TREE) return &aov_kernel_tex<RT_AOV_WALK_TREE>;
    if (w.traversal == RT_TRAVERSAL_QUEUE) return &aov_kernel_tex<RT_AOV_WALK_QUEUE>;
    if (w.traversal == RT_TRAVERSAL_WIDE4) return &aov_kernel_tex<RT_AOV_WALK_WIDE4>;
    return &aov_kernel_tex<RT_AOV_WALK_STACK>;
}
// the FULL forms (§35)
static decltype(&aov_kernel_full<RT_AOV_WALK_STACK>) aov_kernel_full_for(const DeviceWorld& w) {
    if (w.kind == RT_WORLD_LIST) return &aov_kernel_full<RT_AOV_WALK_LIST>;
    if (w.kind == RT_WORLD_NODE_TREE) return &aov_kernel_full<RT_AOV_WALK_TREE>;
    if (w.traversal == RT_TRAVERSAL_QUEUE) return &aov_kernel_full<RT_AOV_WALK_QUEUE>;
    if (w.traversal == RT_TRAVERSAL_WIDE4) return &aov_kernel_full<RT_AOV_WALK_WIDE4>;
    return &aov_kernel_full<RT_AOV_WALK_STACK>;
}

// ---------------------------------------------------------------------------------------------
// Renderer
// ---------------------------------------------------------------------------------------------
static bool another_renderer_busy(const rt_renderer* self);   // is the last call of another renderer on self's device still unfinished?

// a device buffer that can change hands: what is replaced as a whole (a launch image, a rider's table) is built aside and swapped in
struct OwnedBuf : DevBuf {
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept { *this = std::move(o); }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
};

// The light-sampling modes, a row each: the image the mode launches on (0: the plain one; 1 to 4: the one with the light table of mode 1, 2, 4, 16 — rows 0 to 3
// in that order), the key bits it adds to stream_kernel_key() (a world without triangles is a TRI world too), whether it samples the environment map (§24, §26:
// it then needs the map and its distribution, and refuses what the map's estimator does not cover), and the pieces of its refusals.
struct LightMode { uint32_t mode, image, key_bits; bool env; const char *tag, *beside, *medium, *no_form; };
static const LightMode LIGHT_MODES[6] = {
    {RT_LIGHT_SAMPLING_QUADS, 1u, RT_KEY_NEE, false, "", "", "", "this world's kernel has no light-sampling form"},
    {RT_LIGHT_SAMPLING_ALL, 2u, RT_KEY_NEE, false, "", "", "", "this world's kernel has no light-sampling form"},
    {RT_LIGHT_SAMPLING_MESH, 3u, RT_KEY_NEE, false, "", "", "", "this world's kernel has no light-sampling form"},
    {RT_LIGHT_SAMPLING_TREE, 4u, RT_KEY_NEE | RT_KEY_TRI | RT_KEY_LTREE, false, "", "", "", "this world's kernel has no light-sampling form"},
    {RT_LIGHT_SAMPLING_ENV, 0u, RT_KEY_NEE | RT_KEY_TRI | RT_KEY_ENVL, true, "mode 32: ", "", "which the environment estimator does not cover", "this world's kernel has no environment-sampling form"},
    {RT_LIGHT_SAMPLING_ENV_TREE, 4u, RT_KEY_NEE | RT_KEY_TRI | RT_KEY_LTREE | RT_KEY_ENVL, true, "mode 48: ", " beside its lights",
     "which neither the environment estimator nor the light tree covers", "this world's kernel has no form that samples the map and the light tree"},
};
static const LightMode* light_mode(uint32_t mode) {   // NULL: off, or no mode
    for (const LightMode& m : LIGHT_MODES) if (m.mode == mode) return &m;
    return nullptr;
}

// The four per-material tables, a rung each, lowest first: normal maps (§28), microfacet surfaces (§29), solid glass (§32), alpha cutouts (§34).  A rung's form
// reads its own table and every table below it, so a launch runs the form of the highest rung that is on, plain or under mode 48.  A row: the key bits of the
// rung's form, and the words its refusals are built from.
struct FormRung { uint32_t key_bits; const char *api, *a, *table, *surfaces_render, *variant_5_6; };
enum : uint32_t { RUNG_NMAP, RUNG_MFAC, RUNG_INTR, RUNG_CUT, N_RUNGS };
static const FormRung FORM_LADDER[N_RUNGS] = {
    {RT_KEY_NMAP, "rt_renderer_normal_maps", "a", "normal-map table", "normal maps render", "reads no texture table and no normal-map table"},
    {RT_KEY_MFAC, "rt_renderer_microfacets", "a", "microfacet table", "microfacet surfaces render", "reads no microfacet table"},
    {RT_KEY_MFAC | RT_KEY_INTR, "rt_renderer_interiors", "an", "interior table", "solid glass renders", "reads no interior table"},
    {RT_KEY_MFAC | RT_KEY_INTR | RT_KEY_CUT, "rt_renderer_cutouts", "a", "cutout table", "alpha cutouts render", "reads no cutout table"},
};

struct rt_renderer {
    rt_render_config cfg{};
    rt_camera cam{};
    DeviceScene scene;
    TileMap tm{};
    DevBuf fb;
    // A frame slot: what one call's generator and tracer write and its resolve reads.
    //   samples = sample buffer of one pass (12 B per sample).
    //   primary = primary rays of one pass: 3 arrays of 16 B per sample index (origin|time, direction, RNG state), generated before the streaming kernel
    //   on the same stream: generating pass k + 1 on a second stream WHILE pass k is traced was measured and is harmful (the persistent kernel ran 40 %
    //   slower with the generator's waves co-resident: 100 ms instead of 70).
    // Every renderer has slot[0].  A renderer whose Render() is one pass of a streaming kernel gets a second set and two streams of its own, and a plain
    // render_async then runs ahead ("Run-ahead"): call k generates and traces into slot k mod 2 on that slot's stream, which waits for
    // nothing of the caller's, and only its resolve — the one kernel that touches `out` — runs on the caller's stream.
    //   traced = the slot's last tracer has finished (the resolve waits for it); consumed = whatever last read or wrote the slot's buffers on a caller's
    //   stream has finished (the slot's next generator waits for it).
    struct Slot { DevBuf samples, primary, work_counter; hipStream_t stream = nullptr; hipEvent_t traced = nullptr, consumed = nullptr; };
    Slot slot[2];
    uint32_t n_slots = 1;
    uint64_t n_ahead = 0, n_overlapped = 0;   // calls that ran ahead; those that found the call before them still in flight when they were enqueued
    DevBuf running;              // running sums (16 B per pixel) when spp needs several passes
    uint32_t pass_spp = 0;       // samples per pixel per pass
    uint32_t n_cus = 0;
    uint32_t stream_lds_bytes = 0;
    uint32_t n_top = 0;  // BIG kernels: wide nodes (breadth-first order) staged in the LDS
    uint32_t stream_block = RT_STREAM_BLOCK;
    uint32_t stream_blocks_per_cu = 0;
    uint32_t variant = 0;        // resolved kernel variant (see rt_render_config::variant)
    const void* stream_kernel = nullptr;   // variants 2 to 6: what stream_kernel_for() gave for this world
    bool tol = false;            // variant 3 with the tolerance-mode box test (requested as variant 6)
    uint32_t tune[5] = {RT_INNER_KEEP, RT_SHADE_MIN, RT_LEAF_MIN, RT_INNER_DROP, RT_INNER_FLOOR};  // scheduling thresholds of the streaming kernel
    bool tune_exit_forced = false;   // RT06_TUNE named inner_drop and inner_floor: they hold for every kernel of this renderer
    // render_kernel_xchg (variant 5): roles, ring capacities, population and thresholds (RT06_XCHG=tracers,extra,swap,shade,patience,prio)
    struct { uint32_t n_tracers = 9, tq_cap = 0, sq_cap = 0, pop_extra = 192, swap_min = 16, shade_min = 48, patience = 6, prio = 1, scene_vec4 = 0, extra_in_lds = 0, keep = 44, shards = 1; } xc;
    DevBuf xchg_error;           // set by the kernel when a bounded ring wait ran out (a protocol bug, never expected)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    // per-kernel HIP events of the last RT_TIMES_RING render calls, on the stream the kernels run on, four per PASS:
    // [4k] before primary_rays_kernel of pass k, [4k+1] before the streaming kernel, [4k+2] after it, [4k+3] after resolve_kernel.
    // Created at first use (a 10 000-spp render of a 4K frame has > 100 passes).
    // A call that ran ahead has [0] to [2] on its slot's stream and [3] on the caller's, where the resolve starts behind a wait for the tracer: its
    // resolve is timed from an event of its own (kev_resolve0) behind that wait.
    static constexpr uint32_t RT_TIMES_RING = 32;
    std::vector<hipEvent_t> kev[RT_TIMES_RING];
    hipEvent_t kev_resolve0[RT_TIMES_RING] = {};
    bool kev_ahead[RT_TIMES_RING] = {};
    uint32_t kev_passes[RT_TIMES_RING] = {};   // passes of the call each ring slot holds: a Render() has n_passes, a refine step a count of its own
    uint64_t n_renders = 0;
    uint32_t n_passes = 1;
    // progressive refinement (rt_renderer_refine*): samples [0, refine_done) of every pixel are in `accum` = (sum R, sum G, sum B, sum Y^2) per local
    // pixel, a buffer of its own (allocated at the first refine call) so that a Render() between two steps disturbs neither
    DevBuf accum, noise_partials, noise_out;
    uint32_t refine_done = 0;
    // first-hit feature buffers (rt_renderer_aov_enable): two float4 per local pixel, continued by aov_kernel after each refine pass; they share the
    // refinement state's lifecycle.  aov_done = samples [0, aov_done) of every pixel are in them (<= aov_max when that is not 0).
    DevBuf aov;
    bool aov_on = false;
    uint32_t aov_max = 0, aov_done = 0;
    uint32_t aov_mode = RT_AOV_PLAIN;    // the mode of the last successful enable: RT_AOV_TEXTURED launches the TEX forms, RT_AOV_FULL the FULL forms (§35)
    const char* aov_refused = nullptr;   // the first material of the world the plain feature pass does not cover (a medium, a noise or an image texture)
    // light sampling (rt_renderer_light_sampling_enable).  tab[i]: the world's lights as rt_world_light_table gave them at creation for the table modes 1, 2, 4
    // and 16 (or why it gave none; mode 16, §20, with cdf and the tree's nodes).  image[0]: the plain image; image[1 + i]: the image with tab[i]'s table, from
    // the first enable of a mode that launches on it.  resolved[k]: the key and the kernel of LIGHT_MODES[k], from its first enable.  launch_on() reads them.
    struct LightTable { uint32_t n = 0; std::vector<uint32_t> kind, index; std::vector<float> area, sphere /* 4 per light */, cdf, nodes /* 8 per node */;
                        std::string refused; bool none = false /* refused for having no light: what mode 48 accepts (§26) */; };
    // One launch image ("The launch images"): scene | light table (if any) | tail header | tail (if any), in ONE device buffer, composed anew
    // whenever a rider changes.  The plain image while no rider is on is scene.blob itself: its buffer here stays empty.
    struct Image { OwnedBuf blob; uint32_t table_vec4 = 0, lds_bytes = 0, blocks_per_cu = 0; };
    struct { uint32_t mode = RT_LIGHT_SAMPLING_OFF; LightTable tab[4]; Image image[5]; struct { uint32_t key = 0; const void* kernel = nullptr; } resolved[6];
             bool on() const { return mode != RT_LIGHT_SAMPLING_OFF; } } nee;
    // The riders: what every launch image carries in its tail while it is on.  Each setter builds the next state of its rider and hands it to replace_rider().
    // smooth shading (rt_renderer_shading_normals): the table as given (9 floats per triangle of the world) and a flat copy for the feature pass
    struct { bool on = false; uint32_t n_smooth = 0; std::vector<float> host; OwnedBuf table; uint32_t count() const { return n_smooth; } } vn;
    // texture coordinates (rt_renderer_texture_coords): the table as given (6 floats per triangle of the world)
    struct { bool on = false; uint32_t n_mapped = 0; std::vector<float> host; uint32_t count() const { return n_mapped; } } uv;
    // the environment map (rt_renderer_environment) of a background-2 world: the image as given (3 floats per texel) and a device buffer of the
    // renderer's own with one float4 per texel; the tail carries only a two-vec4 record that points to it (a 2048 x 1024 map is 32 MiB, and there are up to five images)
    // (§24: while dist_on, the records' fourth lane holds the sampling density and `dist` rowc[H], rowy[H + 1], colc[H W] of rt_environment_distribution)
    struct Environment { bool on = false, dist_on = false; uint32_t w = 0, h = 0; float u0 = 0.0f; std::vector<float> host; OwnedBuf texels, dist; } env;
    bool has_medium = false;   // the world has a constant medium (RT_MAT_ISOTROPIC): the modes that sample the map refuse it
    // the texture table (rt_renderer_textures): the entries and the texels as given (3 bytes per texel), and a device buffer of the renderer's own
    // with one dword r | g << 8 | b << 16 per texel, all images back to back; the tail carries (pointer low, pointer high, n, -) and one vec4 per entry
    struct { bool on = false; std::vector<rt_texture> records; std::vector<uint8_t> host; OwnedBuf texels; uint32_t count() const { return (uint32_t)records.size(); } } tex;
    // normal maps (rt_renderer_normal_maps): one record per material as given; the tail carries them behind the texture table, whose header points
    // there.  While on, a plain launch and a mode-48 launch run the NMAP form of their kernel (plain / envt, resolved when the table or the mode comes on).
    struct NormalMaps { bool on = false; uint32_t n_mapped = 0; std::vector<rt_normal_map> host; uint32_t count() const { return n_mapped; } } nm;
    // microfacet surfaces (rt_renderer_microfacets): one record per material as given; the tail carries them last, and the bits above bit 0 of its
    // header's first lane say where.  While on, a plain launch and a mode-48 launch run the MFAC form of their kernel, which reads the normal-map table too.
    struct Microfacets { bool on = false; uint32_t n_on = 0; std::vector<rt_microfacet> host; uint32_t count() const { return n_on; } } mf;
    // solid glass (rt_renderer_interiors): one record per material as given; with a table the tail's first lane counts to a sub-header, behind which
    // the microfacet and the interior records lie.  While on, a plain launch and a mode-48 launch run the INTR form of their kernel, which reads all three tables.
    struct Interiors { bool on = false; uint32_t n_on = 0; std::vector<rt_interior> host; uint32_t count() const { return n_on; } } in;
    // alpha cutouts (rt_renderer_cutouts): one record per material as given, behind the interior records; the sub-header's third lane says where.
    // While on, a plain launch and a mode-48 launch run the CUT form of their kernel, which reads all four tables, whichever of the others are there.
    struct Cutouts { bool on = false; uint32_t n_on = 0; std::vector<rt_cutout> host; uint32_t count() const { return n_on; } } cut;
    // the rungs' forms (FORM_LADDER): the key and the kernel of rung g's form, plain [g][0] and under mode 48 [g][1], each from the first time its table and its mode met
    struct { uint32_t key = 0; const void* kernel = nullptr; } form[N_RUNGS][2];
    bool rung_on(uint32_t g) const { return g == RUNG_NMAP ? nm.on : g == RUNG_MFAC ? mf.on : g == RUNG_INTR ? in.on : cut.on; }
    bool tail_on() const { return vn.on || uv.on || env.on || tex.on || mf.on || in.on || cut.on; }
    // rung g's form of the renderer's kernel: the world's own shape at EXT 2 with TRI and the rung's bits, plain or with mode 48's (0: a world no such form walks)
    uint32_t form_key(uint32_t g, bool envt) const {
        if (variant < 2 || variant == 5 || tol || scene.queue || scene.dw.kind == RT_WORLD_NODE_TREE) return 0u;
        const uint32_t base = stream_kernel_key(variant, false, scene);
        return stream_key(stream_key_field(base, 0), false, (int)stream_key_field(base, 2), 2, stream_key_field(base, 4), stream_key_field(base, 5)) | RT_KEY_TRI |
               FORM_LADDER[g].key_bits | (envt ? RT_KEY_NEE | RT_KEY_LTREE | RT_KEY_ENVL : 0u);
    }
    // whether a launch is refused for a table's records (normal maps §28, roughness maps §29, cutout masks §34): one that is `mapped` names an entry (*which) the
    // renderer's texture table does not have
    template <typename Rider, typename Mapped> bool entry_missing(const Rider& rider, Mapped mapped, uint32_t* which) const {
        if (!rider.on) return false;
        for (const auto& m : rider.host)
            if (mapped(m) && (!tex.on || m.image >= tex.records.size() || tex.records[m.image].width == 0u)) { *which = m.image; return true; }
        return false;
    }
    // ... or for its image materials (§25): one of them names an index (*which) the renderer does not serve
    bool image_index_unserved(uint32_t* which) const {
        for (const uint32_t k : scene.image_indices)
            if (tex.on ? (k >= tex.records.size() || tex.records[k].width == 0u) : k != 0u) { *which = k; return true; }
        return false;
    }
    // The map in e.host (e.w x e.h, 3 floats per texel) onto the device, into e's own buffers: one record per texel, and — with_dist, §24 — the sampling density in
    // the records' fourth lane and the tables in e.dist.  An all-black map is refused (RT_ERR_INVALID, `who` names the caller).
    static int upload_environment(const char* who, Environment& e, bool with_dist) {
        const size_t n_texels = (size_t)e.w * e.h;
        const float* rgb = e.host.data();
        std::vector<float> tables, density;
        if (with_dist) {
            tables.resize(2u * (size_t)e.h + 1u + n_texels); density.resize(n_texels);
            if (const char* why = rt_environment_distribution_refusal(e.w, e.h, rgb, tables.data(), tables.data() + e.h, tables.data() + 2u * (size_t)e.h + 1u, density.data()))
                return rt_fail(RT_ERR_INVALID, "%s: %s", who, why);
        }
        std::vector<float4> records(n_texels);
        for (size_t i = 0; i < n_texels; i++) records[i] = make_float4(rgb[3u * i], rgb[3u * i + 1u], rgb[3u * i + 2u], with_dist ? density[i] : 0.0f);
        HIP_TRY(e.texels.upload(records.data(), n_texels * sizeof(float4)));
        if (with_dist) HIP_TRY(e.dist.upload(tables.data(), tables.size() * sizeof(float)));
        e.dist_on = with_dist;
        return RT_OK;
    }
    // What a launch in light-sampling `mode` (RT_LIGHT_SAMPLING_OFF: the plain kernel) runs and on what: the one place that knows which image, kernel, LDS and
    // workgroup count belong together.  `lights` is what rt_renderer_light_sampling_info reports: the table's lights, or the texels of a map sampled alone.
    struct LaunchOn { const void* kernel; uint32_t key; const uint4* blob; uint32_t blob_vec4, lds_bytes, blocks_per_cu, lights; };
    LaunchOn launch_on(uint32_t mode) const {
        const LightMode* m = light_mode(mode);
        const uint32_t i = m ? m->image : 0u;
        const Image& im = nee.image[i];
        const LightTable& t = nee.tab[i ? i - 1u : 0u];   // (off: the quad lights)
        LaunchOn l;
        l.kernel = m ? nee.resolved[m - LIGHT_MODES].kernel : stream_kernel;
        l.key = m ? nee.resolved[m - LIGHT_MODES].key : stream_kernel_key(variant, tol, scene);
        if (!m || mode == RT_LIGHT_SAMPLING_ENV_TREE)   // the form of the highest rung that is on (the other modes are refused while a table is on)
            for (uint32_t g = N_RUNGS; g-- > 0u;)
                if (rung_on(g)) { l.kernel = form[g][m ? 1 : 0].kernel; l.key = form[g][m ? 1 : 0].key; break; }
        l.blob = (im.blob.p ? im.blob : scene.blob).as<uint4>();
        l.blob_vec4 = scene.packed.blob_vec4 + im.table_vec4;
        l.lds_bytes = i ? im.lds_bytes : stream_lds_bytes;
        l.blocks_per_cu = i ? im.blocks_per_cu : stream_blocks_per_cu;
        l.lights = m && !i ? env.w * env.h : t.refused.empty() ? t.n : 0u;
        return l;
    }
    // Rung g's form of the plain kernel, or of mode 48's, once: the kernel and its LDS limit
    int resolve_form_kernel(uint32_t g, bool envt, uint32_t lds_bytes) {
        auto& slot_of = form[g][envt ? 1 : 0];
        if (slot_of.kernel) return RT_OK;
        const uint32_t key = form_key(g, envt);
        const void* k = key ? stream_kernel_for(key) : nullptr;
        if (!k) return rt_fail(RT_ERR_INVALID, "%s: this world's kernel has no form that reads %s %s", FORM_LADDER[g].api, FORM_LADDER[g].a, FORM_LADDER[g].table);
        HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        slot_of.key = key; slot_of.kernel = k;
        return RT_OK;
    }
    // Image i (0: the plain one; 1 to 4: with the light table of mode 1, 2, 4, 16) from the riders as they stand, into `fresh`: scene | light table | tail
    // (rt_launch_image.hpp has both layouts).  The scene part is copied device to device, the rest uploaded once.  The plain image without a tail gets no buffer.
    int compose(uint32_t i, Image& fresh) const {
        std::vector<rt_image::Vec4> rest;
        if (i) {
            const LightTable& t = nee.tab[i - 1u];
            rt_image::append_light_table(rest, LIGHT_MODES[i - 1u].mode, t.n, t.kind.data(), t.index.data(), t.area.data(), t.sphere.data(), t.cdf.data(), t.nodes.data());
            fresh.table_vec4 = (uint32_t)rest.size();
            PackedSceneRef with_table = scene.packed;
            with_table.blob_vec4 += fresh.table_vec4;
            fresh.lds_bytes = (uint32_t)stream_kernel_lds_bytes(stream_block, with_table, scene.big, scene.wide, n_top);
            if (fresh.lds_bytes > RT_LDS_PER_CU)
                return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: the light table (%u bytes) does not fit beside the scene image in the LDS", fresh.table_vec4 * 16u);
            fresh.blocks_per_cu = std::min(2u, RT_LDS_PER_CU / fresh.lds_bytes);
        } else if (!tail_on()) return RT_OK;
        rt_image::Riders<rt_texture> rd;
        if (vn.on) { rd.normals = vn.host.data(); rd.n_normal_floats = vn.host.size(); }
        if (uv.on) { rd.coords = uv.host.data(); rd.n_coord_floats = uv.host.size(); }
        rd.env = env.on; rd.env_w = env.w; rd.env_h = env.h; rd.env_u0 = env.u0;
        rd.env_texels = (uint64_t)reinterpret_cast<uintptr_t>(env.texels.p); rd.env_dist = env.dist_on ? (uint64_t)reinterpret_cast<uintptr_t>(env.dist.p) : 0ull;
        rd.textures = tex.on; rd.texture = tex.records.data(); rd.n_textures = tex.records.size(); rd.texture_texels = (uint64_t)reinterpret_cast<uintptr_t>(tex.texels.p);
        if (nm.on) { rd.normal_maps = nm.host.data(); rd.n_normal_maps = nm.host.size(); }
        if (mf.on) { rd.microfacets = mf.host.data(); rd.n_microfacets = mf.host.size(); }
        if (in.on) { rd.interiors = in.host.data(); rd.n_interiors = in.host.size(); }
        if (cut.on) { rd.cutouts = cut.host.data(); rd.n_cutouts = cut.host.size(); }
        rt_image::append_tail(rest, rd);
        const size_t scene_bytes = (size_t)scene.packed.blob_vec4 * sizeof(uint4);
        HIP_TRY(fresh.blob.alloc(scene_bytes + rest.size() * sizeof(uint4)));
        HIP_TRY(hipMemcpy(fresh.blob.p, scene.blob.p, scene_bytes, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(fresh.blob.as<uint4>() + scene.packed.blob_vec4, rest.data(), rest.size() * sizeof(uint4), hipMemcpyHostToDevice));
        return RT_OK;
    }
    // Every image there is — the plain one and those whose table has been built — anew, all or none: into fresh buffers that are swapped in only when every one
    // has succeeded.  The caller has waited for the launches that read the old buffers (wait_last_call).
    int recompose() {
        Image fresh[5];
        for (uint32_t i = 0; i < 5u; i++)
            if (!i || nee.image[i].blob.p)
                if (const int rc = compose(i, fresh[i])) return rc;
        for (uint32_t i = 0; i < 5u; i++)
            if (!i || nee.image[i].blob.p) std::swap(nee.image[i], fresh[i]);
        return RT_OK;
    }
    // A rider's state replaced by `next` and the images composed anew; on failure the rider gets its old state back, and no image and nothing of the refinement
    // has changed.  On success the refinement and its first hits start anew: samples drawn on the old images belong to another frame.
    template <typename Rider> int replace_rider(Rider& rider, Rider& next) {
        std::swap(rider, next);
        const int rc = recompose();
        if (rc != RT_OK) { std::swap(rider, next); return rc; }
        refine_done = aov_done = 0u;
        return RT_OK;
    }
    // Whether `next` is the state the rider is in: both off, or both on with the same (canonical) host table.  Then nothing changes and the refinement goes on.
    template <typename Rider> static bool same_table(const Rider& rider, const Rider& next) {
        if (!next.on || !rider.on) return next.on == rider.on;
        return rider.host.size() == next.host.size() && std::memcmp(rider.host.data(), next.host.data(), next.host.size() * sizeof(next.host[0])) == 0;
    }
    // denoiser (rt_renderer_denoise): guide records, the two colour buffers the iterations ping-pong, the output frame; allocated at first use
    DevBuf dn_g0, dn_g1, dn_a, dn_b, dn_out;
    // ordering between refine steps and the filter, whichever streams the caller gives them: refine_ev = end of the last refine step (the filter
    // reads accum / aov behind it), dn_ev = end of the last filter (the next step, which overwrites accum / aov, and the next filter, which
    // shares the colour buffers, start behind it)
    hipEvent_t dn_ev = nullptr, refine_ev = nullptr;
    bool dn_valid = false;
    static constexpr uint32_t SAMPLE_BYTES = RT_SAMPLE_BYTES, PRIMARY_BYTES = 48;   // HBM per sample index of a pass: radiance (float4) + primary ray record

    // Pick the kernel variant; size the LDS, the exchange rings and the per-pass sample buffer.
    //   0 = default (the fastest validated variant), 1 = baseline wave-per-pixel kernel,
    //   2 = streaming kernel with verbatim box tests, 3 = streaming kernel with the fast exact division,
    //   4 = 3 + filtered box-pair predicates (experimental), 5 = ray exchange, 6 = 3 with the tolerance-mode box test.
    // The streaming kernel's scheduling thresholds: every family runs the fixed exit rule of the node loop (inner_drop 0, inner_floor 64: "fewer than
    // inner_keep") unless it was measured to gain from the entry-relative one (EXPERIMENTS.md E18).  RT06_TUNE="keep,shade,leaf" or
    // "keep,shade,leaf,drop,floor" overrides them for scheduling experiments (results never change); 0 for keep, shade, leaf or floor leaves the planned value.
    void plan_thresholds() {
        // measured: the hot loop of variant 3, on all four workloads, every kind of image (E18).  The generic node loop, tolerance mode and the
        // light-sampling forms (call_params) were not, and keep the fixed rule.
        if (variant == 3 && !tol) { tune[3] = RT_INNER_DROP_HOT; tune[4] = RT_INNER_FLOOR_HOT; }
        const char* env = std::getenv("RT06_TUNE");
        if (!env) return;
        unsigned v[5] = {0, 0, 0, 0, 0};
        const int n = std::sscanf(env, "%u,%u,%u,%u,%u", &v[0], &v[1], &v[2], &v[3], &v[4]);
        if ((n != 3 && n != 5) || v[0] > 64 || v[1] > 64 || v[2] > 64 || v[3] > 64 || v[4] > 64) return;
        for (int k = 0; k < 3; k++)
            if (v[k]) tune[k] = v[k];
        if (n == 5) { tune[3] = v[3]; if (v[4]) tune[4] = v[4]; tune_exit_forced = true; }
    }
    int plan() {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, cfg.device));
        n_cus = (uint32_t)prop.multiProcessorCount;
        if (const int rc = resolve_variant(size_stream_lds())) return rc;
        if (variant == 5)
            if (const int rc = size_xchg_rings()) return rc;
        plan_thresholds();
        if (variant < 2) return RT_OK;
        if (const int rc = size_passes()) return rc;
        stream_kernel = stream_kernel_for(stream_kernel_key(variant, tol, scene));
        HIP_TRY(hipFuncSetAttribute(stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)stream_lds_bytes));
        if (std::getenv("RT06_DEBUG")) {
            int occ = -1;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, stream_kernel, (int)stream_block, stream_lds_bytes);
            fprintf(stderr, "[rt06] stream kernel: block %u, LDS %u B, planned %u blocks/CU, runtime occupancy query %d blocks/CU\n",
                    stream_block, stream_lds_bytes, stream_blocks_per_cu, occ);
        }
        return RT_OK;
    }
    // LDS of a render_kernel_stream workgroup (RT_STREAM_BLOCK lanes in every instantiation, so the variant can be chosen knowing it); false = the world cannot stream
    bool size_stream_lds() {
        if (!scene.has_packed) return false;
        if (scene.big) {  // beside the per-lane stacks, in what two workgroups per CU leave free: the top of the tree
            const uint32_t node_bytes = RT_NODE_DWORDS_BIG * 4u, stacks = (uint32_t)stream_kernel_lds_bytes(stream_block, scene.packed, true, scene.wide, 0u);
            const uint32_t budget = stacks + 4096u <= RT_LDS_PER_CU / 2u ? RT_LDS_PER_CU / 2u : RT_LDS_PER_CU;
            uint32_t top_bytes = std::min((budget > stacks ? budget - stacks : 0u) & ~63u, scene.packed.n_inner * node_bytes);
            if (const char* env = std::getenv("RT06_TOP_NODES")) top_bytes = std::min(top_bytes, (uint32_t)std::atoi(env) * node_bytes);
            if (scene.queue) top_bytes = 0;   // the queue walk reads the flat world's own nodes
            n_top = top_bytes / node_bytes;
        }
        stream_lds_bytes = (uint32_t)stream_kernel_lds_bytes(stream_block, scene.packed, scene.big, scene.wide, n_top);
        if (stream_lds_bytes <= RT_LDS_PER_CU) stream_blocks_per_cu = std::min(2u, RT_LDS_PER_CU / stream_lds_bytes);
        return stream_lds_bytes <= RT_LDS_PER_CU;
    }
    // cfg.variant -> variant and tol, or the refusal of a world the requested kernel cannot take
    int resolve_variant(bool can_stream) {
        uint32_t want = cfg.variant;
        if (want > 6) return rt_fail(RT_ERR_INVALID, "unknown kernel variant %u", want);
        const bool want_tol = want == 6;   // variant 6: variant 3 with the tolerance-mode box test (opt-in; inside |delta| < 1e-3, not bit-exact by construction)
        if (want_tol) want = 3;
        const bool can_xchg = can_stream && !scene.big && !scene.extended && scene.dw.kind == RT_WORLD_BVH && scene.regular_boxes && !scene.queue;
        if (scene.queue && want >= 3)
            return rt_fail(RT_ERR_INVALID, "kernel variants 3 to 5 walk the tree with the stack of BVH.cu:54-106: a world with another traversal rule (RT_TRAVERSAL_QUEUE, RT_TRAVERSAL_WIDE4) renders on variant 2 (or 0) and on the baseline kernel (1)");
        if (want == 0) want = can_stream ? ((scene.dw.kind == RT_WORLD_BVH && scene.regular_boxes && !scene.queue) ? 3u : 2u) : 1u;
        if (want == 3 && cfg.variant == 0 && can_xchg) {
            const char* env = std::getenv("RT06_DEFAULT_XCHG");
            if (env && env[0] == '1') want = 5;
        }
        if (scene.dw.background == 2u) {   // §23: the environment map is looked up in render_kernel_stream's EXT 2 forms only
            if (want == 1) return rt_fail(RT_ERR_INVALID, "the baseline kernel (variant 1) looks no environment map up: a world with background mode 2 renders on variant 0, 2 or 3");
            if (want == 5) return rt_fail(RT_ERR_INVALID, "kernel variant 5 (ray exchange) looks no environment map up: a world with background mode 2 renders on variant 0, 2 or 3");
            if (want_tol) return rt_fail(RT_ERR_INVALID, "kernel variant 6 (tolerance-mode box test) looks no environment map up: a world with background mode 2 renders on variant 0, 2 or 3");
        }
        if (want == 5 && !can_xchg)
            return rt_fail(RT_ERR_INVALID, "kernel variant 5 (ray exchange) needs an LDS-resident RT_WORLD_BVH world of the reference's feature set with box coordinates in the fast-division class");
        if (want == 4 && can_stream && scene.big)
            return rt_fail(RT_ERR_INVALID, "kernel variant 4 needs a world whose LDS image fits in 160 KiB: use variant 0, 2 or 3");
        if (want == 4 && scene.extended)
            return rt_fail(RT_ERR_INVALID, "kernel variant 4 renders the reference's feature set only (no quads / lights / constant background): use variant 0, 2 or 3");
        if (want >= 3 && want <= 4 && scene.dw.kind != RT_WORLD_BVH)
            return rt_fail(RT_ERR_INVALID, "kernel variants 3 and 4 need an RT_WORLD_BVH world (a HittableList / bvh_node world runs on variant 2)");
        if (want >= 2 && !can_stream)
            return rt_fail(RT_ERR_INVALID, "kernel variant %u cannot take this world (its references or per-lane stacks do not fit)", want);
        if (want >= 3 && !scene.regular_boxes)
            return rt_fail(RT_ERR_INVALID, "kernel variants 3 and 4 need every box coordinate to be 0 or within [2^-40, 2^40)");
        variant = want;
        if (want_tol) {
            // Kept for the reference's own feature set only (spheres: a sphere touches its box at six points, so a box decision that flips by an ulp
            // almost never meets a hit).  Worlds with quads are refused: a quad's edges ARE its box's edges, and the Cornell box at its own 5000 spp moved
            // one pixel by 2.1e-3, outside the tolerance; the global-memory form gains 8 %, below the 15 % it would have to (EXPERIMENTS.md E4)
            if (scene.big || scene.extended)
                return rt_fail(RT_ERR_INVALID, "kernel variant 6 (tolerance-mode box test) is instantiated for LDS-resident RT_WORLD_BVH worlds of the reference's feature set only (spheres, the three scattering materials, the sky): use variant 0");
            tol = true;
        }
        return RT_OK;
    }
    // render_kernel_xchg: the largest ring pair that fits beside the scene in half a CU's LDS (two workgroups per CU); when none does, the default
    // falls back to variant 3.  LDS of a workgroup: nodes | spheres | (second centres when a sphere moves) | tracer stacks | rings
    int size_xchg_rings() {
        if (const char* env = std::getenv("RT06_XCHG")) {
            unsigned v[8] = {xc.n_tracers, xc.pop_extra, xc.swap_min, xc.shade_min, xc.patience, xc.prio, xc.keep, xc.shards};
            const int n = std::sscanf(env, "%u,%u,%u,%u,%u,%u,%u,%u", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7]);
            if (n >= 1 && v[0] >= 1 && v[0] <= RT_XCHG_BLOCK / 64 - 1) xc.n_tracers = v[0];
            if (n >= 2 && v[1] <= 1024) xc.pop_extra = v[1];
            if (n >= 3 && v[2] >= 1 && v[2] <= 64) xc.swap_min = v[2];
            if (n >= 4 && v[3] >= 1 && v[3] <= 64) xc.shade_min = v[3];
            if (n >= 5 && v[4] <= 1000) xc.patience = v[4];
            if (n >= 6) xc.prio = v[5] ? 1u : 0u;
            if (n >= 7 && v[6] >= 1 && v[6] <= 64) xc.keep = v[6];
            if (n >= 8 && (v[7] == 1 || v[7] == 2)) xc.shards = v[7];
        }
        if (xc.shards > xc.n_tracers || xc.shards > RT_XCHG_BLOCK / 64 - xc.n_tracers) xc.shards = 1;   // every shard needs a tracer and a shader
        xc.extra_in_lds = scene.any_moving ? 1u : 0u;
        xc.scene_vec4 = scene.any_moving ? scene.packed.off_mats : scene.packed.off_extra;
        const uint32_t fixed = xc.scene_vec4 * 16u + ((xc.n_tracers * 64u * scene.packed.stack_cap * 2u + 15u) & ~15u) + xc.shards * XC_WORDS * 4u;
        static const uint32_t caps[][2] = {{128, 128}, {64, 128}, {64, 64}, {32, 64}, {32, 32}, {16, 32}, {16, 16}};   // per workgroup: divided by the shards
        for (const auto& c : caps) {
            const uint32_t total = fixed + c[0] * (4u + XC_TQ_ENTRY_BYTES) + c[1] * (4u + XC_SQ_ENTRY_BYTES);
            if (total > RT_LDS_PER_CU / 2u || c[0] / xc.shards < 16u) continue;
            xc.tq_cap = c[0] / xc.shards; xc.sq_cap = c[1] / xc.shards;
            // the population must stay below what the places that can hold a ray add up to (no full-ring deadlock)
            xc.pop_extra = std::min(xc.pop_extra, xc.shards * (xc.tq_cap + xc.sq_cap - 16u));
            stream_block = RT_XCHG_BLOCK;
            stream_lds_bytes = (total + 15u) & ~15u;
            stream_blocks_per_cu = 2;
            HIP_TRY(xchg_error.alloc_zeroed(64u + (size_t)n_cus * 2u * (RT_XCHG_BLOCK / 64u) * RT_XCHG_DEBUG_WORDS * 4u));
            return RT_OK;
        }
        if (cfg.variant == 5) return rt_fail(RT_ERR_INVALID, "kernel variant 5: the scene image leaves no room for the ray rings in the LDS");
        variant = 3;   // chosen by default only: fall back to the streaming kernel
        return RT_OK;
    }
    // HBM of one pass: every sample index owns SAMPLE_BYTES of radiance + PRIMARY_BYTES of primary-ray record.  The default
    // budget — 120 GiB of the 288, but never more than 45 % of what is free on the device right now, so that two renderers of a
    // big frame can live side by side — gives the 1200x800x500 headline one pass (28.8 GB) and a 3840x2160 frame 258 spp per
    // pass (40 GiB, round 2's default, gave 86: 117 passes instead of 39 for 10 000 spp cost 1.1 % in per-pass tails).
    int size_passes() {
        uint64_t budget = 120ull << 30;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) budget = std::min<uint64_t>(budget, (uint64_t)free_b / 100u * 45u);
        const uint64_t per_sample = SAMPLE_BYTES + PRIMARY_BYTES;
        if (const char* env = std::getenv("RT06_PASS_BUDGET_BYTES")) {  // bytes of ALL per-sample buffers of a pass
            unsigned long long v = std::strtoull(env, nullptr, 10);
            if (v >= per_sample) budget = v;
        }
        const uint64_t n_pixels = n_local_pixels(tm);
        uint64_t max_spp = std::max<uint64_t>(1, budget / (n_pixels * per_sample));
        if (const char* env = std::getenv("RT06_PASS_SPP")) {  // tests force multi-pass rendering with this
            unsigned long long v = std::strtoull(env, nullptr, 10);
            if (v >= 1) max_spp = v;
        }
        max_spp = std::min<uint64_t>(max_spp, (0xF0000000ull - 1) / n_pixels);   // sample indices of a pass are 32 bits wide
        if (max_spp == 0) return rt_fail(RT_ERR_INVALID, "image too large for one pass");
        pass_spp = (uint32_t)std::min<uint64_t>(cfg.samples_per_pixel, max_spp);
        for (;;) {   // a device that cannot give the pass its buffers gets smaller passes, not an error: halve until they fit
            hipError_t e = slot[0].samples.alloc((size_t)(n_pixels * pass_spp * SAMPLE_BYTES));
            if (e == hipSuccess) e = slot[0].primary.alloc((size_t)(n_pixels * pass_spp * PRIMARY_BYTES));
            if (e == hipSuccess) break;
            (void)hipGetLastError();   // (clears the sticky out-of-memory status)
            slot[0].samples.release(); slot[0].primary.release();
            if (e != hipErrorOutOfMemory || pass_spp == 1u)
                return rt_fail(RT_ERR_HIP, "per-pass buffers (%llu bytes per sample index x %llu sample indices): %s", (unsigned long long)per_sample,
                               (unsigned long long)(n_pixels * pass_spp), hipGetErrorString(e));
            pass_spp = (pass_spp + 1u) / 2u;
        }
        n_passes = (cfg.samples_per_pixel + pass_spp - 1) / pass_spp;
        if (n_passes > 1) HIP_TRY(running.alloc((size_t)(n_pixels * 16ull)));
#ifndef RT_PHASE_TIMERS   // (the phase-timer build synchronises inside every launch: nothing to run ahead of)
        const char* ahead = std::getenv("RT06_RUN_AHEAD");
        // (BVH worlds: a HittableList or a bvh_node tree tests far more per ray, its frames are long and their tails a small share, like a multi-pass call's)
        if (n_passes == 1 && scene.dw.kind == RT_WORLD_BVH && 2u * n_pixels * pass_spp * per_sample <= budget && !(ahead && ahead[0] == '0')) add_second_slot();
#endif
        return RT_OK;
    }
    // The second frame slot, its streams and events.  A multi-pass call stays on one slot: its passes are long (the tail is ~0.1 % of them) and its buffers
    // are what the budget allowed.  A device that cannot give the second set leaves the renderer what it was: one slot, every call on the caller's stream.
    void add_second_slot() {
        hipError_t e = slot[1].samples.alloc(slot[0].samples.bytes);
        if (e == hipSuccess) e = slot[1].primary.alloc(slot[0].primary.bytes);
        if (e == hipSuccess) e = slot[1].work_counter.alloc(256);
        for (Slot& s : slot) {
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s.traced, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming);
        }
        if (e == hipSuccess) { n_slots = 2; return; }
        (void)hipGetLastError();
        drop_second_slot();
    }
    void drop_second_slot() {
        slot[1].samples.release(); slot[1].primary.release(); slot[1].work_counter.release();
        for (Slot& s : slot) {
            if (s.stream) (void)hipStreamDestroy(s.stream);
            if (s.traced) (void)hipEventDestroy(s.traced);
            if (s.consumed) (void)hipEventDestroy(s.consumed);
            s.stream = nullptr; s.traced = s.consumed = nullptr;
        }
        n_slots = 1;
    }
    // the host waits for everything queued on the slots: the generators and tracers on their streams, and the resolves that read them
    int drain_slots() {
        for (Slot& s : slot)
            if (s.stream) { HIP_TRY(hipStreamSynchronize(s.stream)); HIP_TRY(hipEventSynchronize(s.consumed)); }
        return RT_OK;
    }

    // One call's launches: samples [first_s, first_s + n_s) of every pixel, cut into passes of at most pass_spp.  Render() is (0, samples_per_pixel)
    // resolved through `running`; a refine step is (refine_done, n) resolved into `accum` (refine = true), which carries the sums from call to call.
    // run_ahead: a plain render_async.  On a two-slot renderer its generator and tracer go to the stream of slot k mod 2 (k = the calls that ran ahead so
    // far), which waits for the slot's `consumed` and for nothing of `st`: what they read is by value in the kernel arguments (the camera too) or
    // immutable after creation (the scene images), and what they write is the slot's own.  Every other call is serial on `st`, behind all that is queued.
    int launch(hipStream_t st, float* out, uint32_t first_s, uint32_t n_s, bool refine, bool run_ahead) {
        if (variant == 1) {
            RenderParams p;
            frame_params(p, cfg.samples_per_pixel, slot[0]);
            p.out = out;
            return launch_render(p, variant, st);
        }
        // two slots: one pass, a streaming kernel.  Two frames in flight on a device is what pays: a caller that already keeps a frame of ANOTHER renderer
        // in flight (bench.py --pipeline 2) would have four with run-ahead, and two generators beside the tracers (measured: 79.7 instead of 66.4 ms per frame)
        const bool ahead = run_ahead && n_slots == 2 && !another_renderer_busy(this);
        Slot& sl = slot[ahead ? n_ahead % 2u : 0u];
        const hipStream_t gs = ahead ? sl.stream : st;   // the generator's and the tracer's stream
        if (ahead) {
            if (n_ahead && hipEventQuery(slot[(n_ahead - 1u) % 2u].consumed) == hipErrorNotReady) { n_overlapped++; (void)hipGetLastError(); }
            HIP_TRY(hipStreamWaitEvent(gs, sl.consumed, 0));   // the resolve two calls ago has read these buffers
            n_ahead++;
        } else if (n_slots == 2) {
            for (Slot& s : slot) { HIP_TRY(hipStreamWaitEvent(st, s.traced, 0)); HIP_TRY(hipStreamWaitEvent(st, s.consumed, 0)); }
        }
        const LaunchOn on = launch_on(nee.mode);
        const uint32_t end_s = first_s + n_s, n_pixels = (uint32_t)n_local_pixels(tm), grid = n_cus * on.blocks_per_cu;
        StreamParams p = call_params(refine ? end_s : cfg.samples_per_pixel, sl, on);
        const uint32_t ring_at = (uint32_t)(n_renders % RT_TIMES_RING);
        kev_ahead[ring_at] = ahead;
        if (ahead && !kev_resolve0[ring_at]) HIP_TRY(hipEventCreate(&kev_resolve0[ring_at]));
        std::vector<hipEvent_t>& ring = kev[n_renders % RT_TIMES_RING];   // the event ring: this call's slot, four events per pass, created at first use
        const uint32_t call_passes = kev_passes[n_renders % RT_TIMES_RING] = (n_s + pass_spp - 1u) / pass_spp;
        while (ring.size() < (size_t)call_passes * 4u) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            ring.push_back(e);
        }
        hipEvent_t* ke = ring.data();
        for (uint32_t first = first_s; first < end_s; first += pass_spp, ke += 4) {
            const uint32_t counter_start = pass_params(p, first, end_s, grid);
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)sl.work_counter.p, (int)counter_start, 1, gs));
#ifdef RT_PHASE_TIMERS
            DevBuf phase_acc;
            HIP_TRY(phase_acc.alloc(PHASE_WORDS * sizeof(unsigned long long)));
            HIP_TRY(hipMemsetAsync(phase_acc.p, 0, PHASE_WORDS * sizeof(unsigned long long), gs));
            p.phase_acc = phase_acc.as<unsigned long long>();
#endif
            HIP_TRY(hipEventRecord(ke[0], gs));
            // RT06_PRIMARY_LDS: the generator declares LDS it does not use, more than two resident persistent workgroups leave free on a CU (160 KiB -
            // 2 x ~77 KiB).  Alone on the GPU that changes nothing.  With a SECOND frame in flight (run-ahead, or bench.py --pipeline 2) it keeps the next
            // frame's generator from moving in beside the persistent kernel's main phase and lets it start when workgroups of the draining frame exit.
            // Off by default, on both paths: measured under run-ahead it is the slower setting (EXPERIMENTS.md E13), as it was with two renderers.
            static const uint32_t primary_lds = [] { const char* e = std::getenv("RT06_PRIMARY_LDS"); return e ? (uint32_t)std::atoi(e) : 0u; }();
            for (uint32_t b0 = 0; b0 < tm.n_local_tiles; b0 += 65535u) {   // grid.y = 64-pixel block, at most 65535 per launch
                const uint32_t nb = std::min(65535u, tm.n_local_tiles - b0);
                const dim3 pgrid((64u * p.pass_spp + 255u) / 256u, nb);
                if (p.cam.type >= RT_CAM_PERSPECTIVE) hipLaunchKernelGGL(primary_rays_lens_kernel_for(p.cam), pgrid, dim3(256), primary_lds, gs, p, b0);   // this launch's camera: it may change between queued frames
                else primary_rays_kernel<<<pgrid, 256, primary_lds, gs>>>(p, b0);
                HIP_TRY(hipGetLastError());
            }
            void* args[] = {&p};
            XchgParams xp;
            if (variant == 5) { xp = xchg_params(p); args[0] = &xp; }
            HIP_TRY(hipEventRecord(ke[1], gs));
            HIP_TRY(hipLaunchKernel(on.kernel, dim3(grid), dim3(stream_block), args, on.lds_bytes, gs));
            HIP_TRY(hipEventRecord(ke[2], gs));
#ifdef RT_PHASE_TIMERS
            if (const int rc = report_phase_timers(phase_acc, gs)) return rc;
#endif
            if (ahead) {   // back to the caller's stream: the resolve writes `out`, in the caller's order
                HIP_TRY(hipEventRecord(sl.traced, gs));
                HIP_TRY(hipStreamWaitEvent(st, sl.traced, 0));
                HIP_TRY(hipEventRecord(kev_resolve0[ring_at], st));
            }
            const uint32_t last = first + p.pass_spp >= end_s ? 1u : 0u;
            if (refine) refine_resolve_kernel<<<(n_pixels + 255) / 256, 256, 0, st>>>(p, accum.as<float4>(), out, last, end_s);
            else resolve_kernel<<<(n_pixels + 255) / 256, 256, 0, st>>>(p, running.as<float4>(), out, last);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ke[3], st));
            // feature pass: after the pass's fourth timing event (rt_renderer_kernel_times keeps its meaning), before the next pass's generator
            // overwrites the primary-ray records
            if (refine && aov_on)
                if (const int rc = launch_aov(p, st)) return rc;
        }
        if (n_slots == 2) HIP_TRY(hipEventRecord(sl.consumed, st));   // (a serial call has used slot 0)
        n_renders++;
        return RT_OK;
    }
    // what the baseline and the streaming kernels' parameters share; spp = the sample count the pixels are resolved against
    template <typename Params> void frame_params(Params& p, uint32_t spp, const Slot& sl) const {
        p.width = cfg.width; p.height = cfg.height;
        p.spp = spp; p.max_depth = cfg.max_depth;
        p.seed = cfg.seed;
        p.cam = cam;
        p.world = scene.dw;
        p.tm = tm;
        p.work_counter = sl.work_counter.as<uint32_t>();
    }
    // what every pass of a call shares
    StreamParams call_params(uint32_t spp, const Slot& sl, const LaunchOn& on) const {
        StreamParams p;
        frame_params(p, spp, sl);
        p.scene = scene.packed;
        p.scene.n_top = scene.big ? n_top : 0u;
        p.scene.blob = on.blob; p.scene.blob_vec4 = on.blob_vec4;   // the mode's image: the light table, if any, is staged with the scene; the tail behind it is not
        p.samples = sl.samples.as<float4>();
        p.inner_keep = tune[0] ? tune[0] : 1u; p.shade_min = tune[1]; p.leaf_min = tune[2];
        p.inner_drop = tune[3]; p.inner_floor = tune[4];
        if (nee.on() && !tune_exit_forced) { p.inner_drop = RT_INNER_DROP; p.inner_floor = RT_INNER_FLOOR; }   // not retuned (plan_thresholds)
        const size_t n_pass = n_local_pixels(tm) * pass_spp;   // 16-B records per array
        p.prim_o = sl.primary.as<float4>();
        p.prim_d = sl.primary.as<float4>() + n_pass;
        p.prim_rng = reinterpret_cast<uint4*>(sl.primary.as<float4>() + 2 * n_pass);
        return p;
    }
    // the pass that starts at sample `first`: its share of the samples and the work-queue granularity; returns where the work counter starts
    uint32_t pass_params(StreamParams& p, uint32_t first, uint32_t end_s, uint32_t grid) const {
        p.pass_first_s = first;
        p.pass_spp = std::min(pass_spp, end_s - first);
        p.total = (uint32_t)n_local_pixels(tm) * p.pass_spp;
        // work-queue granularity: ~32 fetches per wave keep the tail short when a shard is small (multi-GPU)
        const uint32_t n_waves = grid * (stream_block / 64u);
        p.chunk = std::max(64u, std::min(RT_CHUNK_MAX, (p.total / (n_waves * 32u)) & ~63u));
        if (const char* env = std::getenv("RT06_CHUNK")) { int v = std::atoi(env); if (v >= 64 && v <= 1024) p.chunk = (uint32_t)v & ~63u; }
        // the streaming kernel's waves own their first chunk (chunk w for wave w): the counter starts behind those; the exchange
        // kernel's shader waves draw every chunk from the counter
        const uint64_t first_shared = variant == 5 ? 0ull : (uint64_t)n_waves * p.chunk;
        return (uint32_t)std::min<uint64_t>(first_shared, 0xF0000000ull);
    }
    XchgParams xchg_params(const StreamParams& p) const {
        XchgParams xp;
        xp.s = p;
        if (std::getenv("RT06_XCHG")) xp.s.inner_keep = xc.keep;
        xp.n_tracers = xc.n_tracers; xp.n_shards = xc.shards; xp.tq_cap = xc.tq_cap; xp.sq_cap = xc.sq_cap;
        xp.pop_extra = xc.pop_extra;
        xp.swap_min = xc.swap_min; xp.shade_min = xc.shade_min; xp.shade_patience = xc.patience;
        xp.scene_vec4 = xc.scene_vec4; xp.extra_in_lds = xc.extra_in_lds; xp.shader_prio = xc.prio;
        xp.error_flag = xchg_error.as<uint32_t>();
#ifdef RT_PHASE_TIMERS
        xp.xphase_acc = p.phase_acc;
#endif
        return xp;
    }
#ifdef RT_PHASE_TIMERS
    static constexpr size_t PHASE_WORDS = 32 + 96 * 16;   // cycles and visits of 16 phases, then the 96 x 16 trace histogram
    int report_phase_timers(const DevBuf& phase_acc, hipStream_t st) const {
        static unsigned long long h[PHASE_WORDS];
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(h, phase_acc.p, sizeof(h), hipMemcpyDeviceToHost));
        if (const char* hp = std::getenv("RT06_TRACE_HIST")) {   // joint histogram (inner steps x leaf tests) per trace, for tools/sched_model.py
            if (FILE* f = std::fopen(hp, "w")) {
                for (int a = 0; a < 96; a++) { for (int b = 0; b < 16; b++) std::fprintf(f, "%llu ", h[32 + a * 16 + b]); std::fprintf(f, "\n"); }
                std::fclose(f);
            }
        }
        static const char* names_stream[16] = {"hot inner loop", "irregular loop", "leaf phase", "shade (tail)", "regenerate", "begin trace", "(inner steps)", "loop top",
                                        "schedule check", "shade: miss/sky + hit common", "shade: dielectric prep", "shade: dielectric dir", "shade: on-unit-sphere loop", "shade: metal/lambert/checker", "(exact far redos)", "(... over a sign)"};
        static const char* names_xchg[16] = {"T hot inner loop", "T irregular loop", "T leaf phase", "T exchange", "T idle", "(lanes per hot step)", "(lanes per leaf phase)", "(finished per exchange)",
                                             "S wait", "S pop", "S shade", "S new samples", "S begin trace", "S push", "(traces per shade round)", "-"};
        const char* const* names = variant == 5 ? names_xchg : names_stream;
        unsigned long long tot = 0;
        for (int i = 0; i < 16; i++) if (!(variant == 5 && (i == 5 || i == 6 || i == 7 || i == 14))) tot += h[i];
        for (int i = 0; i < 16; i++)
            fprintf(stderr, "[phase] %-16s %6.2f %% of wave time, %12llu visits, %8.1f cycles per visit\n", names[i], 100.0 * h[i] / (double)tot, h[16 + i], h[16 + i] ? (double)h[i] / h[16 + i] : 0.0);
        return RT_OK;
    }
#endif
    // the feature pass of the pass in `sp`: one aov_kernel launch over its samples below aov_max (0 = all of them)
    int launch_aov(const StreamParams& sp, hipStream_t st) {
        const uint32_t pass_end = sp.pass_first_s + sp.pass_spp, upto = aov_max ? std::min(aov_max, pass_end) : pass_end;
        if (upto <= sp.pass_first_s) return RT_OK;
        const dim3 grid(((uint32_t)n_local_pixels(tm) + RT_AOV_BLOCK - 1u) / RT_AOV_BLOCK), block(RT_AOV_BLOCK);
        AovParams p;
        p.tm = sp.tm; p.world = sp.world;
        p.pass_first_s = sp.pass_first_s; p.pass_spp = sp.pass_spp; p.n_take = upto - sp.pass_first_s;
        p.prim_o = sp.prim_o; p.prim_d = sp.prim_d;
        const uint32_t first_tri = scene.dw.n_prims + scene.dw.n_quads - scene.n_triangles;
        if (aov_mode == RT_AOV_FULL) {   // §35: the plain image's tail as in mode 1, the pass's RNG records, and whether that tail holds cutout records
            const LaunchOn plain = launch_on(RT_LIGHT_SAMPLING_OFF);
            aov_kernel_full_for(scene.dw)<<<grid, block, 0, st>>>(p, aov.as<float4>(), sp.prim_rng, vn.on ? vn.table.as<rt_tri_normals>() : nullptr, plain.blob, plain.blob_vec4,
                                                                  first_tri, cut.on ? 1u : 0u);
        } else
        if (aov_mode == RT_AOV_TEXTURED) {   // §27: the plain image, whose header is zero while no rider is on; every image's tail holds the same tables
            const LaunchOn plain = launch_on(RT_LIGHT_SAMPLING_OFF);
            const uint4* blob = plain.blob;
            const uint32_t blob_vec4 = plain.blob_vec4;
            if (nm.on) {   // §28: the mapped normal; a table is on only where the world is a list or a BVH walked by the stack
                const rt_tri_normals* vt = vn.on ? vn.table.as<rt_tri_normals>() : nullptr;
                if (scene.dw.kind == RT_WORLD_LIST) aov_kernel_nmap<RT_AOV_WALK_LIST><<<grid, block, 0, st>>>(p, aov.as<float4>(), vt, blob, blob_vec4, first_tri);
                else aov_kernel_nmap<RT_AOV_WALK_STACK><<<grid, block, 0, st>>>(p, aov.as<float4>(), vt, blob, blob_vec4, first_tri);
            } else
            if (!vn.on) aov_kernel_tex_for(scene.dw)<<<grid, block, 0, st>>>(p, aov.as<float4>(), blob, blob_vec4, first_tri);
            else if (scene.dw.kind == RT_WORLD_LIST) aov_kernel_smooth_tex<RT_AOV_WALK_LIST><<<grid, block, 0, st>>>(p, aov.as<float4>(), vn.table.as<rt_tri_normals>(), blob, blob_vec4, first_tri);
            else aov_kernel_smooth_tex<RT_AOV_WALK_STACK><<<grid, block, 0, st>>>(p, aov.as<float4>(), vn.table.as<rt_tri_normals>(), blob, blob_vec4, first_tri);
        } else
        if (vn.on) {   // §21: the first-hit normal is the shading normal; a table is on only where the world is a list or a BVH walked by the stack
            if (scene.dw.kind == RT_WORLD_LIST) aov_kernel_smooth<RT_AOV_WALK_LIST><<<grid, block, 0, st>>>(p, aov.as<float4>(), vn.table.as<rt_tri_normals>(), first_tri);
            else aov_kernel_smooth<RT_AOV_WALK_STACK><<<grid, block, 0, st>>>(p, aov.as<float4>(), vn.table.as<rt_tri_normals>(), first_tri);
        } else
        aov_kernel_for(scene.dw)<<<grid, block, 0, st>>>(p, aov.as<float4>());
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
    ~rt_renderer() {
        if (dn_ev) (void)hipEventDestroy(dn_ev);
        if (refine_ev) (void)hipEventDestroy(refine_ev);
        for (auto& q : kev) for (hipEvent_t e : q) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : kev_resolve0) if (e) (void)hipEventDestroy(e);
        drop_second_slot();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// the renderers alive in this process: what a renderer that could run ahead asks about the others (launch())
static std::mutex g_live_mutex;
static std::vector<rt_renderer*> g_live;
static bool another_renderer_busy(const rt_renderer* self) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    for (const rt_renderer* o : g_live)
        if (o != self && o->cfg.device == self->cfg.device && o->timed && hipEventQuery(o->ev1) == hipErrorNotReady) { (void)hipGetLastError(); return true; }
    return false;
}

// The lens cameras exist in the streaming kernels' ray generator only: the baseline kernel calls camera_sample_ray itself
static int lens_camera_variant_check(const char* who, uint32_t variant, const rt_camera* cam) {
    if (cam->type >= RT_CAM_PERSPECTIVE && variant < 2)
        return rt_fail(RT_ERR_INVALID, "%s: the baseline kernel (variant 1) samples the reference's three cameras inside the kernel and knows no lens camera (type %u): "
                       "use a streaming variant (0, or 2 to 6) on a world that streams", who, cam->type);
    return RT_OK;
}

extern "C" int rt_renderer_create(const rt_render_config* cfg, const rt_camera* cam, const rt_world_flat* world, rt_renderer** out) {
    if (!cfg || !cam || !world || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_create: null argument");
    if (cfg->width == 0 || cfg->height == 0 || cfg->samples_per_pixel == 0)
        return rt_fail(RT_ERR_INVALID, "rt_renderer_create: width, height and samples_per_pixel must be > 0");
    if ((uint64_t)cfg->width * cfg->height > 0x7fffffffull) return rt_fail(RT_ERR_INVALID, "rt_renderer_create: image too large");
    if (cfg->world_size == 0 || cfg->rank >= cfg->world_size) return rt_fail(RT_ERR_INVALID, "rt_renderer_create: bad rank %u / world_size %u", cfg->rank, cfg->world_size);
    if (const int crc = rt_camera_check("rt_renderer_create", cam)) return crc;
    int rc = select_device(cfg->device);
    if (rc != RT_OK) return rc;
    rt_renderer* r = new rt_renderer();
    r->cfg = *cfg;
    for (uint32_t i = 0; i < world->n_materials && world->materials; i++) {
        const uint32_t t = world->materials[i].type;
        const char* refused = t == RT_MAT_ISOTROPIC ? "a constant medium (RT_MAT_ISOTROPIC)" : t == RT_MAT_LAMBERTIAN_NOISE ? "a noise texture (RT_MAT_LAMBERTIAN_NOISE)"
                            : t == RT_MAT_LAMBERTIAN_IMAGE ? "an image texture (RT_MAT_LAMBERTIAN_IMAGE)" : nullptr;
        if (!r->aov_refused) r->aov_refused = refused;   // the first such material
        if (t == RT_MAT_ISOTROPIC) r->has_medium = true;
    }
    for (uint32_t k = 0; k < 4u; k++) {   // the table modes: LIGHT_MODES' first four rows
        const uint32_t mode = LIGHT_MODES[k].mode;
        rt_renderer::LightTable& t = r->nee.tab[k];
        const uint32_t cap = mode == RT_LIGHT_SAMPLING_TREE ? RT_MAX_LIGHTS_TREE : RT_MAX_LIGHTS_MESH;
        t.kind.assign(cap, 0u); t.index.assign(cap, 0u); t.area.assign(cap, 0.0f);
        if (rt_world_light_table(world, mode, cap, t.kind.data(), t.index.data(), t.area.data(), &t.n) != RT_OK) { t.refused = rt_last_error(); t.n = 0; }
        t.none = t.refused.find("has no light to sample") != std::string::npos;
        t.kind.resize(t.n); t.index.resize(t.n); t.area.resize(t.n); t.sphere.assign((size_t)t.n * 4u, 0.0f);
        if (mode == RT_LIGHT_SAMPLING_TREE && t.n) {
            uint32_t n_nodes = 0;
            t.cdf.assign(t.n, 0.0f); t.nodes.assign((size_t)(2u * t.n - 1u) * 8u, 0.0f);
            if (rt_world_light_tree(world, t.n, t.nodes.data(), &n_nodes, t.cdf.data()) != RT_OK) { t.refused = rt_last_error(); t.n = 0; }
        }
        for (uint32_t i = 0; i < t.n; i++)
            if (t.kind[i] == RT_LIGHT_SPHERE) {   // the world's arrays are borrowed during creation only: what the table says of a sphere is taken now
                const rt_prim& pr = world->prims[t.index[i]];
                t.sphere[4u * i] = pr.c0[0]; t.sphere[4u * i + 1u] = pr.c0[1]; t.sphere[4u * i + 2u] = pr.c0[2]; t.sphere[4u * i + 3u] = pr.radius;
            }
    }
    r->cam = *cam;   // the camera of the first launch; rt_renderer_set_camera replaces it (Renderer.cu:117 reads the caller's camera at every Render())
    rc = r->scene.upload(world, true);
    if (rc != RT_OK) { delete r; return rc; }
    r->tm = make_tile_map(cfg->width, cfg->height, cfg->rank, cfg->world_size);
    size_t fb_floats = r->tm.direct ? (size_t)cfg->width * cfg->height * 4 : n_local_pixels(r->tm) * 4;
    hipError_t e = r->fb.alloc_zeroed(fb_floats * sizeof(float));
    if (e == hipSuccess) e = r->slot[0].work_counter.alloc(256);
    if (e == hipSuccess) {
        rc = r->plan();
        if (rc == RT_OK) rc = lens_camera_variant_check("rt_renderer_create", r->variant, cam);
        if (rc != RT_OK) { delete r; return rc; }
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&r->ev0);
    if (e == hipSuccess) e = hipEventCreate(&r->ev1);
    if (e != hipSuccess) { delete r; return rt_fail(RT_ERR_HIP, "rt_renderer_create: %s", hipGetErrorString(e)); }
    { std::lock_guard<std::mutex> lock(g_live_mutex); g_live.push_back(r); }
    *out = r;
    return RT_OK;
}

extern "C" void rt_renderer_destroy(rt_renderer* r) {
    if (!r) return;
    (void)hipSetDevice(r->cfg.device);
    { std::lock_guard<std::mutex> lock(g_live_mutex); g_live.erase(std::remove(g_live.begin(), g_live.end(), r), g_live.end()); }
    (void)r->drain_slots();   // queued launches read and write what is freed below
    delete r;
}

// one call's launches between the renderer's two timing events on the caller's stream (a call that runs ahead has its resolve between them, and
// the wait for its tracer)
static int enqueue_call(rt_renderer* r, void* hip_stream, float* d_out, uint32_t first_s, uint32_t n_s, bool refine, bool run_ahead = false) {
    if (r->scene.dw.background == 2u && !r->env.on)   // never launch with a dangling record
        return rt_fail(RT_ERR_INVALID, "the world's background is an environment map (mode 2) and the renderer has none: give it one with rt_renderer_environment before rendering");
    if (uint32_t k = 0u; r->image_index_unserved(&k))   // never launch on an index the table does not hold
        return rt_fail(RT_ERR_INVALID, "an image material of the world names image %u and the renderer's texture table has no such entry: give it one with rt_renderer_textures before rendering", k);
    if (uint32_t k = 0u; r->entry_missing(r->nm, [](const rt_normal_map& m) { return m.on != 0u; }, &k))   // ... nor on a normal map the table does not hold
        return rt_fail(RT_ERR_INVALID, "a normal map of the world names image %u and the renderer's texture table has no such entry: give it one with rt_renderer_textures before rendering", k);
    if (uint32_t k = 0u; r->entry_missing(r->cut, [](const rt_cutout& m) { return m.on != RT_CUTOUT_OFF; }, &k))   // ... nor on a cutout mask it does not hold: every record that is on names one
        return rt_fail(RT_ERR_INVALID, "a cutout record of the world names image %u and the renderer's texture table has no such entry: give it one with rt_renderer_textures before rendering", k);
    if (uint32_t k = 0u; r->entry_missing(r->mf, [](const rt_microfacet& m) { return m.on == RT_MICROFACET_MAPPED || m.on == RT_MICROFACET_GLASS_MAPPED; }, &k))   // ... nor on a roughness map it does not hold; constant records need no texture table
        return rt_fail(RT_ERR_INVALID, "a roughness map of the world names image %u and the renderer's texture table has no such entry: give it one with rt_renderer_textures before rendering", k);
    HIP_TRY(hipSetDevice(r->cfg.device));
    hipStream_t st = (hipStream_t)hip_stream;  // NULL is the HIP null stream, as for any HIP launch
    HIP_TRY(hipEventRecord(r->ev0, st));
    int rc = r->launch(st, d_out ? d_out : r->fb.as<float>(), first_s, n_s, refine, run_ahead);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipEventRecord(r->ev1, st));
    r->timed = true;
    return RT_OK;
}

extern "C" int rt_renderer_render_async(rt_renderer* r, void* hip_stream, float* d_out) {
    if (!r) return rt_fail(RT_ERR_INVALID, "rt_renderer_render_async: null renderer");
    return enqueue_call(r, hip_stream, d_out, 0u, r->cfg.samples_per_pixel, false, true);
}

// the work of the last call may be on a caller's stream (the _async entry points): its end event orders what reads the results
static int wait_last_call(rt_renderer* r) {
    HIP_TRY(hipSetDevice(r->cfg.device));
    if (r->timed) HIP_TRY(hipEventSynchronize(r->ev1));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return r->drain_slots();   // ... and calls before the last may have been given other streams
}

// after a synchronisation: ray-exchange protocol error / traversal-queue overflow (both flags are read and cleared by their checks)
int rt_renderer_check_device_flags(rt_renderer* r) {
    const int rc = check_xchg_error(r->xchg_error);
    return rc != RT_OK ? rc : check_traversal_overflow(r->scene);
}

// A tile-major buffer of one shard that is the whole frame (world_size 1), `fpp` floats per local pixel, into the frame's row-major order on the host.
static int download_tile_major(rt_renderer* r, const DevBuf& src, uint32_t fpp, float* host) {
    if (const int rc = wait_last_call(r)) return rc;
    const uint32_t n_local = (uint32_t)n_local_pixels(r->tm);
    std::vector<float> local((size_t)n_local * fpp);
    HIP_TRY(hipMemcpy(local.data(), src.p, local.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<uint32_t> gid(n_local);
    if (const int rc = rt_shard_pixel_map(r->cfg.width, r->cfg.height, 1u, 0u, gid.data(), gid.size())) return rc;
    for (uint32_t L = 0; L < n_local; L++)
        if (gid[L] != 0xffffffffu) std::memcpy(host + (size_t)gid[L] * fpp, local.data() + (size_t)L * fpp, fpp * sizeof(float));
    return RT_OK;
}

extern "C" int rt_renderer_set_camera(rt_renderer* r, const rt_camera* cam) {
    if (!r || !cam) return rt_fail(RT_ERR_INVALID, "rt_renderer_set_camera: null argument");
    if (const int rc = rt_camera_check("rt_renderer_set_camera", cam)) return rc;
    if (const int rc = lens_camera_variant_check("rt_renderer_set_camera", r->variant, cam)) return rc;
    if (std::memcmp(&r->cam, cam, sizeof(rt_camera)) == 0) return RT_OK;   // the same bytes: nothing moves, the refinement goes on
    r->cam = *cam;          // travels by value in the kernel arguments of the NEXT launch; launches already enqueued keep theirs (those that run ahead too: no drain)
    r->refine_done = 0;     // samples accumulated under another camera belong to another frame
    r->aov_done = 0;        // ... and so do their first hits
    return RT_OK;
}

// Light sampling.  Off: every launch is what it was.  On: the mode's form of the renderer's own kernel on the mode's image (LIGHT_MODES, rt_renderer::launch_on).
// One sequence for every mode: refusals — variant; for the modes of the map: background, queue, medium, no map; the table's own —, then, behind a wait for every
// launch already enqueued (they keep their kernel and their image: nothing below frees or overwrites a buffer a queued launch may read), the image, the kernel,
// its LDS limit and the map's distribution, each built once.  A failure leaves the mode as it was, and what was not finished is tried again by the next call.
extern "C" int rt_renderer_light_sampling_enable(rt_renderer* r, uint32_t on) {
    if (!r) return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: null renderer");
    const LightMode* m = light_mode(on);
    if (on != RT_LIGHT_SAMPLING_OFF && !m)   // 3 is no mode
        return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: on must be 0 (off), 1 (quad lights), 2 (quad and sphere lights), 4 (quad, sphere and triangle lights), 16 (those, through a light tree, chosen by area) or 32 (the environment map), or 48 (the map and the light tree together)");
    if (on == r->nee.mode) return RT_OK;   // nothing changes, the refinement goes on
    if (m) {
        const rt_renderer::LightTable* t = m->image ? &r->nee.tab[m->image - 1u] : nullptr;
        if (r->variant < 2 || r->variant == 5 || r->tol)
            return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: kernel variant %u has no light-sampling form (the baseline kernel 1, the ray exchange 5 and the tolerance mode 6 do not; use variant 0, 2 or 3)", r->tol ? 6u : r->variant);
        for (uint32_t g = 0; g < N_RUNGS; g++)   // (the lowest rung that is on speaks)
            if (const FormRung& f = FORM_LADDER[g]; r->rung_on(g) && on != RT_LIGHT_SAMPLING_ENV_TREE)
                return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: the renderer has %s %s, and light-sampling mode %u has no kernel that reads one: %s with light sampling off or in mode 48 (take the table away with %s(NULL, 0) first)", f.a, f.table, on, f.surfaces_render, f.api);
        if (m->env && r->scene.dw.background != 2u)   // a world of this kind takes the modes of the light tables only, so the message lists them
            return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: mode %u samples the environment map of a world with background mode 2 (rt_scene_set_environment)%s; this world's is %u, for which on must be 0 (off), 1 (quad lights), 2 (quad and sphere lights), 4 (quad, sphere and triangle lights) or 16 (those, through a light tree, chosen by area)", on, m->beside, r->scene.dw.background);
        if (m->env && r->scene.queue)
            return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: %sa world with a queue or wide4 traversal renders on lane walks that have no light-sampling form (RT_TRAVERSAL_STACK and lists do)", m->tag);
        if (m->env && r->has_medium)
            return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: %sthe world has a constant medium (RT_MAT_ISOTROPIC), %s", m->tag, m->medium);
        if (m->env && !r->env.on)
            return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: %sthe renderer has no environment map to sample: give it one with rt_renderer_environment first", m->tag);
        if (t && !t->refused.empty() && !(m->env && t->none))   // beside the map, a world with no light at all is the map alone (§26): its table is the header
            return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: %s%s", m->tag, t->refused.c_str());
        if (const int rc = wait_last_call(r)) return rc;   // (sets the device)
        if (m->image && !r->nee.image[m->image].blob.p) {   // the image with the mode's table, once (mode 16's serves mode 48 too)
            rt_renderer::Image fresh;
            if (const int rc = r->compose(m->image, fresh)) return rc;
            std::swap(r->nee.image[m->image], fresh);
        }
        auto& resolved = r->nee.resolved[m - LIGHT_MODES];
        if (!resolved.kernel) {   // set last: a failure on the way is tried again
            const uint32_t key = stream_kernel_key(r->variant, false, r->scene) | m->key_bits;
            const void* k = stream_kernel_for(key);
            if (!k) return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_enable: %s%s", m->tag, m->no_form);
            uint32_t lds_set = r->launch_on(on).lds_bytes;   // one kernel may serve several tables: the attribute covers the largest of its own
            for (const LightMode& o : LIGHT_MODES)
                if (r->nee.resolved[&o - LIGHT_MODES].kernel == k) lds_set = std::max(lds_set, r->launch_on(o.mode).lds_bytes);
            HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_set));
            resolved.key = key;
            resolved.kernel = k;
        }
        for (uint32_t g = 0; g < N_RUNGS; g++)   // mode 48's form of every rung that is on, on the image of mode 16's table
            if (r->rung_on(g))
                if (const int rc = r->resolve_form_kernel(g, true, r->launch_on(on).lds_bytes)) return rc;
        if (m->env && !r->env.dist_on) {   // the distribution of the map as it stands (a map given while the mode is on brings its own: rt_renderer_environment); an all-black map is refused here
            char who[64];
            std::snprintf(who, sizeof(who), "rt_renderer_light_sampling_enable: mode %u", on);
            rt_renderer::Environment next;
            next.on = true; next.w = r->env.w; next.h = r->env.h; next.u0 = r->env.u0; next.host = r->env.host;
            if (const int rc = rt_renderer::upload_environment(who, next, true)) return rc;
            if (const int rc = r->replace_rider(r->env, next)) return rc;
        }
    }
    r->nee.mode = on;       // of the NEXT launch
    r->refine_done = 0;     // samples drawn by another estimator belong to another sequence
    r->aov_done = 0;
    return RT_OK;
}

extern "C" int rt_renderer_light_sampling_info(rt_renderer* r, uint32_t out[2]) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_light_sampling_info: null argument");
    out[0] = r->nee.mode;
    out[1] = r->launch_on(r->nee.mode).lights;   // §24: of a map sampled alone, its texels
    return RT_OK;
}

// The table setters.  Each builds the next state of its rider — its own record loop and canonical form (what no kernel reads is zero, so that equal tables are
// equal bytes) — between a shared beginning and a shared end.
// The beginning of a per-triangle table's setter (vertex normals, texture coordinates): what it refuses before it reads a record.
static int triangle_table_refusal(const char* api, const char* what, rt_renderer* r, bool has_table, uint32_t n) {
    if (!r) return rt_fail(RT_ERR_INVALID, "%s: null renderer", api);
    if (has_table != (n != 0u)) return rt_fail(RT_ERR_INVALID, "%s: a table and its count go together (NULL, 0 turns it off)", api);
    if (!n) return RT_OK;
    if (r->variant < 2) return rt_fail(RT_ERR_INVALID, "%s: the baseline kernel (variant 1) reads no %s; use variant 0, 2 or 3", api, what);
    if (r->scene.queue) return rt_fail(RT_ERR_INVALID, "%s: a world with a queue or wide4 traversal renders on lane walks that read no %s (RT_TRAVERSAL_STACK and lists do)", api, what);
    if (r->variant == 5 || r->tol) return rt_fail(RT_ERR_INVALID, "%s: kernel variant %u renders no triangles", api, r->tol ? 6u : 5u);
    if (n != r->scene.n_triangles) return rt_fail(RT_ERR_INVALID, "%s: %u records for a world of %u triangles", api, n, r->scene.n_triangles);
    return RT_OK;
}
// The beginning of a per-material table's setter (rung g of FORM_LADDER); `extra` holds the setter's own refusals, which come before the count's.
template <typename Extra> static int material_table_refusal(uint32_t g, rt_renderer* r, bool has_table, uint32_t n, Extra extra) {
    const FormRung& f = FORM_LADDER[g];
    if (!r) return rt_fail(RT_ERR_INVALID, "%s: null renderer", f.api);
    if (has_table != (n != 0u)) return rt_fail(RT_ERR_INVALID, "%s: a table and its count go together (NULL, 0 turns it off)", f.api);
    if (!n) return RT_OK;
    if (r->variant < 2) return rt_fail(RT_ERR_INVALID, "%s: the baseline kernel (variant 1) reads no %s; use variant 0, 2 or 3", f.api, f.table);
    if (r->variant == 5 || r->tol) return rt_fail(RT_ERR_INVALID, "%s: kernel variant %u %s", f.api, r->tol ? 6u : 5u, f.variant_5_6);
    if (r->scene.queue) return rt_fail(RT_ERR_INVALID, "%s: a world with a queue or wide4 traversal renders on lane walks that read no %s (RT_TRAVERSAL_STACK and lists do)", f.api, f.table);
    if (r->scene.dw.kind == RT_WORLD_NODE_TREE) return rt_fail(RT_ERR_INVALID, "%s: a bvh_node tree renders on a walk that reads no %s (BVHs walked by the stack and lists do)", f.api, f.table);
    if (r->nee.on() && r->nee.mode != RT_LIGHT_SAMPLING_ENV_TREE)
        return rt_fail(RT_ERR_INVALID, "%s: light-sampling mode %u is on, which has no kernel that reads %s %s: %s with light sampling off or in mode 48", f.api, r->nee.mode, f.a, f.table, f.surfaces_render);
    if (const int rc = extra()) return rc;
    if (n != r->scene.dw.n_mats) return rt_fail(RT_ERR_INVALID, "%s: %u records for a world of %u materials", f.api, n, r->scene.dw.n_mats);
    return RT_OK;
}
// The end of every table's setter.  Nothing happens if `next` is the state the rider is in.  Else, behind a wait for the launches already enqueued, which read the
// images that are replaced (it sets the device), the forms of the table's rung are resolved (g; N_RUNGS: a table every kernel reads) and the rider replaced.  A
// failure leaves table, kernels, images and refinement as they were.
template <typename Rider> static int install_table(rt_renderer* r, uint32_t g, Rider& rider, Rider& next) {
    if (rt_renderer::same_table(rider, next)) return RT_OK;
    if (const int rc = wait_last_call(r)) return rc;
    if (next.on && g < N_RUNGS) {   // the plain form, and mode 48's while that mode is on
        if (const int rc = r->resolve_form_kernel(g, false, r->stream_lds_bytes)) return rc;
        if (r->nee.mode == RT_LIGHT_SAMPLING_ENV_TREE)
            if (const int rc = r->resolve_form_kernel(g, true, r->launch_on(RT_LIGHT_SAMPLING_ENV_TREE).lds_bytes)) return rc;
    }
    return r->replace_rider(rider, next);
}

// Smooth shading.  Off: every launch is what it was.  On: the same kernels on images whose tail holds the table.
extern "C" int rt_renderer_shading_normals(rt_renderer* r, const rt_tri_normals* table, uint32_t n) {
    if (const int rc = triangle_table_refusal("rt_renderer_shading_normals", "table of vertex normals", r, table != nullptr, n)) return rc;
    decltype(r->vn) next;   // off, unless a table is given; the other riders stay as they are
    for (uint32_t i = 0; i < n; i++) {
        const float* v = table[i].n0;   // nine floats: n0, n1, n2
        uint32_t n_zero = 0;
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(v[k])) return rt_fail(RT_ERR_INVALID, "rt_renderer_shading_normals: record %u: a value that is not finite", i);
        for (int k = 0; k < 3; k++)
            if (v[3 * k] == 0.0f && v[3 * k + 1] == 0.0f && v[3 * k + 2] == 0.0f) n_zero++;
        if (n_zero != 0u && n_zero != 3u) return rt_fail(RT_ERR_INVALID, "rt_renderer_shading_normals: record %u: %u of its three normals are zero (all zero = a flat triangle, or none)", i, n_zero);
        if (n_zero == 0u) next.n_smooth++;
    }
    if (n) { next.on = true; next.host.assign(table[0].n0, table[0].n0 + (size_t)n * 9u); }
    if (n && !rt_renderer::same_table(r->vn, next)) {   // the feature pass's flat copy, of a table that will be installed
        HIP_TRY(hipSetDevice(r->cfg.device));
        HIP_TRY(next.table.upload(next.host.data(), next.host.size() * sizeof(float)));
    }
    return install_table(r, N_RUNGS, r->vn, next);
}

// Texture coordinates, as the normals above: off, every launch is what it was; on, the same kernels on images whose tail holds the table.
extern "C" int rt_renderer_texture_coords(rt_renderer* r, const rt_tri_uvs* table, uint32_t n) {
    if (const int rc = triangle_table_refusal("rt_renderer_texture_coords", "table of texture coordinates", r, table != nullptr, n)) return rc;
    decltype(r->uv) next;
    static const float identity[6] = {0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f};
    for (uint32_t i = 0; i < n; i++) {
        const float* v = table[i].t0;   // six floats: t0, t1, t2
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(v[k])) return rt_fail(RT_ERR_INVALID, "rt_renderer_texture_coords: record %u: a value that is not finite", i);
        for (int k = 0; k < 6; k++)
            if (v[k] != identity[k]) { next.n_mapped++; break; }
    }
    if (n) { next.on = true; next.host.assign(table[0].t0, table[0].t0 + (size_t)n * 6u); }
    return install_table(r, N_RUNGS, r->uv, next);
}

// What a table's _info query answers: whether the rider is on, and how many of its records say something
template <typename Rider> static int rider_info(const char* api, rt_renderer* r, uint32_t out[2], Rider rt_renderer::* rider) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "%s: null argument", api);
    out[0] = (r->*rider).on ? 1u : 0u;
    out[1] = (r->*rider).on ? (r->*rider).count() : 0u;
    return RT_OK;
}
extern "C" int rt_renderer_texture_coords_info(rt_renderer* r, uint32_t out[2]) { return rider_info("rt_renderer_texture_coords_info", r, out, &rt_renderer::uv); }

// The environment map of a background-2 world.  The texels live in a buffer of the renderer's own; every image it launches on gets the tail record
// that points there.  Off, a background-2 renderer refuses to launch (enqueue_call).
extern "C" int rt_renderer_environment(rt_renderer* r, uint32_t width, uint32_t height, const float* rgb, float u0) {
    if (!r) return rt_fail(RT_ERR_INVALID, "rt_renderer_environment: null renderer");
    const bool off = rgb == nullptr && width == 0u && height == 0u;
    if (!off) {
        if (r->scene.dw.background != 2u)
            return rt_fail(RT_ERR_INVALID, "rt_renderer_environment: the world's background mode is %u; an environment map belongs to a world created with mode 2 (rt_scene_set_environment)", r->scene.dw.background);
        if (const char* why = rt_environment_image_refusal(width, height, rgb)) return rt_fail(RT_ERR_INVALID, "rt_renderer_environment: %s", why);
        if (!(u0 >= 0.0f && u0 < 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_renderer_environment: u0 must lie in [0, 1)");
    }
    const size_t n_texels = (size_t)width * height;
    if (off ? !r->env.on : (r->env.on && r->env.w == width && r->env.h == height && std::memcmp(&r->env.u0, &u0, 4) == 0 &&
                            std::memcmp(r->env.host.data(), rgb, n_texels * 3u * sizeof(float)) == 0)) return RT_OK;   // nothing changes, the refinement goes on
    const bool sampled = r->nee.mode == RT_LIGHT_SAMPLING_ENV || r->nee.mode == RT_LIGHT_SAMPLING_ENV_TREE;   // §24, §26: the map is being sampled: it cannot leave, and its successor brings a distribution
    if (sampled && off)
        return rt_fail(RT_ERR_INVALID, "rt_renderer_environment: the map is being sampled (light-sampling mode %u): switch light sampling off before taking the map away", r->nee.mode);
    if (const int rc = wait_last_call(r)) return rc;   // launches already enqueued read the images and the texels that are replaced below
    rt_renderer::Environment next;
    if (!off) {   // a map that is being sampled brings its distribution; an all-black successor is refused here, and the old map stays as it is
        char who[64] = "rt_renderer_environment";
        if (sampled) std::snprintf(who, sizeof(who), "rt_renderer_environment: light-sampling mode %u is on", r->nee.mode);
        next.on = true; next.w = width; next.h = height; next.u0 = u0;
        next.host.assign(rgb, rgb + n_texels * 3u);
        if (const int rc = rt_renderer::upload_environment(who, next, sampled)) return rc;
    }
    return r->replace_rider(r->env, next);   // (samples lit by another sky belong to another frame)
}

extern "C" int rt_renderer_environment_info(rt_renderer* r, uint32_t out[4]) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_environment_info: null argument");
    out[0] = r->env.on ? 1u : 0u; out[1] = r->env.w; out[2] = r->env.h;
    std::memcpy(&out[3], &r->env.u0, 4);
    return RT_OK;
}

// The texture table.  The texels live in a buffer of the renderer's own, one dword per texel; every image it launches on gets the entries in its
// tail.  Off, image hits read the world's image as ever, and a launch whose materials name an image above 0 is refused (enqueue_call).
extern "C" int rt_renderer_textures(rt_renderer* r, const rt_texture* records, uint32_t n, const uint8_t* texels) {
    if (!r) return rt_fail(RT_ERR_INVALID, "rt_renderer_textures: null renderer");
    const bool off = records == nullptr && n == 0u;
    uint64_t n_texels = 0;
    if (!off) {
        if (r->variant < 2) return rt_fail(RT_ERR_INVALID, "rt_renderer_textures: the baseline kernel (variant 1) reads no texture table; use variant 0, 2 or 3");
        if (r->variant == 5 || r->tol) return rt_fail(RT_ERR_INVALID, "rt_renderer_textures: kernel variant %u renders no image textures and reads no texture table", r->tol ? 6u : 5u);
        if (const char* why = rt_texture_table_refusal(records, n, texels, &n_texels)) return rt_fail(RT_ERR_INVALID, "rt_renderer_textures: %s", why);
    }
    if (off ? !r->tex.on : (r->tex.on && r->tex.records.size() == n && std::memcmp(r->tex.records.data(), records, n * sizeof(rt_texture)) == 0 &&
                            (n_texels == 0u || std::memcmp(r->tex.host.data(), texels, n_texels * 3u) == 0))) return RT_OK;   // nothing changes, the refinement goes on
    decltype(r->tex) next;   // everything that can fail comes before anything changes
    if (!off) {
        std::vector<uint32_t> dwords(n_texels ? n_texels : 1u, 0u);
        for (uint64_t i = 0; i < n_texels; i++) dwords[i] = (uint32_t)texels[3u * i] | (uint32_t)texels[3u * i + 1u] << 8 | (uint32_t)texels[3u * i + 2u] << 16;
        HIP_TRY(hipSetDevice(r->cfg.device));
        HIP_TRY(next.texels.upload(dwords.data(), dwords.size() * sizeof(uint32_t)));
        next.on = true; next.records.assign(records, records + n); next.host.assign(texels, texels + n_texels * 3u);
    }
    if (const int rc = wait_last_call(r)) return rc;   // launches already enqueued read the images and the texels that are replaced below
    return r->replace_rider(r->tex, next);   // (samples textured by other images belong to another frame)
}

// Normal maps.  Off: every launch is what it was.  On: the NMAP form of the renderer's kernel on images whose tail holds the records behind the
// texture table.  The entries the records name are checked at every launch (enqueue_call), as an image material's is: the tables come and go independently.
extern "C" int rt_renderer_normal_maps(rt_renderer* r, const rt_normal_map* table, uint32_t n) {
    if (const int rc = material_table_refusal(RUNG_NMAP, r, table != nullptr, n, [&] {
            return r->aov_on && r->aov_mode == RT_AOV_PLAIN
                ? rt_fail(RT_ERR_INVALID, "rt_renderer_normal_maps: the plain feature pass is on, whose normals know no normal map: enable it in RT_AOV_TEXTURED mode (rt_renderer_aov_enable_mode)") : RT_OK;
        })) return rc;
    rt_renderer::NormalMaps next;
    for (uint32_t i = 0; i < n; i++) {
        if (!table[i].on) continue;
        const uint32_t type = r->scene.mat_types[i];
        if (type == RT_MAT_DIELECTRIC || type == RT_MAT_DIFFUSE_LIGHT || type == RT_MAT_ISOTROPIC)
            return rt_fail(RT_ERR_INVALID, "rt_renderer_normal_maps: record %u: a dielectric, a light or a medium takes no normal map", i);
        if (table[i].image >= RT_MAX_IMAGES) return rt_fail(RT_ERR_INVALID, "rt_renderer_normal_maps: record %u: an image index lies in [0, %u)", i, RT_MAX_IMAGES);
        if (!(std::isfinite(table[i].strength) && table[i].strength >= 0.0f)) return rt_fail(RT_ERR_INVALID, "rt_renderer_normal_maps: record %u: a strength must be finite and >= 0", i);
        next.n_mapped++;
    }
    if (n) {
        next.on = true; next.host.assign(table, table + n);
        for (rt_normal_map& m : next.host) { m.pad = 0u; if (!m.on) m = rt_normal_map{0u, 0u, 0.0f, 0u}; }
    }
    return install_table(r, RUNG_NMAP, r->nm, next);   // (samples shaded with other normals belong to another frame)
}

extern "C" int rt_renderer_normal_maps_info(rt_renderer* r, uint32_t out[2]) { return rider_info("rt_renderer_normal_maps_info", r, out, &rt_renderer::nm); }

// Microfacet surfaces.  Off: every launch is what it was.  On: the MFAC form of the renderer's kernel on images whose tail ends with the records.
// The entries mapped records name are checked at every launch (enqueue_call), as a normal map's are: the tables come and go independently.
extern "C" int rt_renderer_microfacets(rt_renderer* r, const rt_microfacet* table, uint32_t n) {
    if (const int rc = material_table_refusal(RUNG_MFAC, r, table != nullptr, n, [] { return RT_OK; })) return rc;
    rt_renderer::Microfacets next;
    for (uint32_t i = 0; i < n; i++) {
        if (table[i].on == RT_MICROFACET_OFF) continue;
        const bool glass = table[i].on == RT_MICROFACET_GLASS || table[i].on == RT_MICROFACET_GLASS_MAPPED;   // §30: kinds of their own, on dielectrics alone
        if (glass) {
            if (r->scene.mat_types[i] != RT_MAT_DIELECTRIC) return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: a rough-glass record (on = %u) belongs on a dielectric alone", i, table[i].on);
            if (table[i].on == RT_MICROFACET_GLASS_MAPPED && table[i].image >= RT_MAX_IMAGES) return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: a rough-glass record's image index lies in [0, %u)", i, RT_MAX_IMAGES);
            if (!(std::isfinite(table[i].roughness) && table[i].roughness >= 0.0f && table[i].roughness <= 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: a rough-glass record's roughness must be finite and in [0, 1]", i);
            if (table[i].specular != 0.0f) return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: a rough-glass record reads no specular; it is stored as 0", i);
            next.n_on++;
            continue;
        }
        if (table[i].on > RT_MICROFACET_MAPPED) return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: on is 0 (off), 1 (constant roughness) or 2 (roughness under a map), not %u", i, table[i].on);
        const uint32_t type = r->scene.mat_types[i];
        if (type == RT_MAT_DIELECTRIC || type == RT_MAT_DIFFUSE_LIGHT || type == RT_MAT_ISOTROPIC)
            return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: a dielectric, a light or a medium takes no microfacet record", i);
        if (table[i].on == RT_MICROFACET_MAPPED && table[i].image >= RT_MAX_IMAGES) return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: an image index lies in [0, %u)", i, RT_MAX_IMAGES);
        if (!(std::isfinite(table[i].roughness) && table[i].roughness >= 0.0f && table[i].roughness <= 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: a roughness must be finite and in [0, 1]", i);
        if (!(std::isfinite(table[i].specular) && table[i].specular >= 0.0f && table[i].specular <= 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_renderer_microfacets: record %u: a specular must be finite and in [0, 1]", i);
        next.n_on++;
    }
    if (n) {
        next.on = true; next.host.assign(table, table + n);
        for (rt_microfacet& m : next.host) {
            if (m.on == RT_MICROFACET_OFF) m = rt_microfacet{RT_MICROFACET_OFF, 0u, 0.0f, 0.0f};
            if (m.on == RT_MICROFACET_CONSTANT || m.on == RT_MICROFACET_GLASS) m.image = 0u;
            if (m.on == RT_MICROFACET_GLASS || m.on == RT_MICROFACET_GLASS_MAPPED) m.specular = 0.0f;
        }
    }
    return install_table(r, RUNG_MFAC, r->mf, next);   // (samples scattered by another rule belong to another frame)
}

extern "C" int rt_renderer_microfacets_info(rt_renderer* r, uint32_t out[2]) { return rider_info("rt_renderer_microfacets_info", r, out, &rt_renderer::mf); }

// Solid glass.  Off: every launch is what it was.  On: the INTR form of the renderer's kernel on images whose tail ends with a sub-header and both
// record tables.  A refusal leaves the table and the kernel as they were.
extern "C" int rt_renderer_interiors(rt_renderer* r, const rt_interior* table, uint32_t n) {
    if (const int rc = material_table_refusal(RUNG_INTR, r, table != nullptr, n, [] { return RT_OK; })) return rc;
    rt_renderer::Interiors next;
    for (uint32_t i = 0; i < n; i++) {
        if (table[i].on == RT_INTERIOR_OFF) continue;
        if (table[i].on != RT_INTERIOR_SOLID) return rt_fail(RT_ERR_INVALID, "rt_renderer_interiors: record %u: on is 0 (off) or 1 (solid), not %u", i, table[i].on);
        if (r->scene.mat_types[i] != RT_MAT_DIELECTRIC) return rt_fail(RT_ERR_INVALID, "rt_renderer_interiors: record %u: an interior record belongs on a dielectric alone", i);
        if (r->cut.on && r->cut.host[i].on != RT_CUTOUT_OFF) return rt_fail(RT_ERR_INVALID, "rt_renderer_interiors: record %u: the material has a cutout record, and a holed solid has no inside", i);
        for (int c = 0; c < 3; c++)
            if (!(std::isfinite(table[i].sigma[c]) && table[i].sigma[c] >= 0.0f)) return rt_fail(RT_ERR_INVALID, "rt_renderer_interiors: record %u: an absorption coefficient must be finite and >= 0", i);
        next.n_on++;
    }
    if (n) {
        next.on = true; next.host.assign(table, table + n);
        for (rt_interior& m : next.host)   // (-0 is 0)
            for (int c = 0; c < 3; c++) m.sigma[c] = m.on == RT_INTERIOR_OFF ? 0.0f : m.sigma[c] + 0.0f;
    }
    return install_table(r, RUNG_INTR, r->in, next);   // (samples that crossed the glass by another rule belong to another frame)
}

extern "C" int rt_renderer_interiors_info(rt_renderer* r, uint32_t out[2]) { return rider_info("rt_renderer_interiors_info", r, out, &rt_renderer::in); }

// Alpha cutouts.  Off: every launch is what it was.  On: the CUT form of the renderer's kernel on images whose tail ends with a sub-header and
// the record tables, the cutout records last.  A refusal leaves the table and the kernel as they were.  The entries the records name are checked at every
// launch (enqueue_call), as a normal map's are: the tables come and go independently.
extern "C" int rt_renderer_cutouts(rt_renderer* r, const rt_cutout* table, uint32_t n) {
    if (const int rc = material_table_refusal(RUNG_CUT, r, table != nullptr, n, [&] {
            if (r->aov_on && r->aov_mode != RT_AOV_FULL)   // §35: mode 2 follows the table
                return rt_fail(RT_ERR_INVALID, "rt_renderer_cutouts: feature buffers are on, and the feature pass does not know the cutout rule: its first hits would be the solid cards, and a denoiser guided by them would be wrong without a sign");
            if (!r->tex.on) return rt_fail(RT_ERR_INVALID, "rt_renderer_cutouts: the renderer has no texture table to take a mask from: give it one with rt_renderer_textures first");
            return (int)RT_OK;
        })) return rc;
    rt_renderer::Cutouts next;
    for (uint32_t i = 0; i < n; i++) {
        if (table[i].on == RT_CUTOUT_OFF) continue;
        if (table[i].on != RT_CUTOUT_MASKED) return rt_fail(RT_ERR_INVALID, "rt_renderer_cutouts: record %u: on is 0 (off) or 1 (masked), not %u", i, table[i].on);
        const uint32_t type = r->scene.mat_types[i];
        if (type == RT_MAT_DIFFUSE_LIGHT || type == RT_MAT_ISOTROPIC)
            return rt_fail(RT_ERR_INVALID, "rt_renderer_cutouts: record %u: a light or a medium takes no cutout", i);
        if (r->in.on && r->in.host[i].on != RT_INTERIOR_OFF) return rt_fail(RT_ERR_INVALID, "rt_renderer_cutouts: record %u: the material has an interior record, and a holed solid has no inside", i);
        if (table[i].image >= RT_MAX_IMAGES) return rt_fail(RT_ERR_INVALID, "rt_renderer_cutouts: record %u: an image index lies in [0, %u)", i, RT_MAX_IMAGES);
        if (!(std::isfinite(table[i].cutoff) && table[i].cutoff >= 0.0f && table[i].cutoff <= 1.0f)) return rt_fail(RT_ERR_INVALID, "rt_renderer_cutouts: record %u: a cutoff must be finite and in [0, 1]", i);
        next.n_on++;
    }
    if (n) {
        next.on = true; next.host.assign(table, table + n);
        for (rt_cutout& m : next.host) {   // (-0 is 0)
            m.reserved = 0u;
            if (m.on == RT_CUTOUT_OFF) m = rt_cutout{RT_CUTOUT_OFF, 0u, 0.0f, 0u}; else m.cutoff = m.cutoff + 0.0f;
        }
    }
    return install_table(r, RUNG_CUT, r->cut, next);   // (samples that saw the cards whole belong to another frame)
}

extern "C" int rt_renderer_cutouts_info(rt_renderer* r, uint32_t out[2]) { return rider_info("rt_renderer_cutouts_info", r, out, &rt_renderer::cut); }

extern "C" int rt_renderer_textures_info(rt_renderer* r, uint32_t out[2]) { return rider_info("rt_renderer_textures_info", r, out, &rt_renderer::tex); }

extern "C" int rt_renderer_shading_normals_info(rt_renderer* r, uint32_t out[2]) { return rider_info("rt_renderer_shading_normals_info", r, out, &rt_renderer::vn); }

extern "C" int rt_renderer_refine_async(rt_renderer* r, void* hip_stream, float* d_out, uint32_t n_samples) {
    if (!r) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_async: null renderer");
    if (r->variant < 2)
        return rt_fail(RT_ERR_INVALID, "rt_renderer_refine: the baseline kernel (variant 1) keeps no per-sample buffer to accumulate from; refinement needs a streaming variant (0, or 2 to 6)");
    if (n_samples == 0) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine: n_samples must be > 0");
    if ((uint64_t)r->refine_done + n_samples > 0x80000000ull)
        return rt_fail(RT_ERR_INVALID, "rt_renderer_refine: %u + %u samples per pixel pass 2^31", r->refine_done, n_samples);
    HIP_TRY(hipSetDevice(r->cfg.device));
    if (!r->accum.p) HIP_TRY(r->accum.alloc_zeroed(n_local_pixels(r->tm) * sizeof(float4)));   // padding pixels of a shard are never written: they read as zeros
    if (!r->refine_ev) HIP_TRY(hipEventCreate(&r->refine_ev));
    if (r->dn_valid) HIP_TRY(hipStreamWaitEvent((hipStream_t)hip_stream, r->dn_ev, 0));   // a filter may still read what this step overwrites
    int rc = enqueue_call(r, hip_stream, d_out, r->refine_done, n_samples, true);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipEventRecord(r->refine_ev, (hipStream_t)hip_stream));
    r->refine_done += n_samples;
    if (r->aov_on) r->aov_done = r->aov_max ? std::min(r->aov_max, r->refine_done) : r->refine_done;
    return RT_OK;
}

extern "C" int rt_renderer_refine(rt_renderer* r, uint32_t n_samples) {
    if (!r) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine: null renderer");
    int rc = rt_renderer_refine_async(r, r->stream, nullptr, n_samples);
    if (rc == RT_OK) rc = wait_last_call(r);
    return rc != RT_OK ? rc : rt_renderer_check_device_flags(r);
}

extern "C" int rt_renderer_refine_reset(rt_renderer* r) {
    if (!r) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_reset: null renderer");
    r->refine_done = 0;   // the next step's first pass starts from zero instead of loading the accumulation
    r->aov_done = 0;
    return RT_OK;
}

extern "C" int rt_renderer_refine_info(rt_renderer* r, uint64_t out[3]) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_info: null argument");
    out[0] = r->refine_done;
    out[1] = r->variant >= 2 ? r->pass_spp : 0u;
    out[2] = r->accum.bytes + r->noise_partials.bytes + r->noise_out.bytes;
    return RT_OK;
}

extern "C" int rt_renderer_refine_download_sums(rt_renderer* r, float* host, size_t n_floats) {
    if (!r || !host) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_download_sums: null argument");
    if (r->cfg.world_size != 1) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_download_sums: renderer holds one shard of %u", r->cfg.world_size);
    const size_t need = (size_t)r->cfg.width * r->cfg.height * 4;
    if (n_floats != need) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_download_sums: buffer holds %zu floats, image needs %zu", n_floats, need);
    if (r->refine_done == 0 || !r->accum.p) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_download_sums: nothing accumulated (refine first)");
    return download_tile_major(r, r->accum, 4u, host);   // the accumulation is tile-major like a shard
}

extern "C" int rt_renderer_refine_noise(rt_renderer* r, double* out) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_noise: null argument");
    if (r->refine_done < 2 || !r->accum.p) return rt_fail(RT_ERR_INVALID, "rt_renderer_refine_noise: a variance needs 2 samples per pixel; %u accumulated", r->refine_done);
    if (const int rc = wait_last_call(r)) return rc;
    const uint32_t n_local = (uint32_t)n_local_pixels(r->tm);
    const uint32_t n_blocks = (n_local + RT_NOISE_BLOCK - 1u) / RT_NOISE_BLOCK;
    if (!r->noise_partials.p) {
        HIP_TRY(r->noise_partials.alloc((size_t)n_blocks * sizeof(NoiseSums)));
        HIP_TRY(r->noise_out.alloc(sizeof(NoiseSums)));
    }
    refine_noise_kernel<<<n_blocks, RT_NOISE_BLOCK, 0, r->stream>>>(r->tm, r->accum.as<float4>(), r->refine_done, r->noise_partials.as<NoiseSums>());
    HIP_TRY(hipGetLastError());
    refine_noise_finish_kernel<<<1, RT_NOISE_BLOCK, 0, r->stream>>>(r->noise_partials.as<NoiseSums>(), n_blocks, r->noise_out.as<NoiseSums>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(r->stream));
    NoiseSums sums = {0.0, 0.0, 0.0};   // over the pixels of this renderer's share of the frame: padding and non-finite pixels left out
    HIP_TRY(hipMemcpy(&sums, r->noise_out.p, sizeof(sums), hipMemcpyDeviceToHost));
    if (sums.pixels == 0.0) { *out = (double)INFINITY; return RT_OK; }
    const double mean_v = sums.v / sums.pixels, mean_m = sums.m / sums.pixels;
    *out = mean_m == 0.0 ? (double)INFINITY : std::sqrt(mean_v) / mean_m;   // a black frame has no relative error: +inf, not an error
    return RT_OK;
}

// ---------------------------------------------------------------------------------------------
// Feature buffers and denoiser (rt06.h; kernels: rt_aov_kernel.hpp)
// ---------------------------------------------------------------------------------------------
// `who` = the entry point the caller used: rt_renderer_aov_enable keeps its messages
static int aov_enable(const char* who, rt_renderer* r, uint32_t max_samples, uint32_t mode) {
    if (!r) return rt_fail(RT_ERR_INVALID, "%s: null renderer", who);
    if (mode > RT_AOV_FULL) return rt_fail(RT_ERR_INVALID, "%s: unknown mode %u (RT_AOV_PLAIN = 0, RT_AOV_TEXTURED = 1, RT_AOV_FULL = 2)", who, mode);
    if (r->variant < 2)
        return rt_fail(RT_ERR_INVALID, "%s: the baseline kernel (variant 1) cannot refine and keeps no primary-ray records; feature buffers need a streaming variant (0, or 2 to 6)", who);
    if (mode == RT_AOV_PLAIN && r->nm.on)
        return rt_fail(RT_ERR_INVALID, "%s: the renderer has a normal-map table, and the plain feature pass's normals know no normal map: enable the pass in RT_AOV_TEXTURED mode (rt_renderer_aov_enable_mode)", who);
    if (r->cut.on && mode != RT_AOV_FULL)   // §35: mode 2 puts its candidates to the rule
        return rt_fail(RT_ERR_INVALID, "%s: the renderer has a cutout table, and the feature pass does not know the cutout rule: its first hits would be the solid cards, and a denoiser guided by them would be wrong without a sign (take the table away with rt_renderer_cutouts(NULL, 0) first)", who);
    if (mode == RT_AOV_PLAIN && r->aov_refused)
        return rt_fail(RT_ERR_INVALID, "%s: the world has %s: the feature pass covers spheres and quads with Lambertian, metal, dielectric, checker and light materials", who, r->aov_refused);
    if (mode == RT_AOV_TEXTURED && r->has_medium)   // §27: a medium's first event is an RNG draw, which no trace of the feature pass makes
        return rt_fail(RT_ERR_INVALID, "%s: the world has a constant medium (RT_MAT_ISOTROPIC): the textured feature pass covers spheres and quads with Lambertian, metal, dielectric, checker, light, noise and image materials", who);
    HIP_TRY(hipSetDevice(r->cfg.device));
    if (!r->aov.p) HIP_TRY(r->aov.alloc_zeroed(n_local_pixels(r->tm) * 2u * sizeof(float4)));   // padding pixels are never written: they read as zeros
    r->aov_on = true;
    r->aov_mode = mode;
    r->aov_max = max_samples;
    r->refine_done = 0;   // like rt_renderer_refine_reset: colour and features restart together
    r->aov_done = 0;
    return RT_OK;
}
extern "C" int rt_renderer_aov_enable(rt_renderer* r, uint32_t max_samples) { return aov_enable("rt_renderer_aov_enable", r, max_samples, RT_AOV_PLAIN); }
extern "C" int rt_renderer_aov_enable_mode(rt_renderer* r, uint32_t max_samples, uint32_t mode) { return aov_enable("rt_renderer_aov_enable_mode", r, max_samples, mode); }

extern "C" int rt_renderer_aov_mode(rt_renderer* r, uint32_t* out_mode) {
    if (!r || !out_mode) return rt_fail(RT_ERR_INVALID, "rt_renderer_aov_mode: null argument");
    *out_mode = r->aov_mode;
    return RT_OK;
}

extern "C" int rt_renderer_aov_info(rt_renderer* r, uint64_t out[3]) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_aov_info: null argument");
    out[0] = r->aov_on ? 1u : 0u;
    out[1] = r->aov_done;
    out[2] = r->aov.bytes;
    return RT_OK;
}

extern "C" int rt_renderer_aov_download(rt_renderer* r, float* host, size_t n_floats) {
    if (!r || !host) return rt_fail(RT_ERR_INVALID, "rt_renderer_aov_download: null argument");
    if (r->cfg.world_size != 1) return rt_fail(RT_ERR_INVALID, "rt_renderer_aov_download: renderer holds one shard of %u", r->cfg.world_size);
    const size_t need = (size_t)r->cfg.width * r->cfg.height * 8;
    if (n_floats != need) return rt_fail(RT_ERR_INVALID, "rt_renderer_aov_download: buffer holds %zu floats, the feature buffers need %zu", n_floats, need);
    if (!r->aov_on || r->aov_done == 0) return rt_fail(RT_ERR_INVALID, "rt_renderer_aov_download: no feature samples (rt_renderer_aov_enable, then refine)");
    return download_tile_major(r, r->aov, 8u, host);
}

extern "C" int rt_renderer_denoise_async(rt_renderer* r, void* hip_stream, const rt_denoise_params* params) {
    if (!r || !params) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise: null argument");
    if (r->cfg.world_size != 1) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise: renderer holds one shard of %u; the filter needs the whole frame", r->cfg.world_size);
    if (params->iterations < 1 || params->iterations > 8) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise: iterations must be 1..8, not %u", params->iterations);
    if (!(params->sigma_depth > 0.0f) || !(params->sigma_lum > 0.0f) || !std::isfinite(params->sigma_depth) || !std::isfinite(params->sigma_lum))
        return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise: sigma_depth and sigma_lum must be finite and > 0");
    if (params->demodulate > 1) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise: demodulate must be 0 or 1");
    if (!r->aov_on || r->aov_done == 0) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise: no feature buffers (rt_renderer_aov_enable, then refine)");
    if (r->refine_done < 2 || !r->accum.p) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise: a variance needs 2 samples per pixel; %u accumulated", r->refine_done);
    HIP_TRY(hipSetDevice(r->cfg.device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint32_t n_px = r->cfg.width * r->cfg.height;
    if (!r->dn_ev) HIP_TRY(hipEventCreate(&r->dn_ev));
    for (DevBuf* b : {&r->dn_g0, &r->dn_g1, &r->dn_a, &r->dn_b, &r->dn_out})   // each at its first use: a call that failed half-way is simply continued
        if (!b->p) HIP_TRY(b->alloc((size_t)n_px * sizeof(float4)));
    HIP_TRY(hipStreamWaitEvent(st, r->refine_ev, 0));                   // the last refine step may have run on another stream
    if (r->dn_valid) HIP_TRY(hipStreamWaitEvent(st, r->dn_ev, 0));     // ... and so may the last filter, whose buffers this one reuses
    DenoiseParams dp;
    dp.width = r->cfg.width; dp.height = r->cfg.height;
    dp.sigma_depth = params->sigma_depth; dp.sigma_lum = params->sigma_lum; dp.demodulate = params->demodulate;
    const uint32_t n_local = (uint32_t)n_local_pixels(r->tm);
    float4 *src = r->dn_a.as<float4>(), *dst = r->dn_b.as<float4>();
    denoise_prepare_kernel<<<(n_local + 255u) / 256u, 256, 0, st>>>(r->tm, dp, r->accum.as<float4>(), r->aov.as<float4>(), r->refine_done, r->aov_done,
                                                                    r->dn_g0.as<float4>(), r->dn_g1.as<float4>(), src);
    HIP_TRY(hipGetLastError());
    const dim3 grid((dp.width + RT_DN_TILE - 1u) / RT_DN_TILE, (dp.height + RT_DN_TILE - 1u) / RT_DN_TILE), block(RT_DN_TILE * RT_DN_TILE);
    for (uint32_t i = 0; i < params->iterations; i++) {
        if (i == 0) denoise_filter_tile_kernel<1><<<grid, block, 0, st>>>(dp, r->dn_g0.as<float4>(), src, dst);
        else if (i == 1) denoise_filter_tile_kernel<2><<<grid, block, 0, st>>>(dp, r->dn_g0.as<float4>(), src, dst);
        else denoise_filter_direct_kernel<<<grid, block, 0, st>>>(dp, 1 << i, r->dn_g0.as<float4>(), src, dst);
        HIP_TRY(hipGetLastError());
        std::swap(src, dst);
    }
    denoise_final_kernel<<<(n_px + 255u) / 256u, 256, 0, st>>>(dp, r->dn_g1.as<float4>(), src, r->dn_out.as<float4>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->dn_ev, st));
    r->dn_valid = true;
    return RT_OK;
}

extern "C" int rt_renderer_denoise(rt_renderer* r, const rt_denoise_params* params) {
    if (!r || !params) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise: null argument");
    int rc = rt_renderer_denoise_async(r, r->stream, params);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(r->stream));
    return RT_OK;
}

extern "C" int rt_renderer_denoise_download(rt_renderer* r, float* host_rgba, size_t n_floats) {
    if (!r || !host_rgba) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise_download: null argument");
    const size_t need = (size_t)r->cfg.width * r->cfg.height * 4;
    if (n_floats != need) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise_download: buffer holds %zu floats, image needs %zu", n_floats, need);
    if (!r->dn_valid) return rt_fail(RT_ERR_INVALID, "rt_renderer_denoise_download: nothing denoised yet (rt_renderer_denoise first)");
    HIP_TRY(hipSetDevice(r->cfg.device));
    HIP_TRY(hipEventSynchronize(r->dn_ev));
    HIP_TRY(hipMemcpy(host_rgba, r->dn_out.p, need * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_renderer_render(rt_renderer* r) {
    if (!r) return rt_fail(RT_ERR_INVALID, "rt_renderer_render: null renderer");
    int rc = enqueue_call(r, r->stream, nullptr, 0u, r->cfg.samples_per_pixel, false);   // serial: the host waits below, there is nothing to run ahead of
    if (rc == RT_OK) rc = wait_last_call(r);
    return rc != RT_OK ? rc : rt_renderer_check_device_flags(r);
}

extern "C" int rt_renderer_last_kernel_ms(rt_renderer* r, float* out_ms) {
    if (!r || !out_ms) return rt_fail(RT_ERR_INVALID, "rt_renderer_last_kernel_ms: null argument");
    if (!r->timed) return rt_fail(RT_ERR_INVALID, "rt_renderer_last_kernel_ms: nothing rendered yet");
    HIP_TRY(hipSetDevice(r->cfg.device));
    HIP_TRY(hipEventSynchronize(r->ev1));
    HIP_TRY(hipEventElapsedTime(out_ms, r->ev0, r->ev1));
    return RT_OK;
}

extern "C" int rt_renderer_kernel_times(rt_renderer* r, uint32_t renders_back, float out_ms[3]) {
    if (!r || !out_ms) return rt_fail(RT_ERR_INVALID, "rt_renderer_kernel_times: null argument");
    if (r->variant < 2) return rt_fail(RT_ERR_INVALID, "rt_renderer_kernel_times: the baseline kernel (variant 1) is one launch; use rt_renderer_last_kernel_ms");
    if (renders_back >= rt_renderer::RT_TIMES_RING || renders_back >= r->n_renders)
        return rt_fail(RT_ERR_INVALID, "rt_renderer_kernel_times: render %u calls back is not recorded (%llu rendered, ring of %u)", renders_back,
                       (unsigned long long)r->n_renders, rt_renderer::RT_TIMES_RING);
    HIP_TRY(hipSetDevice(r->cfg.device));
    const uint64_t slot = (r->n_renders - 1 - renders_back) % rt_renderer::RT_TIMES_RING;
    const std::vector<hipEvent_t>& ring = r->kev[slot];
    const uint32_t call_passes = r->kev_passes[slot];   // of THAT call: a refine step has a pass count of its own
    HIP_TRY(hipEventSynchronize(ring[(size_t)call_passes * 4u - 1u]));
    for (int k = 0; k < 3; k++) out_ms[k] = 0.0f;
    for (uint32_t pass = 0; pass < call_passes; pass++)   // a call is that many launches of each kernel: the SUM is the call's time in it
        for (int k = 0; k < 3; k++) {
            float ms = 0.0f;
            // (a call that ran ahead is one pass; its resolve starts behind the wait for its tracer, at an event of its own)
            HIP_TRY(hipEventElapsedTime(&ms, k == 2 && r->kev_ahead[slot] ? r->kev_resolve0[slot] : ring[pass * 4u + k], ring[pass * 4u + k + 1]));
            out_ms[k] += ms;
        }
    return RT_OK;
}

extern "C" int rt_renderer_run_ahead_info(rt_renderer* r, uint64_t out[4]) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_run_ahead_info: null argument");
    out[0] = r->n_slots;
    out[1] = r->n_ahead;
    out[2] = r->n_overlapped;
    out[3] = r->slot[1].samples.bytes + r->slot[1].primary.bytes;
    return RT_OK;
}

extern "C" int rt_renderer_pass_info(rt_renderer* r, uint64_t out[4]) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_pass_info: null argument");
    out[0] = r->variant >= 2 ? r->n_passes : 1u;
    out[1] = r->variant >= 2 ? r->pass_spp : r->cfg.samples_per_pixel;
    out[2] = r->variant >= 2 ? rt_renderer::SAMPLE_BYTES + rt_renderer::PRIMARY_BYTES : 0u;
    out[3] = r->slot[0].samples.bytes + r->slot[0].primary.bytes + r->running.bytes;   // of one slot: what a call's passes use (the second set: rt_renderer_run_ahead_info)
    return RT_OK;
}

extern "C" int rt_renderer_kernel_info(rt_renderer* r, uint32_t out[4]) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_kernel_info: null argument");
    out[0] = r->tol ? 6u : r->variant;
    out[1] = (r->variant >= 2 && !r->scene.big) ? 1u : 0u;
    out[2] = r->variant >= 2 ? r->stream_block : 64u;
    out[3] = r->variant >= 2 ? r->stream_blocks_per_cu : 0u;
    return RT_OK;
}

extern "C" int rt_renderer_kernel_form(rt_renderer* r, uint32_t out[9]) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_kernel_form: null argument");
    for (int i = 0; i < 9; i++) out[i] = 0u;
    if (r->variant < 2) { out[0] = RT_KERNEL_BASELINE; return RT_OK; }
    // the key launch() resolves: plan()'s for the plain kernel, rt_renderer_light_sampling_enable's while sampling is on
    const rt_renderer::LaunchOn on = r->launch_on(r->nee.mode);
    const uint32_t key = on.key;
    if (stream_kernel_for(key) != on.kernel) return rt_fail(RT_ERR_INVALID, "rt_renderer_kernel_form: the key does not name the kernel the renderer holds");
    if (key == RT_KEY_XCHG) { out[0] = RT_KERNEL_XCHG; return RT_OK; }
    out[0] = RT_KERNEL_STREAM;
    stream_key_fields(key, out + 1);
    return RT_OK;
}

// Whether the NEXT launch runs an instantiation whose key has `bit`: queries of their own, so that rt_renderer_kernel_form's nine outputs stay what they are.
// (The baseline kernel has no key; no plain key has a family's bit.)
static int kernel_has(const char* api, rt_renderer* r, uint32_t* out, uint32_t bit) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "%s: null argument", api);
    *out = r->variant >= 2 && (r->launch_on(r->nee.mode).key & bit) ? 1u : 0u;
    return RT_OK;
}
extern "C" int rt_renderer_kernel_triangles(rt_renderer* r, uint32_t* out) { return kernel_has("rt_renderer_kernel_triangles", r, out, RT_KEY_TRI); }         // §18
extern "C" int rt_renderer_kernel_light_tree(rt_renderer* r, uint32_t* out) { return kernel_has("rt_renderer_kernel_light_tree", r, out, RT_KEY_LTREE); }     // §20
extern "C" int rt_renderer_kernel_env_light(rt_renderer* r, uint32_t* out) { return kernel_has("rt_renderer_kernel_env_light", r, out, RT_KEY_ENVL); }        // §24
// the rungs of FORM_LADDER: a form says 1 to its own query and to that of every bit its key carries (a cutout form is a solid-glass and a microfacet form too;
// none of them carries RT_KEY_NMAP, though all read the normal-map table)
extern "C" int rt_renderer_kernel_normal_map(rt_renderer* r, uint32_t* out) { return kernel_has("rt_renderer_kernel_normal_map", r, out, RT_KEY_NMAP); }     // §28
extern "C" int rt_renderer_kernel_microfacet(rt_renderer* r, uint32_t* out) { return kernel_has("rt_renderer_kernel_microfacet", r, out, RT_KEY_MFAC); }      // §29
extern "C" int rt_renderer_kernel_interior(rt_renderer* r, uint32_t* out) { return kernel_has("rt_renderer_kernel_interior", r, out, RT_KEY_INTR); }          // §32
extern "C" int rt_renderer_kernel_cutout(rt_renderer* r, uint32_t* out) { return kernel_has("rt_renderer_kernel_cutout", r, out, RT_KEY_CUT); }               // §34

extern "C" int rt_renderer_download(rt_renderer* r, float* host_rgba, size_t n_floats) {
    if (!r || !host_rgba) return rt_fail(RT_ERR_INVALID, "rt_renderer_download: null argument");
    if (r->cfg.world_size != 1) return rt_fail(RT_ERR_INVALID, "rt_renderer_download: renderer holds one shard of %u; gather and rt_renderer_assemble first", r->cfg.world_size);
    size_t need = (size_t)r->cfg.width * r->cfg.height * 4;
    if (n_floats != need) return rt_fail(RT_ERR_INVALID, "rt_renderer_download: buffer holds %zu floats, image needs %zu", n_floats, need);
    if (const int rc = wait_last_call(r)) return rc;
    HIP_TRY(hipMemcpy(host_rgba, r->fb.p, need * sizeof(float), hipMemcpyDeviceToHost));
    return rt_renderer_check_device_flags(r);
}

extern "C" int rt_renderer_shard_floats(const rt_renderer* r, size_t* out) {
    if (!r || !out) return rt_fail(RT_ERR_INVALID, "rt_renderer_shard_floats: null argument");
    *out = n_local_pixels(r->tm) * 4;
    return RT_OK;
}

// de-interleave the gathered shards (rank-major, tile-major inside a shard) into the row-major image
__global__ void assemble_kernel(const float4* __restrict__ gathered, float4* __restrict__ image, TileMap tm, uint32_t shard_pixels) {
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= tm.width * tm.height) return;
    uint32_t x = gid % tm.width, y = gid / tm.width;
    uint32_t gt = (y / RT_TILE) * tm.tiles_x + (x / RT_TILE);
    uint32_t rank = gt % tm.world_size, tl = gt / tm.world_size;
    uint32_t p = (y % RT_TILE) * RT_TILE + (x % RT_TILE);
    image[gid] = gathered[(size_t)rank * shard_pixels + (size_t)tl * (RT_TILE * RT_TILE) + p];
}

extern "C" int rt_renderer_assemble(rt_renderer* r, const float* d_gathered, float* d_image, void* hip_stream) {
    if (!r || !d_gathered || !d_image) return rt_fail(RT_ERR_INVALID, "rt_renderer_assemble: null argument");
    HIP_TRY(hipSetDevice(r->cfg.device));
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t n = r->cfg.width * r->cfg.height;
    assemble_kernel<<<(n + 255) / 256, 256, 0, st>>>((const float4*)d_gathered, (float4*)d_image, r->tm, (uint32_t)n_local_pixels(r->tm));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

hipStream_t rt_renderer_own_stream(rt_renderer* r) { return r->stream; }
float* rt_renderer_own_framebuffer(rt_renderer* r) { return r->fb.as<float>(); }
void rt_renderer_one_slot(rt_renderer* r) { r->drop_second_slot(); }

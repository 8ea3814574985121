// rt_probes.hip — rt_probe_* (one hot-path function per call over arrays: the parity tests' entry points) and rt_selftest_* (exhaustive checks of
// the exact-division building blocks).  Test entry points of the C ABI; nothing here is on the render path.
#include "rt_runtime.hpp"
#include "rt_fastdiv.hpp"
#include <deque>

// ---------------------------------------------------------------------------------------------
// probes
// ---------------------------------------------------------------------------------------------
__global__ void probe_aabb_kernel(size_t n, const float* boxes, const float* rays, const float* maxd, int32_t* hit, float* dist) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = ld3(rays + 6 * i); r.d = ld3(rays + 6 * i + 3); r.time = 0.0f;
    float d = 0.0f;
    hit[i] = aabb_intersects(ld3(boxes + 6 * i), ld3(boxes + 6 * i + 3), r, maxd[i], d) ? 1 : 0;
    dist[i] = d;
}
__global__ void probe_sphere_kernel(size_t n, const float* rays, const float* spheres, float* out_t) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = ld3(rays + 6 * i); r.d = ld3(rays + 6 * i + 3); r.time = 0.0f;
    out_t[i] = sphere_closest_intersection(r, ld3(spheres + 4 * i), spheres[4 * i + 3]);
}
__global__ void probe_trace_kernel(DeviceWorld w, size_t n, const float* rays, int32_t* hit, float* t, int32_t* prim, float* normal) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = ld3(rays + 7 * i); r.d = ld3(rays + 7 * i + 3); r.time = rays[7 * i + 6];
    HitRec rec;
    rec.distance = RT_MISS_DIST; rec.normal = mk3(0.0f); rec.prim = -1; rec.mat = 0;
    Rng g;
    g.init(0u, (uint32_t)i, 0u, 0x7ACEu);  // only a constant medium draws from it (same key as the oracle's probe)
    hit[i] = world_closest_intersection(w, r, rec, &g) ? 1 : 0;
    t[i] = rec.distance; prim[i] = rec.prim;
    st3(normal + 3 * i, rec.normal);
}
// the world's own walk, then the smooth-shading rule (shading_normal) on a triangle hit: vn = one record per triangle, or null
__global__ void probe_shading_normal_kernel(DeviceWorld w, const rt_tri_normals* vn, uint32_t first_tri, size_t n, const float* rays, int32_t* hit, float* normal, uint32_t* interpolated) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = ld3(rays + 7 * i); r.d = ld3(rays + 7 * i + 3); r.time = rays[7 * i + 6];
    HitRec rec;
    rec.distance = RT_MISS_DIST; rec.normal = mk3(0.0f); rec.prim = -1; rec.mat = 0;
    Rng g;
    g.init(0u, (uint32_t)i, 0u, 0x7ACEu);
    const bool h = world_closest_intersection(w, r, rec, &g);
    bool took = false;
    if (h && vn && (uint32_t)rec.prim >= first_tri) took = shading_normal_flat(w.quads[(uint32_t)rec.prim - w.n_prims], vn[(uint32_t)rec.prim - first_tri], r, rec.distance, rec.normal);
    hit[i] = h ? 1 : 0;
    interpolated[i] = took ? 1u : 0u;
    st3(normal + 3 * i, rec.normal);
}
// the world's own walk, then the texture-coordinate rule (tri_uv) on a triangle hit: uv = one record per triangle, or null = the identity on each;
// a parallelogram keeps its planar coordinates, whatever the table says
__global__ void probe_tri_uv_kernel(DeviceWorld w, const rt_tri_uvs* uv, uint32_t first_tri, size_t n, const float* rays, int32_t* hit, float* out_uv) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = ld3(rays + 7 * i); r.d = ld3(rays + 7 * i + 3); r.time = rays[7 * i + 6];
    HitRec rec;
    rec.distance = RT_MISS_DIST; rec.normal = mk3(0.0f); rec.prim = -1; rec.mat = 0;
    Rng g;
    g.init(0u, (uint32_t)i, 0u, 0x7ACEu);
    const bool h = world_closest_intersection(w, r, rec, &g);
    float tu = 0.0f, tv = 0.0f;
    if (h && (uint32_t)rec.prim >= w.n_prims) {
        const rt_quad& q = w.quads[(uint32_t)rec.prim - w.n_prims];
        const f3 hit_p = ray_at(r, rec.distance);
        if (uv && (uint32_t)rec.prim >= first_tri) {
            const rt_tri_uvs& t = uv[(uint32_t)rec.prim - first_tri];
            tri_uv(ld3(q.Q), ld3(q.u), ld3(q.v), ld3(q.w), t.t0, t.t1, t.t2, hit_p, tu, tv);
        } else {   // image_value_quad's coordinates
            const f3 planar = hit_p - ld3(q.Q);
            tu = dot(ld3(q.w), cross(planar, ld3(q.v)));
            tv = dot(ld3(q.w), cross(ld3(q.u), planar));
        }
    }
    hit[i] = h ? 1 : 0;
    out_uv[2 * i] = tu; out_uv[2 * i + 1] = tv;
}
// the environment rule (environment_value), one lane per direction, on the map as the renderer holds it: one float4 per texel
__global__ void probe_environment_kernel(size_t n, const float4* texels, uint32_t width, uint32_t height, float u0, const float* dirs, float* out_rgb, uint32_t* out_texel) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 d = ld3(dirs + 3 * i);
    out_texel[i] = environment_texel_index(width, height, u0, d);
    st3(out_rgb + 3 * i, environment_value(texels, width, height, u0, d));
}
// the texture rule (texture_value), one lane per lookup, on the table as the renderer holds it; the host has checked every index
__global__ void probe_texture_kernel(size_t n, const uint32_t* texels, const uint4* entries, const uint32_t* index, const float* u, const float* v, float* out_rgb) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st3(out_rgb + 3 * i, texture_value(texels, entries[index[i]], u[i], v[i]));
}
// the normal-map rule (normal_map_apply and the tangents) on one case: what rt_normal_map_batch runs on the host and the probe one lane each
RT_HD uint32_t normal_map_case(const uint32_t* texels, uint4 entry, uint32_t surface, f3 a, f3 b, const float* t, f3 ray_d, float u, float v, float strength, f3& normal) {
    f3 dPdu = a, dPdv = b;
    if (surface == RT_NMAP_SURFACE_SPHERE) normal_map_sphere_tangents(a, dPdu, dPdv);
    else if (surface == RT_NMAP_SURFACE_TRI_UV && !normal_map_tri_tangents(a, b, t, t + 2, t + 4, dPdu, dPdv)) return RT_NMAP_NO_FRAME;
    return normal_map_apply(texture_value(texels, entry, u, v), strength, dPdu, dPdv, ray_d, normal);
}
__global__ void probe_normal_map_kernel(size_t n, const uint32_t* texels, const uint4* entries, const uint32_t* surface, const float* a, const float* b, const float* tri_uv,
                                        const float* normal, const float* ray_d, const float* u, const float* v, const uint32_t* index, const float* strength,
                                        float* out_normal, uint32_t* out_path) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f3 nn = ld3(normal + 3 * i);
    out_path[i] = normal_map_case(texels, entries[index[i]], surface[i], ld3(a + 3 * i), ld3(b + 3 * i), tri_uv ? tri_uv + 6 * i : nullptr, ld3(ray_d + 3 * i), u[i], v[i],
                                  strength[i], nn);
    st3(out_normal + 3 * i, nn);
}
__global__ void probe_noise_value_kernel(size_t n, const rt_perlin* perlin, f3 albedo, float scale, const float* points, float* out_rgb) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st3(out_rgb + 3 * i, noise_value(perlin, albedo, scale, ld3(points + 3 * i)));
}
// SphereHittable / MovingSphereHittable::ClosestIntersection on one sphere per ray, rec.distance preset by the caller: the leaf
// test every traversal calls (prim_closest_intersection), as a plain sphere (material 0 = a Lambertian, the moving bit kept)
__global__ void probe_sphere_hit_kernel(size_t n, const rt_prim* prims, const rt_material* mat, const float* rays, const float* preset,
                                        int32_t* hit, float* dist, float* normal) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = ld3(rays + 7 * i); r.d = ld3(rays + 7 * i + 3); r.time = rays[7 * i + 6];
    HitRec rec;
    rec.distance = preset[i]; rec.normal = mk3(0.0f); rec.prim = -1; rec.mat = 0;
    rt_prim p = prims[i];
    p.mat &= RT_PRIM_MOVING;
    Rng g;
    g.init(0u, (uint32_t)i, 0u, 0x7ACEu);   // not drawn from: a Lambertian sphere is no constant medium
    hit[i] = prim_closest_intersection(p, (int32_t)i, r, rec, mat, &g) ? 1 : 0;
    dist[i] = rec.distance;
    st3(normal + 3 * i, rec.normal);
}
// A tape of k in [1, 2^24] in place of Rng: u = k * 2^-24 (next) and (k - 2^23) * 2^-23 (next_signed), the two forms Rng returns
// for its word (rt_math.hpp).  Reaches the edges of measure zero under the generator's stream (k = 2^23 three times, |v| == 1, ...).
// Past the end of its tape it serves k = 2^23 + 1, which every rejection loop accepts (no hang), and keeps counting: draws > the
// tape's length reports the overrun.
struct TapeRng {
    const uint32_t* k;
    uint32_t n, draws;
    RT_HD uint32_t take() { const uint32_t v = draws < n ? k[draws] : 0x800001u; draws++; return v; }
    RT_HD float next() { return (float)take() * 5.9604644775390625e-08f; }
    RT_HD float next_signed() { return (float)(int32_t)(take() - 0x800000u) * 1.1920928955078125e-07f; }
};
// How the generator of case i is made: a seeded Rng from (pixel, sample) keys, or a TapeRng from a tape and (offset, length) pairs
struct KeyedRng {
    uint64_t seed;
    const uint32_t* keys;
    __device__ Rng operator()(size_t i) const { Rng g; g.init(seed, keys[2 * i], keys[2 * i + 1], RT_STREAM_RENDER); return g; }
};
struct TapedRng {
    const uint32_t *tape, *offsets;
    __device__ TapeRng operator()(size_t i) const { return TapeRng{tape + offsets[2 * i], offsets[2 * i + 1], 0u}; }
};
template <typename MakeRng>
__global__ void probe_scatter_kernel(MakeRng make_rng, size_t n, const rt_material* mats, const float* rays, const float* dist,
                                     const float* normals, int32_t* scattered, float* out_rays, float* atten, uint32_t* draws) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray in;
    in.o = ld3(rays + 7 * i); in.d = ld3(rays + 7 * i + 3); in.time = rays[7 * i + 6];
    HitRec rec;
    rec.distance = dist[i]; rec.normal = ld3(normals + 3 * i); rec.prim = 0; rec.mat = 0;
    auto g = make_rng(i);
    Ray out;
    out.o = mk3(0.0f); out.d = mk3(0.0f); out.time = 0.0f;
    f3 att = mk3(0.0f);
    scattered[i] = material_scatter(mats[i], in, rec, g, out, att) ? 1 : 0;
    st3(out_rays + 7 * i, out.o); st3(out_rays + 7 * i + 3, out.d); out_rays[7 * i + 6] = out.time;
    st3(atten + 3 * i, att);
    draws[i] = g.draws;
}
template <typename MakeRng>
__global__ void probe_camera_kernel(MakeRng make_rng, rt_camera cam, size_t n, const float* st, float* out_rays, uint32_t* draws) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto g = make_rng(i);
    Ray r = camera_sample_ray(cam, st[2 * i], st[2 * i + 1], g);
    st3(out_rays + 7 * i, r.o); st3(out_rays + 7 * i + 3, r.d); out_rays[7 * i + 6] = r.time;
    draws[i] = g.draws;
}
// the camera's rule on one case with its tape: what rt_camera_rays_batch runs on the host (any type) and rt_probe_camera_lens one lane each (a lens camera)
RT_HD void camera_rays_case(const rt_camera& cam, size_t i, const float* st, const uint32_t* tape, const uint32_t* offsets, float* out_rays, uint32_t* out_draws) {
    TapeRng g{tape + offsets[2 * i], offsets[2 * i + 1], 0u};
    const Ray r = cam.type >= RT_CAM_PERSPECTIVE ? lens_camera_sample_ray(cam, st[2 * i], st[2 * i + 1], g) : camera_sample_ray(cam, st[2 * i], st[2 * i + 1], g);
    st3(out_rays + 7 * i, r.o); st3(out_rays + 7 * i + 3, r.d); out_rays[7 * i + 6] = r.time;
    out_draws[i] = g.draws;
}
__global__ void probe_camera_lens_kernel(rt_camera cam, size_t n, const float* st, const uint32_t* tape, const uint32_t* offsets, float* out_rays, uint32_t* out_draws) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    camera_rays_case(cam, i, st, tape, offsets, out_rays, out_draws);
}
// the microfacet rule (microfacet_scatter) on one case with its tape: what rt_microfacet_batch runs on the host and the probe one lane each
RT_HD void microfacet_case(size_t i, const float* normal, const float* ray_d, const float* roughness, const float* f0, const uint32_t* coat, const uint32_t* tape,
                           const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    TapeRng g{tape + offsets[2 * i], offsets[2 * i + 1], 0u};
    f3 dir = mk3(0.0f), weight = mk3(0.0f);
    const bool is_coat = coat[i] != 0u;
    out_path[i] = microfacet_scatter(ld3(normal + 3 * i), ld3(ray_d + 3 * i), roughness[i], is_coat ? mk3(f0[3 * i]) : ld3(f0 + 3 * i), is_coat, g, dir, weight);
    st3(out_dir + 3 * i, dir); st3(out_weight + 3 * i, weight);
    out_draws[i] = g.draws;
}
__global__ void probe_microfacet_kernel(size_t n, const float* normal, const float* ray_d, const float* roughness, const float* f0, const uint32_t* coat,
                                        const uint32_t* tape, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    microfacet_case(i, normal, ray_d, roughness, f0, coat, tape, offsets, out_dir, out_weight, out_path, out_draws);
}
// the rough-glass rule (rough_glass_scatter) on one case with its tape, likewise
RT_HD void rough_glass_case(size_t i, const float* normal, const float* ray_d, const float* roughness, const float* ior, const uint32_t* tape, const uint32_t* offsets,
                            float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    TapeRng g{tape + offsets[2 * i], offsets[2 * i + 1], 0u};
    f3 dir = mk3(0.0f);
    float weight = 0.0f;
    out_path[i] = rough_glass_scatter(ld3(normal + 3 * i), ld3(ray_d + 3 * i), roughness[i], ior[i], g, dir, weight);
    st3(out_dir + 3 * i, dir); out_weight[i] = weight;
    out_draws[i] = g.draws;
}
__global__ void probe_rough_glass_kernel(size_t n, const float* normal, const float* ray_d, const float* roughness, const float* ior, const uint32_t* tape,
                                         const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rough_glass_case(i, normal, ray_d, roughness, ior, tape, offsets, out_dir, out_weight, out_path, out_draws);
}
__global__ void probe_radiance_kernel(DeviceWorld w, rt_camera cam, uint32_t width, uint32_t height, uint32_t max_depth,
                                      uint64_t seed, size_t n, const uint32_t* keys, float* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f3 rad = one_sample(w, cam, width, height, max_depth, seed, keys[2 * i], keys[2 * i + 1]);
    st3(out + 3 * i, rad);
}
// The reference's one gtest computes, per pixel, the index of the nearest sphere by brute force (google_testing/test.cpp:112-135,
// host twin :87-106).  Here: one work-item per pixel of a flat index space, the sphere table staged through the LDS in slabs of
// 256 so that the 64 lanes of a wave read each sphere as a broadcast; NDC = i / (extent - 1) * 2 - 1 is that test's convention
// (test.cpp:118-119), not the renderer's pixel-centre one.
__global__ __launch_bounds__(256) void probe_sphere_index_kernel(const float4* __restrict__ spheres, uint32_t n_spheres, rt_camera cam,
                                                                 uint32_t width, uint32_t height, int32_t* __restrict__ nearest) {
    __shared__ float4 slab[256];
    const uint32_t pixel = blockIdx.x * 256u + threadIdx.x;
    const bool live = pixel < width * height;
    const uint32_t px = live ? pixel % width : 0u, py = live ? pixel / width : 0u;
    Ray ray;
    ray.o = mk3(cam.o[0], cam.o[1], cam.o[2]);
    const float s = (float)px / ((float)width - 1.0f) * 2 - 1, t = (float)py / ((float)height - 1.0f) * 2 - 1;
    ray.d = mk3(cam.w[0], cam.w[1], cam.w[2]) + mk3(cam.u[0], cam.u[1], cam.u[2]) * s + mk3(cam.v[0], cam.v[1], cam.v[2]) * t;
    ray.time = 0.0f;
    float nearest_t = RT_MISS_DIST;
    int32_t winner = -1;
    for (uint32_t base = 0; base < n_spheres; base += 256u) {
        const uint32_t count = min(256u, n_spheres - base);
        __syncthreads();
        if (threadIdx.x < count) slab[threadIdx.x] = spheres[base + threadIdx.x];
        __syncthreads();
        for (uint32_t k = 0; k < count; k++) {
            const float4 sp = slab[k];
            const float tk = sphere_closest_intersection(ray, mk3(sp.x, sp.y, sp.z), sp.w);
            if (tk < nearest_t) { nearest_t = tk; winner = (int32_t)(base + k); }   // strict: the first of equal distances wins
        }
    }
    if (live) nearest[pixel] = winner;
}
__global__ void probe_rng_kernel(uint64_t seed, size_t n, const uint32_t* keys, uint32_t n_draws, float* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng g;
    g.init(seed, keys[2 * i], keys[2 * i + 1], RT_STREAM_RENDER);
    for (uint32_t k = 0; k < n_draws; k++) out[i * n_draws + k] = g.next();
}
// ---------------------------------------------------------------------------------------------
// The host side of one probe call: selects the device and owns the call's device buffers.  in() uploads a typed host array, out()
// allocates a device array (cleared on request) and registers its download; finish() takes the launch's error, synchronises, then
// downloads in the order of registration.  Counts are ELEMENTS of the pointer's type, so every array states its stride once
// (7 * n floats: n rays with a time).  The first failure sticks: the steps after it, launch() included, do nothing and finish()
// returns its code.  Everything runs on the null stream.
// ---------------------------------------------------------------------------------------------
struct ProbeRun {
    struct Download { void* host; const DevBuf* dev; };
    std::deque<DevBuf> bufs;   // (a deque: a buffer stays where it was made)
    std::vector<Download> downloads;
    int rc;

    explicit ProbeRun(int device) : rc(select_device(device)) {}
    bool ok() const { return rc == RT_OK; }
    void step(hipError_t e, const char* what) {
        if (e != hipSuccess) rc = rt_fail(RT_ERR_HIP, "probe: %s failed: %s", what, hipGetErrorString(e));
    }
    template <typename T> const T* in(const T* host, size_t count) {
        if (!ok()) return nullptr;
        step(bufs.emplace_back().upload(host, count * sizeof(T)), "upload");
        return bufs.back().as<T>();
    }
    template <typename T> T* out(T* host, size_t count, bool cleared = false) {
        if (!ok()) return nullptr;
        DevBuf& b = bufs.emplace_back();
        step(cleared ? b.alloc_zeroed(count * sizeof(T)) : b.alloc(count * sizeof(T)), "allocation");
        downloads.push_back({host, &b});
        return b.as<T>();
    }
    static dim3 per_case(size_t n) { return dim3((unsigned)((n + 127) / 128)); }   // blocks of 128 threads, one thread per case
    template <typename... P, typename... A> void launch(void (*kernel)(P...), dim3 grid, unsigned block, A... args) {
        if (ok()) kernel<<<grid, dim3(block)>>>(args...);
    }
    int finish() {
        if (ok()) step(hipGetLastError(), "launch");
        if (ok()) step(hipDeviceSynchronize(), "kernel");
        for (const Download& d : downloads)
            if (ok()) step(hipMemcpy(d.host, d.dev->p, d.dev->bytes, hipMemcpyDeviceToHost), "download");
        return rc;
    }
};

extern "C" int rt_probe_aabb(int device, size_t n, const float* boxes, const float* rays, const float* max_dist, int32_t* out_hit, float* out_dist) {
    if (!boxes || !rays || !max_dist || !out_hit || !out_dist) return rt_fail(RT_ERR_INVALID, "rt_probe_aabb: null argument");
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    auto b = p.in(boxes, 6 * n); auto r = p.in(rays, 6 * n); auto m = p.in(max_dist, n);
    auto h = p.out(out_hit, n); auto d = p.out(out_dist, n);
    p.launch(probe_aabb_kernel, p.per_case(n), 128, n, b, r, m, h, d);
    return p.finish();
}
extern "C" int rt_probe_sphere(int device, size_t n, const float* rays, const float* spheres, float* out_t) {
    if (!rays || !spheres || !out_t) return rt_fail(RT_ERR_INVALID, "rt_probe_sphere: null argument");
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    auto r = p.in(rays, 6 * n); auto s = p.in(spheres, 4 * n);
    auto t = p.out(out_t, n);
    p.launch(probe_sphere_kernel, p.per_case(n), 128, n, r, s, t);
    return p.finish();
}
extern "C" int rt_probe_trace(int device, const rt_world_flat* world, size_t n, const float* rays, int32_t* out_hit, float* out_t,
                              int32_t* out_prim, float* out_normal) {
    if (!rays || !out_hit || !out_t || !out_prim || !out_normal) return rt_fail(RT_ERR_INVALID, "rt_probe_trace: null argument");
    ProbeRun p(device);
    DeviceScene sc;
    if (p.ok()) p.rc = sc.upload(world);
    if (!p.ok() || n == 0) return p.rc;
    auto r = p.in(rays, 7 * n);
    auto h = p.out(out_hit, n); auto t = p.out(out_t, n); auto pr = p.out(out_prim, n); auto nn = p.out(out_normal, 3 * n);
    p.launch(probe_trace_kernel, p.per_case(n), 128, sc.dw, n, r, h, t, pr, nn);
    return p.finish() != RT_OK ? p.rc : check_traversal_overflow(sc);
}
extern "C" int rt_probe_shading_normal(int device, const rt_world_flat* world, const rt_tri_normals* table, uint32_t n_table, size_t n, const float* rays,
                                       int32_t* out_hit, float* out_normal, uint32_t* out_interpolated) {
    if (!rays || !out_hit || !out_normal || !out_interpolated) return rt_fail(RT_ERR_INVALID, "rt_probe_shading_normal: null argument");
    if ((table == nullptr) != (n_table == 0u)) return rt_fail(RT_ERR_INVALID, "rt_probe_shading_normal: a table and its count go together");
    ProbeRun p(device);
    DeviceScene sc;
    if (p.ok()) p.rc = sc.upload(world);
    if (p.ok() && n_table && n_table != sc.n_triangles) p.rc = rt_fail(RT_ERR_INVALID, "rt_probe_shading_normal: %u records for a world of %u triangles", n_table, sc.n_triangles);
    if (!p.ok() || n == 0) return p.rc;
    auto r = p.in(rays, 7 * n);
    const rt_tri_normals* vn = n_table ? p.in(table, (size_t)n_table) : nullptr;
    auto h = p.out(out_hit, n); auto nn = p.out(out_normal, 3 * n); auto it = p.out(out_interpolated, n);
    p.launch(probe_shading_normal_kernel, p.per_case(n), 128, sc.dw, vn, world->n_prims + world->n_quads - sc.n_triangles, n, r, h, nn, it);
    return p.finish() != RT_OK ? p.rc : check_traversal_overflow(sc);
}
extern "C" int rt_probe_tri_uv(int device, const rt_world_flat* world, const rt_tri_uvs* table, uint32_t n_table, size_t n, const float* rays, int32_t* out_hit, float* out_uv) {
    if (!rays || !out_hit || !out_uv) return rt_fail(RT_ERR_INVALID, "rt_probe_tri_uv: null argument");
    if ((table == nullptr) != (n_table == 0u)) return rt_fail(RT_ERR_INVALID, "rt_probe_tri_uv: a table and its count go together");
    ProbeRun p(device);
    DeviceScene sc;
    if (p.ok()) p.rc = sc.upload(world);
    if (p.ok() && n_table && n_table != sc.n_triangles) p.rc = rt_fail(RT_ERR_INVALID, "rt_probe_tri_uv: %u records for a world of %u triangles", n_table, sc.n_triangles);
    if (!p.ok() || n == 0) return p.rc;
    auto r = p.in(rays, 7 * n);
    const rt_tri_uvs* uv = n_table ? p.in(table, (size_t)n_table) : nullptr;
    auto h = p.out(out_hit, n); auto o = p.out(out_uv, 2 * n);
    p.launch(probe_tri_uv_kernel, p.per_case(n), 128, sc.dw, uv, world->n_prims + world->n_quads - sc.n_triangles, n, r, h, o);
    return p.finish() != RT_OK ? p.rc : check_traversal_overflow(sc);
}
static int environment_args(const char* who, size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* dirs, float* out_rgb, uint32_t* out_texel) {
    if (const char* why = rt_environment_image_refusal(width, height, rgb)) return rt_fail(RT_ERR_INVALID, "%s: %s", who, why);
    if (!(u0 >= 0.0f && u0 < 1.0f)) return rt_fail(RT_ERR_INVALID, "%s: u0 must lie in [0, 1)", who);
    if (n && (!dirs || !out_rgb || !out_texel)) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    return RT_OK;
}
static std::vector<float4> environment_texels(uint32_t width, uint32_t height, const float* rgb) {   // the renderer's form: one 16-byte record per texel
    std::vector<float4> t((size_t)width * height);
    for (size_t i = 0; i < t.size(); i++) t[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
    return t;
}
extern "C" int rt_probe_environment(int device, size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* dirs, float* out_rgb, uint32_t* out_texel) {
    if (const int rc = environment_args("rt_probe_environment", n, width, height, rgb, u0, dirs, out_rgb, out_texel)) return rc;
    if (n == 0) return RT_OK;
    const std::vector<float4> texels = environment_texels(width, height, rgb);
    ProbeRun p(device);
    auto t = p.in(texels.data(), texels.size());
    auto d = p.in(dirs, 3 * n);
    auto o = p.out(out_rgb, 3 * n); auto x = p.out(out_texel, n);
    p.launch(probe_environment_kernel, p.per_case(n), 128, n, t, width, height, u0, d, o, x);
    return p.finish();
}
// HOST (no GPU): the kernels' environment_value() over arrays
extern "C" int rt_environment_batch(size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* dirs, float* out_rgb, uint32_t* out_texel) {
    if (const int rc = environment_args("rt_environment_batch", n, width, height, rgb, u0, dirs, out_rgb, out_texel)) return rc;
    if (n == 0) return RT_OK;
    const std::vector<float4> texels = environment_texels(width, height, rgb);
    for (size_t i = 0; i < n; i++) {
        const f3 d = ld3(dirs + 3 * i);
        out_texel[i] = environment_texel_index(width, height, u0, d);
        st3(out_rgb + 3 * i, environment_value(texels.data(), width, height, u0, d));
    }
    return RT_OK;
}
// Environment light sampling: what the renderer uploads in mode RT_LIGHT_SAMPLING_ENV — the records with the density in their fourth lane, and
// rowc | rowy | colc in one array — or the refusal of a bad image, a bad u0, a null argument or an all-black map
static int environment_sample_args(const char* who, size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* uniforms, float* out_dir, uint32_t* out_texel,
                                   float* out_density, std::vector<float4>& records, std::vector<float>& tables) {
    if (const char* why = rt_environment_image_refusal(width, height, rgb)) return rt_fail(RT_ERR_INVALID, "%s: %s", who, why);
    if (!(u0 >= 0.0f && u0 < 1.0f)) return rt_fail(RT_ERR_INVALID, "%s: u0 must lie in [0, 1)", who);
    if (n && (!uniforms || !out_dir || !out_texel || !out_density)) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    for (size_t i = 0; i < 4u * n; i++)
        if (!(uniforms[i] > 0.0f && uniforms[i] <= 1.0f)) return rt_fail(RT_ERR_INVALID, "%s: uniform %zu is outside (0, 1]", who, i);
    const size_t n_texels = (size_t)width * height;
    std::vector<float> density(n_texels);
    tables.resize(2u * (size_t)height + 1u + n_texels);
    if (const char* why = rt_environment_distribution_refusal(width, height, rgb, tables.data(), tables.data() + height, tables.data() + 2u * (size_t)height + 1u, density.data()))
        return rt_fail(RT_ERR_INVALID, "%s: %s", who, why);
    records.resize(n_texels);
    for (size_t i = 0; i < n_texels; i++) records[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], density[i]);
    return RT_OK;
}
// the sampling rule (environment_sample, environment_density), one lane per quadruple of uniforms
__global__ void probe_environment_sample_kernel(size_t n, const float4* texels, const float* dist, uint32_t width, uint32_t height, float u0, const float* uniforms,
                                                float* out_dir, uint32_t* out_texel, float* out_density) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t texel = 0u;
    const f3 d = environment_sample(dist, width, height, u0, uniforms[4 * i], uniforms[4 * i + 1], uniforms[4 * i + 2], uniforms[4 * i + 3], &texel);
    st3(out_dir + 3 * i, d);
    out_texel[i] = texel;
    out_density[i] = environment_density(texels, width, height, u0, d);
}
extern "C" int rt_probe_environment_sample(int device, size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* uniforms, float* out_dir,
                                           uint32_t* out_texel, float* out_density) {
    std::vector<float4> records;
    std::vector<float> tables;
    if (const int rc = environment_sample_args("rt_probe_environment_sample", n, width, height, rgb, u0, uniforms, out_dir, out_texel, out_density, records, tables)) return rc;
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    auto t = p.in(records.data(), records.size()); auto c = p.in(tables.data(), tables.size());
    auto u = p.in(uniforms, 4 * n);
    auto d = p.out(out_dir, 3 * n); auto x = p.out(out_texel, n); auto y = p.out(out_density, n);
    p.launch(probe_environment_sample_kernel, p.per_case(n), 128, n, t, c, width, height, u0, u, d, x, y);
    return p.finish();
}
// HOST (no GPU): the kernels' environment_sample() and environment_density() over arrays
extern "C" int rt_environment_sample_batch(size_t n, uint32_t width, uint32_t height, const float* rgb, float u0, const float* uniforms, float* out_dir, uint32_t* out_texel,
                                           float* out_density) {
    std::vector<float4> records;
    std::vector<float> tables;
    if (const int rc = environment_sample_args("rt_environment_sample_batch", n, width, height, rgb, u0, uniforms, out_dir, out_texel, out_density, records, tables)) return rc;
    for (size_t i = 0; i < n; i++) {
        uint32_t texel = 0u;
        const f3 d = environment_sample(tables.data(), width, height, u0, uniforms[4 * i], uniforms[4 * i + 1], uniforms[4 * i + 2], uniforms[4 * i + 3], &texel);
        st3(out_dir + 3 * i, d);
        out_texel[i] = texel;
        out_density[i] = environment_density(records.data(), width, height, u0, d);
    }
    return RT_OK;
}
// The texture table in the renderer's form: one dword per texel, one vec4 per entry
struct TextureTable { std::vector<uint32_t> dwords; std::vector<uint4> entries; };
static int texture_table_args(const char* who, const rt_texture* records, uint32_t n, const uint8_t* texels, const uint32_t* index, const float* u, const float* v,
                              size_t count, float* out_rgb, TextureTable& t) {
    uint64_t n_texels = 0;
    if (const char* why = rt_texture_table_refusal(records, n, texels, &n_texels)) return rt_fail(RT_ERR_INVALID, "%s: %s", who, why);
    if (count && (!index || !u || !v || !out_rgb)) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    for (size_t i = 0; i < count; i++)
        if (index[i] >= n || records[index[i]].width == 0u) return rt_fail(RT_ERR_INVALID, "%s: lookup %zu: the table has no entry %u", who, i, index[i]);
    t.dwords.assign(n_texels ? n_texels : 1u, 0u);
    for (uint64_t i = 0; i < n_texels; i++) t.dwords[i] = (uint32_t)texels[3u * i] | (uint32_t)texels[3u * i + 1u] << 8 | (uint32_t)texels[3u * i + 2u] << 16;
    t.entries.resize(n);
    for (uint32_t k = 0; k < n; k++) t.entries[k] = make_uint4(records[k].width, records[k].height, records[k].wrap | records[k].filter << 8, records[k].first);
    return RT_OK;
}
extern "C" int rt_probe_texture(int device, const rt_texture* records, uint32_t n, const uint8_t* texels, const uint32_t* index, const float* u, const float* v,
                                size_t count, float* out_rgb) {
    TextureTable t;
    if (const int rc = texture_table_args("rt_probe_texture", records, n, texels, index, u, v, count, out_rgb, t)) return rc;
    if (count == 0) return RT_OK;
    ProbeRun p(device);
    auto dw = p.in(t.dwords.data(), t.dwords.size());
    auto en = p.in(t.entries.data(), t.entries.size());
    auto ix = p.in(index, count); auto du = p.in(u, count); auto dv = p.in(v, count);
    auto o = p.out(out_rgb, 3 * count);
    p.launch(probe_texture_kernel, p.per_case(count), 128, count, dw, en, ix, du, dv, o);
    return p.finish();
}
// HOST (no GPU): the kernels' texture_value() over arrays
extern "C" int rt_texture_lookup_batch(const rt_texture* records, uint32_t n, const uint8_t* texels, const uint32_t* index, const float* u, const float* v, size_t count,
                                       float* out_rgb) {
    TextureTable t;
    if (const int rc = texture_table_args("rt_texture_lookup_batch", records, n, texels, index, u, v, count, out_rgb, t)) return rc;
    for (size_t i = 0; i < count; i++) st3(out_rgb + 3 * i, texture_value(t.dwords.data(), t.entries[index[i]], u[i], v[i]));
    return RT_OK;
}
// Normal maps: the rule over arrays of cases, on the device and — HOST (no GPU) — here
static int normal_map_args(const char* who, const rt_texture* records, uint32_t n, const uint8_t* texels, size_t count, const uint32_t* surface, const float* a, const float* b,
                           const float* tri_uv, const float* normal, const float* ray_d, const float* u, const float* v, const uint32_t* index, const float* strength,
                           float* out_normal, uint32_t* out_path, TextureTable& t) {
    if (count && (!surface || !a || !b || !normal || !ray_d || !strength || !out_path)) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    if (const int rc = texture_table_args(who, records, n, texels, index, u, v, count, out_normal, t)) return rc;
    for (size_t i = 0; i < count; i++) {
        if (surface[i] > RT_NMAP_SURFACE_GIVEN) return rt_fail(RT_ERR_INVALID, "%s: case %zu: unknown surface %u", who, i, surface[i]);
        if (surface[i] == RT_NMAP_SURFACE_TRI_UV && !tri_uv) return rt_fail(RT_ERR_INVALID, "%s: case %zu is a triangle with coordinates, and tri_uv is null", who, i);
        if (!(std::isfinite(strength[i]) && strength[i] >= 0.0f)) return rt_fail(RT_ERR_INVALID, "%s: case %zu: a strength must be finite and >= 0", who, i);
    }
    return RT_OK;
}
extern "C" int rt_probe_normal_map(int device, const rt_texture* records, uint32_t n, const uint8_t* texels, size_t count, const uint32_t* surface, const float* a,
                                   const float* b, const float* tri_uv, const float* normal, const float* ray_d, const float* u, const float* v, const uint32_t* index,
                                   const float* strength, float* out_normal, uint32_t* out_path) {
    TextureTable t;
    if (const int rc = normal_map_args("rt_probe_normal_map", records, n, texels, count, surface, a, b, tri_uv, normal, ray_d, u, v, index, strength, out_normal, out_path, t)) return rc;
    if (count == 0) return RT_OK;
    ProbeRun p(device);
    auto dw = p.in(t.dwords.data(), t.dwords.size());
    auto en = p.in(t.entries.data(), t.entries.size());
    auto sf = p.in(surface, count); auto da = p.in(a, 3 * count); auto db = p.in(b, 3 * count);
    const float* dt = tri_uv ? p.in(tri_uv, 6 * count) : nullptr;
    auto dn = p.in(normal, 3 * count); auto dd = p.in(ray_d, 3 * count); auto du = p.in(u, count); auto dv = p.in(v, count);
    auto ix = p.in(index, count); auto st = p.in(strength, count);
    auto on = p.out(out_normal, 3 * count); auto op = p.out(out_path, count);
    p.launch(probe_normal_map_kernel, p.per_case(count), 128, count, dw, en, sf, da, db, dt, dn, dd, du, dv, ix, st, on, op);
    return p.finish();
}
extern "C" int rt_normal_map_batch(const rt_texture* records, uint32_t n, const uint8_t* texels, size_t count, const uint32_t* surface, const float* a, const float* b,
                                   const float* tri_uv, const float* normal, const float* ray_d, const float* u, const float* v, const uint32_t* index, const float* strength,
                                   float* out_normal, uint32_t* out_path) {
    TextureTable t;
    if (const int rc = normal_map_args("rt_normal_map_batch", records, n, texels, count, surface, a, b, tri_uv, normal, ray_d, u, v, index, strength, out_normal, out_path, t)) return rc;
    for (size_t i = 0; i < count; i++) {
        f3 nn = ld3(normal + 3 * i);
        out_path[i] = normal_map_case(t.dwords.data(), t.entries[index[i]], surface[i], ld3(a + 3 * i), ld3(b + 3 * i), tri_uv ? tri_uv + 6 * i : nullptr, ld3(ray_d + 3 * i),
                                      u[i], v[i], strength[i], nn);
        st3(out_normal + 3 * i, nn);
    }
    return RT_OK;
}
// Alpha cutouts: cutout_keeps over arrays of cases, on the device and — HOST (no GPU) — here.  A case whose material's record is off keeps its hit
// without a lookup, as the leaf phase does; its (u, v) and value read as zeros.
RT_HD void cutout_case(size_t i, const uint32_t* texels, const uint4* entries, const rt_quad* quads, const rt_tri_uvs* uv, const float* rays, const float* t,
                       const rt_cutout* records, const uint32_t* material, uint32_t* out_keep, float* out_uv, float* out_value) {
    const rt_cutout rec = records[material[i]];
    float tu = 0.0f, tv = 0.0f;
    f3 c = mk3(0.0f);
    bool keep = true;
    if (rec.on != RT_CUTOUT_OFF) {
        Ray r;
        r.o = ld3(rays + 6 * i); r.d = ld3(rays + 6 * i + 3); r.time = 0.0f;
        keep = cutout_keeps(texels, entries[rec.image], rec.cutoff, ld3(quads[i].Q), ld3(quads[i].u), ld3(quads[i].v), ld3(quads[i].w), uv ? uv[i].t0 : nullptr, r, t[i], tu, tv, c);
    }
    out_keep[i] = keep ? 1u : 0u; out_uv[2 * i] = tu; out_uv[2 * i + 1] = tv; out_value[i] = c.y;
}
__global__ void probe_cutout_kernel(size_t count, const uint32_t* texels, const uint4* entries, const rt_quad* quads, const rt_tri_uvs* uv, const float* rays, const float* t,
                                    const rt_cutout* records, const uint32_t* material, uint32_t* out_keep, float* out_uv, float* out_value) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    cutout_case(i, texels, entries, quads, uv, rays, t, records, material, out_keep, out_uv, out_value);
}
static int cutout_args(const char* who, const rt_texture* textures, uint32_t n_textures, const uint8_t* texels, size_t count, const rt_quad* quads, const float* rays,
                       const float* t, const rt_cutout* records, uint32_t n_records, const uint32_t* material, uint32_t* out_keep, float* out_uv, float* out_value,
                       TextureTable& tab) {
    if (const int rc = texture_table_args(who, textures, n_textures, texels, nullptr, nullptr, nullptr, 0, nullptr, tab)) return rc;
    if (count && (!quads || !rays || !t || !records || !material || !out_keep || !out_uv || !out_value)) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    for (uint32_t k = 0; k < n_records; k++) {
        if (records[k].on == RT_CUTOUT_OFF) continue;
        if (records[k].on != RT_CUTOUT_MASKED) return rt_fail(RT_ERR_INVALID, "%s: record %u: on is 0 (off) or 1 (masked), not %u", who, k, records[k].on);
        if (records[k].image >= n_textures || textures[records[k].image].width == 0u) return rt_fail(RT_ERR_INVALID, "%s: record %u: the table has no entry %u", who, k, records[k].image);
        if (!(std::isfinite(records[k].cutoff) && records[k].cutoff >= 0.0f && records[k].cutoff <= 1.0f)) return rt_fail(RT_ERR_INVALID, "%s: record %u: a cutoff must be finite and in [0, 1]", who, k);
    }
    for (size_t i = 0; i < count; i++)
        if (material[i] >= n_records) return rt_fail(RT_ERR_INVALID, "%s: case %zu: there is no record %u", who, i, material[i]);
    return RT_OK;
}
extern "C" int rt_probe_cutout(int device, const rt_texture* textures, uint32_t n_textures, const uint8_t* texels, size_t count, const rt_quad* quads, const rt_tri_uvs* uv,
                               const float* rays, const float* t, const rt_cutout* records, uint32_t n_records, const uint32_t* material, uint32_t* out_keep, float* out_uv,
                               float* out_value) {
    TextureTable tab;
    if (const int rc = cutout_args("rt_probe_cutout", textures, n_textures, texels, count, quads, rays, t, records, n_records, material, out_keep, out_uv, out_value, tab)) return rc;
    if (count == 0) return RT_OK;
    ProbeRun p(device);
    auto dw = p.in(tab.dwords.data(), tab.dwords.size());
    auto en = p.in(tab.entries.data(), tab.entries.size());
    auto dq = p.in(quads, count);
    const rt_tri_uvs* du = uv ? p.in(uv, count) : nullptr;
    auto dr = p.in(rays, 6 * count); auto dt = p.in(t, count); auto dc = p.in(records, n_records); auto dm = p.in(material, count);
    auto ok = p.out(out_keep, count); auto ouv = p.out(out_uv, 2 * count); auto ov = p.out(out_value, count);
    p.launch(probe_cutout_kernel, p.per_case(count), 128, count, dw, en, dq, du, dr, dt, dc, dm, ok, ouv, ov);
    return p.finish();
}
extern "C" int rt_cutout_batch(const rt_texture* textures, uint32_t n_textures, const uint8_t* texels, size_t count, const rt_quad* quads, const rt_tri_uvs* uv, const float* rays,
                               const float* t, const rt_cutout* records, uint32_t n_records, const uint32_t* material, uint32_t* out_keep, float* out_uv, float* out_value) {
    TextureTable tab;
    if (const int rc = cutout_args("rt_cutout_batch", textures, n_textures, texels, count, quads, rays, t, records, n_records, material, out_keep, out_uv, out_value, tab)) return rc;
    for (size_t i = 0; i < count; i++) cutout_case(i, tab.dwords.data(), tab.entries.data(), quads, uv, rays, t, records, material, out_keep, out_uv, out_value);
    return RT_OK;
}
// The marble: the kernels' noise_value() over arrays, on the device and — HOST (no GPU) — here
extern "C" int rt_probe_noise_value(int device, const rt_perlin* perlin, const float albedo[3], float scale, const float* points, size_t n, float* out_rgb) {
    if (!perlin || !albedo || !points || !out_rgb) return rt_fail(RT_ERR_INVALID, "rt_probe_noise_value: null argument");
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    auto t = p.in(perlin, 1); auto pt = p.in(points, 3 * n);
    auto o = p.out(out_rgb, 3 * n);
    p.launch(probe_noise_value_kernel, p.per_case(n), 128, n, t, ld3(albedo), scale, pt, o);
    return p.finish();
}
extern "C" int rt_noise_value_batch(const rt_perlin* perlin, const float albedo[3], float scale, const float* points, size_t n, float* out_rgb) {
    if (!perlin || !albedo || !points || !out_rgb) return rt_fail(RT_ERR_INVALID, "rt_noise_value_batch: null argument");
    for (size_t i = 0; i < n; i++) st3(out_rgb + 3 * i, noise_value(perlin, ld3(albedo), scale, ld3(points + 3 * i)));
    return RT_OK;
}
// HOST (no GPU): the kernels' tri_uv() over arrays
extern "C" int rt_tri_uv_batch(size_t n, const rt_quad* tris, const rt_tri_uvs* uv, const float* rays, const float* t, float* out_uv) {
    if (n && (!tris || !uv || !rays || !t || !out_uv)) return rt_fail(RT_ERR_INVALID, "rt_tri_uv_batch: null argument");
    for (size_t i = 0; i < n; i++) {
        Ray r;
        r.o = ld3(rays + 6 * i); r.d = ld3(rays + 6 * i + 3); r.time = 0.0f;
        tri_uv(ld3(tris[i].Q), ld3(tris[i].u), ld3(tris[i].v), ld3(tris[i].w), uv[i].t0, uv[i].t1, uv[i].t2, ray_at(r, t[i]), out_uv[2 * i], out_uv[2 * i + 1]);
    }
    return RT_OK;
}
// HOST (no GPU): the kernels' shading_normal() over arrays — here, not in rt_host.cpp, because this translation unit sees rt_device_funcs.hpp
extern "C" int rt_shading_normal_batch(size_t n, const rt_quad* tris, const rt_tri_normals* vn, const float* rays, const float* t, float* out_normal, uint32_t* out_interpolated) {
    if (n && (!tris || !vn || !rays || !t || !out_normal || !out_interpolated)) return rt_fail(RT_ERR_INVALID, "rt_shading_normal_batch: null argument");
    for (size_t i = 0; i < n; i++) {
        Ray r;
        r.o = ld3(rays + 6 * i); r.d = ld3(rays + 6 * i + 3); r.time = 0.0f;
        f3 normal = ld3(tris[i].normal);
        if (dot(r.d, normal) > 0) normal = -normal;
        out_interpolated[i] = shading_normal_flat(tris[i], vn[i], r, t[i], normal) ? 1u : 0u;
        st3(out_normal + 3 * i, normal);
    }
    return RT_OK;
}
extern "C" int rt_probe_sphere_hit(int device, size_t n, const rt_prim* prims, const float* rays, const float* preset, int32_t* out_hit,
                                   float* out_dist, float* out_normal) {
    if (!prims || !rays || !preset || !out_hit || !out_dist || !out_normal) return rt_fail(RT_ERR_INVALID, "rt_probe_sphere_hit: null argument");
    if (n == 0) return RT_OK;
    rt_material lambertian{};
    lambertian.type = RT_MAT_LAMBERTIAN;
    ProbeRun p(device);
    auto pr = p.in(prims, n); auto m = p.in(&lambertian, 1); auto r = p.in(rays, 7 * n); auto ps = p.in(preset, n);
    auto h = p.out(out_hit, n); auto d = p.out(out_dist, n); auto nn = p.out(out_normal, 3 * n);
    p.launch(probe_sphere_hit_kernel, p.per_case(n), 128, n, pr, m, r, ps, h, d, nn);
    return p.finish();
}

static int check_materials(const char* fn, size_t n, const rt_material* mats) {
    for (size_t i = 0; i < n; i++)
        if (mats[i].type > RT_MAT_ISOTROPIC) return rt_fail(RT_ERR_INVALID, "%s: case %zu: unknown material type", fn, i);
    return RT_OK;
}
// every case's [offset, length) must lie inside the tape: the kernels read tape[offset + j] for j < length only
static int check_tape(const char* fn, size_t n, size_t tape_len, const uint32_t* offsets) {
    for (size_t i = 0; i < n; i++)
        if ((uint64_t)offsets[2 * i] + offsets[2 * i + 1] > tape_len)
            return rt_fail(RT_ERR_INVALID, "%s: case %zu: tape range [%u, +%u) outside a tape of %zu", fn, i, offsets[2 * i], offsets[2 * i + 1], tape_len);
    return RT_OK;
}
// the two scatter probes and the two camera probes behind their checks; the caller has put its generator's arrays into p
template <typename MakeRng>
static int scatter_cases(ProbeRun& p, MakeRng make_rng, size_t n, const rt_material* mats, const float* rays, const float* dist, const float* normals,
                         int32_t* out_scattered, float* out_rays, float* out_atten, uint32_t* out_draws) {
    auto m = p.in(mats, n); auto r = p.in(rays, 7 * n); auto d = p.in(dist, n); auto nn = p.in(normals, 3 * n);
    auto s = p.out(out_scattered, n); auto orr = p.out(out_rays, 7 * n); auto a = p.out(out_atten, 3 * n); auto dr = p.out(out_draws, n);
    p.launch(probe_scatter_kernel<MakeRng>, p.per_case(n), 128, make_rng, n, m, r, d, nn, s, orr, a, dr);
    return p.finish();
}
template <typename MakeRng>
static int camera_cases(ProbeRun& p, MakeRng make_rng, const rt_camera& cam, size_t n, const float* st, float* out_rays, uint32_t* out_draws) {
    auto s = p.in(st, 2 * n);
    auto r = p.out(out_rays, 7 * n); auto d = p.out(out_draws, n);
    p.launch(probe_camera_kernel<MakeRng>, p.per_case(n), 128, make_rng, cam, n, s, r, d);
    return p.finish();
}
extern "C" int rt_probe_scatter(int device, uint64_t seed, size_t n, const rt_material* mats, const float* rays, const float* dist,
                                const float* normals, const uint32_t* keys, int32_t* out_scattered, float* out_rays, float* out_atten,
                                uint32_t* out_draws) {
    if (!mats || !rays || !dist || !normals || !keys || !out_scattered || !out_rays || !out_atten || !out_draws)
        return rt_fail(RT_ERR_INVALID, "rt_probe_scatter: null argument");
    if (n == 0) return RT_OK;
    if (int rc = check_materials("rt_probe_scatter", n, mats)) return rc;
    ProbeRun p(device);
    const KeyedRng make_rng{seed, p.in(keys, 2 * n)};
    return scatter_cases(p, make_rng, n, mats, rays, dist, normals, out_scattered, out_rays, out_atten, out_draws);
}
extern "C" int rt_probe_camera(int device, uint64_t seed, const rt_camera* cam, size_t n, const float* st, const uint32_t* keys,
                               float* out_rays, uint32_t* out_draws) {
    if (!cam || !st || !keys || !out_rays || !out_draws) return rt_fail(RT_ERR_INVALID, "rt_probe_camera: null argument");
    if (cam->type > RT_CAM_MOTION) return rt_fail(RT_ERR_INVALID, "rt_probe_camera: unknown camera type");
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    const KeyedRng make_rng{seed, p.in(keys, 2 * n)};
    return camera_cases(p, make_rng, *cam, n, st, out_rays, out_draws);
}
extern "C" int rt_probe_scatter_tape(int device, size_t n, const rt_material* mats, const float* rays, const float* dist, const float* normals,
                                     const uint32_t* tape, size_t tape_len, const uint32_t* offsets, int32_t* out_scattered, float* out_rays,
                                     float* out_atten, uint32_t* out_draws) {
    if (!mats || !rays || !dist || !normals || !tape || !offsets || !out_scattered || !out_rays || !out_atten || !out_draws)
        return rt_fail(RT_ERR_INVALID, "rt_probe_scatter_tape: null argument");
    if (n == 0) return RT_OK;
    if (int rc = check_materials("rt_probe_scatter_tape", n, mats)) return rc;
    if (int rc = check_tape("rt_probe_scatter_tape", n, tape_len, offsets)) return rc;
    ProbeRun p(device);
    const TapedRng make_rng{p.in(tape, tape_len), p.in(offsets, 2 * n)};
    return scatter_cases(p, make_rng, n, mats, rays, dist, normals, out_scattered, out_rays, out_atten, out_draws);
}
extern "C" int rt_probe_camera_tape(int device, const rt_camera* cam, size_t n, const float* st, const uint32_t* tape, size_t tape_len,
                                    const uint32_t* offsets, float* out_rays, uint32_t* out_draws) {
    if (!cam || !st || !tape || !offsets || !out_rays || !out_draws) return rt_fail(RT_ERR_INVALID, "rt_probe_camera_tape: null argument");
    if (cam->type > RT_CAM_MOTION) return rt_fail(RT_ERR_INVALID, "rt_probe_camera_tape: unknown camera type");
    if (n == 0) return RT_OK;
    if (int rc = check_tape("rt_probe_camera_tape", n, tape_len, offsets)) return rc;
    ProbeRun p(device);
    const TapedRng make_rng{p.in(tape, tape_len), p.in(offsets, 2 * n)};
    return camera_cases(p, make_rng, *cam, n, st, out_rays, out_draws);
}
// Lens cameras: the rule over arrays of cases, on the device and — HOST (no GPU) — here
static int camera_rays_args(const char* who, const rt_camera* cam, size_t n, const float* st, const uint32_t* tape, size_t tape_len, const uint32_t* offsets,
                            float* out_rays, uint32_t* out_draws) {
    if (!cam || !st || !tape || !offsets || !out_rays || !out_draws) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    if (int rc = rt_camera_check(who, cam)) return rc;
    return check_tape(who, n, tape_len, offsets);
}
extern "C" int rt_probe_camera_lens(int device, const rt_camera* cam, size_t n, const float* st, const uint32_t* tape, size_t tape_len, const uint32_t* offsets,
                                    float* out_rays, uint32_t* out_draws) {
    if (const int rc = camera_rays_args("rt_probe_camera_lens", cam, n, st, tape, tape_len, offsets, out_rays, out_draws)) return rc;
    if (cam->type < RT_CAM_PERSPECTIVE) return rt_fail(RT_ERR_INVALID, "rt_probe_camera_lens: camera type %u is no lens camera (rt_probe_camera_tape probes the reference's three)", cam->type);
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    const uint32_t no_tape = 0x800001u;   // an empty tape, as rt_probe_microfacet uploads it
    auto s = p.in(st, 2 * n); auto dt = tape_len ? p.in(tape, tape_len) : p.in(&no_tape, 1); auto dof = p.in(offsets, 2 * n);
    auto r = p.out(out_rays, 7 * n); auto d = p.out(out_draws, n);
    p.launch(probe_camera_lens_kernel, p.per_case(n), 128, *cam, n, s, dt, dof, r, d);
    return p.finish();
}
extern "C" int rt_camera_rays_batch(const rt_camera* cam, size_t n, const float* st, const uint32_t* tape, size_t tape_len, const uint32_t* offsets, float* out_rays,
                                    uint32_t* out_draws) {
    if (const int rc = camera_rays_args("rt_camera_rays_batch", cam, n, st, tape, tape_len, offsets, out_rays, out_draws)) return rc;
    for (size_t i = 0; i < n; i++) camera_rays_case(*cam, i, st, tape, offsets, out_rays, out_draws);
    return RT_OK;
}
// Microfacet surfaces: the rule over arrays of cases, on the device and — HOST (no GPU) — here
static int microfacet_args(const char* who, size_t count, const float* normal, const float* ray_d, const float* roughness, const float* f0, const uint32_t* coat,
                           const uint32_t* tape, size_t tape_len, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    if (!normal || !ray_d || !roughness || !f0 || !coat || !tape || !offsets || !out_dir || !out_weight || !out_path || !out_draws)
        return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    if (int rc = check_tape(who, count, tape_len, offsets)) return rc;
    for (size_t i = 0; i < count; i++)
        if (!(std::isfinite(roughness[i]) && roughness[i] >= 0.0f && roughness[i] <= 1.0f))
            return rt_fail(RT_ERR_INVALID, "%s: case %zu: a roughness must be finite and in [0, 1]", who, i);
    return RT_OK;
}
extern "C" int rt_probe_microfacet(int device, size_t count, const float* normal, const float* ray_d, const float* roughness, const float* f0, const uint32_t* coat,
                                   const uint32_t* tape, size_t tape_len, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path,
                                   uint32_t* out_draws) {
    if (const int rc = microfacet_args("rt_probe_microfacet", count, normal, ray_d, roughness, f0, coat, tape, tape_len, offsets, out_dir, out_weight, out_path, out_draws)) return rc;
    if (count == 0) return RT_OK;
    ProbeRun p(device);
    auto dn = p.in(normal, 3 * count); auto dd = p.in(ray_d, 3 * count); auto dr = p.in(roughness, count); auto df = p.in(f0, 3 * count); auto dc = p.in(coat, count);
    const uint32_t no_tape = 0x800001u;   // an empty tape: every case's range is empty, and one word keeps the upload from being one of no bytes
    auto dt = tape_len ? p.in(tape, tape_len) : p.in(&no_tape, 1); auto dof = p.in(offsets, 2 * count);
    auto od = p.out(out_dir, 3 * count); auto ow = p.out(out_weight, 3 * count); auto op = p.out(out_path, count); auto on = p.out(out_draws, count);
    p.launch(probe_microfacet_kernel, p.per_case(count), 128, count, dn, dd, dr, df, dc, dt, dof, od, ow, op, on);
    return p.finish();
}
extern "C" int rt_microfacet_batch(size_t count, const float* normal, const float* ray_d, const float* roughness, const float* f0, const uint32_t* coat, const uint32_t* tape,
                                   size_t tape_len, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    if (const int rc = microfacet_args("rt_microfacet_batch", count, normal, ray_d, roughness, f0, coat, tape, tape_len, offsets, out_dir, out_weight, out_path, out_draws)) return rc;
    for (size_t i = 0; i < count; i++) microfacet_case(i, normal, ray_d, roughness, f0, coat, tape, offsets, out_dir, out_weight, out_path, out_draws);
    return RT_OK;
}
// Rough glass: its rule over arrays of cases, on the device and — HOST (no GPU) — here
static int rough_glass_args(const char* who, size_t count, const float* normal, const float* ray_d, const float* roughness, const float* ior, const uint32_t* tape,
                            size_t tape_len, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    if (!normal || !ray_d || !roughness || !ior || !tape || !offsets || !out_dir || !out_weight || !out_path || !out_draws)
        return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    if (int rc = check_tape(who, count, tape_len, offsets)) return rc;
    for (size_t i = 0; i < count; i++)
        if (!(std::isfinite(roughness[i]) && roughness[i] >= 0.0f && roughness[i] <= 1.0f))
            return rt_fail(RT_ERR_INVALID, "%s: case %zu: a roughness must be finite and in [0, 1]", who, i);
    return RT_OK;
}
extern "C" int rt_probe_rough_glass(int device, size_t count, const float* normal, const float* ray_d, const float* roughness, const float* ior, const uint32_t* tape,
                                    size_t tape_len, const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    if (const int rc = rough_glass_args("rt_probe_rough_glass", count, normal, ray_d, roughness, ior, tape, tape_len, offsets, out_dir, out_weight, out_path, out_draws)) return rc;
    if (count == 0) return RT_OK;
    ProbeRun p(device);
    auto dn = p.in(normal, 3 * count); auto dd = p.in(ray_d, 3 * count); auto dr = p.in(roughness, count); auto di = p.in(ior, count);
    const uint32_t no_tape = 0x800001u;   // an empty tape, as rt_probe_microfacet uploads it
    auto dt = tape_len ? p.in(tape, tape_len) : p.in(&no_tape, 1); auto dof = p.in(offsets, 2 * count);
    auto od = p.out(out_dir, 3 * count); auto ow = p.out(out_weight, count); auto op = p.out(out_path, count); auto on = p.out(out_draws, count);
    p.launch(probe_rough_glass_kernel, p.per_case(count), 128, count, dn, dd, dr, di, dt, dof, od, ow, op, on);
    return p.finish();
}
extern "C" int rt_rough_glass_batch(size_t count, const float* normal, const float* ray_d, const float* roughness, const float* ior, const uint32_t* tape, size_t tape_len,
                                    const uint32_t* offsets, float* out_dir, float* out_weight, uint32_t* out_path, uint32_t* out_draws) {
    if (const int rc = rough_glass_args("rt_rough_glass_batch", count, normal, ray_d, roughness, ior, tape, tape_len, offsets, out_dir, out_weight, out_path, out_draws)) return rc;
    for (size_t i = 0; i < count; i++) rough_glass_case(i, normal, ray_d, roughness, ior, tape, offsets, out_dir, out_weight, out_path, out_draws);
    return RT_OK;
}
extern "C" int rt_probe_radiance(const rt_render_config* cfg, const rt_camera* cam, const rt_world_flat* world, size_t n,
                                 const uint32_t* keys, float* out_radiance) {
    if (!cfg || !cam || !keys || !out_radiance) return rt_fail(RT_ERR_INVALID, "rt_probe_radiance: null argument");
    if (cfg->width == 0 || cfg->height == 0) return rt_fail(RT_ERR_INVALID, "rt_probe_radiance: empty image");
    if (cam->type > RT_CAM_MOTION) return rt_fail(RT_ERR_INVALID, "rt_probe_radiance: unknown camera type");
    for (size_t i = 0; i < n; i++)
        if (keys[2 * i] >= cfg->width * cfg->height) return rt_fail(RT_ERR_INVALID, "rt_probe_radiance: key %zu: pixel out of range", i);
    if (world && world->background == 2u)
        return rt_fail(RT_ERR_INVALID, "rt_probe_radiance: the probe runs sample_world, which looks no environment map up (background mode 2); rt_probe_environment probes the map");
    for (uint32_t i = 0; world && world->materials && i < world->n_materials; i++)
        if (world->materials[i].type == RT_MAT_LAMBERTIAN_IMAGE && world->materials[i].albedo2[0] != 0.0f)
            return rt_fail(RT_ERR_INVALID, "rt_probe_radiance: the probe runs sample_world, which reads no texture table (material %u names an image other than 0); rt_probe_texture probes the table", i);
    ProbeRun p(cfg->device);
    DeviceScene sc;
    if (p.ok()) p.rc = sc.upload(world);
    if (!p.ok() || n == 0) return p.rc;
    auto k = p.in(keys, 2 * n);
    auto o = p.out(out_radiance, 3 * n);
    p.launch(probe_radiance_kernel, p.per_case(n), 128, sc.dw, *cam, cfg->width, cfg->height, cfg->max_depth, cfg->seed, n, k, o);
    return p.finish() != RT_OK ? p.rc : check_traversal_overflow(sc);
}
extern "C" int rt_probe_sphere_index(int device, const rt_camera* cam, uint32_t width, uint32_t height, size_t n_spheres,
                                     const float* spheres, int32_t* out_index) {
    if (!cam || !spheres || !out_index) return rt_fail(RT_ERR_INVALID, "rt_probe_sphere_index: null argument");
    if (width == 0 || height == 0) return RT_OK;
    ProbeRun p(device);
    auto s = p.in(reinterpret_cast<const float4*>(spheres), n_spheres);
    auto o = p.out(out_index, (size_t)width * height);
    if (!p.ok()) return p.rc;   // (sizes that cannot even be allocated are reported as that)
    if (n_spheres > 0x7fffffffull || (uint64_t)width * height > 0xffffff00ull) return rt_fail(RT_ERR_INVALID, "rt_probe_sphere_index: too large");
    p.launch(probe_sphere_index_kernel, dim3((width * height + 255u) / 256u), 256, s, (uint32_t)n_spheres, *cam, width, height, o);
    return p.finish();
}
extern "C" int rt_probe_rng(int device, uint64_t seed, size_t n, const uint32_t* keys, uint32_t n_draws, float* out) {
    if (!keys || !out) return rt_fail(RT_ERR_INVALID, "rt_probe_rng: null argument");
    if (n == 0 || n_draws == 0) return RT_OK;
    ProbeRun p(device);
    auto k = p.in(keys, 2 * n);
    auto o = p.out(out, n * n_draws);
    p.launch(probe_rng_kernel, p.per_case(n), 128, seed, n, k, n_draws, o);
    return p.finish();
}
__global__ void probe_math_kernel(int fn, size_t n, const float* a, const float* b, float* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fn == 0 ? rt_logf(a[i]) : fn == 1 ? rt_sinf(a[i]) : fn == 2 ? rt_acosf(a[i]) : rt_atan2f(a[i], b[i]);
}
extern "C" int rt_probe_math(int device, int fn, size_t n, const float* a, const float* b, float* out) {
    if (!a || !b || !out) return rt_fail(RT_ERR_INVALID, "rt_probe_math: null argument");
    if (fn < 0 || fn > 3) return rt_fail(RT_ERR_INVALID, "rt_probe_math: unknown function %d", fn);
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    auto da = p.in(a, n); auto db = p.in(b, n);
    auto o = p.out(out, n);
    p.launch(probe_math_kernel, p.per_case(n), 128, fn, n, da, db, o);
    return p.finish();
}
// Solid glass: rt_expf and the rule over arrays of cases, on the device and — HOST (no GPU) — here
__global__ void probe_expf_kernel(size_t n, const float* x, float* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = rt_expf(x[i]);
}
extern "C" int rt_probe_expf(int device, size_t count, const float* x, float* out) {
    if (!x || !out) return rt_fail(RT_ERR_INVALID, "rt_probe_expf: null argument");
    if (count == 0) return RT_OK;
    ProbeRun p(device);
    auto dx = p.in(x, count);
    auto o = p.out(out, count);
    p.launch(probe_expf_kernel, p.per_case(count), 128, count, dx, o);
    return p.finish();
}
extern "C" int rt_expf_batch(size_t count, const float* x, float* out) {
    if (!x || !out) return rt_fail(RT_ERR_INVALID, "rt_expf_batch: null argument");
    for (size_t i = 0; i < count; i++) out[i] = rt_expf(x[i]);
    return RT_OK;
}
// one case of the rule: the facing on the stored normal, or — a sphere — on the outward one, then interior_hit
RT_HD void interior_case(size_t i, const float* Ng, const float* n, const float* d, const float* t, const float* ior, const float* sigma, const uint32_t* sphere,
                         uint32_t* out_back, float* out_eta, float* out_T) {
    const f3 dir = ld3(d + 3 * i);
    const bool back = dot(dir, sphere[i] != 0u ? ld3(n + 3 * i) : ld3(Ng + 3 * i)) > 0;
    float eta;
    f3 T;
    interior_hit(back, dir, t[i], ior[i], ld3(sigma + 3 * i), eta, T);
    out_back[i] = back ? 1u : 0u; out_eta[i] = eta; st3(out_T + 3 * i, T);
}
__global__ void probe_interior_kernel(size_t count, const float* Ng, const float* n, const float* d, const float* t, const float* ior, const float* sigma,
                                      const uint32_t* sphere, uint32_t* out_back, float* out_eta, float* out_T) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    interior_case(i, Ng, n, d, t, ior, sigma, sphere, out_back, out_eta, out_T);
}
static int interior_args(const char* who, const float* Ng, const float* n, const float* d, const float* t, const float* ior, const float* sigma, const uint32_t* sphere,
                         uint32_t* out_back, float* out_eta, float* out_T) {
    if (!Ng || !n || !d || !t || !ior || !sigma || !sphere || !out_back || !out_eta || !out_T) return rt_fail(RT_ERR_INVALID, "%s: null argument", who);
    return RT_OK;
}
extern "C" int rt_probe_interior(int device, size_t count, const float* Ng, const float* n, const float* d, const float* t, const float* ior, const float* sigma,
                                 const uint32_t* sphere, uint32_t* out_back, float* out_eta, float* out_T) {
    if (const int rc = interior_args("rt_probe_interior", Ng, n, d, t, ior, sigma, sphere, out_back, out_eta, out_T)) return rc;
    if (count == 0) return RT_OK;
    ProbeRun p(device);
    auto dg = p.in(Ng, 3 * count); auto dn = p.in(n, 3 * count); auto dd = p.in(d, 3 * count); auto dt = p.in(t, count); auto di = p.in(ior, count);
    auto ds = p.in(sigma, 3 * count); auto dk = p.in(sphere, count);
    auto ob = p.out(out_back, count); auto oe = p.out(out_eta, count); auto oT = p.out(out_T, 3 * count);
    p.launch(probe_interior_kernel, p.per_case(count), 128, count, dg, dn, dd, dt, di, ds, dk, ob, oe, oT);
    return p.finish();
}
extern "C" int rt_interior_batch(size_t count, const float* Ng, const float* n, const float* d, const float* t, const float* ior, const float* sigma, const uint32_t* sphere,
                                 uint32_t* out_back, float* out_eta, float* out_T) {
    if (const int rc = interior_args("rt_interior_batch", Ng, n, d, t, ior, sigma, sphere, out_back, out_eta, out_T)) return rc;
    for (size_t i = 0; i < count; i++) interior_case(i, Ng, n, d, t, ior, sigma, sphere, out_back, out_eta, out_T);
    return RT_OK;
}

// The device half of the math vocabulary (csrc/rt_math.hpp) over arrays: the functions the fixtures tests/golden/glm_*.f32 —
// generated by the REFERENCE's vendored GLM + glm_utils.h (oracle/ref_glm_probe.cpp) — cover, plus Ray::at / isBackfacing
// (tests/golden/ref_ray_*, from the reference's ray_data.cuh).  The one direct reference -> HIP check there is.
__global__ void probe_glm_kernel(int fn, size_t n, uint32_t nin, uint32_t nout, const float* __restrict__ in, float* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = in + i * nin;
    float* o = out + i * nout;
    switch (fn) {
        case 0: o[0] = dot(ld3(a), ld3(a + 3)); break;
        case 1: st3(o, cross(ld3(a), ld3(a + 3))); break;
        case 2: st3(o, normalize(ld3(a))); break;
        case 3: st3(o, reflect(ld3(a), ld3(a + 3))); break;
        case 4: st3(o, refract(ld3(a), ld3(a + 3), a[6])); break;
        case 5: st3(o, mix(ld3(a), ld3(a + 3), a[6])); break;
        case 6: o[0] = mix(a[0], a[1], a[2]); break;
        case 7: st3(o, glm_min(ld3(a), ld3(a + 3))); break;
        case 8: st3(o, glm_max(ld3(a), ld3(a + 3))); break;
        case 9: o[0] = comp_max(ld3(a)); break;
        case 10: o[0] = comp_min(ld3(a)); break;
        case 11: st3(o, clamp01_sqrt(ld3(a))); break;
        case 12: o[0] = near_zero(ld3(a)) ? 1.0f : 0.0f; break;
        case 13: o[0] = length2(ld3(a)); break;
        case 14: st3(o, linear_interpolate(ld3(a), ld3(a + 3), a[6])); break;
        case 15: o[0] = radians(a[0]); break;
        default: {  // 16: Ray::at (ray_data.cuh:14) + isBackfacing (ray_data.cuh:44-46): (o, d, t, normal) -> (at, backfacing)
            Ray r; r.o = ld3(a); r.d = ld3(a + 3); r.time = 0.0f;
            st3(o, ray_at(r, a[6]));
            o[3] = dot(r.d, ld3(a + 7)) > 0 ? 1.0f : 0.0f;
        }
    }
}
extern "C" int rt_probe_glm(int device, int fn, size_t n, const float* in, float* out) {
    static const uint32_t shape[17][2] = {{6, 1}, {6, 3}, {3, 3}, {6, 3}, {7, 3}, {7, 3}, {3, 1}, {6, 3}, {6, 3}, {3, 1}, {3, 1}, {3, 3}, {3, 1},
                                          {3, 1}, {7, 3}, {1, 1}, {10, 4}};
    if (!in || !out) return rt_fail(RT_ERR_INVALID, "rt_probe_glm: null argument");
    if (fn < 0 || fn > 16) return rt_fail(RT_ERR_INVALID, "rt_probe_glm: unknown function %d", fn);
    if (n == 0) return RT_OK;
    const uint32_t nin = shape[fn][0], nout = shape[fn][1];
    ProbeRun p(device);
    auto di = p.in(in, n * nin);
    auto dout = p.out(out, n * nout);
    p.launch(probe_glm_kernel, p.per_case(n), 128, fn, n, nin, nout, di, dout);
    return p.finish();
}

// ---------------------------------------------------------------------------------------------
// verification of rt_fastdiv.hpp
// ---------------------------------------------------------------------------------------------
__global__ void probe_aabb_regular_kernel(size_t n, const float* boxes, const float* rays, const float* maxd, int32_t* regular,
                                          int32_t* hit, float* dist) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = ld3(rays + 6 * i); r.d = ld3(rays + 6 * i + 3); r.time = 0.0f;
    f3 bmin = ld3(boxes + 6 * i), bmax = ld3(boxes + 6 * i + 3);
    bool reg = ray_is_regular(r) && coord_is_regular(bmin.x) && coord_is_regular(bmin.y) && coord_is_regular(bmin.z) &&
               coord_is_regular(bmax.x) && coord_is_regular(bmax.y) && coord_is_regular(bmax.z);
    regular[i] = reg ? 1 : 0;
    float d = 0.0f;
    bool h = false;
    if (reg) {
        f3 inv_d = mk3(rcp_exact_regular(r.d.x), rcp_exact_regular(r.d.y), rcp_exact_regular(r.d.z));  // as the render kernel does
        h = aabb_intersects_regular(bmin, bmax, r, inv_d, maxd[i], d);
    }
    hit[i] = h ? 1 : 0;
    dist[i] = d;
}

extern "C" int rt_probe_aabb_regular(int device, size_t n, const float* boxes, const float* rays, const float* max_dist,
                                     int32_t* out_regular, int32_t* out_hit, float* out_dist) {
    if (!boxes || !rays || !max_dist || !out_regular || !out_hit || !out_dist) return rt_fail(RT_ERR_INVALID, "rt_probe_aabb_regular: null argument");
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    auto b = p.in(boxes, 6 * n); auto r = p.in(rays, 6 * n); auto m = p.in(max_dist, n);
    auto g = p.out(out_regular, n); auto h = p.out(out_hit, n); auto d = p.out(out_dist, n);
    p.launch(probe_aabb_regular_kernel, p.per_case(n), 128, n, b, r, m, g, h, d);
    return p.finish();
}

// one block per divisor significand; its 256 threads sweep all 2^23 numerator significands
__global__ __launch_bounds__(256) void selftest_fastrcp_kernel(unsigned long long* counts, uint32_t* example) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long n = 0, bad = 0;
    for (uint64_t u = i; u < (1ull << 32); u += stride) {
        const uint32_t bits = (uint32_t)u;
        const uint32_t e = (bits >> 23) & 0xffu;
        if (e < 127u - 40u || e > 127u + 39u) continue;
        const float x = __uint_as_float(bits);
        n++;
        if (__float_as_uint(rcp_exact_regular(x)) != __float_as_uint(1.0f / x)) { bad++; *example = bits; }
    }
    atomicAdd(counts + 0, n);
    atomicAdd(counts + 1, bad);
}

extern "C" int rt_selftest_fastrcp(int device, uint64_t* checked, uint64_t* mismatches, uint32_t* example) {
    if (!checked || !mismatches || !example) return rt_fail(RT_ERR_INVALID, "rt_selftest_fastrcp: null argument");
    unsigned long long h[2] = {0, 0};
    ProbeRun p(device);
    auto counts = p.out(h, 2, true); auto ex = p.out(example, 1, true);   // the kernel adds to them
    p.launch(selftest_fastrcp_kernel, dim3(8192), 256, counts, ex);
    if (p.finish() != RT_OK) return p.rc;
    *checked = h[0];
    *mismatches = h[1];
    return RT_OK;
}

__global__ __launch_bounds__(256) void selftest_fastdiv_kernel(uint32_t first_den, uint32_t num_exp_bits, uint32_t den_exp_bits,
                                                               unsigned long long* mismatches, uint32_t* example) {
    uint32_t md = first_den + blockIdx.x;
    float d = __uint_as_float(den_exp_bits | md);
    float r = 1.0f / d;
    float rl = rcp_low_word(d, r);
    uint32_t bad = 0;
    uint32_t bad_n = 0;
    for (uint32_t mn = threadIdx.x; mn < (1u << 23); mn += 256u) {
        float n = __uint_as_float((num_exp_bits & ~1u) | mn);
        float q = (num_exp_bits & 1u) ? fast_div_exact4(n, d, r, rl) : fast_div_exact(n, d, r);   // bit 0 of the exponent word = mode
        float ref = n / d;
        if (__float_as_uint(q) != __float_as_uint(ref)) { bad++; bad_n = __float_as_uint(n); }
    }
    if (bad) {
        atomicAdd(mismatches, (unsigned long long)bad);
        example[0] = bad_n;
        example[1] = __float_as_uint(d);
    }
}

// mode: bit 0 of the kernel's numerator exponent word — 0 fast_div_exact, 1 fast_div_exact4
static int selftest_fastdiv(const char* fn, uint32_t mode, int device, uint32_t first_den, uint32_t n_den, int32_t num_exp, int32_t den_exp,
                            uint64_t* mismatches, uint32_t example[2]) {
    if (!mismatches || !example) return rt_fail(RT_ERR_INVALID, "%s: null argument", fn);
    if (first_den >= (1u << 23) || n_den == 0 || n_den > (1u << 23) - first_den) return rt_fail(RT_ERR_INVALID, "%s: significand range out of bounds", fn);
    if (num_exp < -126 || num_exp > 127 || den_exp < -126 || den_exp > 127) return rt_fail(RT_ERR_INVALID, "%s: exponent out of range", fn);
    unsigned long long bad = 0;
    ProbeRun p(device);
    auto cnt = p.out(&bad, 1, true); auto ex = p.out(example, 2, true);   // the kernel adds to the count
    p.launch(selftest_fastdiv_kernel, dim3(n_den), 256, first_den, ((uint32_t)(num_exp + 127) << 23) | mode, (uint32_t)(den_exp + 127) << 23, cnt, ex);
    if (p.finish() == RT_OK) *mismatches = bad;
    return p.rc;
}
extern "C" int rt_selftest_fastdiv(int device, uint32_t first_den, uint32_t n_den, int32_t num_exp, int32_t den_exp,
                                   uint64_t* mismatches, uint32_t example[2]) {
    return selftest_fastdiv("rt_selftest_fastdiv", 0u, device, first_den, n_den, num_exp, den_exp, mismatches, example);
}
extern "C" int rt_selftest_fastdiv4(int device, uint32_t first_den, uint32_t n_den, int32_t num_exp, int32_t den_exp,
                                    uint64_t* mismatches, uint32_t example[2]) {
    return selftest_fastdiv("rt_selftest_fastdiv4", 1u, device, first_den, n_den, num_exp, den_exp, mismatches, example);
}
// One case of the two box-pair probes: the ray, the two boxes (12 coordinates) and the 8-int record
// [regular, uncertain, hit_left, hit_right, swap | verbatim: hit_left, hit_right, left_dist > right_dist].
struct BoxPairCase {
    Ray r;
    const float* b;
    int32_t* o;
    bool regular;   // ray and coordinates inside the fast-division class, boxes not inverted: only then is the rest of the record filled in
};
__device__ BoxPairCase boxpair_case(size_t i, const float* boxes, const float* rays, int32_t* out) {
    BoxPairCase c;
    c.r.o = ld3(rays + 6 * i); c.r.d = ld3(rays + 6 * i + 3); c.r.time = 0.0f;
    c.b = boxes + 12 * i;
    c.regular = ray_is_regular(c.r);
    for (int k = 0; k < 12; k++) c.regular = c.regular && coord_is_regular(c.b[k]);
    for (int k = 0; k < 3; k++) c.regular = c.regular && c.b[k] <= c.b[3 + k] && c.b[6 + k] <= c.b[9 + k];
    c.o = out + 8 * i;
    for (int k = 0; k < 8; k++) c.o[k] = 0;
    c.o[0] = c.regular ? 1 : 0;
    return c;
}
// o[5..7]: the decisions of the verbatim box tests
__device__ void boxpair_verbatim(const BoxPairCase& c, float max_dist) {
    float dl = RT_MISS_DIST, dr = RT_MISS_DIST;
    const bool hl = aabb_intersects(ld3(c.b), ld3(c.b + 3), c.r, max_dist, dl);
    const bool hr = aabb_intersects(ld3(c.b + 6), ld3(c.b + 9), c.r, max_dist, dr);
    c.o[5] = hl; c.o[6] = hr; c.o[7] = dl > dr;
}

// box_pair_filtered vs the exact decisions, on regular inputs only
__global__ void probe_boxpair_filtered_kernel(size_t n, const float* boxes, const float* rays, const float* maxd, int32_t* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BoxPairCase c = boxpair_case(i, boxes, rays, out);
    if (!c.regular) return;
    const Ray& r = c.r;
    const float* b = c.b;
    f3 inv_d = mk3(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
    BoxPairDecision d = box_pair_filtered(ld3(b), ld3(b + 3), ld3(b + 6), ld3(b + 9), r, inv_d, maxd[i]);
    c.o[1] = d.uncertain; c.o[2] = d.hit_left; c.o[3] = d.hit_right; c.o[4] = d.swap;
    boxpair_verbatim(c, maxd[i]);
}

// The hot loop's box pair (rt_fastdiv.hpp: CERTIFIED FAR PLANES) next to the verbatim box tests: near parameters as exact quotients, far parameters as
// products whose `tmin <= tmax` decisions are certified — a lane that cannot certify redoes its far planes exactly (the kernel does that for the whole wave).
// The two hit decisions and the order are written as render_kernel_stream writes them, but they are a copy: as scalar helpers shared with the hot loops
// they changed the machine code of the stream (hit decision) and exchange (order) kernels.
__global__ void probe_boxpair_certified_kernel(size_t n, const float* boxes, const float* rays, const float* maxd, int32_t* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BoxPairCase c = boxpair_case(i, boxes, rays, out);
    if (!c.regular) return;
    const Ray& r = c.r;
    const float* b = c.b;
    const f3 inv_d = mk3(rcp_exact_regular(r.d.x), rcp_exact_regular(r.d.y), rcp_exact_regular(r.d.z));
    const f3 inv_lo = mk3(rcp_low_word(r.d.x, inv_d.x), rcp_low_word(r.d.y, inv_d.y), rcp_low_word(r.d.z, inv_d.z));
    // near = the plane the ray enters through (box min where d >= 0), as the kernel's (min, max, min) triples deliver it
    const bool sx = r.d.x < 0, sy = r.d.y < 0, sz = r.d.z < 0;
    const float lnx = sx ? b[3] : b[0], lny = sy ? b[4] : b[1], lnz = sz ? b[5] : b[2], lfx = sx ? b[0] : b[3], lfy = sy ? b[1] : b[4], lfz = sz ? b[2] : b[5];
    const float rnx = sx ? b[9] : b[6], rny = sy ? b[10] : b[7], rnz = sz ? b[11] : b[8], rfx = sx ? b[6] : b[9], rfy = sy ? b[7] : b[10], rfz = sz ? b[8] : b[11];
    const float tl = slab_near_exact(lnx, lny, lnz, r, inv_d, inv_lo), tr = slab_near_exact(rnx, rny, rnz, r, inv_d, inv_lo);
    float far_l = slab_far_product(lfx, lfy, lfz, r, inv_d), far_r = slab_far_product(rfx, rfy, rfz, r, inv_d);
    const bool unc = far_pair_uncertain(tl, far_l, tr, far_r);
    if (unc) { far_l = slab_far_exact(lfx, lfy, lfz, r, inv_d, inv_lo); far_r = slab_far_exact(rfx, rfy, rfz, r, inv_d, inv_lo); }
    const float rec_t = maxd[i];
    const bool hl = tl <= far_l && tl < rec_t && far_l > 0, hr = tr <= far_r && tr < rec_t && far_r > 0;
    c.o[1] = unc; c.o[2] = hl; c.o[3] = hr; c.o[4] = hr && (!hl || tl > tr);
    boxpair_verbatim(c, maxd[i]);
}

// The same pair with the far parameters as one fma each (rt_fastdiv.hpp: CERTIFIED FAR PLANES, ONE FMA EACH): the per-ray offset and margin, the far
// parameters and the certificate come from the helpers the hot loop calls; the redo and the decisions are written as above.
__global__ void probe_boxpair_certified_fma_kernel(size_t n, const float* boxes, const float* rays, const float* maxd, int32_t* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BoxPairCase c = boxpair_case(i, boxes, rays, out);
    if (!c.regular) return;
    const Ray& r = c.r;
    const float* b = c.b;
    const f3 inv_d = mk3(rcp_exact_regular(r.d.x), rcp_exact_regular(r.d.y), rcp_exact_regular(r.d.z));
    const f3 inv_lo = mk3(rcp_low_word(r.d.x, inv_d.x), rcp_low_word(r.d.y, inv_d.y), rcp_low_word(r.d.z, inv_d.z));
    const f3 far_c = slab_fma_offset(r, inv_d);
    const float s_eps = slab_fma_margin(far_c);
    const bool sx = r.d.x < 0, sy = r.d.y < 0, sz = r.d.z < 0;
    const float lnx = sx ? b[3] : b[0], lny = sy ? b[4] : b[1], lnz = sz ? b[5] : b[2], lfx = sx ? b[0] : b[3], lfy = sy ? b[1] : b[4], lfz = sz ? b[2] : b[5];
    const float rnx = sx ? b[9] : b[6], rny = sy ? b[10] : b[7], rnz = sz ? b[11] : b[8], rfx = sx ? b[6] : b[9], rfy = sy ? b[7] : b[10], rfz = sz ? b[8] : b[11];
    const float tl = slab_near_exact(lnx, lny, lnz, r, inv_d, inv_lo), tr = slab_near_exact(rnx, rny, rnz, r, inv_d, inv_lo);
    float far_l = slab_far_fma(lfx, lfy, lfz, inv_d, far_c), far_r = slab_far_fma(rfx, rfy, rfz, inv_d, far_c);
    const bool unc = far_pair_uncertain_fma(tl, far_l, tr, far_r, s_eps);
    if (unc) { far_l = slab_far_exact(lfx, lfy, lfz, r, inv_d, inv_lo); far_r = slab_far_exact(rfx, rfy, rfz, r, inv_d, inv_lo); }
    const float rec_t = maxd[i];
    const bool hl = tl <= far_l && tl < rec_t && far_l > 0, hr = tr <= far_r && tr < rec_t && far_r > 0;
    c.o[1] = unc; c.o[2] = hl; c.o[3] = hr; c.o[4] = hr && (!hl || tl > tr);
    boxpair_verbatim(c, maxd[i]);
}

static int boxpair_probe(const char* fn, void (*kernel)(size_t, const float*, const float*, const float*, int32_t*), int device, size_t n,
                         const float* boxes, const float* rays, const float* max_dist, int32_t* out) {
    if (!boxes || !rays || !max_dist || !out) return rt_fail(RT_ERR_INVALID, "%s: null argument", fn);
    if (n == 0) return RT_OK;
    ProbeRun p(device);
    auto b = p.in(boxes, 12 * n); auto r = p.in(rays, 6 * n); auto m = p.in(max_dist, n);
    auto o = p.out(out, 8 * n);
    p.launch(kernel, p.per_case(n), 128, n, b, r, m, o);
    return p.finish();
}
extern "C" int rt_probe_boxpair_certified(int device, size_t n, const float* boxes, const float* rays, const float* max_dist, int32_t* out) {
    return boxpair_probe("rt_probe_boxpair_certified", probe_boxpair_certified_kernel, device, n, boxes, rays, max_dist, out);
}
extern "C" int rt_probe_boxpair_certified_fma(int device, size_t n, const float* boxes, const float* rays, const float* max_dist, int32_t* out) {
    return boxpair_probe("rt_probe_boxpair_certified_fma", probe_boxpair_certified_fma_kernel, device, n, boxes, rays, max_dist, out);
}
extern "C" int rt_probe_boxpair_filtered(int device, size_t n, const float* boxes, const float* rays, const float* max_dist, int32_t* out) {
    return boxpair_probe("rt_probe_boxpair_filtered", probe_boxpair_filtered_kernel, device, n, boxes, rays, max_dist, out);
}

// What follows the scene in a launch image ("The launch images"): the light table of a light-sampling mode and the tail of the riders.
// Host code without any device type: the layouts' arithmetic alone, so that tests/cpp_launch_image holds it word for word under sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rt_image {

struct Vec4 { uint32_t x, y, z, w; };   // 16 bytes, the unit of every image: uint4 on the device

inline uint32_t float_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// The light table of `mode`, appended to `out`: a header (n_l, A, -, -), n_l entries (index, area, kind, c_j), — all modes but 1 (quad lights) — n_l more
// (Cx, Cy, Cz, r), zeros for what is no sphere, and — mode 16 (the light tree, §20) with n_l > 0 — 2 n_l - 1 nodes of two vec4: 6 n_l - 1 vec4 in all.
// A = cdf[n_l - 1] and c_j = cdf[j] are written in mode 16 only; an empty mode-16 table (mode 48 on a world without lights, §26) is the header alone.
// index, area, kind: n each; sphere: 4 n; cdf: n and nodes: 8 (2 n - 1), read in mode 16 only.
inline void append_light_table(std::vector<Vec4>& out, uint32_t mode, uint32_t n, const uint32_t* kind, const uint32_t* index, const float* area,
                               const float* sphere, const float* cdf, const float* nodes) {
    const bool tree = mode == 16u;
    const size_t at = out.size(), n_nodes = tree && n ? 2u * (size_t)n - 1u : 0u;
    out.resize(at + 1u + (size_t)n * (mode == 1u ? 1u : 2u) + 2u * n_nodes, Vec4{0u, 0u, 0u, 0u});
    out[at].x = n;
    for (uint32_t i = 0; i < n; i++) {
        out[at + 1u + i] = Vec4{index[i], float_bits(area[i]), kind[i], tree ? float_bits(cdf[i]) : 0u};
        if (mode != 1u) std::memcpy(&out[at + 1u + n + i], sphere + 4u * (size_t)i, 16);
    }
    if (n_nodes) {
        out[at].y = float_bits(cdf[n - 1u]);
        std::memcpy(&out[at + 1u + 2u * (size_t)n], nodes, n_nodes * 32u);
    }
}

// The riders as the tail takes them.  normals: 9 floats per triangle, coords: 6 (NULL = off); the environment record (§23): the map's size, u0, where its
// texel records are on the device and — 0 until a mode that samples the map has built it (§24) — its distribution; the texture table (§25): n_textures entries
// of anything with rt_texture's fields, and where the texels are.
template <typename Texture> struct Riders {
    const float* normals = nullptr; size_t n_normal_floats = 0;
    const float* coords = nullptr; size_t n_coord_floats = 0;
    bool env = false; uint32_t env_w = 0, env_h = 0; float env_u0 = 0.0f; uint64_t env_texels = 0, env_dist = 0;
    bool textures = false; const Texture* texture = nullptr; size_t n_textures = 0; uint64_t texture_texels = 0;
    const void* normal_maps = nullptr; size_t n_normal_maps = 0;   // §28: 16 bytes (on, image, strength bits, -) per material; read only beside a texture table
    const void* microfacets = nullptr; size_t n_microfacets = 0;   // §29: 16 bytes (on, image, roughness bits, specular bits) per material; needs no texture table
    const void* interiors = nullptr; size_t n_interiors = 0;       // §32: 16 bytes (on, sigma bits x 3) per material; needs neither table
    const void* cutouts = nullptr; size_t n_cutouts = 0;           // §34: 16 bytes (on, image, cutoff bits, -) per material; read only beside a texture table
};

// The tail, appended to `out`: a header (normals follow ? 1 : 0, vec4 from the header to the coordinates or 0, ... to the environment record or 0, ... to the
// texture table or 0), then, each from a 16-byte boundary, the normals, the coordinates, the environment record (W, H, u0 bits, -), (texels low, texels high,
// distribution low, distribution high) and the texture table (texels low, texels high, n, -), (W, H, wrap | filter << 8, first texel) per entry.
// Normal maps (§28) hang off the texture table: its header's fourth lane is the number of vec4 from that header to one vec4 (on, image, strength bits, -)
// per material, behind the entries; 0 = none, and the tail is then byte for byte what it was before there were any.
// Microfacet records (§29) come last, one vec4 (on, image, roughness bits, specular bits) per material, and the header's first lane says where: bit 0 is
// "normals follow" as ever, the bits above it are the number of vec4 from the header to the records; 0 = none, and the tail is then byte for byte what it was.
// Only the MFAC forms of the streaming kernel launch on such a tail, and they mask the lane; the feature-pass kernels read the second and fourth lanes alone.
// Interior records (§32): with a table of them the first lane's upper bits count the vec4 to ONE sub-header (vec4 from the header to the microfacet records or 0,
// vec4 from the header to the interior records, -, -), and both tables lie behind it, the microfacet records first.  Only the INTR forms launch on such a tail, and
// they know by template that the sub-header is there; without an interior table the tail is byte for byte what it was.
// Cutout records (§34) lie behind the interior records, and the sub-header's third lane counts the vec4 from the header to them (0 = none).  The sub-header is
// there when there is an interior table or a cutout table; with cutouts alone its second lane is 0.  Only the CUT forms launch on a tail with cutout records;
// without them the tail is byte for byte what it was.
// With everything off it is one zero vec4: the header every kernel reads.
template <typename Texture> inline void append_tail(std::vector<Vec4>& out, const Riders<Texture>& r) {
    const size_t at = out.size();
    const size_t vn_vec4 = r.normals ? (r.n_normal_floats * sizeof(float) + 15u) / 16u : 0u, uv_vec4 = r.coords ? (r.n_coord_floats * sizeof(float) + 15u) / 16u : 0u;
    const size_t uv_at = 1u + vn_vec4, env_at = uv_at + uv_vec4, tex_at = env_at + (r.env ? 2u : 0u);
    const bool nmaps = r.textures && r.normal_maps && r.n_normal_maps;
    const size_t nm_at = 1u + r.n_textures;
    const bool mfacs = r.microfacets && r.n_microfacets;
    const size_t mf_at = tex_at + (r.textures ? 1u + r.n_textures : 0u) + (nmaps ? r.n_normal_maps : 0u);
    const bool intrs = r.interiors && r.n_interiors;
    const bool cuts = r.cutouts && r.n_cutouts;
    const bool sub = intrs || cuts;
    const size_t sub_at = mf_at, mf_rec_at = sub_at + (sub ? 1u : 0u), in_at = mf_rec_at + (mfacs ? r.n_microfacets : 0u), cut_at = in_at + (intrs ? r.n_interiors : 0u);
    out.resize(at + cut_at + (cuts ? r.n_cutouts : 0u), Vec4{0u, 0u, 0u, 0u});
    out[at] = Vec4{(r.normals ? 1u : 0u) | (mfacs || sub ? (uint32_t)sub_at << 1 : 0u), r.coords ? (uint32_t)uv_at : 0u, r.env ? (uint32_t)env_at : 0u, r.textures ? (uint32_t)tex_at : 0u};
    if (r.normals) std::memcpy(&out[at + 1u], r.normals, r.n_normal_floats * sizeof(float));
    if (r.coords) std::memcpy(&out[at + uv_at], r.coords, r.n_coord_floats * sizeof(float));
    if (r.env) {
        out[at + env_at] = Vec4{r.env_w, r.env_h, float_bits(r.env_u0), 0u};
        out[at + env_at + 1u] = Vec4{(uint32_t)r.env_texels, (uint32_t)(r.env_texels >> 32), (uint32_t)r.env_dist, (uint32_t)(r.env_dist >> 32)};
    }
    if (r.textures) {
        out[at + tex_at] = Vec4{(uint32_t)r.texture_texels, (uint32_t)(r.texture_texels >> 32), (uint32_t)r.n_textures, nmaps ? (uint32_t)nm_at : 0u};
        if (nmaps) std::memcpy(&out[at + tex_at + nm_at], r.normal_maps, r.n_normal_maps * 16u);
        for (size_t k = 0; k < r.n_textures; k++)
            out[at + tex_at + 1u + k] = Vec4{r.texture[k].width, r.texture[k].height, r.texture[k].wrap | r.texture[k].filter << 8, r.texture[k].first};
    }
    if (mfacs) std::memcpy(&out[at + mf_rec_at], r.microfacets, r.n_microfacets * 16u);
    if (sub) out[at + sub_at] = Vec4{mfacs ? (uint32_t)mf_rec_at : 0u, intrs ? (uint32_t)in_at : 0u, cuts ? (uint32_t)cut_at : 0u, 0u};
    if (intrs) std::memcpy(&out[at + in_at], r.interiors, r.n_interiors * 16u);
    if (cuts) std::memcpy(&out[at + cut_at], r.cutouts, r.n_cutouts * 16u);
}

}   // namespace rt_image

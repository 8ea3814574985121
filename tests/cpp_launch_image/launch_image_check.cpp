// The two layouts of csrc/rt_launch_image.hpp, word for word, against arrays written out by hand from DESIGN.md §6 ("The launch images").
// Built with -fsanitize=address,undefined: a builder that writes or reads past what the layout says ends the program.
#include "rt_launch_image.hpp"

#include <cstdio>

using rt_image::Vec4;
struct Texture { uint32_t width, height, wrap, filter, first; };   // the fields of rt_texture

static const Vec4 SENTINEL = {0xdeadbeefu, 0xfeedfaceu, 0x0badf00du, 0xcafef00du};   // what `out` held before: both builders append
static int failures = 0;

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static void check(const char* name, const std::vector<Vec4>& got, const std::vector<Vec4>& want) {
    bool ok = got.size() == want.size() + 1u && std::memcmp(&got[0], &SENTINEL, 16) == 0;
    for (size_t i = 0; ok && i < want.size(); i++)
        if (std::memcmp(&got[i + 1u], &want[i], 16) != 0) {
            std::printf("%s: vec4 %zu is (%#x, %#x, %#x, %#x), expected (%#x, %#x, %#x, %#x)\n", name, i, got[i + 1u].x, got[i + 1u].y, got[i + 1u].z, got[i + 1u].w,
                        want[i].x, want[i].y, want[i].z, want[i].w);
            ok = false;
        }
    if (!ok) { std::printf("%s: FAILED (%zu vec4 behind the sentinel, expected %zu)\n", name, got.size() - 1u, want.size()); failures++; }
}

static std::vector<Vec4> tail(const rt_image::Riders<Texture>& r) {
    std::vector<Vec4> out(1, SENTINEL);
    rt_image::append_tail(out, r);
    return out;
}

static std::vector<Vec4> lights(uint32_t mode, uint32_t n, const uint32_t* kind, const uint32_t* index, const float* area, const float* sphere, const float* cdf,
                                const float* nodes) {
    std::vector<Vec4> out(1, SENTINEL);
    rt_image::append_light_table(out, mode, n, kind, index, area, sphere, cdf, nodes);
    return out;
}

int main() {
    // ---- the tail ----------------------------------------------------------------------------------------------------------------------------------------
    // normal float i has the bits 0x40000000 + i, coordinate float i the bits 0x41000000 + i: exactly sized arrays, so that a read past them is caught
    std::vector<float> normals27(27), coords18(18);
    for (uint32_t i = 0; i < 27u; i++) normals27[i] = from_bits(0x40000000u + i);
    for (uint32_t i = 0; i < 18u; i++) coords18[i] = from_bits(0x41000000u + i);
    const std::vector<float> normals9(normals27.begin(), normals27.begin() + 9), coords6(coords18.begin(), coords18.begin() + 6);
    const std::vector<Texture> two = {{5u, 3u, 1u, 1u, 0u}, {8u, 4u, 0u, 1u, 15u}};

    check("tail: nothing on", tail({}), {{0u, 0u, 0u, 0u}});
    {
        rt_image::Riders<Texture> r;
        r.normals = normals9.data(); r.n_normal_floats = 9;
        check("tail: normals only", tail(r), {{1u, 0u, 0u, 0u},
              {0x40000000u, 0x40000001u, 0x40000002u, 0x40000003u}, {0x40000004u, 0x40000005u, 0x40000006u, 0x40000007u}, {0x40000008u, 0u, 0u, 0u}});
    }
    {
        rt_image::Riders<Texture> r;
        r.coords = coords6.data(); r.n_coord_floats = 6;
        check("tail: coordinates only", tail(r), {{0u, 1u, 0u, 0u}, {0x41000000u, 0x41000001u, 0x41000002u, 0x41000003u}, {0x41000004u, 0x41000005u, 0u, 0u}});
    }
    for (const uint64_t dist : {0x0ull, 0x00007f00deadbee0ull}) {
        rt_image::Riders<Texture> r;
        r.normals = normals27.data(); r.n_normal_floats = 27;
        r.coords = coords18.data(); r.n_coord_floats = 18;
        r.env = true; r.env_w = 16u; r.env_h = 8u; r.env_u0 = 0.125f; r.env_texels = 0x0000001234567890ull; r.env_dist = dist;
        r.textures = true; r.texture = two.data(); r.n_textures = 2; r.texture_texels = 0x00000abcdef01230ull;
        const Vec4 pointers = dist ? Vec4{0x34567890u, 0x00000012u, 0xdeadbee0u, 0x00007f00u} : Vec4{0x34567890u, 0x00000012u, 0u, 0u};
        check(dist ? "tail: all four, with a distribution" : "tail: all four", tail(r), {
            {1u, 8u, 13u, 15u},
            {0x40000000u, 0x40000001u, 0x40000002u, 0x40000003u}, {0x40000004u, 0x40000005u, 0x40000006u, 0x40000007u},     // 1: 27 floats in 7 vec4
            {0x40000008u, 0x40000009u, 0x4000000au, 0x4000000bu}, {0x4000000cu, 0x4000000du, 0x4000000eu, 0x4000000fu},
            {0x40000010u, 0x40000011u, 0x40000012u, 0x40000013u}, {0x40000014u, 0x40000015u, 0x40000016u, 0x40000017u},
            {0x40000018u, 0x40000019u, 0x4000001au, 0u},
            {0x41000000u, 0x41000001u, 0x41000002u, 0x41000003u}, {0x41000004u, 0x41000005u, 0x41000006u, 0x41000007u},     // 8: 18 floats in 5 vec4
            {0x41000008u, 0x41000009u, 0x4100000au, 0x4100000bu}, {0x4100000cu, 0x4100000du, 0x4100000eu, 0x4100000fu},
            {0x41000010u, 0x41000011u, 0u, 0u},
            {16u, 8u, 0x3e000000u, 0u}, pointers,                                                                             // 13: the environment record
            {0xdef01230u, 0x00000abcu, 2u, 0u}, {5u, 3u, 0x00000101u, 0u}, {8u, 4u, 0x00000100u, 15u}});                  // 15: the texture table
    }

    // ---- the light tables --------------------------------------------------------------------------------------------------------------------------------
    // three lights: a quad (kind 0), a sphere (kind 1) at (1, 2, 3) of radius 0.5, a triangle (kind 2); areas 2, 4, 3; running sums 2, 6, 9
    const uint32_t kind[3] = {0u, 1u, 2u}, index[3] = {3u, 9u, 5u};
    const float area[3] = {2.0f, 4.0f, 3.0f}, sphere[12] = {0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 2.0f, 3.0f, 0.5f, 0.0f, 0.0f, 0.0f, 0.0f}, cdf[3] = {2.0f, 6.0f, 9.0f};
    std::vector<float> nodes(40);   // five nodes of eight floats: float i has the bits 0x42000000 + i
    for (uint32_t i = 0; i < 40u; i++) nodes[i] = from_bits(0x42000000u + i);
    const std::vector<float> one_node(nodes.begin(), nodes.begin() + 8);
    const float cdf1[1] = {2.0f};

    check("lights: mode 1, two", lights(1u, 2u, kind, index, area, sphere, nullptr, nullptr), {{2u, 0u, 0u, 0u}, {3u, 0x40000000u, 0u, 0u}, {9u, 0x40800000u, 1u, 0u}});
    check("lights: mode 2, two", lights(2u, 2u, kind, index, area, sphere, nullptr, nullptr),
          {{2u, 0u, 0u, 0u}, {3u, 0x40000000u, 0u, 0u}, {9u, 0x40800000u, 1u, 0u}, {0u, 0u, 0u, 0u}, {0x3f800000u, 0x40000000u, 0x40400000u, 0x3f000000u}});
    check("lights: mode 16, none", lights(16u, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), {{0u, 0u, 0u, 0u}});
    check("lights: mode 16, one", lights(16u, 1u, kind, index, area, sphere, cdf1, one_node.data()),
          {{1u, 0x40000000u, 0u, 0u}, {3u, 0x40000000u, 0u, 0x40000000u}, {0u, 0u, 0u, 0u},
           {0x42000000u, 0x42000001u, 0x42000002u, 0x42000003u}, {0x42000004u, 0x42000005u, 0x42000006u, 0x42000007u}});
    check("lights: mode 16, three", lights(16u, 3u, kind, index, area, sphere, cdf, nodes.data()), {
        {3u, 0x41100000u, 0u, 0u},                                                                                               // A = cdf[2] = 9
        {3u, 0x40000000u, 0u, 0x40000000u}, {9u, 0x40800000u, 1u, 0x40c00000u}, {5u, 0x40400000u, 2u, 0x41100000u},        // c_j = 2, 6, 9
        {0u, 0u, 0u, 0u}, {0x3f800000u, 0x40000000u, 0x40400000u, 0x3f000000u}, {0u, 0u, 0u, 0u},
        {0x42000000u, 0x42000001u, 0x42000002u, 0x42000003u}, {0x42000004u, 0x42000005u, 0x42000006u, 0x42000007u},       // 2 * 3 - 1 = 5 nodes
        {0x42000008u, 0x42000009u, 0x4200000au, 0x4200000bu}, {0x4200000cu, 0x4200000du, 0x4200000eu, 0x4200000fu},
        {0x42000010u, 0x42000011u, 0x42000012u, 0x42000013u}, {0x42000014u, 0x42000015u, 0x42000016u, 0x42000017u},
        {0x42000018u, 0x42000019u, 0x4200001au, 0x4200001bu}, {0x4200001cu, 0x4200001du, 0x4200001eu, 0x4200001fu},
        {0x42000020u, 0x42000021u, 0x42000022u, 0x42000023u}, {0x42000024u, 0x42000025u, 0x42000026u, 0x42000027u}});   // 17 = 6 * 3 - 1 vec4
    check("lights: mode 4, three", lights(4u, 3u, kind, index, area, sphere, nullptr, nullptr), {
        {3u, 0u, 0u, 0u}, {3u, 0x40000000u, 0u, 0u}, {9u, 0x40800000u, 1u, 0u}, {5u, 0x40400000u, 2u, 0u},
        {0u, 0u, 0u, 0u}, {0x3f800000u, 0x40000000u, 0x40400000u, 0x3f000000u}, {0u, 0u, 0u, 0u}});
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

// The tail of csrc/rt_launch_image.hpp with a cutout table, word for word, against arrays written out by hand: the cutout records lie behind the
// interior records, the sub-header's third lane counts the vec4 from the header to them, and the sub-header is there when there is an interior table or a cutout
// table — and without a cutout table the tail is what tests/cpp_launch_image, §29 and §32 hold it to.  Built with -fsanitize=address,undefined: a builder
// that writes or reads past what the layout says ends the program.
#include "rt_launch_image.hpp"

#include <cstdio>

using rt_image::Vec4;
struct Texture { uint32_t width, height, wrap, filter, first; };   // the fields of rt_texture

static const Vec4 SENTINEL = {0xdeadbeefu, 0xfeedfaceu, 0x0badf00du, 0xcafef00du};   // what `out` held before: the builder appends
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

int main() {
    // record k of a table has the words base + 4 k ... base + 4 k + 3: exactly sized arrays, so that a read past them is caught
    auto records = [](uint32_t base, uint32_t n) { std::vector<Vec4> v(n); for (uint32_t k = 0; k < n; k++) v[k] = Vec4{base + 4u * k, base + 4u * k + 1u, base + 4u * k + 2u, base + 4u * k + 3u}; return v; };
    const std::vector<Vec4> mf2 = records(0x50000000u, 2), in2 = records(0x60000000u, 2), cut2 = records(0x80000000u, 2);
    const std::vector<Vec4> nm3 = records(0x70000000u, 3), mf3 = records(0x50000000u, 3), in3 = records(0x60000000u, 3), cut3 = records(0x80000000u, 3);
    std::vector<float> normals9(9), coords6(6);
    for (uint32_t i = 0; i < 9u; i++) normals9[i] = from_bits(0x40000000u + i);
    for (uint32_t i = 0; i < 6u; i++) coords6[i] = from_bits(0x41000000u + i);
    const std::vector<Texture> two = {{5u, 3u, 1u, 1u, 0u}, {8u, 4u, 0u, 1u, 15u}};

    rt_image::Riders<Texture> defaults;
    if (defaults.cutouts != nullptr || defaults.n_cutouts != 0u) { std::printf("Riders: the cutout field has a default of none\n"); failures++; }
    {   // without a cutout table: the older tails, byte for byte
        rt_image::Riders<Texture> r;
        check("tail: nothing", tail(r), {{0u, 0u, 0u, 0u}});
        r.microfacets = mf2.data(); r.n_microfacets = 2;
        check("tail: microfacets, no cutouts", tail(r), {{1u << 1, 0u, 0u, 0u}, mf2[0], mf2[1]});
        r.cutouts = cut2.data(); r.n_cutouts = 0;   // a table of no records is no table
        check("tail: microfacets, an empty cutout table", tail(r), {{1u << 1, 0u, 0u, 0u}, mf2[0], mf2[1]});
        r.cutouts = nullptr;
        r.interiors = in2.data(); r.n_interiors = 2;
        check("tail: microfacets and interiors, no cutouts", tail(r), {{1u << 1, 0u, 0u, 0u}, {2u, 4u, 0u, 0u}, mf2[0], mf2[1], in2[0], in2[1]});
        r.microfacets = nullptr; r.n_microfacets = 0;
        check("tail: interiors alone", tail(r), {{1u << 1, 0u, 0u, 0u}, {0u, 2u, 0u, 0u}, in2[0], in2[1]});
    }
    {   // cutouts alone: the sub-header is there, its first two lanes say "none"
        rt_image::Riders<Texture> r;
        r.cutouts = cut2.data(); r.n_cutouts = 2;
        check("tail: cutouts alone", tail(r), {{1u << 1, 0u, 0u, 0u}, {0u, 0u, 2u, 0u}, cut2[0], cut2[1]});
        r.interiors = in2.data(); r.n_interiors = 2;
        check("tail: interiors and cutouts", tail(r), {{1u << 1, 0u, 0u, 0u}, {0u, 2u, 4u, 0u}, in2[0], in2[1], cut2[0], cut2[1]});
        r.microfacets = mf2.data(); r.n_microfacets = 2;
        check("tail: microfacets, interiors and cutouts", tail(r), {{1u << 1, 0u, 0u, 0u}, {2u, 4u, 6u, 0u}, mf2[0], mf2[1], in2[0], in2[1], cut2[0], cut2[1]});
        r.interiors = nullptr; r.n_interiors = 0;
        check("tail: microfacets and cutouts", tail(r), {{1u << 1, 0u, 0u, 0u}, {2u, 0u, 4u, 0u}, mf2[0], mf2[1], cut2[0], cut2[1]});
    }
    {   // everything before them too: normals (9 floats in 3 vec4), coordinates (6 floats in 2 vec4), a texture table of two entries with three normal-map records
        rt_image::Riders<Texture> r;
        r.normals = normals9.data(); r.n_normal_floats = 9;
        r.coords = coords6.data(); r.n_coord_floats = 6;
        r.textures = true; r.texture = two.data(); r.n_textures = 2; r.texture_texels = 0x00000abcdef01230ull;
        r.normal_maps = nm3.data(); r.n_normal_maps = 3;
        r.microfacets = mf3.data(); r.n_microfacets = 3;
        r.interiors = in3.data(); r.n_interiors = 3;
        r.cutouts = cut3.data(); r.n_cutouts = 3;
        const std::vector<Vec4> front = {
            {1u | 12u << 1, 4u, 0u, 6u},
            {0x40000000u, 0x40000001u, 0x40000002u, 0x40000003u}, {0x40000004u, 0x40000005u, 0x40000006u, 0x40000007u}, {0x40000008u, 0u, 0u, 0u},   // 1: the normals
            {0x41000000u, 0x41000001u, 0x41000002u, 0x41000003u}, {0x41000004u, 0x41000005u, 0u, 0u},                                                // 4: the coordinates
            {0xdef01230u, 0x00000abcu, 2u, 3u}, {5u, 3u, 0x00000101u, 0u}, {8u, 4u, 0x00000100u, 15u}, nm3[0], nm3[1], nm3[2]};                      // 6: the texture table
        std::vector<Vec4> want = front;
        want.insert(want.end(), {{13u, 16u, 19u, 0u},                                                                                                // 12: the sub-header
                                 mf3[0], mf3[1], mf3[2], in3[0], in3[1], in3[2], cut3[0], cut3[1], cut3[2]});
        check("tail: normals, coordinates, textures, normal maps, microfacets, interiors, cutouts", tail(r), want);
        r.cutouts = nullptr; r.n_cutouts = 0;   // ... and the same riders without the table: §32's tail
        want = front;
        want.insert(want.end(), {{13u, 16u, 0u, 0u}, mf3[0], mf3[1], mf3[2], in3[0], in3[1], in3[2]});
        check("tail: the same without cutouts", tail(r), want);
        r.interiors = nullptr; r.n_interiors = 0;   // ... and without either: no sub-header, the records at 12
        want = front;
        want.insert(want.end(), {mf3[0], mf3[1], mf3[2]});
        check("tail: the same without interiors and cutouts", tail(r), want);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

// aov_textured_app.cpp — a viewer's loop step on a textured world, written against include/rt06/rt06.hpp: a sphere, a tiled floor and a UV-mapped triangle under
// three images (SceneBuilder::AddImage), EnableAOV(0, AovMode::Textured), Refine, Denoise.
//
//   aov_textured_app W H DEPTH N PREFIX   refuses the plain mode first (and says so), then Refine(N) with the textured feature buffers on and Denoise() with the
//                                         default parameters; writes PREFIX_aov.f32 (W*H*8 floats, unscaled sums) and PREFIX_denoised.f32.
// tests/test_gpu_aov_textured.py builds the same world through Python and compares the two files with what the C ABI gives there, byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt06/rt06.hpp"

static void write_file(const std::string& path, const std::vector<glm::vec4>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    std::fwrite(v.data(), sizeof(glm::vec4), v.size(), f);
    std::fclose(f);
}

// a computed w x h image: red grows to the right, green downwards, blue alternates
static std::vector<uint8_t> image(uint32_t w, uint32_t h, uint32_t salt) {
    std::vector<uint8_t> px;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) { px.push_back((uint8_t)(40u + 200u * x / w)); px.push_back((uint8_t)(30u + 180u * y / h)); px.push_back((uint8_t)(((x + y + salt) & 1u) ? 220u : 60u)); }
    return px;
}

int main(int argc, char** argv) {
    try {
        if (argc < 6) {
            std::fprintf(stderr, "usage: aov_textured_app W H DEPTH N PREFIX\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), depth = (uint32_t)std::atoi(argv[3]);
        const uint32_t n = (uint32_t)std::atoi(argv[4]);
        const std::string prefix = argv[5];
        rt06::SceneBuilder b;
        const std::vector<uint8_t> globe = image(8, 4, 0), tiles = image(2, 2, 1), atlas = image(5, 3, 0);
        rt06::check(rt_scene_set_image(b.get(), 8, 4, globe.data()), "rt_scene_set_image");   // entry 0, the world's own image
        const uint32_t i_tiles = b.AddImage(2, 2, tiles.data(), RT_WRAP_REPEAT, RT_FILTER_NEAREST);
        const uint32_t i_atlas = b.AddImage(5, 3, atlas.data(), RT_WRAP_CLAMP, RT_FILTER_BILINEAR);
        ImageTextureAbstract<Quad> m_globe, m_tiles(i_tiles), m_atlas(i_atlas);
        const int32_t globe_mat = b.material(&m_globe), tiles_mat = b.material(&m_tiles), atlas_mat = b.material(&m_atlas);
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, tiles_mat, nullptr), "floor");
        const float c[3] = {-1.2f, 1.0f, 0.0f};
        rt06::check(rt_scene_add_sphere(b.get(), c, 1.0f, globe_mat, nullptr), "sphere");
        const float ta[3] = {0.5f, 0.1f, 0.5f}, tb[3] = {3.0f, 0.1f, 0.0f}, tc[3] = {1.5f, 2.6f, 0.2f};
        const float ua[2] = {-0.5f, 0.0f}, ub[2] = {1.5f, 0.25f}, uc[2] = {0.5f, 1.5f};
        rt06::check(rt_scene_add_triangle_uv(b.get(), ta, tb, tc, nullptr, nullptr, nullptr, ua, ub, uc, atlas_mat, nullptr), "triangle");
        const float sky[3] = {0.6f, 0.7f, 0.9f};
        rt06::check(rt_scene_set_background(b.get(), 1, sky), "background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(0.5f, 2.5f, 7), glm::vec3(0, 1.0f, 0), glm::vec3(0, 1, 0), 50.0f, width / (float)height);
        {
            Renderer renderer = Renderer::MakeRenderer(width, height, n, depth, &cam, &world);
            try {
                renderer.EnableAOV();
                std::printf("plain: enabled\n");
            } catch (const std::exception& e) {
                std::printf("plain: refused (%s)\n", std::strstr(e.what(), "RT_MAT_LAMBERTIAN_IMAGE") ? "names RT_MAT_LAMBERTIAN_IMAGE" : e.what());
            }
            renderer.EnableAOV(0, AovMode::Textured);
            std::printf("mode=%s\n", renderer.AOVMode() == AovMode::Textured ? "textured" : "plain");
            renderer.Refine(n);
            renderer.Denoise();
            std::vector<glm::vec4> aov((size_t)width * height * 2), den((size_t)width * height);
            renderer.DownloadAOV(aov.data());
            renderer.DownloadDenoised(den.data());
            write_file(prefix + "_aov.f32", aov);
            write_file(prefix + "_denoised.f32", den);
            std::printf("samples=%llu\n", (unsigned long long)renderer.SamplesAccumulated());
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

// aov_full_app.cpp — a viewer's loop step on a world the first two feature modes refuse, written against include/rt06/rt06.hpp: a floor, a ball, a fence under a
// checker mask (SceneBuilder::SetCutout) and a constant medium in front of them, EnableAOV(0, AovMode::Full), Refine, Denoise.
//
//   aov_full_app W H DEPTH N PREFIX   tries the plain and the textured mode first (and says what they answer), then Refine(N) with the full feature buffers on and
//                                     Denoise() with the default parameters; writes PREFIX_aov.f32 (W*H*8 floats, unscaled sums) and PREFIX_denoised.f32; then
//                                     takes the cutout table away under the same buffers and writes PREFIX_solid_aov.f32.
// tests/test_cpp_aov_full.py builds the same world through Python and compares the files with what the C ABI gives there, byte for byte.
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

int main(int argc, char** argv) {
    try {
        if (argc < 6) {
            std::fprintf(stderr, "usage: aov_full_app W H DEPTH N PREFIX\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), depth = (uint32_t)std::atoi(argv[3]);
        const uint32_t n = (uint32_t)std::atoi(argv[4]);
        const std::string prefix = argv[5];
        rt06::SceneBuilder b;
        LambertianAbstract<Quad> m_floor(glm::vec3(0.5f, 0.5f, 0.5f)), m_fence(glm::vec3(0.7f, 0.5f, 0.3f));
        MetalAbstract<Quad> m_ball(glm::vec3(0.8f, 0.8f, 0.9f), 0.1f);
        IsotropicAbstract<Quad> m_fog(glm::vec3(0.8f, 0.85f, 0.9f), 0.3f);
        const int32_t floor_mat = b.material(&m_floor), fence_mat = b.material(&m_fence), ball_mat = b.material(&m_ball), fog_mat = b.material(&m_fog);
        std::vector<uint8_t> mask(8u * 4u * 3u);   // an 8 x 4 checker of opaque and empty texels
        for (uint32_t j = 0; j < 4u; j++)
            for (uint32_t i = 0; i < 8u; i++)
                for (uint32_t c = 0; c < 3u; c++) mask[(j * 8u + i) * 3u + c] = ((i + j) & 1u) ? 255u : 0u;
        const uint32_t image = b.AddImage(8, 4, mask.data(), RT_WRAP_CLAMP, RT_FILTER_NEAREST);
        b.SetCutout((uint32_t)fence_mat, image);
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, floor_mat, nullptr), "floor");
        const float fq[3] = {-3, 0, 2}, fu[3] = {6, 0, 0}, fv[3] = {0, 3, 0};
        rt06::check(rt_scene_add_quad(b.get(), fq, fu, fv, fence_mat, nullptr), "fence");
        const float c1[3] = {0.0f, 1.0f, 0.0f}, c2[3] = {1.0f, 1.5f, 3.5f};
        rt06::check(rt_scene_add_sphere(b.get(), c1, 1.0f, ball_mat, nullptr), "ball");
        rt06::check(rt_scene_add_sphere(b.get(), c2, 1.4f, fog_mat, nullptr), "fog");
        const float sky[3] = {0.6f, 0.7f, 0.9f};
        rt06::check(rt_scene_set_background(b.get(), 1, sky), "background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(0.5f, 2.0f, 7), glm::vec3(0, 1.0f, 0), glm::vec3(0, 1, 0), 50.0f, width / (float)height);
        Renderer renderer = Renderer::MakeRenderer(width, height, n, depth, &cam, &world);
        for (AovMode mode : {AovMode::Plain, AovMode::Textured}) {
            const char* name = mode == AovMode::Plain ? "plain" : "textured";
            try {
                renderer.EnableAOV(0, mode);
                std::printf("%s: enabled\n", name);
            } catch (const std::exception& e) {
                std::printf("%s: refused (%s)\n", name, std::strstr(e.what(), "cutout table") ? "names the cutout table" : e.what());
            }
        }
        renderer.EnableAOV(0, AovMode::Full);
        std::printf("mode=%s\n", renderer.AOVMode() == AovMode::Full ? "full" : "other");
        renderer.Refine(n);
        renderer.Denoise();
        std::vector<glm::vec4> aov((size_t)width * height * 2), den((size_t)width * height);
        renderer.DownloadAOV(aov.data());
        renderer.DownloadDenoised(den.data());
        write_file(prefix + "_aov.f32", aov);
        write_file(prefix + "_denoised.f32", den);
        std::printf("samples=%llu\n", (unsigned long long)renderer.SamplesAccumulated());
        renderer.SetCutouts(nullptr, 0);   // accepted under mode Full: colour and features restart together
        std::printf("after the table: samples=%llu mode=%s\n", (unsigned long long)renderer.SamplesAccumulated(), renderer.AOVMode() == AovMode::Full ? "full" : "other");
        renderer.Refine(n);
        renderer.DownloadAOV(aov.data());
        write_file(prefix + "_solid_aov.f32", aov);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

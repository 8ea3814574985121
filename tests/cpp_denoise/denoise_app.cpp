// denoise_app.cpp — a viewer's loop step written against include/rt06/rt06.hpp: Cornell box, EnableAOV, Refine, Denoise.
//
//   denoise_app W H DEPTH N PREFIX   Refine(N) with the feature buffers on, Denoise() with the default parameters; writes PREFIX_frame.f32
//                                    (the refined frame), PREFIX_aov.f32 (W*H*8 floats, unscaled sums) and PREFIX_denoised.f32.
// tests/test_gpu_denoise_tools.py compares the three files with what the C ABI gives through Python, byte for byte.
#include <cstdio>
#include <cstdlib>
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
            std::fprintf(stderr, "usage: denoise_app W H DEPTH N PREFIX\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), depth = (uint32_t)std::atoi(argv[3]);
        const uint32_t n = (uint32_t)std::atoi(argv[4]);
        const std::string prefix = argv[5];
        rt_scene* scene = nullptr;
        rt06::check(rt_scene_cornell_box(&scene), "rt_scene_cornell_box");
        BVH world(scene);
        PinholeCamera cam(glm::vec3(278, 278, -800), glm::vec3(278, 278, 0), glm::vec3(0, 1, 0), 40.0f, width / (float)height);
        {
            Renderer renderer = Renderer::MakeRenderer(width, height, n, depth, &cam, &world);
            renderer.EnableAOV();
            renderer.Refine(n);
            renderer.Denoise();
            std::vector<glm::vec4> frame((size_t)width * height), aov((size_t)width * height * 2), den((size_t)width * height);
            renderer.DownloadRenderbuffer(frame.data());
            renderer.DownloadAOV(aov.data());
            renderer.DownloadDenoised(den.data());
            write_file(prefix + "_frame.f32", frame);
            write_file(prefix + "_aov.f32", aov);
            write_file(prefix + "_denoised.f32", den);
            std::printf("samples=%llu\n", (unsigned long long)renderer.SamplesAccumulated());
        }
        rt_scene_destroy(scene);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

// cutouts_app.cpp — a floor, a ball and a fence in front of them, rendered through include/rt06/rt06.hpp.
//
//   cutouts_app W H SPP DEPTH   builds the world with SceneBuilder::SetCutout over a mask added with rt_scene_add_image; MakeRenderer pushes the scene's texture
//                               table and its cutout table; renders and prints a hash of the frame, then takes the cutout table away and prints the hash of
//                               that frame — a solid card — too.
// tests/test_cpp_cutouts.py builds the same world through Python and compares both hashes with the C ABI's frames.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt06/rt06.hpp"

static uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char** argv) {
    try {
        if (argc < 5) {
            std::fprintf(stderr, "usage: cutouts_app W H SPP DEPTH\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
        rt06::SceneBuilder b;
        LambertianAbstract<Quad> m_floor(glm::vec3(0.5f, 0.5f, 0.5f)), m_fence(glm::vec3(0.7f, 0.5f, 0.3f));
        MetalAbstract<Quad> m_ball(glm::vec3(0.8f, 0.8f, 0.9f), 0.1f);
        const int32_t floor_mat = b.material(&m_floor), fence_mat = b.material(&m_fence), ball_mat = b.material(&m_ball);
        std::vector<uint8_t> mask(8u * 4u * 3u);   // an 8 x 4 checker of opaque and empty texels
        for (uint32_t j = 0; j < 4u; j++)
            for (uint32_t i = 0; i < 8u; i++)
                for (uint32_t c = 0; c < 3u; c++) mask[(j * 8u + i) * 3u + c] = ((i + j) & 1u) ? 255u : 0u;
        uint32_t image = 0;
        rt06::check(rt_scene_add_image(b.get(), 8, 4, mask.data(), RT_WRAP_CLAMP, RT_FILTER_NEAREST, &image), "rt_scene_add_image");
        b.SetCutout((uint32_t)fence_mat, image, 0.9f);
        b.SetCutout((uint32_t)fence_mat, image);   // the last call counts: cutoff 1/2
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, floor_mat, nullptr), "floor");
        const float fq[3] = {-3, 0, 2}, fu[3] = {6, 0, 0}, fv[3] = {0, 3, 0};
        rt06::check(rt_scene_add_quad(b.get(), fq, fu, fv, fence_mat, nullptr), "fence");
        const float c1[3] = {0.0f, 1.0f, 0.0f};
        rt06::check(rt_scene_add_sphere(b.get(), c1, 1.0f, ball_mat, nullptr), "ball");
        const float sky[3] = {0.6f, 0.7f, 0.9f};
        rt06::check(rt_scene_set_background(b.get(), 1, sky), "background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        const rt_cutout* table = nullptr;
        if (b.Cutouts(&table) != 3u || table[fence_mat].on != RT_CUTOUT_MASKED || table[fence_mat].image != image || table[fence_mat].cutoff != 0.5f ||
            table[floor_mat].on != RT_CUTOUT_OFF || table[ball_mat].on != RT_CUTOUT_OFF)
            throw std::runtime_error("three materials, one cutout record");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(0.5f, 2.0f, 7), glm::vec3(0, 1.0f, 0), glm::vec3(0, 1, 0), 50.0f, width / (float)height);
        Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
        std::vector<glm::vec4> fb((size_t)width * height);
        renderer.Render();
        renderer.DownloadRenderbuffer(fb.data());
        std::printf("cutouts %ux%u spp=%u depth=%u fnv=%016llx\n", width, height, spp, depth, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        renderer.SetCutouts(nullptr, 0);
        renderer.Render();
        renderer.DownloadRenderbuffer(fb.data());
        std::printf("off: fnv=%016llx\n", (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        b.ClearCutout((uint32_t)fence_mat);
        if (b.Cutouts(&table) != 0u || table != nullptr) throw std::runtime_error("cleared records leave no table");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

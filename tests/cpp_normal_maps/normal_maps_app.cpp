// normal_maps_app.cpp — a floor and two balls with computed normal maps, rendered through include/rt06/rt06.hpp.
//
//   normal_maps_app W H SPP DEPTH   builds the world with SceneBuilder::AddImage and SceneBuilder::SetNormalMap; MakeRenderer pushes the scene's texture table and
//                                   its normal-map table (Renderer::SetTextures, Renderer::SetNormalMaps); renders and prints a hash of the frame, then takes the
//                                   normal-map table away and prints the hash of that frame too.
// tests/test_cpp_normal_maps.py builds the same world through Python and compares both hashes with the C ABI's frames.
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

// a computed w x h normal map in integers: x and y lean by the texel's position, z stays high
static std::vector<uint8_t> bumps(uint32_t w, uint32_t h, uint32_t salt) {
    std::vector<uint8_t> px;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) { px.push_back((uint8_t)(88u + 80u * ((x + salt) % 2u))); px.push_back((uint8_t)(98u + 60u * ((y + salt) % 2u))); px.push_back((uint8_t)(230u + x % 3u)); }
    return px;
}

int main(int argc, char** argv) {
    try {
        if (argc < 5) {
            std::fprintf(stderr, "usage: normal_maps_app W H SPP DEPTH\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
        rt06::SceneBuilder b;
        const std::vector<uint8_t> coarse = bumps(4, 4, 0), fine = bumps(8, 6, 1);
        const uint32_t i_coarse = b.AddImage(4, 4, coarse.data(), RT_WRAP_REPEAT, RT_FILTER_BILINEAR);
        const uint32_t i_fine = b.AddImage(8, 6, fine.data(), RT_WRAP_REPEAT, RT_FILTER_NEAREST);
        LambertianAbstract<Quad> m_floor(glm::vec3(0.5f, 0.5f, 0.5f)), m_ball(glm::vec3(0.7f, 0.3f, 0.3f));
        MetalAbstract<Quad> m_metal(glm::vec3(0.8f, 0.8f, 0.8f), 0.2f);
        const int32_t floor_mat = b.material(&m_floor), ball_mat = b.material(&m_ball), metal_mat = b.material(&m_metal);
        b.SetNormalMap((uint32_t)floor_mat, i_fine, 0.5f);
        b.SetNormalMap((uint32_t)ball_mat, i_coarse);
        b.SetNormalMap((uint32_t)metal_mat, i_fine, 2.0f);
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, floor_mat, nullptr), "floor");
        const float c1[3] = {-1.2f, 1.0f, 0.0f}, c2[3] = {1.3f, 1.0f, 0.5f};
        rt06::check(rt_scene_add_sphere(b.get(), c1, 1.0f, ball_mat, nullptr), "ball");
        rt06::check(rt_scene_add_sphere(b.get(), c2, 1.0f, metal_mat, nullptr), "metal ball");
        const float sky[3] = {0.6f, 0.7f, 0.9f};
        rt06::check(rt_scene_set_background(b.get(), 1, sky), "background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        const rt_normal_map* table = nullptr;
        if (b.NormalMaps(&table) != 3u) throw std::runtime_error("three materials, three records");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(0.5f, 2.5f, 7), glm::vec3(0, 1.0f, 0), glm::vec3(0, 1, 0), 50.0f, width / (float)height);
        Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
        std::vector<glm::vec4> fb((size_t)width * height);
        renderer.Render();
        renderer.DownloadRenderbuffer(fb.data());
        std::printf("normal maps %ux%u spp=%u depth=%u fnv=%016llx\n", width, height, spp, depth, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        renderer.SetNormalMaps(nullptr, 0);
        renderer.Render();
        renderer.DownloadRenderbuffer(fb.data());
        std::printf("off: fnv=%016llx\n", (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

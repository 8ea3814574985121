// env_tree_app.cpp — three spheres on a floor under an environment map with a small sun AND a quad light and a triangle lamp, rendered through
// include/rt06/rt06.hpp with the map and the light tree sampled together.
//
//   env_tree_app W H SPP DEPTH   builds cpp_env_light's world plus two lights, switches LightSampling::EnvTree on, renders and prints a hash of the frame; then
//                                tries to take the map away while it is sampled and reports the refusal; then renders in LightSampling::Env and prints that hash.
// tests/test_gpu_env_tree.py builds the same world through Python and compares both hashes with the C ABI's frames.
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
            std::fprintf(stderr, "usage: env_tree_app W H SPP DEPTH\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
        static_assert((uint32_t)LightSampling::EnvTree == 48u, "LightSampling::EnvTree is RT_LIGHT_SAMPLING_ENV_TREE");
        LambertianAbstract<Quad> white(glm::vec3(0.73f, 0.73f, 0.73f));
        rt06::SceneBuilder b;
        std::vector<float> map;   // a 16 x 8 map: red grows to the right, green downwards, blue bright (far above 1) in one texel of the top rows
        for (uint32_t y = 0; y < 8; y++)
            for (uint32_t x = 0; x < 16; x++) { map.push_back(0.0625f * (float)x); map.push_back(0.125f * (float)y); map.push_back(x == 5 && y == 1 ? 40.0f : 0.25f); }
        b.SetEnvironment(16, 8, map.data(), 45.0f);
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        const int32_t floor_mat = b.material(&white);
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, floor_mat, nullptr), "floor");
        const float red[3] = {0.7f, 0.3f, 0.3f}, steel[3] = {0.8f, 0.8f, 0.9f}, warm[3] = {8.0f, 7.0f, 5.0f}, cold[3] = {4.0f, 8.0f, 12.0f};
        int32_t m_red = 0, m_steel = 0, m_warm = 0, m_cold = 0;
        rt06::check(rt_scene_add_material(b.get(), RT_MAT_LAMBERTIAN, red, 0.0f, nullptr, &m_red), "material");
        rt06::check(rt_scene_add_material(b.get(), RT_MAT_METAL, steel, 0.1f, nullptr, &m_steel), "material");
        rt06::check(rt_scene_add_material(b.get(), RT_MAT_DIFFUSE_LIGHT, warm, 0.0f, nullptr, &m_warm), "material");
        rt06::check(rt_scene_add_material(b.get(), RT_MAT_DIFFUSE_LIGHT, cold, 0.0f, nullptr, &m_cold), "material");
        const float c0[3] = {-2.2f, 1.0f, 0.0f}, c1[3] = {0.0f, 1.0f, 0.0f}, c2[3] = {2.2f, 1.0f, 0.0f};
        rt06::check(rt_scene_add_sphere(b.get(), c0, 1.0f, m_red, nullptr), "sphere");
        rt06::check(rt_scene_add_sphere(b.get(), c1, 1.0f, m_steel, nullptr), "sphere");
        rt06::check(rt_scene_add_sphere(b.get(), c2, 1.0f, m_red, nullptr), "sphere");
        const float lq[3] = {-1, 4, -1}, lu[3] = {2, 0, 0}, lv[3] = {0, 0, 2};
        rt06::check(rt_scene_add_quad(b.get(), lq, lu, lv, m_warm, nullptr), "quad light");
        const float ta[3] = {3.5f, 1.0f, -2.0f}, tb[3] = {3.5f, 3.0f, -1.0f}, tc[3] = {3.6f, 1.5f, 1.0f};
        rt06::check(rt_scene_add_triangle(b.get(), ta, tb, tc, m_cold, nullptr), "triangle lamp");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(0.5f, 2.5f, 7), glm::vec3(0, 1.0f, 0), glm::vec3(0, 1, 0), 50.0f, width / (float)height);
        {
            Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
            std::vector<glm::vec4> fb((size_t)width * height);
            renderer.SetLightSampling(LightSampling::EnvTree);
            renderer.Render();
            renderer.DownloadRenderbuffer(fb.data());
            std::printf("env tree %ux%u spp=%u depth=%u fnv=%016llx\n", width, height, spp, depth, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
            try {
                renderer.SetEnvironment(0, 0, nullptr);   // a map that is being sampled cannot leave
                std::printf("map off: accepted\n");
            } catch (const std::exception& e) {
                std::printf("map off: refused (%s)\n", std::strstr(e.what(), "switch light sampling off") ? "says to switch light sampling off" : e.what());
            }
            renderer.SetLightSampling(LightSampling::Env);
            renderer.Render();
            renderer.DownloadRenderbuffer(fb.data());
            std::printf("env fnv=%016llx\n", (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

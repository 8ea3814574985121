// light_tree_app.cpp — a room lit by two emissive triangles of different areas, rendered through include/rt06/rt06.hpp with LightSampling::Tree.
//
//   light_tree_app W H SPP DEPTH   builds the room, switches RT_LIGHT_SAMPLING_TREE on, renders and prints a hash of the frame.
// tests/test_cpp_light_tree.py builds the same room through Python and compares the hash with the C ABI's frame.
#include <cstdio>
#include <cstdlib>
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
            std::fprintf(stderr, "usage: light_tree_app W H SPP DEPTH\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
        LambertianAbstract<Quad> white(glm::vec3(0.73f, 0.73f, 0.73f)), red(glm::vec3(0.65f, 0.05f, 0.05f));
        DiffuseLightAbstract<Quad> lamp(glm::vec3(14.0f, 12.0f, 9.0f));
        rt06::SceneBuilder b;
        const float o[3] = {0, 0, 0}, top[3] = {0, 10, 0}, back[3] = {0, 0, 10}, x[3] = {10, 0, 0}, y[3] = {0, 10, 0}, z[3] = {0, 0, 10};
        rt06::check(rt_scene_add_quad(b.get(), o, x, z, b.material(&white), nullptr), "floor");
        rt06::check(rt_scene_add_quad(b.get(), top, x, z, b.material(&white), nullptr), "ceiling");
        rt06::check(rt_scene_add_quad(b.get(), o, y, z, b.material(&red), nullptr), "left wall");
        rt06::check(rt_scene_add_quad(b.get(), back, x, y, b.material(&white), nullptr), "back wall");
        b.AddTriangle(glm::vec3(3.5f, 9.5f, 4.0f), glm::vec3(6.5f, 9.7f, 4.5f), glm::vec3(5.0f, 9.2f, 7.0f), &lamp);
        b.AddTriangle(glm::vec3(0.3f, 5.0f, 3.0f), glm::vec3(0.3f, 7.0f, 4.0f), glm::vec3(0.4f, 5.5f, 6.0f), &lamp);
        b.AddTriangle(glm::vec3(2.0f, 0.0f, 5.0f), glm::vec3(5.0f, 0.0f, 4.0f), glm::vec3(3.5f, 3.0f, 6.0f), &red);
        const float black[3] = {0, 0, 0};
        rt06::check(rt_scene_set_background(b.get(), 1, black), "rt_scene_set_background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(5, 5, 0.5f), glm::vec3(5, 4, 10), glm::vec3(0, 1, 0), 80.0f, width / (float)height);
        {
            Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
            renderer.SetLightSampling(LightSampling::Tree);
            renderer.Render();
            std::vector<glm::vec4> fb((size_t)width * height);
            renderer.DownloadRenderbuffer(fb.data());
            std::printf("light tree %ux%u spp=%u depth=%u fnv=%016llx\n", width, height, spp, depth, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

// interiors_app.cpp — a floor, a tinted solid glass box and a tinted glass ball, rendered through include/rt06/rt06.hpp.
//
//   interiors_app W H SPP DEPTH   builds the world with SceneBuilder::SetInterior; MakeRenderer pushes the scene's interior table; renders and prints a hash of the
//                                 frame, then takes the table away and prints the hash of that frame — a box that is entered at every face — too.
// tests/test_cpp_interiors.py builds the same world through Python and compares both hashes with the C ABI's frames.
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
            std::fprintf(stderr, "usage: interiors_app W H SPP DEPTH\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
        rt06::SceneBuilder b;
        LambertianAbstract<Quad> m_floor(glm::vec3(0.5f, 0.5f, 0.5f));
        DielectricAbstract<Quad> m_box(glm::vec3(1.0f, 1.0f, 1.0f), 1.5f), m_ball(glm::vec3(1.0f, 1.0f, 1.0f), 1.33f);
        const int32_t floor_mat = b.material(&m_floor), box_mat = b.material(&m_box), ball_mat = b.material(&m_ball);
        b.SetInterior((uint32_t)box_mat, glm::vec3(2.0f, 2.0f, 2.0f));
        b.SetInterior((uint32_t)box_mat, glm::vec3(1.0f, 0.25f, 0.5f));   // the last call counts
        b.SetInterior((uint32_t)ball_mat, glm::vec3(0.125f, 0.5f, 1.0f));
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, floor_mat, nullptr), "floor");
        const float lo[3] = {0.2f, 0.1f, -0.8f}, hi[3] = {2.0f, 1.9f, 1.0f}, nowhere[3] = {0, 0, 0};
        rt06::check(rt_scene_add_box(b.get(), lo, hi, box_mat, 20.0f, nowhere, nullptr), "box");
        const float c1[3] = {-1.4f, 1.0f, 0.2f};
        rt06::check(rt_scene_add_sphere(b.get(), c1, 1.0f, ball_mat, nullptr), "ball");
        const float sky[3] = {0.6f, 0.7f, 0.9f};
        rt06::check(rt_scene_set_background(b.get(), 1, sky), "background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        const rt_interior* table = nullptr;
        if (b.Interiors(&table) != 3u || table[box_mat].on != RT_INTERIOR_SOLID || table[box_mat].sigma[1] != 0.25f || table[ball_mat].on != RT_INTERIOR_SOLID ||
            table[floor_mat].on != RT_INTERIOR_OFF)
            throw std::runtime_error("three materials, two interior records");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(0.5f, 2.5f, 7), glm::vec3(0, 1.0f, 0), glm::vec3(0, 1, 0), 50.0f, width / (float)height);
        Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
        std::vector<glm::vec4> fb((size_t)width * height);
        renderer.Render();
        renderer.DownloadRenderbuffer(fb.data());
        std::printf("interiors %ux%u spp=%u depth=%u fnv=%016llx\n", width, height, spp, depth, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        renderer.SetInteriors(nullptr, 0);
        renderer.Render();
        renderer.DownloadRenderbuffer(fb.data());
        std::printf("off: fnv=%016llx\n", (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        b.ClearInterior((uint32_t)ball_mat);
        b.ClearInterior((uint32_t)box_mat);
        if (b.Interiors(&table) != 0u || table != nullptr) throw std::runtime_error("cleared records leave no table");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

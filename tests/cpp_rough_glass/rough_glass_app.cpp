// rough_glass_app.cpp — a floor, a frosted ball and a frosted pane under a roughness map, rendered through include/rt06/rt06.hpp.
//
//   rough_glass_app W H SPP DEPTH   builds the world with SceneBuilder::AddImage, SetRoughGlass and SetRoughnessMap; MakeRenderer pushes the scene's texture
//                                   table and its microfacet table; renders and prints a hash of the frame, then takes the table away and prints the hash of
//                                   that frame — clear glass — too.
// tests/test_cpp_rough_glass.py builds the same world through Python and compares both hashes with the C ABI's frames.
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

// a computed w x h roughness map in integers: the green channel steps with the texel's position
static std::vector<uint8_t> steps(uint32_t w, uint32_t h) {
    std::vector<uint8_t> px;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) { px.push_back((uint8_t)(10u * x)); px.push_back((uint8_t)(40u + 50u * ((x + y) % 4u))); px.push_back((uint8_t)(200u + y)); }
    return px;
}

int main(int argc, char** argv) {
    try {
        if (argc < 5) {
            std::fprintf(stderr, "usage: rough_glass_app W H SPP DEPTH\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
        rt06::SceneBuilder b;
        const std::vector<uint8_t> map = steps(6, 4);
        const uint32_t i_map = b.AddImage(6, 4, map.data(), RT_WRAP_REPEAT, RT_FILTER_BILINEAR);
        LambertianAbstract<Quad> m_floor(glm::vec3(0.5f, 0.5f, 0.5f));
        DielectricAbstract<Quad> m_ball(glm::vec3(1.0f, 1.0f, 1.0f), 1.5f), m_pane(glm::vec3(0.9f, 1.0f, 0.9f), 1.33f);
        const int32_t floor_mat = b.material(&m_floor), ball_mat = b.material(&m_ball), pane_mat = b.material(&m_pane);
        b.SetRoughGlass((uint32_t)ball_mat, 0.6f);
        b.SetRoughGlass((uint32_t)ball_mat, 0.4f);
        b.SetRoughGlass((uint32_t)pane_mat, 1.0f);
        b.SetRoughnessMap((uint32_t)pane_mat, i_map);
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, floor_mat, nullptr), "floor");
        const float c1[3] = {-1.2f, 1.0f, 0.0f};
        rt06::check(rt_scene_add_sphere(b.get(), c1, 1.0f, ball_mat, nullptr), "ball");
        const float pq[3] = {0.4f, 0.2f, 1.0f}, pu[3] = {2.0f, 0, -0.6f}, pv[3] = {0, 2.0f, 0};
        rt06::check(rt_scene_add_quad(b.get(), pq, pu, pv, pane_mat, nullptr), "pane");
        const float sky[3] = {0.6f, 0.7f, 0.9f};
        rt06::check(rt_scene_set_background(b.get(), 1, sky), "background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        const rt_microfacet* table = nullptr;
        if (b.Microfacets(&table) != 3u || table[ball_mat].on != RT_MICROFACET_GLASS || table[ball_mat].roughness != 0.4f || table[pane_mat].on != RT_MICROFACET_GLASS_MAPPED ||
            table[floor_mat].on != RT_MICROFACET_OFF)
            throw std::runtime_error("three materials, two glass records");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(0.5f, 2.5f, 7), glm::vec3(0, 1.0f, 0), glm::vec3(0, 1, 0), 50.0f, width / (float)height);
        Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
        std::vector<glm::vec4> fb((size_t)width * height);
        renderer.Render();
        renderer.DownloadRenderbuffer(fb.data());
        std::printf("rough glass %ux%u spp=%u depth=%u fnv=%016llx\n", width, height, spp, depth, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        renderer.SetMicrofacets(nullptr, 0);
        renderer.Render();
        renderer.DownloadRenderbuffer(fb.data());
        std::printf("off: fnv=%016llx\n", (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

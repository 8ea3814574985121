// textures_app.cpp — a sphere, a tiled floor and a UV-mapped triangle under three images, rendered through include/rt06/rt06.hpp.
//
//   textures_app W H SPP DEPTH   builds the world with SceneBuilder::AddImage / SetImageSampling and ImageTextureAbstract(index); MakeRenderer pushes the scene's
//                                table (Renderer::SetTextures); renders, prints a hash of the frame, then turns the table off and reports the refusal.
// tests/test_cpp_textures.py builds the same world through Python and compares the hash with the C ABI's frame.
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

// a computed w x h image: red grows to the right, green downwards, blue alternates
static std::vector<uint8_t> image(uint32_t w, uint32_t h, uint32_t salt) {
    std::vector<uint8_t> px;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) { px.push_back((uint8_t)(40u + 200u * x / w)); px.push_back((uint8_t)(30u + 180u * y / h)); px.push_back((uint8_t)(((x + y + salt) & 1u) ? 220u : 60u)); }
    return px;
}

int main(int argc, char** argv) {
    try {
        if (argc < 5) {
            std::fprintf(stderr, "usage: textures_app W H SPP DEPTH\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
        rt06::SceneBuilder b;
        const std::vector<uint8_t> globe = image(8, 4, 0), tiles = image(2, 2, 1), atlas = image(5, 3, 0);
        rt06::check(rt_scene_set_image(b.get(), 8, 4, globe.data()), "rt_scene_set_image");   // entry 0, the world's own image
        const uint32_t i_tiles = b.AddImage(2, 2, tiles.data(), RT_WRAP_REPEAT, RT_FILTER_NEAREST);
        const uint32_t i_atlas = b.AddImage(5, 3, atlas.data());
        b.SetImageSampling(i_atlas, RT_WRAP_CLAMP, RT_FILTER_BILINEAR);
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
            Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
            renderer.Render();
            std::vector<glm::vec4> fb((size_t)width * height);
            renderer.DownloadRenderbuffer(fb.data());
            std::printf("textures %ux%u spp=%u depth=%u fnv=%016llx\n", width, height, spp, depth, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
            renderer.SetTextures(nullptr, 0, nullptr);   // off: the floor and the triangle name images the renderer no longer has
            try {
                renderer.Render();
                std::printf("off: rendered\n");
            } catch (const std::exception& e) {
                std::printf("off: refused (%s)\n", std::strstr(e.what(), "rt_renderer_textures") ? "names rt_renderer_textures" : e.what());
            }
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

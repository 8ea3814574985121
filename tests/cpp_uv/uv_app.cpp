// uv_app.cpp — an octahedron with texture coordinates over a floor, image-textured, rendered through include/rt06/rt06.hpp.
//
//   uv_app W H SPP DEPTH   builds the world with SceneBuilder::AddMesh's and AddTriangle's overloads with texture coordinates; MakeRenderer pushes the scene's
//                          table (Renderer::SetTextureCoords); renders and prints a hash of the frame.
// tests/test_gpu_texture_coords.py builds the same world through Python and compares the hash with the C ABI's frame.
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
            std::fprintf(stderr, "usage: uv_app W H SPP DEPTH\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
        LambertianAbstract<Quad> white(glm::vec3(0.73f, 0.73f, 0.73f));
        ImageTextureAbstract<Quad> image;
        rt06::SceneBuilder b;
        std::vector<uint8_t> rgb;   // an 8 x 4 image: red grows to the right, green downwards
        for (uint32_t y = 0; y < 4; y++)
            for (uint32_t x = 0; x < 8; x++) { rgb.push_back((uint8_t)(20 + 30 * x)); rgb.push_back((uint8_t)(40 + 60 * y)); rgb.push_back((uint8_t)(250 - 25 * x - 10 * y)); }
        b.image(8, 4, rgb.data());
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, b.material(&white), nullptr), "floor");
        const std::vector<glm::vec3> v = {glm::vec3(1, 0, 0), glm::vec3(-1, 0, 0), glm::vec3(0, 1, 0), glm::vec3(0, -1, 0), glm::vec3(0, 0, 1), glm::vec3(0, 0, -1)};
        const std::vector<glm::vec2> t = {glm::vec2(0.0f, 0.5f), glm::vec2(1.0f, 0.5f), glm::vec2(0.5f, 1.25f), glm::vec2(0.5f, -0.25f), glm::vec2(0.25f, 0.5f), glm::vec2(0.75f, 0.5f)};
        const std::vector<uint32_t> f = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
        b.AddMesh(v, v, t, f, {}, {}, &image, 1.5f, 20.0f, glm::vec3(0.0f, 1.8f, 0.0f));
        b.AddTriangle(glm::vec3(-3, 0.1f, -2), glm::vec3(-1.5f, 0.1f, -2.5f), glm::vec3(-2.5f, 2, -2), nullptr, glm::vec2(0.1f, 0.1f), glm::vec2(0.9f, 0.2f), glm::vec2(0.4f, 0.95f), &image);
        const float sky[3] = {0.6f, 0.7f, 0.9f};
        rt06::check(rt_scene_set_background(b.get(), 1, sky), "rt_scene_set_background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        BVH world(b.get());
        PinholeCamera cam(glm::vec3(0.5f, 2.5f, 7), glm::vec3(0, 1.5f, 0), glm::vec3(0, 1, 0), 50.0f, width / (float)height);
        {
            Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
            renderer.Render();
            std::vector<glm::vec4> fb((size_t)width * height);
            renderer.DownloadRenderbuffer(fb.data());
            std::printf("uv %ux%u spp=%u depth=%u fnv=%016llx\n", width, height, spp, depth, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

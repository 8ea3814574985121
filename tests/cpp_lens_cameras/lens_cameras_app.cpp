// lens_cameras_app.cpp — the four lens cameras written against include/rt06/rt06.hpp: a floor and a ball under a constant sky, rendered through ONE renderer whose
// camera object the caller replaces between Render() calls (the renderer keeps the pointer and reads the camera at every call).
//
//   lens_cameras_app W H SPP DEPTH PREFIX   writes PREFIX_perspective.f32, PREFIX_orthographic.f32, PREFIX_fisheye.f32 and PREFIX_panorama.f32 (W*H*4 floats each);
//                                           the perspective and the fisheye camera have a lens and a shutter.  Then shows what a bad record and the baseline
//                                           kernel answer.
// tests/test_gpu_lens_cameras.py builds the same world through Python and compares the files with what the C ABI gives there, byte for byte.
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
            std::fprintf(stderr, "usage: lens_cameras_app W H SPP DEPTH PREFIX\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[1]), height = (uint32_t)std::atoi(argv[2]), spp = (uint32_t)std::atoi(argv[3]);
        const uint32_t depth = (uint32_t)std::atoi(argv[4]);
        const std::string prefix = argv[5];
        const float aspect = width / (float)height;
        rt06::SceneBuilder b;
        LambertianAbstract<Quad> m_floor(glm::vec3(0.5f, 0.5f, 0.5f));
        MetalAbstract<Quad> m_ball(glm::vec3(0.8f, 0.8f, 0.9f), 0.1f);
        const int32_t floor_mat = b.material(&m_floor), ball_mat = b.material(&m_ball);
        const float q[3] = {-6, 0, -6}, x[3] = {12, 0, 0}, z[3] = {0, 0, 12};
        rt06::check(rt_scene_add_quad(b.get(), q, x, z, floor_mat, nullptr), "floor");
        const float c1[3] = {0.0f, 1.0f, 0.0f};
        rt06::check(rt_scene_add_sphere(b.get(), c1, 1.0f, ball_mat, nullptr), "ball");
        const float sky[3] = {0.6f, 0.7f, 0.9f};
        rt06::check(rt_scene_set_background(b.get(), 1, sky), "background");
        rt06::check(rt_scene_build_bvh_topdown(b.get()), "rt_scene_build_bvh_topdown");
        BVH world(b.get());
        const glm::vec3 eye(0.5f, 2.0f, 7.0f), at(0, 1.0f, 0), up(0, 1, 0);
        LensCamera cam = LensCamera::Perspective(eye, at, up, 50.0f, aspect, 0.4f, 7.0f, 0.0f, 1.0f);
        Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world);
        std::vector<glm::vec4> frame((size_t)width * height);
        const char* names[4] = {"perspective", "orthographic", "fisheye", "panorama"};
        for (int k = 0; k < 4; k++) {
            if (k == 1) cam = LensCamera::Orthographic(eye, at, up, 6.0f, aspect);
            if (k == 2) cam = LensCamera::Fisheye(eye, at, up, 180.0f, aspect, 0.4f, 7.0f, 0.0f, 1.0f);
            if (k == 3) cam = LensCamera::Panorama(eye, at, up);
            renderer.Render();   // the caller's camera as it is now
            renderer.DownloadRenderbuffer(frame.data());
            write_file(prefix + "_" + names[k] + ".f32", frame);
            std::printf("%s: type=%u\n", names[k], cam.cam.type);
        }
        try {
            LensCamera::Fisheye(eye, at, up, 300.0f, aspect);
            std::printf("fisheye 300: accepted\n");
        } catch (const std::exception& e) {
            std::printf("fisheye 300: refused (%s)\n", std::strstr(e.what(), "pi") ? "names the bound" : e.what());
        }
        try {
            Renderer baseline = Renderer::MakeRenderer(width, height, spp, depth, &cam, &world, 1984, 0, 1, 1);
            std::printf("variant 1: accepted\n");
        } catch (const std::exception& e) {
            std::printf("variant 1: refused (%s)\n", std::strstr(e.what(), "baseline kernel") ? "names the baseline kernel" : e.what());
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

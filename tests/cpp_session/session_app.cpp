// session_app.cpp — a caller that keeps ONE Renderer across frames, compiled against include/rt06/rt06.hpp.
//
// FirstApp's flow (main/src/FirstApp.cpp:20-56, 94-106: camera, scene, Renderer::MakeRenderer, Render, DownloadRenderbuffer) on the
// Book-2 moving-spheres world, and then what a viewer or an animation loop does with the same renderer object:
//
//   session_app camera W H SPP DEPTH PREFIX   Render(); the camera OBJECT is mutated in place (no call on the renderer), Render() again;
//                                             the first camera restored, Render(); a camera of another TYPE written into the object,
//                                             Render().  The reference reads `*m.cam` at every Render() (Renderer.cu:117): each frame
//                                             follows the object.  Writes PREFIX_0.f32 .. PREFIX_3.f32 (raw float framebuffers).
//   session_app refine W H DEPTH PREFIX N...  Refine(N) for every N given, one frame file per step (PREFIX_<samples>.f32); prints the samples
//                                             accumulated and the noise figure after each step.  Then the camera moves and one more step
//                                             shows that the accumulation started over.
// tests/test_gpu_session.py puts every frame against the CPU oracle, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt06/rt06.hpp"

static uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

static void write_frame(const std::string& path, const std::vector<glm::vec4>& fb) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    std::fwrite(fb.data(), sizeof(glm::vec4), fb.size(), f);
    std::fclose(f);
}

int main(int argc, char** argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if ((mode != "camera" || argc < 7) && (mode != "refine" || argc < 7)) {
            std::fprintf(stderr, "usage: session_app camera W H SPP DEPTH PREFIX | session_app refine W H DEPTH PREFIX N...\n");
            return 2;
        }
        const uint32_t width = (uint32_t)std::atoi(argv[2]), height = (uint32_t)std::atoi(argv[3]);
        const float aspect = width / (float)height;
        rt_scene* scene = nullptr;
        rt06::check(rt_scene_book2_moving(1984, &scene), "rt_scene_book2_moving");   // the world first_app builds through the vocabulary
        BVH world(scene);
        const glm::vec3 lookat(0, 0, 0), up(0, 1, 0);
        auto cam = new MotionBlurCamera(glm::vec3(13, 2, 3), lookat, up, 30.0f, aspect, 0.1f, 1.0f);   // FirstApp.cpp:25-30
        const MotionBlurCamera first = *cam;
        std::vector<glm::vec4> fb((size_t)width * height);
        auto show = [&](Renderer& renderer, const char* what, const std::string& path) {
            renderer.DownloadRenderbuffer(fb.data());
            std::printf("%s fnv=%016llx\n", what, (unsigned long long)fnv1a(fb.data(), fb.size() * sizeof(glm::vec4)));
            write_frame(path, fb);
        };
        if (mode == "camera") {
            const uint32_t spp = (uint32_t)std::atoi(argv[4]), depth = (uint32_t)std::atoi(argv[5]);
            const std::string prefix = argv[6];
            Renderer renderer = Renderer::MakeRenderer(width, height, spp, depth, cam, &world);
            renderer.Render();
            show(renderer, "frame 0 (first camera)", prefix + "_0.f32");
            *cam = MotionBlurCamera(glm::vec3(-9, 3, 6), glm::vec3(0, 0.5f, 0), up, 35.0f, aspect, 0.0f, 0.5f);   // the camera moves; the renderer is not told
            renderer.Render();
            show(renderer, "frame 1 (moved camera)", prefix + "_1.f32");
            *cam = first;
            renderer.Render();
            show(renderer, "frame 2 (first camera again)", prefix + "_2.f32");
            cam->cam = PinholeCamera(glm::vec3(4, 5, 12), lookat, up, 40.0f, aspect).cam;   // another camera TYPE in the same object
            renderer.Render();
            show(renderer, "frame 3 (pinhole camera)", prefix + "_3.f32");
        } else {
            const uint32_t depth = (uint32_t)std::atoi(argv[4]);
            const std::string prefix = argv[5];
            Renderer renderer = Renderer::MakeRenderer(width, height, 16, depth, cam, &world);   // 16: what ONE pass is sized for, not a limit
            for (int a = 6; a < argc; a++) {
                renderer.Refine((uint32_t)std::atoi(argv[a]));
                const unsigned long long done = renderer.SamplesAccumulated();
                if (done >= 2) std::printf("samples=%llu noise=%.17g\n", done, renderer.Noise());
                else std::printf("samples=%llu\n", done);
                show(renderer, "refined", prefix + "_" + std::to_string(done) + ".f32");
            }
            *cam = MotionBlurCamera(glm::vec3(-9, 3, 6), glm::vec3(0, 0.5f, 0), up, 35.0f, aspect, 0.0f, 0.5f);
            renderer.Refine(2);   // the moved camera restarts the accumulation: this frame has 2 samples, not done + 2
            std::printf("after the camera moved: samples=%llu\n", (unsigned long long)renderer.SamplesAccumulated());
            show(renderer, "moved", prefix + "_moved.f32");
        }
        delete cam;   // after the renderer: it reads the camera until its last Render()
        rt_scene_destroy(scene);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

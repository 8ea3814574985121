// rt_internal.hpp — declarations shared by the host and device translation units of librt06.so.
#pragma once
#include <stdint.h>

#define RT_MAX_STACK 32  // _PRIO_QUEUE_ELEM_COUNT, rt_engine/geometry/BVH.cu:17
#define RT_TILE 8        // 8x8-pixel tiles: the reference's thread-block shape, Renderer.cu:130

int rt_fail(int code, const char* fmt, ...);
struct rt_camera;
int rt_camera_check(const char* who, const rt_camera* cam);   // rt_host.cpp: RT_OK for the three reference types and a valid lens camera (types 16 to 19), else the refusal
const char* rt_environment_image_refusal(uint32_t width, uint32_t height, const float* rgb);   // rt_host.cpp: why an environment map is refused, or null
// rt_host.cpp: rt_environment_distribution's tables of a valid image, or why it has none (an all-black map)
const char* rt_environment_distribution_refusal(uint32_t width, uint32_t height, const float* rgb, float* rowc, float* rowy, float* colc, float* density);
// rt_host.cpp, the texture table: whether `param` of an image material is an image index (an integer in [0, RT_MAX_IMAGES)); why a table is
// refused, or null (*out_texels = how many texels its entries hold together)
struct rt_texture;
bool rt_image_index_ok(float param);
const char* rt_texture_table_refusal(const rt_texture* records, uint32_t n, const uint8_t* texels, uint64_t* out_texels);

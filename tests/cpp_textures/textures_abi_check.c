/* The texture-table entry points of include/rt06.h from plain C11 (-pedantic): sizes are compile-time assertions, the address of each entry point is taken,
 * and a scene's images are added, refused, given modes and read back, and the rule applied to a few coordinates, on the host.  No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_world_flat) == 128, "rt_world_flat stays 128 bytes: the table travels beside it");
_Static_assert(sizeof(rt_material) == 32, "rt_material stays 32 bytes: the image index rides in albedo2[0]");
_Static_assert(sizeof(rt_texture) == 20, "rt_texture is five 32-bit words");
_Static_assert(RT_MAX_IMAGES == 256u, "256 images");
_Static_assert(RT_WRAP_CLAMP == 0 && RT_WRAP_REPEAT == 1 && RT_FILTER_NEAREST == 0 && RT_FILTER_BILINEAR == 1, "the modes' values");

int main(void) {
    int (*add)(rt_scene*, uint32_t, uint32_t, const uint8_t*, uint32_t, uint32_t, uint32_t*) = rt_scene_add_image;
    int (*modes)(rt_scene*, uint32_t, uint32_t, uint32_t) = rt_scene_image_sampling;
    int (*get)(const rt_scene*, const rt_texture**, uint32_t*, const uint8_t**) = rt_scene_textures;
    int (*batch)(const rt_texture*, uint32_t, const uint8_t*, const uint32_t*, const float*, const float*, size_t, float*) = rt_texture_lookup_batch;
    int (*r_set)(rt_renderer*, const rt_texture*, uint32_t, const uint8_t*) = rt_renderer_textures;
    int (*r_info)(rt_renderer*, uint32_t[2]) = rt_renderer_textures_info;
    int (*m_set)(rt_multi_renderer*, const rt_texture*, uint32_t, const uint8_t*) = rt_multi_renderer_textures;
    int (*probe)(int, const rt_texture*, uint32_t, const uint8_t*, const uint32_t*, const float*, const float*, size_t, float*) = rt_probe_texture;
    /* a 2 x 2 image: top row (10, 0, 0), (20, 0, 0); bottom row (30, 0, 0), (40, 0, 0); and a 1 x 1 image (255, 128, 0) */
    const uint8_t four[2 * 2 * 3] = {10, 0, 0, 20, 0, 0, 30, 0, 0, 40, 0, 0}, one[3] = {255, 128, 0};
    const float white[3] = {1, 1, 1}, c[3] = {0, 0, -1}, half[3] = {1.5f, 0, 0}, minus[3] = {-1, 0, 0}, many[3] = {256, 0, 0}, two[3] = {2, 0, 0};
    const float k = 0x1.010102p-8f;
    /* (u, v): the bottom-left texel's centre; the same a period away; the middle of the image; the 1 x 1 image anywhere */
    const uint32_t index[4] = {1, 1, 1, 2};
    const float u[4] = {0.25f, -0.75f, 0.5f, 7.5f}, v[4] = {0.25f, 2.25f, 0.5f, -3.25f};
    float rgb[4 * 3];
    const rt_texture* rec = NULL;
    const uint8_t* texels = NULL;
    uint32_t n = 9, at = 0;
    rt_scene* s = NULL;
    rt_world_flat flat;
    int32_t mat = -1;
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += get(s, &rec, &n, &texels) != RT_OK || n != 0 || rec != NULL || texels != NULL;                       /* no image, default modes: no table */
    bad += add(s, 2, 2, four, RT_WRAP_REPEAT, RT_FILTER_NEAREST, &at) != RT_OK || at != 1;
    bad += add(s, 1, 1, one, RT_WRAP_CLAMP, RT_FILTER_BILINEAR, &at) != RT_OK || at != 2;
    bad += add(s, 0, 2, four, 0, 0, &at) != RT_ERR_INVALID || strstr(rt_last_error(), "bad size") == NULL;
    bad += add(s, 2, 2, four, 2, 0, &at) != RT_ERR_INVALID || strstr(rt_last_error(), "wrap") == NULL;
    bad += add(s, 2, 2, four, 0, 2, &at) != RT_ERR_INVALID || strstr(rt_last_error(), "filter") == NULL || at != 2;
    bad += modes(s, 3, 0, 0) != RT_ERR_INVALID || strstr(rt_last_error(), "no image 3") == NULL;
    bad += get(s, &rec, &n, &texels) != RT_OK || n != 3 || rec[0].width != 0 || rec[1].width != 2 || rec[1].wrap != RT_WRAP_REPEAT || rec[1].first != 0 ||
           rec[2].first != 4 || rec[2].filter != RT_FILTER_BILINEAR || memcmp(texels, four, sizeof(four)) != 0 || memcmp(texels + 12, one, 3) != 0;
    bad += batch(rec, n, texels, index, u, v, 4, rgb) != RT_OK;
    bad += !(rgb[0] == 30.0f * k && rgb[3] == 30.0f * k);                                                        /* v = 0 is the bottom row; REPEAT is periodic */
    bad += !(rgb[9] == 255.0f * k && rgb[10] == 128.0f * k && rgb[11] == 0.0f);                                  /* a constant image is exactly constant */
    bad += modes(s, 1, RT_WRAP_CLAMP, RT_FILTER_BILINEAR) != RT_OK;
    bad += get(s, &rec, &n, &texels) != RT_OK || batch(rec, n, texels, index, u, v, 4, rgb) != RT_OK;
    bad += !(rgb[0] == 30.0f * k && fabsf(rgb[6] - 25.0f * k) < 1e-6f);                                          /* a centre is its texel; the middle the mean of four */
    bad += batch(rec, n, texels, &n, u, v, 1, rgb) != RT_ERR_INVALID || strstr(rt_last_error(), "no entry 3") == NULL;
    at = 0;
    bad += batch(rec, n, texels, &at, u, v, 1, rgb) != RT_ERR_INVALID || strstr(rt_last_error(), "no entry 0") == NULL;   /* entry 0 is empty */
    /* the index rides in albedo2[0]; param means nothing for this type */
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN_IMAGE, white, 0.0f, half, &mat) != RT_ERR_INVALID || strstr(rt_last_error(), "image index") == NULL;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN_IMAGE, white, 0.0f, minus, &mat) != RT_ERR_INVALID;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN_IMAGE, white, 0.0f, many, &mat) != RT_ERR_INVALID || mat != -1;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN_IMAGE, white, 0.5f, two, &mat) != RT_OK;
    bad += rt_scene_add_sphere(s, c, 0.5f, mat, NULL) != RT_OK || rt_scene_set_world_list(s) != RT_OK;
    bad += rt_scene_get_flat(s, &flat) != RT_OK || flat.image != NULL || flat.materials[mat].albedo2[0] != 2.0f;   /* the flat world knows entry 0 only */
    bad += r_set(NULL, NULL, 0, NULL) != RT_ERR_INVALID || strstr(rt_last_error(), "rt_renderer_textures") == NULL;
    bad += m_set(NULL, NULL, 0, NULL) != RT_ERR_INVALID;
    bad += r_info(NULL, NULL) != RT_ERR_INVALID;
    bad += rt_multi_renderer_textures_info(NULL, NULL) != RT_ERR_INVALID;
    bad += probe == NULL;
    rt_scene_destroy(s);
    if (bad) { printf("textures ABI: %d checks failed\n", bad); return 1; }
    printf("textures ABI ok\n");
    return 0;
}

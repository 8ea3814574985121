/* The environment-map entry points of include/rt06.h from plain C11 (-pedantic): sizes are compile-time assertions, the address of each entry point is taken,
 * and a scene's map is set, refused, read back and dropped, and the rule applied to a few directions, on the host.  No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_world_flat) == 128, "rt_world_flat stays 128 bytes: background mode 2 is a value of a field it had");
_Static_assert(sizeof(rt_quad) == 80, "rt_quad stays 80 bytes");
_Static_assert(RT_ENV_MAX_TEXELS == 33554432u, "2^25 texels");

int main(void) {
    int (*set)(rt_scene*, uint32_t, uint32_t, const float*, float) = rt_scene_set_environment;
    int (*get)(const rt_scene*, uint32_t*, uint32_t*, const float**, float*) = rt_scene_environment;
    int (*batch)(size_t, uint32_t, uint32_t, const float*, float, const float*, float*, uint32_t*) = rt_environment_batch;
    int (*r_set)(rt_renderer*, uint32_t, uint32_t, const float*, float) = rt_renderer_environment;
    int (*r_info)(rt_renderer*, uint32_t[4]) = rt_renderer_environment_info;
    int (*m_set)(rt_multi_renderer*, uint32_t, uint32_t, const float*, float) = rt_multi_renderer_environment;
    int (*probe)(int, size_t, uint32_t, uint32_t, const float*, float, const float*, float*, uint32_t*) = rt_probe_environment;
    /* a 4 x 2 map: texel (i, j) holds (i, j, 10 i + j) */
    float map[4 * 2 * 3], bad_map[4 * 2 * 3];
    const float grey[3] = {0.5f, 0.5f, 0.5f}, c[3] = {0, 0, -1}, sky[3] = {0.1f, 0.2f, 0.3f};
    /* +y: the top row; -y: the bottom row; +x: u = 0.5; -z: u = 0.75; +z: u = 0.25 */
    const float dirs[5 * 3] = {0, 2, 0, 0, -0.5f, 0, 3, 0, 0, 0, 0, -1, 0, 0, 1};
    float rgb[5 * 3], u0 = -1.0f;
    uint32_t texel[5], w = 9, h = 9;
    const float* back = NULL;
    rt_scene* s = NULL;
    rt_world_flat flat;
    int32_t mat = -1;
    int bad = 0;
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 4; i++) { map[(j * 4 + i) * 3] = (float)i; map[(j * 4 + i) * 3 + 1] = (float)j; map[(j * 4 + i) * 3 + 2] = (float)(10 * i + j); }
    memcpy(bad_map, map, sizeof(map));
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &mat) != RT_OK;
    bad += rt_scene_add_sphere(s, c, 0.5f, mat, NULL) != RT_OK;
    bad += get(s, &w, &h, &back, &u0) != RT_OK || w != 0 || h != 0 || back != NULL;                       /* no map yet */
    bad += set(s, 4, 2, map, 90.0f) != RT_OK;
    bad_map[5] = -1.0f;
    bad += set(s, 4, 2, bad_map, 0.0f) != RT_ERR_INVALID || strstr(rt_last_error(), "negative") == NULL;   /* refused, the scene keeps its map */
    bad_map[5] = NAN;
    bad += set(s, 4, 2, bad_map, 0.0f) != RT_ERR_INVALID || strstr(rt_last_error(), "not finite") == NULL;
    bad += set(s, 0, 2, map, 0.0f) != RT_ERR_INVALID || set(s, 4, 0, map, 0.0f) != RT_ERR_INVALID;
    bad += set(s, 8192, 4097, map, 0.0f) != RT_ERR_INVALID || strstr(rt_last_error(), "2^25") == NULL;    /* refused on its size, before a texel is read */
    bad += get(s, &w, &h, &back, &u0) != RT_OK || w != 4 || h != 2 || back == NULL || u0 != 0.25f || memcmp(back, map, sizeof(map)) != 0;
    bad += rt_scene_set_world_list(s) != RT_OK;
    bad += rt_scene_get_flat(s, &flat) != RT_OK || flat.background != 2u;
    bad += batch(5, 4, 2, map, 0.0f, dirs, rgb, texel) != RT_OK;
    bad += !(texel[0] / 4 == 0 && texel[1] / 4 == 1);                                                       /* row 0 is the top */
    bad += !(texel[2] == 6 && texel[3] == 7 && texel[4] == 5);                                              /* +x, -z, +z: on the horizon v = 0.5 -> j = 1; i = 2, 3, 1 */
    bad += batch(5, 4, 2, map, 0.25f, dirs, rgb, texel) != RT_OK || !(texel[2] % 4 == 3 && texel[3] % 4 == 0 && texel[4] % 4 == 2);   /* a quarter turn: one column on, with the wrap */
    bad += !(rgb[3 * 3] == 0.0f && rgb[3 * 3 + 2] == (float)(texel[3] / 4));                                /* the texel as stored */
    bad += batch(1, 4, 2, map, 1.0f, dirs, rgb, texel) != RT_ERR_INVALID || strstr(rt_last_error(), "u0") == NULL;
    bad += rt_scene_set_background(s, 1, sky) != RT_OK;                                                    /* a constant colour drops the map */
    bad += get(s, &w, &h, &back, &u0) != RT_OK || w != 0 || back != NULL;
    bad += rt_scene_get_flat(s, &flat) != RT_OK || flat.background != 1u;
    bad += r_set(NULL, 0, 0, NULL, 0.0f) != RT_ERR_INVALID || strstr(rt_last_error(), "rt_renderer_environment") == NULL;
    bad += m_set(NULL, 0, 0, NULL, 0.0f) != RT_ERR_INVALID;
    bad += r_info(NULL, NULL) != RT_ERR_INVALID;
    bad += probe == NULL;
    rt_scene_destroy(s);
    if (bad) { printf("env ABI: %d checks failed\n", bad); return 1; }
    printf("env ABI ok\n");
    return 0;
}

/* The declarations of mode RT_LIGHT_SAMPLING_MESH of include/rt06.h from plain C11 (-pedantic): the defines are compile-time assertions, the address of
 * rt_world_light_table is taken, and the table of a small world with one light of each kind is asked for on the host.  No GPU is touched. */
#include <stdio.h>

#include "rt06.h"

_Static_assert(RT_LIGHT_SAMPLING_MESH == 4 && RT_LIGHT_SAMPLING_ALL == 2 && RT_LIGHT_SAMPLING_QUADS == 1 && RT_LIGHT_SAMPLING_OFF == 0, "3 is no mode");
_Static_assert(RT_LIGHT_QUAD == 0 && RT_LIGHT_SPHERE == 1 && RT_LIGHT_TRIANGLE == 2, "the kinds of a table entry");
_Static_assert(RT_MAX_LIGHTS == 16 && RT_MAX_LIGHTS_MESH == 64, "modes 1 and 2 keep their cap");

int main(void) {
    int (*light_table)(const rt_world_flat*, uint32_t, uint32_t, uint32_t*, uint32_t*, float*, uint32_t*) = rt_world_light_table;
    const float o[3] = {0, 0, 0}, x[3] = {2, 0, 0}, z[3] = {0, 0, 3}, c[3] = {0, 2, 0}, emit[3] = {4, 4, 4};
    rt_scene* s = NULL;
    rt_world_flat w;
    int32_t light = -1, tri = -1;
    uint32_t kind[RT_MAX_LIGHTS_MESH], index[RT_MAX_LIGHTS_MESH], n = 99;
    float area[RT_MAX_LIGHTS_MESH];
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, emit, 0.0f, NULL, &light) != RT_OK;
    bad += rt_scene_add_triangle(s, o, x, z, light, &tri) != RT_OK;
    bad += rt_scene_add_quad(s, c, x, z, light, NULL) != RT_OK;
    bad += rt_scene_add_sphere(s, c, 0.5f, light, NULL) != RT_OK;
    bad += rt_scene_set_world_list(s) != RT_OK;
    bad += rt_scene_get_flat(s, &w) != RT_OK;
    bad += light_table(&w, RT_LIGHT_SAMPLING_MESH, RT_MAX_LIGHTS_MESH, kind, index, area, &n) != RT_OK || n != 3;
    bad += !(kind[0] == RT_LIGHT_QUAD && kind[1] == RT_LIGHT_SPHERE && kind[2] == RT_LIGHT_TRIANGLE && index[0] == 0 && index[2] == 1);
    bad += !(area[0] == 6.0f && area[2] == 3.0f);   /* the triangle: half its parallelogram */
    bad += light_table(&w, RT_LIGHT_SAMPLING_ALL, RT_MAX_LIGHTS_MESH, kind, index, area, &n) != RT_OK || n != 2;
    bad += light_table(&w, RT_LIGHT_SAMPLING_QUADS, RT_MAX_LIGHTS_MESH, kind, index, area, &n) != RT_OK || n != 1;
    bad += light_table(&w, RT_LIGHT_SAMPLING_MESH, 2, kind, index, area, &n) != RT_ERR_INVALID || n != 0;
    bad += light_table(&w, 3, RT_MAX_LIGHTS_MESH, kind, index, area, &n) != RT_ERR_INVALID;
    bad += light_table(NULL, RT_LIGHT_SAMPLING_MESH, RT_MAX_LIGHTS_MESH, kind, index, area, &n) != RT_ERR_INVALID;
    rt_scene_destroy(s);
    if (bad) { printf("mesh light ABI: %d checks failed\n", bad); return 1; }
    printf("mesh light ABI ok\n");
    return 0;
}

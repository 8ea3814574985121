/* The declarations of mode RT_LIGHT_SAMPLING_TREE of include/rt06.h from plain C11 (-pedantic): the defines are compile-time assertions, the addresses of
 * rt_world_light_tree and rt_renderer_kernel_light_tree are taken, and the table and the tree of a small world with one light of each kind are asked for on
 * the host.  No GPU is touched. */
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(RT_LIGHT_SAMPLING_TREE == 16 && RT_LIGHT_SAMPLING_MESH == 4 && RT_LIGHT_SAMPLING_ALL == 2 && RT_LIGHT_SAMPLING_QUADS == 1, "the modes");
_Static_assert(RT_MAX_LIGHTS_TREE == 4096 && RT_MAX_LIGHTS_MESH == 64 && RT_MAX_LIGHTS == 16, "the older modes keep their caps");

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(void) {
    int (*light_tree)(const rt_world_flat*, uint32_t, float*, uint32_t*, float*) = rt_world_light_tree;
    int (*kernel_light_tree)(rt_renderer*, uint32_t*) = rt_renderer_kernel_light_tree;
    const float o[3] = {0, 0, 0}, x[3] = {2, 0, 0}, z[3] = {0, 0, 3}, c[3] = {10, 2, 0}, far_c[3] = {20, 2, 0}, emit[3] = {4, 4, 4};
    rt_scene* s = NULL;
    rt_world_flat w;
    int32_t light = -1;
    uint32_t kind[3], index[3], n = 99, n_nodes = 99, i, leaves = 0;
    float area[3], cdf[3], nodes[8 * 5];
    int bad = 0;
    bad += !(RT_LIGHT_TREE_K > 1.0f && RT_LIGHT_TREE_K < 1.001f && RT_LIGHT_TREE_PAD > 0.0f && RT_LIGHT_TREE_PAD_SPHERE > 0.0f);   /* k slightly above 1 */
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, emit, 0.0f, NULL, &light) != RT_OK;
    bad += rt_scene_add_triangle(s, o, x, z, light, NULL) != RT_OK;
    bad += rt_scene_add_quad(s, c, x, z, light, NULL) != RT_OK;
    bad += rt_scene_add_sphere(s, far_c, 0.5f, light, NULL) != RT_OK;
    bad += rt_scene_set_world_list(s) != RT_OK;
    bad += rt_scene_get_flat(s, &w) != RT_OK;
    bad += rt_world_light_table(&w, RT_LIGHT_SAMPLING_TREE, 3, kind, index, area, &n) != RT_OK || n != 3;
    /* split on x, the longest axis of the centroids: the triangle, then the quad, then the sphere */
    bad += !(kind[0] == RT_LIGHT_TRIANGLE && kind[1] == RT_LIGHT_QUAD && kind[2] == RT_LIGHT_SPHERE);
    bad += light_tree(&w, 3, nodes, &n_nodes, cdf) != RT_OK || n_nodes != 5;
    bad += !(cdf[0] == area[0] && cdf[1] == area[0] + area[1] && cdf[2] == (area[0] + area[1]) + area[2] && area[0] == 3.0f && area[1] == 6.0f);
    bad += bits(nodes[3]) != 5u || bits(nodes[7]) != 0xffffffffu;   /* the root: skip = the end, an inner node */
    for (i = 0; i < n_nodes; i++)
        if (bits(nodes[8 * i + 7]) != 0xffffffffu) bad += bits(nodes[8 * i + 7]) != leaves++ || bits(nodes[8 * i + 3]) != i + 1;   /* leaves in table order */
    bad += leaves != 3;
    bad += light_tree(&w, 2, nodes, &n_nodes, cdf) != RT_ERR_INVALID || n_nodes != 0;
    bad += light_tree(NULL, 3, nodes, &n_nodes, cdf) != RT_ERR_INVALID;
    bad += kernel_light_tree(NULL, &n) != RT_ERR_INVALID;
    rt_scene_destroy(s);
    if (bad) { printf("light tree ABI: %d checks failed\n", bad); return 1; }
    printf("light tree ABI ok\n");
    return 0;
}

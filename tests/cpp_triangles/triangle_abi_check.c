/* rt_quad's layout with the kind in it, and the triangle / mesh entry points of include/rt06.h from plain C11 (-pedantic): sizes and offsets are
 * compile-time assertions, the address of each entry point is taken, and a small scene is flattened on the host.  No GPU is touched. */
#include <stddef.h>
#include <stdio.h>

#include "rt06.h"

_Static_assert(sizeof(rt_quad) == 80, "rt_quad stays 80 bytes");
_Static_assert(sizeof(rt_world_flat) == 128, "rt_world_flat stays 128 bytes");
_Static_assert(offsetof(rt_quad, Q) == 0 && offsetof(rt_quad, D) == 12 && offsetof(rt_quad, u) == 16 && offsetof(rt_quad, mat) == 28, "rt_quad: Q, D, u, mat");
_Static_assert(offsetof(rt_quad, v) == 32 && offsetof(rt_quad, kind) == 44 && sizeof(((rt_quad*)0)->kind) == 4, "the kind takes pad0's four bytes");
_Static_assert(offsetof(rt_quad, normal) == 48 && offsetof(rt_quad, w) == 64, "rt_quad: normal, w");
_Static_assert(RT_QUAD_PARALLELOGRAM == 0 && RT_QUAD_TRIANGLE == 1, "0 is a parallelogram: every earlier world keeps its bytes");

int main(void) {
    int (*add_triangle)(rt_scene*, const float[3], const float[3], const float[3], int32_t, int32_t*) = rt_scene_add_triangle;
    int (*add_mesh)(rt_scene*, uint32_t, const float*, uint32_t, const uint32_t*, int32_t, float, float, const float[3], int32_t*, uint32_t*) = rt_scene_add_mesh;
    int (*world_triangles)(const rt_world_flat*, uint32_t*) = rt_world_triangles;
    const float a[3] = {0, 0, 0}, b[3] = {1, 0, 0}, c[3] = {0, 1, 0}, grey[3] = {0.5f, 0.5f, 0.5f};
    const float xyz[12] = {0, 0, 1, 1, 0, 1, 0, 1, 1, 2, 0, 1};
    const uint32_t faces[9] = {0, 1, 2, 0, 1, 3, 1, 3, 2}, bad_faces[3] = {0, 1, 4};
    rt_scene* s = NULL;
    rt_world_flat w;
    int32_t mat = -1, first = -1, quad = -1;
    uint32_t added = 99, n = 99;
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &mat) != RT_OK;
    bad += add_triangle(NULL, a, b, c, mat, NULL) != RT_ERR_INVALID;
    bad += add_triangle(s, a, b, b, mat, NULL) != RT_ERR_INVALID;           /* degenerate */
    bad += add_triangle(s, a, b, c, mat, &quad) != RT_OK || quad != 0;
    bad += rt_scene_add_quad(s, a, b, c, mat, &quad) != RT_OK || quad != 0;  /* goes in front of the triangle */
    bad += add_mesh(s, 4, xyz, 1, bad_faces, mat, 1.0f, 0.0f, NULL, &first, &added) != RT_ERR_INVALID;
    bad += add_mesh(s, 4, xyz, 3, faces, mat, 1.0f, 0.0f, NULL, &first, &added) != RT_OK || first != 2 || added != 2;   /* (0, 1, 3) is a line */
    bad += rt_scene_set_world_list(s) != RT_OK;
    bad += rt_scene_get_flat(s, &w) != RT_OK;
    bad += world_triangles(&w, &n) != RT_OK || n != 3 || w.n_quads != 4;
    bad += world_triangles(NULL, &n) != RT_ERR_INVALID;
    bad += !(w.quads[0].kind == RT_QUAD_PARALLELOGRAM && w.quads[1].kind == RT_QUAD_TRIANGLE && w.quads[3].kind == RT_QUAD_TRIANGLE);
    rt_scene_destroy(s);
    if (bad) { printf("triangle ABI: %d checks failed\n", bad); return 1; }
    printf("triangle ABI ok\n");
    return 0;
}

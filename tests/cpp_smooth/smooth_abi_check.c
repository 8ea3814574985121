/* rt_tri_normals and the smooth-shading entry points of include/rt06.h from plain C11 (-pedantic): sizes are compile-time assertions, the address of each
 * entry point is taken, and a small scene with vertex normals is built, permuted and read back on the host.  No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_tri_normals) == 36, "rt_tri_normals is nine floats");
_Static_assert(offsetof(rt_tri_normals, n0) == 0 && offsetof(rt_tri_normals, n1) == 12 && offsetof(rt_tri_normals, n2) == 24, "n0, n1, n2");
_Static_assert(sizeof(rt_quad) == 80, "rt_quad stays 80 bytes: the normals travel beside the flat world");
_Static_assert(sizeof(rt_world_flat) == 128, "rt_world_flat stays 128 bytes");

int main(void) {
    int (*add_tri)(rt_scene*, const float[3], const float[3], const float[3], const float[3], const float[3], const float[3], int32_t, int32_t*) = rt_scene_add_triangle_smooth;
    int (*add_mesh)(rt_scene*, uint32_t, const float*, uint32_t, const float*, uint32_t, const uint32_t*, const uint32_t*, int32_t, float, float, const float[3], int32_t*,
                    uint32_t*) = rt_scene_add_mesh_smooth;
    int (*normals)(const rt_scene*, const rt_tri_normals**, uint32_t*) = rt_scene_vertex_normals;
    int (*batch)(size_t, const rt_quad*, const rt_tri_normals*, const float*, const float*, float*, uint32_t*) = rt_shading_normal_batch;
    int (*set)(rt_renderer*, const rt_tri_normals*, uint32_t) = rt_renderer_shading_normals;
    int (*set_multi)(rt_multi_renderer*, const rt_tri_normals*, uint32_t) = rt_multi_renderer_shading_normals;
    int (*info)(rt_renderer*, uint32_t[2]) = rt_renderer_shading_normals_info;
    int (*probe)(int, const rt_world_flat*, const rt_tri_normals*, uint32_t, size_t, const float*, int32_t*, float*, uint32_t*) = rt_probe_shading_normal;
    const float a[3] = {0, 0, 0}, b[3] = {2, 0, 0}, c[3] = {0, 2, 0}, grey[3] = {0.5f, 0.5f, 0.5f};
    const float up[3] = {0, 0, 2}, tilt[3] = {3, 0, 4}, zero[3] = {0, 0, 0}, nan3[3] = {NAN, 0, 1};
    const float xyz[9] = {0, 0, 1, 1, 0, 1, 0, 1, 1}, nrm[6] = {0, 0, 5, 0, 3, 4};
    const uint32_t face[3] = {0, 1, 2}, nface[3] = {0, 1, 1}, bad_nface[3] = {0, 1, 2};
    const rt_tri_normals* table = NULL;
    rt_scene* s = NULL;
    rt_world_flat w;
    int32_t mat = -1, quad = -1, first = -1;
    uint32_t n = 99, added = 99, took = 99;
    float out[3] = {0, 0, 0};
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &mat) != RT_OK;
    bad += rt_scene_add_triangle(s, a, b, c, mat, &quad) != RT_OK;
    bad += normals(s, &table, &n) != RT_OK || n != 0 || table != NULL;                 /* no triangle has normals yet */
    bad += add_tri(s, a, b, c, up, zero, up, mat, NULL) != RT_ERR_INVALID;              /* a zero normal */
    bad += add_tri(s, a, b, c, up, nan3, up, mat, NULL) != RT_ERR_INVALID;              /* a normal that is not finite */
    bad += add_tri(s, a, b, c, up, tilt, up, mat, &quad) != RT_OK || quad != 1;
    bad += add_mesh(s, 3, xyz, 2, nrm, 1, face, bad_nface, mat, 1.0f, 0.0f, NULL, &first, &added) != RT_ERR_INVALID;   /* normal index 2 of 2 */
    bad += add_mesh(s, 3, xyz, 2, nrm, 1, face, nface, mat, 1.0f, 0.0f, NULL, &first, &added) != RT_OK || first != 2 || added != 1;
    bad += rt_scene_add_quad(s, a, b, c, mat, &quad) != RT_OK || quad != 0;             /* goes in front of the triangles: their records stay theirs */
    bad += rt_scene_set_world_list(s) != RT_OK;
    bad += rt_scene_get_flat(s, &w) != RT_OK || w.n_quads != 4;
    bad += normals(s, &table, &n) != RT_OK || n != 3 || table == NULL;
    if (!bad) {
        bad += !(table[0].n0[2] == 0.0f && table[0].n1[2] == 0.0f && table[0].n2[2] == 0.0f);                           /* the flat triangle */
        bad += !(table[1].n0[2] == 1.0f && table[1].n1[0] == 0.6f && table[1].n1[2] == 0.8f && table[1].n2[2] == 1.0f);   /* normalised on the host */
        bad += !(table[2].n0[2] == 1.0f && table[2].n1[1] == 0.6f && table[2].n2[1] == 0.6f && table[2].n2[2] == 0.8f);   /* through the normal indices */
        const float ray[6] = {0.5f, 0.5f, 3, 0, 0, -3}, t = 1.0f;
        bad += batch(1, &w.quads[2], &table[1], ray, &t, out, &took) != RT_OK || took != 1 || !(out[0] > 0.0f && out[2] > 0.9f);
        bad += batch(1, &w.quads[1], &table[0], ray, &t, out, &took) != RT_OK || took != 0 || !(out[0] == 0.0f && out[2] == 1.0f);
    }
    bad += set(NULL, NULL, 0) != RT_ERR_INVALID || strstr(rt_last_error(), "rt_renderer_shading_normals") == NULL;
    bad += set_multi(NULL, NULL, 0) != RT_ERR_INVALID;
    bad += info(NULL, NULL) != RT_ERR_INVALID;
    bad += probe == NULL;
    rt_scene_destroy(s);
    if (bad) { printf("smooth ABI: %d checks failed\n", bad); return 1; }
    printf("smooth ABI ok\n");
    return 0;
}

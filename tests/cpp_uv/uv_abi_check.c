/* rt_tri_uvs and the texture-coordinate entry points of include/rt06.h from plain C11 (-pedantic): sizes are compile-time assertions, the address of each
 * entry point is taken, and a small scene with texture coordinates is built, permuted and read back on the host.  No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_tri_uvs) == 24, "rt_tri_uvs is six floats");
_Static_assert(offsetof(rt_tri_uvs, t0) == 0 && offsetof(rt_tri_uvs, t1) == 8 && offsetof(rt_tri_uvs, t2) == 16, "t0, t1, t2");
_Static_assert(sizeof(rt_tri_normals) == 36, "rt_tri_normals stays nine floats");
_Static_assert(sizeof(rt_quad) == 80, "rt_quad stays 80 bytes: the texture coordinates travel beside the flat world");
_Static_assert(sizeof(rt_world_flat) == 128, "rt_world_flat stays 128 bytes");

int main(void) {
    int (*add_tri)(rt_scene*, const float[3], const float[3], const float[3], const float[3], const float[3], const float[3], const float[2], const float[2],
                   const float[2], int32_t, int32_t*) = rt_scene_add_triangle_uv;
    int (*add_mesh)(rt_scene*, uint32_t, const float*, uint32_t, const float*, uint32_t, const float*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*,
                    int32_t, float, float, const float[3], int32_t*, uint32_t*) = rt_scene_add_mesh_uv;
    int (*coords)(const rt_scene*, const rt_tri_uvs**, uint32_t*) = rt_scene_texture_coords;
    int (*batch)(size_t, const rt_quad*, const rt_tri_uvs*, const float*, const float*, float*) = rt_tri_uv_batch;
    int (*set)(rt_renderer*, const rt_tri_uvs*, uint32_t) = rt_renderer_texture_coords;
    int (*set_multi)(rt_multi_renderer*, const rt_tri_uvs*, uint32_t) = rt_multi_renderer_texture_coords;
    int (*info)(rt_renderer*, uint32_t[2]) = rt_renderer_texture_coords_info;
    int (*probe)(int, const rt_world_flat*, const rt_tri_uvs*, uint32_t, size_t, const float*, int32_t*, float*) = rt_probe_tri_uv;
    const float a[3] = {0, 0, 0}, b[3] = {2, 0, 0}, c[3] = {0, 2, 0}, grey[3] = {0.5f, 0.5f, 0.5f}, up[3] = {0, 0, 2};
    const float ta[2] = {0.25f, 0.5f}, tb[2] = {0.75f, 0.5f}, tc[2] = {0.25f, 1.5f}, bad_t[2] = {NAN, 0};
    const float xyz[9] = {0, 0, 1, 1, 0, 1, 0, 1, 1}, uvs[6] = {0.5f, 0.5f, 1.0f, 0.5f, 0.5f, 0.0f};
    const uint32_t face[3] = {0, 1, 2}, tface[3] = {2, 1, 0}, bad_tface[3] = {0, 1, 3};
    const rt_tri_uvs* table = NULL;
    const rt_tri_normals* normals = NULL;
    rt_scene* s = NULL;
    rt_world_flat w;
    int32_t mat = -1, quad = -1, first = -1;
    uint32_t n = 99, added = 99;
    float out[2] = {0, 0};
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &mat) != RT_OK;
    bad += rt_scene_add_triangle(s, a, b, c, mat, &quad) != RT_OK;
    bad += coords(s, &table, &n) != RT_OK || n != 0 || table != NULL;                               /* every record is the identity */
    bad += add_tri(s, a, b, c, NULL, NULL, NULL, ta, bad_t, tc, mat, NULL) != RT_ERR_INVALID;        /* a coordinate that is not finite */
    bad += add_tri(s, a, b, c, up, NULL, up, ta, tb, tc, mat, NULL) != RT_ERR_INVALID;               /* three normals or none */
    bad += add_tri(s, a, b, c, NULL, NULL, NULL, ta, tb, tc, mat, &quad) != RT_OK || quad != 1;
    bad += add_tri(s, a, b, c, up, up, up, ta, tb, tc, mat, &quad) != RT_OK || quad != 2;
    bad += add_mesh(s, 3, xyz, 0, NULL, 3, uvs, 1, face, NULL, bad_tface, mat, 1.0f, 0.0f, NULL, &first, &added) != RT_ERR_INVALID;   /* index 3 of 3 */
    bad += add_mesh(s, 3, xyz, 0, NULL, 3, uvs, 1, face, NULL, tface, mat, 1.0f, 0.0f, NULL, &first, &added) != RT_OK || first != 3 || added != 1;
    bad += rt_scene_add_quad(s, a, b, c, mat, &quad) != RT_OK || quad != 0;                          /* goes in front of the triangles: their records stay theirs */
    bad += rt_scene_set_world_list(s) != RT_OK;
    bad += rt_scene_get_flat(s, &w) != RT_OK || w.n_quads != 5;
    bad += coords(s, &table, &n) != RT_OK || n != 4 || table == NULL;
    bad += rt_scene_vertex_normals(s, &normals, &n) != RT_OK || n != 4 || normals == NULL;
    if (!bad) {
        bad += !(table[0].t0[0] == 0.0f && table[0].t1[0] == 1.0f && table[0].t2[1] == 1.0f && table[0].t1[1] == 0.0f);   /* the identity */
        bad += !(table[1].t0[0] == 0.25f && table[1].t1[0] == 0.75f && table[1].t2[1] == 1.5f);
        bad += !(normals[1].n0[2] == 0.0f && normals[2].n0[2] == 1.0f);                                                     /* flat, smooth */
        bad += !(table[3].t0[1] == 0.0f && table[3].t1[0] == 1.0f && table[3].t2[0] == 0.5f && table[3].t2[1] == 0.5f);   /* through the indices */
        const float ray[6] = {1, 0, 3, 0, 0, -3}, t = 1.0f;   /* the midpoint of ab */
        bad += batch(1, &w.quads[2], &table[1], ray, &t, out) != RT_OK || !(out[0] == 0.5f && out[1] == 0.5f);
        bad += batch(1, &w.quads[1], &table[0], ray, &t, out) != RT_OK || !(out[0] == 0.5f && out[1] == 0.0f);
    }
    bad += set(NULL, NULL, 0) != RT_ERR_INVALID || strstr(rt_last_error(), "rt_renderer_texture_coords") == NULL;
    bad += set_multi(NULL, NULL, 0) != RT_ERR_INVALID;
    bad += info(NULL, NULL) != RT_ERR_INVALID;
    bad += probe == NULL;
    rt_scene_destroy(s);
    if (bad) { printf("uv ABI: %d checks failed\n", bad); return 1; }
    printf("uv ABI ok\n");
    return 0;
}

/* The cutout entry points of include/rt06.h from plain C11 (-pedantic): the record's size and the kinds' values are compile-time assertions, the address of
 * each entry point is taken, a scene's cutout records are set, refused, cleared and read back, and the rule applied to a few cases, on the host.
 * No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_cutout) == 16, "rt_cutout has 16 bytes");
_Static_assert(offsetof(rt_cutout, image) == 4 && offsetof(rt_cutout, cutoff) == 8 && offsetof(rt_cutout, reserved) == 12, "on, image, cutoff, reserved");
_Static_assert(RT_CUTOUT_OFF == 0 && RT_CUTOUT_MASKED == 1, "the kinds' values");

int main(void) {
    int (*set)(rt_scene*, uint32_t, uint32_t, float) = rt_scene_set_cutout;
    int (*clear)(rt_scene*, uint32_t) = rt_scene_clear_cutout;
    int (*get)(const rt_scene*, const rt_cutout**, uint32_t*) = rt_scene_cutouts;
    int (*batch)(const rt_texture*, uint32_t, const uint8_t*, size_t, const rt_quad*, const rt_tri_uvs*, const float*, const float*, const rt_cutout*, uint32_t,
                 const uint32_t*, uint32_t*, float*, float*) = rt_cutout_batch;
    int (*probe)(int, const rt_texture*, uint32_t, const uint8_t*, size_t, const rt_quad*, const rt_tri_uvs*, const float*, const float*, const rt_cutout*, uint32_t,
                 const uint32_t*, uint32_t*, float*, float*) = rt_probe_cutout;
    int (*push)(rt_renderer*, const rt_cutout*, uint32_t) = rt_renderer_cutouts;
    int (*info)(rt_renderer*, uint32_t*) = rt_renderer_cutouts_info;
    int (*kernel)(rt_renderer*, uint32_t*) = rt_renderer_kernel_cutout;
    int (*multi)(rt_multi_renderer*, const rt_cutout*, uint32_t) = rt_multi_renderer_cutouts;
    int (*multi_info)(rt_multi_renderer*, uint32_t*) = rt_multi_renderer_cutouts_info;
    const float grey[3] = {0.5f, 0.5f, 0.5f}, tint[3] = {0.1f, 0.1f, 0.1f};
    /* a 2 x 1 mask, nearest and clamped: the left texel empty, the right one opaque; the unit square in the plane z = 0, met from above at (1/4, 1/2) and (3/4, 1/2) */
    const rt_texture tex[2] = {{0, 0, RT_WRAP_CLAMP, RT_FILTER_NEAREST, 0}, {2, 1, RT_WRAP_CLAMP, RT_FILTER_NEAREST, 0}};
    const uint8_t texels[6] = {0, 0, 0, 255, 255, 255};
    rt_quad q[3];
    const rt_tri_uvs flipped[3] = {{{1, 0}, {0, 0}, {1, 1}}, {{1, 0}, {0, 0}, {1, 1}}, {{1, 0}, {0, 0}, {1, 1}}};   /* u runs the other way */
    const float rays[18] = {0.25f, 0.5f, 2, 0, 0, -1, 0.75f, 0.5f, 2, 0, 0, -1, 0.25f, 0.5f, 2, 0, 0, -1}, t[3] = {2, 2, 2};
    const rt_cutout rec[3] = {{RT_CUTOUT_OFF, 0, 0, 0}, {RT_CUTOUT_MASKED, 1, 0.5f, 0}, {RT_CUTOUT_MASKED, 1, 0.0f, 0}};
    const uint32_t mat_on[3] = {1, 1, 0}, mat_zero[3] = {2, 2, 2}, mat_bad[3] = {1, 3, 1};
    uint32_t keep[3], n = 9;
    float uv[6], value[3];
    const rt_cutout* table = NULL;
    rt_scene* s = NULL;
    int32_t lam = -1, metal = -1, glass = -1, light = -1, fog = -1;
    int bad = 0, i;
    memset(q, 0, sizeof q);
    for (i = 0; i < 3; i++) { q[i].u[0] = 1; q[i].v[1] = 1; q[i].normal[2] = 1; q[i].w[2] = 1; }
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &lam) != RT_OK || rt_scene_add_material(s, RT_MAT_METAL, grey, 0.2f, NULL, &metal) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_DIELECTRIC, grey, 1.5f, NULL, &glass) != RT_OK || rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, grey, 0.0f, NULL, &light) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_ISOTROPIC, grey, 0.5f, NULL, &fog) != RT_OK;
    bad += set(s, (uint32_t)light, 1, 0.5f) != RT_ERR_INVALID || strstr(rt_last_error(), "whole area as emitting") == NULL;
    bad += set(s, (uint32_t)fog, 1, 0.5f) != RT_ERR_INVALID || strstr(rt_last_error(), "is a medium") == NULL;
    bad += set(s, 5, 1, 0.5f) != RT_ERR_INVALID || strstr(rt_last_error(), "no material 5") == NULL;
    bad += set(s, (uint32_t)lam, RT_MAX_IMAGES, 0.5f) != RT_ERR_INVALID || strstr(rt_last_error(), "image index") == NULL;
    bad += set(s, (uint32_t)lam, 1, -0.1f) != RT_ERR_INVALID || strstr(rt_last_error(), "cutoff") == NULL;
    bad += set(s, (uint32_t)lam, 1, 1.5f) != RT_ERR_INVALID || set(s, (uint32_t)lam, 1, NAN) != RT_ERR_INVALID || set(s, (uint32_t)lam, 1, INFINITY) != RT_ERR_INVALID;
    bad += set(NULL, 0, 1, 0.5f) != RT_ERR_INVALID;
    bad += get(s, &table, &n) != RT_OK || n != 0 || table != NULL;                                             /* the refusals changed nothing */
    bad += set(s, (uint32_t)metal, 3, 0.25f) != RT_OK || get(s, &table, &n) != RT_OK || n != 5 || table[metal].on != RT_CUTOUT_MASKED || table[metal].image != 3 ||
           table[metal].cutoff != 0.25f || table[metal].reserved != 0 || table[lam].on != RT_CUTOUT_OFF;
    bad += set(s, (uint32_t)lam, 0, -0.0f) != RT_OK || get(s, &table, &n) != RT_OK || table[lam].on != RT_CUTOUT_MASKED || signbit(table[lam].cutoff);   /* -0 is stored as 0 */
    bad += set(s, (uint32_t)lam, 2, 1.0f) != RT_OK || get(s, &table, &n) != RT_OK || table[lam].image != 2 || table[lam].cutoff != 1.0f;     /* the last call counts */
    /* a holed solid has no inside: either record refuses the other */
    bad += rt_scene_set_interior(s, (uint32_t)glass, tint) != RT_OK || set(s, (uint32_t)glass, 1, 0.5f) != RT_ERR_INVALID || strstr(rt_last_error(), "no inside") == NULL;
    bad += rt_scene_clear_interior(s, (uint32_t)glass) != RT_OK || set(s, (uint32_t)glass, 1, 0.5f) != RT_OK;
    bad += rt_scene_set_interior(s, (uint32_t)glass, tint) != RT_ERR_INVALID || strstr(rt_last_error(), "no inside") == NULL;
    bad += clear(s, (uint32_t)glass) != RT_OK || rt_scene_set_interior(s, (uint32_t)glass, tint) != RT_OK;
    bad += clear(s, (uint32_t)metal) != RT_OK || get(s, &table, &n) != RT_OK || n != 5 || table[metal].on != RT_CUTOUT_OFF || table[metal].image != 0;
    bad += clear(s, (uint32_t)lam) != RT_OK || clear(s, (uint32_t)light) != RT_OK || get(s, &table, &n) != RT_OK || n != 0 || table != NULL;
    bad += clear(s, 5) != RT_ERR_INVALID || clear(NULL, 0) != RT_ERR_INVALID || get(s, NULL, &n) != RT_ERR_INVALID;
    /* the rule: the empty texel turns the hit down, the opaque one keeps it, a record that is off asks nothing */
    bad += batch(tex, 2, texels, 3, q, NULL, rays, t, rec, 3, mat_on, keep, uv, value) != RT_OK;
    bad += !(keep[0] == 0 && uv[0] == 0.25f && uv[1] == 0.5f && value[0] == 0.0f && keep[1] == 1 && uv[2] == 0.75f && value[1] > 0.99f);
    bad += !(keep[2] == 1 && uv[4] == 0.0f && uv[5] == 0.0f && value[2] == 0.0f);
    bad += batch(tex, 2, texels, 3, q, flipped, rays, t, rec, 3, mat_on, keep, uv, value) != RT_OK;          /* under coordinates that run the other way */
    bad += !(keep[0] == 1 && uv[0] == 0.75f && uv[1] == 0.5f && keep[1] == 0 && uv[2] == 0.25f && keep[2] == 1);
    bad += batch(tex, 2, texels, 3, q, NULL, rays, t, rec, 3, mat_zero, keep, uv, value) != RT_OK || !(keep[0] == 1 && keep[1] == 1 && keep[2] == 1);   /* cutoff 0 keeps all */
    bad += batch(tex, 2, texels, 3, q, NULL, rays, t, rec, 3, mat_bad, keep, uv, value) != RT_ERR_INVALID || strstr(rt_last_error(), "no record 3") == NULL;
    bad += batch(tex, 2, texels, 3, NULL, NULL, rays, t, rec, 3, mat_on, keep, uv, value) != RT_ERR_INVALID;
    bad += batch(tex, 1, texels, 3, q, NULL, rays, t, rec, 3, mat_on, keep, uv, value) != RT_ERR_INVALID;   /* the mask's entry is missing */
    bad += push(NULL, NULL, 0) != RT_ERR_INVALID || info(NULL, &n) != RT_ERR_INVALID || kernel(NULL, &n) != RT_ERR_INVALID || multi(NULL, NULL, 0) != RT_ERR_INVALID ||
           multi_info(NULL, &n) != RT_ERR_INVALID;
    bad += probe == NULL;
    rt_scene_destroy(s);
    if (bad) {
        printf("cutouts ABI: %d checks failed (%s)\n", bad, rt_last_error());
        return 1;
    }
    printf("cutouts ABI ok\n");
    return 0;
}

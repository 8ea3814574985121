/* The solid-glass entry points of include/rt06.h from plain C11 (-pedantic): the record's size and the kinds' values are compile-time assertions, the address of
 * each entry point is taken, a scene's interior records are set, refused, cleared and read back, and the rule and rt_expf applied to a few cases, on the host.
 * No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_interior) == 16, "rt_interior has 16 bytes");
_Static_assert(offsetof(rt_interior, sigma) == 4, "on, then sigma");
_Static_assert(RT_INTERIOR_OFF == 0 && RT_INTERIOR_SOLID == 1, "the kinds' values");

int main(void) {
    int (*set)(rt_scene*, uint32_t, const float*) = rt_scene_set_interior;
    int (*clear)(rt_scene*, uint32_t) = rt_scene_clear_interior;
    int (*get)(const rt_scene*, const rt_interior**, uint32_t*) = rt_scene_interiors;
    int (*batch)(size_t, const float*, const float*, const float*, const float*, const float*, const float*, const uint32_t*, uint32_t*, float*, float*) = rt_interior_batch;
    int (*probe)(int, size_t, const float*, const float*, const float*, const float*, const float*, const float*, const uint32_t*, uint32_t*, float*, float*) = rt_probe_interior;
    int (*expf_host)(size_t, const float*, float*) = rt_expf_batch;
    int (*expf_probe)(int, size_t, const float*, float*) = rt_probe_expf;
    int (*push)(rt_renderer*, const rt_interior*, uint32_t) = rt_renderer_interiors;
    int (*info)(rt_renderer*, uint32_t*) = rt_renderer_interiors_info;
    int (*kernel)(rt_renderer*, uint32_t*) = rt_renderer_kernel_interior;
    int (*multi)(rt_multi_renderer*, const rt_interior*, uint32_t) = rt_multi_renderer_interiors;
    /* a slab whose stored normal is +y: entered from above; left from below after 1.5 of a direction of length 2, through sigma = (0, 1/2, 100); the same on a
     * sphere, where the shading normal decides and Ng is not read */
    const float Ng[9] = {0, 1, 0, 0, 1, 0, 1, 0, 0}, nn[9] = {0, 1, 0, 0, -1, 0, 0, 1, 0}, d[9] = {0, -2, 0, 0, 2, 0, 0, 2, 0};
    const float t[3] = {1.0f, 1.5f, 1.5f}, ior[3] = {1.5f, 1.5f, 1.5f}, sigma[9] = {0, 0.5f, 100, 0, 0.5f, 100, 0, 0.5f, 100};
    const uint32_t sphere[3] = {0, 0, 1};
    const float x[6] = {0.0f, -0.0f, -1.0f, -87.0f, -1000.0f, NAN}, grey[3] = {0.5f, 0.5f, 0.5f}, tint[3] = {0.25f, 0.0f, 2.0f}, minus[3] = {0.1f, -0.1f, 0.1f},
                inf[3] = {0.1f, INFINITY, 0.1f}, nan3[3] = {NAN, 0.1f, 0.1f}, none[3] = {-0.0f, 0.0f, 0.0f};
    uint32_t back[3], n = 9;
    float eta[3], T[9], y[6];
    const rt_interior* table = NULL;
    rt_scene* s = NULL;
    int32_t lam = -1, metal = -1, glass = -1, light = -1, glass2 = -1;
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &lam) != RT_OK || rt_scene_add_material(s, RT_MAT_METAL, grey, 0.2f, NULL, &metal) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_DIELECTRIC, grey, 1.5f, NULL, &glass) != RT_OK || rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, grey, 0.0f, NULL, &light) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_DIELECTRIC, grey, 1.33f, NULL, &glass2) != RT_OK;
    bad += set(s, (uint32_t)lam, tint) != RT_ERR_INVALID || strstr(rt_last_error(), "no dielectric") == NULL;
    bad += set(s, (uint32_t)metal, tint) != RT_ERR_INVALID || set(s, (uint32_t)light, tint) != RT_ERR_INVALID;
    bad += set(s, 5, tint) != RT_ERR_INVALID || strstr(rt_last_error(), "no material 5") == NULL;
    bad += set(s, (uint32_t)glass, minus) != RT_ERR_INVALID || strstr(rt_last_error(), "absorption coefficient") == NULL;
    bad += set(s, (uint32_t)glass, inf) != RT_ERR_INVALID || set(s, (uint32_t)glass, nan3) != RT_ERR_INVALID;
    bad += set(NULL, 0, tint) != RT_ERR_INVALID || set(s, (uint32_t)glass, NULL) != RT_ERR_INVALID;
    bad += get(s, &table, &n) != RT_OK || n != 0 || table != NULL;                                             /* the refusals changed nothing */
    bad += set(s, (uint32_t)glass, tint) != RT_OK || get(s, &table, &n) != RT_OK || n != 5 || table[glass].on != RT_INTERIOR_SOLID ||
           table[glass].sigma[0] != 0.25f || table[glass].sigma[1] != 0.0f || table[glass].sigma[2] != 2.0f || table[lam].on != RT_INTERIOR_OFF || table[glass2].on != RT_INTERIOR_OFF;
    bad += set(s, (uint32_t)glass2, none) != RT_OK || get(s, &table, &n) != RT_OK || table[glass2].on != RT_INTERIOR_SOLID || signbit(table[glass2].sigma[0]) ||
           table[glass2].sigma[0] != 0.0f;                                                                     /* -0 is stored as 0 */
    bad += clear(s, (uint32_t)glass) != RT_OK || get(s, &table, &n) != RT_OK || n != 5 || table[glass].on != RT_INTERIOR_OFF || table[glass].sigma[2] != 0.0f;
    bad += clear(s, (uint32_t)glass2) != RT_OK || clear(s, (uint32_t)lam) != RT_OK || get(s, &table, &n) != RT_OK || n != 0 || table != NULL;
    bad += clear(s, 5) != RT_ERR_INVALID || clear(NULL, 0) != RT_ERR_INVALID || get(s, NULL, &n) != RT_ERR_INVALID;
    bad += batch(3, Ng, nn, d, t, ior, sigma, sphere, back, eta, T) != RT_OK;
    bad += !(back[0] == 0 && eta[0] == 1 / 1.5f && T[0] == 1.0f && T[1] == 1.0f && T[2] == 1.0f);
    bad += !(back[1] == 1 && eta[1] == 1.5f && T[3] == 1.0f && fabsf(T[4] - 0.22313016f) < 1e-6f && T[5] == 0.0f);
    bad += !(back[2] == 1 && eta[2] == 1.5f && T[6] == 1.0f && T[7] == T[4] && T[8] == 0.0f);
    bad += batch(3, NULL, nn, d, t, ior, sigma, sphere, back, eta, T) != RT_ERR_INVALID || batch(3, Ng, nn, d, t, ior, sigma, sphere, back, eta, NULL) != RT_ERR_INVALID;
    bad += expf_host(6, x, y) != RT_OK || !(y[0] == 1.0f && y[1] == 1.0f && fabsf(y[2] - 0.36787944f) < 1e-7f && y[3] == 0.0f && y[4] == 0.0f && y[5] == 0.0f);
    bad += expf_host(6, NULL, y) != RT_ERR_INVALID;
    bad += push(NULL, NULL, 0) != RT_ERR_INVALID || info(NULL, &n) != RT_ERR_INVALID || kernel(NULL, &n) != RT_ERR_INVALID || multi(NULL, NULL, 0) != RT_ERR_INVALID;
    bad += probe == NULL || expf_probe == NULL;
    rt_scene_destroy(s);
    if (bad) {
        printf("interiors ABI: %d checks failed (%s)\n", bad, rt_last_error());
        return 1;
    }
    printf("interiors ABI ok\n");
    return 0;
}

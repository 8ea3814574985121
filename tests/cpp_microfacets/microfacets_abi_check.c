/* The microfacet entry points of include/rt06.h from plain C11 (-pedantic): sizes are compile-time assertions, the address of each entry point is taken, a
 * scene's records are set, refused, mapped, cleared and read back, and the rule applied to four cases, on the host.  No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_world_flat) == 128, "rt_world_flat stays 128 bytes: the table travels beside it");
_Static_assert(sizeof(rt_material) == 32, "rt_material stays 32 bytes");
_Static_assert(sizeof(rt_microfacet) == 16 && offsetof(rt_microfacet, roughness) == 8 && offsetof(rt_microfacet, specular) == 12, "rt_microfacet is one 16-byte record");
_Static_assert(RT_MICROFACET_OFF == 0 && RT_MICROFACET_CONSTANT == 1 && RT_MICROFACET_MAPPED == 2, "the kinds' values");
_Static_assert(RT_MFAC_SPECULAR == 1 && RT_MFAC_BASE == 2 && RT_MFAC_ABSORBED == 3 && RT_MFAC_BACKSIDE == 4, "the ways' values");

int main(void) {
    int (*set)(rt_scene*, uint32_t, float, float) = rt_scene_set_microfacet;
    int (*map)(rt_scene*, uint32_t, uint32_t) = rt_scene_set_roughness_map;
    int (*clear)(rt_scene*, uint32_t) = rt_scene_clear_microfacet;
    int (*get)(const rt_scene*, const rt_microfacet**, uint32_t*) = rt_scene_microfacets;
    int (*batch)(size_t, const float*, const float*, const float*, const float*, const uint32_t*, const uint32_t*, size_t, const uint32_t*, float*, float*, uint32_t*,
                 uint32_t*) = rt_microfacet_batch;
    int (*probe)(int, size_t, const float*, const float*, const float*, const float*, const uint32_t*, const uint32_t*, size_t, const uint32_t*, float*, float*, uint32_t*,
                 uint32_t*) = rt_probe_microfacet;
    int (*r_set)(rt_renderer*, const rt_microfacet*, uint32_t) = rt_renderer_microfacets;
    int (*r_info)(rt_renderer*, uint32_t[2]) = rt_renderer_microfacets_info;
    int (*r_kernel)(rt_renderer*, uint32_t*) = rt_renderer_kernel_microfacet;
    int (*m_set)(rt_multi_renderer*, const rt_microfacet*, uint32_t) = rt_multi_renderer_microfacets;
    int (*m_info)(rt_multi_renderer*, uint32_t[2]) = rt_multi_renderer_microfacets_info;
    /* a floor seen from straight above at the disk's centre (t1 = t2 = 0: the words of a signed draw of 0): a mirror bounce straight back up.  A conductor; a coat
     * whose toss (u = 1/4 < F = 1/2) is specular; the same with u = 3/4, which falls to the base; and the floor seen from below */
    const float normal[12] = {0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0}, ray_d[12] = {0, -2, 0, 0, -2, 0, 0, -2, 0, 0, 2, 0};
    const float roughness[4] = {0.5f, 0.5f, 0.5f, 0.5f}, f0[12] = {0.9f, 0.5f, 0.25f, 0.5f, 0, 0, 0.5f, 0, 0, 0.5f, 0, 0};
    const uint32_t coat[4] = {0, 1, 1, 1}, tape[6] = {0x800000u, 0x800000u, 0x400000u, 0x800000u, 0x800000u, 0xc00000u}, offsets[8] = {0, 2, 0, 3, 3, 3, 0, 0};
    const float grey[3] = {0.5f, 0.5f, 0.5f}, bad_rough[4] = {0.5f, 1.5f, 0.5f, 0.5f};
    float dir[12], weight[12];
    uint32_t path[4], draws[4], n = 9;
    const rt_microfacet* table = NULL;
    rt_scene* s = NULL;
    int32_t lam = -1, metal = -1, glass = -1, light = -1, fog = -1;
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &lam) != RT_OK || rt_scene_add_material(s, RT_MAT_METAL, grey, 0.2f, NULL, &metal) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_DIELECTRIC, grey, 1.5f, NULL, &glass) != RT_OK || rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, grey, 0.0f, NULL, &light) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_ISOTROPIC, grey, 0.5f, NULL, &fog) != RT_OK;
    bad += get(s, &table, &n) != RT_OK || n != 0 || table != NULL;                                           /* no record: no table */
    bad += map(s, (uint32_t)lam, 1) != RT_ERR_INVALID || strstr(rt_last_error(), "no microfacet record") == NULL;   /* a map needs a record */
    bad += set(s, (uint32_t)lam, 0.5f, 0.04f) != RT_OK || set(s, (uint32_t)metal, 0.25f, 0.0f) != RT_OK;
    bad += set(s, (uint32_t)glass, 0.5f, 0.04f) != RT_ERR_INVALID || strstr(rt_last_error(), "dielectric") == NULL;
    bad += set(s, (uint32_t)light, 0.5f, 0.04f) != RT_ERR_INVALID || set(s, (uint32_t)fog, 0.5f, 0.04f) != RT_ERR_INVALID;
    bad += set(s, 5, 0.5f, 0.04f) != RT_ERR_INVALID || strstr(rt_last_error(), "no material 5") == NULL;
    bad += set(s, (uint32_t)lam, -0.1f, 0.04f) != RT_ERR_INVALID || set(s, (uint32_t)lam, 1.5f, 0.04f) != RT_ERR_INVALID || set(s, (uint32_t)lam, NAN, 0.04f) != RT_ERR_INVALID;
    bad += set(s, (uint32_t)lam, 0.5f, -0.1f) != RT_ERR_INVALID || set(s, (uint32_t)lam, 0.5f, 1.5f) != RT_ERR_INVALID || set(s, (uint32_t)lam, 0.5f, INFINITY) != RT_ERR_INVALID;
    bad += map(s, (uint32_t)lam, RT_MAX_IMAGES) != RT_ERR_INVALID || map(s, 5, 1) != RT_ERR_INVALID;
    bad += get(s, &table, &n) != RT_OK || n != 5 || table[lam].on != RT_MICROFACET_CONSTANT || table[lam].roughness != 0.5f || table[lam].specular != 0.04f ||
           table[metal].roughness != 0.25f || table[glass].on != 0 || table[light].on != 0 || table[fog].on != 0;   /* the refusals changed nothing */
    bad += map(s, (uint32_t)lam, 3) != RT_OK || get(s, &table, &n) != RT_OK || table[lam].on != RT_MICROFACET_MAPPED || table[lam].image != 3 || table[lam].roughness != 0.5f;
    bad += set(s, (uint32_t)lam, 0.75f, 0.1f) != RT_OK || get(s, &table, &n) != RT_OK || table[lam].on != RT_MICROFACET_MAPPED || table[lam].image != 3 ||
           table[lam].roughness != 0.75f;                                                                     /* new values keep the map */
    bad += clear(s, (uint32_t)lam) != RT_OK || get(s, &table, &n) != RT_OK || n != 5 || table[lam].on != 0 || table[metal].on != 1;
    bad += clear(s, (uint32_t)metal) != RT_OK || get(s, &table, &n) != RT_OK || n != 0 || table != NULL;
    bad += clear(s, 5) != RT_ERR_INVALID;
    bad += batch(4, normal, ray_d, roughness, f0, coat, tape, 6, offsets, dir, weight, path, draws) != RT_OK;
    bad += !(path[0] == RT_MFAC_SPECULAR && draws[0] == 2 && dir[0] == 0.0f && dir[1] == 1.0f && dir[2] == 0.0f && weight[0] == 0.9f && weight[1] == 0.5f && weight[2] == 0.25f);
    bad += !(path[1] == RT_MFAC_SPECULAR && draws[1] == 3 && dir[4] == 1.0f && weight[3] == 1.0f && weight[4] == 1.0f && weight[5] == 1.0f);   /* the toss paid F */
    bad += !(path[2] == RT_MFAC_BASE && draws[2] == 3 && dir[7] == 0.0f && weight[6] == 0.0f);
    bad += !(path[3] == RT_MFAC_BACKSIDE && draws[3] == 0);
    bad += batch(4, normal, ray_d, bad_rough, f0, coat, tape, 6, offsets, dir, weight, path, draws) != RT_ERR_INVALID || strstr(rt_last_error(), "roughness") == NULL;
    bad += batch(4, normal, ray_d, roughness, f0, coat, tape, 5, offsets, dir, weight, path, draws) != RT_ERR_INVALID || strstr(rt_last_error(), "outside a tape") == NULL;
    bad += batch(4, NULL, ray_d, roughness, f0, coat, tape, 6, offsets, dir, weight, path, draws) != RT_ERR_INVALID;
    bad += batch(4, normal, ray_d, roughness, f0, coat, tape, 6, offsets, dir, weight, path, NULL) != RT_ERR_INVALID;
    bad += r_set(NULL, NULL, 0) != RT_ERR_INVALID || strstr(rt_last_error(), "rt_renderer_microfacets") == NULL;
    bad += r_info(NULL, NULL) != RT_ERR_INVALID || r_kernel(NULL, NULL) != RT_ERR_INVALID || m_set(NULL, NULL, 0) != RT_ERR_INVALID || m_info(NULL, NULL) != RT_ERR_INVALID;
    bad += get(NULL, &table, &n) != RT_ERR_INVALID || set(NULL, 0, 0.5f, 0.04f) != RT_ERR_INVALID || map(NULL, 0, 0) != RT_ERR_INVALID || clear(NULL, 0) != RT_ERR_INVALID;
    bad += probe == NULL;
    rt_scene_destroy(s);
    if (bad) { printf("microfacets ABI: %d checks failed\n", bad); return 1; }
    printf("microfacets ABI ok\n");
    return 0;
}

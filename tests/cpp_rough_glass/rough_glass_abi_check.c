/* The rough-glass entry points of include/rt06.h from plain C11 (-pedantic): the kinds' values are compile-time assertions, the address of each entry point is
 * taken, a scene's glass records are set, refused, mapped, cleared and read back, and the rule applied to four cases, on the host.  No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_microfacet) == 16, "rt_microfacet keeps its 16 bytes");
_Static_assert(RT_MICROFACET_GLASS == 4 && RT_MICROFACET_GLASS_MAPPED == 6, "the glass kinds' values");
_Static_assert(RT_MFAC_TRANSMITTED == 5 && RT_MFAC_SPECULAR == 1 && RT_MFAC_BASE == 2 && RT_MFAC_ABSORBED == 3, "the ways' values");

int main(void) {
    int (*set)(rt_scene*, uint32_t, float) = rt_scene_set_rough_glass;
    int (*batch)(size_t, const float*, const float*, const float*, const float*, const uint32_t*, size_t, const uint32_t*, float*, float*, uint32_t*, uint32_t*) =
        rt_rough_glass_batch;
    int (*probe)(int, size_t, const float*, const float*, const float*, const float*, const uint32_t*, size_t, const uint32_t*, float*, float*, uint32_t*, uint32_t*) =
        rt_probe_rough_glass;
    /* a pane seen from straight above at the disk's centre (t1 = t2 = 0: the words of a signed draw of 0), so M = n and F = 0.04: a toss of 2^-24 reflects straight
     * back, a toss of 1/2 goes straight through; the same from below, through; and the pane seen edge on, which is the smooth dielectric's */
    const float normal[12] = {0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0}, ray_d[12] = {0, -2, 0, 0, -2, 0, 0, 2, 0, 1, 0, 0};
    const float roughness[4] = {0.5f, 0.5f, 0.5f, 0.5f}, ior[4] = {1.5f, 1.5f, 1.5f, 1.5f}, bad_rough[4] = {0.5f, 1.5f, 0.5f, 0.5f};
    const uint32_t tape[4] = {0x800000u, 0x800000u, 1u, 0x800000u}, offsets[8] = {0, 3, 0, 2, 0, 2, 0, 3};
    const float grey[3] = {0.5f, 0.5f, 0.5f};
    float dir[12], weight[4];
    uint32_t path[4], draws[4], n = 9;
    const rt_microfacet* table = NULL;
    rt_scene* s = NULL;
    int32_t lam = -1, metal = -1, glass = -1, light = -1, fog = -1;
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &lam) != RT_OK || rt_scene_add_material(s, RT_MAT_METAL, grey, 0.2f, NULL, &metal) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_DIELECTRIC, grey, 1.5f, NULL, &glass) != RT_OK || rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, grey, 0.0f, NULL, &light) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_ISOTROPIC, grey, 0.5f, NULL, &fog) != RT_OK;
    bad += set(s, (uint32_t)lam, 0.5f) != RT_ERR_INVALID || strstr(rt_last_error(), "no dielectric") == NULL;
    bad += set(s, (uint32_t)metal, 0.5f) != RT_ERR_INVALID || set(s, (uint32_t)light, 0.5f) != RT_ERR_INVALID || set(s, (uint32_t)fog, 0.5f) != RT_ERR_INVALID;
    bad += set(s, 5, 0.5f) != RT_ERR_INVALID || strstr(rt_last_error(), "no material 5") == NULL;
    bad += set(s, (uint32_t)glass, -0.1f) != RT_ERR_INVALID || set(s, (uint32_t)glass, 1.5f) != RT_ERR_INVALID || set(s, (uint32_t)glass, NAN) != RT_ERR_INVALID;
    bad += set(NULL, 0, 0.5f) != RT_ERR_INVALID;
    bad += rt_scene_microfacets(s, &table, &n) != RT_OK || n != 0 || table != NULL;                             /* the refusals changed nothing */
    bad += rt_scene_set_microfacet(s, (uint32_t)glass, 0.5f, 0.04f) != RT_ERR_INVALID || strstr(rt_last_error(), "dielectric") == NULL;   /* as ever */
    bad += rt_scene_set_roughness_map(s, (uint32_t)glass, 1) != RT_ERR_INVALID || strstr(rt_last_error(), "no microfacet record") == NULL;
    bad += set(s, (uint32_t)glass, 0.25f) != RT_OK || rt_scene_microfacets(s, &table, &n) != RT_OK || n != 5 || table[glass].on != RT_MICROFACET_GLASS ||
           table[glass].image != 0 || table[glass].roughness != 0.25f || table[glass].specular != 0.0f || table[lam].on != 0;
    bad += rt_scene_set_roughness_map(s, (uint32_t)glass, 3) != RT_OK || rt_scene_microfacets(s, &table, &n) != RT_OK || table[glass].on != RT_MICROFACET_GLASS_MAPPED ||
           table[glass].image != 3 || table[glass].roughness != 0.25f;
    bad += set(s, (uint32_t)glass, 0.75f) != RT_OK || rt_scene_microfacets(s, &table, &n) != RT_OK || table[glass].on != RT_MICROFACET_GLASS_MAPPED ||
           table[glass].image != 3 || table[glass].roughness != 0.75f;                                            /* a new roughness keeps the map */
    bad += rt_scene_clear_microfacet(s, (uint32_t)glass) != RT_OK || rt_scene_microfacets(s, &table, &n) != RT_OK || n != 0 || table != NULL;
    bad += batch(4, normal, ray_d, roughness, ior, tape, 4, offsets, dir, weight, path, draws) != RT_OK;
    bad += !(path[0] == RT_MFAC_SPECULAR && draws[0] == 3 && dir[0] == 0.0f && dir[1] == 1.0f && dir[2] == 0.0f && weight[0] == 1.0f);
    bad += !(path[1] == RT_MFAC_TRANSMITTED && draws[1] == 3 && dir[3] == 0.0f && dir[4] == -1.0f && dir[5] == 0.0f && weight[1] == 1.0f);   /* past its end the tape serves 1/2 */
    bad += !(path[2] == RT_MFAC_TRANSMITTED && draws[2] == 3 && dir[7] == 1.0f && weight[2] == 1.0f);
    bad += !(path[3] == RT_MFAC_BASE && draws[3] == 0 && dir[9] == 0.0f && weight[3] == 0.0f);
    bad += batch(4, normal, ray_d, bad_rough, ior, tape, 4, offsets, dir, weight, path, draws) != RT_ERR_INVALID || strstr(rt_last_error(), "roughness") == NULL;
    bad += batch(4, normal, ray_d, roughness, ior, tape, 2, offsets, dir, weight, path, draws) != RT_ERR_INVALID || strstr(rt_last_error(), "outside a tape") == NULL;
    bad += batch(4, NULL, ray_d, roughness, ior, tape, 4, offsets, dir, weight, path, draws) != RT_ERR_INVALID;
    bad += batch(4, normal, ray_d, roughness, ior, tape, 4, offsets, dir, weight, path, NULL) != RT_ERR_INVALID;
    bad += probe == NULL;
    rt_scene_destroy(s);
    if (bad) { printf("rough glass ABI: %d checks failed\n", bad); return 1; }
    printf("rough glass ABI ok\n");
    return 0;
}

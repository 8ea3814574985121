/* The normal-map entry points of include/rt06.h from plain C11 (-pedantic): sizes are compile-time assertions, the address of each entry point is taken, a
 * scene's maps are set, refused, cleared and read back, and the rule applied to three cases, on the host.  No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(sizeof(rt_world_flat) == 128, "rt_world_flat stays 128 bytes: the table travels beside it");
_Static_assert(sizeof(rt_material) == 32, "rt_material stays 32 bytes");
_Static_assert(sizeof(rt_normal_map) == 16 && offsetof(rt_normal_map, strength) == 8, "rt_normal_map is one 16-byte record: on, image, strength, pad");
_Static_assert(RT_NMAP_REPLACED == 1 && RT_NMAP_FLAT == 2 && RT_NMAP_NO_TANGENT == 3 && RT_NMAP_NO_LENGTH == 4 && RT_NMAP_FACING == 5 && RT_NMAP_NO_FRAME == 6, "the paths' values");
_Static_assert(RT_NMAP_SURFACE_SPHERE == 0 && RT_NMAP_SURFACE_PLANAR == 1 && RT_NMAP_SURFACE_TRI_UV == 2 && RT_NMAP_SURFACE_GIVEN == 3, "the surfaces' values");

int main(void) {
    int (*set)(rt_scene*, uint32_t, uint32_t, float) = rt_scene_set_normal_map;
    int (*clear)(rt_scene*, uint32_t) = rt_scene_clear_normal_map;
    int (*get)(const rt_scene*, const rt_normal_map**, uint32_t*) = rt_scene_normal_maps;
    int (*batch)(const rt_texture*, uint32_t, const uint8_t*, size_t, const uint32_t*, const float*, const float*, const float*, const float*, const float*, const float*,
                 const float*, const uint32_t*, const float*, float*, uint32_t*) = rt_normal_map_batch;
    int (*probe)(int, const rt_texture*, uint32_t, const uint8_t*, size_t, const uint32_t*, const float*, const float*, const float*, const float*, const float*,
                 const float*, const float*, const uint32_t*, const float*, float*, uint32_t*) = rt_probe_normal_map;
    int (*r_set)(rt_renderer*, const rt_normal_map*, uint32_t) = rt_renderer_normal_maps;
    int (*r_info)(rt_renderer*, uint32_t[2]) = rt_renderer_normal_maps_info;
    int (*r_kernel)(rt_renderer*, uint32_t*) = rt_renderer_kernel_normal_map;
    int (*m_set)(rt_multi_renderer*, const rt_normal_map*, uint32_t) = rt_multi_renderer_normal_maps;
    int (*m_info)(rt_multi_renderer*, uint32_t[2]) = rt_multi_renderer_normal_maps_info;
    /* a 2 x 1 map: a flat texel and one leaning fully towards +u (x = 1, z = 0 after the decode) */
    const uint8_t map[2 * 3] = {128, 128, 255, 255, 128, 128};
    const rt_texture rec[1] = {{2, 1, RT_WRAP_CLAMP, RT_FILTER_NEAREST, 0}};
    /* a floor seen from above: the flat texel, the leaning one (the bent normal is the tangent: it grazes, and a ray straight down no longer faces it), and the
     * leaning one at strength 1/2 under a slanted ray */
    const uint32_t surface[3] = {RT_NMAP_SURFACE_PLANAR, RT_NMAP_SURFACE_PLANAR, RT_NMAP_SURFACE_GIVEN}, index[3] = {0, 0, 0};
    const float a[9] = {2, 0, 0, 2, 0, 0, 1, 0, 0}, b[9] = {0, 0, -3, 0, 0, -3, 0, 0, -1}, normal[9] = {0, 1, 0, 0, 1, 0, 0, 1, 0};
    const float ray_d[9] = {0, -1, 0, 0, -1, 0, -0.5f, -1, 0}, u[3] = {0.25f, 0.75f, 0.75f}, v[3] = {0.5f, 0.5f, 0.5f}, strength[3] = {1.0f, 1.0f, 0.5f};
    const float grey[3] = {0.5f, 0.5f, 0.5f};
    float out[9];
    uint32_t path[3], n = 9;
    const rt_normal_map* table = NULL;
    rt_scene* s = NULL;
    int32_t lam = -1, metal = -1, glass = -1, light = -1, fog = -1;
    int bad = 0;
    bad += rt_scene_create(&s) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_LAMBERTIAN, grey, 0.0f, NULL, &lam) != RT_OK || rt_scene_add_material(s, RT_MAT_METAL, grey, 0.2f, NULL, &metal) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_DIELECTRIC, grey, 1.5f, NULL, &glass) != RT_OK || rt_scene_add_material(s, RT_MAT_DIFFUSE_LIGHT, grey, 0.0f, NULL, &light) != RT_OK;
    bad += rt_scene_add_material(s, RT_MAT_ISOTROPIC, grey, 0.5f, NULL, &fog) != RT_OK;
    bad += get(s, &table, &n) != RT_OK || n != 0 || table != NULL;                                           /* no map: no table */
    bad += set(s, (uint32_t)lam, 1, 0.5f) != RT_OK || set(s, (uint32_t)metal, 0, 2.0f) != RT_OK;
    bad += set(s, (uint32_t)glass, 1, 1.0f) != RT_ERR_INVALID || strstr(rt_last_error(), "dielectric") == NULL;
    bad += set(s, (uint32_t)light, 1, 1.0f) != RT_ERR_INVALID || set(s, (uint32_t)fog, 1, 1.0f) != RT_ERR_INVALID;
    bad += set(s, 5, 1, 1.0f) != RT_ERR_INVALID || strstr(rt_last_error(), "no material 5") == NULL;
    bad += set(s, (uint32_t)lam, RT_MAX_IMAGES, 1.0f) != RT_ERR_INVALID || set(s, (uint32_t)lam, 1, -1.0f) != RT_ERR_INVALID || set(s, (uint32_t)lam, 1, NAN) != RT_ERR_INVALID;
    bad += get(s, &table, &n) != RT_OK || n != 5 || table[lam].on != 1 || table[lam].image != 1 || table[lam].strength != 0.5f || table[metal].strength != 2.0f ||
           table[glass].on != 0 || table[light].on != 0 || table[fog].on != 0;                                 /* the refusals changed nothing */
    bad += clear(s, (uint32_t)lam) != RT_OK || get(s, &table, &n) != RT_OK || n != 5 || table[lam].on != 0 || table[metal].on != 1;
    bad += clear(s, (uint32_t)metal) != RT_OK || get(s, &table, &n) != RT_OK || n != 0 || table != NULL;
    bad += clear(s, 5) != RT_ERR_INVALID;
    bad += batch(rec, 1, map, 3, surface, a, b, NULL, normal, ray_d, u, v, index, strength, out, path) != RT_OK;
    bad += !(path[0] == RT_NMAP_FLAT && out[0] == 0.0f && out[1] == 1.0f && out[2] == 0.0f);
    bad += !(path[1] == RT_NMAP_FACING && out[3] == 0.0f && out[4] == 1.0f && out[5] == 0.0f);
    bad += !(path[2] == RT_NMAP_REPLACED && out[6] == 1.0f && out[7] == 0.0f && out[8] == 0.0f);               /* z = 0: the bent normal is the tangent itself */
    bad += batch(rec, 1, map, 3, surface, a, b, NULL, normal, ray_d, u, v, surface, strength, out, path) != RT_ERR_INVALID || strstr(rt_last_error(), "no entry") == NULL;
    bad += r_set(NULL, NULL, 0) != RT_ERR_INVALID || strstr(rt_last_error(), "rt_renderer_normal_maps") == NULL;
    bad += r_info(NULL, NULL) != RT_ERR_INVALID || r_kernel(NULL, NULL) != RT_ERR_INVALID || m_set(NULL, NULL, 0) != RT_ERR_INVALID || m_info(NULL, NULL) != RT_ERR_INVALID;
    bad += probe == NULL;
    rt_scene_destroy(s);
    if (bad) { printf("normal maps ABI: %d checks failed\n", bad); return 1; }
    printf("normal maps ABI ok\n");
    return 0;
}

/* The environment-light-sampling entry points of include/rt06.h from plain C11 (-pedantic): the mode's value is a compile-time assertion, the address of each
 * entry point is taken, and the distribution of a small map is built, read and refused, and the rule applied to a few quadruples, on the host.  No GPU is touched. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(RT_LIGHT_SAMPLING_ENV == 32, "mode 32, beside 1, 2, 4 and 16");
_Static_assert(RT_LIGHT_SAMPLING_TREE == 16 && RT_LIGHT_SAMPLING_MESH == 4 && RT_LIGHT_SAMPLING_ALL == 2 && RT_LIGHT_SAMPLING_QUADS == 1, "the other modes keep their bits");

int main(void) {
    int (*dist)(uint32_t, uint32_t, const float*, float*, float*, float*, float*) = rt_environment_distribution;
    int (*batch)(size_t, uint32_t, uint32_t, const float*, float, const float*, float*, uint32_t*, float*) = rt_environment_sample_batch;
    int (*probe)(int, size_t, uint32_t, uint32_t, const float*, float, const float*, float*, uint32_t*, float*) = rt_probe_environment_sample;
    int (*family)(rt_renderer*, uint32_t*) = rt_renderer_kernel_env_light;
    /* a 4 x 2 map: black but for texel (2, 0) = white 3 and texel (1, 1) = white 1 */
    float map[4 * 2 * 3] = {0}, black[4 * 2 * 3] = {0};
    float rowc[2], rowy[3], colc[8], density[8];
    /* x1 small: the top row; x1 = 1: the bottom row.  a = b = 0.5: the middle of the texel */
    const float u[3 * 4] = {0.01f, 0.5f, 0.5f, 0.5f, 1.0f, 1.0f, 0.5f, 0.5f, 0.7f, 0.3f, 1.0f, 1.0f};
    float dir[3 * 3], dens[3], bad_u[4] = {0.5f, 0.0f, 0.5f, 0.5f};
    uint32_t texel[3], on = 7;
    int bad = 0;
    for (int k = 0; k < 3; k++) { map[(0 * 4 + 2) * 3 + k] = 3.0f; map[(1 * 4 + 1) * 3 + k] = 1.0f; }
    bad += dist(4, 2, map, rowc, rowy, colc, density) != RT_OK;
    bad += !(rowy[0] == 1.0f && fabsf(rowy[1]) < 1e-7f && rowy[2] == -1.0f);                /* the ends exactly; cos(pi / 2) in double is 6e-17 */
    bad += !(colc[0] == 0.0f && colc[1] == 0.0f && colc[2] == 3.0f && colc[3] == 3.0f);      /* h_0 = 1, luminance of white 3 = 3 (the weights add up to 1) */
    bad += !(colc[4] == 0.0f && colc[5] == 1.0f && colc[7] == 1.0f);
    bad += !(rowc[0] == 3.0f && rowc[1] == 4.0f);
    /* density = P / omega, omega = (2 pi / 4) * 1: 0.75 and 0.25 of the draws, and nothing elsewhere */
    bad += !(fabsf(density[2] - 0.75f / 1.5707964f) < 1e-6f && fabsf(density[5] - 0.25f / 1.5707964f) < 1e-6f);
    for (int i = 0; i < 8; i++) bad += (i != 2 && i != 5) && density[i] != 0.0f;
    bad += dist(4, 2, black, rowc, rowy, colc, density) != RT_ERR_INVALID || strstr(rt_last_error(), "all black") == NULL;
    bad += dist(4, 2, map, NULL, rowy, colc, density) != RT_ERR_INVALID;
    bad += dist(0, 2, map, rowc, rowy, colc, density) != RT_ERR_INVALID;
    map[0] = -1.0f;
    bad += dist(4, 2, map, rowc, rowy, colc, density) != RT_ERR_INVALID || strstr(rt_last_error(), "negative") == NULL;
    map[0] = 0.0f;
    bad += batch(3, 4, 2, map, 0.0f, u, dir, texel, dens) != RT_OK;
    bad += !(texel[0] == 2 && texel[1] == 5 && texel[2] == 2);                               /* only the two lit texels are ever drawn */
    bad += !(dir[1] == 0.5f && dir[4] == -0.5f && dir[7] == 1.0f);                           /* n.y: the middle of each band; b = 1: the band's upper edge */
    bad += !(dens[0] == density[2] && dens[1] == density[5]);
    for (int i = 0; i < 3; i++) bad += !(fabsf(dir[3 * i] * dir[3 * i] + dir[3 * i + 1] * dir[3 * i + 1] + dir[3 * i + 2] * dir[3 * i + 2] - 1.0f) < 1e-5f);
    bad += batch(1, 4, 2, map, 0.0f, bad_u, dir, texel, dens) != RT_ERR_INVALID || strstr(rt_last_error(), "(0, 1]") == NULL;
    bad += batch(1, 4, 2, map, 1.0f, u, dir, texel, dens) != RT_ERR_INVALID || strstr(rt_last_error(), "u0") == NULL;
    bad += batch(1, 4, 2, black, 0.0f, u, dir, texel, dens) != RT_ERR_INVALID || strstr(rt_last_error(), "all black") == NULL;
    bad += batch(0, 4, 2, map, 0.0f, NULL, NULL, NULL, NULL) != RT_OK;
    bad += rt_renderer_light_sampling_enable(NULL, RT_LIGHT_SAMPLING_ENV) != RT_ERR_INVALID;
    bad += family(NULL, &on) != RT_ERR_INVALID || family(NULL, NULL) != RT_ERR_INVALID;
    bad += probe == NULL;
    if (bad) { printf("env light ABI: %d checks failed\n", bad); return 1; }
    printf("env light ABI ok\n");
    return 0;
}

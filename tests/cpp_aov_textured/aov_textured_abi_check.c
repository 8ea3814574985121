/* The textured feature mode's entry points of include/rt06.h from plain C11 (-pedantic): the address of each one is taken, so the translation unit compiles only
 * if the header declares them in plain C and links only if librt06.so exports them.  No GPU is touched. */
#include <stdio.h>

#include "rt06.h"

int main(void) {
    int (*enable_mode)(rt_renderer*, uint32_t, uint32_t) = rt_renderer_aov_enable_mode;
    int (*aov_mode)(rt_renderer*, uint32_t*) = rt_renderer_aov_mode;
    int (*noise_batch)(const rt_perlin*, const float[3], float, const float*, size_t, float*) = rt_noise_value_batch;
    int (*noise_probe)(int, const rt_perlin*, const float[3], float, const float*, size_t, float*) = rt_probe_noise_value;
    static rt_perlin tables;   /* zeros: every gradient is 0, the turbulence 0, the marble albedo * (1 + sin(scale * z)) */
    const float albedo[3] = {0.5f, 0.25f, 1.0f}, point[3] = {1.5f, -2.25f, 0.0f};
    float rgb[3] = {-1.0f, -1.0f, -1.0f};
    uint32_t mode = 9u;
    int bad = 0;
    bad += !(RT_AOV_PLAIN == 0u && RT_AOV_TEXTURED == 1u);
    /* null handles and null arguments are refused before any device is touched */
    bad += enable_mode(NULL, 0, RT_AOV_TEXTURED) != RT_ERR_INVALID;
    bad += aov_mode(NULL, &mode) != RT_ERR_INVALID || mode != 9u;
    bad += noise_batch(NULL, albedo, 4.0f, point, 1, rgb) != RT_ERR_INVALID;
    bad += noise_batch(&tables, NULL, 4.0f, point, 1, rgb) != RT_ERR_INVALID;
    bad += noise_batch(&tables, albedo, 4.0f, NULL, 1, rgb) != RT_ERR_INVALID;
    bad += noise_batch(&tables, albedo, 4.0f, point, 1, NULL) != RT_ERR_INVALID;
    bad += noise_probe(0, NULL, albedo, 4.0f, point, 1, rgb) != RT_ERR_INVALID;
    bad += noise_probe(0, &tables, albedo, 4.0f, point, 1, NULL) != RT_ERR_INVALID;
    bad += noise_batch(&tables, albedo, 4.0f, point, 1, rgb) != RT_OK;
    bad += !(rgb[0] == 0.5f && rgb[1] == 0.25f && rgb[2] == 1.0f);   /* z = 0 and no turbulence: sin(0) = 0 */
    if (bad) { printf("textured feature ABI: %d checks failed\n", bad); return 1; }
    printf("textured feature ABI ok\n");
    return 0;
}

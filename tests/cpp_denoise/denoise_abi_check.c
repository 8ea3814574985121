/* The feature-buffer and denoiser entry points of include/rt06.h from plain C11 (-pedantic): the address of each one is taken, so the
 * translation unit compiles only if the header declares them in plain C and links only if librt06.so exports them.  No GPU is touched. */
#include <stdio.h>

#include "rt06.h"

int main(void) {
    int (*aov_enable)(rt_renderer*, uint32_t) = rt_renderer_aov_enable;
    int (*aov_info)(rt_renderer*, uint64_t[3]) = rt_renderer_aov_info;
    int (*aov_download)(rt_renderer*, float*, size_t) = rt_renderer_aov_download;
    int (*params_default)(rt_denoise_params*) = rt_denoise_params_default;
    int (*denoise)(rt_renderer*, const rt_denoise_params*) = rt_renderer_denoise;
    int (*denoise_async)(rt_renderer*, void*, const rt_denoise_params*) = rt_renderer_denoise_async;
    int (*denoise_download)(rt_renderer*, float*, size_t) = rt_renderer_denoise_download;
    rt_denoise_params dp;
    uint64_t info[3];
    float px[8];
    int bad = 0;
    bad += params_default(&dp) != RT_OK;
    bad += !(dp.iterations == 5 && dp.demodulate == 1 && dp.sigma_depth > 0.0f && dp.sigma_lum > 0.0f);
    /* null handles and null arguments are refused before any device is touched */
    bad += params_default(NULL) != RT_ERR_INVALID;
    bad += aov_enable(NULL, 0) != RT_ERR_INVALID;
    bad += aov_info(NULL, info) != RT_ERR_INVALID;
    bad += aov_download(NULL, px, 8) != RT_ERR_INVALID;
    bad += denoise(NULL, &dp) != RT_ERR_INVALID;
    bad += denoise_async(NULL, NULL, &dp) != RT_ERR_INVALID;
    bad += denoise_download(NULL, px, 4) != RT_ERR_INVALID;
    if (bad) { printf("denoise ABI: %d checks failed\n", bad); return 1; }
    printf("denoise ABI ok\n");
    return 0;
}

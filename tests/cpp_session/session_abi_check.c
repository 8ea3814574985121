/* The session entry points of include/rt06.h from plain C11 (-pedantic): the address of each one is taken, so the translation unit
 * compiles only if the header declares them in plain C and links only if librt06.so exports them.  No GPU is touched. */
#include <stdio.h>

#include "rt06.h"

int main(void) {
    int (*set_camera)(rt_renderer*, const rt_camera*) = rt_renderer_set_camera;
    int (*multi_set_camera)(rt_multi_renderer*, const rt_camera*) = rt_multi_renderer_set_camera;
    int (*refine)(rt_renderer*, uint32_t) = rt_renderer_refine;
    int (*refine_async)(rt_renderer*, void*, float*, uint32_t) = rt_renderer_refine_async;
    int (*refine_reset)(rt_renderer*) = rt_renderer_refine_reset;
    int (*refine_info)(rt_renderer*, uint64_t[3]) = rt_renderer_refine_info;
    int (*download_sums)(rt_renderer*, float*, size_t) = rt_renderer_refine_download_sums;
    int (*noise)(rt_renderer*, double*) = rt_renderer_refine_noise;
    int (*multi_refine)(rt_multi_renderer*, uint32_t) = rt_multi_renderer_refine;
    /* null handles are refused before any device is touched */
    rt_camera cam;
    uint64_t info[3];
    double v;
    float px[4];
    int bad = 0;
    cam.type = RT_CAM_PINHOLE;
    bad += set_camera(NULL, &cam) != RT_ERR_INVALID;
    bad += multi_set_camera(NULL, &cam) != RT_ERR_INVALID;
    bad += refine(NULL, 1) != RT_ERR_INVALID;
    bad += refine_async(NULL, NULL, NULL, 1) != RT_ERR_INVALID;
    bad += refine_reset(NULL) != RT_ERR_INVALID;
    bad += refine_info(NULL, info) != RT_ERR_INVALID;
    bad += download_sums(NULL, px, 4) != RT_ERR_INVALID;
    bad += noise(NULL, &v) != RT_ERR_INVALID;
    bad += multi_refine(NULL, 1) != RT_ERR_INVALID;
    if (bad) { printf("session ABI: %d entry points accepted a null handle\n", bad); return 1; }
    printf("session ABI ok\n");
    return 0;
}

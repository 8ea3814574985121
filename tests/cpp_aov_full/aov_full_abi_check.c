/* The full feature mode of include/rt06.h from plain C11 (-pedantic): the constant, and the two entry points that take and report it, whose addresses are taken, so
 * the translation unit compiles only if the header declares them in plain C and links only if librt06.so exports them.  No GPU is touched. */
#include <stdio.h>
#include <string.h>

#include "rt06.h"

int main(void) {
    int (*enable_mode)(rt_renderer*, uint32_t, uint32_t) = rt_renderer_aov_enable_mode;
    int (*aov_mode)(rt_renderer*, uint32_t*) = rt_renderer_aov_mode;
    int (*cutouts)(rt_renderer*, const rt_cutout*, uint32_t) = rt_renderer_cutouts;
    uint32_t mode = 9u;
    int bad = 0;
    bad += !(RT_AOV_PLAIN == 0u && RT_AOV_TEXTURED == 1u && RT_AOV_FULL == 2u);
    /* null handles are refused before any device is touched, in every mode, and the message names the entry point */
    bad += enable_mode(NULL, 0, RT_AOV_FULL) != RT_ERR_INVALID;
    bad += strstr(rt_last_error(), "rt_renderer_aov_enable_mode") == NULL;
    bad += enable_mode(NULL, 4, RT_AOV_FULL + 1u) != RT_ERR_INVALID;
    bad += aov_mode(NULL, &mode) != RT_ERR_INVALID || mode != 9u;
    bad += cutouts(NULL, NULL, 0) != RT_ERR_INVALID;
    if (bad) { printf("full feature ABI: %d checks failed\n", bad); return 1; }
    printf("full feature ABI ok\n");
    return 0;
}

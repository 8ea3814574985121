/* Light-sampling mode 48 of include/rt06.h from plain C11 (-pedantic): the mode's value is a compile-time assertion, the entry points that take it and report it
 * are addressed and refuse a null handle.  No GPU is touched. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

_Static_assert(RT_LIGHT_SAMPLING_ENV_TREE == 48, "mode 48");
_Static_assert(RT_LIGHT_SAMPLING_ENV_TREE == (RT_LIGHT_SAMPLING_TREE | RT_LIGHT_SAMPLING_ENV), "the light tree's bit and the map's");
_Static_assert(RT_LIGHT_SAMPLING_ENV == 32 && RT_LIGHT_SAMPLING_TREE == 16 && RT_LIGHT_SAMPLING_MESH == 4 && RT_LIGHT_SAMPLING_ALL == 2 && RT_LIGHT_SAMPLING_QUADS == 1,
               "the other modes keep their bits");

int main(void) {
    int (*enable)(rt_renderer*, uint32_t) = rt_renderer_light_sampling_enable;
    int (*enable_all)(rt_multi_renderer*, uint32_t) = rt_multi_renderer_light_sampling_enable;
    int (*info)(rt_renderer*, uint32_t[2]) = rt_renderer_light_sampling_info;
    int (*tree)(rt_renderer*, uint32_t*) = rt_renderer_kernel_light_tree;
    int (*map)(rt_renderer*, uint32_t*) = rt_renderer_kernel_env_light;
    uint32_t out[2] = {7, 7};
    int bad = 0;
    bad += enable(NULL, RT_LIGHT_SAMPLING_ENV_TREE) != RT_ERR_INVALID || strstr(rt_last_error(), "rt_renderer_light_sampling_enable") == NULL;
    bad += enable_all(NULL, RT_LIGHT_SAMPLING_ENV_TREE) != RT_ERR_INVALID;
    bad += info(NULL, out) != RT_ERR_INVALID;
    bad += tree(NULL, out) != RT_ERR_INVALID || map(NULL, out) != RT_ERR_INVALID;
    bad += !(out[0] == 7 && out[1] == 7);
    if (bad) { printf("env tree ABI: %d checks failed\n", bad); return 1; }
    printf("env tree ABI ok\n");
    return 0;
}

/* The lens cameras of include/rt06.h from plain C11 (-pedantic): the record keeps its size, the four type values, the constructors and the host batch, whose
 * addresses are taken, so the translation unit compiles only if the header declares them in plain C and links only if librt06.so exports them.  No GPU is touched. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "rt06.h"

typedef int (*lens_ctor)(const float[3], const float[3], const float[3], float, float, float, float, float, float, rt_camera*);

int main(void) {
    const lens_ctor ctors[4] = {rt_camera_perspective, rt_camera_orthographic, rt_camera_fisheye, rt_camera_panorama};
    int (*batch)(const rt_camera*, size_t, const float*, const uint32_t*, size_t, const uint32_t*, float*, uint32_t*) = rt_camera_rays_batch;
    int (*probe)(int, const rt_camera*, size_t, const float*, const uint32_t*, size_t, const uint32_t*, float*, uint32_t*) = rt_probe_camera_lens;
    const float from[3] = {0, 0, 0}, at[3] = {1, 0, 0}, up[3] = {0, 1, 0};
    const float p0[4] = {40.0f, 2.0f, 180.0f, 360.0f}, p1[4] = {1.5f, 1.5f, 1.5f, 180.0f};
    const float st[2] = {0.0f, 0.0f};
    const uint32_t tape[4] = {0x800001u, 0x800001u, 0x400000u, 0x400000u}, offsets[2] = {0u, 4u};
    float ray[7];
    uint32_t draws = 99u;
    rt_camera cam, defocus;
    int bad = 0, i;
    bad += !(sizeof(rt_camera) == 76 && offsetof(rt_camera, viewport_width) == 52 && offsetof(rt_camera, t1) == 72);
    bad += !(RT_CAM_PINHOLE == 0 && RT_CAM_DEFOCUS == 1 && RT_CAM_MOTION == 2);
    bad += !(RT_CAM_PERSPECTIVE == 16 && RT_CAM_ORTHOGRAPHIC == 17 && RT_CAM_FISHEYE == 18 && RT_CAM_PANORAMA == 19);
    for (i = 0; i < 4; i++) {
        memset(&cam, 0xff, sizeof cam);
        bad += ctors[i](from, at, up, p0[i], p1[i], 0.2f, 3.0f, 0.0f, 1.0f, &cam) != RT_OK;
        bad += cam.type != 16u + (uint32_t)i || cam.lens_radius != 0.1f || cam.focus_dist != 3.0f || cam.t1 != 1.0f;
        bad += batch(&cam, 1, st, tape, 4, offsets, ray, &draws) != RT_OK || draws != 3u;   /* the lens point, then the time */
        bad += ctors[i](from, at, up, p0[i], p1[i], 0.2f, 3.0f, 0.0f, 1.0f, NULL) != RT_ERR_INVALID;
        bad += ctors[i](from, at, up, p0[i], p1[i], -1.0f, 3.0f, 0.0f, 1.0f, &cam) != RT_ERR_INVALID || strstr(rt_last_error(), "lens_radius") == NULL;
        bad += cam.lens_radius != 0.1f;   /* a refused call writes nothing */
    }
    /* rt_camera_perspective's basis and viewport are rt_camera_defocus's */
    bad += rt_camera_defocus(from, at, up, 40.0f, 1.5f, 0.2f, 3.0f, &defocus) != RT_OK;
    bad += rt_camera_perspective(from, at, up, 40.0f, 1.5f, 0.2f, 3.0f, 0.0f, 0.0f, &cam) != RT_OK;
    defocus.type = RT_CAM_PERSPECTIVE; defocus.t0 = 0.0f; defocus.t1 = 0.0f;
    bad += memcmp(&cam, &defocus, sizeof cam) != 0;
    /* the types between and beyond stay unknown, and the probe refuses before any device is touched */
    cam.type = 3u;
    bad += batch(&cam, 1, st, tape, 4, offsets, ray, &draws) != RT_ERR_INVALID || strstr(rt_last_error(), "unknown camera type") == NULL;
    cam.type = 20u;
    bad += probe(0, &cam, 1, st, tape, 4, offsets, ray, &draws) != RT_ERR_INVALID || strstr(rt_last_error(), "unknown camera type") == NULL;
    bad += probe(0, NULL, 1, st, tape, 4, offsets, ray, &draws) != RT_ERR_INVALID;
    if (bad) { printf("lens cameras ABI: %d checks failed\n", bad); return 1; }
    printf("lens cameras ABI ok\n");
    return 0;
}

/* rt_oracle_draws.inc — the oracle's functions that take uniforms: cuRandomInUnit<2> / cuRandomOnUnit<3>, Material::Scatter and
 * the cameras' sample_ray.  Included twice by rt_oracle.c: with the build's generator (rng_t, the names as they are: the render
 * path) and with a tape of k (u = k * 2^-24, names suffixed _tape: orc_scatter_tape / orc_camera_tape, for the edges the
 * generator's stream never reaches).  One text, so the two cannot differ; no per-draw mode test reaches orc_render.
 *   DRAW_GEN      the generator type
 *   DRAW_NEXT(g)  the next uniform in (0, 1]
 *   DRAW_FN(name) the name of a function of this file for that generator */
/* glm::cuRandomInUnit<2>, utilities/glm_utils.h:84-90 */
static inline void DRAW_FN(rng_in_unit2)(DRAW_GEN* g, float* ox, float* oy) {
    for (;;) {
        float x = DRAW_NEXT(g) * 2.0f - 1.0f;
        float y = DRAW_NEXT(g) * 2.0f - 1.0f;
        if (length2_2(x, y) < 1.0f) { *ox = x; *oy = y; return; }
    }
}
/* glm::cuRandomOnUnit<3>, utilities/glm_utils.h:92-98 */
static inline v3 DRAW_FN(rng_on_unit3)(DRAW_GEN* g) {
    for (;;) {
        v3 v;
        v.x = DRAW_NEXT(g) * 2.0f - 1.0f;
        v.y = DRAW_NEXT(g) * 2.0f - 1.0f;
        v.z = DRAW_NEXT(g) * 2.0f - 1.0f;
        if (!near_zero(v) && length2_3(v) < 1.0f) return normalize(v);
    }
}

/* Material::Scatter for the four material classes:
 *  LambertianAbstract  …/shaders/cu_materials.cuh:52-64
 *  MetalAbstract       :77-95
 *  DielectricAbstract  :115-143
 *  LambertianTexture   :27-40 */
static int DRAW_FN(material_scatter)(const orc_material* m, const ray_t* in_ray, const rec_t* rec, DRAW_GEN* g,
                            ray_t* out, v3* attenuation, const orc_world* w) {
    v3 normal = rec->normal;
    if (m->type == 4) return 0; /* diffuse_light of "The Next Week": emits (material_emitted), never scatters */
    switch (m->type) {
    case 0:
    case 3:
    case 6:   /* lambertian(noise_texture) */
    case 7: { /* lambertian(image_texture) */
        v3 ray_dir = add(normal, DRAW_FN(rng_on_unit3)(g));
        if (near_zero(ray_dir)) return 0;
        out->o = ray_at(in_ray, rec->distance); out->d = ray_dir; out->time = in_ray->time;
        if (m->type == 0) *attenuation = ld3(m->albedo);
        else if (m->type == 3) *attenuation = checker_value(m, ray_at(in_ray, rec->distance));
        else if (m->type == 6) *attenuation = noise_value(w->perlin, ld3(m->albedo), m->param, ray_at(in_ray, rec->distance));
        else if (rec->prim >= 0 && (uint32_t)rec->prim >= w->n_prims)
            *attenuation = image_value_quad(w->image, w->image_width, w->image_height, &w->quads[(uint32_t)rec->prim - w->n_prims], ray_at(in_ray, rec->distance));
        else *attenuation = image_value(w->image, w->image_width, w->image_height, normal);
        return 1;
    }
    case 1: {
        v3 refl = reflect(in_ray->d, normal);
        v3 scatter_dir = add(refl, muls(DRAW_FN(rng_on_unit3)(g), m->param));
        if (dot(scatter_dir, normal) < 0 || near_zero(scatter_dir)) return 0;
        out->o = ray_at(in_ray, rec->distance); out->d = scatter_dir; out->time = in_ray->time;
        *attenuation = ld3(m->albedo);
        return 1;
    }
    case 5: { /* isotropic phase function of "The Next Week" (extension): a uniformly random direction, always scatters */
        out->o = ray_at(in_ray, rec->distance); out->d = DRAW_FN(rng_on_unit3)(g); out->time = in_ray->time;
        *attenuation = ld3(m->albedo);
        return 1;
    }
    default: {
        float ior = m->param;
        int hit_backface = dot(in_ray->d, normal) > 0; /* isBackfacing, ray_data.cuh:44-46 */
        if (hit_backface) normal = neg(normal);
        float ior_ratio = hit_backface ? ior : 1 / ior;
        v3 unit_dir = normalize(in_ray->d);
        float cos_theta = fminf(dot(neg(unit_dir), normal), 1.0f);
        float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
        float reflect_prob = reflectance(cos_theta, ior_ratio);
        v3 scatter_dir;
        if (ior_ratio * sin_theta > 1.0f || reflect_prob > DRAW_NEXT(g))
            scatter_dir = reflect(unit_dir, normal);
        else
            scatter_dir = refract(unit_dir, normal, ior_ratio);
        out->o = ray_at(in_ray, rec->distance); out->d = scatter_dir; out->time = in_ray->time;
        *attenuation = ld3(m->albedo);
        return 1;
    }
    }
}

/* sample_ray :27-30 (pinhole), :54-64 (defocus), :87-89 (motion) */
static inline ray_t DRAW_FN(camera_sample_ray)(const orc_camera* c, float s, float t, DRAW_GEN* g) {
    ray_t r;
    v3 o = ld3(c->o), u = ld3(c->u), v = ld3(c->v), w = ld3(c->w);
    if (c->type == 1) {
        float dx, dy;
        DRAW_FN(rng_in_unit2)(g, &dx, &dy);
        v3 offset = add(muls(u, dx), muls(v, dy));
        offset = muls(offset, c->lens_radius);
        v3 forward = muls(w, c->focus_dist);
        v3 hori = muls(muls(u, c->viewport_width), c->focus_dist);
        v3 vert = muls(muls(v, c->viewport_height), c->focus_dist);
        r.o = add(o, offset);
        r.d = sub(add(add(forward, muls(hori, s)), muls(vert, t)), offset);
        r.time = 0.0f;
    } else {
        r.o = o;
        r.d = add(add(w, muls(u, s)), muls(v, t));
        r.time = (c->type == 2) ? mix1(c->t0, c->t1, DRAW_NEXT(g)) : 0.0f;
    }
    return r;
}


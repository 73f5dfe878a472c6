/* fan_ref.c -- a plain-C restatement of the occlusion fan's definition (include/rt_abi.h),
 * compiled at test time with cc -O2 -ffp-contract=off (tests/fan_common.py).  It shares no code with
 * csrc/host/fan_expand.cpp or the kernel: the tests hold rt_fan_expand against it word for word.
 *
 * origins: n records of 8 words {o.xyz, tmax, n.xyz, reserved}; dirs: k records of 4 words {d.xyz, -};
 * rays: n * k records of 8 words {o.xyz, tmax, d.xyz, 0}, ray (i, j) at i * k + j; traced: n * k bytes. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static int is_finite(float x) { return !isnan(x) && !isinf(x); }

/* the ray queries' validity rule: finite origin and direction, non-zero direction, tmax > 0.001f (no NaN) */
static int ray_valid(const float* o, float tmax, const float* d) {
    int c;
    for (c = 0; c < 3; ++c)
        if (!is_finite(o[c]) || !is_finite(d[c])) return 0;
    if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) return 0;
    if (isnan(tmax)) return 0;
    return tmax > 0.001f;
}

void fan_ref_expand(const uint32_t* origins, int64_t n, const uint32_t* dirs, int32_t k, uint32_t* rays, uint8_t* traced) {
    int64_t i;
    int32_t j;
    for (i = 0; i < n; ++i) {
        float o[8];
        memcpy(o, origins + 8 * i, 32);
        for (j = 0; j < k; ++j) {
            float d[4];
            uint32_t* r = rays + 8 * (i * k + j);
            int ok;
            memcpy(d, dirs + 4 * j, 16);
            memcpy(r, origins + 8 * i, 16);      /* o.xyz and the tmax word, bit for bit */
            memcpy(r + 4, dirs + 4 * j, 12);     /* d.xyz */
            r[7] = 0u;
            ok = ray_valid(o, o[3], d) && is_finite(o[4]) && is_finite(o[5]) && is_finite(o[6]);
            if (ok && !(o[4] == 0.0f && o[5] == 0.0f && o[6] == 0.0f)) {
                const float facing = fmaf(o[6], d[2], fmaf(o[5], d[1], o[4] * d[0]));
                ok = facing > 0.0f;
            }
            traced[i * k + j] = (uint8_t)ok;
        }
    }
}

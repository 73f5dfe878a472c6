// fan_expand.cpp -- rt_fan_expand (include/rt_abi.h): the definition of an occlusion fan
// in host code.  Ray (i, j) = {o_i, tmax_i, dirs[j].xyz}; it is traced iff it is a valid ray by the ray
// queries' rule (query_ray_ok of csrc/rt_kernel_body.inc), n_i is finite, and n_i is zero or
// dot(n_i, d_j) > 0 with rt_device_math.h's dot on the raw input words.  fan_kernel computes the same
// flag per lane; this file is what the tests hold it against.  No context, no GPU.
#include <cmath>
#include <cstdint>

#include "rt_abi.h"

namespace {

constexpr float kTmin = 0.001f;   // volumeRender.cl:640
constexpr int64_t kMaxFanOrigins = 1ll << 26;

inline bool finite3(float x, float y, float z) {
    return std::fabs(x) < INFINITY && std::fabs(y) < INFINITY && std::fabs(z) < INFINITY;
}

}  // namespace

extern "C" int rt_fan_expand(const rt_fan_origin* origins, int64_t n, const rt_float4* dirs, int32_t k, rt_ray* rays,
                             uint8_t* traced) {
    if (n < 0 || n > kMaxFanOrigins) return RT_ERR_INVALID_ARG;
    if (n == 0) return RT_OK;
    if (k < 1 || k > RT_FAN_MAX_DIRS) return RT_ERR_INVALID_ARG;
    if (!origins || !dirs || !rays || !traced) return RT_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; ++i) {
        const rt_fan_origin& o = origins[i];
        const bool origin_ok = finite3(o.ox, o.oy, o.oz) && o.tmax > kTmin;   // (false for a NaN tmax too)
        const bool normal_ok = finite3(o.nx, o.ny, o.nz);
        const bool no_cull = o.nx == 0.0f && o.ny == 0.0f && o.nz == 0.0f;
        for (int32_t j = 0; j < k; ++j) {
            const rt_float4& d = dirs[j];
            rt_ray& r = rays[i * k + j];
            r.ox = o.ox; r.oy = o.oy; r.oz = o.oz; r.tmax = o.tmax;
            r.dx = d.x; r.dy = d.y; r.dz = d.z; r.reserved = 0u;
            const bool dir_ok = finite3(d.x, d.y, d.z) && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
            // opencl.bc _Z3dotDv3_fS_: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), a = n_i, b = d_j
            const float facing = std::fmaf(o.nz, d.z, std::fmaf(o.ny, d.y, o.nx * d.x));
            traced[i * k + j] = (origin_ok && dir_ok && normal_ok && (no_cull || facing > 0.0f)) ? 1 : 0;
        }
    }
    return RT_OK;
}

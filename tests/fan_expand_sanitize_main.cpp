// Drives csrc/host/fan_expand.cpp (rt_fan_expand) alone under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_fan.py): the edge set of the rule (normals zero, -0, NaN, inf,
// 1e30; directions zero, NaN, inf, subnormal, axis-aligned, 1e30; tmax 0.001, the float above it, +inf,
// NaN) into buffers of exactly n * k records, the largest k, and hostile sizes, which must be refused
// before a byte is read or written.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_abi.h"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

const float kInf = std::numeric_limits<float>::infinity();
const float kNan = std::numeric_limits<float>::quiet_NaN();
const float kSub = std::numeric_limits<float>::denorm_min();

rt_fan_origin origin(float tmax, float nx, float ny, float nz) {
    rt_fan_origin o{};
    o.ox = 0.5f; o.oy = -0.25f; o.oz = 2.0f; o.tmax = tmax;
    o.nx = nx; o.ny = ny; o.nz = nz; o.reserved = 0xDEADBEEFu;
    return o;
}

// the rule, restated: what traced[i * k + j] must be
bool want(const rt_fan_origin& o, const rt_float4& d) {
    const float v[6] = {o.ox, o.oy, o.oz, d.x, d.y, d.z};
    for (float x : v)
        if (std::isnan(x) || std::isinf(x)) return false;
    if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) return false;
    if (!(o.tmax > 0.001f)) return false;
    const float nv[3] = {o.nx, o.ny, o.nz};
    for (float x : nv)
        if (std::isnan(x) || std::isinf(x)) return false;
    if (o.nx == 0.0f && o.ny == 0.0f && o.nz == 0.0f) return true;
    return std::fmaf(o.nz, d.z, std::fmaf(o.ny, d.y, o.nx * d.x)) > 0.0f;
}

void run(const std::vector<rt_fan_origin>& os, const std::vector<rt_float4>& ds, const char* what) {
    const int64_t n = (int64_t)os.size();
    const int32_t k = (int32_t)ds.size();
    std::vector<rt_ray> rays((size_t)(n * k));          // exactly n * k: one record more is out of bounds
    std::vector<uint8_t> traced((size_t)(n * k), 9);
    EXPECT(rt_fan_expand(os.data(), n, ds.data(), k, rays.data(), traced.data()) == RT_OK);
    int bad = 0, on = 0;
    for (int64_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < k; ++j) {
            const rt_ray& r = rays[(size_t)(i * k + j)];
            if (std::memcmp(&r, &os[(size_t)i], 16) != 0 || std::memcmp(&r.dx, &ds[(size_t)j], 12) != 0 || r.reserved != 0u) ++bad;
            const uint8_t t = traced[(size_t)(i * k + j)];
            if (t != (want(os[(size_t)i], ds[(size_t)j]) ? 1 : 0)) ++bad;
            on += t;
        }
    EXPECT(bad == 0);
    std::printf("%s: %lld x %d, %d traced\n", what, (long long)n, k, on);
}

}  // namespace

int main() {
    const float tmaxs[] = {0.001f, std::nextafter(0.001f, 1.0f), kInf, kNan, RT_RAY_TMAX_DEFAULT, 0.0f, -1.0f};
    const float normals[][3] = {{0, 0, 0}, {-0.0f, -0.0f, -0.0f}, {kNan, 0, 0}, {0, kInf, 0}, {0, 0, -kInf},
                                {1e30f, 1e30f, 1e30f}, {1e30f, -1e30f, 0}, {-1e30f, -1e30f, -1e30f}, {0, 0, 1},
                                {kSub, 0, 0}, {3, -4, 0.5f}};
    std::vector<rt_fan_origin> os;
    for (const auto& nv : normals)
        for (float t : tmaxs) os.push_back(origin(t, nv[0], nv[1], nv[2]));
    rt_fan_origin b = origin(1.0f, 0, 0, 1);
    b.ox = kNan; os.push_back(b);
    b.ox = 0.0f; b.oy = kInf; os.push_back(b);
    const std::vector<rt_float4> ds = {{0, 0, 0, 1}, {-0.0f, 0, -0.0f, kNan}, {kNan, 1, 0, 0}, {kInf, 0, 0, 0}, {0, -kInf, 1, 0},
                                       {kSub, 0, 0, 0}, {kSub, kSub, kSub, 0}, {1, 0, 0, 0}, {0, -1, 0, 0}, {0, 0, 1, kInf},
                                       {1e30f, 1e30f, 1e30f, 0}, {-1e30f, -1e30f, -1e30f, 0}, {3e38f, 3e38f, 3e38f, 0},
                                       {1, 2, 3, 0}, {-3, 4, -0.5f, 0}};
    run(os, ds, "edge set");
    {   // group and chunk edges, and the largest direction table
        for (int n : {1, 63, 64, 65})
            for (int k : {1, 31, 32, 33, 65}) {
                std::vector<rt_fan_origin> o2;
                std::vector<rt_float4> d2;
                for (int i = 0; i < n; ++i) o2.push_back(origin(10.0f, std::sin((float)i), std::cos((float)i), 0.25f));
                for (int j = 0; j < k; ++j) d2.push_back(rt_float4{std::cos(1.7f * j), std::sin(1.7f * j), 0.1f * j - 1.0f, 0});
                run(o2, d2, "shape");
            }
        std::vector<rt_float4> d3(RT_FAN_MAX_DIRS, rt_float4{0, 0, 1, 0});
        run({origin(1.0f, 0, 0, 1), origin(1.0f, 0, 0, -1)}, d3, "RT_FAN_MAX_DIRS");
    }
    {   // hostile sizes: refused with one-record buffers untouched (a read or write past them is a report)
        std::vector<rt_fan_origin> o1 = {origin(1.0f, 0, 0, 0)};
        std::vector<rt_float4> d1 = {rt_float4{0, 0, 1, 0}};
        std::vector<rt_ray> r1(1);
        std::vector<uint8_t> t1(1, 9);
        std::memset(r1.data(), 0x5A, sizeof(rt_ray));
        const int64_t bad_n[] = {-1, (1ll << 26) + 1, 1ll << 31, 1ll << 40, std::numeric_limits<int64_t>::max(),
                                 std::numeric_limits<int64_t>::min()};
        for (int64_t n : bad_n) EXPECT(rt_fan_expand(o1.data(), n, d1.data(), 1, r1.data(), t1.data()) == RT_ERR_INVALID_ARG);
        const int32_t bad_k[] = {0, -1, RT_FAN_MAX_DIRS + 1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};
        for (int32_t k : bad_k) EXPECT(rt_fan_expand(o1.data(), 1, d1.data(), k, r1.data(), t1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(rt_fan_expand(nullptr, 1, d1.data(), 1, r1.data(), t1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(rt_fan_expand(o1.data(), 1, nullptr, 1, r1.data(), t1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(rt_fan_expand(o1.data(), 1, d1.data(), 1, nullptr, t1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(rt_fan_expand(o1.data(), 1, d1.data(), 1, r1.data(), nullptr) == RT_ERR_INVALID_ARG);
        EXPECT(t1[0] == 9 && ((const unsigned char*)r1.data())[0] == 0x5A && ((const unsigned char*)r1.data())[31] == 0x5A);
        EXPECT(rt_fan_expand(nullptr, 0, nullptr, 0, nullptr, nullptr) == RT_OK);
        EXPECT(rt_fan_expand(nullptr, 0, nullptr, -5, nullptr, nullptr) == RT_OK);   // k is checked with n > 0
        EXPECT(rt_fan_expand(o1.data(), 1, d1.data(), 1, r1.data(), t1.data()) == RT_OK);
        EXPECT(t1[0] == 1 && r1[0].reserved == 0u && r1[0].dz == 1.0f);
        std::printf("arguments: ok\n");
    }
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}

// Microbenchmark: packed f32 against pairs of plain f32 ops on the VALU alone.  The
// traversal's inner step issues 12 packed ops (slab2_pk: 6 v_pk_add_f32, 6 v_pk_mul_f32 in S_ref);
// the CDNA guides report a packed f32 op as costlier than two plain ones beside MFMAs, and nobody had
// measured it without them.  A wave runs a loop of 8 independent v_pk_mul_f32 / v_pk_add_f32 (8
// register pairs), or of the 16 plain v_mul_f32 / v_add_f32 that do the same work on the same 16
// registers, at one wave per SIMD (one block of 4 waves, alone on the chip) and at 8 waves per SIMD
// (two blocks of 16 waves on every CU); prints shader cycles (s_memtime) and ns (s_memrealtime,
// 100 MHz) per packed op, and per PAIR of plain ops, of block 0's first wave; and, from the launch's
// event time, the shader clock those two give and the launch's waves per SIMD, the cycles a SIMD
// spends per op (simd_cycles_per_op: what the wave figure must be set against when the waves of a
// launch may not all be resident together).
#include <hip/hip_runtime.h>
#include <cstdio>

typedef float v2f __attribute__((ext_vector_type(2)));

#define PK8(op) op " %0, %0, %8\n " op " %1, %1, %8\n " op " %2, %2, %8\n " op " %3, %3, %8\n " \
                op " %4, %4, %8\n " op " %5, %5, %8\n " op " %6, %6, %8\n " op " %7, %7, %8\n"
#define PL8(op) op " %0, %8, %0\n " op " %1, %8, %1\n " op " %2, %8, %2\n " op " %3, %8, %3\n " \
                op " %4, %8, %4\n " op " %5, %8, %5\n " op " %6, %8, %6\n " op " %7, %8, %7\n"

// V: 0 = v_pk_mul_f32, 1 = v_pk_add_f32, 2 = v_mul_f32 pairs, 3 = v_add_f32 pairs; the body is
// kUnroll x 8 packed ops (or 16 plain ones)
constexpr int kUnroll = 8;
template <int V>
__global__ void __launch_bounds__(1024) body(int iters, float b, unsigned long long* t) {
    const float x = (float)(threadIdx.x & 7u);
    v2f p0 = {x, x + 1}, p1 = {x + 2, x + 3}, p2 = {x + 4, x + 5}, p3 = {x + 6, x + 7}, p4 = {x + 8, x + 9},
        p5 = {x + 10, x + 11}, p6 = {x + 12, x + 13}, p7 = {x + 14, x + 15};
    float a0 = x, a1 = x + 1, a2 = x + 2, a3 = x + 3, a4 = x + 4, a5 = x + 5, a6 = x + 6, a7 = x + 7, a8 = x + 8,
          a9 = x + 9, a10 = x + 10, a11 = x + 11, a12 = x + 12, a13 = x + 13, a14 = x + 14, a15 = x + 15;
    const v2f bb = {b, b};
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            if (V == 0) asm volatile(PK8("v_pk_mul_f32") : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(bb));
            if (V == 1) asm volatile(PK8("v_pk_add_f32") : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(bb));
            if (V == 2) {   // (an asm statement takes at most 30 operands: two of 8 ops)
                asm volatile(PL8("v_mul_f32_e32") : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));
                asm volatile(PL8("v_mul_f32_e32") : "+v"(a8), "+v"(a9), "+v"(a10), "+v"(a11), "+v"(a12), "+v"(a13), "+v"(a14), "+v"(a15) : "v"(b));
            }
            if (V == 3) {   // (an asm statement takes at most 30 operands: two of 8 ops)
                asm volatile(PL8("v_add_f32_e32") : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));
                asm volatile(PL8("v_add_f32_e32") : "+v"(a8), "+v"(a9), "+v"(a10), "+v"(a11), "+v"(a12), "+v"(a13), "+v"(a14), "+v"(a15) : "v"(b));
            }
        }
    }
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime(), c1 = __builtin_amdgcn_s_memtime();
    const float s = p0.x + p0.y + p1.x + p1.y + p2.x + p2.y + p3.x + p3.y + p4.x + p4.y + p5.x + p5.y + p6.x + p6.y + p7.x +
                    p7.y + a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + a8 + a9 + a10 + a11 + a12 + a13 + a14 + a15;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        t[0] = r1 - r0;
        t[1] = c1 - c0;
    }
    if (s == 1234.5f) t[2] = 1;
}

template <int V>
void run(const char* name, int per_simd, int cus, unsigned long long* d) {
    const int iters = 4000;
    const long ops = (long)iters * kUnroll * 8;   // packed ops, or pairs of plain ops
    const dim3 grid(per_simd == 1 ? 1 : 2 * cus), block(per_simd == 1 ? 256 : 1024);
    unsigned long long h[3];
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    float ms = 0.0f;
    for (int rep = 0; rep < 3; ++rep) {
        (void)hipEventRecord(e0, 0);
        hipLaunchKernelGGL((body<V>), grid, block, 0, 0, iters, V % 2 ? 1e-7f : 1.0f, d);
        (void)hipEventRecord(e1, 0);
        if (hipDeviceSynchronize() != hipSuccess) {
            printf("{\"variant\": \"%s\", \"error\": \"launch failed\"}\n", name);
            return;
        }
        (void)hipEventElapsedTime(&ms, e0, e1);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    const double ghz = (double)h[1] / (h[0] * 10.0);   // shader cycles per ns, from the timed wave's two clocks
    printf("{\"variant\": \"%s\", \"waves_per_simd\": %d, \"ns_per_op\": %.3f, \"cycles_per_op\": %.3f, "
           "\"launch_ms\": %.4f, \"simd_cycles_per_op\": %.3f}\n", name, per_simd, h[0] * 10.0 / ops, (double)h[1] / ops, ms,
           ms * 1e6 * ghz / ((double)ops * per_simd));
}

int main() {
    unsigned long long* d;
    if (hipMalloc(&d, 8 * sizeof(unsigned long long)) != hipSuccess) return 1;
    (void)hipMemset(d, 0, 8 * sizeof(unsigned long long));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) return 1;
    for (int per_simd : {1, 8}) {
        run<0>("v_pk_mul_f32", per_simd, cus, d);
        run<2>("v_mul_f32 x2", per_simd, cus, d);
        run<1>("v_pk_add_f32", per_simd, cus, d);
        run<3>("v_add_f32 x2", per_simd, cus, d);
    }
    (void)hipFree(d);
    return 0;
}

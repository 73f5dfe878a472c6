// Micro check + price list for the traversal prologue and the leaf decode.
//
// 1. Does a packed f32 op read BOTH halves of a scalar register pair on gfx950?  The wave-uniform
//    prologue holds an inner record in SGPRs (s_load_dwordx8); its slab test wants
//    v_pk_add_f32 v[a:b], s[m:n], v[c:d] with the box pair as the scalar src0.  The assembler takes
//    it; whether the hardware delivers s[n] to the high lane, or replicates s[m], is what one wave
//    checks here, in both op_sel forms the slab test uses (the ray's value in the low or the high
//    half of its pair), against the same op fed from a VGPR copy.
// 2. What the decode's integer ops cost: v_mad_u64_u32 against v_mad_u32_u24 and v_lshl_add_u32,
//    8 independent chains at one wave per SIMD and at 8, shader cycles per op of block 0's wave 0.
//
// Prints one JSON line per result.  Exit status 1 when the scalar pair is NOT read as a pair.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

typedef float v2f __attribute__((ext_vector_type(2)));

// out[lane] = {S0 form from SGPR pair, S0 from VGPR pair, S1 from SGPR pair, S1 from VGPR pair}
__global__ void __launch_bounds__(64) pair_check(float lo, float hi, float4* out_lo, float4* out_hi) {
    const float l = (float)threadIdx.x;
    const v2f box = {lo, hi};             // kernel arguments: uniform, an SGPR pair under "s"
    const v2f O = {l * 0.25f, l + 1000.0f};
    v2f s0, v0, s1, v1, bv = box;
    asm volatile("" : "+v"(bv));          // a VGPR copy of the pair
    asm volatile("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(s0) : "s"(box), "v"(O));
    asm volatile("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(v0) : "v"(bv), "v"(O));
    asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(s1) : "s"(box), "v"(O));
    asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(v1) : "v"(bv), "v"(O));
    out_lo[threadIdx.x] = make_float4(s0.x, v0.x, s1.x, v1.x);
    out_hi[threadIdx.x] = make_float4(s0.y, v0.y, s1.y, v1.y);
}

#define OP8(t) t("%0") t("%1") t("%2") t("%3") t("%4") t("%5") t("%6") t("%7")
#define MAD64(r) "v_mad_u64_u32 " r ", vcc, %8, %9, " r "\n "
#define MAD24(r) "v_mad_u32_u24 " r ", %8, %9, " r "\n "
#define LSHLADD(r) "v_lshl_add_u32 " r ", %8, 4, " r "\n "

// V: 0 = v_mad_u64_u32, 1 = v_mad_u32_u24, 2 = v_lshl_add_u32
constexpr int kUnroll = 8;
template <int V>
__global__ void __launch_bounds__(1024) int_ops(int iters, uint32_t m, unsigned long long* t) {
    const uint32_t x = threadIdx.x & 7u;
    unsigned long long w0 = x, w1 = x + 1, w2 = x + 2, w3 = x + 3, w4 = x + 4, w5 = x + 5, w6 = x + 6, w7 = x + 7;
    uint32_t a0 = x, a1 = x + 1, a2 = x + 2, a3 = x + 3, a4 = x + 4, a5 = x + 5, a6 = x + 6, a7 = x + 7;
    const uint32_t k = x + 3;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (V == 0) asm volatile(OP8(MAD64) : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3), "+v"(w4), "+v"(w5), "+v"(w6), "+v"(w7) : "v"(k), "v"(m) : "vcc");
            if (V == 1) asm volatile(OP8(MAD24) : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(k), "v"(m));
            if (V == 2) asm volatile(OP8(LSHLADD) : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(k), "v"(m));
        }
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    const unsigned long long s = w0 + w1 + w2 + w3 + w4 + w5 + w6 + w7 + a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
    if (blockIdx.x == 0 && threadIdx.x == 0) t[0] = c1 - c0;
    if (s == 0x123456789abcull) t[1] = 1;
}

template <int V>
static void price(const char* name, int per_simd, int cus, unsigned long long* d) {
    const int iters = 2000;
    const long ops = (long)iters * kUnroll * 8;
    const dim3 grid(per_simd == 1 ? 1 : 2 * cus), block(per_simd == 1 ? 256 : 1024);
    for (int rep = 0; rep < 2; ++rep) {
        hipLaunchKernelGGL((int_ops<V>), grid, block, 0, 0, iters, 48u, d);
        if (hipDeviceSynchronize() != hipSuccess) {
            printf("{\"op\": \"%s\", \"error\": \"launch failed\"}\n", name);
            return;
        }
    }
    unsigned long long h = 0;
    (void)hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
    printf("{\"op\": \"%s\", \"waves_per_simd\": %d, \"cycles_per_op\": %.3f}\n", name, per_simd, (double)h / ops);
}

int main() {
    float4 *d_lo, *d_hi;
    unsigned long long* d;
    if (hipMalloc(&d_lo, 64 * sizeof(float4)) != hipSuccess || hipMalloc(&d_hi, 64 * sizeof(float4)) != hipSuccess ||
        hipMalloc(&d, 8 * sizeof(unsigned long long)) != hipSuccess)
        return 2;
    (void)hipMemset(d, 0, 8 * sizeof(unsigned long long));
    const float lo = 3.0f, hi = 500.0f;
    hipLaunchKernelGGL(pair_check, dim3(1), dim3(64), 0, 0, lo, hi, d_lo, d_hi);
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    float4 h_lo[64], h_hi[64];
    (void)hipMemcpy(h_lo, d_lo, sizeof(h_lo), hipMemcpyDeviceToHost);
    (void)hipMemcpy(h_hi, d_hi, sizeof(h_hi), hipMemcpyDeviceToHost);
    int pair_ok = 1, same_as_vgpr = 1, replicated = 1;
    for (int l = 0; l < 64; ++l) {
        const float o0 = l * 0.25f, o1 = l + 1000.0f;
        // expected: S0 = {lo - O.lo, hi - O.lo}; S1 = {lo - O.hi, hi - O.hi}
        if (h_lo[l].x != lo - o0 || h_hi[l].x != hi - o0 || h_lo[l].z != lo - o1 || h_hi[l].z != hi - o1) pair_ok = 0;
        if (memcmp(&h_lo[l].x, &h_lo[l].y, 4) || memcmp(&h_hi[l].x, &h_hi[l].y, 4) || memcmp(&h_lo[l].z, &h_lo[l].w, 4) ||
            memcmp(&h_hi[l].z, &h_hi[l].w, 4))
            same_as_vgpr = 0;
        if (h_hi[l].x != lo - o0 || h_hi[l].z != lo - o1) replicated = 0;
    }
    printf("{\"check\": \"v_pk_add_f32 scalar pair src0\", \"reads_both_halves\": %d, \"equals_vgpr_form\": %d, "
           "\"replicates_low_half\": %d, \"lane1\": [%g, %g, %g, %g]}\n", pair_ok, same_as_vgpr, replicated,
           h_lo[1].x, h_hi[1].x, h_lo[1].z, h_hi[1].z);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) return 2;
    for (int per_simd : {1, 8}) {
        price<0>("v_mad_u64_u32", per_simd, cus, d);
        price<1>("v_mad_u32_u24", per_simd, cus, d);
        price<2>("v_lshl_add_u32", per_simd, cus, d);
    }
    (void)hipFree(d_lo);
    (void)hipFree(d_hi);
    (void)hipFree(d);
    return pair_ok && same_as_vgpr ? 0 : 1;
}

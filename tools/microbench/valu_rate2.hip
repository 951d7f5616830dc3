// Issue-rate microbenchmark, round 2: is ANY VALU op class issued faster than one wave64
// instruction per 4 cycles per SIMD on gfx950?  (MI355X_MICROARCH.md states SIMD-32 units and
// 2 cycles for v_fma_f32 at more than one wave per SIMD; round 1 measured 4.4 for the packed-16
// and plain int32 ops only.)  Every op is written as inline asm so that the instruction named is
// the instruction timed; 16 independent chains per wave.  Rates are reported against the wall
// clock (nominal 2.4 GHz) AND in s_memtime ticks (= shader cycles per the guide).
// Build: hipcc --offload-arch=gfx950 -O3 tools/microbench/valu_rate2.hip -o /tmp/valu_rate2
// Run:   valu_rate2 (first batch) | valu_rate2 second | valu_rate2 handover [CASE] (the lane hand-over's instructions and sequences;
//        with CASE one case alone, so that a job can give every case a time limit of its own)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>

#define ITER 4096
#define UNROLL 16

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

enum Op {
    PK_MAX_I16, ADD_F32, FMA_F32, MAX_F32, MAX3_F32, MAX3_I32, PK_FMA_F32, PK_ADD_F32, ADD3_U32, MAX_I32,
    ADD_U32, PK_MAXIMUM3_F16, MAXIMUM3_F32, MAX3_I16, MED3_I32, MOV_DPP, AND_B32, MAD_U32_U24, PK_MAD_U16,
    PERM_B32, ADD_F32_CLAMP, PK_ADD_F16, MIN3_U32, SUB_SAT_U32, ADD_I32_SAT, MAX3_U16, CNDMASK, PK_MUL_F32, PK_MOV_B32,
    DOT2_I32_I16, SAD_U16, LSHL_ADD, BFE, MAX_U16,
    // second batch: the bit operations and 16-bit forms the tagged alignment kernels are made of, and a 1:1 mix
    AND_OR_B32, BFI_B32, LSHL_OR_B32, OR3_B32, XOR_B32, OR_B32, LSHLREV_B32, PK_ADD_I16, PK_ADD_I16_CLAMP,
    PK_SUB_U16_CLAMP, PK_LSHLREV_B16, SUB_U32, MAX_I16, ADD_U16, BITOP3_B32, MIX_PKMAX_AND, MIX_PKMAX_AND_2TO1, ADD_U32_SDWA, ASHRREV_I32, BFE_I32,
    // third batch: what the lane hand-over of the tilted sweep's step is made of (dp_kernels.hip.h: group_prev_or / row_prev_or), alone
    // and as the two hand-overs of a step between 130 packed maxima -- the 8 x 19 tile's ratio
    CNDMASK_E64_SGPR, OR_B32_DPP_SHR2, MOV_DPP_SHR2, MOV_DPP_WAVE_SHR1, HANDOVER_OLD_130, HANDOVER_NEW_130, NO_HANDOVER_130
};

// wave instructions per pass of the timed loop's body: UNROLL of the op itself, or one block of a sequence case
constexpr int kSeqOthers = 130;
constexpr bool is_sequence(int op) { return op == HANDOVER_OLD_130 || op == HANDOVER_NEW_130 || op == NO_HANDOVER_130; }
constexpr int instr_per_pass(int op) {
    return op == HANDOVER_OLD_130 ? kSeqOthers + 7 : op == HANDOVER_NEW_130 ? kSeqOthers + 2 : op == NO_HANDOVER_130 ? kSeqOthers : UNROLL;
}

template <int OP>
__global__ void __launch_bounds__(512) rate(unsigned *out, unsigned seed, long long *cycles) {
    unsigned r[UNROLL];
    u32x2 w[UNROLL];
#pragma unroll
    for (int i = 0; i < UNROLL; ++i) {
        r[i] = seed * (i + 1) + threadIdx.x;
        w[i] = u32x2{r[i], r[i] ^ 0x5555u};
    }
    unsigned g = seed | 0x00030003u, h = seed * 7u;
    u32x2 gw = u32x2{g, h};
    asm volatile("" : "+v"(g), "+v"(h), "+v"(gw));
    unsigned long long lm = 0xFEFEFEFEFEFEFEFEull;            // "not the first lane of a group of 8" in an SGPR pair
    asm volatile("" : "+s"(lm));
    long long t0 = clock64();
    for (int it = 0; it < ITER; ++it) {
        if (is_sequence(OP)) {
            // the two hand-overs of a step first, as the step has them, then the others; sources and destinations are chains whose
            // last write lies eight instructions back (a DPP read needs two wait states after the write)
            if (OP == HANDOVER_OLD_130) {
                unsigned t, u;
                asm volatile("v_mov_b32 %0, 0" : "=v"(t));
                asm volatile("v_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(t) : "v"(r[8]));
                asm volatile("v_cndmask_b32_e64 %0, %0, 0, %1" : "+v"(t) : "s"(lm));
                asm volatile("v_or_b32 %0, %1, %2" : "=v"(r[9]) : "v"(t), "v"(g));
                asm volatile("v_mov_b32 %0, 0" : "=v"(u));
                asm volatile("v_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(u) : "v"(r[10]));
                asm volatile("v_cndmask_b32_e64 %0, %1, 0, %2" : "=v"(r[11]) : "v"(u), "s"(lm));
            }
            if (OP == HANDOVER_NEW_130) {
                asm volatile("v_or_b32_dpp %0, %1, %2 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r[9]) : "v"(r[8]), "v"(g));
                asm volatile("v_mov_b32_dpp %0, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r[11]) : "v"(r[10]));
            }
#pragma unroll
            for (int j = 0; j < kSeqOthers; ++j) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(r[j % UNROLL]) : "v"(g), "v"(h));
            continue;
        }
#pragma unroll
        for (int i = 0; i < UNROLL; ++i) {
            if (OP == PK_MAX_I16) asm volatile("v_pk_max_i16 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == ADD_F32) asm volatile("v_add_f32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == FMA_F32) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == MAX_F32) asm volatile("v_max_f32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == MAX3_F32) asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == MAX3_I32) asm volatile("v_max3_i32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == PK_FMA_F32) asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(w[i]) : "v"(gw));
            if (OP == PK_ADD_F32) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(w[i]) : "v"(gw));
            if (OP == PK_MUL_F32) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(w[i]) : "v"(gw));
            if (OP == PK_MOV_B32) asm volatile("v_pk_mov_b32 %0, %0, %1" : "+v"(w[i]) : "v"(gw));
            if (OP == ADD3_U32) asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == MAX_I32) asm volatile("v_max_i32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == ADD_U32) asm volatile("v_add_u32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == PK_MAXIMUM3_F16) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == MAXIMUM3_F32) asm volatile("v_maximum3_f32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == MAX3_I16) asm volatile("v_max3_i16 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == MAX3_U16) asm volatile("v_max3_u16 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == MAX_U16) asm volatile("v_max_u16 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == MED3_I32) asm volatile("v_med3_i32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == MOV_DPP) asm volatile("v_mov_b32_dpp %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(r[i]));
            if (OP == AND_B32) asm volatile("v_and_b32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == MAD_U32_U24) asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == PK_MAD_U16) asm volatile("v_pk_mad_u16 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == PERM_B32) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == ADD_F32_CLAMP) asm volatile("v_add_f32 %0, %0, %1 clamp" : "+v"(r[i]) : "v"(g));
            if (OP == PK_ADD_F16) asm volatile("v_pk_add_f16 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == MIN3_U32) asm volatile("v_min3_u32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == SUB_SAT_U32) asm volatile("v_sub_u32 %0, %0, %1 clamp" : "+v"(r[i]) : "v"(g));
            if (OP == ADD_I32_SAT) asm volatile("v_add_i32 %0, %0, %1 clamp" : "+v"(r[i]) : "v"(g));
            if (OP == CNDMASK) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(r[i]) : "v"(g));
            if (OP == DOT2_I32_I16) asm volatile("v_dot2_i32_i16 %0, %1, %2, %0" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == SAD_U16) asm volatile("v_sad_u16 %0, %1, %2, %0" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == LSHL_ADD) asm volatile("v_lshl_add_u32 %0, %0, 2, %1" : "+v"(r[i]) : "v"(g));
            if (OP == BFE) asm volatile("v_bfe_u32 %0, %0, 3, 9" : "+v"(r[i]));
            if (OP == AND_OR_B32) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == BFI_B32) asm volatile("v_bfi_b32 %0, %1, %0, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == LSHL_OR_B32) asm volatile("v_lshl_or_b32 %0, %0, 4, %1" : "+v"(r[i]) : "v"(g));
            if (OP == OR3_B32) asm volatile("v_or3_b32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == XOR_B32) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == OR_B32) asm volatile("v_or_b32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == LSHLREV_B32) asm volatile("v_lshlrev_b32 %0, 1, %0" : "+v"(r[i]));
            if (OP == PK_ADD_I16) asm volatile("v_pk_add_i16 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == PK_ADD_I16_CLAMP) asm volatile("v_pk_add_i16 %0, %0, %1 clamp" : "+v"(r[i]) : "v"(g));
            if (OP == PK_SUB_U16_CLAMP) asm volatile("v_pk_sub_u16 %0, %0, %1 clamp" : "+v"(r[i]) : "v"(g));
            if (OP == PK_LSHLREV_B16) asm volatile("v_pk_lshlrev_b16 %0, 1, %0" : "+v"(r[i]));
            if (OP == SUB_U32) asm volatile("v_sub_u32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == MAX_I16) asm volatile("v_max_i16 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == ADD_U16) asm volatile("v_add_u16 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            if (OP == BITOP3_B32) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(r[i]) : "v"(g), "v"(h));
            if (OP == ADD_U32_SDWA) asm volatile("v_add_u32_sdwa %0, %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "+v"(r[i]) : "v"(g));
            if (OP == ASHRREV_I32) asm volatile("v_ashrrev_i32 %0, 16, %0" : "+v"(r[i]));
            if (OP == BFE_I32) asm volatile("v_bfe_i32 %0, %0, 0, 16" : "+v"(r[i]));
            if (OP == CNDMASK_E64_SGPR) asm volatile("v_cndmask_b32_e64 %0, %0, 0, %1" : "+v"(r[i]) : "s"(lm));
            if (OP == OR_B32_DPP_SHR2) asm volatile("v_or_b32_dpp %0, %0, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(r[i]) : "v"(g));
            if (OP == MOV_DPP_SHR2) asm volatile("v_mov_b32_dpp %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(r[i]));
            if (OP == MOV_DPP_WAVE_SHR1) asm volatile("v_mov_b32_dpp %0, %0 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(r[i]));
            if (OP == MIX_PKMAX_AND) {          // half of the instructions packed maxima, half plain ANDs
                if (i & 1) asm volatile("v_and_b32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
                else asm volatile("v_pk_max_i16 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            }
            if (OP == MIX_PKMAX_AND_2TO1) {     // two packed per AND, roughly the tagged affine fill's mix
                if (i % 3 == 2) asm volatile("v_and_b32 %0, %0, %1" : "+v"(r[i]) : "v"(g));
                else asm volatile("v_pk_max_i16 %0, %0, %1" : "+v"(r[i]) : "v"(g));
            }
        }
    }
    long long t1 = clock64();
    unsigned acc = 0;
#pragma unroll
    for (int i = 0; i < UNROLL; ++i) acc ^= r[i] ^ w[i].x ^ w[i].y;
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
    if (threadIdx.x % 64 == 0) cycles[blockIdx.x * 8 + threadIdx.x / 64] = t1 - t0;
}

template <int OP>
void run(const char *name) {
    unsigned *out;
    long long *cyc;
    hipMalloc(&out, 256 * 512 * 8 * sizeof(unsigned));
    hipMalloc(&cyc, 8 * 4096 * sizeof(long long));
    for (int waves_per_simd : {1, 2, 4, 8}) {
        const int threads = 64 * 4 * (waves_per_simd > 2 ? 2 : waves_per_simd);   // block = up to 8 waves
        const int blocks_per_cu = waves_per_simd > 2 ? waves_per_simd / 2 : 1;
        const int blocks = 256 * blocks_per_cu;
        hipEvent_t e0, e1;
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        hipMemset(cyc, 0, 8 * 4096 * sizeof(long long));
        rate<OP><<<blocks, threads>>>(out, 12345u, cyc);
        hipDeviceSynchronize();
        hipEventRecord(e0);
        rate<OP><<<blocks, threads>>>(out, 12345u, cyc);
        hipEventRecord(e1);
        hipDeviceSynchronize();
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        const int wpb = threads / 64;
        std::vector<long long> h(blocks * 8);
        hipMemcpy(h.data(), cyc, blocks * 8 * sizeof(long long), hipMemcpyDeviceToHost);
        double avg = 0;
        for (int b = 0; b < blocks; ++b)
            for (int w = 0; w < wpb; ++w) avg += (double)h[b * 8 + w];
        avg /= (double)blocks * wpb;
        const double instr_per_wave = (double)ITER * instr_per_pass(OP);
        const double wave_instr = instr_per_wave * blocks * wpb;
        const double per_simd_per_s = wave_instr / (ms * 1e-3) / 1024.0;
        // ticks per instruction per SIMD: a wave's own ticks / its instructions / waves sharing the SIMD
        printf("%-20s waves/SIMD %d: %7.3f ms  %.2f cyc/instr/SIMD at 2.4 GHz wall | %.2f by s_memtime\n", name,
               waves_per_simd, ms, 2.4e9 / per_simd_per_s, avg / instr_per_wave / waves_per_simd);
        if (is_sequence(OP))           // a sequence case: the block of instr_per_pass instructions is the unit
            printf("%-20s waves/SIMD %d: %.1f ticks per block of %d per SIMD by s_memtime\n", name, waves_per_simd,
                   avg / ITER / waves_per_simd, instr_per_pass(OP));
    }
    hipFree(out);
    hipFree(cyc);
}

int main(int argc, char **argv) {
#define RUN(op) run<op>(#op)
    if (argc > 1 && std::string(argv[1]) == "handover") {       // third batch; a second argument names one case (a run of its own)
        const std::string only = argc > 2 ? argv[2] : "";
#define RUN_IF(op) if (only.empty() || only == #op) run<op>(#op)
        RUN_IF(PK_MAXIMUM3_F16); RUN_IF(CNDMASK_E64_SGPR); RUN_IF(OR_B32_DPP_SHR2); RUN_IF(MOV_DPP_SHR2); RUN_IF(MOV_DPP_WAVE_SHR1); RUN_IF(OR_B32);
        RUN_IF(NO_HANDOVER_130); RUN_IF(HANDOVER_OLD_130); RUN_IF(HANDOVER_NEW_130);
        return 0;
    }
    if (argc > 1) {                                 // second batch only
        RUN(AND_OR_B32); RUN(BFI_B32); RUN(LSHL_OR_B32); RUN(OR3_B32); RUN(XOR_B32); RUN(OR_B32); RUN(LSHLREV_B32);
        RUN(PK_ADD_I16); RUN(PK_ADD_I16_CLAMP); RUN(PK_SUB_U16_CLAMP); RUN(PK_LSHLREV_B16); RUN(SUB_U32); RUN(MAX_I16);
        RUN(ADD_U16); RUN(BITOP3_B32); RUN(MIX_PKMAX_AND); RUN(MIX_PKMAX_AND_2TO1); RUN(ADD_U32_SDWA); RUN(ASHRREV_I32); RUN(BFE_I32);
        return 0;
    }
    RUN(PK_MAX_I16); RUN(MAX_I32); RUN(ADD_U32); RUN(ADD_F32); RUN(FMA_F32); RUN(MAX_F32); RUN(MAX3_F32);
    RUN(MAXIMUM3_F32); RUN(MAX3_I32); RUN(MIN3_U32); RUN(MED3_I32); RUN(ADD3_U32); RUN(ADD_F32_CLAMP);
    RUN(SUB_SAT_U32); RUN(ADD_I32_SAT); RUN(PK_FMA_F32); RUN(PK_ADD_F32); RUN(PK_MUL_F32); RUN(PK_MOV_B32);
    RUN(PK_MAXIMUM3_F16); RUN(PK_ADD_F16); RUN(PK_MAD_U16); RUN(MAX3_I16); RUN(MAX3_U16); RUN(MAX_U16); RUN(MOV_DPP); RUN(AND_B32);
    RUN(MAD_U32_U24); RUN(PERM_B32); RUN(CNDMASK); RUN(DOT2_I32_I16); RUN(SAD_U16); RUN(LSHL_ADD); RUN(BFE);
    return 0;
}

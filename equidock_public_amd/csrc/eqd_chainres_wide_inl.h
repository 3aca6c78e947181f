// k_rowchain_res_fwd_wide: the forward node chain of the 69-wide FIRST layer (node_mlp.0 with 69 outputs + LeakyReLU
// [+ dropout] + LayerNorm over 69 features -> node_mlp.4 with K = 69) at DB5.5 sizes - one 16-row tile per workgroup, no more
// tiles than CUs, fp32 - with every weight chunk of both jobs, the tile's source rows AND the 5-column remainders of the
// 69-wide sources resident in LDS, filled by LDS-DMA (glds16, eqd_common.h) at kernel entry.  It replaces the last forward
// chain that ran on k_rowchain<1, false, 1>'s staged general body (eqd_linear_inl.h, linear_tile) at these sizes.
//
// The list it takes (crw_pack, eqd_node_kernels.hip): job 0 with M = 69 and four sources of K = 69, 64, 69, 69, job 1 with
// M = 64 and one source of K = 69 that is job 0's LDS tile.  Nothing is carried behind job 1.
//
// Layout.  A full chunk is the swizzled image of eqd_chainres_inl.h (cr_at) with 80 rows: rows 0 .. 63 are copied by the
// wave that multiplies them (wave w: rows 16 w .. 16 w + 15), rows 64 .. 79 - output block 4, features 64 .. 68, which wave 0
// multiplies, the ownership of the general body - four rows per wave, rows beyond 68 clamped to row 68 (their products
// belong to features that the epilogue drops).  So every wave issues the same number of copies and one counted wait serves
// all; wave 0 reads rows it did not copy, hence one lds_barrier() per chunk behind the wait.
// A remainder image holds, per row, two 16-byte pieces: columns 64 .. 67 and the four columns that END at column 68 (65 ..
// 68: a piece that started at column 68 would run past the end of a 69-float row).  The k assignment of a 16-deep step is
// k = 4 g + j: lane group 0 takes piece 0, group 1 takes the last float of piece 1 as k = 4, everything else is the zero
// padding the general body stores (crw_rem_frag) - the MFMA operands are the same numbers, zeros included.
// Order per wave: X0 X1 X2 X3 Xr | W0 x5 Wr0 | W1 x5 | W2 x5 Wr2 | W3 x5 Wr3 | Wn2 x4 Wn2r = 33 copies.
// Ordinary loads (epilogue operands, dropout factors) are requested BEFORE the copies and first touched behind the
// vm_wait<0> that follows the last chunk of node_mlp.0 (keep_after_wait).
//
// Arithmetic: per output element the MFMA sequence is the general body's - source by source: the full chunk, then that
// source's 16-deep step; k = 16 (j >> 2) + 4 g + (j & 3) inside a chunk; two accumulator sets; wave w owns blocks w and
// w + 4, so the LayerNorm partial sums combine in the same order - and job 1 is linear_tile_lean's (full chunk, remainder
// step, its epilogue).  Every epilogue expression is copied: the results are bit-identical to k_rowchain's.
#pragma once
#include "eqd_chainres_inl.h"

#define CRW_CHUNK (80 * 64)     /* floats of an 80-row weight chunk image */
#define CRW_REM (128 * 8)       /* floats of a remainder image: 128 rows x 2 pieces x 4 floats (one copy per wave) */
struct alignas(1024) ChainResWideSmem {
    float W[4][CRW_CHUNK];      // node_mlp.0 chunks 0 .. 3 (sources h, aggr_msg, aggr_cross, h0)
    float W1[CR_CHUNK];         // node_mlp.4, columns 0 .. 63
    float Wr[4][CRW_REM];       // columns 64 .. 68 of sources 0, 2, 3 and of node_mlp.4
    float X[4][CR_XTILE];
    float Xr[4][256];           // columns 64 .. 68 of the rows of sources 0, 2, 3 (slot 3: wave 3's copy, never read)
};
struct ChainResWideArg {
    int rows, M;        // M: outputs of job 0 = K of sources 0, 2, 3 and of job 1 (69)
    int act0, ld_mul0, ld_pre, ldy0;
    int act1, w1_rs, ldy1;
    float slope0, ln_eps, alpha0, beta0, slope1, alpha1, beta1;
    CrfSrc s[4];        // node_mlp.0's sources
    const float *bias0, *ln_g, *ln_b, *mul0;
    float *pre_ln, *Y0;
    const float *W1, *bias1;      // node_mlp.4
    float* Y1;
};

// the wave's five copies of a k-contiguous 64-deep chunk of M (<= 80) rows into the swizzled image
__device__ __forceinline__ void crw_copy_chunk(const float* Wg, int w_rs, int M, float* img, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = 16 * wave + 4 * i + (lane >> 4);
        glds16(Wg + (size_t)m * w_rs + 4 * ((lane & 15) ^ (m & 15)), &img[64 * (16 * wave + 4 * i)]);
    }
    const int r = 64 + 4 * wave + (lane >> 4);
    const int m = r < M ? r : M - 1;
    glds16(Wg + (size_t)m * w_rs + 4 * ((lane & 15) ^ (r & 15)), &img[64 * (64 + 4 * wave)]);
}
// the wave's copy of columns 64 .. K - 1 (K = 69) of 32 rows of a matrix of M rows: lane -> row 32 wave + (lane >> 1),
// piece lane & 1
__device__ __forceinline__ void crw_copy_rem(const float* Wg, int w_rs, int M, int K, float* img, int wave, int lane) {
    const int r = 32 * wave + (lane >> 1);
    const int m = r < M ? r : M - 1;
    glds16(Wg + (size_t)m * w_rs + ((lane & 1) ? K - 4 : 64), &img[256 * wave]);
}
// the 16-deep step's fragment of row r: k = 4 g + j, columns 64 + k < 69, zeros beyond
__device__ __forceinline__ f32x4 crw_rem_frag(const float* __restrict__ img, int r, int g) {
    const f32x4 v = *(const f32x4*)&img[8 * r + (g == 1 ? 4 : 0)];
    f32x4 o;
    o[0] = g == 0 ? v[0] : (g == 1 ? v[3] : 0.f);
    o[1] = g == 0 ? v[1] : 0.f;
    o[2] = g == 0 ? v[2] : 0.f;
    o[3] = g == 0 ? v[3] : 0.f;
    return o;
}
// one 64-deep chunk for the wave's output block (and block 4 on the wave that owns it): lin_mma<1, NOWN, 4, false>'s order
// per accumulator
__device__ __forceinline__ void crw_mma(f32x4 (&acc)[2], f32x4 (&acc2)[2], const float* __restrict__ Wi,
                                        const float* __restrict__ Xi, int wave, bool own1, int l15, int g) {
    f32x4 a[4], a4[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = *(const f32x4*)&Wi[cr_at(16 * wave + l15, 4 * q + g)];
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = *(const f32x4*)&Xi[cr_at(l15, 4 * q + g)];
    if (own1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a4[q] = *(const f32x4*)&Wi[cr_at(64 + l15, 4 * q + g)];
    }
#ifndef EQD_HOSTSIM
    __builtin_amdgcn_sched_barrier(0);      // every fragment read is issued before the first MFMA (see lin_mma)
#endif
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[0] = mfma4(a[q][0], b[q][0], acc[0]);
        acc2[0] = mfma4(a[q][1], b[q][1], acc2[0]);
        acc[0] = mfma4(a[q][2], b[q][2], acc[0]);
        acc2[0] = mfma4(a[q][3], b[q][3], acc2[0]);
    }
    if (own1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[1] = mfma4(a4[q][0], b[q][0], acc[1]);
            acc2[1] = mfma4(a4[q][1], b[q][1], acc2[1]);
            acc[1] = mfma4(a4[q][2], b[q][2], acc[1]);
            acc2[1] = mfma4(a4[q][3], b[q][3], acc2[1]);
        }
    }
    keep_after_wait(acc[0]);      // (see cr_mma: both chains are complete here, not behind a later wait)
    keep_after_wait(acc2[0]);
    keep_after_wait(acc[1]);
    keep_after_wait(acc2[1]);
}
// the 16-deep step behind it: lin_mma<1, NOWN, 1, false>'s order per accumulator
__device__ __forceinline__ void crw_mma_rem(f32x4 (&acc)[2], f32x4 (&acc2)[2], const float* __restrict__ Wr, const f32x4 b,
                                            int wave, bool own1, int l15, int g) {
    const f32x4 a = crw_rem_frag(Wr, 16 * wave + l15, g);
    acc[0] = mfma4(a[0], b[0], acc[0]);
    acc2[0] = mfma4(a[1], b[1], acc2[0]);
    acc[0] = mfma4(a[2], b[2], acc[0]);
    acc2[0] = mfma4(a[3], b[3], acc2[0]);
    if (own1) {
        const f32x4 a4 = crw_rem_frag(Wr, 64 + l15, g);
        acc[1] = mfma4(a4[0], b[0], acc[1]);
        acc2[1] = mfma4(a4[1], b[1], acc2[1]);
        acc[1] = mfma4(a4[2], b[2], acc[1]);
        acc2[1] = mfma4(a4[3], b[3], acc2[1]);
    }
}

__global__ __launch_bounds__(EQD_BLOCK, 1) void k_rowchain_res_fwd_wide(ChainResWideArg A) {
    __shared__ ChainResWideSmem S;
    __shared__ __attribute__((aligned(16))) float Lt[16 * LIN_S];      // LayerNorm output: node_mlp.4's source rows
    __shared__ float stat[EQD_WAVES][16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, g = lane >> 4;
    const int row0 = (int)blockIdx.x * 16, rows = A.rows, M = A.M;
    // the tile's columns M .. 79 stay zero: node_mlp.4's 16-deep step reads them (k_rowchain zeroes its tiles the same way)
    for (int i = t; i < 16 * LIN_S; i += EQD_BLOCK) Lt[i] = 0.f;
    // ---- ordinary loads first: the epilogue operands of both jobs (linear_tile's addresses) ----------------------------------
    const int mbn = (M + 15) >> 4;
    const int mbs[2] = {wave, wave + 4};
    const bool own[2] = {wave < mbn, wave + 4 < mbn};
    const int rowi = row0 + l15;
    const bool rv = rowi < rows;
    const int rowe = rv ? rowi : rows - 1;
    f32x4 bias[2], lg[2], lb[2], mulr[2], bias1;
    int nf[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f0 = 16 * mbs[i] + 4 * g;
        nf[i] = own[i] ? M - f0 : 0;      // valid features at f0 (<= 0: none)
        // (branch-free: an absent operand reads valid bytes of ln_g that are dropped below - a load under a branch gets a
        //  wait of its own, a chain of round trips in front of the copies)
        const float* const bp = A.bias0 ? A.bias0 : A.ln_g;
        const float* const mp = A.mul0 ? A.mul0 + (size_t)rowe * A.ld_mul0 : A.ln_g;
        bias[i] = ld4u_raw(bp + f0, nf[i], bp);
        lg[i] = ld4u_raw(A.ln_g + f0, nf[i], A.ln_g);
        lb[i] = ld4u_raw(A.ln_b + f0, nf[i], A.ln_b);
        mulr[i] = ld4u_raw(mp + f0, nf[i], mp);
    }
    bias1 = *(const EQD_GAS f4v*)((A.bias1 ? A.bias1 : A.ln_g) + 16 * wave + 4 * g);
    // ---- the copies, in the order they are consumed ------------------------------------------------------------------
    {
        const int r = 4 * wave + (lane >> 4);      // row of the tile this lane copies a piece of
        const int c = 4 * ((lane & 15) ^ (r & 15));
        int row = row0 + r;
        row = row < rows ? row : rows - 1;
#pragma unroll
        for (int s = 0; s < 4; ++s) glds16(A.s[s].X + (size_t)row * A.s[s].ldx + c, &S.X[s][256 * wave]);
        // columns 64 .. M - 1 of the rows of sources 0, 2, 3: wave 0, 1, 2 (wave 3 repeats source 3, so that every wave
        // counts the same copies); lane -> row (lane >> 1) & 15, piece lane & 1
        const float* const xp = wave == 0 ? A.s[0].X : (wave == 1 ? A.s[2].X : A.s[3].X);
        const int xl = wave == 0 ? A.s[0].ldx : (wave == 1 ? A.s[2].ldx : A.s[3].ldx);
        int rr = row0 + ((lane >> 1) & 15);
        rr = rr < rows ? rr : rows - 1;
        glds16(xp + (size_t)rr * xl + ((lane & 1) ? M - 4 : 64), S.Xr[wave]);
    }
    crw_copy_chunk(A.s[0].W, A.s[0].w_rs, M, S.W[0], wave, lane);
    crw_copy_rem(A.s[0].W, A.s[0].w_rs, M, M, S.Wr[0], wave, lane);
    crw_copy_chunk(A.s[1].W, A.s[1].w_rs, M, S.W[1], wave, lane);
    crw_copy_chunk(A.s[2].W, A.s[2].w_rs, M, S.W[2], wave, lane);
    crw_copy_rem(A.s[2].W, A.s[2].w_rs, M, M, S.Wr[1], wave, lane);
    crw_copy_chunk(A.s[3].W, A.s[3].w_rs, M, S.W[3], wave, lane);
    crw_copy_rem(A.s[3].W, A.s[3].w_rs, M, M, S.Wr[2], wave, lane);
    cr_copy_chunk(A.W1, A.w1_rs, S.W1, wave, lane);
    crw_copy_rem(A.W1, A.w1_rs, 64, M, S.Wr[3], wave, lane);
    // ---- node_mlp.0: source by source, the full chunk and then its 16-deep step (33 copies: the counts are what was issued
    //      BEHIND the ones a step reads) -----------------------------------------------------------------------------------
    f32x4 acc[2] = {f4zero(), f4zero()}, acc2[2] = {f4zero(), f4zero()};
    const bool own1 = own[1];
    vm_wait<22>();
    lds_barrier();      // the row tiles and their remainders, source 0's chunk and remainder (and Lt's zeros)
    crw_mma(acc, acc2, S.W[0], S.X[0], wave, own1, l15, g);
    crw_mma_rem(acc, acc2, S.Wr[0], crw_rem_frag(S.Xr[0], l15, g), wave, own1, l15, g);
    vm_wait<17>();
    lds_barrier();
    crw_mma(acc, acc2, S.W[1], S.X[1], wave, own1, l15, g);
    vm_wait<11>();
    lds_barrier();
    crw_mma(acc, acc2, S.W[2], S.X[2], wave, own1, l15, g);
    crw_mma_rem(acc, acc2, S.Wr[1], crw_rem_frag(S.Xr[1], l15, g), wave, own1, l15, g);
    vm_wait<5>();
    lds_barrier();
    crw_mma(acc, acc2, S.W[3], S.X[3], wave, own1, l15, g);
    crw_mma_rem(acc, acc2, S.Wr[2], crw_rem_frag(S.Xr[2], l15, g), wave, own1, l15, g);
    vm_wait<0>();       // node_mlp.4's rows too: nothing is in flight here, the ordinary loads are first touched behind it
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        keep_after_wait(bias[i]); keep_after_wait(lg[i]); keep_after_wait(lb[i]); keep_after_wait(mulr[i]);
    }
    keep_after_wait(bias1);
    if (!A.bias0) bias[0] = bias[1] = f4zero();
    if (!A.bias1) bias1 = f4zero();
    // ---- epilogue of node_mlp.0 (linear_tile's, M not a multiple of 4, expression for expression) -------------------------
    {
        const float slope = A.slope0;
        float4 bs[2], lgv[2], lbv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            bs[i] = ld4u_fix(bias[i], nf[i]);
            lgv[i] = ld4u_fix(lg[i], nf[i]);
            lbv[i] = ld4u_fix(lb[i], nf[i]);
        }
        float v[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float bb[4] = {bs[i].x, bs[i].y, bs[i].z, bs[i].w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float y = (acc[i][r] + acc2[i][r]) + bb[r];
                if (A.act0) y = lrelu(y, slope);
                v[i][r] = r < nf[i] ? y : 0.f;
            }
        }
        if (A.mul0) {      // dropout factors (training mode only)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 mm = ld4u_fix(mulr[i], nf[i]);
                v[i][0] *= mm.x; v[i][1] *= mm.y; v[i][2] *= mm.z; v[i][3] *= mm.w;
            }
        }
        const float invM = 1.f / (float)M;
        float s1 = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) s1 += v[i][r];
        s1 = group_sum(s1);
        if (g == 0) stat[wave][l15] = s1;
        __syncthreads();
        const float mean = (stat[0][l15] + stat[1][l15] + stat[2][l15] + stat[3][l15]) * invM;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dlt = r < nf[i] ? v[i][r] - mean : 0.f;
                q += dlt * dlt;
            }
        q = group_sum(q);
        __syncthreads();
        if (g == 0) stat[wave][l15] = q;
        __syncthreads();
        const float rstd = 1.f / sqrtf((stat[0][l15] + stat[1][l15] + stat[2][l15] + stat[3][l15]) * invM + A.ln_eps);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float gg[4] = {lgv[i].x, lgv[i].y, lgv[i].z, lgv[i].w};
            const float be[4] = {lbv[i].x, lbv[i].y, lbv[i].z, lbv[i].w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < nf[i]) {
                    const int f = 16 * mbs[i] + 4 * g + r;
                    if (A.pre_ln && rv) ((EQD_GAS float*)A.pre_ln)[(size_t)rowi * A.ld_pre + f] = v[i][r];
                    v[i][r] = (v[i][r] - mean) * rstd * gg[r] + be[r];
                }
        }
        const float alpha = A.alpha0, beta = A.beta0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f0 = 16 * mbs[i] + 4 * g;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float y = alpha * v[i][r] + beta * 0.f;      // (no residual on this job: eligibility)
                if (r < nf[i]) {
                    if (A.Y0 && rv) ((EQD_GAS float*)A.Y0)[(size_t)rowi * A.ldy0 + f0 + r] = y;
                    Lt[l15 * LIN_S + f0 + r] = y;
                }
            }
        }
    }
    __syncthreads();
    // ---- node_mlp.4 on the tile in LDS (linear_tile_lean: the full chunk, the 16-deep step, its epilogue) -----------------
    {
        f32x4 c = f4zero(), c2 = f4zero();
        cr_mma<true>(c, c2, S.W1, Lt, wave, l15, g);
        const f32x4 a = crw_rem_frag(S.Wr[3], 16 * wave + l15, g);
        const f32x4 b = *(const f32x4*)&Lt[l15 * LIN_S + 64 + 4 * g];
        c = mfma4(a[0], b[0], c);
        c2 = mfma4(a[1], b[1], c2);
        c = mfma4(a[2], b[2], c);
        c2 = mfma4(a[3], b[3], c2);
        const float slope = A.slope1;
        const int f0 = 16 * wave + 4 * g;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float y = (c[r] + c2[r]) + bias1[r];
            if (A.act1) y = lrelu(y, slope);
            v[r] = y;
        }
        const float alpha = A.alpha1, beta = A.beta1;
        f32x4 yv;
#pragma unroll
        for (int r = 0; r < 4; ++r) yv[r] = alpha * v[r] + beta * 0.f;      // (no residual: 69 -> 64 has no skip)
        if (A.Y1 && rv) *(EQD_GAS f4v*)&A.Y1[(size_t)rowi * A.ldy1 + f0] = yv;
    }
}

// k_rowchain_res_bwd_wide: the backward node chain of the 69-wide FIRST layer of a model with >= 2 layers and cross messages,
// at DB5.5 sizes - one 16-row tile per workgroup, no more tiles than CUs, fp32 - with every operand resident in LDS, filled by
// LDS-DMA (glds16, eqd_common.h).  It replaces the last node-level chain that ran on k_rowchain<1, false, 1>'s staged general
// body.  The six-job list (node_bwd_chain, eqd_driver.hip; matched by crbw_pack, eqd_node_kernels.hip):
//   1  dh of layer 1: M = 64, six transposed 64-deep sources, residual (1 - s) dH(2) -> dH(1), LDS tile 2.  This IS the DH
//      part of k_rowchain_res_bwd<true> (eqd_chainres_bwd_inl.h): its copies, slabs, crb_mma and epilogue.
//   2  da1n = alpha dH(1) Wn2: M = 69, K = 64 -> tile 0 (not stored).  M != 64: linear_tile's GENERAL path, wave w owns output
//      blocks w and w + 4; block 4 (features 64 .. 68) is wave 0's.
//   3  LeakyReLU / LayerNorm backward over 69 features: chain_lnbwd<1>'s arithmetic (a wave takes four rows, a lane holds
//      features lane and lane + 64, wave_sum reductions) -> dz, tile 1, the workgroup's 256-float ln_part row.
//   4  dz Wn1[:, 69 .. 132]  -> d aggr_msg:   M = 64, K = 69: linear_tile_lean, full chunk + 16-deep remainder step.
//   5  dz Wn1[:, 133 .. 201] -> d aggr_cross: M = 69, K = 69, pad_to 80: general path, columns 69 .. 79 written as zeros.
//   6  dz Wn1[:, 202 .. 265] -> dh0acc (+=):  M = 64 of the 69 columns, ldy = 69: lean path with residual R == Y.
// Every job has ONE source, so "the full chunk, then its 16-deep step" is the order of both paths.
//
// Layout.  The 64 x 64 part of every transposed chunk is the per-wave slab of crb_copy_chunk (private to the wave that
// multiplies it).  What is new here is shared between the waves and consumed only behind the vm_wait<0> + barrier:
//   B4[0], B4[1]  output block 4 (m = 64 .. 68) of Wn2 and of job 5's block, k = 0 .. 63: per row k two 16-byte pieces,
//                 m = 64 .. 67 at 8 k and m = 65 .. 68 at 8 k + 4 (a piece that started at m = 68 would run past the end of
//                 the last row of the matrix; the general body's ld4u_raw shifts the same way).  Waves 0, 1 copy Wn2's two
//                 halves (32 rows x 2 pieces each), waves 2, 3 job 5's.
//   Kr            the rows k = 64 .. 68 of all three Wn1 blocks: 3 x 5 rows x 64 floats (m = 0 .. 63) = 240 lanes, float
//                 320 j + 64 r + m; behind them the same five rows of job 5's block 4, two pieces per row, at 960 + 8 r;
//                 the last six lanes repeat lane 249's source (read and never used).  One copy per wave.
// A 16-deep step's fragment is k = 4 g + j (+ 64), zeros beyond k = 68: the numbers lin_store_s stores, zeros included; the
// tile's columns 69 .. 79 are the zeros the kernel starts with, as in k_rowchain.  Block 4's rows m >= 69 are zeros too.
//
// Copy order per wave and the wait of every consumer (N of vm_wait<N> = copies issued later that may stay in flight):
//   X0 .. X5 R | D0 x4 | D1 x4 | D2 x4 | D3 x4 | D4 x4 | D5 x4 | B4 | Kr            33 copies at entry
//         row tiles published      vm_wait<26>  + barrier
//         dh chunk 0               vm_wait<22>  (D1 .. D5, B4, Kr)                      then Wn2 x4  -> slot 0
//         dh chunk 1               vm_wait<22>  (D2 .. D5, B4, Kr, Wn2)                 then Wn1a x4 -> slot 1
//         dh chunk 2               vm_wait<22>  (D3 .. D5, B4, Kr, Wn2, Wn1a)           then Wn1b x4 -> slot 2
//         dh chunk 3               vm_wait<22>  (D4, D5, B4, Kr, Wn2, Wn1a, Wn1b)       then Wn1c x4 -> slot 3
//         dh chunk 4               vm_wait<22>  (D5, B4, Kr, Wn2, Wn1a, Wn1b, Wn1c)
//         dh chunk 5               vm_wait<18>  (B4, Kr, Wn2, Wn1a, Wn1b, Wn1c)                              49 copies in all
//         dh epilogue (residual from LDS, store of dH(1), tile 2), then vm_wait<0> + barrier
// The ordinary loads - 19 per lane, requested BEFORE the first copy, branch-free: ln_g (2), y_act (8), the dropout factors
// (8; absent: bytes of ln_g that are dropped), the dh0acc accumulator rows (1) - are first touched behind that vm_wait<0>
// (keep_after_wait).  At most 19 + 33 = 52 vector-memory operations are outstanding (vmcnt counts to 63).
//
// Arithmetic: per output element the MFMA sequence of the path the job takes in k_rowchain (chunk, then the zero-padded
// 16-deep step; k = 16 q + 4 g + j inside a chunk; two accumulator sets; (acc + acc2) + 0, alpha v + beta R) and
// chain_lnbwd<1>'s LayerNorm backward in its reduction order.  Bit-identical to k_rowchain<1, false, 1>.
#pragma once
#include "eqd_chainres_bwd_inl.h"

struct ChainResBwdWideArg {
    ChainResBwdArg c;   // the jobs as the 64-wide body names them: dh, a = Wn2, the LayerNorm backward, x / xo = the Wn1 blocks
    int M, pad_to;      // features of the layer (69); width d aggr_cross is zero-padded to (80)
};
struct alignas(1024) ChainResBwdWideSmem {
    float W[6][EQD_WAVES][CRB_SLAB];
    float X[7][CR_XTILE];
    float B4[2][512];
    float Kr[1024];
};

// block 4's fragment of row k of a B4-style image (8 floats per row): W(m = 64 + l15, k), zero for m >= 69
__device__ __forceinline__ float crbw_b4(const float* __restrict__ img, int k, int l15) {
    const float v = img[8 * k + (l15 < 4 ? l15 : 7)];
    return l15 < 5 ? v : 0.f;
}
// one 64-deep transposed chunk for the wave's output block (and block 4 on the wave that owns it): per accumulator the
// instruction order of lin_mma<1, NOWN, 4, true>
__device__ __forceinline__ void crbw_mma(f32x4 (&acc)[2], f32x4 (&acc2)[2], const float* __restrict__ slab,
                                         const float* __restrict__ b4, const f32x4 (&b)[4], bool own1, int lane, int l15, int g) {
    f32x4 a[4], a4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[q][j] = slab[256 * q + 64 * j + lane];
    if (own1) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) a4[q][j] = crbw_b4(b4, 16 * q + 4 * g + j, l15);
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
}
// the 16-deep step behind it (k = 64 + 4 g + j, zeros beyond k = 68): lin_mma<1, NOWN, 1, false>'s order per accumulator.
// kr: the job's 5 x 64 rows in Kr; kr4: block 4's five rows (two pieces per row), read when own1
__device__ __forceinline__ void crbw_mma_rem(f32x4 (&acc)[2], f32x4 (&acc2)[2], const float* __restrict__ kr,
                                             const float* __restrict__ kr4, const f32x4 b, bool own1, int wave, int l15, int g) {
    f32x4 a, a4 = f4zero();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * g + j, kc = k < 5 ? k : 4;
        const float v = kr[64 * kc + 16 * wave + l15];
        a[j] = k < 5 ? v : 0.f;
    }
    acc[0] = mfma4(a[0], b[0], acc[0]);
    acc2[0] = mfma4(a[1], b[1], acc2[0]);
    acc[0] = mfma4(a[2], b[2], acc[0]);
    acc2[0] = mfma4(a[3], b[3], acc2[0]);
    if (own1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * g + j, kc = k < 5 ? k : 4;
            const float v = crbw_b4(kr4, kc, l15);
            a4[j] = k < 5 ? v : 0.f;
        }
        acc[1] = mfma4(a4[0], b[0], acc[1]);
        acc2[1] = mfma4(a4[1], b[1], acc2[1]);
        acc[1] = mfma4(a4[2], b[2], acc[1]);
        acc2[1] = mfma4(a4[3], b[3], acc2[1]);
    }
}

// chain_lnbwd<1> (eqd_node_kernels.hip) on operands that were requested at kernel entry: tile 0 -> dz, tile 1, the ln_part
// row.  g0r / g1r: ln_g at features lane / lane + 64 (the latter at a clamped index); y0s / y1s, m0s / m1s: y_act and the
// dropout factors of rows 4 wave + rr at the same features.  Expression for expression, reduction for reduction.
__device__ __forceinline__ void crbw_lnbwd(const ChainResBwdArg& A, const int d, float (*Lb)[LIN_LOCALS][16 * LIN_S],
                                           float (*red)[256], int row0, float g0r, float g1r, const float (&y0s)[4],
                                           const float (&y1s)[4], const float (&m0s)[4], const float (&m1s)[4]) {
    EQD_GAS float* const jY = (EQD_GAS float*)A.dz;
    EQD_GAS float* const jaux = (EQD_GAS float*)A.aux;
    const int rows = A.rows, ldy = A.ld_dz;
    const float slope = A.slope, ln_eps = A.ln_eps;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int f0 = lane, f1 = lane + 64;
    const bool v0 = f0 < d, v1 = f1 < d;
    const float g0 = v0 ? g0r : 0.f, g1 = v1 ? g1r : 0.f;
    const float invd = 1.f / (float)d;
    float dg0 = 0.f, dg1 = 0.f, db0 = 0.f, db1 = 0.f;
    const float* __restrict__ din = Lb[0][0];
    float* __restrict__ dout = Lb[0][1];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int lr = 4 * wave + rr;
        const int row = row0 + lr;
        const bool rv = row < rows;
        const float y0 = (rv && v0) ? y0s[rr] : 0.f, y1 = (rv && v1) ? y1s[rr] : 0.f;
        const float o0 = (rv && v0) ? din[lr * LIN_S + f0] : 0.f, o1 = (rv && v1) ? din[lr * LIN_S + f1] : 0.f;
        const float mean = wave_sum(y0 + y1) * invd;
        const float c0 = v0 ? y0 - mean : 0.f, c1 = v1 ? y1 - mean : 0.f;
        const float rstd = 1.f / sqrtf(wave_sum(c0 * c0 + c1 * c1) * invd + ln_eps);
        const float xh0 = c0 * rstd, xh1 = c1 * rstd;
        const float dx0 = o0 * g0, dx1 = o1 * g1;
        const float s1 = wave_sum(dx0 + dx1) * invd;
        const float s2 = wave_sum(dx0 * xh0 + dx1 * xh1) * invd;
        float z0 = rstd * (dx0 - s1 - xh0 * s2) * lrelu_grad(y0, slope);
        float z1 = rstd * (dx1 - s1 - xh1 * s2) * lrelu_grad(y1, slope);
        if (A.mul) {
            z0 *= m0s[rr];
            z1 *= m1s[rr];
        }
        if (v0) dout[lr * LIN_S + f0] = rv ? z0 : 0.f;
        if (v1) dout[lr * LIN_S + f1] = rv ? z1 : 0.f;
        if (rv && jY) {
            if (v0) jY[(size_t)row * ldy + f0] = z0;
            if (v1) jY[(size_t)row * ldy + f1] = z1;
        }
        if (rv) {
            dg0 += o0 * xh0;
            dg1 += o1 * xh1;
            db0 += o0;
            db1 += o1;
        }
    }
    red[wave][lane] = dg0;
    red[wave][64 + lane] = dg1;
    red[wave][128 + lane] = db0;
    red[wave][192 + lane] = db1;
    __syncthreads();
    jaux[(size_t)blockIdx.x * 256 + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

__global__ __launch_bounds__(EQD_BLOCK, 1) void k_rowchain_res_bwd_wide(ChainResBwdWideArg AW) {
    __shared__ ChainResBwdWideSmem S;
    __shared__ __attribute__((aligned(16))) float Lb[1][LIN_LOCALS][16 * LIN_S];      // tiles 0, 1, 2 of the chain
    __shared__ float red[EQD_WAVES][256];                                             // chain_lnbwd<1>'s partial sums
    const ChainResBwdArg& A = AW.c;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, g = lane >> 4;
    const int row0 = (int)blockIdx.x * 16, rows = A.rows, M = AW.M;
    // tiles 0 and 1 keep zeros in their columns M .. 79: the 16-deep steps read them (k_rowchain zeroes its tiles the same way)
    for (int i = t; i < LIN_LOCALS * 16 * LIN_S; i += EQD_BLOCK) (&Lb[0][0][0])[i] = 0.f;
    // ---- ordinary loads first, branch-free: first touched behind the vm_wait<0> ----------------------------------------------
    const int f0 = 16 * wave + 4 * g;
    const int rowi = row0 + l15;
    const bool rv = rowi < rows;
    const int rowe = rv ? rowi : rows - 1;
    const int fb = lane + 64 < M ? lane + 64 : 0;      // (chain_lnbwd: a feature beyond the layer reads column 0)
    float g0r = ((const EQD_GAS float*)A.ln_g)[lane], g1r = ((const EQD_GAS float*)A.ln_g)[fb];
    float y0s[4], y1s[4], m0s[4], m1s[4];
    {
        // (no dropout: valid bytes of ln_g that crbw_lnbwd drops - a load under a branch gets a wait of its own)
        const EQD_GAS float* const mp = (const EQD_GAS float*)(A.mul ? A.mul : A.ln_g);
        const int ldm = A.mul ? A.ld_mul : 0;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            int row = row0 + 4 * wave + rr;
            row = row < rows ? row : rows - 1;
            const size_t o = (size_t)row * A.ld_y, mo = (size_t)row * ldm;
            y0s[rr] = ((const EQD_GAS float*)A.y_act)[o + lane];
            y1s[rr] = ((const EQD_GAS float*)A.y_act)[o + fb];
            m0s[rr] = mp[mo + lane];
            m1s[rr] = mp[mo + fb];
        }
    }
    f32x4 res2 = *(const EQD_GAS f4v*)(A.xo[2].R + (size_t)rowe * A.xo[2].ldr + f0);
    // ---- the copies, in the order they are consumed ----------------------------------------------------------------------
    f32x4 acc = f4zero(), acc2 = f4zero();
#pragma unroll
    for (int s = 0; s < 6; ++s) crb_copy_rows(A.dh[s].X, A.dh[s].ldx, S.X[s], row0, rows, wave, lane);
    crb_copy_rows(A.dho.R, A.dho.ldr, S.X[6], row0, rows, wave, lane);
#pragma unroll
    for (int c = 0; c < 6; ++c) crb_copy_chunk(A.dh[c].W, A.dh[c].wcs, S.W[c][wave], wave, lane);
    {   // B4: block 4 of Wn2 (waves 0, 1) and of job 5's block (waves 2, 3), rows k = 32 (wave & 1) + (lane >> 1)
        const bool n2 = wave < 2;
        const float* const Wb = n2 ? A.a.W : A.x[1].W;
        const int wcs = n2 ? A.a.wcs : A.x[1].wcs;
        const int k = 32 * (wave & 1) + (lane >> 1);
        glds16(Wb + (size_t)k * wcs + ((lane & 1) ? M - 4 : 64), &S.B4[wave >> 1][256 * (wave & 1)]);
    }
    {   // Kr: rows k = 64 .. 68 of the three Wn1 blocks (m = 0 .. 63), then of job 5's block 4
        int G = 64 * wave + lane;
        G = G < 249 ? G : 249;
        const bool blk = G < 240;      // a row of one of the three blocks; otherwise a piece of block 4
        const int j = blk ? G / 80 : 1;
        const int r = blk ? (G % 80) >> 4 : (G - 240) >> 1;
        const int m = blk ? 4 * (G & 15) : ((G & 1) ? M - 4 : 64);
        // (the blocks are adjacent columns of one matrix - crbw_pack checks it: 64, M and 64 wide.  Arithmetic, not a
        //  per-lane choice among A.x[j].W: that compiles to an indexed load from the kernarg segment and a full wait)
        const int c0 = j == 0 ? 0 : (j == 1 ? 64 : 64 + M);
        glds16(A.x[0].W + (size_t)(64 + r) * A.x[0].wcs + c0 + m, &S.Kr[256 * wave]);
    }
    vm_wait<26>();
    lds_barrier();      // the row tiles of all six sources and the residual rows are in LDS (and Lb's zeros)
    // ---- dh of layer 1: six resident chunks; slots 0 .. 3 are refilled behind their own reads -------------------------------
    vm_wait<22>();
    crb_mma<false>(acc, acc2, S.W[0][wave], S.X[0], lane, l15, g);
    lds_reads_done();
    crb_copy_chunk(A.a.W, A.a.wcs, S.W[0][wave], wave, lane);
    vm_wait<22>();
    crb_mma<false>(acc, acc2, S.W[1][wave], S.X[1], lane, l15, g);
    lds_reads_done();
    crb_copy_chunk(A.x[0].W, A.x[0].wcs, S.W[1][wave], wave, lane);
    vm_wait<22>();
    crb_mma<false>(acc, acc2, S.W[2][wave], S.X[2], lane, l15, g);
    lds_reads_done();
    crb_copy_chunk(A.x[1].W, A.x[1].wcs, S.W[2][wave], wave, lane);
    vm_wait<22>();
    crb_mma<false>(acc, acc2, S.W[3][wave], S.X[3], lane, l15, g);
    lds_reads_done();
    crb_copy_chunk(A.x[2].W, A.x[2].wcs, S.W[3][wave], wave, lane);
    vm_wait<22>();
    crb_mma<false>(acc, acc2, S.W[4][wave], S.X[4], lane, l15, g);
    vm_wait<18>();
    crb_mma<false>(acc, acc2, S.W[5][wave], S.X[5], lane, l15, g);
    {
        const f32x4 resd = *(const f32x4*)&S.X[6][cr_at(l15, 4 * wave + g)];      // columns f0 .. f0 + 3 of row l15
        const f32x4 yv = crb_epilogue(acc, acc2, A.dho.alpha, A.dho.beta, resd);
        if (rv) *(EQD_GAS f4v*)&A.dho.Y[(size_t)rowi * A.dho.ldy + f0] = yv;
        *(f32x4*)&Lb[0][2][l15 * LIN_S + f0] = yv;
    }
    vm_wait<0>();      // nothing is in flight from here on: __syncthreads() is a plain barrier again
    keep_after_wait(g0r); keep_after_wait(g1r); keep_after_wait(res2);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        keep_after_wait(y0s[rr]); keep_after_wait(y1s[rr]); keep_after_wait(m0s[rr]); keep_after_wait(m1s[rr]);
    }
    __syncthreads();   // tile 2 is complete; B4 and Kr are published
    const bool own1 = wave == 0;      // (M + 15) / 16 = 5 output blocks: block 4 is wave 0's
    const int nf4 = M - 64 - 4 * g;   // valid features of block 4 at 64 + 4 g (<= 0: none)
    f32x4 av[2], av2[2], b[4];
    // ---- alpha dH(1) Wn2 -> tile 0 (general path: blocks wave and wave + 4) --------------------------------------------------
    av[0] = av[1] = av2[0] = av2[1] = f4zero();
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = *(const f32x4*)&Lb[0][2][l15 * LIN_S + 16 * q + 4 * g];
    crbw_mma(av, av2, S.W[0][wave], S.B4[0], b, own1, lane, l15, g);
    *(f32x4*)&Lb[0][0][l15 * LIN_S + f0] = crb_epilogue(av[0], av2[0], A.a_alpha, A.a_beta, f4zero());
    if (own1) {
        const f32x4 y4 = crb_epilogue(av[1], av2[1], A.a_alpha, A.a_beta, f4zero());
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < nf4) Lb[0][0][l15 * LIN_S + 64 + 4 * g + r] = y4[r];
    }
    __syncthreads();
    // ---- LeakyReLU / LayerNorm backward over M features: tile 0 -> dz, tile 1, the workgroup's ln_part row ------------------
    crbw_lnbwd(A, M, Lb, red, row0, g0r, g1r, y0s, y1s, m0s, m1s);
    __syncthreads();
    // ---- dz times the three column blocks of Wn1: the tile's fragments are the same for all three ---------------------------
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = *(const f32x4*)&Lb[0][1][l15 * LIN_S + 16 * q + 4 * g];
    const f32x4 brem = *(const f32x4*)&Lb[0][1][l15 * LIN_S + 64 + 4 * g];
    {   // d aggr_msg (lean path)
        av[0] = av[1] = av2[0] = av2[1] = f4zero();
        crbw_mma(av, av2, S.W[1][wave], S.B4[1], b, false, lane, l15, g);
        crbw_mma_rem(av, av2, &S.Kr[0], &S.Kr[960], brem, false, wave, l15, g);
        const f32x4 yv = crb_epilogue(av[0], av2[0], A.xo[0].alpha, A.xo[0].beta, f4zero());
        if (rv) *(EQD_GAS f4v*)&A.xo[0].Y[(size_t)rowi * A.xo[0].ldy + f0] = yv;
    }
    {   // d aggr_cross (general path: block 4 and the zero padding up to pad_to are wave 0's)
        av[0] = av[1] = av2[0] = av2[1] = f4zero();
        crbw_mma(av, av2, S.W[2][wave], S.B4[1], b, own1, lane, l15, g);
        crbw_mma_rem(av, av2, &S.Kr[320], &S.Kr[960], brem, own1, wave, l15, g);
        const f32x4 yv = crb_epilogue(av[0], av2[0], A.xo[1].alpha, A.xo[1].beta, f4zero());
        if (rv) *(EQD_GAS f4v*)&A.xo[1].Y[(size_t)rowi * A.xo[1].ldy + f0] = yv;
        if (own1) {
            const f32x4 y4 = crb_epilogue(av[1], av2[1], A.xo[1].alpha, A.xo[1].beta, f4zero());
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 64 + 4 * g + r;
                if (rv && (r < nf4 || f < AW.pad_to)) ((EQD_GAS float*)A.xo[1].Y)[(size_t)rowi * A.xo[1].ldy + f] = r < nf4 ? y4[r] : 0.f;
            }
        }
    }
    {   // dh0acc += (lean path, residual = the accumulator's rows)
        av[0] = av[1] = av2[0] = av2[1] = f4zero();
        crbw_mma(av, av2, S.W[3][wave], S.B4[1], b, false, lane, l15, g);
        crbw_mma_rem(av, av2, &S.Kr[640], &S.Kr[960], brem, false, wave, l15, g);
        const f32x4 yv = crb_epilogue(av[0], av2[0], A.xo[2].alpha, A.xo[2].beta, res2);
        if (rv) *(EQD_GAS f4v*)&A.xo[2].Y[(size_t)rowi * A.xo[2].ldy + f0] = yv;
    }
}

// k_rowchain_res_fwd: the forward node chain of a 64-wide layer (node_mlp.0 + LeakyReLU [+ dropout] + LayerNorm ->
// node_mlp.4 + skip) at DB5.5 sizes - one 16-row tile per workgroup, no more tiles than CUs - with every 64-wide weight
// chunk of BOTH jobs and the tile's source rows resident in LDS, filled by LDS-DMA (glds16, eqd_common.h) at kernel entry.
//
// Why: k_rowchain<1, false, 1> stages one K chunk at a time through a single buffer: global -> VGPR -> LDS -> barrier ->
// fragment reads -> MFMA -> barrier, 1 750 - 2 000 clocks per chunk for 512 clocks of MFMA, and the workgroup is alone on
// its CU, so every one of those clocks is wall time.  The chain's weights (64 KB + 16 KB) and rows (16 KB) fit the CU's
// LDS beside everything else; with all of them requested up front no buffer is reused, so no step waits for the one
// before it to be read.
//
// Layout.  A 64 x 64 chunk is a linear image of 256-byte rows, exactly what one glds16 per wave writes for four rows.  The
// fragment reads are b128 at (row 16 wave + l15, 16-byte column 4 q + g): 16 lanes of a group in one column of a linear
// image would meet in four banks, so the image is XOR-swizzled in 16-byte units, column c of row r lies at c ^ (r & 15);
// the permutation is applied to the per-lane SOURCE address of the copy and again by the reader (cr_at).
// Ownership.  Wave w multiplies output block w, i.e. weight rows 16 w .. 16 w + 15 of every chunk: it copies exactly
// those rows (4 copies per chunk) and needs only its own counted wait to read them - no barrier between the chunks of
// a job.  The four 16 x 64 source-row tiles are shared: each wave copies four rows of each, first of all, and ONE barrier
// publishes them.
// Order per wave: X0 X1 X2 X3 | W0 x4 | W1 x4 | W2 x4 | W3 x4 | Wn2 x4 = 24 copies; chunk c starts behind vm_wait<16 - 4 c>.
// Ordinary loads (epilogue operands of both jobs, the dropout factors, the 5-column remainder of the 69-wide h0 source)
// are requested BEFORE the copies - a use of an ordinary load makes the compiler wait for everything in flight - and are
// first touched behind the vm_wait<0> that follows the last chunk (keep_after_wait).
//
// Arithmetic: per output element the MFMA sequence, the k assignment inside a chunk (k = 16 (j >> 2) + 4 g + (j & 3)),
// the two accumulator sets, the order of sources and chunks (four full chunks, then the remainder step) and every epilogue
// expression are those of linear_tile_lean: the results are bit-identical to k_rowchain's.
#pragma once
#include "eqd_linear_inl.h"

#define CR_CHUNK (64 * 64)      /* floats of a weight chunk image */
#define CR_XTILE (16 * 64)      /* floats of a source-row tile image */
struct alignas(1024) ChainResFwdSmem {
    float W[5][CR_CHUNK];       // node_mlp.0 chunks 0 .. 3 (sources h, aggr_msg, aggr_cross, h0[:64]), node_mlp.4
    float X[4][CR_XTILE];
};
// float offset of 16-byte column c16 of row r in a swizzled image of 64-float rows
__device__ __forceinline__ int cr_at(int r, int c16) { return r * 64 + 4 * (c16 ^ (r & 15)); }

// 16 MFMAs of one 64-deep chunk for the wave's output block; Wi: the chunk image (rows = output features), Xi: the row tile
// (swizzled image, or a [16][LIN_S] tile when XPAD).  Same instruction order as lin_mma<1, 1, 4, false>.
template <bool XPAD>
__device__ __forceinline__ void cr_mma(f32x4& acc, f32x4& acc2, const float* __restrict__ Wi, const float* __restrict__ Xi,
                                       int wave, int l15, int g) {
    f32x4 a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = *(const f32x4*)&Wi[cr_at(16 * wave + l15, 4 * q + g)];
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = XPAD ? *(const f32x4*)&Xi[l15 * LIN_S + 16 * q + 4 * g] : *(const f32x4*)&Xi[cr_at(l15, 4 * q + g)];
#ifndef EQD_HOSTSIM
    __builtin_amdgcn_sched_barrier(0);      // every fragment read is issued before the first MFMA (see lin_mma)
#endif
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc = mfma4(a[q][0], b[q][0], acc);
        acc2 = mfma4(a[q][1], b[q][1], acc2);
        acc = mfma4(a[q][2], b[q][2], acc);
        acc2 = mfma4(a[q][3], b[q][3], acc2);
    }
    // both accumulator chains are complete HERE: left alone, the set that is only read in the epilogue sinks behind every
    // later wait, and its 32 MFMAs per chunk run after the last copy has landed instead of under the wait for the next
    keep_after_wait(acc);
    keep_after_wait(acc2);
}

__global__ __launch_bounds__(EQD_BLOCK, 1) void k_rowchain_res_fwd(EqdChainArg A) {
    __shared__ ChainResFwdSmem S;
    __shared__ LinSmem<1> sm;      // the remainder step's staging tiles and the LayerNorm exchange
    __shared__ __attribute__((aligned(16))) float Lt[16 * LIN_S];      // LayerNorm output: node_mlp.4's source rows
    const EqdLinJob& J0 = A.j[0].lin;
    const EqdLinJob& J1 = A.j[1].lin;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, g = lane >> 4;
    const int row0 = (int)blockIdx.x * 16, rows = J0.rows;
    EQD_TR_WG();
    EQD_TR(200);
    EQD_TR(210);
    // ---- ordinary loads first: epilogue operands of both jobs (features f0 .. f0 + 3 of row row0 + l15) ... -----------
    const int f0 = 16 * wave + 4 * g;
    const int rowi = row0 + l15;
    const bool rv = rowi < rows;
    const int rowe = rv ? rowi : rows - 1;
    f32x4 bias0 = f4zero(), lg = f4zero(), lb = f4zero(), mul0 = {1.f, 1.f, 1.f, 1.f}, bias1 = f4zero(), res1 = f4zero();
    if (J0.bias) bias0 = *(const EQD_GAS f4v*)(J0.bias + f0);
    lg = *(const EQD_GAS f4v*)(J0.ln_g + f0);
    lb = *(const EQD_GAS f4v*)(J0.ln_b + f0);
    if (J0.mul) mul0 = *(const EQD_GAS f4v*)(J0.mul + (size_t)rowe * J0.ld_mul + f0);
    if (J1.bias) bias1 = *(const EQD_GAS f4v*)(J1.bias + f0);
    if (J1.R) res1 = *(const EQD_GAS f4v*)(J1.R + (size_t)rowe * J1.ldr + f0);
    // ... and the remainder step of source 3 (columns 64 .. K - 1 of the 69-wide h0 and of its weight columns)
    EqdLinSrc S3 = J0.s[3];
    S3.mask = nullptr;      // (eligibility: no masked source)
    const LinStep crem = {3, 64, S3.K - 64 < 16 ? S3.K - 64 : 16};      // (K <= 80: one small step)
    LinRegs<1> RR;
    lin_load_s<1>(S3, 64, rows, false, crem, row0, t, RR);
    EQD_TR(211);      // (no stamp between here and vm_wait<0>: its store would count on vmcnt among the copies)
    // ---- the copies, in the order they are consumed ------------------------------------------------------------------
    {
        const int r = 4 * wave + (lane >> 4);      // row of the tile this lane copies a piece of
        const int c = 4 * ((lane & 15) ^ (r & 15));
        int row = row0 + r;
        row = row < rows ? row : rows - 1;
#pragma unroll
        for (int s = 0; s < 4; ++s) glds16(J0.s[s].X + (size_t)row * J0.s[s].ldx + c, &S.X[s][256 * wave]);
    }
#pragma unroll
    for (int ch = 0; ch < 5; ++ch) {
        const float* const Wg = ch < 4 ? J0.s[ch].W : J1.s[0].W;
        const int w_rs = ch < 4 ? J0.s[ch].w_rs : J1.s[0].w_rs;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = 16 * wave + 4 * i + (lane >> 4);
            glds16(Wg + (size_t)m * w_rs + 4 * ((lane & 15) ^ (m & 15)), &S.W[ch][64 * (16 * wave + 4 * i)]);
        }
    }
    // ---- node_mlp.0: four resident chunks, then the remainder step -----------------------------------------------------
    f32x4 acc = f4zero(), acc2 = f4zero();
    vm_wait<20>();
    lds_barrier();      // the row tiles of all four sources are in LDS
    vm_wait<16>();
    cr_mma<false>(acc, acc2, S.W[0], S.X[0], wave, l15, g);
    vm_wait<12>();
    cr_mma<false>(acc, acc2, S.W[1], S.X[1], wave, l15, g);
    vm_wait<8>();
    cr_mma<false>(acc, acc2, S.W[2], S.X[2], wave, l15, g);
    vm_wait<4>();
    cr_mma<false>(acc, acc2, S.W[3], S.X[3], wave, l15, g);
    vm_wait<0>();       // node_mlp.4's rows too: nothing is in flight from here on, __syncthreads() is a plain barrier again
    {
        float x = RR.x[0][0];
        keep_after_wait(x);
        RR.x[0][0] = x;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            float w = RR.w[j][0];
            keep_after_wait(w);
            RR.w[j][0] = w;
        }
    }
    keep_after_wait(bias0); keep_after_wait(lg); keep_after_wait(lb); keep_after_wait(mul0);
    keep_after_wait(bias1); keep_after_wait(res1);
    lin_store_s<1>(S3, 64, J0.slope, false, crem, t, RR, sm);
    __syncthreads();
    {
        f32x4 accv[1][2] = {{acc, f4zero()}}, acc2v[1][2] = {{acc2, f4zero()}};
        const float* Xs[1] = {sm.Xl[0]};
        const int mbs[2] = {wave, wave + 4};
        lin_mma<1, 1, 1, false, false, true>(accv, acc2v, Xs, sm.Wl, mbs, l15, g);
        acc = accv[0][0];
        acc2 = acc2v[0][0];
    }
    EQD_TR(212);
    EQD_TR(213);
    // ---- epilogue of node_mlp.0 (linear_tile_lean's, expression for expression) ---------------------------------------
    {
        const float slope = J0.slope;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float y = (acc[r] + acc2[r]) + bias0[r];
            if (J0.act) y = lrelu(y, slope);
            v[r] = y;
        }
        if (J0.mul) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= mul0[r];
        }
        const float invM = 1.f / 64.f;
        float s1 = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) s1 += v[r];
        s1 = group_sum(s1);
        if (g == 0) sm.stat[0][wave][l15] = s1;
        __syncthreads();
        const float mean = (sm.stat[0][0][l15] + sm.stat[0][1][l15] + sm.stat[0][2][l15] + sm.stat[0][3][l15]) * invM;
        float q = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dlt = v[r] - mean;
            q += dlt * dlt;
        }
        q = group_sum(q);
        __syncthreads();
        if (g == 0) sm.stat[0][wave][l15] = q;
        __syncthreads();
        const float rstd = 1.f / sqrtf((sm.stat[0][0][l15] + sm.stat[0][1][l15] + sm.stat[0][2][l15] + sm.stat[0][3][l15]) * invM +
                                       J0.ln_eps);
        if (J0.pre_ln && rv) *(EQD_GAS f4v*)&J0.pre_ln[(size_t)rowi * J0.ld_pre + f0] = f32x4{v[0], v[1], v[2], v[3]};
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (v[r] - mean) * rstd * lg[r] + lb[r];
        const float alpha = J0.alpha, beta = J0.beta;
        f32x4 yv;
#pragma unroll
        for (int r = 0; r < 4; ++r) yv[r] = alpha * v[r] + beta * 0.f;      // (no residual on this job: eligibility)
        if (J0.Y && rv) *(EQD_GAS f4v*)&J0.Y[(size_t)rowi * J0.ldy + f0] = yv;
        if (J0.Yb && rv) *(EQD_GAS s16x4*)&J0.Yb[(size_t)rowi * J0.ldyb + f0] = pack_bf4(yv[0], yv[1], yv[2], yv[3]);
        *(f32x4*)&Lt[l15 * LIN_S + f0] = yv;
    }
    __syncthreads();
    EQD_TR(201);
    EQD_TR(214);
    EQD_TR(215);
    // ---- node_mlp.4 (+ skip) on the tile in LDS ------------------------------------------------------------------------
    acc = f4zero();
    acc2 = f4zero();
    cr_mma<true>(acc, acc2, S.W[4], Lt, wave, l15, g);
    EQD_TR(216);
    EQD_TR(217);
    {
        const float slope = J1.slope;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float y = (acc[r] + acc2[r]) + bias1[r];
            if (J1.act) y = lrelu(y, slope);
            v[r] = y;
        }
        const float alpha = J1.alpha, beta = J1.beta;
        f32x4 yv;
#pragma unroll
        for (int r = 0; r < 4; ++r) yv[r] = alpha * v[r] + beta * res1[r];
        if (J1.Y && rv) *(EQD_GAS f4v*)&J1.Y[(size_t)rowi * J1.ldy + f0] = yv;
        if (J1.Yb && rv) *(EQD_GAS s16x4*)&J1.Yb[(size_t)rowi * J1.ldyb + f0] = pack_bf4(yv[0], yv[1], yv[2], yv[3]);
    }
    EQD_TR(202);
    EQD_TR_WG_END();
}

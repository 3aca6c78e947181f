// k_rowchain_res_bwd: the backward node chain of a 64-wide layer at DB5.5 sizes - one 16-row tile per workgroup, no more
// tiles than CUs, fp32 - with every 64 x 64 weight chunk of every job and every source-row tile resident in LDS, filled by
// LDS-DMA (glds16, eqd_common.h).  The chain is the one eqd_model_backward builds per layer (eqd_driver.hip, "ONE row chain"):
//   DH (six jobs, layers L-2 .. 1):  dh of the layer above (six transposed 64 x 64 sources, residual (1 - skip) dH(l+2),
//                                    written to dH(l+1) and kept as LDS tile 2)
//   both forms:                      alpha dH Wn2 -> tile 0;  LeakyReLU / LayerNorm backward -> dz, tile 1, the ln_part row;
//                                    dz times three 64-column blocks of Wn1 -> d aggr_msg, d aggr_cross, dh0acc (+= in DH)
//   !DH (five jobs, last layer):     the same without the dh job; dH(L) is a global source
//
// Why: k_rowchain<1, false, 1> stages one chunk at a time (global -> VGPR -> LDS -> barrier -> fragment reads -> MFMA ->
// barrier) and every single-chunk job pays a prologue, a prefetch and an epilogue around 512 clocks of MFMA; the workgroup is
// alone on its CU, so all of it is wall time.  Here every operand is requested at entry and the arithmetic runs under the
// CU's weight stream (see eqd_chainres_inl.h, the forward half).
//
// Layout.  All ten chunks are transposed sources, W[m + k w_cs]: in memory 64 rows (k) of 64 consecutive floats (m).  Wave w
// multiplies output block w, i.e. columns m = 16 w .. 16 w + 15 of all 64 rows: it copies exactly that 64-row x 64-byte slab
// (four glds16, one contiguous 4 KB image per wave) and reads nothing but LDS it filled itself - its own counted wait is all
// the ordering a chunk needs.  linear_tile_lean reads such a chunk as Wl[k][m], four scalar reads per lane and k-group q:
// a[q][j] = W(k = 16 q + 4 g + j, m = 16 w + l15).  The slab is laid out so that this is slab[256 q + 64 j + lane]: every
// read takes 64 consecutive floats, one per bank.  (Rows 4 apart - the four lane groups g of one read - would meet in the
// same 16 banks of a linear image: the image stores row k = 16 q + 4 g + j as row 16 q + 4 j + g.)  Copy i of a chunk fills
// slab[256 i .. 256 i + 255]: lane L brings the 16 bytes at k = 16 i + 4 ((L & 15) >> 2) + (L >> 4), m = 16 w + 4 (L & 3).
// The 16 x 64 source-row tiles (and the dh job's residual rows) are shared between the waves: swizzled images as in the
// forward body (cr_at), each wave copies four rows of each, first of all, and ONE barrier publishes them.
//
// No ring.  A slab is private to its wave, so the wave refills it as soon as its own fragment reads of it have returned
// (lds_reads_done), without a workgroup barrier: after the MFMA group of dh chunk c = 0 .. 3 it requests, into slot c, Wn2
// and then the three Wn1 column blocks.  They land under the remaining dh chunks and the dh epilogue.
//
// Copy order per wave and the wait of every consumer (N of vm_wait<N> = copies issued later that may stay in flight):
//   DH:   X0 .. X5 R | D0 x4 | D1 x4 | D2 x4 | D3 x4 | D4 x4 | D5 x4          31 copies at entry (R: the dh residual rows)
//         row tiles published      vm_wait<24>  + barrier
//         dh chunk 0               vm_wait<20>  (D1 .. D5)                      then Wn2 x4  -> slot 0
//         dh chunk 1               vm_wait<20>  (D2 .. D5, Wn2)                 then Wn1a x4 -> slot 1
//         dh chunk 2               vm_wait<20>  (D3 .. D5, Wn2, Wn1a)           then Wn1b x4 -> slot 2
//         dh chunk 3               vm_wait<20>  (D4, D5, Wn2, Wn1a, Wn1b)       then Wn1c x4 -> slot 3
//         dh chunk 4               vm_wait<20>  (D5, Wn2, Wn1a, Wn1b, Wn1c)
//         dh chunk 5               vm_wait<16>  (Wn2, Wn1a, Wn1b, Wn1c)                                       47 copies in all
//         dh epilogue (residual from LDS, store of dH(l+1), tile 2), then vm_wait<0> + barrier
//   !DH:  X0 | Wn2 x4 | Wn1a x4 | Wn1b x4 | Wn1c x4 = 17 copies, vm_wait<0> + barrier
// From that vm_wait<0> on nothing is in flight: __syncthreads() is a plain barrier again, which is what the exchanges of
// the LayerNorm backward (chain_lnbwd64_t) use, and the ordinary loads - requested BEFORE the first copy: y_act, ln_g, the
// dropout factors, the dh0acc accumulator rows - are first touched behind it (keep_after_wait).  The stream of the CU's
// copies is the bound up to that point; waiting for the three Wn1 blocks before Wn2's 16 MFMAs instead of after them gives
// away those MFMAs and the LayerNorm backward (about 1 500 clocks) and keeps every later step free of counted waits.
//
// Arithmetic: the order of sources and chunks, the k assignment inside a chunk, the two accumulator sets and every epilogue
// expression are linear_tile_lean's ((acc + acc2) + bias with bias = 0, alpha v + beta R); the LayerNorm backward IS
// chain_lnbwd64's.  Bit-identical to k_rowchain.
#pragma once
#include "eqd_chainres_inl.h"

// the compact argument: what this body reads and nothing else, packed by the host (crb_pack, eqd_node_kernels.hip), so that
// the kernel fetches it from the kernarg segment in one batch of scalar loads
struct CrbSrc {
    const float* X;     // [rows][ldx], 64 columns
    const float* W;     // element (m, k) at W[m + k * wcs]
    int ldx, wcs;
};
struct CrbOut {
    float* Y;           // [rows][ldy], 64 columns written; NULL: not stored
    const float* R;     // residual [rows][ldr], or NULL
    int ldy, ldr;
    float alpha, beta;
};
struct ChainResBwdArg {
    int rows, ld_y, ld_mul, ld_dz;
    float slope, ln_eps;
    CrbSrc dh[6];       // DH: the dh job's sources ...
    CrbOut dho;         // ... and its output (R is not NULL)
    CrbSrc a;           // alpha dH Wn2: W = Wn2; X = dH(L), read in the !DH form only
    float a_alpha, a_beta;
    const float *y_act, *ln_g, *mul;      // LayerNorm backward (mul: dropout factors or NULL)
    float *dz, *aux;
    CrbSrc x[3];        // dz times a Wn1 column block (X unused: the source is LDS tile 1) ...
    CrbOut xo[3];       // ... -> d aggr_msg, d aggr_cross, dh0acc (R on the last one only)
};

// the LayerNorm-backward job as chain_lnbwd64_t reads it: tile 0 -> tile 1, the operands requested at kernel entry
struct CrbLnJob {
    const ChainResBwdArg& A;
    f32x4 g4, y4, m4;
    __device__ __forceinline__ int rows() const { return A.rows; }
    __device__ __forceinline__ int src_l() const { return 0; }
    __device__ __forceinline__ int out_l() const { return 1; }
    __device__ __forceinline__ float slope() const { return A.slope; }
    __device__ __forceinline__ float ln_eps() const { return A.ln_eps; }
    __device__ __forceinline__ f32x4 gam(int) const { return g4; }
    __device__ __forceinline__ f32x4 y_act(int, int) const { return y4; }
    __device__ __forceinline__ float* Y() const { return A.dz; }
    __device__ __forceinline__ int ldy() const { return A.ld_dz; }
    __device__ __forceinline__ float* aux() const { return A.aux; }
    __device__ __forceinline__ f32x4 mul(int, int) const { return m4; }
};

#define CRB_SLAB 1024      /* floats of one wave's slab of a chunk */
template <bool DH>
struct alignas(1024) ChainResBwdSmem {
    float W[DH ? 6 : 4][EQD_WAVES][CRB_SLAB];
    float X[DH ? 7 : 1][CR_XTILE];
};

// the wave's four copies of one transposed chunk into its slab (see "Layout")
__device__ __forceinline__ void crb_copy_chunk(const float* W, int wcs, float* slab, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = 16 * i + 4 * ((lane & 15) >> 2) + (lane >> 4);
        glds16(W + (size_t)k * wcs + 16 * wave + 4 * (lane & 3), slab + 256 * i);
    }
}
// four rows per wave of a 16 x 64 row tile -> swizzled image (rows beyond the matrix: the last row, read and never written)
__device__ __forceinline__ void crb_copy_rows(const float* X, int ldx, float* tile, int row0, int rows, int wave, int lane) {
    const int r = 4 * wave + (lane >> 4);
    const int c = 4 * ((lane & 15) ^ (r & 15));
    int row = row0 + r;
    row = row < rows ? row : rows - 1;
    glds16(X + (size_t)row * ldx + c, tile + 256 * wave);
}
// 16 MFMAs of one 64-deep transposed chunk for the wave's output block: the instruction order of lin_mma<1, 1, 4, true>
template <bool XPAD>
__device__ __forceinline__ void crb_mma(f32x4& acc, f32x4& acc2, const float* __restrict__ slab, const float* __restrict__ Xi,
                                        int lane, int l15, int g) {
    f32x4 a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[q][j] = slab[256 * q + 64 * j + lane];
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
    keep_after_wait(acc);       // (both chains complete HERE, not behind a later wait: see cr_mma)
    keep_after_wait(acc2);
}
// linear_tile_lean's epilogue of a job without bias, activation and LayerNorm
__device__ __forceinline__ f32x4 crb_epilogue(const f32x4& acc, const f32x4& acc2, float alpha, float beta, const f32x4& res) {
    f32x4 yv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float y = (acc[r] + acc2[r]) + 0.f;
        yv[r] = alpha * y + beta * res[r];
    }
    return yv;
}

template <bool DH>
__global__ __launch_bounds__(EQD_BLOCK, 1) void k_rowchain_res_bwd(ChainResBwdArg A) {
    __shared__ ChainResBwdSmem<DH> S;
    __shared__ __attribute__((aligned(16))) float Lb[1][LIN_LOCALS][16 * LIN_S];      // tiles 0, 1, 2 of the chain
    __shared__ float stat[4][EQD_WAVES][16];                                          // chain_lnbwd64's exchange slots
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, g = lane >> 4;
    const int row0 = (int)blockIdx.x * 16, rows = A.rows;
    EQD_TR_WG();
    EQD_TR(200);
    // ---- ordinary loads first (features f0 .. f0 + 3 of row row0 + l15): first touched behind the vm_wait<0> ------------
    const int f0 = 16 * wave + 4 * g;
    const int rowi = row0 + l15;
    const bool rv = rowi < rows;
    const int rowe = rv ? rowi : rows - 1;
    f32x4 gam = *(const EQD_GAS f4v*)(A.ln_g + f0);
    f32x4 yp = *(const EQD_GAS f4v*)(A.y_act + (size_t)rowe * A.ld_y + f0);
    f32x4 mulv = {1.f, 1.f, 1.f, 1.f};
    if (A.mul) mulv = *(const EQD_GAS f4v*)(A.mul + (size_t)rowe * A.ld_mul + f0);
    f32x4 res2 = f4zero();
    if (A.xo[2].R) res2 = *(const EQD_GAS f4v*)(A.xo[2].R + (size_t)rowe * A.xo[2].ldr + f0);
    EQD_TR(201);      // (no stamp between here and the vm_wait<0>: its store would count on vmcnt among the copies)
    // ---- the copies, in the order they are consumed -------------------------------------------------------------------
    f32x4 acc = f4zero(), acc2 = f4zero();
    if constexpr (DH) {
#pragma unroll
        for (int s = 0; s < 6; ++s) crb_copy_rows(A.dh[s].X, A.dh[s].ldx, S.X[s], row0, rows, wave, lane);
        crb_copy_rows(A.dho.R, A.dho.ldr, S.X[6], row0, rows, wave, lane);
#pragma unroll
        for (int c = 0; c < 6; ++c) crb_copy_chunk(A.dh[c].W, A.dh[c].wcs, S.W[c][wave], wave, lane);
        vm_wait<24>();
        lds_barrier();      // the row tiles of all six sources and the residual rows are in LDS
        // ---- dh of the layer above: six resident chunks; slots 0 .. 3 are refilled behind their own reads ----------------
        vm_wait<20>();
        crb_mma<false>(acc, acc2, S.W[0][wave], S.X[0], lane, l15, g);
        lds_reads_done();
        crb_copy_chunk(A.a.W, A.a.wcs, S.W[0][wave], wave, lane);
        vm_wait<20>();
        crb_mma<false>(acc, acc2, S.W[1][wave], S.X[1], lane, l15, g);
        lds_reads_done();
        crb_copy_chunk(A.x[0].W, A.x[0].wcs, S.W[1][wave], wave, lane);
        vm_wait<20>();
        crb_mma<false>(acc, acc2, S.W[2][wave], S.X[2], lane, l15, g);
        lds_reads_done();
        crb_copy_chunk(A.x[1].W, A.x[1].wcs, S.W[2][wave], wave, lane);
        vm_wait<20>();
        crb_mma<false>(acc, acc2, S.W[3][wave], S.X[3], lane, l15, g);
        lds_reads_done();
        crb_copy_chunk(A.x[2].W, A.x[2].wcs, S.W[3][wave], wave, lane);
        vm_wait<20>();
        crb_mma<false>(acc, acc2, S.W[4][wave], S.X[4], lane, l15, g);
        vm_wait<16>();
        crb_mma<false>(acc, acc2, S.W[5][wave], S.X[5], lane, l15, g);
        EQD_TR(202);      // (behind the last counted wait: from here only vm_wait<0> follows)
        {
            const f32x4 resd = *(const f32x4*)&S.X[6][cr_at(l15, 4 * wave + g)];      // columns f0 .. f0 + 3 of row l15
            const f32x4 yv = crb_epilogue(acc, acc2, A.dho.alpha, A.dho.beta, resd);
            if (rv) *(EQD_GAS f4v*)&A.dho.Y[(size_t)rowi * A.dho.ldy + f0] = yv;
            *(f32x4*)&Lb[0][2][l15 * LIN_S + f0] = yv;
        }
        EQD_TR(203);
    } else {
        crb_copy_rows(A.a.X, A.a.ldx, S.X[0], row0, rows, wave, lane);
        crb_copy_chunk(A.a.W, A.a.wcs, S.W[0][wave], wave, lane);
#pragma unroll
        for (int c = 0; c < 3; ++c) crb_copy_chunk(A.x[c].W, A.x[c].wcs, S.W[1 + c][wave], wave, lane);
    }
    vm_wait<0>();      // nothing is in flight from here on: __syncthreads() is a plain barrier again
    keep_after_wait(gam); keep_after_wait(yp); keep_after_wait(mulv); keep_after_wait(res2);
    __syncthreads();   // DH: tile 2 is complete; !DH: the row tile of dH(L) is in LDS
    EQD_TR(204);
    // ---- alpha dH Wn2 -> tile 0 ------------------------------------------------------------------------------------------
    acc = f4zero();
    acc2 = f4zero();
    if constexpr (DH) crb_mma<true>(acc, acc2, S.W[0][wave], Lb[0][2], lane, l15, g);
    else crb_mma<false>(acc, acc2, S.W[0][wave], S.X[0], lane, l15, g);
    *(f32x4*)&Lb[0][0][l15 * LIN_S + f0] = crb_epilogue(acc, acc2, A.a_alpha, A.a_beta, f4zero());
    __syncthreads();
    EQD_TR(205);
    // ---- LeakyReLU / LayerNorm backward: tile 0 -> dz, tile 1, the workgroup's ln_part row -------------------------------
    chain_lnbwd64_t(CrbLnJob{A, gam, yp, mulv}, Lb, stat, row0);
    __syncthreads();
    EQD_TR(206);
    // ---- dz times the three column blocks of Wn1 --------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        acc = f4zero();
        acc2 = f4zero();
        crb_mma<true>(acc, acc2, S.W[1 + j][wave], Lb[0][1], lane, l15, g);
        const f32x4 yv = crb_epilogue(acc, acc2, A.xo[j].alpha, A.xo[j].beta, j == 2 ? res2 : f4zero());
        if (rv) *(EQD_GAS f4v*)&A.xo[j].Y[(size_t)rowi * A.xo[j].ldy + f0] = yv;
        EQD_TR(207 + j);
    }
    EQD_TR_WG_END();
}

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

//
// The carrying forms (NP = 5, NP = 1).  The tile of h[l+1] that node_mlp.4 leaves is the source of the next layer's five node
// projections (P, Q of the split first edge Linear, attention q / k / v: NP = 5) or, behind the last layer, of the head's
// mlp_h_mean_ROT (NP = 1).  As launches of their own (k_linear_simple, k_linear<1>) they pay a launch, a cold weight stream
// per CU and a second read of rows that were in this workgroup's LDS a few microseconds earlier; here the tile goes to LDS
// (the remainder step's staging tile, free since the LayerNorm exchanges) and the wave multiplies it by its 16 rows of every
// projection chunk: cr_mma<true> and k_linear_simple's / linear_tile_lean's epilogue expressions, the same bits.
// Their weights: requested right behind the vm_wait<0> that ends node_mlp.0's chunks, into slots W[0 .. 3] - each wave
// refills the rows it alone reads, behind its own lds_reads_done(), no barrier - and one more slot W[5]; they land under
// the remainder step, the LayerNorm epilogue and node_mlp.4, whose barriers are lds_barrier() in these forms
// (__syncthreads() would wait for every copy in flight).  Order P Q q k v: job j starts behind vm_wait<4 (NP - 1 - j)>.
// Why not earlier, behind each node_mlp.0 chunk: the epilogue operands are ordinary loads, and the compiler puts its own
// wait in front of their first use, counted WITHOUT the copies it cannot see - with projection copies in flight at that
// point it would wait for all of them.  The CU's copy stream is the bound up to the vm_wait<0> and the job chain behind
// it (about 1 000 clocks per job) is longer than the 80 KB take to arrive, so the later request costs one memory latency.
// Stores count on vmcnt as the copies do: in these forms every global store (pre_ln, a1n, h[l+1], the projections) is held
// in registers until the last chunk has been waited for.
#define CR_CHUNK (64 * 64)      /* floats of a weight chunk image */
#define CR_XTILE (16 * 64)      /* floats of a source-row tile image */
template <int NW>
struct alignas(1024) ChainResFwdSmem {
    float W[NW][CR_CHUNK];      // node_mlp.0 chunks 0 .. 3 (sources h, aggr_msg, aggr_cross, h0[:64]), node_mlp.4[, a projection]
    float X[4][CR_XTILE];
};
// the compact argument: what this body reads and nothing else, packed by the host (crf_pack, eqd_node_kernels.hip) while
// it matches the job list, so that the kernel fetches it from the kernarg segment in one batch of scalar loads
struct CrfSrc {
    const float* X;     // [rows][ldx]
    const float* W;     // element (m, k) at W[m * w_rs + k]
    int ldx, w_rs;
};
struct CrfProj {        // a carried job: Y = alpha * act((h[l+1] W^T) + bias) [* pmul]
    const float* W;
    const float* bias;  // or NULL
    float* Y;
    int w_rs, ldy, act;
    float slope, alpha, beta;
};
struct ChainResFwdArg {
    int rows, K3;       // K3: width of source 3 (65 .. 80)
    int act0, ld_mul0, ld_pre, ldy0, ldyb0;
    int act1, w1_rs, ldr1, ldy1, ldyb1, ld_pmul;
    float slope0, ln_eps, alpha0, beta0, slope1, alpha1, beta1;
    CrfSrc s[4];        // node_mlp.0's sources
    const float *bias0, *ln_g, *ln_b, *mul0;
    float *pre_ln, *Y0;
    unsigned short* Yb0;
    const float *W1, *bias1, *R1;      // node_mlp.4
    float* Y1;
    unsigned short* Yb1;
    const float* pmul;  // NP = 1: the head's dropout factors [rows][ld_pmul], or NULL
    CrfProj p[5];
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

// cr_mma<true> with the row tile's fragments b[q] = Xi[l15][16 q + 4 g ..] already in registers (same MFMA order, same bits)
__device__ __forceinline__ void cr_mma_b(f32x4& acc, f32x4& acc2, const float* __restrict__ Wi, const f32x4 (&b)[4], int wave,
                                         int l15, int g) {
    f32x4 a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = *(const f32x4*)&Wi[cr_at(16 * wave + l15, 4 * q + g)];
#ifndef EQD_HOSTSIM
    __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc = mfma4(a[q][0], b[q][0], acc);
        acc2 = mfma4(a[q][1], b[q][1], acc2);
        acc = mfma4(a[q][2], b[q][2], acc);
        acc2 = mfma4(a[q][3], b[q][3], acc2);
    }
    keep_after_wait(acc);
    keep_after_wait(acc2);
}
// the barrier of a step that exchanges through LDS only: with copies in flight (CNT) the one that leaves them in flight
template <bool CNT>
__device__ __forceinline__ void cr_bar() {
    if constexpr (CNT) lds_barrier();
    else __syncthreads();
}
// the wave's four copies of its 16 rows of a k-contiguous 64 x 64 chunk into the swizzled image
__device__ __forceinline__ void cr_copy_chunk(const float* Wg, int w_rs, float* img, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = 16 * wave + 4 * i + (lane >> 4);
        glds16(Wg + (size_t)m * w_rs + 4 * ((lane & 15) ^ (m & 15)), &img[64 * (16 * wave + 4 * i)]);
    }
}
// slot of the carried job j's chunk
__device__ __forceinline__ constexpr int cr_pslot(int j) { return j < 4 ? j : 5; }

template <int NP>
__global__ __launch_bounds__(EQD_BLOCK, 1) void k_rowchain_res_fwd(ChainResFwdArg A) {
    static_assert(NP == 0 || NP == 1 || NP == 5, "two jobs, + the head's job, + the next layer's five projections");
    constexpr bool PJ = NP > 0;
    __shared__ ChainResFwdSmem<(NP > 4 ? 6 : 5)> S;
    __shared__ LinSmem<1> sm;      // the remainder step's staging tiles and the LayerNorm exchange
    __shared__ __attribute__((aligned(16))) float Lt[16 * LIN_S];      // LayerNorm output: node_mlp.4's source rows
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, g = lane >> 4;
    const int row0 = (int)blockIdx.x * 16, rows = A.rows;
    EQD_TR_WG();
    EQD_TR(200);
    EQD_TR(210);
    // ---- ordinary loads first: epilogue operands of every job (features f0 .. f0 + 3 of row row0 + l15) ... ------------
    const int f0 = 16 * wave + 4 * g;
    const int rowi = row0 + l15;
    const bool rv = rowi < rows;
    const int rowe = rv ? rowi : rows - 1;
    f32x4 bias0 = f4zero(), lg = f4zero(), lb = f4zero(), mul0 = {1.f, 1.f, 1.f, 1.f}, bias1 = f4zero(), res1 = f4zero();
    if (A.bias0) bias0 = *(const EQD_GAS f4v*)(A.bias0 + f0);
    lg = *(const EQD_GAS f4v*)(A.ln_g + f0);
    lb = *(const EQD_GAS f4v*)(A.ln_b + f0);
    if (A.mul0) mul0 = *(const EQD_GAS f4v*)(A.mul0 + (size_t)rowe * A.ld_mul0 + f0);
    if (A.bias1) bias1 = *(const EQD_GAS f4v*)(A.bias1 + f0);
    if (A.R1) res1 = *(const EQD_GAS f4v*)(A.R1 + (size_t)rowe * A.ldr1 + f0);
    f32x4 pbias[PJ ? NP : 1], pmul = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int j = 0; j < (PJ ? NP : 1); ++j) pbias[j] = f4zero();
    if constexpr (PJ) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {      // (branch-free: a job without bias reads 16 valid bytes that are dropped below)
            const float* const bp = A.p[j].bias ? A.p[j].bias : A.ln_g;
            pbias[j] = *(const EQD_GAS f4v*)(bp + f0);
        }
        if (NP == 1 && A.pmul) pmul = *(const EQD_GAS f4v*)(A.pmul + (size_t)rowe * A.ld_pmul + f0);
    }
    // ... and the remainder step of source 3 (columns 64 .. K - 1 of the 69-wide h0 and of its weight columns)
    EqdLinSrc S3;
    S3.X = A.s[3].X; S3.mask = nullptr; S3.W = A.s[3].W;      // (eligibility: no masked source)
    S3.ldx = A.s[3].ldx; S3.K = A.K3; S3.w_rs = A.s[3].w_rs; S3.w_cs = 1;
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
        for (int s = 0; s < 4; ++s) glds16(A.s[s].X + (size_t)row * A.s[s].ldx + c, &S.X[s][256 * wave]);
    }
#pragma unroll
    for (int ch = 0; ch < 5; ++ch) cr_copy_chunk(ch < 4 ? A.s[ch].W : A.W1, ch < 4 ? A.s[ch].w_rs : A.w1_rs, S.W[ch], wave, lane);
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
    vm_wait<0>();       // node_mlp.4's rows too: nothing is in flight here, the ordinary loads are first touched behind it
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
    EQD_TR(203);      // (behind the vm_wait<0>: older than every copy that follows)
    if constexpr (PJ) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            keep_after_wait(pbias[j]);
            if (!A.p[j].bias) pbias[j] = f4zero();
        }
        keep_after_wait(pmul);
        // the carried jobs' chunks, in the order they are consumed: slots 0 .. 3 behind this wave's own reads of them
        lds_reads_done();
#pragma unroll
        for (int j = 0; j < NP; ++j) cr_copy_chunk(A.p[j].W, A.p[j].w_rs, S.W[cr_pslot(j)], wave, lane);
    }
    lin_store_s<1>(S3, 64, A.slope0, false, crem, t, RR, sm);
    cr_bar<PJ>();
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
    f32x4 pre4 = f4zero(), y0v = f4zero(), y1v = f4zero();      // PJ: what the plain form stores as it goes
    {
        const float slope = A.slope0;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float y = (acc[r] + acc2[r]) + bias0[r];
            if (A.act0) y = lrelu(y, slope);
            v[r] = y;
        }
        if (A.mul0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= mul0[r];
        }
        const float invM = 1.f / 64.f;
        float s1 = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) s1 += v[r];
        s1 = group_sum(s1);
        if (g == 0) sm.stat[0][wave][l15] = s1;
        cr_bar<PJ>();
        const float mean = (sm.stat[0][0][l15] + sm.stat[0][1][l15] + sm.stat[0][2][l15] + sm.stat[0][3][l15]) * invM;
        float q = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dlt = v[r] - mean;
            q += dlt * dlt;
        }
        q = group_sum(q);
        cr_bar<PJ>();
        if (g == 0) sm.stat[0][wave][l15] = q;
        cr_bar<PJ>();
        const float rstd = 1.f / sqrtf((sm.stat[0][0][l15] + sm.stat[0][1][l15] + sm.stat[0][2][l15] + sm.stat[0][3][l15]) * invM +
                                       A.ln_eps);
        if constexpr (PJ) pre4 = f32x4{v[0], v[1], v[2], v[3]};
        else if (A.pre_ln && rv) *(EQD_GAS f4v*)&A.pre_ln[(size_t)rowi * A.ld_pre + f0] = f32x4{v[0], v[1], v[2], v[3]};
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (v[r] - mean) * rstd * lg[r] + lb[r];
        const float alpha = A.alpha0, beta = A.beta0;
        f32x4 yv;
#pragma unroll
        for (int r = 0; r < 4; ++r) yv[r] = alpha * v[r] + beta * 0.f;      // (no residual on this job: eligibility)
        if constexpr (PJ) y0v = yv;
        else {
            if (A.Y0 && rv) *(EQD_GAS f4v*)&A.Y0[(size_t)rowi * A.ldy0 + f0] = yv;
            if (A.Yb0 && rv) *(EQD_GAS s16x4*)&A.Yb0[(size_t)rowi * A.ldyb0 + f0] = pack_bf4(yv[0], yv[1], yv[2], yv[3]);
        }
        *(f32x4*)&Lt[l15 * LIN_S + f0] = yv;
    }
    cr_bar<PJ>();
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
        const float slope = A.slope1;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float y = (acc[r] + acc2[r]) + bias1[r];
            if (A.act1) y = lrelu(y, slope);
            v[r] = y;
        }
        const float alpha = A.alpha1, beta = A.beta1;
        f32x4 yv;
#pragma unroll
        for (int r = 0; r < 4; ++r) yv[r] = alpha * v[r] + beta * res1[r];
        if constexpr (PJ) y1v = yv;
        else {
            if (A.Y1 && rv) *(EQD_GAS f4v*)&A.Y1[(size_t)rowi * A.ldy1 + f0] = yv;
            if (A.Yb1 && rv) *(EQD_GAS s16x4*)&A.Yb1[(size_t)rowi * A.ldyb1 + f0] = pack_bf4(yv[0], yv[1], yv[2], yv[3]);
        }
    }
    EQD_TR(202);
    // ---- the carried jobs on the tile of h[l+1] ------------------------------------------------------------------------
    if constexpr (PJ) {
        float* const Ht = sm.Xl[0];      // (last read by the remainder step, four barriers ago)
        *(f32x4*)&Ht[l15 * LIN_S + f0] = y1v;
        lds_barrier();
        f32x4 hb[4], po[NP];      // the tile's fragments are the same for every carried job: read once
#pragma unroll
        for (int q = 0; q < 4; ++q) hb[q] = *(const f32x4*)&Ht[l15 * LIN_S + 16 * q + 4 * g];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            // copies issued behind job j's: 4 per later job
            if (j == NP - 1) vm_wait<0>();
            else if (j == NP - 2) vm_wait<4>();
            else if (j == NP - 3) vm_wait<8>();
            else if (j == NP - 4) vm_wait<12>();
            else vm_wait<16>();
            if (j == NP - 1) {      // no counted wait is left: everything held back so far goes out under the last job
                if (A.pre_ln && rv) *(EQD_GAS f4v*)&A.pre_ln[(size_t)rowi * A.ld_pre + f0] = pre4;
                if (A.Y0 && rv) *(EQD_GAS f4v*)&A.Y0[(size_t)rowi * A.ldy0 + f0] = y0v;
                if (A.Yb0 && rv) *(EQD_GAS s16x4*)&A.Yb0[(size_t)rowi * A.ldyb0 + f0] = pack_bf4(y0v[0], y0v[1], y0v[2], y0v[3]);
                if (A.Y1 && rv) *(EQD_GAS f4v*)&A.Y1[(size_t)rowi * A.ldy1 + f0] = y1v;
                if (A.Yb1 && rv) *(EQD_GAS s16x4*)&A.Yb1[(size_t)rowi * A.ldyb1 + f0] = pack_bf4(y1v[0], y1v[1], y1v[2], y1v[3]);
#pragma unroll
                for (int i = 0; i < NP - 1; ++i)
                    if (rv) *(EQD_GAS f4v*)&A.p[i].Y[(size_t)rowi * A.p[i].ldy + f0] = po[i];
            }
            acc = f4zero();
            acc2 = f4zero();
            cr_mma_b(acc, acc2, S.W[cr_pslot(j)], hb, wave, l15, g);
            const CrfProj& P = A.p[j];
            const float slope = P.slope, alpha = P.alpha, beta = P.beta;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float y = (acc[r] + acc2[r]) + pbias[j][r];
                if (P.act) y = lrelu(y, slope);
                if (NP == 1 && A.pmul) y *= pmul[r];
                po[j][r] = alpha * y + beta * 0.f;      // (no residual: linear_tile_lean's expression with res = 0)
            }
            EQD_TR(218 + j);
        }
        if (rv) *(EQD_GAS f4v*)&A.p[NP - 1].Y[(size_t)rowi * A.p[NP - 1].ldy + f0] = po[NP - 1];
    }
    EQD_TR_WG_END();
}

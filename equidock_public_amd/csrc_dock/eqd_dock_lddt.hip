// Batched lDDT and interface lDDT (include/equidock_dock.h): the superposition-free comparison of a model with its native
// over EVERY heavy atom of C complexes in one device pass - per atom how many of its native neighbours (other residues,
// closer than the inclusion radius) keep their distance in the model within each of four thresholds, over all partners and
// over the partners on the other side.
//   d = sqrt((dx dx + dy dy) + dz dz); included: d_n < radius; preserved at k: fabs(d_m - d_n) < t_k
//   fp64 from the fp32 rows, -ffp-contract=off
//
// Work decomposition.  Four launches, whatever C is; a complex's atoms are its ligand rows followed by its receptor rows,
// and the rows of each side are cut into blocks of LD_BLOCK consecutive rows (ligand blocks first):
//   k_ld_bounds    one thread per atom: its global residue index (a search of its side's residue table), its ten counters
//                  zeroed; the thread of a block's first row also adds up the block's native centroid in row order and
//                  finds its radius, the thread of a complex's first row zeroes the complex's count of skipped block pairs
//   k_ld_pairs     items (complex, row block a, LD_STAGE consecutive column blocks): the workgroup stages the native and
//                  model positions and the residue index of the column atoms in LDS; lane l of every wave owns row l of
//                  block a (positions in fp64 and counters in registers) and wave w walks the staged blocks w, w + 4, ...
//                  reading one column atom at a time - an LDS broadcast.  A block pair the bound rules out is passed over
//                  (prune != 0) and counted; inside a block pair the square root is skipped where s >= (radius + 1e-6)^2,
//                  and the model distance is evaluated only for included pairs.  Whether a partner is on the other side
//                  is a property of the block pair.  The four waves' counters meet in LDS and leave with integer atomics.
//   k_ld_residues  one thread per residue: the 64-bit sums of its atoms' counters and its two scores
//   k_ld_finish    one workgroup per complex: thread-strided 64-bit sums of the ligand's and of the receptor's counters,
//                  combined through LDS; one thread writes the row
// Every output is an integer count or a quotient of two such counts, and integer addition does not care about order: a
// complex's results are bit-identical alone, in any batch, at any position, with prune on or off and from run to run.
#include "../csrc/eqd_common.h"
#include "../../include/equidock_dock.h"

#include <math.h>
#include <vector>

#define LD_BLOCK EQD_DOCK_LDDT_BLOCK    // rows per block (one per lane)
#define LD_STAGE 8                      // column blocks staged per item
#define LD_COLS (LD_BLOCK * LD_STAGE)   // column atoms staged per item
#define LD_NCNT 10                      // counters per atom
#define LD_SKIP_MARGIN 1e-6

static_assert(LD_BLOCK == 64, "one row per lane");
static_assert(LD_STAGE % EQD_WAVES == 0 && LD_COLS % EQD_BLOCK == 0, "the waves split the staged blocks evenly");

struct LddtDesc {           // one complex of the batch (entry C: the totals)
    int32_t la0, nla, ra0, nra;     // atom rows
    int32_t lr0, nlr, rr0, nrr;     // residues
    int32_t a0;                     // first row of the complex in the per-atom workspace arrays (= la0 + ra0)
    int32_t nbl, nb;                // blocks of the ligand, of both sides
    int32_t nrange;                 // items per row block = ceil(nb / LD_STAGE)
    int32_t item_base, blk_base;    // first item, first block
    int32_t pad[2];
};

struct LddtWs {
    const LddtDesc* desc;   // [C + 1]
    int32_t* resid;         // [A_l + A_r] global residue index (receptor residues after all ligand residues)
    double* blk;            // [blocks][4] native centroid and radius
    int32_t* skipped;       // [C] ordered block pairs the bound ruled out
};

struct LddtParams {
    double radius, skip2, bound;    // inclusion radius, (radius + 1e-6)^2, radius + 1e-6
    double t[4];
};

// the complex that owns atom / item / residue `v`: the largest c with base(c) <= v (kind 0 atoms, 1 ligand residues,
// 2 receptor residues, 3 items; the bases are strictly increasing)
template <int kKind>
__device__ __forceinline__ int ld_find(const LddtDesc* __restrict__ D, int C, int v) {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int b = kKind == 0 ? D[mid].a0 : kKind == 1 ? D[mid].lr0 : kKind == 2 ? D[mid].rr0 : D[mid].item_base;
        if (b <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// block b of complex d: its first local row and its rows
__device__ __forceinline__ void ld_block(const LddtDesc& d, int b, int& g0, int& n) {
    const bool l = b < d.nbl;
    const int q0 = (l ? b : b - d.nbl) * LD_BLOCK, ns = l ? d.nla : d.nra;
    g0 = (l ? 0 : d.nla) + q0;
    n = ns - q0 < LD_BLOCK ? ns - q0 : LD_BLOCK;
}

// local row g (0 <= g < nla + nra) of complex d: the row of its side's arrays
__device__ __forceinline__ size_t ld_row(const LddtDesc& d, int g) {
    return g < d.nla ? (size_t)d.la0 + g : (size_t)d.ra0 + (g - d.nla);
}

__device__ __forceinline__ double ld_dist(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

__device__ __forceinline__ double ld_score(long long N, long long P0, long long P1, long long P2, long long P3) {
    return N == 0 ? __builtin_nan("") : (double)(P0 + P1 + P2 + P3) / (4.0 * (double)N);
}

__global__ __launch_bounds__(EQD_BLOCK) void k_ld_bounds(int C, const float* __restrict__ lig_true,
                                                         const float* __restrict__ rec_true,
                                                         const int32_t* __restrict__ lfirst,
                                                         const int32_t* __restrict__ rfirst, int32_t* __restrict__ lig_counts,
                                                         int32_t* __restrict__ rec_counts, LddtWs W) {
    const int t = blockIdx.x * EQD_BLOCK + threadIdx.x;
    if (t >= W.desc[C].a0) return;
    const int c = ld_find<0>(W.desc, C, t);
    const LddtDesc d = W.desc[c];
    const int g = t - d.a0;
    const bool l = g < d.nla;
    const int row = (int)ld_row(d, g);
    // the last residue of this side of the complex whose first row is not behind the atom
    const int32_t* __restrict__ first = l ? lfirst : rfirst;
    int lo = l ? d.lr0 : d.rr0, hi = lo + (l ? d.nlr : d.nrr) - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    W.resid[t] = l ? lo : W.desc[C].lr0 + lo;
    int32_t* __restrict__ o = (l ? lig_counts : rec_counts) + (size_t)row * LD_NCNT;
#pragma unroll
    for (int k = 0; k < LD_NCNT; ++k) o[k] = 0;
    if (g == 0) W.skipped[c] = 0;
    const int q = l ? g : g - d.nla;
    if (q % LD_BLOCK == 0) {
        const int ns = l ? d.nla : d.nra, n = ns - q < LD_BLOCK ? ns - q : LD_BLOCK;
        const float* __restrict__ x = (l ? lig_true : rec_true) + (size_t)row * 3;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int a = 0; a < n; ++a) {
            sx += (double)x[a * 3];
            sy += (double)x[a * 3 + 1];
            sz += (double)x[a * 3 + 2];
        }
        const double cx = sx / (double)n, cy = sy / (double)n, cz = sz / (double)n;
        double far = 0.0;
        for (int a = 0; a < n; ++a) {
            const double e = ld_dist((double)x[a * 3] - cx, (double)x[a * 3 + 1] - cy, (double)x[a * 3 + 2] - cz);
            far = e > far ? e : far;
        }
        double* __restrict__ b = W.blk + ((size_t)d.blk_base + (l ? 0 : d.nbl) + q / LD_BLOCK) * 4;
        b[0] = cx;
        b[1] = cy;
        b[2] = cz;
        b[3] = far;
    }
}

__global__ __launch_bounds__(EQD_BLOCK) void k_ld_pairs(int C, const float* __restrict__ lig_pred,
                                                        const float* __restrict__ rec_pred,
                                                        const float* __restrict__ lig_true,
                                                        const float* __restrict__ rec_true, LddtParams P, int prune,
                                                        int32_t* __restrict__ lig_counts, int32_t* __restrict__ rec_counts,
                                                        LddtWs W) {
    __shared__ double cn[3][LD_COLS], cm[3][LD_COLS];           // column atoms: native, model
    __shared__ int32_t cres[LD_COLS];
    __shared__ int32_t acc[LD_BLOCK * LD_NCNT];
    const int item = blockIdx.x;
    if (item >= W.desc[C].item_base) return;
    const int c = ld_find<3>(W.desc, C, item);
    const LddtDesc d = W.desc[c];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int a = (item - d.item_base) / d.nrange, b0 = ((item - d.item_base) % d.nrange) * LD_STAGE;
    for (int s = tid; s < LD_COLS; s += EQD_BLOCK) {
        const int b = b0 + s / LD_BLOCK, r = s % LD_BLOCK;
        if (b >= d.nb) continue;
        int g0, n;
        ld_block(d, b, g0, n);
        if (r >= n) continue;
        const int g = g0 + r;
        const bool l = g < d.nla;
        const size_t row = ld_row(d, g);
        const float* __restrict__ xn = (l ? lig_true : rec_true) + row * 3;
        const float* __restrict__ xm = (l ? lig_pred : rec_pred) + row * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            cn[k][s] = (double)xn[k];
            cm[k][s] = (double)xm[k];
        }
        cres[s] = W.resid[d.a0 + g];
    }
    for (int e = tid; e < LD_BLOCK * LD_NCNT; e += EQD_BLOCK) acc[e] = 0;
    __syncthreads();
    int ga0, na;
    ld_block(d, a, ga0, na);
    const bool valid = lane < na;
    const int gi = ga0 + (valid ? lane : 0);
    const bool lig_a = a < d.nbl;
    const size_t rowi = ld_row(d, gi);
    const float* __restrict__ xn = (lig_a ? lig_true : rec_true) + rowi * 3;
    const float* __restrict__ xm = (lig_a ? lig_pred : rec_pred) + rowi * 3;
    const double nx = (double)xn[0], ny = (double)xn[1], nz = (double)xn[2];
    const double mx = (double)xm[0], my = (double)xm[1], mz = (double)xm[2];
    const int res_i = W.resid[d.a0 + gi];
    const double* __restrict__ ba = W.blk + ((size_t)d.blk_base + a) * 4;
    const double ax = ba[0], ay = ba[1], az = ba[2], ar = ba[3];
    int cnt[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};         // [same side | other side]: n, p_0..p_3
    int nskip = 0;
    for (int k = w; k < LD_STAGE; k += EQD_WAVES) {
        const int b = b0 + k;                                   // (wave-uniform, like everything up to the column loop)
        if (b >= d.nb) break;
        if (prune) {
            const double* __restrict__ bb = W.blk + ((size_t)d.blk_base + b) * 4;
            const double gap = (ld_dist(ax - bb[0], ay - bb[1], az - bb[2]) - ar) - bb[3];
            if (gap >= P.bound) {                               // no atom pair of (a, b) can be included
                ++nskip;
                continue;
            }
        }
        int g0, n;
        ld_block(d, b, g0, n);
        const int inter = (b < d.nbl) != lig_a ? 1 : 0;
        int m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
        for (int j = 0; j < n; ++j) {
            const int s = k * LD_BLOCK + j;
            const double dx = nx - cn[0][s], dy = ny - cn[1][s], dz = nz - cn[2][s];
            const double sq = (dx * dx + dy * dy) + dz * dz;
            if (sq >= P.skip2) continue;                        // d_n >= radius for certain
            const double dn = sqrt(sq);
            if (!(dn < P.radius) || cres[s] == res_i) continue;
            const double dm = ld_dist(mx - cm[0][s], my - cm[1][s], mz - cm[2][s]);
            const double diff = fabs(dm - dn);
            m0 += 1;
            m1 += diff < P.t[0] ? 1 : 0;
            m2 += diff < P.t[1] ? 1 : 0;
            m3 += diff < P.t[2] ? 1 : 0;
            m4 += diff < P.t[3] ? 1 : 0;
        }
        cnt[inter][0] += m0;
        cnt[inter][1] += m1;
        cnt[inter][2] += m2;
        cnt[inter][3] += m3;
        cnt[inter][4] += m4;
    }
    if (valid) {                                                // (integer atomics: the order changes nothing)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int all = cnt[0][k] + cnt[1][k];
            if (all) atomicAdd(&acc[lane * LD_NCNT + k], all);
            if (cnt[1][k]) atomicAdd(&acc[lane * LD_NCNT + 5 + k], cnt[1][k]);
        }
    }
    if (lane == 0 && nskip) atomicAdd(&W.skipped[c], nskip);
    __syncthreads();
    int32_t* __restrict__ o = (lig_a ? lig_counts : rec_counts) + ld_row(d, ga0) * LD_NCNT;
    for (int e = tid; e < na * LD_NCNT; e += EQD_BLOCK) {
        const int v = acc[e];
        if (v) atomicAdd(&o[e], v);
    }
}

// atom rows [a0, a1) of residue g, held inside its complex's rows [lo, hi) whatever the table says
__device__ __forceinline__ void ld_range(const int32_t* __restrict__ first, int g, int lo, int hi, int& a0, int& a1) {
    a0 = first[g];
    a1 = first[g + 1];
    a0 = a0 < lo ? lo : (a0 > hi ? hi : a0);
    a1 = a1 < a0 ? a0 : (a1 > hi ? hi : a1);
}

__global__ __launch_bounds__(EQD_BLOCK) void k_ld_residues(int C, const int32_t* __restrict__ lfirst,
                                                           const int32_t* __restrict__ rfirst,
                                                           const int32_t* __restrict__ lig_counts,
                                                           const int32_t* __restrict__ rec_counts,
                                                           double* __restrict__ lig_res_lddt,
                                                           double* __restrict__ rec_res_lddt, LddtWs W) {
    const int Rl = W.desc[C].lr0, Rr = W.desc[C].rr0;
    int r = blockIdx.x * EQD_BLOCK + threadIdx.x;
    if (r >= Rl + Rr) return;
    const bool l = r < Rl;
    if (!l) r -= Rl;
    const LddtDesc d = W.desc[l ? ld_find<1>(W.desc, C, r) : ld_find<2>(W.desc, C, r)];
    int a0, a1;
    if (l) ld_range(lfirst, r, d.la0, d.la0 + d.nla, a0, a1);
    else ld_range(rfirst, r, d.ra0, d.ra0 + d.nra, a0, a1);
    const int32_t* __restrict__ cnt = l ? lig_counts : rec_counts;
    long long v[LD_NCNT];
#pragma unroll
    for (int k = 0; k < LD_NCNT; ++k) v[k] = 0;
    for (int a = a0; a < a1; ++a) {
#pragma unroll
        for (int k = 0; k < LD_NCNT; ++k) v[k] += (long long)cnt[(size_t)a * LD_NCNT + k];
    }
    double* __restrict__ o = (l ? lig_res_lddt : rec_res_lddt) + (size_t)r * 2;
    o[0] = ld_score(v[0], v[1], v[2], v[3], v[4]);
    o[1] = ld_score(v[5], v[6], v[7], v[8], v[9]);
}

__global__ __launch_bounds__(EQD_BLOCK) void k_ld_finish(int C, const int32_t* __restrict__ lig_counts,
                                                         const int32_t* __restrict__ rec_counts, double* __restrict__ rows,
                                                         LddtWs W) {
    __shared__ long long red[2 * LD_NCNT][EQD_BLOCK];           // every thread's sums: the ligand's ten, the receptor's ten
    __shared__ long long tot[2 * LD_NCNT];
    const int c = blockIdx.x;
    if (c >= C) return;
    const LddtDesc d = W.desc[c];
    const int tid = threadIdx.x;
    for (int side = 0; side < 2; ++side) {
        const int32_t* __restrict__ cnt = side ? rec_counts + (size_t)d.ra0 * LD_NCNT : lig_counts + (size_t)d.la0 * LD_NCNT;
        const int n = side ? d.nra : d.nla;
        long long v[LD_NCNT];
#pragma unroll
        for (int k = 0; k < LD_NCNT; ++k) v[k] = 0;
        for (int a = tid; a < n; a += EQD_BLOCK) {
#pragma unroll
            for (int k = 0; k < LD_NCNT; ++k) v[k] += (long long)cnt[(size_t)a * LD_NCNT + k];
        }
#pragma unroll
        for (int k = 0; k < LD_NCNT; ++k) red[side * LD_NCNT + k][tid] = v[k];
    }
    __syncthreads();
    if (tid < 2 * LD_NCNT) {
        long long s = 0;
        for (int k = 0; k < EQD_BLOCK; ++k) s += red[tid][k];  // (integers: the order changes nothing)
        tot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const long long* L = tot;
        const long long* R = tot + LD_NCNT;
        double* __restrict__ o = rows + (size_t)c * EQD_DOCK_LDDT_COLS;
        o[0] = ld_score(L[0] + R[0], L[1] + R[1], L[2] + R[2], L[3] + R[3], L[4] + R[4]);
        o[1] = ld_score(L[5] + R[5], L[6] + R[6], L[7] + R[7], L[8] + R[8], L[9] + R[9]);
        o[2] = ld_score(L[0], L[1], L[2], L[3], L[4]);
        o[3] = ld_score(R[0], R[1], R[2], R[3], R[4]);
        o[4] = (double)(L[0] + R[0]);
        o[5] = (double)(L[5] + R[5]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[6 + k] = (double)(L[1 + k] + R[1 + k]);
            o[10 + k] = (double)(L[6 + k] + R[6 + k]);
        }
        o[14] = (double)W.skipped[c];
        o[15] = 0.0;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
static int ld_cdiv(int a, int b) { return (a + b - 1) / b; }

// validated item table of a batch (+ entry C with the totals); returns EQD_OK or an error code with the message set
static int ld_plan(const char* fn, int C, const int32_t* lao, const int32_t* rao, const int32_t* lro, const int32_t* rro,
                   std::vector<LddtDesc>& D) {
    if (!lao || !rao || !lro || !rro) {
        eqd_set_error("%s: NULL offsets", fn);
        return EQD_ERR_NULL;
    }
    if (C < 1) {
        eqd_set_error("%s: n_complex = %d (need >= 1)", fn, C);
        return EQD_ERR_SHAPE;
    }
    if (lao[0] != 0 || rao[0] != 0 || lro[0] != 0 || rro[0] != 0) {
        eqd_set_error("%s: lig_atom_off[0] = %d, rec_atom_off[0] = %d, lig_res_off[0] = %d, rec_res_off[0] = %d (need 0)", fn,
                      lao[0], rao[0], lro[0], rro[0]);
        return EQD_ERR_SHAPE;
    }
    D.assign((size_t)C + 1, LddtDesc{});
    int64_t item = 0, blk = 0;
    for (int c = 0; c < C; ++c) {
        const int64_t nla = (int64_t)lao[c + 1] - lao[c], nra = (int64_t)rao[c + 1] - rao[c];
        const int64_t nlr = (int64_t)lro[c + 1] - lro[c], nrr = (int64_t)rro[c + 1] - rro[c];
        if (nla < 1 || nra < 1) {
            eqd_set_error("%s: complex %d has %lld ligand and %lld receptor atoms (offsets must increase; every complex "
                          "needs >= 1 atom on each side)", fn, c, (long long)nla, (long long)nra);
            return EQD_ERR_SHAPE;
        }
        if (nlr < 1 || nrr < 1 || nlr > nla || nrr > nra) {
            eqd_set_error("%s: complex %d has %lld ligand residues for %lld atoms and %lld receptor residues for %lld atoms "
                          "(a residue table tiles its complex's atoms: 1 <= residues <= atoms on each side)", fn, c,
                          (long long)nlr, (long long)nla, (long long)nrr, (long long)nra);
            return EQD_ERR_SHAPE;
        }
        if (nla + nra > INT32_MAX - LD_COLS || ((int64_t)lao[c + 1] + rao[c + 1]) * LD_NCNT > INT32_MAX) {
            eqd_set_error("%s: %lld ligand and %lld receptor atoms up to complex %d do not fit 32-bit offsets (split the "
                          "batch)", fn, (long long)lao[c + 1], (long long)rao[c + 1], c);
            return EQD_ERR_SHAPE;
        }
        LddtDesc& d = D[c];
        d.la0 = lao[c]; d.nla = (int32_t)nla; d.ra0 = rao[c]; d.nra = (int32_t)nra;
        d.lr0 = lro[c]; d.nlr = (int32_t)nlr; d.rr0 = rro[c]; d.nrr = (int32_t)nrr;
        d.a0 = d.la0 + d.ra0;
        d.nbl = ld_cdiv(d.nla, LD_BLOCK);
        d.nb = d.nbl + ld_cdiv(d.nra, LD_BLOCK);
        d.nrange = ld_cdiv(d.nb, LD_STAGE);
        d.item_base = (int32_t)item;
        d.blk_base = (int32_t)blk;
        item += (int64_t)d.nb * d.nrange;
        blk += d.nb;
        if (item > INT32_MAX) {
            eqd_set_error("%s: %lld work items up to complex %d do not fit a launch (split the batch)", fn, (long long)item, c);
            return EQD_ERR_SHAPE;
        }
    }
    LddtDesc& e = D[C];
    e.la0 = lao[C]; e.ra0 = rao[C]; e.lr0 = lro[C]; e.rr0 = rro[C];
    e.a0 = e.la0 + e.ra0;
    e.item_base = (int32_t)item;
    e.blk_base = (int32_t)blk;
    return EQD_OK;
}

static size_t ld_carve(int C, const std::vector<LddtDesc>& D, EqdArena& A, LddtWs* W) {
    const LddtDesc& e = D[C];
    LddtWs w;
    w.desc = A.take<LddtDesc>((size_t)C + 1);
    w.resid = A.take<int32_t>((size_t)e.a0);
    w.blk = A.take<double>((size_t)e.blk_base * 4);
    w.skipped = A.take<int32_t>((size_t)C);
    if (W) *W = w;
    return A.off;
}

// plan + carve of a call on a workspace
static int ld_open(const char* fn, int C, const int32_t* lao, const int32_t* rao, const int32_t* lro, const int32_t* rro,
                   void* workspace, size_t ws_bytes, std::vector<LddtDesc>& D, LddtWs* W) {
    if (!workspace) {
        eqd_set_error("%s: NULL workspace", fn);
        return EQD_ERR_NULL;
    }
    if (int rc = ld_plan(fn, C, lao, rao, lro, rro, D)) return rc;
    EqdArena A(workspace, ws_bytes);
    ld_carve(C, D, A, W);
    if (!A.ok) {
        eqd_set_error("%s: workspace too small (%zu needed, %zu given)", fn, A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_lddt_abi(void) { return EQD_DOCK_LDDT_ABI; }

extern "C" EQD_DOCK_API size_t eqd_dock_lddt_workspace_bytes(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                             const int32_t* lig_res_off, const int32_t* rec_res_off) {
    std::vector<LddtDesc> D;
    if (ld_plan("eqd_dock_lddt_workspace_bytes", C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, D) != EQD_OK) return 0;
    EqdArena A(nullptr, 0);
    return ld_carve(C, D, A, nullptr) + 256;
}

extern "C" EQD_DOCK_API int eqd_dock_lddt_init(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                               const int32_t* lig_res_off, const int32_t* rec_res_off, void* workspace,
                                               size_t ws_bytes, void* stream) {
    std::vector<LddtDesc> D;
    LddtWs W;
    if (int rc = ld_open("eqd_dock_lddt_init", C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, workspace, ws_bytes, D, &W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync((void*)W.desc, D.data(), sizeof(LddtDesc) * D.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        eqd_set_error("eqd_dock_lddt_init: copy failed");
        return EQD_ERR_LAUNCH;
    }
#ifndef EQD_HOSTSIM
    if (hipStreamSynchronize(s) != hipSuccess) {      // `D` is a local host buffer
        eqd_set_error("eqd_dock_lddt_init: stream synchronisation failed");
        return EQD_ERR_LAUNCH;
    }
#endif
    return EQD_OK;
}

static bool ld_positive(double v) { return v > 0.0 && v < (double)INFINITY; }

extern "C" EQD_DOCK_API int eqd_dock_lddt_eval(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                               const int32_t* lig_res_off, const int32_t* rec_res_off, const float* lig_pred,
                                               const float* rec_pred, const float* lig_true, const float* rec_true,
                                               const int32_t* lig_res_first, const int32_t* rec_res_first,
                                               double inclusion_radius, const double* thresholds, int prune,
                                               int32_t* lig_counts, int32_t* rec_counts, double* lig_res_lddt,
                                               double* rec_res_lddt, double* rows, void* workspace, size_t ws_bytes,
                                               void* stream) {
    const char* fn = "eqd_dock_lddt_eval";
    if (!lig_pred || !lig_true || !rec_true || !lig_res_first || !rec_res_first || !thresholds || !lig_counts || !rec_counts ||
        !lig_res_lddt || !rec_res_lddt || !rows) {
        eqd_set_error("%s: NULL argument", fn);
        return EQD_ERR_NULL;
    }
    if (!ld_positive(inclusion_radius)) {
        eqd_set_error("%s: inclusion_radius = %g (need a finite value > 0)", fn, inclusion_radius);
        return EQD_ERR_SHAPE;
    }
    LddtParams P;
    for (int k = 0; k < 4; ++k) {
        if (!ld_positive(thresholds[k])) {
            eqd_set_error("%s: thresholds[%d] = %g (need a finite value > 0)", fn, k, thresholds[k]);
            return EQD_ERR_SHAPE;
        }
        P.t[k] = thresholds[k];
    }
    P.radius = inclusion_radius;
    P.bound = inclusion_radius + LD_SKIP_MARGIN;
    P.skip2 = P.bound * P.bound;
    std::vector<LddtDesc> D;
    LddtWs W;
    if (int rc = ld_open(fn, C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, workspace, ws_bytes, D, &W)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!rec_pred) rec_pred = rec_true;                         // the model's receptor is the native's
    const unsigned n_atom = (unsigned)D[C].a0, n_item = (unsigned)D[C].item_base;
    const unsigned n_res = (unsigned)D[C].lr0 + (unsigned)D[C].rr0;
    hipLaunchKernelGGL(k_ld_bounds, dim3((n_atom + EQD_BLOCK - 1) / EQD_BLOCK), dim3(EQD_BLOCK), 0, s, C, lig_true, rec_true,
                       lig_res_first, rec_res_first, lig_counts, rec_counts, W);
    if (int rc = eqd_check_launch("k_ld_bounds")) return rc;
    hipLaunchKernelGGL(k_ld_pairs, dim3(n_item), dim3(EQD_BLOCK), 0, s, C, lig_pred, rec_pred, lig_true, rec_true, P,
                       prune ? 1 : 0, lig_counts, rec_counts, W);
    if (int rc = eqd_check_launch("k_ld_pairs")) return rc;
    hipLaunchKernelGGL(k_ld_residues, dim3((n_res + EQD_BLOCK - 1) / EQD_BLOCK), dim3(EQD_BLOCK), 0, s, C, lig_res_first,
                       rec_res_first, lig_counts, rec_counts, lig_res_lddt, rec_res_lddt, W);
    if (int rc = eqd_check_launch("k_ld_residues")) return rc;
    hipLaunchKernelGGL(k_ld_finish, dim3((unsigned)C), dim3(EQD_BLOCK), 0, s, C, lig_counts, rec_counts, rows, W);
    return eqd_check_launch("k_ld_finish");
}

// Batched docking quality (include/equidock_dock.h): the CAPRI quantities and DockQ (Basu & Wallner 2016) of C docked
// complexes in one device pass, from every heavy atom of the model (lig_pred, rec_pred) and of the native (lig_true,
// rec_true), whose rows correspond one to one.
//   contact      a (ligand residue, receptor residue) pair with some atom pair closer than contact_cutoff;
//                N / M / S contacts of the native / of the model / of both; fnat = S / N, fnonnat = (M - S) / M
//   interface    a residue with some NATIVE atom pair closer than interface_cutoff to the other side
//   iRMSD(bb)    Kabsch RMSD of the model onto the native over the backbone rows of the interface residues of both sides
//   LRMSD(bb)    the Kabsch transform of rec_pred onto rec_true over the receptor's backbone rows, applied to lig_pred;
//                RMSD to lig_true over the ligand's backbone rows
//   DockQ        (fnat + 1 / (1 + (iRMSD / 1.5)^2) + 1 / (1 + (LRMSD / 8.5)^2)) / 3
//   clashes      atom pairs of the model closer than clash_cutoff
// d = sqrt((dx dx + dy dy) + dz dz) in fp64 from the fp32 inputs, compared as d < cutoff; -ffp-contract=off.
//
// Work decomposition.  Six launches, whatever C is:
//   k_dq_bounds     one thread per (side, pose, residue): the fp64 centroid of its atoms and the radius around it; the
//                   native ligand / receptor threads also zero the residue's interface mark and write the residue of
//                   every atom
//   k_dq_pairs      items (complex, tile of DQ_TILE ligand residues, chunk of DQ_CHUNK receptor residues): the chunk's
//                   receptor atoms of both poses staged in LDS; one thread per (residue pair, pose) tests the bound -
//                   skipped when (centroid distance - radius - radius) >= largest cutoff + 1e-6, which no atom pair of
//                   the two residues can undercut - and puts the survivors on a list in LDS that the workgroup then
//                   walks with all lanes, one residue pair of one pose per thread and step -> the item's own slot of
//                   integer counts (N, M, S, clashes, pruned) and integer adds to the interface marks
//   k_dq_moments    items (complex, tile of 256 rows of the concatenated ligand + receptor atoms): the weighted moments of
//                   the interface backbone set and of the receptor backbone set, the ligand's backbone rows and the
//                   interface residues of each side -> 35 doubles in the item's own slot, relative to the complex's
//                   first lig_true row
//   k_dq_solve      one thread per (complex, set): the slots in tile order, dm_kabsch (eqd_dock_kabsch.h)
//   k_dq_residuals  items as in k_dq_moments: sum w |R p + b - t|^2 of the interface set under its own transform and of
//                   the ligand's backbone rows under the receptor set's (an explicit second pass)
//   k_dq_finish     one wave per complex: the integer slots (any order), the double slots in tile order -> quality[c][16]
// The item tables depend only on each complex's own sizes, every floating-point partial has its own slot and the slots
// are combined in item order; the only atomics are integer adds (a slot number on an item's list, the interface marks),
// whose result does not depend on their order: a complex's row is bit-identical alone, in any batch, at any position and
// from run to run.
#include "../csrc/eqd_common.h"
#include "../../include/equidock_dock.h"
#include "eqd_dock_kabsch.h"

#include <math.h>
#include <vector>

#define DQ_TILE 8           // ligand residues per pairs item
#define DQ_CHUNK 32         // receptor residues per pairs item (DQ_TILE * DQ_CHUNK = EQD_BLOCK residue pairs)
#define DQ_STAGE 512        // receptor atoms of a chunk kept in LDS per pose; atoms beyond are read from global memory
#define DQ_ROWS EQD_BLOCK   // rows per moments / residuals item
#define DQ_NMOM 35          // 2 x (1 + 3 + 3 + 9), ligand backbone rows, interface residues of the ligand / the receptor
#define DQ_NCNT 5           // N, M, S, clashes, pruned (residue pair, pose) tests
#define DQ_PRUNE_MARGIN 1e-6

static_assert(DQ_TILE * DQ_CHUNK == EQD_BLOCK, "one residue pair per thread");

struct QualDesc {           // one complex of the batch (entry C: the totals)
    int32_t la0, nla, ra0, nra;     // atom rows
    int32_t lr0, nlr, rr0, nrr;     // residues
    int32_t ntile, nchunk;          // pairs items: ntile x nchunk
    int32_t pair_base;              // first k_dq_pairs item
    int32_t mom_base, nt;           // first k_dq_moments / k_dq_residuals item, tiles of the concatenated rows
    int32_t pad[3];
};

struct QualWs {
    const QualDesc* desc;   // [C + 1]
    double* bl;             // [2][R_l][4] centroid and radius of every ligand residue, native then model
    double* br;             // [2][R_r][4]
    int32_t* ml;            // [R_l] interface marks: partner residues under the interface cutoff
    int32_t* mr;            // [R_r]
    int32_t* rl;            // [A_l] residue (global) of every ligand atom
    int32_t* rr;            // [A_r]
    int32_t* cnt;           // [pair items][DQ_NCNT]
    double* mom;            // [moment items][DQ_NMOM]
    double* rb;             // [C][2][DM_NRB]
    double* res;            // [moment items][2]
    int32_t* flags;         // [C][2]
};

// the complex that owns item / residue `v`: the largest c with base(c) <= v (kind 0 pairs items, 1 moments items, 2 ligand
// residues, 3 receptor residues; the bases are strictly increasing)
template <int kKind>
__device__ __forceinline__ int dq_find(const QualDesc* __restrict__ D, int C, int v) {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int b = kKind == 0 ? D[mid].pair_base : kKind == 1 ? D[mid].mom_base : kKind == 2 ? D[mid].lr0 : D[mid].rr0;
        if (b <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// atom rows [a0, a1) of residue g, held inside its complex's rows [lo, hi) whatever the table says
__device__ __forceinline__ void dq_range(const int32_t* __restrict__ first, int g, int lo, int hi, int& a0, int& a1) {
    a0 = first[g];
    a1 = first[g + 1];
    a0 = a0 < lo ? lo : (a0 > hi ? hi : a0);
    a1 = a1 < a0 ? a0 : (a1 > hi ? hi : a1);
}

__device__ __forceinline__ int dq_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(EQD_BLOCK) void k_dq_bounds(int C, const float* __restrict__ lig_true,
                                                         const float* __restrict__ lig_pred,
                                                         const float* __restrict__ rec_true,
                                                         const float* __restrict__ rec_pred,
                                                         const int32_t* __restrict__ lfirst,
                                                         const int32_t* __restrict__ rfirst, QualWs W) {
    const int Rl = W.desc[C].lr0, Rr = W.desc[C].rr0;
    int g = blockIdx.x * EQD_BLOCK + threadIdx.x;
    if (g >= 2 * (Rl + Rr)) return;
    const bool lig = g < 2 * Rl;
    if (!lig) g -= 2 * Rl;
    const int R = lig ? Rl : Rr;
    const int pose = g >= R ? 1 : 0;
    if (pose) g -= R;
    const int c = lig ? dq_find<2>(W.desc, C, g) : dq_find<3>(W.desc, C, g);
    const QualDesc d = W.desc[c];
    int a0, a1;
    if (lig) dq_range(lfirst, g, d.la0, d.la0 + d.nla, a0, a1);
    else dq_range(rfirst, g, d.ra0, d.ra0 + d.nra, a0, a1);
    const float* __restrict__ x = lig ? (pose ? lig_pred : lig_true) : (pose ? rec_pred : rec_true);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int a = a0; a < a1; ++a) {
        sx += (double)x[(size_t)a * 3];
        sy += (double)x[(size_t)a * 3 + 1];
        sz += (double)x[(size_t)a * 3 + 2];
    }
    const double na = (double)(a1 - a0);
    const double cx = sx / na, cy = sy / na, cz = sz / na;
    double rad = 0.0;
    for (int a = a0; a < a1; ++a) {
        const double dx = (double)x[(size_t)a * 3] - cx, dy = (double)x[(size_t)a * 3 + 1] - cy, dz = (double)x[(size_t)a * 3 + 2] - cz;
        const double r = sqrt((dx * dx + dy * dy) + dz * dz);
        rad = r > rad ? r : rad;
    }
    double* __restrict__ o = (lig ? W.bl : W.br) + ((size_t)pose * R + g) * 4;
    o[0] = cx;
    o[1] = cy;
    o[2] = cz;
    o[3] = rad;
    if (!pose) {
        (lig ? W.ml : W.mr)[g] = 0;
        int32_t* __restrict__ ro = lig ? W.rl : W.rr;
        for (int a = a0; a < a1; ++a) ro[a] = g;
    }
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dq_pairs(int C, const float* __restrict__ lig_true,
                                                        const float* __restrict__ lig_pred,
                                                        const float* __restrict__ rec_true,
                                                        const float* __restrict__ rec_pred,
                                                        const int32_t* __restrict__ lfirst,
                                                        const int32_t* __restrict__ rfirst, double contact_cut,
                                                        double iface_cut, double clash_cut, int prune, double prune_at,
                                                        QualWs W) {
    __shared__ float st[2][DQ_STAGE][3];                    // the chunk's receptor atoms: native, model
    __shared__ int32_t todo[2 * EQD_BLOCK];                 // (pose << 16) | residue pair of the item
    __shared__ int32_t n_todo;
    __shared__ int32_t cn[EQD_BLOCK], cm[EQD_BLOCK];        // the pair is a contact of the native / of the model
    __shared__ int32_t lmark[DQ_TILE], rmark[DQ_CHUNK];
    __shared__ int32_t red[EQD_WAVES][DQ_NCNT];
    const int item = blockIdx.x;
    if (item >= W.desc[C].pair_base) return;
    const int c = dq_find<0>(W.desc, C, item);
    const QualDesc d = W.desc[c];
    const int q = item - d.pair_base;
    const int tile = q / d.nchunk, chunk = q - tile * d.nchunk;
    const int i0 = tile * DQ_TILE, j0 = chunk * DQ_CHUNK;
    const int nj = d.nrr - j0 < DQ_CHUNK ? d.nrr - j0 : DQ_CHUNK;
    const int tid = threadIdx.x;
    const int32_t* __restrict__ lf = lfirst + d.lr0;
    const int32_t* __restrict__ rf = rfirst + d.rr0;
    const int llo = d.la0, lhi = d.la0 + d.nla, rlo = d.ra0, rhi = d.ra0 + d.nra;
    int s0, s1, e0, e1;
    dq_range(rf, j0, rlo, rhi, s0, s1);
    dq_range(rf, j0 + nj - 1, rlo, rhi, e0, e1);
    const int rb0 = s0;                                      // first atom row of the chunk
    const int ns = e1 - rb0 < DQ_STAGE ? (e1 - rb0 > 0 ? e1 - rb0 : 0) : DQ_STAGE;
    if (tid == 0) n_todo = 0;
    if (tid < DQ_TILE) lmark[tid] = 0;
    if (tid < DQ_CHUNK) rmark[tid] = 0;
    cn[tid] = 0;
    cm[tid] = 0;
    for (int k = tid; k < 3 * ns; k += EQD_BLOCK) {
        st[0][k / 3][k % 3] = rec_true[(size_t)rb0 * 3 + k];
        st[1][k / 3][k % 3] = rec_pred[(size_t)rb0 * 3 + k];
    }
    __syncthreads();
    const int r = tid / DQ_CHUNK, jj = tid - r * DQ_CHUNK;
    int cut = 0;
    if (i0 + r < d.nlr && jj < nj) {
#pragma unroll
        for (int pose = 0; pose < 2; ++pose) {
            const double* __restrict__ a = W.bl + ((size_t)pose * W.desc[C].lr0 + d.lr0 + i0 + r) * 4;
            const double* __restrict__ b = W.br + ((size_t)pose * W.desc[C].rr0 + d.rr0 + j0 + jj) * 4;
            const double ex = a[0] - b[0], ey = a[1] - b[1], ez = a[2] - b[2];
            if (prune && (sqrt((ex * ex + ey * ey) + ez * ez) - a[3]) - b[3] >= prune_at) ++cut;
            else todo[atomicAdd(&n_todo, 1)] = (pose << 16) | tid;      // (an integer slot counter: order is free)
        }
    }
    __syncthreads();
    const int nt = n_todo;
    int clashes = 0;
    for (int t = tid; t < nt; t += EQD_BLOCK) {
        const int pose = todo[t] >> 16, pr = todo[t] & 0xffff;
        const int pi = pr / DQ_CHUNK, pj = pr - pi * DQ_CHUNK;
        int a0, a1, b0, b1;
        dq_range(lf, i0 + pi, llo, lhi, a0, a1);
        dq_range(rf, j0 + pj, rlo, rhi, b0, b1);
        const float* __restrict__ L = pose ? lig_pred : lig_true;
        const float* __restrict__ G = pose ? rec_pred : rec_true;
        int contact = 0, iface = 0, clash = 0;
        for (int a = a0; a < a1; ++a) {
            const double ax = (double)L[(size_t)a * 3], ay = (double)L[(size_t)a * 3 + 1], az = (double)L[(size_t)a * 3 + 2];
            for (int b = b0; b < b1; ++b) {
                const int rel = b - rb0;
                const bool in_lds = (unsigned)rel < (unsigned)ns;
                const double bx = in_lds ? (double)st[pose][rel][0] : (double)G[(size_t)b * 3];
                const double by = in_lds ? (double)st[pose][rel][1] : (double)G[(size_t)b * 3 + 1];
                const double bz = in_lds ? (double)st[pose][rel][2] : (double)G[(size_t)b * 3 + 2];
                const double dx = ax - bx, dy = ay - by, dz = az - bz;
                const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                contact |= dist < contact_cut ? 1 : 0;
                iface |= dist < iface_cut ? 1 : 0;
                clash += dist < clash_cut ? 1 : 0;
            }
        }
        if (pose) {
            cm[pr] = contact;
            clashes += clash;
        } else {
            cn[pr] = contact;
            if (iface) {
                atomicAdd(&lmark[pi], 1);
                atomicAdd(&rmark[pj], 1);
            }
        }
    }
    __syncthreads();
    int v[DQ_NCNT] = {cn[tid], cm[tid], cn[tid] & cm[tid], clashes, cut};
#pragma unroll
    for (int k = 0; k < DQ_NCNT; ++k) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v[k] += __shfl_xor(v[k], m);
        if ((tid & 63) == 0) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < DQ_NCNT) W.cnt[(size_t)item * DQ_NCNT + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    if (tid < DQ_TILE && i0 + tid < d.nlr && lmark[tid]) atomicAdd(W.ml + d.lr0 + i0 + tid, lmark[tid]);
    if (tid >= 64 && tid < 64 + nj && rmark[tid - 64]) atomicAdd(W.mr + d.rr0 + j0 + (tid - 64), rmark[tid - 64]);
}

// row g of complex d's concatenated atoms, relative to the complex's first lig_true row
struct DqRow {
    double p[3], t[3];
    double w_if, w_rec, w_lig;      // 1 or 0: interface backbone row, receptor backbone row, ligand backbone row
    double first_l, first_r;        // 1 or 0: the first atom of an interface residue of the ligand / of the receptor
};
__device__ __forceinline__ DqRow dq_row(const QualDesc& d, int g, const float* __restrict__ lig_pred,
                                        const float* __restrict__ rec_pred, const float* __restrict__ lig_true,
                                        const float* __restrict__ rec_true, const int32_t* __restrict__ lfirst,
                                        const int32_t* __restrict__ rfirst, const uint8_t* __restrict__ lig_bb,
                                        const uint8_t* __restrict__ rec_bb, const QualWs& W) {
    DqRow r;
    const float* __restrict__ o = lig_true + (size_t)d.la0 * 3;
    const bool lig = g < d.nla;
    const int row = lig ? d.la0 + g : d.ra0 + (g - d.nla);
    const float* __restrict__ p = (lig ? lig_pred : rec_pred) + (size_t)row * 3;
    const float* __restrict__ t = (lig ? lig_true : rec_true) + (size_t)row * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.p[a] = (double)p[a] - (double)o[a];
        r.t[a] = (double)t[a] - (double)o[a];
    }
    const int res = lig ? dq_clamp(W.rl[row], d.lr0, d.lr0 + d.nlr - 1) : dq_clamp(W.rr[row], d.rr0, d.rr0 + d.nrr - 1);
    const bool marked = (lig ? W.ml : W.mr)[res] > 0;
    const bool bb = (lig ? lig_bb : rec_bb)[row] != 0;
    const bool first = (lig ? lfirst : rfirst)[res] == row;
    r.w_if = marked && bb ? 1.0 : 0.0;
    r.w_rec = !lig && bb ? 1.0 : 0.0;
    r.w_lig = lig && bb ? 1.0 : 0.0;
    r.first_l = lig && marked && first ? 1.0 : 0.0;
    r.first_r = !lig && marked && first ? 1.0 : 0.0;
    return r;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dq_moments(int C, const float* __restrict__ lig_pred,
                                                          const float* __restrict__ rec_pred,
                                                          const float* __restrict__ lig_true,
                                                          const float* __restrict__ rec_true,
                                                          const int32_t* __restrict__ lfirst,
                                                          const int32_t* __restrict__ rfirst,
                                                          const uint8_t* __restrict__ lig_bb,
                                                          const uint8_t* __restrict__ rec_bb, QualWs W) {
    __shared__ double red[EQD_WAVES];
    const int item = blockIdx.x;
    if (item >= W.desc[C].mom_base) return;
    const int c = dq_find<1>(W.desc, C, item);
    const QualDesc d = W.desc[c];
    const int n = d.nla + d.nra;
    const int g = (item - d.mom_base) * DQ_ROWS + threadIdx.x;
    const bool valid = g < n;
    const DqRow r = dq_row(d, valid ? g : n - 1, lig_pred, rec_pred, lig_true, rec_true, lfirst, rfirst, lig_bb, rec_bb, W);
    double v[DQ_NMOM];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double w = !valid ? 0.0 : (s == 0 ? r.w_if : r.w_rec);
        double* o = v + 16 * s;
        o[0] = w;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wp = w * r.p[a];
            o[1 + a] = wp;
            o[4 + a] = w * r.t[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) o[7 + 3 * a + b] = wp * r.t[b];
        }
    }
    v[32] = valid ? r.w_lig : 0.0;
    v[33] = valid ? r.first_l : 0.0;
    v[34] = valid ? r.first_r : 0.0;
    double* __restrict__ slot = W.mom + (size_t)item * DQ_NMOM;
#pragma unroll
    for (int k = 0; k < DQ_NMOM; ++k) {
        const double tot = dm_block_sum(v[k], red);
        if (threadIdx.x == 0) slot[k] = tot;
    }
}

__global__ __launch_bounds__(64) void k_dq_solve(int C, QualWs W) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    const int c = idx >> 1, set = idx & 1;
    if (c >= C) return;
    const QualDesc d = W.desc[c];
    double m[16];
    for (int k = 0; k < 16; ++k) m[k] = 0.0;
    for (int t = 0; t < d.nt; ++t) {
        const double* __restrict__ slot = W.mom + (size_t)(d.mom_base + t) * DQ_NMOM + 16 * set;
        for (int k = 0; k < 16; ++k) m[k] += slot[k];
    }
    const bool reflect = dm_kabsch(m, W.rb + ((size_t)c * 2 + set) * DM_NRB);
    W.flags[2 * c + set] = reflect ? 1 : 0;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dq_residuals(int C, const float* __restrict__ lig_pred,
                                                            const float* __restrict__ rec_pred,
                                                            const float* __restrict__ lig_true,
                                                            const float* __restrict__ rec_true,
                                                            const int32_t* __restrict__ lfirst,
                                                            const int32_t* __restrict__ rfirst,
                                                            const uint8_t* __restrict__ lig_bb,
                                                            const uint8_t* __restrict__ rec_bb, QualWs W) {
    __shared__ double red[EQD_WAVES];
    const int item = blockIdx.x;
    if (item >= W.desc[C].mom_base) return;
    const int c = dq_find<1>(W.desc, C, item);
    const QualDesc d = W.desc[c];
    const int n = d.nla + d.nra;
    const int g = (item - d.mom_base) * DQ_ROWS + threadIdx.x;
    const bool valid = g < n;
    const DqRow r = dq_row(d, valid ? g : n - 1, lig_pred, rec_pred, lig_true, rec_true, lfirst, rfirst, lig_bb, rec_bb, W);
    double v[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double* __restrict__ rb = W.rb + ((size_t)c * 2 + s) * DM_NRB;
        double e2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double q = ((rb[3 * a] * r.p[0] + rb[3 * a + 1] * r.p[1]) + rb[3 * a + 2] * r.p[2]) + rb[9 + a] - r.t[a];
            e2 += q * q;
        }
        const double w = !valid ? 0.0 : (s == 0 ? r.w_if : r.w_lig);
        v[s] = w * e2;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double tot = dm_block_sum(v[s], red);
        if (threadIdx.x == 0) W.res[(size_t)item * 2 + s] = tot;
    }
}

__global__ __launch_bounds__(64) void k_dq_finish(int C, double* __restrict__ quality, QualWs W) {
    const int c = blockIdx.x;
    if (c >= C) return;
    const QualDesc d = W.desc[c];
    const int lane = threadIdx.x;
    int v[DQ_NCNT] = {0, 0, 0, 0, 0};
    const int nitem = d.ntile * d.nchunk;
    for (int t = lane; t < nitem; t += 64) {
        const int32_t* __restrict__ s = W.cnt + (size_t)(d.pair_base + t) * DQ_NCNT;
#pragma unroll
        for (int k = 0; k < DQ_NCNT; ++k) v[k] += s[k];
    }
#pragma unroll
    for (int k = 0; k < DQ_NCNT; ++k) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v[k] += __shfl_xor(v[k], m);      // (integers: the order changes nothing)
    }
    if (lane != 0) return;
    double w_if = 0.0, w_rec = 0.0, w_lig = 0.0, n_il = 0.0, n_ir = 0.0, e_if = 0.0, e_lig = 0.0;
    for (int t = 0; t < d.nt; ++t) {
        const double* __restrict__ slot = W.mom + (size_t)(d.mom_base + t) * DQ_NMOM;
        w_if += slot[0];
        w_rec += slot[16];
        w_lig += slot[32];
        n_il += slot[33];
        n_ir += slot[34];
        e_if += W.res[(size_t)(d.mom_base + t) * 2];
        e_lig += W.res[(size_t)(d.mom_base + t) * 2 + 1];
    }
    const double nan = __builtin_nan("");
    const double N = (double)v[0], M = (double)v[1], S = (double)v[2];
    const double fnat = v[0] > 0 ? S / N : nan;
    const double fnonnat = v[1] > 0 ? (M - S) / M : 0.0;
    const bool have_if = w_if > 0.0, have_l = w_rec > 0.0 && w_lig > 0.0;
    const double irmsd = have_if ? sqrt(e_if / w_if) : nan;
    const double lrmsd = have_l ? sqrt(e_lig / w_lig) : nan;
    const double qi = irmsd / 1.5, ql = lrmsd / 8.5;
    const int32_t* __restrict__ fb = W.flags + 2 * (size_t)c;
    double* __restrict__ o = quality + (size_t)c * EQD_DOCK_QUALITY_COLS;
    o[0] = ((fnat + 1.0 / (1.0 + qi * qi)) + 1.0 / (1.0 + ql * ql)) / 3.0;      // NaN when a term is
    o[1] = fnat;
    o[2] = fnonnat;
    o[3] = irmsd;
    o[4] = lrmsd;
    o[5] = N;
    o[6] = M;
    o[7] = S;
    o[8] = n_il;
    o[9] = n_ir;
    o[10] = w_if;
    o[11] = (double)v[3];
    o[12] = (double)((have_if && fb[0] ? 1 : 0) | (have_l && fb[1] ? 2 : 0));
    o[13] = (double)v[4];
    o[14] = 0.0;
    o[15] = 0.0;
}

// ---- host side ------------------------------------------------------------------------------------------------
static int dq_cdiv(int a, int b) { return (a + b - 1) / b; }

// validated item table of a batch (+ entry C with the totals); returns EQD_OK or an error code with the message set
static int dq_plan(const char* fn, int C, const int32_t* lao, const int32_t* rao, const int32_t* lro, const int32_t* rro,
                   std::vector<QualDesc>& D) {
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
    D.assign((size_t)C + 1, QualDesc{});
    int64_t pair = 0, mom = 0;
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
        if (nla + nra > INT32_MAX - DQ_ROWS || ((int64_t)lao[c + 1] + rao[c + 1]) * 3 > INT32_MAX) {
            eqd_set_error("%s: %lld ligand and %lld receptor atoms up to complex %d do not fit 32-bit offsets (split the "
                          "batch)", fn, (long long)lao[c + 1], (long long)rao[c + 1], c);
            return EQD_ERR_SHAPE;
        }
        QualDesc& d = D[c];
        d.la0 = lao[c]; d.nla = (int32_t)nla; d.ra0 = rao[c]; d.nra = (int32_t)nra;
        d.lr0 = lro[c]; d.nlr = (int32_t)nlr; d.rr0 = rro[c]; d.nrr = (int32_t)nrr;
        d.ntile = dq_cdiv(d.nlr, DQ_TILE); d.nchunk = dq_cdiv(d.nrr, DQ_CHUNK);
        d.nt = dq_cdiv(d.nla + d.nra, DQ_ROWS);
        d.pair_base = (int32_t)pair; d.mom_base = (int32_t)mom;
        pair += (int64_t)d.ntile * d.nchunk;
        mom += d.nt;
        if (pair * DQ_NCNT > INT32_MAX) {
            eqd_set_error("%s: %lld residue-pair items up to complex %d do not fit 32-bit offsets (split the batch)", fn,
                          (long long)pair, c);
            return EQD_ERR_SHAPE;
        }
    }
    QualDesc& e = D[C];
    e.la0 = lao[C]; e.ra0 = rao[C]; e.lr0 = lro[C]; e.rr0 = rro[C];
    e.pair_base = (int32_t)pair; e.mom_base = (int32_t)mom;
    return EQD_OK;
}

static size_t dq_carve(int C, const std::vector<QualDesc>& D, EqdArena& A, QualWs* W) {
    const QualDesc& e = D[C];
    QualWs w;
    w.desc = A.take<QualDesc>((size_t)C + 1);
    w.bl = A.take<double>((size_t)e.lr0 * 8);
    w.br = A.take<double>((size_t)e.rr0 * 8);
    w.ml = A.take<int32_t>((size_t)e.lr0);
    w.mr = A.take<int32_t>((size_t)e.rr0);
    w.rl = A.take<int32_t>((size_t)e.la0);
    w.rr = A.take<int32_t>((size_t)e.ra0);
    w.cnt = A.take<int32_t>((size_t)e.pair_base * DQ_NCNT);
    w.mom = A.take<double>((size_t)e.mom_base * DQ_NMOM);
    w.rb = A.take<double>((size_t)C * 2 * DM_NRB);
    w.res = A.take<double>((size_t)e.mom_base * 2);
    w.flags = A.take<int32_t>((size_t)C * 2);
    if (W) *W = w;
    return A.off;
}

// plan + carve of a call on a workspace
static int dq_open(const char* fn, int C, const int32_t* lao, const int32_t* rao, const int32_t* lro, const int32_t* rro,
                   void* workspace, size_t ws_bytes, std::vector<QualDesc>& D, QualWs* W) {
    if (!workspace) {
        eqd_set_error("%s: NULL workspace", fn);
        return EQD_ERR_NULL;
    }
    if (int rc = dq_plan(fn, C, lao, rao, lro, rro, D)) return rc;
    EqdArena A(workspace, ws_bytes);
    dq_carve(C, D, A, W);
    if (!A.ok) {
        eqd_set_error("%s: workspace too small (%zu needed, %zu given)", fn, A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_quality_abi(void) { return EQD_DOCK_QUALITY_ABI; }

extern "C" EQD_DOCK_API size_t eqd_dock_quality_workspace_bytes(int C, const int32_t* lig_atom_off,
                                                                const int32_t* rec_atom_off, const int32_t* lig_res_off,
                                                                const int32_t* rec_res_off) {
    std::vector<QualDesc> D;
    if (dq_plan("eqd_dock_quality_workspace_bytes", C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, D) != EQD_OK) return 0;
    EqdArena A(nullptr, 0);
    return dq_carve(C, D, A, nullptr) + 256;
}

extern "C" EQD_DOCK_API int eqd_dock_quality_init(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                  const int32_t* lig_res_off, const int32_t* rec_res_off, void* workspace,
                                                  size_t ws_bytes, void* stream) {
    std::vector<QualDesc> D;
    QualWs W;
    if (int rc = dq_open("eqd_dock_quality_init", C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, workspace, ws_bytes, D, &W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync((void*)W.desc, D.data(), sizeof(QualDesc) * D.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        eqd_set_error("eqd_dock_quality_init: copy failed");
        return EQD_ERR_LAUNCH;
    }
#ifndef EQD_HOSTSIM
    if (hipStreamSynchronize(s) != hipSuccess) {      // `D` is a local host buffer
        eqd_set_error("eqd_dock_quality_init: stream synchronisation failed");
        return EQD_ERR_LAUNCH;
    }
#endif
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_quality_eval(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                  const int32_t* lig_res_off, const int32_t* rec_res_off,
                                                  const float* lig_pred, const float* rec_pred, const float* lig_true,
                                                  const float* rec_true, const int32_t* lig_res_first,
                                                  const int32_t* rec_res_first, const uint8_t* lig_backbone,
                                                  const uint8_t* rec_backbone, double contact_cutoff,
                                                  double interface_cutoff, double clash_cutoff, int prune, double* quality,
                                                  void* workspace, size_t ws_bytes, void* stream) {
    const char* fn = "eqd_dock_quality_eval";
    if (!lig_pred || !lig_true || !rec_true || !lig_res_first || !rec_res_first || !lig_backbone || !rec_backbone || !quality) {
        eqd_set_error("%s: NULL argument", fn);
        return EQD_ERR_NULL;
    }
    const double cuts[3] = {contact_cutoff, interface_cutoff, clash_cutoff};
    const char* names[3] = {"contact_cutoff", "interface_cutoff", "clash_cutoff"};
    double cmax = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!(cuts[k] > 0.0) || !(cuts[k] < (double)INFINITY)) {
            eqd_set_error("%s: %s = %g (need a finite value > 0)", fn, names[k], cuts[k]);
            return EQD_ERR_SHAPE;
        }
        cmax = cuts[k] > cmax ? cuts[k] : cmax;
    }
    std::vector<QualDesc> D;
    QualWs W;
    if (int rc = dq_open(fn, C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, workspace, ws_bytes, D, &W)) return rc;
    if (!rec_pred) rec_pred = rec_true;
    hipStream_t s = (hipStream_t)stream;
    const unsigned n_res = 2u * ((unsigned)D[C].lr0 + (unsigned)D[C].rr0);
    const unsigned n_pair = (unsigned)D[C].pair_base, n_mom = (unsigned)D[C].mom_base;
    hipLaunchKernelGGL(k_dq_bounds, dim3((n_res + EQD_BLOCK - 1) / EQD_BLOCK), dim3(EQD_BLOCK), 0, s, C, lig_true, lig_pred,
                       rec_true, rec_pred, lig_res_first, rec_res_first, W);
    if (int rc = eqd_check_launch("k_dq_bounds")) return rc;
    hipLaunchKernelGGL(k_dq_pairs, dim3(n_pair), dim3(EQD_BLOCK), 0, s, C, lig_true, lig_pred, rec_true, rec_pred,
                       lig_res_first, rec_res_first, contact_cutoff, interface_cutoff, clash_cutoff, prune ? 1 : 0,
                       cmax + DQ_PRUNE_MARGIN, W);
    if (int rc = eqd_check_launch("k_dq_pairs")) return rc;
    hipLaunchKernelGGL(k_dq_moments, dim3(n_mom), dim3(EQD_BLOCK), 0, s, C, lig_pred, rec_pred, lig_true, rec_true,
                       lig_res_first, rec_res_first, lig_backbone, rec_backbone, W);
    if (int rc = eqd_check_launch("k_dq_moments")) return rc;
    hipLaunchKernelGGL(k_dq_solve, dim3((unsigned)dq_cdiv(2 * C, 64)), dim3(64), 0, s, C, W);
    if (int rc = eqd_check_launch("k_dq_solve")) return rc;
    hipLaunchKernelGGL(k_dq_residuals, dim3(n_mom), dim3(EQD_BLOCK), 0, s, C, lig_pred, rec_pred, lig_true, rec_true,
                       lig_res_first, rec_res_first, lig_backbone, rec_backbone, W);
    if (int rc = eqd_check_launch("k_dq_residuals")) return rc;
    hipLaunchKernelGGL(k_dq_finish, dim3((unsigned)C), dim3(64), 0, s, C, quality, W);
    return eqd_check_launch("k_dq_finish");
}

// Batched graph construction (include/equidock_dock.h): compute_dig_kNN_graph of the reference
// (src/utils/protein_utils.py:311-397) for the 2C proteins of C complexes in one device pass.  The arithmetic of the
// single-protein kernels k_pg_distances / k_pg_select / k_pg_edges (csrc/eqd_data_kernels.hip) is restated here
// expression for expression - fp64, the same operation order, -ffp-contract=off - so that a protein's outputs are
// bit-identical to the per-protein path.
//
// Work decomposition.  One launch per phase, whatever the number of proteins:
//   k_dg_centroids  one thread per residue: the fp64 centroid of its atoms (the pruning bound)
//   k_dg_distances  items (protein, tile of DG_ROWS residues i, chunk of EQD_BLOCK partner residues j): the tile's atoms
//                   staged in LDS, the item's unpruned pairs i < j listed in LDS and shared out evenly over the threads,
//                   D[i][j] = D[j][i], +inf on the diagonal and on pruned pairs
//   k_dg_select     items (protein, EQD_WAVES residues), one wave per residue: neighbour selection and mu_r_norm
//   k_dg_scan       one workgroup: exclusive scan of the degrees -> per-residue and per-protein edge offsets, and per
//                   protein the first residue without a neighbour
//   k_dg_edges      one thread per (residue, neighbour slot): src / dst (local to the protein) and the 27 edge features
// The item tables depend only on each protein's own size, every value is computed by one thread from its own inputs in
// a fixed order, and the only atomics are integer counters (the pruned pairs; a slot number on an item's pair list, where
// the order changes nothing): a protein's bits do not depend on the batch.
//
// Exact pruning.  The mean all-atom distance of two residues is never below the distance of their atom centroids
// (triangle inequality), and entries >= cutoff never enter the graph (the count test and the `< cutoff` filter drop
// them; when more than K qualify the K smallest are all below the cutoff).  A pair whose fp64 centroid distance is at
// least cutoff + 1e-6 is therefore not evaluated and counts as +inf.
#include "../csrc/eqd_common.h"
#include "../../include/equidock_dock.h"

#include <vector>

// residues i per distance item.  Measured on the 1 270-residue fixture protein with / without pruning (DESIGN.md
// section 8): 1 row 194 / 176 us, 2 rows 120 / 186, 4 rows 129 / 221, 8 rows 151 / 271 - more rows give the pair list more
// to share out, fewer rows more workgroups in flight
#define DG_ROWS 2
#define DG_MAXATOMS 64       // atoms of a residue kept in LDS; longer residues are read from global memory
#define DG_PRUNE_MARGIN 1e-6

struct GraphDesc {           // one protein of the batch (entry P: the totals)
    int32_t r0, n;           // first residue (global), residues
    int32_t ntile, nchunk;   // distance items: ntile x nchunk
    int32_t dist_base;       // first k_dg_distances item
    int32_t sel_base;        // first k_dg_select item (ceil(n / EQD_WAVES))
    int64_t d_base;          // D [n][n] of this protein inside the workspace
};

struct GraphWs {
    const GraphDesc* desc;   // [P + 1]
    double* cen;             // [R][3] atom centroids
    double* D;               // sum n^2
    int32_t* nbr;            // [R][K] neighbours, local to the protein
    double* nbd;             // [R][K] their distances
    int32_t* reoff;          // [R + 1] first edge of every residue
    int32_t* rprot;          // [R] protein of every residue
};

// the protein that owns `item` (largest p with base(p) <= item; the bases are strictly increasing, entry P = total)
template <int kSel>
__device__ __forceinline__ int dg_find(const GraphDesc* __restrict__ D, int P, int item) {
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int b = kSel ? D[mid].sel_base : D[mid].dist_base;
        if (b <= item) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ double dg_shfl_xor_d(double v, int m) {
    long long b = __builtin_bit_cast(long long, v);
    int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
    lo = __shfl_xor(lo, m);
    hi = __shfl_xor(hi, m);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned long long)(unsigned)lo);
}
// lanes with p set, as a 64-bit mask (built from shuffles so that the x86 simulator runs the same code)
__device__ __forceinline__ unsigned long long dg_ballot(bool p) {
    const int lane = threadIdx.x & 63;
    int mine_lo = (p && lane < 32) ? (1 << lane) : 0, mine_hi = (p && lane >= 32) ? (1 << (lane - 32)) : 0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        mine_lo |= __shfl_xor(mine_lo, m);
        mine_hi |= __shfl_xor(mine_hi, m);
    }
    return ((unsigned long long)(unsigned)mine_hi << 32) | (unsigned)mine_lo;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dg_centroids(int R, const float* __restrict__ atoms,
                                                            const int32_t* __restrict__ atom_off,
                                                            double* __restrict__ cen, int32_t* __restrict__ n_pruned) {
    const int g = blockIdx.x * EQD_BLOCK + threadIdx.x;
    if (g == 0) *n_pruned = 0;
    if (g >= R) return;
    const int a0 = atom_off[g], a1 = atom_off[g + 1];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int a = a0; a < a1; ++a) {
        sx += (double)atoms[(size_t)a * 3];
        sy += (double)atoms[(size_t)a * 3 + 1];
        sz += (double)atoms[(size_t)a * 3 + 2];
    }
    const double na = (double)(a1 - a0);
    cen[(size_t)g * 3] = sx / na;
    cen[(size_t)g * 3 + 1] = sy / na;
    cen[(size_t)g * 3 + 2] = sz / na;
}

// D[i][j] = mean over atoms a of residue i, b of residue j of |a - b| (:322-329), for i < j, mirrored.  Two steps per
// item: every thread tests the pairs (tile row, its partner j) - pruned ones get +inf at once, the others go on a list
// in LDS - and then the workgroup walks the list 256 pairs at a time, so that lanes whose pairs were pruned or lie below
// the diagonal take over pairs of other lanes.  Which thread evaluates a pair changes nothing in its value.
__global__ __launch_bounds__(EQD_BLOCK) void k_dg_distances(int P, const float* __restrict__ atoms,
                                                            const int32_t* __restrict__ atom_off, int prune,
                                                            double prune_at, GraphWs W, int32_t* __restrict__ n_pruned) {
    __shared__ float ai[DG_ROWS][DG_MAXATOMS][3];
    __shared__ int32_t todo[DG_ROWS * EQD_BLOCK];            // (row of the tile << 16) | partner of the chunk
    __shared__ int32_t n_todo;
    const int item = blockIdx.x;
    if (item >= W.desc[P].dist_base) return;
    const int p = dg_find<0>(W.desc, P, item);
    const GraphDesc d = W.desc[p];
    const int q = item - d.dist_base;
    const int tile = q / d.nchunk, chunk = q - tile * d.nchunk;
    const int i0 = tile * DG_ROWS, j0 = chunk * EQD_BLOCK;
    if (j0 + EQD_BLOCK <= i0) return;                       // every j of the chunk is below every i of the tile
    const int n = d.n;
    const int nrow = n - i0 < DG_ROWS ? n - i0 : DG_ROWS;
    const int32_t* __restrict__ aoff = atom_off + d.r0;     // atom offsets of this protein's residues (global rows)
    if (threadIdx.x == 0) n_todo = 0;
    for (int r = 0; r < nrow; ++r) {
        const int a0 = aoff[i0 + r], na = aoff[i0 + r + 1] - a0;
        if (na <= DG_MAXATOMS)
            for (int k = threadIdx.x; k < 3 * na; k += EQD_BLOCK) ai[r][k / 3][k % 3] = atoms[(size_t)a0 * 3 + k];
    }
    __syncthreads();
    double* __restrict__ Dm = W.D + d.d_base;
    const double* __restrict__ cen = W.cen + (size_t)d.r0 * 3;
    const int j = j0 + threadIdx.x;
    int cut = 0;
    if (j < n) {
        const double cjx = cen[(size_t)j * 3], cjy = cen[(size_t)j * 3 + 1], cjz = cen[(size_t)j * 3 + 2];
        for (int r = 0; r < nrow; ++r) {
            const int i = i0 + r;
            if (j == i) Dm[(size_t)i * n + i] = __builtin_inf();          // np.full(..., np.inf), :320
            if (j <= i) continue;
            const double ex = cen[(size_t)i * 3] - cjx, ey = cen[(size_t)i * 3 + 1] - cjy, ez = cen[(size_t)i * 3 + 2] - cjz;
            if (prune && sqrt(ex * ex + ey * ey + ez * ez) >= prune_at) {
                Dm[(size_t)i * n + j] = __builtin_inf();
                Dm[(size_t)j * n + i] = __builtin_inf();
                ++cut;
            } else {
                todo[atomicAdd(&n_todo, 1)] = (r << 16) | (int)threadIdx.x;   // (an integer slot counter: order is free)
            }
        }
    }
    __syncthreads();
    const int nt = n_todo;
    for (int t = threadIdx.x; t < nt; t += EQD_BLOCK) {
        const int r = todo[t] >> 16, i = i0 + r, jj = j0 + (todo[t] & 0xffff);
        const int a0 = aoff[i], na = aoff[i + 1] - a0;
        const int b0 = aoff[jj], b1 = aoff[jj + 1];
        const bool in_lds = na <= DG_MAXATOMS;
        double s = 0.0;
        for (int a = 0; a < na; ++a) {
            const double ax = in_lds ? (double)ai[r][a][0] : (double)atoms[(size_t)(a0 + a) * 3];
            const double ay = in_lds ? (double)ai[r][a][1] : (double)atoms[(size_t)(a0 + a) * 3 + 1];
            const double az = in_lds ? (double)ai[r][a][2] : (double)atoms[(size_t)(a0 + a) * 3 + 2];
            for (int b = b0; b < b1; ++b) {
                const double dx = ax - (double)atoms[(size_t)b * 3], dy = ay - (double)atoms[(size_t)b * 3 + 1],
                             dz = az - (double)atoms[(size_t)b * 3 + 2];
                s += sqrt(dx * dx + dy * dy + dz * dz);
            }
        }
        const double m = s / (double)((long long)na * (long long)(b1 - b0));
        Dm[(size_t)i * n + jj] = m;
        Dm[(size_t)jj * n + i] = m;
    }
    if (prune) {                                             // (uniform over the block) one integer add per wave
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) cut += __shfl_xor(cut, m);
        if ((threadIdx.x & 63) == 0 && cut) atomicAdd(n_pruned, cut);
    }
}

// one wave per residue: the sources j with D[i][j] < cutoff in index order, or - when more than K qualify - the K
// smallest distances in ascending order (np.argsort, :339-343), plus the surface feature mu_r_norm (:351-359)
__global__ __launch_bounds__(EQD_BLOCK) void k_dg_select(int P, int K, double cutoff, const double* __restrict__ xall,
                                                         int32_t* __restrict__ deg, float* __restrict__ mu, GraphWs W) {
    const int item = blockIdx.x;
    if (item >= W.desc[P].sel_base) return;
    const int p = dg_find<1>(W.desc, P, item);
    const GraphDesc d = W.desc[p];
    const int lane = threadIdx.x & 63;
    const int n = d.n;
    const int i = (item - d.sel_base) * EQD_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const size_t gi = (size_t)d.r0 + i;
    const double* __restrict__ row = W.D + d.d_base + (size_t)i * n;
    const double* __restrict__ x = xall + (size_t)d.r0 * 3;
    int32_t* __restrict__ nbr = W.nbr;
    double* __restrict__ nbd = W.nbd;
    int count = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const bool v = j < n && row[j] < cutoff;
        count += __popcll(dg_ballot(v));
    }
    int dg;
    if (count <= K) {                 // np.where order (:339)
        int base = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const bool v = j < n && row[j] < cutoff;
            const unsigned long long mk = dg_ballot(v);
            if (v) {
                const int pos = base + __popcll(mk & ((1ull << lane) - 1ull));
                nbr[gi * K + pos] = j;
                nbd[gi * K + pos] = row[j];
            }
            base += __popcll(mk);
        }
        dg = count;
    } else {                          // the K smallest distances, ascending (np.argsort(row)[0:K], :342-343)
        double dprev = -1.0;
        int jprev = -1;
        for (int r = 0; r < K; ++r) {
            double best = __builtin_inf();
            int bj = 0x7fffffff;
            for (int j = lane; j < n; j += 64) {
                const double dd = row[j];
                const bool after = dd > dprev || (dd == dprev && j > jprev);
                if (after && (dd < best || (dd == best && j < bj))) {
                    best = dd;
                    bj = j;
                }
            }
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const double od = dg_shfl_xor_d(best, m);
                const int oj = __shfl_xor(bj, m);
                if (od < best || (od == best && oj < bj)) {
                    best = od;
                    bj = oj;
                }
            }
            if (lane == 0) {
                nbr[gi * K + r] = bj;
                nbd[gi * K + r] = best;
            }
            dprev = best;
            jprev = bj;
        }
        dg = K;
    }
    if (lane == 0) {
        deg[gi] = dg;
        W.rprot[gi] = p;
    }
    // surface feature (:351-359): for sigma in {1, 2, 5, 10, 30}: w = softmax_k(-d_k^2 / sigma),
    // mu = | sum_k w_k (x_i - x_k) | / sum_k w_k |x_i - x_k|          (lanes 0..4, one sigma each)
    wave_lds_fence();
    if (lane < 5) {
        const double sg[5] = {1., 2., 5., 10., 30.};
        const double sigma = sg[lane];
        double mx = -__builtin_inf();
        for (int k = 0; k < dg; ++k) {
            const double dd = ((volatile double*)nbd)[gi * K + k];
            mx = fmax(mx, -(dd * dd) / sigma);
        }
        double se = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, den = 0.0;
        for (int k = 0; k < dg; ++k) {
            const double dd = ((volatile double*)nbd)[gi * K + k];
            const int j = ((volatile int32_t*)nbr)[gi * K + k];
            const double w = exp(-(dd * dd) / sigma - mx);
            const double vx = x[(size_t)i * 3] - x[(size_t)j * 3], vy = x[(size_t)i * 3 + 1] - x[(size_t)j * 3 + 1],
                         vz = x[(size_t)i * 3 + 2] - x[(size_t)j * 3 + 2];
            se += w;
            m0 += w * vx; m1 += w * vy; m2 += w * vz;
            den += w * sqrt(vx * vx + vy * vy + vz * vz);
        }
        m0 /= se; m1 /= se; m2 /= se; den /= se;
        mu[gi * 5 + lane] = (float)(sqrt(m0 * m0 + m1 * m1 + m2 * m2) / den);
    }
}

// one workgroup: reoff = exclusive scan of deg over all residues (thread t owns a contiguous segment), edge_off[p] =
// reoff at the protein's first residue, no_nbr[p] = the protein's first residue of degree 0 (local index) or -1
__global__ __launch_bounds__(EQD_BLOCK) void k_dg_scan(int P, int R, const int32_t* __restrict__ deg, GraphWs W,
                                                       int32_t* __restrict__ edge_off, int32_t* __restrict__ no_nbr) {
    __shared__ int sums[EQD_BLOCK];
    __shared__ int first0[EQD_BLOCK];
    const int tid = threadIdx.x;
    const int per = (R + EQD_BLOCK - 1) / EQD_BLOCK;
    const int s0 = tid * per < R ? tid * per : R, s1 = s0 + per < R ? s0 + per : R;
    int s = 0, z = 0x7fffffff;
    for (int g = s0; g < s1; ++g) {
        const int dg = deg[g];
        if (dg == 0 && z == 0x7fffffff) z = g;
        s += dg;
    }
    sums[tid] = s;
    first0[tid] = z;
    __syncthreads();
    int base = 0;
    for (int t = 0; t < tid; ++t) base += sums[t];
    for (int g = s0; g < s1; ++g) {
        W.reoff[g] = base;
        base += deg[g];
    }
    if (tid == EQD_BLOCK - 1) {
        W.reoff[R] = base;
        edge_off[P] = base;
    }
    for (int p = tid; p < P; p += EQD_BLOCK) {
        const int r0 = W.desc[p].r0, r1 = r0 + W.desc[p].n;
        int t = r0 / per;
        int e = 0;
        for (int u = 0; u < t; ++u) e += sums[u];
        for (int g = t * per; g < r0; ++g) e += deg[g];
        edge_off[p] = e;
        int found = -1;
        const int seg_end = (t + 1) * per < r1 ? (t + 1) * per : r1;
        for (int g = r0; g < seg_end && found < 0; ++g)
            if (deg[g] == 0) found = g;
        for (++t; found < 0 && t < EQD_BLOCK && t * per < r1; ++t)
            if (first0[t] != 0x7fffffff) {       // the first residue of degree 0 behind r0: this protein's, or a later one's
                if (first0[t] < r1) found = first0[t];
                break;
            }
        no_nbr[p] = found < 0 ? -1 : found - r0;
    }
}

// destination-major edge list, 15 distance RBFs (:71-86) and the 12 orientation features p, q, k, t in the
// destination's local frame (:370-387)
__global__ __launch_bounds__(EQD_BLOCK) void k_dg_edges(int R, int K, const double* __restrict__ xall,
                                                        const double* __restrict__ fnall, const double* __restrict__ fuall,
                                                        const double* __restrict__ fvall, int32_t* __restrict__ src,
                                                        int32_t* __restrict__ dst, float* __restrict__ he, GraphWs W) {
    const long long idx = (long long)blockIdx.x * EQD_BLOCK + threadIdx.x;
    const int g = (int)(idx / K), k = (int)(idx - (long long)g * K);
    if (g >= R) return;
    const int e0 = W.reoff[g];
    if (k >= W.reoff[g + 1] - e0) return;
    const int r0 = W.desc[W.rprot[g]].r0;
    const int i = g - r0;
    const double* __restrict__ x = xall + (size_t)r0 * 3;
    const double* __restrict__ fn = fnall + (size_t)r0 * 3;
    const double* __restrict__ fu = fuall + (size_t)r0 * 3;
    const double* __restrict__ fv = fvall + (size_t)r0 * 3;
    const int e = e0 + k, j = W.nbr[(size_t)g * K + k];
    src[e] = j;
    dst[e] = i;
    const double d = W.nbd[(size_t)g * K + k];
    float* __restrict__ o = he + (size_t)e * 27;
    double ls = 1.0;
    for (int c = 0; c < 15; ++c) {        // distance_list_featurizer (:71-86): exp(-(d - 0)^2 / 1.5^c)
        o[c] = (float)exp(-(d * d) / ls);
        ls *= 1.5;
    }
    const double* B[3] = {fn + (size_t)i * 3, fu + (size_t)i * 3, fv + (size_t)i * 3};   // basis rows n_i, u_i, v_i of dst
    const double vec[4][3] = {{x[(size_t)j * 3] - x[(size_t)i * 3], x[(size_t)j * 3 + 1] - x[(size_t)i * 3 + 1],
                               x[(size_t)j * 3 + 2] - x[(size_t)i * 3 + 2]},
                              {fn[(size_t)j * 3], fn[(size_t)j * 3 + 1], fn[(size_t)j * 3 + 2]},
                              {fu[(size_t)j * 3], fu[(size_t)j * 3 + 1], fu[(size_t)j * 3 + 2]},
                              {fv[(size_t)j * 3], fv[(size_t)j * 3 + 1], fv[(size_t)j * 3 + 2]}};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 3; ++r)
            o[15 + 3 * q + r] = (float)((B[r][0] * vec[q][0] + B[r][1] * vec[q][1]) + B[r][2] * vec[q][2]);
}

// ---- host side ------------------------------------------------------------------------------------------------
static int dg_cdiv(int a, int b) { return (a + b - 1) / b; }

// validated item table of a batch (+ entry P with the totals); returns EQD_OK or an error code with the message set
static int dg_plan(const char* fn, int P, const int32_t* res_off, const int32_t* prot_atom_off, int K,
                   std::vector<GraphDesc>& D) {
    if (!res_off || !prot_atom_off) {
        eqd_set_error("%s: NULL offsets", fn);
        return EQD_ERR_NULL;
    }
    if (P < 1) {
        eqd_set_error("%s: n_protein = %d (need >= 1)", fn, P);
        return EQD_ERR_SHAPE;
    }
    if (K < 1 || K > 64) {
        eqd_set_error("%s: max_neighbor %d outside 1..64", fn, K);
        return EQD_ERR_UNSUPPORTED;
    }
    if (res_off[0] != 0 || prot_atom_off[0] != 0) {
        eqd_set_error("%s: res_off[0] = %d, prot_atom_off[0] = %d (need 0)", fn, res_off[0], prot_atom_off[0]);
        return EQD_ERR_SHAPE;
    }
    D.assign((size_t)P + 1, GraphDesc{});
    int64_t dist = 0, sel = 0, dsz = 0;
    for (int p = 0; p < P; ++p) {
        const int64_t n = (int64_t)res_off[p + 1] - res_off[p], na = (int64_t)prot_atom_off[p + 1] - prot_atom_off[p];
        if (n < 1 || na < n) {
            eqd_set_error("%s: protein %d has %lld residues and %lld atoms (offsets must increase; a protein needs >= 1 "
                          "residue and at least as many atoms as residues)", fn, p, (long long)n, (long long)na);
            return EQD_ERR_SHAPE;
        }
        GraphDesc& d = D[p];
        d.r0 = res_off[p]; d.n = (int32_t)n;
        d.ntile = dg_cdiv(d.n, DG_ROWS); d.nchunk = dg_cdiv(d.n, EQD_BLOCK);
        d.dist_base = (int32_t)dist; d.sel_base = (int32_t)sel; d.d_base = dsz;
        dist += (int64_t)d.ntile * d.nchunk;
        sel += dg_cdiv(d.n, EQD_WAVES);
        dsz += n * n;
        // (half of sum n^2 bounds the pruned-pair counter, an int32)
        if (dist > INT32_MAX || dsz > 2 * (int64_t)INT32_MAX || (int64_t)res_off[p + 1] * 64 * 27 > INT32_MAX) {
            eqd_set_error("%s: %lld residues, %lld distance entries, %lld work items up to protein %d do not fit 32-bit "
                          "offsets (split the batch)", fn, (long long)res_off[p + 1], (long long)dsz, (long long)dist, p);
            return EQD_ERR_SHAPE;
        }
    }
    GraphDesc& e = D[P];
    e.r0 = res_off[P];
    e.dist_base = (int32_t)dist; e.sel_base = (int32_t)sel; e.d_base = dsz;
    return EQD_OK;
}

static size_t dg_carve(int P, int K, const std::vector<GraphDesc>& D, EqdArena& A, GraphWs* W) {
    const GraphDesc& e = D[P];
    const size_t R = (size_t)e.r0;
    GraphWs w;
    w.desc = A.take<GraphDesc>((size_t)P + 1);
    w.cen = A.take<double>(R * 3);
    w.D = A.take<double>((size_t)e.d_base);
    w.nbr = A.take<int32_t>(R * K);
    w.nbd = A.take<double>(R * K);
    w.reoff = A.take<int32_t>(R + 1);
    w.rprot = A.take<int32_t>(R);
    if (W) *W = w;
    return A.off;
}

// plan + carve of a call on an initialised workspace
static int dg_open(const char* fn, int P, const int32_t* res_off, const int32_t* prot_atom_off, int K, void* workspace,
                   size_t ws_bytes, std::vector<GraphDesc>& D, GraphWs* W) {
    if (!workspace) {
        eqd_set_error("%s: NULL workspace", fn);
        return EQD_ERR_NULL;
    }
    if (int rc = dg_plan(fn, P, res_off, prot_atom_off, K, D)) return rc;
    EqdArena A(workspace, ws_bytes);
    dg_carve(P, K, D, A, W);
    if (!A.ok) {
        eqd_set_error("%s: workspace too small (%zu needed, %zu given)", fn, A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_graph_abi(void) { return EQD_DOCK_GRAPH_ABI; }

extern "C" EQD_DOCK_API size_t eqd_dock_graph_workspace_bytes(int P, const int32_t* res_off, const int32_t* prot_atom_off,
                                                              int max_neighbor) {
    std::vector<GraphDesc> D;
    if (dg_plan("eqd_dock_graph_workspace_bytes", P, res_off, prot_atom_off, max_neighbor, D) != EQD_OK) return 0;
    EqdArena A(nullptr, 0);
    return dg_carve(P, max_neighbor, D, A, nullptr) + 256;
}

extern "C" EQD_DOCK_API int eqd_dock_graph_init(int P, const int32_t* res_off, const int32_t* prot_atom_off,
                                                int max_neighbor, void* workspace, size_t ws_bytes, void* stream) {
    std::vector<GraphDesc> D;
    GraphWs W;
    if (int rc = dg_open("eqd_dock_graph_init", P, res_off, prot_atom_off, max_neighbor, workspace, ws_bytes, D, &W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync((void*)W.desc, D.data(), sizeof(GraphDesc) * D.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        eqd_set_error("eqd_dock_graph_init: copy failed");
        return EQD_ERR_LAUNCH;
    }
#ifndef EQD_HOSTSIM
    if (hipStreamSynchronize(s) != hipSuccess) {      // `D` is a local host buffer
        eqd_set_error("eqd_dock_graph_init: stream synchronisation failed");
        return EQD_ERR_LAUNCH;
    }
#endif
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_graph_select(int P, const int32_t* res_off, const int32_t* prot_atom_off,
                                                  const float* atoms, const int32_t* atom_off, const double* x,
                                                  double cutoff, int max_neighbor, int prune, int32_t* deg,
                                                  int32_t* edge_off, float* mu_r_norm, int32_t* no_neighbor,
                                                  int32_t* n_pruned, void* workspace, size_t ws_bytes, void* stream) {
    if (!atoms || !atom_off || !x || !deg || !edge_off || !mu_r_norm || !no_neighbor || !n_pruned) {
        eqd_set_error("eqd_dock_graph_select: NULL argument");
        return EQD_ERR_NULL;
    }
    std::vector<GraphDesc> D;
    GraphWs W;
    if (int rc = dg_open("eqd_dock_graph_select", P, res_off, prot_atom_off, max_neighbor, workspace, ws_bytes, D, &W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const int R = D[P].r0;
    hipLaunchKernelGGL(k_dg_centroids, dim3((unsigned)dg_cdiv(R, EQD_BLOCK)), dim3(EQD_BLOCK), 0, s, R, atoms, atom_off,
                       W.cen, n_pruned);
    if (int rc = eqd_check_launch("k_dg_centroids")) return rc;
    hipLaunchKernelGGL(k_dg_distances, dim3((unsigned)D[P].dist_base), dim3(EQD_BLOCK), 0, s, P, atoms, atom_off,
                       prune ? 1 : 0, cutoff + DG_PRUNE_MARGIN, W, n_pruned);
    if (int rc = eqd_check_launch("k_dg_distances")) return rc;
    hipLaunchKernelGGL(k_dg_select, dim3((unsigned)D[P].sel_base), dim3(EQD_BLOCK), 0, s, P, max_neighbor, cutoff, x, deg,
                       mu_r_norm, W);
    if (int rc = eqd_check_launch("k_dg_select")) return rc;
    hipLaunchKernelGGL(k_dg_scan, dim3(1), dim3(EQD_BLOCK), 0, s, P, R, deg, W, edge_off, no_neighbor);
    return eqd_check_launch("k_dg_scan");
}

extern "C" EQD_DOCK_API int eqd_dock_graph_edges(int P, const int32_t* res_off, const int32_t* prot_atom_off,
                                                 int max_neighbor, const double* x, const double* n_i, const double* u_i,
                                                 const double* v_i, int32_t* src, int32_t* dst, float* he,
                                                 void* workspace, size_t ws_bytes, void* stream) {
    if (!x || !n_i || !u_i || !v_i || !src || !dst || !he) {
        eqd_set_error("eqd_dock_graph_edges: NULL argument");
        return EQD_ERR_NULL;
    }
    std::vector<GraphDesc> D;
    GraphWs W;
    if (int rc = dg_open("eqd_dock_graph_edges", P, res_off, prot_atom_off, max_neighbor, workspace, ws_bytes, D, &W))
        return rc;
    const int R = D[P].r0;
    const long long total = (long long)R * max_neighbor;
    hipLaunchKernelGGL(k_dg_edges, dim3((unsigned)((total + EQD_BLOCK - 1) / EQD_BLOCK)), dim3(EQD_BLOCK), 0,
                       (hipStream_t)stream, R, max_neighbor, x, n_i, u_i, v_i, src, dst, he, W);
    return eqd_check_launch("k_dg_edges");
}

// Batched solvent-accessible surface (include/equidock_dock.h): Shrake-Rupley over EVERY heavy atom of C complexes in one
// device pass - per atom the sphere points left exposed by its own side (alone) and by both sides (in complex), from which
// the SASA of each partner and of the complex, the buried surface area and the buried atoms and residues follow.
//   R_i = (double)r_i + probe;  point k of atom i: q = x_i + R_i * u_k (one multiply, one add per component)
//   buried by j != i when s = (dx dx + dy dy) + dz dz < R_j R_j, d = q - x_j; fp64 from the fp32 rows, -ffp-contract=off
//
// Work decomposition.  Five launches, whatever C is; a complex's atoms are its ligand rows followed by its receptor rows:
//   k_sa_bounds    one thread per residue: the fp64 centroid of its atoms and its reach - the radius around the centroid
//                  plus the largest expanded radius of its atoms
//   k_sa_lists     items (complex, tile of SA_TILE atoms): the workgroup walks ALL residues of the complex in chunks of
//                  SA_CHUNK residues staged in LDS (centroid, reach, atom rows); thread (atom, wave) tests every fourth
//                  residue of the chunk - a wave reads one residue at a time, an LDS broadcast - and passes over it when
//                  the squared centroid distance is >= (R_i + reach + 2e-6)^2: then no atom of it can pass the atom test.
//                  The atoms of the other residues are read from global memory and partner j is kept unless the squared
//                  centre distance is >= (R_i + R_j + 1e-6)^2, where no point of i can lie inside j's sphere.
//                  Kept partners go on the atom's list of SA_CAP entries: same-side partners from the front, other-side
//                  partners from the back, slots handed out by two integer counters per atom in LDS.  The counters are
//                  stored whole, so an atom whose partners do not fit is known.
//   k_sa_points    one wave per atom, one lane per sphere point, ceil(P / 64) passes.  The wave stages up to 64 partners
//                  (centre, R_j^2; the atom itself gets R_j^2 = -1) in its own LDS rows, then every lane tests its point
//                  against them by broadcast reads: same-side partners first (a hit buries the point alone and in
//                  complex), other-side partners after (a hit buries it in complex).  Every SA_STEP partners an integer
//                  shuffle reduction asks whether any lane's point is still exposed; if none, the wave leaves the phase.
//                  An atom whose list overflowed - or every atom when all_partners != 0 - walks ALL rows of its complex
//                  instead of the list, own side first: each lane applies the rule of k_sa_lists to one of the 64 rows
//                  of a segment and the kept ones are packed into the wave's LDS rows (an integer slot counter again).
//   k_sa_residues  one thread per residue: its atoms' areas in row order, and whether an atom of it lost a point
//   k_sa_finish    one workgroup per complex: the atom terms of SA_ROWS rows at a time into LDS, then threads 0-3 each
//                  add one of the four running sums (side alone, complex, BSA, the side's share) in row order, ligand
//                  before receptor; integer totals by thread-strided sums and an integer shuffle reduction
// Whether a point is buried does not depend on the order in which partners are tested, so the order of a list (the only
// thing the integer slot counters leave open) changes no output; every floating-point sum has one owner and a fixed
// order; the item table depends only on each complex's own sizes: a complex's results are bit-identical alone, in any
// batch, at any position, from run to run and between the list and the all-partners path.
#include "../csrc/eqd_common.h"
#include "../../include/equidock_dock.h"

#include <math.h>
#include <vector>

#define SA_TILE 64          // atoms per lists item (one per lane; the four waves split the chunk's partners)
#define SA_CHUNK 256        // residues staged per step of the lists kernel
#define SA_CAP 96           // list entries per atom (same side from the front, other side from the back)
#define SA_SEG 64           // partners a wave of the point kernel stages at a time
#define SA_STEP 16          // partners between two "is any point still exposed" reductions
#define SA_ROWS 256         // atom rows per step of the finish kernel
#define SA_MAX_POINTS EQD_DOCK_SASA_MAX_POINTS
#define SA_SKIP_MARGIN 1e-6
#define SA_FOUR_PI (4.0 * 3.14159265358979323846)

static_assert(SA_TILE * EQD_WAVES == EQD_BLOCK, "lists kernel: one atom per lane, the waves split the partners");
static_assert(SA_CHUNK == EQD_BLOCK, "lists kernel: every thread stages one residue");
static_assert(SA_TILE % EQD_WAVES == 0 && SA_SEG == 64, "one wave per atom, one lane per staged row");
static_assert(SA_ROWS == EQD_BLOCK, "finish kernel: one row per thread and step");

struct SasaDesc {           // one complex of the batch (entry C: the totals)
    int32_t la0, nla, ra0, nra;     // atom rows
    int32_t lr0, nlr, rr0, nrr;     // residues
    int32_t tile_base, ntile;       // first lists item, tiles of the concatenated rows
    int32_t a0;                     // first row of the complex in the per-atom workspace arrays (= la0 + ra0)
    int32_t pad;
};

struct SasaWs {
    const SasaDesc* desc;   // [C + 1]
    int32_t* cnt;           // [A_l + A_r][2] partners kept: same side, other side
    int32_t* list;          // [A_l + A_r][SA_CAP] local rows of the kept partners
    double* bl4;            // [R_l][4] centroid of every ligand residue and its reach: radius + largest expanded radius
    double* br4;            // [R_r][4]
    int32_t* bl;            // [R_l] 1 when an atom of the ligand residue lost a point on binding
    int32_t* br;            // [R_r]
};

// the complex that owns item / residue `v`: the largest c with base(c) <= v (kind 0 tiles, 1 ligand residues, 2 receptor
// residues; the bases are strictly increasing)
template <int kKind>
__device__ __forceinline__ int sa_find(const SasaDesc* __restrict__ D, int C, int v) {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int b = kKind == 0 ? D[mid].tile_base : kKind == 1 ? D[mid].lr0 : D[mid].rr0;
        if (b <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// local row g (0 <= g < nla + nra) of complex d: centre and expanded radius in fp64
__device__ __forceinline__ void sa_atom(const SasaDesc& d, int g, const float* __restrict__ lig,
                                        const float* __restrict__ rec, const float* __restrict__ lrad,
                                        const float* __restrict__ rrad, double probe, double& x, double& y, double& z,
                                        double& R) {
    const bool l = g < d.nla;
    const size_t row = l ? (size_t)d.la0 + g : (size_t)d.ra0 + (g - d.nla);
    const float* __restrict__ p = (l ? lig : rec) + row * 3;
    x = (double)p[0];
    y = (double)p[1];
    z = (double)p[2];
    R = (double)(l ? lrad : rrad)[row] + probe;
}

// atom rows [a0, a1) of residue g, held inside its complex's rows [lo, hi) whatever the table says
__device__ __forceinline__ void sa_range(const int32_t* __restrict__ first, int g, int lo, int hi, int& a0, int& a1) {
    a0 = first[g];
    a1 = first[g + 1];
    a0 = a0 < lo ? lo : (a0 > hi ? hi : a0);
    a1 = a1 < a0 ? a0 : (a1 > hi ? hi : a1);
}

__global__ __launch_bounds__(EQD_BLOCK) void k_sa_bounds(int C, const float* __restrict__ lig, const float* __restrict__ rec,
                                                         const float* __restrict__ lrad, const float* __restrict__ rrad,
                                                         const int32_t* __restrict__ lfirst,
                                                         const int32_t* __restrict__ rfirst, double probe, SasaWs W) {
    const int Rl = W.desc[C].lr0, Rr = W.desc[C].rr0;
    int r = blockIdx.x * EQD_BLOCK + threadIdx.x;
    if (r >= Rl + Rr) return;
    const bool l = r < Rl;
    if (!l) r -= Rl;
    const SasaDesc d = W.desc[l ? sa_find<1>(W.desc, C, r) : sa_find<2>(W.desc, C, r)];
    int a0, a1;
    if (l) sa_range(lfirst, r, d.la0, d.la0 + d.nla, a0, a1);
    else sa_range(rfirst, r, d.ra0, d.ra0 + d.nra, a0, a1);
    const float* __restrict__ x = l ? lig : rec;
    const float* __restrict__ rad = l ? lrad : rrad;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int a = a0; a < a1; ++a) {
        sx += (double)x[(size_t)a * 3];
        sy += (double)x[(size_t)a * 3 + 1];
        sz += (double)x[(size_t)a * 3 + 2];
    }
    const double na = (double)(a1 - a0 > 0 ? a1 - a0 : 1);
    const double cx = sx / na, cy = sy / na, cz = sz / na;
    double far = 0.0, big = 0.0;
    for (int a = a0; a < a1; ++a) {
        const double dx = (double)x[(size_t)a * 3] - cx, dy = (double)x[(size_t)a * 3 + 1] - cy, dz = (double)x[(size_t)a * 3 + 2] - cz;
        const double e = sqrt((dx * dx + dy * dy) + dz * dz), R = (double)rad[a] + probe;
        far = e > far ? e : far;
        big = R > big ? R : big;
    }
    double* __restrict__ o = (l ? W.bl4 : W.br4) + (size_t)r * 4;
    o[0] = cx;
    o[1] = cy;
    o[2] = cz;
    o[3] = far + big;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_sa_lists(int C, const float* __restrict__ lig, const float* __restrict__ rec,
                                                        const float* __restrict__ lrad, const float* __restrict__ rrad,
                                                        const int32_t* __restrict__ lfirst,
                                                        const int32_t* __restrict__ rfirst, double probe, SasaWs W) {
    __shared__ double px[SA_CHUNK], py[SA_CHUNK], pz[SA_CHUNK], pr[SA_CHUNK];      // a residue's centroid and reach
    __shared__ int32_t pa0[SA_CHUNK], pa1[SA_CHUNK];                               // its local rows [pa0, pa1)
    __shared__ int32_t ns[SA_TILE], no[SA_TILE];
    const int item = blockIdx.x;
    if (item >= W.desc[C].tile_base) return;
    const int c = sa_find<0>(W.desc, C, item);
    const SasaDesc d = W.desc[c];
    const int n = d.nla + d.nra, nres = d.nlr + d.nrr;
    const int tid = threadIdx.x, a = tid & (SA_TILE - 1), w = tid / SA_TILE;
    const int g = (item - d.tile_base) * SA_TILE + a;
    const bool valid = g < n;
    const int gi = valid ? g : n - 1;
    double xi, yi, zi, Ri;
    sa_atom(d, gi, lig, rec, lrad, rrad, probe, xi, yi, zi, Ri);
    const bool lig_i = gi < d.nla;
    int32_t* __restrict__ L = W.list + ((size_t)d.a0 + gi) * SA_CAP;
    if (tid < SA_TILE) {
        ns[tid] = 0;
        no[tid] = 0;
    }
    for (int q0 = 0; q0 < nres; q0 += SA_CHUNK) {
        __syncthreads();                                        // the previous chunk has been read (the counters are zero)
        if (q0 + tid < nres) {
            const int q = q0 + tid;
            const bool l = q < d.nlr;
            const double* __restrict__ b = l ? W.bl4 + ((size_t)d.lr0 + q) * 4 : W.br4 + ((size_t)d.rr0 + (q - d.nlr)) * 4;
            px[tid] = b[0];
            py[tid] = b[1];
            pz[tid] = b[2];
            pr[tid] = b[3];
            int a0, a1;
            if (l) sa_range(lfirst, d.lr0 + q, d.la0, d.la0 + d.nla, a0, a1);
            else sa_range(rfirst, d.rr0 + (q - d.nlr), d.ra0, d.ra0 + d.nra, a0, a1);
            pa0[tid] = l ? a0 - d.la0 : a0 - d.ra0 + d.nla;
            pa1[tid] = l ? a1 - d.la0 : a1 - d.ra0 + d.nla;
        }
        __syncthreads();
        const int nq = nres - q0 < SA_CHUNK ? nres - q0 : SA_CHUNK;
        if (valid) {
            for (int jj = w; jj < nq; jj += EQD_WAVES) {
                // no atom of the residue is nearer than (centroid distance - radius): with 2e-6 here, none can pass the
                // atom test below, whose slack is 1e-6
                const double ex = xi - px[jj], ey = yi - py[jj], ez = zi - pz[jj];
                const double far = (Ri + pr[jj]) + 2.0 * SA_SKIP_MARGIN;
                if ((ex * ex + ey * ey) + ez * ez >= far * far) continue;
                for (int j = pa0[jj]; j < pa1[jj]; ++j) {
                    if (j == g) continue;
                    double xj, yj, zj, Rj;
                    sa_atom(d, j, lig, rec, lrad, rrad, probe, xj, yj, zj, Rj);
                    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
                    const double s = (dx * dx + dy * dy) + dz * dz;
                    const double reach = (Ri + Rj) + SA_SKIP_MARGIN;
                    if (s < reach * reach) {
                        const bool same = (j < d.nla) == lig_i;
                        const int slot = atomicAdd(same ? &ns[a] : &no[a], 1);      // (an integer slot counter: order is free)
                        if (slot < SA_CAP) L[same ? slot : SA_CAP - 1 - slot] = j;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (tid < SA_TILE && valid) {
        W.cnt[((size_t)d.a0 + g) * 2] = ns[tid];
        W.cnt[((size_t)d.a0 + g) * 2 + 1] = no[tid];
    }
}

__global__ __launch_bounds__(EQD_BLOCK) void k_sa_points(int C, const float* __restrict__ lig, const float* __restrict__ rec,
                                                         const float* __restrict__ lrad, const float* __restrict__ rrad,
                                                         const double* __restrict__ sphere, int P, double probe,
                                                         int all_partners, int32_t* __restrict__ lig_points,
                                                         int32_t* __restrict__ rec_points, SasaWs W) {
    __shared__ double sx[EQD_WAVES][SA_SEG], sy[EQD_WAVES][SA_SEG], sz[EQD_WAVES][SA_SEG], sq[EQD_WAVES][SA_SEG];
    __shared__ int32_t kc[EQD_WAVES];                           // partners a wave has kept on the all-partners path
    const int per_tile = SA_TILE / EQD_WAVES;                  // workgroups per tile of atoms
    const int item = blockIdx.x / per_tile;
    if (item >= W.desc[C].tile_base) return;
    const int c = sa_find<0>(W.desc, C, item);
    const SasaDesc d = W.desc[c];
    const int n = d.nla + d.nra;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = (item - d.tile_base) * SA_TILE + (blockIdx.x % per_tile) * EQD_WAVES + w;
    if (g >= n) return;                                         // (the whole wave; this kernel has no workgroup barrier)
    double xi, yi, zi, Ri;
    sa_atom(d, g, lig, rec, lrad, rrad, probe, xi, yi, zi, Ri);
    const bool lig_i = g < d.nla;
    const int n_same_kept = W.cnt[((size_t)d.a0 + g) * 2], n_other_kept = W.cnt[((size_t)d.a0 + g) * 2 + 1];
    const bool walk_all = all_partners != 0 || n_same_kept > SA_CAP || n_other_kept > SA_CAP ||
                          n_same_kept + n_other_kept > SA_CAP || n_same_kept < 0 || n_other_kept < 0;
    const int own0 = lig_i ? 0 : d.nla, own_n = lig_i ? d.nla : d.nra;
    const int oth0 = lig_i ? d.nla : 0, oth_n = lig_i ? d.nra : d.nla;
    const int32_t* __restrict__ L = W.list + ((size_t)d.a0 + g) * SA_CAP;
    int tot_alone = 0, tot_cplx = 0, kbase = 0;
    if (lane == 0) kc[w] = 0;                                   // (ordered before its first use by the fence below)
    for (int p0 = 0; p0 < P; p0 += 64) {
        const bool ok = p0 + lane < P;
        const double* __restrict__ u = sphere + (size_t)(ok ? p0 + lane : P - 1) * 3;
        const double qx = xi + Ri * u[0], qy = yi + Ri * u[1], qz = zi + Ri * u[2];
        int ea = ok ? 1 : 0, ec = ea;                           // the point is exposed alone / in complex
        for (int phase = 0; phase < 2; ++phase) {
            const int m_all = walk_all ? (phase ? oth_n : own_n) : (phase ? n_other_kept : n_same_kept);
            bool live = true;
            int since = SA_STEP;                                // partners tested since the last "any point exposed" look
            for (int s0 = 0; s0 < m_all && live; s0 += SA_SEG) {
                const int m = m_all - s0 < SA_SEG ? m_all - s0 : SA_SEG;
                wave_lds_fence();                               // the previous segment has been read
                if (lane < m) {
                    const int e = s0 + lane;
                    int j = walk_all ? (phase ? oth0 : own0) + e : (phase ? L[SA_CAP - 1 - e] : L[e]);
                    j = j < 0 ? 0 : (j >= n ? n - 1 : j);
                    double x, y, z, R;
                    sa_atom(d, j, lig, rec, lrad, rrad, probe, x, y, z, R);
                    int slot = lane;
                    bool keep = true;
                    if (walk_all) {                             // the rule of k_sa_lists, the kept partners packed
                        const double dx = xi - x, dy = yi - y, dz = zi - z;
                        const double reach = (Ri + R) + SA_SKIP_MARGIN;
                        keep = j != g && (dx * dx + dy * dy) + dz * dz < reach * reach;
                        if (keep) slot = atomicAdd(&kc[w], 1) - kbase;      // (an integer slot counter: order is free)
                    }
                    if (keep) {
                        sx[w][slot] = x;
                        sy[w][slot] = y;
                        sz[w][slot] = z;
                        sq[w][slot] = j == g ? -1.0 : R * R;
                    }
                }
                wave_lds_fence();
                const int mk = walk_all ? kc[w] - kbase : m;    // (wave-uniform)
                kbase += walk_all ? mk : 0;
                for (int b0 = 0; b0 < mk; b0 += SA_STEP) {
                    const int b1 = b0 + SA_STEP < mk ? b0 + SA_STEP : mk;
                    if (since >= SA_STEP) {
                        since = 0;
                        int any = phase ? ec : ea;
#pragma unroll
                        for (int k = 1; k < 64; k <<= 1) any |= __shfl_xor(any, k);
                        if (!any) {                             // (wave-uniform) no point is left to bury in this phase
                            live = false;
                            break;
                        }
                    }
                    since += b1 - b0;
                    for (int b = b0; b < b1; ++b) {
                        const double dx = qx - sx[w][b], dy = qy - sy[w][b], dz = qz - sz[w][b];
                        const double s = (dx * dx + dy * dy) + dz * dz;
                        const int hit = s < sq[w][b] ? 1 : 0;
                        ec &= ~hit;
                        if (phase == 0) ea &= ~hit;
                    }
                }
            }
        }
        tot_alone += ea;
        tot_cplx += ec;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {                          // (integers: the order changes nothing)
        tot_alone += __shfl_xor(tot_alone, k);
        tot_cplx += __shfl_xor(tot_cplx, k);
    }
    if (lane == 0) {
        int32_t* __restrict__ o = lig_i ? lig_points + ((size_t)d.la0 + g) * 2 : rec_points + ((size_t)d.ra0 + (g - d.nla)) * 2;
        o[0] = tot_alone;
        o[1] = tot_cplx;
    }
}

// area of one exposed point of an atom of expanded radius R
__device__ __forceinline__ double sa_point_area(double R, int P) { return SA_FOUR_PI * R * R / (double)P; }

__global__ __launch_bounds__(EQD_BLOCK) void k_sa_residues(int C, const float* __restrict__ lrad,
                                                           const float* __restrict__ rrad,
                                                           const int32_t* __restrict__ lfirst,
                                                           const int32_t* __restrict__ rfirst, int P, double probe,
                                                           const int32_t* __restrict__ lig_points,
                                                           const int32_t* __restrict__ rec_points,
                                                           double* __restrict__ lig_res_area,
                                                           double* __restrict__ rec_res_area, SasaWs W) {
    const int Rl = W.desc[C].lr0, Rr = W.desc[C].rr0;
    int r = blockIdx.x * EQD_BLOCK + threadIdx.x;
    if (r >= Rl + Rr) return;
    const bool l = r < Rl;
    if (!l) r -= Rl;
    const SasaDesc d = W.desc[l ? sa_find<1>(W.desc, C, r) : sa_find<2>(W.desc, C, r)];
    int a0, a1;
    if (l) sa_range(lfirst, r, d.la0, d.la0 + d.nla, a0, a1);
    else sa_range(rfirst, r, d.ra0, d.ra0 + d.nra, a0, a1);
    const float* __restrict__ rad = l ? lrad : rrad;
    const int32_t* __restrict__ pts = l ? lig_points : rec_points;
    double alone = 0.0, cplx = 0.0;
    int buried = 0;
    for (int a = a0; a < a1; ++a) {
        const double wgt = sa_point_area((double)rad[a] + probe, P);
        const int na = pts[(size_t)a * 2], nc = pts[(size_t)a * 2 + 1];
        alone += wgt * (double)na;
        cplx += wgt * (double)nc;
        buried |= na > nc ? 1 : 0;
    }
    double* __restrict__ o = (l ? lig_res_area : rec_res_area) + (size_t)r * 2;
    o[0] = alone;
    o[1] = cplx;
    (l ? W.bl : W.br)[r] = buried;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_sa_finish(int C, const float* __restrict__ lrad,
                                                         const float* __restrict__ rrad, int P, double probe,
                                                         const int32_t* __restrict__ lig_points,
                                                         const int32_t* __restrict__ rec_points, double* __restrict__ rows,
                                                         SasaWs W) {
    __shared__ double t[3][SA_ROWS];                            // the terms of SA_ROWS rows: alone, in complex, buried
    __shared__ int32_t red[EQD_WAVES][6];
    const int c = blockIdx.x;
    if (c >= C) return;
    const SasaDesc d = W.desc[c];
    const int tid = threadIdx.x;
    // threads 0-3 each own one running sum, added in row order: 0 the side's area alone, 1 the complex's area, 2 the BSA,
    // 3 the side's share of the BSA (0 and 3 start again at the receptor)
    const double* __restrict__ mine = t[tid < 2 ? tid : 2];
    double acc = 0.0, kept[2] = {0.0, 0.0};
    int nbur[2] = {0, 0}, nres[2] = {0, 0}, pa = 0, pc = 0;
    for (int side = 0; side < 2; ++side) {
        const int first = side ? d.ra0 : d.la0, cnt = side ? d.nra : d.nla;
        const float* __restrict__ rad = side ? rrad : lrad;
        const int32_t* __restrict__ pts = side ? rec_points : lig_points;
        for (int r0 = 0; r0 < cnt; r0 += SA_ROWS) {
            const int m = cnt - r0 < SA_ROWS ? cnt - r0 : SA_ROWS;
            if (tid < m) {
                const size_t a = (size_t)first + r0 + tid;
                const double wgt = sa_point_area((double)rad[a] + probe, P);
                const int na = pts[a * 2], nc = pts[a * 2 + 1];
                t[0][tid] = wgt * (double)na;
                t[1][tid] = wgt * (double)nc;
                t[2][tid] = wgt * (double)(na - nc);
                nbur[side] += na > nc ? 1 : 0;
                pa += na;
                pc += nc;
            }
            __syncthreads();
            if (tid < 4) {
                if (m == SA_ROWS) {
#pragma unroll 16
                    for (int k = 0; k < SA_ROWS; ++k) acc += mine[k];      // row order
                } else {
                    for (int k = 0; k < m; ++k) acc += mine[k];
                }
            }
            __syncthreads();
        }
        kept[side] = acc;
        if (tid == 0 || tid == 3) acc = 0.0;
        const int32_t* __restrict__ flag = side ? W.br + d.rr0 : W.bl + d.lr0;
        const int nr = side ? d.nrr : d.nlr;
        for (int r = tid; r < nr; r += EQD_BLOCK) nres[side] += flag[r] ? 1 : 0;
    }
    int v[6] = {nbur[0], nbur[1], nres[0], nres[1], pa, pc};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v[k] += __shfl_xor(v[k], m);       // (integers: the order changes nothing)
        if ((tid & 63) == 0) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    double* __restrict__ o = rows + (size_t)c * EQD_DOCK_SASA_COLS;
    if (tid == 0) {
        o[0] = kept[0];
        o[1] = kept[1];
    } else if (tid == 1) {
        o[2] = kept[1];
    } else if (tid == 2) {
        o[3] = kept[1];
    } else if (tid == 3) {
        o[4] = kept[0];
        o[5] = kept[1];
    } else if (tid >= 64 && tid < 70) {
        const int k = tid - 64;
        o[6 + k] = (double)((red[0][k] + red[1][k]) + (red[2][k] + red[3][k]));
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
static int sa_cdiv(int a, int b) { return (a + b - 1) / b; }

// validated item table of a batch (+ entry C with the totals); returns EQD_OK or an error code with the message set
static int sa_plan(const char* fn, int C, const int32_t* lao, const int32_t* rao, const int32_t* lro, const int32_t* rro,
                   int P, std::vector<SasaDesc>& D) {
    if (!lao || !rao || !lro || !rro) {
        eqd_set_error("%s: NULL offsets", fn);
        return EQD_ERR_NULL;
    }
    if (C < 1) {
        eqd_set_error("%s: n_complex = %d (need >= 1)", fn, C);
        return EQD_ERR_SHAPE;
    }
    if (P < 1 || P > SA_MAX_POINTS) {
        eqd_set_error("%s: n_points = %d (need 1..%d)", fn, P, SA_MAX_POINTS);
        return EQD_ERR_SHAPE;
    }
    if (lao[0] != 0 || rao[0] != 0 || lro[0] != 0 || rro[0] != 0) {
        eqd_set_error("%s: lig_atom_off[0] = %d, rec_atom_off[0] = %d, lig_res_off[0] = %d, rec_res_off[0] = %d (need 0)", fn,
                      lao[0], rao[0], lro[0], rro[0]);
        return EQD_ERR_SHAPE;
    }
    D.assign((size_t)C + 1, SasaDesc{});
    int64_t tile = 0;
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
        if (nla + nra > INT32_MAX - SA_CHUNK || ((int64_t)lao[c + 1] + rao[c + 1]) * 3 > INT32_MAX) {
            eqd_set_error("%s: %lld ligand and %lld receptor atoms up to complex %d do not fit 32-bit offsets (split the "
                          "batch)", fn, (long long)lao[c + 1], (long long)rao[c + 1], c);
            return EQD_ERR_SHAPE;
        }
        SasaDesc& d = D[c];
        d.la0 = lao[c]; d.nla = (int32_t)nla; d.ra0 = rao[c]; d.nra = (int32_t)nra;
        d.lr0 = lro[c]; d.nlr = (int32_t)nlr; d.rr0 = rro[c]; d.nrr = (int32_t)nrr;
        d.ntile = sa_cdiv(d.nla + d.nra, SA_TILE);
        d.tile_base = (int32_t)tile;
        d.a0 = d.la0 + d.ra0;
        tile += d.ntile;
        if (tile * (SA_TILE / EQD_WAVES) > INT32_MAX) {
            eqd_set_error("%s: %lld atom tiles up to complex %d do not fit a launch (split the batch)", fn, (long long)tile, c);
            return EQD_ERR_SHAPE;
        }
    }
    SasaDesc& e = D[C];
    e.la0 = lao[C]; e.ra0 = rao[C]; e.lr0 = lro[C]; e.rr0 = rro[C];
    e.tile_base = (int32_t)tile;
    e.a0 = e.la0 + e.ra0;
    return EQD_OK;
}

static size_t sa_carve(int C, const std::vector<SasaDesc>& D, EqdArena& A, SasaWs* W) {
    const SasaDesc& e = D[C];
    SasaWs w;
    w.desc = A.take<SasaDesc>((size_t)C + 1);
    w.cnt = A.take<int32_t>((size_t)e.a0 * 2);
    w.list = A.take<int32_t>((size_t)e.a0 * SA_CAP);
    w.bl4 = A.take<double>((size_t)e.lr0 * 4);
    w.br4 = A.take<double>((size_t)e.rr0 * 4);
    w.bl = A.take<int32_t>((size_t)e.lr0);
    w.br = A.take<int32_t>((size_t)e.rr0);
    if (W) *W = w;
    return A.off;
}

// plan + carve of a call on a workspace
static int sa_open(const char* fn, int C, const int32_t* lao, const int32_t* rao, const int32_t* lro, const int32_t* rro,
                   int P, void* workspace, size_t ws_bytes, std::vector<SasaDesc>& D, SasaWs* W) {
    if (!workspace) {
        eqd_set_error("%s: NULL workspace", fn);
        return EQD_ERR_NULL;
    }
    if (int rc = sa_plan(fn, C, lao, rao, lro, rro, P, D)) return rc;
    EqdArena A(workspace, ws_bytes);
    sa_carve(C, D, A, W);
    if (!A.ok) {
        eqd_set_error("%s: workspace too small (%zu needed, %zu given)", fn, A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_sasa_abi(void) { return EQD_DOCK_SASA_ABI; }

extern "C" EQD_DOCK_API size_t eqd_dock_sasa_workspace_bytes(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                             const int32_t* lig_res_off, const int32_t* rec_res_off,
                                                             int n_points) {
    std::vector<SasaDesc> D;
    if (sa_plan("eqd_dock_sasa_workspace_bytes", C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, n_points, D) != EQD_OK)
        return 0;
    EqdArena A(nullptr, 0);
    return sa_carve(C, D, A, nullptr) + 256;
}

extern "C" EQD_DOCK_API int eqd_dock_sasa_init(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                               const int32_t* lig_res_off, const int32_t* rec_res_off, int n_points,
                                               void* workspace, size_t ws_bytes, void* stream) {
    std::vector<SasaDesc> D;
    SasaWs W;
    if (int rc = sa_open("eqd_dock_sasa_init", C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, n_points, workspace,
                         ws_bytes, D, &W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync((void*)W.desc, D.data(), sizeof(SasaDesc) * D.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        eqd_set_error("eqd_dock_sasa_init: copy failed");
        return EQD_ERR_LAUNCH;
    }
#ifndef EQD_HOSTSIM
    if (hipStreamSynchronize(s) != hipSuccess) {      // `D` is a local host buffer
        eqd_set_error("eqd_dock_sasa_init: stream synchronisation failed");
        return EQD_ERR_LAUNCH;
    }
#endif
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_sasa_eval(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                               const int32_t* lig_res_off, const int32_t* rec_res_off, const float* lig,
                                               const float* rec, const float* lig_radius, const float* rec_radius,
                                               const int32_t* lig_res_first, const int32_t* rec_res_first,
                                               const double* sphere, int n_points, double probe, int all_partners,
                                               int32_t* lig_points, int32_t* rec_points, double* lig_res_area,
                                               double* rec_res_area, double* rows, void* workspace, size_t ws_bytes,
                                               void* stream) {
    const char* fn = "eqd_dock_sasa_eval";
    if (!lig || !rec || !lig_radius || !rec_radius || !lig_res_first || !rec_res_first || !sphere || !lig_points ||
        !rec_points || !lig_res_area || !rec_res_area || !rows) {
        eqd_set_error("%s: NULL argument", fn);
        return EQD_ERR_NULL;
    }
    if (!(probe > 0.0) || !(probe < (double)INFINITY)) {
        eqd_set_error("%s: probe = %g (need a finite value > 0)", fn, probe);
        return EQD_ERR_SHAPE;
    }
    std::vector<SasaDesc> D;
    SasaWs W;
    if (int rc = sa_open(fn, C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, n_points, workspace, ws_bytes, D, &W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const unsigned n_tile = (unsigned)D[C].tile_base, n_res = (unsigned)D[C].lr0 + (unsigned)D[C].rr0;
    hipLaunchKernelGGL(k_sa_bounds, dim3((n_res + EQD_BLOCK - 1) / EQD_BLOCK), dim3(EQD_BLOCK), 0, s, C, lig, rec, lig_radius,
                       rec_radius, lig_res_first, rec_res_first, probe, W);
    if (int rc = eqd_check_launch("k_sa_bounds")) return rc;
    hipLaunchKernelGGL(k_sa_lists, dim3(n_tile), dim3(EQD_BLOCK), 0, s, C, lig, rec, lig_radius, rec_radius, lig_res_first,
                       rec_res_first, probe, W);
    if (int rc = eqd_check_launch("k_sa_lists")) return rc;
    hipLaunchKernelGGL(k_sa_points, dim3(n_tile * (SA_TILE / EQD_WAVES)), dim3(EQD_BLOCK), 0, s, C, lig, rec, lig_radius,
                       rec_radius, sphere, n_points, probe, all_partners ? 1 : 0, lig_points, rec_points, W);
    if (int rc = eqd_check_launch("k_sa_points")) return rc;
    hipLaunchKernelGGL(k_sa_residues, dim3((n_res + EQD_BLOCK - 1) / EQD_BLOCK), dim3(EQD_BLOCK), 0, s, C, lig_radius,
                       rec_radius, lig_res_first, rec_res_first, n_points, probe, lig_points, rec_points, lig_res_area,
                       rec_res_area, W);
    if (int rc = eqd_check_launch("k_sa_residues")) return rc;
    hipLaunchKernelGGL(k_sa_finish, dim3((unsigned)C), dim3(EQD_BLOCK), 0, s, C, lig_radius, rec_radius, n_points, probe, lig_points,
                       rec_points, rows, W);
    return eqd_check_launch("k_sa_finish");
}

// Batched residue depth (include/equidock_dock.h): for EVERY heavy atom of C complexes the distance to the nearest vertex of
// its protein's surface, alone (the vertices of its own side) and in complex (the vertices of both sides), in one device
// pass.  A vertex is the van-der-Waals contact point x_i + r_i * u_k of a sphere point that the Shrake-Rupley rule of
// eqd_dock_sasa_* leaves exposed under the probe - the contact patch of the solvent-excluded surface; re-entrant patches are
// not modelled (this is not MSMS).
//   exposure   R_i = (double)r_i + probe, q = x_i + R_i * u_k, buried by j != i when (dx dx + dy dy) + dz dz < R_j R_j, d = q - x_j
//   vertex     v_ik = x_i + (double)r_i * u_k (one multiply, one add per component)
//   s(j)       min over the vertices of the state of (dx dx + dy dy) + dz dz, d = x_j - v_ik;  depth = sqrt(s)
// fp64 from the fp32 rows, -ffp-contract=off.
//
// Work decomposition.  Five launches, whatever C is.  A tile is DP_TILE consecutive rows of ONE side of one complex (rows
// are residue-contiguous, so a tile is spatially compact); the tiles of a complex are its ligand tiles, then its receptor
// tiles.
//   k_dp_masks     one wave per atom, one lane per sphere point, ceil(P / 64) passes - the all-rows walk of k_sa_points:
//                  each lane applies the partner rule (squared centre distance < (R_i + R_j + 1e-6)^2) to one of 64 rows
//                  of a segment, own side first, the kept rows are packed into the wave's LDS rows (an integer slot
//                  counter) and every lane tests its point against them by broadcast reads.  The two exposure bits of
//                  the 64 points of a pass become two 64-bit words by an integer OR over the lanes: mask[atom][state][word].
//                  There is no partner list and therefore no list capacity.
//   k_dp_tiles     one wave per tile: per state the fp64 centre of the atoms that own an exposed vertex (row order), the
//                  reach - max over those atoms of centre distance + r_i - and the vertex count, one owner lane per state
//   k_dp_search    items (tile of target atoms, state), one target atom per lane; the four waves split the vertex tiles
//                  (the target's own tile first, then its side's following tiles, then the other side's).  A wave
//                  stages a tile's centres and radii and DP_WCHUNK mask words per atom in its own LDS rows and walks the
//                  set bits; every lane tests the broadcast vertex against its own atom, the sphere table in LDS.
//                  Before a tile, and before an atom of it with at least DP_ATOM_VOTE vertices, the lanes vote on the
//                  skip bound: (centre distance - reach - 1e-6)^2 >= running minimum, written without a square root per
//                  test as centre distance^2 >= (sqrt(minimum at the tile's start) + reach + 1e-6)^2.  The four waves'
//                  minima are combined through LDS - a minimum, so the order is free.
//   k_dp_residues  one thread per residue: its atoms' depths in row order, its CA row's depths, whether an atom deepened
//   k_dp_finish    one workgroup per complex: the atom terms of DP_ROWS rows at a time into LDS, then threads 0-4 each own
//                  one running sum or maximum in row order, ligand before receptor; integer totals by thread-strided
//                  sums and an integer shuffle reduction
// A minimum does not depend on the order of its terms and a skipped group holds no vertex below the running minimum, so
// s is the same whatever the decomposition and with pruning on or off; no wave reads another wave's running minimum, so
// the count of skipped groups depends only on the complex's own tiles; every floating-point sum has one owner and a
// fixed order: a complex's results are bit-identical alone, in any batch, at any position and from run to run.
#include "../csrc/eqd_common.h"
#include "../../include/equidock_dock.h"

#include <math.h>
#include <vector>

#define DP_TILE 64          // rows per tile (one target atom per lane; one staged vertex atom per lane)
#define DP_SEG 64           // rows a wave of the mask kernel looks at per step
#define DP_STEP 16          // partners between two "is any point still exposed" reductions
#define DP_WCHUNK 4         // mask words per atom a wave of the search stages at a time (256 sphere points)
#define DP_LDS_POINTS 256   // sphere points held in LDS by the search (points beyond are read from global memory)
#define DP_ATOM_VOTE 4      // vertices an atom needs before the lanes vote on passing over it
#define DP_ROWS 256         // atom rows per step of the finish kernel
#define DP_MAX_POINTS EQD_DOCK_SASA_MAX_POINTS
#define DP_SKIP_MARGIN 1e-6

static_assert(DP_TILE == 64 && DP_SEG == 64, "one row per lane");
static_assert(DP_TILE % EQD_WAVES == 0, "mask kernel: one wave per atom, EQD_WAVES atoms per workgroup");
static_assert(DP_ROWS == EQD_BLOCK, "finish kernel: one row per thread and step");
static_assert(DP_LDS_POINTS == DP_WCHUNK * 64, "the first chunk of mask words is the LDS part of the sphere table");

struct DepthDesc {          // one complex of the batch (entry C: the totals)
    int32_t la0, nla, ra0, nra;     // atom rows
    int32_t lr0, nlr, rr0, nrr;     // residues
    int32_t t0, ntl, ntr;           // first tile, ligand tiles, receptor tiles
    int32_t a0;                     // first row of the complex in the per-atom workspace arrays (= la0 + ra0)
};

struct DepthWs {
    const DepthDesc* desc;          // [C + 1]
    unsigned long long* mask;       // [A_l + A_r][2][ceil(P / 64)] exposed points: alone, in complex
    double* tb;                     // [T][2][4] per tile and state: centre of the atoms that own a vertex, reach
    int32_t* tc;                    // [T][2] vertices
    int32_t* skip;                  // [T][2] vertex groups the search item passed over
    int32_t* dl;                    // [R_l] 1 when an atom of the ligand residue deepened
    int32_t* dr;                    // [R_r]
};

// the complex that owns tile / residue `v`: the largest c with base(c) <= v (kind 0 tiles, 1 ligand residues, 2 receptor
// residues; the bases are strictly increasing)
template <int kKind>
__device__ __forceinline__ int dp_find(const DepthDesc* __restrict__ D, int C, int v) {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int b = kKind == 0 ? D[mid].t0 : kKind == 1 ? D[mid].lr0 : D[mid].rr0;
        if (b <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// tile t (0 <= t < ntl + ntr) of complex d: its side, its first row inside that side and its rows
__device__ __forceinline__ void dp_tile(const DepthDesc& d, int t, int& side, int& r0, int& n) {
    side = t >= d.ntl ? 1 : 0;
    r0 = (side ? t - d.ntl : t) * DP_TILE;
    const int ns = side ? d.nra : d.nla;
    n = ns - r0 < DP_TILE ? ns - r0 : DP_TILE;
}

// local row g (0 <= g < nla + nra; ligand rows first) of complex d: centre and radius in fp64
__device__ __forceinline__ void dp_atom(const DepthDesc& d, int g, const float* __restrict__ lig,
                                        const float* __restrict__ rec, const float* __restrict__ lrad,
                                        const float* __restrict__ rrad, double& x, double& y, double& z, double& r) {
    const bool l = g < d.nla;
    const size_t row = l ? (size_t)d.la0 + g : (size_t)d.ra0 + (g - d.nla);
    const float* __restrict__ p = (l ? lig : rec) + row * 3;
    x = (double)p[0];
    y = (double)p[1];
    z = (double)p[2];
    r = (double)(l ? lrad : rrad)[row];
}

// atom rows [a0, a1) of residue g, held inside its complex's rows [lo, hi) whatever the table says
__device__ __forceinline__ void dp_range(const int32_t* __restrict__ first, int g, int lo, int hi, int& a0, int& a1) {
    a0 = first[g];
    a1 = first[g + 1];
    a0 = a0 < lo ? lo : (a0 > hi ? hi : a0);
    a1 = a1 < a0 ? a0 : (a1 > hi ? hi : a1);
}

// (wave-uniform) whether `v` is non-zero on any lane: an integer OR over the lanes
__device__ __forceinline__ int dp_any(int v) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) v |= __shfl_xor(v, k);
    return v;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dp_masks(int C, const float* __restrict__ lig, const float* __restrict__ rec,
                                                        const float* __restrict__ lrad, const float* __restrict__ rrad,
                                                        const double* __restrict__ sphere, int P, double probe, DepthWs W) {
    __shared__ double sx[EQD_WAVES][DP_SEG], sy[EQD_WAVES][DP_SEG], sz[EQD_WAVES][DP_SEG], sq[EQD_WAVES][DP_SEG];
    __shared__ int32_t kc[EQD_WAVES];                           // partners a wave has kept
    const int per_tile = DP_TILE / EQD_WAVES;                  // workgroups per tile of atoms
    const int T = blockIdx.x / per_tile;
    if (T >= W.desc[C].t0) return;
    const DepthDesc d = W.desc[dp_find<0>(W.desc, C, T)];
    const int n = d.nla + d.nra, nw = (P + 63) >> 6;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int side, r0, nt;
    dp_tile(d, T - d.t0, side, r0, nt);
    const int rt = (blockIdx.x % per_tile) * EQD_WAVES + w;
    if (rt >= nt) return;                                       // (the whole wave; this kernel has no workgroup barrier)
    const int g = (side ? d.nla : 0) + r0 + rt;
    double xi, yi, zi, ri;
    dp_atom(d, g, lig, rec, lrad, rrad, xi, yi, zi, ri);
    const double Ri = ri + probe;
    const int own0 = side ? d.nla : 0, own_n = side ? d.nra : d.nla;
    const int oth0 = side ? 0 : d.nla, oth_n = side ? d.nla : d.nra;
    unsigned long long* __restrict__ M = W.mask + ((size_t)d.a0 + g) * 2 * nw;
    int kbase = 0;
    if (lane == 0) kc[w] = 0;                                   // (ordered before its first use by the fence below)
    for (int p0 = 0; p0 < P; p0 += 64) {
        const bool ok = p0 + lane < P;
        const double* __restrict__ u = sphere + (size_t)(ok ? p0 + lane : P - 1) * 3;
        const double qx = xi + Ri * u[0], qy = yi + Ri * u[1], qz = zi + Ri * u[2];
        int ea = ok ? 1 : 0, ec = ea;                           // the point is exposed alone / in complex
        for (int phase = 0; phase < 2; ++phase) {
            const int m_all = phase ? oth_n : own_n;
            bool live = true;
            int since = DP_STEP;                                // partners tested since the last "any point exposed" look
            for (int s0 = 0; s0 < m_all && live; s0 += DP_SEG) {
                const int m = m_all - s0 < DP_SEG ? m_all - s0 : DP_SEG;
                wave_lds_fence();                               // the previous segment has been read
                if (lane < m) {
                    int j = (phase ? oth0 : own0) + s0 + lane;
                    j = j < 0 ? 0 : (j >= n ? n - 1 : j);
                    double x, y, z, r;
                    dp_atom(d, j, lig, rec, lrad, rrad, x, y, z, r);
                    const double R = r + probe;
                    const double dx = xi - x, dy = yi - y, dz = zi - z;
                    const double reach = (Ri + R) + DP_SKIP_MARGIN;
                    if (j != g && (dx * dx + dy * dy) + dz * dz < reach * reach) {
                        const int slot = atomicAdd(&kc[w], 1) - kbase;     // (an integer slot counter: order is free)
                        sx[w][slot] = x;
                        sy[w][slot] = y;
                        sz[w][slot] = z;
                        sq[w][slot] = R * R;
                    }
                }
                wave_lds_fence();
                const int mk = kc[w] - kbase;                   // (wave-uniform)
                kbase += mk;
                for (int b0 = 0; b0 < mk; b0 += DP_STEP) {
                    const int b1 = b0 + DP_STEP < mk ? b0 + DP_STEP : mk;
                    if (since >= DP_STEP) {
                        since = 0;
                        if (!dp_any(phase ? ec : ea)) {         // (wave-uniform) no point is left to bury in this phase
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
        // the 64 exposure bits of the pass as two 32-bit halves per state (integers: the order changes nothing)
        const int bit = (int)(1u << (lane & 31));
        int a_lo = ea && lane < 32 ? bit : 0, a_hi = ea && lane >= 32 ? bit : 0;
        int c_lo = ec && lane < 32 ? bit : 0, c_hi = ec && lane >= 32 ? bit : 0;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            a_lo |= __shfl_xor(a_lo, k);
            a_hi |= __shfl_xor(a_hi, k);
            c_lo |= __shfl_xor(c_lo, k);
            c_hi |= __shfl_xor(c_hi, k);
        }
        if (lane == 0) {
            M[p0 >> 6] = ((unsigned long long)(unsigned)a_hi << 32) | (unsigned long long)(unsigned)a_lo;
            M[nw + (p0 >> 6)] = ((unsigned long long)(unsigned)c_hi << 32) | (unsigned long long)(unsigned)c_lo;
        }
    }
}

__global__ __launch_bounds__(DP_TILE) void k_dp_tiles(int C, const float* __restrict__ lig, const float* __restrict__ rec,
                                                      const float* __restrict__ lrad, const float* __restrict__ rrad, int P,
                                                      DepthWs W) {
    __shared__ double ax[DP_TILE], ay[DP_TILE], az[DP_TILE], ar[DP_TILE], ae[2][DP_TILE], cen[2][3];
    __shared__ int32_t nv[2][DP_TILE];
    const int T = blockIdx.x, lane = threadIdx.x;
    if (T >= W.desc[C].t0) return;
    const DepthDesc d = W.desc[dp_find<0>(W.desc, C, T)];
    const int nw = (P + 63) >> 6;
    int side, r0, nt;
    dp_tile(d, T - d.t0, side, r0, nt);
    nv[0][lane] = 0;
    nv[1][lane] = 0;
    if (lane < nt) {
        const int g = (side ? d.nla : 0) + r0 + lane;
        dp_atom(d, g, lig, rec, lrad, rrad, ax[lane], ay[lane], az[lane], ar[lane]);
        const unsigned long long* __restrict__ M = W.mask + ((size_t)d.a0 + g) * 2 * nw;
        int na = 0, nc = 0;
        for (int q = 0; q < nw; ++q) {
            na += __popcll(M[q]);
            nc += __popcll(M[nw + q]);
        }
        nv[0][lane] = na;
        nv[1][lane] = nc;
    }
    __syncthreads();
    if (lane < 2) {                                             // one owner per state: row order
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int m = 0, tot = 0;
        for (int a = 0; a < nt; ++a) {
            if (nv[lane][a] == 0) continue;
            sx += ax[a];
            sy += ay[a];
            sz += az[a];
            m += 1;
            tot += nv[lane][a];
        }
        const double dm = (double)(m > 0 ? m : 1);
        cen[lane][0] = sx / dm;
        cen[lane][1] = sy / dm;
        cen[lane][2] = sz / dm;
        W.tc[(size_t)T * 2 + lane] = tot;
    }
    __syncthreads();
    if (lane < nt) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double dx = ax[lane] - cen[s][0], dy = ay[lane] - cen[s][1], dz = az[lane] - cen[s][2];
            ae[s][lane] = nv[s][lane] ? sqrt((dx * dx + dy * dy) + dz * dz) + ar[lane] : 0.0;
        }
    }
    __syncthreads();
    if (lane < 2) {
        double reach = 0.0;
        for (int a = 0; a < nt; ++a) reach = ae[lane][a] > reach ? ae[lane][a] : reach;
        double* __restrict__ o = W.tb + ((size_t)T * 2 + lane) * 4;
        o[0] = cen[lane][0];
        o[1] = cen[lane][1];
        o[2] = cen[lane][2];
        o[3] = reach;
    }
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dp_search(int C, const float* __restrict__ lig, const float* __restrict__ rec,
                                                         const float* __restrict__ lrad, const float* __restrict__ rrad,
                                                         const double* __restrict__ sphere, int P, int prune,
                                                         double* __restrict__ lig_depth, double* __restrict__ rec_depth,
                                                         DepthWs W) {
    __shared__ double su[DP_LDS_POINTS * 3];
    __shared__ double vx[EQD_WAVES][DP_TILE], vy[EQD_WAVES][DP_TILE], vz[EQD_WAVES][DP_TILE], vr[EQD_WAVES][DP_TILE];
    __shared__ unsigned long long vm[EQD_WAVES][DP_TILE * DP_WCHUNK];
    __shared__ double red[EQD_WAVES][DP_TILE];
    __shared__ int32_t rsk[EQD_WAVES];
    const int T = blockIdx.x >> 1, state = blockIdx.x & 1;
    if (T >= W.desc[C].t0) return;
    const DepthDesc d = W.desc[dp_find<0>(W.desc, C, T)];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int nw = (P + 63) >> 6;
    const int n_lds = (P < DP_LDS_POINTS ? P : DP_LDS_POINTS) * 3;
    for (int e = tid; e < n_lds; e += EQD_BLOCK) su[e] = sphere[e];
    __syncthreads();
    int side, r0, nt;
    dp_tile(d, T - d.t0, side, r0, nt);
    const bool valid = lane < nt;
    const int gj = (side ? d.nla : 0) + r0 + (valid ? lane : 0);
    double xj, yj, zj, rj;
    dp_atom(d, gj, lig, rec, lrad, rrad, xj, yj, zj, rj);
    // the vertex tiles of the item: the target's own tile, its side's following tiles (cyclic), then - in complex - the
    // other side's
    const int own_n = side ? d.ntr : d.ntl, own_b = side ? d.ntl : 0, own_i = T - d.t0 - own_b;
    const int oth_n = state ? (side ? d.ntl : d.ntr) : 0, oth_b = side ? 0 : d.ntl;
    double smin = (double)INFINITY;
    int nskip = 0;
    for (int k = w; k < own_n + oth_n; k += EQD_WAVES) {       // (wave-uniform, like everything but the lane's own atom)
        const int vt = k < own_n ? own_b + (own_i + k) % own_n : oth_b + (k - own_n);
        const size_t VT = (size_t)d.t0 + vt;
        if (W.tc[VT * 2 + state] == 0) continue;               // a tile without vertices is never visited
        double dcur = 0.0;
        if (prune) {
            // no vertex of the tile is nearer than (centre distance - reach); with dcur = sqrt(smin):
            // centre distance >= dcur + reach + 1e-6 proves that none of them is below the running minimum
            const double* __restrict__ b = W.tb + (VT * 2 + state) * 4;
            dcur = sqrt(smin);
            const double ex = xj - b[0], ey = yj - b[1], ez = zj - b[2];
            const double far = (dcur + b[3]) + DP_SKIP_MARGIN;
            const int can = valid && !((ex * ex + ey * ey) + ez * ez >= far * far) ? 1 : 0;
            if (!dp_any(can)) {
                ++nskip;
                continue;
            }
        }
        int vside, vr0, vn;
        dp_tile(d, vt, vside, vr0, vn);
        const int vg0 = (vside ? d.nla : 0) + vr0;
        wave_lds_fence();                                       // the previous tile has been read
        if (lane < vn) dp_atom(d, vg0 + lane, lig, rec, lrad, rrad, vx[w][lane], vy[w][lane], vz[w][lane], vr[w][lane]);
        for (int wc = 0; wc < nw; wc += DP_WCHUNK) {
            const int cw = nw - wc < DP_WCHUNK ? nw - wc : DP_WCHUNK;
            if (wc) wave_lds_fence();                           // the previous chunk of words has been read
            if (lane < vn) {
                const unsigned long long* __restrict__ M = W.mask + (((size_t)d.a0 + vg0 + lane) * 2 + state) * nw + wc;
                for (int q = 0; q < cw; ++q) vm[w][lane * DP_WCHUNK + q] = M[q];
            }
            wave_lds_fence();
            for (int a = 0; a < vn; ++a) {
                int nb = 0;
                for (int q = 0; q < cw; ++q) nb += __popcll(vm[w][a * DP_WCHUNK + q]);
                if (nb == 0) continue;
                const double ax = vx[w][a], ay = vy[w][a], az = vz[w][a], ar = vr[w][a];
                if (prune && nb >= DP_ATOM_VOTE) {              // the atom's vertices lie within ar of its centre
                    const double ex = xj - ax, ey = yj - ay, ez = zj - az;
                    const double far = (dcur + ar) + DP_SKIP_MARGIN;
                    const int can = valid && !((ex * ex + ey * ey) + ez * ez >= far * far) ? 1 : 0;
                    if (!dp_any(can)) {
                        ++nskip;
                        continue;
                    }
                }
                for (int q = 0; q < cw; ++q) {
                    unsigned long long m = vm[w][a * DP_WCHUNK + q];
                    while (m) {
                        const int kk = (wc + q) * 64 + __builtin_ctzll(m);
                        m &= m - 1;
                        double ux, uy, uz;
                        if (kk < DP_LDS_POINTS) {
                            ux = su[kk * 3];
                            uy = su[kk * 3 + 1];
                            uz = su[kk * 3 + 2];
                        } else {
                            ux = sphere[(size_t)kk * 3];
                            uy = sphere[(size_t)kk * 3 + 1];
                            uz = sphere[(size_t)kk * 3 + 2];
                        }
                        const double px = ax + ar * ux, py = ay + ar * uy, pz = az + ar * uz;
                        const double dx = xj - px, dy = yj - py, dz = zj - pz;
                        const double s = (dx * dx + dy * dy) + dz * dz;
                        smin = s < smin ? s : smin;
                    }
                }
            }
        }
    }
    red[w][lane] = smin;
    if (lane == 0) rsk[w] = nskip;
    __syncthreads();
    if (tid < DP_TILE) {
        const double a = red[0][tid] < red[1][tid] ? red[0][tid] : red[1][tid];
        const double b = red[2][tid] < red[3][tid] ? red[2][tid] : red[3][tid];
        const double s = a < b ? a : b;
        if (valid) {
            double* __restrict__ o = side ? rec_depth + ((size_t)d.ra0 + r0 + tid) * 4 : lig_depth + ((size_t)d.la0 + r0 + tid) * 4;
            o[state] = s;
            o[2 + state] = sqrt(s);
        }
        if (tid == 0) W.skip[(size_t)T * 2 + state] = (rsk[0] + rsk[1]) + (rsk[2] + rsk[3]);
    }
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dp_residues(int C, const int32_t* __restrict__ lfirst,
                                                           const int32_t* __restrict__ rfirst,
                                                           const int32_t* __restrict__ lca, const int32_t* __restrict__ rca,
                                                           const double* __restrict__ lig_depth,
                                                           const double* __restrict__ rec_depth,
                                                           double* __restrict__ lig_res_depth,
                                                           double* __restrict__ rec_res_depth, DepthWs W) {
    const int Rl = W.desc[C].lr0, Rr = W.desc[C].rr0;
    int r = blockIdx.x * EQD_BLOCK + threadIdx.x;
    if (r >= Rl + Rr) return;
    const bool l = r < Rl;
    if (!l) r -= Rl;
    const DepthDesc d = W.desc[l ? dp_find<1>(W.desc, C, r) : dp_find<2>(W.desc, C, r)];
    const int lo = l ? d.la0 : d.ra0, hi = lo + (l ? d.nla : d.nra);
    int a0, a1;
    dp_range(l ? lfirst : rfirst, r, lo, hi, a0, a1);
    const double* __restrict__ dep = l ? lig_depth : rec_depth;
    double alone = 0.0, cplx = 0.0;
    int deep = 0;
    for (int a = a0; a < a1; ++a) {
        const double* __restrict__ p = dep + (size_t)a * 4;
        alone += p[2];
        cplx += p[3];
        deep |= p[1] > p[0] ? 1 : 0;
    }
    const double na = (double)(a1 - a0);
    const int ca = (l ? lca : rca)[r];
    const bool has_ca = ca >= lo && ca < hi;                    // (a row outside the residue's own complex and side: none)
    double* __restrict__ o = (l ? lig_res_depth : rec_res_depth) + (size_t)r * 4;
    o[0] = alone / na;
    o[1] = cplx / na;
    o[2] = has_ca ? dep[(size_t)ca * 4 + 2] : (double)NAN;
    o[3] = has_ca ? dep[(size_t)ca * 4 + 3] : (double)NAN;
    (l ? W.dl : W.dr)[r] = deep;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dp_finish(int C, const double* __restrict__ lig_depth,
                                                         const double* __restrict__ rec_depth, double* __restrict__ rows,
                                                         DepthWs W) {
    __shared__ double t[3][DP_ROWS];                            // the terms of DP_ROWS rows: alone, in complex, the gain
    __shared__ int32_t red[EQD_WAVES][8];
    const int c = blockIdx.x;
    if (c >= C) return;
    const DepthDesc d = W.desc[c];
    const int tid = threadIdx.x;
    // threads 0-4 each own one running value, taken in row order: 0 the side's sum of depths alone, 1 the sum of depths
    // in complex, 2 the side's sum of gains, 3 the side's largest depth alone, 4 the largest depth in complex (0, 2 and 3
    // start again at the receptor)
    const double* __restrict__ mine = t[tid < 3 ? tid : (tid == 3 ? 0 : 1)];
    const bool is_max = tid >= 3;
    double acc = 0.0, kept[2] = {0.0, 0.0};
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};                        // deepened atoms l / r, residues l / r, vertices alone l / r, in complex, skipped
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int cnt = side ? d.nra : d.nla;
        const double* __restrict__ dep = side ? rec_depth + (size_t)d.ra0 * 4 : lig_depth + (size_t)d.la0 * 4;
        for (int r0 = 0; r0 < cnt; r0 += DP_ROWS) {
            const int m = cnt - r0 < DP_ROWS ? cnt - r0 : DP_ROWS;
            if (tid < m) {
                const double* __restrict__ p = dep + (size_t)(r0 + tid) * 4;
                t[0][tid] = p[2];
                t[1][tid] = p[3];
                t[2][tid] = p[3] - p[2];
                v[side] += p[1] > p[0] ? 1 : 0;
            }
            __syncthreads();
            if (tid < 5) {
                if (is_max) {
#pragma unroll 16
                    for (int k = 0; k < m; ++k) acc = mine[k] > acc ? mine[k] : acc;
                } else {
#pragma unroll 16
                    for (int k = 0; k < m; ++k) acc += mine[k];            // row order
                }
            }
            __syncthreads();
        }
        kept[side] = acc;
        if (tid == 0 || tid == 2 || tid == 3) acc = 0.0;
        const int32_t* __restrict__ flag = side ? W.dr + d.rr0 : W.dl + d.lr0;
        const int nr = side ? d.nrr : d.nlr;
        for (int r = tid; r < nr; r += EQD_BLOCK) v[2 + side] += flag[r] ? 1 : 0;
        const int tb = d.t0 + (side ? d.ntl : 0), ntile = side ? d.ntr : d.ntl;
        for (int q = tid; q < ntile; q += EQD_BLOCK) {
            v[4 + side] += W.tc[(size_t)(tb + q) * 2];
            v[6] += W.tc[(size_t)(tb + q) * 2 + 1];
            v[7] += W.skip[(size_t)(tb + q) * 2] + W.skip[(size_t)(tb + q) * 2 + 1];
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v[k] += __shfl_xor(v[k], m);       // (integers: the order changes nothing)
        if ((tid & 63) == 0) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    double* __restrict__ o = rows + (size_t)c * EQD_DOCK_DEPTH_COLS;
    const double nl = (double)d.nla, nr = (double)d.nra;
    if (tid == 0) {
        o[0] = kept[0] / nl;
        o[1] = kept[1] / nr;
    } else if (tid == 1) {
        o[2] = kept[1] / (double)(d.nla + d.nra);
    } else if (tid == 2) {
        o[6] = kept[0] / nl;
        o[7] = kept[1] / nr;
    } else if (tid == 3) {
        o[3] = kept[0];
        o[4] = kept[1];
    } else if (tid == 4) {
        o[5] = kept[1];
    } else if (tid == 64) {
        int s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        o[8] = (double)s[0];
        o[9] = (double)s[1];
        o[10] = (double)s[2];
        o[11] = (double)s[3];
        o[12] = (double)(s[4] + s[5]);
        o[13] = (double)s[6];
        o[14] = (double)s[7];
        o[15] = (double)((s[4] == 0 ? EQD_DOCK_DEPTH_FLAG_NO_LIGAND_VERTEX : 0) |
                         (s[5] == 0 ? EQD_DOCK_DEPTH_FLAG_NO_RECEPTOR_VERTEX : 0) |
                         (s[6] == 0 ? EQD_DOCK_DEPTH_FLAG_NO_COMPLEX_VERTEX : 0));
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
static int dp_cdiv(int a, int b) { return (a + b - 1) / b; }

// validated tile table of a batch (+ entry C with the totals); returns EQD_OK or an error code with the message set
static int dp_plan(const char* fn, int C, const int32_t* lao, const int32_t* rao, const int32_t* lro, const int32_t* rro,
                   int P, std::vector<DepthDesc>& D) {
    if (!lao || !rao || !lro || !rro) {
        eqd_set_error("%s: NULL offsets", fn);
        return EQD_ERR_NULL;
    }
    if (C < 1) {
        eqd_set_error("%s: n_complex = %d (need >= 1)", fn, C);
        return EQD_ERR_SHAPE;
    }
    if (P < 1 || P > DP_MAX_POINTS) {
        eqd_set_error("%s: n_points = %d (need 1..%d)", fn, P, DP_MAX_POINTS);
        return EQD_ERR_SHAPE;
    }
    if (lao[0] != 0 || rao[0] != 0 || lro[0] != 0 || rro[0] != 0) {
        eqd_set_error("%s: lig_atom_off[0] = %d, rec_atom_off[0] = %d, lig_res_off[0] = %d, rec_res_off[0] = %d (need 0)", fn,
                      lao[0], rao[0], lro[0], rro[0]);
        return EQD_ERR_SHAPE;
    }
    D.assign((size_t)C + 1, DepthDesc{});
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
        if (nla + nra > INT32_MAX - DP_ROWS || ((int64_t)lao[c + 1] + rao[c + 1]) * 4 > INT32_MAX) {
            eqd_set_error("%s: %lld ligand and %lld receptor atoms up to complex %d do not fit 32-bit offsets (split the "
                          "batch)", fn, (long long)lao[c + 1], (long long)rao[c + 1], c);
            return EQD_ERR_SHAPE;
        }
        DepthDesc& d = D[c];
        d.la0 = lao[c]; d.nla = (int32_t)nla; d.ra0 = rao[c]; d.nra = (int32_t)nra;
        d.lr0 = lro[c]; d.nlr = (int32_t)nlr; d.rr0 = rro[c]; d.nrr = (int32_t)nrr;
        d.ntl = dp_cdiv(d.nla, DP_TILE);
        d.ntr = dp_cdiv(d.nra, DP_TILE);
        d.t0 = (int32_t)tile;
        d.a0 = d.la0 + d.ra0;
        tile += d.ntl + d.ntr;
        if (tile * (DP_TILE / EQD_WAVES) > INT32_MAX) {
            eqd_set_error("%s: %lld atom tiles up to complex %d do not fit a launch (split the batch)", fn, (long long)tile, c);
            return EQD_ERR_SHAPE;
        }
    }
    DepthDesc& e = D[C];
    e.la0 = lao[C]; e.ra0 = rao[C]; e.lr0 = lro[C]; e.rr0 = rro[C];
    e.t0 = (int32_t)tile;
    e.a0 = e.la0 + e.ra0;
    return EQD_OK;
}

static size_t dp_carve(int C, int P, const std::vector<DepthDesc>& D, EqdArena& A, DepthWs* W) {
    const DepthDesc& e = D[C];
    DepthWs w;
    w.desc = A.take<DepthDesc>((size_t)C + 1);
    w.mask = A.take<unsigned long long>((size_t)e.a0 * 2 * (size_t)((P + 63) / 64));
    w.tb = A.take<double>((size_t)e.t0 * 8);
    w.tc = A.take<int32_t>((size_t)e.t0 * 2);
    w.skip = A.take<int32_t>((size_t)e.t0 * 2);
    w.dl = A.take<int32_t>((size_t)e.lr0);
    w.dr = A.take<int32_t>((size_t)e.rr0);
    if (W) *W = w;
    return A.off;
}

// plan + carve of a call on a workspace
static int dp_open(const char* fn, int C, const int32_t* lao, const int32_t* rao, const int32_t* lro, const int32_t* rro,
                   int P, void* workspace, size_t ws_bytes, std::vector<DepthDesc>& D, DepthWs* W) {
    if (!workspace) {
        eqd_set_error("%s: NULL workspace", fn);
        return EQD_ERR_NULL;
    }
    if (int rc = dp_plan(fn, C, lao, rao, lro, rro, P, D)) return rc;
    EqdArena A(workspace, ws_bytes);
    dp_carve(C, P, D, A, W);
    if (!A.ok) {
        eqd_set_error("%s: workspace too small (%zu needed, %zu given)", fn, A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_depth_abi(void) { return EQD_DOCK_DEPTH_ABI; }

extern "C" EQD_DOCK_API size_t eqd_dock_depth_workspace_bytes(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                              const int32_t* lig_res_off, const int32_t* rec_res_off,
                                                              int n_points) {
    std::vector<DepthDesc> D;
    if (dp_plan("eqd_dock_depth_workspace_bytes", C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, n_points, D) != EQD_OK)
        return 0;
    EqdArena A(nullptr, 0);
    return dp_carve(C, n_points, D, A, nullptr) + 256;
}

extern "C" EQD_DOCK_API int eqd_dock_depth_init(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                const int32_t* lig_res_off, const int32_t* rec_res_off, int n_points,
                                                void* workspace, size_t ws_bytes, void* stream) {
    std::vector<DepthDesc> D;
    DepthWs W;
    if (int rc = dp_open("eqd_dock_depth_init", C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, n_points, workspace,
                         ws_bytes, D, &W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync((void*)W.desc, D.data(), sizeof(DepthDesc) * D.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        eqd_set_error("eqd_dock_depth_init: copy failed");
        return EQD_ERR_LAUNCH;
    }
#ifndef EQD_HOSTSIM
    if (hipStreamSynchronize(s) != hipSuccess) {      // `D` is a local host buffer
        eqd_set_error("eqd_dock_depth_init: stream synchronisation failed");
        return EQD_ERR_LAUNCH;
    }
#endif
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_depth_eval(int C, const int32_t* lig_atom_off, const int32_t* rec_atom_off,
                                                const int32_t* lig_res_off, const int32_t* rec_res_off, const float* lig,
                                                const float* rec, const float* lig_radius, const float* rec_radius,
                                                const int32_t* lig_res_first, const int32_t* rec_res_first,
                                                const int32_t* lig_res_ca, const int32_t* rec_res_ca, const double* sphere,
                                                int n_points, double probe, int prune, double* lig_depth, double* rec_depth,
                                                double* lig_res_depth, double* rec_res_depth, double* rows, void* workspace,
                                                size_t ws_bytes, void* stream) {
    const char* fn = "eqd_dock_depth_eval";
    if (!lig || !rec || !lig_radius || !rec_radius || !lig_res_first || !rec_res_first || !lig_res_ca || !rec_res_ca ||
        !sphere || !lig_depth || !rec_depth || !lig_res_depth || !rec_res_depth || !rows) {
        eqd_set_error("%s: NULL argument", fn);
        return EQD_ERR_NULL;
    }
    if (!(probe > 0.0) || !(probe < (double)INFINITY)) {
        eqd_set_error("%s: probe = %g (need a finite value > 0)", fn, probe);
        return EQD_ERR_SHAPE;
    }
    std::vector<DepthDesc> D;
    DepthWs W;
    if (int rc = dp_open(fn, C, lig_atom_off, rec_atom_off, lig_res_off, rec_res_off, n_points, workspace, ws_bytes, D, &W))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const unsigned n_tile = (unsigned)D[C].t0, n_res = (unsigned)D[C].lr0 + (unsigned)D[C].rr0;
    hipLaunchKernelGGL(k_dp_masks, dim3(n_tile * (DP_TILE / EQD_WAVES)), dim3(EQD_BLOCK), 0, s, C, lig, rec, lig_radius,
                       rec_radius, sphere, n_points, probe, W);
    if (int rc = eqd_check_launch("k_dp_masks")) return rc;
    hipLaunchKernelGGL(k_dp_tiles, dim3(n_tile), dim3(DP_TILE), 0, s, C, lig, rec, lig_radius, rec_radius, n_points, W);
    if (int rc = eqd_check_launch("k_dp_tiles")) return rc;
    hipLaunchKernelGGL(k_dp_search, dim3(n_tile * 2), dim3(EQD_BLOCK), 0, s, C, lig, rec, lig_radius, rec_radius, sphere,
                       n_points, prune ? 1 : 0, lig_depth, rec_depth, W);
    if (int rc = eqd_check_launch("k_dp_search")) return rc;
    hipLaunchKernelGGL(k_dp_residues, dim3((n_res + EQD_BLOCK - 1) / EQD_BLOCK), dim3(EQD_BLOCK), 0, s, C, lig_res_first,
                       rec_res_first, lig_res_ca, rec_res_ca, lig_depth, rec_depth, lig_res_depth, rec_res_depth, W);
    if (int rc = eqd_check_launch("k_dp_residues")) return rc;
    hipLaunchKernelGGL(k_dp_finish, dim3((unsigned)C), dim3(EQD_BLOCK), 0, s, C, lig_depth, rec_depth, rows, W);
    return eqd_check_launch("k_dp_finish");
}

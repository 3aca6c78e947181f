// Batched RMSD meter (include/equidock_dock.h): Meter_Unbound_Bound.update_rmsd of the reference (src/utils/eval.py:12-36)
// and the CRMSD / IRMSD of src/test_all_methods/eval_pdb_outputset.py:80-100 for C complexes in one device pass.
//   ligand / receptor RMSD   sqrt(mean |p - t|^2), no alignment
//   complex RMSD             Kabsch over the concatenated n_l + n_r rows (src/utils/protein_utils.py:31-64):
//                            H = (P - c_P)^T (T - c_T) = U S V^T, R = V U^T (third column of V negated when det R < 0),
//                            b = c_T - R c_P, RMSD of R p + b - t
//   interface RMSD           the same over the pair list {(i, j): |lig_true_i - rec_true_j| < cutoff}, in which a row
//                            appears once per partner: the weighted Kabsch RMSD with the integer weights
//                            w_i = #{j : d_ij < cutoff} (ligand rows), w_j = #{i : d_ij < cutoff} (receptor rows)
// All arithmetic is fp64 from the fp32 inputs, -ffp-contract=off.
//
// Work decomposition.  Five launches, whatever C is (four without the interface):
//   k_dm_counts     items (complex, side, tile of 256 rows): one row per thread against ALL partners of the other side,
//                   staged in LDS 512 at a time; d2 = (dx dx + dy dy) + dz dz, sqrt(d2) < cutoff (the operation order of
//                   scipy's cdist and of inference.complex_and_interface_rmsd).  A row's count is written once, by its
//                   own thread: no atomics, nothing to zero.
//   k_dm_moments    items (complex, tile of 256 rows of the concatenated ligand + receptor rows): for the plain set
//                   (w = 1) and the interface set (w = count) sum w, sum w p, sum w t, sum w p t^T, and sum |p - t|^2 of
//                   the ligand rows and of the receptor rows -> 34 doubles in the item's own slot.  Every coordinate is
//                   taken relative to the complex's first lig_true row (PDB frames are not centred).
//   k_dm_solve      one thread per (complex, set): the slots in tile order, centroids, H, a 3 x 3 one-sided Jacobi SVD,
//                   the proper rotation that maps the two leading left singular vectors onto the right ones, b, flags
//   k_dm_residuals  items as in k_dm_moments: sum w |R p + b - t|^2 for both sets (an explicit second pass: the closed
//                   form G_P + G_T - 2 sum s cancels to nothing for an exact prediction)
//   k_dm_finish     one thread per complex: the slots in tile order -> metrics[c][8]
// The item table depends only on each complex's own sizes, every partial has its own slot, the slots are combined in
// item order and the block sums are fixed butterflies: a complex's row of results is bit-identical alone, in any batch,
// at any position and from run to run.  The only cross-lane traffic is __shfl_xor on int halves of a double.
#include "../csrc/eqd_common.h"
#include "../../include/equidock_dock.h"
#include "eqd_dock_kabsch.h"

#include <math.h>
#include <vector>

#define DM_ROWS EQD_BLOCK   // rows per work item (one per thread)
#define DM_CHUNK 512        // partners staged in LDS at a time (6 KiB as three float arrays)
#define DM_NMOM 34          // doubles per moments slot: 2 x (1 + 3 + 3 + 9), ligand and receptor sum |p - t|^2

struct MeterDesc {          // one complex of the batch (entry C: the totals)
    int32_t l0, nl, r0, nr; // row offsets and sizes
    int32_t ntl, ntr;       // count items: ligand tiles, then receptor tiles
    int32_t nt;             // tiles of the concatenated rows (moments / residuals items)
    int32_t cnt_base;       // first k_dm_counts item
    int32_t mom_base;       // first k_dm_moments / k_dm_residuals item
    int32_t pad;
};

struct MeterWs {
    const MeterDesc* desc;  // [C + 1]
    int32_t* wl;            // [sum n_l] interface partners of every ligand row
    int32_t* wr;            // [sum n_r] of every receptor row
    double* mom;            // [items][DM_NMOM]
    double* rb;             // [C][2][DM_NRB]
    double* res;            // [items][2]
    int32_t* flags;         // [C][2] reflection branch taken, per set
};

template <int kMom>
__device__ __forceinline__ int dm_find(const MeterDesc* __restrict__ D, int C, int item) {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int b = kMom ? D[mid].mom_base : D[mid].cnt_base;
        if (b <= item) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dm_counts(int C, const float* __restrict__ lig_true,
                                                         const float* __restrict__ rec_true, double cutoff, MeterWs W) {
    __shared__ float px[DM_CHUNK], py[DM_CHUNK], pz[DM_CHUNK];
    const int item = blockIdx.x;
    if (item >= W.desc[C].cnt_base) return;
    const int c = dm_find<0>(W.desc, C, item);
    const MeterDesc d = W.desc[c];
    const int q = item - d.cnt_base;
    const bool lig_rows = q < d.ntl;
    const int tile = lig_rows ? q : q - d.ntl;
    const int nrow = lig_rows ? d.nl : d.nr, npart = lig_rows ? d.nr : d.nl;
    const float* __restrict__ rows = lig_rows ? lig_true + (size_t)d.l0 * 3 : rec_true + (size_t)d.r0 * 3;
    const float* __restrict__ part = lig_rows ? rec_true + (size_t)d.r0 * 3 : lig_true + (size_t)d.l0 * 3;
    const int i = tile * DM_ROWS + threadIdx.x;
    const int ic = i < nrow ? i : nrow - 1;
    const double ax = (double)rows[(size_t)ic * 3], ay = (double)rows[(size_t)ic * 3 + 1], az = (double)rows[(size_t)ic * 3 + 2];
    int count = 0;
    for (int k0 = 0; k0 < npart; k0 += DM_CHUNK) {
        const int nc = npart - k0 < DM_CHUNK ? npart - k0 : DM_CHUNK;
        __syncthreads();                                    // the previous chunk has been read
        for (int k = threadIdx.x; k < nc; k += EQD_BLOCK) {
            px[k] = part[(size_t)(k0 + k) * 3];
            py[k] = part[(size_t)(k0 + k) * 3 + 1];
            pz[k] = part[(size_t)(k0 + k) * 3 + 2];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < nc; ++k) {
            const double dx = ax - (double)px[k], dy = ay - (double)py[k], dz = az - (double)pz[k];
            count += sqrt((dx * dx + dy * dy) + dz * dz) < cutoff ? 1 : 0;
        }
    }
    if (i < nrow) (lig_rows ? W.wl + d.l0 : W.wr + d.r0)[i] = count;
}

// row g of complex d's concatenated rows, relative to the complex's first lig_true row; wi: its interface weight
struct DmRow {
    double p[3], t[3];
    double wi;
    bool lig;
};
__device__ __forceinline__ DmRow dm_row(const MeterDesc& d, int g, const float* __restrict__ lig_pred,
                                        const float* __restrict__ rec_pred, const float* __restrict__ lig_true,
                                        const float* __restrict__ rec_true, int interface, const MeterWs& W) {
    DmRow r;
    const float* __restrict__ o = lig_true + (size_t)d.l0 * 3;
    r.lig = g < d.nl;
    const size_t row = r.lig ? (size_t)d.l0 + g : (size_t)d.r0 + (g - d.nl);
    const float* __restrict__ p = (r.lig ? lig_pred : rec_pred) + row * 3;
    const float* __restrict__ t = (r.lig ? lig_true : rec_true) + row * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.p[a] = (double)p[a] - (double)o[a];
        r.t[a] = (double)t[a] - (double)o[a];
    }
    r.wi = interface ? (double)(r.lig ? W.wl : W.wr)[row] : 0.0;
    return r;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dm_moments(int C, const float* __restrict__ lig_pred,
                                                          const float* __restrict__ rec_pred,
                                                          const float* __restrict__ lig_true,
                                                          const float* __restrict__ rec_true, int interface, MeterWs W) {
    __shared__ double red[EQD_WAVES];
    const int item = blockIdx.x;
    if (item >= W.desc[C].mom_base) return;
    const int c = dm_find<1>(W.desc, C, item);
    const MeterDesc d = W.desc[c];
    const int n = d.nl + d.nr;
    const int g = (item - d.mom_base) * DM_ROWS + threadIdx.x;
    const bool valid = g < n;
    const DmRow r = dm_row(d, valid ? g : n - 1, lig_pred, rec_pred, lig_true, rec_true, interface, W);
    double v[DM_NMOM];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double w = !valid ? 0.0 : (s == 0 ? 1.0 : r.wi);
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
    const double ex = r.p[0] - r.t[0], ey = r.p[1] - r.t[1], ez = r.p[2] - r.t[2];
    const double e2 = (ex * ex + ey * ey) + ez * ez;
    v[32] = valid && r.lig ? e2 : 0.0;
    v[33] = valid && !r.lig ? e2 : 0.0;
    double* __restrict__ slot = W.mom + (size_t)item * DM_NMOM;
#pragma unroll
    for (int k = 0; k < DM_NMOM; ++k) {
        const double tot = dm_block_sum(v[k], red);
        if (threadIdx.x == 0) slot[k] = tot;
    }
}

__global__ __launch_bounds__(64) void k_dm_solve(int C, MeterWs W) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    const int c = idx >> 1, set = idx & 1;
    if (c >= C) return;
    const MeterDesc d = W.desc[c];
    double m[16];
    for (int k = 0; k < 16; ++k) m[k] = 0.0;
    for (int t = 0; t < d.nt; ++t) {
        const double* __restrict__ slot = W.mom + (size_t)(d.mom_base + t) * DM_NMOM + 16 * set;
        for (int k = 0; k < 16; ++k) m[k] += slot[k];
    }
    const bool reflect = dm_kabsch(m, W.rb + ((size_t)c * 2 + set) * DM_NRB);
    W.flags[2 * c + set] = reflect ? 1 : 0;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dm_residuals(int C, const float* __restrict__ lig_pred,
                                                            const float* __restrict__ rec_pred,
                                                            const float* __restrict__ lig_true,
                                                            const float* __restrict__ rec_true, int interface, MeterWs W) {
    __shared__ double red[EQD_WAVES];
    const int item = blockIdx.x;
    if (item >= W.desc[C].mom_base) return;
    const int c = dm_find<1>(W.desc, C, item);
    const MeterDesc d = W.desc[c];
    const int n = d.nl + d.nr;
    const int g = (item - d.mom_base) * DM_ROWS + threadIdx.x;
    const bool valid = g < n;
    const DmRow r = dm_row(d, valid ? g : n - 1, lig_pred, rec_pred, lig_true, rec_true, interface, W);
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
        const double w = !valid ? 0.0 : (s == 0 ? 1.0 : r.wi);
        v[s] = w * e2;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double tot = dm_block_sum(v[s], red);
        if (threadIdx.x == 0) W.res[(size_t)item * 2 + s] = tot;
    }
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dm_finish(int C, int interface, double* __restrict__ metrics, MeterWs W) {
    const int c = blockIdx.x * EQD_BLOCK + threadIdx.x;
    if (c >= C) return;
    const MeterDesc d = W.desc[c];
    double e_lig = 0.0, e_rec = 0.0, e_cpx = 0.0, e_int = 0.0, w_int = 0.0;
    for (int t = 0; t < d.nt; ++t) {
        const double* __restrict__ slot = W.mom + (size_t)(d.mom_base + t) * DM_NMOM;
        e_lig += slot[32];
        e_rec += slot[33];
        w_int += slot[16];
        e_cpx += W.res[(size_t)(d.mom_base + t) * 2];
        e_int += W.res[(size_t)(d.mom_base + t) * 2 + 1];
    }
    const int32_t* __restrict__ fb = W.flags + 2 * (size_t)c;
    const bool have = interface && w_int > 0.0;
    double* __restrict__ o = metrics + (size_t)c * EQD_DOCK_METER_COLS;
    o[0] = sqrt(e_lig / (double)d.nl);
    o[1] = sqrt(e_rec / (double)d.nr);
    o[2] = sqrt(e_cpx / (double)(d.nl + d.nr));
    o[3] = have ? sqrt(e_int / w_int) : __builtin_nan("");
    o[4] = have ? w_int * 0.5 : 0.0;                        // every pair weighs once on each side
    o[5] = (double)((fb[0] ? 1 : 0) | (have && fb[1] ? 2 : 0));
    o[6] = 0.0;
    o[7] = 0.0;
}

// ---- host side ------------------------------------------------------------------------------------------------
static int dm_cdiv(int a, int b) { return (a + b - 1) / b; }

// validated item table of a batch (+ entry C with the totals); returns EQD_OK or an error code with the message set
static int dm_plan(const char* fn, int C, const int32_t* lig_off, const int32_t* rec_off, std::vector<MeterDesc>& D) {
    if (!lig_off || !rec_off) {
        eqd_set_error("%s: NULL offsets", fn);
        return EQD_ERR_NULL;
    }
    if (C < 1) {
        eqd_set_error("%s: n_complex = %d (need >= 1)", fn, C);
        return EQD_ERR_SHAPE;
    }
    if (lig_off[0] != 0 || rec_off[0] != 0) {
        eqd_set_error("%s: lig_off[0] = %d, rec_off[0] = %d (need 0)", fn, lig_off[0], rec_off[0]);
        return EQD_ERR_SHAPE;
    }
    D.assign((size_t)C + 1, MeterDesc{});
    int64_t cnt = 0, mom = 0;
    for (int c = 0; c < C; ++c) {
        const int64_t nl = (int64_t)lig_off[c + 1] - lig_off[c], nr = (int64_t)rec_off[c + 1] - rec_off[c];
        if (nl < 1 || nr < 1) {
            eqd_set_error("%s: complex %d has %lld ligand and %lld receptor rows (offsets must increase; every complex "
                          "needs >= 1 row on each side)", fn, c, (long long)nl, (long long)nr);
            return EQD_ERR_SHAPE;
        }
        if (nl + nr > INT32_MAX - DM_ROWS || ((int64_t)lig_off[c + 1] + rec_off[c + 1]) * 3 > INT32_MAX) {
            eqd_set_error("%s: %lld ligand and %lld receptor rows up to complex %d do not fit 32-bit offsets (split the "
                          "batch)", fn, (long long)lig_off[c + 1], (long long)rec_off[c + 1], c);
            return EQD_ERR_SHAPE;
        }
        MeterDesc& d = D[c];
        d.l0 = lig_off[c]; d.nl = (int32_t)nl; d.r0 = rec_off[c]; d.nr = (int32_t)nr;
        d.ntl = dm_cdiv(d.nl, DM_ROWS); d.ntr = dm_cdiv(d.nr, DM_ROWS);
        d.nt = dm_cdiv(d.nl + d.nr, DM_ROWS);
        d.cnt_base = (int32_t)cnt; d.mom_base = (int32_t)mom;
        cnt += d.ntl + d.ntr;
        mom += d.nt;
    }
    MeterDesc& e = D[C];
    e.l0 = lig_off[C]; e.r0 = rec_off[C];
    e.cnt_base = (int32_t)cnt; e.mom_base = (int32_t)mom;
    return EQD_OK;
}

static size_t dm_carve(int C, const std::vector<MeterDesc>& D, EqdArena& A, MeterWs* W) {
    const MeterDesc& e = D[C];
    MeterWs w;
    w.desc = A.take<MeterDesc>((size_t)C + 1);
    w.wl = A.take<int32_t>((size_t)e.l0);
    w.wr = A.take<int32_t>((size_t)e.r0);
    w.mom = A.take<double>((size_t)e.mom_base * DM_NMOM);
    w.rb = A.take<double>((size_t)C * 2 * DM_NRB);
    w.res = A.take<double>((size_t)e.mom_base * 2);
    w.flags = A.take<int32_t>((size_t)C * 2);
    if (W) *W = w;
    return A.off;
}

// plan + carve of a call on a workspace
static int dm_open(const char* fn, int C, const int32_t* lig_off, const int32_t* rec_off, void* workspace,
                   size_t ws_bytes, std::vector<MeterDesc>& D, MeterWs* W) {
    if (!workspace) {
        eqd_set_error("%s: NULL workspace", fn);
        return EQD_ERR_NULL;
    }
    if (int rc = dm_plan(fn, C, lig_off, rec_off, D)) return rc;
    EqdArena A(workspace, ws_bytes);
    dm_carve(C, D, A, W);
    if (!A.ok) {
        eqd_set_error("%s: workspace too small (%zu needed, %zu given)", fn, A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_meter_abi(void) { return EQD_DOCK_METER_ABI; }

extern "C" EQD_DOCK_API size_t eqd_dock_meter_workspace_bytes(int C, const int32_t* lig_off, const int32_t* rec_off) {
    std::vector<MeterDesc> D;
    if (dm_plan("eqd_dock_meter_workspace_bytes", C, lig_off, rec_off, D) != EQD_OK) return 0;
    EqdArena A(nullptr, 0);
    return dm_carve(C, D, A, nullptr) + 256;
}

extern "C" EQD_DOCK_API int eqd_dock_meter_init(int C, const int32_t* lig_off, const int32_t* rec_off, void* workspace,
                                                size_t ws_bytes, void* stream) {
    std::vector<MeterDesc> D;
    MeterWs W;
    if (int rc = dm_open("eqd_dock_meter_init", C, lig_off, rec_off, workspace, ws_bytes, D, &W)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync((void*)W.desc, D.data(), sizeof(MeterDesc) * D.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        eqd_set_error("eqd_dock_meter_init: copy failed");
        return EQD_ERR_LAUNCH;
    }
#ifndef EQD_HOSTSIM
    if (hipStreamSynchronize(s) != hipSuccess) {      // `D` is a local host buffer
        eqd_set_error("eqd_dock_meter_init: stream synchronisation failed");
        return EQD_ERR_LAUNCH;
    }
#endif
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_meter_eval(int C, const int32_t* lig_off, const int32_t* rec_off,
                                                const float* lig_pred, const float* rec_pred, const float* lig_true,
                                                const float* rec_true, double cutoff, int interface, double* metrics,
                                                void* workspace, size_t ws_bytes, void* stream) {
    if (!lig_pred || !lig_true || !rec_true || !metrics) {
        eqd_set_error("eqd_dock_meter_eval: NULL argument");
        return EQD_ERR_NULL;
    }
    if (!(cutoff > 0.0) || !(cutoff < (double)INFINITY)) {
        eqd_set_error("eqd_dock_meter_eval: cutoff = %g (need a finite value > 0)", cutoff);
        return EQD_ERR_SHAPE;
    }
    std::vector<MeterDesc> D;
    MeterWs W;
    if (int rc = dm_open("eqd_dock_meter_eval", C, lig_off, rec_off, workspace, ws_bytes, D, &W)) return rc;
    if (!rec_pred) rec_pred = rec_true;
    const int iface = interface ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const unsigned n_cnt = (unsigned)D[C].cnt_base, n_mom = (unsigned)D[C].mom_base;
    if (iface) {
        hipLaunchKernelGGL(k_dm_counts, dim3(n_cnt), dim3(EQD_BLOCK), 0, s, C, lig_true, rec_true, cutoff, W);
        if (int rc = eqd_check_launch("k_dm_counts")) return rc;
    }
    hipLaunchKernelGGL(k_dm_moments, dim3(n_mom), dim3(EQD_BLOCK), 0, s, C, lig_pred, rec_pred, lig_true, rec_true, iface, W);
    if (int rc = eqd_check_launch("k_dm_moments")) return rc;
    hipLaunchKernelGGL(k_dm_solve, dim3((unsigned)dm_cdiv(2 * C, 64)), dim3(64), 0, s, C, W);
    if (int rc = eqd_check_launch("k_dm_solve")) return rc;
    hipLaunchKernelGGL(k_dm_residuals, dim3(n_mom), dim3(EQD_BLOCK), 0, s, C, lig_pred, rec_pred, lig_true, rec_true, iface, W);
    if (int rc = eqd_check_launch("k_dm_residuals")) return rc;
    hipLaunchKernelGGL(k_dm_finish, dim3((unsigned)dm_cdiv(C, EQD_BLOCK)), dim3(EQD_BLOCK), 0, s, C, iface, metrics, W);
    return eqd_check_launch("k_dm_finish");
}

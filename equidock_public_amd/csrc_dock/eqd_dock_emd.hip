// Batched exact transport plans on the device (include/equidock_dock.h: eqd_dock_emd_*): the plans of the pocket OT term
// (src/utils/ot_utils.py:22-29, POT's ot.emd with a = 1/n, b = 1/m) for P problems in ONE launch, so that a training step
// needs neither the host solver nor the device <-> host round trip around it.
//
// The algorithm is emd_uniform of csrc_host/eqd_host_emd.cpp restated operation for operation, so that a problem's plan
// is bit-identical to the host solver's: integer supplies (m / g units per source, n / g per sink, g = gcd(n, m)), costs
// widened from fp32 to fp64, start potentials pv_j = min_i c_ij and pu = 0, successive shortest paths from source
// s = 0, 1, ... while it still has supply, dense Dijkstra on the reduced costs c_ij + pu_i - pv_j (forward) and
// -(c_ij + pu_i - pv_j) (backward, only where f_ij > 0) with negative values clamped to 0, leaving at the first settled
// sink that still has demand, the bottleneck along the path, the flow update, pi_v += min(dist_v, dist_t), and
// plan = (float)((double)f_ij * unit), unit = (double)g / ((double)n * (double)m).
//
// Three details decide the bits:
//   * Settling order.  The node settled next is the not yet settled one with the smallest finite dist; among equal
//     minima the LOWEST NODE INDEX (sources 0 .. n - 1, then sinks n .. n + m - 1) - the host's ascending scan with a
//     strict `<`.  Here lane l owns the block of nodes l * npl .. (l + 1) * npl - 1 (npl = ceil((n + m) / 64)) and scans
//     it in ascending order with the same strict `<`; the wave minimum is exact (a minimum of doubles does not round), and
//     of the lanes that hold it the lowest one holds the lowest index.
//   * Comparisons.  Every comparison is written as the host writes it: `b < a ? b : a`, `du + rc < dist`, `rc < 0.0`.  No
//     fmin / fmax: they treat NaN differently (a NaN cost must never win a comparison, as on the host).
//   * Arithmetic.  The solver only adds and compares doubles (one multiplication per cell makes the plan, as on the host);
//     the library is built with -ffp-contract=off.
//
// Decomposition: one problem = one workgroup = ONE wave; one launch of P workgroups per call.  dist, done, prev, the
// potentials and the remaining supply / demand of every node sit in LDS.  A source step relaxes the m sinks one per lane,
// a sink step the sources lane, lane + 64, ...; the argmin is a DPP minimum inside each row of 16 lanes, eight v_readlane
// for the four rows (two per double), and a ballot for the lowest lane - no ds_bpermute round trip, no __syncthreads, no
// atomics on floating point, no scratch.  Cost and flow matrices live in LDS while n * m <= EQD_DOCK_EMD_RESIDENT_CELLS (the resident body);
// above it the cost is read from the caller's matrix and the flow lives in the call's workspace (the general body):
// same operations, same bits.
//
// Every loop has a bound computed from n and m: at most n + m Dijkstra steps per path, at most n + m arcs on a path, at
// most n * m / g augmentations per problem (each moves >= 1 of the n * m / g units).  A problem that overruns a bound or
// finds no sink with demand (non-finite costs: the host returns NaN there) writes status[p] = 1, fills its plan rows
// with NaN and returns - it cannot spin, whatever the input.
#include "../csrc/eqd_common.h"
#include "../../include/equidock_dock.h"

#include <math.h>
#include <vector>

#define EMD_WAVE 64
#define EMD_MAXN EQD_DOCK_EMD_MAX_NODES
#define EMD_CELLS EQD_DOCK_EMD_RESIDENT_CELLS

// ---- wave-uniform values and the argmin ------------------------------------------------------------------------------
__device__ __forceinline__ double emd_uni(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double emd_min(double a, double b) { return b < a ? b : a; }   // std::min(a, b)

#ifdef EQD_HOSTSIM
__device__ __forceinline__ double emd_xor(double v, int m) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)b, m), hi = (unsigned)__shfl_xor((int)(unsigned)(b >> 32), m);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// (du, u): the wave's smallest `best` and the index held by the lowest lane that has it (u = -1: no finite candidate)
__device__ __forceinline__ int emd_argmin(double best, int idx, double* du_out) {
    double du = best;
    for (int m = 1; m < EMD_WAVE; m <<= 1) du = emd_min(du, emd_xor(du, m));
    *du_out = du;
    if (!(du < (double)INFINITY)) return -1;
    int lane = best == du ? (int)(threadIdx.x & 63) : EMD_WAVE;
    for (int m = 1; m < EMD_WAVE; m <<= 1) {
        const int o = __shfl_xor(lane, m);
        lane = o < lane ? o : lane;
    }
    return __shfl(idx, lane);
}
static inline void emd_flow_fence() {}
__device__ __forceinline__ int32_t emd_gload(const int32_t* p) { return *p; }
__device__ __forceinline__ void emd_gstore(int32_t* p, int32_t v) { *p = v; }
#else
template <int CTRL>
__device__ __forceinline__ double emd_dpp(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int LANE>
__device__ __forceinline__ double emd_readlane(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, LANE);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), LANE);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// All 64 lanes are active here (the control flow around every call is wave-uniform), and every lane of these four
// permutations has a source: lane ^ 1, lane ^ 2 (quad_perm), the other quad of the half row (row_half_mirror), the other
// half of the row (row_mirror).  After them every lane of a row of 16 holds the row's minimum.
__device__ __forceinline__ int emd_argmin(double best, int idx, double* du_out) {
    double r = best;
    r = emd_min(r, emd_dpp<0xB1>(r));       // quad_perm [1, 0, 3, 2]
    r = emd_min(r, emd_dpp<0x4E>(r));       // quad_perm [2, 3, 0, 1]
    r = emd_min(r, emd_dpp<0x141>(r));      // row_half_mirror
    r = emd_min(r, emd_dpp<0x140>(r));      // row_mirror
    const double du = emd_min(emd_min(emd_readlane<0>(r), emd_readlane<16>(r)), emd_min(emd_readlane<32>(r), emd_readlane<48>(r)));
    *du_out = du;
    if (!(du < (double)INFINITY)) return -1;
    const unsigned long long hit = __ballot(best == du);      // not empty: du is some lane's `best`
    return __builtin_amdgcn_readlane(idx, (int)__builtin_ctzll(hit));
}
// General body: the flow matrix is in global memory, written by lane 0 and read by every lane of the same wave.  The
// accesses bypass the (non-coherent) vector L1 - relaxed agent-scope loads and stores of an int32 - and a fence orders the
// stores of a phase in front of the loads of the next.
__device__ __forceinline__ void emd_flow_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent"); }
__device__ __forceinline__ int32_t emd_gload(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void emd_gstore(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

struct EmdLds {
    double* dist;            // [n + m]
    double* pi;              // [n + m]: pu_i, then pv_j
    int32_t* prev;           // [n + m]
    int32_t* cap;            // [n + m]: remaining supply of the sources, then remaining demand of the sinks
    unsigned char* done;     // [n + m]
    float* c;                // [n * m] resident body: the cost matrix (widened at every use: exact)
    int32_t* f;              // [n * m] resident body: the flow
};

template <bool RES>
struct EmdCells {
    const float* c;
    int32_t* f;
    __device__ __forceinline__ double cost(int k) const { return (double)c[k]; }
    __device__ __forceinline__ int32_t flow(int k) const { return RES ? f[k] : emd_gload(f + k); }
    __device__ __forceinline__ void set_flow(int k, int32_t v) const {
        if (RES) f[k] = v;
        else emd_gstore(f + k, v);
    }
    // phase boundary behind a write of the flow
    __device__ __forceinline__ void fence() const {
        if (!RES) emd_flow_fence();
        wave_lds_fence();
    }
};

// returns 0, or 1 when the problem failed (a bound overrun or no sink with demand)
template <bool RES>
__device__ __forceinline__ int emd_solve(int n, int m, const float* __restrict__ cost, int32_t* __restrict__ flow_ws,
                                         float* __restrict__ plan, const EmdLds& S) {
    const int lane = (int)(threadIdx.x & 63);
    const int V = n + m, cells = n * m;
    int g = n;
    for (int b = m; b != 0;) {                      // gcd(n, m): Euclid, at most ~1.44 log2(n + m) rounds
        const int t = g % b;
        g = b;
        b = t;
    }
    const int su = m / g, de = n / g;               // units per source / per sink
    const double unit = (double)g / ((double)n * (double)m);
    const double INF = (double)INFINITY;
    EmdCells<RES> X;
    if (RES) {
        for (int k = lane; k < cells; k += EMD_WAVE) {
            S.c[k] = cost[k];
            S.f[k] = 0;
        }
        X.c = S.c;
        X.f = S.f;
    } else {
        for (int k = lane; k < cells; k += EMD_WAVE) emd_gstore(flow_ws + k, 0);
        X.c = cost;
        X.f = flow_ws;
    }
    for (int v = lane; v < V; v += EMD_WAVE) {
        S.cap[v] = v < n ? su : de;
        if (v < n) S.pi[v] = 0.0;
    }
    X.fence();
    // potentials: pv_j = min_i c_ij in ascending i (pu = 0)
    for (int j = lane; j < m; j += EMD_WAVE) {
        double mn = INF;
        for (int i = 0; i < n; ++i) mn = emd_min(mn, X.cost(i * m + j));
        S.pi[n + j] = mn;
    }
    wave_lds_fence();
    const int npl = (V + EMD_WAVE - 1) / EMD_WAVE;  // nodes per lane: lane l owns l * npl .. (l + 1) * npl - 1
    const int v0 = lane * npl < V ? lane * npl : V, v1 = v0 + npl < V ? v0 + npl : V;
    int aug_left = cells / g;                       // bound: augmentations per problem
    for (int s = 0; s < n; ++s) {
        for (;;) {
            const int sup = uni(S.cap[s]);
            if (sup <= 0) break;
            if (aug_left-- <= 0) return 1;
            // Dijkstra from source s over the nodes {sources 0 .. n - 1, sinks n .. n + m - 1}
            for (int v = lane; v < V; v += EMD_WAVE) {
                S.dist[v] = v == s ? 0.0 : INF;
                S.done[v] = 0;
            }
            if (lane == 0) S.prev[s] = -1;
            wave_lds_fence();
            int target = -1;
            for (int step = 0; step < V; ++step) {  // bound: every step settles one node
                // settle the not yet settled node with the smallest finite dist, the lowest index among equals
                double best = INF;
                int bi = -1;
                for (int v = v0; v < v1; ++v) {
                    const double d = S.dist[v];
                    if (!S.done[v] && d < best) {
                        best = d;
                        bi = v;
                    }
                }
                double du;
                const int u = emd_argmin(best, bi, &du);
                if (u < 0) break;
                if (lane == 0) S.done[u] = 1;
                wave_lds_fence();
                if (u >= n) {                       // a sink
                    const int j = u - n;
                    if (uni(S.cap[u]) > 0) {
                        target = u;
                        break;
                    }
                    // backward arcs j -> i where flow exists
                    const double pvj = S.pi[u];
                    for (int i = lane; i < n; i += EMD_WAVE) {
                        if (S.done[i] || X.flow(i * m + j) <= 0) continue;
                        double rc = -(X.cost(i * m + j) + S.pi[i] - pvj);
                        if (rc < 0.0) rc = 0.0;
                        if (du + rc < S.dist[i]) {
                            S.dist[i] = du + rc;
                            S.prev[i] = u;
                        }
                    }
                } else {                            // a source: forward arcs to every sink
                    const int i = u;
                    const double pui = S.pi[i];
                    for (int j = lane; j < m; j += EMD_WAVE) {
                        if (S.done[n + j]) continue;
                        double rc = X.cost(i * m + j) + pui - S.pi[n + j];
                        if (rc < 0.0) rc = 0.0;
                        if (du + rc < S.dist[n + j]) {
                            S.dist[n + j] = du + rc;
                            S.prev[n + j] = u;
                        }
                    }
                }
                wave_lds_fence();
            }
            if (target < 0) return 1;
            const double dt = emd_uni(S.dist[target]);
            // bottleneck along the path (every lane walks it: the reads are wave-uniform)
            const int dem = uni(S.cap[target]);
            int delta = dem < sup ? dem : sup;
            int len = 0;
            for (int v = target;;) {
                const int u = uni(S.prev[v]);
                if (u < 0) break;
                if (++len > V) return 1;            // bound: arcs on a path
                if (u >= n) {                       // backward arc sink u -> source v
                    const int fl = uni(X.flow(v * m + (u - n)));
                    delta = fl < delta ? fl : delta;
                }
                v = u;
            }
            wave_lds_fence();                       // every lane has read what lane 0 rewrites below
            for (int v = target;;) {                // (at most `len` arcs: the walk above has ended)
                const int u = uni(S.prev[v]);
                if (u < 0) break;
                if (lane == 0) {
                    const int k = u < n ? u * m + (v - n) : v * m + (u - n);      // forward arc u -> v | backward
                    X.set_flow(k, X.flow(k) + (u < n ? delta : -delta));
                }
                v = u;
            }
            if (lane == 0) {
                S.cap[s] = sup - delta;
                S.cap[target] = dem - delta;
            }
            // potentials: pi_v += min(dist_v, dist_t)
            for (int v = lane; v < V; v += EMD_WAVE) S.pi[v] += emd_min(S.dist[v], dt);
            X.fence();
        }
    }
    for (int k = lane; k < cells; k += EMD_WAVE) plan[k] = (float)((double)X.flow(k) * unit);
    return 0;
}

__global__ __launch_bounds__(EMD_WAVE) void k_dock_emd(int P, const int32_t* __restrict__ off, int m,
                                                       const float* __restrict__ cost, float* __restrict__ plan,
                                                       int32_t* __restrict__ status, int32_t* __restrict__ flow_ws,
                                                       int resident) {
    __shared__ double s_dist[EMD_MAXN], s_pi[EMD_MAXN];
    __shared__ int32_t s_prev[EMD_MAXN], s_cap[EMD_MAXN];
    __shared__ unsigned char s_done[EMD_MAXN];
    __shared__ float s_c[EMD_CELLS];
    __shared__ int32_t s_f[EMD_CELLS];
    const int p = (int)blockIdx.x;
    if (p >= P) return;
    const int r0 = uni(off[p]), n = uni(off[p + 1]) - r0;
    const int lane = (int)(threadIdx.x & 63);
    const size_t base = (size_t)r0 * (size_t)m;
    if (n <= 0) {                                    // 0 rows: no plan row to write
        if (lane == 0) status[p] = 0;
        return;
    }
    if (n + m > EMD_MAXN) {                          // (the host has refused it; a failed problem all the same: NaN rows)
        const float nan = __builtin_nanf("");
        for (size_t k = (size_t)lane; k < (size_t)n * (size_t)m; k += EMD_WAVE) plan[base + k] = nan;
        if (lane == 0) status[p] = 1;
        return;
    }
    EmdLds S;
    S.dist = s_dist; S.pi = s_pi; S.prev = s_prev; S.cap = s_cap; S.done = s_done; S.c = s_c; S.f = s_f;
    int bad;
    if (resident && n * m <= EMD_CELLS) bad = emd_solve<true>(n, m, cost + base, flow_ws + base, plan + base, S);
    else bad = emd_solve<false>(n, m, cost + base, flow_ws + base, plan + base, S);
    if (bad) {
        const float nan = __builtin_nanf("");
        for (int k = lane; k < n * m; k += EMD_WAVE) plan[base + k] = nan;
    }
    if (lane == 0) status[p] = bad ? 1 : 0;
}

// ---- host side ------------------------------------------------------------------------------------------------
struct EmdWs {
    int32_t* off;       // [P + 1] the row offsets on the device
    int32_t* flow;      // [sum n][m] the flow of the general body
};

// validates the sizes; returns EQD_OK or an error code with the message set
static int emd_plan(const char* fn, int P, const int32_t* src_off, int m) {
    if (!src_off) {
        eqd_set_error("%s: NULL offsets", fn);
        return EQD_ERR_NULL;
    }
    if (P < 1) {
        eqd_set_error("%s: n_problems = %d (need >= 1)", fn, P);
        return EQD_ERR_SHAPE;
    }
    if (m < 1) {
        eqd_set_error("%s: n_snk = %d (need >= 1)", fn, m);
        return EQD_ERR_SHAPE;
    }
    if (src_off[0] != 0) {
        eqd_set_error("%s: src_off[0] = %d (need 0)", fn, src_off[0]);
        return EQD_ERR_SHAPE;
    }
    for (int p = 0; p < P; ++p) {
        const int64_t n = (int64_t)src_off[p + 1] - src_off[p];
        if (n < 0) {
            eqd_set_error("%s: problem %d has %lld rows (offsets must not decrease)", fn, p, (long long)n);
            return EQD_ERR_SHAPE;
        }
        if (n > 0 && n + m > EQD_DOCK_EMD_MAX_NODES) {
            eqd_set_error("%s: problem %d has %lld sources and %d sinks: more than EQD_DOCK_EMD_MAX_NODES = %d nodes", fn, p,
                          (long long)n, m, EQD_DOCK_EMD_MAX_NODES);
            return EQD_ERR_SHAPE;
        }
    }
    return EQD_OK;
}

static size_t emd_carve(int P, const int32_t* src_off, int m, EqdArena& A, EmdWs* W) {
    EmdWs w;
    w.off = A.take<int32_t>((size_t)P + 1);
    w.flow = A.take<int32_t>((size_t)src_off[P] * (size_t)m + 1);
    if (W) *W = w;
    return A.off;
}

static int emd_open(const char* fn, int P, const int32_t* src_off, int m, void* workspace, size_t ws_bytes, EmdWs* W) {
    if (!workspace) {
        eqd_set_error("%s: NULL workspace", fn);
        return EQD_ERR_NULL;
    }
    if (int rc = emd_plan(fn, P, src_off, m)) return rc;
    EqdArena A(workspace, ws_bytes);
    emd_carve(P, src_off, m, A, W);
    if (!A.ok) {
        eqd_set_error("%s: workspace too small (%zu needed, %zu given)", fn, A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_emd_abi(void) { return EQD_DOCK_EMD_ABI; }

extern "C" EQD_DOCK_API size_t eqd_dock_emd_workspace_bytes(int P, const int32_t* src_off, int n_snk) {
    if (emd_plan("eqd_dock_emd_workspace_bytes", P, src_off, n_snk) != EQD_OK) return 0;
    EqdArena A(nullptr, 0);
    return emd_carve(P, src_off, n_snk, A, nullptr) + 256;
}

extern "C" EQD_DOCK_API int eqd_dock_emd_init(int P, const int32_t* src_off, int n_snk, void* workspace, size_t ws_bytes,
                                              void* stream) {
    EmdWs W;
    if (int rc = emd_open("eqd_dock_emd_init", P, src_off, n_snk, workspace, ws_bytes, &W)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync((void*)W.off, src_off, sizeof(int32_t) * ((size_t)P + 1), hipMemcpyHostToDevice, s) != hipSuccess) {
        eqd_set_error("eqd_dock_emd_init: copy failed");
        return EQD_ERR_LAUNCH;
    }
#ifndef EQD_HOSTSIM
    if (hipStreamSynchronize(s) != hipSuccess) {      // the caller may free or rewrite `src_off` after this call
        eqd_set_error("eqd_dock_emd_init: stream synchronisation failed");
        return EQD_ERR_LAUNCH;
    }
#endif
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_emd_solve(int P, const int32_t* src_off, int n_snk, const float* cost, float* plan,
                                               int32_t* status, int resident, void* workspace, size_t ws_bytes,
                                               void* stream) {
    if (!cost || !plan || !status) {
        eqd_set_error("eqd_dock_emd_solve: NULL argument");
        return EQD_ERR_NULL;
    }
    EmdWs W;
    if (int rc = emd_open("eqd_dock_emd_solve", P, src_off, n_snk, workspace, ws_bytes, &W)) return rc;
    hipLaunchKernelGGL(k_dock_emd, dim3((unsigned)P), dim3(EMD_WAVE), 0, (hipStream_t)stream, P, (const int32_t*)W.off, n_snk,
                       cost, plan, status, W.flow, resident ? 1 : 0);
    return eqd_check_launch("k_dock_emd");
}

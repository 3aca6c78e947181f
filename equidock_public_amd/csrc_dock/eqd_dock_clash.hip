// Batched clash removal (include/equidock_dock.h): the loop of src/inference_rigid.py:207-234 for C complexes in one
// device loop.  Same arithmetic as eqd_clash_iterations (csrc/eqd_data_kernels.hip):
//   a_i = R(euler) p_i + t,   R = RZ(yaw) RY(pitch) RX(roll),  euler = (roll, yaw, pitch)
//   loss = mean_i max(0, ct - G_r(a_i)) + mean_k max(0, ct - G_l(b_k)),  G(x) = -sigma log(1e-3 + sum exp(-|x - c|^2 / sigma))
//   eta = 1e-3; 1e-4 if loss < 2; 1e-2 if it > 1500
//
// Work decomposition.  A work item is (complex, row tile of DK_ROWS rows, partner chunk of DK_CHUNK partners): one row
// per thread, the chunk staged in LDS as float4 and read by every lane at the same address (a broadcast).  Each item
// writes its partial sums to its own slot; whoever needs a total adds the slots in chunk order.  Three launches per
// iteration, whatever C is:
//   k_dock_eval  items (ligand tile x receptor chunk) -> S_lig partials, and (receptor tile x ligand chunk) -> S_rec
//                partials; ligand positions are recomputed from (euler, t) wherever they are needed
//   k_dock_grad  items (ligand tile x receptor chunk): totals S_i, S_k from the partials (fixed order), the gradient of
//                the tile against the chunk chained to (translation, euler) -> 6 partials per item; the items of chunk 0
//                also write the tile's term-1 sum, the items of tile 0 the chunk's term-2 sum
//   k_dock_step  one wave per complex: loss and gradient from those partials (fixed lane assignment), stop rule, update,
//                and one integer increment of the completion counter when the complex finishes
// The item table depends only on each complex's own sizes, so a complex's bits do not depend on the batch.
#include "../csrc/eqd_common.h"
#include "../../include/equidock_dock.h"

#include <stdarg.h>
#include <stdio.h>
#include <vector>

#define DK_ROWS EQD_BLOCK   // rows per work item (one per thread)
#define DK_CHUNK 512        // partners per work item (8 KiB of LDS as float4)

struct DockDesc {           // one complex of the batch (entry C: the totals)
    int32_t l0, nl, r0, nr; // row offsets and sizes
    int32_t max_it;
    int32_t ntl, ncr;       // ligand tiles, receptor chunks
    int32_t ntr, ncl;       // receptor tiles, ligand chunks
    int32_t eval_base;      // first k_dock_eval item (ntl * ncr ligand items, then ntr * ncl receptor items)
    int32_t grad_base;      // first k_dock_grad item (ntl * ncr)
    int32_t tp1_base;       // term-1 sums [ntl]
    int32_t tp2_base;       // term-2 sums [ncr]
    int32_t pad;
    int64_t slig_base;      // S_lig partials [ncr][nl]
    int64_t srec_base;      // S_rec partials [ncl][nr]
};

struct DockWs {
    const DockDesc* desc;   // [C + 1]
    float* slig;
    float* srec;
    float* gpart;           // [grad items][6]
    float* tp1;
    float* tp2;
};

// ---- host-side error string of this library ---------------------------------------------------------------------
static thread_local char g_dock_err[512];
void eqd_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_dock_err, sizeof(g_dock_err), fmt, ap);
    va_end(ap);
}
int eqd_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        eqd_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return EQD_ERR_LAUNCH;
    }
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_abi_version(void) { return EQD_DOCK_ABI_VERSION; }
extern "C" EQD_DOCK_API const char* eqd_dock_last_error(void) { return g_dock_err; }
extern "C" EQD_DOCK_API int eqd_dock_is_simulator(void) {
#ifdef EQD_HOSTSIM
    return 1;
#else
    return 0;
#endif
}

// ---- device side ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dk_rot(const float* e, float R[9]) {
    const float cr = cosf(e[0]), sr = sinf(e[0]), cy = cosf(e[1]), sy = sinf(e[1]), cp = cosf(e[2]), sp = sinf(e[2]);
    R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
    R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
    R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}
// a = R p + t (the one expression every kernel uses, so that recomputed positions agree bit for bit)
__device__ __forceinline__ void dk_move(const float R[9], const float* t, float px, float py, float pz, float& ax,
                                        float& ay, float& az) {
    ax = (R[0] * px + R[1] * py) + R[2] * pz + t[0];
    ay = (R[3] * px + R[4] * py) + R[5] * pz + t[1];
    az = (R[6] * px + R[7] * py) + R[8] * pz + t[2];
}
__device__ __forceinline__ float dk_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();      // red is reused by the next call
    return r;
}
// the complex that owns `item` (largest c with base(c) <= item; the bases are strictly increasing, entry C = total)
template <int kGrad>
__device__ __forceinline__ int dk_find(const DockDesc* __restrict__ D, int C, int item) {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int b = kGrad ? D[mid].grad_base : D[mid].eval_base;
        if (b <= item) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dock_eval(int C, const float* __restrict__ lig0,
                                                         const float* __restrict__ rec, float sigma,
                                                         const EqdClashState* __restrict__ states, DockWs W) {
    __shared__ float4 pts[DK_CHUNK];
    const int item = blockIdx.x;
    if (item >= W.desc[C].eval_base) return;
    const int c = dk_find<0>(W.desc, C, item);
    const DockDesc d = W.desc[c];
    const EqdClashState* st = states + c;
    if (st->done || st->it >= d.max_it) return;
    float R[9];
    const float e[3] = {st->euler[0], st->euler[1], st->euler[2]};
    const float t[3] = {st->trans[0], st->trans[1], st->trans[2]};
    dk_rot(e, R);
    const float inv = 1.f / sigma;
    const int q = item - d.eval_base;
    if (q < d.ntl * d.ncr) {
        // ligand rows of one tile against one receptor chunk
        const int tile = q / d.ncr, chunk = q - tile * d.ncr;
        const int k0 = chunk * DK_CHUNK, nc = d.nr - k0 < DK_CHUNK ? d.nr - k0 : DK_CHUNK;
        const float* rb = rec + (size_t)(d.r0 + k0) * 3;
        for (int k = threadIdx.x; k < nc; k += EQD_BLOCK) pts[k] = make_float4(rb[(size_t)k * 3], rb[(size_t)k * 3 + 1], rb[(size_t)k * 3 + 2], 0.f);
        const int i = tile * DK_ROWS + threadIdx.x;
        const int ic = i < d.nl ? i : d.nl - 1;
        const float* p = lig0 + (size_t)(d.l0 + ic) * 3;
        float ax, ay, az;
        dk_move(R, t, p[0], p[1], p[2], ax, ay, az);
        __syncthreads();
        float S = 0.f;
#pragma unroll 8
        for (int k = 0; k < nc; ++k) {
            const float4 b = pts[k];
            const float dx = b.x - ax, dy = b.y - ay, dz = b.z - az;
            S += expf(-((dx * dx + dy * dy) + dz * dz) * inv);
        }
        if (i < d.nl) W.slig[d.slig_base + (int64_t)chunk * d.nl + i] = S;
    } else {
        // receptor rows of one tile against one chunk of the moved ligand
        const int q2 = q - d.ntl * d.ncr;
        const int tile = q2 / d.ncl, chunk = q2 - tile * d.ncl;
        const int k0 = chunk * DK_CHUNK, nc = d.nl - k0 < DK_CHUNK ? d.nl - k0 : DK_CHUNK;
        const float* lb = lig0 + (size_t)(d.l0 + k0) * 3;
        for (int k = threadIdx.x; k < nc; k += EQD_BLOCK) {
            float ax, ay, az;
            dk_move(R, t, lb[(size_t)k * 3], lb[(size_t)k * 3 + 1], lb[(size_t)k * 3 + 2], ax, ay, az);
            pts[k] = make_float4(ax, ay, az, 0.f);
        }
        const int r = tile * DK_ROWS + threadIdx.x;
        const int rc = r < d.nr ? r : d.nr - 1;
        const float* b = rec + (size_t)(d.r0 + rc) * 3;
        const float bx = b[0], by = b[1], bz = b[2];
        __syncthreads();
        float S = 0.f;
#pragma unroll 8
        for (int k = 0; k < nc; ++k) {
            const float4 a = pts[k];
            const float dx = a.x - bx, dy = a.y - by, dz = a.z - bz;
            S += expf(-((dx * dx + dy * dy) + dz * dz) * inv);
        }
        if (r < d.nr) W.srec[d.srec_base + (int64_t)chunk * d.nr + r] = S;
    }
}

__global__ __launch_bounds__(EQD_BLOCK) void k_dock_grad(int C, const float* __restrict__ lig0,
                                                         const float* __restrict__ rec, float sigma, float ct,
                                                         const EqdClashState* __restrict__ states, DockWs W) {
    __shared__ float4 pts[DK_CHUNK];
    __shared__ float red[EQD_WAVES];
    const int item = blockIdx.x;
    if (item >= W.desc[C].grad_base) return;
    const int c = dk_find<1>(W.desc, C, item);
    const DockDesc d = W.desc[c];
    const EqdClashState* st = states + c;
    // the iteration whose loss comes out <= loss_stop still steps, so its gradient is needed too (k_dock_step decides)
    if (st->done || st->it >= d.max_it) return;
    const int q = item - d.grad_base;
    const int tile = q / d.ncr, chunk = q - tile * d.ncr;
    const int k0 = chunk * DK_CHUNK, nc = d.nr - k0 < DK_CHUNK ? d.nr - k0 : DK_CHUNK;
    // the chunk's receptor atoms with their backward weights [ct - G_l(b_k) >= 0] / (n_rec (1e-3 + S_k))
    float term2 = 0.f;
    for (int k = threadIdx.x; k < nc; k += EQD_BLOCK) {
        const int kk = k0 + k;
        const float* b = rec + (size_t)(d.r0 + kk) * 3;
        float S = 0.f;
        for (int j = 0; j < d.ncl; ++j) S += W.srec[d.srec_base + (int64_t)j * d.nr + kk];
        const float G = -sigma * logf(1e-3f + S);
        term2 += ct - G > 0.f ? ct - G : 0.f;
        pts[k] = make_float4(b[0], b[1], b[2], ct - G >= 0.f ? 1.f / ((float)d.nr * (1e-3f + S)) : 0.f);
    }
    if (tile == 0) {                                        // (uniform over the block)
        const float tot = dk_block_sum(term2, red);
        if (threadIdx.x == 0) W.tp2[d.tp2_base + chunk] = tot;
    }
    const float e[3] = {st->euler[0], st->euler[1], st->euler[2]};
    const float t[3] = {st->trans[0], st->trans[1], st->trans[2]};
    float R[9];
    dk_rot(e, R);
    const int i = tile * DK_ROWS + threadIdx.x;
    const int ic = i < d.nl ? i : d.nl - 1;
    const float* p = lig0 + (size_t)(d.l0 + ic) * 3;
    const float px = p[0], py = p[1], pz = p[2];
    float ax, ay, az;
    dk_move(R, t, px, py, pz, ax, ay, az);
    float Si = 0.f;
    for (int j = 0; j < d.ncr; ++j) Si += W.slig[d.slig_base + (int64_t)j * d.nl + ic];
    const float Gi = -sigma * logf(1e-3f + Si);
    const float wi = (ct - Gi >= 0.f) ? 1.f / ((float)d.nl * (1e-3f + Si)) : 0.f;
    if (chunk == 0) {                                       // (uniform over the block)
        const float term1 = i < d.nl && ct - Gi > 0.f ? ct - Gi : 0.f;
        const float tot = dk_block_sum(term1, red);
        if (threadIdx.x == 0) W.tp1[d.tp1_base + tile] = tot;
    }
    __syncthreads();
    const float inv = 1.f / sigma;
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll 4
    for (int k = 0; k < nc; ++k) {
        const float4 b = pts[k];
        const float dx = ax - b.x, dy = ay - b.y, dz = az - b.z;
        const float w = expf(-((dx * dx + dy * dy) + dz * dz) * inv) * (wi + b.w);
        gx += w * dx; gy += w * dy; gz += w * dz;
    }
    // d loss / d a_i = -2 (gx, gy, gz); a_i = R(euler) p_i + t
    const float g[3] = {i < d.nl ? -2.f * gx : 0.f, i < d.nl ? -2.f * gy : 0.f, i < d.nl ? -2.f * gz : 0.f};
    const float cr = cosf(e[0]), sr = sinf(e[0]), cy = cosf(e[1]), sy = sinf(e[1]), cp = cosf(e[2]), sp = sinf(e[2]);
    // dR/droll, dR/dyaw, dR/dpitch of R = RZ(yaw) RY(pitch) RX(roll)
    const float dRr[9] = {0.f, cy * sp * cr + sy * sr, -cy * sp * sr + sy * cr,
                          0.f, sy * sp * cr - cy * sr, -sy * sp * sr - cy * cr,
                          0.f, cp * cr, -cp * sr};
    const float dRy[9] = {-sy * cp, -sy * sp * sr - cy * cr, -sy * sp * cr + cy * sr,
                          cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                          0.f, 0.f, 0.f};
    const float dRp[9] = {-cy * sp, cy * cp * sr, cy * cp * cr,
                          -sy * sp, sy * cp * sr, sy * cp * cr,
                          -cp, -sp * sr, -sp * cr};
    float out[6];
    out[0] = g[0]; out[1] = g[1]; out[2] = g[2];
    const float* dRs[3] = {dRr, dRy, dRp};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float* dr = dRs[j];
        out[3 + j] = g[0] * ((dr[0] * px + dr[1] * py) + dr[2] * pz) + g[1] * ((dr[3] * px + dr[4] * py) + dr[5] * pz) +
                     g[2] * ((dr[6] * px + dr[7] * py) + dr[8] * pz);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float tot = dk_block_sum(out[j], red);
        if (threadIdx.x == 0) W.gpart[(size_t)item * 6 + j] = tot;
    }
}

// one wave per complex: stop rule, step size, update
__global__ __launch_bounds__(64) void k_dock_step(int C, float loss_stop, EqdClashState* __restrict__ states,
                                                  int32_t* __restrict__ n_done, DockWs W) {
    const int c = blockIdx.x;
    if (c >= C) return;
    const DockDesc d = W.desc[c];
    EqdClashState* st = states + c;
    if (st->done) return;
    const int lane = threadIdx.x;
    // The reference's loop (src/inference_rigid.py:213-232) tests `loss > 0.5 and it < 2000` with the loss of the PREVIOUS
    // evaluation, then evaluates, steps and increments unconditionally; at it == max_it nothing is evaluated any more.
    if (st->it >= d.max_it) {
        if (lane == 0) {
            st->done = 1;
            atomicAdd(n_done, 1);
        }
        return;
    }
    float a = 0.f, b = 0.f;
    for (int q = lane; q < d.ntl; q += 64) a += W.tp1[d.tp1_base + q];
    for (int q = lane; q < d.ncr; q += 64) b += W.tp2[d.tp2_base + q];
    a = wave_sum(a);
    b = wave_sum(b);
    float g[6];
    const int ng = d.ntl * d.ncr;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float s = 0.f;
        for (int q = lane; q < ng; q += 64) s += W.gpart[(size_t)(d.grad_base + q) * 6 + j];
        g[j] = wave_sum(s);
    }
    if (lane != 0) return;
    const float loss = a / (float)d.nl + b / (float)d.nr;
    const int it = st->it;
    st->loss = loss;
    float eta = 1e-3f;
    if (loss < 2.f) eta = 1e-4f;
    if (it > 1500) eta = 1e-2f;
    for (int j = 0; j < 3; ++j) {
        st->trans[j] -= eta * g[j];
        st->euler[j] -= eta * g[3 + j];
    }
    st->it = it + 1;
    if (!(loss > loss_stop)) {
        st->done = 1;
        atomicAdd(n_done, 1);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
static int dk_cdiv(int a, int b) { return (a + b - 1) / b; }

// validated item table of a batch (+ entry C with the totals); returns EQD_OK or an error code with the message set
static int dk_plan(const char* fn, int C, const int32_t* lig_off, const int32_t* rec_off, const int32_t* max_it,
                   std::vector<DockDesc>& D) {
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
    D.assign((size_t)C + 1, DockDesc{});
    int64_t eval = 0, grad = 0, tp1 = 0, tp2 = 0, slig = 0, srec = 0;
    for (int c = 0; c < C; ++c) {
        const int64_t nl = (int64_t)lig_off[c + 1] - lig_off[c], nr = (int64_t)rec_off[c + 1] - rec_off[c];
        if (nl < 1 || nr < 1) {
            eqd_set_error("%s: complex %d has %lld ligand and %lld receptor atoms (offsets must increase; every complex "
                          "needs >= 1 atom on each side)", fn, c, (long long)nl, (long long)nr);
            return EQD_ERR_SHAPE;
        }
        DockDesc& d = D[c];
        d.l0 = lig_off[c]; d.nl = (int32_t)nl; d.r0 = rec_off[c]; d.nr = (int32_t)nr;
        d.max_it = max_it ? max_it[c] : 0;
        d.ntl = dk_cdiv(d.nl, DK_ROWS); d.ncr = dk_cdiv(d.nr, DK_CHUNK);
        d.ntr = dk_cdiv(d.nr, DK_ROWS); d.ncl = dk_cdiv(d.nl, DK_CHUNK);
        d.eval_base = (int32_t)eval; d.grad_base = (int32_t)grad; d.tp1_base = (int32_t)tp1; d.tp2_base = (int32_t)tp2;
        d.slig_base = slig; d.srec_base = srec;
        eval += (int64_t)d.ntl * d.ncr + (int64_t)d.ntr * d.ncl;
        grad += (int64_t)d.ntl * d.ncr;
        tp1 += d.ntl; tp2 += d.ncr;
        slig += (int64_t)d.ncr * d.nl; srec += (int64_t)d.ncl * d.nr;
        if (eval > INT32_MAX || grad > INT32_MAX / 6) {
            eqd_set_error("%s: %lld work items do not fit int32 (split the batch)", fn, (long long)eval);
            return EQD_ERR_SHAPE;
        }
    }
    DockDesc& e = D[C];
    e.l0 = lig_off[C]; e.r0 = rec_off[C];
    e.eval_base = (int32_t)eval; e.grad_base = (int32_t)grad; e.tp1_base = (int32_t)tp1; e.tp2_base = (int32_t)tp2;
    e.slig_base = slig; e.srec_base = srec;
    return EQD_OK;
}

static size_t dk_carve(int C, const std::vector<DockDesc>& D, EqdArena& A, DockWs* W) {
    const DockDesc& e = D[C];
    DockWs w;
    w.desc = A.take<DockDesc>((size_t)C + 1);
    w.slig = A.take<float>((size_t)e.slig_base);
    w.srec = A.take<float>((size_t)e.srec_base);
    w.gpart = A.take<float>((size_t)e.grad_base * 6);
    w.tp1 = A.take<float>((size_t)e.tp1_base);
    w.tp2 = A.take<float>((size_t)e.tp2_base);
    if (W) *W = w;
    return A.off;
}

extern "C" EQD_DOCK_API size_t eqd_dock_clash_workspace_bytes(int C, const int32_t* lig_off, const int32_t* rec_off) {
    std::vector<DockDesc> D;
    if (dk_plan("eqd_dock_clash_workspace_bytes", C, lig_off, rec_off, nullptr, D) != EQD_OK) return 0;
    EqdArena A(nullptr, 0);
    return dk_carve(C, D, A, nullptr) + 256;
}

extern "C" EQD_DOCK_API int eqd_dock_clash_init(int C, const int32_t* lig_off, const int32_t* rec_off,
                                                const int32_t* max_it, EqdClashState* states, int32_t* n_done,
                                                void* workspace, size_t ws_bytes, void* stream) {
    if (!max_it || !states || !n_done || !workspace) {
        eqd_set_error("eqd_dock_clash_init: NULL argument");
        return EQD_ERR_NULL;
    }
    std::vector<DockDesc> D;
    if (int rc = dk_plan("eqd_dock_clash_init", C, lig_off, rec_off, max_it, D)) return rc;
    EqdArena A(workspace, ws_bytes);
    DockWs W;
    dk_carve(C, D, A, &W);
    if (!A.ok) {
        eqd_set_error("eqd_dock_clash_init: workspace too small (%zu needed, %zu given)", A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync((void*)W.desc, D.data(), sizeof(DockDesc) * D.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(states, 0, sizeof(EqdClashState) * (size_t)C, s) != hipSuccess ||
        hipMemsetAsync(n_done, 0, sizeof(int32_t), s) != hipSuccess) {
        eqd_set_error("eqd_dock_clash_init: copy / memset failed");
        return EQD_ERR_LAUNCH;
    }
#ifndef EQD_HOSTSIM
    if (hipStreamSynchronize(s) != hipSuccess) {      // `D` is a local host buffer
        eqd_set_error("eqd_dock_clash_init: stream synchronisation failed");
        return EQD_ERR_LAUNCH;
    }
#endif
    return EQD_OK;
}

extern "C" EQD_DOCK_API int eqd_dock_clash_iterations(int n_iter, int C, const int32_t* lig_off, const int32_t* rec_off,
                                                      const float* lig0, const float* rec, float sigma, float surface_ct,
                                                      float loss_stop, EqdClashState* states, int32_t* n_done,
                                                      void* workspace, size_t ws_bytes, void* stream) {
    if (!lig0 || !rec || !states || !n_done || !workspace) {
        eqd_set_error("eqd_dock_clash_iterations: NULL argument");
        return EQD_ERR_NULL;
    }
    if (!(sigma > 0.f) || n_iter < 0) {
        eqd_set_error("eqd_dock_clash_iterations: sigma = %g, n_iter = %d", sigma, n_iter);
        return EQD_ERR_SHAPE;
    }
    std::vector<DockDesc> D;
    if (int rc = dk_plan("eqd_dock_clash_iterations", C, lig_off, rec_off, nullptr, D)) return rc;
    EqdArena A(workspace, ws_bytes);
    DockWs W;
    dk_carve(C, D, A, &W);
    if (!A.ok) {
        eqd_set_error("eqd_dock_clash_iterations: workspace too small (%zu needed, %zu given)", A.off + 256, ws_bytes);
        return EQD_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned n_eval = (unsigned)D[C].eval_base, n_grad = (unsigned)D[C].grad_base;
    for (int it = 0; it < n_iter; ++it) {
        hipLaunchKernelGGL(k_dock_eval, dim3(n_eval), dim3(EQD_BLOCK), 0, s, C, lig0, rec, sigma, states, W);
        if (int rc = eqd_check_launch("k_dock_eval")) return rc;
        hipLaunchKernelGGL(k_dock_grad, dim3(n_grad), dim3(EQD_BLOCK), 0, s, C, lig0, rec, sigma, surface_ct, states, W);
        if (int rc = eqd_check_launch("k_dock_grad")) return rc;
        hipLaunchKernelGGL(k_dock_step, dim3((unsigned)C), dim3(64), 0, s, C, loss_stop, states, n_done, W);
        if (int rc = eqd_check_launch("k_dock_step")) return rc;
    }
    return EQD_OK;
}

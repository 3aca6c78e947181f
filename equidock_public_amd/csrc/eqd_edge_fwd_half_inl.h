// Edge-message forward of the fused small-batch launch on 16-edge HALF tiles (included by eqd_edge_kernels.hip behind
// edge_fwd_body and the fused kernels, whose types and helpers it uses).
//
// edge_fwd_body gives every node-aligned tile of <= 32 edges to ONE wave; at DB5.5 sizes that is one tile per wave and two
// waves per SIMD, which leave the staging barrier together, run the same program and meet at the matrix pipe.  Here a
// PAIR of waves owns the tile: workgroups are 16 waves (four per SIMD) and 8 tiles; waves w and w + 8 own tile
// blk * 8 + w, half h = wave >> 3 takes the tile's edges 16 h .. 16 h + 15 - block nb = h of edge_fwd_body - through
// edge_tile_forward<1> (the instantiation k_edge_bwd recomputes with).  A column of an MFMA product depends on its own
// column of the B operand only, so every per-edge value is the value edge_fwd_body's wave computes for that edge.
//
// LDS: the pair shares the tile's [32][TS] buffer of EdgeFwdSmem (same 158 720 B union with the attention layout).  The
// [16][FS] feature tiles of the two halves sit in DISJOINT regions that each lie inside the half's OWN message rows: half 0
// at floats 0 .. 719 (its message rows: 0 .. 1 087), half 1 at the END of the buffer, floats 1 456 .. 2 175 (its message
// rows: 1 088 .. 2 175).  A half's message rows therefore overwrite only its own, dead, feature tile - no ordering between
// the two waves is needed before the barrier below.
//
// Per-node means: ONE workgroup barrier between "message rows stored" and the membership product (every wave of the
// workgroup executes it - pairs without a tile and halves without an edge too), then the five output column blocks are
// split: half 0 takes j = 0, 1 and block 4 (the x_rel * coef moments) followed by the x_new update, half 1 takes j = 2, 3.
// A column block's accumulator sees the same eight ks steps in the same order as in edge_fwd_body: the same bits.
#pragma once

#define EDGE_HALF_WAVES (2 * FWD_WAVES)
#define EDGE_HALF_FEAT1 (32 * TS - 16 * FS)   /* first float of half 1's feature tile */
static_assert(16 * FS <= 16 * TS && EDGE_HALF_FEAT1 >= 16 * TS, "a half's feature tile lies inside its own message rows");

// membership product of column blocks J0, J0 + 1 (and, MOM, block 4) over the tile's 32 message rows for the 16 nodes
// nb0 .. nb0 + 15, scaled by 1 / degree and stored
template <int J0, bool MOM>
__device__ __forceinline__ void edge_half_means(const float* __restrict__ tile, float* __restrict__ sxw, int rp, float invl,
                                                int nb0, int nn, int n0, int l15, int g, float* __restrict__ aggr_msg) {
    const int node = nb0 + l15;
    const int lo = __shfl(rp, node), hi = __shfl(rp, node + 1);
    const bool nv = node < nn;
    f32x4 acc[2], accx = f4zero();
    acc[0] = acc[1] = f4zero();
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int e = 4 * ks + g;
        const float am = (nv && e >= lo && e < hi) ? 1.f : 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = mfma4(am, tile[e * TS + 16 * (J0 + j) + l15], acc[j]);
        if constexpr (MOM) accx = mfma4(am, tile[e * TS + 64 + (l15 & 3)], accx);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nd = nb0 + 4 * g + r;                 // output row of this lane
        const float inv = __shfl(invl, nd);
        if (nd < nn) {
#pragma unroll
            for (int j = 0; j < 2; ++j) aggr_msg[(size_t)(n0 + nd) * 64 + 16 * (J0 + j) + l15] = acc[j][r] * inv;
            if constexpr (MOM) {
                if (l15 < 3) sxw[3 * nd + l15] = accx[r] * inv;
            }
        }
    }
}

template <bool DROP>
__device__ __forceinline__ void edge_fwd_half_body(EdgeFwdSmem<FWD_WAVES, false>& S_, const EqdGraph& G, const EqdEdgeParams& P,
                                                   int blk, const float* __restrict__ Pn, const float* __restrict__ Qn,
                                                   const float* __restrict__ x, float* __restrict__ aggr_msg,
                                                   float* __restrict__ x_new) {
    auto& sm = S_.sm;
    EQD_TR_WG();
    EQD_TR(0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = wave & (FWD_WAVES - 1), h = wave >> 3;      // the pair is split by wave number >= 8, not by parity
    const int l15 = lane & 15, g = lane >> 4;
    float* tile = sm.tile[w];
    float* sxw = S_.sxw[w];
    // the tile's index chain (tile -> nodes -> edge range) is walked before the weights are staged, as in edge_fwd_body
    const int t = blk * FWD_WAVES + w;
    const bool live = t < G.n_tiles;      // (wave-uniform)
    int n0 = 0, n1 = 0, e0 = 0, ne = 0;
    if (live) {
        n0 = G.tile_node[t];
        n1 = G.tile_node[t + 1];
        e0 = G.rowptr[n0];
        ne = G.rowptr[n1] - e0;
    }
    edge_stage_weights<FWD_WAVES, 32 * TS, 64 * EDGE_HALF_WAVES>(sm, P);
    EQD_TR(1);
    // row pointers (one per lane) and, half 0, coordinates (3 nn <= 96 contiguous floats) of the tile's nodes: fetched now,
    // used by the aggregation behind the barrier
    const int nn = n1 - n0;   // <= 32 nodes per tile
    const size_t xo = (size_t)n0 * 3;
    const int c0 = lane, c1 = lane + 64;
    int rp = 0;
    float x0a = 0.f, xa = 0.f, x0b = 0.f, xb = 0.f;
    if (live) {
        rp = G.rowptr[n0 + (lane <= nn ? lane : 0)] - e0;
        if (h == 0) {
            x0a = G.x0[xo + (c0 < 3 * nn ? c0 : 0)], xa = x[xo + (c0 < 3 * nn ? c0 : 0)];
            x0b = G.x0[xo + (c1 < 3 * nn ? c1 : 0)], xb = x[xo + (c1 < 3 * nn ? c1 : 0)];
        }
        EdgeTileState<1> S;
        S.n0 = n0;
        S.n1 = n1;
        S.ne = ne - 16 * h;
        S.ne = S.ne < 0 ? 0 : (S.ne > 16 ? 16 : S.ne);
        S.e0 = S.ne > 0 ? e0 + 16 * h : e0;
        const int row = 16 * h + l15;
        if (S.ne > 0) {      // (wave-uniform)
            f32x4 xh[4][1], m[4][1], ch[4][1];
            edge_tile_forward<1, DROP, false>(G, P, sm.w1, sm.w2, sm.wc1, sm.vec, tile + h * EDGE_HALF_FEAT1, Pn, Qn, x, lane, S,
                                              xh, m, ch, nullptr);
            wave_lds_fence();   // this half's feature tile is dead: its message rows [edge][64 + x_moment] go over it
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
                *(float4*)&tile[row * TS + 16 * mb + 4 * g] = make_float4(m[mb][0][0], m[mb][0][1], m[mb][0][2], m[mb][0][3]);
            if (g == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) tile[row * TS + 64 + c] = S.xrel[0][c] * S.coef[0];
                tile[row * TS + 67] = 0.f;
            }
        } else {
            // a half without an edge: its rows meet membership weights of 0 only (edge_fwd_body multiplies the finite
            // rows its idle lanes compute by the same zeros), so any finite value gives the same sums
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) *(float4*)&tile[row * TS + 16 * mb + 4 * g] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g == 0) *(float4*)&tile[row * TS + 64] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    EQD_TR(10);
    __syncthreads();      // both halves' message rows are in place (the only barrier of the tile)
    if (live) {
    // per-node means as a small MFMA product (see edge_fwd_body): out[node][f] = sum_e A[node][e] tile[e][f]
    const int degl = __shfl(rp, (lane + 1) & 63) - rp;    // lane = node
    const float invl = (lane < nn && degl > 0) ? 1.f / (float)degl : 0.f;
    if (h == 0) {
        for (int nb0 = 0; nb0 < nn; nb0 += 16) edge_half_means<0, true>(tile, sxw, rp, invl, nb0, nn, n0, l15, g, aggr_msg);
        wave_lds_fence();
        if (c0 < 3 * nn) x_new[xo + c0] = P.eta * x0a + (1.f - P.eta) * xa + sxw[c0];
        if (c1 < 3 * nn) x_new[xo + c1] = P.eta * x0b + (1.f - P.eta) * xb + sxw[c1];
    } else {
        for (int nb0 = 0; nb0 < nn; nb0 += 16) edge_half_means<2, false>(tile, sxw, rp, invl, nb0, nn, n0, l15, g, aggr_msg);
    }
    }
    EQD_TR(11);
    EQD_TR_WG_END();
}

// The fused small-batch launch of a 64-wide layer on half tiles: workgroups [0, n_edge) run edge_fwd_half_body on 16
// waves, the others one attention work item as two 4-wave groups on their first 512 threads exactly as k_edge_attn_fwd
// (the other eight waves exit at once: a finished wave does not take part in the others' barriers).  Four waves per SIMD:
// 128 registers per wave, for both roles.
template <bool DROP>
__global__ __launch_bounds__(64 * EDGE_HALF_WAVES) void k_edge_attn_fwd_half(EqdGraph G, EqdEdgeParams P, int n_edge,
                                                                              const float* __restrict__ Pn,
                                                                              const float* __restrict__ Qn,
                                                                              const float* __restrict__ x,
                                                                              float* __restrict__ aggr_msg,
                                                                              float* __restrict__ x_new,
                                                                              const float* __restrict__ q,
                                                                              const float* __restrict__ k,
                                                                              const float* __restrict__ v,
                                                                              float* __restrict__ att_out,
                                                                              float* __restrict__ lse) {
    __shared__ EdgeAttnFwdSmem S;
    if ((int)blockIdx.x < n_edge) {
        edge_fwd_half_body<DROP>(S.edge, G, P, (int)blockIdx.x, Pn, Qn, x, aggr_msg, x_new);
    } else {
        if (threadIdx.x >= 512) return;
        const int half = (int)threadIdx.x >> 8;
        attn_fwd_body<4, true, 1, false, true>(S.att[half], G, (int)blockIdx.x - n_edge, half, (int)threadIdx.x & 255, 64, q, k, v,
                                  att_out, lse, true);
    }
}

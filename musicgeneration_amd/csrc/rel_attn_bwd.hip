// Fused relative global attention, backward (autograd of layers.py:86-106 of the reference).
//
// With qs = q/8 (exact pre-scale), delta = i-j, Er[delta] = E[M-1-delta]:
//     S[i,j]  = qs_i.k_j + qs_i.Er[i-j]            P = exp(S - lse_i)   (0 where masked)
//     dP[i,j] = dO_i.v_j                           dS = P o (dP - rowsum(dO o O)_i)
//     dqs_i   = sum_j dS[i,j] (k_j + Er[i-j])      dq = dqs/8
//     dk_j    = sum_i dS[i,j] qs_i                 dv_j = sum_i P[i,j] dO_i
//     dEr[dl] = sum_{b,h} sum_i dS[i,i-dl] qs_i
//
// Every output has a different "owner" axis (query row / key row / relative distance), and summing a non-owned output
// across workgroups with float atomics would cost several GB of atomic traffic per layer at cfg2.  So ONE kernel
// recomputes P and dS flash-style -- the dK/dV kernel, whose outputs need both -- and stores every bf16 dS tile (the operand
// registers of its own dK product) in the workspace; dQ and dE only need dS and are computed from the stored tiles:
//   K2  dkv_kernel   : workgroup = 128 keys, sweeps query tiles (24 MFMA / 32x32 tile); stores dS by (query tile, key tile)
//   K1L dq_lite      : workgroup = 128 query rows, sweeps the stored tiles of its rows (8 MFMA / tile, HBM-bound)
//   K3t de_tiles     : workgroup = 4 tile diagonals, un-skews the stored tiles in LDS (8 MFMA / 64 rows, HBM-bound)
//   K1  dq_kernel    : dQ by full recomputation (20 MFMA / tile) -- the round-2 kernel, kept as an independent cross-check
//   K3  de_kernel    : dE by full recomputation (24 MFMA / tile) -- cross-check (parts bit 4)
// Until round 3 dQ and dK/dV each recomputed P (two kernels x ~0.6 ms per layer at cfg2); reading dS back costs the dQ side
// 0.26 ms instead (profiles/r03_bwd_pipeline_ab.txt).  The skew between (i,j) tiles and (i,delta) chunks is done through LDS
// (rel_attn_common.hpp); the only L x L object that ever exists is the bf16 dS workspace (causal half, tile-blocked),
// written once and read twice per layer.
//
// This file: the pre-pass kernel and the host side (argument checks, workspace layout, launch plan, entry points).  One file per kernel,
// each with its launcher (rel_attn_common.hpp): rel_attn_dkv32.hip (K2), rel_attn_dkv64.hip (K2 for L % 128 == 0: 64 keys per wave, generated
// asm sweep), rel_attn_dq_lite.hip (K1L), rel_attn_de_tiles.hip (K3t), rel_attn_bwd_recompute.hip (K1, K3: cross-checks only).
#include "rel_attn_common.hpp"

using namespace relattn;

// the pre-pass: delta[b,h,i] = sum_c dctx[b,i,h*64+c] * ctx[b,i,h*64+c]         (8 lanes per (row, head))
__global__ __launch_bounds__(256) void attn_delta_kernel(const uint16_t* __restrict__ ctx,
                                                         const uint16_t* __restrict__ dctx, const float* __restrict__ lse,
                                                         float* __restrict__ delta, float* __restrict__ nlse2,
                                                         float* __restrict__ ndelta, int B, int L, int d) {
    const int heads = d >> 6;
    const long total = (long)B * L * heads * 8;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;   // total is a multiple of 8 and blockDim of 64: whole 8-lane groups exit together
    const int sub = (int)(gid & 7);
    // group g = ((b * heads + hd) * L + i): consecutive 8-lane groups are consecutive rows i of ONE head, so the per-row results
    // are written (and lse is read) contiguously -- with the head on the fast axis (rounds 1-3) every 4-byte store went to its own
    // cache line.  The 128-byte reads of ctx / dctx are whole lines either way.
    const long grp = gid >> 3;
    const int i = (int)(grp % L);
    const int hd = (int)((grp / L) % heads);
    const long row = (grp / ((long)L * heads)) * L + i;      // b*L + i
    const size_t off = (size_t)row * d + hd * 64 + sub * 8;
    float a[8], g[8];
    unpack8(*(const u32x4*)(ctx + off), a);
    unpack8(*(const u32x4*)(dctx + off), g);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += a[k] * g[k];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (sub == 0) {
        const size_t si = (size_t)grp;
        delta[si] = s;
        // the dK/dV kernel's copies, in the form it consumes them (the initial accumulators of its S and dP products), so
        // that its LDS-DMA staging needs no arithmetic on the way
        ndelta[si] = -s;
        nlse2[si] = -lse[si] * LOG2E;
    }
}

// ---- workspace layout: byte offsets from the 256-byte aligned base -----------------------------------------------------------
// delta, -lse log2e, -delta: f32 [B,h,L] each (the pre-pass writes all three; the last two in the form the dK/dV kernels consume) |
// EfA, EfT: the fragment-ordered copies of Er (rel_attn_common.hpp) | the causal half of dS by (query tile, key tile), bf16:
// B*h*T tiles of 2 KB, T = nchunk (nchunk + 1) / 2
struct BwdWorkspace { size_t delta, nlse2, ndelta, EfA, EfT, dS, total; };
static BwdWorkspace bwd_workspace(int B, int L, int d) {
    const size_t stat = (((size_t)B * (d / 64) * L * 4) + 255) / 256 * 256, ef = er_frag_bytes(L), nchunk = (size_t)L / 32;
    const size_t dS = 3 * stat + 2 * ef;
    return {0, stat, 2 * stat, 3 * stat, 3 * stat + ef, dS, dS + (size_t)B * (d / 64) * (nchunk * (nchunk + 1) / 2) * 2048};
}

extern "C" size_t mgx_rel_attn_bwd_workspace(int B, int L, int d) { return (B <= 0 || L <= 0 || d <= 0) ? 0 : bwd_workspace(B, L, d).total; }

// ---- launch plan: everything the launches need that depends on the shape, and every shape refusal, before anything is in the stream --
struct BwdPlan {
    int bg;              // batch rows per grid group (q, k, v, ctx, dO: five tensors per row)
    bool dkv64;          // bit 2 and whole 128-key blocks: the 64-keys-per-wave asm kernel (rel_attn_dkv64.hip); otherwise, and for bit 6 whatever
                         // the shape, the 32-key kernel: same bits.  (The A/B switch that sent bit 2 there for every shape is retired: bit 6 does it.)
    dim3 grid;           // x = (b,h) of a batch group, y = (batch group, 128-row block): dQ kernels (query blocks) and 32-key dK/dV (key blocks)
    DeTilesPlan de;      // the dE grouping (parts bit 8 only)
};
static int bwd_plan(BwdPlan& p, int B, int L, int d, int parts) {
    p.bg = batch_group(B, L, d, 5);
    MGX_REQUIRE((long)((L + 127) / 128) * (B / p.bg) <= 65535, MGX_ERR_SHAPE, "mgx_rel_attn_bwd: L/128 * batch groups too large");
    p.grid = dim3(p.bg * (d / 64), ((L + 127) / 128) * (B / p.bg));
    MGX_REQUIRE(!((parts & 4) && (parts & 64)), MGX_ERR_SHAPE, "mgx_rel_attn_bwd: parts 4 and 64 both write dk / dv and the dS tiles");
    p.dkv64 = (parts & 4) && L % 128 == 0;
    if (parts & 8) {
        p.de = de_tiles_plan(B, L, d, p.bg);
        MGX_REQUIRE(p.de.grid < (1L << 31), MGX_ERR_SHAPE, "mgx_rel_attn_bwd: grid too large");
    }
    return MGX_OK;
}

// parts: 1 pre-pass (delta, E re-layout) | 4 dK/dV (stores the dS tiles) | 2 dQ from the stored tiles | 8 dE from the stored
// tiles | 16 dE by recomputation | 32 dQ by recomputation (16, 32: independent of the stored tiles; cross-checks / A-B
// timing) | 64 dK/dV by the 32-key kernel whatever the shape (instead of 4; cross-check of the 64-key kernel).  Launch order inside
// one call: 1, 4 (or 64), 2 (or 32), 8, 16.
extern "C" int mgx_rel_attn_bwd_parts(const uint16_t* qkv, const uint16_t* E, const uint32_t* padbits,
                                      const uint16_t* ctx, const uint16_t* dctx, const float* lse, uint16_t* dqkv,
                                      float* dE, void* workspace, size_t ws_bytes, int B, int L, int d, int M,
                                      int parts, void* stream) {
    MGX_REQUIRE(qkv && E && ctx && dctx && lse && dqkv && dE && workspace, MGX_ERR_NULL, "mgx_rel_attn_bwd: NULL pointer");
    MGX_REQUIRE(B > 0 && L > 0 && d > 0 && d % 64 == 0 && L % 32 == 0 && M >= L, MGX_ERR_SHAPE,
                "mgx_rel_attn_bwd: need d%%64==0, L%%32==0, M>=L (got B=%d L=%d d=%d M=%d)", B, L, d, M);
    const BwdWorkspace ws = bwd_workspace(B, L, d);
    MGX_REQUIRE(ws_bytes >= ws.total && ((uintptr_t)workspace & 255) == 0, MGX_ERR_SHAPE,
                "mgx_rel_attn_bwd: workspace must be 256-byte aligned and >= mgx_rel_attn_bwd_workspace() = %zu bytes (got %zu)", ws.total, ws_bytes);
    MGX_REQUIRE(!((parts & 2) && (parts & 32)), MGX_ERR_SHAPE, "mgx_rel_attn_bwd: parts 2 and 32 both write dq");
    BwdPlan p;
    if (int rc = bwd_plan(p, B, L, d, parts)) return rc;

    char* const base = (char*)workspace;
    float *delta = (float*)(base + ws.delta), *nlse2 = (float*)(base + ws.nlse2), *ndelta = (float*)(base + ws.ndelta);
    u32x4 *EfA = (u32x4*)(base + ws.EfA), *EfT = (u32x4*)(base + ws.EfT);
    uint16_t* dst = (uint16_t*)(base + ws.dS);                     // the dS tiles
    const uint16_t* Er = E + (size_t)(M - L) * 64;
    float* dEr = dE + (size_t)(M - L) * 64;
    if (parts & 1) {
        // delta = rowsum(dO o O) for the kernels that form dS (dK/dV and the two recompute cross-checks)
        const long total = (long)B * L * (d / 64) * 8;
        hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctx, dctx, lse,
                           delta, nlse2, ndelta, B, L, d);
        launch_er_frag(Er, EfA, EfT, L, (hipStream_t)stream);
    }
    if (p.dkv64) {
        if (int rc = dkv64_launch(qkv, EfA, padbits, dctx, nlse2, ndelta, dqkv, dst, B, L, d, p.bg, stream)) return rc;
    } else if (parts & (4 | 64)) {
        dkv32_launch(qkv, EfA, padbits, dctx, nlse2, ndelta, dqkv, dst, p.grid, L, d, p.bg, stream);
    }
    if (parts & 2) dq_lite_launch(qkv, EfT, dst, dqkv, p.grid, L, d, p.bg, stream);
    if (parts & 32) dq_recompute_launch(qkv, EfA, EfT, padbits, dctx, lse, delta, dqkv, p.grid, L, d, p.bg, stream);
    if (parts & 8)
        if (int rc = de_tiles_launch(qkv, dst, dEr, p.de, L, d, stream)) return rc;
    if (parts & 16) de_recompute_launch(qkv, Er, padbits, dctx, lse, delta, dEr, B, L, d, stream);
    MGX_CHECK_LAUNCH("mgx_rel_attn_bwd");
    return MGX_OK;
}

extern "C" int mgx_rel_attn_bwd(const uint16_t* qkv, const uint16_t* E, const uint32_t* padbits, const uint16_t* ctx,
                                const uint16_t* dctx, const float* lse, uint16_t* dqkv, float* dE, void* workspace,
                                size_t ws_bytes, int B, int L, int d, int M, void* stream) {
    return mgx_rel_attn_bwd_parts(qkv, E, padbits, ctx, dctx, lse, dqkv, dE, workspace, ws_bytes, B, L, d, M, 15, stream);
}

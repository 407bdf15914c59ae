// =================================================================================================
// skinny forward (M <= 32: the decode path's projections).  The weights are streamed exactly once:
// workgroup = 32 output columns, its 4 waves split K; W rows and x rows go straight from global/L2 into
// MFMA fragments (no LDS staging, no barriers in the loop); the four partial tiles are combined in LDS.
//   D[n][m] = sum_k W[n][k] x[m][k]   (A = W rows, B = x^T)
// Three kernels share that frame and differ in where x comes from: memory, a LayerNorm, the embedding.
// =================================================================================================
#include <limits.h>
#include "linear_common.hpp"

using namespace relattn;

// what a lane works on: row n0 + l31 of W against row l31 of x, columns w * kq + 8 hh + 16 f .. + 7 (kq = K / 4 per wave, f = 0 ..)
struct SkinnyLane {
    int tid, w, l31, hh, n0, kq;
    bool nv, mv;                                           // the lane's W row / x row exists
};
template <bool FRAG>
MGX_DEV SkinnyLane skinny_lane(int M, int N, int K) {
    SkinnyLane s;
    s.tid = threadIdx.x;
    const int lane = s.tid & 63;
    s.w = __builtin_amdgcn_readfirstlane(s.tid >> 6);
    s.l31 = lane & 31; s.hh = lane >> 5;
    s.n0 = blockIdx.x * 32;
    s.kq = K >> 2;                                         // K per wave (multiple of 16)
    s.nv = FRAG || s.n0 + s.l31 < N; s.mv = s.l31 < M;
    return s;
}
// The lane's first weight fragment.  FRAG: W is in MFMA fragment order (mgx.h: unit ((nt*K/16 + ks)*64 + lane) = W[32 nt + lane%32]
// [16 ks + 8 (lane/32) ..+7], rows padded with zeros to a multiple of 32): a wave load is 1 KB contiguous instead of 32 B of 32
// different rows, and consecutive k-steps are 512 elements apart instead of 16.
template <bool FRAG>
MGX_DEV const uint16_t* skinny_wptr(const uint16_t* W, const SkinnyLane& s, int K) {
    return FRAG ? W + (((size_t)blockIdx.x * (K >> 4) + (size_t)(s.w * s.kq >> 4)) * 64 + (s.tid & 63)) * 8      // (tid & 63: the lane)
                : W + (size_t)(s.nv ? s.n0 + s.l31 : 0) * K + s.w * s.kq + s.hh * 8;
}
// The waves' partial tiles -> C = act(sum + bias), through LDS ([n][m]); thread -> (n = tid >> 3, 4 consecutive m), inside M and N
MGX_DEV void skinny_store(const f32x16& acc, const SkinnyLane& s, const float* __restrict__ bias, int act,
                          uint16_t* __restrict__ C, int M, int N) {
    __shared__ float part[4][32][33];
#pragma unroll
    for (int r = 0; r < 16; ++r) part[s.w][crow(r, s.hh)][s.l31] = acc[r];
    __syncthreads();
    const int n = s.tid >> 3, m4 = (s.tid & 7) * 4;
    if (s.n0 + n >= N) return;
    const float bv = bias ? bias[s.n0 + n] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int m = m4 + k;
        if (m < M) {
            float v = part[0][n][m] + part[1][n][m] + part[2][n][m] + part[3][n][m] + bv;
            if (act == 1) v = relu_f32(v);
            C[(size_t)m * N + s.n0 + n] = f32_to_bf16(v);
        }
    }
}

template <bool FRAG>
__global__ __launch_bounds__(256) void linear_skinny_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ W,
                                                            const float* __restrict__ bias, uint16_t* __restrict__ C,
                                                            int M, int N, int K, int act) {
    const SkinnyLane s = skinny_lane<FRAG>(M, N, K);
    const int w = s.w, hh = s.hh, kq = s.kq;
    const bool nv = s.nv, mv = s.mv;
    const uint16_t* wp = skinny_wptr<FRAG>(W, s, K);
    const int wstep = FRAG ? 512 : 16;                       // elements between consecutive k-steps
    const uint16_t* xp = A + (size_t)(mv ? s.l31 : 0) * K + w * kq + hh * 8;
    f32x16 acc = zero16();
    for (int k0 = 0; k0 < kq; k0 += 128) {                   // 8 k-steps per trip: all 16 loads of a K <= 512 projection at once
        u32x4 wf[8], xf[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const bool in = k0 + 16 * ks < kq;
            wf[ks] = (nv && in) ? *(const u32x4*)(wp + (size_t)((k0 >> 4) + ks) * wstep) : u32x4{0, 0, 0, 0};
            xf[ks] = (mv && in) ? *(const u32x4*)(xp + k0 + 16 * ks) : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            acc = mfma(__builtin_bit_cast(bf16x8, wf[ks]), __builtin_bit_cast(bf16x8, xf[ks]), acc);
    }
    skinny_store(acc, s, bias, act, C, M, N);
}

// =================================================================================================
// skinny forward with a LayerNorm prologue (decode path): Z = LN(X + RES) (layers.py:154-155,159-160, eps 1e-6, no
// dropout in eval) and C = act(Z W^T + b) in ONE launch.  Every workgroup owns 32 output columns and, like the kernel
// above, reads all M <= 32 rows of its operand anyway, so it normalises them itself (row statistics reduced across
// its 4 k-slices through LDS); workgroup 0 also writes Z, which the next LayerNorm needs as its residual.  Removes
// the 12 LayerNorm launches of a decode step (each ~4.6 us at the launch floor).  K <= 1024.
// =================================================================================================
constexpr int SKLN_MAXF = 16;                              // 16-column fragments per wave: K/4/16 <= 16
template <bool FRAG>
__global__ __launch_bounds__(256) void linear_skinny_ln_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ RES,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float eps, const uint16_t* __restrict__ W,
                                                               const float* __restrict__ bias, uint16_t* __restrict__ C,
                                                               uint16_t* __restrict__ Z, int M, int N, int K, int act) {
    __shared__ float stat[2][4][32];
    const SkinnyLane s = skinny_lane<FRAG>(M, N, K);
    const int w = s.w, l31 = s.l31, hh = s.hh;
    const int kq = s.kq, nf = kq >> 4;                               // fragments of 16 columns per wave
    const bool nv = s.nv, mv = s.mv;
    const size_t xoff = (size_t)(mv ? l31 : 0) * K + w * kq + hh * 8;
    float z[SKLN_MAXF][8];
    float s1 = 0.f;
    // the weight fragments are requested first: their latency hides under the statistics
    const uint16_t* wp = skinny_wptr<FRAG>(W, s, K);
    const int wstep = FRAG ? 512 : 16;
    u32x4 wf[SKLN_MAXF];
#pragma unroll
    for (int f = 0; f < SKLN_MAXF; ++f)
        if (f < nf) wf[f] = nv ? *(const u32x4*)(wp + (size_t)f * wstep) : u32x4{0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < SKLN_MAXF; ++f) {
        if (f < nf) {
            float a[8], r[8];
            unpack8(mv ? *(const u32x4*)(X + xoff + 16 * f) : u32x4{0, 0, 0, 0}, a);
            unpack8(mv ? *(const u32x4*)(RES + xoff + 16 * f) : u32x4{0, 0, 0, 0}, r);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                z[f][k] = a[k] + r[k];
                s1 += z[f][k];
            }
        }
    }
    // the statistics in two passes over the registers, as the training kernel (rowwise_ops.hip) takes them: the variance is the
    // mean of (z - mean)^2.  E[z^2] - mean^2 in one pass loses |mean| / std squared in relative accuracy (a row of mean 60 and
    // std 0.25: rstd off by 6e-3); the second LDS exchange and barrier cost 0.7 % of a cfg5 decode step (profiles/README.md)
    s1 += __shfl_xor(s1, 32, 64);
    if (hh == 0) stat[0][w][l31] = s1;
    __syncthreads();
    const float mean = (stat[0][0][l31] + stat[0][1][l31] + stat[0][2][l31] + stat[0][3][l31]) / (float)K;
    float s2 = 0.f;
#pragma unroll
    for (int f = 0; f < SKLN_MAXF; ++f) {
        if (f < nf) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float c = z[f][k] - mean; s2 += c * c; }
        }
    }
    s2 += __shfl_xor(s2, 32, 64);
    if (hh == 0) stat[1][w][l31] = s2;
    __syncthreads();
    const float rstd = rsqrtf((stat[1][0][l31] + stat[1][1][l31] + stat[1][2][l31] + stat[1][3][l31]) / (float)K + eps);
    f32x16 acc = zero16();
#pragma unroll
    for (int f = 0; f < SKLN_MAXF; ++f) {
        if (f < nf) {
            const int kc = w * kq + hh * 8 + 16 * f;
            const f32x4 g0 = *(const f32x4*)(gamma + kc), g1 = *(const f32x4*)(gamma + kc + 4);
            const f32x4 b0 = *(const f32x4*)(beta + kc), b1 = *(const f32x4*)(beta + kc + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            float y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] = (z[f][k] - mean) * rstd * gg[k] + bb[k];
            const u32x4 yf = pack8(y);
            if (blockIdx.x == 0 && mv) *(u32x4*)(Z + xoff + 16 * f) = yf;
            acc = mfma(__builtin_bit_cast(bf16x8, wf[f]), __builtin_bit_cast(bf16x8, mv ? yf : u32x4{0, 0, 0, 0}), acc);
        }
    }
    skinny_store(acc, s, bias, act, C, M, N);
}

// =================================================================================================
// Decode-step fusion (M <= 32 rows = the decode batch): linear_skinny_embed_kernel computes H = emb[tok] sqrt(d) + PE[t]
// (layers.py:226-229) inside the first QKV projection (8.4 us against 4.7 + 5.2 us for the two launches).
// Two further fusions were built and measured in round 3 and are NOT kept (profiles/README.md): the split-K attention merge
// inside the output projection (16.7 us against 4.8 + 5.2: the fp32 partials are 8x the bytes of the bf16 context row and
// every workgroup re-merges them) and LN1 + FFN_pre + ReLU + FFN_suf in one launch with the hidden layer recomputed per
// workgroup (47 us against 9.4 + 5.2: 16 workgroups each stream all of W1 behind a 32-row operand with ~8 KB in flight per
// wave -- the chain is bound by dependent L2 round trips, and recomputation multiplies them).
// =================================================================================================
// stp: the rows' position(s), one shared counter or one per row (StepPos, mgx_common.hpp).
template <bool FRAG>
__global__ __launch_bounds__(256) void linear_skinny_embed_kernel(const int32_t* __restrict__ tok, const float* __restrict__ table,
                                                                  const float* __restrict__ pe, StepPos stp,
                                                                  const uint16_t* __restrict__ W, const float* __restrict__ bias,
                                                                  uint16_t* __restrict__ C, uint16_t* __restrict__ H, int M, int N,
                                                                  int K, int V, float scale) {
    const SkinnyLane s = skinny_lane<FRAG>(M, N, K);
    const int w = s.w, hh = s.hh, kq = s.kq, mrow = s.l31;
    const bool nv = s.nv, mv = s.mv;
    int t = tok[mv ? mrow : 0];
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);
    const int pos = stp.at(mv ? mrow : 0);
    const float* tp = table + (size_t)t * K + w * kq + hh * 8;
    const float* pp = pe + (size_t)pos * K + w * kq + hh * 8;
    const uint16_t* wp = skinny_wptr<FRAG>(W, s, K);
    const int wstep = FRAG ? 32 : 1;                         // elements per unit of k
    f32x16 acc = zero16();
    for (int k0 = 0; k0 < kq; k0 += 16) {
        const u32x4 wf = nv ? *(const u32x4*)(wp + (size_t)k0 * wstep) : u32x4{0, 0, 0, 0};
        const f32x4 a0 = *(const f32x4*)(tp + k0), a1 = *(const f32x4*)(tp + k0 + 4);
        const f32x4 p0 = *(const f32x4*)(pp + k0), p1 = *(const f32x4*)(pp + k0 + 4);
        const float f[8] = {a0.x * scale + p0.x, a0.y * scale + p0.y, a0.z * scale + p0.z, a0.w * scale + p0.w,
                            a1.x * scale + p1.x, a1.y * scale + p1.y, a1.z * scale + p1.z, a1.w * scale + p1.w};
        const u32x4 xf = mv ? pack8(f) : u32x4{0, 0, 0, 0};
        if (blockIdx.x == 0 && mv) *(u32x4*)(H + (size_t)mrow * K + w * kq + hh * 8 + k0) = xf;
        acc = mfma(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, xf), acc);
    }
    skinny_store(acc, s, bias, 0, C, M, N);
}

// ---- entry points: none of them chooses a kernel.  One check and one launch (32 output columns per workgroup) for all of them ----
static int skinny_check(const char* name, bool ptrs, int M, int N, int K, int act, int kmax = INT_MAX) {
    MGX_REQUIRE(ptrs, MGX_ERR_NULL, "%s: NULL pointer", name);
    MGX_REQUIRE(M > 0 && M <= 32 && N > 0 && K > 0 && K % 64 == 0, MGX_ERR_SHAPE, "%s: need 0<M<=32, K%%64==0 (got M=%d N=%d K=%d)", name, M, N, K);
    MGX_REQUIRE(K <= kmax, MGX_ERR_SHAPE, "%s: need K<=%d (got K=%d)", name, kmax, K);
    MGX_REQUIRE(act == 0 || act == 1, MGX_ERR_SHAPE, "%s: act must be 0 (none) or 1 (ReLU)", name);
    return MGX_OK;
}
template <typename... P, typename... A>
static int skinny_launch(const char* name, void (*kernel)(P...), int N, void* stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3((N + 31) / 32), dim3(256), 0, (hipStream_t)stream, args...);
    MGX_CHECK_LAUNCH(name);
    return MGX_OK;
}

void mgx_gemm::skinny_fwd(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* C, int M, int N, int K, int act, void* stream) {
    hipLaunchKernelGGL(linear_skinny_kernel<false>, dim3((N + 31) / 32), dim3(256), 0, (hipStream_t)stream, A, W, bias, C, M, N, K, act);
}

// ---- decode-size projections with the weight in MFMA fragment order (mgx.h; rows zero-padded to a multiple of 32) --------------
extern "C" int mgx_skinny_fwd_frag(const uint16_t* A, const uint16_t* Wf, const float* bias, uint16_t* C, int M, int N, int K, int act,
                                   void* stream) {
    if (int rc = skinny_check("mgx_skinny_fwd_frag", A && Wf && C, M, N, K, act)) return rc;
    return skinny_launch("mgx_skinny_fwd_frag", linear_skinny_kernel<true>, N, stream, A, Wf, bias, C, M, N, K, act);
}

template <bool FRAG>
static int linear_ln_fwd(const uint16_t* X, const uint16_t* RES, const float* gamma, const float* beta, float eps, const uint16_t* W,
                         const float* bias, uint16_t* C, uint16_t* Z, int M, int N, int K, int act, void* stream, const char* name) {
    if (int rc = skinny_check(name, X && RES && gamma && beta && W && C && Z, M, N, K, act, 64 * SKLN_MAXF)) return rc;
    return skinny_launch(name, linear_skinny_ln_kernel<FRAG>, N, stream, X, RES, gamma, beta, eps, W, bias, C, Z, M, N, K, act);
}
extern "C" int mgx_linear_ln_fwd(const uint16_t* X, const uint16_t* RES, const float* gamma, const float* beta, float eps, const uint16_t* W,
                                 const float* bias, uint16_t* C, uint16_t* Z, int M, int N, int K, int act, void* stream) {
    return linear_ln_fwd<false>(X, RES, gamma, beta, eps, W, bias, C, Z, M, N, K, act, stream, "mgx_linear_ln_fwd");
}
extern "C" int mgx_linear_ln_fwd_frag(const uint16_t* X, const uint16_t* RES, const float* gamma, const float* beta, float eps, const uint16_t* Wf,
                                      const float* bias, uint16_t* C, uint16_t* Z, int M, int N, int K, int act, void* stream) {
    return linear_ln_fwd<true>(X, RES, gamma, beta, eps, Wf, bias, C, Z, M, N, K, act, stream, "mgx_linear_ln_fwd_frag");
}

// the two fused-embedding entry points: W row-major or (FRAG) in MFMA fragment order
template <bool FRAG>
static int decode_embed_linear(const int32_t* tok, const float* table, const float* pe, const int32_t* pos_dev, int per_row, const uint16_t* W,
                               const float* bias, uint16_t* C, uint16_t* H, int M, int N, int K, int V, void* stream, const char* name) {
    if (int rc = skinny_check(name, tok && table && pe && pos_dev && W && C && H, M, N, K, 0)) return rc;
    MGX_REQUIRE(V > 0, MGX_ERR_SHAPE, "%s: need V>0 (got %d)", name, V);
    return skinny_launch(name, linear_skinny_embed_kernel<FRAG>, N, stream, tok, table, pe, StepPos{pos_dev, nullptr, per_row}, W, bias, C, H,
                         M, N, K, V, sqrtf((float)K));
}
extern "C" int mgx_decode_embed_linear(const int32_t* tok, const float* table, const float* pe, const int32_t* pos_dev, int per_row,
                                       const uint16_t* W, const float* bias, uint16_t* C, uint16_t* H, int M, int N, int K, int V, void* stream) {
    return decode_embed_linear<false>(tok, table, pe, pos_dev, per_row, W, bias, C, H, M, N, K, V, stream, "mgx_decode_embed_linear");
}
extern "C" int mgx_decode_embed_linear_frag(const int32_t* tok, const float* table, const float* pe, const int32_t* pos_dev, int per_row,
                                            const uint16_t* Wf, const float* bias, uint16_t* C, uint16_t* H, int M, int N, int K, int V,
                                            void* stream) {
    return decode_embed_linear<true>(tok, table, pe, pos_dev, per_row, Wf, bias, C, H, M, N, K, V, stream, "mgx_decode_embed_linear_frag");
}

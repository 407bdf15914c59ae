// Scoring: the log-probability a model gives to every event of a sequence (ABI 24; contracts in include/mgx.h).
//
//   mgx_token_logprob    row-wise on logits that exist (bf16): one wave per row, two sweeps of the row -- the masked maximum, then
//                        the sum, the first id at the maximum and the non-finite flag.  Any V: nothing is kept in registers.
//   mgx_linear_logprob   the vocabulary projection and its log-softmax gather in one kernel; the logits stay in the MFMA
//                        accumulators.  A workgroup owns 32 rows of A, staged once in LDS, and its four waves walk V in tiles of
//                        32 ids (wave w: tiles w, w + 4, ...).  The product is taken as D[v][m] = sum_k W[v][k] A[m][k], so a
//                        lane holds 16 ids of ONE row m (C/D map: column = lane & 31, rows crow(r, lane >> 5)): the row reduction
//                        is 16 registers, then lane ^ 32, then the four waves through LDS.  Every lane carries a running
//                        (max, sum, target logit, arg-max, non-finite flag) across its tiles.
//   mgx_score_reduce     per-sequence totals, one workgroup per sequence, fp64, in a fixed order.
//
// The definitions follow criterion.py:43-67 (the log-softmax and the gather of the target's entry, without the label smoothing)
// and metrics.py:40-52 (the arg-max against the target).
#include <limits.h>
#include "rel_attn_common.hpp"
#include "logit_row.hpp"                                  // the grammar row and its bit test

using namespace relattn;

namespace {
constexpr int SCORE_WAVES = 4;
constexpr int LL_ROWS = 32;               // rows of A per workgroup of mgx_linear_logprob
constexpr int LL_KMAX = 1024;             // 32 rows x 1024 x 2 B = 64 KB of LDS

MGX_DEV int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(64 * SCORE_WAVES) void token_logprob_kernel(
    const uint16_t* __restrict__ logits, int V, int ld, const int32_t* __restrict__ target, const int32_t* __restrict__ prev,
    const uint32_t* __restrict__ allow_table, float inv_temp, float* __restrict__ logp, float* __restrict__ lse_out,
    int32_t* __restrict__ hit, int rows) {
    // every product rounded on its own: x_v = logit_v * (1 / temperature) is the header's definition
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;                                  // wave-uniform
    const uint16_t* lp = logits + (size_t)row * ld;
    const uint32_t* arow = allow_table ? grammar_row(allow_table, prev[row], V) : nullptr;
    // sweep 1: the maximum over the allowed ids (fmaxf: a NaN never is the maximum)
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64)
        if (allowed(arow, v)) mx = fmaxf(mx, bf16_to_f32(lp[v]));
    mx = wave_max(mx);
    if (arow && mx == -INFINITY) {                            // a grammar row that leaves no finite logit is ignored
        arow = nullptr;
        for (int v = lane; v < V; v += 64) mx = fmaxf(mx, bf16_to_f32(lp[v]));
        mx = wave_max(mx);
    }
    // sweep 2: the sum, the smallest id at the maximum, and whether a NaN or +inf is among the allowed logits
    const float xm = mx * inv_temp;
    float sum = 0.f, bad = 0.f;
    int first = INT_MAX;
    for (int v = lane; v < V; v += 64) {
        if (!allowed(arow, v)) continue;
        const float val = bf16_to_f32(lp[v]);
        if (!(val < INFINITY)) bad = 1.f;
        if (val == mx && v < first) first = v;
        sum += expf(val * inv_temp - xm);                     // all -inf: -inf - -inf = NaN, and the row is NaN as the header says
    }
    sum = wave_sum(sum);
    bad = wave_max(bad);
    first = wave_min_i32(first);
    if (lane != 0) return;
    float lse = xm + logf(sum);
    if (bad != 0.f || !(mx > -INFINITY)) lse = __builtin_nanf("");
    if (lse_out) lse_out[row] = lse;
    const int t = target[row];
    if (t < 0 || t >= V) {                                    // unscored
        logp[row] = 0.f;
        hit[row] = -1;
        return;
    }
    const bool ok = allowed(arow, t);
    const float xt = ok ? bf16_to_f32(lp[t]) * inv_temp : -INFINITY;
    logp[row] = xt - lse;
    hit[row] = (ok && first == t) ? 1 : 0;
}

// a lane's (or a row's) running state over the ids it has seen
struct RowState {
    float mx, sum, xt, best;
    int besti, bad;
};
// b's ids come after a's nowhere in particular: the arg-max is decided by (value, smaller id), the sum is rescaled to the joint maximum
MGX_DEV RowState merge(const RowState& a, const RowState& b) {
    RowState r;
    r.mx = fmaxf(a.mx, b.mx);
    r.sum = (a.mx > -INFINITY ? a.sum * expf(a.mx - r.mx) : 0.f) + (b.mx > -INFINITY ? b.sum * expf(b.mx - r.mx) : 0.f);
    // one side holds the target's logit, the other -inf.  fmaxf drops a NaN target logit; such a row has its bad flag set (the
    // target is one of the row's ids), which makes lse and with it logp NaN whatever xt is
    r.xt = fmaxf(a.xt, b.xt);
    const bool tb = b.best > a.best || (b.best == a.best && b.besti < a.besti);
    r.best = tb ? b.best : a.best;
    r.besti = tb ? b.besti : a.besti;
    r.bad = a.bad | b.bad;
    return r;
}

__global__ __launch_bounds__(64 * SCORE_WAVES) void linear_logprob_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ W, const float* __restrict__ bias,
    const int32_t* __restrict__ target, float inv_temp, float* __restrict__ logp, float* __restrict__ lse_out,
    int32_t* __restrict__ hit, int M, int V, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * LL_ROWS;
    // A's row block -> LDS, rows of K bf16 in 16-byte chunks, the chunk index XORed with the row's low three bits (K / 8 is a
    // multiple of 8, so a chunk stays inside its row): the rows of a fragment read -- one chunk index, all rows -- spread over the banks
    const int kc = K >> 3, swz = 7;
    for (int idx = tid; idx < LL_ROWS * kc; idx += 64 * SCORE_WAVES) {
        const int row = idx / kc, c = idx - row * kc;
        const u32x4 v = (m0 + row < M) ? *(const u32x4*)(A + (size_t)(m0 + row) * K + c * 8) : u32x4{0, 0, 0, 0};
        *(u32x4*)(smem + (size_t)row * K * 2 + ((c ^ (row & swz)) << 4)) = v;
    }
    __syncthreads();
    const int m = m0 + l31;
    int t = m < M ? target[m] : -1;
    if (t >= V) t = -1;
    const char* arow = smem + (size_t)l31 * K * 2;
    const int asw = l31 & swz;
    RowState st = {-INFINITY, 0.f, -INFINITY, -INFINITY, INT_MAX, 0};
    for (int n0 = w * 32; n0 < V; n0 += 32 * SCORE_WAVES) {
        const bool nv = n0 + l31 < V;                         // rows >= V of W are never read
        const uint16_t* wp = W + (size_t)(nv ? n0 + l31 : 0) * K + hh * 8;
        f32x16 acc = zero16();
        for (int ks = 0; ks < (K >> 4); ks += 4) {            // K % 64 == 0: four k-steps per trip, their loads first
            u32x4 wf[4], xf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                wf[u] = nv ? *(const u32x4*)(wp + (size_t)(ks + u) * 16) : u32x4{0, 0, 0, 0};
                xf[u] = *(const u32x4*)(arow + (((2 * (ks + u) + hh) ^ asw) << 4));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = mfma(__builtin_bit_cast(bf16x8, wf[u]), __builtin_bit_cast(bf16x8, xf[u]), acc);
        }
        // the tile's 16 ids of this lane's row, in ascending id order; ids >= V are masked before the maximum and the sum
        float x[16], tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int v = n0 + crow(r, hh);
            const bool in = v < V;
            x[r] = in ? (acc[r] + (bias ? bias[v] : 0.f)) * inv_temp : -INFINITY;
            if (in && !(x[r] < INFINITY)) st.bad = 1;         // NaN or +inf
            if (in && v == t) st.xt = x[r];
            if (x[r] > st.best) { st.best = x[r]; st.besti = v; }      // strictly: the smaller id stays among equals
            tmax = fmaxf(tmax, x[r]);
        }
        const float nm = fmaxf(st.mx, tmax);
        if (nm > -INFINITY) {
            float s = st.mx > -INFINITY ? st.sum * expf(st.mx - nm) : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s += expf(x[r] - nm);         // exp(-inf) = 0
            st.sum = s;
            st.mx = nm;
        }
    }
    // the two half-waves hold disjoint ids of the same row
    RowState o;
    o.mx = __shfl_xor(st.mx, 32, 64); o.sum = __shfl_xor(st.sum, 32, 64); o.xt = __shfl_xor(st.xt, 32, 64);
    o.best = __shfl_xor(st.best, 32, 64); o.besti = __shfl_xor(st.besti, 32, 64); o.bad = __shfl_xor(st.bad, 32, 64);
    st = hh == 0 ? merge(st, o) : merge(o, st);
    __syncthreads();                                          // every wave is done with A's block: its LDS is reused
    RowState* part = (RowState*)smem;                         // [wave][row], 4 x 32 x 24 B
    if (hh == 0) part[w * LL_ROWS + l31] = st;
    __syncthreads();
    if (w != 0 || hh != 0 || m >= M) return;
    st = merge(merge(part[l31], part[LL_ROWS + l31]), merge(part[2 * LL_ROWS + l31], part[3 * LL_ROWS + l31]));
    float lse = st.mx + logf(st.sum);
    if (st.bad || !(st.mx > -INFINITY)) lse = __builtin_nanf("");
    if (lse_out) lse_out[m] = lse;
    if (t < 0) {                                              // unscored
        logp[m] = 0.f;
        hit[m] = -1;
        return;
    }
    logp[m] = st.xt - lse;
    hit[m] = st.besti == t ? 1 : 0;
}

constexpr int REDUCE_THREADS = 256;
__global__ __launch_bounds__(REDUCE_THREADS) void score_reduce_kernel(const float* __restrict__ logp, const int32_t* __restrict__ hit,
                                                                      double* __restrict__ sum, int32_t* __restrict__ count,
                                                                      int32_t* __restrict__ hits, int L) {
    __shared__ double s_sum[REDUCE_THREADS];
    __shared__ int s_cnt[REDUCE_THREADS], s_hit[REDUCE_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* lp = logp + (size_t)b * L;
    const int32_t* hp = hit + (size_t)b * L;
    double s = 0.0;
    int c = 0, h = 0;
    for (int i = tid; i < L; i += REDUCE_THREADS) {           // thread tid: columns tid, tid + 256, ... in order
        const int hv = hp[i];
        if (hv >= 0) { s += (double)lp[i]; ++c; }
        if (hv == 1) ++h;
    }
    s_sum[tid] = s; s_cnt[tid] = c; s_hit[tid] = h;
    __syncthreads();
    for (int o = REDUCE_THREADS / 2; o > 0; o >>= 1) {        // a fixed tree: the same bits on every call
        if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; s_hit[tid] += s_hit[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { sum[b] = s_sum[0]; count[b] = s_cnt[0]; hits[b] = s_hit[0]; }
}
}  // namespace

extern "C" int mgx_token_logprob(const uint16_t* logits, int V, int ld, const int32_t* target, const int32_t* prev,
                                 const uint32_t* allow_table, float temperature, float* logp, float* lse_out, int32_t* hit, int rows,
                                 void* stream) {
    MGX_REQUIRE(logits && target && logp && hit, MGX_ERR_NULL, "mgx_token_logprob: NULL pointer");
    MGX_REQUIRE((allow_table == nullptr) == (prev == nullptr), MGX_ERR_NULL,
                "mgx_token_logprob: allow_table and prev are given together or not at all");
    MGX_REQUIRE(rows > 0 && V >= 1 && ld >= V && temperature > 0.f, MGX_ERR_SHAPE,
                "mgx_token_logprob: need rows>0, V>=1, ld>=V, temperature>0 (rows=%d V=%d ld=%d temperature=%g)", rows, V, ld,
                (double)temperature);
    hipLaunchKernelGGL(token_logprob_kernel, dim3((rows + SCORE_WAVES - 1) / SCORE_WAVES), dim3(64 * SCORE_WAVES), 0,
                       (hipStream_t)stream, logits, V, ld, target, prev, allow_table, 1.f / temperature, logp, lse_out, hit, rows);
    MGX_CHECK_LAUNCH("mgx_token_logprob");
    return MGX_OK;
}

extern "C" int mgx_linear_logprob(const uint16_t* A, const uint16_t* W, const float* bias, const int32_t* target, float temperature,
                                  float* logp, float* lse_out, int32_t* hit, int M, int V, int K, void* stream) {
    MGX_REQUIRE(A && W && target && logp && hit, MGX_ERR_NULL, "mgx_linear_logprob: NULL pointer");
    MGX_REQUIRE(M > 0 && V >= 1 && K >= 64 && K <= LL_KMAX && K % 64 == 0 && temperature > 0.f, MGX_ERR_SHAPE,
                "mgx_linear_logprob: need M>0, V>=1, K%%64==0, 64<=K<=%d, temperature>0 (M=%d V=%d K=%d temperature=%g)", LL_KMAX, M, V,
                K, (double)temperature);
    const size_t lds = (size_t)LL_ROWS * K * 2;               // >= 4 KB: holds the waves' 3 KB of partial states afterwards
    hipLaunchKernelGGL(linear_logprob_kernel, dim3((M + LL_ROWS - 1) / LL_ROWS), dim3(64 * SCORE_WAVES), lds, (hipStream_t)stream, A, W,
                       bias, target, 1.f / temperature, logp, lse_out, hit, M, V, K);
    MGX_CHECK_LAUNCH("mgx_linear_logprob");
    return MGX_OK;
}

extern "C" int mgx_score_reduce(const float* logp, const int32_t* hit, double* sum, int32_t* count, int32_t* hits, int B, int L,
                                void* stream) {
    MGX_REQUIRE(logp && hit && sum && count && hits, MGX_ERR_NULL, "mgx_score_reduce: NULL pointer");
    MGX_REQUIRE(B > 0 && L > 0, MGX_ERR_SHAPE, "mgx_score_reduce: need B>0, L>0 (B=%d L=%d)", B, L);
    hipLaunchKernelGGL(score_reduce_kernel, dim3(B), dim3(REDUCE_THREADS), 0, (hipStream_t)stream, logp, hit, sum, count, hits, L);
    MGX_CHECK_LAUNCH("mgx_score_reduce");
    return MGX_OK;
}

// Repetition control on the KV-cache decode (ABI 31; contract in include/mgx.h): one stateless call before the sampler, in place
// on the step's logits.  The row's history is what the decode has on the device already -- out_tokens[b, 0 .. c], the prompt and
// every token the sampler wrote, in absolute columns -- so there is no per-row state, nothing to stage and nothing to gather.
//
//   mgx_repeat_penalty   counts the ids of the last `window` columns and subtracts pen[count] from the counted ids that `subject`
//                        names (presence / frequency penalty), and subtracts `ban` from every id that would complete an n-gram
//                        the row holds already (no-repeat-n-gram).  Both amounts are FINITE: the call never changes which logits
//                        of a row are finite, so the budget, note and grammar guarantees hold as they do without it.
//
// One workgroup per row.  LDS: one count per id and a bitmap of the banned ids; LDS atomics only.  Three passes with a barrier
// between the second and the third: the window's columns into the counts, the candidate n-gram ends into the bitmap (compared
// backwards from the newest token, so a mismatch -- the common case -- costs one load), then the ids with an amount.
#include "mgx_common.hpp"

#include <cmath>

namespace {
constexpr int REPEAT_THREADS = 256;
constexpr int REPEAT_MAX_V = 1024;

__global__ __launch_bounds__(REPEAT_THREADS) void repeat_penalty_kernel(uint16_t* __restrict__ logits, int V, int ld,
                                                                        const int32_t* __restrict__ out_tokens, int out_ld,
                                                                        StepPos stp, const int32_t* __restrict__ subject,
                                                                        const float* __restrict__ pen, int window, int ngram,
                                                                        int span, float ban) {
    __shared__ uint32_t cnt[REPEAT_MAX_V];
    __shared__ uint32_t banned[REPEAT_MAX_V / 32];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int c = stp.step(b);                            // the column of the row's last token: uniform over the workgroup
    if (c < 0 || c >= out_ld) return;
    const int32_t* row = out_tokens + (size_t)b * out_ld;
    if (window > 0)
        for (int v = tid; v < V; v += REPEAT_THREADS) cnt[v] = 0;
    if (tid < REPEAT_MAX_V / 32) banned[tid] = 0;
    __syncthreads();
    if (window > 0) {                                     // columns max(0, c - window + 1) .. c, all inside 0 .. out_ld - 1
        for (int j = max(0, c - window + 1) + tid; j <= c; j += REPEAT_THREADS) {
            const int32_t t = row[j];
            if ((uint32_t)t < (uint32_t)V) atomicAdd(&cnt[t], 1u);
        }
    }
    if (ngram >= 2) {
        const int k = ngram - 1;                          // the context is columns c - k + 1 .. c
        const int lo = span ? max(0, c - span + 1) : 0;
        if (c - k + 1 >= lo) {
            for (int e = lo + k - 1 + tid; e <= c - 1; e += REPEAT_THREADS) {      // e - k + 1 >= lo >= 0 and e + 1 <= c
                int i = 0;
                while (i < k && row[e - i] == row[c - i]) ++i;
                if (i == k) {
                    const int32_t f = row[e + 1];
                    if ((uint32_t)f < (uint32_t)V) atomicOr(&banned[f >> 5], 1u << (f & 31));
                }
            }
        }
    }
    __syncthreads();
    uint16_t* lp = logits + (size_t)b * ld;
    for (int v = tid; v < V; v += REPEAT_THREADS) {
        float a;
        if ((banned[v >> 5] >> (v & 31)) & 1u) {
            a = ban;
        } else {
            if (window <= 0) continue;
            const uint32_t n = cnt[v];                    // <= window: inside pen
            if (n == 0 || subject[v] == 0) continue;
            a = pen[n];
        }
        lp[v] = f32_to_bf16(__fsub_rn(bf16_to_f32(lp[v]), a));       // one f32 subtraction, one rounding: nothing to contract with
    }
}
}  // namespace

extern "C" int mgx_repeat_penalty(uint16_t* logits, int V, int ld, const int32_t* out_tokens, int out_ld, const int32_t* pos_dev,
                                  const int32_t* base_dev, int per_row, const int32_t* subject, const float* pen, int window,
                                  int ngram, int span, float ban, int B, void* stream) {
    MGX_REQUIRE(logits && out_tokens && pos_dev, MGX_ERR_NULL, "mgx_repeat_penalty: NULL pointer");
    MGX_REQUIRE(window <= 0 || (subject && pen), MGX_ERR_NULL, "mgx_repeat_penalty: window > 0 needs subject and pen");
    MGX_REQUIRE(B > 0 && V > 0 && V <= REPEAT_MAX_V && ld >= V && out_ld > 0, MGX_ERR_SHAPE,
                "mgx_repeat_penalty: need B>0, 0<V<=%d, ld>=V, out_ld>0 (B=%d V=%d ld=%d out_ld=%d)", REPEAT_MAX_V, B, V, ld, out_ld);
    MGX_REQUIRE(window >= 0 && window <= MGX_REPEAT_MAX_WINDOW, MGX_ERR_SHAPE, "mgx_repeat_penalty: window must lie in 0 .. %d, got %d",
                MGX_REPEAT_MAX_WINDOW, window);
    MGX_REQUIRE(ngram == 0 || (ngram >= 2 && ngram <= MGX_REPEAT_MAX_NGRAM), MGX_ERR_SHAPE,
                "mgx_repeat_penalty: ngram must be 0 or lie in 2 .. %d, got %d", MGX_REPEAT_MAX_NGRAM, ngram);
    MGX_REQUIRE(span == 0 || span >= ngram, MGX_ERR_SHAPE, "mgx_repeat_penalty: span must be 0 or >= ngram (span=%d ngram=%d)", span,
                ngram);
    MGX_REQUIRE(window != 0 || ngram != 0, MGX_ERR_SHAPE, "mgx_repeat_penalty: window == 0 and ngram == 0: nothing to do");
    MGX_REQUIRE(ngram == 0 || (std::isfinite(ban) && ban > 0.f), MGX_ERR_SHAPE,
                "mgx_repeat_penalty: ban must be finite and > 0 with ngram != 0, got %g", (double)ban);
    hipLaunchKernelGGL(repeat_penalty_kernel, dim3(B), dim3(REPEAT_THREADS), 0, (hipStream_t)stream, logits, V, ld, out_tokens, out_ld,
                       StepPos{pos_dev, base_dev, per_row}, subject, pen, window, ngram, span, ban);
    MGX_CHECK_LAUNCH("mgx_repeat_penalty");
    return MGX_OK;
}

// Length budgets on the KV-cache decode (ABI 27; contracts in include/mgx.h): every row carries a clock on the device -- what it
// may still spend (`remaining`), whether it has ended (`done`) and how many events it kept (`count`) -- in the units of a cost
// table over the vocabulary (centiseconds of time_shift, bars, ...).
//
//   mgx_budget_mask      before the sampler, in place on the step's logits: a live row's ids that cost more than the row has left
//                        become -inf, so no draw (top-k, top-p, grammar, or the grammar's fall-back) can overshoot the budget.
//                        One workgroup per row; the branch on done[b] is the same in every lane of the workgroup.
//   mgx_budget_account   after the sampler and its advance: charges the drawn token, ends the row that has spent its budget and
//                        writes pad_token over what an ended row goes on sampling.  One thread per row.
//
// The positions are never touched: an ended row keeps stepping on pad tokens with the others, so the shared counter, the ragged
// step and the re-anchored window need no new contract.  No atomics: the host reads `done` between runs of replays.
#include "logit_row.hpp"                                  // BF16_NEG_INF

namespace {
constexpr int MASK_THREADS = 256;

__global__ __launch_bounds__(MASK_THREADS) void budget_mask_kernel(uint16_t* __restrict__ logits, int V, int ld,
                                                                   const int32_t* __restrict__ cost,
                                                                   const int32_t* __restrict__ remaining,
                                                                   const int32_t* __restrict__ done) {
    const int b = blockIdx.x;
    if (done[b] != 0) return;                             // uniform over the workgroup
    const int32_t left = remaining[b];
    uint16_t* lp = logits + (size_t)b * ld;
    for (int v = threadIdx.x; v < V; v += MASK_THREADS)
        if (cost[v] > left) lp[v] = BF16_NEG_INF;
}

__global__ __launch_bounds__(256) void budget_account_kernel(int32_t* __restrict__ next_tok, int32_t* __restrict__ out_tokens,
                                                             int out_ld, StepPos stp, const int32_t* __restrict__ cost,
                                                             int32_t* __restrict__ remaining,
                                                             int32_t* __restrict__ done, int32_t* __restrict__ count,
                                                             int pad_token, int inclusive, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int col = stp.step(b);                          // the column the sampler has just written
    bool drop = true;                                     // an ended row: whatever it sampled is pad_token
    if (done[b] == 0) {
        const int tok = next_tok[b];
        const int32_t left = remaining[b] - (tok >= 0 ? cost[tok] : 0);
        remaining[b] = left;
        drop = false;
        if (left > 0) {
            count[b] += 1;
        } else {                                          // the budget is spent: the row ends with this token, or before it
            done[b] = 1;
            if (inclusive) count[b] += 1;
            else drop = true;
        }
    }
    if (drop) {
        next_tok[b] = pad_token;
        if (col >= 0 && col < out_ld) out_tokens[(size_t)b * out_ld + col] = pad_token;   // a column outside the row is not written
    }
}
}  // namespace

extern "C" int mgx_budget_mask(uint16_t* logits, int V, int ld, const int32_t* cost, const int32_t* remaining,
                               const int32_t* done, int B, void* stream) {
    MGX_REQUIRE(logits && cost && remaining && done, MGX_ERR_NULL, "mgx_budget_mask: NULL pointer");
    MGX_REQUIRE(B > 0 && V > 0 && ld >= V, MGX_ERR_SHAPE, "mgx_budget_mask: need B>0, V>0, ld>=V (B=%d V=%d ld=%d)", B, V, ld);
    hipLaunchKernelGGL(budget_mask_kernel, dim3(B), dim3(MASK_THREADS), 0, (hipStream_t)stream, logits, V, ld, cost, remaining, done);
    MGX_CHECK_LAUNCH("mgx_budget_mask");
    return MGX_OK;
}

extern "C" int mgx_budget_account(int32_t* next_tok, int32_t* out_tokens, int out_ld, const int32_t* pos_dev,
                                  const int32_t* base_dev, int per_row, const int32_t* cost, int32_t* remaining, int32_t* done,
                                  int32_t* count, int pad_token, int inclusive, int B, void* stream) {
    MGX_REQUIRE(next_tok && out_tokens && pos_dev && cost && remaining && done && count, MGX_ERR_NULL,
                "mgx_budget_account: NULL pointer");
    MGX_REQUIRE(B > 0 && out_ld > 0, MGX_ERR_SHAPE, "mgx_budget_account: need B>0, out_ld>0 (B=%d out_ld=%d)", B, out_ld);
    hipLaunchKernelGGL(budget_account_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, next_tok, out_tokens, out_ld,
                       StepPos{pos_dev, base_dev, per_row}, cost, remaining, done, count, pad_token, inclusive, B);
    MGX_CHECK_LAUNCH("mgx_budget_account");
    return MGX_OK;
}

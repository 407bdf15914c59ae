// Held-note state on the KV-cache decode (ABI 28; contracts in include/mgx.h): every row carries on the device the set of notes
// it holds -- MGX_NOTE_WORDS words of 32 bits, bit k in word k >> 5 at bit k & 31 -- under a rule table over the vocabulary:
// rule[v] = +(k + 1): id v sets bit k (a note_on), -(k + 1): it clears bit k (a note_off), 0: it touches none.
//
//   mgx_notes_mask      before the sampler, in place on the step's logits: a set-rule id becomes -inf where its bit is set already
//                       or the row holds max_on notes, a clear-rule id where its bit is clear.  One workgroup per row; the row's
//                       words and their popcount are loaded once, the same in every lane.
//   mgx_notes_account   after the sampler: applies the drawn token's rule to the row's words, with no validity check (the fold of
//                       the rules, right behind an unmasked sampler too).  One thread per row.
//
//   mgx_notes_keep      between the two sampler calls of a step and the accounts: a row whose FIRST draw -- made from the logits
//                       before mgx_notes_mask -- is legal keeps it, in next_tok and in the column the second draw was written to.
//                       So a row is the unconstrained row of the same seed until that one breaks a rule.  One thread per row.
//
// mask and account touch no position, no token and no column of the output matrix.  No atomics: one thread owns a row's words in account, mask reads.
#include "logit_row.hpp"                                  // BF16_NEG_INF

namespace {
constexpr int MASK_THREADS = 256;
constexpr int NOTE_BITS = 32 * MGX_NOTE_WORDS;
static_assert(MGX_NOTE_WORDS == 4, "the word select below is written for four words");

__global__ __launch_bounds__(MASK_THREADS) void notes_mask_kernel(uint16_t* __restrict__ logits, int V, int ld,
                                                                  const int32_t* __restrict__ rule,
                                                                  const int32_t* __restrict__ state, int max_on) {
    const int b = blockIdx.x;
    const int32_t* sp = state + (size_t)b * MGX_NOTE_WORDS;               // uniform over the workgroup
    const uint32_t w0 = (uint32_t)sp[0], w1 = (uint32_t)sp[1], w2 = (uint32_t)sp[2], w3 = (uint32_t)sp[3];
    const bool full = __popc(w0) + __popc(w1) + __popc(w2) + __popc(w3) >= max_on;
    uint16_t* lp = logits + (size_t)b * ld;
    for (int v = threadIdx.x; v < V; v += MASK_THREADS) {
        const int32_t r = rule[v];
        if (r == 0 || r > NOTE_BITS || r < -NOTE_BITS) continue;
        const int k = (r > 0 ? r : -r) - 1;
        const uint32_t word = k < 64 ? (k < 32 ? w0 : w1) : (k < 96 ? w2 : w3);      // selects, not an indexed register array
        const bool held = (word >> (k & 31)) & 1u;
        if (r > 0 ? (held || full) : !held) lp[v] = BF16_NEG_INF;
    }
}

__global__ __launch_bounds__(256) void notes_account_kernel(const int32_t* __restrict__ next_tok, const int32_t* __restrict__ rule,
                                                            int32_t* __restrict__ state, int V, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int tok = next_tok[b];
    if (tok < 0 || tok >= V) return;
    const int32_t r = rule[tok];
    if (r == 0 || r > NOTE_BITS || r < -NOTE_BITS) return;
    const int k = (r > 0 ? r : -r) - 1;
    int32_t* wp = state + (size_t)b * MGX_NOTE_WORDS + (k >> 5);          // k < NOTE_BITS: inside the row's words
    const uint32_t bit = 1u << (k & 31), w = (uint32_t)*wp;
    *wp = (int32_t)(r > 0 ? (w | bit) : (w & ~bit));
}

__global__ __launch_bounds__(256) void notes_keep_kernel(const int32_t* __restrict__ first_tok, int32_t* __restrict__ next_tok,
                                                         int32_t* __restrict__ out_tokens, int out_ld, StepPos stp,
                                                         const int32_t* __restrict__ rule, const int32_t* __restrict__ state,
                                                         int max_on, int V, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int tok = first_tok[b];
    if (tok < 0 || tok >= V) return;
    const int32_t r = rule[tok];
    if (r != 0 && r <= NOTE_BITS && r >= -NOTE_BITS) {                    // a rule id: legal under the row's state?
        const int32_t* sp = state + (size_t)b * MGX_NOTE_WORDS;
        const int k = (r > 0 ? r : -r) - 1;
        const bool held = ((uint32_t)sp[k >> 5] >> (k & 31)) & 1u;        // k < NOTE_BITS: inside the row's words
        if (r < 0 ? !held : held) return;
        if (r > 0 && __popc((uint32_t)sp[0]) + __popc((uint32_t)sp[1]) + __popc((uint32_t)sp[2]) + __popc((uint32_t)sp[3]) >= max_on)
            return;
    }
    next_tok[b] = tok;
    if (out_tokens) {
        const int col = stp.step(b);                                      // the column the sampler has just written
        if (col >= 0 && col < out_ld) out_tokens[(size_t)b * out_ld + col] = tok;
    }
}
}  // namespace

extern "C" int mgx_notes_mask(uint16_t* logits, int V, int ld, const int32_t* rule, const int32_t* state, int max_on, int B,
                              void* stream) {
    MGX_REQUIRE(logits && rule && state, MGX_ERR_NULL, "mgx_notes_mask: NULL pointer");
    MGX_REQUIRE(B > 0 && V > 0 && ld >= V, MGX_ERR_SHAPE, "mgx_notes_mask: need B>0, V>0, ld>=V (B=%d V=%d ld=%d)", B, V, ld);
    MGX_REQUIRE(max_on >= 1 && max_on <= NOTE_BITS, MGX_ERR_SHAPE, "mgx_notes_mask: need 1 <= max_on <= %d (max_on=%d)", NOTE_BITS,
                max_on);
    hipLaunchKernelGGL(notes_mask_kernel, dim3(B), dim3(MASK_THREADS), 0, (hipStream_t)stream, logits, V, ld, rule, state, max_on);
    MGX_CHECK_LAUNCH("mgx_notes_mask");
    return MGX_OK;
}

extern "C" int mgx_notes_account(const int32_t* next_tok, const int32_t* rule, int32_t* state, int V, int B, void* stream) {
    MGX_REQUIRE(next_tok && rule && state, MGX_ERR_NULL, "mgx_notes_account: NULL pointer");
    MGX_REQUIRE(B > 0 && V > 0, MGX_ERR_SHAPE, "mgx_notes_account: need B>0, V>0 (B=%d V=%d)", B, V);
    hipLaunchKernelGGL(notes_account_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, next_tok, rule, state, V, B);
    MGX_CHECK_LAUNCH("mgx_notes_account");
    return MGX_OK;
}

extern "C" int mgx_notes_keep(const int32_t* first_tok, int32_t* next_tok, int32_t* out_tokens, int out_ld, const int32_t* pos_dev,
                              const int32_t* base_dev, int per_row, const int32_t* rule, const int32_t* state, int max_on, int V,
                              int B, void* stream) {
    MGX_REQUIRE(first_tok && next_tok && pos_dev && rule && state, MGX_ERR_NULL, "mgx_notes_keep: NULL pointer");
    MGX_REQUIRE(B > 0 && V > 0 && (!out_tokens || out_ld > 0), MGX_ERR_SHAPE, "mgx_notes_keep: need B>0, V>0, out_ld>0 (B=%d V=%d out_ld=%d)",
                B, V, out_ld);
    MGX_REQUIRE(max_on >= 1 && max_on <= NOTE_BITS, MGX_ERR_SHAPE, "mgx_notes_keep: need 1 <= max_on <= %d (max_on=%d)", NOTE_BITS,
                max_on);
    hipLaunchKernelGGL(notes_keep_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, first_tok, next_tok, out_tokens,
                       out_ld, StepPos{pos_dev, base_dev, per_row}, rule, state, max_on, V, B);
    MGX_CHECK_LAUNCH("mgx_notes_keep");
    return MGX_OK;
}

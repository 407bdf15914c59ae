// Entropy-aware sampling on the KV-cache decode (ABI 34; contracts in include/mgx.h): min-p, locally typical sampling and Mirostat
// v2, the three cuts that follow the row's own uncertainty instead of falling at a fixed place.
//
//   mgx_entropy_mask      before the sampler, in place on the step's logits: a PURE MASK -- the ids the three stages drop become
//                         -inf and nothing else is written, so the unchanged sampler draws at the call's own temperature and its
//                         top-k / top-p act on what is left.  One wave per row in the sampler's layout (ids lane + 64 i, 16 per
//                         lane; load_row, logit_row.hpp).  The Mirostat cut and min-p are comparisons against the row's
//                         log-sum-exp and maximum; the typical set's radius is the sampler's exact bisection on float bit
//                         patterns, here on d = |surprise - entropy|, so ids of equal d -- ids of equal logits among them -- stay
//                         together by construction.  Also files the row's log-sum-exp for the account.
//   mgx_entropy_account   after the sampler and its advance, before mgx_budget_account: the surprise in bits of the token that was
//                         drawn, under the row's distribution BEFORE the mask (the kept logits are still there bit for bit), moves
//                         the row's Mirostat threshold mu and is filed in the trace.  One thread per row.
//
// Both are captured with the step: the grid is a function of B only, nothing is read on the host, no atomics, no LDS.
#include "decode_common.hpp"

#include <cmath>

namespace {
constexpr float LN2 = 0.6931471805599453f;

__global__ __launch_bounds__(64) void entropy_mask_kernel(uint16_t* __restrict__ logits, int V, int ld, float inv_t, float ln_min_p,
                                                          float typical_p, const float* __restrict__ mu,
                                                          float* __restrict__ lse_out, const int32_t* __restrict__ tok,
                                                          const uint32_t* __restrict__ allow_table) {
    const int b = blockIdx.x, lane = threadIdx.x;
    uint16_t* lp = logits + (size_t)b * ld;
    const uint32_t* arow = allow_table ? grammar_row(allow_table, tok[b], V) : nullptr;
    // bit i of a mask speaks of id lane + 64 i.  live: the id is in A (load_row, logit_row.hpp)
    float z[SMP_PER_LANE];
    const uint32_t live = load_row(lp, V, arow, lane, z, inv_t).live;       // logit * inv_t: the sampler's arithmetic
    if (!__ballot(live != 0)) {                           // nothing to draw from: the row stays bit for bit
        if (lse_out && lane == 0) lse_out[b] = 0.f;
        return;
    }
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i)
        if ((live >> i) & 1u) m = fmaxf(m, z[i]);
    m = wave_max(m);
    float e[SMP_PER_LANE];                                // e^(z - m) on A, 0 elsewhere
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) {
        e[i] = ((live >> i) & 1u) ? __expf(z[i] - m) : 0.f;
        sum += e[i];
    }
    sum = wave_sum(sum);
    const float ln_sum = logf(sum);
    if (lse_out && lane == 0) lse_out[b] = m + ln_sum;
    uint32_t keep = live;
    // 1. the Mirostat cut: surprise -log2 p = (ln sum - (z - m)) / ln 2 at most mu.  It keeps the likeliest ids, so the maximum
    //    of what is left is still m; where it leaves nothing, the ids at the maximum stand in
    if (mu) {
        const float cut = mu[b];
        uint32_t s1 = 0, top = 0;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) {
            if (!((keep >> i) & 1u)) continue;
            if ((ln_sum - (z[i] - m)) / LN2 <= cut) s1 |= 1u << i;
            if (z[i] == m) top |= 1u << i;
        }
        keep = __ballot(s1 != 0) ? s1 : top;
    }
    // 2. min-p: a ratio to the maximum, which is m at every stage
    if (ln_min_p > -INFINITY) {
        uint32_t s2 = 0;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i)
            if (((keep >> i) & 1u) && z[i] - m >= ln_min_p) s2 |= 1u << i;
        keep = s2;
    }
    // 3. typical: q = p renormalised over what is left, H its entropy, d = |-ln q - H|; the smallest radius delta whose ball
    //    {d <= delta} holds typical_p of the mass.  Non-negative floats order like their bit patterns -> exact bisection on the bits
    if (typical_p < 1.f) {
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) s2 += ((keep >> i) & 1u) ? e[i] : 0.f;
        s2 = wave_sum(s2);
        const float ln_s2 = logf(s2), inv = 1.f / s2;
        float q[SMP_PER_LANE], d[SMP_PER_LANE];
        float h = 0.f;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) {
            const bool in = (keep >> i) & 1u;
            const float lnq = (z[i] - m) - ln_s2;
            q[i] = in ? e[i] * inv : 0.f;
            d[i] = lnq;                                   // |ln q + H| below, once H is known
            h -= (in && q[i] > 0.f) ? q[i] * lnq : 0.f;
        }
        h = wave_sum(h);
        float mass_all = 0.f;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) {
            d[i] = ((keep >> i) & 1u) ? fabsf(d[i] + h) : INFINITY;
            mass_all += q[i];
        }
        mass_all = wave_sum(mass_all);
        const float need = typical_p * mass_all;
        int32_t lo = -1, hi = 0x7f800000;                 // mass{d <= hi} = mass_all >= need; nothing lies at or below "lo"
        while (hi - lo > 1) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            const float dv = __builtin_bit_cast(float, mid);
            float ms = 0.f;
#pragma unroll
            for (int i = 0; i < SMP_PER_LANE; ++i) ms += (d[i] <= dv) ? q[i] : 0.f;
            ms = wave_sum(ms);
            if (ms >= need) hi = mid; else lo = mid;
        }
        const float delta = __builtin_bit_cast(float, hi);
        uint32_t s3 = 0;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i)
            if (((keep >> i) & 1u) && d[i] <= delta) s3 |= 1u << i;
        keep = s3;
    }
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i)
        if (((live & ~keep) >> i) & 1u) lp[lane + 64 * i] = BF16_NEG_INF;
}

__global__ __launch_bounds__(256) void entropy_account_kernel(const int32_t* __restrict__ next_tok, const uint16_t* __restrict__ logits,
                                                              int V, int ld, float inv_t, const float* __restrict__ lse,
                                                              float* __restrict__ mu, float tau, float eta,
                                                              float* __restrict__ surprise_out, int out_ld, StepPos stp, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int t = next_tok[b];
    if (t < 0 || t >= V) return;
    const float x = bf16_to_f32(logits[(size_t)b * ld + t]);
    if (!(fabsf(x) < INFINITY)) return;                   // -inf, +inf or NaN: nothing to account
    const int col = stp.step(b);                          // the column the sampler has just written
    if (surprise_out && (col < 0 || col >= out_ld)) return;
    const float s = (lse[b] - x * inv_t) / LN2;
    // every operation rounded on its own, so the host's float32 recurrence over the filed surprises gives the same bits
    if (mu) mu[b] = __fsub_rn(mu[b], __fmul_rn(eta, __fsub_rn(s, tau)));
    if (surprise_out) surprise_out[(size_t)b * out_ld + col] = s;
}
}  // namespace

extern "C" int mgx_entropy_mask(uint16_t* logits, int V, int ld, float temperature, float min_p, float typical_p, const float* mu,
                                float* lse_out, const int32_t* tok, const uint32_t* allow_table, int B, void* stream) {
    MGX_REQUIRE(logits, MGX_ERR_NULL, "mgx_entropy_mask: NULL pointer");
    MGX_REQUIRE((tok == nullptr) == (allow_table == nullptr), MGX_ERR_NULL,
                "mgx_entropy_mask: tok and allow_table are given together or not at all");
    MGX_REQUIRE(B > 0 && V > 0 && V <= 64 * SMP_PER_LANE && ld >= V, MGX_ERR_SHAPE,
                "mgx_entropy_mask: need B>0, 0<V<=%d, ld>=V (B=%d V=%d ld=%d)", 64 * SMP_PER_LANE, B, V, ld);
    MGX_REQUIRE(std::isfinite(temperature) && temperature > 0.f, MGX_ERR_SHAPE,
                "mgx_entropy_mask: temperature must be finite and > 0, got %g", (double)temperature);
    MGX_REQUIRE(min_p >= 0.f && min_p < 1.f, MGX_ERR_SHAPE, "mgx_entropy_mask: min_p must lie in [0, 1), got %g", (double)min_p);
    MGX_REQUIRE(typical_p > 0.f && typical_p <= 1.f, MGX_ERR_SHAPE, "mgx_entropy_mask: typical_p must lie in (0, 1], got %g",
                (double)typical_p);
    const float ln_min_p = min_p > 0.f ? std::log(min_p) : -INFINITY;
    hipLaunchKernelGGL(entropy_mask_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, V, ld, 1.f / temperature, ln_min_p,
                       typical_p, mu, lse_out, tok, allow_table);
    MGX_CHECK_LAUNCH("mgx_entropy_mask");
    return MGX_OK;
}

extern "C" int mgx_entropy_account(const int32_t* next_tok, const uint16_t* logits, int V, int ld, float temperature, const float* lse,
                                   float* mu, float tau, float eta, float* surprise_out, int out_ld, const int32_t* pos_dev,
                                   const int32_t* base_dev, int per_row, int B, void* stream) {
    MGX_REQUIRE(next_tok && logits && lse && pos_dev, MGX_ERR_NULL, "mgx_entropy_account: NULL pointer");
    MGX_REQUIRE(B > 0 && V > 0 && ld >= V && (!surprise_out || out_ld > 0), MGX_ERR_SHAPE,
                "mgx_entropy_account: need B>0, V>0, ld>=V, out_ld>0 with surprise_out (B=%d V=%d ld=%d out_ld=%d)", B, V, ld, out_ld);
    MGX_REQUIRE(std::isfinite(temperature) && temperature > 0.f, MGX_ERR_SHAPE,
                "mgx_entropy_account: temperature must be finite and > 0, got %g", (double)temperature);
    MGX_REQUIRE(!mu || (std::isfinite(tau) && std::isfinite(eta)), MGX_ERR_SHAPE,
                "mgx_entropy_account: tau and eta must be finite, got %g and %g", (double)tau, (double)eta);
    hipLaunchKernelGGL(entropy_account_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, next_tok, logits, V, ld,
                       1.f / temperature, lse, mu, tau, eta, surprise_out, out_ld, StepPos{pos_dev, base_dev, per_row}, B);
    MGX_CHECK_LAUNCH("mgx_entropy_account");
    return MGX_OK;
}

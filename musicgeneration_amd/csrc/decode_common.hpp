// What the decode kernels of decode.hip and lookahead.hip share: the key ranges, the partial layout and the merge kernel of the
// split-key attention, and the sampler's draw as a device function (one wave per row).
#pragma once
#include "logit_row.hpp"                                // the sampler-layout row: constants, grammar row, masks, thresholds

namespace {
constexpr float LOG2E = 1.4426950408889634f;
}

constexpr int DEC_WAVES = 8;
constexpr int DEC_PART = 68;                                   // floats per partial: acc[64], m, l, 2 pad (16-byte aligned rows)
// What the bf16 and the 8-bit kernel share.  DPL = dims per lane (8: bf16, 16: 8-bit codes), so 64 / DPL lanes per key.
// this split's keys: [lo, hi), shares of ceil((t+1)/nsplit) keys rounded up to the workgroup's 64-key stride
MGX_DEV void dec_key_range(int t, int nsplit, int sp, int& lo, int& hi) {
    const int share = ((t + nsplit) / nsplit + 63) & ~63;
    lo = sp * share, hi = min(t + 1, lo + share);
}

// ctx[b, hd*64 + c] = sum_s acc_s[c] 2^(m_s - m) / sum_s l_s 2^(m_s - m): one wave per (b,h)
static __global__ __launch_bounds__(64) void rel_attn_decode_merge_kernel(const float* __restrict__ partial, uint16_t* __restrict__ ctx,
                                                                          int nsplit, int d) {
    const int heads = d >> 6;
    const int b = blockIdx.x / heads, hd = blockIdx.x % heads, c = threadIdx.x;
    const float* pp = partial + (size_t)blockIdx.x * nsplit * DEC_PART;
    float mm = -INFINITY;
    for (int s = 0; s < nsplit; ++s) mm = fmaxf(mm, pp[s * DEC_PART + 64]);
    float ll = 0.f, o = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const float ms = pp[s * DEC_PART + 64];
        const float a = (ms == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(ms - mm);
        ll += pp[s * DEC_PART + 65] * a;
        o += pp[s * DEC_PART + c] * a;
    }
    ctx[(size_t)b * d + hd * 64 + c] = f32_to_bf16(o / ll);
}

// ---------------------------------------------------------------------------------------------------
// sampling: one wave per row, V <= 64 * SMP_PER_LANE (logit_row.hpp); the uniform: u01 (mgx_common.hpp)
// ---------------------------------------------------------------------------------------------------
// The draw of mgx_sample_topk_topp for one row of logits, by one wave: temperature -> (grammar row `arow`, or nullptr) ->
// softmax -> top-k -> top-p -> inverse CDF at u * (kept mass).  Returns the token in every lane.  The unfiltered softmax goes to
// probs_row f32 [V] (or nullptr) and, with KEEP, into soft[i] for id lane + 64 i: a caller that learns only later whether the
// distribution is wanted.  Lane = threadIdx.x & 63.
template <bool KEEP>
MGX_DEV int sample_draw(const uint16_t* __restrict__ lp, int V, float inv_temp, int top_k, float top_p,
                        const uint32_t* __restrict__ arow, float u, int lane, float* __restrict__ probs_row,
                        float (&soft)[SMP_PER_LANE]) {
    float p[SMP_PER_LANE];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) {
        const int v = lane + 64 * i;
        p[i] = (v < V) ? bf16_to_f32(lp[v]) * inv_temp : -INFINITY;
        if (arow && v < V && !allowed(arow, v)) p[i] = -INFINITY;      // arow first: the wave-uniform test leaves the slots
        mx = fmaxf(mx, p[i]);
    }
    mx = wave_max(mx);
    if (arow && mx == -INFINITY) {                       // empty row: fall back to the unmasked distribution
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) {
            const int v = lane + 64 * i;
            p[i] = (v < V) ? bf16_to_f32(lp[v]) * inv_temp : -INFINITY;
            mx = fmaxf(mx, p[i]);
        }
        mx = wave_max(mx);
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) { p[i] = (lane + 64 * i < V) ? __expf(p[i] - mx) : 0.f; sum += p[i]; }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) p[i] *= inv;
    if (probs_row) {
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i)
            if (lane + 64 * i < V) probs_row[lane + 64 * i] = p[i];
    }
    if constexpr (KEEP) {
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) soft[i] = p[i];
    }
    // threshold tau: keep {p_i >= tau}, top-k then top-p over the ids v < V (logit_row.hpp)
    uint32_t tau_bits = 0;
    if (top_k > 0 && top_k < V) tau_bits = topk_threshold(p, [&](int i) { return lane + 64 * i < V; }, top_k);
    if (top_p < 1.f) tau_bits = topp_threshold(p, tau_bits, top_p);
    const float tau = __builtin_bit_cast(float, tau_bits);
    // categorical draw over the kept set by inverse CDF in index order
    float kept = 0.f;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) { if (!(p[i] >= tau)) p[i] = 0.f; kept += p[i]; }
    const float total = wave_sum(kept);
    const float target = u * total;
    int choice = -1;
    float base = 0.f;
    // index order: v = lane + 64*i  ->  iterate i outer (blocks of 64 consecutive ids), prefix over lanes inner
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) {
        float incl = p[i];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const float blk = __shfl(incl, 63, 64);
        const bool hit = (choice < 0) && (p[i] > 0.f) && (base + incl >= target);
        const unsigned long long mask = __ballot(hit);
        if (choice < 0 && mask) choice = 64 * i + (int)__builtin_ctzll(mask);
        base += blk;
    }
    if (choice < 0) {   // rounding at the top end: take the last kept id
#pragma unroll
        for (int i = SMP_PER_LANE - 1; i >= 0; --i) {
            const unsigned long long mask = __ballot(p[i] > 0.f);
            if (choice < 0 && mask) choice = 64 * i + 63 - (int)__builtin_clzll(mask);
        }
    }
    return choice;
}

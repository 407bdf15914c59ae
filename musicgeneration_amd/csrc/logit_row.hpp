// The logits row as the sampler sees it, defined once: every stage of the decode that shapes, masks or scores a row must treat it
// exactly as the sampler's draw does, or the sampler does not draw from the distribution the stage promised.  Here live the row's
// layout (one wave per row, id lane + 64 i in slot i of a lane), the grammar-row lookup and its bit test, the rule that a grammar
// row which leaves nothing is ignored (in its mask form), and the exact top-k / top-p threshold.  No helper holds a multiply-add
// chain, so floating-point contraction cannot make two callers differ.
#pragma once
#include "mgx_common.hpp"

constexpr uint16_t BF16_NEG_INF = 0xff80u;
constexpr int SMP_PER_LANE = 16;                         // ids per lane: V <= 64 * 16 = 1024

// the grammar row of the previous token `prev` (clamped to 0..V-1), or nullptr without a table
MGX_DEV const uint32_t* grammar_row(const uint32_t* __restrict__ allow_table, int prev, int V) {
    if (!allow_table) return nullptr;
    prev = prev < 0 ? 0 : (prev >= V ? V - 1 : prev);
    return allow_table + (size_t)prev * ((V + 31) >> 5);
}
// whether the grammar row lets id v (0 <= v < V) through; without a row everything passes
MGX_DEV bool allowed(const uint32_t* arow, int v) { return !arow || ((arow[v >> 5] >> (v & 31)) & 1u); }

// Bit i of a row mask speaks of id lane + 64 i.  fin: the value is above -inf; live: it is also in the grammar row -- or, where
// that row leaves nothing, live = fin: a grammar row that leaves nothing is ignored, as the sampler ignores it.
struct RowMasks {
    uint32_t fin, live;
};
// One wave loads a row in the sampler's layout: x[i] = logit * scale for id lane + 64 i (-inf at and past V), and the row's masks.
// scale = 1 leaves the logits as they are.
MGX_DEV RowMasks load_row(const uint16_t* __restrict__ lp, int V, const uint32_t* __restrict__ arow, int lane,
                          float (&x)[SMP_PER_LANE], float scale = 1.f) {
    RowMasks m{0, 0};
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) {
        const int v = lane + 64 * i;
        x[i] = -INFINITY;
        if (v < V) {
            x[i] = bf16_to_f32(lp[v]) * scale;
            if (x[i] > -INFINITY) {
                m.fin |= 1u << i;
                if (allowed(arow, v)) m.live |= 1u << i;
            }
        }
    }
    if (arow && !__ballot(m.live != 0)) m.live = m.fin;
    return m;
}

// The sampler's thresholds on a normalised row p: keep {p_i >= tau}.  Positive floats order like their bit patterns -> exact
// bisection on the bits, which are what is returned.  top-k: the largest tau with count(p >= tau) >= k over the members --
// member(i): is slot i of this lane one?  (A predicate, not a mask: where the caller zeroed p by the same test, the compiler sees
// that a non-member never counts.)  The caller asks only where 0 < k < the members' count.
template <class Member>
MGX_DEV uint32_t topk_threshold(const float (&p)[SMP_PER_LANE], Member member, int top_k) {
    uint32_t lo = 0, hi = 0x3f800001u;              // (p >= lo) holds for all; hi = just above 1.0
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const float tv = __builtin_bit_cast(float, mid);
        float c = 0.f;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) c += (p[i] >= tv && member(i)) ? 1.f : 0.f;
        c = wave_sum(c);
        if (c >= (float)top_k) lo = mid; else hi = mid;
    }
    return lo;
}
// top-p, after top-k's threshold `lo` (0: none): the largest tau with mass(p >= tau) >= top_p of the mass that `lo` left
MGX_DEV uint32_t topp_threshold(const float (&p)[SMP_PER_LANE], uint32_t lo, float top_p) {
    uint32_t hi = 0x3f800001u;
    float mass_all = 0.f;
    {
        const float tv = __builtin_bit_cast(float, lo);
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) mass_all += (p[i] >= tv) ? p[i] : 0.f;
        mass_all = wave_sum(mass_all);
    }
    const float need = top_p * mass_all;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const float tv = __builtin_bit_cast(float, mid);
        float ms = 0.f;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) ms += (p[i] >= tv) ? p[i] : 0.f;
        ms = wave_sum(ms);
        if (ms >= need) lo = mid; else hi = mid;
    }
    return lo;
}

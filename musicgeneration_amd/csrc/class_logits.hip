// Per-class temperature, top-k and top-p on the KV-cache decode (ABI 33; contract in include/mgx.h): one stateless call before the
// sampler, in place on the step's logits.  The row's distribution is taken apart into the classes' total probabilities, which stay
// the model's own at the call's temperature, and the distribution inside every class, which gets the class's own temperature and
// filters; what is written back is bf16(ln p') of the product, so the unchanged sampler at temperature 1 draws from p'.
//
//   mgx_class_logits   one workgroup per row, one wave per class.  Every wave loads the whole row in the sampler's layout (ids
//                      lane + 64 i, 16 per lane) BEFORE the workgroup's only barrier and writes the ids of its own class after it,
//                      so no wave reads what another has rewritten.  The row's log-sum-exp costs a wave 16 exponentials and two
//                      reductions, less than a round trip through LDS and a second barrier would, so every wave forms it itself
//                      -- from the same values in the same order, hence the same bits -- and nothing is exchanged.  A filtered
//                      class runs the sampler's bit-pattern bisections (logit_row.hpp) on its own wave: the
//                      classes' bisections run side by side, not one after the other.
#include "decode_common.hpp"

#include <cmath>

namespace {
__global__ __launch_bounds__(64 * MGX_CLASS_MAX) void class_logits_kernel(uint16_t* __restrict__ logits, int V, int ld,
                                                                          const int32_t* __restrict__ cls,
                                                                          const float* __restrict__ inv_temp,
                                                                          const int32_t* __restrict__ top_k,
                                                                          const float* __restrict__ top_p, float inv_t,
                                                                          const int32_t* __restrict__ tok,
                                                                          const uint32_t* __restrict__ allow_table) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, c = threadIdx.x >> 6;     // c: the wave, and the class it owns
    uint16_t* lp = logits + (size_t)b * ld;
    const uint32_t* arow = allow_table ? grammar_row(allow_table, tok[b], V) : nullptr;
    // bit i of a mask speaks of id lane + 64 i.  live: the id is in A (load_row, logit_row.hpp); mine: it belongs to class c
    float x[SMP_PER_LANE];
    const uint32_t live = load_row(lp, V, arow, lane, x).live;
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i)
        if (lane + 64 * i < V && cls[lane + 64 * i] == c) mine |= 1u << i;
    __syncthreads();                                      // every wave holds the row: from here on the waves write their classes
    if (!__ballot(live != 0)) return;                     // nothing to draw from: the row stays bit for bit (uniform over the waves)
    const uint32_t mem = live & mine;                     // A_c
    float m_all = -INFINITY, m_c = -INFINITY;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) {
        if ((live >> i) & 1u) m_all = fmaxf(m_all, x[i]);
        if ((mem >> i) & 1u) m_c = fmaxf(m_c, x[i]);
    }
    m_all = wave_max(m_all);
    m_c = wave_max(m_c);
    if (m_c == -INFINITY) {                               // A_c is empty: the class's ids, if it has any, are not to be drawn
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i)
            if ((mine >> i) & 1u) lp[lane + 64 * i] = BF16_NEG_INF;
        return;
    }
    // the class stage, at the call's temperature: ln P_c = lse_c - lse_all
    float s_all = 0.f, s_c = 0.f;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) {
        if ((live >> i) & 1u) s_all += __expf((x[i] - m_all) * inv_t);
        if ((mem >> i) & 1u) s_c += __expf((x[i] - m_c) * inv_t);
    }
    s_all = wave_sum(s_all);
    s_c = wave_sum(s_c);
    const float ln_pc = (m_c - m_all) * inv_t + (logf(s_c) - logf(s_all));
    // inside the class, at its own temperature: q = softmax over A_c
    const float it = inv_temp[c], tp = top_p[c];
    const int k = top_k[c];
    float q[SMP_PER_LANE];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i) {
        q[i] = ((mem >> i) & 1u) ? __expf((x[i] - m_c) * it) : 0.f;
        sum += q[i];
    }
    sum = wave_sum(sum);
    const float n_c = wave_sum((float)__popc(mem));       // |A_c| <= 1024: exact
    uint32_t keep = mem;
    float ln_kept = logf(sum);                            // ln of the kept ids' sum of e
    if ((k > 0 && (float)k < n_c) || tp < 1.f) {          // the sampler's thresholds, on q and over A_c
        const float inv = 1.f / sum;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i) q[i] *= inv;
        uint32_t tau_bits = 0;
        if (k > 0 && (float)k < n_c) tau_bits = topk_threshold(q, [&](int i) { return (mem >> i) & 1u; }, k);
        if (tp < 1.f) tau_bits = topp_threshold(q, tau_bits, tp);
        const float tau = __builtin_bit_cast(float, tau_bits);
        float kept = 0.f;
        keep = 0;
#pragma unroll
        for (int i = 0; i < SMP_PER_LANE; ++i)
            if (((mem >> i) & 1u) && q[i] >= tau) { keep |= 1u << i; kept += q[i]; }
        ln_kept += logf(wave_sum(kept));                  // q = e / sum: the kept e sum to sum * kept
    }
    // ln p' = ln P_c + (x - m_c) inv_temp[c] - ln sum_K e: formed in log space, so no kept id underflows to -inf
#pragma unroll
    for (int i = 0; i < SMP_PER_LANE; ++i)
        if ((mine >> i) & 1u)
            lp[lane + 64 * i] = ((keep >> i) & 1u) ? f32_to_bf16(ln_pc + ((x[i] - m_c) * it - ln_kept)) : BF16_NEG_INF;
}
}  // namespace

extern "C" int mgx_class_logits(uint16_t* logits, int V, int ld, const int32_t* cls, int C, const float* inv_temp,
                                const int32_t* top_k, const float* top_p, float temperature, const int32_t* tok,
                                const uint32_t* allow_table, int B, void* stream) {
    MGX_REQUIRE(logits && cls && inv_temp && top_k && top_p, MGX_ERR_NULL, "mgx_class_logits: NULL pointer");
    MGX_REQUIRE((tok == nullptr) == (allow_table == nullptr), MGX_ERR_NULL,
                "mgx_class_logits: tok and allow_table are given together or not at all");
    MGX_REQUIRE(B > 0 && V > 0 && V <= 64 * SMP_PER_LANE && ld >= V, MGX_ERR_SHAPE,
                "mgx_class_logits: need B>0, 0<V<=%d, ld>=V (B=%d V=%d ld=%d)", 64 * SMP_PER_LANE, B, V, ld);
    MGX_REQUIRE(C >= 1 && C <= MGX_CLASS_MAX, MGX_ERR_SHAPE, "mgx_class_logits: C must lie in 1 .. %d, got %d", MGX_CLASS_MAX, C);
    MGX_REQUIRE(std::isfinite(temperature) && temperature > 0.f, MGX_ERR_SHAPE,
                "mgx_class_logits: temperature must be finite and > 0, got %g", (double)temperature);
    hipLaunchKernelGGL(class_logits_kernel, dim3(B), dim3(64 * C), 0, (hipStream_t)stream, logits, V, ld, cls, inv_temp, top_k, top_p,
                       1.f / temperature, tok, allow_table);
    MGX_CHECK_LAUNCH("mgx_class_logits");
    return MGX_OK;
}

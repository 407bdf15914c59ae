// Draft-and-verify decode (ABI 32; contract in include/mgx.h): several tokens per step of the KV-cache decode, same sample.
// A step guesses the next T - 1 tokens of every row, runs the T positions t_b .. t_b + T - 1 of the row as B * T rows of the
// ordinary step (embedding, GEMMs, LayerNorms, vocabulary projection: row-wise, one position per row), draws every position with
// the draw the one-token call would make there -- the sampler's draw is a pure function of (seed, absolute step, row) -- and keeps
// the prefix whose guesses were right.
//
//   mgx_lookahead_draft        the guesses: a guide's columns, or the continuation of the latest earlier occurrence of the row's
//                              last n tokens in its own history (the scan of repeat.hip's n-gram rule), extended periodically.
//   mgx_rel_attn_decode_multi  the attention of the T consecutive queries of a row over that row's cache: every K and V row is
//                              loaded once for the T queries (rel_attn_decode_kernel's walk with T online-softmax states per lane).
//   mgx_lookahead_accept       the sampler's draw at every position, the accepted prefix, and the row's advance.
//
// No rollback: after a step every cache row below the new t_b was written from a verified input (position t_b + i enters the
// cache from draft[b, i], and i < n_b means draft[b, 0..i] were the sampled tokens).  The rows a rejected guess wrote lie at or
// above the new t_b, and the next step appends rows t_b .. t_b + T - 1 again -- and takes them from qkv_new, not from the cache --
// before any query can reach them: query i reads the cache below t_b only.
#include "decode_common.hpp"

namespace {
constexpr int DRAFT_THREADS = 256;

// One workgroup per row.  Every thread walks candidate ends j = s - 1 - tid, - 256, ... downwards and keeps, for every n, the first
// (greatest) j whose n columns ending at j equal the n ending at s, compared backwards from the newest token (a mismatch -- the
// common case -- costs one load); LDS atomicMax merges the threads.  The longest n with a match wins.
__global__ __launch_bounds__(DRAFT_THREADS) void lookahead_draft_kernel(const int32_t* __restrict__ tok,
                                                                        const int32_t* __restrict__ out_tokens, int out_ld,
                                                                        StepPos stp, const int32_t* __restrict__ guide, int guide_ld,
                                                                        int ngram, int pad_token, int32_t* __restrict__ draft,
                                                                        int32_t* __restrict__ pos_rows, int T, int Lmax) {
    __shared__ int best[MGX_LOOKAHEAD_MAX_NGRAM];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = stp.at(b), s = stp.step(b);              // s: the column of the step's input token (uniform over the workgroup)
    if (tid < T) pos_rows[b * T + tid] = max(0, min(t + tid, Lmax - 1));
    const int32_t* row = out_tokens + (size_t)b * out_ld;
    int32_t* dr = draft + (size_t)b * T;
    if (tid == 0) dr[0] = tok[b];
    if (guide) {
        const int32_t* g = guide + (size_t)b * guide_ld;
        if (tid >= 1 && tid < T) dr[tid] = (s >= 0 && s + tid < guide_ld) ? g[s + tid] : pad_token;
        return;
    }
    if (s < 1 || s >= out_ld) {                            // no history behind the token, or a row outside the contract: no guess
        if (tid >= 1 && tid < T) dr[tid] = pad_token;
        return;
    }
    if (tid < MGX_LOOKAHEAD_MAX_NGRAM) best[tid] = -1;
    __syncthreads();
    int lb[MGX_LOOKAHEAD_MAX_NGRAM];
#pragma unroll
    for (int n = 0; n < MGX_LOOKAHEAD_MAX_NGRAM; ++n) lb[n] = -1;
    for (int j = s - 1 - tid; j >= 0; j -= DRAFT_THREADS) {
        const int top = min(ngram, j + 1);                 // n columns ending at j: j - n + 1 >= 0
        int m = 0;
        while (m < top && row[j - m] == row[s - m]) ++m;
#pragma unroll
        for (int n = 0; n < MGX_LOOKAHEAD_MAX_NGRAM; ++n)
            if (m > n && lb[n] < 0) lb[n] = j;
        if (m >= ngram) break;                             // this thread's later candidates are smaller for every n
    }
#pragma unroll
    for (int n = 0; n < MGX_LOOKAHEAD_MAX_NGRAM; ++n)
        if (lb[n] >= 0) atomicMax(&best[n], lb[n]);
    __syncthreads();
    if (tid >= 1 && tid < T) {
        int j = -1;
        for (int n = ngram - 1; n >= 0 && j < 0; --n) j = best[n];
        int v = pad_token;
        if (j >= 0) {
            const int p = s - j;                           // the period: x~[c] = x~[c - p] for c > s
            v = row[s + tid - ((tid + p - 1) / p) * p];
        }
        dr[tid] = v;
    }
}

// rel_attn_decode_kernel (decode.hip) with T queries per workgroup: one workgroup (8 waves) per (batch row, head, key split),
// lane = (key slot, dim group), every (wave, key slot) an online-softmax stream -- T of them per lane, query i at position t + i.
// The keys are 0 .. min(t + T - 1, Lmax - 1): below t from the cache, from t on from qkv_new (row b * T + (j - t); split 0 appends
// those rows for the following steps in the same launch, so no workgroup depends on another one's store).  Query i sees j <= t + i;
// a masked (query, key) pair is an exact no-op of the stream (alpha = 1, p = 0).  Key j meets query i at E row M - 1 - (t + i - j):
// the 8 keys of an iteration touch 8 + T - 1 consecutive rows of E, which every (b, head) shares and the caches serve; K and V,
// the HBM stream, are loaded once for the T queries.  With one split the keys of query i sit in the (wave, slot) streams exactly
// where rel_attn_decode_kernel at position t + i has them.
template <int T>
__global__ __launch_bounds__(64 * DEC_WAVES) void rel_attn_decode_multi_kernel(
    const uint16_t* __restrict__ qkv_new, uint16_t* __restrict__ kcache, uint16_t* __restrict__ vcache,
    const uint16_t* __restrict__ E, const int32_t* __restrict__ pos_dev, uint16_t* __restrict__ ctx, float* __restrict__ partial,
    int Lmax, int d, int M) {
    const int heads = d >> 6;
    const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
    const int nsplit = gridDim.y, sp = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ks = lane >> 3, dg = lane & 7;
    int t = pos_dev[b];
    const bool ok = t >= 0 && t < Lmax;                        // a row outside the contract appends nothing and addresses
    if (!ok) t = 0;                                            // nothing from its position
    const int tmax = min(t + T - 1, Lmax - 1);                 // the last key any query of the row sees
    const uint16_t* qbase = qkv_new + (size_t)b * T * 3 * d + hd * 64;      // query i: + i * 3d
    uint16_t* kc = kcache + ((size_t)b * heads + hd) * Lmax * 64;
    uint16_t* vc = vcache + ((size_t)b * heads + hd) * Lmax * 64;
    if (sp == 0 && ok && tid < 16 * T) {                       // 16 threads per new row: 8 for K, 8 for V
        const int qi = tid >> 4, kv = (tid >> 3) & 1, c = (tid & 7) * 8;
        if (t + qi < Lmax)
            *(u32x4*)((kv ? vc : kc) + (size_t)(t + qi) * 64 + c) = *(const u32x4*)(qbase + (size_t)qi * 3 * d + (1 + kv) * d + c);
    }
    float q[T][8], m[T], l[T], acc[T][8];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        unpack8(*(const u32x4*)(qbase + (size_t)i * 3 * d + dg * 8), q[i]);
        m[i] = -INFINITY, l[i] = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { q[i][k] *= 0.125f * LOG2E; acc[i][k] = 0.f; }     // logits in log2 units
    }
    int lo, hi;
    dec_key_range(tmax, nsplit, sp, lo, hi);
    const int e0 = M - 1 - t;                                  // E row of (query i, key j): e0 + j - i, inside 0 .. M-1 for j <= t + i
    const int imax = tmax - t;                                 // a query beyond the cache (t + i >= Lmax) walks as the last one inside
    for (int j0 = lo + (w * 8); j0 < hi; j0 += DEC_WAVES * 8) {
        const int j = j0 + ks;
        const bool valid = j < hi;
        const int jc = valid ? j : hi - 1;
        const uint16_t* kp = (jc >= t) ? qbase + (size_t)(jc - t) * 3 * d + d : kc + (size_t)jc * 64;
        const uint16_t* vp = (jc >= t) ? qbase + (size_t)(jc - t) * 3 * d + 2 * d : vc + (size_t)jc * 64;
        // K / V are streamed once per step: nontemporal; E rows are shared by every (b, h): cached
        const u32x4 kw = __builtin_nontemporal_load((const u32x4*)(kp + dg * 8));
        const u32x4 vw = __builtin_nontemporal_load((const u32x4*)(vp + dg * 8));
        u32x4 ew[T];
#pragma unroll
        for (int i = 0; i < T; ++i) {                          // a masked pair's row is clamped into E and its score dropped
            const int er = min(max(e0 + jc - min(i, imax), 0), M - 1);
            ew[i] = *(const u32x4*)(E + (size_t)er * 64 + dg * 8);
        }
        float kf[8], vf[8];
        unpack8(kw, kf);
        unpack8(vw, vf);
#pragma unroll
        for (int i = 0; i < T; ++i) {
            float ef[8];
            unpack8(ew[i], ef);
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) s += q[i][k] * (kf[k] + ef[k]);
            s += dpp_mov<0xB1>(s);                             // the key's 8 lanes: xor-1, -2, -4 butterfly as DPP adds
            s += dpp_mov<0x4E>(s);
            s += dpp_mov<0x141>(s);
            if (!valid || jc > t + min(i, imax)) s = -INFINITY;        // causal: query i sees keys 0 .. t + i
            const float mn = fmaxf(m[i], s);
            const float alpha = (mn == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m[i] - mn);
            const float p = (mn == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(s - mn);
            l[i] = l[i] * alpha + p;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[i][k] = acc[i][k] * alpha + p * vf[k];
            m[i] = mn;
        }
    }
    // per query: the key slots of the wave, then the 8 waves through LDS (dec_finish<8> of decode.hip)
    __shared__ float sm[T][DEC_WAVES], sl[T][DEC_WAVES], sacc[T][DEC_WAVES][64];
#pragma unroll
    for (int i = 0; i < T; ++i) {
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) {
            const float mo = __shfl_xor(m[i], o, 64), lo2 = __shfl_xor(l[i], o, 64);
            const float mn = fmaxf(m[i], mo);
            const float a0 = (m[i] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m[i] - mn);
            const float a1 = (mo == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mo - mn);
            l[i] = l[i] * a0 + lo2 * a1;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[i][k] = acc[i][k] * a0 + __shfl_xor(acc[i][k], o, 64) * a1;
            m[i] = mn;
        }
        if (ks == 0) {
            if (dg == 0) { sm[i][w] = m[i]; sl[i][w] = l[i]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) sacc[i][w][dg * 8 + k] = acc[i][k];
        }
    }
    __syncthreads();
    for (int i = w; i < T; i += DEC_WAVES) {                   // wave w merges query w: one output per lane
        float mm = -INFINITY;
#pragma unroll
        for (int u = 0; u < DEC_WAVES; ++u) mm = fmaxf(mm, sm[i][u]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int u = 0; u < DEC_WAVES; ++u) {
            const float a = (sm[i][u] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(sm[i][u] - mm);
            ll += sl[i][u] * a;
            o += sacc[i][u][lane] * a;
        }
        const size_t rh = ((size_t)b * T + i) * heads + hd;
        if (nsplit == 1) {
            ctx[rh * 64 + lane] = f32_to_bf16(o / ll);
        } else {                                               // rel_attn_decode_merge_kernel's record of (row, head, split)
            float* pp = partial + (rh * nsplit + sp) * DEC_PART;
            if (lane == 0) { pp[64] = mm; pp[65] = ll; }
            pp[lane] = o;
        }
    }
}

// One workgroup per batch row, wave i draws position t + i: sample_kernel's draw (sample_draw) from logits row b * T + i with
// (seed, s + i, row0 + b) and the grammar row of draft[b, i].  Then every thread knows the T draws, the accepted prefix and n.
__global__ __launch_bounds__(64 * MGX_LOOKAHEAD_MAX_T) void lookahead_accept_kernel(
    const uint16_t* __restrict__ logits, int V, int ld, float inv_temp, int top_k, float top_p, uint64_t seed,
    int32_t* __restrict__ pos_dev, const int32_t* __restrict__ base_dev, const int32_t* __restrict__ draft,
    const int32_t* __restrict__ limit, int32_t* __restrict__ tok, int32_t* __restrict__ out_tokens, int out_ld,
    float* __restrict__ probs_all, int probs_ld, int32_t* __restrict__ done, int32_t* __restrict__ stats, int T, int row0,
    const uint32_t* __restrict__ allow_table) {
    __shared__ int ys[MGX_LOOKAHEAD_MAX_T];
    const int b = blockIdx.x, lane = threadIdx.x & 63, i = threadIdx.x >> 6;
    const int t = pos_dev[b], s = t + (base_dev ? base_dev[b] : 0);
    const int32_t* dr = draft + (size_t)b * T;
    float soft[SMP_PER_LANE];
    const int y = sample_draw<true>(logits + ((size_t)b * T + i) * ld, V, inv_temp, top_k, top_p, grammar_row(allow_table, dr[i], V),
                                    u01(seed, (uint32_t)(s + i), (uint32_t)(row0 + b)), lane, nullptr, soft);
    if (lane == 0) ys[i] = y;
    __syncthreads();                                           // every wave has read pos_dev[b] before wave 0 moves it
    int a = 0;
    while (a < T - 1 && dr[a + 1] == ys[a]) ++a;               // the guesses 1 .. a were the tokens drawn
    const int n = min(a + 1, limit[b] - s);
    if (n <= 0) {                                              // the row holds its last token: nothing written, the position stays
        if (threadIdx.x == 0) done[b] = 1;
        return;
    }
    if (i < n) {
        const int col = s + 1 + i;
        if (lane == 0 && col >= 0 && col < out_ld) out_tokens[(size_t)b * out_ld + col] = y;
        if (probs_all && s + i >= 0 && s + i < probs_ld) {
            float* pr = probs_all + ((size_t)b * probs_ld + (s + i)) * V;
#pragma unroll
            for (int k = 0; k < SMP_PER_LANE; ++k)
                if (lane + 64 * k < V) pr[lane + 64 * k] = soft[k];
        }
    }
    if (threadIdx.x == 0) {
        tok[b] = ys[n - 1];
        pos_dev[b] = t + n;
        if (stats) { stats[2 * b] += 1; stats[2 * b + 1] += n; }
    }
}
}  // namespace

extern "C" int mgx_lookahead_draft(const int32_t* tok, const int32_t* out_tokens, int out_ld, const int32_t* pos_dev,
                                   const int32_t* base_dev, const int32_t* guide, int guide_ld, int ngram, int pad_token,
                                   int32_t* draft, int32_t* pos_rows, int B, int T, int Lmax, void* stream) {
    const char* name = "mgx_lookahead_draft";
    MGX_REQUIRE(tok && out_tokens && pos_dev && draft && pos_rows, MGX_ERR_NULL, "%s: NULL pointer", name);
    MGX_REQUIRE(B > 0 && out_ld > 0 && Lmax > 0 && T >= 2 && T <= MGX_LOOKAHEAD_MAX_T && (long long)B * T <= 0x7fffffff, MGX_ERR_SHAPE,
                "%s: need B>0, out_ld>0, Lmax>0, 2<=T<=%d (B=%d out_ld=%d Lmax=%d T=%d)", name, MGX_LOOKAHEAD_MAX_T, B, out_ld, Lmax, T);
    MGX_REQUIRE(guide ? guide_ld > 0 : (ngram >= 1 && ngram <= MGX_LOOKAHEAD_MAX_NGRAM), MGX_ERR_SHAPE,
                "%s: need guide_ld>0 with a guide, else 1<=ngram<=%d (guide_ld=%d ngram=%d)", name, MGX_LOOKAHEAD_MAX_NGRAM, guide_ld,
                ngram);
    hipLaunchKernelGGL(lookahead_draft_kernel, dim3(B), dim3(DRAFT_THREADS), 0, (hipStream_t)stream, tok, out_tokens, out_ld,
                       StepPos{pos_dev, base_dev, 1}, guide, guide_ld, ngram, pad_token, draft, pos_rows, T, Lmax);
    MGX_CHECK_LAUNCH(name);
    return MGX_OK;
}

// the key splits are mgx_rel_attn_decode's: the workgroups per split are the same B * h
extern "C" int mgx_rel_attn_decode_multi_splits(int B, int T, int Lmax, int d) {
    return (T < 2 || T > MGX_LOOKAHEAD_MAX_T) ? 0 : mgx_rel_attn_decode_splits(B, Lmax, d);
}

extern "C" size_t mgx_rel_attn_decode_multi_workspace(int B, int T, int Lmax, int d) {
    const int s = mgx_rel_attn_decode_multi_splits(B, T, Lmax, d);
    return s <= 1 ? 0 : (size_t)B * T * (d / 64) * s * DEC_PART * sizeof(float);
}

extern "C" int mgx_rel_attn_decode_multi(const uint16_t* qkv_new, uint16_t* kcache, uint16_t* vcache, const uint16_t* E,
                                         const int32_t* pos_dev, uint16_t* ctx, void* workspace, size_t ws_bytes, int B, int T,
                                         int Lmax, int d, int M, void* stream) {
    const char* name = "mgx_rel_attn_decode_multi";
    MGX_REQUIRE(qkv_new && kcache && vcache && E && pos_dev && ctx, MGX_ERR_NULL, "%s: NULL pointer", name);
    MGX_REQUIRE(B > 0 && T >= 2 && T <= MGX_LOOKAHEAD_MAX_T && d > 0 && d % 64 == 0 && Lmax > 0 && M >= Lmax &&
                    (long long)B * T * (d / 64) <= 0x7fffffff,
                MGX_ERR_SHAPE, "%s: need 2<=T<=%d, d%%64==0 and M>=Lmax (B=%d T=%d Lmax=%d d=%d M=%d)", name, MGX_LOOKAHEAD_MAX_T, B, T,
                Lmax, d, M);
    const int ns = mgx_rel_attn_decode_multi_splits(B, T, Lmax, d);
    const size_t need = mgx_rel_attn_decode_multi_workspace(B, T, Lmax, d);
    MGX_REQUIRE(ns == 1 || (workspace && ws_bytes >= need), MGX_ERR_SHAPE,
                "%s: workspace must hold mgx_rel_attn_decode_multi_workspace() = %zu bytes (got %zu)", name, need, ws_bytes);
    const dim3 grid(B * (d / 64), ns), block(64 * DEC_WAVES);
    const hipStream_t st = (hipStream_t)stream;
#define MGX_MULTI_CASE(N)                                                                                                        \
    case N:                                                                                                                      \
        hipLaunchKernelGGL(rel_attn_decode_multi_kernel<N>, grid, block, 0, st, qkv_new, kcache, vcache, E, pos_dev, ctx,       \
                           (float*)workspace, Lmax, d, M);                                                                       \
        break;
    switch (T) {
        MGX_MULTI_CASE(2) MGX_MULTI_CASE(3) MGX_MULTI_CASE(4) MGX_MULTI_CASE(5) MGX_MULTI_CASE(6) MGX_MULTI_CASE(7) MGX_MULTI_CASE(8)
    }
#undef MGX_MULTI_CASE
    if (ns > 1)
        hipLaunchKernelGGL(rel_attn_decode_merge_kernel, dim3(B * T * (d / 64)), dim3(64), 0, st, (const float*)workspace, ctx, ns, d);
    MGX_CHECK_LAUNCH(name);
    return MGX_OK;
}

extern "C" int mgx_lookahead_accept(const uint16_t* logits, int V, int ld, float temperature, int top_k, float top_p, uint64_t seed,
                                    int32_t* pos_dev, const int32_t* base_dev, const int32_t* draft, const int32_t* limit,
                                    int32_t* tok, int32_t* out_tokens, int out_ld, float* probs_all, int probs_ld, int32_t* done,
                                    int32_t* stats, int B, int T, int row0, const uint32_t* allow_table, void* stream) {
    const char* name = "mgx_lookahead_accept";
    MGX_REQUIRE(logits && pos_dev && draft && limit && tok && out_tokens && done, MGX_ERR_NULL, "%s: NULL pointer", name);
    MGX_REQUIRE(B > 0 && T >= 2 && T <= MGX_LOOKAHEAD_MAX_T && V > 0 && V <= 64 * SMP_PER_LANE && ld >= V && temperature > 0.f &&
                    top_p > 0.f && row0 >= 0 && out_ld > 0 && (!probs_all || probs_ld > 0),
                MGX_ERR_SHAPE, "%s: need 2<=T<=%d, 0<V<=%d, ld>=V, temperature>0, top_p>0, row0>=0, out_ld>0 (T=%d V=%d ld=%d out_ld=%d)",
                name, MGX_LOOKAHEAD_MAX_T, 64 * SMP_PER_LANE, T, V, ld, out_ld);
    hipLaunchKernelGGL(lookahead_accept_kernel, dim3(B), dim3(64 * T), 0, (hipStream_t)stream, logits, V, ld, 1.f / temperature, top_k,
                       top_p, seed, pos_dev, base_dev, draft, limit, tok, out_tokens, out_ld, probs_all, probs_ld, done, stats, T, row0,
                       allow_table);
    MGX_CHECK_LAUNCH(name);
    return MGX_OK;
}

// Beam search on the KV-cache decode (ABI 22; contracts in include/mgx.h).
//
//   mgx_beam_select      the step's last kernel in place of the sampler: the K best of the K*V expansions of a prompt's K beams,
//                        one workgroup per prompt.  Every wave turns whole beams (one logits row each, as the sampler does) into
//                        candidates and keeps the beam's own K best -- a beam cannot contribute more -- so only K*K (<= 256)
//                        candidates reach LDS, where wave 0 merges them.  Selection is K rounds of a maximum over (key, -index) packed in
//                        64 bits, so equal keys are ordered by the smaller flat index k*V + v exactly as the contract says.
//   mgx_kv_beam_reorder  hands slot r the cache rows of its parent: one contiguous run per (r, head), 16-byte vectors.
//   mgx_beam_backtrack   walks the parent table back from every final beam, one thread per row.
//
// Nothing is read back: the positions, parents and scores live on the device, so select and reorder are captured with the step.
#include "logit_row.hpp"                                  // the sampler-layout row: ids per lane, grammar row, bit test

namespace {
constexpr int BEAM_MAX = 16;              // beams per prompt
constexpr int BEAM_WAVES = 4;
constexpr int NO_INDEX = 0x7fffffff;

// A candidate as ONE unsigned 64-bit number whose order is the contract's: the key (its bits mapped so that unsigned order is
// float order) above, the complement of the index below -- the larger key wins, the smaller index among equal keys.  0: none.
MGX_DEV unsigned long long pack_cand(float key, int idx) {
    const uint32_t b = __builtin_bit_cast(uint32_t, key);
    const uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)ord << 32) | (uint32_t)(NO_INDEX - idx);
}
MGX_DEV int cand_index(unsigned long long c) { return NO_INDEX - (int)(uint32_t)c; }
MGX_DEV unsigned long long wave_max_u64(unsigned long long c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(c >> 32), o, 64), lo = __shfl_xor((uint32_t)c, o, 64);
        const unsigned long long c2 = ((unsigned long long)hi << 32) | lo;
        c = c2 > c ? c2 : c;
    }
    return c;
}

__global__ __launch_bounds__(64 * BEAM_WAVES) void beam_select_kernel(
    const uint16_t* __restrict__ logits, int V, int ld, float inv_temp, float* __restrict__ score, int32_t* __restrict__ tok,
    int32_t* __restrict__ parent, int32_t* __restrict__ pos_rows, int32_t* __restrict__ hist_tok, int32_t* __restrict__ hist_parent,
    int out_ld, int K, int advance, const uint32_t* __restrict__ allow_table, int stochastic, uint64_t seed) {
    // every product and sum rounded on its own, whatever the compiler makes of the unrolled loops: two ids of one beam with the
    // SAME logit must get the same key, or the tie rule (the smaller index) could not hold
#pragma clang fp contract(off)
    __shared__ float s_key[BEAM_MAX * BEAM_MAX];          // [beam][rank]: the beam's own K best, -inf where it has fewer
    __shared__ float s_cand[BEAM_MAX * BEAM_MAX];
    __shared__ int s_v[BEAM_MAX * BEAM_MAX];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row_first = b * K;
    const int t = pos_rows[row_first];                    // every beam of the prompt is at the same position

    for (int k = wave; k < K; k += BEAM_WAVES) {
        const int row = row_first + k;
        const float sc = score[row];
        const bool live = sc > -INFINITY;                 // false for a dead beam (and for NaN)
        float cand[SMP_PER_LANE], key[SMP_PER_LANE];
        if (live) {                                       // wave-uniform
            const uint16_t* lp = logits + (size_t)row * ld;
            const uint32_t* arow = allow_table ? grammar_row(allow_table, tok[row], V) : nullptr;
            // the logits as they are first; the maximum is taken off BEFORE the division by the temperature, so that the product
            // is rounded at the size of the differences (logits near -200 would lose five bits to it otherwise)
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < SMP_PER_LANE; ++i) {
                const int v = lane + 64 * i;
                cand[i] = (v < V) ? bf16_to_f32(lp[v]) : -INFINITY;
                if (arow && v < V && !allowed(arow, v)) cand[i] = -INFINITY;      // arow first, as in sample_draw
                mx = fmaxf(mx, cand[i]);
            }
            mx = wave_max(mx);
            if (arow && mx == -INFINITY) {                // a grammar row that leaves no finite logit is ignored
#pragma unroll
                for (int i = 0; i < SMP_PER_LANE; ++i) {
                    const int v = lane + 64 * i;
                    cand[i] = (v < V) ? bf16_to_f32(lp[v]) : -INFINITY;
                    mx = fmaxf(mx, cand[i]);
                }
                mx = wave_max(mx);
            }
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < SMP_PER_LANE; ++i) {
                cand[i] = (cand[i] - mx) * inv_temp;                                // <= 0; -inf for a disallowed id
                sum += expf(cand[i]);                                               // exp(-inf) = 0
            }
            const float lse = logf(wave_sum(sum));
#pragma unroll
            for (int i = 0; i < SMP_PER_LANE; ++i) {
                const int v = lane + 64 * i;
                cand[i] = sc + (cand[i] - lse);                                     // -inf for a disallowed id
                key[i] = cand[i];
                if (stochastic && cand[i] > -INFINITY) {
                    const float u = fminf(u01(seed, (uint32_t)t, (uint32_t)row * 1024u + (uint32_t)v), 1.f - 0x1p-24f);
                    key[i] = cand[i] - logf(-logf(u));
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < SMP_PER_LANE; ++i) cand[i] = key[i] = -INFINITY;
        }
        // the beam's own K best, in order; a key of -inf is never a candidate
        for (int j = 0; j < K; ++j) {
            unsigned long long best = 0;
#pragma unroll
            for (int i = 0; i < SMP_PER_LANE; ++i) {
                const unsigned long long c = key[i] > -INFINITY ? pack_cand(key[i], lane + 64 * i) : 0ull;
                best = c > best ? c : best;
            }
            best = wave_max_u64(best);
            const int bi = best ? cand_index(best) : NO_INDEX;
            float bk = -INFINITY, bc = -INFINITY;
#pragma unroll
            for (int i = 0; i < SMP_PER_LANE; ++i)
                if (lane + 64 * i == bi) { bk = key[i]; bc = cand[i]; key[i] = -INFINITY; }
            bk = wave_max(bk);                                                      // from the one lane that holds them
            bc = wave_max(bc);
            if (lane == 0) {
                s_key[k * BEAM_MAX + j] = bk;
                s_cand[k * BEAM_MAX + j] = bc;
                s_v[k * BEAM_MAX + j] = bi == NO_INDEX ? 0 : bi;
            }
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // merge: K*K <= 256 entries, four per lane; entry e = k * K + j has the flat index k * V + v
    float mkey[4], mcand[4];
    int midx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = lane + 64 * i;
        const bool in = e < K * K;
        const int s = in ? (e / K) * BEAM_MAX + e % K : 0;
        mkey[i] = in ? s_key[s] : -INFINITY;
        mcand[i] = in ? s_cand[s] : -INFINITY;
        midx[i] = in && mkey[i] > -INFINITY ? (e / K) * V + s_v[s] : NO_INDEX;
    }
    int my_tok = 0, my_parent = 0, tok0 = 0, parent0 = 0;
    float my_score = -INFINITY;
    for (int j = 0; j < K; ++j) {
        unsigned long long best = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned long long c = midx[i] != NO_INDEX ? pack_cand(mkey[i], midx[i]) : 0ull;
            best = c > best ? c : best;
        }
        best = wave_max_u64(best);
        const int bi = best ? cand_index(best) : NO_INDEX;
        float bc = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (midx[i] == bi && bi != NO_INDEX) { bc = mcand[i]; mkey[i] = -INFINITY; midx[i] = NO_INDEX; }
        bc = wave_max(bc);
        // fewer than K finite candidates: the slot copies slot 0 and stays dead; none at all: beam 0's token, parent 0
        const int jt = bi != NO_INDEX ? bi % V : (j == 0 ? tok[row_first] : tok0);
        const int jp = bi != NO_INDEX ? bi / V : (j == 0 ? 0 : parent0);
        if (j == 0) { tok0 = jt; parent0 = jp; }
        if (lane == j) { my_tok = jt; my_parent = jp; my_score = bi != NO_INDEX ? bc : -INFINITY; }
    }
    if (lane < K) {
        const int row = row_first + lane;
        score[row] = my_score;
        tok[row] = my_tok;
        parent[row] = my_parent;
        if (t >= -1 && t + 1 < out_ld) {                  // the contract; a position outside the tables is not written
            hist_tok[(size_t)row * out_ld + t + 1] = my_tok;
            hist_parent[(size_t)row * out_ld + t + 1] = my_parent;
        }
        if (advance) pos_rows[row] = t + 1;
    }
}

// one (r, head) run per blockIdx.x, REORDER_UNROLL * 256 units of it per blockIdx.y; UNIT: u32x4 (16 bytes) or uint32_t
constexpr int REORDER_UNROLL = 4;
template <typename UNIT>
__global__ __launch_bounds__(256) void kv_beam_reorder_kernel(UNIT* __restrict__ dst, const UNIT* __restrict__ src,
                                                              const int32_t* __restrict__ parent,
                                                              const int32_t* __restrict__ pos_rows, int K, int heads, int Lmax,
                                                              size_t run_units, int row_bytes) {
    const int r = blockIdx.x / heads, hd = blockIdx.x % heads;
    int n = pos_rows[r];
    n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
    const size_t units = (size_t)n * row_bytes / sizeof(UNIT);        // whole units of the run that hold rows < n
    const size_t first = (size_t)blockIdx.y * (REORDER_UNROLL * 256) + threadIdx.x;
    if ((size_t)blockIdx.y * (REORDER_UNROLL * 256) >= units) return;
    int p = parent[r];
    p = p < 0 ? 0 : (p >= K ? K - 1 : p);
    const UNIT* s = src + ((size_t)(r / K * K + p) * heads + hd) * run_units;
    UNIT* d = dst + ((size_t)r * heads + hd) * run_units;
    UNIT v[REORDER_UNROLL];
#pragma unroll
    for (int u = 0; u < REORDER_UNROLL; ++u)
        if (first + u * 256 < units) v[u] = s[first + u * 256];
#pragma unroll
    for (int u = 0; u < REORDER_UNROLL; ++u)
        if (first + u * 256 < units) d[first + u * 256] = v[u];
}
// the 4-byte rows left over by the 16-byte units of a run (n % 4 of them), one thread per (r, head)
__global__ __launch_bounds__(256) void kv_beam_reorder_tail_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
                                                                   const int32_t* __restrict__ parent,
                                                                   const int32_t* __restrict__ pos_rows, int K, int heads,
                                                                   int Lmax, int runs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= runs) return;
    const int r = i / heads, hd = i % heads;
    int n = pos_rows[r];
    n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
    int p = parent[r];
    p = p < 0 ? 0 : (p >= K ? K - 1 : p);
    const uint32_t* s = src + ((size_t)(r / K * K + p) * heads + hd) * Lmax;
    uint32_t* d = dst + (size_t)i * Lmax;
    for (int j = n & ~3; j < n; ++j) d[j] = s[j];
}

__global__ __launch_bounds__(256) void beam_backtrack_kernel(const int32_t* __restrict__ hist_tok,
                                                             const int32_t* __restrict__ hist_parent,
                                                             const int32_t* __restrict__ c0_rows, int32_t* __restrict__ out,
                                                             int out_ld, int R, int K, int steps) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int first = r / K * K, c0 = c0_rows[r];
    if (c0 < 0 || c0 > out_ld - steps) return;            // outside the tables: nothing to walk
    int cur = r - first;
    for (int s = steps - 1; s >= 0; --s) {
        const size_t at = (size_t)(first + cur) * out_ld + c0 + s;
        out[(size_t)r * out_ld + c0 + s] = hist_tok[at];
        const int p = hist_parent[at];
        cur = p < 0 ? 0 : (p >= K ? K - 1 : p);
    }
}
}  // namespace

extern "C" int mgx_beam_select(const uint16_t* logits, int V, int ld, float temperature, float* score, int32_t* tok,
                               int32_t* parent, int32_t* pos_rows, int32_t* hist_tok, int32_t* hist_parent, int out_ld, int B,
                               int K, int advance, const uint32_t* allow_table, int stochastic, uint64_t seed, void* stream) {
    MGX_REQUIRE(logits && score && tok && parent && pos_rows && hist_tok && hist_parent, MGX_ERR_NULL, "mgx_beam_select: NULL pointer");
    MGX_REQUIRE(B > 0 && V > 0 && V <= 64 * SMP_PER_LANE && ld >= V && temperature > 0.f && K >= 1 && K <= BEAM_MAX && K <= V &&
                    out_ld > 0 && (size_t)B * K <= 0x7fffffff / 1024,
                MGX_ERR_SHAPE, "mgx_beam_select: need 0<V<=%d, ld>=V, temperature>0, 1<=K<=min(%d,V), out_ld>0, B*K<2^21 (V=%d ld=%d K=%d B=%d)",
                64 * SMP_PER_LANE, BEAM_MAX, V, ld, K, B);
    hipLaunchKernelGGL(beam_select_kernel, dim3(B), dim3(64 * BEAM_WAVES), 0, (hipStream_t)stream, logits, V, ld, 1.f / temperature,
                       score, tok, parent, pos_rows, hist_tok, hist_parent, out_ld, K, advance, allow_table, stochastic, seed);
    MGX_CHECK_LAUNCH("mgx_beam_select");
    return MGX_OK;
}

extern "C" int mgx_kv_beam_reorder(void* dst, const void* src, const int32_t* parent, const int32_t* pos_rows, int R, int K,
                                   int heads, int Lmax, int row_bytes, void* stream) {
    MGX_REQUIRE(dst && src && parent && pos_rows, MGX_ERR_NULL, "mgx_kv_beam_reorder: NULL pointer");
    MGX_REQUIRE(dst != src, MGX_ERR_SHAPE, "mgx_kv_beam_reorder: src and dst must be different buffers");
    MGX_REQUIRE(R > 0 && K >= 1 && R % K == 0 && heads > 0 && Lmax > 0 && (row_bytes == 128 || row_bytes == 64 || row_bytes == 4) &&
                    (size_t)R * heads <= 0x7fffffff && (((uintptr_t)dst | (uintptr_t)src) & 15) == 0,
                MGX_ERR_SHAPE, "mgx_kv_beam_reorder: need R>0 a multiple of K>=1, heads>0, Lmax>0, row_bytes 128, 64 or 4, 16-byte "
                "aligned buffers (R=%d K=%d heads=%d Lmax=%d row_bytes=%d)", R, K, heads, Lmax, row_bytes);
    const int runs = R * heads;
    const size_t run_bytes = (size_t)Lmax * row_bytes;
    const unsigned per_block = REORDER_UNROLL * 256;
    if (run_bytes % 16 == 0) {            // every run starts on a 16-byte boundary
        const size_t run_units = run_bytes / 16;
        MGX_REQUIRE((run_units + per_block - 1) / per_block <= 65535, MGX_ERR_SHAPE, "mgx_kv_beam_reorder: Lmax=%d too long", Lmax);
        hipLaunchKernelGGL(kv_beam_reorder_kernel<u32x4>, dim3(runs, (unsigned)((run_units + per_block - 1) / per_block)), dim3(256), 0,
                           (hipStream_t)stream, (u32x4*)dst, (const u32x4*)src, parent, pos_rows, K, heads, Lmax, run_units, row_bytes);
        if (row_bytes == 4)
            hipLaunchKernelGGL(kv_beam_reorder_tail_kernel, dim3((runs + 255) / 256), dim3(256), 0, (hipStream_t)stream, (uint32_t*)dst,
                               (const uint32_t*)src, parent, pos_rows, K, heads, Lmax, runs);
    } else {                              // 4-byte rows, Lmax no multiple of 4: the runs are only 4-byte aligned
        hipLaunchKernelGGL(kv_beam_reorder_kernel<uint32_t>, dim3(runs, (unsigned)((Lmax + per_block - 1) / per_block)), dim3(256), 0,
                           (hipStream_t)stream, (uint32_t*)dst, (const uint32_t*)src, parent, pos_rows, K, heads, Lmax, (size_t)Lmax,
                           row_bytes);
    }
    MGX_CHECK_LAUNCH("mgx_kv_beam_reorder");
    return MGX_OK;
}

extern "C" int mgx_beam_backtrack(const int32_t* hist_tok, const int32_t* hist_parent, const int32_t* c0_rows, int32_t* out,
                                  int out_ld, int R, int K, int steps, void* stream) {
    MGX_REQUIRE(hist_tok && hist_parent && c0_rows && out, MGX_ERR_NULL, "mgx_beam_backtrack: NULL pointer");
    MGX_REQUIRE(R > 0 && K >= 1 && R % K == 0 && steps >= 1 && steps <= out_ld, MGX_ERR_SHAPE,
                "mgx_beam_backtrack: need R>0 a multiple of K>=1, 1<=steps<=out_ld (R=%d K=%d steps=%d out_ld=%d)", R, K, steps, out_ld);
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, hist_tok, hist_parent, c0_rows,
                       out, out_ld, R, K, steps);
    MGX_CHECK_LAUNCH("mgx_beam_backtrack");
    return MGX_OK;
}

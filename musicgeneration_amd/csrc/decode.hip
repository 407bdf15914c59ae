// Autoregressive decode path (replaces the O(W^2)-per-token recompute of network.py:52-77).
//
// One generated token per step and sequence.  Everything the step needs is device resident -- the
// current position is read from a device counter -- so a whole step (all layers + sampling) can be
// captured once in a hipGraph and replayed per token.
//
//   mgx_decode_embed      h = emb[tok]*sqrt(d) + PE[pos]                       (layers.py:226-229)
//   mgx_rel_attn_decode   append k_t, v_t to the cache, then for the single query q_t:
//                         logit_j = (q.k_j + q.E[M-1-(t-j)])/8, j <= t; softmax; ctx = sum p_j v_j
//                         -- HBM-bound: streams K and V of the (b,h) once (2*(t+1)*128 B), E from L2.
//   mgx_sample_topk_topp  temperature -> softmax -> top-k -> top-p -> categorical draw, one wave per row;
//                         top_k = 0 and top_p = 1 reproduce the reference's full-softmax categorical
//                         (network.py:73-74).  Thresholds are exact (bisection on the float bit pattern).
//
// Every kernel that reads the position takes a StepPos (mgx_common.hpp; the header's "Step positions"): one counter shared by
// the rows, or one position per batch row, so that a batch can continue prompts of different lengths in lockstep.  Nothing else
// in a step depends on the position (the relative term E[M-1-(t-j)] only on the row's own t).
// Past max_seq the cache holds a window of the sequence: the position is the one inside the window, and a second counter of
// the same shape, the base, is the output column of window position 0.  Only the sampler reads it (embedding and attention
// get a StepPos without one); mgx_decode_reanchor moves both when the host re-anchors the window.
// mgx_rel_attn_decode_shared (ABI 26) is the per-row attention for N samples per prompt: the prompt's keys are held once per prompt
// and loaded once for several of its samples' queries (rel_attn_decode_shared_kernel, below the merge kernel).
#include "decode_common.hpp"                             // key ranges, partials, the merge kernel, the sampler's draw

__global__ __launch_bounds__(256) void decode_embed_kernel(const int32_t* __restrict__ tok, const float* __restrict__ table,
                                                           const float* __restrict__ pe, StepPos stp, uint16_t* __restrict__ out,
                                                           int B, int d, int V, float scale) {
    const int gpr = d >> 3;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B * gpr) return;
    const int r = g / gpr, c = (g % gpr) * 8;
    int t = tok[r];
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);
    const int pos = stp.at(r);
    const f32x4* tp = (const f32x4*)(table + (size_t)t * d + c);
    const f32x4* pp = (const f32x4*)(pe + (size_t)pos * d + c);
    const f32x4 a0 = tp[0], a1 = tp[1], p0 = pp[0], p1 = pp[1];
    float f[8] = {a0.x * scale + p0.x, a0.y * scale + p0.y, a0.z * scale + p0.z, a0.w * scale + p0.w,
                  a1.x * scale + p1.x, a1.y * scale + p1.y, a1.z * scale + p1.z, a1.w * scale + p1.w};
    *(u32x4*)(out + (size_t)r * d + c) = pack8(f);
}

// One workgroup (8 waves) per (batch, head, key split).  lane = (key slot ks = lane>>3, dim group dg = lane&7): a wave
// handles 8 keys per iteration, each lane 8 of the 64 dims (16-byte loads: a key row is one 128-byte line).
// Every (wave, key slot) runs its own online softmax stream; the 64 streams are merged at the end.
// Split-K: with one workgroup per (b,h) a batch-32, 8-head decode step has 256 workgroups = 8 waves per CU, and the
// bytes those waves keep in flight bound the cache stream at ~4.3 TB/s.  NSPLIT workgroups per (b,h) each take a
// contiguous, 64-key aligned share of the keys 0..t (balanced from the device-side position), write an unnormalised
// partial (m, l, acc[64]) and a tiny second kernel merges them by their maxima.  The new row t is taken from qkv_new by
// whichever split covers it (another workgroup appends it to the cache in the same launch).
// merge the key slots of the wave (lanes with equal dg), then the 8 waves through LDS; 64 threads write ctx (one split) or
// this split's unnormalised partial
template <int DPL>
MGX_DEV void dec_finish(float m, float l, float* acc, uint16_t* __restrict__ ctx, float* __restrict__ partial, int b, int hd, int d,
                        int nsplit, int sp, int tid, int w, int ks, int dg) {
#pragma unroll
    for (int o = 64 / DPL; o < 64; o <<= 1) {
        const float mo = __shfl_xor(m, o, 64), lo2 = __shfl_xor(l, o, 64);
        const float mn = fmaxf(m, mo);
        const float a0 = (m == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m - mn);
        const float a1 = (mo == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mo - mn);
        l = l * a0 + lo2 * a1;
#pragma unroll
        for (int k = 0; k < DPL; ++k) acc[k] = acc[k] * a0 + __shfl_xor(acc[k], o, 64) * a1;
        m = mn;
    }
    __shared__ float sm[DEC_WAVES], sl[DEC_WAVES], sacc[DEC_WAVES][64];
    if (ks == 0) {
        if (dg == 0) { sm[w] = m; sl[w] = l; }
#pragma unroll
        for (int k = 0; k < DPL; ++k) sacc[w][dg * DPL + k] = acc[k];
    }
    __syncthreads();
    if (tid < 64) {
        float mm = -INFINITY;
#pragma unroll
        for (int i = 0; i < DEC_WAVES; ++i) mm = fmaxf(mm, sm[i]);
        float ll = 0.f, o = 0.f;
#pragma unroll
        for (int i = 0; i < DEC_WAVES; ++i) {
            const float a = (sm[i] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(sm[i] - mm);
            ll += sl[i] * a;
            o += sacc[i][tid] * a;
        }
        if (nsplit == 1) {
            ctx[(size_t)b * d + hd * 64 + tid] = f32_to_bf16(o / ll);
        } else {                                                // an empty split leaves (m = -inf, l = 0, acc = 0)
            float* pp = partial + ((size_t)blockIdx.x * nsplit + sp) * DEC_PART;
            if (tid == 0) { pp[64] = mm; pp[65] = ll; }
            pp[tid] = o;
        }
    }
}

__global__ __launch_bounds__(64 * DEC_WAVES) void rel_attn_decode_kernel(
    const uint16_t* __restrict__ qkv_new, uint16_t* __restrict__ kcache, uint16_t* __restrict__ vcache,
    const uint16_t* __restrict__ E, StepPos stp, uint16_t* __restrict__ ctx, float* __restrict__ partial, int Lmax, int d, int M) {
    const int heads = d >> 6;
    const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
    const int nsplit = gridDim.y, sp = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ks = lane >> 3, dg = lane & 7;
    const int t = stp.at(b);                                    // current position; keys 0..t (per row: a short row may leave
                                                                // whole splits empty, which write m = -inf, l = 0)
    const uint16_t* qrow = qkv_new + (size_t)b * 3 * d + hd * 64;
    // caches are head-major [B, h, Lmax, 64]: a workgroup streams one contiguous run of 128-byte rows
    uint16_t* kc = kcache + ((size_t)b * heads + hd) * Lmax * 64;
    uint16_t* vc = vcache + ((size_t)b * heads + hd) * Lmax * 64;
    // append this step's key/value for the following steps (split 0 of each head owns the head's 64 columns); in THIS
    // step row t is read from qkv_new, so no workgroup depends on another one's store
    if (sp == 0) {
        if (tid < 8) *(u32x4*)(kc + (size_t)t * 64 + tid * 8) = *(const u32x4*)(qrow + d + tid * 8);
        else if (tid < 16) *(u32x4*)(vc + (size_t)t * 64 + (tid - 8) * 8) = *(const u32x4*)(qrow + 2 * d + (tid - 8) * 8);
    }
    float q[8];
    unpack8(*(const u32x4*)(qrow + dg * 8), q);
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] *= 0.125f * LOG2E;         // logits in log2 units
    int lo, hi;
    dec_key_range(t, nsplit, sp, lo, hi);

    float m = -INFINITY, l = 0.f, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint16_t* Eb = E + (size_t)(M - 1 - t) * 64;           // E row of key j is Eb + j*64
    for (int j0 = lo + (w * 8); j0 < hi; j0 += DEC_WAVES * 8) {
        const int j = j0 + ks;
        const bool valid = j < hi;
        const int jc = valid ? j : hi - 1;
        const uint16_t* kp = (jc == t) ? qrow + d : kc + (size_t)jc * 64;
        const uint16_t* vp = (jc == t) ? qrow + 2 * d : vc + (size_t)jc * 64;
        float kf[8], ef[8], vf[8];
        // the K / V caches are streamed once per token (3.2 GB per step at cfg5's end): nontemporal; E rows are shared by every (b, h): cached
        unpack8(__builtin_nontemporal_load((const u32x4*)(kp + dg * 8)), kf);
        unpack8(*(const u32x4*)(Eb + (size_t)jc * 64 + dg * 8), ef);
        unpack8(__builtin_nontemporal_load((const u32x4*)(vp + dg * 8)), vf);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += q[k] * (kf[k] + ef[k]);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (!valid) s = -INFINITY;
        const float mn = fmaxf(m, s);
        const float alpha = (mn == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m - mn);
        const float p = (mn == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(s - mn);
        l = l * alpha + p;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = acc[k] * alpha + p * vf[k];
        m = mn;
    }
    dec_finish<8>(m, l, acc, ctx, partial, b, hd, d, nsplit, sp, tid, w, ks, dg);
}

// ---------------------------------------------------------------------------------------------------
// Shared prompt cache (ABI 26): R = Bp * N rows, row r = b * N + n is sample n of prompt b.  The N rows of a prompt sit at one
// position t and share the first p keys (kpre / vpre [Bp, h, Lpre, 64], never written); what a row has appended itself lives
// in kown / vown [R, h, Lown, 64] from row 0 on, so logical key j is prompt row j (j < p) or own row j - p.
// One workgroup per (prompt, head, chunk of NQ queries, key split).  It is rel_attn_decode_kernel's walk over the logical keys
// -- the same (wave, key slot) streams, the same key ranges, the same merge tree -- with NQ online-softmax states per lane.
// An iteration whose 8 keys all lie below p loads K, E and V once for the NQ queries (plain loads: a prompt's rows are read
// by every chunk of the prompt and again at the next step, and a prompt cache is 1/N of the repeated call's); from p on every
// query walks its own rows (nontemporal, as above).  A chunk's spare queries (N % NQ) repeat its last row and store nothing.
// The positions cannot be checked on the host: a prompt whose (t, p) break the contract gets an empty key range and no append.
// ---------------------------------------------------------------------------------------------------
constexpr int SHARED_NQ = MGX_SHARED_NQ;

template <int NQ>
__global__ __launch_bounds__(64 * DEC_WAVES) void rel_attn_decode_shared_kernel(
    const uint16_t* __restrict__ qkv_new, const uint16_t* __restrict__ kpre, const uint16_t* __restrict__ vpre,
    uint16_t* __restrict__ kown, uint16_t* __restrict__ vown, const uint16_t* __restrict__ E,
    const int32_t* __restrict__ pos_rows, const int32_t* __restrict__ pre_rows, uint16_t* __restrict__ ctx,
    float* __restrict__ partial, int N, int Lpre, int Lown, int d, int M) {
    const int heads = d >> 6, chunks = (N + NQ - 1) / NQ;
    const int ch = blockIdx.x % chunks, hd = (blockIdx.x / chunks) % heads, b = blockIdx.x / (chunks * heads);
    const int nsplit = gridDim.y, sp = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ks = lane >> 3, dg = lane & 7;
    const int r0 = b * N + ch * NQ, nq = min(NQ, N - ch * NQ);   // the chunk's rows r0 .. r0 + nq - 1
    int t = pos_rows[b * N], p = pre_rows[b];
    const bool ok = p >= 0 && p <= Lpre && p <= t && t - p < Lown && t < M;
    if (!ok) t = p = 0;                                          // nothing below is addressed from a value outside the contract
    // append every row's k_t, v_t at its own row t - p (split 0; 16 threads per query: 8 for K, 8 for V)
    if (sp == 0 && ok && tid < 16 * NQ) {
        const int qi = tid >> 4, kv = (tid >> 3) & 1, c = (tid & 7) * 8;
        if (qi < nq) {
            uint16_t* dst = (kv ? vown : kown) + (((size_t)(r0 + qi) * heads + hd) * Lown + (t - p)) * 64 + c;
            *(u32x4*)dst = *(const u32x4*)(qkv_new + (size_t)(r0 + qi) * 3 * d + (1 + kv) * d + hd * 64 + c);
        }
    }
    const uint16_t* qrow[NQ];
    size_t own[NQ];                                              // element offset of the query's own rows (wave-uniform)
    float q[NQ][8], m[NQ], l[NQ], acc[NQ][8];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int r = r0 + min(i, nq - 1);
        qrow[i] = qkv_new + (size_t)r * 3 * d + hd * 64;
        own[i] = ((size_t)r * heads + hd) * Lown * 64;
        unpack8(*(const u32x4*)(qrow[i] + dg * 8), q[i]);
        m[i] = -INFINITY, l[i] = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { q[i][k] *= 0.125f * LOG2E; acc[i][k] = 0.f; }
    }
    int lo = 0, hi = 0;
    if (ok) dec_key_range(t, nsplit, sp, lo, hi);
    const uint16_t* kp0 = kpre + ((size_t)b * heads + hd) * Lpre * 64;
    const uint16_t* vp0 = vpre + ((size_t)b * heads + hd) * Lpre * 64;
    const uint16_t* Eb = E + (size_t)(M - 1 - t) * 64;
    // one query's step of the online softmax on the key this lane group holds
    auto step = [&](int i, const float* ke, const float* vf, bool valid) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += q[i][k] * ke[k];
        // the key's 8 lanes: the values of the xor-1, -2, -4 butterfly, as DPP adds (NQ butterflies per key through
        // ds_bpermute would be most of the loop; after two steps a quad holds one sum, so the half-row mirror is the xor-4)
        s += dpp_mov<0xB1>(s);                                  // quad_perm [1,0,3,2]
        s += dpp_mov<0x4E>(s);                                  // quad_perm [2,3,0,1]
        s += dpp_mov<0x141>(s);                                 // row_half_mirror
        if (!valid) s = -INFINITY;
        const float mn = fmaxf(m[i], s);
        const float alpha = (mn == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m[i] - mn);
        const float pr = (mn == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(s - mn);
        l[i] = l[i] * alpha + pr;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[i][k] = acc[i][k] * alpha + pr * vf[k];
        m[i] = mn;
    };
    // The walk is rel_attn_decode_kernel's, in two phases.  While the wave's 8 keys are prompt rows (j0 + 7 < p; jc <= j0 + 7): one
    // load of K, E and V for all NQ queries, the next iteration's issued before this one's arithmetic (two workgroups per CU
    // at NQ = 2, one from NQ = 4 on: little else hides the latency).  From p on (and the iteration that straddles p): row by
    // row, so a split that holds own rows does NQ times the work per key of one that holds prompt rows.
    int j0 = lo + (w * 8);
    const int end_pre = min(hi, p - 7);
    u32x4 kw, ew, vw;
    auto load_pre = [&](int at) {
        const int jc = min(at + ks, hi - 1);
        kw = *(const u32x4*)(kp0 + (size_t)jc * 64 + dg * 8);
        ew = *(const u32x4*)(Eb + (size_t)jc * 64 + dg * 8);
        vw = *(const u32x4*)(vp0 + (size_t)jc * 64 + dg * 8);
    };
    if (j0 < end_pre) load_pre(j0);
    for (; j0 < end_pre; j0 += DEC_WAVES * 8) {
        const bool valid = j0 + ks < hi;
        float kf[8], ef[8], vf[8];
        unpack8(kw, kf);
        unpack8(ew, ef);
        unpack8(vw, vf);
        if (j0 + DEC_WAVES * 8 < end_pre) load_pre(j0 + DEC_WAVES * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) kf[k] += ef[k];
#pragma unroll
        for (int i = 0; i < NQ; ++i) step(i, kf, vf, valid);
    }
    for (; j0 < hi; j0 += DEC_WAVES * 8) {
        const int j = j0 + ks;
        const bool valid = j < hi;
        const int jc = valid ? j : hi - 1;
        float kf[8], ef[8], vf[8];
        unpack8(*(const u32x4*)(Eb + (size_t)jc * 64 + dg * 8), ef);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const uint16_t* kp = jc < p ? kp0 + (size_t)jc * 64 : jc == t ? qrow[i] + d : kown + own[i] + (size_t)(jc - p) * 64;
            const uint16_t* vp = jc < p ? vp0 + (size_t)jc * 64 : jc == t ? qrow[i] + 2 * d : vown + own[i] + (size_t)(jc - p) * 64;
            unpack8(__builtin_nontemporal_load((const u32x4*)(kp + dg * 8)), kf);
            unpack8(__builtin_nontemporal_load((const u32x4*)(vp + dg * 8)), vf);
#pragma unroll
            for (int k = 0; k < 8; ++k) kf[k] += ef[k];
            step(i, kf, vf, valid);
        }
    }
    // dec_finish<8> per query: the key slots of the wave, then the 8 waves through LDS
    __shared__ float sm[NQ][DEC_WAVES], sl[NQ][DEC_WAVES], sacc[NQ][DEC_WAVES][64];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
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
    for (int i = w; i < nq; i += DEC_WAVES) {                   // wave w merges query w (and w + 8): one output per lane
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
        const size_t rh = (size_t)(r0 + i) * heads + hd;
        if (nsplit == 1) {
            ctx[rh * 64 + lane] = f32_to_bf16(o / ll);
        } else {                                                // rel_attn_decode_merge_kernel's record of (row, head, split)
            float* pp = partial + (rh * nsplit + sp) * DEC_PART;
            if (lane == 0) { pp[64] = mm; pp[65] = ll; }
            pp[lane] = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// 8-bit K/V cache (ABI 20): codes uint8 [B, h, Lmax, 64] in OCP e4m3fn, one f32 scale per (b, h, row); element = code * scale.
// A row x of 64 values is quantized in f32:  amax = max |x_i|;  amax == 0: scale 0, codes 0;  else inv = 448 / amax,
// code_i = e4m3fn_rne(x_i * inv), scale = amax / 448  (x_i * inv never rounds above 448: no code is NaN).
// Four consecutive lanes hold one row, 16 values each: a lane's 16 codes are one 16-byte word.
// ---------------------------------------------------------------------------------------------------
MGX_DEV u32x4 fp8_quant16(const float* x, float& scale) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) a = fmaxf(a, fabsf(x[k]));
    a = fmaxf(a, __shfl_xor(a, 1, 64));
    a = fmaxf(a, __shfl_xor(a, 2, 64));
    scale = a / 448.0f;
    const float inv = 448.0f / a;
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int v = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * k] * inv, x[4 * k + 1] * inv, 0, false);
        v = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * k + 2] * inv, x[4 * k + 3] * inv, v, true);
        c[k] = a == 0.f ? 0u : (uint32_t)v;
    }
    return u32x4{c[0], c[1], c[2], c[3]};
}
MGX_DEV void fp8_unpack16(const u32x4& w, float* f) {
    const uint32_t c[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[k], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[k], true);
        f[4 * k] = lo.x; f[4 * k + 1] = lo.y; f[4 * k + 2] = hi.x; f[4 * k + 3] = hi.y;
    }
}
MGX_DEV void unpack16(const uint16_t* p, float* f) {            // 16 bf16 -> f32 (two 16-byte loads)
    unpack8(*(const u32x4*)p, f);
    unpack8(*(const u32x4*)(p + 8), f + 8);
}

// The attention of rel_attn_decode_kernel over the 8-bit cache: the same split-K scheme, partial layout and merge kernel.
// lane = (key slot ks = lane>>2, dim group dg = lane&3): a wave handles 16 keys per iteration, each lane 16 of the 64 dims
// (a 16-byte load of codes; a key costs 64 + 64 bytes of codes and 4 + 4 of scales instead of 256).
// s_j = scale_k[j] (q.code_k[j]) + q.E_row, and p_j scale_v[j] weights the V codes.  Row t enters its own step already
// quantized: the key slot that covers j == t quantizes k_t / v_t from qkv_new in registers with the appender's arithmetic, so
// the call is exactly attention over the dequantized rows 0..t.
__global__ __launch_bounds__(64 * DEC_WAVES) void rel_attn_decode_fp8_kernel(
    const uint16_t* __restrict__ qkv_new, uint8_t* __restrict__ kcache, uint8_t* __restrict__ vcache, float* __restrict__ kscale,
    float* __restrict__ vscale, const uint16_t* __restrict__ E, StepPos stp, uint16_t* __restrict__ ctx, float* __restrict__ partial,
    int Lmax, int d, int M) {
    const int heads = d >> 6;
    const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
    const int nsplit = gridDim.y, sp = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ks = lane >> 2, dg = lane & 3;
    const int t = stp.at(b);
    const uint16_t* qrow = qkv_new + (size_t)b * 3 * d + hd * 64;
    const size_t row0 = ((size_t)b * heads + hd) * Lmax;
    uint8_t* kc = kcache + row0 * 64;
    uint8_t* vc = vcache + row0 * 64;
    float* ksc = kscale + row0;
    float* vsc = vscale + row0;
    // append row t (split 0): lanes 0-3 quantize k_t, lanes 4-7 v_t
    if (sp == 0 && tid < 8) {
        const int kv = tid >> 2;
        float x[16], sc;
        unpack16(qrow + (1 + kv) * d + dg * 16, x);
        const u32x4 c = fp8_quant16(x, sc);
        *(u32x4*)((kv ? vc : kc) + (size_t)t * 64 + dg * 16) = c;
        if (dg == 0) (kv ? vsc : ksc)[t] = sc;
    }
    float q[16];
    unpack16(qrow + dg * 16, q);
#pragma unroll
    for (int k = 0; k < 16; ++k) q[k] *= 0.125f * LOG2E;
    int lo, hi;
    dec_key_range(t, nsplit, sp, lo, hi);

    float m = -INFINITY, l = 0.f, acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
    const uint16_t* Eb = E + (size_t)(M - 1 - t) * 64;
    for (int j0 = lo + (w * 16); j0 < hi; j0 += DEC_WAVES * 16) {
        const int j = j0 + ks;
        const bool valid = j < hi;
        const int jc = valid ? j : hi - 1;
        u32x4 kw = __builtin_nontemporal_load((const u32x4*)(kc + (size_t)jc * 64 + dg * 16));
        u32x4 vw = __builtin_nontemporal_load((const u32x4*)(vc + (size_t)jc * 64 + dg * 16));
        float sk = __builtin_nontemporal_load(ksc + jc), sv = __builtin_nontemporal_load(vsc + jc);
        if (jc == t) {                                          // row t: from qkv_new, quantized here (the append races)
            float x[16];
            unpack16(qrow + d + dg * 16, x);
            kw = fp8_quant16(x, sk);
            unpack16(qrow + 2 * d + dg * 16, x);
            vw = fp8_quant16(x, sv);
        }
        float kf[16], ef[16], vf[16];
        fp8_unpack16(kw, kf);
        unpack16(Eb + (size_t)jc * 64 + dg * 16, ef);
        fp8_unpack16(vw, vf);
        float sq = 0.f, se = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) { sq += q[k] * kf[k]; se += q[k] * ef[k]; }
        float s = sk * sq + se;
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (!valid) s = -INFINITY;
        const float mn = fmaxf(m, s);
        const float alpha = (mn == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m - mn);
        const float p = (mn == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(s - mn);
        l = l * alpha + p;
        const float pv = p * sv;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = acc[k] * alpha + pv * vf[k];
        m = mn;
    }
    dec_finish<16>(m, l, acc, ctx, partial, b, hd, d, nsplit, sp, tid, w, ks, dg);
}

// rows 0..n-1 of the K and V columns of qkv bf16 [B, Lrows, 3d] -> the 8-bit caches: one 4-lane group per (b, row, K|V, head)
// (groups of one row side by side: each reads a 128-byte run of the qkv row, writes a 64-byte run of codes)
__global__ __launch_bounds__(256) void kv_store_fp8_kernel(const uint16_t* __restrict__ qkv, int Lrows, int n,
                                                           uint8_t* __restrict__ kcache, uint8_t* __restrict__ vcache,
                                                           float* __restrict__ kscale, float* __restrict__ vscale, int B, int Lmax,
                                                           int d) {
    const int heads = d >> 6;
    const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const int dg = threadIdx.x & 3;
    if (g >= (size_t)B * n * 2 * heads) return;                  // whole 4-lane groups leave together
    const int hd = (int)(g % heads), kv = (int)((g / heads) & 1);
    const size_t br = g / heads / 2;                             // b * n + row
    const int row = (int)(br % n), b = (int)(br / n);
    float x[16], sc;
    unpack16(qkv + ((size_t)b * Lrows + row) * 3 * d + (1 + kv) * d + hd * 64 + dg * 16, x);
    const u32x4 c = fp8_quant16(x, sc);
    const size_t r = ((size_t)b * heads + hd) * Lmax + row;
    *(u32x4*)((kv ? vcache : kcache) + r * 64 + dg * 16) = c;
    if (dg == 0) (kv ? vscale : kscale)[r] = sc;
}

// ---------------------------------------------------------------------------------------------------
// sampling: one wave per row, V <= 64 * 16 (the draw itself: sample_draw, decode_common.hpp)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sample_kernel(const uint16_t* __restrict__ logits, int V, int ld, float inv_temp,
                                                    int top_k, float top_p, uint64_t seed, StepPos stp,
                                                    int32_t* __restrict__ next_tok, int32_t* __restrict__ out_tokens,
                                                    int out_ld, float* __restrict__ probs_out, int row0,
                                                    const uint32_t* __restrict__ allow_table) {
    const int row = blockIdx.x, lane = threadIdx.x;
    // grammar mask: row `prev` of allow_table (bit v = token v may follow token prev); the previous
    // token is what next_tok still holds.  A row that allows nothing is ignored.
    const uint32_t* arow = allow_table ? grammar_row(allow_table, next_tok[row], V) : nullptr;
    const int step = stp.step(row);                      // the absolute step: the position, plus the window's base if there is one
    float unused[SMP_PER_LANE];
    const int choice = sample_draw<false>(logits + (size_t)row * ld, V, inv_temp, top_k, top_p, arow,
                                          u01(seed, (uint32_t)step, (uint32_t)(row0 + row)), lane,
                                          probs_out ? probs_out + (size_t)row * V : nullptr, unused);
    if (lane == 0) {
        next_tok[row] = choice;
        if (out_tokens) out_tokens[(size_t)row * out_ld + step + 1] = choice;
    }
}
// the sampler's advance over the n counters (n = B per row, 1 shared)
__global__ __launch_bounds__(256) void advance_pos_kernel(int32_t* __restrict__ pos_dev, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pos_dev[i] += 1;
}
// mgx_decode_reanchor, in two launches so that no workgroup reads a position another has already moved: the n counters first
// (as above), then the prefill's token matrix from the moved window
__global__ __launch_bounds__(256) void reanchor_move_kernel(int32_t* __restrict__ pos_dev, int32_t* __restrict__ base_dev, int n,
                                                            int hop) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { pos_dev[i] -= hop; base_dev[i] += hop; }
}
__global__ __launch_bounds__(256) void reanchor_fill_kernel(StepPos stp, const int32_t* __restrict__ out_tokens, int out_ld,
                                                            int32_t* __restrict__ seq, int n_pad, int pad_token, int B) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B * n_pad) return;
    const int b = g / n_pad, i = g % n_pad;
    const int t = stp.at(b), col = stp.base_at(b) + i;
    // the contract keeps col inside the row for i < t; a row that breaks it reads pad_token, never past out_tokens
    seq[g] = (i < t && col >= 0 && col < out_ld) ? out_tokens[(size_t)b * out_ld + col] : pad_token;
}

extern "C" int mgx_decode_embed(const int32_t* tok, const float* table, const float* pe, const int32_t* pos_dev, int per_row,
                                uint16_t* out, int B, int d, int V, void* stream) {
    const char* name = "mgx_decode_embed";
    MGX_REQUIRE(tok && table && pe && pos_dev && out, MGX_ERR_NULL, "%s: NULL pointer", name);
    MGX_REQUIRE(B > 0 && d > 0 && d % 8 == 0 && V > 0, MGX_ERR_SHAPE, "%s: need d%%8==0 (B=%d d=%d)", name, B, d);
    const int total = B * (d / 8);
    hipLaunchKernelGGL(decode_embed_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, tok, table, pe,
                       StepPos{pos_dev, nullptr, per_row}, out, B, d, V, sqrtf((float)d));
    MGX_CHECK_LAUNCH(name);
    return MGX_OK;
}

// key splits per (b,h): enough workgroups to keep ~4 per CU (32 waves) streaming once the cache is long; short caches
// keep one workgroup (the merge launch would cost more than it saves)
static int decode_splits(int B, int Lmax, int d) {
    const int wgs = B * (d / 64);
    if (Lmax < 1024) return 1;
    int s = 1;
    while (s < 8 && wgs * s < 1024 && Lmax / (2 * s) >= 512) s *= 2;
    return s;
}

extern "C" int mgx_rel_attn_decode_splits(int B, int Lmax, int d) {
    return (B <= 0 || d <= 0 || Lmax <= 0) ? 0 : decode_splits(B, Lmax, d);
}

extern "C" size_t mgx_rel_attn_decode_workspace(int B, int Lmax, int d) {
    if (B <= 0 || d <= 0 || Lmax <= 0) return 0;
    const int s = decode_splits(B, Lmax, d);
    return s == 1 ? 0 : (size_t)B * (d / 64) * s * DEC_PART * sizeof(float);
}

// the two attention entry points.  FP8: the caches are e4m3fn codes with their two scale arrays; it takes the bf16 cache's key
// splits, so mgx_rel_attn_decode_workspace / _splits cover both
template <bool FP8>
static int rel_attn_decode(const uint16_t* qkv_new, void* kcache, void* vcache, float* kscale, float* vscale, const uint16_t* E,
                           const int32_t* pos_dev, int per_row, uint16_t* ctx, void* workspace, size_t ws_bytes, int B, int Lmax,
                           int d, int M, void* stream, const char* name) {
    MGX_REQUIRE(qkv_new && kcache && vcache && (!FP8 || (kscale && vscale)) && E && pos_dev && ctx, MGX_ERR_NULL, "%s: NULL pointer",
                name);
    MGX_REQUIRE(B > 0 && d > 0 && d % 64 == 0 && Lmax > 0 && M >= Lmax, MGX_ERR_SHAPE,
                "%s: need d%%64==0 and M>=Lmax (B=%d Lmax=%d d=%d M=%d)", name, B, Lmax, d, M);
    const int ns = decode_splits(B, Lmax, d);
    MGX_REQUIRE(ns == 1 || (workspace && ws_bytes >= mgx_rel_attn_decode_workspace(B, Lmax, d)), MGX_ERR_SHAPE,
                "%s: workspace must hold mgx_rel_attn_decode_workspace() = %zu bytes (got %zu)", name,
                mgx_rel_attn_decode_workspace(B, Lmax, d), ws_bytes);
    const dim3 grid(B * (d / 64), ns), block(64 * DEC_WAVES);
    const StepPos stp{pos_dev, nullptr, per_row};
    if constexpr (FP8)
        hipLaunchKernelGGL(rel_attn_decode_fp8_kernel, grid, block, 0, (hipStream_t)stream, qkv_new, (uint8_t*)kcache,
                           (uint8_t*)vcache, kscale, vscale, E, stp, ctx, (float*)workspace, Lmax, d, M);
    else
        hipLaunchKernelGGL(rel_attn_decode_kernel, grid, block, 0, (hipStream_t)stream, qkv_new, (uint16_t*)kcache,
                           (uint16_t*)vcache, E, stp, ctx, (float*)workspace, Lmax, d, M);
    if (ns > 1)
        hipLaunchKernelGGL(rel_attn_decode_merge_kernel, dim3(B * (d / 64)), dim3(64), 0, (hipStream_t)stream,
                           (const float*)workspace, ctx, ns, d);
    MGX_CHECK_LAUNCH(name);
    return MGX_OK;
}

extern "C" int mgx_rel_attn_decode(const uint16_t* qkv_new, uint16_t* kcache, uint16_t* vcache, const uint16_t* E,
                                   const int32_t* pos_dev, int per_row, uint16_t* ctx, void* workspace, size_t ws_bytes, int B,
                                   int Lmax, int d, int M, void* stream) {
    return rel_attn_decode<false>(qkv_new, kcache, vcache, nullptr, nullptr, E, pos_dev, per_row, ctx, workspace, ws_bytes, B, Lmax,
                                  d, M, stream, "mgx_rel_attn_decode");
}

extern "C" int mgx_rel_attn_decode_fp8(const uint16_t* qkv_new, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                                       const uint16_t* E, const int32_t* pos_dev, int per_row, uint16_t* ctx, void* workspace,
                                       size_t ws_bytes, int B, int Lmax, int d, int M, void* stream) {
    return rel_attn_decode<true>(qkv_new, kcache, vcache, kscale, vscale, E, pos_dev, per_row, ctx, workspace, ws_bytes, B, Lmax, d,
                                 M, stream, "mgx_rel_attn_decode_fp8");
}

// key splits of the shared-prompt attention, from the shapes alone.  A call has Bp * h * ceil(N / NQ) workgroups per split where
// the repeated call has Bp * N * h, so it splits further than decode_splits: up to 16, shares of 512 keys or more
static int shared_splits(int Bp, int N, int Lpre, int Lown, int d) {
    const long long wgs = (long long)Bp * (d / 64) * ((N + SHARED_NQ - 1) / SHARED_NQ), L = (long long)Lpre + Lown;
    if (L < 1024) return 1;
    int s = 1;
    while (s < 16 && wgs * s < 1024 && L / (2 * s) >= 512) s *= 2;
    return s;
}

extern "C" int mgx_rel_attn_decode_shared_splits(int Bp, int N, int Lpre, int Lown, int d) {
    return (Bp <= 0 || N <= 0 || Lpre <= 0 || Lown <= 0 || d <= 0) ? 0 : shared_splits(Bp, N, Lpre, Lown, d);
}

extern "C" size_t mgx_rel_attn_decode_shared_workspace(int Bp, int N, int Lpre, int Lown, int d) {
    if (Bp <= 0 || N <= 0 || Lpre <= 0 || Lown <= 0 || d <= 0) return 0;
    const int s = shared_splits(Bp, N, Lpre, Lown, d);
    return s == 1 ? 0 : (size_t)Bp * N * (d / 64) * s * DEC_PART * sizeof(float);
}

extern "C" int mgx_rel_attn_decode_shared(const uint16_t* qkv_new, const uint16_t* kpre, const uint16_t* vpre, uint16_t* kown,
                                          uint16_t* vown, const uint16_t* E, const int32_t* pos_rows, const int32_t* pre_rows,
                                          uint16_t* ctx, void* workspace, size_t ws_bytes, int Bp, int N, int Lpre, int Lown, int d,
                                          int M, void* stream) {
    const char* name = "mgx_rel_attn_decode_shared";
    MGX_REQUIRE(qkv_new && kpre && vpre && kown && vown && E && pos_rows && pre_rows && ctx, MGX_ERR_NULL, "%s: NULL pointer", name);
    MGX_REQUIRE(Bp > 0 && N >= 1 && N <= MGX_SHARED_MAX_N && Lpre >= 1 && Lown >= 1 && d > 0 && d % 64 == 0 && M >= 1, MGX_ERR_SHAPE,
                "%s: need 1<=N<=%d, Lpre>=1, Lown>=1, d%%64==0, M>=1 (Bp=%d N=%d Lpre=%d Lown=%d d=%d M=%d)", name, MGX_SHARED_MAX_N,
                Bp, N, Lpre, Lown, d, M);
    const long long wgs = (long long)Bp * (d / 64) * ((N + SHARED_NQ - 1) / SHARED_NQ);
    MGX_REQUIRE(wgs <= 0x7fffffff && (long long)Bp * N * (d / 64) <= 0x7fffffff, MGX_ERR_SHAPE, "%s: too many rows (Bp=%d N=%d d=%d)",
                name, Bp, N, d);
    const int ns = shared_splits(Bp, N, Lpre, Lown, d);
    const size_t need = mgx_rel_attn_decode_shared_workspace(Bp, N, Lpre, Lown, d);
    MGX_REQUIRE(ns == 1 || (workspace && ws_bytes >= need), MGX_ERR_SHAPE,
                "%s: workspace must hold mgx_rel_attn_decode_shared_workspace() = %zu bytes (got %zu)", name, need, ws_bytes);
    hipLaunchKernelGGL(rel_attn_decode_shared_kernel<SHARED_NQ>, dim3((unsigned)wgs, ns), dim3(64 * DEC_WAVES), 0, (hipStream_t)stream,
                       qkv_new, kpre, vpre, kown, vown, E, pos_rows, pre_rows, ctx, (float*)workspace, N, Lpre, Lown, d, M);
    if (ns > 1)
        hipLaunchKernelGGL(rel_attn_decode_merge_kernel, dim3(Bp * N * (d / 64)), dim3(64), 0, (hipStream_t)stream,
                           (const float*)workspace, ctx, ns, d);
    MGX_CHECK_LAUNCH(name);
    return MGX_OK;
}

extern "C" int mgx_kv_store_fp8(const uint16_t* qkv, int Lrows, int n, uint8_t* kcache, uint8_t* vcache, float* kscale,
                                float* vscale, int B, int Lmax, int d, void* stream) {
    MGX_REQUIRE(qkv && kcache && vcache && kscale && vscale, MGX_ERR_NULL, "mgx_kv_store_fp8: NULL pointer");
    MGX_REQUIRE(B > 0 && d > 0 && d % 64 == 0 && n >= 0 && n <= Lrows && n <= Lmax, MGX_ERR_SHAPE,
                "mgx_kv_store_fp8: need d%%64==0 and 0<=n<=min(Lrows,Lmax) (B=%d Lrows=%d n=%d Lmax=%d d=%d)", B, Lrows, n, Lmax, d);
    if (n == 0) return MGX_OK;
    const size_t threads = (size_t)B * n * 2 * (d / 64) * 4;
    MGX_REQUIRE((threads + 255) / 256 <= 0x7fffffff, MGX_ERR_SHAPE, "mgx_kv_store_fp8: too many rows (B=%d n=%d d=%d)", B, n, d);
    hipLaunchKernelGGL(kv_store_fp8_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, qkv, Lrows, n,
                       kcache, vcache, kscale, vscale, B, Lmax, d);
    MGX_CHECK_LAUNCH("mgx_kv_store_fp8");
    return MGX_OK;
}

// advance: one more launch moves the position(s) on.  base_dev: the window's base(s), or NULL
extern "C" int mgx_sample_topk_topp(const uint16_t* logits, int V, int ld, float temperature, int top_k, float top_p, uint64_t seed,
                                    int32_t* pos_dev, const int32_t* base_dev, int per_row, int32_t* next_tok, int32_t* out_tokens,
                                    int out_ld, float* probs_out, int B, int row0, int advance, const uint32_t* allow_table,
                                    void* stream) {
    const char* name = "mgx_sample_topk_topp";
    MGX_REQUIRE(logits && pos_dev && next_tok, MGX_ERR_NULL, "%s: NULL pointer", name);
    MGX_REQUIRE(B > 0 && V > 0 && V <= 64 * SMP_PER_LANE && ld >= V && temperature > 0.f && top_p > 0.f && row0 >= 0, MGX_ERR_SHAPE,
                "%s: need 0<V<=%d, ld>=V, temperature>0, top_p>0, row0>=0 (V=%d ld=%d)", name, 64 * SMP_PER_LANE, V, ld);
    hipLaunchKernelGGL(sample_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, V, ld, 1.f / temperature, top_k, top_p, seed,
                       StepPos{pos_dev, base_dev, per_row}, next_tok, out_tokens, out_ld, probs_out, row0, allow_table);
    if (advance) {
        const int n = per_row ? B : 1;
        hipLaunchKernelGGL(advance_pos_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, pos_dev, n);
    }
    MGX_CHECK_LAUNCH(name);
    return MGX_OK;
}

extern "C" int mgx_decode_reanchor(int32_t* pos_dev, int32_t* base_dev, int per_row, const int32_t* out_tokens, int out_ld,
                                   int32_t* seq, int n_pad, int hop, int pad_token, int B, void* stream) {
    MGX_REQUIRE(pos_dev && base_dev && out_tokens && seq, MGX_ERR_NULL, "mgx_decode_reanchor: NULL pointer");
    MGX_REQUIRE(B > 0 && n_pad > 0 && out_ld > 0 && hop >= 0 && (size_t)B * n_pad <= 0x7fffffff, MGX_ERR_SHAPE,
                "mgx_decode_reanchor: need B>0, n_pad>0, out_ld>0, hop>=0, B*n_pad<2^31 (B=%d n_pad=%d out_ld=%d hop=%d)", B, n_pad,
                out_ld, hop);
    const int n = per_row ? B : 1;
    hipLaunchKernelGGL(reanchor_move_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, pos_dev, base_dev, n, hop);
    hipLaunchKernelGGL(reanchor_fill_kernel, dim3((B * n_pad + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       StepPos{pos_dev, base_dev, per_row}, out_tokens, out_ld, seq, n_pad, pad_token, B);
    MGX_CHECK_LAUNCH("mgx_decode_reanchor");
    return MGX_OK;
}

// ---------------------------------------------------------------------------------------------------
// K13: Event_Melody_RNN step pieces (Event_MelodyRNN/network.py:51-61): row gather + fused GRU gates
// ---------------------------------------------------------------------------------------------------
// out bf16 [B, ld] = table bf16 [V, ld][tok]        (ld = embedding width padded to the GEMM's K % 64)
__global__ __launch_bounds__(256) void gather_rows_kernel(const int32_t* __restrict__ tok, const uint16_t* __restrict__ table,
                                                          uint16_t* __restrict__ out, int B, int ld, int V) {
    const int gpr = ld >> 3;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= B * gpr) return;
    const int r = g / gpr, c = (g % gpr) * 8;
    int t = tok[r];
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);
    *(u32x4*)(out + (size_t)r * ld + c) = *(const u32x4*)(table + (size_t)t * ld + c);
}
// torch.nn.GRU cell (gate order r,z,n):  r = s(gi_r+gh_r), z = s(gi_z+gh_z), n = tanh(gi_n + r*gh_n),
// h' = (1-z)*n + z*h.   gi, gh bf16 [B,3H] (biases already added by the GEMM epilogue), h f32 [B,H] in/out,
// h_bf16 [B,H] = bf16(h') for the next GEMM.
__global__ __launch_bounds__(256) void gru_gates_kernel(const uint16_t* __restrict__ gi, const uint16_t* __restrict__ gh,
                                                        float* __restrict__ h, uint16_t* __restrict__ h_bf16, int B, int H) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, k = i % H;
    const size_t o = (size_t)b * 3 * H + k;
    const float ir = bf16_to_f32(gi[o]), iz = bf16_to_f32(gi[o + H]), in_ = bf16_to_f32(gi[o + 2 * H]);
    const float hr = bf16_to_f32(gh[o]), hz = bf16_to_f32(gh[o + H]), hn = bf16_to_f32(gh[o + 2 * H]);
    const float r = 1.f / (1.f + __expf(-(ir + hr)));
    const float z = 1.f / (1.f + __expf(-(iz + hz)));
    const float n = tanhf(in_ + r * hn);
    const float hv = (1.f - z) * n + z * h[i];
    h[i] = hv;
    h_bf16[i] = f32_to_bf16(hv);
}

extern "C" int mgx_gather_rows(const int32_t* tok, const uint16_t* table, uint16_t* out, int B, int ld, int V, void* stream) {
    MGX_REQUIRE(tok && table && out, MGX_ERR_NULL, "mgx_gather_rows: NULL pointer");
    MGX_REQUIRE(B > 0 && V > 0 && ld > 0 && ld % 8 == 0, MGX_ERR_SHAPE, "mgx_gather_rows: need ld%%8==0 (ld=%d)", ld);
    const int total = B * (ld / 8);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, tok, table, out, B, ld, V);
    MGX_CHECK_LAUNCH("mgx_gather_rows");
    return MGX_OK;
}
extern "C" int mgx_gru_gates(const uint16_t* gi, const uint16_t* gh, float* h, uint16_t* h_bf16, int B, int H, void* stream) {
    MGX_REQUIRE(gi && gh && h && h_bf16, MGX_ERR_NULL, "mgx_gru_gates: NULL pointer");
    MGX_REQUIRE(B > 0 && H > 0, MGX_ERR_SHAPE, "mgx_gru_gates: bad shape");
    hipLaunchKernelGGL(gru_gates_kernel, dim3((B * H + 255) / 256), dim3(256), 0, (hipStream_t)stream, gi, gh, h, h_bf16, B, H);
    MGX_CHECK_LAUNCH("mgx_gru_gates");
    return MGX_OK;
}

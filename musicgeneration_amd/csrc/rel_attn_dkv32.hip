// K2 of the attention backward (overview and math: rel_attn_bwd.hip): dK, dV with 32 keys per wave, and the stored dS tiles.
// workgroup = 128 keys (wave = 32 keys, K/V row fragments in registers), sweeps query tiles i0 = J0, J0+32, ...
// orientation: queries on registers, keys on lanes (S, P, dP, dS); accumulators dK^T[c][b], dV^T[c][b].
// This is the kernel for L % 128 != 0 and the cross-check (parts bit 64) of the 64-keys-per-wave kernel with the generated asm
// sweep (rel_attn_dkv64.hip), which runs wherever the sequence is whole 128-key blocks; both give the same bits.
#include <type_traits>
#include "rel_attn_common.hpp"

using namespace relattn;

#ifndef MGX_DKV_PEEL
#define MGX_DKV_PEEL 0      // timing experiments only (tools/peel_dkv.sh): 1 no E loads in the sweep | 2 no dS stores | 4 no skew (bpermute)
#endif                      // | 8 no exponentials | 16 no q / dO tile prefetch+publish (the first tile is reused) | 32 no lse / delta reads
                            // (constants); results are then wrong
// MGX_DKV_STAMP (diagnostic build only, `_build.py --variant dkvstamp -DMGX_DKV_STAMP`; tools/dkv_stamp.py): s_memtime stamps at five
// points of a main-loop step; lane 0 of every wave leaves its sums in its first dk row (the results are then garbage).  Reading
// a stamp waits for lgkmcnt(0), i.e. for the wave's outstanding LDS operations: the stamped kernel is a little slower.
#ifdef MGX_DKV_STAMP
#define DKV_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
                          __builtin_amdgcn_sched_barrier(0); if (!MASKED) st_acc[i] += t_ - st_last; st_last = t_; } while (0)
#else
#define DKV_STAMP(i)
#endif
// (round 4 experiment, removed: log2(e)/8 folded into K and into a scaled copy of the Er fragments, -lse log2(e) as the initial
//  accumulator of the Q.Er^T products, so that S arrives as the exponent's argument -- 16 fewer VALU per tile: 1.258 ms against
//  1.262 at cfg2 / batch 64, nothing; and the backward's P would no longer equal the forward's bit for bit.)
// (experiments, removed -- all at cfg2 / batch 64:
//  * q and dO staged as separate images R and T, conflict-free reads, instead of ONE image R each: 1.252 against 1.227 ms -- two DMA
//    instructions more per wave and tile (a VMEM instruction costs the issuing wave ~50 cycles here, tools/dkv_stamp.py);
//  * the one image as an "image B", conflict-free for the row AND the transposed reads (the 37 M conflict cycles of the kernel's
//    211 M LDS cycles gone): 1.262-1.267 against 1.255-1.259 ms -- the conflicts cost nothing, the longer swizzle a little;
//  * two waves (64 keys) per workgroup -- a shorter diagonal block and twice the workgroups, but every wave stages twice as
//    much: 1.315 against 1.246 ms;
//  * a dynamic-LDS pad for one workgroup per CU, one wave per SIMD instead of two: 1.40 against 1.21 ms.)
namespace k2 {
constexpr int WAVES = 4;                                   // waves (= 32-key tiles) per workgroup
constexpr int OFF_QR = 0;                                  // 2 x 4K  qs image R (row and, with 2-way conflicts, transposed reads)
constexpr int OFF_QT = OFF_QR + 2 * TILE_BYTES;            // 2 x 4K  no longer written (was qs image T)
constexpr int OFF_OR = OFF_QT + 2 * TILE_BYTES;            // 2 x 4K  dO image R
constexpr int OFF_OT = OFF_OR + 2 * TILE_BYTES;            // 2 x 4K  no longer written (was dO image T).  The two holes stay: compacting them
                                                           //         moves every LDS immediate and the kernel's residency arithmetic
constexpr int ST_BYTES = 256 * WAVES;                      // per buffer: 4 waves x (-lse2[32], -delta[32]): every wave stages and reads its own copy
constexpr int OFF_ST = OFF_OT + 2 * TILE_BYTES;            // 2 x 1 KB
constexpr int PATCH_BYTES = 4608;                          // per wave: 32 rows x 144 B, the epilogue's row-major store patch
constexpr int OFF_BAND = OFF_ST + 2 * ST_BYTES;
constexpr int OFF_FLAG = OFF_BAND + WAVES * PATCH_BYTES;   // "a key of this workgroup is padded" flag
constexpr int LDS_BYTES = OFF_FLAG + 16;                   // 53,264 B (the 256 VGPRs limit the kernel to 2 waves per SIMD)
static_assert(LDS_BYTES == 53264, "the layout keeps its two 8 KB holes");
// The Er chunks (B operand of Q.Er^T: column t = lane&31, 16 contiguous bytes of row L-1-32q-t) are
// loaded straight from global/L2 into registers, one new chunk per step (the previous "hi" chunk is
// the next "lo" chunk), so E needs no LDS here.
}  // namespace k2

template <bool EXPORT_DS>     // always true (one instantiation): as a plain function hipcc builds a 36 % longer main loop from the same source
__global__ __launch_bounds__(64 * k2::WAVES, 2) void rel_attn_dkv_kernel(
    const uint16_t* __restrict__ qkv, const u32x4* __restrict__ EfA, const uint32_t* __restrict__ padbits,
    const uint16_t* __restrict__ dctx, const float* __restrict__ nlse2 /* -lse log2(e) */, const float* __restrict__ ndelta /* -delta */,
    uint16_t* __restrict__ dqkv, uint16_t* __restrict__ dst, int L, int d, int bgroup) {
    using namespace k2;
    extern __shared__ __attribute__((aligned(256))) char smem[];     // 256: the band reads XOR bit 7 of absolute LDS addresses
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bl = lane & 31, hh = lane >> 5;
    const int heads = d >> 6;
    const int nkb = (L + 32 * WAVES - 1) / (32 * WAVES);   // y = (batch group, key block): groups as in the dQ kernel
    // x = (b,h) inside the batch group, key-block rank 0 = longest sweep, dispatched first.  (experiment, removed: the (b,h) of a batch
    // group dealt to the XCDs, so that the 16 key-block workgroups of a (b,h) -- which all read its q / dO rows -- share one L2:
    // 1.270 against 1.274 ms at cfg2 / batch 64, nothing)
    const int bh_l = blockIdx.x, kbr = blockIdx.y % nkb;
    const int b = (blockIdx.y / nkb) * bgroup + bh_l / heads, hd = bh_l % heads;
    const int J0 = kbr * 32 * WAVES;
    const int nchunk = L >> 5;
    const int nT = (L - J0) >> 5;                          // query tiles i0 = J0 + 32 t
    const bool wave_on = J0 + w * 32 < L;
    // a wave beyond the end of the sequence (L % 128 != 0) shadows the last valid key block and stores nothing
    const int wk = wave_on ? w : nT - 1;                   // the wave's key tile inside the workgroup; D/32 = t - wk
    const int j0 = J0 + wk * 32;
    const size_t ld = (size_t)3 * d;
    const uint16_t* qkv_b = qkv + (size_t)b * L * ld;
    const size_t stat_base = ((size_t)b * heads + hd) * L;

    // Staging of a query tile (q and dO, one LDS image R each, and the two statistics of its 32 rows) is LDS-DMA: thread tid owns
    // the 16-byte slot tid of every image -- row tid >> 3, PHYSICAL chunk tid & 7 -- and fetches the logical chunk the image's
    // swizzle puts there (rel_attn_common.hpp: dma16), so a tile costs a wave three DMA instructions and neither registers nor
    // ds_write (round 3: 2 loads into registers, then 5 stores).  Every global address of the sweep is (wave-uniform base in
    // SGPRs) + (32-bit per-lane offset).
    const char* q_base = (const char*)(qkv_b + (size_t)J0 * ld + hd * 64);                      // + t * 32 rows
    const char* o_base = (const char*)(dctx + ((size_t)b * L + J0) * d + hd * 64);
    const int srow = tid >> 3, lcR = (tid & 7) ^ ((srow >> 1) & 7);                           // logical chunk: imgR_off inverted
    const uint32_t q_voffR = (uint32_t)((srow * ld + lcR * 8) * 2), o_voffR = (uint32_t)((srow * d + lcR * 8) * 2);
    const uint32_t q_step = (uint32_t)(32 * ld * 2), o_step = (uint32_t)(32 * d * 2);
    // fragment ks of Er chunk q for this lane (fragment-ordered copy: 1 KB contiguous per wave load).  Every load of the
    // sweep is unconditional with a clamped index; data of clamped tiles / chunks is never used.
    const uint32_t lane16 = (uint32_t)lane * 16u;
    auto e_frag = [&](int q, int ks) {
        return __builtin_bit_cast(bf16x8, *(const u32x4*)((const char*)EfA + (size_t)min(max(q, 0), nchunk - 1) * 4096 + ks * 1024 + lane16));
    };
    // -lse log2(e) (lanes 0..31) / -delta (lanes 32..63) of row (lane & 31) of a query tile, from the pre-pass's copies, in the form
    // the kernel consumes them -- the addend of the exponent's fma and the INITIAL ACCUMULATOR of dP = dO V^T (rows = queries) --,
    // so the DMA needs no arithmetic on the way.  Every wave stages (and reads) its own 256-byte copy: no statistic crosses waves.
    const uint32_t st_voff = (uint32_t)(((lane & 32) ? (const char*)ndelta - (const char*)nlse2 : 0) + (lane & 31) * 4);   // |offset| < 2^31: same allocation
    const char* st_base = (const char*)(nlse2 + stat_base + J0);
    const uint32_t lds_w = lds_addr_of(smem) + w * 1024;   // this wave's 1 KB of every 4 KB image; + OFF_ST: its 256 B of statistics
    auto stage = [&](int t, int buf) {                     // tile t (clamped) -> LDS buffers `buf`
        const int tn = (MGX_DKV_PEEL & 16) ? 0 : min(t, nT - 1);
        const char* qb = q_base + (size_t)tn * q_step;
        const char* ob = o_base + (size_t)tn * o_step;
        const uint32_t dw = lds_w + buf * TILE_BYTES;      // slots 64 w .. + 63
        dma16(qb, q_voffR, dw + OFF_QR);
        dma16(ob, o_voffR, dw + OFF_OR);
        dma4(st_base + (size_t)tn * 128, st_voff, lds_addr_of(smem) + OFF_ST + buf * ST_BYTES + w * 256);
    };
    stage(0, 0);
    // E chunk fragments: a step's "hi" chunk (t - wk) sits in e[PAR], the "lo" chunk (t - wk - 1) in e[PAR^1]; the slot of
    // the lo chunk receives chunk t - wk + 1 once it has been used, which is the next step's hi chunk.  The main loop
    // alternates PAR = 0, 1 (two steps per trip); the general body always uses PAR = 0 and swaps the slots afterwards.
    bf16x8 kf[4], vf[4], e[2][4];
    uint32_t padlane = 0;
    int wgpad = 0;
    {
        const uint16_t* kp = qkv_b + (size_t)(j0 + bl) * ld + d + hd * 64 + hh * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf[ks] = __builtin_bit_cast(bf16x8, *(const u32x4*)(kp + ks * 16));
            vf[ks] = __builtin_bit_cast(bf16x8, *(const u32x4*)(kp + d + ks * 16));
            e[0][ks] = e_frag(0, ks);                       // the wave's first step (t = wk) is its diagonal: hi chunk 0
            e[1][ks] = e[0][ks];
        }
        if (padbits) {
            const uint32_t pwv = padbits[(size_t)b * nchunk + (j0 >> 5)];
            padlane = (pwv >> bl) & 1u;
            // any padded key in this workgroup's 128 keys?  (no __syncthreads_or: it allocates static LDS)
            if (tid == 0) *(volatile uint32_t*)(smem + OFF_FLAG) = 0u;
            __syncthreads();
            if (pwv) *(volatile uint32_t*)(smem + OFF_FLAG) = 1u;
            __syncthreads();
            wgpad = __builtin_amdgcn_readfirstlane(*(volatile uint32_t*)(smem + OFF_FLAG));
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // tile 0 has landed (a DMA has no register the compiler could wait on)
    __syncthreads();
    char* band = smem + OFF_BAND + w * PATCH_BYTES;          // the epilogue's store patch
    // rd[r] = byte address (source lane * 4) of the ds_bpermute that skews register r (see `tile`)
    uint32_t rd[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rd[r] = (uint32_t)((hh * 32 + ((crow(r, hh) - bl) & 31)) << 2);
    f32x16 dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
    // Every dS tile goes to the workspace as the operand registers this wave multiplies with q (bf16, the dK
    // product's own rounding): tile (b,h, I = query tile, J = key tile <= I) is 2 KB at ((bh*T + I(I+1)/2 + J)*1024 elements,
    // T = nchunk(nchunk+1)/2 (causal half); inside a tile unit (ss, lane) = 16 bytes at ss*512 + lane*8 elements holds
    // dS[i = crow(8ss+k, hh)][j = lane&31], k = 0..7 -- one wave store instruction writes 1 KB contiguously.  The dQ kernel
    // (dq_lite) and the dE kernel read these tiles instead of recomputing S / P / dP.
    // (wave-uniform base: tile (b,h, I = 0, J = j0/32); a wave beyond the end of the sequence rewrites the last key block's
    // tiles with identical data)
    char* ds_col = nullptr;
    if (EXPORT_DS) {
        const size_t ntri = (size_t)nchunk * (nchunk + 1) / 2;
        ds_col = (char*)(dst + (((size_t)b * heads + hd) * ntri + (size_t)(j0 >> 5)) * 1024) + lane16;
    }
    auto ds_tile = [&](int t) {                           // query tile I = J0/32 + t
        const size_t I = (size_t)(J0 >> 5) + t;
        return ds_col + (I * (I + 1) / 2) * 2048;
    };

    // ---- one query tile.  cur = t & 1 (LDS buffers), PAR = E slot of the hi chunk; MASKED: diagonal / padded-key masks ----
#ifdef MGX_DKV_STAMP
    unsigned long long st_acc[6] = {0, 0, 0, 0, 0, 0}, st_last = 0;
    unsigned st_steps = 0;
    const unsigned long long st_t0 = __builtin_amdgcn_s_memtime(), st_r0 = __builtin_amdgcn_s_memrealtime();   // realtime: constant 100 MHz
#endif
    auto tile = [&](int dq, int cur, auto par_tag, auto masked_tag, char* dsp, int tnext) {
        constexpr int PAR = decltype(par_tag)::value;
        constexpr bool MASKED = decltype(masked_tag)::value;
        DKV_STAMP(5);                                     // [5] from the previous stamp (after the barrier) to here: prefetch issue
        const char* qr = smem + OFF_QR + cur * TILE_BYTES;
        bf16x8 qa[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qa[ks] = frag_R(qr, bl, hh, ks);
        // Q.Er^T for chunks dq ("hi": keys bl <= query, t = a - bl) and dq-1 ("lo": keys bl > query, t = 32 + a - bl); rows =
        // query a, columns = t.  A tile reads column (a - bl) & 31 of row a and needs the hi chunk there for t <= a and the lo
        // chunk for t > a: the two products are MERGED in registers (one v_cndmask per element) and stored once -- 16 band
        // stores per tile instead of 32, a 4 KB band per wave instead of an 8 KB ring, and no parity in any address (this
        // kernel computes both chunks for every tile anyway: unlike the forward / dQ kernels nothing is reused by the next tile).
        const char* st = smem + OFF_ST + cur * ST_BYTES + w * 256;
        f32x16 nl;                                        // -lse2 of the accumulator's query rows
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 l4 = (MGX_DKV_PEEL & 32) ? f32x4{-9.f, -9.f, -9.f, -9.f} : *(const f32x4*)(st + (8 * g4 + 4 * hh) * 4);
            nl[4 * g4] = l4.x; nl[4 * g4 + 1] = l4.y; nl[4 * g4 + 2] = l4.z; nl[4 * g4 + 3] = l4.w;
        }
        f32x16 qe = zero16();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qe = mfma(qa[ks], e[PAR][ks], qe);
        if (!MASKED || dq >= 1) {
            f32x16 ql = zero16();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) ql = mfma(qa[ks], e[PAR ^ 1][ks], ql);
#pragma unroll
            for (int r = 0; r < 16; ++r) qe[r] = (bl <= crow(r, hh)) ? qe[r] : ql[r];
        }
        // the lo slot is free now: fetch the next step's hi chunk into it
        if (!(MGX_DKV_PEEL & 1)) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) e[PAR ^ 1][ks] = e_frag(dq + 1, ks);
        }
        // ... and request the next query tile into the other LDS buffers (every wave is past the barrier that ended their last
        // use).  AFTER the E loads: the compiler's wait for those at the top of the next step counts the operations it knows to
        // be younger (the two dS stores) and so also covers these three -- which have landed by then anyway (see `landed`)
        stage(tnext, cur ^ 1);
        if (!MASKED) __builtin_amdgcn_sched_barrier(0x78F);    // VMEM may not sink below: needed at the top of the next step
        DKV_STAMP(0);                                     // [0] q fragments, 8 Q.Er^T MFMAs, merge
        // The skew is a LANE permutation inside each half-wave: the tile's element (row a = crow(r,hh), key bl) is the merged value
        // merged[a][t = (a - bl) & 31], which lane t of the same half holds in the SAME register r -- one ds_bpermute_b32 per
        // register and no LDS memory (until round 3 the merged tile went through a 4 KB band: 16 stores + 16 loads per tile).
        f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = qe[r];            // (a __builtin_bit_cast of the vector ELEMENT expression itself reads element 0)
            c[r] = (MGX_DKV_PEEL & 4) ? v : __int_as_float(__builtin_amdgcn_ds_bpermute((int)rd[r], __float_as_int(v)));
        }
        DKV_STAMP(1);                                     // [1] 16 ds_bpermute and their results
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) c = mfma(qa[ks], kf[ks], c);
        if (MASKED) {
            if (dq == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) c[r] = (bl > crow(r, hh)) ? -INFINITY : c[r];
            }
            if (padlane) {
#pragma unroll
                for (int r = 0; r < 16; ++r) c[r] = -INFINITY;
            }
        }
        f32x16 dp;                                        // initial accumulator: -delta of the accumulator's query rows
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 d4 = (MGX_DKV_PEEL & 32) ? f32x4{0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(st + 128 + (8 * g4 + 4 * hh) * 4);
            dp[4 * g4] = d4.x; dp[4 * g4 + 1] = d4.y; dp[4 * g4 + 2] = d4.z; dp[4 * g4 + 3] = d4.w;
        }
        const char* orr = smem + OFF_OR + cur * TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) dp = mfma(frag_R(orr, bl, hh, ks), vf[ks], dp);
        f32x16 ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // c = 8 S: q is staged unscaled, 1/8 (exact) rides in this multiplier and in the final scale of dK
            const float p = (MGX_DKV_PEEL & 8) ? c[r] * 1e-9f : __builtin_amdgcn_exp2f(__builtin_fmaf(c[r], 0.125f * LOG2E, nl[r]));
            c[r] = p;
            ds[r] = p * dp[r];
        }
        DKV_STAMP(2);                                     // [2] S, dP MFMAs, statistics, exponentials, dS
        u32x4 dfx[2];
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const bf16x8 pf = acc_to_frag(c, ss);
            const bf16x8 df = acc_to_frag(ds, ss);
            dv0 = mfma(frag_T_onR(orr, lane, ss, 0), pf, dv0);
            dv1 = mfma(frag_T_onR(orr, lane, ss, 1), pf, dv1);
            dk0 = mfma(frag_T_onR(qr, lane, ss, 0), df, dk0);
            dk1 = mfma(frag_T_onR(qr, lane, ss, 1), df, dk1);
            dfx[ss] = __builtin_bit_cast(u32x4, df);
        }
        // streamed (read back from HBM by two later kernels): costs this kernel 55-100 us of its 600 at cfg2 (tools/peel_dkv.sh);
        // issuing them before the dV / dK products instead of after changes nothing
        if (EXPORT_DS && !(MGX_DKV_PEEL & 2)) {           // == DS_STORES below (`landed`)
            __builtin_nontemporal_store(dfx[0], (u32x4*)dsp);
            __builtin_nontemporal_store(dfx[1], (u32x4*)(dsp + 1024));
        }
        DKV_STAMP(3);                                     // [3] packs, transposed fragments, 8 dV / dK MFMAs (issue), dS stores
    };
    // The next query tile's DMA (issued inside `tile`, after the E loads) must have landed before the barrier that ends the
    // step; the only VMEM operations a wave issues after it are the two dS stores of its tile: a COUNTED wait, vmcnt(2).
    // (the count follows the condition under which the stores are compiled: a peel build without them must wait for vmcnt(0))
    constexpr bool DS_STORES = EXPORT_DS && !(MGX_DKV_PEEL & 2);
    auto landed = [&]() {
        if (DS_STORES) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    // ---- general body: the diagonal 128 x 128 block (t < 4: a wave is not started / on its diagonal / full), every
    //      step when a key of this workgroup is padded, and an odd last step ------------------------------------------------
    auto general_step = [&](int t) {
        const int dq = t - wk;
        if (dq >= 0) {
            tile(dq, t & 1, std::integral_constant<int, 0>{}, std::true_type{}, ds_tile(t), t + 1);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) { const bf16x8 x = e[0][ks]; e[0][ks] = e[1][ks]; e[1][ks] = x; }
            landed();                                     // counted, as in the main loop: the two dS stores may stay in flight
        } else {
            stage(t + 1, (t & 1) ^ 1);                    // (a wave that has a tile stages from inside it)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a wave that skipped its tile issued nothing after the DMA
        }
        __syncthreads();
    };
    // (round 4: the four steps of the diagonal block specialised at compile time -- the wave's first tile through the masked body,
    //  later ones through the main loop's branch-free body with its E-slot protocol, instead of the general body below -- made the
    //  kernel SLOWER, 1.31 against 1.265 ms at cfg2 / batch 64: eight more inlined tile bodies, 68 spilled registers outside the main
    //  loop and a 15 K-instruction kernel.  The general body costs 4.2-5.0 K cycles per step against 3.1 K in the main loop,
    //  15 % of a workgroup's time: tools/dkv_stamp.py.)
    int t = 0;
    const int nhead = wgpad ? nT : min(WAVES, nT);        // (WAVES is even: the main loop starts on an even step)
#ifdef MGX_DKV_STAMP
    const unsigned long long st_t1 = __builtin_amdgcn_s_memtime();      // end of the prologue
#endif
    for (; t < nhead; ++t) general_step(t);
#ifdef MGX_DKV_STAMP
    const unsigned long long st_t2 = __builtin_amdgcn_s_memtime();      // end of the diagonal block's general steps
#endif
    // ---- main loop (t >= 4 is even here): every wave's tile is full, no masks: branch-free bodies, two steps per trip so
    //      that the LDS buffer and the E slot of each step are compile-time constants -----------------------------------------
    for (; t + 1 < nT; t += 2) {
        tile(t - wk, 0, std::integral_constant<int, 0>{}, std::false_type{}, ds_tile(t), t + 1);
        landed();
        __syncthreads();
#ifdef MGX_DKV_STAMP
        { constexpr bool MASKED = false; DKV_STAMP(4); st_steps += 2; }     // [4] publish + barrier
#endif
        tile(t + 1 - wk, 1, std::integral_constant<int, 1>{}, std::false_type{}, ds_tile(t + 1), t + 2);
        landed();
        __syncthreads();
#ifdef MGX_DKV_STAMP
        { constexpr bool MASKED = false; DKV_STAMP(4); }
#endif
    }
#ifdef MGX_DKV_STAMP
    const unsigned long long st_t3 = __builtin_amdgcn_s_memtime();      // end of the main loop
#endif
    for (; t < nT; ++t) general_step(t);

    if (wave_on) {
        uint16_t* row0 = dqkv + ((size_t)b * L + j0) * ld + hd * 64;
        store_rows_lds(row0 + d, ld, dk0, dk1, lane, 0.125f, band);      // dk = dS^T (q/8)
        store_rows_lds(row0 + 2 * d, ld, dv0, dv1, lane, 1.f, band);
#ifdef MGX_DKV_STAMP
        if (lane == 0) {
            float* rec = (float*)(row0 + d);
            for (int i = 0; i < 6; ++i) rec[i] = (float)st_acc[i];
            rec[6] = (float)st_steps; rec[7] = (float)(J0 >> 7); rec[8] = (float)w;
            rec[9] = (float)(__builtin_amdgcn_s_memtime() - st_t0); rec[10] = (float)(__builtin_amdgcn_s_memrealtime() - st_r0);
            rec[11] = (float)(st_t1 - st_t0); rec[12] = (float)(st_t2 - st_t1); rec[13] = (float)(st_t3 - st_t2);
        }
#endif
    }
}

void relattn::dkv32_launch(const uint16_t* qkv, const void* EfA, const uint32_t* padbits, const uint16_t* dctx, const float* nlse2,
                           const float* ndelta, uint16_t* dqkv, uint16_t* dst, dim3 grid, int L, int d, int bg, void* stream) {
    static const hipError_t once = hipFuncSetAttribute((const void*)rel_attn_dkv_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, k2::LDS_BYTES);
    (void)once;                                            // function-local static: set exactly once, thread-safe
    hipLaunchKernelGGL(rel_attn_dkv_kernel<true>, grid, dim3(64 * k2::WAVES), k2::LDS_BYTES, (hipStream_t)stream, qkv,
                       (const u32x4*)EfA, padbits, dctx, nlse2, ndelta, dqkv, dst, L, d, bg);
}

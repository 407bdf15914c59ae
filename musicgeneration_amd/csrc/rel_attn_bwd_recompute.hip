// K1 and K3 of the attention backward (overview and math: rel_attn_bwd.hip): dQ and dE by full recomputation of P and dS.
// NOTHING IN TRAINING CALLS THESE TWO KERNELS.  They are the round-2 kernels, independent of the stored dS tiles, kept as
// cross-checks of dq_lite and de_tiles (parts bits 32 and 16 of mgx_rel_attn_bwd_parts: the tests and tools/attn_bench.py).
#include <type_traits>
#include "rel_attn_common.hpp"

using namespace relattn;

#ifndef MGX_DKV_PEEL
#define MGX_DKV_PEEL 0      // rel_attn_dkv32.hip; bit 32 (statistics as constants) also applies to the dE kernel here
#endif

// K1: dQ by recomputation (cross-check of K1L; parts bit 5).  Same sweep as the forward (query-block owner, key tiles
//   0..diagonal).
//   orientation: keys on registers, queries on lanes (S^T, P^T, dP^T, dS^T), dqs^T[c][a] accumulators.
//   E never touches LDS here: the Er row fragments (B operand of Q.Er^T) and the fragments of the
//   transposed copy ErT[c][delta] (A operand of dqs^T += ErT . dQE^T) are loaded from global/L2.
//   K has ONE LDS image (R) that serves both the row reads (S^T) and the transposed reads (dq).
namespace k1 {
constexpr int WAVES = 4;
constexpr int OFF_KR = 0;                                  // 2 x 4K  K image R (row + transposed reads)
constexpr int OFF_VR = OFF_KR + 2 * TILE_BYTES;            // 2 x 4K  V image R (row frags for dP^T)
constexpr int OFF_BAND = OFF_VR + 2 * TILE_BYTES;          // 4 x 8,704 B fp32 rotated band (see common.hpp)
constexpr int DB_STRIDE = 144;                             // bytes per dband row (64 bf16 + pad)
constexpr int OFF_DBAND = OFF_BAND + WAVES * BAND_BYTES;   // 4 x 4,608 B bf16 [32][72]: dS by (query, delta&63)
constexpr int OFF_PAD = OFF_DBAND + WAVES * 32 * DB_STRIDE; // key-padding words of this batch row (first 256)
constexpr int OFF_FLAG = OFF_PAD + 1024;                   // "this batch row has padded keys" flag
constexpr int LDS_BYTES = OFF_FLAG + 16;                   // 70,672 B -> 2 workgroups per CU
}  // namespace k1

__global__ __launch_bounds__(256, 2) void rel_attn_dq_kernel(
    const uint16_t* __restrict__ qkv, const u32x4* __restrict__ EfA, const u32x4* __restrict__ EfT,
    const uint32_t* __restrict__ padbits, const uint16_t* __restrict__ dctx, const float* __restrict__ lse,
    const float* __restrict__ delta, uint16_t* __restrict__ dqkv, int L, int d, int bgroup) {
    using namespace k1;
    extern __shared__ __attribute__((aligned(256))) char smem[];     // 256: the band stores XOR bit 7 of absolute LDS addresses
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int a = lane & 31, hh = lane >> 5;
    const int heads = d >> 6;
    // x = (b,h) of one batch group [fast], y = (batch group, heaviness rank) [slow]: one group's tensors (~100 MB) stay
    // inside the Infinity Cache while its workgroups run (see rel_attn_fwd.hip)
    const int nqb = (L + 127) >> 7;
    const int b = (blockIdx.y / nqb) * bgroup + blockIdx.x / heads, hd = blockIdx.x % heads;
    const int qb = nqb - 1 - (blockIdx.y % nqb);
    const int I0 = qb * 128, Q0 = I0 >> 5;
    const int nchunk = L >> 5;
    const bool wave_on = I0 + w * 32 < L;
    // a wave beyond the end of the sequence (L % 128 != 0) shadows the last valid 32-row block: it recomputes that
    // block's values (its duplicate stores of delta / dS carry identical data) and skips the dq store
    const int q0 = wave_on ? Q0 + w : nchunk - 1;
    const int i0 = q0 * 32;
    const int ntw = min(Q0 + 4, nchunk);                 // key tiles this workgroup visits
    const size_t ld = (size_t)3 * d;
    const uint16_t* qkv_b = qkv + (size_t)b * L * ld;

    const int srow = tid >> 3, sch = tid & 7;
    const int st_offR = imgR_off(srow, sch);
    // Every global address of the sweep is (wave-uniform base in SGPRs) + (32-bit per-lane offset) + immediate, so a load
    // costs no vector address arithmetic (a 64-bit per-lane pointer bumped per step cost 2-3 VALU + SALU per load).
    const char* kv_base = (const char*)(qkv_b + d + hd * 64);                 // K columns of this head; V is d elements further
    const uint32_t kv_voff = (uint32_t)((srow * ld + sch * 8) * 2);            // bytes
    const uint32_t tile_bytes = (uint32_t)(32 * ld * 2);                       // one 32-row step of qkv
    auto k_tile = [&](int t) { return *(const u32x4*)(kv_base + (size_t)t * tile_bytes + kv_voff); };
    auto v_tile = [&](int t) { return *(const u32x4*)(kv_base + (size_t)t * tile_bytes + (size_t)d * 2 + kv_voff); };
    // fragment-ordered copies of Er (er_frag_kernel, rel_attn_common.hpp): 1 KB contiguous per wave load.  Every load
    // of the sweep is unconditional with a clamped index (a load inside a branch makes the compiler drain the whole
    // VMEM queue where the branch rejoins); data of clamped tiles / chunks is never used.
    const uint32_t lane16 = (uint32_t)lane * 16u;
    // Er row fragment ks of chunk q (row t = lane&31 of the chunk, i.e. delta = 32q + t)
    auto e_frag = [&](int q, int ks) {
        return __builtin_bit_cast(bf16x8, *(const u32x4*)((const char*)EfA + (size_t)max(q, 0) * 4096 + ks * 1024 + lane16));
    };
    // ErT fragment: row c = 32*ct + (lane&31), k = t = 16*ks + 8*hh + j of chunk q
    auto et_frag = [&](int q, int ks, int ct) {
        return __builtin_bit_cast(bf16x8, *(const u32x4*)((const char*)EfT + (size_t)max(q, 0) * 4096 + (2 * ks + ct) * 1024 + lane16));
    };

    {   // prologue staging
        *(u32x4*)(smem + OFF_KR + st_offR) = k_tile(0);
        *(u32x4*)(smem + OFF_VR + st_offR) = v_tile(0);
        // zero the dS band (its never-written half must read as 0 on the first step)
        for (int o = tid * 16; o < WAVES * 32 * DB_STRIDE; o += 256 * 16) *(u32x4*)(smem + OFF_DBAND + o) = u32x4{0, 0, 0, 0};
    }
    int anypad = 0;
    if (padbits) {
        if (tid == 0) *(volatile uint32_t*)(smem + OFF_FLAG) = 0u;
        __syncthreads();
        uint32_t acc = 0;
#pragma unroll 1
        for (int t = tid; t < ntw; t += 256) {
            const uint32_t pwv = padbits[(size_t)b * nchunk + t];
            if (t < 256) *(uint32_t*)(smem + OFF_PAD + 4 * t) = pwv;
            acc |= pwv;
        }
        if (acc) *(volatile uint32_t*)(smem + OFF_FLAG) = 1u;
        __syncthreads();
        anypad = __builtin_amdgcn_readfirstlane(*(volatile uint32_t*)(smem + OFF_FLAG));
    }
    auto padword = [&](int kt) -> uint32_t {             // wave-uniform
        if (!anypad) return 0u;
        uint32_t v = *(const uint32_t*)(smem + OFF_PAD + 4 * min(kt, 255));
        if (kt >= 256) v = padbits[(size_t)b * nchunk + kt];
        return __builtin_amdgcn_readfirstlane(v);
    };
    bf16x8 qf[4], dof[4], e[4];
    float lse2 = 0.f, dlt = 0.f;
    {
        const uint16_t* qp = qkv_b + (size_t)(i0 + a) * ld + hd * 64 + hh * 8;
        const uint16_t* dp = dctx + ((size_t)b * L + i0 + a) * d + hd * 64 + hh * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = __builtin_bit_cast(bf16x8, scale8(*(const u32x4*)(qp + ks * 16), 0.125f));
            dof[ks] = __builtin_bit_cast(bf16x8, *(const u32x4*)(dp + ks * 16));
            e[ks] = e_frag(q0, ks);                        // the wave's first "hi" chunk
        }
        const size_t si = ((size_t)b * heads + hd) * L + i0 + a;
        lse2 = lse[si] * LOG2E;
        dlt = delta[si];
    }
    __syncthreads();

    // band addressing (rotated band, rows placed so that the register index r is the row slot and the lane half hh
    // selects a 256-byte-aligned region).  wcl[r] = ABSOLUTE LDS address of (wave band + region + column byte offset): every
    // term but the column is a multiple of 256, so XOR-ing bit 7 of the whole value flips the chunk parity (one VALU per
    // store); the row slot r*272 is the instruction's immediate offset.
    const int band_base = OFF_BAND + w * BAND_BYTES;
    char* dband = smem + OFF_DBAND + w * (32 * DB_STRIDE);
    uint32_t wcl[16];
#pragma unroll
    for (int r = 0; r < 16; ++r)
        wcl[r] = lds_addr_of(smem) + band_base + hh * BAND_REGION + (((crow(r, hh) - a) & 63) << 2);
    const int rbase = band_base + band_rowoff(a) + 16 * hh;
    // PHYSICAL chunk parity = (chunk - q0) & 1: each wave has its own bands, so the assignment is free, and with it the
    // chunk stored in step s has parity (s + 1) & 1 and the tile read in step s parity s & 1 for EVERY wave -- compile-time
    // constants in the two-step main loop (with the chunk's own parity every band store paid a v_bitop3 and every dS store
    // a v_cndmask to select the address at run time).
    auto band_put = [&](const f32x16& v, int par) {      // a chunk of Q.Er^T -> band
        const uint32_t tog = (uint32_t)par << 7;
#pragma unroll
        for (int r = 0; r < 16; ++r) lds_store_f32((wcl[r] ^ tog) + r * BAND_STRIDE, v[r]);
    };
    auto band_get = [&](int par) {                       // Srel^T of a tile
        const char* rb = smem + rbase + (par << 7);
        f32x16 c;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 v = *(const f32x4*)(rb + 32 * g4);
            c[4 * g4] = v.x; c[4 * g4 + 1] = v.y; c[4 * g4 + 2] = v.z; c[4 * g4 + 3] = v.w;
        }
        return c;
    };
    // dband (unrotated, [a][delta&63] bf16): write offsets for D/32 even; odd flips column bit 5
    int dwa0[16], dwa1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        dwa0[r] = a * DB_STRIDE + (((a - crow(r, hh)) & 63) << 1);
        dwa1[r] = a * DB_STRIDE + (((a - crow(r, hh) + 32) & 63) << 1);
    }
    {      // first "hi" chunk -> band
        f32x16 qe = zero16();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qe = mfma(qf[ks], e[ks], qe);
        band_put(qe, 0);                                 // chunk q0: physical parity 0
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) e[ks] = e_frag(q0 - 1, ks);    // new chunk of step 0
    }
    f32x16 dq0 = zero16(), dq1 = zero16();
    const int am = a - 4 * hh;                           // key crow(r,hh) is in the future of query a  <=>  crow(r,0) > am

    // ---- one tile, from S^T (band term already in c) to the dq accumulators ---------------------------------------
    // MASKED: apply the diagonal / key-padding masks (general body only)
    auto tile_tail = [&](f32x16& c, int dq, int p, int cur, uint32_t pw, auto masked_tag, const bf16x8 (&et)[4]) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const char* kt = smem + OFF_KR + cur * TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) c = mfma(frag_R(kt, a, hh, ks), qf[ks], c);
        if (MASKED) {
            if (dq == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) c[r] = (crow(r, 0) > am) ? -INFINITY : c[r];
            }
            if (pw) {
                const uint32_t pwl = pw >> (4 * hh);
#pragma unroll
                for (int r = 0; r < 16; ++r) c[r] = (pwl & (1u << crow(r, 0))) ? -INFINITY : c[r];
            }
        }
        // P^T
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(c[r], LOG2E, -lse2));
        // dP^T = V dO^T
        f32x16 dp = zero16();
        const char* vt = smem + OFF_VR + cur * TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) dp = mfma(frag_R(vt, a, hh, ks), dof[ks], dp);
        // dS^T
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = c[r] * (dp[r] - dlt);
        // dqs^T += K^T dS^T
        bf16x8 df[2];
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            df[ss] = acc_to_frag(c, ss);
            dq0 = mfma(frag_T_onR(kt, lane, ss, 0), df[ss], dq0);
            dq1 = mfma(frag_T_onR(kt, lane, ss, 1), df[ss], dq1);
        }
        // un-skew dS into the (query, delta) band -- the bf16 pairs packed for the product above are stored as their low
        // and high halves (ds_write_b16 / ds_write_b16_d16_hi: no second conversion) --, then the completed chunk feeds dq_rel
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const u32x4 wv = __builtin_bit_cast(u32x4, df[ss]);               // word j: keys 8ss+2j (low), 8ss+2j+1 (high)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r0 = 8 * ss + 2 * j;
                *(uint16_t*)(dband + (p ? dwa1[r0] : dwa0[r0])) = (uint16_t)wv[j];
                *(uint16_t*)(dband + (p ? dwa1[r0 + 1] : dwa0[r0 + 1])) = (uint16_t)(wv[j] >> 16);
            }
        }
        wave_lds_fence();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 gq = *(const bf16x8*)(dband + a * DB_STRIDE + (p * 32 + 16 * ks + 8 * hh) * 2);
            dq0 = mfma(et[2 * ks], gq, dq0);
            dq1 = mfma(et[2 * ks + 1], gq, dq1);
        }
    };
    // ---- main loop: tiles strictly below every wave's diagonal, no padded keys: branch-free, two steps per trip so that the
    //      LDS buffers and the band parities of a step are compile-time constants (nmain = Q0 is a multiple of 4) -------------
    const int nmain = anypad ? 0 : Q0;                    // Q0 <= ntw - 1: a next tile always exists inside this loop
    auto main_step = [&](int s, auto par_tag) {
        constexpr int PAR = decltype(par_tag)::value;     // = s & 1: LDS buffer of tile s, physical parity of chunk dq
        const int tn = min(s + 1, ntw - 1);
        const u32x4 kreg = k_tile(tn);
        const u32x4 vreg = v_tile(tn);
        const int dq = q0 - s;                            // >= 1
        // fragments of ErT for chunk dq (used at the end of this step)
        bf16x8 et[4];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) { et[2 * ks] = et_frag(dq, ks, 0); et[2 * ks + 1] = et_frag(dq, ks, 1); }
        f32x16 c = zero16();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) c = mfma(qf[ks], e[ks], c);
        band_put(c, PAR ^ 1);                             // chunk dq-1
        wave_lds_fence();
        c = band_get(PAR);
        wave_lds_fence();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) e[ks] = e_frag(dq - 2, ks);      // Er chunk of the next step
        __builtin_amdgcn_sched_barrier(0x78F);             // VMEM may not sink below: the fragments are needed at the top of the next step
        tile_tail(c, dq, PAR, PAR, 0u, std::false_type{}, et);
        *(u32x4*)(smem + OFF_KR + (PAR ^ 1) * TILE_BYTES + st_offR) = kreg;
        *(u32x4*)(smem + OFF_VR + (PAR ^ 1) * TILE_BYTES + st_offR) = vreg;
        __syncthreads();
    };
    int s = 0;
    for (; s < nmain; s += 2) {
        main_step(s, std::integral_constant<int, 0>{});
        main_step(s + 1, std::integral_constant<int, 1>{});
    }

    // ---- general body: the diagonal 128 x 128 block (a wave is full / on its diagonal / done), padded keys ------------
    for (; s < ntw; ++s) {
        const int cur = s & 1;
        const int tn = min(s + 1, ntw - 1);
        const u32x4 kreg = k_tile(tn);
        const u32x4 vreg = v_tile(tn);
        const int dq = q0 - s;
        if (dq >= 0) {
            const uint32_t pw = padword(s);
            bf16x8 et[4];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) { et[2 * ks] = et_frag(dq, ks, 0); et[2 * ks + 1] = et_frag(dq, ks, 1); }
            if (dq >= 1) {
                f32x16 qe = zero16();
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) qe = mfma(qf[ks], e[ks], qe);
                band_put(qe, cur ^ 1);
            }
            wave_lds_fence();
            f32x16 c = band_get(cur);
            wave_lds_fence();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) e[ks] = e_frag(dq - 2, ks);
            tile_tail(c, dq, cur, cur, pw, std::true_type{}, et);
        }
        if (s + 1 < ntw) {
            *(u32x4*)(smem + OFF_KR + (cur ^ 1) * TILE_BYTES + st_offR) = kreg;
            *(u32x4*)(smem + OFF_VR + (cur ^ 1) * TILE_BYTES + st_offR) = vreg;
        }
        __syncthreads();
    }
    if (wave_on) store_rows_lds(dqkv + ((size_t)b * L + i0) * ld + hd * 64, ld, dq0, dq1, lane, 0.125f, smem + band_base);
}

// K3: dE.  workgroup = 8 consecutive chunks of 32 relative distances (wave = chunk c, Er chunk
// fragments + dEr[32][64] accumulators in registers).  For query tile i0 the band of chunk c
// covers the lower triangle (b<=a) of key tile u = i0/32 - c and the upper triangle (b>a) of key
// tile u-1: both tiles are computed and merged element-wise before exp/dS.
namespace k3 {
constexpr int W3 = 8;                                      // waves (= distance chunks) per workgroup
constexpr int KV_SLOTS = 10;                               // live key tiles [t-8, t] + the incoming one
constexpr int OFF_KR = 0;                                  // 10 x 4K K image R ring (slot = tile % 10)
constexpr int OFF_VR = OFF_KR + KV_SLOTS * TILE_BYTES;     // 10 x 4K V image R ring
constexpr int OFF_QR = OFF_VR + KV_SLOTS * TILE_BYTES;     // 2 x 4K qs image R
constexpr int OFF_QT = OFF_QR + 2 * TILE_BYTES;            // 2 x 4K qs image T
constexpr int OFF_OR = OFF_QT + 2 * TILE_BYTES;            // 2 x 4K dO image R
constexpr int OFF_ST = OFF_OR + 2 * TILE_BYTES;            // 2 x 256 B
constexpr int OFF_BAND = OFF_ST + 2 * 256;                 // 8 x 4K fp32 [32][32] (QE, then dS)
constexpr int LDS_BYTES = OFF_BAND + W3 * 4096;            // 139,776 B: one 8-wave workgroup per CU
}  // namespace k3

__global__ __launch_bounds__(512, 2) void rel_attn_de_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ Er, const uint32_t* __restrict__ padbits,
    const uint16_t* __restrict__ dctx, const float* __restrict__ lse, const float* __restrict__ delta,
    float* __restrict__ dEr /* = dE + (M-L)*64 */, int L, int d) {
    using namespace k3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bl = lane & 31, hh = lane >> 5;
    const int heads = d >> 6;
    const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
    const int nchunk = L >> 5;
    const int C0 = blockIdx.y * W3;                        // small C0 = longest sweep = dispatched first
    const int cw = C0 + w;
    const bool wave_on = cw < nchunk;
    const int nT = nchunk - C0;
    const size_t ld = (size_t)3 * d;
    const uint16_t* qkv_b = qkv + (size_t)b * L * ld;
    const size_t stat_base = ((size_t)b * heads + hd) * L;
    const uint32_t* pb = padbits ? padbits + (size_t)b * nchunk : nullptr;

    // staging roles: threads 0..255 stage the K and qs tiles, threads 256..511 the V and dO tiles
    const int half = tid >> 8;
    const int srow = (tid & 255) >> 3, sch = tid & 7;
    const int st_offR = imgR_off(srow, sch), st_offT = imgT_off(srow, sch);
    const uint16_t* kg = qkv_b + (size_t)srow * ld + d + half * d + hd * 64 + sch * 8;           // K or V, + u*32*ld
    const uint16_t* qg = qkv_b + (size_t)(32 * C0 + srow) * ld + hd * 64 + sch * 8;              // + t*32*ld
    const uint16_t* og = dctx + ((size_t)b * L + 32 * C0 + srow) * d + hd * 64 + sch * 8;        // + t*32*d
    auto stat_src = [&](int t) {
        const int i = 32 * (C0 + t) + (tid & 31);
        return (tid < 32) ? lse[stat_base + i] * LOG2E : delta[stat_base + i];
    };
    {
        *(u32x4*)(smem + (half ? OFF_VR : OFF_KR) + st_offR) = *(const u32x4*)kg;      // key tile 0 -> slot 0
        if (half == 0) {
            const u32x4 qq = scale8(*(const u32x4*)qg, 0.125f);
            *(u32x4*)(smem + OFF_QR + st_offR) = qq;
            *(u32x4*)(smem + OFF_QT + st_offT) = qq;
        } else {
            *(u32x4*)(smem + OFF_OR + st_offR) = *(const u32x4*)og;
        }
        if (tid < 64) *(float*)(smem + OFF_ST + tid * 4) = stat_src(0);
    }
    bf16x8 ef[4];
    if (wave_on) {
        const uint16_t* ep = Er + (size_t)(L - 1 - 32 * cw - bl) * 64 + hh * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) ef[ks] = __builtin_bit_cast(bf16x8, *(const u32x4*)(ep + ks * 16));
    }
    __syncthreads();
    char* band = smem + OFF_BAND + w * 4096;
    f32x16 de0 = zero16(), de1 = zero16();

    for (int t = 0; t < nT; ++t) {
        const int cur = t & 1;
        u32x4 kreg, qreg;      // K (or V) tile and qs (or dO) tile of the next step, by staging half
        float streg = 0.f;
        const bool have_next = (t + 1 < nT);
        if (have_next) {
            kreg = *(const u32x4*)(kg + (size_t)(t + 1) * 32 * ld);      // key tile t+1 <= nT-1 < nchunk
            qreg = half ? *(const u32x4*)(og + (size_t)(t + 1) * 32 * d) : *(const u32x4*)(qg + (size_t)(t + 1) * 32 * ld);
            if (tid < 64) streg = stat_src(t + 1);
        }
        const int u = t - w;                              // lower key tile; upper = u-1
        if (wave_on && u >= 0) {
            const char* qr = smem + OFF_QR + cur * TILE_BYTES;
            bf16x8 qa[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qa[ks] = frag_R(qr, bl, hh, ks);
            f32x16 qe = zero16();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qe = mfma(qa[ks], ef[ks], qe);
#pragma unroll
            for (int r = 0; r < 16; ++r) *(float*)(band + (crow(r, hh) * 32 + bl) * 4) = qe[r];
            wave_lds_fence();
            f32x16 srel;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ar = crow(r, hh);
                srel[r] = *(const float*)(band + (ar * 32 + ((ar - bl) & 31)) * 4);
            }
            const bool has_up = (u >= 1);
            const char* klo = smem + OFF_KR + (u % KV_SLOTS) * TILE_BYTES;
            const char* vlo = smem + OFF_VR + (u % KV_SLOTS) * TILE_BYTES;
            const char* kup = smem + OFF_KR + ((u + KV_SLOTS - 1) % KV_SLOTS) * TILE_BYTES;
            const char* vup = smem + OFF_VR + ((u + KV_SLOTS - 1) % KV_SLOTS) * TILE_BYTES;
            f32x16 slo = srel, sup = srel;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) slo = mfma(qa[ks], frag_R(klo, bl, hh, ks), slo);
            if (has_up) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) sup = mfma(qa[ks], frag_R(kup, bl, hh, ks), sup);
            }
            bool plo = false, pup = !has_up;              // "masked" flags of this lane's key in each tile
            if (pb) {
                plo = (pb[u] >> bl) & 1u;
                if (has_up) pup = (pb[u - 1] >> bl) & 1u;
            }
            const char* orr = smem + OFF_OR + cur * TILE_BYTES;
            bf16x8 oa[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) oa[ks] = frag_R(orr, bl, hh, ks);
            f32x16 dlo = zero16(), dup = zero16();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) dlo = mfma(oa[ks], frag_R(vlo, bl, hh, ks), dlo);
            if (has_up) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) dup = mfma(oa[ks], frag_R(vup, bl, hh, ks), dup);
            }
            const char* st = smem + OFF_ST + cur * 256;
            f32x16 ds;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 l4 = (MGX_DKV_PEEL & 32) ? f32x4{9.f, 9.f, 9.f, 9.f} : *(const f32x4*)(st + (8 * g4 + 4 * hh) * 4);
                const f32x4 d4 = (MGX_DKV_PEEL & 32) ? f32x4{0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(st + 128 + (8 * g4 + 4 * hh) * 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = 4 * g4 + k;
                    const bool lower = (bl <= crow(r, hh));
                    const bool masked = lower ? plo : pup;
                    const float sv = lower ? slo[r] : sup[r];
                    const float dv = lower ? dlo[r] : dup[r];
                    const float p = masked ? 0.f : __builtin_amdgcn_exp2f(__builtin_fmaf(sv, LOG2E, -l4[k]));
                    ds[r] = p * (dv - d4[k]);
                }
            }
            // un-skew: dQE[a][t] = dS[a][b] with t = (a-b)&31, through the same band buffer
            wave_lds_fence();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ar = crow(r, hh);
                *(float*)(band + (ar * 32 + ((ar - bl) & 31)) * 4) = ds[r];
            }
            wave_lds_fence();
            f32x16 x;
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = *(const float*)(band + (crow(r, hh) * 32 + bl) * 4);
            wave_lds_fence();
            const char* qt = smem + OFF_QT + cur * TILE_BYTES;
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 xf = acc_to_frag(x, ss);
                de0 = mfma(xf, frag_T(qt, lane, ss, 0), de0);
                de1 = mfma(xf, frag_T(qt, lane, ss, 1), de1);
            }
        }
        if (have_next) {
            *(u32x4*)(smem + (half ? OFF_VR : OFF_KR) + ((t + 1) % KV_SLOTS) * TILE_BYTES + st_offR) = kreg;
            if (half == 0) {
                const u32x4 qq = scale8(qreg, 0.125f);
                *(u32x4*)(smem + OFF_QR + (cur ^ 1) * TILE_BYTES + st_offR) = qq;
                *(u32x4*)(smem + OFF_QT + (cur ^ 1) * TILE_BYTES + st_offT) = qq;
            } else {
                *(u32x4*)(smem + OFF_OR + (cur ^ 1) * TILE_BYTES + st_offR) = qreg;
            }
            if (tid < 64) *(float*)(smem + OFF_ST + (cur ^ 1) * 256 + tid * 4) = streg;
        }
        __syncthreads();
    }
    // flush: dEr[delta = 32*cw + t][cc] += de[t][cc]; Er row index = L-1-delta.  One register of the
    // accumulator = two 128-byte row segments per wave instruction (full-rate atomic shape).
    if (wave_on) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dl = 32 * cw + crow(r, hh);
            float* row = dEr + (size_t)(L - 1 - dl) * 64;
            atomicAdd(row + bl, de0[r]);
            atomicAdd(row + 32 + bl, de1[r]);
        }
    }
}

void relattn::dq_recompute_launch(const uint16_t* qkv, const void* EfA, const void* EfT, const uint32_t* padbits, const uint16_t* dctx,
                                  const float* lse, const float* delta, uint16_t* dqkv, dim3 grid, int L, int d, int bg,
                                  void* stream) {
    static const hipError_t once = hipFuncSetAttribute((const void*)rel_attn_dq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k1::LDS_BYTES);
    (void)once;                                            // function-local static: set exactly once, thread-safe
    hipLaunchKernelGGL(rel_attn_dq_kernel, grid, dim3(64 * k1::WAVES), k1::LDS_BYTES, (hipStream_t)stream, qkv, (const u32x4*)EfA,
                       (const u32x4*)EfT, padbits, dctx, lse, delta, dqkv, L, d, bg);
}

void relattn::de_recompute_launch(const uint16_t* qkv, const uint16_t* Er, const uint32_t* padbits, const uint16_t* dctx,
                                  const float* lse, const float* delta, float* dEr, int B, int L, int d, void* stream) {
    static const hipError_t once = hipFuncSetAttribute((const void*)rel_attn_de_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k3::LDS_BYTES);
    (void)once;
    const dim3 grid(B * (d / 64), ((L >> 5) + k3::W3 - 1) / k3::W3);
    hipLaunchKernelGGL(rel_attn_de_kernel, grid, dim3(64 * k3::W3), k3::LDS_BYTES, (hipStream_t)stream, qkv, Er, padbits, dctx, lse,
                       delta, dEr, L, d);
}

// K1L of the attention backward (overview and math: rel_attn_bwd.hip): dQ from STORED dS.
// When dK/dV and dQ are both wanted, the dK/dV kernel runs first and leaves every dS tile in the workspace (bf16, its own
// operand registers); dq = dS (K + Er-band) / 8 then needs no S / Q.Er^T / exp / dP at all: 8 MFMA per 32x32 tile instead of
// 28, fed by a 2 KB tile load.  Same sweep and ownership as the recompute dQ kernel (rel_attn_bwd_recompute.hip: workgroup =
// 128 query rows, wave = 32 rows, key tiles 0..diagonal, K staged through LDS); HBM-bound (the causal half of dS, read once).
//   stored tile: lane (j = lane&31, hh) holds dS[i = crow(8ss+k,hh)][j]: queries on registers, keys on lanes.
//   * dqs^T[c][i] += K^T[c][j] dS^T[j][i]: the tile is parked row-major [j][i] in a wave-private image-T patch and read back
//     with transposing LDS reads as the B operand (k order kappa, matching frag_T of the K tile);
//   * the same registers are scattered into the (query, distance & 63) band exactly as the recompute kernel does; the
//     completed chunk is the B operand of dqs^T += ErT . dS_rel^T.
#include <type_traits>
#include "rel_attn_common.hpp"

using namespace relattn;

#ifndef MGX_DQL_PEEL
#define MGX_DQL_PEEL 0      // timing experiments only (tools/peel_dq_lite.sh): bits drop parts of the dq_lite step, results are then wrong
#endif                    // 1 dS^T patch stores | 2 three quarters of the band stores | 4 half of dS K | 8 half of dS_rel ErT | 16 K / ErT ring refills

namespace k1l {
constexpr int WAVES = 4;
constexpr int OFF_KT = 0;                                  // 2 x 4K  K image T (tile t in slot t & 1)
constexpr int OFF_ET = OFF_KT + 2 * TILE_BYTES;            // 8 x 4K  ErT chunk fragments, ring: chunk Q0 - k in slot k & 7
constexpr int XROW = 72;                                   // bytes per row of the dS^T patch: 32 queries + pad (lane-per-row writes and the
                                                           // transposing reads both hit distinct 8-byte bank groups)
constexpr int OFF_X = OFF_ET + 8 * 4096;                   // 4 x 2,304 B  dS^T tile [32 j][32 i]
constexpr int DB_STRIDE = 144;
constexpr int OFF_DBAND = OFF_X + WAVES * 32 * XROW;       // 4 x 4,608 B bf16 [32][72]: dS by (query, delta&63)
constexpr int LDS_BYTES = OFF_DBAND + WAVES * 32 * DB_STRIDE;   // 68,608 B -> 2 workgroups per CU
constexpr int DEPTH = 4;                                   // dS tiles in flight per wave (2 KB each)
}  // namespace k1l

__global__ __launch_bounds__(256, 2) void rel_attn_dq_lite_kernel(
    const uint16_t* __restrict__ qkv, const u32x4* __restrict__ EfT, const uint16_t* __restrict__ dst,
    uint16_t* __restrict__ dqkv, int L, int d, int bgroup) {
    using namespace k1l;
    extern __shared__ __attribute__((aligned(256))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int a = lane & 31, hh = lane >> 5;
    const int heads = d >> 6;
    // x = (b,h) of one batch group [fast], y = (batch group, heaviness rank) [slow]: one group's tensors (~100 MB) stay
    // inside the Infinity Cache while its workgroups run (see rel_attn_fwd.hip)
    const int nqb = (L + 127) >> 7;
    const int b = (blockIdx.y / nqb) * bgroup + blockIdx.x / heads, hd = blockIdx.x % heads;
    const int qb = nqb - 1 - (blockIdx.y % nqb);           // heaviest query blocks first
    const int I0 = qb * 128, Q0 = I0 >> 5;
    const int nchunk = L >> 5;
    const bool wave_on = I0 + w * 32 < L;
    const int q0 = wave_on ? Q0 + w : nchunk - 1;          // a wave beyond the end runs on clamped data and stores nothing
    const int i0 = q0 * 32;
    const int ntw = min(Q0 + 4, nchunk);
    const size_t ld = (size_t)3 * d;
    const uint16_t* qkv_b = qkv + (size_t)b * L * ld;

    // Per step the workgroup fetches ONE K tile and ONE ErT chunk (4 KB each, 16 bytes per thread) for its four waves -- wave w
    // multiplies with chunk Q0 + w - s, i.e. the chunk wave 0 used w steps earlier -- and each wave its own 2 KB dS tile.  Item k
    // (K tile k / chunk Q0 - k) is requested at the end of step k - 3, parked in registers for two steps, written to LDS at the
    // end of step k - 1 and read from step k on.
    const int srow = tid >> 3, sch = tid & 7;
    // K is only ever read transposed here (A operand of dq^T += K^T dS^T): image T, whose ds_read_b64_tr_b16 are conflict-free.
    // (Rounds 1-3 staged image R, the layout the recompute dQ kernel shares with its row reads: 2-way conflicts on the transposed
    // reads, 27 M of this kernel's 151 M LDS cycles at cfg2 / batch 64, r03_pmc_attn_b64.json.  The A/B switch is retired.)
    const int st_offT = imgT_off(srow, sch);
    const char* k_base = (const char*)(qkv_b + d + hd * 64);
    const uint32_t k_voff = (uint32_t)((srow * ld + sch * 8) * 2);
    const uint32_t tile_bytes = (uint32_t)(32 * ld * 2);
    auto k_tile = [&](int t) { return *(const u32x4*)(k_base + (size_t)min(t, ntw - 1) * tile_bytes + k_voff); };
    const uint32_t tid16 = (uint32_t)tid * 16u, lane16 = (uint32_t)lane * 16u;
    auto e_item = [&](int k) {                             // this thread's 16 bytes of chunk Q0 - k (fragment-ordered copy of ErT)
        return *(const u32x4*)((const char*)EfT + (size_t)min(max(Q0 - k, 0), nchunk - 1) * 4096 + tid16);
    };
    const size_t ntri = (size_t)nchunk * (nchunk + 1) / 2;
    const size_t row_tiles = ((size_t)b * heads + hd) * ntri + (size_t)q0 * (q0 + 1) / 2;      // tile (b,h, I = q0, 0)
    const char* ds_row = (const char*)(dst + row_tiles * 1024);
    // read once: streamed past L2 (K / ErT stay); index clamped to the wave's diagonal, clamped tiles are never used
    auto ds_load = [&](int J, int ss) {
        return __builtin_nontemporal_load((const u32x4*)(ds_row + (size_t)min(J, q0) * 2048 + ss * 1024 + lane16));
    };

    u32x4 dsr[DEPTH][2];
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) { dsr[j][0] = ds_load(j, 0); dsr[j][1] = ds_load(j, 1); }
    *(u32x4*)(smem + OFF_KT + st_offT) = k_tile(0);
#pragma unroll
    for (int k = -3; k <= 0; ++k) *(u32x4*)(smem + OFF_ET + (k & 7) * 4096 + tid16) = e_item(k);
    u32x4 kq[2] = {k_tile(1), k_tile(2)}, eq[2] = {e_item(1), e_item(2)};
    for (int o = tid * 16; o < WAVES * 32 * DB_STRIDE; o += 256 * 16) *(u32x4*)(smem + OFF_DBAND + o) = u32x4{0, 0, 0, 0};
    __syncthreads();

    char* xt = smem + OFF_X + w * (32 * XROW);
    char* dband = smem + OFF_DBAND + w * (32 * DB_STRIDE);
    const int xw0 = a * XROW + 8 * hh;                    // + 16 * (2ss + jq): the 8-byte piece (ss, jq) of this lane's row
    const int xi = lane & 15, xg = lane >> 4;
    const int xr0 = ((xi >> 2) + 4 * hh) * XROW + 32 * (xg & 1) + 8 * (xi & 3);     // transposing read, + (16s + 8jq) * XROW
    int dwa0[16], dwa1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        dwa0[r] = crow(r, hh) * DB_STRIDE + (((crow(r, hh) - a) & 63) << 1);
        dwa1[r] = crow(r, hh) * DB_STRIDE + (((crow(r, hh) - a + 32) & 63) << 1);
    }
    f32x16 dq0 = zero16(), dq1 = zero16();

    // dS^T patch -> B operand (k order kappa): X[16s + 8jq + 4hh + rq][lane&31]
    auto frag_X = [&](int s) {
        bf16x8 out;
#pragma unroll
        for (int jq = 0; jq < 2; ++jq) {
            const bf16x4 t4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(xt + xr0 + (16 * s + 8 * jq) * XROW));
            out[4 * jq + 0] = t4[0]; out[4 * jq + 1] = t4[1]; out[4 * jq + 2] = t4[2]; out[4 * jq + 3] = t4[3];
        }
        return out;
    };
    auto compute = [&](int p, const char* kt, const char* ec, const u32x4 (&t)[2]) {
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            if (!(MGX_DQL_PEEL & 1)) {
                *(u32x2*)(xt + xw0 + 16 * (2 * ss)) = u32x2{t[ss].x, t[ss].y};
                *(u32x2*)(xt + xw0 + 16 * (2 * ss + 1)) = u32x2{t[ss].z, t[ss].w};
            }
#pragma unroll
            for (int j = 0; j < ((MGX_DQL_PEEL & 2) ? 1 : 4); ++j) {
                const int r0 = 8 * ss + 2 * j;
                *(uint16_t*)(dband + (p ? dwa1[r0] : dwa0[r0])) = (uint16_t)t[ss][j];
                *(uint16_t*)(dband + (p ? dwa1[r0 + 1] : dwa0[r0 + 1])) = (uint16_t)(t[ss][j] >> 16);
            }
        }
        wave_lds_fence();
#pragma unroll
        for (int ss = 0; ss < ((MGX_DQL_PEEL & 4) ? 1 : 2); ++ss) {
            const bf16x8 df = frag_X(ss);
            dq0 = mfma(frag_T(kt, lane, ss, 0), df, dq0);
            dq1 = mfma(frag_T(kt, lane, ss, 1), df, dq1);
        }
#pragma unroll
        for (int ks = 0; ks < ((MGX_DQL_PEEL & 8) ? 1 : 2); ++ks) {
            const bf16x8 gq = *(const bf16x8*)(dband + a * DB_STRIDE + (p * 32 + 16 * ks + 8 * hh) * 2);
            dq0 = mfma(*(const bf16x8*)(ec + (2 * ks) * 1024 + lane16), gq, dq0);
            dq1 = mfma(*(const bf16x8*)(ec + (2 * ks + 1) * 1024 + lane16), gq, dq1);
        }
        wave_lds_fence();                                  // the patch and the band half are rewritten by the next step
    };
    // one step: SLOT = s & 3 (registers of the dS tile), PAR = s & 1 (K slot, physical parity of the completed chunk)
    auto step = [&](int s, auto slot_tag, bool active) {
        constexpr int SLOT = decltype(slot_tag)::value, PAR = SLOT & 1;
        const u32x4 t[2] = {dsr[SLOT][0], dsr[SLOT][1]};
        dsr[SLOT][0] = ds_load(s + DEPTH, 0);
        dsr[SLOT][1] = ds_load(s + DEPTH, 1);
        if (active) compute(PAR, smem + OFF_KT + PAR * TILE_BYTES, smem + OFF_ET + ((s - w) & 7) * 4096, t);
        // items s+1 (requested two steps ago): the K slot was last read in step s-1, the chunk slot in step s-4
        if (!(MGX_DQL_PEEL & 16)) {
            *(u32x4*)(smem + OFF_KT + (PAR ^ 1) * TILE_BYTES + st_offT) = kq[PAR];
            *(u32x4*)(smem + OFF_ET + ((s + 1) & 7) * 4096 + tid16) = eq[PAR];
            // the freed registers take items s+3 (no register rotation: a move of a register with a load in flight is a wait)
            kq[PAR] = k_tile(s + 3);
            eq[PAR] = e_item(s + 3);
        }
        __syncthreads();
    };
    using S0_ = std::integral_constant<int, 0>; using S1_ = std::integral_constant<int, 1>;
    using S2_ = std::integral_constant<int, 2>; using S3_ = std::integral_constant<int, 3>;
    static_assert(DEPTH == 4, "the loops below are unrolled by DEPTH");
    // entered with loads in flight the loop gets an s_waitcnt vmcnt(0) at its top (the compiler merges the unknown entry state
    // into every trip): drain once here, the loop then keeps its own four steps of requests outstanding
    __builtin_amdgcn_s_waitcnt(0x0F70);
    int s = 0;
    for (; s < Q0; s += 4) {                               // tiles strictly below every wave's diagonal (Q0 is a multiple of 4)
        step(s, S0_{}, true);
        step(s + 1, S1_{}, true);
        step(s + 2, S2_{}, true);
        step(s + 3, S3_{}, true);
    }
    // the diagonal 128 x 128 block (s = Q0 here): a wave is full / on its diagonal / done
    step(s, S0_{}, q0 - s >= 0);
    if (s + 1 < ntw) step(s + 1, S1_{}, q0 - s - 1 >= 0);
    if (s + 2 < ntw) step(s + 2, S2_{}, q0 - s - 2 >= 0);
    if (s + 3 < ntw) step(s + 3, S3_{}, q0 - s - 3 >= 0);
    if (wave_on) store_rows_lds(dqkv + ((size_t)b * L + i0) * ld + hd * 64, ld, dq0, dq1, lane, 0.125f, dband);
}

void relattn::dq_lite_launch(const uint16_t* qkv, const void* EfT, const uint16_t* dst, uint16_t* dqkv, dim3 grid, int L, int d,
                             int bg, void* stream) {
    static const hipError_t once = hipFuncSetAttribute((const void*)rel_attn_dq_lite_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k1l::LDS_BYTES);
    (void)once;                                            // function-local static: set exactly once, thread-safe
    hipLaunchKernelGGL(rel_attn_dq_lite_kernel, grid, dim3(64 * k1l::WAVES), k1l::LDS_BYTES, (hipStream_t)stream, qkv,
                       (const u32x4*)EfT, dst, dqkv, L, d, bg);
}

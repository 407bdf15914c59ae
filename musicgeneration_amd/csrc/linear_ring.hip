// The 256 x 256 "ring" GEMM kernels that linear.hip picks for the big projections of an encoder block -- LDS-DMA staging into a ring of
// stages, persistent workgroups -- in two generations: eight waves with 128 x 64 wave tiles written in HIP (linear_ring_kernel,
// linear_dw_ring_kernel) and, round 5, four waves with 128 x 128 wave tiles whose main loops are generated gfx950 assembly owning all
// 256 accumulators of a wave (linear_ring4_kernel, linear_dw_ring4_kernel; gen_gemm_asm.py).  All produce forward / dX results
// bit-identical to the 128 x 128 kernels' (linear_tile128.hip).  Diagnostic builds (tools/README.md): MGX_RING_PEEL, MGX_RING_STAMP,
// MGX_DW4_TIMES, MGX_GEMM_DIAG.  All families keep the epilogue contract of mgx.h (bias and ReLU in fp32 before the one rounding, a NaN
// stays a NaN; dX: round, mask, add, round): tests/test_gpu_gemm_kernels.py.
#include "linear_common.hpp"

using namespace relattn;

// Dynamic LDS: `smem` is declared at 16-byte alignment (no kernel here has static LDS: the block starts at offset 0).  The 1024 the
// declarations used to ask for never took effect -- the symbol was shared with the 128 x 128 kernels, whose 16 the compiler met
// first -- and asking for it in earnest changes the integer code around the generated statements: 16 keeps the code that was measured.

// =================================================================================================
// Ring kernel: C[M,NO] = A[M,R] . B^T  for the big projections (forward: B = W [NO,R]; dX: B = W [R,NO], BTRANS).
//   * 256 x 256 output tile per workgroup, 8 waves (2 x 4), wave tile 128 x 64 (8 accumulator tiles): half the operand
//     bytes per flop of the 128 x 128 kernels above.  Measured on the QKV projection (M = 65,536): those kernels spend
//     108 of their 145 us just moving 1.6 GB of operand tiles from L2 into LDS.
//   * operands go global -> LDS by DMA (global_load_lds_dwordx4: 1 KB per wave instruction, no VGPR staging, no ds_write).
//     The LDS destination of a DMA instruction is linear in the lane, so the bank swizzle of an image is applied on the
//     SOURCE side: lane l of piece p fetches the 16 bytes that belong in slot 64 p + l.
//   * reduction steps of 32, a ring of 4 stages (A 256 rows x 64 B + B 16 KB = 32 KB each): the request for step g+4 is
//     made when step g's stage is released and is waited for three steps later with a COUNTED s_waitcnt (never 0 in the
//     steady state) -- with two 64-wide stages the request had one step to land and the waves waited 1,400 cycles per step.
//   * persistent workgroups (one per CU) walk their tiles as ONE stream of reduction steps: the DMA ring runs across tile
//     boundaries, so a tile's epilogue overlaps the next tile's first requests.
//   * inside a step every MFMA is followed by one fragment read of the NEXT block or one DMA piece (a wave issues in
//     order: a group of reads or DMA issues ahead of the MFMAs holds them back for ~100-300 cycles per block).
//   LDS: 4 x 32 KB stages + 8 x 4 KB epilogue patches = 160 KB.
// =================================================================================================
typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef const __attribute__((address_space(1))) void* glb_void_ptr;
MGX_DEV void glds16(const void* g, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((glb_void_ptr)g, (lds_void_ptr)lds_wave_base, 16, 0, 0);
}
MGX_DEV void glds4(const void* g, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((glb_void_ptr)g, (lds_void_ptr)lds_wave_base, 4, 0, 0);
}
template <int N> MGX_DEV void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

constexpr int RG_STAGE = 32768, RG_NST = 4, RG_PATCH = 4096;
constexpr int RG_LDS = RG_NST * RG_STAGE + 8 * RG_PATCH;
// image H (64-byte rows): 16-byte chunk c of row r at r*64 + ((c ^ ((r >> 2) & 3)) << 4): conflict-free ds_read_b128 of
// (row = lane & 31, chunk = 2 ks + hh), and one DMA wave instruction = 16 whole rows.
MGX_DEV int imgH_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// Epilogue of one wave: the C^T accumulators (n on registers, m on lanes) of its 128 (m) x 64 (n) block -> row-major bf16
// through a 4 KB swizzled patch (32 rows x 128 B, 16-byte chunk c of row r at chunk c ^ (r & 7)): every global store
// instruction writes 8 full 128-byte row segments.  bias / ReLU on the accumulator side; ReLU-backward mask and residual
// addend on the row-major side (coalesced loads).  The block lies inside the matrix: 16 unconditional stores.
// ReLU on the fp32 side, before the conversion (relu_f32, mgx_common.hpp: one v_maximum3_f32 per element, NaN stays NaN).  Until
// round 15 it was a 16-bit integer maximum on the packed bf16 pair, half an instruction per element -- which kept a NaN with a clear
// sign bit and turned one with the sign bit set into 0, where the 128 x 128 kernels' fmaxf turned both into 0.
MGX_DEV uint32_t pack_relu_bf16x2(float lo, float hi) { return pack_bf16x2(relu_f32(lo), relu_f32(hi)); }
// FWD: bias / ReLU (forward projection); !FWD: ReLU-backward mask / residual addend (dX).  The variants a kernel cannot take are
// compiled out and `act` selects between two straight-line bodies: the epilogue used to be ~1,500 instructions per wave (per-element
// v_max + v_cndmask on the runtime `act`, both operand paths) -- 5.5 K cycles per tile with the MFMA pipe idle, 17 % of a K = 512
// tile and 30 % of a K = 256 one (tools/ring_stamp.py)
template <bool FWD, int PRE = 0>     // PRE (dX only): 0 plain, 1 ReLU-backward mask, 2 residual addend -- straight-line variants: across a
                                     // runtime branch hipcc's wait for the prefetched rows becomes vmcnt(0) again
MGX_DEV void store_wave_block(uint16_t* __restrict__ C, const uint16_t* __restrict__ relu_y,
                              const uint16_t* __restrict__ addend, f32x16 (&acc)[4][2], bool bias, int act, int mb,
                              int nb, int N, int lane, char* patch) {
    const int l31 = lane & 31, hh = lane >> 5;
    const int rr = lane >> 3, ch = lane & 7;
    // bias: the wave's 64 values were put into its patch by DMA a tile ago (a vector load here would be waited for with
    // the whole DMA ring ahead of it in the in-order VMEM queue); added in place before the patch is reused
    if (FWD && bias) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 b = *(const f32x4*)(patch + (32 * ct + 8 * g4 + 4 * hh) * 4);
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) {
                    acc[rt][ct][4 * g4 + 0] += b.x; acc[rt][ct][4 * g4 + 1] += b.y;
                    acc[rt][ct][4 * g4 + 2] += b.z; acc[rt][ct][4 * g4 + 3] += b.w;
                }
            }
        wave_lds_fence();
    }
    char* wr = patch + l31 * 128 + 8 * hh;
    const int sw = l31 & 7;
    auto park = [&](int rt, auto relu_tag) {                 // 32 rows of the block -> the patch, row-major
        constexpr bool RELU = decltype(relu_tag)::value;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x16& a = acc[rt][ct];
                const uint32_t p0 = RELU ? pack_relu_bf16x2(a[4 * g4 + 0], a[4 * g4 + 1]) : pack_bf16x2(a[4 * g4 + 0], a[4 * g4 + 1]);
                const uint32_t p1 = RELU ? pack_relu_bf16x2(a[4 * g4 + 2], a[4 * g4 + 3]) : pack_bf16x2(a[4 * g4 + 2], a[4 * g4 + 3]);
                *(u32x2*)(wr + (((4 * ct + g4) ^ sw) << 4)) = u32x2{p0, p1};
            }
    };
    const bool relu = FWD && act == 1;
    uint16_t* crow = C + (size_t)(mb + rr) * N + nb + ch * 8;
    if constexpr (!FWD && PRE != 0) {
        // dX with a mask / addend.  Loaded where they are used, the rows of a 32-row slice were waited for with vmcnt(0) -- behind the
        // previous slice's four stores, a full store round trip per slice: 19-32 K cycles per tile instead of 4 K (tools/ring_stamp.py),
        // +27 % on the dX of QKV, +80 % on the dX of FFN_pre.  Now all sixteen rows of the tile are requested at once, after the
        // accumulators have been packed to bf16 (64 registers instead of 128: what makes room for 64 registers of rows in flight),
        // and waited for once: 11-17 K cycles.  What is left is bandwidth, not latency: every workgroup reaches its epilogue at the
        // same time, and 32 MB of rows in + 32 MB of tile out per round of tiles is ~12 us of HBM on its own (with the operand
        // these K <= 512 GEMMs sit at 1.4-1.5 x their HBM floors).  (The host sends a call with BOTH operands to the 128 x 128
        // kernel; the training step never makes one.)
        const uint16_t* prow = (PRE == 2 ? addend : relu_y) + (size_t)(mb + rr) * N + nb + ch * 8;
        u32x4 pre[4][4];
        u32x2 pk[4][8];
        auto fetch = [&](int rt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) pre[rt][i] = *(const u32x4*)(prow + (size_t)(32 * rt + 8 * i) * N);
        };
        __builtin_amdgcn_sched_barrier(0);
        fetch(0); fetch(1);                                  // (hipcc moves these below the packing whatever is put between them)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    pk[rt][4 * ct + g4] = u32x2{pack_bf16x2(acc[rt][ct][4 * g4 + 0], acc[rt][ct][4 * g4 + 1]),
                                                pack_bf16x2(acc[rt][ct][4 * g4 + 2], acc[rt][ct][4 * g4 + 3])};
        __builtin_amdgcn_sched_barrier(0);
        fetch(2); fetch(3);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8) *(u32x2*)(wr + ((c8 ^ sw) << 4)) = pk[rt][c8];
            wave_lds_fence();
            u32x4 o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rr + 8 * i;
                o[i] = *(const u32x4*)(patch + row * 128 + ((ch ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float f[8], a[8];
                unpack8(o[i], f);
                unpack8(pre[rt][i], a);
                if (PRE == 1) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) f[k] = (a[k] > 0.f) ? f[k] : 0.f;
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) f[k] += a[k];
                }
                o[i] = pack8(f);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *(u32x4*)(crow + (size_t)(32 * rt + 8 * i) * N) = o[i];
            wave_lds_fence();
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            if (relu) park(rt, std::true_type{}); else park(rt, std::false_type{});
            wave_lds_fence();
            u32x4 o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rr + 8 * i;
                o[i] = *(const u32x4*)(patch + row * 128 + ((ch ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *(u32x4*)(crow + (size_t)(32 * rt + 8 * i) * N) = o[i];
            wave_lds_fence();
        }
    }
}

#define MGX_SB() __builtin_amdgcn_sched_barrier(0)
#ifndef MGX_RING_PEEL
// diagnostic builds only (results are garbage): 1 no barrier in the loop, 2 no DMA in the loop, 4 no fragment reads.  Round 4, per step of
// cfg2's forward GEMMs at batch 64 (tools/ab_gemm.sh): product 2.71 ms; no barrier 2.70; no DMA 2.31; no fragment reads 2.33; neither
// 1.83; all three 1.64 (= the MFMAs, the epilogue and the loop: 1.25 PF).  The barrier is free; the DMA pieces and the fragment reads
// cost 15 % each and add up -- the waves' in-order issue behind the LDS pipe, not its bandwidth (12 reads + 4 pieces per wave and step)
#define MGX_RING_PEEL 0
#endif
template <bool BTRANS>
__global__ __launch_bounds__(512, 1) void linear_ring_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                            const float* __restrict__ bias,
                                                            const uint16_t* __restrict__ relu_y,
                                                            const uint16_t* __restrict__ addend,
                                                            uint16_t* __restrict__ C, int M, int NO, int R, int act) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 2, wn = w & 3;
    const int l31 = lane & 31, hh = lane >> 5;
    const int ntn = (NO + 255) / 256, ntm = (M + 255) / 256, ntiles = ntm * ntn;
    const int nh = R / 32;                                   // reduction steps per tile
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int G = my_tiles * nh;                             // steps of this workgroup, over all its tiles
    char* patch = smem + RG_NST * RG_STAGE + w * RG_PATCH;
    if (G <= 0) return;
    auto tile_origin = [&](int i, int& m0, int& n0) {        // i-th tile of this workgroup
        const int t = min(xcd_remap((int)blockIdx.x + i * (int)gridDim.x, ntiles), ntiles - 1);   // (a request past the last tile re-reads it)
        m0 = (t / ntn) * 256; n0 = (t % ntn) * 256;
    };

    // ---- DMA stream: wave w stages pieces 2w, 2w+1 of the A image and of the B image of every step ----
    //  A piece p: rows 16p .. 16p+15 of the tile (64 bytes each).
    //  B piece p, !BTRANS: the same for the rows of B;  BTRANS: the step's B tile is [32 r][256 n] = 4 sub-tiles [32][64]
    //  (image T, 128-byte rows): piece p = rows 8 (p & 3) .. +7 of sub-tile p >> 2.
    const uint16_t* ap[2];
    const uint16_t* bp[2];
    int d_i = -1, d_h = 0, d_st = 0, d_k0 = 0;
    char* d_at = nullptr;
    auto dma_begin = [&]() {                                 // addresses of the next request
        if (d_h == 0) {
            ++d_i;
            int m0, n0;
            tile_origin(d_i, m0, n0);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int p = 2 * w + j;
                const int row = 16 * p + (lane >> 2);
                ap[j] = A + (size_t)min(m0 + row, M - 1) * R + ((lane & 3) ^ ((row >> 2) & 3)) * 8;
                if (!BTRANS) {
                    bp[j] = B + (size_t)min(n0 + row, NO - 1) * R + ((lane & 3) ^ ((row >> 2) & 3)) * 8;
                } else {
                    const int r = 8 * (p & 3) + (lane >> 3);
                    const int chunk = (lane & 7) ^ (((r >> 1) & 1) << 2);
                    bp[j] = B + (size_t)r * NO + min(n0 + 64 * (p >> 2) + chunk * 8, NO - 8);
                }
            }
        }
        d_at = smem + d_st * RG_STAGE + (2 * w) * 1024;
        d_k0 = d_h * 32;
        d_h = (d_h + 1 == nh) ? 0 : d_h + 1;
        d_st = (d_st + 1) & 3;
    };
    auto b_src = [&](int j) { return BTRANS ? bp[j] + (size_t)d_k0 * NO : bp[j] + d_k0; };
    auto dma_all = [&]() {
        dma_begin();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            glds16(ap[j] + d_k0, d_at + j * 1024);
            glds16(b_src(j), d_at + 16384 + j * 1024);
        }
    };
    bf16x8 fa[2][4], fb[2][2];
    auto rd_a = [&](int stg, int ks, int i) {
        return *(const bf16x8*)(smem + stg * RG_STAGE + imgH_off(128 * wm + 32 * i + l31, 2 * ks + hh));
    };
    auto rd_b = [&](int stg, int ks, int i) {      // !BTRANS
        return *(const bf16x8*)(smem + stg * RG_STAGE + 16384 + imgH_off(64 * wn + 32 * i + l31, 2 * ks + hh));
    };
    // BTRANS: the B fragments are transposed reads (ds_read_b64_tr_b16 x 2) of sub-tile wn of the step's [32 r][256 n] tile.
    // Through the builtin the compiler puts s_waitcnt vmcnt(0) in front of every such read while a DMA is in flight (it
    // cannot tell the read from the DMA's LDS destination), which drains the ring twice per block: the reads are issued
    // from inline asm instead.  The compiler does not count them, so (a) every block ends with an explicit
    // s_waitcnt lgkmcnt(0) -- before any control flow, where register copies could be placed -- and (b) the two 64-bit halves
    // are only joined into an operand after that wait.  tb[ct]: the lane's byte address of fragTn(sub-tile wn, ks = 0,
    // column half ct) in stage 0 (see fragTn: row = 16 ks + 8 hh + 4 jq + rq; ks and jq are the immediate offset).
    uint32_t tb[2] = {0u, 0u};
    u32x2 hb[2][2][2];                                        // [set][ct][jq]
    if (BTRANS) {
        const int i15 = lane & 15, gq = lane >> 4, rq = i15 >> 2;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int chunk = 4 * ct + 2 * (gq & 1) + ((i15 & 3) >> 1);
            tb[ct] = lds_addr_of(smem) + 16384 + wn * TILE_BYTES + (8 * hh + rq) * 128 +
                     ((chunk ^ (((rq >> 1) & 1) << 2)) << 4) + 8 * (i15 & 1);
        }
    }
    auto rd_bt = [&](int stg, auto ks_tag, int ct, u32x2 (&h)[2]) {
        constexpr int KS = decltype(ks_tag)::value;
        const uint32_t addr = tb[ct] + stg * RG_STAGE;
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(h[0]) : "v"(addr), "n"(2048 * KS));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(h[1]) : "v"(addr), "n"(2048 * KS + 512));
    };
    auto join = [&](const u32x2 (&h)[2]) { return __builtin_bit_cast(bf16x8, u32x4{h[0].x, h[0].y, h[1].x, h[1].y}); };
    // one block: the 8 MFMAs of fragment set `cur`; each gap carries one fragment read of the NEXT block (into set cur ^ 1)
    // or one DMA piece
    auto block = [&](f32x16 (&acc)[4][2], auto cur_tag, int nstg, auto nks_tag, const uint16_t* g0, char* l0, const uint16_t* g1, char* l1, auto first_tag) {
        constexpr int CUR = decltype(cur_tag)::value, NXT = CUR ^ 1, NKS = decltype(nks_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value;   // a tile's first block: C = 0 (an inline constant) instead of 128 v_mov per tile
        const bf16x8(&a)[4] = fa[CUR];
        bf16x8(&na)[4] = fa[NXT];
        bf16x8 b[2];
        if (BTRANS) { b[0] = join(hb[CUR][0]); b[1] = join(hb[CUR][1]); }
        else { b[0] = fb[CUR][0]; b[1] = fb[CUR][1]; }
        MGX_SB();
        // reads in the first three gaps (two per gap), DMA pieces in gaps 3 and 5: by the end of the block the reads have had
        // five MFMAs to return
        // (round 4: which gaps carry the pieces -- 1/3, 3/5, 5/7 -- makes no difference, and neither did spreading the eight waves'
        //  pieces over all eight gaps, which only cost the scalar branches)
#define MGX_GAP(i) do { MGX_SB(); if (!(MGX_RING_PEEL & 2) && (i) == 3) glds16(g0, l0); if (!(MGX_RING_PEEL & 2) && (i) == 5) glds16(g1, l1); MGX_SB(); } while (0)
        acc[0][0] = mfma(b[0], a[0], FIRST ? zero16() : acc[0][0]); MGX_SB();
        if (!(MGX_RING_PEEL & 4)) {
            na[0] = rd_a(nstg, NKS, 0);
            if (BTRANS) rd_bt(nstg, nks_tag, 0, hb[NXT][0]); else fb[NXT][0] = rd_b(nstg, NKS, 0);
        }
        MGX_GAP(0);
        acc[0][1] = mfma(b[1], a[0], FIRST ? zero16() : acc[0][1]); MGX_SB();
        if (!(MGX_RING_PEEL & 4)) {
            na[1] = rd_a(nstg, NKS, 1);
            if (BTRANS) rd_bt(nstg, nks_tag, 1, hb[NXT][1]); else fb[NXT][1] = rd_b(nstg, NKS, 1);
        }
        MGX_GAP(1);
        acc[1][0] = mfma(b[0], a[1], FIRST ? zero16() : acc[1][0]); MGX_SB();
        if (!(MGX_RING_PEEL & 4)) {
            na[2] = rd_a(nstg, NKS, 2);
            na[3] = rd_a(nstg, NKS, 3);
        }
        MGX_GAP(2);
        acc[1][1] = mfma(b[1], a[1], FIRST ? zero16() : acc[1][1]); MGX_GAP(3);
        acc[2][0] = mfma(b[0], a[2], FIRST ? zero16() : acc[2][0]); MGX_GAP(4);
        acc[2][1] = mfma(b[1], a[2], FIRST ? zero16() : acc[2][1]); MGX_GAP(5);
        acc[3][0] = mfma(b[0], a[3], FIRST ? zero16() : acc[3][0]); MGX_GAP(6);
        acc[3][1] = mfma(b[1], a[3], FIRST ? zero16() : acc[3][1]); MGX_GAP(7);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every LDS read of the block has returned (asm reads included)
        MGX_SB();
    };
    using T0 = std::integral_constant<int, 0>;
    using T1 = std::integral_constant<int, 1>;

    // bias of tile i -> the wave's patch (64 floats): one more entry in the in-order VMEM queue, issued when the patch is
    // free (right after the previous tile's epilogue); the counted waits below then leave at most one operation fewer
    // outstanding than they could, which is always safe
    auto dma_bias = [&](int i) {
        int m0, n0;
        tile_origin(i, m0, n0);
        glds4(bias + min(n0 + 64 * wn + lane, NO - 1), patch);
    };
    // prologue: requests 0..3 (a stream shorter than that simply waits for everything)
    if (bias) dma_bias(0);
    dma_all();
    if (G > 1) dma_all();
    if (G > 2) dma_all();
    if (G > 3) dma_all();
    if (G > 3) wait_vmcnt<12>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[0][i] = rd_a(0, 0, i);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (BTRANS) rd_bt(0, T0{}, i, hb[0][i]); else fb[0][i] = rd_b(0, 0, i);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    MGX_SB();
    int g = 0, since_epi = 2, cs = 0;
    // Every block issues its two pieces, with no scalar branch around them.  Block 1 of step 0 has no request begun for it: d_at /
    // b_src still describe the prologue's fourth, whose pieces are complete, and they are fetched once more into the same place.
    bool pend = false;                                       // (only ever true where it is tested: see step)
#ifdef MGX_RING_STAMP
    // diagnostic build only (tools/ring_stamp.py): s_memtime sums per phase, left by lane 0 of every wave in the first bytes of C
    unsigned long long st_acc[5] = {0, 0, 0, 0, 0}, st_last = __builtin_amdgcn_s_memtime();
    const unsigned long long st_t0 = st_last, st_r0 = __builtin_amdgcn_s_memrealtime();
#define RING_STAMP(i) do { MGX_SB(); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); MGX_SB(); st_acc[i] += t_ - st_last; st_last = t_; } while (0)
#else
#define RING_STAMP(i)
#endif
    // one reduction step of the stream (g counts them over all tiles of the workgroup)
    auto step = [&](f32x16 (&acc)[4][2], auto first_tag) {
        const int ns = (cs + 1) & 3;
        // block 1: multiply (stage cs, k 0..15); its gaps read (cs, k 16..31) and issue the B pieces of the request made at
        // the last barrier
        block(acc, T0{}, cs, T1{}, b_src(0), d_at + 16384, b_src(1), d_at + 16384 + 1024, first_tag);
        RING_STAMP(0);
        // (the block ended with lgkmcnt(0): this wave has read everything it needs from stage cs)
        // step g+1 has landed once at most the younger operations are outstanding: requests g+2 and g+3 (4 each) and,
        // for two steps after a tile's epilogue, its 16 stores
        if (g + 3 < G) { if (since_epi < 2) wait_vmcnt<24>(); else wait_vmcnt<8>(); }
        else wait_vmcnt<0>();
        RING_STAMP(1);
        if (!(MGX_RING_PEEL & 1)) __builtin_amdgcn_s_barrier();
        RING_STAMP(2);
        pend = true;                                         // (past the end of the stream the pieces re-read the last tile into a stage
        if (pend) dma_begin();                               //  nobody reads again, instead of four scalar branches per step.  The test
                                                             //  through a variable is kept: a bare call moves two scalar instructions)
        // block 2: multiply (cs, k 16..31); its gaps read (ns, k 0..15) and issue the A pieces of the new request
        block(acc, T1{}, ns, T0{}, ap[0] + d_k0, d_at, ap[1] + d_k0, d_at + 1024, std::false_type{});
        RING_STAMP(3);
        ++since_epi;
        ++g;
        cs = ns;
    };
    // The accumulators live inside the tile loop: after the epilogue has read them they are dead, and the compiler knows it (as
    // one flat loop over steps with a runtime "first step of a tile" test it kept all 128 alive across the epilogue).
    for (int ti = 0; ti < my_tiles; ++ti) {
        f32x16 acc[4][2];
        step(acc, std::true_type{});                         // the tile's first block multiplies with C = 0
        for (int h = 1; h < nh; ++h) step(acc, std::false_type{});
        int m0, n0;
        tile_origin(ti, m0, n0);
        // (the host only takes this kernel for M % 256 == 0 and NO % 256 == 0: every tile is whole, 16 unconditional
        //  stores per wave -- the count the waits above rely on)
        if (BTRANS && addend) store_wave_block<!BTRANS, 2>(C, relu_y, addend, acc, false, 0, m0 + 128 * wm, n0 + 64 * wn, NO, lane, patch);
        else if (BTRANS && relu_y) store_wave_block<!BTRANS, 1>(C, relu_y, addend, acc, false, 0, m0 + 128 * wm, n0 + 64 * wn, NO, lane, patch);
        else store_wave_block<!BTRANS, 0>(C, relu_y, addend, acc, bias != nullptr, act, m0 + 128 * wm, n0 + 64 * wn, NO, lane, patch);
        since_epi = 0;
        if (bias && ti + 1 < my_tiles) dma_bias(ti + 1);
        // the fragments block 2 has just prefetched for the next step are read AGAIN here instead of being kept across the
        // epilogue (48 registers the epilogue's prefetch of the mask / addend rows needs; ~150 cycles per tile)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[0][i] = rd_a(cs, 0, i);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (BTRANS) rd_bt(cs, T0{}, i, hb[0][i]); else fb[0][i] = rd_b(cs, 0, i);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RING_STAMP(4);
    }
    wait_vmcnt<0>();                    // the pieces requested past the end land before the workgroup's LDS is released
#ifdef MGX_RING_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
        float* rec = (float*)C + ((size_t)blockIdx.x * 8 + w) * 16;
        for (int i = 0; i < 5; ++i) rec[i] = (float)st_acc[i];
        rec[5] = (float)G; rec[6] = (float)my_tiles; rec[7] = (float)(__builtin_amdgcn_s_memtime() - st_t0);
        rec[8] = (float)(__builtin_amdgcn_s_memrealtime() - st_r0); rec[9] = (float)w;
    }
#endif
}

// =================================================================================================
// The same ring with FOUR waves, one per SIMD, each holding a 128 x 128 block of the tile = 16 accumulator tiles = all 256 AGPRs
// (round 5).  Per 16-column k-step a wave reads 8 operand fragments for 16 MFMAs instead of 6 for 8: two thirds of the LDS bytes per
// MFMA.  hipcc cannot keep 256 accumulators in place (rounds 3-4), so one TILE's stages are one generated asm statement that owns them
// (gen_gemm_asm.py: ring_tile -> linear_ring4_loop.inc); what stays HIP is the tile loop, the wave's parameter block in LDS (source
// pointers of this and the next tile, the ring's state between two statements) and the epilogue.  The DMA ring runs on across the
// statement's end: the first three stages of the next tile are in flight during the epilogue, whose 32 global stores per wave
// (MGX_RING4_EPI_STORES) the statement's first counted waits allow for.  Same images, same MFMA operand order as the eight-wave kernel:
// bit-identical results.  Stages of 64 reduction columns in two 64 KB slots, so that every DMA instruction fetches whole 128-byte lines
// (gen_gemm_asm.py).  LDS: 2 x 64 KB stages + 4 x 4 KB patches + 4 x 4 KB parameter blocks (bias at + 512) = 160 KB.
// =================================================================================================
#if defined(MGX_GEMM_DIAG) && MGX_GEMM_DIAG
#include "linear_ring4_loop_diag.inc"      // timing-only loops of a diagnostic build (gen_gemm_asm.py with MGX_RING4_DIAG / MGX_DW4_NO*)
#else
#include "linear_ring4_loop.inc"
#endif
#ifdef MGX_DW4_TIMES
extern __device__ unsigned long long mgx_dw4_times_buf[8 * 1024];
#endif
template <bool FWD, int PRE>
MGX_DEV void store_wave_block4(uint16_t* __restrict__ C, const uint16_t* __restrict__ relu_y, const uint16_t* __restrict__ addend,
                               f32x16 (&acc)[4][4], const char* bias_lds, int act, int mb, int nb, int N, int lane, char* patch) {
    const int l31 = lane & 31, hh = lane >> 5;
    const int rr = lane >> 3, ch = lane & 7;
    char* wr = patch + l31 * 128 + 8 * hh;
    const int sw = l31 & 7;
    const bool relu = FWD && act == 1;
#pragma unroll
    for (int half = 0; half < 2; ++half) {                   // 64 columns at a time: the patch holds 32 rows x 64 columns
        // byte offsets from the (uniform) matrix bases in 32 bits (host: the matrix is smaller than 4 GB): sixteen 64-bit row pointers
        // per operand cost 64 registers and spilled
        const uint32_t off0 = (uint32_t)(((size_t)(mb + rr) * N + nb + 64 * half + ch * 8) * 2), rowb = (uint32_t)N * 16u;   // 8 rows
        u32x4 pre[4][4];
        if constexpr (!FWD && PRE != 0) {
            // all sixteen rows of the half-block at once, waited for once (store_wave_block)
            const char* pbase = (const char*)(PRE == 2 ? addend : relu_y);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) pre[rt][i] = *(const u32x4*)(pbase + (off0 + (uint32_t)(4 * rt + i) * rowb));
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 b[2][4];                                       // bias of the lane's columns (parameter block + 512: the statement's DMA)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) b[ct][g4] = FWD ? *(const f32x4*)(bias_lds + (64 * half + 32 * ct + 8 * g4 + 4 * hh) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            // (packed one 32-row slice at a time: the accumulators stay where they are -- AGPRs -- until they are read here.  ReLU as a
            //  straight-line variant: on the runtime flag hipcc computed both and selected, 4 more instructions per 4 values)
            auto park = [&](auto relu_tag) {
                constexpr bool RELU = decltype(relu_tag)::value;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        const f32x16& a = acc[rt][2 * half + ct];
                        const float v0 = a[4 * g4 + 0] + b[ct][g4].x, v1 = a[4 * g4 + 1] + b[ct][g4].y;
                        const float v2 = a[4 * g4 + 2] + b[ct][g4].z, v3 = a[4 * g4 + 3] + b[ct][g4].w;
                        const uint32_t p0 = RELU ? pack_relu_bf16x2(v0, v1) : pack_bf16x2(v0, v1);
                        const uint32_t p1 = RELU ? pack_relu_bf16x2(v2, v3) : pack_bf16x2(v2, v3);
                        *(u32x2*)(wr + (((4 * ct + g4) ^ sw) << 4)) = u32x2{p0, p1};
                    }
            };
            if (relu) park(std::true_type{}); else park(std::false_type{});
            wave_lds_fence();
            u32x4 o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rr + 8 * i;
                o[i] = *(const u32x4*)(patch + row * 128 + ((ch ^ (row & 7)) << 4));
            }
            if constexpr (!FWD && PRE != 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float f[8], a[8];
                    unpack8(o[i], f);
                    unpack8(pre[rt][i], a);
                    if (PRE == 1) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) f[k] = (a[k] > 0.f) ? f[k] : 0.f;
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) f[k] += a[k];
                    }
                    o[i] = pack8(f);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *(u32x4*)((char*)C + (off0 + (uint32_t)(4 * rt + i) * rowb)) = o[i];
            wave_lds_fence();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <bool BTRANS, int PRE>      // PRE (dX): 0 plain, 1 ReLU-backward mask, 2 residual addend -- ONE epilogue per kernel: with the three behind
                                     // runtime branches hipcc moved accumulator tiles between AGPR tuples after the statement and spilled
__global__ __launch_bounds__(256, 1) void linear_ring4_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                             const float* __restrict__ bias, const uint16_t* __restrict__ relu_y,
                                                             const uint16_t* __restrict__ addend, uint16_t* __restrict__ C, int M, int NO,
                                                             int R, int act) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 1, wn = w & 1;
    const int l31 = lane & 31, hh = lane >> 5;
    const int ntn = NO / 256, ntm = M / 256, ntiles = ntm * ntn;           // whole tiles (host)
    const int nd = R / 64;                                   // 64-column stages per tile: even, >= 4 (host)
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    if (my_tiles <= 0) return;
    char* patch = smem + 2 * 65536 + w * RG_PATCH;
    char* pb = smem + 2 * 65536 + 4 * RG_PATCH + w * 4096;
    auto tile_origin = [&](int i, int& m0, int& n0) {        // i-th tile of this workgroup (past the last one: the last one again)
        const int t = min(xcd_remap((int)blockIdx.x + min(i, my_tiles - 1) * (int)gridDim.x, ntiles), ntiles - 1);
        m0 = (t / ntn) * 256; n0 = (t % ntn) * 256;
    };
    auto a_base = [&](int m0) { return (uint64_t)(uintptr_t)(A + (size_t)m0 * R); };
    auto b_base = [&](int n0) { return (uint64_t)(uintptr_t)(BTRANS ? B + n0 : B + (size_t)n0 * R); };
    // ---- the lane's table (layout: gen_gemm_asm.py, ring_tile): DMA source offsets of the wave's pieces 0 and 1, fragment addresses ----
    {
        uint32_t* lt = (uint32_t*)(pb + 1024) + lane;
        // image R (128-byte rows): piece p = rows 8 p .. 8 p + 7; the wave fetches pieces 8 w + j; physical chunk lane & 7 of row
        // r holds logical chunk (lane & 7) ^ ((r >> 1) & 7)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = 64 * w + 8 * j + (lane >> 3);
            const uint32_t offR = (uint32_t)(((size_t)row * R + ((lane & 7) ^ ((row >> 1) & 7)) * 8) * 2);
            lt[64 * j] = offR;
            if (!BTRANS) lt[64 * (2 + j)] = offR;
        }
        if (BTRANS) {                                        // image T: piece 0 of the wave = rows 0 .. 7 of 64-column sub-tile w
            const int r = lane >> 3;
            const int chunk = (lane & 7) ^ (((r >> 1) & 1) << 2);
            lt[64 * 2] = (uint32_t)(((size_t)r * NO + 64 * w + chunk * 8) * 2);
            lt[64 * 3] = 0u;
        }
        lt[64 * 4] = lds_addr_of(smem) + imgR_off(128 * wm + l31, hh);
        if (!BTRANS) { lt[64 * 5] = lds_addr_of(smem) + 32768 + imgR_off(128 * wn + l31, hh); lt[64 * 6] = 0u; }
        else {
            const int i15 = lane & 15, gq = lane >> 4, rq = i15 >> 2;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int chunk = 4 * ct + 2 * (gq & 1) + ((i15 & 3) >> 1);
                lt[64 * (5 + ct)] = lds_addr_of(smem) + 32768 + 2 * wn * TILE_BYTES + (8 * hh + rq) * 128 +
                                    ((chunk ^ (((rq >> 1) & 1) << 2)) << 4) + 8 * (i15 & 1);
            }
        }
    }
    if (!BTRANS) {                                           // no bias: the epilogue adds these zeros (the statement's bias DMA fetches nothing)
        float* bl = (float*)(pb + 512);
        bl[lane] = 0.f;
        bl[64 + lane] = 0.f;
    }
    const uint32_t pba = __builtin_amdgcn_readfirstlane(lds_addr_of(pb));
    for (int ti = 0; ti < my_tiles; ++ti) {
        int m0, n0, m1, n1;
        tile_origin(ti, m0, n0);
        tile_origin(ti + 1, m1, n1);
        if (lane == 0) {
            uint64_t* p64 = (uint64_t*)pb;
            uint32_t* p32 = (uint32_t*)pb;
            if (ti == 0) {
                p64[0] = a_base(m0); p64[1] = b_base(n0);
                p32[11] = p32[19] = (uint32_t)nd;            // requests of A / of B left in the tile that operand's pointer stands in
            }
            p64[2] = a_base(m1); p64[3] = b_base(n1);
            p32[8] = 128u;                                   // bytes per stage: 64 columns of A
            p32[9] = BTRANS ? (uint32_t)(64 * NO * 2) : 128u;
            p32[10] = (uint32_t)nd;
            p32[12] = lds_addr_of(smem);
            p32[13] = (uint32_t)w;
            p32[14] = ti == 0 ? 1u : 0u;
            p32[15] = (uint32_t)(8 * R * 2);                 // 8 rows of A
            p64[8] = (uint64_t)(uintptr_t)(bias ? bias + n0 + 128 * wn : nullptr);      // this tile's bias (0: none -- the zeros below stay)
            p32[18] = BTRANS ? (uint32_t)(8 * NO * 2) : (uint32_t)(8 * R * 2);      // 8 rows of B
        }
        f32x16 acc[4][4];
#ifdef MGX_DW4_TIMES
        const unsigned long long tq0 = __builtin_amdgcn_s_memtime();
#endif
#define MGX_RING4_OPERANDS                                                                                                                  \
    : "=a"(acc[0][0]), "=a"(acc[0][1]), "=a"(acc[0][2]), "=a"(acc[0][3]), "=a"(acc[1][0]), "=a"(acc[1][1]), "=a"(acc[1][2]),                \
      "=a"(acc[1][3]), "=a"(acc[2][0]), "=a"(acc[2][1]), "=a"(acc[2][2]), "=a"(acc[2][3]), "=a"(acc[3][0]), "=a"(acc[3][1]),                \
      "=a"(acc[3][2]), "=a"(acc[3][3])                                                                                                      \
    : "s"(pba)                                                                                                                              \
    : MGX_RING4_CLOBBERS
        if constexpr (BTRANS) asm volatile(MGX_RING4_NN_ASM MGX_RING4_OPERANDS);
        else asm volatile(MGX_RING4_NT_ASM MGX_RING4_OPERANDS);
#undef MGX_RING4_OPERANDS
#ifdef MGX_DW4_TIMES
        const unsigned long long tq1 = __builtin_amdgcn_s_memtime();
#endif
        store_wave_block4<!BTRANS, PRE>(C, relu_y, addend, acc, pb + 512, act, m0 + 128 * wm, n0 + 128 * wn, NO, lane, patch);
#ifdef MGX_DW4_TIMES
        if (tid == 0) {          // per workgroup: [0] statement cycles, [1] epilogue cycles (summed over its tiles), [2] tiles, [3] real time
            const unsigned long long tq2 = __builtin_amdgcn_s_memtime();
            unsigned long long* rec = mgx_dw4_times_buf + 8 * blockIdx.x;
            if (ti == 0) { rec[0] = rec[1] = rec[2] = 0; rec[3] = __builtin_amdgcn_s_memrealtime(); }
            rec[0] += tq1 - tq0; rec[1] += tq2 - tq1; rec[2] += 1;
            rec[4] = __builtin_amdgcn_s_memrealtime() - rec[3];
        }
#endif
    }
    wait_vmcnt<0>();                                         // the requests past the last tile land before the workgroup's LDS is released
}

// =================================================================================================
// Ring kernel for the weight gradients of one encoder block:  gW[N,K] += dY^T X  (TN), same structure as
// linear_ring_kernel (256 x 256 tile, 8 waves, 4-stage DMA ring, reduction steps of 32 rows m), one (tile, M-split) unit per
// workgroup.  Both operand tiles of a step are [32 m][256 cols] = 4 sub-tiles [32][64] (image T), and every fragment
// is a transposed read (ds_read_b64_tr_b16 x 2, issued from inline asm: see linear_ring_kernel).
// A unit leaves its 256 x 256 fp32 partial in the workspace with plain stores (row-major, through the wave's LDS patch);
// dw_fixup_kernel then adds the splits of a tile into gW.  (fp32 atomics run at ~1.3 TB/s chip-wide and stall the issuing
// waves: 63 MB of partials per block would cost ~48 us of every CU's time, plain stores + the fix-up pass ~20.)
// Bias gradient gb[n] += sum_m dY[m][n]: the waves of the first k-tile column with wn == 0 add up the dY fragments they
// hold anyway (v_dot2c_f32_bf16 against (1, 1)).
// =================================================================================================
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

__global__ __launch_bounds__(512, 1) void linear_dw_ring_kernel(const DwRing g, int M, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 2, wn = w & 3;
    const int l31 = lane & 31, hh = lane >> 5;
    // unit order: one XCD runs a contiguous range of (split, tile) pairs, split-major -- the tiles of one M-split read the
    // same rows of dY / X (tiles of one row / column of a weight share an operand tile), so they meet in that XCD's L2
    const int tiles_all = g.first_tile[g.n];
    const int u = xcd_remap(blockIdx.x, gridDim.x);
    const int sp = u / tiles_all, t = u - sp * tiles_all;
    const int unit = t * g.splits + sp;                      // position of the partial tile in the workspace
    int p = 0;
    while (p + 1 < g.n && t >= g.first_tile[p + 1]) ++p;
    const int N = g.N[p], K = g.K[p];
    const int ntk = K >> 8, tl = t - g.first_tile[p];
    const int n0 = (tl / ntk) << 8, k0 = (tl % ntk) << 8;
    const int total = M >> 5;
    const int s0 = sp * g.steps_per_split;
    const int G = min(total, s0 + g.steps_per_split) - s0;   // >= 1 (host)
    char* patch = smem + RG_NST * RG_STAGE + w * RG_PATCH;

    // ---- DMA stream: piece q = 2w + j of an operand image = rows 8 (q & 3) .. +7 of sub-tile q >> 2 ----
    const uint16_t* ap[2];
    const uint16_t* bp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = 2 * w + j;
        const int r = 8 * (q & 3) + (lane >> 3);
        const int chunk = (lane & 7) ^ (((r >> 1) & 1) << 2);
        ap[j] = g.dY[p] + (size_t)(s0 * 32 + r) * N + n0 + 64 * (q >> 2) + chunk * 8;
        bp[j] = g.X[p] + (size_t)(s0 * 32 + r) * K + k0 + 64 * (q >> 2) + chunk * 8;
    }
    int d_st = 0;
    char* d_at = nullptr;
    const uint16_t* da[2] = {nullptr, nullptr};
    const uint16_t* db[2] = {nullptr, nullptr};
    auto dma_begin = [&]() {                                 // addresses of the next request, pointers move one step on
        d_at = smem + d_st * RG_STAGE + (2 * w) * 1024;
        d_st = (d_st + 1) & 3;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            da[j] = ap[j]; db[j] = bp[j];
            ap[j] += (size_t)32 * N; bp[j] += (size_t)32 * K;
        }
    };
    auto dma_all = [&]() {
        dma_begin();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            glds16(da[j], d_at + j * 1024);
            glds16(db[j], d_at + 16384 + j * 1024);
        }
    };
    // ---- fragments: transposed reads; ta[ct] / tbb[ct] = the lane's address of fragTn(first sub-tile of the wave, ks = 0,
    //      column half ct) in stage 0; the immediate offset adds ks, jq and (for the A operand) the second sub-tile ----
    uint32_t ta[2], tbb[2];
    {
        const int i15 = lane & 15, gq = lane >> 4, rq = i15 >> 2;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int chunk = 4 * ct + 2 * (gq & 1) + ((i15 & 3) >> 1);
            const uint32_t in_tile = (8 * hh + rq) * 128 + ((chunk ^ (((rq >> 1) & 1) << 2)) << 4) + 8 * (i15 & 1);
            ta[ct] = lds_addr_of(smem) + 2 * wm * TILE_BYTES + in_tile;
            tbb[ct] = lds_addr_of(smem) + 16384 + wn * TILE_BYTES + in_tile;
        }
    }
    u32x2 ha[2][4][2], hb[2][2][2];                           // [set][fragment][jq]
    auto rd_at = [&](int stg, auto ks_tag, auto i_tag, u32x2 (&h)[2]) {
        constexpr int KS = decltype(ks_tag)::value, I = decltype(i_tag)::value;
        const uint32_t addr = ta[I & 1] + stg * RG_STAGE;
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(h[0]) : "v"(addr), "n"(2048 * KS + 4096 * (I >> 1)));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(h[1]) : "v"(addr), "n"(2048 * KS + 4096 * (I >> 1) + 512));
    };
    auto rd_bt = [&](int stg, auto ks_tag, int ct, u32x2 (&h)[2]) {
        constexpr int KS = decltype(ks_tag)::value;
        const uint32_t addr = tbb[ct] + stg * RG_STAGE;
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(h[0]) : "v"(addr), "n"(2048 * KS));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(h[1]) : "v"(addr), "n"(2048 * KS + 512));
    };
    auto join = [&](const u32x2 (&h)[2]) { return __builtin_bit_cast(bf16x8, u32x4{h[0].x, h[0].y, h[1].x, h[1].y}); };
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc[i][0] = zero16(); acc[i][1] = zero16(); }
    const bool do_bias = __builtin_amdgcn_readfirstlane((g.gb[p] != nullptr) && k0 == 0 && wn == 0);
    float gsum[4] = {0.f, 0.f, 0.f, 0.f};
    using T0 = std::integral_constant<int, 0>;
    using T1 = std::integral_constant<int, 1>;
    using T2 = std::integral_constant<int, 2>;
    using T3 = std::integral_constant<int, 3>;
    auto block = [&](auto cur_tag, int nstg, auto nks_tag, const uint16_t* g0, char* l0, const uint16_t* g1, char* l1, bool on) {
        constexpr int CUR = decltype(cur_tag)::value, NXT = CUR ^ 1;
        bf16x8 a[4], b[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = join(ha[CUR][i]);
        b[0] = join(hb[CUR][0]); b[1] = join(hb[CUR][1]);
        MGX_SB();
        acc[0][0] = mfma(b[0], a[0], acc[0][0]); MGX_SB();
        rd_at(nstg, nks_tag, T0{}, ha[NXT][0]);
        rd_bt(nstg, nks_tag, 0, hb[NXT][0]);
        MGX_SB();
        acc[0][1] = mfma(b[1], a[0], acc[0][1]); MGX_SB();
        rd_at(nstg, nks_tag, T1{}, ha[NXT][1]);
        rd_bt(nstg, nks_tag, 1, hb[NXT][1]);
        MGX_SB();
        acc[1][0] = mfma(b[0], a[1], acc[1][0]); MGX_SB();
        rd_at(nstg, nks_tag, T2{}, ha[NXT][2]);
        rd_at(nstg, nks_tag, T3{}, ha[NXT][3]);
        MGX_SB();
        acc[1][1] = mfma(b[1], a[1], acc[1][1]); MGX_SB();
        if (on) glds16(g0, l0);
        MGX_SB();
        acc[2][0] = mfma(b[0], a[2], acc[2][0]); MGX_SB();
        if (do_bias) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // (element pairs by shufflevector: indexing a u32x4 view of the fragment inside an unrolled loop made
                //  hipcc 7.2 feed the FIRST dword to all four dot products)
                const bf16x2_t one = {(__bf16)1.0f, (__bf16)1.0f};
                gsum[i] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a[i], a[i], 0, 1), one, gsum[i], false);
                gsum[i] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a[i], a[i], 2, 3), one, gsum[i], false);
                gsum[i] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a[i], a[i], 4, 5), one, gsum[i], false);
                gsum[i] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a[i], a[i], 6, 7), one, gsum[i], false);
            }
        }
        MGX_SB();
        acc[2][1] = mfma(b[1], a[2], acc[2][1]); MGX_SB();
        if (on) glds16(g1, l1);
        MGX_SB();
        acc[3][0] = mfma(b[0], a[3], acc[3][0]); MGX_SB();
        acc[3][1] = mfma(b[1], a[3], acc[3][1]); MGX_SB();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every transposed read of the block has returned
        MGX_SB();
    };

    dma_all();
    if (G > 1) dma_all();
    if (G > 2) dma_all();
    if (G > 3) dma_all();
    if (G > 3) wait_vmcnt<12>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    rd_at(0, T0{}, T0{}, ha[0][0]); rd_at(0, T0{}, T1{}, ha[0][1]); rd_at(0, T0{}, T2{}, ha[0][2]); rd_at(0, T0{}, T3{}, ha[0][3]);
    rd_bt(0, T0{}, 0, hb[0][0]); rd_bt(0, T0{}, 1, hb[0][1]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    MGX_SB();
    int cs = 0;
    bool pend = false;
    for (int s = 0; s < G; ++s) {
        const int ns = (cs + 1) & 3;
        block(T0{}, cs, T1{}, db[0], d_at + 16384, db[1], d_at + 16384 + 1024, pend);
        if (s + 3 < G) wait_vmcnt<8>(); else wait_vmcnt<0>();   // step s+1 has landed (requests s+2, s+3 may be outstanding)
        __builtin_amdgcn_s_barrier();
        pend = (s + 4 < G);
        if (pend) dma_begin();
        block(T1{}, ns, T0{}, da[0], d_at, da[1], d_at + 1024, pend);
        cs = ns;
    }

    // ---- epilogue: fp32 partial tile -> workspace, row-major [n][k], 128-byte row segments per 8 lanes ----
    float* wsu = ws + (size_t)unit * 65536;
    const int rr = lane >> 3, ch = lane & 7;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *(f32x4*)(patch + l31 * 128 + (((2 * g4 + hh) ^ (l31 & 7)) << 4)) =
                    f32x4{acc[rt][ct][4 * g4], acc[rt][ct][4 * g4 + 1], acc[rt][ct][4 * g4 + 2], acc[rt][ct][4 * g4 + 3]};
            wave_lds_fence();
            f32x4 o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rr + 8 * i;
                o[i] = *(const f32x4*)(patch + row * 128 + ((ch ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *(f32x4*)(wsu + (size_t)(128 * wm + 32 * rt + rr + 8 * i) * 256 + 64 * wn + 32 * ct + 4 * ch) = o[i];
            wave_lds_fence();
        }
    if (do_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = gsum[i] + __shfl_xor(gsum[i], 32, 64);
            if (hh == 0) {
                if (g.detb[p]) det_add(g.detb[p] + n0 + 128 * wm + 32 * i + l31, v);
                else atomicAdd(g.gb[p] + n0 + 128 * wm + 32 * i + l31, v);
            }
        }
    }
}

// ---- the same unit with FOUR waves, one per SIMD, each holding a 128 x 128 output tile = 16 accumulator tiles = all 256 AGPRs ----
// The eight-wave kernel above reads 6 operand fragments from LDS for 8 MFMAs per k-step and wave: 96 KB of transposing reads + 32 KB
// of DMA writes per stage and workgroup against 1024 MFMA cycles per SIMD -- the LDS (128 B/clk) is as busy as the MFMA pipe, and the
// kernel sat at ~49 % MFMA-busy.  128 x 128 wave tiles read 8 fragments for 16 MFMAs: 64 + 32 KB per stage.  hipcc cannot keep 256
// accumulators in place for one wave (rounds 3-4: it shuffles them between the register files), so the main loop is one generated asm
// statement that owns them (gen_gemm_asm.py -> linear_dw_ring4_loop.inc; parameters through an LDS block as in rel_attn_dkv64.hip);
// unit decoding, the parameter block and the epilogue stay HIP.  Same images, same stage order, same MFMA operand order as the
// eight-wave kernel: the partial tiles are bit-identical to its.
#if defined(MGX_GEMM_DIAG) && MGX_GEMM_DIAG
#include "linear_dw_ring4_loop_diag.inc"
#else
#include "linear_dw_ring4_loop.inc"
#endif
#ifdef MGX_DW4_TIMES
// diagnostic builds: s_memrealtime (100 MHz) at a unit's start, loop start, loop end and end, per workgroup (tools/dw4_times.py)
__device__ unsigned long long mgx_dw4_times_buf[8 * 1024];     // [workgroup][4 real-time stamps, 4 shader-clock stamps]
extern "C" int mgx_debug_dw4_times(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mgx_dw4_times_buf), sizeof(unsigned long long) * n);
}
#define DW4_TIME(k) do { if (tid == 0) { mgx_dw4_times_buf[8 * blockIdx.x + (k)] = __builtin_amdgcn_s_memrealtime(); \
                                        mgx_dw4_times_buf[8 * blockIdx.x + 4 + (k)] = __builtin_amdgcn_s_memtime(); } } while (0)
#else
#define DW4_TIME(k) do { } while (0)
#endif
__global__ __launch_bounds__(256, 1) void linear_dw_ring4_kernel(const DwRing g, int M, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 1, wn = w & 1;
    const int l31 = lane & 31, hh = lane >> 5;
    DW4_TIME(0);
    const int tiles_all = g.first_tile[g.n];
    const int u = xcd_remap(blockIdx.x, gridDim.x);          // unit order: see linear_dw_ring_kernel
    const int sp = u / tiles_all, t = u - sp * tiles_all;
    const int unit = t * g.splits + sp;
    int p = 0;
    while (p + 1 < g.n && t >= g.first_tile[p + 1]) ++p;
    const int N = g.N[p], K = g.K[p];
    const int ntk = (K + 255) >> 8, tl = t - g.first_tile[p];
    const int n0 = (tl / ntk) << 8, k0 = (tl % ntk) << 8;     // a weight's last tile row / column may be ragged (N, K % 8 == 0)
    const int total = M >> 5;
    const int s0 = sp * g.steps_per_split;
    const int G = min(total, s0 + g.steps_per_split) - s0;   // >= 1 (host)
    char* patch = smem + RG_NST * RG_STAGE + w * RG_PATCH;
    // bias gradient gb[n] += sum_m dY[m][n]: the 2 ntk waves that hold the same dY fragments (wn = 0, 1 of every k-tile of the tile row)
    // share the sums -- one fragment each when there are four or more of them, two each when there are two (gen_gemm_asm.py:
    // BIAS_VARIANTS; 32 v_dot2c per stage in one wave of a workgroup slowed the whole workgroup by a fifth)
    int bias_mode = 0, bias_mask = 0;
    if (g.gb[p] != nullptr) {
        const int j = 2 * (k0 >> 8) + wn;
        if (ntk >= 2) { if (j < 4) { bias_mode = 4 + j; bias_mask = 1 << j; } }
        else { bias_mode = 2 + j; bias_mask = 3 << (2 * j); }
    }
    bias_mode = __builtin_amdgcn_readfirstlane(bias_mode);
    bias_mask = __builtin_amdgcn_readfirstlane(bias_mask);

    // ---- parameter block (layout: gen_gemm_asm.py, prologue), in the wave's epilogue patch ----
    {
        uint32_t* lt = (uint32_t*)(patch + 256) + lane;
        // DMA: this wave fetches pieces q = 4 w + j of both images = rows 8 j .. 8 j + 7 of 64-column sub-tile w
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 8 * j + (lane >> 3);
            const int chunk = (lane & 7) ^ (((r >> 1) & 1) << 2);
            // columns past a ragged edge: fetch the row's last 8 columns instead (in bounds; output element (n, k) depends on dY
            // column n and X column k alone, and the fix-up pass never reads the rows / columns past the edge)
            const int cy = min(64 * w + chunk * 8, N - 8 - n0), cx = min(64 * w + chunk * 8, K - 8 - k0);
            lt[64 * j] = (uint32_t)(((size_t)r * N + cy) * 2);
            lt[64 * (4 + j)] = (uint32_t)(((size_t)r * K + cx) * 2);
        }
        const int i15 = lane & 15, gq = lane >> 4, rq = i15 >> 2;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int chunk = 4 * ct + 2 * (gq & 1) + ((i15 & 3) >> 1);
            const uint32_t in_tile = (8 * hh + rq) * 128 + ((chunk ^ (((rq >> 1) & 1) << 2)) << 4) + 8 * (i15 & 1);
            lt[64 * (8 + ct)] = lds_addr_of(smem) + 2 * wm * TILE_BYTES + in_tile;
            lt[64 * (10 + ct)] = lds_addr_of(smem) + 16384 + 2 * wn * TILE_BYTES + in_tile;
        }
        if (lane == 0) {
            uint64_t* p64 = (uint64_t*)patch;
            p64[0] = (uint64_t)(uintptr_t)(g.dY[p] + (size_t)(s0 * 32) * N + n0);
            p64[1] = (uint64_t)(uintptr_t)(g.X[p] + (size_t)(s0 * 32) * K + k0);
            uint32_t* p32 = (uint32_t*)patch;
            p32[4] = (uint32_t)(32 * N * 2);                 // bytes per stage
            p32[5] = (uint32_t)(32 * K * 2);
            p32[6] = (uint32_t)G;
            p32[7] = lds_addr_of(smem);
            p32[8] = (uint32_t)w;
            p32[9] = (uint32_t)bias_mode;
            p32[10] = p32[11] = 0u;
        }
    }
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = zero16();
    float gsum[4] = {0.f, 0.f, 0.f, 0.f};
    const uint32_t pba = __builtin_amdgcn_readfirstlane(lds_addr_of(patch));
    DW4_TIME(1);
    asm volatile(MGX_DW4_LOOP_ASM
                 : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[1][0]), "+a"(acc[1][1]), "+a"(acc[1][2]),
                   "+a"(acc[1][3]), "+a"(acc[2][0]), "+a"(acc[2][1]), "+a"(acc[2][2]), "+a"(acc[2][3]), "+a"(acc[3][0]), "+a"(acc[3][1]),
                   "+a"(acc[3][2]), "+a"(acc[3][3]), "+v"(gsum[0]), "+v"(gsum[1]), "+v"(gsum[2]), "+v"(gsum[3])
                 : "s"(pba)
                 : MGX_DW4_LOOP_CLOBBERS);
    DW4_TIME(2);

    // ---- epilogue: fp32 partial tile -> workspace, row-major [n][k], 128-byte row segments per 8 lanes ----
    float* wsu = ws + (size_t)unit * 65536;
    const int rr = lane >> 3, ch = lane & 7;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *(f32x4*)(patch + l31 * 128 + (((2 * g4 + hh) ^ (l31 & 7)) << 4)) =
                    f32x4{acc[rt][ct][4 * g4], acc[rt][ct][4 * g4 + 1], acc[rt][ct][4 * g4 + 2], acc[rt][ct][4 * g4 + 3]};
            wave_lds_fence();
            f32x4 o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rr + 8 * i;
                o[i] = *(const f32x4*)(patch + row * 128 + ((ch ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *(f32x4*)(wsu + (size_t)(128 * wm + 32 * rt + rr + 8 * i) * 256 + 128 * wn + 32 * ct + 4 * ch) = o[i];
            wave_lds_fence();
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if ((bias_mask >> i) & 1) {
            const float v = gsum[i] + __shfl_xor(gsum[i], 32, 64);
            if (hh == 0 && n0 + 128 * wm + 32 * i + l31 < N) {
                if (g.detb[p]) det_add(g.detb[p] + n0 + 128 * wm + 32 * i + l31, v);
                else atomicAdd(g.gb[p] + n0 + 128 * wm + 32 * i + l31, v);
            }
        }
    }
    DW4_TIME(3);
}

// gW tile += sum over the M-splits of its partial tiles (fp32, 16 bytes per thread, fully coalesced)
__global__ __launch_bounds__(256) void dw_fixup_kernel(const DwRing g, const float* __restrict__ ws) {
    const int t = blockIdx.y;
    int p = 0;
    while (p + 1 < g.n && t >= g.first_tile[p + 1]) ++p;
    const int K = g.K[p], ntk = (K + 255) >> 8, tl = t - g.first_tile[p];
    const int n0 = (tl / ntk) << 8, k0 = (tl % ntk) << 8;
    const int e4 = blockIdx.x * 256 + threadIdx.x;           // float4 index inside the tile: 0 .. 16383
    if (n0 + (e4 >> 6) >= g.N[p] || k0 + 4 * (e4 & 63) >= K) return;      // past a ragged edge
    const float* src = ws + (size_t)t * g.splits * 65536 + (size_t)e4 * 4;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < g.splits; ++s) {
        const f32x4 v = *(const f32x4*)(src + (size_t)s * 65536);
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
    }
    float* dst = g.gW[p] + (size_t)(n0 + (e4 >> 6)) * K + k0 + 4 * (e4 & 63);
    f32x4 o = *(f32x4*)dst;
    o.x += sum.x; o.y += sum.y; o.z += sum.z; o.w += sum.w;
    *(f32x4*)dst = o;
}

// ---- launchers (linear_common.hpp) ---------------------------------------------------------------------------------------------
static void set_attrs() {
    static const bool once = [] {                          // thread-safe one-time init (C++11 function-local static)
        for (const void* k : {(const void*)linear_ring_kernel<false>, (const void*)linear_ring_kernel<true>,
                              (const void*)linear_ring4_kernel<false, 0>, (const void*)linear_ring4_kernel<true, 0>,
                              (const void*)linear_ring4_kernel<true, 1>, (const void*)linear_ring4_kernel<true, 2>,
                              (const void*)linear_dw_ring_kernel, (const void*)linear_dw_ring4_kernel})
            hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, RG_LDS);
        return true;
    }();
    (void)once;
}

// C [M,NO] = A [M,R] . B^T, forward (B = W [NO,R]; bias, act) or, `btrans`, dX (B = W [R,NO] read transposed; relu_y, addend [M,NO]).
// The kernels have ONE straight-line epilogue per dX operand (addend, else mask): a call with both never gets here (linear.hip:
// dx_route).  The four-wave epilogue's 32-bit offsets (bounded by ring4_shape's out_elems check) address C, relu_y and addend alike.
void mgx_gemm::ring_gemm(bool four, bool btrans, int grid, const uint16_t* A, const uint16_t* B, const float* bias, const uint16_t* relu_y,
                         const uint16_t* addend, uint16_t* C, int M, int NO, int R, int act, void* stream) {
    set_attrs();
#define MGX_RING_LAUNCH(kernel, threads) hipLaunchKernelGGL((kernel), dim3(grid), dim3(threads), RG_LDS, (hipStream_t)stream, A, B, bias, \
                                                            relu_y, addend, C, M, NO, R, act)
    if (!four) { if (btrans) MGX_RING_LAUNCH(linear_ring_kernel<true>, 512); else MGX_RING_LAUNCH(linear_ring_kernel<false>, 512); }
    else if (!btrans) MGX_RING_LAUNCH((linear_ring4_kernel<false, 0>), 256);
    else if (addend) MGX_RING_LAUNCH((linear_ring4_kernel<true, 2>), 256);
    else if (relu_y) MGX_RING_LAUNCH((linear_ring4_kernel<true, 1>), 256);
    else MGX_RING_LAUNCH((linear_ring4_kernel<true, 0>), 256);
#undef MGX_RING_LAUNCH
}

void mgx_gemm::ring_dw(const DwRing& g, int M, float* workspace, void* stream) {
    set_attrs();
    static const int four = gemm_knob("MGX_DW_RING4", 1);  // 0: the eight-wave HIP kernel (A/B, experiment builds)
    const int tiles = g.first_tile[g.n];
    if (four || g.ragged)
        hipLaunchKernelGGL(linear_dw_ring4_kernel, dim3(tiles * g.splits), dim3(256), RG_LDS, (hipStream_t)stream, g, M, workspace);
    else
        hipLaunchKernelGGL(linear_dw_ring_kernel, dim3(tiles * g.splits), dim3(512), RG_LDS, (hipStream_t)stream, g, M, workspace);
    hipLaunchKernelGGL(dw_fixup_kernel, dim3(64, tiles), dim3(256), 0, (hipStream_t)stream, g, (const float*)workspace);
}

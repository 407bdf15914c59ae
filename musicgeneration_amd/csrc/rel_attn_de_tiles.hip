// K3t of the attention backward (overview and math: rel_attn_bwd.hip).
// dE from the dS tiles the dK/dV kernel stored (by query tile x key tile, NOT yet un-skewed):
//     dEr[delta][c] = 1/8 sum_{b,h} sum_{i >= delta} dS[b,h][i][i-delta] q[b,i,h,c]
// A workgroup owns four tile DIAGONALS I - J = c0 + m, m = 0..3, for a fixed number of 64-row steps of the flattened
// (b, h, i-block) sweep, so every stored tile is read exactly once by this kernel.  Tile m holds the distances
// 32(c0+m) - 31 .. + 31: the four diagonals touch FIVE chunks of 32 distances, c0-1 .. c0+3 (the first and the last only
// through one triangle of their tiles; the neighbouring workgroups add the other triangles -- dE is summed with atomics
// anyway).  The skew happens while a step's tiles are parked in LDS: element (i, j) of tile m goes to row i, column
// 32(m+1) + i - j of a [64 rows][160 distances] image -- every write lands inside the row (no predication, no wrap);
// positions no tile writes are zeroed once and stay zero.  Wave w (of 5) multiplies columns 32w .. 32w+31 = chunk c0-1+w.
#include "rel_attn_common.hpp"

using namespace relattn;

#ifndef MGX_DET_PEEL
#define MGX_DET_PEEL 0      // timing experiments only (tools/peel_de_tiles.sh): 1 three quarters of the scatter stores | 2 no products |
#endif                      // 4 q tile re-read from row block 0 (L2-resident) | 8 no atomic flush of the chunk sums; results are then wrong

namespace k3t {
// (experiment, removed: 16 or 64 steps per workgroup instead of 32 ran 0.593 / 0.588 against 0.576 ms at cfg2 / batch 64)
constexpr int DIAGS = 4, RS = 64, STEPS = 32, NW = 5;
constexpr int AROW = 352;                                  // bytes per image row: 160 bf16 + pad (4 consecutive rows -> 4 bank groups)
constexpr int OFF_A = 0;                                   // [64 i][160 distance columns]
constexpr int OFF_Q = RS * AROW;                           // q tile [64 i][64 c]: 2 sub-tiles image T
constexpr int LDS_BYTES = OFF_Q + 2 * TILE_BYTES;          // 30,720 B
constexpr int SLOTS = 2;                                   // tiles per wave and step: 8 tiles on waves 0..3
}  // namespace k3t

// natural-k transposed fragment: X[16*ks + 8*hh + j][32*ct + (lane&31)], j = 0..7, from an image-T tile.  (Not an instance of
// frag_tr in rel_attn_common.hpp with another row order: built that way, the kernel's listing moves.)
MGX_DEV bf16x8 frag_Tn(const char* tile, int lane, int ks, int ct) {
    const int i = lane & 15, g = lane >> 4, hh = lane >> 5;
    const int rq = i >> 2;
    const int chunk = 4 * ct + 2 * (g & 1) + ((i & 3) >> 1);
    const int byte_in = 8 * (i & 1);
    bf16x8 out;
#pragma unroll
    for (int jq = 0; jq < 2; ++jq) {
        const int row = 16 * ks + 8 * hh + 4 * jq + rq;
        bf16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(tile + imgT_off(row, chunk) + byte_in));
        out[4 * jq + 0] = t[0]; out[4 * jq + 1] = t[1]; out[4 * jq + 2] = t[2]; out[4 * jq + 3] = t[3];
    }
    return out;
}

__global__ __launch_bounds__(320, 4) void rel_attn_de_tiles_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dst, float* __restrict__ dEr /* = dE + (M-L)*64 */,
    int bgroup, int ngroups, int wg_per_group, int L, int d,
    long long* __restrict__ det /* deterministic mode: [L][64] fixed-point image of this launch's dEr */) {
    using namespace k3t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int heads = d >> 6, nbh = bgroup * heads;
    const size_t ld = (size_t)3 * d;
    const int nchunk = L >> 5;
    // workgroup -> (batch group, diagonal group t, slice of its flattened (bh, row-block) sweep); inside a batch group the
    // diagonal groups are laid out longest sweep first
    int t = 0, first = 0, ns = 0;
    // Batch groups are dealt to the XCDs (workgroups b and b + 8 share one, MI355X_MICROARCH.md): workgroup 8 k + x belongs to group
    // 8 (k / wg_per_group) + x.  A group's workgroups -- all the diagonal groups that re-read the same q rows -- then share an L2,
    // and with groups of ONE batch row (2 MB of q at cfg2) the re-reads are L2 hits instead of fabric reads.  Speed only.
    // (ngroups % 8 == 0 on this path; otherwise -- e.g. cfg4's four batch rows per GPU -- the host passes ngroups < 0 and the
    // groups are laid out one after the other: a round of eight with idle XCDs would leave part of the chip without work)
    const bool dealt = ngroups > 0;
    const int xk = dealt ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int grp = dealt ? (xk / wg_per_group) * 8 + (int)(blockIdx.x & 7) : xk / wg_per_group;
    {
        int rest = xk % wg_per_group;
        const int ntile = (nchunk + DIAGS - 1) / DIAGS;
        for (t = 0; t < ntile; ++t) {
            ns = (L - t * DIAGS * 32 + RS - 1) / RS;       // row blocks i0 = 32 c0, +64, ... < L (query tiles I >= c0)
            const int nwg = (nbh * ns + STEPS - 1) / STEPS;
            if (rest < nwg) break;
            rest -= nwg;
        }
        if (t == ntile) return;
        first = rest * STEPS;
    }
    const int total = nbh * ns;
    const int last = min(total, first + STEPS);
    const int c0 = t * DIAGS, d0 = c0 * 32;
    const size_t ntri = (size_t)nchunk * (nchunk + 1) / 2;
    const int qrow = tid >> 3, qch = tid & 7;              // threads 0..255 stage q
    const uint32_t lane16 = (uint32_t)lane * 16u;
    // slot k of wave w < 4 = tile idx = w + 4k of the step: query tile rb = idx / 4 (of 2), diagonal m = idx % 4 = w
    const int wm = w & 3;
    // scatter address of register r (query crow(r,hh), key l31): row crow*AROW, column 32(m+1) + crow - l31
    const int sc_lane = hh * 4 * (AROW + 2) - 2 * l31;      // + crow(r,0) * (AROW + 2) as the immediate
    u32x4 areg[SLOTS][2], qreg[2];
    bool a_ok[SLOTS], q_ok[2];
    auto load_tiles = [&](int g) {
        const int bhl = g / ns, i0 = d0 + (g - bhl * ns) * RS;
        const int bh = grp * nbh + bhl;
        const int bb = bh / heads, hd = bh - bb * heads;
        const int I0 = i0 >> 5;
        const char* tp = (const char*)(dst + (size_t)bh * ntri * 1024) + lane16;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {                  // slot k = query tile I0 + k; wave 4 loads (clamped) data it never uses
            const int I = I0 + k, J = I - c0 - wm;
            a_ok[k] = I < nchunk && J >= 0;
            const size_t Ic = (size_t)min(I, nchunk - 1), Jc = (size_t)max(J, 0);      // clamped: a valid address either way
            const char* p = tp + (Ic * (Ic + 1) / 2 + min(Jc, Ic)) * 2048;
            areg[k][0] = __builtin_nontemporal_load((const u32x4*)p);
            areg[k][1] = __builtin_nontemporal_load((const u32x4*)(p + 1024));
        }
        const uint16_t* qp = qkv + ((size_t)bb * L + ((MGX_DET_PEEL & 4) ? 0 : i0)) * ld + hd * 64 + (qch & 7) * 8;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = (qrow & 31) + 32 * i;
            q_ok[i] = i0 + r < L;
            qreg[i] = *(const u32x4*)(qp + (size_t)min(r, L - 1 - i0) * ld);
        }
    };
    auto store_tiles = [&]() {
        const u32x4 zero = {0, 0, 0, 0};
        if (w < 4) {                                       // wave-uniform
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) {
                char* base = smem + OFF_A + k * 32 * AROW + 64 * (wm + 1) + sc_lane;
#pragma unroll
                for (int ss = 0; ss < 2; ++ss) {
                    const u32x4 v = a_ok[k] ? areg[k][ss] : zero;
#pragma unroll
                    for (int j = 0; j < ((MGX_DET_PEEL & 1) ? 1 : 4); ++j) {
                        const int r0 = 8 * ss + 2 * j;
                        *(uint16_t*)(base + crow(r0, 0) * (AROW + 2)) = (uint16_t)v[j];
                        *(uint16_t*)(base + crow(r0 + 1, 0) * (AROW + 2)) = (uint16_t)(v[j] >> 16);
                    }
                }
            }
            char* qt = smem + OFF_Q;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = qrow + 32 * i;
                *(u32x4*)(qt + (r >> 5) * TILE_BYTES + imgT_off(r & 31, qch)) = q_ok[i] ? qreg[i] : zero;
            }
        }
    };
    f32x16 de0 = zero16(), de1 = zero16();
    // A fragment: A[m = distance column 32w + (lane&31)][k = i = 16ks + 8hh + j] from the [i][distance] image (transposing reads)
    const int fa_i = lane & 15, fa_g = lane >> 4;
    const int fa_off = (fa_i >> 2) * AROW + (32 * w) * 2 + (2 * (fa_g & 1) + ((fa_i & 3) >> 1)) * 16 + 8 * (fa_i & 1) + 8 * hh * AROW;
    auto multiply = [&]() {
        if (MGX_DET_PEEL & 2) return;
        const char* at = smem + OFF_A + fa_off;
        const char* qt = smem + OFF_Q;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 af;
#pragma unroll
            for (int jq = 0; jq < 2; ++jq) {
                const bf16x4 tq = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(at + (16 * ks + 4 * jq) * AROW));
                af[4 * jq + 0] = tq[0]; af[4 * jq + 1] = tq[1]; af[4 * jq + 2] = tq[2]; af[4 * jq + 3] = tq[3];
            }
            const char* qs = qt + (ks >> 1) * TILE_BYTES;
            de0 = mfma(af, frag_Tn(qs, lane, ks & 1, 0), de0);
            de1 = mfma(af, frag_Tn(qs, lane, ks & 1, 1), de1);
        }
    };
    // image positions that no tile writes (the triangles that belong to the neighbouring diagonal groups) must read as zero
    for (int o = tid * 16; o < RS * AROW; o += NW * 64 * 16) *(u32x4*)(smem + OFF_A + o) = u32x4{0, 0, 0, 0};
    __syncthreads();
    if (first < last) {
        load_tiles(first);
        store_tiles();
    }
    __syncthreads();
    for (int g = first; g + 1 < last; ++g) {
        load_tiles(g + 1);
        __builtin_amdgcn_sched_barrier(0);              // keep the prefetch ahead of the products
        multiply();
        __syncthreads();                                // every wave has read the image
        store_tiles();
        __syncthreads();
    }
    if (first < last) multiply();
    // flush: rows = distances 32(c0-1+w) + crow(r,hh), columns on lanes; q was not pre-scaled -> 1/8 here
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int dl = d0 - 32 + 32 * w + crow(r, hh);
        if ((MGX_DET_PEEL & 8) && de0[r] + de1[r] != 12345.f) continue;      // peel: no flush (timing only)
        if (dl >= 0 && dl < L) {
            if (det) {
                long long* drow = det + (size_t)(L - 1 - dl) * 64;
                det_add(drow + l31, 0.125f * de0[r]);
                det_add(drow + 32 + l31, 0.125f * de1[r]);
                continue;
            }
            float* row = dEr + (size_t)(L - 1 - dl) * 64;
            atomicAdd(row + l31, 0.125f * de0[r]);
            atomicAdd(row + 32 + l31, 0.125f * de1[r]);
        }
    }
}

// Groups of ONE batch row, dealt to the XCDs, where B is whole rounds of eight; the attention kernels' batch group `bg`, laid out
// one after the other, otherwise (see the kernel).  (The rows per dealt group were an A/B switch, retired: one row against the
// attention kernels' 8 at cfg2 / batch 64 took the fabric reads from 3.19 to 2.45 GB per launch, the time unchanged within noise.)
relattn::DeTilesPlan relattn::de_tiles_plan(int B, int L, int d, int bg) {
    DeTilesPlan p{B % 8 == 0, B % 8 == 0 ? 1 : bg, 0, 0, 0};
    p.ngroups = B / p.rows;
    for (int t = 0; t < (L / 32 + k3t::DIAGS - 1) / k3t::DIAGS; ++t)
        p.wg_per_group += ((long)p.rows * (d / 64) * ((L - t * k3t::DIAGS * 32 + k3t::RS - 1) / k3t::RS) + k3t::STEPS - 1) / k3t::STEPS;
    p.grid = p.wg_per_group * p.ngroups;
    return p;
}

int relattn::de_tiles_launch(const uint16_t* qkv, const uint16_t* dst, float* dEr, const DeTilesPlan& p, int L, int d, void* stream) {
    static const hipError_t once = hipFuncSetAttribute((const void*)rel_attn_de_tiles_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k3t::LDS_BYTES);
    (void)once;                                            // function-local static: set exactly once, thread-safe
    int rc;
    long long* det = mgx_det_scratch((size_t)L * 64, stream, &rc);      // deterministic mode: integer atomics + fold
    if (rc != MGX_OK) return rc;
    hipLaunchKernelGGL(rel_attn_de_tiles_kernel, dim3((unsigned)p.grid), dim3(64 * k3t::NW), k3t::LDS_BYTES, (hipStream_t)stream, qkv,
                       dst, dEr, p.rows, p.dealt ? p.ngroups : -p.ngroups, (int)p.wg_per_group, L, d, det);
    if (det) launch_det_fold(det, dEr, (size_t)L * 64, 1.f, 1, (hipStream_t)stream);
    return MGX_OK;
}

// Train-time augmentation on the device (ABI 29; contract in include/mgx.h): mgx_crop_augment cuts one crop per row out of a
// 16-bit corpus that lives in device memory, stretches its time, transposes it and writes the model's x / y pair.
//
// One workgroup per row.  The source is walked in tiles of CROP_TILE = CROP_THREADS * CROP_PER_THREAD tokens; a thread owns
// CROP_PER_THREAD CONSECUTIVE tokens of the tile, so its part of either scan is a short serial run in registers.  Per tile:
//   scan 1 (64-bit)  the time units u of every token -> the cumulative time T_i (carried from tile to tile),
//                    S_i = floor((T_i q + 500) / 1000): a time token emits S_i - S_{i-1} units as ids of at most n_ts units each;
//   scan 2 (64-bit)  the number of ids every token emits -> the position of its first id in the output (carried likewise);
//   compaction       every thread writes its tokens' ids at their positions, through the transposition table.
// The loop ends as soon as n ids are out; what a short row leaves is filled with pad_token.  Plain loads and stores, no atomics:
// every output element has one writer.  Without a stretch the same code runs with q = 1000 and an empty time run (every token
// emits itself).
#include "mgx_common.hpp"

namespace {
constexpr int CROP_THREADS = 256;
constexpr int CROP_PER_THREAD = 4;
constexpr int CROP_TILE = CROP_THREADS * CROP_PER_THREAD;      // 1024 source tokens per pass (tests/test_gpu_augment_kernels.py: T)
constexpr int CROP_WAVES = CROP_THREADS / 64;

// Exclusive prefix sum of `v` over the workgroup's threads (in thread order) and the workgroup's total.  Inclusive scan inside
// each wave by shuffles, the four wave totals through LDS.  `part` holds CROP_WAVES entries; the two barriers make it reusable
// by the next call.
MGX_DEV long long block_exclusive_scan(long long v, long long* part, long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CROP_WAVES; ++w) {
        const long long p = part[w];
        if (w < wave) before += p;
        all += p;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

struct CropOut {
    int32_t* x;
    int32_t* y;
    long long row;                // b * stride_b
    long long stride_t;
    int n;
    const int32_t* perm;          // the row of the transposition table, or NULL
    int V;
};

// out[j] = id: x[j] for j < n - 1 (j < n without y), y[j - 1] for 1 <= j < n
MGX_DEV void put(const CropOut& o, long long j, int id, bool mapped) {
    if (j >= o.n) return;
    if (mapped && o.perm && id >= 0 && id < o.V) id = o.perm[id];
    if (o.y) {
        if (j < o.n - 1) o.x[o.row + j * o.stride_t] = id;
        if (j >= 1) o.y[o.row + (j - 1) * o.stride_t] = id;
    } else {
        o.x[o.row + j * o.stride_t] = id;
    }
}

__global__ __launch_bounds__(CROP_THREADS) void crop_augment_kernel(const uint16_t* __restrict__ corpus, size_t corpus_len,
                                                                    const int64_t* __restrict__ start,
                                                                    const int32_t* __restrict__ avail,
                                                                    const int32_t* __restrict__ perm, int S, int V,
                                                                    const int32_t* __restrict__ shift_row,
                                                                    const int32_t* __restrict__ stretch_q, int ts0, int n_ts,
                                                                    int32_t* __restrict__ x, int32_t* __restrict__ y, int stride_b,
                                                                    int stride_t, int32_t* __restrict__ n_out, int pad_token, int n) {
    __shared__ long long part[CROP_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;

    // the row's source: corpus[st .. st + n_src), inside the corpus whatever start / avail hold
    const long long st = start[b];
    const long long av = avail[b];
    long long n_src = stretch_q ? 2LL * n : (long long)n;
    if (st < 0 || av < 0 || (unsigned long long)st >= corpus_len) {
        n_src = 0;
    } else {
        if (av < n_src) n_src = av;
        const unsigned long long left = corpus_len - (unsigned long long)st;
        if (left < (unsigned long long)n_src) n_src = (long long)left;
    }
    long long q = 1000;
    int run = 0;                                              // ids ts0 .. ts0 + run - 1 carry time
    if (stretch_q) {
        const int qb = stretch_q[b];
        if (qb >= 500 && qb <= 2000) q = qb;
        run = n_ts;
    }
    CropOut o;
    o.x = x; o.y = y; o.row = (long long)b * stride_b; o.stride_t = stride_t; o.n = n; o.V = V;
    o.perm = nullptr;
    if (perm) {
        const int s = shift_row[b];
        if (s >= 0 && s < S) o.perm = perm + (size_t)s * V;
    }

    long long t_carry = 0;                                    // T of the last token before this tile
    long long emitted = 0;                                    // ids out before this tile
    for (long long t0 = 0; t0 < n_src && emitted < n; t0 += CROP_TILE) {          // uniform over the workgroup
        const long long i0 = t0 + (long long)tid * CROP_PER_THREAD;
        int tok[CROP_PER_THREAD], u[CROP_PER_THREAD];
        long long usum = 0;
#pragma unroll
        for (int k = 0; k < CROP_PER_THREAD; ++k) {
            const bool live = i0 + k < n_src;
            tok[k] = live ? (int)corpus[st + i0 + k] : -1;
            u[k] = (live && run > 0 && tok[k] >= ts0 && tok[k] - ts0 < run) ? tok[k] - ts0 + 1 : 0;
            usum += u[k];
        }
        long long t_tile;
        long long T = t_carry + block_exclusive_scan(usum, part, &t_tile);
        t_carry += t_tile;

        int full[CROP_PER_THREAD], rem[CROP_PER_THREAD];     // a token emits `full` ids of n_ts units, then `rem` units if > 0
        long long cnt = 0;
        long long s_prev = (T * q + 500) / 1000;
#pragma unroll
        for (int k = 0; k < CROP_PER_THREAD; ++k) {
            full[k] = 0; rem[k] = 0;
            if (u[k] > 0) {
                T += u[k];
                const long long s_now = (T * q + 500) / 1000;
                const long long delta = s_now - s_prev;      // <= 2 n_ts: q <= 2000 and u <= n_ts
                s_prev = s_now;
                full[k] = (int)(delta / run);
                rem[k] = (int)(delta % run);
                cnt += full[k] + (rem[k] > 0);
            } else if (tok[k] >= 0) {
                cnt += 1;
            }
        }
        long long c_tile;
        long long pos = emitted + block_exclusive_scan(cnt, part, &c_tile);
        emitted += c_tile;

#pragma unroll
        for (int k = 0; k < CROP_PER_THREAD; ++k) {
            if (u[k] > 0) {
                for (int f = 0; f < full[k] && pos < n; ++f) put(o, pos++, ts0 + run - 1, true);
                if (rem[k] > 0) put(o, pos++, ts0 + rem[k] - 1, true);
            } else if (tok[k] >= 0) {
                put(o, pos++, tok[k], true);
            }
        }
    }
    const long long got = emitted < n ? emitted : (long long)n;
    for (long long j = got + tid; j < n; j += CROP_THREADS) put(o, j, pad_token, false);
    if (n_out && tid == 0) n_out[b] = (int32_t)got;
}
}  // namespace

extern "C" int mgx_crop_augment(const uint16_t* corpus, size_t corpus_len, const int64_t* start, const int32_t* avail,
                                const int32_t* perm, int S, int V, const int32_t* shift_row, const int32_t* stretch_q, int ts0,
                                int n_ts, int32_t* x, int32_t* y, int stride_b, int stride_t, int32_t* n_out, int pad_token, int B,
                                int n, void* stream) {
    MGX_REQUIRE(corpus && start && avail && x, MGX_ERR_NULL, "mgx_crop_augment: NULL pointer");
    MGX_REQUIRE((perm != nullptr) == (shift_row != nullptr), MGX_ERR_NULL,
                "mgx_crop_augment: perm and shift_row must both be given or both be NULL");
    MGX_REQUIRE(B > 0 && n > 0 && V > 0, MGX_ERR_SHAPE, "mgx_crop_augment: need B>0, n>0, V>0 (B=%d n=%d V=%d)", B, n, V);
    MGX_REQUIRE(!perm || S > 0, MGX_ERR_SHAPE, "mgx_crop_augment: a table needs S>0 rows (S=%d)", S);
    MGX_REQUIRE(stride_b > 0 && stride_t > 0, MGX_ERR_SHAPE, "mgx_crop_augment: need stride_b>0, stride_t>0 (%d, %d)", stride_b,
                stride_t);
    MGX_REQUIRE(!stretch_q || (ts0 >= 0 && n_ts >= 1 && (long long)ts0 + n_ts <= 65536), MGX_ERR_SHAPE,
                "mgx_crop_augment: the time run must lie inside the 16-bit ids (ts0=%d n_ts=%d)", ts0, n_ts);
    hipLaunchKernelGGL(crop_augment_kernel, dim3(B), dim3(CROP_THREADS), 0, (hipStream_t)stream, corpus, corpus_len, start, avail,
                       perm, S, V, shift_row, stretch_q, ts0, n_ts, x, y, stride_b, stride_t, n_out, pad_token, n);
    MGX_CHECK_LAUNCH("mgx_crop_augment");
    return MGX_OK;
}

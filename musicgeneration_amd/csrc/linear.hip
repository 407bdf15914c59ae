// Projection / FFN / vocabulary GEMMs of the hot path (layers.py:71-84,108,157-158; network.py:39) and their backward: the C entry
// points that choose a kernel, their argument checks and the routing.  The kernels and their launchers live one family per file:
// linear_tile128.hip (128 x 128 tiles, any shape), linear_ring.hip (256 x 256 persistent ring, eight or four waves),
// linear_skinny.hip (M <= 32, with the decode path's entry points, which never choose).  Which call takes which family is decided
// here and nowhere else: fwd_route / dx_route for forward and dX, dw_plan for the grouped weight gradients.  A/B knobs (experiment
// builds only; linear_common.hpp: gemm_knob): MGX_GEMM_RING and MGX_RING4 here, MGX_DW_RING4 in the ring launcher.
#include "linear_common.hpp"

// ---- forward and dX: one routing decision ---------------------------------------------------------------------------------------
// The ring kernel pays when its 256 x 256 tiles fill the chip (one persistent workgroup per CU) without much padding.
// MGX_GEMM_RING=0 / 1 forces it off / on where the shape allows (A/B timing; experiment builds only).
static int ring_grid(int M, int NO, int R, void* stream) {
    static const int env = gemm_knob("MGX_GEMM_RING", -1);
    const int cus = mgx_stream_cu_count(stream);            // a CU-masked stream: one persistent workgroup per CU it may use
    if (env == 0 || R % 32 != 0 || R < 128 || M % 256 != 0 || NO % 256 != 0) return 0;     // whole tiles only
    const long ntiles = (long)(M / 256) * (NO / 256);
    if (env != 1 && ntiles * 4 < (long)cus * 3) return 0;                            // < 3/4 of the CUs busy
    return (int)(ntiles < cus ? ntiles : cus);
}

// the four-wave kernel's tile statement runs whole rounds of its two-slot ring, at least two (reduction % 128 == 0, >= 256);
// MGX_RING4=0 keeps the eight-wave kernel (A/B; experiment builds only)
// ... and it does not win everywhere.  Measured per call site inside the training step (profiles/r05_ring4_in_step.txt, cfg2; cfg4 with
// MGX_RING4=0/1/2): it wins 3-7 % on the QKV and output projections, forward and dX (8-24 stages of 64 columns per tile, output 512
// columns or wider; cfg4's 768 x 768 projection with ONE tile per workgroup included), and loses 10-14 % on the FFN's GEMMs: tiles of
// only four stages (reduction 256) pay the statement's fixed costs (parameter block, fragment addresses, first reads: ~1.5 K cycles)
// per 11 K, and with a 256-column output every workgroup streams its own A rows against the same B tile -- two 64 KB requests in
// flight keep the HBM less busy than the eight-wave kernel's four 32 KB ones.  Those stay on the eight-wave kernel.
static bool ring4_shape(int R, int NO, long long out_elems) {
    static const int env = gemm_knob("MGX_RING4", 1);
    if (env == 0 || R % 128 != 0 || R < 256 || out_elems * 2 >= (1ll << 32)) return false;     // (the epilogue addresses the output with 32-bit offsets)
    return env == 2 || (R >= 512 && NO >= 512);              // MGX_RING4=2 (experiment builds): wherever the shape allows
}

struct GemmRoute { int family, grid; };    // MGX_GEMM_SKINNY | TILE128 | RING8 | RING4 (mgx.h); persistent workgroups of a ring kernel, else 0
// output [M,NO], reduction R, on `stream`
static GemmRoute ring_route(int M, int NO, int R, void* stream) {
    const int rg = ring_grid(M, NO, R, stream);
    if (!rg) return {MGX_GEMM_TILE128, 0};
    return {ring4_shape(R, NO, (long long)M * NO) ? MGX_GEMM_RING4 : MGX_GEMM_RING8, rg};
}
// forward: C [M,N] = A [M,K] . W [N,K]^T; decode-size batches take the weight-streaming skinny kernel
static GemmRoute fwd_route(int M, int N, int K, void* stream) {
    if (M <= 32) return {MGX_GEMM_SKINNY, 0};
    return ring_route(M, N, K, stream);
}
// dX [M,K] = dY [M,N] . W [N,K], reduction over N.  The ring kernels have one epilogue per operand: a call with both a ReLU mask and
// an addend takes the 128 x 128 kernel (the training step never makes one)
static GemmRoute dx_route(int M, int N, int K, bool mask, bool addend, void* stream) {
    if (mask && addend) return {MGX_GEMM_TILE128, 0};
    return ring_route(M, K, N, stream);
}

extern "C" int mgx_linear_fwd(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* C, int M, int N,
                              int K, int act, void* stream) {
    MGX_REQUIRE(A && W && C, MGX_ERR_NULL, "mgx_linear_fwd: NULL pointer");
    MGX_REQUIRE(M > 0 && N > 0 && K > 0 && K % 64 == 0 && N % 4 == 0, MGX_ERR_SHAPE,
                "mgx_linear_fwd: need K%%64==0 and N%%4==0 (got M=%d N=%d K=%d)", M, N, K);
    MGX_REQUIRE(act == 0 || act == 1, MGX_ERR_SHAPE, "mgx_linear_fwd: act must be 0 (none) or 1 (ReLU)");
    const GemmRoute r = fwd_route(M, N, K, stream);
    switch (r.family) {
        case MGX_GEMM_SKINNY: mgx_gemm::skinny_fwd(A, W, bias, C, M, N, K, act, stream); break;
        case MGX_GEMM_TILE128: mgx_gemm::tile128_fwd(A, W, bias, C, M, N, K, act, stream); break;
        default: mgx_gemm::ring_gemm(r.family == MGX_GEMM_RING4, false, r.grid, A, W, bias, nullptr, nullptr, C, M, N, K, act, stream);
    }
    MGX_CHECK_LAUNCH("mgx_linear_fwd");
    return MGX_OK;
}

extern "C" int mgx_linear_dx(const uint16_t* dY, const uint16_t* W, const uint16_t* relu_y, const uint16_t* addend,
                             uint16_t* dX, int M, int N, int K, void* stream) {
    MGX_REQUIRE(dY && W && dX, MGX_ERR_NULL, "mgx_linear_dx: NULL pointer");
    MGX_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0 && K % 8 == 0, MGX_ERR_SHAPE,
                "mgx_linear_dx: need N%%8==0 and K%%8==0 (got M=%d N=%d K=%d)", M, N, K);
    const GemmRoute r = dx_route(M, N, K, relu_y != nullptr, addend != nullptr, stream);
    if (r.family == MGX_GEMM_TILE128) mgx_gemm::tile128_dx(dY, W, relu_y, addend, dX, M, N, K, stream);
    else mgx_gemm::ring_gemm(r.family == MGX_GEMM_RING4, true, r.grid, dY, W, nullptr, relu_y, addend, dX, M, K, N, 0, stream);
    MGX_CHECK_LAUNCH("mgx_linear_dx");
    return MGX_OK;
}

// Which kernel family a forward / dX call of this shape takes on `stream` (mgx.h: mgx_linear_kernel_id; tests assert that the
// bench-shape calls they check really run the ring kernels of THIS binary): the decision the two entry points above switch on.
// kind 0: forward; 1 / 2 / 3 / 4: dX with no epilogue operand / a ReLU mask / a residual addend / both.
extern "C" int mgx_linear_kernel_id(int kind, int M, int N, int K, void* stream) {
    MGX_REQUIRE(kind >= 0 && kind <= 4 && M > 0 && N > 0 && K > 0, MGX_ERR_SHAPE, "mgx_linear_kernel_id: kind 0..4, positive sizes");
    return (kind == 0 ? fwd_route(M, N, K, stream) : dx_route(M, N, K, kind == 2 || kind == 4, kind == 3 || kind == 4, stream)).family;
}

// ---- weight gradients -----------------------------------------------------------------------------------------------------------
extern "C" int mgx_linear_dw(const uint16_t* dY, const uint16_t* X, float* gW, float* gb, int M, int N, int K,
                             void* stream) {
    MGX_REQUIRE(dY && X && gW, MGX_ERR_NULL, "mgx_linear_dw: NULL pointer");
    MGX_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0 && K % 8 == 0, MGX_ERR_SHAPE,
                "mgx_linear_dw: need N%%8==0 and K%%8==0 (got M=%d N=%d K=%d)", M, N, K);
    int rc;
    long long* det = mgx_det_scratch((size_t)N * K + N, stream, &rc);      // deterministic mode: integer atomics + fold
    if (rc != MGX_OK) return rc;
    mgx_gemm::tile128_dw(dY, X, gW, gb, M, N, K, det, det ? det + (size_t)N * K : nullptr, stream);
    if (det) {
        launch_det_fold(det, gW, (size_t)N * K, 1.f, 1, (hipStream_t)stream);
        if (gb) launch_det_fold(det + (size_t)N * K, gb, (size_t)N, 1.f, 1, (hipStream_t)stream);
    }
    MGX_CHECK_LAUNCH("mgx_linear_dw");
    return MGX_OK;
}

// The ring kernel takes the weights that fill their 256 x 256 tiles at least to 60 % (N, K multiples of 8, at least 64): every
// encoder-block projection tiles exactly; the vocabulary projection (448 x 512: 87.5 %) and cfg4's FFN weights (384 x 768: 75 %)
// have a ragged last tile row / column, whose DMA offsets the kernel clamps and whose outer part the fix-up pass skips -- the wasted
// MFMA work costs less than the 128 x 128 kernel's atomics and its half-idle MFMA pipe (round 5: 148 -> ~75 us for the vocabulary
// projection at M = 131072).
static bool dw_ring_shape(int N, int K) {
    if (N % 8 != 0 || K % 8 != 0 || N < 64 || K < 64) return false;
    const long long tiles = (long long)((N + 255) / 256) * ((K + 255) / 256);
    return (long long)N * K * 10 >= tiles * 65536 * 6;
}

// What a group of weight gradients that share M does on `cus` CUs.  The problems whose weights fill their tiles (dw_ring_shape) take
// the ring kernel in one launch, the others the 128 x 128 grouped kernel -- until round 4 one such weight sent the whole block there
// (cfg4: 219 us per block, 12 % of the step).  The ring's M-splits are chosen so that tiles x splits fills the CUs once, every split
// with at least one 32-row step; when that cannot be done (M, more tiles than CUs) the whole group, in its order, is left.
struct DwPlan {
    DwRing ring;                                           // ring.n == 0: nothing takes the ring
    size_t ws_bytes;                                       // the ring's partial tiles: one 256 x 256 fp32 tile per (tile, split)
    mgx_dw_problem rest[MGX_DW_MAX_GROUP];                 // left for the 128 x 128 kernels
    int nrest;
};
static DwPlan dw_plan(const mgx_dw_problem* problems, int count, int M, int cus) {
    static const int env = gemm_knob("MGX_GEMM_RING", -1);
    DwPlan p;
    DwRing& g = p.ring;
    g.n = g.ragged = g.first_tile[0] = p.nrest = 0;
    p.ws_bytes = 0;
    for (int i = 0; i < count; ++i) {
        const mgx_dw_problem& q = problems[i];
        if (!dw_ring_shape(q.N, q.K)) { p.rest[p.nrest++] = q; continue; }
        const int j = g.n++;
        g.dY[j] = q.dY; g.X[j] = q.X; g.gW[j] = q.gW; g.gb[j] = q.gb; g.detb[j] = nullptr; g.N[j] = q.N; g.K[j] = q.K;
        g.ragged |= (q.N % 256 != 0 || q.K % 256 != 0);
        g.first_tile[j + 1] = g.first_tile[j] + ((q.N + 255) / 256) * ((q.K + 255) / 256);
    }
    const int tiles = g.first_tile[g.n], total = M / 32;
    if (env == 0 || M % 32 != 0 || M < 4096 || tiles == 0 || tiles > cus) {
        for (int i = 0; i < count; ++i) p.rest[i] = problems[i];
        p.nrest = count, g.n = 0;
        return p;
    }
    const int splits = cus / tiles < total ? cus / tiles : total;
    g.steps_per_split = (total + splits - 1) / splits;
    g.splits = (total + g.steps_per_split - 1) / g.steps_per_split;
    p.ws_bytes = (size_t)tiles * g.splits * 65536 * sizeof(float);
    return p;
}

extern "C" size_t mgx_linear_dw_grouped_workspace(const mgx_dw_problem* problems, int count, int M) {
    if (!problems || count <= 0 || count > MGX_DW_MAX_GROUP) return 0;
    // (no stream here: planned for the whole device -- a CU-masked stream runs fewer M-splits, so this is an upper bound for it)
    return dw_plan(problems, count, M, mgx_stream_cu_count(nullptr)).ws_bytes;
}

extern "C" int mgx_linear_dw_grouped(const mgx_dw_problem* problems, int count, int M, void* workspace, size_t ws_bytes,
                                     void* stream) {
    MGX_REQUIRE(problems && count > 0 && count <= MGX_DW_MAX_GROUP && M > 0, MGX_ERR_SHAPE,
                "mgx_linear_dw_grouped: need 1..%d problems and M > 0 (got %d, M=%d)", MGX_DW_MAX_GROUP, count, M);
    for (int i = 0; i < count; ++i) {
        const mgx_dw_problem& q = problems[i];
        MGX_REQUIRE(q.dY && q.X && q.gW, MGX_ERR_NULL, "mgx_linear_dw_grouped: NULL pointer in problem %d", i);
        MGX_REQUIRE(q.N > 0 && q.K > 0 && q.N % 8 == 0 && q.K % 8 == 0, MGX_ERR_SHAPE,
                    "mgx_linear_dw_grouped: need N%%8==0 and K%%8==0 (problem %d: N=%d K=%d)", i, q.N, q.K);
    }
    // the M-splits are planned for the CUs of the stream the call is issued on -- except in deterministic mode: the partial tiles
    // are added in split order, so the number of splits is part of the result's bits, and a run with the weight gradients on a
    // CU-masked side stream must equal the one-stream run bit for bit (tests/test_gpu_dp.py): there the plan is the whole device's
    DwPlan p = dw_plan(problems, count, M, mgx_stream_cu_count(mgx_deterministic() ? nullptr : stream));
    if (DwRing& rg = p.ring; rg.n) {
        MGX_REQUIRE(workspace && ws_bytes >= p.ws_bytes && ((uintptr_t)workspace & 15) == 0, MGX_ERR_SHAPE,
                    "mgx_linear_dw_grouped: workspace must be 16-byte aligned and >= mgx_linear_dw_grouped_workspace() = %zu bytes "
                    "(got %zu)", p.ws_bytes, ws_bytes);
        // deterministic mode: the weight tiles already are (partial tiles in the workspace, added in split order by the fix-up
        // pass); the bias gradients, which the M-splits add with atomics, go through the fixed-point scratch
        size_t nb = 0;
        for (int i = 0; i < rg.n; ++i) nb += rg.gb[i] ? (size_t)rg.N[i] : 0;
        int rc;
        long long* det = nb ? mgx_det_scratch(nb, stream, &rc) : (rc = MGX_OK, nullptr);
        if (rc != MGX_OK) return rc;
        for (int i = 0; det && i < rg.n; ++i)
            if (rg.gb[i]) { rg.detb[i] = det; det += rg.N[i]; }
        mgx_gemm::ring_dw(rg, M, (float*)workspace, stream);
        for (int i = 0; i < rg.n; ++i)
            if (rg.detb[i]) launch_det_fold(rg.detb[i], rg.gb[i], (size_t)rg.N[i], 1.f, 1, (hipStream_t)stream);
        MGX_CHECK_LAUNCH("mgx_linear_dw_grouped");
    }
    if (p.nrest && mgx_deterministic()) {          // the grouped 128 x 128 kernel adds with fp32 atomics: one deterministic launch per weight
        for (int i = 0; i < p.nrest; ++i)
            if (int rc = mgx_linear_dw(p.rest[i].dY, p.rest[i].X, p.rest[i].gW, p.rest[i].gb, M, p.rest[i].N, p.rest[i].K, stream))
                return rc;
    } else if (p.nrest) {
        mgx_gemm::tile128_dw_grouped(p.rest, p.nrest, M, stream);
        MGX_CHECK_LAUNCH("mgx_linear_dw_grouped");
    }
    return MGX_OK;
}

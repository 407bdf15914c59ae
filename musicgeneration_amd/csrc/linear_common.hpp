// What the GEMM sources share.  linear.hip holds the C entry points, their argument checks and the routing; each kernel family lives in
// a file of its own with its launchers: linear_tile128.hip (128 x 128 tiles, any shape), linear_ring.hip (256 x 256 persistent LDS-DMA
// ring, the big projections of an encoder block), linear_skinny.hip (M <= 32, the decode path).
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "rel_attn_common.hpp"
#include "mgx.h"

// A/B knobs (MGX_GEMM_RING, MGX_RING4, MGX_DW_RING4) exist in experiment builds only
// (`_build.py --variant NAME --experiments`, -DMGX_EXPERIMENTS=1): the product library reads no environment variable.
// tests/test_gpu_ring.py builds such a variant to run the ring and the 128 x 128 kernels on the same inputs.
#ifndef MGX_EXPERIMENTS
#define MGX_EXPERIMENTS 0
#endif
static inline int gemm_knob(const char* name, int unset) {
#if MGX_EXPERIMENTS
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
#else
    (void)name;
    return unset;
#endif
}

MGX_DEV int xcd_remap(int bid, int nwg) {    // bijective: one XCD walks a contiguous run of tiles
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8, idx = bid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// One launch of the ring weight-gradient kernels: the weights that take it, and the M-split plan (linear.hip: dw_plan)
struct DwRing {
    const uint16_t* dY[MGX_DW_MAX_GROUP];
    const uint16_t* X[MGX_DW_MAX_GROUP];
    float* gW[MGX_DW_MAX_GROUP];
    float* gb[MGX_DW_MAX_GROUP];
    long long* detb[MGX_DW_MAX_GROUP];                     // deterministic mode: fixed-point images of the bias-gradient updates (else NULL)
    int N[MGX_DW_MAX_GROUP], K[MGX_DW_MAX_GROUP];
    int first_tile[MGX_DW_MAX_GROUP + 1];                  // prefix sums of the 256 x 256 tile counts
    int n, splits, steps_per_split;
    int ragged;                                            // some weight does not tile into whole 256 x 256 tiles (four-wave kernel only)
};

// The launchers the entry points of linear.hip call.  Each sets the attributes of its kernels once and launches on `stream`; the
// arguments have been checked and the family chosen by the caller, which also checks the launch.
namespace mgx_gemm {
void skinny_fwd(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* C, int M, int N, int K, int act, void* stream);
void tile128_fwd(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* C, int M, int N, int K, int act, void* stream);
void tile128_dx(const uint16_t* dY, const uint16_t* W, const uint16_t* relu_y, const uint16_t* addend, uint16_t* dX, int M, int N, int K,
                void* stream);
// detW / detb: the fixed-point scratch of deterministic mode, or NULL
void tile128_dw(const uint16_t* dY, const uint16_t* X, float* gW, float* gb, int M, int N, int K, long long* detW, long long* detb,
                void* stream);
void tile128_dw_grouped(const mgx_dw_problem* problems, int count, int M, void* stream);
// four: the four-wave kernel with the generated tile statement, else the eight-wave one; grid: persistent workgroups; btrans: dX
void ring_gemm(bool four, bool btrans, int grid, const uint16_t* A, const uint16_t* B, const float* bias, const uint16_t* relu_y,
               const uint16_t* addend, uint16_t* C, int M, int NO, int R, int act, void* stream);
void ring_dw(const DwRing& g, int M, float* workspace, void* stream);       // the units, then the fix-up pass
}  // namespace mgx_gemm

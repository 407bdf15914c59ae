/* mgx.h -- C ABI of libmgx.so: the MI355X (gfx950) kernels of the Music Transformer hot path.
 *
 * The reference (SJTMusicTeam/MusicGeneration) has no native/FFI layer: its hot path is a
 * sequence of ATen ops inside torch.nn.Module classes.  Each entry point below replaces one such
 * op sequence; the reference lines it replaces are cited per function (paths relative to
 * mg/model/MusicTransformer/).  INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked "host".
 *  - the caller owns all buffers; the library allocates nothing and keeps no state.
 *  - all launches are asynchronous on `stream` (a hipStream_t passed as void*); capturable.
 *  - bf16 tensors are uint16_t storage (round-to-nearest-even), row-major, innermost dim last.
 *  - return value: MGX_OK (0) or a negative mgx_status; mgx_last_error() gives a message.
 *  - dh (head dim) is fixed at 64 and heads = d/64, as in the reference (layers.py:219).
 */
#ifndef MGX_H
#define MGX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MGX_OK = 0,
    MGX_ERR_SHAPE = -1,    /* unsupported shape (message says which constraint) */
    MGX_ERR_NULL = -2,     /* required pointer is NULL */
    MGX_ERR_LAUNCH = -3,   /* hipGetLastError() != hipSuccess after launch */
    MGX_ERR_NO_DEVICE = -4 /* no HIP device visible */
} mgx_status;

/* thread-local, NUL-terminated description of the last failure on this thread */
const char* mgx_last_error(void);
/* library/ABI version (bumped on any signature change) */
int mgx_abi_version(void);   /* 2: mgx_rel_attn_bwd takes a workspace; 3: mgx_linear_dx takes an addend; 4: mgx_linear_dw_grouped; 5: GRU training ops; 6: sampler grammar mask; 7: mgx_linear_ln_fwd; 8: mgx_rel_attn_fwd/_weights take a workspace; 9: mgx_rel_attn_decode takes a workspace (split-K); 10: mgx_linear_dw_grouped takes a workspace; 11: decode K/V caches are head-major [B,h,Lmax,64]; 12: mgx_decode_embed_linear, mgx_rel_attn_decode_splits; attention partials are 68 floats (acc[64], m, l, 2 pad); 13: mgx_rel_attn_bwd_parts: dK/dV stores the dS tiles, bits 1/3 read them, bit 5 = dQ by recomputation; 14: mgx_gru_step_fwd/bwd, mgx_gru_step_x_fwd, fragment-ordered weights (*_frag), mgx_rel_attn_fwd_nomask; 15: the sampler over rows [row0, row0+B) of a larger batch; 16: mgx_smooth_ce_bwd takes a device-side scale, mgx_pad_bitmap a flag, mgx_set_deterministic; 17: mgx_rel_attn_bwd_parts bit 6; 18: mgx_pad_bitmap's flag records LEADING pads only, mgx_stream_create_cu_mask / mgx_stream_set_cus / mgx_stream_cus / mgx_stream_destroy, mgx_set_deterministic_stream, mgx_linear_kernel_id; 19: per-row decode positions (ragged prompts); 20: 8-bit (fp8 e4m3fn) K/V cache: mgx_kv_store_fp8, mgx_rel_attn_decode_fp8; 21: re-anchored decode window: the sampler's base, mgx_decode_reanchor; 22: beam search on the KV-cache decode: mgx_beam_select, mgx_kv_beam_reorder, mgx_beam_backtrack; 23: scheduled sampling for Event_Melody_RNN: mgx_gru_step_x_fwd_save, mgx_dropout_bf16_at, mgx_gru_next_event; 24: scoring: mgx_token_logprob, mgx_linear_logprob, mgx_score_reduce; 25: global gradient-norm clipping and the non-finite-step guard: mgx_grad_norm, mgx_adam_step_clipped; 26: N samples per prompt over a shared prompt K/V cache: mgx_rel_attn_decode_shared, mgx_rel_attn_decode_shared_splits, mgx_rel_attn_decode_shared_workspace; 27: per-row length budgets on the KV-cache decode: mgx_budget_mask, mgx_budget_account; 28: per-row held-note state on the KV-cache decode: mgx_notes_mask, mgx_notes_account, mgx_notes_keep, MGX_NOTE_WORDS; 29: train-time augmentation on the device: mgx_crop_augment; 30: one step-position convention (pos_dev, base_dev, per_row) and one entry point per decode operation: the _ragged, _rows and _window entry points of ABI 15 / 19 / 20 / 21 are gone, their namesakes take per_row (the sampler also row0 and base_dev; mgx_decode_reanchor takes per_row next to its counters); 31: repetition control on the KV-cache decode: mgx_repeat_penalty, MGX_REPEAT_MAX_WINDOW, MGX_REPEAT_MAX_NGRAM; 32: draft-and-verify decode: mgx_lookahead_draft, mgx_rel_attn_decode_multi (with _splits and _workspace), mgx_lookahead_accept, MGX_LOOKAHEAD_MAX_T, MGX_LOOKAHEAD_MAX_NGRAM; 33: per-class temperature, top-k and top-p on the KV-cache decode: mgx_class_logits, MGX_CLASS_MAX; 34: entropy-aware sampling on the KV-cache decode (min-p, typical, Mirostat v2): mgx_entropy_mask, mgx_entropy_account; 35: AdamW per parameter group, frozen parameters and a weight EMA in the Adam sweep: mgx_adam_step_groups */
#define MGX_ABI_VERSION 35
/* number of visible HIP devices, or a negative mgx_status */
int mgx_device_count(void);

/* ---- deterministic-reduction mode (ABI 16)                               SURVEY 5.2 / 8c "DP N-GPU vs 1-GPU"
 * The sums that cross workgroups -- dE (mgx_rel_attn_bwd), the dW / db of mgx_linear_dw (the vocabulary projection), the bias
 * gradients of mgx_linear_dw_grouped, the embedding gradient (mgx_embed_bwd) and the four statistics of mgx_smooth_ce_fwd --
 * end in fp32 atomics, so their last bits depend on the order in which workgroups arrive.  After
 * mgx_set_deterministic(scratch, bytes) those kernels add 64-bit FIXED-POINT integers (value * 2^30, each partial sum rounded
 * once) into `scratch` and a fold pass converts the totals: integer addition is associative, so two runs on the same inputs
 * -- and a data-parallel run against a single-process run of the same global batch, up to the all-reduce's own order -- give
 * the same bits.  Partial sums are quantised to 2^-30 ~ 9.3e-10 (a FIXED quantum: an element whose partials are of magnitude m
 * keeps log2(m) + 30 bits -- tests/test_gpu_fullsize.py::test_deterministic_mode_at_the_bench_shape states the bound) and must
 * stay below 2^31 ~ 2.1e9 in magnitude: a partial that is NaN, infinite or larger POISONS its destination -- the fold writes NaN
 * there, as it does for a total outside +-2^31 -- so a diverging run stays recognisable from its loss and gradients.  The poison
 * is sticky (ABI 18): it lives in a word of its own, only ever OR-ed, never in the sum that later partials keep adding to.  The
 * cfg2 training step takes 1.1 % longer.  Everything else in the library is deterministic as it is.
 *   scratch: device memory, EXACTLY 32 MiB used, aligned to 32 MiB (ABI 18: sums in the lower 16 MiB -- 2 M destinations, the
 *            largest user needs max(N*K + N, V*d, 64*L) of them, cfg4: 1.8 M -- and each sum's poison word at the same offset in
 *            the upper 16 MiB, so that no kernel needs a second pointer), owned by the caller and alive until the mode is
 *            switched off with mgx_set_deterministic(NULL, 0).
 *   PROCESS-GLOBAL STATE -- the one exception to "every entry point is stateless and takes its stream" (SURVEY 8b): (a) the
 *   setting applies to all threads and all model instances of the process, (b) switching it while such a call is in flight is
 *   undefined, (c) the scratch registered here serves the calls of ONE stream at a time (two streams sharing it would zero / fold
 *   each other's partial sums): every FURTHER stream that issues such calls -- the CU-masked side stream of the backward's
 *   off-critical-path kernels, below -- registers a buffer of its own with mgx_set_deterministic_stream (ABI 18); a stream
 *   without one uses the buffer registered here.                                                                        */
#define MGX_DET_SCRATCH_BYTES 33554432   /* the 32 MiB above: size and alignment of every scratch */
int mgx_set_deterministic(void* scratch, size_t bytes);
int mgx_deterministic(void);          /* 1 while a scratch is registered */
/* ABI 18: a scratch of its own for the calls issued on `stream` (same requirements as above; NULL forgets it).  The mode must be
 * on (mgx_set_deterministic); switching the mode off forgets every per-stream buffer.                                    */
int mgx_set_deterministic_stream(void* stream, void* scratch, size_t bytes);

/* ---- CU-masked streams (ABI 18)                      the backward of layers.py:152-161 as train.py:265-277 drives it; SURVEY 8e
 * A training step is half MFMA-bound kernels (attention dK/dV and forward, the QKV / output-projection GEMMs) and half kernels
 * at the HBM rate, some of which feed only the optimiser (dE, the weight gradients): they can run BESIDE the critical path
 * instead of inside it -- if the two are kept on disjoint CUs, since workgroups of two unrestricted streams are dispatched
 * one kernel after the other.  The same mask keeps CUs free for RCCL's kernels under data parallelism.
 *   mgx_stream_create_cu_mask: *stream = a new HIP stream (hipExtStreamCreateWithCUMask) restricted to the CUs whose bits are
 *     set in mask[0 .. words-1].  Bit i is the driver's logical CU i: consecutive bits go round the XCDs first, then round the
 *     shader engines of an XCD, so "the low n bits" = n/8 CUs of every XCD (tools/cumask_probe.hip prints the mapping of a box).
 *   mgx_stream_set_cus / mgx_stream_cus: the number of CUs the library assumes for `stream` (set by the call above; settable for
 *     a stream created elsewhere; 0 forgets; an unknown stream = the whole device).  The persistent GEMM kernels launch one
 *     workgroup per CU of the stream they run on and plan their M-splits for that many.
 *   mgx_stream_destroy: forgets the stream (CU count, deterministic scratch) and destroys it.                            */
int mgx_stream_create_cu_mask(void** stream, const uint32_t* mask, int words);
int mgx_stream_set_cus(void* stream, int cus);
int mgx_stream_cus(void* stream);
int mgx_stream_destroy(void* stream);

/* ---- K1: token embedding * sqrt(d) + sinusoid PE (+dropout)      layers.py:226-229, 22-39 ----
 * tok int32 [rows] (rows = B*L), table f32 [V,d], pe f32 [L,d] (precomputed once, device resident),
 * out bf16 [rows,d].  dropout: keep-prob 1-p, inverted scaling; mask is a pure function of
 * (seed, element index) so the backward regenerates it.  p == 0 disables it.                  */
int mgx_embed_pe_fwd(const int32_t* tok, const float* table, const float* pe, uint16_t* out,
                     int B, int L, int d, int V, float p_drop, uint64_t seed, void* stream);
/* dtable f32 [V,d] += scatter-add of dout bf16 [rows,d] (per vocabulary row and token range one block-wide sum, added with
 * one fp32 atomic per element: the order of those few adds, hence the last bits, may differ between runs) */
int mgx_embed_bwd(const int32_t* tok, const uint16_t* dout, float* dtable,
                  int B, int L, int d, int V, float p_drop, uint64_t seed, void* stream);

/* ---- A3: key-padding bitmap from tokens                          utils.py:58-83 --------------
 * bits uint32 [B, L/32]: bit (j&31) of word j>>5 set iff tok[b,j] == pad.  L % 32 == 0.
 * flag (ABI 16; device uint32[1] or NULL): bit 0 is OR-ed in, and never cleared, when a row STARTS with a pad token and holds a
 *   real token later (ABI 18; until then: any pad followed by a real token).  Only leading padding creates queries whose
 *   visible keys are all padding; such a query has no defined result in the reference (softmax of -1e9 + x in fp32,
 *   layers.py:99-102) and is outside the parity contract, so the host side reads this flag at its next synchronisation point
 *   and refuses such input (no host sync on the hot path).  Trailing and interior pads are masked as keys exactly like the
 *   reference's look-ahead mask does (utils.py:58-83) and are accepted.                                                  */
int mgx_pad_bitmap(const int32_t* tok, uint32_t* bits, uint32_t* flag, int B, int L, int pad, void* stream);

/* ---- K3+K4: fused relative global attention (Shaw/Huang skewing)  layers.py:86-106,111-133 ---
 * qkv bf16 [B,L,3d]: columns [0,d)=Q, [d,2d)=K, [2d,3d)=V, head hd at columns hd*64..hd*64+63
 *     (exactly the output of one fused [d -> 3d] projection; no permute is needed).
 * E   bf16 [M,64] relative embedding of this layer (shared by heads and batch), M >= L.
 * padbits uint32 [B,L/32] from mgx_pad_bitmap, or NULL for "no key padding".
 * ctx bf16 [B,L,d] (heads merged: the input of the `fc` projection), lse f32 [B,h,L].
 *   logit[i,j] = (q_i.k_j + q_i.E[M-1-(i-j)])/8 ; j>i masked ; padded keys get -1e9 ;
 *   ctx_i = softmax_j(logit) v_j.  The L x L matrix is never materialised.
 * Constraints: d % 64 == 0, L % 32 == 0, M >= L.
 * Rows whose every key j<=i is padding (leading pads; never produced by the reference's data
 * path, data.py:96-107) attend uniformly over j<=i (the reference's result there is a rounding
 * artefact of -1e9+x in fp32 and is outside the parity contract).                             */
/* workspace: caller-provided scratch, 256-byte aligned, >= mgx_rel_attn_fwd_workspace(L) bytes (a copy of E in
 * the order the MFMA lanes consume it, rebuilt by a pre-pass on every call: 128*L bytes).                    */
size_t mgx_rel_attn_fwd_workspace(int L);
int mgx_rel_attn_fwd(const uint16_t* qkv, const uint16_t* E, const uint32_t* padbits,
                     uint16_t* ctx, float* lse, void* workspace, size_t ws_bytes,
                     int B, int L, int d, int M, void* stream);
/* The reference's SAMPLING call Decoder(x, mask=None) (network.py:60-62): every query attends to every key j < Lk (no look-ahead, no
 * padding mask), the relative term is what _qe_masking + _skewing leave of it: q_i.E[M-1-(i-j)] for j <= i, 0 for j > i.  Lk <= L =
 * real length of the window; rows / keys Lk..L-1 only pad it to a multiple of 32.  Inference only.                          */
int mgx_rel_attn_fwd_nomask(const uint16_t* qkv, const uint16_t* E, uint16_t* ctx, float* lse, void* workspace, size_t ws_bytes,
                            int B, int L, int Lk, int d, int M, void* stream);
/* eval/debug output of the reference (`attention_weights`, layers.py:102,109): weights f32 [B,h,L,L] =
 * softmax rows recomputed from qkv and the lse of mgx_rel_attn_fwd.  The caller zero-fills `weights`
 * first (tiles above the diagonal are not visited); masked entries inside visited tiles are written as 0. */
int mgx_rel_attn_weights(const uint16_t* qkv, const uint16_t* E, const uint32_t* padbits, const float* lse,
                         float* weights, void* workspace, size_t ws_bytes, int B, int L, int d, int M, void* stream);
/* backward of the above (autograd of layers.py:86-106).  dctx bf16 [B,L,d] -> dqkv bf16 [B,L,3d];
 * dE f32 [M,64] is ACCUMULATED into (caller zeroes it once per optimiser step).
 * workspace: caller-provided scratch, 256-byte aligned, >= mgx_rel_attn_bwd_workspace(B,L,d) bytes
 * (rowsum(dctx*ctx) [B,h,L] f32, two lane-ordered bf16 copies of E, and the causal half of dS by (query tile, key tile)
 * in 32x32 bf16 tiles that the dK/dV kernel leaves for the dQ and dE kernels -- B*h*(L/32)(L/32+1)/2 * 2 KB,
 * 0.55 GB at cfg2/B=16). */
size_t mgx_rel_attn_bwd_workspace(int B, int L, int d);
int mgx_rel_attn_bwd(const uint16_t* qkv, const uint16_t* E, const uint32_t* padbits,
                     const uint16_t* ctx, const uint16_t* dctx, const float* lse,
                     uint16_t* dqkv, float* dE, void* workspace, size_t ws_bytes,
                     int B, int L, int d, int M, void* stream);
/* same, running only the selected sub-kernels, in this order inside one call:
 *   bit0 (1)  pre-pass: delta = rowsum(dctx*ctx), E re-layout
 *   bit2 (4)  dK + dV; stores every dS tile in the workspace (L % 128 == 0: the 64-keys-per-wave kernel whose sweep is a generated,
 *             hand-scheduled gfx950 asm block, csrc/rel_attn_dkv64.hip; any other L: the 32-key HIP kernel)
 *   bit6 (64) dK + dV by the 32-key HIP kernel whatever the shape (instead of bit2: cross-check, the two give the same bits)
 *   bit1 (2)  dQ from the dS tiles a bit2 run (this call or an earlier one) left in the SAME workspace
 *   bit5 (32) dQ by full recomputation instead (independent of the stored tiles: cross-check; not together with bit1)
 *   bit3 (8)  dE from the stored dS tiles
 *   bit4 (16) dE by full recomputation (independent of the stored tiles: cross-check)
 * bench.py times each kernel on its own this way.  parts == 15 is mgx_rel_attn_bwd.                     */
int mgx_rel_attn_bwd_parts(const uint16_t* qkv, const uint16_t* E, const uint32_t* padbits,
                           const uint16_t* ctx, const uint16_t* dctx, const float* lse,
                           uint16_t* dqkv, float* dE, void* workspace, size_t ws_bytes,
                           int B, int L, int d, int M, int parts, void* stream);

/* ---- K6: out = LayerNorm(dropout(x) + res) * gamma + beta, eps    layers.py:154-155,159-160 --
 * x,res,out bf16 [rows,d]; gamma,beta f32 [d]; mean,rstd f32 [rows] saved for the backward.
 * mean is the fp32 sum divided by d (a correctly rounded division): a row whose elements are all equal has mean = that
 * value, rstd = 1/sqrt(eps) and out = beta exactly.                                              */
int mgx_add_ln_fwd(const uint16_t* x, const uint16_t* res, const float* gamma, const float* beta,
                   uint16_t* out, float* mean, float* rstd, int rows, int d, float eps,
                   float p_drop, uint64_t seed, void* stream);
/* dout bf16 [rows,d] -> dx (grad of x, dropout applied), dres (grad of res) bf16 [rows,d];
 * dgamma,dbeta f32 [d] are ACCUMULATED into; dxsum f32 [d] (or NULL) += column sums of dx, i.e. the bias
 * gradient of the projection that produced x.  dx may alias dres when p_drop == 0.
 * workspace: caller scratch >= mgx_add_ln_bwd_workspace(rows,d) bytes (per-block column partials).  */
size_t mgx_add_ln_bwd_workspace(int rows, int d);
int mgx_add_ln_bwd(const uint16_t* dout, const uint16_t* x, const uint16_t* res, const float* gamma,
                   const float* mean, const float* rstd, uint16_t* dx, uint16_t* dres,
                   float* dgamma, float* dbeta, float* dxsum, void* workspace, size_t ws_bytes,
                   int rows, int d, float p_drop, uint64_t seed, void* stream);

/* ---- K9+K10: label-smoothed cross entropy + accuracy              criterion.py:43-67, metrics.py:22-60
 * logits bf16 [rows,ld] (row stride ld >= V elements; columns >= V are ignored), target int32 [rows].
 * stats f32 [4] is ACCUMULATED into: [0]=sum of per-row loss over target!=pad, [1]=#target!=pad,
 *   [2]=#(argmax==target) over ALL rows, [3]=rows.   argmax int32 [rows] (LogitsBucketting).
 * row_lse f32 [rows] is saved for the backward.                                               */
int mgx_smooth_ce_fwd(const uint16_t* logits, const int32_t* target, float* stats, int32_t* argmax,
                      float* row_lse, int rows, int V, int ld, float eps_ls, int pad, void* stream);
/* dlogits bf16 [rows,ld] (columns >= V written as 0) = g/stats[1] * (softmax - q') for target!=pad rows, else 0, where
 * g = gscale * (gscale_dev ? *gscale_dev : 1): the upstream gradient of the scalar loss -- a host constant (1/accum) times,
 * optionally, a device-side f32 scalar (autograd's grad_output, the data-parallel loss weight): both are read on the device,
 * as stats is (no host sync, no extra elementwise pass over dlogits) (ABI 16).  stats[1] is the count the call is GIVEN (it
 * includes whatever the caller accumulated before); when it is 0 -- every target is pad -- dlogits is all zeros, never NaN. */
int mgx_smooth_ce_bwd(const uint16_t* logits, const int32_t* target, const float* stats,
                      const float* row_lse, uint16_t* dlogits, int rows, int V, int ld,
                      float eps_ls, int pad, float gscale, const float* gscale_dev, void* stream);

/* ---- K11: Adam over one flat fp32 parameter buffer                train.py:143, criterion.py:81-87
 * p,g,m,v f32 [n]; shadow bf16 [n] (the bf16 copy the GEMMs/attention read) written in the same
 * pass.  step >= 1 (bias correction as torch.optim.Adam), gscale multiplies g (e.g. 1/world).   */
int mgx_adam_step(float* p, const float* g, float* m, float* v, uint16_t* shadow, size_t n,
                  float lr, float beta1, float beta2, float eps, int step, float gscale, void* stream);
/* ---- K11b (ABI 25): clip the global gradient norm on the device; skip a non-finite step        torch.nn.utils.clip_grad_norm_
 * mgx_grad_norm measures g f32 [n] (16-byte aligned) and leaves, in *state, the factor the following mgx_adam_step_clipped
 * multiplies g by -- no host round trip, no allocation, no synchronisation (capturable); two launches, no atomics:
 *   1. min(max(ceil(n/4/256), 1), MGX_GRAD_NORM_PARTS) blocks (a function of n only); block b writes workspace[b] = the sum of
 *      g[i]^2 over its share.  Every square is formed IN FP64 (exact for fp32 inputs) and every addition is fp64, in a fixed
 *      order: the result is bit-reproducible whatever mgx_set_deterministic says, the relative error of the sum of n
 *      non-negative terms is <= (n-1) 2^-53 in any order, squares of 1e25 or 1e-30 neither overflow nor vanish, and the sum is
 *      non-finite IF AND ONLY IF some g[i] is +-inf or NaN.
 *   2. one block: sum = the partials written, in index order; norm = sqrt(sum) * |gscale|, all in fp64.
 *        norm finite:  coef = min(1, max_norm / (norm + 1e-6))       (clip_grad_norm_'s formula, in fp64)
 *                      scale = (float)((double)gscale * coef)        rounded once;  skipped_last = 0;  n_clipped += (coef < 1)
 *        otherwise:    scale = 0;  skipped_last = 1;  n_skipped += 1
 *      norm is stored either way (a non-finite one says what was met).
 *   gscale is the factor the gradient is scaled by anyway (mgx_adam_step's gscale, e.g. 1/world): the norm is that of g * gscale
 *   (a gscale that is itself inf or NaN makes the norm non-finite: the step is skipped).
 *   max_norm > 0; +inf = measure and guard, never clip (coef = 1, scale == gscale bit for bit); <= 0 or NaN: MGX_ERR_SHAPE.
 *   workspace: double [MGX_GRAD_NORM_PARTS], caller-owned, 8-byte aligned; only the first `blocks` entries are written.
 *   state: 32 bytes, 8-byte aligned, ZEROED ONCE by the caller; the counters then run over the calls.  Nothing else is written. */
typedef struct {
    double norm;           /* sqrt(sum g^2) * |gscale| of the last call, before clipping */
    float scale;           /* what mgx_adam_step_clipped multiplies g by: gscale * coef, or 0 for a skipped step */
    uint32_t skipped_last; /* 1: the last call met a non-finite gradient */
    uint64_t n_clipped;    /* calls with coef < 1 */
    uint64_t n_skipped;    /* calls with a non-finite norm */
} mgx_clip_state;
#define MGX_GRAD_NORM_PARTS 1024
int mgx_grad_norm(const float* g, size_t n, float gscale, float max_norm, double* workspace, mgx_clip_state* state,
                  void* stream);
/* mgx_adam_step with gscale = state->scale, read on the device (one uniform load at kernel entry): the same per-element code,
 * bc1 and bc2s from the host's `step` as in mgx_adam_step -- with max_norm = +inf and finite gradients the result is
 * BIT-IDENTICAL to mgx_adam_step(..., step, gscale).  If state->skipped_last is set the kernel returns before its first store:
 * p, m, v and shadow keep their bits.  `step` counts optimiser CALLS, skipped ones included (the bias correction of the step
 * after a skipped one is that of step + 1): a device-side counter would cost the host a read for every state_dict.        */
int mgx_adam_step_clipped(float* p, const float* g, float* m, float* v, uint16_t* shadow, size_t n, float lr, float beta1,
                          float beta2, float eps, int step, const mgx_clip_state* state, void* stream);
/* ---- K11c (ABI 35): decoupled weight decay, frozen parameters and a moving average of the weights, in the same sweep
 * torch.optim.AdamW with param_groups, torch.optim.swa_utils.AveragedModel
 * The flat buffer is cut into chunks of 64 elements; group_of uint8 [ceil(n / 64)] names the group of each (a caller that places
 * every parameter at a multiple of 64 elements never has two parameters in a chunk), lr_scale and weight_decay f32 [n_groups],
 * 1 <= n_groups <= 256, hold the groups' settings; all three are DEVICE arrays.  Per element of a chunk of group k, with
 * s = lr_scale[k] and w = weight_decay[k], everything in fp32 and in torch.optim.AdamW's order:
 *   s == 0, or group_of >= n_groups (outside the contract; the byte is then never used as an index):
 *           the element is FROZEN -- nothing is stored for it, neither p, m, v, shadow nor ema
 *   else    p <- p * (1 - lr s w);  mgx_adam_step's update with lr s in place of lr;  shadow <- bf16(p) if shadow;
 *           ema <- ema_decay * ema + (1 - ema_decay) * p (the new p) if ema
 * The gradient scale is gscale if state == NULL, else state->scale read on the device, and a set state->skipped_last makes the
 * kernel return before its first store (mgx_adam_step_clipped's rule; ema keeps its bits too).  shadow and ema may be NULL.
 * With one group (1, 0) and ema == NULL the result is BIT-IDENTICAL to mgx_adam_step (state == NULL) and to
 * mgx_adam_step_clipped (state given): p * (1 - 0) is exact and the per-element code is shared.
 * MGX_ERR_NULL: p, g, m, v, group_of, lr_scale or weight_decay is NULL.  MGX_ERR_SHAPE: n == 0, step < 1, n_groups outside
 * 1 .. 256, ema given and ema_decay outside [0, 1), p / g / m / v / ema not 16-byte aligned, shadow / state not 8-byte aligned,
 * a table not 4-byte aligned.  Nothing is launched then.  Same grid as mgx_adam_step; no atomics.                         */
int mgx_adam_step_groups(float* p, const float* g, float* m, float* v, uint16_t* shadow, float* ema, size_t n,
                         float lr, float beta1, float beta2, float eps, int step, float gscale,
                         const mgx_clip_state* state,
                         const uint8_t* group_of, const float* lr_scale, const float* weight_decay, int n_groups,
                         float ema_decay, void* stream);
/* shadow bf16 [n] = round(p f32 [n]): nearest even, subnormals kept, +-inf kept, NaN -> a NaN (payload unspecified) */
int mgx_cast_bf16(const float* p, uint16_t* shadow, size_t n, void* stream);

/* ---- K2/K5/K7/K8: C = act(A @ W^T + bias)                         layers.py:71-84,108,157-158; network.py:39
 * A bf16 [M,K] row-major, W bf16 [N,K] row-major (torch.nn.Linear layout), bias f32 [N] or NULL,
 * C bf16 [M,N].  act: 0 none, 1 ReLU.  K % 64 == 0, N % 4 == 0 (pad the weight rows, as the
 * vocabulary projection does); M arbitrary (edge tiles are masked).
 * Epilogue contract, the same in every kernel family (tests/test_gpu_gemm_kernels.py): the sum is accumulated in fp32, the bias
 * is added and the ReLU applied IN FP32, then the value is rounded to bf16 ONCE, to nearest even.  The ReLU PROPAGATES NaN:
 * a NaN pre-activation of either sign gives NaN (a diverged run stays recognisable), +inf gives +inf, -inf and -0 give +0.
 * Nothing outside C's M x N elements is written, nothing outside A, W, bias is read.                                    */
int mgx_linear_fwd(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* C,
                   int M, int N, int K, int act, void* stream);

/* decode-size fusion (M <= 32, K <= 1024): Z bf16 [M,K] = LayerNorm(X + RES) (layers.py:154-155,159-160 in eval mode,
 * eps as given) and C bf16 [M,N] = act(Z W^T + bias) in one launch -- the LayerNorm of a decode step rides in the
 * projection that consumes it.                                                                         */
int mgx_linear_ln_fwd(const uint16_t* X, const uint16_t* RES, const float* gamma, const float* beta, float eps,
                      const uint16_t* W, const float* bias, uint16_t* C, uint16_t* Z, int M, int N, int K, int act,
                      void* stream);

/* Decode-step fusion (ABI 12; M <= 32 rows): H bf16 [M,K] = table[tok]*sqrt(K) + pe[t] (layers.py:226-229) and
 * C bf16 [M,N] = H W^T + bias in one launch (the embedding rides in the first QKV projection of a decode step).
 * pos_dev, per_row: "Step positions" under K12 below, for the M rows.                                                   */
int mgx_decode_embed_linear(const int32_t* tok, const float* table, const float* pe, const int32_t* pos_dev, int per_row,
                            const uint16_t* W, const float* bias, uint16_t* C, uint16_t* H, int M, int N, int K, int V,
                            void* stream);
/* The three decode-size projections with the weight in MFMA FRAGMENT ORDER (see the fused GRU step below for the layout; rows
 * zero-padded to a multiple of 32): a wave load of weights is 1 KB contiguous instead of 32 bytes of 32 different rows.   */
int mgx_skinny_fwd_frag(const uint16_t* A, const uint16_t* Wf, const float* bias, uint16_t* C, int M, int N, int K, int act,
                        void* stream);                                    /* M <= 32 only: MGX_ERR_SHAPE otherwise (a fragment-ordered
                                                                           * weight must never reach mgx_linear_fwd) */
int mgx_linear_ln_fwd_frag(const uint16_t* X, const uint16_t* RES, const float* gamma, const float* beta, float eps,
                           const uint16_t* Wf, const float* bias, uint16_t* C, uint16_t* Z, int M, int N, int K, int act,
                           void* stream);
int mgx_decode_embed_linear_frag(const int32_t* tok, const float* table, const float* pe, const int32_t* pos_dev, int per_row,
                                 const uint16_t* Wf, const float* bias, uint16_t* C, uint16_t* H, int M, int N, int K, int V,
                                 void* stream);

/* backward of the above (autograd of the same reference lines):
 * dX bf16 [M,K] = dY bf16 [M,N] @ W bf16 [N,K]; if relu_y (bf16 [M,K]) is given, dX is zeroed where
 * relu_y <= 0 (the backward of a ReLU fused into the producer of this layer's input); if addend
 * (bf16 [M,K]) is given it is added last -- the gradient arriving over the residual connection
 * (layers.py:155,160: out = LN(x + branch(x))) joins the branch's input gradient without a separate pass.
 * N % 8 == 0, K % 8 == 0.
 * Epilogue contract, the same in every kernel family: the fp32 product is ROUNDED to bf16 (nearest even); the mask KEEPS an
 * element iff relu_y > 0 as an IEEE comparison (so +0, -0, negative values, -inf and NaN of either sign zero it, the smallest
 * subnormal and +inf keep it) and writes +0 otherwise; the addend is added to that bf16 value in fp32 and the sum is rounded
 * to bf16 ONCE MORE.  With no addend the output is the (masked) first rounding.                                          */
int mgx_linear_dx(const uint16_t* dY, const uint16_t* W, const uint16_t* relu_y, const uint16_t* addend,
                  uint16_t* dX, int M, int N, int K, void* stream);
/* gW f32 [N,K] += dY^T @ X (dY bf16 [M,N], X bf16 [M,K]); gb f32 [N] += column sums of dY (or NULL).
 * Both ACCUMULATE (fp32 atomics), so gradient accumulation over micro-batches needs no extra pass. */
int mgx_linear_dw(const uint16_t* dY, const uint16_t* X, float* gW, float* gb,
                  int M, int N, int K, void* stream);
/* ABI 18: which kernel family mgx_linear_fwd (kind 0: C [M,N], reduction K) or mgx_linear_dx (kind 1 / 2 / 3: no epilogue
 * operand / ReLU mask / residual addend; kind 4: both, which always takes the 128 x 128 kernel; dX [M,K], reduction N)
 * launches for this shape on `stream` -- no launch, no device access.  For tests and profiles: which of the binary's GEMM kernels a measured or checked call really ran.              */
#define MGX_GEMM_SKINNY 0    /* M <= 32: weight-streaming kernel */
#define MGX_GEMM_TILE128 1   /* 128 x 128 tiles, four waves */
#define MGX_GEMM_RING8 2     /* 256 x 256 tiles, persistent LDS-DMA ring, eight waves */
#define MGX_GEMM_RING4 3     /* 256 x 256 tiles, four waves, generated asm tile statement */
int mgx_linear_kernel_id(int kind, int M, int N, int K, void* stream);
/* the same for up to MGX_DW_MAX_GROUP weights whose dY / X share the row count M (the four projections of one
 * encoder block, layers.py:152-161), in one launch: fewer M-splits fill the chip, so less atomic traffic.  */
#define MGX_DW_MAX_GROUP 8
typedef struct mgx_dw_problem {
    const uint16_t* dY;   /* bf16 [M,N] */
    const uint16_t* X;    /* bf16 [M,K] */
    float* gW;            /* f32 [N,K], accumulated */
    float* gb;            /* f32 [N], accumulated, or NULL */
    int N, K;
} mgx_dw_problem;
/* workspace: caller scratch >= mgx_linear_dw_grouped_workspace(problems, count, M) bytes, 16-byte aligned (fp32 partial
 * tiles of the M-splits; 0 when the group runs on the tiled kernel, NULL is accepted then).  With M >= 4096, M % 32 == 0,
 * the weights whose N x K fills its 256 x 256 tiles to 60 % or more (N, K % 8 == 0; a ragged last tile row / column is
 * allowed: the vocabulary projection 448 x 512) take the split-then-fix-up path -- one fp32 partial tile per (tile, M-split)
 * in the workspace, added into gW in split order by a second pass, no fp32 atomics on gW; a group of ONE weight is the way
 * to send a single large weight gradient (mgx_linear_dw's shapes) down that path.                                         */
size_t mgx_linear_dw_grouped_workspace(const mgx_dw_problem* problems, int count, int M);
int mgx_linear_dw_grouped(const mgx_dw_problem* problems, int count, int M, void* workspace, size_t ws_bytes,
                          void* stream);

/* ---- K12: autoregressive decode with a KV cache (replaces the per-token full-window recompute of
 * network.py:52-77; causal semantics).  The step's position lives in device memory so that one captured
 * graph of a whole step can be replayed for every token.
 *
 * Step positions -- the one convention of every decode call that reads a position (ABI 30):
 *   pos_dev   device int32: t, the position of the step's input token.  per_row == 0: ONE counter, pos_dev[0], shared by the
 *             call's rows.  per_row != 0: int32 [B], one position per row (B = the call's rows; M for the fused embedding), so
 *             one batch continues prompts of different lengths; row b computes exactly what the shared call computes with
 *             pos_dev[0] = pos_dev[b].
 *   base_dev  where the call takes one: device int32 of pos_dev's shape, or NULL for 0.  Past max_seq a row's cache holds a
 *             WINDOW of its sequence (mgx_decode_reanchor): t is the position inside the window and base the column of
 *             out_tokens that holds window position 0.  base + t is the ABSOLUTE step and, where tokens are written, the output
 *             column.  A base of zeros gives the result of NULL bit for bit.  Embedding and attention work inside the window
 *             and take no base.
 *   The arguments come in one order: pos_dev, base_dev, per_row (pos_dev, per_row without a base).
 *   Contract (not checked: the values live on the device): 0 <= t < Lmax <= M for the attention, t < the rows of pe for the
 *   embedding, 0 <= base + t and base + t + 1 < out_ld for the sampler when out_tokens is given.
 *
 * mgx_decode_embed: out bf16 [B,d] = table[tok]*sqrt(d) + pe[t]            (layers.py:226-229)          */
int mgx_decode_embed(const int32_t* tok, const float* table, const float* pe, const int32_t* pos_dev, int per_row,
                     uint16_t* out, int B, int d, int V, void* stream);
/* qkv_new bf16 [B,3d] (projection of the token at position t): k_t, v_t are appended to
 * kcache/vcache bf16 [B,h,Lmax,64] (head-major: the workgroup of (b,h) streams one contiguous run of 128-byte rows)
 * at row t, then ctx bf16 [B,d] = softmax_j((q.k_j + q.E[M-1-(t-j)])/8) v_j
 * over j = 0..t.  t < Lmax <= M.                                                                      */
/* Long caches are split over several workgroups per (b,h) whose partial results a second kernel merges: workspace =
 * caller scratch >= mgx_rel_attn_decode_workspace(B, Lmax, d) bytes (0 for short caches: NULL is accepted then).  The splits
 * are a function of the shapes; with per-row positions a short row may leave whole splits empty (the merge skips them).  */
size_t mgx_rel_attn_decode_workspace(int B, int Lmax, int d);
/* key splits per (b,h) for this cache length (1 = no workspace, no merge launch).                                    */
int mgx_rel_attn_decode_splits(int B, int Lmax, int d);
int mgx_rel_attn_decode(const uint16_t* qkv_new, uint16_t* kcache, uint16_t* vcache, const uint16_t* E,
                        const int32_t* pos_dev, int per_row, uint16_t* ctx, void* workspace, size_t ws_bytes,
                        int B, int Lmax, int d, int M, void* stream);
/* logits bf16 [B,ld] -> next_tok int32 [B] drawn from softmax(logits/temperature) restricted to the top_k
 * most likely ids (0 = all) and then to the smallest set whose mass reaches top_p (1 = all).
 * Both cuts are thresholds on the probability -- top-k keeps {p >= tau} for the largest tau with count(p >= tau) >= top_k,
 * top-p then the largest tau with mass(p >= tau) >= top_p * (the mass top-k kept) -- so ids whose probabilities are EQUAL
 * are kept or dropped together: a tie across the k-th value keeps more than top_k ids.  The draw is the first kept id, in id
 * order, whose inclusive CDF reaches u * (kept mass).
 * With s = base + t, the absolute step: out_tokens int32 [B,out_ld] (or NULL): column s+1 receives the token; probs_out
 * f32 [B,V] (or NULL) receives the unfiltered softmax.  The draw is a pure function of (seed, s, row0 + row): the call's rows
 * are rows [row0, row0+B) of a larger batch (every pointer addresses the sub-batch's first row), so a batch sampled in several
 * independent sub-batches (KV-cache decode runs them on separate streams, each with its own pos_dev) gets the tokens the whole
 * batch would get.  advance != 0: every entry of pos_dev += 1 after sampling (base_dev is never written).  V <= 1024.
 * allow_table (optional, NULL = none): uint32 [V, ceil(V/32)] grammar mask -- bit v of row t set iff token v may follow
 * token t (t = the token next_tok holds on entry); disallowed logits are -inf before temperature/top-k/top-p.  A grammar row
 * that leaves no finite logit (it allows nothing, or only ids whose logit is -inf) is ignored for that draw.     */
int mgx_sample_topk_topp(const uint16_t* logits, int V, int ld, float temperature, int top_k, float top_p,
                         uint64_t seed, int32_t* pos_dev, const int32_t* base_dev, int per_row, int32_t* next_tok,
                         int32_t* out_tokens, int out_ld, float* probs_out, int B, int row0, int advance,
                         const uint32_t* allow_table, void* stream);

/* ---- 8-bit K/V cache (ABI 20): the decode attention over caches that hold OCP fp8 e4m3fn codes (not the fnuz variant).
 * kcache, vcache: uint8 [B,h,Lmax,64] codes; kscale, vscale: float [B,h,Lmax], one scale per (b,h,row).  An element is
 * float(code) * scale.  A row x of 64 bf16 values is quantized with all arithmetic in f32:
 *   amax = max |x_i|;
 *   amax == 0:  scale = 0, every code 0;
 *   otherwise:  inv = 448.0f / amax (IEEE division), code_i = e4m3fn(x_i * inv) rounded to nearest even, scale = amax / 448.0f
 *               (x_i * inv never rounds above 448, so no code is NaN).
 * mgx_kv_store_fp8: rows 0..n-1 of the K and V columns (d..2d-1, 2d..3d-1) of qkv bf16 [B,Lrows,3d] are quantized into cache
 *   rows 0..n-1 (n <= Lrows, n <= Lmax; n = 0 does nothing); the other rows are not touched.                              */
int mgx_kv_store_fp8(const uint16_t* qkv, int Lrows, int n, uint8_t* kcache, uint8_t* vcache,
                     float* kscale, float* vscale, int B, int Lmax, int d, void* stream);
/* mgx_rel_attn_decode over the 8-bit cache: k_t, v_t of qkv_new are quantized as above and appended at row t, and row t enters
 * this call already quantized, so ctx is exactly softmax_j((q.k~_j + q.E[M-1-(t-j)])/8) v~_j over the dequantized rows
 * k~_j, v~_j, j = 0..t.  q, E and ctx stay bf16.  The key splits, workspace and partials are those of mgx_rel_attn_decode
 * (mgx_rel_attn_decode_workspace / _splits cover both).                                                                 */
int mgx_rel_attn_decode_fp8(const uint16_t* qkv_new, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                            const uint16_t* E, const int32_t* pos_dev, int per_row, uint16_t* ctx, void* workspace,
                            size_t ws_bytes, int B, int Lmax, int d, int M, void* stream);

/* ---- Re-anchored decode window (ABI 21): the KV-cache decode past max_seq.  A row's cache holds a window of its sequence
 * ("Step positions" above: pos_dev and base_dev of one shape), and every `hop` tokens the window drops its oldest hop tokens,
 * renumbers the rest from 0 and rebuilds their K/V in one full-sequence pass.
 * mgx_decode_reanchor, in stream order: t' = pos_dev - hop and base' = base_dev + hop replace pos_dev and base_dev (every entry),
 * then the prefill's token matrix seq int32 [B,n_pad] is filled from the moved window: seq[b,i] = out_tokens[b, base'_b + i]
 * for i < t'_b and pad_token elsewhere (out_tokens int32 [B,out_ld]; base_dev is required).  The counters move in a launch of
 * their own before seq is filled, so no workgroup reads a position another has already moved.  hop >= 0 (0 only fills seq).
 * Contract (not checked: the counters live on the device): t'_b >= 0 and base'_b + t'_b < out_ld; a column outside
 * out_tokens is not read (seq gets pad_token there).                                                                    */
int mgx_decode_reanchor(int32_t* pos_dev, int32_t* base_dev, int per_row, const int32_t* out_tokens, int out_ld, int32_t* seq,
                        int n_pad, int hop, int pad_token, int B, void* stream);

/* ---- Beam search on the KV-cache decode (ABI 22).  R = B * K rows: row r = b * K + k is beam k (0 <= k < K <= 16) of prompt b.
 * A step runs the decode chain with per-row positions on all R rows (pos_rows int32 [R]; the K beams of a prompt always hold one
 * position), then
 * mgx_beam_select in place of the sampler, then mgx_kv_beam_reorder once per cache tensor; mgx_beam_backtrack ends the search.
 *
 * mgx_beam_select: the K best of the K * V one-token expansions of every prompt's beams.
 *   logits bf16 [R,ld]: only columns < V are read.  V <= 1024, K <= min(16, V), temperature > 0.
 *   score f32 [B,K], in/out: the sum of log-probabilities of beam k; -inf marks a DEAD beam (it has no expansions).
 *   tok int32 [R], in/out: in, every beam's last token (read only for allow_table); out, slot j's chosen token.
 *   parent int32 [R], out: the LOCAL index 0..K-1 of the beam that slot j extends.
 *   pos_rows int32 [R]: t, the position of the step's input token, the same for the K rows of a prompt (the kernel reads row
 *     b * K); advance != 0 adds 1 to each of the R entries.
 *   hist_tok, hist_parent int32 [R,out_ld]: column t + 1 of row b * K + j receives slot j's token and parent; no other column
 *     is written.  Contract (not checked on the host: t lives on the device): 0 <= t + 1 < out_ld; outside it nothing is stored.
 *   allow_table (optional, NULL = none): the sampler's grammar mask uint32 [V, ceil(V/32)], the row taken by the beam's own
 *     tok (clamped to 0..V-1), under the sampler's rule: disallowed logits are -inf, and a grammar row that leaves no finite
 *     logit is ignored for that beam.
 * Definition, all arithmetic in f32.  For a live beam k and an id v, with x = logit * (1 / temperature):
 *     logp[k,v] = x[k,v] - logsumexp over the allowed ids of x[k,.]          (-inf for a disallowed id)
 *     cand[k,v] = score[k] + logp[k,v]                                        (-inf for every v of a dead beam)
 *   stochastic == 0: key = cand.   stochastic != 0: key = cand + g with g = -log(-log(min(u, 1 - 2^-24))) and u the sampler's
 *   counter-based uniform of (seed, t, (b * K + k) * 1024 + v) -- the same hash, with that number as its row.
 *   Slots j = 0..K-1 receive the K candidates of largest key among those with cand > -inf, in descending order of key; exactly
 *   equal keys are ordered by the smaller flat index k * V + v.  A candidate with cand = -inf is never chosen.  Slot j gets
 *   tok = v, parent = k and score = cand[k,v] -- the UNPERTURBED sum also when stochastic.
 *   With only n < K finite candidates, slots n..K-1 get slot 0's token and parent and score -inf: they stay dead.  (n = 0, a
 *   prompt whose beams are all dead: every slot keeps beam 0's token, parent 0, score -inf.)
 *   One workgroup per prompt; a beam's own K best are found first (it cannot contribute more), so K * K candidates are merged. */
int mgx_beam_select(const uint16_t* logits, int V, int ld, float temperature, float* score, int32_t* tok, int32_t* parent,
                    int32_t* pos_rows, int32_t* hist_tok, int32_t* hist_parent, int out_ld, int B, int K, int advance,
                    const uint32_t* allow_table, int stochastic, uint64_t seed, void* stream);
/* mgx_kv_beam_reorder: every slot takes over its parent's cache rows.  src, dst: ONE cache tensor [R,heads,Lmax] whose elements
 * are rows of row_bytes bytes -- 128 (bf16 K or V), 64 (fp8 codes) or 4 (the fp8 scales) -- in two DIFFERENT buffers, both
 * 16-byte aligned.  With n_r = pos_rows[r] clamped to 0..Lmax (as it stands when the kernel runs: after the select's advance
 * these are the rows the step's attention has filled) and p_r = parent[r] clamped to 0..K-1:
 *     dst[r, h, 0..n_r) = src[(r / K) * K + p_r, h, 0..n_r)         for every r < R, h < heads, bit for bit.
 * Rows >= n_r of dst and all of src are not written.  The grid is sized from (R, heads, Lmax), never from the device-side n.  */
int mgx_kv_beam_reorder(void* dst, const void* src, const int32_t* parent, const int32_t* pos_rows, int R, int K, int heads,
                        int Lmax, int row_bytes, void* stream);
/* mgx_beam_backtrack: the token sequence of every final beam.  hist_tok, hist_parent int32 [R,out_ld] as mgx_beam_select left
 * them after `steps` steps whose first wrote column c0_rows[r] (int32 [R], the same for the K rows of a prompt).  For row
 * r = b * K + k:  cur = k;  for s = steps-1 .. 0:  out[r, c0 + s] = hist_tok[b * K + cur, c0 + s], then
 * cur = hist_parent[b * K + cur, c0 + s] (clamped to 0..K-1).  out int32 [R,out_ld]: only columns c0 .. c0 + steps - 1 are written
 * (the prompt columns are the caller's); a row with c0 < 0 or c0 + steps > out_ld is left alone.  One thread per row.           */
int mgx_beam_backtrack(const int32_t* hist_tok, const int32_t* hist_parent, const int32_t* c0_rows, int32_t* out, int out_ld,
                       int R, int K, int steps, void* stream);

/* ---- Shared prompt cache (ABI 26): N samples per prompt over ONE copy of the prompt's K/V.  R = Bp * N rows: row r = b * N + n
 * is sample n (0 <= n < N <= MGX_SHARED_MAX_N) of prompt b.  Per layer two pairs of bf16 tensors:
 *   kpre, vpre [Bp,h,Lpre,64]: the prompt cache, one per prompt, written by the prefill only -- this call never writes it;
 *   kown, vown [R,h,Lown,64]:  what every row has appended itself, from row 0 on.
 * pre_rows int32 [Bp]: p_b, the prompt-cache rows of prompt b.  Logical key j of row r is kpre[b,h,j] for j < p_b and
 * kown[r,h,j - p_b] for j >= p_b.  pos_rows int32 [R], one position per row (per_row != 0 above); the N rows of a prompt hold ONE position (the
 * kernel reads row b * N), as the K beams of mgx_beam_select do.
 * mgx_rel_attn_decode_shared: with t = pos_rows[b * N] and p = pre_rows[b], row r's k_t, v_t (qkv_new bf16 [R,3d]) are stored at
 *   kown / vown[r,h,t - p], and ctx bf16 [R,d] = softmax_j((q_r.k_j + q_r.E[M-1-(t-j)])/8) v_j over the logical keys j = 0..t
 *   (key t is read from qkv_new).  It is what mgx_rel_attn_decode with per_row != 0 computes on R rows whose caches are the prompt rows
 *   followed by the own rows, with a prompt's key, value and E row loaded once for MGX_SHARED_NQ queries at a time.
 * Contract: 0 <= p <= min(t, Lpre), t - p < Lown, t < M; Lpre >= 1 and Lown >= 1 (p = 0: everything lives in the own cache;
 *   p = t: the own cache holds the new key only).  t and p live on the device and are not checked on the host; the kernel
 *   checks them, and no value turns into an access outside the buffers the shapes describe: a prompt whose (t, p) break the
 *   contract leaves both caches untouched and its N rows of ctx unspecified.
 * Key splits: a function of the shapes only (the call stays capturable) -- 1 while Lpre + Lown < 1024, else doubled up to
 *   16 while the workgroups of a split, Bp * h * ceil(N / MGX_SHARED_NQ), times the splits stay below 1024 and a share holds
 *   512 keys or more.  Ranges are those of mgx_rel_attn_decode over the logical keys 0..t, so a range may straddle p; the
 *   partials are its 68-float records at [(r * h + head) * splits + split] and its merge kernel serves unchanged.
 *   workspace >= mgx_rel_attn_decode_shared_workspace() bytes (0 for one split: NULL is accepted then).                       */
#define MGX_SHARED_MAX_N 16
#ifndef MGX_SHARED_NQ        /* an A/B build of the library may set another (profiles/r20_shared_prompt_decode.txt) */
#define MGX_SHARED_NQ 2      /* queries per workgroup: N > MGX_SHARED_NQ takes ceil(N / MGX_SHARED_NQ) workgroups per (b, head, split) */
#endif
int mgx_rel_attn_decode_shared_splits(int Bp, int N, int Lpre, int Lown, int d);
size_t mgx_rel_attn_decode_shared_workspace(int Bp, int N, int Lpre, int Lown, int d);
int mgx_rel_attn_decode_shared(const uint16_t* qkv_new, const uint16_t* kpre, const uint16_t* vpre, uint16_t* kown,
                               uint16_t* vown, const uint16_t* E, const int32_t* pos_rows, const int32_t* pre_rows,
                               uint16_t* ctx, void* workspace, size_t ws_bytes, int Bp, int N, int Lpre, int Lown, int d, int M,
                               void* stream);

/* ---- Length budgets (ABI 27): every row of the KV-cache decode generates to a budget of its own -- seconds, bars, anything a
 * table over the vocabulary can price -- and ends on its own.  The state lives on the device, so both calls are captured with the
 * step:  cost int32 [V] (>= 0: what every id costs),  remaining int32 [B] (what row b may still spend; INT32_MAX = no budget),
 * done int32 [B] (0 = live),  count int32 [B] (the events row b has kept).  A row is LIVE while done[b] == 0, and the two calls keep
 * live => remaining[b] > 0.  A step is: logits, mgx_budget_mask, the sampler with advance != 0, mgx_budget_account.
 * mgx_budget_mask, in place on the step's logits bf16 [B,ld] before the sampler: for a live row, logits[b,v] = -inf (0xFF80) for
 *   every v < V with cost[v] > remaining[b].  Rows with done[b] != 0, columns >= V and every other id are left bit for bit.  The
 *   mask is in the logits themselves, so it holds under top-k / top-p and under the sampler's grammar -- also when a grammar row
 *   leaves no finite logit and is ignored.  (An id of cost 0 is never masked.)  One workgroup per row.
 * mgx_budget_account, after the sampler and its advance.  The sampler has just written next_tok[b] to column
 *   col = base + t of out_tokens int32 [B,out_ld] ("Step positions", K12), t as it stands AFTER the advance.  For a live row, with
 *   c = cost[next_tok[b]]:  remaining[b] -= c, then
 *     remaining[b] > 0:   count[b] += 1, the row stays live;
 *     remaining[b] <= 0:  done[b] = 1 (after the mask this is remaining[b] == 0, and c > 0).  inclusive != 0: the token stays
 *                         and count[b] += 1 -- the row lands exactly on its budget (seconds).  inclusive == 0: the token is
 *                         dropped, out_tokens[b,col] = next_tok[b] = pad_token -- it closes what the budget counts and is not
 *                         part of it (the N-th new `bar`).
 *   For a row with done[b] != 0 on entry: out_tokens[b,col] = next_tok[b] = pad_token; its state is not touched.
 *   Neither call moves a position: an ended row keeps stepping on pad tokens beside the others, so the shared counter, the
 *   per-row step and mgx_decode_reanchor's t' >= 0 hold as they do without budgets.  Plain loads and stores, no atomics: the host
 *   reads `done` between replays.  One thread per row.
 * Contract (not checked: the values live on the device): 0 <= next_tok[b] < the entries of cost (a negative id costs 0);
 *   a column outside 0..out_ld-1 is not written.                                                                           */
int mgx_budget_mask(uint16_t* logits, int V, int ld, const int32_t* cost, const int32_t* remaining, const int32_t* done, int B,
                    void* stream);
int mgx_budget_account(int32_t* next_tok, int32_t* out_tokens, int out_ld, const int32_t* pos_dev, const int32_t* base_dev,
                       int per_row, const int32_t* cost, int32_t* remaining, int32_t* done, int32_t* count, int pad_token,
                       int inclusive, int B, void* stream);

/* ---- Held-note state (ABI 28): every row of the KV-cache decode carries the set of notes it holds, so the sampler can be kept
 * to well-formed streams -- no note_off of a silent pitch, no note_on of a sounding one -- and to a cap on polyphony.  The state
 * lives on the device, so both calls are captured with the step:  rule int32 [V]: rule[v] = +(k+1): id v SETS bit k (a note_on
 * of key k), -(k+1): id v CLEARS bit k (its note_off), 0: id v touches no bit; 0 <= k < 32 * MGX_NOTE_WORDS, and a value outside
 * -128 .. 128 counts as 0 in both calls.  state int32 [B, MGX_NOTE_WORDS]: bit k of row b lives in word k >> 5 at bit k & 31.
 * A step is: logits, (mgx_budget_mask,) the sampler's first draw, mgx_notes_mask, the sampler, mgx_notes_keep, (mgx_budget_account,)
 * mgx_notes_account.
 * mgx_notes_mask, in place on the step's logits bf16 [B,ld] before the sampler, with n_b = popcount(state[b]) as the call finds it:
 *   for every v < V with a set-rule:    logits[b,v] = -inf (0xFF80) if the bit is set or n_b >= max_on;
 *   for every v < V with a clear-rule:  logits[b,v] = -inf if the bit is clear.
 *   Ids with rule 0, columns >= V, rule and state are left bit for bit.  1 <= max_on <= 128; 128 is no cap (a set-rule id of a
 *   clear bit is then always allowed).  The mask is in the logits themselves, so it holds under top-k / top-p.  Where every bit
 *   with a set-rule has a clear-rule and the reverse, the mask never empties a row that had a finite logit on those ids: a set
 *   bit's clear id stays, with no bit set every set id stays (max_on >= 1), and rule-0 ids always stay.  One workgroup per row.
 * mgx_notes_account, after the sampler (and after mgx_budget_account, whose pad_token then freezes an ended row: its rule is 0):
 *   tok = next_tok[b]; for 0 <= tok < V, rule[tok] = +(k+1) sets bit k of state[b] and -(k+1) clears it, whatever the bit was --
 *   no validity check, so the state is the fold of the rules over the tokens behind an unmasked sampler too: a bit is set iff the
 *   last token that touched it set it.  Any other tok and rule 0 leave the row as it is.  Writes nothing but state.  Plain loads
 *   and stores, no atomics.  One thread per row.
 * mgx_notes_keep makes a constrained row the unconstrained row of the same seed for as long as that one is legal.  The sampler
 *   draws by inverse CDF, so a draw from the masked logits differs from the unmasked draw of the same random number even where
 *   the latter was legal.  The step therefore draws twice: FIRST from the logits as they stand before mgx_notes_mask, with the
 *   call's seed, into first_tok int32 [B] (no advance, no column written); then mgx_notes_mask; then from the masked logits with
 *   ANOTHER seed, into next_tok and its column, with the advance.  mgx_notes_keep then, for every row whose first_tok[b] = t is
 *   legal -- 0 <= t < V and mgx_notes_mask, as called with this state and max_on, does not ban t -- writes next_tok[b] = t and
 *   out_tokens[b, col] = t, col = base + pos as in mgx_budget_account (the column the second draw was written to; out_tokens
 *   NULL or a column outside 0..out_ld-1: not written).  Other rows keep the second draw.  With independent random numbers the
 *   token has exactly the masked distribution when neither top_k nor top_p cuts: p(t) + p(banned) p(t) / (1 - p(banned)).
 *   Under top-k / top-p the first draw is filtered from the unmasked, the second from the masked logits; the token is legal
 *   either way.  Reads state, writes next_tok and that column only.  One thread per row.
 * MGX_ERR_NULL for a NULL pointer, MGX_ERR_SHAPE unless B > 0, V > 0 (mask: ld >= V; mask, keep: 1 <= max_on <= 128).
 * Contract (not checked: the values live on the device): rule has at least V entries.                                      */
#define MGX_NOTE_WORDS 4
int mgx_notes_mask(uint16_t* logits, int V, int ld, const int32_t* rule, const int32_t* state, int max_on, int B, void* stream);
int mgx_notes_account(const int32_t* next_tok, const int32_t* rule, int32_t* state, int V, int B, void* stream);
int mgx_notes_keep(const int32_t* first_tok, int32_t* next_tok, int32_t* out_tokens, int out_ld, const int32_t* pos_dev,
                   const int32_t* base_dev, int per_row, const int32_t* rule, const int32_t* state, int max_on, int V, int B,
                   void* stream);

/* ---- Repetition control (ABI 31): a presence / frequency penalty over the row's recent tokens and a no-repeat-n-gram rule, in
 * one stateless call.  The row's history is what the decode holds on the device already: out_tokens int32 [B,out_ld], the prompt
 * and every token the sampler has written, in absolute columns whatever the window does.  So there is no state to keep, stage or
 * gather, and the call is captured with the step.  Every amount is FINITE (a "banned" id gets `ban` subtracted, not -inf), so the
 * call never changes which logits of a row are finite: the sampler still ignores a grammar row that leaves no finite logit,
 * mgx_budget_mask still never masks a cost-0 id, mgx_notes_mask still never empties a row -- and where every other id is masked
 * away the banned id is what is left and is drawn.
 * A step is: logits, (mgx_budget_mask,) mgx_repeat_penalty, (the sampler's first draw, mgx_notes_mask,) the sampler,
 * (mgx_notes_keep,) (mgx_budget_account,) (mgx_notes_account) -- before the first draw, because mgx_notes_keep lets a legal first
 * draw stand: drawn from unpenalised logits it would carry most samples past the penalty.
 * mgx_repeat_penalty, in place on the step's logits bf16 [B,ld] before the sampler.  For row b, with c = base + t ("Step
 *   positions", K12), the column of the step's input token -- the row's last token: the prompt's last on the first step, afterwards
 *   the one the sampler wrote.  A row with c < 0 or c >= out_ld is left bit for bit.
 *   Counts (window > 0):  cnt[v] = the number of columns j, max(0, c - window + 1) <= j <= c, with out_tokens[b,j] == v, for
 *     0 <= v < V.  History ids outside 0..V-1 (a pad id, a negative filler) count for nothing.
 *   N-gram (ngram = n >= 2):  k = n - 1, lo = span ? max(0, c - span + 1) : 0.  If c - k + 1 >= lo, the context is
 *     out_tokens[b, c-k+1 .. c], and for every e, lo + k - 1 <= e <= c - 1, whose k columns e-k+1 .. e equal the context element
 *     by element, the follower f = out_tokens[b, e+1] is BANNED if 0 <= f < V.  The comparison is on raw int32 values, out-of-range
 *     ids included; occurrences may overlap the context (e + 1 <= c); one that begins before lo does not count.
 *   Amount, for v < V:  a[v] = ban if v is banned;  else pen[cnt[v]] if window > 0, subject[v] != 0 and cnt[v] > 0;  else none.  A
 *     banned id that is also counted gets ban, not the sum.  Where there is one, logits[b,v] = bf16(f32(logits[b,v]) - a[v]): ONE
 *     f32 subtraction rounded to nearest, then one rounding to bf16, nearest-even.  -inf stays -inf; a NaN becomes a NaN of
 *     unspecified payload.  Ids without an amount, columns >= V, out_tokens, pos_dev, base_dev, subject and pen are not written.
 *   pen float [window + 1] (pen[0] is never read) and subject int32 [V] may be NULL if and only if window == 0.
 * MGX_ERR_NULL for a NULL logits, out_tokens or pos_dev, or subject / pen missing with window > 0.  MGX_ERR_SHAPE unless B > 0,
 *   0 < V <= 1024, ld >= V, out_ld > 0;  0 <= window <= MGX_REPEAT_MAX_WINDOW;  ngram == 0 or 2 <= ngram <= MGX_REPEAT_MAX_NGRAM;
 *   span == 0 or span >= ngram;  not both window == 0 and ngram == 0;  with ngram != 0, ban finite and > 0.
 * Contract (not checked: the values live on the device): pen finite, the positions as under "Step positions".
 * One workgroup of 256 threads per row; the grid is a function of B only (no host read, no allocation).  LDS atomics on the counts
 * and the ban bitmap, no global atomics.                                                                                   */
#define MGX_REPEAT_MAX_WINDOW 4096
#define MGX_REPEAT_MAX_NGRAM  64
int mgx_repeat_penalty(uint16_t* logits, int V, int ld, const int32_t* out_tokens, int out_ld, const int32_t* pos_dev,
                       const int32_t* base_dev, int per_row, const int32_t* subject, const float* pen, int window, int ngram,
                       int span, float ban, int B, void* stream);

/* ---- Draft and verify (ABI 32): several tokens per step of the KV-cache decode, same sample    (the sampling loop of
 * network.py:52-77, T positions of it per step).  A step of B rows runs as B * T rows of the ordinary step chain: row b * T + i is
 * position t_b + i of batch row b on the guessed input draft[b,i].  Every position is then drawn with the draw the one-token step
 * makes there -- the sampler's draw is a pure function of (seed, absolute step, row) -- and the prefix whose guesses were right is
 * kept, so the result is the one-token call's sample for that seed up to the rounding difference between two attention kernels.
 * A step is: mgx_lookahead_draft, the chain on B * T rows with pos_rows as its per-row positions and mgx_rel_attn_decode_multi as
 * its attention, mgx_lookahead_accept.  2 <= T <= MGX_LOOKAHEAD_MAX_T.
 * Step positions ("Step positions", K12): pos_dev int32 [B], ALWAYS one position per row (t_b, the position of the step's input
 * token tok[b]); base_dev of the same shape or NULL, where the call takes one; s = base + t is the column of tok[b] in out_tokens.
 * No rollback is needed: position t_b + i enters the cache from draft[b,i], and i < n_b (below) means draft[b,0..i] were the tokens
 * drawn, so after a step every cache row below the new t_b was written from a verified input.  Rejected rows lie at or above the
 * new t_b and the next step rewrites them -- and reads them from its own qkv_new -- before any query can reach them.
 *
 * mgx_lookahead_draft, one launch per step.  out_tokens int32 [B,out_ld] holds the row's history, out_tokens[b,s] == tok[b].
 *   draft int32 [B,T]: draft[b,0] = tok[b].  pos_rows int32 [B*T]: pos_rows[b*T+i] = min(t_b + i, Lmax - 1) (never below 0).
 *   guide != NULL (int32 [B,guide_ld]): draft[b,i] = guide[b,s+i] where s + i < guide_ld, else pad_token (i >= 1).
 *   guide == NULL, history: for n = ngram, ngram-1, .., 1 (an n with s-n+1 < 0 is skipped) find the greatest j < s, j >= n-1, with
 *     out_tokens[b, j-n+1 .. j] == out_tokens[b, s-n+1 .. s] (raw int32 values); the first n with a match wins.  With
 *     x~[c] = out_tokens[b,c] for c <= s and x~[c] = x~[c - (s-j)] for c > s (the match extended periodically where it runs into
 *     the present), draft[b,i] = x~[s+i].  No match at any n (or s outside 1 .. out_ld-1): draft[b,i>=1] = pad_token.
 *   A draft is only a guess: any id is legal.  1 <= ngram <= MGX_LOOKAHEAD_MAX_NGRAM.  Writes draft and pos_rows only.  One
 *   workgroup of 256 threads per row, the scan of mgx_repeat_penalty's n-gram rule; LDS atomics only.
 * mgx_rel_attn_decode_multi: qkv_new bf16 [B*T,3d], row b*T+i the projection of draft[b,i] at position t_b + i.  k and v of every
 *   i with t_b + i < Lmax are appended to rows t_b + i of kcache / vcache bf16 [B,h,Lmax,64], and
 *   ctx[b*T+i] = softmax_j((q_i.k_j + q_i.E[M-1-(t_b+i-j)])/8) v_j over j = 0 .. t_b + i  (ctx bf16 [B*T,d]): query i never sees a
 *   row above t_b + i, and rows t_b .. t_b + T - 1 are read from qkv_new, never from the cache rows this launch writes.  Rows with
 *   t_b + i >= Lmax append nothing; their ctx is unspecified but finite.  One workgroup per (b, head, key split) with T
 *   online-softmax states per lane: every K and V row is loaded once for the T queries.  Key splits, partial records (at
 *   [((b*T+i) * h + head) * splits + split]) and the merge kernel are mgx_rel_attn_decode's; workspace >=
 *   mgx_rel_attn_decode_multi_workspace() bytes (0 for one split: NULL is accepted then).
 *   Contract (not checked on the host: t lives on the device): 0 <= t_b < Lmax <= M; a row outside it appends nothing and no
 *   value turns into an access outside the buffers the shapes describe.
 * mgx_lookahead_accept in place of the sampler.  logits bf16 [B*T,ld].  y_i is exactly the draw mgx_sample_topk_topp makes from
 *   row b*T+i with (seed, s+i, row0+b): the same temperature / top_k / top_p thresholds and tie rule, and the same allow_table
 *   grammar whose previous token is draft[b,i].  a = the largest k <= T-1 with draft[b,i] == y_{i-1} for all 1 <= i <= k.
 *   limit int32 [B]: the column of every row's last token; n_b = min(a + 1, limit[b] - s).
 *     n_b <= 0: the row is finished -- nothing is written, its position stays, done[b] = 1 (done int32 [B]).
 *     else:     out_tokens[b, s+1+i] = y_i for i < n_b, tok[b] = y_{n_b-1}, pos_dev[b] += n_b; probs_all f32 [B,probs_ld,V] (or
 *               NULL) receives the unfiltered softmax of row b*T+i at column s+i for i < n_b; stats int32 [B,2] (or NULL)
 *               += (1, n_b).
 *   Plain loads and stores, no atomics.  One workgroup of T waves per row.  V <= 1024.
 *   Contract (not checked: the values live on the device): limit[b] < out_ld; a column outside the matrices is not written. */
#define MGX_LOOKAHEAD_MAX_T 8
#define MGX_LOOKAHEAD_MAX_NGRAM 8
int mgx_lookahead_draft(const int32_t* tok, const int32_t* out_tokens, int out_ld, const int32_t* pos_dev,
                        const int32_t* base_dev, const int32_t* guide, int guide_ld, int ngram, int pad_token, int32_t* draft,
                        int32_t* pos_rows, int B, int T, int Lmax, void* stream);
int mgx_rel_attn_decode_multi_splits(int B, int T, int Lmax, int d);
size_t mgx_rel_attn_decode_multi_workspace(int B, int T, int Lmax, int d);
int mgx_rel_attn_decode_multi(const uint16_t* qkv_new, uint16_t* kcache, uint16_t* vcache, const uint16_t* E,
                              const int32_t* pos_dev, uint16_t* ctx, void* workspace, size_t ws_bytes, int B, int T, int Lmax,
                              int d, int M, void* stream);
int mgx_lookahead_accept(const uint16_t* logits, int V, int ld, float temperature, int top_k, float top_p, uint64_t seed,
                         int32_t* pos_dev, const int32_t* base_dev, const int32_t* draft, const int32_t* limit, int32_t* tok,
                         int32_t* out_tokens, int out_ld, float* probs_all, int probs_ld, int32_t* done, int32_t* stats, int B,
                         int T, int row0, const uint32_t* allow_table, void* stream);

/* ---- Per-class sampling (ABI 33): a temperature, a top-k and a top-p of its own for every class of ids (a codec's event types),
 * in one stateless call, in place on the step's logits bf16 [B,ld] before the sampler.  The row's distribution is sampled in two
 * stages -- the class at the call's temperature, then the id inside the class at the class's -- and the call writes the logarithm
 * of the product, so the UNCHANGED sampler, run at temperature 1, draws from it.  No state, nothing gathered; captured with the step.
 * A step is: logits, (mgx_budget_mask,) (mgx_repeat_penalty,) mgx_class_logits, the sampler or mgx_lookahead_accept at
 * temperature 1, (mgx_budget_account).  It is not combined with the two draws of the note rules (mgx_notes_mask): an in-place
 * rewrite cannot serve both.
 * mgx_class_logits.  cls int32 [V]: the class of every id, 0 <= cls[v] < C.  inv_temp float [C], top_k int32 [C], top_p float [C],
 *   all on the device.  tok int32 [B] and allow_table uint32 [V, ceil(V/32)] (both or neither): the sampler's grammar, whose
 *   previous token is tok[b] (clamped to 0 .. V-1); under draft and verify tok is the draft, one entry per logits row.
 *   For row b, with x_v = f32(logits[b,v]):
 *   Live ids:  A = {v < V: x_v > -inf, and bit v of the grammar row of tok[b] is set, if there is a table}.  A table under which A
 *     is empty is ignored for the row (A = {x_v > -inf}): the sampler's own fallback.  If A is still empty the row is left bit for
 *     bit.  NaN: unspecified.
 *   Class stage:  P_c = sum_{v in A, cls[v] = c} exp(x_v / temperature) / sum_{v in A} exp(x_v / temperature).
 *   Inside class c (A_c = {v in A: cls[v] = c} not empty):  q_v = softmax over A_c of x_v * inv_temp[c], then the thresholds and
 *     the tie rule of mgx_sample_topk_topp on q: with 0 < top_k[c] < |A_c|, tau = the largest value with #{q >= tau} >= top_k[c];
 *     with top_p[c] < 1, tau rises to the largest value with mass{q >= tau} >= top_p[c] * mass{q >= the top-k tau}.
 *     K_c = {v in A_c: q_v >= tau} (ties stay together), q'_v = q_v / sum_{K_c} q.
 *   Result:  p'_v = P_{cls[v]} q'_v on the union of the K_c.  logits[b,v] = bf16(ln p'_v) there and -inf at every other v < V whose
 *     class lies in 0 .. C-1.  ln p'_v is formed in log space, (lse_c - lse_all) at the call's temperature plus
 *     (x_v - max_{A_c} x) * inv_temp[c] - ln sum_{K_c} e, so a kept id never becomes -inf through underflow; ONE rounding to bf16,
 *     nearest-even.  A probability read back from the result is off by at most |ln p'| 2^-8 relative: the order of the bf16 logits
 *     themselves.  Columns >= V, cls, the parameter arrays, tok and the table are not written.
 * MGX_ERR_NULL for a NULL logits, cls, inv_temp, top_k or top_p, or exactly one of tok / allow_table NULL.  MGX_ERR_SHAPE unless
 *   B > 0, 0 < V <= 1024, ld >= V, 1 <= C <= MGX_CLASS_MAX, temperature finite and > 0.
 * Contract (not checked: the values live on the device): 0 <= cls[v] < C (an id of another class is not written), inv_temp finite
 *   and > 0, top_k >= 0, 0 < top_p <= 1.
 * One workgroup of C waves per row, wave c owns class c (the classes' threshold searches run side by side); ids lane + 64 i, 16
 * per lane, as in the sampler.  Every wave reads the row before the workgroup's one barrier and writes its class's ids after it.
 * The grid is a function of B only (no host read, no allocation); no LDS, no atomics.                                          */
#define MGX_CLASS_MAX 16
int mgx_class_logits(uint16_t* logits, int V, int ld, const int32_t* cls, int C, const float* inv_temp, const int32_t* top_k,
                     const float* top_p, float temperature, const int32_t* tok, const uint32_t* allow_table, int B, void* stream);

/* ---- Entropy-aware sampling (ABI 34): min-p, locally typical sampling and Mirostat v2 on the KV-cache decode (the sampling step of
 * network.py:52-77, which has a temperature alone) -- three cuts that follow the row's own uncertainty instead of falling at a
 * fixed place.  Two calls bracket the sampler, as the budget's do; both are captured with the step.
 * A step is: logits, (mgx_budget_mask,) (mgx_repeat_penalty,) (mgx_class_logits,) mgx_entropy_mask, the sampler or
 * mgx_lookahead_accept, (mgx_entropy_account,) (mgx_budget_account).  The mask and the account take the SAMPLER's temperature:
 * 1 after mgx_class_logits.  Not combined with the two draws of the note rules (mgx_notes_mask).
 * mgx_entropy_mask, in place on the step's logits bf16 [B,ld] before the sampler.  A PURE MASK: it writes -inf (0xFF80) and nothing
 *   else; every kept id, every column >= V and every id outside the live set stay bit for bit, and the sampler then runs at the
 *   call's own temperature with its own top-k / top-p.  tok int32 [B] and allow_table uint32 [V, ceil(V/32)] (both or neither):
 *   the sampler's grammar, whose previous token is tok[b] (clamped to 0 .. V-1); under draft and verify tok is the draft.
 *   For row b, with z_v = f32(logits[b,v]) * (1 / temperature), the sampler's arithmetic:
 *   Live ids:  A as in mgx_class_logits -- {v < V: z_v > -inf, and bit v of the grammar row of tok[b] is set, if there is a
 *     table}; a table under which A is empty is ignored for the row.  If A is still empty the row is left bit for bit and
 *     lse_out[b] = 0.  NaN: unspecified.
 *   lse = ln sum_A e^z, ln p_v = z_v - lse.  lse_out f32 [B] (may be NULL) receives lse.
 *   Three stages, each on the survivors of the one before:
 *   1. Mirostat cut (mu != NULL; f32 [B], read only):  S1 = {v in A: -ln p_v / ln 2 <= mu[b]}; if that is empty,
 *      S1 = {v in A: z_v = max_A z}.
 *   2. min-p (min_p > 0):  S2 = {v in S1: z_v - max_{S1} z >= ln(min_p)}.  A ratio to the maximum does not change under
 *      renormalisation, so its place in the order does not matter.
 *   3. Typical (typical_p < 1):  q = p renormalised over S2, H = -sum q ln q, d_v = |-ln q_v - H|, delta = the smallest value with
 *      mass_q{d <= delta} >= typical_p (of the mass as the kernel sums it), S3 = {v in S2: d_v <= delta}.  delta is found by exact
 *      bisection on the bit patterns of d, as the sampler finds its thresholds: ids whose d the kernel computes equal -- ids of
 *      equal logits among them -- stay together.
 *   The stages are sequential on purpose: computed on one common p, typical and min-p can have an empty intersection
 *   (p = (0.4, 0.06 x 10), min_p 0.2, typical_p 0.5).  Every v in A \ S3 becomes -inf; S3 is never empty.
 *   With mu == NULL, min_p == 0 and typical_p == 1 the call is legal and writes only lse_out.
 * MGX_ERR_NULL for a NULL logits, or exactly one of tok / allow_table NULL.  MGX_ERR_SHAPE unless B > 0, 0 < V <= 1024, ld >= V,
 *   temperature finite and > 0, 0 <= min_p < 1, 0 < typical_p <= 1.
 * One wave per row; ids lane + 64 i, 16 per lane, as in the sampler.  The grid is a function of B only (no host read, no
 * allocation); plain loads and vector stores, no LDS, no atomics.
 * mgx_entropy_account, after the sampler and its advance and BEFORE mgx_budget_account (which may replace the token by a pad).
 *   logits bf16 [B,ld] are the step's, as the mask left them; lse f32 [B] is the mask's lse_out.  For row b:
 *   s = (lse[b] - f32(logits[b,next_tok[b]]) * (1 / temperature)) / ln 2, the surprise in bits of the token that was drawn under
 *   the row's distribution BEFORE the mask (the kept logits are still there bit for bit).
 *   mu != NULL (f32 [B]):  mu[b] <- mu[b] - eta * (s - tau), every operation rounded to f32 on its own.
 *   surprise_out f32 [B,out_ld] (may be NULL) receives s at column col = base + t ("Step positions", K12), t as it stands AFTER the
 *   advance: the column the sampler has just written, as in mgx_budget_account.
 *   Nothing is written for a row whose next_tok lies outside 0 .. V-1, whose logit there is not finite, or -- with surprise_out --
 *   whose column lies outside 0 .. out_ld-1.
 * MGX_ERR_NULL for a NULL next_tok, logits, lse or pos_dev.  MGX_ERR_SHAPE unless B > 0, V > 0, ld >= V, temperature finite and
 *   > 0, out_ld > 0 where surprise_out is given, tau and eta finite where mu is given.
 * One thread per row; no atomics.                                                                                          */
int mgx_entropy_mask(uint16_t* logits, int V, int ld, float temperature, float min_p, float typical_p, const float* mu,
                     float* lse_out, const int32_t* tok, const uint32_t* allow_table, int B, void* stream);
int mgx_entropy_account(const int32_t* next_tok, const uint16_t* logits, int V, int ld, float temperature, const float* lse,
                        float* mu, float tau, float eta, float* surprise_out, int out_ld, const int32_t* pos_dev,
                        const int32_t* base_dev, int per_row, int B, void* stream);

/* ---- K13: Event_Melody_RNN step (Event_MelodyRNN/network.py:51-61): the GRU projections run on
 * mgx_linear_fwd; these two kernels are the rest of a step.
 * out bf16 [B,ld] = table bf16 [V,ld][tok] (ld = embedding width padded to a multiple of 64).          */
int mgx_gather_rows(const int32_t* tok, const uint16_t* table, uint16_t* out, int B, int ld, int V, void* stream);
/* torch.nn.GRU cell, gate order (r,z,n): gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh bf16 [B,3H];
 * h f32 [B,H] is updated in place, h_bf16 [B,H] receives its bf16 copy (input of the next projection). */
int mgx_gru_gates(const uint16_t* gi, const uint16_t* gh, float* h, uint16_t* h_bf16, int B, int H, void* stream);

/* ---- K13b: Event_Melody_RNN training (Event_MelodyRNN/network.py:63-84,109-116 SeqForward/Train; torch.nn.GRU cell).
 * The sequence's input projections are one mgx_linear_fwd per layer; per time step the recurrent projection
 * (mgx_linear_fwd, M = B) and this cell remain:  h_next f32, y bf16 [B,H] = cell(gi, gh bf16 [B,3H], h_prev f32).   */
int mgx_gru_cell_fwd(const uint16_t* gi, const uint16_t* gh, const float* h_prev, float* h_next, uint16_t* y,
                     int B, int H, void* stream);
/* backward of one step: dh = dh_direct (f32) + d_rec (bf16: step t+1's dgh @ W_hh) + dy (bf16: layer above), each
 * may be NULL; gates are recomputed from gi/gh.  Out: dgi, dgh bf16 [B,3H], dh_prev_direct f32 [B,H] = dh * z.   */
int mgx_gru_cell_bwd(const uint16_t* gi, const uint16_t* gh, const float* h_prev, const float* dh_direct,
                     const uint16_t* d_rec, const uint16_t* dy, uint16_t* dgi, uint16_t* dgh,
                     float* dh_prev_direct, int B, int H, void* stream);
/* Fused time step (ABI 14): the recurrent projection and the cell in ONE launch each way (H % 64 == 0).
 * The weights of these three entry points are bf16 in FRAGMENT ORDER: for a matrix W [N,K] (N % 32 == 0, K % 16 == 0) the
 * 16-byte unit ((nt * K/16 + ks) * 64 + lane) holds W[32 nt + lane % 32][16 ks + 8 (lane / 32) .. +7] -- what lane `lane` feeds
 * the MFMA for row tile nt and k-step ks, so a wave load is 1 KB contiguous (ops.pack_frag / melody_rnn._pack build it).
 * forward: gh = h_prev_bf16 W_hh^T + b_hh (W_hh [3H,H] in fragment order, rounded to bf16 and stored in gh_out [B,3H] for the backward),
 *          then h_next f32, y bf16 [B,H] = cell(gi, gh, h_prev) exactly as mgx_gru_cell_fwd.                               */
int mgx_gru_step_fwd(const uint16_t* gi, const uint16_t* h_prev_bf16, const float* h_prev, const uint16_t* Whh,
                     const float* bhh, float* h_next, uint16_t* y, uint16_t* gh_out, int B, int H, void* stream);
/* sampling step of one layer: gi = x W_ih^T + b_ih (x bf16 [B,Kx], W_ih [3H,Kx] and W_hh in fragment order, Kx % 64 == 0), gh as above, the cell -- one
 * launch instead of two projections + mgx_gru_gates.  NOT in place: h_next / y must differ from h_prev / h_prev_bf16.     */
int mgx_gru_step_x_fwd(const uint16_t* x, const uint16_t* Wih, const float* bih, int Kx, const uint16_t* h_prev_bf16,
                       const float* h_prev, const uint16_t* Whh, const float* bhh, float* h_next, uint16_t* y, int B, int H,
                       void* stream);
/* backward of step t: d_rec = dgh_next W_hh (dgh_next bf16 [B,3H] = step t+1's dgh, NULL at the last step; WhhT = W_hh^T
 * [H,3H] in fragment order), then mgx_gru_cell_bwd with it: dgi, dgh bf16 [B,3H], dh_out f32 [B,H] = dh * z.  final != 0: no cell,
 * dh_out = dh_direct + d_rec (the gradient of the layer's initial state; gi/gh/h_prev/dgi/dgh may be NULL).           */
int mgx_gru_step_bwd(const uint16_t* gi, const uint16_t* gh, const float* h_prev, const float* dh_direct,
                     const uint16_t* dgh_next, const uint16_t* WhhT, const uint16_t* dy, uint16_t* dgi, uint16_t* dgh,
                     float* dh_out, int B, int H, int final, void* stream);
/* inverted dropout on a bf16 buffer (nn.GRU's inter-layer dropout); stateless mask = f(seed, index): calling it on
 * the gradient with the same (p, seed) is its backward.  n % 8 == 0.                                             */
int mgx_dropout_bf16(const uint16_t* x, uint16_t* out, size_t n, float p_drop, uint64_t seed, void* stream);
/* dst f32 [V,cols] row idx[r] += src bf16 [n,ld] row r, columns 0..cols-1 (nn.Embedding backward).                */
int mgx_scatter_add_rows(const int32_t* idx, const uint16_t* src, float* dst, int n, int ld, int cols, int V,
                         void* stream);

/* ---- Scheduled sampling for Event_Melody_RNN (ABI 23): the free-running TRAINING forward of Event_MelodyRNN/train.py:221-245,
 * model.generate(..., events, teacher_forcing_ratio, output_type='logit') -> network.py:144-162.  Step t + 1 of every layer
 * depends on step t of the top layer, so the forward runs step-major: per step one mgx_gru_step_x_fwd_save per layer,
 * mgx_dropout_bf16_at between layers, the output projection, then mgx_gru_next_event, which chooses the next input of every row.
 * What it leaves behind is what the backward-through-time above reads; no gradient flows through the choice of a token.
 *
 * mgx_gru_step_x_fwd_save is mgx_gru_step_x_fwd with two more outputs, same arguments, same requirements:
 *   gi_out, gh_out bf16 [B,3H]: the bf16-rounded x W_ih^T + b_ih and h_prev_bf16 W_hh^T + b_hh the cell consumed -- the form in
 *   which mgx_gru_step_bwd reads gi and gh of the step.  h_next and y are bit for bit those of mgx_gru_step_x_fwd on the same
 *   inputs (one kernel body, a compile-time switch).  Rows >= B of no output are written.                                   */
int mgx_gru_step_x_fwd_save(const uint16_t* x, const uint16_t* Wih, const float* bih, int Kx, const uint16_t* h_prev_bf16,
                            const float* h_prev, const uint16_t* Whh, const float* bhh, float* h_next, uint16_t* y,
                            uint16_t* gi_out, uint16_t* gh_out, int B, int H, void* stream);
/* mgx_dropout_bf16 on a slice of a larger buffer.  x, out: the n elements of the slice itself (16-byte aligned), which are
 * elements index0 .. index0 + n - 1 of the buffer; n % 8 == 0, index0 % 8 == 0, 0 <= p_drop < 1.  The mask is mgx_dropout_bf16's
 * function of (seed, index0 + i), and the seed is READ FROM DEVICE MEMORY when the kernel runs (seed_dev uint64[1]), so a
 * captured launch does not bake it in.  Slices that tile a buffer give, bit for bit, what one mgx_dropout_bf16 call over the
 * whole buffer gives with the same seed: that whole-buffer call on the gradient is still the backward.                    */
int mgx_dropout_bf16_at(const uint16_t* x, uint16_t* out, size_t n, size_t index0, float p_drop, const uint64_t* seed_dev,
                        void* stream);
/* mgx_gru_next_event: the next input of every row, and its embedding.  One workgroup per row.
 *   logits bf16 [B,ld]: only columns < V are read.  0 < V <= 1024, ld >= V, temperature > 0.
 *   flag_dev int32[1], read when the kernel runs: bit 0 = this step is FORCED, bit 1 = this step is GREEDY.
 *   events int32 [B] or NULL: the ground-truth next event of every row; NULL: no step is forced, whatever bit 0 says.
 *   seed_dev uint64[1], read when the kernel runs; step: the host's step counter.
 *   emb bf16 [V,Ep], Ep % 8 == 0 (the padded embedding table of mgx_gather_rows).
 *   out: tok int32 [B], used_out int32 [B] (the same value: the running token and the record of what was fed),
 *        x_out bf16 [B,Ep] = emb[tok], bit for bit.  Nothing else is written.
 * Rule per row b:
 *   forced:              tok = events[b], clamped to 0..V-1.
 *   greedy, not forced:  the smallest id whose logit equals the row maximum (bf16 values compare exactly; -0 equals +0).  A NaN
 *                        logit never wins and never counts as the maximum; a row without any finite logit gives id 0.
 *   neither:             x_v = logit_v * (1 / temperature) in f32, p_v = exp(x_v - max x) (0 for a NaN logit, and for every id
 *                        when the maximum is not finite), mass = sum p, u = the sampler's counter-based uniform of
 *                        (seed, step, b).  tok = the first id, in id order, with p > 0 whose inclusive CDF reaches u * mass; if
 *                        rounding leaves none, the last id with p > 0; if no id has p > 0, id 0.  The CDF is summed in fp32 in
 *                        an order of the kernel's choosing: it is within V * 2^-23 * mass of the exact one.                 */
int mgx_gru_next_event(const uint16_t* logits, int V, int ld, const int32_t* flag_dev, const int32_t* events, float temperature,
                       const uint64_t* seed_dev, uint32_t step, const uint16_t* emb, int Ep, int32_t* tok, int32_t* used_out,
                       uint16_t* x_out, int B, void* stream);

/* ---- Scoring (ABI 24): the log-probability the model gives to every event of a sequence -- the log-softmax and the gather of the
 * target's entry of criterion.py:43-67 without the label smoothing, and the arg-max against the target of metrics.py:40-52.  The
 * three entry points share these rules.  All arithmetic is f32.  For row r, over the ALLOWED ids v (all ids without a grammar):
 *     x_v = logit_v * (1 / temperature),   lse = logsumexp_v x_v
 *     logp[r] = x_t - lse for t = target[r] in 0..V-1 (-inf for a disallowed t)
 *     hit[r]  = 1 if t is the SMALLEST allowed id whose logit equals the row maximum, else 0 (-0 equals +0; a NaN never wins)
 *   A row with target[r] < 0 or >= V is UNSCORED: logp = 0, hit = -1; lse_out is still written.
 *   A NaN or +inf among a row's allowed logits gives logp = lse = NaN, and so does a row whose allowed logits are all -inf: a
 *   diverged run stays recognisable.
 *   logp f32, hit int32, lse_out f32 (optional, NULL = not wanted): `rows` (M) elements each; nothing else is written.
 *
 * mgx_token_logprob: on logits that exist.  logits bf16 [rows,ld]: only columns < V are read; any V >= 1, ld >= V,
 *   temperature > 0.  allow_table and prev int32 [rows] are both given or both NULL: allow_table is the sampler's grammar mask
 *   uint32 [V, ceil(V/32)], the row taken by prev[r] clamped to 0..V-1, under the sampler's rule -- a disallowed id counts as
 *   -inf, and a table row that leaves no finite logit (the NaN-ignoring maximum over its ids is -inf) is ignored for that row.
 *   This is mgx_beam_select's logp.  hit compares the bf16 values exactly.  One wave per row.                               */
int mgx_token_logprob(const uint16_t* logits, int V, int ld, const int32_t* target, const int32_t* prev,
                      const uint32_t* allow_table, float temperature, float* logp, float* lse_out, int32_t* hit, int rows,
                      void* stream);
/* mgx_linear_logprob: the vocabulary projection fused with the above; the logits never leave the accumulators.
 *   A bf16 [M,K] (the last LayerNorm's output), W bf16 [V,K] (fc.weight), bias f32 [V] or NULL.  K % 64 == 0, 64 <= K <= 1024,
 *   V >= 1, temperature > 0; other shapes return MGX_ERR_SHAPE.
 *     x_v = (sum_k A[r,k] W[v,k] + bias_v) * (1 / temperature)
 *   with the sum accumulated in fp32 on the MFMA units, bias and scale applied in fp32: NO rounding to bf16 anywhere.  No grammar.
 *   hit compares the fp32 values and takes the smallest id among equal maxima.  Exactly V rows of W and V elements of bias are
 *   read.  A workgroup owns 32 rows of A (staged once in LDS) and walks V in tiles of 32 ids with a running
 *   (max, sum, target logit, arg-max) per row; the summation order is fixed, so two calls give the same bits.               */
int mgx_linear_logprob(const uint16_t* A, const uint16_t* W, const float* bias, const int32_t* target, float temperature,
                       float* logp, float* lse_out, int32_t* hit, int M, int V, int K, void* stream);
/* mgx_score_reduce: per-sequence totals of logp f32 [B,L] and hit int32 [B,L].  count[b] = columns with hit >= 0,
 *   hits[b] = columns with hit == 1, sum[b] (f64) = the sum of logp over the counted columns, accumulated in fp64 in a fixed
 *   order (two calls give the same bits); a counted -inf or NaN propagates.  One workgroup per row b.                       */
int mgx_score_reduce(const float* logp, const int32_t* hit, double* sum, int32_t* count, int32_t* hits, int B, int L,
                     void* stream);

/* ---- Train-time augmentation on the device (ABI 29): the crop of data.py:96-107, the transposition of utils/shared.py:36-68 as
 * PerformanceRNN/train.py:220-222 applies it, and a time stretch, in one launch.  Per row the kernel cuts a crop out of a corpus
 * that lives in device memory, stretches its time, transposes it and writes the model's x and y; no token crosses the host.
 * One workgroup per row; the source is walked in tiles, for any n >= 1.
 *
 *   corpus uint16 [corpus_len]: the pieces, one after the other.  start int64 [B], avail int32 [B]: where row b's crop begins
 *   and how many tokens lie between start[b] and the end of its piece.
 * Source.  Row b reads src[i] = corpus[start[b] + i] for i < n_src, with
 *     n_src = min(n, avail[b], corpus_len - start[b])      without a stretch (stretch_q NULL),
 *     n_src = min(2n, avail[b], corpus_len - start[b])     with one.
 *   A negative start[b] or avail[b], or start[b] >= corpus_len, gives an empty source.  No value in device memory turns into an
 *   access outside corpus[0 .. corpus_len), perm[0 .. S*V) or the elements of x / y named under "Output".
 * Stretch.  stretch_q int32 [B] in per-mille, or NULL: none.  q = stretch_q[b] if 500 <= stretch_q[b] <= 2000, else 1000.  The
 *   codec's time ids are the run ts0 .. ts0 + n_ts - 1, id ts0 + j lasting j + 1 units (ts0 >= 0, n_ts >= 1, ts0 + n_ts <= 65536;
 *   both ignored without a stretch).
 *     u_i = src[i] - ts0 + 1 if src[i] lies in the run, else 0;   T_i = u_0 + ... + u_i (64 bits);
 *     S_i = floor((T_i q + 500) / 1000),  S_{-1} = 0.
 *   A token with u_i = 0 is emitted as it is.  A time token emits delta_i = S_i - S_{i-1} units: floor(delta_i / n_ts) ids
 *   ts0 + n_ts - 1, then id ts0 + (delta_i mod n_ts) - 1 if the remainder is above 0; nothing when delta_i = 0.  The cumulative
 *   time is rounded, never the single shift: the ids emitted for src[0 .. i] last exactly S_i units, drift does not accumulate.
 *   q = 1000 emits the source.  (Six 100-unit shifts at q = 1005, n_ts = 100: S = 101 201 302 402 503 603, deltas 101 100 101 100 101 100,
 *   emitted units 100 1 100 100 1 100 100 1 100.)
 * Transposition.  perm int32 [S,V] and shift_row int32 [B], both given or both NULL (none).  Every emitted id v with 0 <= v < V
 *   becomes perm[shift_row[b] * V + v]; with shift_row[b] outside 0 .. S-1, or v >= V, the id stays as it is.
 * Output.  out[0 ..) is the emitted stream; its first n ids count.
 *     x[b*stride_b + j*stride_t] = out[j]           for j < n - 1 (y given) or j < n (y NULL)
 *     y[b*stride_b + (j-1)*stride_t] = out[j]       for 1 <= j < n
 *   x, y int32; strides (L, 1) give the transformer's [B, L] pair with L = n - 1, strides (1, B) a time-major [T, B].  Where the
 *   row emitted fewer than n ids the rest is pad_token, as it is (not transposed).  n_out int32 [B] or NULL:
 *   n_out[b] = min(emitted, n).  Nothing else is written; no input is written.
 * Length.  With q >= 500 any two consecutive source tokens emit at least one id (two time tokens of u units in all give
 *   floor or ceil of u q / 1000 >= 1 units between them), so 2n source tokens always give n ids; with q >= 1000 every source
 *   token emits at least one.  A row comes up short only where its piece ends: within n tokens of it, or within 2n for q < 1000.
 * B > 0, n > 0, V > 0, stride_b > 0, stride_t > 0, S > 0 with a table; otherwise MGX_ERR_SHAPE / MGX_ERR_NULL.  Plain loads and
 * stores, no atomics; the result is a pure function of the inputs, and every per-row value is read when the kernel runs, so a
 * captured launch follows the arrays.                                                                                       */
int mgx_crop_augment(const uint16_t* corpus, size_t corpus_len, const int64_t* start, const int32_t* avail, const int32_t* perm,
                     int S, int V, const int32_t* shift_row, const int32_t* stretch_q, int ts0, int n_ts, int32_t* x, int32_t* y,
                     int stride_b, int stride_t, int32_t* n_out, int pad_token, int B, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H */

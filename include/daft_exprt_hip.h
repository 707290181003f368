/* C ABI of libdaft_exprt_hip.so: the gfx950 kernels behind the Daft-Exprt acoustic-model forward/backward path.
 *
 * The reference (claussss/ubisoft-laforge-daft-exprt) is pure Python/PyTorch and has no FFI of its own; each entry point
 * below replaces the ATen work of one reference call site (cited per function, paths relative to
 * src/daft_exprt/).  The Python host in ubisoft_laforge_daft_exprt_amd/ binds this file with ctypes; INTEGRATION.md shows
 * the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch caching allocator); the library never allocates or frees
 *   - activations are fp32, channels-last: a (B, N, C) tensor is [B*N] rows of C floats with a leading dimension (ld*)
 *   - lens[b] (int32, device) = valid rows of batch row b; rows n >= lens[b] are padding
 *   - `stream` is a hipStream_t; all work is enqueued on it, nothing synchronises (graph-capture safe)
 *   - return value: 0 = ok, non-zero = error; dx_last_error() returns the message of the calling thread's last error
 *   - reduced precision: every entry point with a `bf16` / `*_bf16` argument (and the pack functions) also exists with the suffix
 *     `_f16` (e.g. dx_conv_gemm_f16): the same kernel built for IEEE fp16 operands and storage (v_mfma_f32_16x16x32_f16), where each
 *     of those arguments then means "fp16".  BASELINE.json config 2 runs the bf16 build, config 5 the fp16 build.
 *   - dropout: counter-based (seed, element index); the backward entry points regenerate the mask from the same seed.
 *     seed_offset (optional device scalar) is added to the seed(s) on the device: a captured HIP graph draws a new dropout
 *     stream on every replay by bumping that scalar, although the launch arguments are frozen
 */
#ifndef DAFT_EXPRT_HIP_H
#define DAFT_EXPRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ----------------------------------------------------------------------------------------------------- */
int dx_version(void);
const char* dx_last_error(void);

/* ---- host-side integer durations: DaftExprt.get_int_durations, model.py:950-973 -> duration_to_integer, extract_features.py:69-125 ----
 * HOST pointers, no GPU work.  dur: (B, L) seconds, already thresholded (values < filter_length / sampling_rate / 2 set to 0);
 * out: (B, L) frames per symbol; totals[b] = sum of row b; status[b]: 0 ok, 1 the phones ran out before the frames did (the reference
 * raises IndexError / ValueError for that utterance), 2 count mismatch (the reference's index assignment raises).  Double-precision
 * arithmetic with int() truncation, operation for operation what the reference's Python does; bit-exact. */
int dx_int_durations(const float* dur, int B, int L, int sampling_rate, int filter_length, int hop_length, int centered,
                     long long* out, long long* totals, int* status);

/* ---- Conv1d / Linear as MFMA GEMM: model.py:57-72 (LinearNorm), :75-94 (ConvNorm1D), :165-186 (MHA in/out proj) ---- */
/* dims[4] = {CoutP_fwd, CinP_fwd, CinP_bwd, CoutP_bwd}: padded sizes of the packed weights (element counts
 * taps*dims[0]*dims[1] and taps*dims[2]*dims[3]); bf16 = 0 packs f32 (exact MFMA), 1 packs bf16 */
int dx_pack_dims(int Cout, int Cin, int bf16, int* dims);
/* W: checkpoint layout (Cout, Cin, taps) fp32 -> fwd pack, bwd pack (input-gradient conv: channels transposed, taps flipped) or NULL.
 * The packs are opaque operands of dx_conv_gemm at the same precision: f32 packs are [taps][CoutP][CinP]; bf16 packs hold the
 * same zero-padded matrices fragment-major (16-row x 32-k blocks in v_mfma_f32_16x16x32_bf16 A-operand order). */
int dx_pack_weights(const float* W, void* fwd, void* bwd, int Cout, int Cin, int taps, int bf16, void* stream);
/* every layer of a model in one launch; descs = device array of n 56-byte records
 * {const float* W; void* fwd; void* bwd; int32 Cout, Cin, taps, CoutP_f, CinP_f, CinP_b, CoutP_b, pad} */
int dx_pack_weights_batched(const void* descs, int n, int bf16, void* stream);
/* the same from a HOST array of the records: the descriptors travel as kernel arguments (chunks of 60 layers) and the grid holds one
 * wave per 16 x 32 block of the whole model -- what an optimiser step is followed by (one launch for the 57 packed layers of DaftExprt) */
int dx_pack_weights_host(const void* descs, int n, int bf16, void* stream);
/* Y[b,n,:] = out_scale * mask( relu_aux>0 ? . : 0 )( post_scale * relu?( bias + conv(X) ) + post_shift )  (+= if accumulate)
 * taps 1 (Linear) or 3 (zero 'same' padding inside each batch row).  NULL disables an epilogue stage.
 * skip_halo >= 0: 128-token tiles that start at or beyond lens[b] + skip_halo are padding nobody reads: zero-filled, not computed
 * (the reference computes the whole padded grid; rows within the halo of a k=3 stack are still computed).
 * rows_exist (optional, device int32 [B]): input rows n >= rows_exist[b] of batch row b do not exist -- they read as the conv's zero
 * 'same' padding although the buffers hold N rows per batch row.  NULL: every batch row has N rows (the reference's padded grid, whose
 * N is the longest utterance: model.py:14-24).  With it, ONE allocation / captured HIP graph of N rows serves every batch whose longest
 * utterance is <= N with unchanged results (rows_exist[b] = that batch's max length), and a batch row can be made to behave as if it
 * were run alone (rows_exist[b] = lens[b]: scripts/synthesize.py:420-448 runs the accent encoder per reference wav).  Output rows
 * n >= rows_exist[b] do not exist either: they are written as zero (with accumulate: left as they are).  That makes the input-gradient
 * convolution of a bucketed training step (dY -> dX) match the same launch on the tensors cut to rows_exist[b] rows. */
int dx_conv_gemm(const void* X, int ldx, const void* Wp, const float* bias, void* Y, int ldy,
                 int B, int N, int Cin, int Cout, int taps, int bf16,
                 int relu, const float* post_scale, const float* post_shift,
                 const void* relu_aux, int ld_aux, int accumulate,
                 const int* lens, int mask_rows, float out_scale, int skip_halo,
                 int x_bf16, int y_bf16, int aux_bf16, const int* rows_exist, void* stream);
/* x_bf16 / y_bf16 / aux_bf16 = 1: that tensor is stored as bf16 (bf16 operand mode only; ld* count elements).  Used for the
 * 1024-wide hidden activations of the conv feed-forward and the prenet, whose HBM traffic otherwise bounds the step.
 * bf16 (operand mode): 0 = exact f32 (f32 pack), 1 = bf16 (bf16 pack), 2 = split bf16: fp32 storage and the f32 pack, every operand
 * split as x = hi + lo (hi = bf16_rne(x), lo = bf16_rne(x - hi), lo = 0 where hi is not finite: an inf / NaN operand makes the same
 * outputs non-finite as in mode 0, though an inf may come out as NaN; a finite |x| above bf16's largest value, 3.39e38, splits
 * as hi = inf) and each product formed as
 * hi*lo + lo*hi + hi*hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation (~16 mantissa bits).  Mode 2 needs x_bf16 = y_bf16 =
 * aux_bf16 = 0; any other value or combination is an error before any launch.  dx_conv_gemm_f16 rejects mode 2. */
/* G (fp32, caller-initialised, the parameter's OWN checkpoint layout (Cout, Cin, taps)) += dY^T * shifted X   (autograd of the conv
 * w.r.t. its weight, train.py:435 loss.backward()).  G may be a zeroed scratch gradient or a live `.grad` / all-reduce bucket view. */
int dx_conv_wgrad(const void* dY, int ldy, const void* X, int ldx, float* G,
                  int B, int N, int Cin, int Cout, int taps, const int* lens, int skip_halo,
                  int bf16, int dy_bf16, int x_bf16, float* dbias, const int* rows_exist, void* stream);
/* bf16 (operand mode): 0 = exact f32, 1 = bf16, 2 = split bf16 (as in dx_conv_gemm; needs dy_bf16 = x_bf16 = 0; the bias gradient is
 * summed from the fp32 dY, in the exact-f32 kernel's order).  dx_conv_wgrad_f16 rejects mode 2.
 * dbias (optional, caller-zeroed [Cout]): the bias gradient sum_rows dY is accumulated by the same launch from the staged dY tiles.
 * rows_exist (optional, device int32 [B], as in dx_conv_gemm): dY and X rows n >= rows_exist[b] read as zero, so nothing stored there
 * reaches G or dbias (NULL: all N rows exist). */
/* Up to 32 weight gradients of one kind (same taps, same operand storage, bf16 / fp16 operand mode, Cin % 128 == 0) in ONE launch:
 * the eight k = 3 layers of a 4-block FFT stack fill the chip at a 4-way token split instead of 16-way per layer (a quarter of the fp32
 * atomics); more layers run as further rounds of workgroups of the same launch (their atomic epilogues overlap the next round).  `jobs` is a HOST array of njobs DxWgradJob (read during the call; the descriptors travel as kernel arguments); every field
 * has the meaning of the dx_conv_wgrad argument of the same name. */
typedef struct DxWgradJob {
  const void* dY; const void* X; float* G; float* dbias; const int* lens;
  int ldy, ldx, B, N, Cin, Cout, skip_halo, reserved;
  const int* rows_exist;      /* optional, as in dx_conv_wgrad (after `reserved`: the earlier fields keep their offsets) */
} DxWgradJob;
int dx_conv_wgrad_batched(const void* jobs, int njobs, int taps, int dy_bf16, int x_bf16, void* stream);
/* ---- launch plans: which kernel a dispatcher picks for a shape, at which tile width and grid ---------------------------------------
 * Host code only: no device pointer, no stream, no HIP call (they answer on a machine without a GPU).  Each dispatcher above and below
 * calls its plan function and switches on the record, so a rule is stated once; profiling.py and the tests ask here too.  All five fill
 * one record of DX_PLAN_INTS ints (fields a family does not use are 0).  The arguments are the dispatcher's own, the scalars the
 * decision depends on; dx_ln_plan: backward != 0 plans dx_ln_bwd.  The _f16 twins answer alike and reject operand mode 2. */
#define DX_PLAN_INTS 14
#define DX_PLAN_KERNEL 0         /* one of the DX_K_* ids below */
#define DX_PLAN_TOK 1            /* tokens (conv, feed-forward pair) or rows (LayerNorm) one workgroup owns per pass */
#define DX_PLAN_GRID_X 2         /* the launch dimensions: grid x, y, z and threads per workgroup */
#define DX_PLAN_GRID_Y 3
#define DX_PLAN_GRID_Z 4
#define DX_PLAN_THREADS 5
#define DX_PLAN_SPLIT 6          /* weight gradients: split-K (== grid z) */
#define DX_PLAN_CHUNK 7          /* weight gradients: tokens per K chunk */
#define DX_PLAN_ROUNDS 8         /* batched weight gradient: rounds of workgroups */
#define DX_PLAN_SWEEP 9          /* dx_ln_fwd: rows one pass of the grid covers */
#define DX_PLAN_PASSES 10        /* dx_ln_fwd: passes of its grid-stride loop */
#define DX_PLAN_COUTP 11         /* dx_conv_gemm: the pack's padded dimensions (dims[0], dims[1] of dx_pack_dims for that mode) */
#define DX_PLAN_CINP 12
#define DX_PLAN_SWIZZLE 13       /* deep-K conv: the XCD swizzle width the grid was rounded for (0: none) */
#define DX_K_CONV_GEMM_F32 1     /* conv_gemm_kernel<float>: tiled, 64 or 128 tokens */
#define DX_K_CONV_GEMM_H16 2     /* conv_gemm_kernel<16-bit> */
#define DX_K_CONV_GEMM_SPLIT 3   /* conv_gemm_kernel<split bf16> */
#define DX_K_CONV_WS 4           /* conv_ws_kernel: weight-stationary, CinP == 128 */
#define DX_K_CONV_DK 5           /* conv_dk_kernel: deep-K, CinP >= 256 */
#define DX_K_WGRAD_F32 6         /* wgrad_kernel (also the 16-bit modes' fallback for dimensions that are no multiple of 8) */
#define DX_K_WGRAD_SPLIT 7       /* wgrad_split_kernel */
#define DX_K_WGRAD_H16 8         /* wgrad_bf16_kernel, 64 input channels per workgroup (256 threads) */
#define DX_K_WGRAD_H16_WIDE 9    /* wgrad_bf16_kernel, 128 input channels per workgroup (512 threads); every batched launch */
#define DX_K_FF_PAIR 10          /* ff_pair_kernel: 126- or 62-token tiles */
#define DX_K_LN_FWD 11           /* ln_fwd_kernel */
#define DX_K_LN_BWD 12           /* ln_bwd_kernel: THREADS / 64 waves, TOK rows per block */
int dx_conv_gemm_plan(int B, int N, int Cin, int Cout, int taps, int bf16, int ldx, int* plan);
int dx_conv_wgrad_plan(int B, int N, int Cin, int Cout, int taps, int bf16, int ldx, int ldy, int dy_bf16, int x_bf16, int* plan);
int dx_conv_wgrad_batched_plan(const void* jobs, int njobs, int taps, int dy_bf16, int x_bf16, int* plan);
int dx_ff_pair_plan(int B, int N, int* plan);
int dx_ln_plan(int B, int N, int C, int backward, int* plan);
/* Fused conv feed-forward pair (model.py:206-217 PositionWiseConvFF.forward: conv k3 128->F, ReLU, conv k3 F->128) and the
 * input-gradient chain of the same pair, bf16 MFMA operands, ONE launch; the F-wide hidden tensor is consumed from LDS.
 *   Y[b,n,:] (+)= bias_b + conv3(Wb, Hm)[b,n,:],   Hm = mid(bias_a + conv3(Wa, X)),  H <- Hm (bf16, kept for the weight gradients)
 * X [B][N][128] bf16; Wa / Wb: bf16 packs of dx_pack_weights (forward: conv1.fwd, conv2.fwd; backward: conv2.bwd, conv1.bwd);
 * mid = ReLU if relu_mid; aux (bf16 [B][N][F], optional): mid zeroes every position where aux <= 0 (ReLU backward).
 * Token tiles starting at or beyond min(lens[b] + skip_halo, N) are padding nobody reads: zero-filled (H, and Y unless accumulate). */
int dx_ff_pair(const void* X, int ldx, const void* Wa, const void* Wb, const float* bias_a, const float* bias_b,
               const void* aux, int ld_aux, void* H, int ldh, float* Y, int ldy,
               int B, int N, int F, int relu_mid, int accumulate, const int* lens, int skip_halo, const int* rows_exist, void* stream);
/* dx_ff_pair (forward) with the FFT block's SECOND LayerNorm folded into its epilogue (model.py:225-233 after :206-217): the output tile
 * is normalised while it is in LDS.  Z = res + dropout(pair output) (fp32 [B][N][128], what dx_ln_fwd leaves in `a`), Yln / mean / rstd /
 * film / seeds as in dx_ln_fwd with C = 128 and halo 0 (rows >= lens[b] are masked); lens is required; skip_halo as in dx_ff_pair (it
 * only decides which whole tiles are computed: the hidden rows of the halo are still written to H for the weight gradients). */
/* H may be NULL in the forward entry points (dx_ff_pair with relu_mid, dx_ff_pair_ln, dx_ff_pair_ln_qkv): the mid activation is then not
 * written (inference: nothing reads it; 2 KB per token saved).
 * hmask (optional; dx_ff_pair_ln / dx_ff_pair_ln_qkv write it, dx_ff_block_bwd reads it INSTEAD of aux for the ReLU gradient): the sign of
 * the hidden activation, one bit per element, as uint32 [B * ceil(N / 126)][F / 128][4][2][64] -- the kernel's own register layout, one
 * coalesced dword per lane (128 B per token instead of re-reading 2 KB of H with 8-byte strided loads in the backward's producer epilogue;
 * model.py:213 ReLU backward).  Forward and backward must use the same tile width (they do: both default to 126-token tiles). */
int dx_ff_pair_ln(const void* X, int ldx, const void* Wa, const void* Wb, const float* bias_a, const float* bias_b, void* H, int ldh, float* Z,
                  int B, int N, int F, const int* lens, int skip_halo, const int* rows_exist,
                  const float* res, const float* ln_w, const float* ln_b, const float* film, int ld_film, float* Yln, float* mean, float* rstd,
                  uint64_t seed_pre, float p_pre, const uint64_t* seed_offset, void* hmask, void* stream);
/* dx_ff_pair_ln followed, on the same tile, by the NEXT FFT block's attention in-projection (model.py:163-171, F.multi_head_attention_forward's
 * linear(x, in_proj_weight, in_proj_bias)): QKV (16-bit [B][N][384]) = Yln x Wq^T + bias_q, what dx_conv_gemm(Yln, Wq, bias_q, taps = 1,
 * lens, skip_halo = 0, y 16-bit) writes (rows >= lens[b] of a live tile = the bias; tiles beyond the halo = 0).  Wq: the forward pack of
 * the (384, 128) weight in the mode's 16-bit type. */
int dx_ff_pair_ln_qkv(const void* X, int ldx, const void* Wa, const void* Wb, const float* bias_a, const float* bias_b, void* H, int ldh, float* Z,
                      int B, int N, int F, const int* lens, int skip_halo, const int* rows_exist,
                      const float* res, const float* ln_w, const float* ln_b, const float* film, int ld_film, float* Yln, float* mean, float* rstd,
                      uint64_t seed_pre, float p_pre, const uint64_t* seed_offset, const void* Wq, const float* bias_q, void* QKV, void* hmask, void* stream);
/* dx_ff_pair (input-gradient pair, accumulate = 1) with the BACKWARD of the block's first LayerNorm folded into its epilogue: Y holds the
 * residual-branch gradient on entry and dz1 = LayerNorm-backward(Y + pair result) on return; DG (16-bit [B][N][128]) = dropout(dz1), the
 * operand of the out-projection's backward GEMMs; dw / db (caller-initialised [128]) accumulate the affine gradients.  z / mean / rstd /
 * ln_w / ln_b / seed_pre / p_pre: the arguments of dx_ln_bwd with C = 128, no FiLM, halo 0 (model.py:188-191 backward). */
int dx_ff_pair_lnbwd(const void* X, int ldx, const void* Wa, const void* Wb, const void* aux, int ld_aux, void* H, int ldh, float* Y,
                     int B, int N, int F, const int* lens, int skip_halo,
                     const float* z, const float* mean, const float* rstd, const float* ln_w, const float* ln_b, void* DG, float* dw, float* db,
                     uint64_t seed_pre, float p_pre, const uint64_t* seed_offset, void* stream);
/* The conv feed-forward half of an FFT block's backward in ONE launch (model.py:225-233, :206-217, :188-191 backward): the backward of
 * the SECOND LayerNorm as the prologue that produces the pair's input tile, the input-gradient pair, the backward of the FIRST LayerNorm as
 * its epilogue.  dY2 [B][N][128] fp32 = d(loss)/d(block output); z2 / mean2 / rstd2 / ln2_* / film / seed2 / p2 and z1 / ... / seed1 / p1:
 * the arguments of the two dx_ln_bwd calls it replaces (C = 128, halo 0); Wa / Wb / aux / H / lens / skip_halo: those of dx_ff_pair
 * (input-gradient pair).  Outputs: Y = dz1 (fp32, the residual gradient for the attention half), DG1 = dropout(dz1) and DG2 = dropout(dz2)
 * as 16 bits (operands of the out-projection's and the second conv's backward GEMMs), H = the hidden gradient; dw* / db* / dfilm accumulate.
 * Wout_bwd / DATT (optional, together): the backward pack of the attention out-projection's (128, 128) weight and a 16-bit [B][N][128]
 * output: the epilogue then also computes DATT = DG1 x W_out, the input gradient of the out-projection (what dx_attention_bwd takes as dctx).
 * rows_exist (optional, device int32 [B], as in dx_conv_gemm): rows n >= rows_exist[b] do not exist for the two convolutions and the two
 * LayerNorms: dY2 there reads as zero and every gradient row there (Y, DG1, DG2, DATT, H) is zero. */
int dx_ff_block_bwd(const float* dY2, const float* z2, const float* mean2, const float* rstd2, const float* ln2_w, const float* ln2_b,
                    const float* film, int ld_film, void* DG2, float* dw2, float* db2, float* dfilm, int ld_dfilm, uint64_t seed2, float p2,
                    const void* Wa, const void* Wb, const void* aux, int ld_aux, void* H, int ldh, float* Y,
                    int B, int N, int F, const int* lens, int skip_halo,
                    const float* z1, const float* mean1, const float* rstd1, const float* ln1_w, const float* ln1_b, void* DG1, float* dw1, float* db1,
                    uint64_t seed1, float p1, const void* Wout_bwd, void* DATT, const uint64_t* seed_offset, const void* hmask,
                    const int* rows_exist, void* stream);
/* out[c] += sum_rows X[row][c]   (bias gradients) */
int dx_colsum(const void* X, int ldx, float* out, long rows, int C, int x_bf16, void* stream);

/* ---- multi-head attention: model.py:165-186 (nn.MultiheadAttention slow path), called from :255 ------------------- */
/* order[0..B) = utterance indices sorted by length, longest first (stable): the optional `order` argument of the attention entry
 * points.  A workgroup's work grows with its utterance's length and workgroups start in blockIdx order: longest first removes the tail
 * of a launch.  Pure scheduling: results do not depend on it.  (No reference counterpart: get_mask_from_lengths, model.py:14-24, is
 * the only use the reference makes of the lengths.) */
int dx_length_order(const int* lens, int* order, int B, void* stream);
int dx_attention_fwd(const void* qkv, int ld, const int* lens, void* ctx, int ldc, float* lse,
                     int B, int N, int H, int D, uint64_t seed, const uint64_t* seed_offset, float p_drop, int bf16, int qkv_bf16, int ctx_bf16,
                     const int* order, void* stream);
/* dx_attention_fwd (16-bit q/k/v and context, 2 heads x 64) + dx_proj_ln_fwd on its result in ONE launch, bit-identical outputs: the
 * attention, out-projection, dropout, residual and first LayerNorm of an FFT block (model.py:165-191, forward).  Arguments as in the two
 * entry points (halo 0).  Every entry point with 16-bit operands also exists as <name>_f16. */
int dx_attention_proj_ln_fwd(const void* qkv, int ld, const int* lens, void* ctx, int ldc, float* lse, int B, int N, int H, int D,
                             uint64_t seed, const uint64_t* seed_offset, float p_drop,
                             const void* Wpack, const float* proj_bias, float* z, const float* res, const float* w, const float* bias,
                             const float* film, int ld_film, float* y, float* mean, float* rstd, uint64_t seed_pre, float p_pre,
                             void* y_bf16_copy, void* stream);
int dx_attention_bwd(const void* qkv, int ld, const void* ctx, const void* dctx, int ldc, const float* lse, float* delta,
                     const int* lens, void* dqkv, int ldg, int B, int N, int H, int D, uint64_t seed, const uint64_t* seed_offset, float p_drop, int bf16,
                     int qkv_bf16, int dqkv_bf16, int ctx_bf16, const int* order, void* stream);
/* bf16 = 1: QK^T / PV (and the five backward products) on v_mfma_f32_16x16x32_bf16, softmax and accumulation in fp32;
 * qkv_bf16 / dqkv_bf16 / ctx_bf16 = 1: the in-projection output / its gradient / the attention context are stored as bf16 (ld in
 * elements; ctx and dctx share ldc AND the storage type: ctx_bf16 = 1 means both are 16-bit).  The context is only ever consumed as a 16-bit GEMM operand (out-projection, its weight gradient)
 * and in delta = rowsum(dctx * ctx), so storing it in 16 bits halves four passes over it.
 * bf16 = 2 (split-bf16 operand mode, dx_attention_fwd and dx_attention_bwd): fp32 storage (every *_bf16 flag 0); the seven products run
 * on split-bf16 operands as in dx_conv_gemm, P and dS split in registers, softmax, dropout and accumulation in fp32.  The _f16 twins
 * reject 2; any other value is an error. */

/* ---- dropout + residual + LayerNorm + FiLM + mask: model.py:188-191, :225-233, :256-258, :655-669 ------------------- */
/* z = drop_pre(a) + res is written back over `a`; y = mask(film(drop_post(LN(z)))); C in {128, 1024}.
 * rows n >= lens[b] + halo are zero-filled and not computed: halo = 0 is the reference's padding mask, halo > 0 serves the
 * unmasked prenet LayerNorms whose rows inside the conv halo are still needed */
int dx_ln_fwd(void* a, const void* res, const float* w, const float* bias, const float* film, int ld_film,
              const int* lens, int halo, void* y, float* mean, float* rstd, int B, int N, int C,
              uint64_t seed_pre, float p_pre, uint64_t seed_post, float p_post, const uint64_t* seed_offset, int io_bf16, void* y_bf16_copy,
              void* stream);
/* FiLM parameters of all FFT blocks in one launch: StyleAdapter.forward, model.py:779-800 (scalar post-multiplier affine, gamma | beta
 * concatenation, per-block split).  gammas / betas: (B, nb*C) predictor outputs; pm: (2, nb) post-multipliers or null (then gamma + 1, beta);
 * film: (nb, B, 2C), block i = the (B, 2C) tensor the LayerNorm kernels of FFT block i read.  The backward takes a HOST array of nb device
 * pointers to the per-block gradients (null entries = no gradient), writes dgammas / dbetas and ACCUMULATES dpm (2, nb). */
int dx_film_affine_fwd(const float* gammas, const float* betas, const float* pm, float* film, int B, int nb, int C, void* stream);
int dx_film_affine_bwd(const void* dfilm_ptrs, const float* gammas, const float* betas, const float* pm, float* dgammas, float* dbetas, float* dpm,
                       int B, int nb, int C, void* stream);
/* Out-projection + dropout + residual + LayerNorm (+ FiLM + mask) of an FFT block in ONE launch (16-bit operand modes):
 *   z = dropout(X W^T + proj_bias) + res;  y = mask(FiLM(LayerNorm(z)))      attn.out_proj (model.py:165-186) + model.py:188-191
 * X: 16-bit [B*N][ldx], 128 columns (the attention context); Wpack: the forward pack (dx_pack_weights) of the (128, 128) weight.
 * z / y / mean / rstd / y_bf16_copy / film / lens / halo / seeds: exactly the arguments of dx_ln_fwd with C = 128 (z = its `a` afterwards).
 * A 64-row tile owns whole output rows, so the projection result feeds the row statistics from LDS and never goes to HBM. */
int dx_proj_ln_fwd(const void* X, int ldx, const void* Wpack, const float* proj_bias, float* z, const float* res, const float* w, const float* bias,
                   const float* film, int ld_film, const int* lens, int halo, float* y, float* mean, float* rstd, int B, int N,
                   uint64_t seed_pre, float p_pre, const uint64_t* seed_offset, void* y_bf16_copy, void* stream);
int dx_ln_bwd(const void* dy, const void* z, const float* mean, const float* rstd, const float* w, const float* bias,
              const float* film, int ld_film, const int* lens, int halo, void* dz, void* da, float* dw, float* dbias,
              float* dfilm, int ld_dfilm, int B, int N, int C, int relu_mask,
              uint64_t seed_pre, float p_pre, uint64_t seed_post, float p_post, const uint64_t* seed_offset, int io_bf16, void* dg_bf16_copy,
              void* stream);
/* y_bf16_copy / dg_bf16_copy (optional, C = 128): a second, bf16 copy of y / of the gradient that feeds the GEMM backward.  The
 * next GEMM would round its fp32 operand to bf16 while staging anyway, so results are bit-identical and the operand costs half the bytes.
 * io_bf16 = 1 (C = 1024 only): a / res / y and dy / z / dz / da are stored as bf16; statistics and parameter gradients stay fp32 */

/* ---- embeddings, positions, masks, pooling: model.py:119-150, :597-604, :554-557, :687-716 --------------------------- */
int dx_add_pos(const float* x, const long* sym, const float* emb, const float* pe, const int* lens, float* out,
               int B, int N, int D, int pe_rows, void* stream);
int dx_mask_rows(const float* in, const int* lens, float* out, int B, int N, int C, void* stream);
int dx_embedding_bwd(const float* dout, const long* sym, const int* lens, float* demb, int B, int N, int D, void* stream);
int dx_accent_sum(const float* prenet, const float* energy, const float* pitch, const float* we, const float* be,
                  const float* wp, const float* bp, const float* pe, const int* lens, float* out,
                  int B, int N, int D, int pe_rows, void* stream);
int dx_scalar_conv_wgrad(const float* dout, int ldd, const float* rowscale, const float* s0, const float* s1, const int* lens,
                         float* dw0, float* db0, float* dw1, float* db1, int B, int N, int D, void* stream);
int dx_mean_pool(const float* x, const int* lens, float* out, int B, int N, int C, void* stream);
int dx_mean_pool_bwd(const float* dout, const int* lens, float* dx, int B, int N, int C, void* stream);
int dx_transpose(const float* in, float* out, int B, int R, int Cc, int accumulate, void* stream);   /* accumulate: out += in^T */
int dx_relu_bwd(const float* dy, const float* y, float* out, long n, void* stream);
int dx_channel_affine(const void* x, const float* scale, const float* shift, void* out, long rows, int C, int io_bf16, void* stream); /* layers/pitch_predictor.py:49-62 (BatchNorm1d, eval); io_bf16: x / out stored in the mode's 16-bit type */
int dx_l2_normalize(const float* x, float* y, int rows, int C, void* stream);            /* model.py:904 */
int dx_cross_entropy(const float* logits, const long* target, float* loss, float* dlogits, int B, int S, void* stream); /* loss.py:85 */

/* ---- Gaussian upsampling: model.py:417-510 ---------------------------------------------------------------------------- */
int dx_duration_scan(const long* dur_int, float* mu, long* totals, int B, int L, void* stream);
int dx_upsample_prep(const float* enc, const float* dur, const float* energy, const float* pitch,
                     const float* wd, const float* bd, const float* we, const float* be, const float* wp, const float* bp,
                     const float* wr, const float* br, const int* lens, float* xs, float* z, float* sigma,
                     int B, int L, int D, void* stream);
int dx_upsample_fwd(const float* xs, const float* mu, const float* sigma, const int* lens, float* weights, float* xup,
                    int B, int L, int T, int D, void* stream);
int dx_upsample_bwd(const float* dxup, const float* xs, const float* mu, const float* sigma, const float* weights, const int* lens,
                    float* dxs, float* dsigma, int B, int L, int T, int D, void* stream);
int dx_upsample_sym_bwd(const float* dxs_in, const float* dsigma, const float* xs, const float* z, const float* dur, const int* lens,
                        const float* wd, const float* bd, const float* wr, float* dxs_out, float* dz, float* dwr, float* dbr,
                        int B, int L, int D, void* stream);

/* ---- loss reductions and gradients: loss.py:99-146 ------------------------------------------------------------------- */
int dx_mel_stats(const float* mel_pred, const float* mel_target, float* ep, float* et, float* l1sum, float* l2sum,
                 int B, int M, int T, void* stream);
/* rows_exist (optional, device int32 [B], as in dx_conv_gemm): frames t >= rows_exist[b] are the smoothing window's zero padding */
int dx_energy_diff(const float* ep, const float* et, const int* lens, float* des, float* esum, int B, int T, const int* rows_exist, void* stream);
/* e_per_total = 1: c_e is divided by sum_b lens[b] on the device (loss.py:129 normalises the energy term by the batch's valid frames) */
int dx_mel_grad(const float* mel_pred, const float* mel_target, const float* ep, const float* des, const int* lens,
                float c_l1, float c_l2, float c_e, int e_per_total, float* dmel, int B, int M, int T, void* stream);
/* Dynamic loss scale (see "dynamic loss scaling" below): dx_mel_grad_dyn, dx_pitch_grad_dyn and dx_loss_finalize_dyn are the launches
 * of the same names with one more argument, scale_dev (device float, required): c_l1 / c_l2 / c_e, scale and grad_scale are multiplied
 * by *scale_dev on the device, so a captured graph follows a scale that changes between replays.  *scale_dev is a power of two: the
 * product is exact and the results are bitwise those of the static launch given the host product. */
int dx_mel_grad_dyn(const float* mel_pred, const float* mel_target, const float* ep, const float* des, const int* lens,
                    float c_l1, float c_l2, float c_e, int e_per_total, const float* scale_dev, float* dmel, int B, int M, int T, void* stream);
/* loss.py:85-157 assembled on the device: terms[7] = {speaker_loss, speaker_ce_raw, post_mult_loss, mel_l1, mel_l2, energy, pitch},
 * total[1] = speaker + post_mult + l1 + l2 + ecw * energy + pcw * pitch; d_spk = dlogits * w; d_pm = pmw * pm / ||pm||_2.
 * w = *spk_w_dev if given (device scalar, re-read by every replay of a captured graph) else spk_w.  NULL ce / pm / esum / psum: term off.
 * grad_scale multiplies d_spk and d_pm (not the terms): the factor d(total)/d(what the caller differentiates), e.g. loss scale / accumulation steps. */
int dx_loss_finalize(const float* ce, const float* spk_w_dev, float spk_w, const float* dlogits, float* d_spk, int n_logits,
                     const float* pm, float* d_pm, int n_pm, float pmw,
                     const float* l1sum, const float* l2sum, const int* lens, int B, int M, float msw,
                     const float* esum, float ecw, const float* psum, float pcw, float* terms, float* total, float grad_scale, void* stream);
int dx_pitch_mse(const float* pp, int ldp, const float* gt, const int* lens, float* sums, int B, int T, void* stream);   /* ldp / ldd: element stride between consecutive frames of pp / dpp (the predictor's last conv writes 4-wide rows, channel 0 is the prediction) */
int dx_pitch_grad(const float* pp, int ldp, const float* gt, const int* lens, const float* sums, float scale, float* dpp, int ldd, int B, int T, void* stream);
int dx_pitch_grad_dyn(const float* pp, int ldp, const float* gt, const int* lens, const float* sums, float scale, const float* scale_dev,
                      float* dpp, int ldd, int B, int T, void* stream);
int dx_loss_finalize_dyn(const float* ce, const float* spk_w_dev, float spk_w, const float* dlogits, float* d_spk, int n_logits,
                         const float* pm, float* d_pm, int n_pm, float pmw,
                         const float* l1sum, const float* l2sum, const int* lens, int B, int M, float msw,
                         const float* esum, float ecw, const float* psum, float pcw, float* terms, float* total, float grad_scale,
                         const float* scale_dev, void* stream);
/* The frozen pitch predictor of the pitch-consistency term, one launch per direction (layers/pitch_predictor.py:38-74 applied in loss.py:131-140):
 * mel (B, M = 80, T) fp32 -> pp (B, T), and its input-gradient chain dpp (B, T) -> dmel (B, M, T) +=.  w0..w2: the 16-bit packs of the three
 * 256-wide k = 3 convolutions written by dx_pack_weights (fwd takes the forward packs, bwd the backward packs); b*: biases; s* / t*: eval-mode
 * BatchNorm folded to a scale / shift per channel; w3: row 0 of the last convolution's weight in checkpoint layout (256, 3) fp32, b3 its bias;
 * masks: (B, T, 3, 8) uint32 written by fwd (ReLU sign bits: the network is frozen, so the backward needs no activations), read by bwd.
 * Only tokens n < lens[b] are produced (the loss and the model mask the rest).  Every entry point with 16-bit packs also exists as <name>_f16.
 * rows_exist (optional, device int32 [B], as in dx_conv_gemm): frames n >= rows_exist[b] are the convolutions' zero padding although T frames
 * are stored (fwd ignores the mel there, bwd ignores dpp / masks there); NULL: all T frames exist.
 * What callers (and tests/test_pitch_exact_gpu.py) may rely on, with E = min(rows_exist[b], T) and len = min(lens[b], T) <= E:
 *   - the mel of every frame n < E is a convolution input, the frames at and past len included (only pp and dmel stop at len);
 *   - fwd writes pp[b][n] for n < len and nothing else of pp; bwd adds to dmel[b][:][n] for n < len and touches nothing else of dmel;
 *   - dpp[b][n] must be zero for n >= len (dx_pitch_grad writes it so): bwd reads dpp up to the end of the last tile's window and does not
 *     mask it by len, and the mask frames it needs past len are exactly those that a zero there leaves;
 *   - mask words: bit c % 32 of word c / 32 of (b, n, l) is "pre-activation of channel c of layer l at frame n > 0" (strictly).  For len > 0, fwd
 *     writes the words of layer l on every frame n < min(len + 3 - l, T) at least (to the end of the last tile's window; zeros at n >= E),
 *     and bwd's result depends on them for n <= len + 2 - l, n < E only: one frame further out per layer below the last, because the
 *     gradient at frame len - 1 comes through frame len of layer 2, len + 1 of layer 1 and len + 2 of layer 0.  Words of other frames may
 *     hold anything.  An utterance with lens[b] <= 0 runs no tile: nothing of it is read or written. */
int dx_pitch_chain_fwd(const float* mel, int B, int M, int T, const int* lens, const void* w0, const void* w1, const void* w2,
                       const float* b0, const float* b1, const float* b2, const float* s0, const float* s1, const float* s2,
                       const float* t0, const float* t1, const float* t2, const float* w3, float b3, float* pp, void* masks,
                       const int* rows_exist, void* stream);
int dx_pitch_chain_bwd(const float* dpp, int B, int M, int T, const int* lens, const void* w0, const void* w1, const void* w2,
                       const float* s0, const float* s1, const float* s2, const float* w3, const void* masks, float* dmel,
                       const int* rows_exist, void* stream);

/* ---- on-device batch conditioning: dynamic_stats.py:131-195 ------------------------------------------------ */
int dx_condition_prosody(const float* in, float* out, const long* speaker_ids, const float* table, const int* valid,
                         int which, int B, int N, int S, void* stream);
int dx_gather_speaker_rows(const float* emb, const long* speaker_ids, const int* valid, float* out, int B, int E, int S, void* stream);

/* ---- fused optimiser step: train.py:278-280 (Adam), :443 (clip_grad_norm_) ------------------------------ */
int dx_sumsq(const float* x, long n, float* out, void* stream);
/* skipped (optional device int): a non-finite *normsq (an overflowed fp16-mode gradient) skips the whole update -- p, m, v untouched --
   and increments *skipped; the reference has no loss scaling and therefore no counterpart (train.py:443-450 steps on NaN).
   norm_out (optional): receives sqrt(*normsq) * grad_scale = the value clip_grad_norm_ returns (train.py:443).
   zero_after (optional, != normsq): one float this launch sets to zero (the caller's other squared-norm accumulator). */
int dx_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, const float* normsq, float max_norm, float grad_scale, int* skipped,
                 float* norm_out, float* zero_after, void* stream);
/* ---- dynamic loss scaling (fp16 operand mode; the rules of torch.amp.GradScaler, no reference counterpart) -------------------------
 * The scaler state is eight 32-bit words in device memory, 4-byte aligned, owned by the caller:
 *   [0] scale          float, a power of two: what the NEXT backward multiplies its loss gradients by (the *_dyn loss launches)
 *   [1] inv_scale_used float, 1 / the scale the gradients now in the buckets were produced with
 *   [2] apply          int, 1: this update is applied, 0: skipped (non-finite norm)
 *   [3] applied        int, updates applied so far = the bias-correction step
 *   [4] good_steps     int, consecutive applied updates since the scale last changed
 *   [5] skipped        int, updates skipped so far
 *   [6] bc1            float, 1 - beta1^applied        [7] bc2_sqrt  float, sqrt(1 - beta2^applied)   (double arithmetic, rounded once)
 * The caller initialises [0], [3], [4], [5]; the rest is written before it is read.
 * dx_scaler_update (one workgroup, after dx_sumsq / the all-reduce, before dx_adam_step_dyn) reads *normsq and first sets
 * inv_scale_used = 1 / scale.  Non-finite: apply = 0, skipped += 1, good_steps = 0, scale = max(scale * backoff, min_scale).  Finite:
 * apply = 1, applied += 1, bc1 / bc2_sqrt from the new applied, good_steps += 1 and, when it reaches growth_interval, scale =
 * min(scale * growth, max_scale) and good_steps = 0.  growth >= 1 and backoff <= 1 must be powers of two.  A pure function of the
 * norm and the state: ranks that hold the same state and the same all-reduced norm agree without communication. */
int dx_scaler_update(void* state, const float* normsq, float beta1, float beta2, float growth, float backoff, int growth_interval,
                     float min_scale, float max_scale, void* stream);
/* dx_adam_step with grad_scale = inv_scale_used, the bias corrections and the skip decision read from the scaler state (apply == 0:
 * p, m, v untouched); normsq is required; norm_out / zero_after as in dx_adam_step (written whether or not the update is applied). */
int dx_adam_step_dyn(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, const float* normsq, float max_norm, const void* scaler, float* norm_out, float* zero_after,
                     void* stream);

/* ---- HiFi-GAN V1 / V2 / V3 vocoder, inference (reference vocoder/hifigan.py HiFiGANGenerator.forward; csrc/dx_vocoder.hip) ----------------
 * Activations are fp32, channels-last [B][samples][C] (conv_pre reads the (B, 80, T) mel through its strides).  frames (device int32
 * [B]) with a samples-per-frame scale gives each batch row's valid length: input rows at or past it read as the conv's zero padding,
 * output rows there are written as 0, so batch row b equals what the same row computes alone (bitwise: fixed summation order, no
 * atomics).  bf16 (operand mode) = 0: exact f32 (v_mfma_f32_16x16x4_f32), 1: bf16 operands (v_mfma_f32_16x16x32_bf16), 2: split bf16
 * (dx_voc_pack[_size], dx_voc_conv[_win], dx_voc_pair[_win]; dx_voc_chain[_win] refuses it): every operand is x = hi + lo, hi =
 * bf16_rne(x), lo = bf16_rne(x - hi), lo = 0 where hi is not finite, every product hi*lo + lo*hi + hi*hi in that order on three
 * v_mfma_f32_16x16x32_bf16 (~16 mantissa bits).  Activations are split after the fp32 leaky-ReLU while they are staged, weights once
 * by dx_voc_pack.  fp32 accumulate and storage in every mode; a pack serves the mode it was written for and no other. */
/* bytes of the weight pack dx_voc_pack writes for one layer (up > 1: a ConvTranspose1d in polyphase form, taps = 2).  Mode 2 packs a
 * lane's eight hi then its eight lo per k step: 32 bytes, so the pack is the f32 pack's size whenever Cin % 32 == 0 (and rounds Cin up
 * to 32 where the f32 pack rounds it to 16). */
int dx_voc_pack_size(int Cout, int Cin, int taps, int up, int bf16, long* bytes);
/* folded weights -> the operand pack of dx_voc_conv / dx_voc_pair.  up == 1: W (Cout, Cin, taps) of a Conv1d; up > 1 (even): W (Cin,
 * Cout, 2 up) of ConvTranspose1d(stride up, padding up / 2), packed as up phases of 2 taps (output sample s up + r reads input
 * samples s + base_r and s + base_r + 1, base_r = -1 if r + up / 2 < up else 0). */
int dx_voc_pack(const float* W, void* Wp, int Cout, int Cin, int taps, int up, int bf16, void* stream);
/* Y = acc_mode( conv(lrelu?(X)) + bias (+ R) ): a dilated Conv1d ('same' padding dil (taps - 1) / 2; odd taps <= 11, dil (taps - 1) <= 72; Cout in {16, 32, ..., 512}) or, with up > 1
 * and taps = 2, the polyphase ConvTranspose1d (N input rows -> N up output rows).  X element (b, n, c) at X[b sxb + n sxn + c sxc];
 * Y and R (optional residual, may equal Y; Y must not alias X) are channels-last with batch stride syb; a channels-last X is 16-byte aligned.  Input rows n >= min(frames[b] in_scale, N) are
 * zero.  acc_mode 0: Y = v, 1: Y += v, 2: Y = (Y + v) / 3 (the generator's stage mean over its three ResBlocks). */
int dx_voc_conv(const float* X, long sxb, long sxn, long sxc, const void* Wp, const float* bias, float* Y, long syb, const float* R,
                const int* frames, int in_scale, int B, int N, int Cin, int Cout, int taps, int dil, int up, int lrelu_in, int acc_mode,
                int bf16, void* stream);
/* One ResBlock1 pair in one launch (C in {16, 32, 64}): Y = acc_mode( conv2(lrelu(conv1(lrelu(X)) + b1)) + b2 + X ), conv1 dilation dil,
 * conv2 dilation 1, both `taps` wide; the intermediate stays in LDS with its halo.  X, Y channels-last [B][N][C] with batch stride
 * sxb; Y must not alias X. */
int dx_voc_pair(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y,
                const int* frames, int scale, int B, int N, int C, int taps, int dil, int acc_mode, int bf16, void* stream);
/* One ResBlock2 (the V3 generator) in one launch (C in {32, 64}; taps 3, 5 or 7; d1 (taps - 1) <= 18, d2 (taps - 1) <= 72):
 * x1 = conv_d1(lrelu(X)) + b1 + X, Y = acc_mode( conv_d2(lrelu(x1)) + b2 + x1 ).  x1 is computed with the second conv's halo and stays on
 * the CU: its bf16 / f32 operand copy in LDS, the fp32 values the second residual adds in registers.  X, Y as for dx_voc_pair. */
int dx_voc_chain(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y,
                 const int* frames, int scale, int B, int N, int C, int taps, int d1, int d2, int acc_mode, int bf16, void* stream);
/* conv_post: Y[b][s] = clip(tanh(conv7(lrelu(X)) + bias), -1, 1) for s < min(frames[b] scale, N), 0 for the rest of the ncols samples.
 * X channels-last [B][N][32] (batch stride sxb), W the folded (1, 32, 7) fp32 weight. */
int dx_voc_post(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy, const int* frames, int scale,
                int B, int N, int ncols, void* stream);
/* dx_voc_post for C input channels, C in {16, 32} (V2's last stage runs padded to 16): X [B][N][C], W the folded (1, C, 7) weight. */
int dx_voc_post_c(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy, const int* frames, int scale,
                  int B, int N, int ncols, int C, void* stream);
/* The windowed forms: the streaming generator (vocoder.stream_plan).  A launch reads the chunk index c from the device int32 `cursor`
 * and computes rows [c == 0 ? 0 : c step + lag, (c + 1) step + lag) of its tile-row axis (the rows of X for the conv and the transposed
 * conv, whose output rows are those times up; the samples for the pair and conv_post), clipped by the row's valid length; its grid
 * covers step + lag rows.  N is the LOGICAL row count (frames axis length times scale).  Tensors are rings: logical row n lives at slot
 * n & mask, mask = ring size - 1 (a power of two minus 1), or 0 for plain indexing (the mel read by conv_pre, a whole-length tensor).
 * Nothing outside the window is stored, no zeros either: those slots hold older rows.  Zero padding at the two ends of an utterance is
 * unchanged (logical rows outside [0, length) read as 0).  Each element is bit for bit what the unwindowed entry point writes at the
 * same logical row, given the same rows in its receptive field.  R has its own batch stride srb; the pair's Y its own syb.
 * dx_voc_post_win writes sample s to column s - c step of Y (B, ncols >= step + lag), 0 at and past the row's end (my must be 0). */
int dx_voc_conv_win(const float* X, long sxb, long sxn, long sxc, const void* Wp, const float* bias, float* Y, long syb, const float* R,
                    long srb, const int* frames, int in_scale, int B, int N, int Cin, int Cout, int taps, int dil, int up, int lrelu_in,
                    int acc_mode, int bf16, const int* cursor, int step, int lag, int mx, int my, int mr, void* stream);
int dx_voc_pair_win(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y, long syb,
                    const int* frames, int scale, int B, int N, int C, int taps, int dil, int acc_mode, int bf16, const int* cursor,
                    int step, int lag, int mx, int my, void* stream);
int dx_voc_chain_win(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y, long syb,
                     const int* frames, int scale, int B, int N, int C, int taps, int d1, int d2, int acc_mode, int bf16,
                     const int* cursor, int step, int lag, int mx, int my, void* stream);
int dx_voc_post_win(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy, const int* frames, int scale,
                    int B, int N, int ncols, const int* cursor, int step, int lag, int mx, int my, void* stream);
int dx_voc_post_c_win(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy, const int* frames, int scale,
                      int B, int N, int ncols, int C, const int* cursor, int step, int lag, int mx, int my, void* stream);
/* *cursor += 1 by one thread: the last launch of a chunk, so that replaying the same launches computes the next window. */
int dx_voc_stream_advance(int* cursor, void* stream);

/* ---- HiFi-GAN generator training, f32 operands (csrc/dx_vocoder_bwd.hip) -----------------------------------------------------------
 * The data gradients of the generator are dx_voc_conv launches on packs built by the host (vocoder_train.py); these are the rest of the
 * backward.  frames / scale as above: rows at or past min(frames[b] scale, N) read as zero and are written as zero.  No atomics: partial
 * sums go to the caller's workspace and are added in a fixed order, so two calls give the same bits. */
/* bytes of the workspace dx_voc_wgrad needs for this shape (up > 1: a transposed conv, taps = 3) */
int dx_voc_wgrad_size(int B, int N, int Cin, int Cout, int taps, int up, long* bytes);
/* Weight and bias gradient of one convolution (v_mfma_f32_16x16x4_f32, the position as the MFMA k):
 *   up == 1: G (Cout, Cin, taps), G[co][ci][t] = sum_b sum_n act(X[b][n - dil (taps - 1) / 2 + t dil][ci]) dY[b][n][co]
 *   up > 1 (even, taps = 3, dil = 1): G (Cin, Cout, 2 up) of ConvTranspose1d(stride up, padding up / 2) with N INPUT rows, from the
 *            view of its output gradient (N up, Cout) as (N, up Cout): G[ci][co][d up + r + up / 2] = sum act(X[b][m][ci]) dY[b][m + d][r Cout + co]
 *   dbias (optional) [Cout] = sum of dY over rows (and phases).
 * X element (b, n, c) at X[b sxb + n sxn + c sxc] (conv_pre reads the (B, 80, T) mel in place); dY element (b, n, c) at
 * dY[b dyb + n ldy + dyc + c], ldy >= dyc + up Cout.  act 0: identity, 1: leaky-ReLU(0.1).  Cin, Cout multiples of 16 up to 512. */
int dx_voc_wgrad(const float* X, long sxb, long sxn, long sxc, const float* dY, long dyb, int ldy, int dyc, float* G, float* dbias,
                 float* workspace, long workspace_bytes, const int* frames, int scale, int B, int N, int Cin, int Cout, int taps, int dil,
                 int up, int act, void* stream);
/* dX = (acc ? dX : 0) + (R ? R : 0) + gscale lrelu'(Xs) U, the product and the sum one fma; (B, N, C) channels-last tensors, contiguous;
 * Xs NULL: slope 1; R may equal dX.  lrelu'(x) = 1 for x > 0, else 0.1. */
int dx_voc_act_bwd(const float* Xs, const float* U, const float* R, float* dX, const int* frames, int scale, int B, int N, int C,
                   float gscale, int acc, void* stream);
int dx_voc_post_bwd_size(int B, int N, int C, long* bytes);
/* conv_post backward from its saved output Y = clip(tanh z) and the upstream dY (both (B, ldy)): dz = dY (1 - Y^2), 0 past the length;
 * dX[b][n][c] = lrelu'(X) sum_t dz[n + 3 - t] W[c][t]; dW (1, C, 7) and db (1) by the fixed-order two-stage sum.  C in {16, 32}. */
int dx_voc_post_bwd(const float* X, long sxb, const float* W, const float* Y, const float* dY, int ldy, float* dX, float* dW, float* db,
                    float* workspace, long workspace_bytes, const int* frames, int scale, int B, int N, int C, void* stream);

/* ---- mel front end (reference extract_features.py mel_spectrogram_HiFi, vocoder/dataset.py mel_spectrogram, center = False;
 * csrc/dx_mel.hip) ------------------------------------------------------------------------------------------------------------
 * n_fft = win = 1024, hop = 256, reflect padding of 384 samples per side with each row's own first / last samples.  kmax: the bins
 * [0, kmax) where the filter bank has a non-zero column (rounded up to 64 inside), n_mels % 16 == 0 and <= 128. */
/* bytes of the DFT basis and of the filter-bank operand dx_mel_pack writes */
int dx_mel_basis_size(int n_mels, int kmax, long* basis_bytes, long* fb_bytes);
/* fb (n_mels, n_freq) fp32 filter bank -> the two MFMA operands of dx_mel: the periodic-Hann-windowed cos / sin basis (computed in
 * double, rounded once to f32) and the packed filter bank (zero past n_freq). */
int dx_mel_pack(const float* fb, int n_mels, int n_freq, int kmax, void* basis, void* fbp, void* stream);
/* wav [B][sxb] fp32 (S samples allocated per row), lengths device int32 [B] (samples past min(lengths[b], S) are never read) ->
 * mel [B][n_mels][T_max] (batch stride smb) = log(max(fb . sqrt(|STFT|^2 + 1e-9), clip)) and energy [B][T_max] = L2 norm of the
 * clamped mel over channels.  Row b has lengths[b] / 256 frames (none if lengths[b] <= 384); everything past them is written as 0. */
int dx_mel(const float* wav, long sxb, int S, const int* lengths, const void* basis, const void* fb, float* mel, long smb,
           float* energy, int B, int T_max, int n_mels, int kmax, float clip, void* stream);
/* The two extra operands of dx_mel_bwd: the basis packed with samples as columns and the filter bank packed with bins as columns.
 * Their sizes are those dx_mel_basis_size returns (basisT: basis_bytes, fbT: fb_bytes). */
int dx_mel_bwd_pack(const float* fb, int n_mels, int n_freq, int kmax, void* basisT, void* fbT, void* stream);
/* Waveform gradient of sum(gmel . mel) for the mel of dx_mel (fp32; the energy output has no gradient here).  wav, lengths, basis, fb,
 * T_max, n_mels, kmax, clip as in the forward call; gmel [B][n_mels][T_max] (batch stride sgb) -> dwav [B][sxb], all S samples of
 * every row written.  Nothing was saved by the forward: each valid frame's spectrum and linear mel are recomputed with the forward's
 * own arithmetic, then dlin = gmel / lin where lin >= clip (else 0), dmag = fb^T dlin, dre = dmag re / mag, dim = dmag im / mag,
 * dframe = [dre | dim] . basis^T, overlap-added over the four frames that cover a padded sample, the 384 reflected samples of each
 * end folded back onto the samples they mirror.  Samples at or past lengths[b] get 0 (all of a row with lengths[b] <= 384); wav and
 * gmel are never read past a row's samples / frames.  One launch, no workspace, no atomics: every element is summed in a fixed order,
 * so two runs, and a batch row and the utterance alone, are bitwise equal.  dwav must not alias wav. */
int dx_mel_bwd(const float* wav, long sxb, int S, const int* lengths, const void* basis, const void* fb, const void* basisT,
               const void* fbT, const float* gmel, long sgb, float* dwav, int B, int T_max, int n_mels, int kmax, float clip,
               void* stream);

/* ---- prosody transfer and PCM (reference generate.py generate_batch_mel_specs; csrc/dx_prosody.hip) --------------------------------
 * fp32 and integers only.  One launch each, no workspace, no atomics, every reduction in a fixed order that depends on the row alone:
 * a batch row is bitwise that utterance run alone.  dur_int is int64 (as dx_duration_scan takes it), in_lens device int32 [B];
 * positions l >= in_lens[b] of every (B, L) output are written as 0. */
/* extract_features.py:287-342 (get_symbols_energy / get_symbols_pitch): symbol l with d = dur_int[b][l] > 0 covers the frames
 * [off, off + d), off = the sum of the row's earlier durations.  sym_energy = their mean, sym_pitch = the mean of those > 0 (0 if
 * none); d == 0: both 0, no frame consumed.  frames_* [B][ldt], T frames valid per row; frames at or past T are never read, so a row
 * whose durations sum past T (a caller error, checked by the Python wrapper) yields wrong means and nothing worse. */
int dx_symbol_prosody(const float* frames_energy, const float* frames_pitch, long ldt, const long* dur_int, const int* in_lens,
                      float* sym_energy, float* sym_pitch, int B, int T, int L, void* stream);
/* generate.py:165-185 (_normalize_external_feature), :265-269 (alpha scaling), model.py:1077-1087 (factors, zero where dur_int == 0)
 * and model.py:975-1024 (pitch_shift / pitch_multiply), per element in that order, each operation rounded on its own:
 *   normalize != 0: v == 0 stays 0; else [has_source: v = (v - src_mean) / src_std * tgt_std + tgt_mean;] v = (v - tgt_mean) / tgt_std;
 *                   v *= alpha
 *   energy *= energy_factors (NULL: skipped); energy = pitch = 0 where dur_int == 0 (NULL: skipped)
 *   mode 0: pitch unchanged; 1 (add): p = (log(exp(std p + mean) + factor) - mean) / std; 2 (multiply): p += (p - m) factor, m = the
 *   mean of the row's non-zero p at this point; p == 0 (unvoiced) stays exactly 0 in both, and an all-unvoiced row is all zeros.
 * stats [B][4] = the row's target {energy mean, energy std, pitch mean, pitch std} (needed by normalize and by mode 1), source [4] the
 * same four of the source speaker (read iff has_source).  normalize == 0 is model.inference's own pre-processing in the same launch.
 * All tensors [B][L] contiguous; the outputs may not alias the inputs. */
int dx_prosody_condition(const float* energy, const float* pitch, const long* dur_int, const int* in_lens, const float* energy_factors,
                         const float* pitch_factors, const float* stats, const float* source, int has_source, float alpha_energy,
                         float alpha_pitch, int mode, int normalize, float* energy_out, float* pitch_out, int B, int L, void* stream);
/* generate.py:327 ((audio * 32767.5).clip(-32768, 32767).astype(np.int16)): fp32 multiply, clamp, truncation toward zero.
 * audio [B][S] fp32 -> pcm [B][S] int16, 0 at or past sample_lengths[b] (device int32 [B]); both 16-byte aligned, B <= 65535. */
int dx_pcm16(const float* audio, const int* sample_lengths, short* pcm, int B, long S, void* stream);

/* ---- Griffin-Lim vocoding without a checkpoint (reference griffin_lim.py:100-198; csrc/dx_griffin_lim.hip) -------------------------
 * fp32 only, n_fft = win = 1024 and hop = 256 only.  No atomics and no workspace; every sum in a fixed order that depends on the row
 * alone, so two runs, and a batch row and that utterance alone, are bitwise equal. */
/* griffin_lim.py:150-167, one pass of the while loop of reconstruct_signal_griffin_lim for a padded batch in one launch.
 * x_in, x_out [B][sxb] (sxb >= 256 T_max + 1024, a multiple of 4; both 16-byte aligned; they must not alias: the caller ping-pongs).
 * Row b has frames[b] frames (device int32, clamped to [0, T_max]) starting at samples 256 i under the SYMMETRIC Hann window
 * np.hanning(1024): S_i = rfft(w x[256 i : 256 i + 1024]), P_i = M_i S_i / |S_i| ((M_i, 0) where S_i == 0, as np.angle(0) = 0),
 * y_i = w irfft(P_i) (DC and Nyquist taken as real), x_out = overlap_add(y) / 2.  mag [B][T_max][513] frame-major (batch stride smb):
 * the reference's (513, T) magnitudes transposed, repacked once outside the loop.  Samples at or past 256 frames[b] + 768 are written
 * as 0 (the last 256 samples of the reference's signal are touched by no frame); x_in and mag are never read past a row's own frames.
 * tab: 3072 floats computed in double on the host and rounded once: the window, then the cos and -sin twiddles of the radix-4 passes
 * Ns = 4, 16, 64, 256 at offset Ns - 4 as [r - 1][q] = 2 pi q r / (4 Ns), r = 1..3, q < Ns. */
int dx_gl_iter(const float* x_in, float* x_out, long sxb, const float* mag, long smb, const int* frames, const float* tab, int B,
               int T_max, int n_fft, int hop, void* stream);
/* griffin_lim.py:196 (waveform / np.max(abs(waveform))) per row: y[b] = x[b] / max|x[b]| over the row's S samples; an all-zero row
 * stays zero (the reference divides by zero there).  y may alias x. */
int dx_gl_peak_normalize(const float* x, float* y, long sxb, int B, long S, void* stream);
/* HOST pointers: the hop blocks of 256 samples one workgroup of dx_gl_iter owns (its tile; tests place row lengths around it) and the
 * 32-bit words of the packed filter bank dx_nnls_mel takes */
int dx_gl_layout(int* tile_blocks, int* pack_words);
/* griffin_lim.py:100-114 (mel_to_linear -> nnls): mel [B][n_mels][T] LINEAR-scale mel (batch stride smb), lengths device int32 [B] ->
 * X [B][T][513] frame-major (batch stride sxb), X >= 0, approximately minimising |A X - mel|^2 per frame: x0 = max(pinv(A) mel, 0),
 * then `iters` FISTA steps of size `step` (1 / |A|_2^2).  The problem is underdetermined (80 equations, 513 unknowns): the reference's
 * L-BFGS-B answer is one minimiser among many and is not reproduced; the residual is.  Frames at or past lengths[b] are written as 0.
 * pinvT [n_mels][576] fp32 = pinv(A) transposed, zero past bin 512.  pack (dx_gl_layout's pack_words words, built and validated by the
 * host: every bin weighs at most two channels, every channel's non-zeros are one run of bins): [0, 576) per bin i0 | i1 << 16,
 * [576, 1152) and [1152, 1728) its two weights, then 128 words each of every channel's first bin, bin count and weight offset, then
 * 1536 words of channel-major weights. */
int dx_nnls_mel(const float* mel, long smb, const int* lengths, const float* pinvT, const void* pack, float step, int iters, float* X,
                long sxb, int B, int T, int n_mels, int n_freq, void* stream);

/* ---- HiFi-GAN discriminators, forward (reference vocoder/discriminators.py; csrc/dx_disc.hip) -------------------------------------
 * Activations are fp32, channels-last.  A "row" is one independent 1-D signal: a batch row of the Multi-Scale Discriminator
 * ([B][T][C]: rdiv = 1) or one column of the Multi-Period Discriminator's period-folded tensor ([B][H][p][C]: rdiv = p, row = b p + w).
 * Element (row, n, c) is at X[(row / rdiv) sxb + (row % rdiv) sxr + n sxn + c].  There are no lengths: every row has N positions, as
 * in the reference.  Real and generated audio are rows of one batch.  No atomics: every output element and every loss is summed in
 * an order fixed by the shapes alone, so two runs, and a batch row and that row alone, are bitwise equal.  bf16 = 0: exact f32
 * (v_mfma_f32_16x16x4_f32), 1: bf16 operands (v_mfma_f32_16x16x32_bf16), fp32 accumulate and storage. */
/* bytes of the pack dx_disc_pack writes for a folded weight (Cout, Cin_g, taps), Cin_g = input channels per group */
int dx_disc_pack_size(int Cout, int Cin_g, int taps, int bf16, long* bytes);
/* folded fp32 weight (Cout, Cin_g, taps) of a (grouped) Conv1d, or of a Conv2d with a (taps, 1) kernel, -> dx_disc_conv's operand:
 * [column block][64-channel chunk][k step][lane] MFMA fragments, k = tap * chunk width + channel, zero-padded to the k step. */
int dx_disc_pack(const float* W, void* Wp, int Cout, int Cin_g, int taps, int bf16, void* stream);
/* Y = lrelu_0.1?(conv(X) + bias): DiscriminatorP.convs[1:] (discriminators.py:39-46: (5, 1) kernels, stride (3, 1) or 1, along H for
 * each of the p columns) and DiscriminatorS.convs[1:] (:106-111: k = 41 grouped with strides 1, 2, 4, and the dense k = 5).  N input
 * positions per row -> (N + 2 pad - taps) / stride + 1 output positions; Y is addressed like X with (syb, syr, syn) and Cout
 * channels.  taps <= 41, stride <= 4, pad <= 20; channels per group: in 8, 16, 32 or a multiple of 64, out 16, 32 or a multiple of
 * 64; Cout % 64 == 0.  X 16-byte aligned with strides % 4 == 0; Y must not alias X. */
int dx_disc_conv(const float* X, long sxb, long sxr, long sxn, const void* Wp, const float* bias, float* Y, long syb, long syr, long syn,
                 int rows, int rdiv, int N, int Cin, int Cout, int groups, int taps, int stride, int pad, int act, int bf16,
                 void* stream);
/* The Cin = 1 first layers, fp32 FMAs (DiscriminatorP.forward :52-60 with convs[0], p > 1; DiscriminatorS.convs[0] :105, p = 1):
 * x [B][sxb] with T samples per row is read through the period view x[b][h p + w], h < H = ceil(T / p); samples at or past T are the
 * reference's right reflect padding (F.pad(x, (0, p - T % p), 'reflect'): index 2 (T - 1) - i), applied while reading.
 * Y [B][Hout][p][Cout] = lrelu_0.1(conv along h + bias), Hout = (H + 2 pad - taps) / stride + 1; W is the folded (Cout, 1, taps). */
int dx_disc_first(const float* x, long sxb, int T, const float* W, const float* bias, float* Y, int B, int p, int Cout, int taps,
                  int stride, int pad, void* stream);
/* The Cout = 1 last layers (conv_post, :48 and :113; no activation), fp32: Y[(row / rdiv) syb + (row % rdiv) syr + n syn] =
 * sum_t sum_c X(row, n - (taps - 1) / 2 + t, c) W[c][t] + bias[0]; X addressed as in dx_disc_conv, W the folded (1, C, taps). */
int dx_disc_post(const float* X, long sxb, long sxr, long sxn, const float* W, const float* bias, float* Y, long syb, long syr, long syn,
                 int rows, int rdiv, int N, int C, int taps, void* stream);
/* MultiScaleDiscriminator.meanpools (:139-142): AvgPool1d(4, 2, padding = 2), padding counted; x [R][T] -> y [R][T / 2 + 1] */
int dx_disc_pool(const float* x, float* y, int R, int T, void* stream);
/* floats of the partial-sum workspace dx_disc_losses needs for n entries of at most max_count elements */
int dx_disc_losses_workspace(long max_count, int n, long* floats);
/* discriminator_loss, generator_loss and feature_loss (:163-194) in one call, no host synchronisation.  table: n device entries of
 * {const float* r, const float* g, long count, long code}, code = kind + 2 set; kind 0 is a score pair (dr, dg), kind 1 a feature-map
 * pair.  out[3 n_sets + 3 e + {0, 1, 2}] = entry e's mean (1 - dr)^2, mean dg^2, mean (1 - dg)^2 (kind 0) or mean |r - g|, 0, 0
 * (kind 1); out[3 s + {0, 1, 2}] = set s's discriminator_loss (sum of r_loss + g_loss), generator_loss and feature_loss (x 2)
 * totals, the entries added in table order.  Each entry is summed in chunks of 16384 elements, the chunk sums then in a fixed order.
 * max_count: the largest count, total_count: their sum. */
int dx_disc_losses(const void* table, int n, int n_sets, long max_count, long total_count, float* partial, float* out, void* stream);

/* ---- HiFi-GAN discriminators, backward to the generated waveform (csrc/dx_disc_bwd.hip) ---------------------------
 * The gradient of loss_gen + loss_fm with respect to the generated rows only: no gradient to the real rows or to any weight.  Buffers
 * and row addressing are the forward's.  R / G are the real / generated halves of a stored feature map; gw_* point to ONE device float
 * each, the upstream gradient of the generator loss / the feature loss of this discriminator (read on the device, no host sync).
 * "Epilogue" (epilogue = 1): out = (acc + gw_fm fm_scale sign(G - R)) * (G > 0 ? 1 : 0.1) with fm_scale = 2 / numel(G), sign(0) = 0:
 * the pre-activation gradient of the layer whose output G is; epilogue = 0 writes acc (R, G, gw_fm may be null).  No atomics. */
/* bytes of the transposed, per-stride-phase pack of a folded weight (Cout, Cin / groups, taps) */
int dx_disc_dgrad_pack_size(int Cin, int Cout, int groups, int taps, int stride, int bf16, long* bytes);
/* -> [phase][16 input channels][chunk][k step][lane] MFMA fragments, k = (tap index inside the phase) * chunk width + output channel;
 * zero past a phase's taps; 8-channel groups: two groups per column block, block-diagonal */
int dx_disc_dgrad_pack(const float* W, void* Wp, int Cin, int Cout, int groups, int taps, int stride, int bf16, void* stream);
/* Data gradient of dx_disc_conv's layer: dZ (rows of (N + 2 pad - taps) / stride + 1 positions, Cout channels, strides szb, szr, szn)
 * -> dX, R, G (rows of N positions, Cin channels, strides sxb, sxr, sxn): dX[n][ci] = sum over co of ci's group and taps t with
 * (n + pad - t) % stride == 0 of dZ[(n + pad - t) / stride][co] W[co][ci][t], then the epilogue.  Every dX[n][ci], n < N, is written
 * once.  stride <= taps <= 41, stride <= 4, pad <= 20; channels per group: in 8, 16, 32 or a multiple of 64, out 16, 32 or a multiple
 * of 64; Cin % 16 == 0.  dZ 16-byte aligned with strides % 4 == 0; dX must not alias dZ. */
int dx_disc_conv_dgrad(const float* dZ, long szb, long szr, long szn, const void* Wp, float* dX, const float* R, const float* G, long sxb,
                       long sxr, long sxn, const float* gw_fm, float fm_scale, int rows, int rdiv, int N, int Cin, int Cout, int groups,
                       int taps, int stride, int pad, int epilogue, int bf16, void* stream);
/* The Cout = 1 last layer transposed, from the scores: dS[m] = s_scale (gw_gen (Sg[m] - 1) + gw_fm sign(Sg[m] - Sr[m])), s_scale =
 * 2 / numel(Sg); dZ[n][c] = sum_t dS[n + (taps - 1) / 2 - t] W[c][t], then the epilogue with the last conv layer's map.  Sr / Sg are
 * addressed with (ssb, ssr, ssn), dZ / R / G with (sxb, sxr, sxn) and C channels; W the folded (1, C, taps). */
int dx_disc_post_bwd(const float* Sr, const float* Sg, long ssb, long ssr, long ssn, const float* W, float* dZ, const float* R, const float* G,
                     long sxb, long sxr, long sxn, const float* gw_gen, const float* gw_fm, float s_scale, float fm_scale, int rows, int rdiv,
                     int N, int C, int taps, int epilogue, void* stream);
/* The Cin = 1 first layer transposed, through the period view: dZ [B][Hout][p][Cout] -> dy [B][sdb], T samples per row.  Sample i sums
 * its own folded position and, where 2 (T - 1) - i lies in the reflect-padded tail [T, H p), that position too.  accumulate = 1 adds
 * to dy. */
int dx_disc_first_bwd(const float* dZ, const float* W, float* dy, long sdb, int T, int B, int p, int Cout, int taps, int stride, int pad,
                      int accumulate, void* stream);
/* AvgPool1d(4, 2, padding = 2) transposed: dy [R][T / 2 + 1] -> dx [R][T], dx[i] = (dy[i / 2] + dy[i / 2 + 1]) / 4 (terms past the end
 * dropped); accumulate = 1 adds to dx. */
int dx_disc_pool_bwd(const float* dy, float* dx, int R, int T, int accumulate, void* stream);

/* ---- HiFi-GAN discriminators, the discriminator step (csrc/dx_disc_wgrad.hip) ---------------------------------
 * The gradient of loss_disc with respect to the folded (weight, bias) of every layer, over all rows of a pass (real rows first), f32
 * operands only.  Buffers and row addressing are the forward's; the data gradient between the layers is dx_disc_conv_dgrad with
 * R = G = the whole stored map and gw_fm -> a device zero.  No atomics: every sum runs over a fixed number of runs, a function of the
 * shape alone, whose partial sums go through the caller's workspace and are added in order by a second launch. */
/* bytes of workspace dx_disc_wgrad needs; splits (may be null): the number of runs its k axis is cut into */
int dx_disc_wgrad_size(int rows, int N, int Cin, int Cout, int groups, int taps, int stride, int pad, long* bytes, int* splits);
/* Weight gradient of dx_disc_conv's layer.  A: the layer's input map (rows of N positions, Cin channels, strides sxb, sxr, sxn), dZ:
 * its pre-activation gradient (rows of Nout = (N + 2 pad - taps) / stride + 1 positions, Cout channels, strides szb, szr, szn) ->
 * G (Cout, Cin / groups, taps), G[co][ci][t] = sum over rows and m < Nout of A[row][m stride - pad + t][group(co) Cin / groups + ci]
 * dZ[row][m][co] (positions outside [0, N) read as zero), and dbias[co] = sum dZ[row][m][co].  v_mfma_f32_16x16x4_f32, the flattened
 * (row, m) sequence as k.  taps <= 41, stride <= 4, pad <= 20; channels per group: in 8, 16, 32 or a multiple of 64, out 16, 32 or a
 * multiple of 64.  A and dZ 16-byte aligned with strides % 4 == 0; workspace 16-byte aligned. */
int dx_disc_wgrad(const float* A, long sxb, long sxr, long sxn, const float* dZ, long szb, long szr, long szn, float* G, float* dbias,
                  void* workspace, long workspace_bytes, int rows, int rdiv, int N, int Cin, int Cout, int groups, int taps, int stride,
                  int pad, void* stream);
int dx_disc_post_wgrad_size(int rows, int N, int C, int taps, long* bytes);
/* The score seed and the Cout = 1 last layer: dS[row][m] = gw[0] s_scale (S[row][m] - 1) for row < half_rows (the real rows),
 * gw[0] s_scale S[row][m] for the others (the generated rows); s_scale = 2 / numel of one half of the scores.  dZ[row][n][c] =
 * (A[row][n][c] > 0 ? 1 : 0.1) sum_t dS[row][n + (taps - 1) / 2 - t] W[c][t], A the last conv layer's stored map; dW[c][t] = sum
 * dS[row][m] A[row][m - (taps - 1) / 2 + t][c]; db[0] = sum dS, added in double.  S is addressed with (ssb, ssr, ssn), A and dZ with
 * (sxb, sxr, sxn) and C channels; W the folded (1, C, taps); odd taps <= 8; dZ must not alias A; workspace 8-byte aligned. */
int dx_disc_post_wgrad(const float* S, long ssb, long ssr, long ssn, const float* W, const float* A, float* dZ, long sxb, long sxr, long sxn,
                       const float* gw, float s_scale, float* dW, float* db, void* workspace, long workspace_bytes, int rows,
                       int half_rows, int rdiv, int N, int C, int taps, void* stream);
int dx_disc_first_wgrad_size(int R, int T, int p, int Cout, int taps, int stride, int pad, long* bytes);
/* The Cin = 1 first layer: x [R][sxb] waveforms of T samples read through the period view (H = ceil(T / p) rows of p columns, the
 * tail reflect-padded while reading, as dx_disc_first reads), dZ [R][Hout][p][Cout] -> dW (Cout, 1, taps), dW[co][t] = sum
 * x_view[b][m stride - pad + t][column] dZ[b][m][column][co], and db[co] = sum dZ.  Cout a divisor of 256, taps <= 16. */
int dx_disc_first_wgrad(const float* x, long sxb, int T, const float* dZ, float* dW, float* db, void* workspace, long workspace_bytes, int R,
                        int p, int Cout, int taps, int stride, int pad, void* stream);

/* ---- HiFi-GAN fine-tuning, the optimiser step (csrc/dx_vocoder_optim.hip) ---------------------------------------
 * Reference call sites: torch.optim.AdamW over generator.parameters() and over chain(msd.parameters(), mpd.parameters())
 * (vocoder/finetune_hifigan.py:130-135), optim_d.step() (:226), optim_g.step() (:243), with torch.nn.utils.weight_norm's backward and
 * fold around them.  One launch steps every tensor of one optimiser from a job table in DEVICE memory.
 *
 * A job is 11 longs on the host: kind, R, n, then the device addresses v, g, dW, m_v, s_v, m_g, s_g, W.
 *   kind 1, weight-normed: v (R, n) with contiguous rows, g (R), the norm over each row (torch._weight_norm(v, g, 0)); dW the gradient
 *     of the FOLDED weight in v's layout; m_*, s_* AdamW's exp_avg and exp_avg_sq of v and g; W (R, n) receives the folded weight.
 *     Per row: nrm = |v_r|, dg = <dW_r, v_r> / nrm, dv = (g / nrm) (dW_r - (dg / nrm) v_r); AdamW on (g, dg) and on (v_r, dv);
 *     W_r = g' v'_r / |v'_r| from the values as stored.  n <= 6144.  A row with |v_r| = 0 gives non-finite values, as torch does.
 *   kind 0, plain: AdamW on the n elements of v with the gradient dW and the moments m_v, s_v; R = 1; g, m_g, s_g, W are not read.
 * AdamW as torch defines it: p <- p (1 - lr wd); m <- b1 m + (1 - b1) grad; s <- b2 s + (1 - b2) grad^2;
 * p <- p - (lr / (1 - b1^step)) m / (sqrt(s) / sqrt(1 - b2^step) + eps); the factors are formed on the host in double.
 * v, dW, m_v, s_v, W 16-byte aligned, g, m_g, s_g 4-byte.  Fixed-order sums, no atomics: the result bits depend on the job alone, not
 * on the other jobs of the table. */
/* bytes of the table for these jobs (host memory, checked as dx_wn_adamw_table checks them) and the number of workgroups of a launch */
int dx_wn_adamw_table_size(const long* jobs, int njobs, long* bytes, int* blocks);
/* checks every job and lays the table out in HOST memory (`table`, `bytes` as reported); the caller copies it to the device */
int dx_wn_adamw_table(const long* jobs, int njobs, void* table, long bytes);
/* the step: in place on v, g and the moments, W written; table: the device copy; step >= 1, betas in [0, 1) */
int dx_wn_adamw(const void* table, int njobs, int blocks, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                void* stream);
/* W of every weight-normed job from its stored v and g, through the step's own fold code (the same bits); plain jobs are skipped */
int dx_wn_fold(const void* table, int njobs, int blocks, void* stream);

/* ---- HiFi-GAN fine-tuning batches from a device-resident corpus (reference vocoder/dataset.py:118-148; csrc/dx_finetune_data.hip) ----
 * The corpus: wav, every utterance's int16 samples (utterance u at wav + wav_off[u], wav_len[u] samples; every offset a multiple of 8
 * and the buffer padded to one, so that 16-byte loads stay inside it), and mel, every utterance's predicted mel as (n_mels, mel_len[u])
 * fp32 at mel + mel_off[u]; n_utt utterances.  One launch assembles B rows:
 *   utterance of row b: utts[b], or order[order_pos + b] when utts is NULL (order holds n_order entries);
 *   start frame of row b: starts_in[b], or, when starts_in is NULL, 0 for an utterance shorter than segment_size samples and otherwise
 *     (uint64(r >> 32) * n) >> 32 with r = dx_rand64(seed, counter | (by_utt ? utterance : b)) and n = mel_len - fps: a value of
 *     [0, mel_len - fps - 1], the range of the reference's randint;
 *   y[b][i] = wav[start * hop_size + i] / 32768 (exact) and x[b][c][f] = mel[c][start + f], i < segment_size, f < fps; samples and frames
 *     at or past the utterance's own length are 0 (torch's F.pad of a short utterance) and are never read.
 * starts_out, utts_out (optional, int32 [B]) receive what the row used.  An utterance index outside [0, n_utt) gives a row of zeros.
 * segment_size = fps * hop_size, hop_size % 8 == 0; wav and y 16-byte aligned.  Vector stores only, no atomics, no workspace: a row's
 * bits depend on its own (utterance, start) alone. */
int dx_ft_batch(const short* wav, const long* wav_off, const int* wav_len, const float* mel, const long* mel_off, const int* mel_len,
                int n_utt, const int* utts, const int* order, long order_pos, long n_order, const int* starts_in, uint64_t seed,
                uint64_t counter, int by_utt, float* x, float* y, int* starts_out, int* utts_out, int B, int segment_size, int hop_size,
                int fps, int n_mels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DAFT_EXPRT_HIP_H */

/* aaclip.h -- C ABI of libaaclip_hip.so: the MI355X (gfx950) AA-CLIP inference hot path.
 *
 * The reference (liu20050510/AA-CLIP-IQM) has no FFI of its own: its callers reach
 * into nn.Module attributes.  This header is therefore the boundary a binding for
 * the reference's hot path would use; every entry point names the reference code it
 * replaces (file:line under the reference root).  INTEGRATION.md shows the ctypes
 * stub a maintainer would add on the reference side.
 *
 * Conventions
 *  - All pointers are DEVICE pointers into memory owned by the caller (torch tensors
 *    on the Python side); the library allocates nothing it returns.  Scratch is a
 *    caller-provided workspace (aaclip_workspace_bytes).
 *  - `stream` is a hipStream_t passed as void*; every call only enqueues work on it.
 *  - `dtype` selects the arithmetic type of the matrix products:
 *      AACLIP_F32  exact fp32 MFMA (v_mfma_f32_32x32x2_f32), parity path
 *      AACLIP_F16 / AACLIP_BF16  16-bit operands, fp32 accumulate (v_mfma_f32_32x32x16)
 *      AACLIP_F16X2  split fp16: every matrix-product operand is carried as hi = fp16(v) plus a correction for v - hi
 *                    and a product is accumulated into one fp32 accumulator as main term + correction terms -- the mode
 *                    that meets 1e-3 abs + 1e-2 rel against the fp32 reference on taps and anomaly maps at MFMA speed.
 *                    GEMMs: A.W^T = Ah.Wh^T (fp16 MFMA) + Al8.Wh8^T + Ah8.Wl8^T (block-scaled e4m3 MFMA,
 *                    v_mfma_scale_f32_16x16x128_f8f6f4, twice the fp16 rate; the corrections are 2^-11 of the main
 *                    term, so 4 significant bits in them leave ~2^-15 per operand).  Attention: q.k^T = Kh.Qh + Kl.Qh
 *                    + Kh.Ql on the fp16 MFMAs, p.v with p and v in fp16.  Row formats, 4 bytes per element, row
 *                    strides counted in halves (>= 2C for a logical width C):
 *                      split8  [hi: C x fp16][lo8: C x e4m3 = (v - hi) * 2^10][hi8: C x e4m3 = v]
 *                              the A operand of aaclip_gemm, the context rows aaclip_attention writes, the output of
 *                              AACLIP_EPI_BIAS_GELU and of aaclip_layernorm(out_dtype = AACLIP_F16X2);
 *                              weights [out, in] likewise: [Wh: in x fp16][e4m3(W * 2^6)][e4m3((W - Wh) * 2^17)]
 *                      split16 [hi: C x fp16][lo: C x fp16 = v - hi]
 *                              the packed q|k|v rows aaclip_attention reads (C = 3 * H * 64) = the output of
 *                              AACLIP_EPI_BIAS.  (Inside aaclip_block / aaclip_blocks*, for rows of >= 512 tokens, q and k
 *                              travel from the QKV product to the attention kernel as fp16 + a 128-byte
 *                              [lo8 | hi8] e4m3 record per head instead, and the two correction products of q.k^T run
 *                              on v_mfma_scale_f32_32x32x64_f8f6f4 -- a workspace-internal format, not part of this
 *                              interface.)
 *                    e4m3 = OCP e4m3fn; the scales are fixed (activations 0.016 ... 448 and weights 2.4e-4 ... 7 keep
 *                    >= 4 significant bits in their correction operands; beyond, that element's correction degrades
 *                    towards plain fp16, never the main term).  A weight whose values are exact in fp16 (OpenAI's
 *                    CLIP checkpoints are stored in fp16) and whose in_features is a multiple of 256 may be passed
 *                    WITHOUT its last plane ([out, 3 * in] bytes) where an `exact16` flag exists
 *                    (aaclip_block_weights): the Ah8.Wl8^T product is then skipped.  K must be a multiple of 128.
 *    Weights of matrix products are passed already converted to `dtype`, row-major
 *    [out_features, in_features] exactly like nn.Linear.weight.  LayerNorm
 *    parameters, biases, embeddings, the residual stream and all outputs are fp32.
 *  - Return value: 0 on success, negative on error; aaclip_last_error() returns a
 *    thread-local message.  No exceptions cross the ABI.
 */
#ifndef AACLIP_H
#define AACLIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AACLIP_ABI_VERSION 10   /* 10: the block path's forms of the building blocks (aaclip_gemm_fused and the entries beside it) */

enum { AACLIP_F32 = 0, AACLIP_F16 = 1, AACLIP_BF16 = 2, AACLIP_F16X2 = 3 };
enum { AACLIP_ACT_NONE = 0, AACLIP_ACT_LEAKY = 1, AACLIP_ACT_RELU = 2,
       AACLIP_ACT_GELU = 3 /* aaclip_act_backward only */ };
/* generic GEMM epilogues (aaclip_gemm) */
enum { AACLIP_EPI_BIAS = 0, AACLIP_EPI_BIAS_GELU = 1, AACLIP_EPI_BIAS_RESID = 2, AACLIP_EPI_ACT_F32 = 3 };

int aaclip_version(void);            /* AACLIP_ABI_VERSION the library was built from; bind only if it matches */
const char* aaclip_last_error(void);

/* Scratch needed by any call below for `rows` token rows of width D, MLP width F,
 * embed width E (pass the largest you will use). */
size_t aaclip_workspace_bytes(int dtype, long rows, int D, int F, int E);

/* Weights of one ResidualAttentionBlock (reference model/transformer.py:183-258)
 * plus the optional residual adapter applied after it (model/adapter.py:163-170). */
typedef struct aaclip_block_weights {
  /* ABI version >= 3: sizeof(aaclip_block_weights) as the CALLER compiled it.  Every entry point that takes this
   * struct rejects (rc < 0, nothing launched) an element whose struct_bytes differs from the library's own sizeof, so
   * a binding generated from an older header (13 or 19 pointer fields, no size field: its first word is the ln1_w
   * pointer; or version 3's 20 fields without `exact16`) is refused instead of being read past its end. */
  size_t struct_bytes;
  const float* ln1_w;   /* [D] */
  const float* ln1_b;
  const void* qkv_w;    /* attn.in_proj_weight [3D, D], dtype */
  const float* qkv_b;   /* attn.in_proj_bias [3D] */
  const void* out_w;    /* attn.out_proj.weight [D, D], dtype */
  const float* out_b;
  const float* ln2_w;
  const float* ln2_b;
  const void* fc_w;     /* mlp.c_fc.weight [F, D], dtype */
  const float* fc_b;
  const void* proj_w;   /* mlp.c_proj.weight [D, F], dtype */
  const float* proj_b;
  const void* adapter_w; /* SimpleAdapter fc.0.weight [D, D], dtype; NULL = no adapter */
  /* Optional (all three or none; ABI version >= 2): ln_2 folded into c_fc.  When present and the block runs
   * on the large-batch 16-bit kernels, the ln_2 pass disappears: out_proj's epilogue also emits the new
   * residual rows in `dtype` with per-row sums, and c_fc computes
   *   rstd_m * (x16 . fc_w_fold^T)_mn - rstd_m * mean_m * fc_fold_s[n] + fc_fold_b[n]
   * which equals c_fc(ln_2(x)) up to rounding.  Otherwise the fields are ignored. */
  const void* fc_w_fold;  /* [F, D] dtype: c_fc.weight * ln_2.weight[None, :] */
  const float* fc_fold_s; /* [F]: row sums of fc_w_fold (as stored, in fp32) */
  const float* fc_fold_b; /* [F]: c_fc.bias + c_fc.weight @ ln_2.bias */
  /* The same for ln_1 and the QKV product; used by aaclip_blocks for every block after the first of a call
   * (the previous block's last epilogue, or its adapter mix, emits the 16-bit rows and their statistics). */
  const void* qkv_w_fold;  /* [3D, D] dtype: in_proj_weight * ln_1.weight[None, :] */
  const float* qkv_fold_s; /* [3D] */
  const float* qkv_fold_b; /* [3D]: in_proj_bias + in_proj_weight @ ln_1.bias */
  /* ABI version >= 4, AACLIP_F16X2 only (ignored otherwise): bit mask of the matrix weights above that are passed in
   * the 3-plane form (fp16 plane + e4m3 plane, 3 bytes per element) because every value is exact in fp16; the others
   * carry all three planes (4 bytes per element). */
  unsigned exact16;
} aaclip_block_weights;
enum { AACLIP_EXACT16_QKV = 1, AACLIP_EXACT16_OUT = 2, AACLIP_EXACT16_FC = 4, AACLIP_EXACT16_PROJ = 8,
       AACLIP_EXACT16_ADAPTER = 16 };

/* Patch embedding + class token + positional embedding + ln_pre.
 * Replaces reference model/adapter.py:139-156 (== model/transformer.py:507-526).
 * img [B,3,H,W] fp32 NCHW; conv_w = conv1.weight reshaped [D, 3*ps*ps] and zero
 * padded to [D, Kpad], Kpad = round_up(3*ps*ps, 64), dtype; pos [L, D];
 * x (out) [B*L, D] fp32 with L = (H/ps)*(W/ps)+1 (pixels behind the last whole patch are not read).  The unfolded
 * patch rows in the workspace are zero padded to Kpad by the library itself.  Kpad <= 640; AACLIP_F16X2 needs Kpad to
 * be a multiple of 128.  A rejected call (rc < 0) launches nothing. */
int aaclip_patch_embed(const float* img, const void* conv_w, const float* cls, const float* pos,
                       const float* ln_pre_w, const float* ln_pre_b, float* x, int B, int H, int W, int ps, int D,
                       int dtype, void* ws, size_t ws_bytes, void* stream);

/* One pre-LN residual attention block, in place on the fp32 residual stream
 * x [B*L, D]:  x += out_proj(MHA(ln_1 x));  x += c_proj(gelu_erf(c_fc(ln_2 x)));
 * then, if w->adapter_w: a = LeakyReLU(x Wa^T); x = mix*a*|x|/|a| + (1-mix)*x.
 * Replaces ResidualAttentionBlock.forward (reference model/transformer.py:239-258,
 * nn.MultiheadAttention at :200,237) and the adapter lines model/adapter.py:162-170
 * (visual, AACLIP_ATTN_FULL) / :285-295 (text, AACLIP_ATTN_CAUSAL: mask of model/transformer.py:629-635).
 * AACLIP_ATTN_VV_BATCH: the block after VisionTransformer.DAPM_replace (reference
 * model/transformer.py:406-425): its attention is the "surgery" module (:102-152) with
 * q = k = v = value projection, which -- fed the LND stream -- attends over the BATCH axis per
 * token position.  Reproduced as the reference runs it (outputs depend on the batch); needs F >= 4*D.
 * H heads of 64; D = 64*H. */
enum { AACLIP_ATTN_FULL = 0, AACLIP_ATTN_CAUSAL = 1, AACLIP_ATTN_VV_BATCH = 2 };
int aaclip_block(float* x, const aaclip_block_weights* w, float mix, int B, int L, int D, int H, int F, int attn_mode,
                 int dtype, void* ws, size_t ws_bytes, void* stream);

/* n_blocks consecutive blocks (w[0..n_blocks-1], same mix / shape / attn_mode) in one call, in place on x.
 * Identical to n_blocks aaclip_block calls, except that nothing else can touch x in between, which lets the
 * library fold ln_1 of blocks 1..n-1 into their QKV products (see aaclip_block_weights).  Callers split the
 * tower at the layers whose output they read (reference model/adapter.py:171-172 taps). */
int aaclip_blocks(float* x, const aaclip_block_weights* w, int n_blocks, float mix, int B, int L, int D, int H, int F,
                  int attn_mode, int dtype, void* ws, size_t ws_bytes, void* stream);

/* As aaclip_blocks, but the stream is READ from x_in, which stays untouched, and continued in x (the first residual
 * update reads x_in and writes x; x_in == x is aaclip_blocks).  This is how a caller keeps the tower's state at a
 * tap layer -- CLIP.encode_image(image, out_layers), reference model/transformer.py:295-317 -- without copying it:
 * the tap tensor is the buffer the previous run wrote, the next run writes a fresh one. */
int aaclip_blocks_to(const float* x_in, float* x, const aaclip_block_weights* w, int n_blocks, float mix, int B, int L,
                     int D, int H, int F, int attn_mode, int dtype, void* ws, size_t ws_bytes, void* stream);

/* A whole tower with taps in ONE call: x_out[i] is the buffer that holds the stream AFTER block i; block i reads
 * the stream from x_in (i = 0) or from x_out[i-1] and writes x_out[i] (in place when they are the same buffer; a buffer
 * that is not written again keeps the tower's state at that layer).  Equivalent to one aaclip_blocks_to call per run
 * of blocks between taps, except that the library sees the whole sequence, so ln_1 of the first block after a tap is
 * folded into its QKV product like every other (those calls run it as a LayerNorm pass: nothing tells them that the
 * workspace still holds the previous call's rows).  Reference: model/transformer.py:295-317 (out_layers),
 * model/adapter.py:160-172 (levels). */
int aaclip_blocks_taps(const float* x_in, float* const* x_out, const aaclip_block_weights* w, int n_blocks, float mix,
                       int B, int L, int D, int H, int F, int attn_mode, int dtype, void* ws, size_t ws_bytes,
                       void* stream);

/* Tap head: ln_post -> seg_proj (Linear no bias [+LeakyReLU]) -> F.normalize, CLS row
 * dropped.  Replaces reference model/adapter.py:171-182.  x [B*L, D] fp32 (tap of the
 * residual stream); proj_w [E, D] dtype; seg_out [B, L-1, E] fp32 unit rows.
 * If det_w != NULL also writes det_out [B, E] = mean over patches of
 * F.normalize(det_proj(ln_post x)) (model/adapter.py:183-184). */
int aaclip_tap_head(const float* x, const float* ln_post_w, const float* ln_post_b, const void* proj_w, int act,
                    float* seg_out, const void* det_w, float* det_out, int B, int L, int D, int E, int dtype, void* ws,
                    size_t ws_bytes, void* stream);

/* The same, and the LayerNorm'ed rows ln_post(x) [B*L, D] are left in ln_rows_out in the layout of `dtype` (fp32 /
 * fp16 / bf16 rows of D elements; AACLIP_F16X2: split8 rows of 4 D bytes whose first 2 D bytes are the fp16 values):
 * the IQM branch reads exactly these rows again (reference model/adapter.py:205-208 applies ln_post to every tap a
 * second time), so they are computed once. */
int aaclip_tap_head_keep_rows(const float* x, const float* ln_post_w, const float* ln_post_b, const void* proj_w, int act,
                              float* seg_out, const void* det_w, float* det_out, void* ln_rows_out, int B, int L, int D,
                              int E, int dtype, void* ws, size_t ws_bytes, void* stream);

/* Detection head alone (reference model/adapter.py:183-184). */
int aaclip_det_head(const float* x, const float* ln_post_w, const float* ln_post_b, const void* det_w, int act,
                    float* det_out, int B, int L, int D, int E, int dtype, void* ws, size_t ws_bytes, void* stream);

/* Fused test-mode anomaly map over NL tap levels: per level s = 100 f.t,
 * m = (s1 + 1 - s0)/2, Gaussian blur (ksize, sigma; reflect), bilinear
 * align_corners=True to S x S; out [B,S,S] = sum over levels.  Replaces
 * calculate_similarity_map(test=True) (reference forward_utils.py:196-213) applied per
 * level and the level sum of test_last.py:95-100,149.  seg[l] [B, g*g, E] unit rows;
 * anchors [E,2] (anchor_bstride 0) or [B,E,2] (anchor_bstride E*2).  NL <= 4, g <= 40.
 * ksize 1 skips the blur. */
int aaclip_anomaly_map(const float* const* seg, int NL, const float* anchors, long anchor_bstride, float* out, int B,
                       int g, int E, int S, int ksize, float sigma, void* ws, size_t ws_bytes, void* stream);

/* Train-mode similarity map: bilinear on both channels then softmax over C=2,
 * out [B,2,S,S].  Replaces calculate_similarity_map(test=False)
 * (reference forward_utils.py:199-203,211-215). */
int aaclip_similarity_map_train(const float* seg, const float* anchors, long anchor_bstride, float* out, int B, int g,
                                int E, int S, void* ws, size_t ws_bytes, void* stream);

/* ---- Training: the loss side of the text-adapter stage (reference train.py:38-114, SURVEY.md 8 / VERDICT.md #5).
 * Every reduction runs in a fixed order (no float atomics): repeated calls give bit-identical results. */

/* Backward of aaclip_similarity_map_train.  preds = its output [B,2,S,S], d_preds = d loss / d preds (same shape):
 * softmax backward per pixel, the transpose of the align-corners bilinear upsample (a gather over each coarse cell's
 * support window), x100, then
 *   d_anchors[b, e, c] = sum_p seg[b, p, e] dS[b, p, c]   ([B, E, 2]; anchor_bstride 0: one [E, 2] pair, summed over b)
 *   d_seg[b, p, e]     = sum_c dS[b, p, c] anchors[b, e, c]
 * Either output may be NULL.  g <= 40, S <= 2048, E a supported row width. */
size_t aaclip_similarity_map_train_backward_workspace_bytes(int B, int g, int S);
int aaclip_similarity_map_train_backward(const float* seg, const float* anchors, long anchor_bstride,
                                         const float* preds, const float* d_preds, float* d_anchors, float* d_seg,
                                         int B, int g, int E, int S, void* ws, size_t ws_bytes, void* stream);

/* The IQM map term of the stage-2 loss (reference train.py:173-212), one tap level per call.
 *   p[b, i]      = sigmoid(cos(seg[b, i], queries[b, 1]) - cos(seg[b, i], queries[b, 0]))     (row 0 normal, 1 abnormal)
 *   out[b, 1]    = half-pixel (align_corners=False) bilinear upsample of p to S x S: bit-identical to aaclip_iqm_map
 *                  with this one level, w_iqm = 1 and no base
 *   out[b, 0]    = the same interpolation of the values 1 - p (the reference interpolates the concatenated pair)
 * seg [B, g*g, E], queries [B, 2, E], grid_out [B, g*g] (= p, kept for the backward), out [B, 2, S, S]; all fp32 and
 * 16-byte aligned.  g <= 40, S <= 2048, E a supported row width.
 * cos is F.cosine_similarity's x.y / sqrt(max(|x|^2 |y|^2, 1e-16)). */
int aaclip_iqm_map_train(const float* seg, const float* queries, float* grid_out, float* out, int B, int g, int E, int S,
                         void* stream);
/* Its backward: d_preds [B, 2, S, S] -> d_seg [B, g*g, E] and d_queries [B, 2, E]; either may be NULL, not both.
 *   dU = d_preds[:, 1] - d_preds[:, 0]; the transpose of the half-pixel upsample as a gather over each coarse cell's
 *   support window (coarse index 0 collects every fine index whose source clamps to 0, the last one both terms);
 *   dz = p (1 - p) dgrid;
 *   d_seg[b, i]     = dz_i [(q1 / (|f||q1|) - c1 f / |f|^2) - (q0 / (|f||q0|) - c0 f / |f|^2)]
 *   d_queries[b, 1] = sum_i (dz_i / |f_i|) f_i / |q1| - (sum_i dz_i c1_i) q1 / |q1|^2, row 0 likewise with q0, c0 and
 *                     the opposite sign; the sum over i in 32 chunks, reduced in chunk order.
 * Degenerate rows: the gradient is that of the function the forward computes.  Where |f|^2 |q|^2 <= 1e-16 the clamp is
 * active and the denominator is a constant 1e-8: only the x.y term is differentiated, the c f / |f|^2 and c q / |q|^2
 * terms are absent (torch clamps the two norms separately there and differs).  Every output stays finite.
 * The same checks as the forward, all before the first launch; the workspace size is the last one. */
size_t aaclip_iqm_map_train_backward_workspace_bytes(int B, int g, int E, int S);
int aaclip_iqm_map_train_backward(const float* seg, const float* queries, const float* grid, const float* d_preds,
                                  float* d_seg, float* d_queries, int B, int g, int E, int S, void* ws, size_t ws_bytes,
                                  void* stream);

/* Segmentation loss, reference forward_utils.py:21-108,223-227 (calculate_seg_loss = FocalLoss + BinaryDiceLoss on
 * channel 0 against 1 - mask + BinaryDiceLoss on channel 1 against mask):
 *   focal = mean over B*P pixels of -(1 - pt)^2 log pt,  pt = sum_c clamp(onehot_c, 1e-5, 1 - 1e-5) p_c + 1e-5
 *           (gamma 2, alpha 1; the class of a pixel is its mask value truncated: masks hold 0 / 1)
 *   dice0 = 1 - mean_b (2 sum p0 (1 - m) + 1) / (sum p0 + sum (1 - m) + 1),  dice1 likewise with p1 and m.
 * preds: channel c of image b at preds + b * img_stride + c * chan_stride (P pixels; [B,2,S,S]: P, 2P, P), mask
 * [B, P] fp32.  terms: the AACLIP_SEG_LOSS_* that are computed (the others read 0).  loss (out, device) [4] =
 * {focal + dice0 + dice1, focal, dice0, dice1}; coef (out) [B, 4]: per-image dice coefficients the backward reads.
 * Two passes: per (image, pixel chunk) sums, then a one-block pass over the chunks in order (double). */
enum { AACLIP_SEG_LOSS_FOCAL = 1, AACLIP_SEG_LOSS_DICE0 = 2, AACLIP_SEG_LOSS_DICE1 = 4, AACLIP_SEG_LOSS_ALL = 7 };
size_t aaclip_seg_loss_workspace_bytes(int B);
int aaclip_seg_loss(const float* preds, long img_stride, long chan_stride, const float* mask, int terms, float* loss,
                    float* coef, int B, long P, void* ws, size_t ws_bytes, void* stream);
/* d_preds (same layout as preds) from d_loss (device [4], the gradient of the loss vector) and the forward's coef.
 * A channel that no computed term reads is not written, so chan_stride 0 is allowed for the single dice terms. */
int aaclip_seg_loss_backward(const float* preds, long img_stride, long chan_stride, const float* mask, int terms,
                             const float* coef, const float* d_loss, float* d_preds, int B, long P, void* stream);

/* ---- Training: backward of the adapted text tower (reference model/adapter.py:273-304 under train.py:62-68,97-100).
 * Everything below is fp32 whatever dtype the forward ran in (the reference trains in fp32), uses no float atomics and
 * sums in a fixed order: repeated calls give bit-identical results.  Only the text_adapter weights receive gradients;
 * CLIP's own parameters are frozen, so no bias, LayerNorm-parameter or CLIP weight gradient is formed.
 * Workspace: every entry point below that takes one accepts aaclip_text_backward_workspace_bytes(rows, D, F) bytes,
 * rows = the token rows it is given and D = the width of those rows (aaclip_gemm_wgrad: D = I, its input features, and
 * F = 0; aaclip_row_head_backward: rows = n*T, F = 0).  Monotonic in rows.
 * Alignment: fp32 rows move as 16-byte vectors, so every fp32 pointer passed below (and the workspace) must be 16-byte
 * aligned; a misaligned pointer is rejected (rc < 0). */
size_t aaclip_text_backward_workspace_bytes(long rows, int D, int F);

/* Weight gradient of y = u W^T over an arbitrary number of rows: dw[o, i] = sum_r dz[r, o] u[r, i] on the exact-fp32
 * MFMA.  dz [rows, ldz >= O], u [rows, ldu >= I], dw [O, I] (overwritten); O and I multiples of 128, O <= 1024, strides multiples
 * of 4, pointers 16-byte aligned.  The rows are split into at most 16 chunks whose partial products a second pass adds
 * in order. */
int aaclip_gemm_wgrad(const float* dz, long ldz, const float* u, long ldu, float* dw, long rows, int O, int I, void* ws,
                      size_t ws_bytes, void* stream);

/* Backward of aaclip_attention(AACLIP_F32): from the packed q|k|v rows [B*L, 3*H*64] (q pre-scaled, as the forward
 * takes it) and d_ctx [B*L, H*64] to d_qkv [B*L, 3*H*64]; the dq columns are multiplied by dq_scale (pass the q scale to
 * get the gradient of the unscaled projection, 1 otherwise).  Probabilities are recomputed on chip.  Head dim 64,
 * causal != 0 = the text tower's mask, every L <= 128; anything else is rejected before a launch. */
int aaclip_attention_backward(const float* qkv, const float* d_ctx, float* d_qkv, int B, int L, int H, int causal,
                              float dq_scale, void* stream);

/* The same gradients for ANY L >= 1 (the visual tower's 1370 rows), in three tiled passes on the exact-fp32 MFMA: row
 * statistics (maximum, 1 / sum, delta; 3*B*H*L floats in the workspace), then dk | dv, then dq.  Nothing of size L x L
 * reaches memory; no atomics, every output element is summed by one wave in a fixed order.  Layouts, dq_scale and the
 * alignment rule as above (the workspace is 16-byte aligned too).  ws_bytes >=
 * aaclip_attention_backward_long_workspace_bytes(B, L, H), which is 0 for an empty problem and monotonic in each
 * argument.  Null pointers, empty problems, B or H above 65535, misaligned pointers and a short workspace are rejected
 * before a launch.  aaclip_attention_backward is unchanged: its arithmetic differs (VALU chains), so the two agree to
 * rounding, not bit for bit. */
size_t aaclip_attention_backward_long_workspace_bytes(int B, int L, int H);
int aaclip_attention_backward_long(const float* qkv, const float* d_ctx, float* d_qkv, int B, int L, int H, int causal,
                                   float dq_scale, void* ws, size_t ws_bytes, void* stream);

/* LayerNorm input gradient (weight and bias are frozen): d_x = d_resid + dLN(x; w)^T d_y, d_resid may be NULL; d_x may
 * alias d_y or d_resid. */
int aaclip_layernorm_backward(const float* x, const float* w, const float* d_y, const float* d_resid, float* d_x,
                              long rows, int D, float eps, void* stream);

/* Backward of the adapter mix y = weight * a |u| / |a| + (1 - weight) * u with a = LeakyReLU(z), z = u Wa^T
 * (aaclip_adapter_mix; both norms are functions of the inputs): d_z for the weight gradient (and for d_z Wa, the part of
 * d u that runs through the product) and the direct d_u.  d_z may alias z, d_u may alias d_y.  LeakyReLU's derivative is
 * 1 for z > 0 and 0.01 for z <= 0 here and in every backward below: the kink itself takes the negative side's slope,
 * like the backward of torch's leaky_relu (AACLIP_ACT_RELU: 0 at 0). */
int aaclip_adapter_mix_backward(const float* u, const float* z, const float* d_y, float* d_z, float* d_u, long rows,
                                int D, float weight, void* stream);

/* Backward of one aaclip_block (AACLIP_ATTN_FULL or AACLIP_ATTN_CAUSAL, L <= 128) from its INPUT x_in [B*L, D]: the
 * block's internals are recomputed in fp32, nothing else needs to be kept from the forward.  w: the block's weights as
 * AACLIP_F32; wt: a second struct whose matrix fields (qkv_w, out_w, fc_w, proj_w, adapter_w) hold the TRANSPOSED fp32
 * weights [in_features, out_features] -- the input-gradient products are aaclip_gemm(AACLIP_F32) calls on them; its
 * other fields are ignored, and it is not read when d_in is NULL.  d_out [B*L, D]: gradient of the block's output.
 * d_in (out): gradient of x_in; may alias d_out; NULL = not wanted (then only the adapter's weight gradient is formed).
 * d_adapter_w (out) [D, D] fp32, overwritten; required when w->adapter_w is set, ignored otherwise. */
int aaclip_block_backward(const float* x_in, const aaclip_block_weights* w, const aaclip_block_weights* wt, float mix,
                          int B, int L, int D, int H, int F, int attn_mode, const float* d_out, float* d_in,
                          float* d_adapter_w, void* ws, size_t ws_bytes, void* stream);

/* aaclip_block_backward without the limit on L (the visual tower: L = 1370, D = 1024, F = 4096): the same walk with
 * aaclip_attention_backward_long in the attention step, every other launch identical.  Same arguments; ws_bytes >=
 * aaclip_block_backward_long_workspace_bytes(B, L, D, F) = the text-backward layout for B*L rows plus the attention
 * statistics (0 for an empty problem).  Error messages carry the "block_backward:" prefix of the short form. */
size_t aaclip_block_backward_long_workspace_bytes(int B, int L, int D, int F);
int aaclip_block_backward_long(const float* x_in, const aaclip_block_weights* w, const aaclip_block_weights* wt,
                               float mix, int B, int L, int D, int H, int F, int attn_mode, const float* d_out,
                               float* d_in, float* d_adapter_w, void* ws, size_t ws_bytes, void* stream);

/* ---- bf16x3: a second, opt-in arithmetic for the backward of the visual blocks.  A value v is carried as
 * hi = bf16(v), lo = bf16(v - hi) (round to nearest even; bf16 has fp32's exponent, so there is no scale anywhere) and a
 * product is summed as Ah.Bh + Al.Bh + Ah.Bl in fp32 accumulators on the bf16 MFMA: about 16 significant bits per
 * operand over fp32's whole range, at 3/16 of the matrix-pipe time of the exact-fp32 MFMA.  The fp32 entry points above
 * are unchanged and stay the default; nothing selects these by itself.
 *
 * aaclip_split3_rows: fp32 src [rows, K] -> bf16 dst [rows, 3K] = [hi | lo | hi] per row, the A operand of
 * aaclip_gemm(AACLIP_BF16) over K' = 3K against a stacked weight [N, 3K] = [Wh | Wh | Wl]: one plain bf16 product
 * then accumulates exactly the three terms.  K a multiple of 64, pointers 16-byte aligned. */
int aaclip_split3_rows(const float* src, void* dst, long rows, int K, void* stream);

/* aaclip_attention_backward_long in this arithmetic: the same arguments, layouts (fp32 in, fp32 out), masks, dq_scale
 * and refusals; the same three passes (statistics, dk | dv, dq) behind a pre-pass that writes the hi and lo planes of q,
 * k, v and d_ctx into the workspace.  The row statistics, the exponent and ds = p (dp - delta) are fp32; p and ds are
 * split in registers.  No atomics, nothing of size L x L in memory, every output element summed by one wave in a fixed
 * order: repeated calls give the same bits.  The workspace holds the statistics and the planes
 * (1024 bytes per image, head and row). */
size_t aaclip_attention_backward_long_bf16x3_workspace_bytes(int B, int L, int H);
int aaclip_attention_backward_long_bf16x3(const float* qkv, const float* d_ctx, float* d_qkv, int B, int L, int H,
                                          int causal, float dq_scale, void* ws, size_t ws_bytes, void* stream);

/* aaclip_block_backward_long in this arithmetic: the same recomputation from x_in in the same order.  The eight
 * products of the block proper (in_proj, out_proj, c_fc, c_proj and their four input-gradient products) run as bf16
 * products over 3K on split3 rows, the attention backward is the entry above; the recomputed forward attention, the
 * adapter's three products and every row op are the fp32 kernels of aaclip_block_backward_long.  Which field is read
 * from which struct, and as what:
 *   w    fp32: ln1_w, ln1_b, out_b, ln2_w, ln2_b, fc_b, proj_b, adapter_w [D, D] (NULL = no adapter).  Its qkv_w, qkv_b,
 *        out_w, fc_w and proj_w are not read.
 *   w3   bf16 stacked weights [N, 3K] = [Wh | Wh | Wl]: qkv_w [3D, 3D] with its first D rows (q) times 1/8, out_w
 *        [D, 3D], fc_w [F, 3D], proj_w [D, 3F]; fp32: qkv_b [3D] with its first D entries times 1/8 (the q scale is a
 *        power of two, so this is exact and qkv comes out pre-scaled without a column scale in the epilogue).  Nothing
 *        else is read.
 *   wt3  bf16 stacked TRANSPOSED weights (unscaled): qkv_w [D, 9D], out_w [D, 3D], fc_w [D, 3F], proj_w [F, 3D]; fp32:
 *        adapter_w [D, D], the transposed adapter weight.  Not read when d_in is NULL.
 * d_out, d_in (may alias d_out, may be NULL), d_adapter_w and mix as in aaclip_block_backward.  Rejected before a launch:
 * null pointers, D != 64*H, a bad attn_mode, F not a multiple of 128, a row width the row kernels do not take, misaligned
 * pointers and ws_bytes < aaclip_block_backward_long_bf16x3_workspace_bytes(B, L, D, F). */
size_t aaclip_block_backward_long_bf16x3_workspace_bytes(int B, int L, int D, int F);
int aaclip_block_backward_long_bf16x3(const float* x_in, const aaclip_block_weights* w, const aaclip_block_weights* w3,
                                      const aaclip_block_weights* wt3, float mix, int B, int L, int D, int H, int F,
                                      int attn_mode, const float* d_out, float* d_in, float* d_adapter_w, void* ws,
                                      size_t ws_bytes, void* stream);

/* Backward of aaclip_row_head(AACLIP_F32): x, tokens, ln_w, ln_b, act, mode as there; proj_w [E, D] and its transpose
 * proj_wt [D, E] in fp32 (proj_wt may be NULL when d_x is); d_out [n, E].  d_proj_w (out) [E, D], overwritten.  d_x
 * (out, may be NULL) [n*T, D]: zero except the n picked rows, which receive the LayerNorm input gradient -- a scatter of
 * n distinct rows.  E a multiple of 128, <= 1024. */
int aaclip_row_head_backward(const float* x, const int32_t* tokens, const float* ln_w, const float* ln_b,
                             const float* proj_w, const float* proj_wt, int act, const float* d_out, float* d_x,
                             float* d_proj_w, int n, int T, int D, int E, int mode, void* ws, size_t ws_bytes,
                             void* stream);

/* ---- Training: backward of the tap and det heads (reference model/adapter.py:171-184 under train.py:150-163), the
 * first step of stage 2 behind the loss.  Same rules as the text-tower backward above: fp32 whatever dtype the forward
 * ran in, no float atomics, fixed summation order (repeated calls give bit-identical results), every fp32 pointer and
 * the workspace 16-byte aligned, every check before the first launch.
 *
 * Backward of aaclip_tap_head(AACLIP_F32) from the tap stream x [B*L, D] (CLS row included): ln_post(x), the projection
 * rows and their norms are recomputed, nothing is kept from the forward.  proj_w [E, D] and its transpose proj_wt [D, E];
 * d_seg [B, L-1, E]: gradient of the unit patch rows.  det_w / det_wt / d_det [B, E] / d_det_w: the det head of the same
 * stream (aaclip_tap_head's det_w) -- det_w, d_det and d_det_w are given together or all NULL (det_wt NULL too).  d_seg may
 * be NULL when the det part is present (proj_w, proj_wt and d_proj_w are then ignored): that is the backward of
 * aaclip_det_head.  One of the two parts must be present.
 * d_proj_w (out) [E, D] and d_det_w (out) [E, D] are overwritten.  d_x (out) [B*L, D], overwritten, CLS rows exactly
 * zero; may be NULL when only the projections train -- then proj_wt / det_wt may be NULL too and no input-gradient
 * product runs.  Otherwise the transpose of every part that is present is required.
 * D, E supported row widths (256, 512, 768, 1024), L > 1, B*L <= 2^26 - 4, act one of AACLIP_ACT_*.
 * ws_bytes >= aaclip_tap_head_backward_workspace_bytes(B, L, D, E): 0 for an empty problem, monotonic in each
 * argument.  Errors carry the "tap_head_backward:" prefix.
 * The IQM branch's backward: its key / value side in the projected form, from the gradient of the cross-attention's
 * weighted row sums to query_adapters and the tap streams (aaclip_cross_rows_backward below plus aaclip_gemm_wgrad,
 * aaclip_gemm and aaclip_layernorm_backward; aaclip_hip/autograd.py iqm_visual_rows), the 2-row query side (the entries
 * under "Backward building blocks of the IQM branch's query side"), and the folded 16-bit aaclip_cross_rows_levels form
 * that inference runs at the defaults (aaclip_cross_rows_levels_backward; aaclip_hip/autograd.py IqmQueriesFolded,
 * selected by AACLIP_IQM_TRAIN_FORM=folded) -- see DESIGN.md section 10. */
size_t aaclip_tap_head_backward_workspace_bytes(int B, int L, int D, int E);
int aaclip_tap_head_backward(const float* x, const float* ln_post_w, const float* ln_post_b, const float* proj_w,
                             const float* proj_wt, int act, const float* d_seg, const float* det_w, const float* det_wt,
                             const float* d_det, float* d_x, float* d_proj_w, float* d_det_w, int B, int L, int D, int E,
                             void* ws, size_t ws_bytes, void* stream);

/* Image pre-processing in front of the patch embed: Pillow's 8-bit BICUBIC resize to S x S,
 * ToTensor (v/255) and Normalize((v - mean)/std), bit-exact.  Replaces the reference's
 * dataset transform (reference dataset/__init__.py:150-161 and :62-71: transforms.Resize(
 * (S,S), Image.BICUBIC) -> ToTensor -> Normalize), which runs in the DataLoader workers on CPU.
 *   aaclip_resample_ksize / aaclip_resample_table are HOST functions: they fill host buffers
 *   bounds[2*out] (first source index, tap count) and coefs[out*ksize] (22-bit fixed point) with
 *   Pillow's weights for one axis; the caller uploads them once per (source size, S).
 *   aaclip_preprocess: src uint8 [B,Hs,Ws,3] (HWC, device), tables for the horizontal (Ws -> S)
 *   and vertical (Hs -> S) pass (device), lut fp32 [3,256] = normalised value of every byte per
 *   channel (device), out fp32 [B,3,S,S]. */
int aaclip_resample_ksize(int in_size, int out_size);
int aaclip_resample_table(int in_size, int out_size, int32_t* bounds, int32_t* coefs);
int aaclip_preprocess(const uint8_t* src, int B, int Hs, int Ws, int S, const int32_t* hbounds, const int32_t* hcoefs,
                      const int32_t* vbounds, const int32_t* vcoefs, const float* lut, float* out, void* stream);

/* Buffers of a call.  For the data-side entries below -- the input work, the metrics and their bootstrap, the optimiser's
 * gradient norm, the support bank, the coreset, tiles, overlays and PNG encoding -- one rule holds, checked before the
 * first launch: every buffer the call WRITES (outputs, records, the workspace, over the lengths stated at the entry, the
 * workspace over its *_workspace_bytes) shares no byte with any other buffer of the call; buffers the call only reads may
 * alias one another.  A NULL or empty buffer overlaps nothing, and a range may end on the last byte of the address space.
 * A refusal carries the entry's name and the word "overlap".  Two entries take an in-place form, named where they are
 * described: aaclip_color_jitter with dst == src and aaclip_metrics_normalise with out == scores; a partial overlap of
 * the two is refused.  The rule covers these pairs, which earlier revisions of the library let through:
 *   aaclip_metrics_sort        keys x labels, labels_sorted x scores, out_of_range x scores, out_of_range x labels
 *   aaclip_metrics_range       image_max x labels, record x labels
 *   aaclip_metrics_normalise   out x range_record
 *   aaclip_color_jitter        ws x src, dst, factors, apply; dst x factors, apply
 *   aaclip_augment_geometric   image_out, mask_out x angle_deg, shift, flags
 *   aaclip_optim_grad_norm     record, workspace x every tensor's gradient
 *   aaclip_support_map         ws x out, base, the level pointers; out x the level pointers
 *   aaclip_png_encode          workspace x pixels, payload, offsets; payload x offsets
 * Alignment is checked on every pointer that is given, from the same table (csrc/buffers.h). */

/* Train-time input work on raw frames (reference dataset/__init__.py:37-102).  The reference draws its random numbers
 * inside DataLoader workers; here every drawn number is an argument, so a call is a pure function of its inputs and two
 * calls give the same bits.  All checks run before the first launch.  Errors carry the entry point's name as prefix.
 *   aaclip_color_jitter: src / dst uint8 [B,H,W,3] (device; dst == src is allowed, a partial overlap is not: "Buffers of a call").  Per
 *   frame b: factors[3b .. 3b+2] = brightness, contrast, saturation factor (fp32, device), apply[b] bit 0 / 1 / 2 =
 *   run that step (int32, device); a clear bit skips the step.  Each step is Pillow's ImageEnhance: blend(degenerate,
 *   image, factor) = fp32 d + f * (s - d), clipped to [0, 255], truncated; degenerate = 0 (brightness), the constant
 *   int(mean(L) + 0.5) of the frame after its brightness step (contrast), the pixel's own L (saturation);
 *   L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  The mean is an exact integer sum.  ws 8-byte aligned,
 *   ws_bytes >= aaclip_color_jitter_workspace_bytes(B, H, W) (0 for an empty problem).
 *   aaclip_nearest_table is a HOST function: idx[out_size] = source index of every output index under Pillow's NEAREST
 *   resize of one axis (identity for equal sizes); the caller uploads it.
 *   aaclip_mask_preprocess: src uint8 [B,Hm,Wm] (device) -> out fp32 [B,1,S,S], 1 where the NEAREST-resized mask is
 *   non-zero: Resize((S,S), NEAREST) -> ToTensor -> (!= 0).  xmap [S] / ymap [S]: aaclip_nearest_table(Wm / Hm, S) on
 *   the device (entries are clamped into the source).  normal int32 [B] (device) or NULL: a non-zero entry writes
 *   zeros for that frame without reading its source.
 *   aaclip_augment_geometric: image fp32 [B,3,S,S], mask fp32 [B,1,S,S] -> image_out, mask_out of the same shapes, none
 *   overlapping another.  Per frame (device arrays): angle_deg fp32 [B], shift int32 [B,2] = (tx, ty), flags int32 [B]:
 *   bit 0 rotate by angle_deg (counter-clockwise, about the centre), bit 1 shift by (tx, ty), bit 2 horizontal flip,
 *   bit 3 vertical flip -- applied in that order, nearest sampling, zero fill, as torchvision's RandomRotation /
 *   RandomAffine / RandomHorizontalFlip / RandomVerticalFlip do on a tensor.  One gather per output pixel composes the
 *   four; the rotation's source coordinate is evaluated in fp64. */
size_t aaclip_color_jitter_workspace_bytes(int B, int H, int W);
int aaclip_color_jitter(const uint8_t* src, uint8_t* dst, int B, int H, int W, const float* factors,
                        const int32_t* apply, void* ws, size_t ws_bytes, void* stream);
int aaclip_nearest_table(int in_size, int out_size, int32_t* idx);
int aaclip_mask_preprocess(const uint8_t* src, int B, int Hm, int Wm, int S, const int32_t* xmap, const int32_t* ymap,
                           const int32_t* normal, float* out, void* stream);
int aaclip_augment_geometric(const float* image, const float* mask, int B, int S, const float* angle_deg,
                             const int32_t* shift, const int32_t* flags, float* image_out, float* mask_out,
                             void* stream);

/* Exact AUROC and average precision of one class on the device (csrc/metrics.hip): what sklearn's roc_auc_score and
 * average_precision_score return for the min-max normalised scores of reference forward_utils.py:233-308 -- the same
 * tie groups and definitions, no histogram.  n = number of scores, 2 .. 2^31 - 1 (1 .. for aaclip_metrics_normalise).
 * No floating-point atomics, every floating-point sum in an order fixed by n and the number of tie groups: two calls
 * give the same bits.  All checks precede the first launch, the workspace size last; errors carry the entry's name.
 * Every *_workspace_bytes is 0 for a refused n and monotonic in n.  scores / keys 4-byte, records and workspaces 8-byte
 * aligned; what a call writes overlaps no other buffer of it ("Buffers of a call" above).
 *   aaclip_metrics_range: record <- {min, max, number of non-finite scores (left out of min and max), number of
 *   non-zero labels (0 when labels is NULL)} in two stages (per-workgroup partials, one workgroup folds them in index
 *   order).  per_image > 0 (n a multiple of it): image_max[n / per_image] <- the maximum of every image; 0: none.
 *   aaclip_metrics_normalise: out = (x - min) / (max - min) in fp32, an IEEE subtraction and a correctly rounded
 *   division (numpy's bits; where min is a zero and the scores hold zeros of both signs, a normalised zero may carry
 *   the other sign than numpy's), when the record's max != 1.0f; otherwise out = x (reference forward_utils.py:246-253).
 *   The record is read on the device.  out == scores is allowed.  The map is monotone, so the image maxima of the raw
 *   scores go through the same call to become the maxima of the normalised images (:277).
 *   aaclip_metrics_sort: keys[n] <- the ascending order-preserving uint32 images of the scores (-0.0 counts as +0.0),
 *   by a stable LSD radix sort of four 8-bit passes.  packed = 1: for scores in [0, 1] (bit pattern below 2^30) the
 *   key is bits << 1 | (label != 0) and labels_sorted is not used; *out_of_range <- the number of scores outside
 *   [0, 1], for which the result is void.  packed = 0: any finite scores; key = bits ^ (sign ? ~0 : 1 << 31) and
 *   labels_sorted[n] <- the labels in the keys' order.  One workgroup takes aaclip_metrics_sort_group_items() keys.
 *   aaclip_metrics_curve: from the sorted keys, record <- {num, P, N, groups, ap}: P / N positives / negatives, groups
 *   = distinct scores, and over the groups from the top, with (tp, fp) the counts down to and including a group and
 *   (tp0, fp0) those above it: num = sum (fp - fp0)(tp + tp0), an exact integer with AUROC = num / (2 P N);
 *   ap = sum ((tp - tp0) / P)(tp / (tp + fp)) in fp64.  P = 0 gives a NaN ap; the caller checks the classes first. */
typedef struct aaclip_metrics_range_record {
  float min, max;
  unsigned long long nonfinite, positives;
} aaclip_metrics_range_record;
typedef struct aaclip_metrics_curve_record {
  unsigned long long num, P, N, groups;
  double ap;
} aaclip_metrics_curve_record;
size_t aaclip_metrics_range_workspace_bytes(long n, long per_image);
int aaclip_metrics_range(const float* scores, const uint8_t* labels, long n, long per_image, float* image_max,
                         void* record, void* ws, size_t ws_bytes, void* stream);
int aaclip_metrics_normalise(const float* scores, float* out, long n, const void* range_record, void* stream);
size_t aaclip_metrics_sort_workspace_bytes(long n);
long aaclip_metrics_sort_group_items(void);
int aaclip_metrics_sort(const float* scores, const uint8_t* labels, long n, int packed, uint32_t* keys,
                        uint8_t* labels_sorted, unsigned long long* out_of_range, void* ws, size_t ws_bytes,
                        void* stream);
size_t aaclip_metrics_curve_workspace_bytes(long n);
int aaclip_metrics_curve(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed, void* record, void* ws,
                         size_t ws_bytes, void* stream);

/* Per-region overlap (AUPRO) of one class on the device (csrc/regions.hip, the pair sort in csrc/metrics.hip): the PRO
 * curve over every distinct threshold, integrated up to a false-positive rate fpr_limit and divided by it -- exact, no
 * threshold grid.  The conventions are those of the entries above (checks before the first launch, the workspace size
 * last, *_workspace_bytes 0 for refused sizes and monotonic, overlap checks, no floating-point atomics, floating-point
 * sums in an order fixed by the sizes).  This ABI number is unchanged: the entries are additions.
 *   aaclip_metrics_regions: mask u8 [images * H * W], non-zero = anomalous; n = images * H * W in 2 .. 2^31 - 1.  The
 *   connected components (connectivity 8: the 3x3 structure of the MVTec evaluation, or 4) of every image on its own:
 *   nothing joins across images or across the row wrap.  region[p] <- 0 for a normal pixel, else 1 + the flat index in
 *   the whole buffer of the first pixel, in row-major order, of p's component; area[p] <- the component's pixel count, 0
 *   for a normal pixel; record <- {regions, anomalous pixels, normal pixels}.  A union-find on a 32-bit parent array
 *   whose entries are only ever lowered, by an integer atomic minimum (parent[i] <= i: every find / union loop is
 *   bounded by its start index), read inside the loops by relaxed atomic loads; areas by integer atomic adds at the
 *   root.  Minima and integer sums: the result does not depend on the order of execution.
 *   aaclip_metrics_sort_pairs: aaclip_metrics_sort's stable sort with its unpacked key (any finite scores, -0.0 as
 *   +0.0) and a 32-bit value beside it: keys[n] ascending, values_sorted[n] in their order, equal keys in input order.
 *   aaclip_metrics_pro_curve: keys / areas_sorted from the pair sort of (normalised scores, area); area 0 marks a
 *   normal pixel.  Tie groups from the highest key down; after group g, fp_g = normal pixels so far, S_g = the fp64
 *   sum of 1.0 / area over the anomalous pixels so far, x_g = fp_g / N_ok, y_g = min(1, S_g / R), (x, y) = (0, 0) in
 *   front; R is read on the device from regions_record (the record of aaclip_metrics_regions), N_ok is the number of
 *   zero areas.  Area = the trapezoids of the groups with x_g <= fpr_limit plus, for the first group beyond it whose
 *   predecessor lies below it, the trapezoid up to the linearly interpolated point at fpr_limit.
 *   record <- {aupro = area / fpr_limit, R, N_ok, groups, y at the limit}.  fpr_limit in (0, 1].  R = 0 or N_ok = 0
 *   give a NaN aupro; the caller checks the regions record first. */
typedef struct aaclip_metrics_regions_record {
  unsigned long long regions, anomalous, normal;
} aaclip_metrics_regions_record;
typedef struct aaclip_metrics_pro_record {
  double aupro;
  unsigned long long regions, normal, groups;
  double y_limit;
} aaclip_metrics_pro_record;
size_t aaclip_metrics_regions_workspace_bytes(long images, long H, long W);
int aaclip_metrics_regions(const uint8_t* mask, long images, long H, long W, int connectivity, uint32_t* region,
                           uint32_t* area, void* record, void* ws, size_t ws_bytes, void* stream);
size_t aaclip_metrics_sort_pairs_workspace_bytes(long n);
int aaclip_metrics_sort_pairs(const float* scores, const uint32_t* values, long n, uint32_t* keys,
                              uint32_t* values_sorted, void* ws, size_t ws_bytes, void* stream);
size_t aaclip_metrics_pro_curve_workspace_bytes(long n);
int aaclip_metrics_pro_curve(const uint32_t* keys, const uint32_t* areas_sorted, long n, const void* regions_record,
                             double fpr_limit, void* record, void* ws, size_t ws_bytes, void* stream);

/* Exact F1-max of one class and its operating point on the device (csrc/metrics.hip), and the masks at a threshold.  The
 * conventions are those of the entries above (checks before the first launch, the workspace size last,
 * *_workspace_bytes 0 for refused sizes and monotonic, overlap checks); integers only, no atomics: any order of
 * execution gives the same record.  This ABI number is unchanged: the entries are additions.
 *   aaclip_metrics_f1max: the arguments of aaclip_metrics_curve (sorted keys, packed or with labels_sorted) and its
 *   first phases (tile sums, scan, the list of tie-group starts).  After the group that starts at ascending index i,
 *   walking down from the highest score: tp = positives at or above its score, m = n - i elements at or above it,
 *   F1 = 2 tp / (m + P).  The winner is the group with the largest F1, compared as tp_a (m_b + P) > tp_b (m_a + P) in
 *   unsigned 64-bit integers (tp < 2^31, m + P < 2^32: exact); among groups of exactly equal F1 the one with the
 *   highest score.  record <- {tp, fp = m - tp, P, N, groups, start = i, key = the score part of keys[i] (packed: the
 *   key >> 1, which is the fp32 bit pattern), threshold = the fp32 score decoded from it}; predicted = score >=
 *   threshold.  P = 0 leaves tp = 0 and the lowest group; the caller checks the classes first.
 *   aaclip_metrics_threshold: flagged = (v >= threshold) for every raw score, with v = the score, or, when range_record
 *   (the record of aaclip_metrics_range) is given, the score normalised on the fly with aaclip_metrics_normalise's
 *   arithmetic and its max != 1.0f decision; IEEE comparison, so -0.0 counts as +0.0 and a NaN is never flagged.  The
 *   threshold is read on the device from f1max_record (an aaclip_metrics_f1max_record, of which only `threshold` is
 *   used: no host round trip after aaclip_metrics_f1max).  Outputs, each may be NULL but not all three: mask u8 [n] (1 =
 *   flagged); image_counts u32 [n / per_image][4] = tp, fp, fn, tn of every image (needs labels and per_image > 0);
 *   totals <- {tp, fp, fn, tn} over all n -- with labels NULL every label counts as 0: fp = flagged, tn = the rest.
 *   Two stages: per-workgroup integer partials, one workgroup folds them in index order.  per_image 0: one segment. */
typedef struct aaclip_metrics_f1max_record {
  unsigned long long tp, fp, P, N, groups, start;
  unsigned int key;
  float threshold;
} aaclip_metrics_f1max_record;
typedef struct aaclip_metrics_threshold_record {
  unsigned long long tp, fp, fn, tn;
} aaclip_metrics_threshold_record;
size_t aaclip_metrics_f1max_workspace_bytes(long n);
int aaclip_metrics_f1max(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed, void* record, void* ws,
                         size_t ws_bytes, void* stream);
size_t aaclip_metrics_threshold_workspace_bytes(long n, long per_image);
int aaclip_metrics_threshold(const float* scores, const uint8_t* labels, long n, long per_image,
                             const void* range_record, const void* f1max_record, uint8_t* mask,
                             uint32_t* image_counts, void* totals, void* ws, size_t ws_bytes, void* stream);

/* The table of the regions of one class on the device (csrc/region_table.hip; the code it shares with a host program is
 * csrc/region_table.h): what a user reads off an operating point -- which image every defect is in, where, how large, how
 * strong -- from the outputs of aaclip_metrics_regions on the predicted masks of aaclip_metrics_threshold.  The
 * conventions are those of the entries above (checks before the first launch, the workspace size last,
 * *_workspace_bytes 0 for refused sizes and monotonic, overlap checks); integer minima, maxima and sums only, no
 * floating-point atomics: a second call gives the same bytes.  This ABI number is unchanged: the entries are additions.
 *   aaclip_region_table: region / area u32 [images * H * W] as aaclip_metrics_regions leaves them, scores fp32 of the
 *   same size (finite), other u8 of the same size or NULL (non-zero = set).  One aaclip_region_row for every region
 *   with area >= min_area (min_area >= 1), in canonical order: ascending (image, first), the order of the region ids
 *   and of scipy.ndimage.label's numbers.
 *     image           index of the image
 *     label           1-based number of the region among ALL regions of its image, before the min_area filter
 *     first           flat index within the image of the region's first pixel in row-major order
 *     area            pixel count
 *     x0, y0, x1, y1  bounding box, x0 / y0 inclusive, x1 / y1 exclusive (scipy.ndimage.find_objects' slices)
 *     peak            fp32 bits of the largest compared score of the region; the compared score of a pixel is scores[p],
 *                     or with range_record (the record of aaclip_metrics_range) scores[p] normalised on the fly with
 *                     aaclip_metrics_normalise's arithmetic and its max != 1.0f decision; -0.0 counts as +0.0
 *     peak_x, peak_y  the pixel of the LOWEST flat index among those that attain the peak
 *     overlap         the region's pixels where other is non-zero; 0 when other is NULL
 *   image_offsets i32 [images + 1]: rows in front of image i; image_offsets[images] = the rows kept.  kept_mask u8
 *   [images * H * W] or NULL: 1 exactly on the pixels of kept regions.  record <- {rows kept, regions seen, kept regions
 *   with overlap > 0, rows dropped for lack of capacity}.  When more rows are kept than `capacity`, the first `capacity`
 *   rows in canonical order are written and nothing behind rows[capacity] is touched; kept, the offsets, kept_mask and
 *   the overlap count stay the true ones and dropped = kept - capacity.  rows may be NULL when capacity is 0.
 *   Row numbers and labels come from scans over the root flags (region[p] == p + 1).  A pixel's share travels as one
 *   64-bit word, order-preserving score key << 32 | (0xFFFFFFFF - flat index in the image), whose integer maximum is
 *   the peak with the lowest-index rule; lanes of a wave that follow one another in a region are folded first, then the
 *   workgroup's runs of one row in the LDS, then one integer atomic per field at the row.
 *   Alignment: region / area / scores / image_offsets 4 bytes; rows, the records and the workspace 8 bytes. */
typedef struct aaclip_region_row {
  uint32_t image, label, first, area, x0, y0, x1, y1, peak_x, peak_y, peak, overlap;
} aaclip_region_row;
typedef struct aaclip_region_table_record {
  unsigned long long kept, regions, hit, dropped;
} aaclip_region_table_record;
size_t aaclip_region_table_workspace_bytes(long images, long H, long W);
int aaclip_region_table(const uint32_t* region, const uint32_t* area, const float* scores, const void* range_record,
                        const uint8_t* other, long images, long H, long W, long min_area, long capacity, void* rows,
                        int32_t* image_offsets, uint8_t* kept_mask, void* record, void* ws, size_t ws_bytes,
                        void* stream);

/* Few-shot support bank (csrc/support.hip; the code it shares with a host program is csrc/support_pack.h): the
 * nearest bank row of every query row, for the memory-bank score built from k known-good images.  The conventions are
 * those of the entries above (checks before the first launch, *_workspace_bytes 0 for refused sizes, overlap checks,
 * only kernels and one memset enqueued on the caller's stream).  This ABI number is unchanged: the entries are additions.
 *   aaclip_support_nearest: best_cos[m] = max over j of <q_m, bank_j>, best_idx[m] = the LOWEST j that attains it
 *   (best_idx may be NULL).  q fp32 [M, E]; bank [N, E] as aaclip_support_bank_rows wrote it for the same form.
 *   M, N in 1 .. 2^31 - 1, E a multiple of 32 in 64 .. 1024, inputs finite.  The M x N cosines stay in MFMA
 *   accumulators; a row's candidates travel as 64-bit words, order-preserving key of the cosine << 32 |
 *   (0xFFFFFFFF - j), merged by an integer maximum (no floating-point atomics): a second call gives the same bytes,
 *   and -0.0 counts as +0.0.  Padding rows of the last tiles are never compared and never written.
 *     AACLIP_SUPPORT_FP16  both operands are multiplied by 2^4 (exact) and rounded to fp16, the products run on
 *                          v_mfma_f32_16x16x32_f16 with an fp32 accumulator that is multiplied by 2^-8 (exact).  For
 *                          rows of norm <= 1: |best_cos - exact| <= 2u + u^2 + E * 2^-24 < 1.1e-3, u = 2^-11.  Components
 *                          of magnitude >= 4094 overflow fp16: the form is meant for unit rows.
 *     AACLIP_SUPPORT_FP32  fp32 operands on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per cosine).
 *   aaclip_support_bank_rows: rows fp32 [N, E] -> bank: fp16 [N, E] of rows * 2^4 (FP16, N * E * 2 bytes) or a copy
 *   (FP32, N * E * 4 bytes).
 *   aaclip_support_map: out [B, S, S] = base + weight * sum over levels of upsample(blur(1 - best_cos[l])), with
 *   aaclip_anomaly_map's blur, align-corners upsample and level order; best_cos[l] fp32 [B * g * g]; base [B, S, S] or
 *   NULL (= 0); the distance is not clamped.  Workspace: NL * B * g * g * 4 bytes.  out and the workspace overlap neither
 *   each other nor base or a level ("Buffers of a call").
 *   Alignment: q, rows and bank 16 bytes; best_cos, best_idx 4 bytes; the workspace 8 bytes. */
#define AACLIP_SUPPORT_FP32 0
#define AACLIP_SUPPORT_FP16 1
size_t aaclip_support_nearest_workspace_bytes(long M, long N, int E, int form);
int aaclip_support_nearest(const float* q, long M, const void* bank, long N, int E, int form, float* best_cos,
                           int* best_idx, void* ws, size_t ws_bytes, void* stream);
int aaclip_support_bank_rows(const float* rows, long N, int E, int form, void* bank, void* stream);
int aaclip_support_map(const float* const* best_cos, int NL, const float* base, float weight, float* out, int B, int g,
                       int S, int ksize, float sigma, void* ws, size_t ws_bytes, void* stream);

/* Coreset of the support bank (csrc/coreset.hip; the code it shares with a host program is csrc/coreset_pack.h):
 * greedy k-center selection of n of the N bank rows, so that a bank of hundreds of images is searched at the cost of a
 * few.  Integer arithmetic throughout, so the picks are the same on every run and equal a host definition bit for bit.
 * The conventions are those of the support entries (checks before the first launch, *_workspace_bytes 0 for refused
 * sizes, overlap checks, only kernels and one memset enqueued on the caller's stream).  This ABI number is unchanged:
 * the entries are additions.
 *   aaclip_coreset_rows: rows fp32 [N, E] -> q int16 [N, E], q_i = clamp(rint(v_i * 2^14), -32767, 32767) (the product
 *   is exact, rint is round-half-even, -0.0 and NaN give 0), and norm2 int32 [N] = sum q_i^2, saturated at 2^31 - 1.
 *   aaclip_coreset_select: with d2(x, c) = norm2_x + norm2_c - 2 <q_x, q_c> (the exact squared distance of the integer
 *   rows, a uint32):
 *       min_d2[i] = UINT32_MAX for all i;  radius2[0] = UINT32_MAX;  pick[0] = start
 *       for t = 0 .. n-1:  min_d2[i] = min(min_d2[i], d2(i, pick[t]));  radius2[t+1] = max_i min_d2[i];
 *                          pick[t+1] = the LOWEST i that attains it (stored while t + 1 < n)
 *   picks int32 [n], radius2 uint32 [n + 1] (never increases; 0 from the pick after which every row duplicates a pick),
 *   min_d2 uint32 [N] after n picks.  The first k picks of a call for n are the call for k.  PRECONDITION: norm2 came
 *   from aaclip_coreset_rows and every value is below 2^29 (rows of norm up to 1.41), so that every dot product fits
 *   int32; the entry does not read the device to check it (engine.coreset_select does).  N in 1 .. 2^31 - 1, n in
 *   1 .. N, start in 0 .. N - 1, E a multiple of 32 in 32 .. 1024.  One launch per pick, chained by stream order;
 *   launch t merges one 64-bit candidate per workgroup, min_d2 << 32 | (0xFFFFFFFF - row), into word t + 1 of the
 *   workspace by an integer maximum.  No workgroup waits for another.  Workspace: (n + 1) * 8 bytes, rounded up.
 *   aaclip_coreset_unit_rows: out = rows / max(|row|, 1e-12) per row of fp32 [N, E], not in place.
 *   Alignment: rows, q and out 16 bytes; norm2, picks, radius2, min_d2 4 bytes; the workspace 8 bytes. */
int aaclip_coreset_rows(const float* rows, long N, int E, int16_t* q, int32_t* norm2, void* stream);
int aaclip_coreset_unit_rows(const float* rows, long N, int E, float* out, void* stream);
size_t aaclip_coreset_select_workspace_bytes(long N, int E, long n);
int aaclip_coreset_select(const int16_t* q, const int32_t* norm2, long N, int E, long n, long start, int32_t* picks,
                          uint32_t* radius2, uint32_t* min_d2, void* ws, size_t ws_bytes, void* stream);

/* Tiled inference (csrc/tiles.hip; the geometry it shares with a host program is csrc/tile_plan.h): a frame larger
 * than the model's input is cut into overlapping tiles of the model's size and the tile maps are blended back into one
 * map.  S = tile side, G = grid >= 1 tiles per side, O = overlap in pixels, 0 <= O <= S / 2, stride T = S - O, canvas
 * side C = S + (G - 1) * T.  Tile t = i * G + j covers canvas rows [i * T, i * T + S) and columns [j * T, j * T + S);
 * a canvas pixel lies in at most 2 tiles per axis.  canvas fp32 [images, channels, C, C]; tiles fp32
 * [images * G * G, channels, S, S].
 *   aaclip_tile_canvas: C on the host, or -1 for a refused geometry (nothing is launched).
 *   aaclip_tile_gather: tiles[b * G * G + t, c, y, x] = canvas[b, c, i * T + y, j * T + x], a copy of bits.
 *   aaclip_tile_stitch: with w1(u) = min(u + 1, S - u) and the weight w1(y) * w1(x) of a tile at its (y, x): a canvas
 *   pixel under exactly one tile takes that tile's value, the same bits; any other pixel is
 *   (sum_t w_t * v_t) / (sum_t w_t) over its covering tiles in ascending t, in fp32, every product, sum and the division
 *   rounded on its own.  Across an overlap the two 1-D weights add up to O + 1: a linear cross-fade.  The weights and
 *   their sums are exact in fp32 for S <= 4096.  The stitch is a gather over output pixels: no atomics, no workspace,
 *   no memset, and a second call gives the same bytes.
 * Each call is one launch on plan->stream (the stream travels in the plan, a hipStream_t).  Every check happens before
 * the launch, and a failed one returns -1, leaves an error text that starts with the entry's name and writes nothing:
 * a null plan, a struct_bytes other than sizeof, images < 0, channels < 1, tile < 1, grid < 1, overlap outside
 * 0 .. tile / 2, a canvas side above INT_MAX, images * grid^2 * channels above 2^31 - 1, tensors of more than 2^59
 * elements, a null or not 4-byte aligned pointer, canvas and tiles overlapping.  images == 0 returns 0 without a
 * launch.  Vector accesses (16 or 8 bytes) are used where S and T are multiples of 4 or 2 and both pointers are aligned
 * to that size; any other S, T and 4-byte aligned pointers take scalar accesses.  This ABI number is unchanged: the
 * entries are additions. */
typedef struct aaclip_tile_plan {
  size_t struct_bytes;   /* sizeof(aaclip_tile_plan); any other value is refused */
  int images;
  int channels;
  int tile;
  int grid;
  int overlap;
  void* stream;          /* hipStream_t */
} aaclip_tile_plan;
int aaclip_tile_canvas(int tile, int grid, int overlap);
int aaclip_tile_gather(const aaclip_tile_plan* plan, const float* canvas, float* tiles);
int aaclip_tile_stitch(const aaclip_tile_plan* plan, const float* tiles, float* canvas);

/* Heat-map overlays (csrc/overlay.hip; the plan checks, offsets and pixel functions it shares with a host program are
 * csrc/overlay_plan.h): the frame the model saw, the heat map over it and the ground truth over it as uint8 RGB panels.
 * frames fp32 [images, 3, H, W] (the normalised model input), maps fp32 [images, H, W] (raw scores), range_record the
 * record of aaclip_metrics_range or NULL, pred / truth uint8 [images, H, W] or NULL (non-zero = set), lut uint8
 * [256, 3], out uint8 [images, n * H, W, 3]: the n panels that `panels` selects (bit 0 frame, bit 1 heat, bit 2 truth),
 * in that order, stacked vertically.  Per pixel:
 *   frame byte  F[c] = clamp(rint(((x[c] * std[c]) + mean[c]) * 255), 0, 255): every operation rounded to fp32 on its
 *               own, rint to even, NaN -> 0.
 *   heat byte   n = (x - min) / (max - min) in fp32 (aaclip_metrics_normalise's bits) when the record's max != 1, else
 *               x; x itself without a record.  q = 0 for a NaN n, else the truncation of min(max(n, 0), 1) * 255 with
 *               the fp32 product rounded toward zero.
 *   contour(M)  true at (y, x) when M[y, x] != 0 and some pixel INSIDE the image with |dy| <= T and |dx| <= T has
 *               M == 0, T = thickness; T = 0 draws none.
 *   blend(u, v) = (alpha256 * u + (256 - alpha256) * v + 128) >> 8 per channel, in integers.
 *   frame panel F.  heat panel blend(F, lut[q]), pred_colour on contour(pred).  truth panel blend(F, truth_colour) where
 *   truth != 0, else F; then truth_colour on contour(truth); then pred_colour on contour(pred).  A NULL mask draws
 *   nothing.
 * One launch on plan->stream: a gather over output pixels with no workspace, no memset and no atomics, so a second call
 * gives the same bytes; every offset is 64-bit; out may have any byte alignment (it is written in aligned 16-byte
 * chunks, the ends of a run in narrower stores).  Every check happens before the launch, and a failed one returns -1,
 * leaves an error text that starts with the entry's name and writes nothing: a null plan, a struct_bytes other than
 * sizeof, images < 0, height or width < 1, no panel or an unknown panel bit, the truth panel with a NULL truth,
 * alpha256 outside 0 .. 256, thickness outside 0 .. 8, a std that is not positive and finite, a NULL frames, maps, lut
 * or out, frames or maps not 4-byte aligned, a record not 8-byte aligned, more than 2^56 pixels, out overlapping an
 * input.  images == 0 checks all of that and launches nothing.  This ABI number is unchanged: the entry is an
 * addition. */
#define AACLIP_OVERLAY_FRAME 1u
#define AACLIP_OVERLAY_HEAT 2u
#define AACLIP_OVERLAY_TRUTH 4u
typedef struct aaclip_overlay_plan {
  size_t struct_bytes;      /* sizeof(aaclip_overlay_plan); any other value is refused */
  int images;
  int height;
  int width;
  unsigned panels;          /* AACLIP_OVERLAY_FRAME | AACLIP_OVERLAY_HEAT | AACLIP_OVERLAY_TRUTH */
  int alpha256;             /* weight of the frame in a blend, 0 .. 256 */
  int thickness;            /* T, 0 .. 8 */
  uint8_t pred_colour[3];   /* RGB */
  uint8_t truth_colour[3];
  float mean[3];            /* the normalisation of frames, undone for the frame byte */
  float std[3];
  void* stream;             /* hipStream_t */
} aaclip_overlay_plan;
int aaclip_overlay_render(const aaclip_overlay_plan* plan, const float* frames, const float* maps, const void* range_record,
                          const uint8_t* pred, const uint8_t* truth, const uint8_t* lut, uint8_t* out);

/* PNG encoding on the device (csrc/png.hip; the format, the code builder and the checks it shares with a host program
 * are csrc/png_plan.h).  pixels uint8 [images, height, width, channels], channels 1 (grey) or 3 (RGB), contiguous, at
 * any byte alignment -- aaclip_overlay_render's output is such a tensor.  The result is one zlib stream per image, the
 * content of a PNG's IDAT chunk: image i's stream is payload[offsets[i] .. offsets[i + 1]), offsets int64
 * [images + 1], offsets[0] = 0.  The caller wraps it in the signature, IHDR (8 bit, colour type 2 or 0, no interlace),
 * IDAT and IEND with their CRC-32.  With R = width * channels:
 *   filters   the filtered stream of an image is `height` rows of 1 + R bytes: the filter type and the row's bytes under
 *             it, PNG's five types with bpp = channels, the row above row 0 all zeros.  A row takes the type with the
 *             smallest sum of min(b, 256 - b) over its R filtered bytes, ties to the lowest type.
 *   segments  max(1, 32768 / (1 + R)) whole rows of that stream (the last segment may be shorter), compressed on their
 *             own into one deflate block each that ends on a byte.
 *   tokens    distance-1 matches only.  A maximal run of n equal bytes inside a segment is a literal; the other n - 1
 *             bytes follow in pieces of 258, and a last piece of 3 or more is a match, one of 1 or 2 literals.
 *   code      leaves in (count, symbol) order, merged from two queues, a leaf before an internal node of the same
 *             weight.  The tree gives the number of codes of every length, a leaf deeper than the limit (15; 7 for the
 *             code-length alphabet) counted at the limit; while their Kraft sum exceeds 1, one code of the limit's
 *             length goes and the longest shorter code becomes two codes one bit longer; the lengths are handed out
 *             in leaf order, the longest to the rarest.  The distance alphabet is one code (HDIST = 0) of length 1 where
 *             the segment has a match, else 0.  The lengths are sent as one sequence (literal / length, then distance):
 *             a non-zero length as itself, of a zero run of z one symbol 18 of min(z, 138) while z >= 11, then one
 *             symbol 17 if 3 or more are left, else symbols 0.  Symbol 16 is never used.
 *   block     BFINAL = 0, BTYPE = 2, the header, the tokens, end-of-block, three zero bits (an empty stored block),
 *             padding to the byte and 00 00 FF FF; or, where that is not shorter, the stored block 00 LEN NLEN and the
 *             bytes.  A segment never takes more than its length + 5 bytes.
 *   stream    78 01, the segments, 03 00 (an empty final fixed block), the Adler-32 of the filtered stream, big-endian,
 *             combined from per-segment integer sums in segment order.
 * Two launches on plan->stream, no global atomics, integers only: a second call gives the same bytes, and nothing past
 * offsets[images] is written.  aaclip_png_capacity_bytes = images * (8 + height * (1 + R) + 5 * segments) is the
 * largest payload; aaclip_png_workspace_bytes the workspace (a slot and a record per segment).  Both return 0 for a
 * plan that is refused.  Every check happens before the first launch, and a failed one returns -1, leaves an error
 * text that starts with the entry's name and writes nothing: a null plan, a struct_bytes other than sizeof, a negative
 * size, height or width 0 with images > 0, channels other than 1 or 3, 1 + R above 32768, sizes whose products
 * overflow ("too large"), a null pointer, a workspace or a capacity that is too small, a workspace not 16-byte or
 * offsets not 8-byte aligned, the workspace, payload or offsets overlapping one another or pixels ("Buffers of a call").
 * images == 0 checks the plan, launches nothing
 * and returns 0.  This ABI number is unchanged: the entries are additions. */
typedef struct aaclip_png_plan {
  size_t struct_bytes;      /* sizeof(aaclip_png_plan); any other value is refused */
  int images;
  int height;
  int width;
  int channels;             /* 1 or 3 */
  void* stream;             /* hipStream_t */
} aaclip_png_plan;
size_t aaclip_png_workspace_bytes(const aaclip_png_plan* plan);
size_t aaclip_png_capacity_bytes(const aaclip_png_plan* plan);
int aaclip_png_encode(const aaclip_png_plan* plan, const uint8_t* pixels, void* workspace, size_t ws_bytes,
                      uint8_t* payload, size_t capacity, int64_t* offsets);

/* Bootstrap of AUROC / AP over the IMAGES of one class (csrc/bootstrap.hip; the definition is
 * forward_utils.bootstrap_eval, DESIGN.md section 6 "Bootstrap intervals on the device").  This ABI number is unchanged:
 * the entries are additions.  The conventions are those of the metrics entries (checks before the first launch, the
 * workspace size last, *_workspace_bytes 0 for refused sizes, no atomics, the fp64 sum in an order fixed by n alone:
 * two calls give the same bytes).
 *   keys [n] ascending and payload [n] = image << 1 | label in their order: what aaclip_metrics_sort_pairs gives for the
 *   values image << 1 | label.  n in 1 .. 2^31 - 1, images in 1 .. aaclip_bootstrap_max_images(); a payload whose
 *   image is not below `images` is read as the last image.  counts u8 [R][images]: replicate r gives every element of
 *   image i the weight counts[r][i].  R in 1 .. 2^20.  The CALLER guarantees sum_i counts[r][i] * (elements of image i)
 *   < 2^31 for every r (the counts live on the device; aaclip_hip.engine checks it on the host).
 *   records [R] <- {num, P, N, ap}: P / N the weighted positives / negatives, num the integer AUROC numerator
 *   (AUROC = num / (2 P N)), ap the fp64 average-precision sum over the tie groups, a group without a weighted positive
 *   adding exactly 0.  P == 0 or N == 0 marks an INVALID replicate: num = 0, ap = 0.
 *   The workspace does not grow with R beyond 512: the entry walks the replicates in chunks of 8 blocks of 64.
 *   The sizes and the stream travel in a plan, as in aaclip_png_plan; every launch goes to plan->stream and the call
 *   only enqueues work on it (it may be captured into a graph). */
typedef struct aaclip_bootstrap_record {   /* 32 bytes */
  unsigned long long num, P, N;
  double ap;
} aaclip_bootstrap_record;
typedef struct aaclip_bootstrap_plan {
  size_t struct_bytes;      /* sizeof(aaclip_bootstrap_plan); any other value is refused */
  long n;                   /* sorted elements */
  long images;
  long replicates;          /* R */
  void* stream;             /* hipStream_t */
} aaclip_bootstrap_plan;
long aaclip_bootstrap_max_images(void);
size_t aaclip_bootstrap_workspace_bytes(long n, long images, long R);
int aaclip_bootstrap_curves(const aaclip_bootstrap_plan* plan, const uint32_t* keys, const uint32_t* payload,
                            const uint8_t* counts, void* records, void* ws, size_t ws_bytes);

/* Fused Adam / AdamW step over a list of tensors, and the gradient norm that clips it (csrc/optim.hip).  fp32
 * parameters, gradients and state only.  One launch serves up to 24 tensors and 640 chunks of 16384 elements; its table
 * travels by value in the kernel arguments, so a call copies nothing to the device, allocates nothing and waits for
 * nothing.  Every argument check happens before the first launch and a bad argument returns -1: a null struct, a
 * struct_bytes other than sizeof, count < 0, items null with count > 0, n < 0 or n > 2^27 * 16384, a null or not
 * 4-byte aligned pointer of a tensor with n > 0, a group index outside [0, n_groups), n_groups outside
 * 1 .. AACLIP_OPTIM_MAX_GROUPS, step < 1, a negative or non-finite lr / eps / weight_decay, a beta outside [0, 1), decoupled
 * other than 0 / 1, max_norm not above 0, record / workspace null or not 8-byte aligned, a workspace too small.
 * Tensors with n == 0 are skipped.  This ABI number is unchanged: the entries are additions.
 *   aaclip_optim_grad_norm: only g and n of every tensor are read.  Stage 1, one workgroup per chunk: the sum of g^2
 *   over the chunk in fp64, stored in the workspace slot of that chunk (no atomics).  Stage 2, one workgroup: the slots
 *   added in fp64 in a fixed order; record <- {total_norm = fp32(sqrt(sum)), clip_coef = min(1, max_norm / (total_norm
 *   + 1e-6))} in fp32, torch.nn.utils.clip_grad_norm_'s formula.  The same inputs give the same bits.  A NaN or inf
 *   gradient gives a NaN or inf norm and a NaN or 0 coefficient; nothing is skipped.
 *   aaclip_optim_adam_step: per element, in fp32 with every operation rounded on its own,
 *     g' = g * coef (+ weight_decay * p when decoupled == 0);  p' = p * (1 - lr * weight_decay) when decoupled == 1
 *     m = beta1 * m + (1 - beta1) * g';  v = beta2 * v + (1 - beta2) * g' * g'
 *     p = p' - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),  bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
 *   coef = record->clip_coef read on the device (no host round trip after aaclip_optim_grad_norm), or 1 when record is
 *   NULL.  1 - beta, 1 - lr * weight_decay, lr / bc1 and sqrt(bc2) are formed on the host in fp64 and rounded once to
 *   fp32.  UNLIKE clip_grad_norm_, the gradients in memory are not rescaled: g is read only.  16-byte loads and stores
 *   where p, g, m and v of a tensor are all 16-byte aligned, 4-byte ones otherwise, with the same arithmetic: a
 *   tensor's result does not depend on its alignment, on its place in the list or on the other tensors. */
#define AACLIP_OPTIM_MAX_GROUPS 8
typedef struct aaclip_optim_tensor {
  void* p;          /* parameter, fp32 [n], updated in place */
  const void* g;    /* gradient, fp32 [n], read only */
  void* m;          /* exp_avg, fp32 [n], updated in place */
  void* v;          /* exp_avg_sq, fp32 [n], updated in place */
  long n;
  int group;        /* index into the groups of aaclip_optim_adam_step; ignored by aaclip_optim_grad_norm */
} aaclip_optim_tensor;
typedef struct aaclip_optim_tensors {
  size_t struct_bytes;               /* sizeof(aaclip_optim_tensors) */
  const aaclip_optim_tensor* items;  /* HOST array */
  long count;
} aaclip_optim_tensors;
typedef struct aaclip_optim_group {
  double lr, beta1, beta2, eps, weight_decay;
  int decoupled;    /* 1: AdamW, 0: Adam (the decay joins the gradient) */
  long step;        /* the step being taken, 1 for the first */
} aaclip_optim_group;
typedef struct aaclip_optim_record {
  float total_norm, clip_coef;
} aaclip_optim_record;
size_t aaclip_optim_grad_norm_workspace_bytes(const aaclip_optim_tensors* tensors);   /* 0 for a refused list */
int aaclip_optim_grad_norm(const aaclip_optim_tensors* tensors, float max_norm, void* record, void* workspace,
                           size_t workspace_bytes, void* stream);
int aaclip_optim_adam_step(const aaclip_optim_tensors* tensors, const aaclip_optim_group* groups, int n_groups,
                           const void* record_or_null, void* stream);

/* Text embedding: x[i*T+t] = token_embedding[tokens[i,t]] + positional_embedding[t].
 * Replaces reference model/adapter.py:277-281 (model/model.py:192-194).  Token ids outside [0, vocab) are CLAMPED
 * to 0 / vocab - 1 (the reference's nn.Embedding raises instead); D a multiple of 4. */
int aaclip_text_embed(const int32_t* tokens, const float* table, const float* pos, float* x, int n, int T, int D,
                      int vocab, void* stream);

/* Row head: LayerNorm, pick one row per sequence, project.
 *   mode 0: row at argmax(tokens[i,:]) (EOT) -- ln_final + text_adapter[-1] / text_projection,
 *           reference model/adapter.py:297-299 and model/model.py:198-200
 *   mode 1: row 0 (CLS) -- ln_post + visual.proj, reference model/transformer.py:542-546
 * x [n*T, D] fp32; proj_w [E, D] dtype (pass text_projection / visual.proj transposed);
 * out [n, E] fp32. */
int aaclip_row_head(const float* x, const int32_t* tokens, const float* ln_w, const float* ln_b, const void* proj_w,
                    int act, float* out, int n, int T, int D, int E, int mode, int dtype, void* ws, size_t ws_bytes,
                    void* stream);

/* In-stream timing of the kernels inside aaclip_block for the benchmark's roofline leg:
 * begin(tag_mask, capacity) arms hipEvent pairs around kernels whose tag bit is set
 * (0 layernorm, 1 qkv gemm, 2 attention, 3 out_proj gemm, 4 c_fc gemm, 5 c_proj gemm,
 * 6 adapter); end() synchronises the recorded events and returns how many (ms[i], tags[i])
 * pairs it wrote.  Not part of the reference's surface; measurement only. */
int aaclip_profile_begin(unsigned tag_mask, int capacity);
int aaclip_profile_end(float* ms, int* tags, int max_n);

/* Kernel selection for A/B measurements (tools/bench_gemm.py, tools/bench_attn.py); 0 = automatic (default).
 * bits 0..7   GEMM: 1 = always the 128x128-tile kernel; 80 / 81 / 82 = where the automatic choice is a 256-row-tile
 *             kernel, always the 8-wave 256x256 one with one tile per workgroup / the 4-wave 256x128 half-tile one /
 *             the 8-wave one walking its tiles (split operands; one workgroup per CU) -- bit-identical results; 0
 *             picks the fastest.
 * bits 8..15  attention: 1 = always the 128-query kernel
 * bit 17      turn the LayerNorm folding of aaclip_block(s) off
 * Every selectable kernel computes the same function.  Any other value is rejected (rc < 0) and leaves the selection
 * unchanged. */
int aaclip_set_gemm_variant(int v);

/* Split fp16 blocks (aaclip_block(s), FULL / CAUSAL attention): where the 256x256 tiles of a residual product (out_proj,
 * c_proj) leave the last round of the walking kernel partly empty (at least two full rounds, a tail of at most half the
 * CUs), the product runs as two launches on the caller's stream -- the rows of the full rounds, then ONE launch whose
 * workgroups run the tail tiles or the LayerNorm that follows the product on the rows already complete -- and only the
 * LayerNorm of the last rows remains a pass.  Results are bit-identical either way.  on = 0 keeps the single launch and
 * the whole pass.  Default: on. */
int aaclip_set_tail_overlap(int on);
/* For tests: the CU count the row split above is planned with, so that a tail exists at small shapes.
 * cus = 0 (default): the device's count; otherwise a multiple of 8, 8 .. 1024 (anything else: rc < 0, no change). */
int aaclip_set_plan_cus(int cus);
/* How many tail launches (the second launch above) this process has issued so far: tests tell an engaged split from a
 * single launch by it. */
long aaclip_tail_overlap_count(void);

/* Building blocks, exported for unit parity tests and for callers that fuse differently.
 * Row limits.  A launch covers its grid only below 2^24 workgroups of 256 threads, so the entries whose kernels take
 * one workgroup per row (group) refuse more (rc < 0, nothing launched): rows <= 2^26 - 4 for aaclip_layernorm,
 * aaclip_layernorm_split, aaclip_adapter_mix, aaclip_adapter_mix_fold, aaclip_residual_layernorm,
 * aaclip_layernorm_backward, aaclip_adapter_mix_backward and aaclip_layernorm_param_grad (4 rows per workgroup);
 * rows * H < 2^24 for aaclip_head_expand and rows < 2^24 for aaclip_head_diag (one workgroup per row);
 * rows * K <= 2^35 - 2048 for aaclip_split3_rows; n / per_image < 2^24 images for aaclip_metrics_range and
 * aaclip_metrics_threshold (their *_workspace_bytes, and aaclip_layernorm_param_grad's, are 0 beyond).  The block
 * entries run the same row kernels: aaclip_block(s), aaclip_blocks_to / _taps, aaclip_block_backward(_long, _bf16x3) and
 * aaclip_tap_head_backward take B * L <= 2^26 - 4 rows.  aaclip_ln_stats_finalize takes rows < 2^27.  The
 * other row and element entries (aaclip_split_rows, aaclip_combine3, aaclip_linear_smallk, aaclip_act_backward,
 * aaclip_bias_grad, aaclip_drop_cls_rows) walk any count with a bounded grid. */
int aaclip_layernorm(const float* x, const float* w, const float* b, void* out, int out_dtype, long rows, int D,
                     float eps, void* stream);
int aaclip_gemm(int dtype, int epi, const void* A, long lda, const void* W, const float* bias, void* out, long ldc,
                int M, int N, int K, int act, int scale_cols, float scale, void* stream);
int aaclip_attention(int dtype, const void* qkv, void* ctx, int B, int L, int H, int causal, void* stream);
/* The same with q already in log2 units: q = (x Wq^T + b) * head_dim^-1/2 * log2(e), rounded to `dtype` once -- what
 * the QKV epilogue of aaclip_block produces (16-bit dtypes only).  This is the kernel variant the block path runs
 * (one v_exp_f32 per score, no per-score multiply); exported so that it can be tested and timed on its own. */
int aaclip_attention_log2q(int dtype, const void* qkv, void* ctx, int B, int L, int H, int causal, void* stream);
int aaclip_adapter_mix(float* x, const float* a, long rows, int D, float weight, void* stream);

/* The block path's forms of the building blocks (ABI version >= 10): what aaclip_block(s) selects on fields and flags
 * that the entries above cannot set, exported so that each form is tested per element on its own.  Every check
 * precedes the first launch; a field that the kernel this call would run does not implement is REFUSED (rc < 0,
 * aaclip_last_error, nothing launched), never ignored.  Errors carry the entry's name as prefix.
 *
 * aaclip_gemm_fused = aaclip_gemm plus the fields of the struct below; with all of them zero it is aaclip_gemm:
 *   resid      AACLIP_EPI_BIAS_RESID: the residual is READ here ([M, ldc] fp32, left untouched) instead of from `out`.
 *   out16, stats_out (together)  AACLIP_EPI_BIAS_RESID, fp16 / bf16, a 256-row-tile kernel (M >= 4096, N a multiple of
 *              256, ldc a multiple of 8, GEMM variant other than 1): out16 [M, N] <- the new rows rounded to dtype;
 *              stats_out [M][N / 64][2] <- (sum, sum of squares) of those ROUNDED values per 64-column slice.
 *   row_ab, col_s (together)     AACLIP_EPI_BIAS / AACLIP_EPI_BIAS_GELU, same kernels: row_ab [M][2] = (a, b) per row,
 *              col_s [N]; the epilogue's input becomes fmaf(a_m, acc, b_m * s_n) (+ bias_n): LayerNorm folded into the
 *              product, with (a, b) = (rstd, -mean * rstd) and s = the row sums of the gamma-scaled weight.
 *   w_exact16  AACLIP_F16X2, K a multiple of 256: W is [N, 3K] bytes (no lo plane; the weight is exact in fp16).
 *   out_qk8    AACLIP_EPI_BIAS, AACLIP_F16X2, the 256-row-tile kernel: a multiple of 64, <= N.  The output row is
 *              [N fp16: hi][per 64 columns below out_qk8: lo8 64 B | hi8 64 B] = N + out_qk8 halves (ldc >= that): the
 *              [q k v hi | q8 | k8] records of aaclip_attention_split(qk8) for N = 3 * 64 H, out_qk8 = 2 * 64 H.
 *              Columns >= out_qk8 are rounded to fp16 (no correction).
 *   out_no_hi8 AACLIP_EPI_BIAS_GELU, AACLIP_F16X2: the hi8 plane of the split8 output rows is not written (for a
 *              consumer whose weight is exact in fp16, which never reads it).
 * aaclip_ln_stats_finalize: partials [rows][D / 64][2] (stats_out) -> row_ab [rows][2] = (rstd, -mean * rstd) with the
 *   one-pass biased variance max(q / D - mean^2, 0) in fp32.  Its relative error grows with mean(x^2) / (var + eps)
 *   (DESIGN.md 3c).  D a supported row width, rows < 2^27.
 * aaclip_adapter_mix_fold: aaclip_adapter_mix (x bit-identical) that also writes out16 [rows, D] = the new rows in dtype
 *   (fp16 / bf16) and row_ab [rows][2] of those rounded values, eps 1e-5.
 * aaclip_attention_split: aaclip_attention / _log2q (log2q != 0) for AACLIP_F16X2 with the launcher's flags: hi8 = 0
 *   leaves the hi8 plane of the context rows unwritten; qk8 != 0 reads [q k v hi | q8 | k8] records of 10 * 64 H bytes
 *   (refused unless log2q, L >= 512 and not causal).
 * aaclip_layernorm_split / aaclip_split_rows: aaclip_layernorm(AACLIP_F16X2) / fp32 [rows, D] -> split8 rows [rows, 4D]
 *   bytes, with hi8 = 0 leaving the hi8 plane unwritten. */
typedef struct aaclip_gemm_fused_args {
  size_t struct_bytes;    /* sizeof(aaclip_gemm_fused_args) as the caller compiled it; any other value is refused */
  const float* resid;
  void* out16;
  float* stats_out;
  const float* row_ab;
  const float* col_s;
  int w_exact16;
  int out_qk8;
  int out_no_hi8;
} aaclip_gemm_fused_args;
int aaclip_gemm_fused(int dtype, int epi, const void* A, long lda, const void* W, const float* bias, void* out, long ldc,
                      int M, int N, int K, int act, int scale_cols, float scale, const aaclip_gemm_fused_args* f,
                      void* stream);
int aaclip_ln_stats_finalize(const float* partials, float* row_ab, long rows, int D, float eps, void* stream);
int aaclip_adapter_mix_fold(int dtype, float* x, const float* a, long rows, int D, float weight, void* out16,
                            float* row_ab, void* stream);
int aaclip_attention_split(const void* qkv, void* ctx, int B, int L, int H, int causal, int log2q, int qk8, int hi8,
                           void* stream);
int aaclip_layernorm_split(const float* x, const float* w, const float* b, void* out, long rows, int D, float eps,
                           int hi8, void* stream);
int aaclip_split_rows(const float* src, void* dst, long rows, int D, int hi8, void* stream);

/* ---- IQM side branch (reference model/iqm.py, the glue of model/adapter.py:186-269 and the IQM maps of
 * test_last.py:102-147).  Its matrix products -- class_query_mlp, query_adapters,
 * visual_feature_proj, every query / key / value / dense / intermediate Linear of IQMLayer -- go through aaclip_gemm
 * (AACLIP_EPI_BIAS for 16-bit key / value / patch operands, AACLIP_EPI_BIAS_GELU for intermediate_query,
 * AACLIP_EPI_ACT_F32 with a bias for the 2-row query side).  The entry points below are what is left. */

/* Cross-attention of IQM without the key / value projections of the patch rows (reference model/iqm.py:108-139 with
 * encoder_hidden_states = the 4 x 1369 projected patch rows; the reference projects every row through W_k and W_v):
 *   scores_j = q_h . (W_k[h] x_j + b_k[h]) / sqrt(d) = (W_k[h]^T q_h / sqrt(d)) . x_j + const  (softmax-invariant)
 *   ctx_h    = sum_j p_j (W_v[h] x_j + b_v[h])       = W_v[h] (sum_j p_j x_j) + b_v[h]
 * aaclip_head_expand builds the A operand of the effective-query product (q [rows, D] fp32 -> [rows * H, D] dtype, row
 * (r, h) = q[r] * scale on head h's columns, zero elsewhere; qt = that . W_k through aaclip_gemm);
 * aaclip_cross_rows computes out[b, r] = softmax_j(qt[b, r] . x[b, j]) . x[b] for R = queries x heads effective
 * queries per image over the raw rows x [B * Lk, Dk] (x_dtype), fp32 accumulation, qt / out [B, R, Dk] fp32;
 * aaclip_head_diag picks the head-diagonal blocks of the [rows * H, D] product W_v . ebar + b_v -> ctx [rows, D]. */
size_t aaclip_cross_rows_workspace_bytes(int B, int R, int Lk, int Dk);
int aaclip_cross_rows(int x_dtype, const float* qt, const void* x, float* out, int B, int R, int Lk, int Dk, void* ws,
                      size_t ws_bytes, void* stream);
/* Backward of aaclip_cross_rows from d_out [B, R, Dk]: with p_rj the forward's probabilities (recomputed: nothing of
 * size Lk x Dk is kept from the forward or placed in the workspace), g_rj = d_out[b, r] . x[b, j] and
 * delta_r = sum_j p_rj g_rj,
 *   ds_rj = p_rj (g_rj - delta_r),  d_qt[b, r] = sum_j ds_rj x[b, j],  d_x[b, j] = sum_r (p_rj d_out[b, r] + ds_rj qt[b, r]).
 * qt, d_out, d_qt [B, R, Dk] and d_x [B, Lk, Dk] are fp32 whatever x_dtype (fp32, fp16, bf16) is; d_qt or d_x may be
 * NULL, not both.  accumulate != 0: d_x += the gradient (both IQM layers, and the key and the value role inside a
 * layer, read the same rows: their gradients are summed in place); 0: d_x is overwritten.  d_qt is always overwritten.
 * act (AACLIP_ACT_*): the contribution to d_x is multiplied by the activation's derivative taken from the sign of the
 * row's own value -- x is then the activation's OUTPUT, both activations keep the sign, slope 1 for x > 0 and 0.01
 * (LEAKY) / 0 (RELU) for x <= 0, the kink convention stated at aaclip_adapter_mix_backward -- so that d_x is the
 * gradient of the pre-activation product without a pass of its own over the rows.
 * R, Lk, Dk as aaclip_cross_rows (R 4, 8, 12 or 16; Dk 256, 512, 768 or 1024; Lk >= 1), B <= 65535.  Every pointer and
 * the workspace 16-byte aligned.  ws_bytes >= aaclip_cross_rows_backward_workspace_bytes(B, R, Lk, Dk) = scores and
 * d_out products [B, Lk, 32], row statistics and per-slice partial sums of d_qt (at most 128 slices per image); 0 for
 * an empty problem, monotonic in each argument.  No atomics, every sum in a fixed order: two calls on the same inputs
 * give the same bits, and each element of d_x is written by one thread.  All checks precede the first launch; errors
 * carry the "cross_rows_backward:" prefix. */
size_t aaclip_cross_rows_backward_workspace_bytes(int B, int R, int Lk, int Dk);
int aaclip_cross_rows_backward(int x_dtype, const float* qt, const void* x, const float* d_out, float* d_qt, float* d_x,
                               int act, int accumulate, int B, int R, int Lk, int Dk, void* ws, size_t ws_bytes,
                               void* stream);
/* The same over up to 4 SEGMENTS of 16-bit rows that share one softmax, on the matrix cores: segment s has its own row
 * buffer x[s] (image b's keys are rows b * rows_per_image + row0 + j, j < Lk, of ldx elements each, the first Dk of
 * which are read) and its own effective queries: qt, out [B, R, nseg, Dk] fp32,
 *   p = softmax over all (s, j) of qt[b, r, s] . x[s][b, j];   out[b, r, s] = sum_j p_(s, j) x[s][b, j].
 * This is the visual cross-attention of IQM on the LayerNorm'ed tap rows themselves (aaclip_tap_head_keep_rows; row0 = 1
 * skips the CLS row): with query_adapters[s] (reference model/adapter.py:205-208, a Linear without bias when relu is
 * off), torch.cat over the levels (:210-211), visual_feature_proj (:213-221) and the key / value Linear all linear in
 * the rows, each moves to the query side (qt[., s] = W_qa[s]^T P^T W_k[h]^T q_h / sqrt(d)) and behind the weighted
 * sums (sum_s W_qa[s] out[., s], then P, W_v) as [R, .] products through aaclip_gemm -- no per-row projection is left.
 * x_dtype AACLIP_F16 or AACLIP_BF16 (for the fp16 halves of split8 rows pass AACLIP_F16 and ldx = 2 Dk), R <= 16,
 * Dk 768 or 1024, ldx a multiple of 8. */
size_t aaclip_cross_rows_levels_workspace_bytes(int B, int nseg, int Lk, int Dk);
int aaclip_cross_rows_levels(int x_dtype, const float* qt, const void* const* x, int nseg, float* out, int B, int R,
                             int rows_per_image, int row0, int Lk, int Dk, long ldx, void* ws, size_t ws_bytes,
                             void* stream);
/* Backward of aaclip_cross_rows_levels from d_out [B, R, nseg, Dk]: with p the forward's one softmax over all (s, j)
 * (recomputed: nothing of size Lk x Dk is kept from the forward or placed in the workspace),
 * g_(r,s,j) = d_out[b, r, s] . x[s][b, j] and delta_r = sum_(s,j) p g,
 *   ds = p (g - delta_r),  d_qt[b, r, s] = sum_j ds_(r,s,j) x[s][b, j],
 *   d_x[s][b, j] = sum_r (p_(r,s,j) d_out[b, r, s] + ds_(r,s,j) qt[b, r, s]).
 * fp32 arithmetic on the 16-bit row values as they are.  qt, d_out, d_qt fp32 [B, R, nseg, Dk]; x as the forward takes
 * it; d_x[s] fp32 [B * rows_per_image, Dk] (dense rows of Dk floats), addressed by the same row index
 * b * rows_per_image + row0 + j as x[s]: rows outside the key range (the CLS row) are never written.  d_qt may be NULL,
 * or d_x (the whole array) may be NULL, not both.  accumulate != 0: d_x[s] += the gradient (the two IQM layers read
 * the same rows); 0: the key rows of d_x[s] are overwritten.  d_qt is always overwritten.
 * x_dtype AACLIP_F16 or AACLIP_BF16; R 4, 8, 12 or 16; nseg 1..4; Dk 768 or 1024; Lk >= 1; ldx >= Dk and a multiple of 8
 * (2 Dk for the fp16 halves of split8 rows); rows_per_image >= row0 + Lk, row0 >= 0, an image's rows of x[s] span less
 * than 2 GiB (as for the forward); B <= 65535; every pointer and the
 * workspace 16-byte aligned.  ws_bytes >= aaclip_cross_rows_levels_backward_workspace_bytes(B, R, nseg, Lk, Dk) =
 * scores and d_out products [B, nseg, Lk, 32], row statistics and per-slice partial sums of d_qt (at most 128 slices
 * per segment); 0 for an empty problem, monotonic in each argument.  No atomics, every sum in a fixed order: two calls
 * on the same inputs give the same bits, and each element of d_x is written by one thread.  All checks precede the
 * first launch; errors carry the "cross_rows_levels_backward:" prefix. */
size_t aaclip_cross_rows_levels_backward_workspace_bytes(int B, int R, int nseg, int Lk, int Dk);
int aaclip_cross_rows_levels_backward(int x_dtype, const float* qt, const void* const* x, int nseg, const float* d_out,
                                      float* d_qt, float* const* d_x, int accumulate, int B, int R, int rows_per_image,
                                      int row0, int Lk, int Dk, long ldx, void* ws, size_t ws_bytes, void* stream);
int aaclip_head_expand(int dtype, const float* q, void* qm, long rows, int H, int D, float scale, void* stream);
int aaclip_head_diag(const float* full, float* ctx, long rows, int H, int D, void* stream);
/* softmax(q k^T * scale) v per (image, head) for nq <= 4 queries over Lk <= 8192 keys: the core of
 * IQM_MultiHeadAttention.forward (reference model/iqm.py:108-139; masks are all-zero on this path, dropout is the
 * identity in eval).  q, out [B, nq, H*hd] fp32; k, v [B*Lk, H*hd] in kv_dtype; hd a multiple of 4, <= 128. */
int aaclip_small_attention(int kv_dtype, const float* q, const void* k, const void* v, float* out, int B, int nq, int Lk,
                           int H, int hd, float scale, void* stream);
/* out = LayerNorm(a + b) over the last dimension D (b may be NULL): IQM_SelfOutput / IQM_Output (reference
 * model/iqm.py:143-154,219-230, eps 1e-12), IQM.layernorm (:617) and iqm_layer_norm (model/adapter.py:265, eps 1e-5). */
int aaclip_residual_layernorm(const float* a, const float* b, const float* w, const float* bias, float* out, long rows,
                              int D, float eps, void* stream);
/* out = wa a + wb b + wc c (b, c may be NULL): the fixed 0.4 / 0.3 / 0.3 fusion of reference model/iqm.py:311-315 and
 * the query + positional embedding sum of model/adapter.py:199-203. */
int aaclip_combine3(const float* a, const float* b, const float* c, float wa, float wb, float wc, float* out, long n,
                    void* stream);
/* y = x W^T + bias for in_features K <= 4: text_feature_proj, which the reference creates as Linear(2, 768) because
 * the anchors reach the branch as [B, 768, 2] (model/adapter.py:229-246).  x fp32 [R, K], W fp32 [N, K], y [R, N] in
 * out_dtype. */
int aaclip_linear_smallk(int out_dtype, const float* x, const float* W, const float* bias, void* y, long R, int N, int K,
                         void* stream);
/* ---- Backward building blocks of the IQM branch's 2-row query side (class_query_mlp, IQM.layernorm, the self-attention,
 * the query-side products of the cross-attentions, the feed-forward and iqm_layer_norm): what aaclip_gemm (fp32, on the
 * transposed weight), aaclip_gemm_wgrad, aaclip_layernorm_backward and aaclip_cross_rows_backward do not cover.  The
 * gradient of aaclip_head_expand is aaclip_head_diag times the scale and the other way round, that of aaclip_combine3 is
 * aaclip_combine3.  fp32 only; no atomics, every sum in a fixed order: two calls on the same inputs give the same bits.
 * Every pointer (and workspace) 16-byte aligned; all checks precede the first launch; each entry's errors carry its own
 * name as prefix.  Every *_workspace_bytes is 0 for an empty problem and monotonic in each argument. */

/* Backward of aaclip_small_attention for fp32 k and v.  q, d_out, d_q [B, nq, H*hd]; k, v, d_k, d_v [B*Lk, H*hd].  With
 * p_a = softmax_j(scale q_a . k_j) recomputed, g_aj = d_out_a . v_j, ds_aj = p_aj (g_aj - sum_j p_aj g_aj):
 *   d_v_j = sum_a p_aj d_out_a,  d_k_j = scale sum_a ds_aj q_a,  d_q_a = scale sum_j ds_aj k_j.
 * d_q, d_k, d_v may each be NULL, not all three.  nq <= 4, hd a multiple of 4 and <= 128 (the forward's limits), Lk in
 * 1..256, B and H <= 65535.  One workgroup per (head, image); each element of d_k and d_v is written by one thread. */
int aaclip_small_attention_backward(const float* q, const float* k, const float* v, const float* d_out, float* d_q,
                                    float* d_k, float* d_v, int B, int nq, int Lk, int H, int hd, float scale,
                                    void* stream);
/* d_w[c] = sum_r d_y[r, c] xhat[r, c], d_b[c] = sum_r d_y[r, c], xhat = (x - mean) * rstd of row r under eps: the affine
 * parameters of y = LayerNorm(x).  For LayerNorm(a + b) pass x = a + b (aaclip_combine3); the input gradient is
 * aaclip_layernorm_backward.  x, d_y [rows, D]; rows >= 1; D a multiple of 64, <= 4096; d_w or d_b may be NULL, not both. */
size_t aaclip_layernorm_param_grad_workspace_bytes(long rows, int D);
int aaclip_layernorm_param_grad(const float* x, const float* d_y, float* d_w, float* d_b, long rows, int D, float eps,
                                void* ws, size_t ws_bytes, void* stream);
/* db[n] = sum_r dz[r, n] for dz [rows, ldz >= N] (only the first N columns of a row are read). */
size_t aaclip_bias_grad_workspace_bytes(long rows, int N);
int aaclip_bias_grad(const float* dz, long ldz, float* db, long rows, int N, void* ws, size_t ws_bytes, void* stream);
/* d_z = d_y * act'.  AACLIP_ACT_GELU (erf form): zy is the PRE-ACTIVATION z, act' = Phi(z) + z phi(z).
 * AACLIP_ACT_RELU: zy is the activation's OUTPUT, act' = 1 for zy > 0 and 0 otherwise (the kink convention stated at
 * aaclip_adapter_mix_backward).  n elements; d_z may alias d_y. */
int aaclip_act_backward(int act, const float* zy, const float* d_y, float* d_z, long n, void* stream);
/* Backward of aaclip_linear_smallk for its parameters: dW[n, k] = sum_r d_y[r, n] x[r, k], db[n] = sum_r d_y[r, n];
 * x fp32 [R, K], d_y fp32 [R, N], K in 1..4; d_w or d_b may be NULL, not both.  The rows are cut into chunks whose
 * partial sums are added in chunk order.  No d_x: the anchors are constants in stage 2. */
size_t aaclip_linear_smallk_backward_workspace_bytes(long R, int N, int K);
int aaclip_linear_smallk_backward(const float* x, const float* d_y, float* d_w, float* d_b, long R, int N, int K, void* ws,
                                  size_t ws_bytes, void* stream);
/* Rows 1..L-1 of every image of src [B, L, E] (dtype) -> rows row_off.. of every image of dst [B, rows_per_image, E]:
 * the torch.cat over dim 1 of the projected tap levels without their CLS row (model/adapter.py:171,206-211). */
int aaclip_drop_cls_rows(int dtype, const void* src, void* dst, int B, int L, int E, int rows_per_image, int row_off,
                         void* stream);
/* IQM anomaly map, reference test_last.py:102-147: per level sigmoid(cos(f, q_abnormal) - cos(f, q_normal)) on the
 * patch grid, bilinear (align_corners=False) to S x S, summed over NL <= 4 levels; out = w_base * base + w_iqm * that
 * (base = the text anomaly map, 0.6 / 0.4 in test_last.py:67-68,141-147; base NULL = IQM map alone).
 * seg[l] [B, g*g, E] fp32, queries [B, 2, E] fp32 (row 0 normal, row 1 abnormal), ws >= NL*B*g*g floats. */
int aaclip_iqm_map(const float* const* seg, int NL, const float* queries, const float* base, float* out, int B, int g,
                   int E, int S, float w_base, float w_iqm, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AACLIP_H */

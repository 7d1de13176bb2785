// Internal launch interface between the C-ABI (capi.hip) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/aaclip.h"
#include "optim_pack.h"
#include "tail_plan.h"

namespace aaclip {

enum { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_RESID = 2, EPI_ACT_F32 = 3, EPI_PATCH = 4 };

struct GemmParams {
  const void* A;  // [M, lda] compute dtype
  long lda;
  const void* W;  // [N, K] compute dtype
  int M, N, K;
  const float* bias;  // [N] fp32 or null
  void* out;          // compute dtype or fp32, by epilogue
  long ldc;
  int scale_cols;  // EPI_BIAS: columns < scale_cols are multiplied by scale
  float scale;
  int act;           // EPI_ACT_F32: 0 none, 1 LeakyReLU(0.01)
  const float* pos;  // EPI_PATCH: positional embedding [L, N]
  int P, L;          // EPI_PATCH: patches per image, tokens per image
  const float* resid;      // EPI_BIAS_RESID: where the residual is READ ([M, ldc] fp32); null = in place, from `out`
  // LayerNorm folding (16x16x32 256-tile kernels only; all null = off), see capi.hip aaclip_block:
  void* out16;             // EPI_BIAS_RESID: also write the new residual rows in the compute dtype, [M, N]
  float* stats_out;        // EPI_BIAS_RESID: per row and 64-column slice (sum, sum of squares) of the new rows, [M][N/64][2]
  const float* row_ab;     // EPI_BIAS / EPI_BIAS_GELU: per row (a, b); value = a*acc + b*col_s[n] + bias[n]
  const float* col_s;      //   [N] row sums of the (gamma-scaled) weight
  // AACLIP_F16X2 (split fp16, common.h): A is [M, >= 2K] (hi | lo per row, lda = row stride), W is [N, 2K] (hi | lo)
  // or, with w_exact16, [N, K] (the weight is exact in fp16: the Ah.Wl product is skipped); 16-bit outputs are split
  // rows too ([M, >= 2N], ldc = row stride, lo plane N columns after the hi plane).
  int w_exact16;
  int out_qk8;                // EPI_BIAS, split fp16, 256-tile kernel only: > 0 = the output is the attention kernel's
                              // [hi: N fp16][per 64 columns below out_qk8: lo8 64 B | hi8 64 B] record: 2N + 2 out_qk8 bytes, so
                              // ldc >= N + out_qk8 halves (gemm_check; the QKV product: N = 3D, out_qk8 = 2D, ldc = 5D)
  int out_no_hi8;             // EPI_BIAS_GELU, split fp16: the consumer's weight is exact in fp16 -- skip the hi8 plane
};

const char* gemm_check(int dtype, int epi, const GemmParams& p);
void launch_gemm(int dtype, int epi, const GemmParams& p, hipStream_t s);
bool gemm256_applicable(int dtype, const GemmParams& p);
// 256-tile kernels on 16x16x32 MFMAs (gemm256t.hip), bit-identical to one another: the 8-wave 256 x 256 kernel, the
// 4-wave 256 x 128 half tile, and the 8-wave kernel walking its tiles (split operands only; plain operands run the
// 256 x 256 form).  Plain operands with an odd K-tile count run the one-set 8-wave kernel whatever form is asked for.
enum Gemm256Form { GEMM256_TILE, GEMM256_HALF_TILE, GEMM256_WALK };
void launch_gemm256t(int dtype, int epi, const GemmParams& p, hipStream_t s, Gemm256Form form);
// The LayerNorm that follows a split fp16 residual product, run beside the product's partial last round (tail_plan.h).
// LnRows: its weights, its split8 output rows and the hi8 flag of launch_layernorm; it reads the product's output.
struct LnRows { const float* w; const float* b; void* out; float eps; bool hi8; };
// kernel argument of the tail launch (gemm256t.hip); all zero for every other launch of the kernel
struct LnTail {
  const float* x; const float* w; const float* b;
  _Float16* out;
  long rows;
  float eps;
  int nch, hi8;
  TailSlots slots;
};
// gemm256t.hip: launches A and B, returns the rows whose LayerNorm is done (0: plan not engaged, nothing launched)
long launch_resid_ln_tail(const GemmParams& p, const LnRows& ln, hipStream_t s);
// gemm.hip: the residual product p, and where the tail overlap applies (split fp16 on the walking kernel, switch on, plan
// engaged) the LayerNorm `ln` of its first rows with it; returns how many rows of `ln` are done (0: none, plain launch)
long launch_gemm_resid_ln(int dtype, const GemmParams& p, const LnRows& ln, hipStream_t s);
void set_tail_overlap(bool on);
void set_plan_cus(int cus);   // CU count the row split is planned with; 0 = the device's (tests: a tail at small shapes)
long tail_launch_count();     // tail launches (launch B) issued so far
// Kernel selection, for the tests that compare the forms with one another: GEMM variants 0 (automatic), 1 (128-tile
// kernel) and 80 / 81 / 82 (the 256-tile forms, gemm.hip), attention variants 0 and 1 (128-query kernel).  Both return
// false for anything else and leave the selection alone.
bool set_gemm_variant(int v);
bool set_attn_variant(int v);
// Sticky per-thread launch error: set by a launcher that was asked for a kernel it does not have; capi's finish()
// reports and clears it, so the entry point returns rc < 0 instead of running something else.
void set_launch_error(const char* msg);
const char* take_launch_error();
// Run-time launcher arguments as compile-time constants: f(std::integral_constant<int, EPI_...>{}) / f(std::bool_constant<b>{}).
// An epilogue nobody knows launches nothing and records a launch error (gemm_check refuses it before any launcher runs).
template <typename F> void dispatch_epi(int epi, F&& f) {
  switch (epi) {
    case EPI_BIAS: f(std::integral_constant<int, EPI_BIAS>{}); break;
    case EPI_BIAS_GELU: f(std::integral_constant<int, EPI_BIAS_GELU>{}); break;
    case EPI_BIAS_RESID: f(std::integral_constant<int, EPI_BIAS_RESID>{}); break;
    case EPI_ACT_F32: f(std::integral_constant<int, EPI_ACT_F32>{}); break;
    case EPI_PATCH: f(std::integral_constant<int, EPI_PATCH>{}); break;
    default: set_launch_error("gemm: no kernel for this epilogue");
  }
}
template <typename F> void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// fused softmax(q k^T) v over packed qkv [B*L, 3*H*64] (q pre-scaled) -> ctx [B*L, H*64]
// log2q != 0: q is pre-multiplied by log2(e) as well (16-bit kernels only)
void launch_attention(int dtype, const void* qkv, void* ctx, int B, int L, int H, int causal, int log2q,
                      hipStream_t s, bool hi8 = true, bool qk8 = false);
// qk8 (split fp16, log2q, L >= 512 only): qkv rows are [q k v hi: 3D fp16][q8][k8] records of 10 D bytes (attention.hip,
// GemmParams::out_qk8) instead of split16 rows
bool attention_qk8_applicable(int L, int causal);

// row ops (rowops.hip); D in {256, 768, 1024}
const char* row_width_check(int D);
// hi8 = false (split fp16 only): do not write the hi8 plane of the split8 rows -- for a consumer whose weight is exact
// in fp16 and therefore never reads it (common.h); the same flag exists on every producer of split8 rows
void launch_layernorm(int out_dtype, const float* x, const float* w, const float* b, void* out, long rows, int D,
                      float eps, hipStream_t s, bool hi8 = true);
void launch_adapter_mix(float* x, const float* a, long rows, int D, float weight, hipStream_t s);
void launch_adapter_mix_fold(int dtype, float* x, const float* a, long rows, int D, float weight, void* out16,
                             float* rowab, hipStream_t s);   // also emits the 16-bit rows and (rstd, -mean*rstd)
void launch_im2col(int dtype, const float* img, void* cols, int B, int C, int H, int W, int ps, int Kpad,
                   hipStream_t s);
void launch_cls_rows(float* x, const float* cls, const float* pos, int B, int L, int D, hipStream_t s);
void launch_embed_text(const int32_t* tokens, const float* table, const float* pos, float* x, int n, int T, int D,
                       int vocab, hipStream_t s);
void launch_gather_rows(int dtype, const void* src, void* dst, const int32_t* tokens, int n, int T, int D, int mode,
                        hipStream_t s);
void launch_normalize_rows(const float* src, float* dst, int B, int L, int skip, int E, hipStream_t s);
void launch_det_mean(const float* src, float* scratch, size_t scratch_floats, float* dst, int B, int L, int skip, int E,
                     hipStream_t s);

// anomaly map (anomaly_map.hip)
// mode 0: test-mode map m = (s1 + 1 - s0)/2 -> pre [B, P]; mode 1: raw scores -> [B, 2, P]
void launch_patch_scores(const float* seg, const float* anchors, long anchor_bstride, float* pre, int B, int P, int E,
                         int mode, hipStream_t s);
// pre [NL][B, g, g] -> out [B, S, S] = sum over levels of upsample(blur(pre_l)); NL <= 4, g <= 40
void launch_blur_upsample(const float* pre, float* out, int B, int g, int S, int NL, int ksize, float sigma,
                          hipStream_t s);
void launch_upsample_softmax2(const float* scores, float* out, int B, int g, int S, hipStream_t s);
void launch_cast_rows(int dtype, const float* src, void* dst, long n, hipStream_t s);
void launch_split_rows(const float* src, void* dst, long rows, int D, hipStream_t s, bool hi8 = true);   // fp32 [rows, D] -> split fp16 [rows, 2D]
// LayerNorm folding: [M][slots][2] partial (sum, sumsq) -> [M][2] (rstd, -mean*rstd)
void launch_ln_stats_finalize(const float* partials, float* ab, long rows, int slots, int D, float eps, hipStream_t s);
bool gemm_routes_to_256t(int dtype, const GemmParams& p);   // launch_gemm will run a kernel with the folding epilogue
bool gemm_split_routes_to_256t(const GemmParams& p);        // split fp16: ... the 256-tile kernel (out_qk8 epilogue)
// V-V "surgery" attention over the batch axis: regroup v [B*L,D] -> packed q|k|v rows l*B+b and back
void launch_vv_spread(int dtype, const void* v, void* qkv, int B, int L, int D, float scale, hipStream_t s);
void launch_vv_regroup(int dtype, const void* src, void* dst, int B, int L, int D, hipStream_t s);

// ---- iqm.hip : the IQM side branch's small kernels (include/aaclip.h, "IQM side branch")
const char* small_attention_check(int nq, int Lk, int H, int hd);
void launch_small_attention(int kv_dtype, const float* q, const void* k, const void* v, float* out, int B, int nq, int Lk,
                            int H, int hd, float scale, hipStream_t s);
const char* cross_rows_check(int R, int Lk, int Dk);
size_t cross_rows_ws_bytes(int B, int R, int Lk, int Dk);
void launch_cross_rows(int x_dtype, const float* qt, const void* x, float* out, void* ws, int B, int R, int Lk, int Dk,
                       hipStream_t s);
const char* cross_rows_levels_check(int x_dtype, int R, int nseg, int Lk, int Dk, long ldx);
size_t cross_rows_levels_ws_bytes(int B, int nseg, int Lk, int Dk);
void launch_cross_rows_levels(int x_dtype, const float* qt, const void* const* x, int nseg, float* out, void* ws, int B,
                              int R, int rows_per_image, int row0, int Lk, int Dk, long ldx, hipStream_t s);
void launch_head_expand(int dtype, const float* q, void* qm, long rows, int H, int D, float scale, hipStream_t s);
void launch_head_diag(const float* full, float* ctx, long rows, int H, int D, hipStream_t s);
void launch_residual_layernorm(const float* a, const float* b, const float* w, const float* bias, float* out, long rows,
                               int D, float eps, hipStream_t s);
void launch_combine3(const float* a, const float* b, const float* c, float wa, float wb, float wc, float* out, long n,
                     hipStream_t s);
void launch_linear_smallk(int out_dtype, const float* x, const float* W, const float* bias, void* y, long R, int N, int K,
                          hipStream_t s);
void launch_drop_cls_rows(int dtype, const void* src, void* dst, int B, int L, int E, int rows_per_image, int row_off,
                          hipStream_t s);
void launch_iqm_scores(const float* seg, const float* q, float* grid, int B, int P, int E, hipStream_t s);
void launch_iqm_upsample(const float* grids, const float* base, float* out, int B, int g, int S, int NL, float w_base,
                         float w_iqm, hipStream_t s);

// ---- train_loss.hip : segmentation loss (focal + dice) with its gradient, train-mode similarity map backward
enum { SEG_LOSS_FOCAL = 1, SEG_LOSS_DICE0 = 2, SEG_LOSS_DICE1 = 4 };   // = AACLIP_SEG_LOSS_* (include/aaclip.h)
constexpr int SEG_LOSS_CHUNKS = 64;   // pixel chunks per image of the first pass
constexpr int SEG_LOSS_NSUM = 6;      // per-chunk sums
constexpr int SIMMAP_BWD_MAX_S = 2048;
inline size_t seg_loss_part_bytes(int B) {
  return ((size_t)B * SEG_LOSS_CHUNKS * SEG_LOSS_NSUM * 4 + 255) & ~(size_t)255;
}
inline size_t seg_loss_ws_bytes(int B) { return seg_loss_part_bytes(B) + (size_t)B * 3 * 8; }
inline size_t simmap_bwd_t_floats(int B, int g, int S) { return (size_t)B * S * g; }
inline size_t simmap_bwd_ws_bytes(int B, int g, int S) { return (simmap_bwd_t_floats(B, g, S) + (size_t)B * g * g) * 4; }
// preds: image b, channel c, pixel i at preds[b * img_stride + c * chan_stride + i]; mask [B, P]; coef [B, 4]
void launch_seg_loss(const float* preds, long img_stride, long chan_stride, const float* mask, int terms, float* loss,
                     float* coef, int B, long P, void* ws, hipStream_t s);
void launch_seg_loss_grad(const float* preds, long img_stride, long chan_stride, const float* mask, int terms,
                          const float* coef, const float* d_loss, float* d_preds, int B, long P, hipStream_t s);
void launch_similarity_map_train_bwd(const float* seg, const float* anchors, long anchor_bstride, const float* preds,
                                     const float* d_preds, float* d_anchors, float* d_seg, int B, int g, int E, int S,
                                     void* ws, hipStream_t s);

// ---- iqm_loss.hip : the IQM map term of the stage-2 loss, one tap level per call (half-pixel upsample of (1 - p, p))
constexpr int IQ_QCHUNKS = 32;   // patch chunks of the query-gradient sum: E / 256 * 32 * B workgroups
// chunk sums [B, IQ_QCHUNKS, 2, E] | T [B, S, g] | dz [B, P] | per-row scalars [B, P, 4] | [B, IQ_QCHUNKS, 2]
inline size_t iqm_map_train_bwd_ws_bytes(int B, int g, int E, int S) {
  return ((size_t)B * S * g + (size_t)B * g * g * 5 + (size_t)B * IQ_QCHUNKS * 2 * ((size_t)E + 1)) * 4;
}
// grid (out) [B, g*g] = launch_iqm_scores' values; out [B, 2, S, S]
void launch_iqm_map_train(const float* seg, const float* q, float* grid, float* out, int B, int g, int E, int S,
                          hipStream_t s);
// d_seg [B, g*g, E] and d_q [B, 2, E]: either may be null
void launch_iqm_map_train_bwd(const float* seg, const float* q, const float* grid, const float* d_preds, float* d_seg,
                              float* d_q, int B, int g, int E, int S, void* ws, hipStream_t s);

// ---- iqm_backward.hip : backward of aaclip_cross_rows (d_qt [B, R, Dk] and d_x [B, Lk, Dk]; either may be null)
constexpr int CRB_MAX_SLICES = 128;   // key slices per image: slices x B workgroups, slices x R x Dk partial sums of d_qt
int cross_rows_backward_slices(int Lk);
size_t cross_rows_backward_ws_bytes(int B, int R, int Lk, int Dk);
void launch_cross_rows_backward(int x_dtype, const float* qt, const void* x, const float* dout, float* d_qt, float* d_x,
                                int act, int accumulate, int B, int R, int Lk, int Dk, void* ws, hipStream_t s);

// ---- iqm_levels_backward.hip : backward of aaclip_cross_rows_levels (qt, d_out, d_qt [B, R, nseg, Dk]; d_x[s] fp32
// [B * rows_per_image, Dk]; d_qt or the whole d_x array may be null); a segment's keys are sliced as above
const char* cross_rows_levels_backward_check(int x_dtype, int R, int nseg, int Lk, int Dk, long ldx);
size_t cross_rows_levels_backward_ws_bytes(int B, int R, int nseg, int Lk, int Dk);
void launch_cross_rows_levels_backward(int x_dtype, const float* qt, const void* const* x, int nseg, const float* dout,
                                       float* d_qt, float* const* d_x, int accumulate, int B, int R, int rows_per_image,
                                       int row0, int Lk, int Dk, long ldx, void* ws, hipStream_t s);

// ---- iqm_query_backward.hip : backward building blocks of the IQM branch's 2-row query side (fp32, fixed-order sums)
constexpr int SAB_MAXK = 256;          // keys of small_attention_backward: one per thread
constexpr int IQB_CHUNK_ROWS = 32;     // rows of a chunk of the column sums, up to IQB_MAX_CHUNKS chunks (then longer ones)
constexpr int IQB_MAX_CHUNKS = 64;
int iqb_chunks(long rows);
void launch_small_attention_backward(const float* q, const float* k, const float* v, const float* dout, float* d_q,
                                     float* d_k, float* d_v, int B, int nq, int Lk, int H, int hd, float scale,
                                     hipStream_t s);
size_t layernorm_param_grad_ws_bytes(long rows, int D);
void launch_layernorm_param_grad(const float* x, const float* dy, float* d_w, float* d_b, long rows, int D, float eps,
                                 void* ws, hipStream_t s);
size_t bias_grad_ws_bytes(long rows, int N);
void launch_bias_grad(const float* dz, long ldz, float* db, long rows, int N, void* ws, hipStream_t s);
void launch_iqm_act_backward(int act, const float* zy, const float* dy, float* dz, long n, hipStream_t s);
size_t linear_smallk_backward_ws_bytes(long R, int N, int K);
void launch_linear_smallk_backward(const float* x, const float* dy, float* d_w, float* d_b, long R, int N, int K, void* ws,
                                   hipStream_t s);

// ---- text_backward.hip : backward of the adapted text tower (fp32, fixed-order reductions)
constexpr int ATTN_BWD_MAX_L = 128;
constexpr int WGRAD_MAX_CHUNKS = 16;
// dw[O, I] = sum_r dz[r, o] u[r, i]; O, I multiples of 128, ldz / ldu multiples of 4; ws >= wgrad_ws_bytes
size_t wgrad_ws_bytes(long rows, int O, int I);
void launch_wgrad(const float* dz, long ldz, const float* u, long ldu, float* dw, long rows, int O, int I, void* ws,
                  hipStream_t s);
const char* attention_backward_check(int B, int L, int H);
// qkv [B*L, 3*H*64] (q pre-scaled), dctx [B*L, H*64] -> dqkv [B*L, 3*H*64]; the dq columns are multiplied by dq_scale
void launch_attention_backward(const float* qkv, const float* dctx, float* dqkv, int B, int L, int H, int causal,
                               float dq_scale, hipStream_t s);
// attention_backward.hip: the same for any L, tiled on the fp32 MFMA; ws holds the 3*B*H*L row statistics
const char* attention_backward_long_check(int B, int L, int H);
size_t attention_backward_long_ws_bytes(int B, int L, int H);
void launch_attention_backward_long(const float* qkv, const float* dctx, float* dqkv, int B, int L, int H, int causal,
                                    float dq_scale, void* ws, hipStream_t s);
// dx[out_rows ? out_rows[r] : r] = LayerNorm input gradient of row r (+ add, read at the output row)
void launch_layernorm_backward(const float* x, const float* w, const float* dy, const float* add, float* dx,
                               const int* out_rows, long rows, int D, float eps, hipStream_t s);
void launch_adapter_mix_backward(const float* u, const float* z, const float* dy, float* dz, float* du, long rows, int D,
                                 float weight, hipStream_t s);
void launch_gelu_forward(const float* f, float* out, long n, hipStream_t s);
void launch_gelu_backward(const float* f, const float* dg, float* df, long n, hipStream_t s);
void launch_act_backward(const float* z, const float* dy, float* dz, long n, int act, hipStream_t s);
void launch_add_rows(const float* a, const float* b, float* out, long n, hipStream_t s);
// in place on z [B*L, E] (pre-activation rows of a tap / det head): z <- dz of y = normalize(act(z)); det == 0: d is
// d_seg [B, L-1, E]; det != 0: d is d_det [B, E], the gradient of the mean over the patch rows.  CLS rows <- 0.
void launch_head_normalize_backward(float* z, const float* d, int B, int L, int E, int act, int det, hipStream_t s);
void launch_pick_rows(const float* x, float* dst, int* idx, const int32_t* tokens, int n, int T, int D, int mode,
                      hipStream_t s);

// ---- preprocess.hip : 8-bit bicubic resize + ToTensor + Normalize (Pillow-exact)
int resample_ksize(int in_size, int out_size);
void resample_table(int in_size, int out_size, int32_t* bounds, int32_t* coefs);   // host buffers
int preprocess_tile_rows(int in_size, int out_size, int ty);
int preprocess_row_pitch(int in_w, int out_size);
void launch_preprocess(const uint8_t* src, int B, int Hs, int Ws, int S, const int32_t* hb, const int32_t* hk, int kx,
                       const int32_t* vb, const int32_t* vk, int ky, int TY, int lds_rows, int pitch, const float* lut,
                       float* out, hipStream_t s);

// ---- augment.hip : train-time colour jitter (Pillow-exact), mask resize, rotation / shift / flips in one gather
int color_jitter_sum_blocks(long pixels);   // workgroups per frame of the luma sum = 64-bit partials per frame
// ws: [B * color_jitter_sum_blocks(H * W)] 64-bit partial sums, then [B] int32 means
void launch_color_jitter(const uint8_t* src, uint8_t* dst, int B, int H, int W, const float* factors,
                         const int32_t* apply, void* ws, hipStream_t s);
void nearest_table(int in_size, int out_size, int32_t* idx);   // host buffer
void launch_mask_preprocess(const uint8_t* src, int B, int Hm, int Wm, int S, const int32_t* xmap, const int32_t* ymap,
                            const int32_t* normal, float* out, hipStream_t s);
void launch_augment_geometric(const float* image, const float* mask, int B, int S, const float* angle_deg,
                              const int32_t* shift, const int32_t* flags, float* image_out, float* mask_out,
                              hipStream_t s);

// ---- metrics.hip : exact AUROC / AP of one class: range, normalise, ordered keys, stable radix sort, curve sums
long metrics_range_partials(long n, long per_image);   // workgroups of the first range stage (per_image 0: one segment)
size_t metrics_range_ws_bytes(long n, long per_image);
void launch_metrics_range(const float* scores, const uint8_t* labels, long n, long per_image, float* image_max,
                          void* record, void* ws, hipStream_t s);
void launch_metrics_normalise(const float* in, float* out, long n, const void* record, hipStream_t s);
long metrics_sort_group_items();                       // keys one workgroup of the sort takes
size_t metrics_sort_ws_bytes(long n);
void launch_metrics_sort(const float* scores, const uint8_t* labels, long n, int packed, uint32_t* keys,
                         uint8_t* labels_sorted, unsigned long long* out_of_range, void* ws, hipStream_t s);
size_t metrics_curve_ws_bytes(long n);
void launch_metrics_curve(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed, void* record, void* ws,
                          hipStream_t s);
size_t metrics_f1max_ws_bytes(long n);                 // F1-max: the curve's first phases, then an integer argmax
void launch_metrics_f1max(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed, void* record, void* ws,
                          hipStream_t s);
size_t metrics_threshold_ws_bytes(long n, long per_image);
void launch_metrics_threshold(const float* scores, const uint8_t* labels, long n, long per_image,
                              const void* range_record, const void* f1max_record, uint8_t* mask,
                              uint32_t* image_counts, void* totals, void* ws, hipStream_t s);
size_t metrics_sort_pairs_ws_bytes(long n);
void launch_metrics_sort_pairs(const float* scores, const uint32_t* values, long n, uint32_t* keys,
                               uint32_t* values_sorted, void* ws, hipStream_t s);
// ---- regions.hip : per-region overlap (AUPRO): connected components with canonical ids and areas, the PRO curve
size_t metrics_regions_ws_bytes(long n);
void launch_metrics_regions(const uint8_t* mask, long n, int H, int W, int connectivity, uint32_t* region,
                            uint32_t* area, void* record, void* ws, hipStream_t s);
size_t metrics_pro_curve_ws_bytes(long n);
void launch_metrics_pro_curve(const uint32_t* keys, const uint32_t* areas_sorted, long n, const void* regions_record,
                              double fpr_limit, void* record, void* ws, hipStream_t s);
// ---- region_table.hip : one row per region of launch_metrics_regions: box, peak, overlap with a second mask
size_t region_table_ws_bytes(long n, long images);
void launch_region_table(const uint32_t* region, const uint32_t* area, const float* scores, const void* range_record,
                         const uint8_t* other, long images, int H, int W, long min_area, long capacity, void* rows,
                         int32_t* image_offsets, uint8_t* kept_mask, void* record, void* ws, hipStream_t s);

// ---- support.hip : nearest bank row of every query row (the candidate word, tiling and workspace are support_pack.h)
size_t support_ws_bytes(long M);
void launch_support_nearest(const float* q, long M, const void* bank, long N, int E, int form, float* best_cos,
                            int* best_idx, void* ws, hipStream_t s);
void launch_support_bank_rows(const float* rows, long N, int E, int form, void* bank, hipStream_t s);
void launch_support_dist(const float* cosine, float* d, long n, hipStream_t s);              // d = 1 - cosine
void launch_support_add(const float* base, float weight, float* out, long n, hipStream_t s);   // out = base + weight * out

// ---- coreset.hip : greedy k-center selection over quantised bank rows (the quantiser, the candidate word, the plan and
// the workspace are coreset_pack.h)
size_t coreset_ws_bytes(long n);
void launch_coreset_rows(const float* rows, long N, int E, int16_t* q, int32_t* norm2, hipStream_t s);
void launch_coreset_select(const int16_t* q, const int32_t* norm2, long N, int E, long n, long start, int32_t* picks,
                           uint32_t* radius2, uint32_t* min_d2, void* ws, hipStream_t s);
void launch_coreset_unit_rows(const float* rows, long N, int E, float* out, hipStream_t s);   // out = rows / |row|

// ---- bootstrap.hip : bootstrap of AUROC / AP over images, a weighted curve pass over ONE sort (the records, the group
// term and the workspace layout are bootstrap_plan.h)
size_t bootstrap_ws_bytes(long n, long R);
long bootstrap_max_images();
void launch_bootstrap_curves(const uint32_t* keys, const uint32_t* payload, long n, const uint8_t* counts, long images,
                             long R, void* records, void* ws, hipStream_t s);

// ---- multi-tensor optimizer (optim.hip; the launch packing is optim_pack.h)
struct OptimGroupScalars {   // one group's hyper-parameters as the kernel reads them: formed in fp64, rounded once
  float beta1, one_minus_beta1, beta2, one_minus_beta2;
  float step_size;           // lr / (1 - beta1^step)
  float sqrt_bc2;            // sqrt(1 - beta2^step)
  float eps;
  float weight_decay;        // coupled: g += weight_decay * p
  float decay;               // decoupled: p *= 1 - lr * weight_decay; exactly 1 otherwise
  int coupled;
};
size_t optim_grad_norm_ws_bytes(long chunks);
// items: the caller's list; counts[i] = items[i].n (what optim_pack.h walks); record: aaclip_optim_record on the device
void launch_optim_grad_norm(const aaclip_optim_tensor* items, const long* counts, long tensors, float max_norm,
                            void* record, void* ws, hipStream_t s);
void launch_optim_adam_step(const aaclip_optim_tensor* items, const long* counts, long tensors,
                            const OptimGroupScalars* groups, int n_groups, const void* record, hipStream_t s);

}  // namespace aaclip

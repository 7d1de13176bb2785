// Launch interface of the three-term bf16 backward (split3_rows.hip, attention_backward_bf16x3.hip), next to kernels.h.
//
// bf16x3: a value v is carried as hi = bf16(v), lo = bf16(v - hi) (round to nearest even, no scale anywhere: bf16 has
// fp32's exponent), and a product is summed as Ah.Bh + Al.Bh + Ah.Bl in fp32 accumulators (Al.Bl, <= 2^-16 of the main
// term, is dropped).  About 16 significant bits per operand over fp32's whole range -- what gradients need and the
// fp16-based split formats of common.h, with their fixed scales, do not give.
//   split3 row     bf16 [rows, 3K] = [hi | lo | hi]: the A operand of a plain bf16 GEMM over K' = 3K against the stacked
//                  weight [N, 3K] = [Wh | Wh | Wl] (engine.split3_weight): the three terms in one accumulator.
#pragma once
#include "kernels.h"

namespace aaclip {

// fp32 [rows, K] -> split3 rows; K a multiple of 64, 16-byte aligned pointers
void launch_split3_rows(const float* src, void* dst, long rows, int K, hipStream_t s);
// split3 rows of gelu_erf(f) / of dg * gelu_erf'(f) (text_backward.hip's element-wise kernel, mode 0 / 1) without the
// fp32 rows in between: the F-wide A operands of c_proj and of the c_fc input-gradient product
void launch_gelu_forward_split3(const float* f, void* dst, long rows, int K, hipStream_t s);
void launch_gelu_backward_split3(const float* f, const float* dg, void* dst, long rows, int K, hipStream_t s);

// launch_attention_backward_long's contract on the bf16 MFMA; ws >= attention_backward_long_bf16x3_ws_bytes
size_t attention_backward_long_bf16x3_ws_bytes(int B, int L, int H);
void launch_attention_backward_long_bf16x3(const float* qkv, const float* dctx, float* dqkv, int B, int L, int H,
                                           int causal, float dq_scale, void* ws, hipStream_t s);

}  // namespace aaclip

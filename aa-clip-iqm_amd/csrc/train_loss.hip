// Training-side kernels of the text-adapter stage (reference train.py:38-114): the segmentation loss of
// forward_utils.py:21-108,223-227 (focal + two dice terms) with its gradient, and the backward of the train-mode
// similarity map (forward_utils.py:196-216, test=False), whose forward is upsample_softmax2_kernel (anomaly_map.hip).
//   seg_loss_sums   per (image, pixel chunk): focal sum and the four dice sums, fp32 inside a block, fixed tree
//   seg_loss_final  per image in double over the chunks in chunk order -> loss[4] and the per-image gradient
//                   coefficients of the dice terms
//   seg_loss_grad   per pixel: d loss / d preds
//   upsample_bwd_rows / _cols   d preds -> softmax backward -> transpose of the align-corners bilinear upsample, as a
//                   gather over each coarse cell's support window (separable: fine columns, then fine rows); x100
//   anchor_grad     d anchors[b, e, c] = sum_p f[b, p, e] dS[b, p, c] (4 waves over p, summed in wave order)
//   patch_grad      d f[b, p, e] = sum_c dS[b, p, c] t[b, e, c]
// Every reduction runs in a fixed order (no atomics): two calls on the same inputs give bit-identical results.
#include "common.h"
#include "kernels.h"

namespace aaclip {

constexpr int SL_THREADS = 256;
constexpr float SL_SMOOTH = 1e-5f;   // FocalLoss.smooth: one-hot clamp and the + smooth of pt

// the mask's class index as the reference forms it (target.cpu().long(): truncation; masks hold 0 / 1)
AACLIP_DEV int mask_class(float m) { return m >= 1.0f ? 1 : 0; }

AACLIP_DEV float block_sum256(float v, float* red) {   // fixed tree: wave shuffle, then the 4 waves in order
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// part[(b * chunks + chunk) * SEG_LOSS_NSUM + k], k: 0 focal, 1 sum p0, 2 sum p0 (1 - m), 3 sum p1, 4 sum p1 m, 5 sum m
__global__ __launch_bounds__(SL_THREADS) void seg_loss_sums_kernel(const float* __restrict__ preds, long img_stride,
                                                                    long chan_stride, const float* __restrict__ mask,
                                                                    int terms, float* __restrict__ part, long P,
                                                                    int chunks) {
  __shared__ float red[4];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const long per = (P + chunks - 1) / chunks;
  const long i0 = chunk * per;
  const long i1 = i0 + per < P ? i0 + per : P;
  const float* p0 = preds + b * img_stride;
  const float* p1 = p0 + chan_stride;
  const float* m = mask + b * P;
  float s[SEG_LOSS_NSUM] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long i = i0 + threadIdx.x; i < i1; i += SL_THREADS) {
    const float a = p0[i], c = p1[i], mv = m[i];
    if (terms & SEG_LOSS_FOCAL) {
      const int k = mask_class(mv);
      const float oh0 = k == 0 ? 1.0f - SL_SMOOTH : SL_SMOOTH, oh1 = k == 1 ? 1.0f - SL_SMOOTH : SL_SMOOTH;
      const float pt = (oh0 * a + oh1 * c) + SL_SMOOTH;
      const float q = 1.0f - pt;
      s[0] += -(q * q) * logf(pt);
    }
    s[1] += a;
    s[2] += a * (1.0f - mv);
    s[3] += c;
    s[4] += c * mv;
    s[5] += mv;
  }
  float* out = part + ((long)b * chunks + chunk) * SEG_LOSS_NSUM;
#pragma unroll
  for (int k = 0; k < SEG_LOSS_NSUM; ++k) {
    const float t = block_sum256(s[k], red);
    if (threadIdx.x == 0) out[k] = t;
  }
}

// one block: images in order.  loss[4] = {total, focal, dice0, dice1} (a term not in `terms` is 0); coef[b * 4 ..] =
// {a0, c0, a1, c1}: d(dice0)/d p0 = a0 (1 - m) + c0 and d(dice1)/d p1 = a1 m + c1 at every pixel of image b
__global__ __launch_bounds__(SL_THREADS) void seg_loss_final_kernel(const float* __restrict__ part, int chunks, int B,
                                                                     long P, int terms, float* __restrict__ loss,
                                                                     float* __restrict__ coef,
                                                                     double* __restrict__ img) {
  for (int b = threadIdx.x; b < B; b += SL_THREADS) {
    double s[SEG_LOSS_NSUM] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < chunks; ++c)
      for (int k = 0; k < SEG_LOSS_NSUM; ++k) s[k] += (double)part[((long)b * chunks + c) * SEG_LOSS_NSUM + k];
    const double num0 = 2.0 * s[2] + 1.0, den0 = s[1] + ((double)P - s[5]) + 1.0;
    const double num1 = 2.0 * s[4] + 1.0, den1 = s[3] + s[5] + 1.0;
    img[b * 3 + 0] = s[0];
    img[b * 3 + 1] = num0 / den0;
    img[b * 3 + 2] = num1 / den1;
    coef[b * 4 + 0] = (float)(-2.0 / ((double)B * den0));
    coef[b * 4 + 1] = (float)(num0 / ((double)B * den0 * den0));
    coef[b * 4 + 2] = (float)(-2.0 / ((double)B * den1));
    coef[b * 4 + 3] = (float)(num1 / ((double)B * den1 * den1));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double f = 0, d0 = 0, d1 = 0;
    for (int b = 0; b < B; ++b) {
      f += img[b * 3 + 0];
      d0 += img[b * 3 + 1];
      d1 += img[b * 3 + 2];
    }
    const float focal = (terms & SEG_LOSS_FOCAL) ? (float)(f / ((double)B * (double)P)) : 0.f;
    const float dice0 = (terms & SEG_LOSS_DICE0) ? (float)(1.0 - d0 / B) : 0.f;
    const float dice1 = (terms & SEG_LOSS_DICE1) ? (float)(1.0 - d1 / B) : 0.f;
    loss[0] = (focal + dice0) + dice1;   // calculate_seg_loss: loss = focal; loss += dice0; loss += dice1
    loss[1] = focal;
    loss[2] = dice0;
    loss[3] = dice1;
  }
}

// d_loss[4]: gradient of the loss[4] output; a channel no enabled term reads is not written
__global__ __launch_bounds__(SL_THREADS) void seg_loss_grad_kernel(const float* __restrict__ preds, long img_stride,
                                                                    long chan_stride, const float* __restrict__ mask,
                                                                    int terms, const float* __restrict__ coef,
                                                                    const float* __restrict__ d_loss,
                                                                    float* __restrict__ d_preds, int B, long P) {
  const long idx = (long)blockIdx.x * SL_THREADS + threadIdx.x;
  if (idx >= (long)B * P) return;
  const long b = idx / P, i = idx - b * P;
  const float g = d_loss[0];
  const float wf = g + d_loss[1], w0 = g + d_loss[2], w1 = g + d_loss[3];
  const float a = preds[b * img_stride + i], c = preds[b * img_stride + chan_stride + i], mv = mask[idx];
  float g0 = 0.f, g1 = 0.f;
  if (terms & SEG_LOSS_FOCAL) {
    const int k = mask_class(mv);
    const float oh0 = k == 0 ? 1.0f - SL_SMOOTH : SL_SMOOTH, oh1 = k == 1 ? 1.0f - SL_SMOOTH : SL_SMOOTH;
    const float pt = (oh0 * a + oh1 * c) + SL_SMOOTH;
    const float q = 1.0f - pt;
    // d/dpt of -(1 - pt)^2 log pt, over the B*P pixels of the mean
    const float dpt = wf * (2.0f * q * logf(pt) - q * q / pt) / ((float)B * (float)P);
    g0 = dpt * oh0;
    g1 = dpt * oh1;
  }
  const float* cf = coef + b * 4;
  if (terms & SEG_LOSS_DICE0) g0 += w0 * (cf[0] * (1.0f - mv) + cf[1]);
  if (terms & SEG_LOSS_DICE1) g1 += w1 * (cf[2] * mv + cf[3]);
  if (terms & (SEG_LOSS_FOCAL | SEG_LOSS_DICE0)) d_preds[b * img_stride + i] = g0;
  if (terms & (SEG_LOSS_FOCAL | SEG_LOSS_DICE1)) d_preds[b * img_stride + chan_stride + i] = g1;
}

void launch_seg_loss(const float* preds, long img_stride, long chan_stride, const float* mask, int terms, float* loss,
                     float* coef, int B, long P, void* ws, hipStream_t s) {
  float* part = (float*)ws;
  double* img = (double*)((char*)ws + seg_loss_part_bytes(B));
  hipLaunchKernelGGL(seg_loss_sums_kernel, dim3(SEG_LOSS_CHUNKS, B), dim3(SL_THREADS), 0, s, preds, img_stride,
                     chan_stride, mask, terms, part, P, SEG_LOSS_CHUNKS);
  hipLaunchKernelGGL(seg_loss_final_kernel, dim3(1), dim3(SL_THREADS), 0, s, part, SEG_LOSS_CHUNKS, B, P, terms, loss,
                     coef, img);
}

void launch_seg_loss_grad(const float* preds, long img_stride, long chan_stride, const float* mask, int terms,
                          const float* coef, const float* d_loss, float* d_preds, int B, long P, hipStream_t s) {
  const long n = (long)B * P;
  hipLaunchKernelGGL(seg_loss_grad_kernel, dim3((unsigned)((n + SL_THREADS - 1) / SL_THREADS)), dim3(SL_THREADS), 0, s,
                     preds, img_stride, chan_stride, mask, terms, coef, d_loss, d_preds, B, P);
}

// ---- backward of the train-mode similarity map --------------------------------------------------------------------
// The forward's interpolation weight of coarse index c at fine index y (exactly as upsample_softmax2_kernel forms
// them: i0 = (int)(scale * y), i1 = i0 + (i0 < g - 1), l1 = scale * y - i0, l0 = 1 - l1); both terms count when
// i0 == i1 == c.
AACLIP_DEV float up_weight(int y, int c, float scale, int g) {
  const float sy = scale * y;
  const int i0 = (int)sy;
  const int i1 = i0 + (i0 < g - 1 ? 1 : 0);
  const float l1 = sy - i0, l0 = 1.0f - l1;
  return (i0 == c ? l0 : 0.f) + (i1 == c ? l1 : 0.f);
}

// fine indices whose weight on coarse index c can be non-zero, with one index of margin on either side
AACLIP_DEV void up_support(int c, float scale, int S, int& lo, int& hi) {
  if (scale <= 0.f) {
    lo = 0;
    hi = S - 1;
    return;
  }
  lo = (int)floorf((float)(c - 1) / scale) - 1;
  hi = (int)ceilf((float)(c + 1) / scale) + 1;
  if (lo < 0) lo = 0;
  if (hi > S - 1) hi = S - 1;
}

// grid (S, B): fine row y of image b -> T[b, y, cx] = sum_x w(x, cx) dU[b, y, x], with dU = d(upsampled channel-0
// scores) = p0 p1 (dP0 - dP1) (softmax backward over the channel pair; the channel-1 gradient is its negative)
__global__ __launch_bounds__(256) void upsample_bwd_rows_kernel(const float* __restrict__ preds,
                                                                const float* __restrict__ d_preds,
                                                                float* __restrict__ T, int g, int S) {
  __shared__ float du[SIMMAP_BWD_MAX_S];
  const int y = blockIdx.x, b = blockIdx.y;
  const long SS = (long)S * S;
  const float* p0 = preds + (long)b * 2 * SS + (long)y * S;
  const float* d0 = d_preds + (long)b * 2 * SS + (long)y * S;
  for (int x = threadIdx.x; x < S; x += 256) {
    const float a = p0[x], c = p0[SS + x];
    du[x] = a * c * (d0[x] - d0[SS + x]);
  }
  __syncthreads();
  const float scale = S > 1 ? (float)(g - 1) / (float)(S - 1) : 0.f;
  for (int cx = threadIdx.x; cx < g; cx += 256) {
    int lo, hi;
    up_support(cx, scale, S, lo, hi);
    float acc = 0.f;
    for (int x = lo; x <= hi; ++x) acc = fmaf(up_weight(x, cx, scale, g), du[x], acc);
    T[((long)b * S + y) * g + cx] = acc;
  }
}

// grid (B): dS[b, cy * g + cx] = 100 * sum_y w(y, cy) T[b, y, cx]  (gradient of the channel-0 patch scores f.t0)
__global__ __launch_bounds__(256) void upsample_bwd_cols_kernel(const float* __restrict__ T, float* __restrict__ dS,
                                                                int g, int S) {
  const int b = blockIdx.x;
  const float scale = S > 1 ? (float)(g - 1) / (float)(S - 1) : 0.f;
  for (int p = threadIdx.x; p < g * g; p += 256) {
    const int cy = p / g, cx = p - cy * g;
    int lo, hi;
    up_support(cy, scale, S, lo, hi);
    float acc = 0.f;
    for (int y = lo; y <= hi; ++y) acc = fmaf(up_weight(y, cy, scale, g), T[((long)b * S + y) * g + cx], acc);
    dS[(long)b * g * g + p] = 100.0f * acc;
  }
}

// grid (E / 64, nb): nb = B (per-image anchors [B, E, 2]) or 1 (one anchor pair [E, 2] shared by all images: the
// images are summed in order).  Wave w sums patches [w * P / 4, (w + 1) * P / 4) for the 64 columns of its block.
__global__ __launch_bounds__(256) void anchor_grad_kernel(const float* __restrict__ seg, const float* __restrict__ dS,
                                                          float* __restrict__ d_anchors, int B, int P, int E,
                                                          int shared) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const int b_begin = shared ? 0 : blockIdx.y, b_end = shared ? B : blockIdx.y + 1;
  const int per = (P + 3) / 4;
  const int p_begin = w * per, p_end = p_begin + per < P ? p_begin + per : P;
  float acc = 0.f;
  for (int b = b_begin; b < b_end; ++b) {
    const float* f = seg + (long)b * P * E + e;
    const float* d = dS + (long)b * P;
    for (int p = p_begin; p < p_end; ++p) acc = fmaf(f[(long)p * E], d[p], acc);
  }
  red[w][lane] = acc;
  __syncthreads();
  if (w == 0) {
    const float v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    float* out = d_anchors + (shared ? 0 : (long)blockIdx.y * E * 2) + 2 * e;
    out[0] = v;
    out[1] = -v;
  }
}

// d seg [B, P, E] = dS (t0 - t1): the scores' gradients are dS and -dS
__global__ __launch_bounds__(256) void patch_grad_kernel(const float* __restrict__ dS, const float* __restrict__ anchors,
                                                         long anchor_bstride, float* __restrict__ d_seg, int P, int E,
                                                         long n) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const long row = idx / E;
  const int e = (int)(idx - row * E);
  const long b = row / P;
  const float* t = anchors + b * anchor_bstride + 2 * e;
  const float d = dS[row];
  d_seg[idx] = d * t[0] - d * t[1];
}

void launch_similarity_map_train_bwd(const float* seg, const float* anchors, long anchor_bstride, const float* preds,
                                     const float* d_preds, float* d_anchors, float* d_seg, int B, int g, int E, int S,
                                     void* ws, hipStream_t s) {
  const int P = g * g;
  float* T = (float*)ws;
  float* dS = T + simmap_bwd_t_floats(B, g, S);
  hipLaunchKernelGGL(upsample_bwd_rows_kernel, dim3(S, B), dim3(256), 0, s, preds, d_preds, T, g, S);
  hipLaunchKernelGGL(upsample_bwd_cols_kernel, dim3(B), dim3(256), 0, s, T, dS, g, S);
  if (d_anchors) {
    const int shared = anchor_bstride == 0 ? 1 : 0;
    hipLaunchKernelGGL(anchor_grad_kernel, dim3(E / 64, shared ? 1 : B), dim3(256), 0, s, seg, dS, d_anchors, B, P, E,
                       shared);
  }
  if (d_seg) {
    const long n = (long)B * P * E;
    hipLaunchKernelGGL(patch_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dS, anchors,
                       anchor_bstride, d_seg, P, E, n);
  }
}

}  // namespace aaclip

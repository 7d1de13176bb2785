// The IQM map term of the stage-2 loss (reference train.py:165-212), one tap level per call, forward and backward:
//   p = sigmoid(cos(f, q_abnormal) - cos(f, q_normal)) per patch (iqm_scores_kernel, iqm.hip), the channel pair
//   (1 - p, p) upsampled with half-pixel (align_corners=False) bilinear weights to [B, 2, S, S].
//   iqm_upsample2       grid [B, g, g] -> out [B, 2, S, S]; channel 1 with the arithmetic of iqm_upsample_kernel (one
//                       level, weight 1, no base), channel 0 the same expression on the values 1 - p
//   iqm_bwd_rows / _cols   dU = d_preds[:, 1] - d_preds[:, 0] -> transpose of the half-pixel upsample as a gather over
//                       each coarse cell's support window (separable: fine columns, then fine rows) -> sigmoid backward
//                       dz = p (1 - p) dgrid
//   iqm_bwd_patch       wave per patch row: d_seg and the per-row scalars of the query gradient
//   iqm_bwd_query_part / _final   d_queries: the sum over the patches in IQ_QCHUNKS chunks, reduced in chunk order
// The gradient is that of the function the forward computes, c = x.y / sqrt(max(|x|^2 |y|^2, 1e-16)): where the clamp
// is active the denominator is a constant, so only the x.y term is differentiated.
// Everything is fp32, without atomics and reduced in a fixed order: two calls on the same inputs give identical bits.
#include "common.h"
#include "kernels.h"

namespace aaclip {

constexpr int IQL_MAXG = 40;
constexpr int IQL_BAND = 8;   // fine rows per workgroup of the forward

// the forward's half-pixel source position and weights at fine index y, exactly as iqm_upsample_kernel forms them
AACLIP_DEV void hp_source(int y, float scale, int g, int& i0, int& i1, float& l0, float& l1) {
  float s = scale * ((float)y + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i1 = i0 + (i0 < g - 1 ? 1 : 0);
  l1 = s - i0;
  l0 = 1.0f - l1;
}

// weight of coarse index c at fine index y; both terms count when i0 == i1 == c (the last coarse index)
AACLIP_DEV float hp_weight(int y, int c, float scale, int g) {
  int i0, i1;
  float l0, l1;
  hp_source(y, scale, g, i0, i1, l0, l1);
  return (i0 == c ? l0 : 0.f) + (i1 == c ? l1 : 0.f);
}

// fine indices whose weight on coarse index c can be non-zero (source in (c - 1, c + 1)), with one index of margin on
// either side; coarse index 0 starts at fine index 0 (every source clamped to 0), the last one ends at S - 1
AACLIP_DEV void hp_support(int c, float scale, int S, int& lo, int& hi) {
  lo = (int)floorf(((float)c - 0.5f) / scale - 0.5f) - 1;
  hi = (int)ceilf(((float)c + 1.5f) / scale - 0.5f) + 1;
  if (lo < 0) lo = 0;
  if (hi > S - 1) hi = S - 1;
}

// grid (bands, B): fine rows [band * IQL_BAND, ...) of image b, both channels
__global__ __launch_bounds__(256) void iqm_upsample2_kernel(const float* __restrict__ grid, float* __restrict__ out, int g,
                                                            int S) {
  __shared__ float m1[IQL_MAXG * IQL_MAXG], m0[IQL_MAXG * IQL_MAXG];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < g * g; i += 256) {
    const float p = grid[(long)b * g * g + i];
    m1[i] = p;
    m0[i] = 1.0f - p;
  }
  __syncthreads();
  const float scale = (float)g / (float)S;
  const int y_begin = blockIdx.x * IQL_BAND;
  int y_end = y_begin + IQL_BAND;
  if (y_end > S) y_end = S;
  const long SS = (long)S * S;
  for (long i = (long)y_begin * S + tid; i < (long)y_end * S; i += 256) {
    const int y = i / S, x = i - (long)y * S;
    float sy = scale * ((float)y + 0.5f) - 0.5f, sx = scale * ((float)x + 0.5f) - 0.5f;
    sy = sy < 0.f ? 0.f : sy;
    sx = sx < 0.f ? 0.f : sx;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < g - 1 ? 1 : 0), x1 = x0 + (x0 < g - 1 ? 1 : 0);
    const float ly1 = sy - y0, ly0 = 1.0f - ly1, lx1 = sx - x0, lx0 = 1.0f - lx1;
    const float* p = m1;
    const float v1 = ly0 * (lx0 * p[y0 * g + x0] + lx1 * p[y0 * g + x1]) + ly1 * (lx0 * p[y1 * g + x0] + lx1 * p[y1 * g + x1]);
    p = m0;
    const float v0 = ly0 * (lx0 * p[y0 * g + x0] + lx1 * p[y0 * g + x1]) + ly1 * (lx0 * p[y1 * g + x0] + lx1 * p[y1 * g + x1]);
    out[(long)b * 2 * SS + i] = v0;
    out[(long)b * 2 * SS + SS + i] = 1.0f * v1;   // iqm_upsample_kernel's w_iqm * acc with w_iqm = 1
  }
}

void launch_iqm_map_train(const float* seg, const float* q, float* grid, float* out, int B, int g, int E, int S,
                          hipStream_t s) {
  launch_iqm_scores(seg, q, grid, B, g * g, E, s);
  hipLaunchKernelGGL(iqm_upsample2_kernel, dim3((S + IQL_BAND - 1) / IQL_BAND, B), dim3(256), 0, s, grid, out, g, S);
}

// grid (S, B): fine row y of image b -> T[b, y, cx] = sum_x w(x, cx) dU[b, y, x], dU = d_preds[:, 1] - d_preds[:, 0]
__global__ __launch_bounds__(256) void iqm_bwd_rows_kernel(const float* __restrict__ d_preds, float* __restrict__ T, int g,
                                                           int S) {
  __shared__ float du[SIMMAP_BWD_MAX_S];
  const int y = blockIdx.x, b = blockIdx.y;
  const long SS = (long)S * S;
  const float* d0 = d_preds + (long)b * 2 * SS + (long)y * S;
  for (int x = threadIdx.x; x < S; x += 256) du[x] = d0[SS + x] - d0[x];
  __syncthreads();
  const float scale = (float)g / (float)S;
  for (int cx = threadIdx.x; cx < g; cx += 256) {
    int lo, hi;
    hp_support(cx, scale, S, lo, hi);
    float acc = 0.f;
    for (int x = lo; x <= hi; ++x) acc = fmaf(hp_weight(x, cx, scale, g), du[x], acc);
    T[((long)b * S + y) * g + cx] = acc;
  }
}

// grid (g, B), one wave: coarse row cy of image b -> dz[b, cy * g + cx] = p (1 - p) sum_y w(y, cy) T[b, y, cx]
__global__ __launch_bounds__(64) void iqm_bwd_cols_kernel(const float* __restrict__ T, const float* __restrict__ grid,
                                                          float* __restrict__ dz, int g, int S) {
  const int cy = blockIdx.x, b = blockIdx.y, cx = threadIdx.x;
  if (cx >= g) return;
  const float scale = (float)g / (float)S;
  int lo, hi;
  hp_support(cy, scale, S, lo, hi);
  float acc = 0.f;
  for (int y = lo; y <= hi; ++y) acc = fmaf(hp_weight(y, cy, scale, g), T[((long)b * S + y) * g + cx], acc);
  const long o = (long)b * g * g + cy * g + cx;
  const float p = grid[o];
  dz[o] = p * (1.0f - p) * acc;
}

// Four rows per workgroup, one wave per patch row (the layout of iqm_scores_kernel, whose sums it recomputes):
//   d_seg[b, p, :] = dz [(q1 / (|f||q1|) - c1 f / |f|^2) - (q0 / (|f||q0|) - c0 f / |f|^2)]
// and sc[row * 4 ..] = {dz / den0, dz / den1, dz c0, dz c1} for the query gradient; den_k = sqrt(max(|f|^2 |q_k|^2,
// 1e-16)), and where that clamp is active the c_k terms are dropped (d_seg) or stored as 0 (sc).  d_seg may be null.
template <int NCH>
__global__ __launch_bounds__(256) void iqm_bwd_patch_kernel(const float* __restrict__ seg, const float* __restrict__ qv,
                                                            const float* __restrict__ dz, float* __restrict__ d_seg,
                                                            float* __restrict__ sc, int B, int P) {
  constexpr int E = NCH * 256;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * P) return;
  const long b = row / P;
  const float* f = seg + row * E;
  const float* q0 = qv + b * 2 * E;
  const float* q1 = q0 + E;
  f32x4 fv[NCH], a[NCH], bb[NCH];
  float ff = 0.f, d0 = 0.f, d1 = 0.f, n0 = 0.f, n1 = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int e0 = (c * 64 + lane) * 4;
    fv[c] = *(const f32x4*)(f + e0);
    a[c] = *(const f32x4*)(q0 + e0);
    bb[c] = *(const f32x4*)(q1 + e0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ff = fmaf(fv[c][j], fv[c][j], ff);
      d0 = fmaf(fv[c][j], a[c][j], d0); n0 = fmaf(a[c][j], a[c][j], n0);
      d1 = fmaf(fv[c][j], bb[c][j], d1); n1 = fmaf(bb[c][j], bb[c][j], n1);
    }
  }
  ff = wave_sum(ff); d0 = wave_sum(d0); d1 = wave_sum(d1); n0 = wave_sum(n0); n1 = wave_sum(n1);   // the same in every lane
  const float s0 = ff * n0, s1 = ff * n1;
  const float inv0 = 1.0f / sqrtf(fmaxf(s0, 1e-16f)), inv1 = 1.0f / sqrtf(fmaxf(s1, 1e-16f));
  const float c0 = s0 > 1e-16f ? d0 * inv0 : 0.f, c1 = s1 > 1e-16f ? d1 * inv1 : 0.f;   // 0: the clamp is active
  const float gz = dz[row];
  if (d_seg) {
    const float a0 = s0 > 1e-16f ? c0 / ff : 0.f, a1 = s1 > 1e-16f ? c1 / ff : 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = gz * ((bb[c][j] * inv1 - a1 * fv[c][j]) - (a[c][j] * inv0 - a0 * fv[c][j]));
      *(f32x4*)(d_seg + row * E + (c * 64 + lane) * 4) = o;
    }
  }
  if (lane == 0) {
    float* o = sc + row * 4;
    o[0] = gz * inv0;
    o[1] = gz * inv1;
    o[2] = gz * c0;
    o[3] = gz * c1;
  }
}

// grid (E / 256, IQ_QCHUNKS, B): chunk c of image b's patches, 256 columns; wave w sums rows begin + w, begin + w + 4,
// ... for four columns per lane, the four waves are added in wave order:
//   part[((b * IQ_QCHUNKS + c) * 2 + k) * E + e] = sum_p sc[p][k] f[p][e];  column block 0 also sums sc[p][2 + k] into
//   tpart[(b * IQ_QCHUNKS + c) * 2 + k].  A chunk past the last patch writes zeros.
__global__ __launch_bounds__(256) void iqm_bwd_query_part_kernel(const float* __restrict__ seg, const float* __restrict__ sc,
                                                                 float* __restrict__ part, float* __restrict__ tpart,
                                                                 int P, int E) {
  __shared__ f32x4 red[2][4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.y, b = blockIdx.z;
  const int per = (P + IQ_QCHUNKS - 1) / IQ_QCHUNKS;
  const int begin = c * per < P ? c * per : P, end = begin + per < P ? begin + per : P;
  const int e0 = blockIdx.x * 256 + lane * 4;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int p = begin + w; p < end; p += 4) {
    const long row = (long)b * P + p;
    const f32x4 fv = *(const f32x4*)(seg + row * E + e0);
    const float u0 = sc[row * 4], u1 = sc[row * 4 + 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc0[j] = fmaf(u0, fv[j], acc0[j]);
      acc1[j] = fmaf(u1, fv[j], acc1[j]);
    }
  }
  red[0][w][lane] = acc0;
  red[1][w][lane] = acc1;
  __syncthreads();
  if (w < 2) {
    const f32x4 v = ((red[w][0][lane] + red[w][1][lane]) + red[w][2][lane]) + red[w][3][lane];
    *(f32x4*)(part + (((long)b * IQ_QCHUNKS + c) * 2 + w) * E + e0) = v;
  }
  if (blockIdx.x == 0 && threadIdx.x >= 128 && threadIdx.x < 130) {
    const int k = threadIdx.x - 128;
    float t = 0.f;
    for (int p = begin; p < end; ++p) t += sc[((long)b * P + p) * 4 + 2 + k];
    tpart[((long)b * IQ_QCHUNKS + c) * 2 + k] = t;
  }
}

// grid (E / 256, 2, B): d_queries[b, k, e] = sign_k (A_k[e] - T_k q_k[e] / |q_k|^2), A and T summed over the chunks in
// chunk order; sign + for the abnormal query (k = 1), - for the normal one
__global__ __launch_bounds__(256) void iqm_bwd_query_final_kernel(const float* __restrict__ qv, const float* __restrict__ part,
                                                                  const float* __restrict__ tpart, float* __restrict__ d_q,
                                                                  int E) {
  __shared__ float red[4];
  const int k = blockIdx.y, b = blockIdx.z;
  const float* q = qv + ((long)b * 2 + k) * E;
  float n = 0.f;
  for (int e = threadIdx.x; e < E; e += 256) n = fmaf(q[e], q[e], n);
  n = wave_sum(n);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  n = ((red[0] + red[1]) + red[2]) + red[3];
  const int e = blockIdx.x * 256 + threadIdx.x;
  float A = 0.f, T = 0.f;
  for (int c = 0; c < IQ_QCHUNKS; ++c) {
    A += part[(((long)b * IQ_QCHUNKS + c) * 2 + k) * E + e];
    T += tpart[((long)b * IQ_QCHUNKS + c) * 2 + k];
  }
  const float v = A - (n > 0.f ? T * q[e] / n : 0.f);
  d_q[((long)b * 2 + k) * E + e] = k == 1 ? v : -v;
}

void launch_iqm_map_train_bwd(const float* seg, const float* q, const float* grid, const float* d_preds, float* d_seg,
                              float* d_q, int B, int g, int E, int S, void* ws, hipStream_t s) {
  const int P = g * g;
  float* part = (float*)ws;   // first: it is written as 16-byte vectors
  float* T = part + (size_t)B * IQ_QCHUNKS * 2 * E;
  float* dz = T + (size_t)B * S * g;
  float* sc = dz + (size_t)B * P;
  float* tpart = sc + (size_t)B * P * 4;
  hipLaunchKernelGGL(iqm_bwd_rows_kernel, dim3(S, B), dim3(256), 0, s, d_preds, T, g, S);
  hipLaunchKernelGGL(iqm_bwd_cols_kernel, dim3(g, B), dim3(64), 0, s, T, grid, dz, g, S);
  dim3 rows((unsigned)(((long)B * P + 3) / 4));
  switch (E / 256) {
    case 1: hipLaunchKernelGGL(iqm_bwd_patch_kernel<1>, rows, dim3(256), 0, s, seg, q, dz, d_seg, sc, B, P); break;
    case 2: hipLaunchKernelGGL(iqm_bwd_patch_kernel<2>, rows, dim3(256), 0, s, seg, q, dz, d_seg, sc, B, P); break;
    case 3: hipLaunchKernelGGL(iqm_bwd_patch_kernel<3>, rows, dim3(256), 0, s, seg, q, dz, d_seg, sc, B, P); break;
    case 4: hipLaunchKernelGGL(iqm_bwd_patch_kernel<4>, rows, dim3(256), 0, s, seg, q, dz, d_seg, sc, B, P); break;
  }
  if (d_q) {
    hipLaunchKernelGGL(iqm_bwd_query_part_kernel, dim3(E / 256, IQ_QCHUNKS, B), dim3(256), 0, s, seg, sc, part, tpart, P, E);
    hipLaunchKernelGGL(iqm_bwd_query_final_kernel, dim3(E / 256, 2, B), dim3(256), 0, s, q, part, tpart, d_q, E);
  }
}

}  // namespace aaclip

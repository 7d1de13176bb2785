// Backward building blocks of the IQM branch's 2-row query side (class_query_mlp, IQM.layernorm and per layer the 2 x 2
// self-attention, the query-side products of the two cross-attentions, the 0.4 / 0.3 / 0.3 fusion, the GELU
// feed-forward and iqm_layer_norm: model/iqm.py, model/adapter.py _iqm_branch).  The rows are 2 B, or 2 B H in the
// head-expanded form: every kernel here is latency-bound, wave per row or thread per column, fp32, and the matrix
// products stay on aaclip_gemm / aaclip_gemm_wgrad.
//   small_attention_bwd   backward of small_attention_kernel (iqm.hip) for fp32 k / v and at most 256 keys: one
//                         workgroup per (head, image), thread j owns key j; the probabilities are recomputed
//                           s_aj = scale q_a . k_j, p_a = softmax_j s_a, g_aj = d_out_a . v_j, delta_a = sum_j p_aj g_aj
//                           ds_aj = p_aj (g_aj - delta_a)
//                           d_v_j = sum_a p_aj d_out_a,  d_k_j = scale sum_a ds_aj q_a,  d_q_a = scale sum_j ds_aj k_j
//   ln_stats / ln_param   d_w[c] = sum_r d_y[r, c] xhat[r, c], d_b[c] = sum_r d_y[r, c]: mean and rstd per row (wave per
//                         row, the arithmetic of residual_layernorm_kernel), then thread per column over a chunk of rows
//   bias_grad             db[n] = sum_r dz[r, n], thread per column over a chunk of rows
//   act_bwd               d_z = d_y GELU'(z) from the pre-activation, or d_y [y > 0] from the ReLU's output
//   smallk_bwd            dW[n, k] = sum_r d_y[r, n] x[r, k] (k < K <= 4) and db[n], thread per column over a chunk of rows
//   chunk_combine         the chunks' partial sums added in chunk order
// No atomics: every output element is written by one thread and every sum runs in a fixed order, so two calls on the
// same inputs give the same bits.
#include "common.h"
#include "kernels.h"

namespace aaclip {

namespace {

constexpr int SAB_MAXQ = 4, SAB_MAXHD = 128;   // SAB_MAXK keys (kernels.h): one key per thread

// a value per thread -> red[a][tid]; thread a < nq folds the 256 values in index order with `op`
template <typename F>
AACLIP_DEV void sab_fold(float (&val)[SAB_MAXQ], float (*red)[256], float* res, int nq, int tid, F op) {
  __syncthreads();
#pragma unroll
  for (int a = 0; a < SAB_MAXQ; ++a) red[a][tid] = val[a];
  __syncthreads();
  if (tid < nq) {
    float t = red[tid][0];
    for (int i = 1; i < 256; ++i) t = op(t, red[tid][i]);
    res[tid] = t;
  }
  __syncthreads();
}

}  // namespace

// grid (H, B), 256 threads; Lk <= 256, nq <= 4, hd % 4 == 0, hd <= 128.  d_q / d_k / d_v may be null.
__global__ __launch_bounds__(256) void small_attention_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ v,
                                                                  const float* __restrict__ dout, float* __restrict__ d_q,
                                                                  float* __restrict__ d_k, float* __restrict__ d_v, int nq,
                                                                  int Lk, int H, int hd, float scale) {
  __shared__ float qs[SAB_MAXQ][SAB_MAXHD];    // q * scale, as the forward forms it
  __shared__ float dos[SAB_MAXQ][SAB_MAXHD];
  __shared__ float ps[SAB_MAXQ][SAB_MAXK];
  __shared__ float dss[SAB_MAXQ][SAB_MAXK];
  __shared__ float red[SAB_MAXQ][256];
  __shared__ float stat[3][SAB_MAXQ];          // max, 1 / sum, delta
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int D = H * hd;
  for (int i = tid; i < nq * hd; i += 256) {
    const long o = ((long)b * nq + i / hd) * D + h * hd + i % hd;
    qs[i / hd][i % hd] = q[o] * scale;
    dos[i / hd][i % hd] = dout[o];
  }
  __syncthreads();
  const bool alive = tid < Lk;
  const long krow = ((long)b * Lk + (alive ? tid : 0)) * D + h * hd;
  float s[SAB_MAXQ] = {0.f, 0.f, 0.f, 0.f}, g[SAB_MAXQ] = {0.f, 0.f, 0.f, 0.f};
  if (alive) {
    for (int d = 0; d < hd; d += 4) {
      const f32x4 kv = *(const f32x4*)(k + krow + d);
      const f32x4 vv = *(const f32x4*)(v + krow + d);
#pragma unroll
      for (int a = 0; a < SAB_MAXQ; ++a)
        if (a < nq) {
          s[a] = fmaf(kv[3], qs[a][d + 3], fmaf(kv[2], qs[a][d + 2], fmaf(kv[1], qs[a][d + 1], fmaf(kv[0], qs[a][d], s[a]))));
          g[a] = fmaf(vv[3], dos[a][d + 3], fmaf(vv[2], dos[a][d + 2], fmaf(vv[1], dos[a][d + 1], fmaf(vv[0], dos[a][d], g[a]))));
        }
    }
  }
  float t[SAB_MAXQ];
#pragma unroll
  for (int a = 0; a < SAB_MAXQ; ++a) t[a] = alive ? s[a] : -INFINITY;
  sab_fold(t, red, stat[0], nq, tid, [](float x, float y) { return fmaxf(x, y); });
  float e[SAB_MAXQ];
#pragma unroll
  for (int a = 0; a < SAB_MAXQ; ++a) e[a] = (alive && a < nq) ? expf(s[a] - stat[0][a]) : 0.f;
  sab_fold(e, red, stat[1], nq, tid, [](float x, float y) { return x + y; });
  float p[SAB_MAXQ];
#pragma unroll
  for (int a = 0; a < SAB_MAXQ; ++a) {
    p[a] = a < nq ? e[a] * (1.0f / stat[1][a]) : 0.f;
    t[a] = p[a] * g[a];
  }
  sab_fold(t, red, stat[2], nq, tid, [](float x, float y) { return x + y; });
  if (alive) {
#pragma unroll
    for (int a = 0; a < SAB_MAXQ; ++a)
      if (a < nq) {
        ps[a][tid] = p[a];
        dss[a][tid] = p[a] * (g[a] - stat[2][a]);
      }
  }
  __syncthreads();
  // d_k, d_v: element (j, c) of the head's [Lk, hd] slice per thread and step
  if (d_k || d_v) {
    for (int i = tid; i < Lk * hd; i += 256) {
      const int j = i / hd, c = i - j * hd;
      float ak = 0.f, av = 0.f;
#pragma unroll
      for (int a = 0; a < SAB_MAXQ; ++a)
        if (a < nq) {
          ak = fmaf(dss[a][j], qs[a][c], ak);
          av = fmaf(ps[a][j], dos[a][c], av);
        }
      const long o = ((long)b * Lk + j) * D + h * hd + c;
      if (d_k) d_k[o] = ak;
      if (d_v) d_v[o] = av;
    }
  }
  // d_q: element (a, c) per thread and step, the keys in index order
  if (d_q) {
    for (int i = tid; i < nq * hd; i += 256) {
      const int a = i / hd, c = i - a * hd;
      const float* kc = k + (long)b * Lk * D + h * hd + c;
      float acc = 0.f;
      for (int j = 0; j < Lk; ++j) acc = fmaf(dss[a][j], kc[(long)j * D], acc);
      d_q[((long)b * nq + a) * D + h * hd + c] = acc * scale;
    }
  }
}

void launch_small_attention_backward(const float* q, const float* k, const float* v, const float* dout, float* d_q,
                                     float* d_k, float* d_v, int B, int nq, int Lk, int H, int hd, float scale,
                                     hipStream_t s) {
  hipLaunchKernelGGL(small_attention_bwd_kernel, dim3(H, B), dim3(256), 0, s, q, k, v, dout, d_q, d_k, d_v, nq, Lk, H, hd,
                     scale);
}

// ------------------------------------------------------------------------------------------------ row chunks
// rows are cut into at most IQB_MAX_CHUNKS chunks of `per` rows; a workgroup row of the grid owns a chunk
int iqb_chunks(long rows) {
  const long c = (rows + IQB_CHUNK_ROWS - 1) / IQB_CHUNK_ROWS;
  return c > IQB_MAX_CHUNKS ? IQB_MAX_CHUNKS : (int)c;
}
static long iqb_per(long rows) {
  const int c = iqb_chunks(rows);
  return (rows + c - 1) / c;
}

// out0[i] (i < n0) = sum_c part[c * stride + i], out1[i] (i < n1) = sum_c part[c * stride + n0 + i]; either may be null
__global__ __launch_bounds__(256) void chunk_combine_kernel(const float* __restrict__ part, int chunks, long stride,
                                                            float* __restrict__ out0, long n0, float* __restrict__ out1,
                                                            long n1) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n0 + n1) return;
  float* dst = i < n0 ? (out0 ? out0 + i : nullptr) : (out1 ? out1 + (i - n0) : nullptr);
  if (!dst) return;
  float t = 0.f;
  for (int c = 0; c < chunks; ++c) t += part[c * stride + i];
  *dst = t;
}
static void launch_chunk_combine(const float* part, int chunks, long stride, float* out0, long n0, float* out1, long n1,
                                 hipStream_t s) {
  hipLaunchKernelGGL(chunk_combine_kernel, dim3((unsigned)((n0 + n1 + 255) / 256)), dim3(256), 0, s, part, chunks, stride,
                     out0, n0, out1, n1);
}

// ------------------------------------------------------------------------------------------------ layernorm_param_grad
// stats[r] = (mean, rstd) of row r: one wave per row, the sums of residual_layernorm_kernel
__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ x, float* __restrict__ stats, long rows,
                                                       int D, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* px = x + row * D;
  float sum = 0.f;
  for (int i = lane; i < D; i += 64) sum += px[i];
  const float mean = wave_sum(sum) / (float)D;
  float var = 0.f;
  for (int i = lane; i < D; i += 64) { const float c = px[i] - mean; var = fmaf(c, c, var); }
  const float rstd = rsqrtf(wave_sum(var) / (float)D + eps);
  if (lane == 0) {
    stats[row * 2] = mean;
    stats[row * 2 + 1] = rstd;
  }
}
// grid (ceil(D / 256), chunks): part[chunk][0:D] = the chunk's share of d_w, part[chunk][D:2D] = of d_b
__global__ __launch_bounds__(256) void ln_param_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                       const float* __restrict__ stats, float* __restrict__ part, long rows,
                                                       int D, long per) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  const long r0 = (long)blockIdx.y * per, r1 = min(rows, r0 + per);
  float aw = 0.f, ab = 0.f;
  for (long r = r0; r < r1; ++r) {
    const float g = dy[r * D + c];
    aw = fmaf(g, (x[r * D + c] - stats[r * 2]) * stats[r * 2 + 1], aw);
    ab += g;
  }
  float* o = part + (long)blockIdx.y * 2 * D;
  o[c] = aw;
  o[D + c] = ab;
}

static size_t ln_param_stats_floats(long rows) { return ((size_t)rows * 2 + 63) & ~(size_t)63; }
size_t layernorm_param_grad_ws_bytes(long rows, int D) {
  if (rows <= 0 || D <= 0) return 0;
  return (ln_param_stats_floats(rows) + (size_t)iqb_chunks(rows) * 2 * D) * 4;
}
void launch_layernorm_param_grad(const float* x, const float* dy, float* d_w, float* d_b, long rows, int D, float eps,
                                 void* ws, hipStream_t s) {
  float* stats = (float*)ws;
  float* part = stats + ln_param_stats_floats(rows);
  const int chunks = iqb_chunks(rows);
  hipLaunchKernelGGL(ln_stats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, stats, rows, D, eps);
  hipLaunchKernelGGL(ln_param_kernel, dim3((D + 255) / 256, chunks), dim3(256), 0, s, x, dy, stats, part, rows, D,
                     iqb_per(rows));
  launch_chunk_combine(part, chunks, 2L * D, d_w, D, d_b, D, s);
}

// ------------------------------------------------------------------------------------------------ bias_grad
// grid (ceil(N / 256), chunks): part[chunk][n] = sum over the chunk's rows of dz[r, n]
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ dz, long ldz, float* __restrict__ part,
                                                        long rows, int N, long per) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const long r0 = (long)blockIdx.y * per, r1 = min(rows, r0 + per);
  float t = 0.f;
  for (long r = r0; r < r1; ++r) t += dz[r * ldz + n];
  part[(long)blockIdx.y * N + n] = t;
}
size_t bias_grad_ws_bytes(long rows, int N) {
  if (rows <= 0 || N <= 0) return 0;
  return (size_t)iqb_chunks(rows) * N * 4;
}
void launch_bias_grad(const float* dz, long ldz, float* db, long rows, int N, void* ws, hipStream_t s) {
  const int chunks = iqb_chunks(rows);
  hipLaunchKernelGGL(bias_grad_kernel, dim3((N + 255) / 256, chunks), dim3(256), 0, s, dz, ldz, (float*)ws, rows, N,
                     iqb_per(rows));
  launch_chunk_combine((const float*)ws, chunks, N, db, N, nullptr, 0, s);
}

// ------------------------------------------------------------------------------------------------ act_backward
// GELU (erf form): zy is the pre-activation z, d_z = d_y (Phi(z) + z phi(z)).  ReLU: zy is the activation's OUTPUT,
// d_z = d_y for zy > 0 and 0 otherwise (the kink takes the negative side's slope, like aaclip_adapter_mix_backward).
// d_z may alias d_y: an element is read and written by the same thread.
template <int ACT>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* zy, const float* dy, float* dz, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float x = zy[i], g = dy[i];
    if (ACT == AACLIP_ACT_GELU) {
      const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
      const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
      dz[i] = g * (cdf + x * pdf);
    } else {
      dz[i] = x > 0.f ? g : 0.f;
    }
  }
}
void launch_iqm_act_backward(int act, const float* zy, const float* dy, float* dz, long n, hipStream_t s) {
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (act == AACLIP_ACT_GELU)
    hipLaunchKernelGGL(act_bwd_kernel<AACLIP_ACT_GELU>, dim3((unsigned)blocks), dim3(256), 0, s, zy, dy, dz, n);
  else
    hipLaunchKernelGGL(act_bwd_kernel<AACLIP_ACT_RELU>, dim3((unsigned)blocks), dim3(256), 0, s, zy, dy, dz, n);
}

// ------------------------------------------------------------------------------------------------ linear_smallk_backward
// grid (ceil(N / 256), chunks): part[chunk][n * K + k] = the chunk's share of dW[n, k], part[chunk][N * K + n] = of db[n]
template <int K>
__global__ __launch_bounds__(256) void smallk_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ part, long R, int N, long per) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const long r0 = (long)blockIdx.y * per, r1 = min(R, r0 + per);
  float aw[K], ab = 0.f;
#pragma unroll
  for (int kk = 0; kk < K; ++kk) aw[kk] = 0.f;
  for (long r = r0; r < r1; ++r) {
    const float g = dy[r * N + n];
#pragma unroll
    for (int kk = 0; kk < K; ++kk) aw[kk] = fmaf(g, x[r * K + kk], aw[kk]);
    ab += g;
  }
  float* o = part + (long)blockIdx.y * N * (K + 1);
#pragma unroll
  for (int kk = 0; kk < K; ++kk) o[(long)n * K + kk] = aw[kk];
  o[(long)N * K + n] = ab;
}
size_t linear_smallk_backward_ws_bytes(long R, int N, int K) {
  if (R <= 0 || N <= 0 || K <= 0) return 0;
  return (size_t)iqb_chunks(R) * N * (K + 1) * 4;
}
void launch_linear_smallk_backward(const float* x, const float* dy, float* d_w, float* d_b, long R, int N, int K, void* ws,
                                   hipStream_t s) {
  const int chunks = iqb_chunks(R);
  const long per = iqb_per(R);
  float* part = (float*)ws;
  const dim3 g((N + 255) / 256, chunks), blk(256);
  switch (K) {
    case 1: hipLaunchKernelGGL(smallk_bwd_kernel<1>, g, blk, 0, s, x, dy, part, R, N, per); break;
    case 2: hipLaunchKernelGGL(smallk_bwd_kernel<2>, g, blk, 0, s, x, dy, part, R, N, per); break;
    case 3: hipLaunchKernelGGL(smallk_bwd_kernel<3>, g, blk, 0, s, x, dy, part, R, N, per); break;
    case 4: hipLaunchKernelGGL(smallk_bwd_kernel<4>, g, blk, 0, s, x, dy, part, R, N, per); break;
    default: set_launch_error("linear_smallk_backward: no kernel for this K"); return;
  }
  launch_chunk_combine(part, chunks, (long)N * (K + 1), d_w, (long)N * K, d_b, N, s);
}

}  // namespace aaclip

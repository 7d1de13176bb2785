// Backward kernels of the adapted text tower (stage 1 of the reference's training, train.py:38-114): everything between
// the gradient of the sentence embeddings and the gradients of the text_adapter weights.  fp32 throughout (the reference
// trains in fp32).  No float atomics anywhere: every reduction runs in a fixed order, so two backward passes over the
// same data are bit-identical.
//   wgrad_kernel / wgrad_reduce_kernel   dW[o, i] = sum_r dZ[r, o] U[r, i] on v_mfma_f32_32x32x2_f32, split over row
//                                        chunks, the chunks added in order by a second pass
//   attn_bwd_kernel                      dq, dk, dv of softmax(q k^T) v per (sequence, head), head dim 64, L <= 128;
//                                        probabilities are recomputed in LDS, never stored in HBM
//   ln_bwd_kernel                        LayerNorm input gradient (gamma, beta frozen), wave per row
//   adapter_mix_bwd_kernel               backward of y = w a |u| / |a| + (1 - w) u, a = LeakyReLU(z), wave per row
//   gelu / gelu_bwd / act_bwd / gather   element-wise helpers of the block and row-head backward
//   head_norm_bwd_kernel                 backward of activation + F.normalize (+ patch mean) of the tap / det head, wave
//                                        per row
#include "common.h"
#include "kernels.h"

namespace aaclip {

// ------------------------------------------------------------------------------------------------ weight gradient
// One workgroup: a 128 x 128 tile of dW for one row chunk.  Both operands are already "k-major" (the reduction index
// r is the row index of dZ and of U), so a K-step of 16 rows is staged into LDS as it lies in memory; rows past the
// chunk's end are zero-filled.  A wave owns 64 x 64 (2 x 2 MFMA tiles), like gemm32_kernel.
__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ dz, long ldz, const float* __restrict__ u,
                                                    long ldu, float* __restrict__ out, long rows, int rows_per_chunk,
                                                    int O, int I) {
  constexpr int LD = 132;
  __shared__ __attribute__((aligned(16))) float As[16 * LD];
  __shared__ __attribute__((aligned(16))) float Bs[16 * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int tiles_i = I / 128;
  const int to = blockIdx.x / tiles_i, ti = blockIdx.x - to * tiles_i;
  const long r0 = (long)blockIdx.y * rows_per_chunk;
  const long r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  int sk[2], sc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = tid + 256 * j;
    sk[j] = f >> 5;
    sc[j] = (f & 31) * 4;
  }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long k0 = r0; k0 < r1; k0 += 16) {
    f32x4 ra[2], rb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long row = k0 + sk[j];
      const bool ok = row < r1;
      ra[j] = ok ? *(const f32x4*)(dz + row * ldz + to * 128 + sc[j]) : zero;
      rb[j] = ok ? *(const f32x4*)(u + row * ldu + ti * 128 + sc[j]) : zero;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *(f32x4*)(As + sk[j] * LD + sc[j]) = ra[j];
      *(f32x4*)(Bs + sk[j] * LD + sc[j]) = rb[j];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int k = 2 * ks + h;
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = As[k * LD + wr * 64 + 32 * i + r];
        b[i] = Bs[k * LD + wc * 64 + 32 * i + r];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  float* o = out + (size_t)blockIdx.y * O * I;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = to * 128 + wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
#pragma unroll
      for (int j = 0; j < 2; ++j) o[(size_t)row * I + ti * 128 + wc * 64 + j * 32 + r] = acc[i][j][e];
    }
}

// dW = part[0] + part[1] + ... in that order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                           long n4, int chunks) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 s = *(const f32x4*)(part + i * 4);
  for (int c = 1; c < chunks; ++c) s += *(const f32x4*)(part + ((size_t)c * n4 + i) * 4);
  *(f32x4*)(dw + i * 4) = s;
}

void wgrad_chunking(long rows, int* rows_per_chunk, int* chunks) {
  long nc = (rows + 127) / 128;
  if (nc < 1) nc = 1;
  if (nc > WGRAD_MAX_CHUNKS) nc = WGRAD_MAX_CHUNKS;
  long rpc = ((rows + nc - 1) / nc + 15) / 16 * 16;
  if (rpc < 16) rpc = 16;
  *rows_per_chunk = (int)rpc;
  *chunks = (int)((rows + rpc - 1) / rpc);
}

size_t wgrad_ws_bytes(long rows, int O, int I) {
  int rpc, nc;
  wgrad_chunking(rows, &rpc, &nc);
  return nc > 1 ? (size_t)nc * O * I * 4 : 0;
}

void launch_wgrad(const float* dz, long ldz, const float* u, long ldu, float* dw, long rows, int O, int I, void* ws,
                  hipStream_t s) {
  int rpc, nc;
  wgrad_chunking(rows, &rpc, &nc);
  float* part = nc > 1 ? (float*)ws : dw;
  hipLaunchKernelGGL(wgrad_kernel, dim3((O / 128) * (I / 128), nc), dim3(256), 0, s, dz, ldz, u, ldu, part, rows, rpc,
                     O, I);
  if (nc > 1) {
    const long n4 = (long)O * I / 4;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, part, dw, n4, nc);
  }
}

// ------------------------------------------------------------------------------------------------ attention backward
// One workgroup of 4 waves per (sequence, head).  Forward: s_ij = q_i . k_j (q pre-scaled), p = softmax_j, ctx_i = sum_j
// p_ij v_j.  Backward, with dp_ij = dctx_i . v_j and delta_i = sum_j p_ij dp_ij:  ds_ij = p_ij (dp_ij - delta_i),
//   dq_i = sum_j ds_ij k_j,   dk_j = sum_i ds_ij q_i,   dv_j = sum_i p_ij dctx_i.
// Phase A (K, V in LDS; a wave per query row): lanes over the keys form s, dp, the row's softmax statistics and ds; the ds
// row goes through a per-wave LDS row, then lanes over the 64 head dims form dq_i.  Phase B (Q, dctx in LDS; a wave per
// key row): lanes over the queries re-form p and ds from the saved (max, 1 / sum, delta) of each query row -- the same
// fmaf chain as in phase A, so the same bits -- and lanes over the head dims form dk_j and dv_j.  Every sum runs over an
// index in ascending order inside one wave: deterministic.
// LDS (floats): 2 x L x 65 tiles (row stride 65: lanes over rows hit 64 different banks), 3 L statistics, per wave two
// 64-float operand rows and two 128-float p / ds rows.
constexpr int ATTN_BWD_LD = 65;
inline size_t attn_bwd_lds_bytes(int L) { return ((size_t)2 * L * ATTN_BWD_LD + 3 * L + 4 * (2 * 64 + 2 * 128)) * 4; }

AACLIP_DEV void attn_bwd_stage(float* dst, const float* __restrict__ src, long ld, int L, int tid) {
  for (int idx = tid; idx < L * 16; idx += 256) {
    const int row = idx >> 4, c = (idx & 15) * 4;
    const f32x4 v = *(const f32x4*)(src + (long)row * ld + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[row * ATTN_BWD_LD + c + e] = v[e];
  }
}

__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                       float* __restrict__ dqkv, int L, int H, int causal,
                                                       float dq_scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, hd = blockIdx.x;
  const int D = 64 * H;
  const long ld3 = 3L * D;
  float* T0 = sm;                          // K, then Q
  float* T1 = T0 + L * ATTN_BWD_LD;        // V, then dctx
  float* st_m = T1 + L * ATTN_BWD_LD;      // per query row: max, 1 / sum, delta
  float* st_l = st_m + L;
  float* st_d = st_l + L;
  float* rowA = st_d + L + wave * 64;      // per wave: q_i (phase A) / k_j (phase B)
  float* rowB = st_d + L + 4 * 64 + wave * 64;
  float* pbuf = st_d + L + 8 * 64 + wave * 128;
  float* dsbuf = st_d + L + 8 * 64 + 4 * 128 + wave * 128;
  const float* q_g = qkv + (long)b * L * ld3 + hd * 64;
  const float* k_g = q_g + D;
  const float* v_g = q_g + 2 * D;
  const float* do_g = dctx + (long)b * L * D + hd * 64;
  float* dq_g = dqkv + (long)b * L * ld3 + hd * 64;

  attn_bwd_stage(T0, k_g, ld3, L, tid);
  attn_bwd_stage(T1, v_g, ld3, L, tid);
  __syncthreads();
  // ---- phase A
  for (int i = wave; i < L; i += 4) {
    rowA[lane] = q_g[(long)i * ld3 + lane];
    rowB[lane] = do_g[(long)i * D + lane];
    __builtin_amdgcn_wave_barrier();
    const int jmax = causal ? i + 1 : L;
    float s[2], dp[2];
    bool ok[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = lane + 64 * jj;
      ok[jj] = j < jmax;
      const int jr = ok[jj] ? j : 0;
      float a0 = 0.f, a1 = 0.f;
      for (int d = 0; d < 64; ++d) {
        a0 = fmaf(rowA[d], T0[jr * ATTN_BWD_LD + d], a0);
        a1 = fmaf(rowB[d], T1[jr * ATTN_BWD_LD + d], a1);
      }
      s[jj] = a0;
      dp[jj] = a1;
    }
    const float m = wave_max(fmaxf(ok[0] ? s[0] : -INFINITY, ok[1] ? s[1] : -INFINITY));
    float e[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) e[jj] = ok[jj] ? expf(s[jj] - m) : 0.f;
    const float linv = 1.0f / wave_sum(e[0] + e[1]);
    const float p0 = e[0] * linv, p1 = e[1] * linv;
    const float delta = wave_sum(p0 * dp[0] + p1 * dp[1]);
    if (lane == 0) {
      st_m[i] = m;
      st_l[i] = linv;
      st_d[i] = delta;
    }
    dsbuf[lane] = p0 * (dp[0] - delta);
    dsbuf[lane + 64] = p1 * (dp[1] - delta);
    __builtin_amdgcn_wave_barrier();
    float acc = 0.f;
    for (int j = 0; j < jmax; ++j) acc = fmaf(dsbuf[j], T0[j * ATTN_BWD_LD + lane], acc);
    dq_g[(long)i * ld3 + lane] = acc * dq_scale;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  attn_bwd_stage(T0, q_g, ld3, L, tid);
  attn_bwd_stage(T1, do_g, D, L, tid);
  __syncthreads();
  // ---- phase B
  for (int j = wave; j < L; j += 4) {
    rowA[lane] = k_g[(long)j * ld3 + lane];
    rowB[lane] = v_g[(long)j * ld3 + lane];
    __builtin_amdgcn_wave_barrier();
    const int imin = causal ? j : 0;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const int i = lane + 64 * ii;
      const bool ok = i >= imin && i < L;
      const int ir = ok ? i : 0;
      float a0 = 0.f, a1 = 0.f;
      for (int d = 0; d < 64; ++d) {
        a0 = fmaf(T0[ir * ATTN_BWD_LD + d], rowA[d], a0);
        a1 = fmaf(T1[ir * ATTN_BWD_LD + d], rowB[d], a1);
      }
      const float p = ok ? expf(a0 - st_m[ir]) * st_l[ir] : 0.f;
      pbuf[i] = p;
      dsbuf[i] = ok ? p * (a1 - st_d[ir]) : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    float dk = 0.f, dv = 0.f;
    for (int i = imin; i < L; ++i) {
      dk = fmaf(dsbuf[i], T0[i * ATTN_BWD_LD + lane], dk);
      dv = fmaf(pbuf[i], T1[i * ATTN_BWD_LD + lane], dv);
    }
    dq_g[(long)j * ld3 + D + lane] = dk;
    dq_g[(long)j * ld3 + 2 * D + lane] = dv;
    __builtin_amdgcn_wave_barrier();
  }
}

const char* attention_backward_check(int B, int L, int H) {
  if (B <= 0 || L <= 0 || H <= 0) return "attention_backward: empty problem";
  if (L > ATTN_BWD_MAX_L) return "attention_backward: sequences of at most 128 tokens";
  if (B > 65535 || H > 65535) return "attention_backward: grid limit";
  if ((long)B * L * 3 * 64 * H >= (1L << 40)) return "attention_backward: problem too large";
  return nullptr;
}

void launch_attention_backward(const float* qkv, const float* dctx, float* dqkv, int B, int L, int H, int causal,
                               float dq_scale, hipStream_t s) {
  // up to 72.5 KiB of LDS at L = 128: above the 64 KiB a kernel gets without asking.  The attribute belongs to the
  // current device's copy of the kernel, so it is set on every call (a host-side table update)
  if (hipFuncSetAttribute((const void*)attn_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)attn_bwd_lds_bytes(ATTN_BWD_MAX_L)) != hipSuccess) {
    (void)hipGetLastError();
    set_launch_error("attention_backward: the device refused 72.5 KiB of dynamic LDS");
    return;
  }
  hipLaunchKernelGGL(attn_bwd_kernel, dim3(H, B), dim3(256), attn_bwd_lds_bytes(L), s, qkv, dctx, dqkv, L, H, causal,
                     dq_scale);
}

// ------------------------------------------------------------------------------------------------ row kernels
template <int NCH>
AACLIP_DEV void load_row4(const float* p, int lane, f32x4 (&v)[NCH]) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) v[c] = *(const f32x4*)(p + (c * 64 + lane) * 4);
}

// LayerNorm backward, input gradient only: with xh = (x - mean) rstd and g = dy gamma,
//   dx = rstd (g - mean(g) - xh mean(g xh))  [+ add].
// Row r of x and dy -> row out_rows[r] of dx (out_rows NULL: row r); dx may alias dy or add.
template <int NCH>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* x, const float* __restrict__ w, const float* dy,
                                                     const float* add, float* dx, const int* __restrict__ out_rows,
                                                     long rows, float eps) {
  constexpr int D = NCH * 256;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  f32x4 v[NCH], g[NCH];
  load_row4<NCH>(x + row * D, lane, v);
  load_row4<NCH>(dy + row * D, lane, g);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
  const float mean = wave_sum(s) * (1.0f / D);
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[c][e] -= mean;
      q = fmaf(v[c][e], v[c][e], q);
    }
  const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
  float sg = 0.f, sgx = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const f32x4 gm = *(const f32x4*)(w + (c * 64 + lane) * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[c][e] *= rstd;
      g[c][e] *= gm[e];
      sg += g[c][e];
      sgx = fmaf(g[c][e], v[c][e], sgx);
    }
  }
  const float mg = wave_sum(sg) * (1.0f / D), mgx = wave_sum(sgx) * (1.0f / D);
  const long orow = out_rows ? out_rows[row] : row;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 4;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = rstd * (g[c][e] - mg - v[c][e] * mgx);
    if (add) o += *(const f32x4*)(add + orow * D + col);
    *(f32x4*)(dx + orow * D + col) = o;
  }
}

void launch_layernorm_backward(const float* x, const float* w, const float* dy, const float* add, float* dx,
                               const int* out_rows, long rows, int D, float eps, hipStream_t s) {
  dim3 g((unsigned)((rows + 3) / 4));
  switch (D / 256) {
    case 1: hipLaunchKernelGGL(ln_bwd_kernel<1>, g, dim3(256), 0, s, x, w, dy, add, dx, out_rows, rows, eps); break;
    case 2: hipLaunchKernelGGL(ln_bwd_kernel<2>, g, dim3(256), 0, s, x, w, dy, add, dx, out_rows, rows, eps); break;
    case 3: hipLaunchKernelGGL(ln_bwd_kernel<3>, g, dim3(256), 0, s, x, w, dy, add, dx, out_rows, rows, eps); break;
    case 4: hipLaunchKernelGGL(ln_bwd_kernel<4>, g, dim3(256), 0, s, x, w, dy, add, dx, out_rows, rows, eps); break;
  }
}

// Adapter mix backward.  Forward (adapter_mix_kernel): a = LeakyReLU(z), s = |u| / |a|, y = w s a + (1 - w) u.
// With c = w <dy, a> (the gradient of s):
//   du = (1 - w) dy + c / (|a| |u|) u          (direct part: the path through z = u Wa^T is the caller's GEMM)
//   da = w s dy - c |u| / |a|^3 a,   dz = da * LeakyReLU'(z)
// LeakyReLU'(z) is 1 for z > 0 and 0.01 for z <= 0: the kink itself (z = +0 or -0) takes the negative side's slope, as
// the backward of torch's leaky_relu does.
// dz may alias z, du may alias dy.
template <int NCH>
__global__ __launch_bounds__(256) void adapter_mix_bwd_kernel(const float* u, const float* z, const float* dy, float* dz,
                                                              float* du, long rows, float weight) {
  constexpr int D = NCH * 256;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  f32x4 uv[NCH], zv[NCH], gv[NCH];
  load_row4<NCH>(u + row * D, lane, uv);
  load_row4<NCH>(z + row * D, lane, zv);
  load_row4<NCH>(dy + row * D, lane, gv);
  float su = 0.f, sa = 0.f, dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = leaky(zv[c][e]);
      su = fmaf(uv[c][e], uv[c][e], su);
      sa = fmaf(a, a, sa);
      dot = fmaf(gv[c][e], a, dot);
    }
  const float nu = sqrtf(wave_sum(su)), na = sqrtf(wave_sum(sa));
  const float cs = weight * wave_sum(dot);
  const float k_u = cs / (na * nu), k_dy = weight * nu / na, k_a = cs * nu / (na * na * na);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 4;
    f32x4 odz, odu;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float zz = zv[c][e];
      const float da = k_dy * gv[c][e] - k_a * leaky(zz);
      odz[e] = zz > 0.f ? da : 0.01f * da;
      odu[e] = (1.0f - weight) * gv[c][e] + k_u * uv[c][e];
    }
    *(f32x4*)(dz + row * D + col) = odz;
    *(f32x4*)(du + row * D + col) = odu;
  }
}

void launch_adapter_mix_backward(const float* u, const float* z, const float* dy, float* dz, float* du, long rows, int D,
                                 float weight, hipStream_t s) {
  dim3 g((unsigned)((rows + 3) / 4));
  switch (D / 256) {
    case 1: hipLaunchKernelGGL(adapter_mix_bwd_kernel<1>, g, dim3(256), 0, s, u, z, dy, dz, du, rows, weight); break;
    case 2: hipLaunchKernelGGL(adapter_mix_bwd_kernel<2>, g, dim3(256), 0, s, u, z, dy, dz, du, rows, weight); break;
    case 3: hipLaunchKernelGGL(adapter_mix_bwd_kernel<3>, g, dim3(256), 0, s, u, z, dy, dz, du, rows, weight); break;
    case 4: hipLaunchKernelGGL(adapter_mix_bwd_kernel<4>, g, dim3(256), 0, s, u, z, dy, dz, du, rows, weight); break;
  }
}

// ------------------------------------------------------------------------------------------------ element-wise
// mode 0: out = gelu_erf(f)                       (the c_proj input, recomputed from the c_fc pre-activation)
// mode 1: out = g * gelu_erf'(f), gelu' = Phi(f) + f phi(f)
// mode 2: out = g * act'(f)  (act 0 identity, 1 LeakyReLU(0.01), 2 ReLU; at f = 0 both take the slope of the negative
//         side, 0.01 and 0, like torch)
// mode 3: out = f + g
template <int MODE>
__global__ __launch_bounds__(256) void ew_kernel(const float* f, const float* g, float* out, long n4, int act) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4 fv = *(const f32x4*)(f + i * 4);
  f32x4 gv = fv, o;
  if (MODE != 0) gv = *(const f32x4*)(g + i * 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = fv[e];
    if (MODE == 0) {
      o[e] = gelu_erf(x);
    } else if (MODE == 1) {
      const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
      const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
      o[e] = gv[e] * (cdf + x * pdf);
    } else if (MODE == 2) {
      const float d = act == 1 ? (x > 0.f ? 1.0f : 0.01f) : act == 2 ? (x > 0.f ? 1.0f : 0.f) : 1.0f;
      o[e] = gv[e] * d;
    } else {
      o[e] = x + gv[e];
    }
  }
  *(f32x4*)(out + i * 4) = o;
}

void launch_gelu_forward(const float* f, float* out, long n, hipStream_t s) {
  hipLaunchKernelGGL(ew_kernel<0>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, f, nullptr, out, n / 4, 0);
}
void launch_gelu_backward(const float* f, const float* dg, float* df, long n, hipStream_t s) {
  hipLaunchKernelGGL(ew_kernel<1>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, f, dg, df, n / 4, 0);
}
void launch_act_backward(const float* z, const float* dy, float* dz, long n, int act, hipStream_t s) {
  hipLaunchKernelGGL(ew_kernel<2>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, z, dy, dz, n / 4, act);
}
void launch_add_rows(const float* a, const float* b, float* out, long n, hipStream_t s) {
  hipLaunchKernelGGL(ew_kernel<3>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, a, b, out, n / 4, 0);
}

// Backward of the tail of the tap / det head (rowops.hip: normalize_rows_kernel, det_partial_kernel), in place on the
// projection rows z [B*L, E] (pre-activation).  Forward: a = act(z), n = max(|a|, 1e-12), y = a / n.  Backward:
//   dz = act'(z) (g - y <y, g>) / n      (a row below the clamp has a constant n: dz = act'(z) g / n)
// act'(0) is the slope of the negative side (LeakyReLU 0.01, ReLU 0), like torch.
// det == 0: g = row (b, t - 1) of d [B, L-1, E], the gradient of the unit patch rows.  det != 0: d is [B, E], the
// gradient of the mean over an image's L - 1 unit rows, so every patch row of image b takes g = d[b] / (L - 1).
// The CLS row (t = 0) of every image reaches neither output: dz = 0, so the products behind run over all B*L rows.
// Wave per row, the row in registers, like adapter_mix_bwd_kernel.
template <int NCH>
__global__ __launch_bounds__(256) void head_norm_bwd_kernel(float* z, const float* __restrict__ d, long rows, int L,
                                                            int act, int det) {
  constexpr int E = NCH * 256;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long b = row / L;
  const int t = (int)(row - b * L);
  float* zp = z + row * E;
  if (t == 0) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c) *(f32x4*)(zp + (c * 64 + lane) * 4) = zero;
    return;
  }
  f32x4 zv[NCH], gv[NCH];
  load_row4<NCH>(zp, lane, zv);
  load_row4<NCH>(det ? d + b * E : d + (b * (L - 1) + (t - 1)) * E, lane, gv);
  const float gs = det ? 1.0f / (float)(L - 1) : 1.0f;
  float q = 0.f, dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = zv[c][e];
      const float a = act == 1 ? leaky(x) : act == 2 ? fmaxf(x, 0.f) : x;
      gv[c][e] *= gs;
      q = fmaf(a, a, q);
      dot = fmaf(a, gv[c][e], dot);
    }
  const float nrm = sqrtf(wave_sum(q));
  const float inv = 1.0f / fmaxf(nrm, 1e-12f);
  const float ag = wave_sum(dot);
  const float yg = nrm > 1e-12f ? ag * inv : 0.f;   // <y, g>
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = zv[c][e];
      const float a = act == 1 ? leaky(x) : act == 2 ? fmaxf(x, 0.f) : x;
      const float k = act == 1 ? (x > 0.f ? 1.0f : 0.01f) : act == 2 ? (x > 0.f ? 1.0f : 0.f) : 1.0f;
      o[e] = k * ((gv[c][e] - (a * inv) * yg) * inv);
    }
    *(f32x4*)(zp + (c * 64 + lane) * 4) = o;
  }
}

void launch_head_normalize_backward(float* z, const float* d, int B, int L, int E, int act, int det, hipStream_t s) {
  const long rows = (long)B * L;
  dim3 g((unsigned)((rows + 3) / 4));
  switch (E / 256) {
    case 1: hipLaunchKernelGGL(head_norm_bwd_kernel<1>, g, dim3(256), 0, s, z, d, rows, L, act, det); break;
    case 2: hipLaunchKernelGGL(head_norm_bwd_kernel<2>, g, dim3(256), 0, s, z, d, rows, L, act, det); break;
    case 3: hipLaunchKernelGGL(head_norm_bwd_kernel<3>, g, dim3(256), 0, s, z, d, rows, L, act, det); break;
    case 4: hipLaunchKernelGGL(head_norm_bwd_kernel<4>, g, dim3(256), 0, s, z, d, rows, L, act, det); break;
  }
}

// Row pick of the row head (gather_rows_kernel's rule: the first maximum of the token ids, or row 0): copies the picked
// rows of x [n * T, D] to dst [n, D] and records their row numbers.
__global__ void pick_rows_kernel(const float* __restrict__ x, float* __restrict__ dst, int* __restrict__ idx,
                                 const int32_t* __restrict__ tokens, int Tn, int D, int mode) {
  const int i = blockIdx.x;
  __shared__ int pick;
  if (threadIdx.x == 0) {
    int best = 0;
    if (mode == 0) {
      int bv = tokens[(long)i * Tn];
      for (int t = 1; t < Tn; ++t) {
        const int v = tokens[(long)i * Tn + t];
        if (v > bv) { bv = v; best = t; }
      }
    }
    pick = best;
    idx[i] = i * Tn + best;
  }
  __syncthreads();
  const float* s = x + ((long)i * Tn + pick) * D;
  for (int d = threadIdx.x; d < D; d += blockDim.x) dst[(long)i * D + d] = s[d];
}

void launch_pick_rows(const float* x, float* dst, int* idx, const int32_t* tokens, int n, int T, int D, int mode,
                      hipStream_t s) {
  hipLaunchKernelGGL(pick_rows_kernel, dim3(n), dim3(256), 0, s, x, dst, idx, tokens, T, D, mode);
}

}  // namespace aaclip

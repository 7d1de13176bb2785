// Greedy coreset (k-center) selection over the rows of a support bank, in exact integer arithmetic:
//   min_d2[i] = UINT32_MAX;  pick[0] = start
//   for t = 0 .. n-1:  min_d2[i] = min(min_d2[i], d2(i, pick[t]));  radius2[t+1] = max_i min_d2[i];
//                      pick[t+1] = the LOWEST i that attains it
// on rows quantised once to int16 (csrc/coreset_pack.h: the quantiser, d2, the candidate word, the plan, the workspace).
//   coreset_rows_kernel    fp32 rows -> int16 rows and their int32 squared norms
//   coreset_pick_kernel    ONE launch per pick, chained by stream order: launch t reads pick t from word t (launch t-1
//                          finished it), streams every row once against that centre (int16 x int16 -> int32 on
//                          v_dot2c_i32_i16, 16 bytes per lane and load), updates min_d2, folds its rows into one
//                          candidate per workgroup and merges it into word t+1 by a no-return 64-bit integer maximum.
//                          No workgroup waits for another: no cooperative launch, no grid barrier, no flag.  The words
//                          are cleared by one memset before the first launch and nothing is reset between picks.
//   coreset_decode_kernel  the words -> picks / radius2
//   coreset_unit_rows_kernel  fp32 rows -> rows / max(|row|, 1e-12), one wave per row (the projected rows of
//                          engine.support_bank_coreset)
// The pass is a matrix-vector product: 2 bytes per multiply-add, memory-bound; the grid is sized by the bytes in flight
// (coreset_plan), not by arithmetic.  Integer sums and an integer maximum: the result does not depend on the order in
// which lanes, waves or workgroups arrive, and a second call gives the same bytes.
#include "common.h"
#include "kernels.h"
#include "coreset_pack.h"

namespace aaclip {

namespace {

typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef short i16x8 __attribute__((ext_vector_type(8)));

AACLIP_DEV int dot8(u32x4 a, u32x4 b, int acc) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t x = a[e], y = b[e];   // scalars first: a bit cast of a vector ELEMENT reads the vector's first word
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, x), __builtin_bit_cast(i16x2, y), acc, false);
  }
  return acc;
}
AACLIP_DEV unsigned long long shfl_xor_u64(unsigned long long v, int mask) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, mask, 64);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), mask, 64);
  return ((unsigned long long)hi << 32) | lo;
}

}  // namespace

// lanes = 1 << lanes_log2 lanes share a row: lane j of the row reads chunk j and chunk j + lanes (where E / 8 reaches it)
__global__ __launch_bounds__(CORESET_THREADS) void coreset_pick_kernel(const int16_t* __restrict__ q,
                                                                       const int32_t* __restrict__ norm2, long N, int E,
                                                                       int lanes_log2, long t, uint32_t start,
                                                                       unsigned long long* __restrict__ words,
                                                                       uint32_t* __restrict__ min_d2) {
  __shared__ unsigned long long wave_best[CORESET_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lanes = 1 << lanes_log2, j = lane & (lanes - 1), sub = lane >> lanes_log2;
  const int rows_per_wave = 64 >> lanes_log2, chunks = E >> 3;
  const bool second = j + lanes < chunks;
  const u32x4 zero = {0u, 0u, 0u, 0u};

  // the centre: launch t-1 is complete, so word t is final
  const uint32_t centre = t == 0 ? start : coreset_word_row(words[t]);
  if ((long)centre >= N) return;   // never with a word that a launch wrote; keeps a stray word from becoming an address
  const int16_t* crow = q + (long)centre * E;
  const u32x4 c0 = *(const u32x4*)(crow + 8 * j);
  const u32x4 c1 = second ? *(const u32x4*)(crow + 8 * (j + lanes)) : zero;
  const int32_t nc = norm2[centre];

  const long groups = (N + rows_per_wave - 1) / rows_per_wave;
  const long stride = (long)gridDim.x * CORESET_WAVES;
  unsigned long long best = 0ull;
  for (long g0 = (long)blockIdx.x * CORESET_WAVES + wave; g0 < groups; g0 += stride * CORESET_UNROLL) {
    u32x4 a0[CORESET_UNROLL], a1[CORESET_UNROLL];
    long row[CORESET_UNROLL];
    uint32_t old[CORESET_UNROLL];
    int32_t nx[CORESET_UNROLL];
#pragma unroll
    for (int u = 0; u < CORESET_UNROLL; ++u) {
      const long g = g0 + (long)u * stride;
      row[u] = g < groups ? g * rows_per_wave + sub : N;
      const bool in = row[u] < N;
      const int16_t* p = q + row[u] * (long)E;
      a0[u] = in ? *(const u32x4*)(p + 8 * j) : zero;
      a1[u] = in && second ? *(const u32x4*)(p + 8 * (j + lanes)) : zero;
      const bool lead = in && j == 0;
      nx[u] = lead ? norm2[row[u]] : 0;
      old[u] = lead && t != 0 ? min_d2[row[u]] : CORESET_D2_INIT;
    }
#pragma unroll
    for (int u = 0; u < CORESET_UNROLL; ++u) {
      int dot = dot8(a1[u], c1, dot8(a0[u], c0, 0));
      for (int m = lanes >> 1; m > 0; m >>= 1) dot += __shfl_xor(dot, m, 64);
      if (row[u] < N && j == 0) {
        const uint32_t d2 = coreset_d2(nx[u], nc, dot);
        const uint32_t now = d2 < old[u] ? d2 : old[u];
        if (t == 0 || now != old[u]) min_d2[row[u]] = now;
        best = coreset_merge(best, coreset_word(now, (uint32_t)row[u]));
      }
    }
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) best = coreset_merge(best, shfl_xor_u64(best, m));
  if (lane == 0) wave_best[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < CORESET_WAVES; ++w) best = coreset_merge(best, wave_best[w]);
    if (best != 0ull) atomicMax(words + t + 1, best);
  }
}

__global__ __launch_bounds__(256) void coreset_decode_kernel(const unsigned long long* __restrict__ words, long n,
                                                             uint32_t start, int32_t* __restrict__ picks,
                                                             uint32_t* __restrict__ radius2) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t > n) return;
  const unsigned long long w = words[t];
  radius2[t] = t == 0 ? CORESET_D2_INIT : coreset_word_d2(w);
  if (t < n) picks[t] = t == 0 ? (int32_t)start : (int32_t)coreset_word_row(w);
}

// the quantiser: the lanes of a row as in coreset_pick_kernel, 8 floats per chunk
__global__ __launch_bounds__(256) void coreset_rows_kernel(const float* __restrict__ rows, long N, int E, int lanes_log2,
                                                           int16_t* __restrict__ q, int32_t* __restrict__ norm2) {
  const int lane = threadIdx.x & 63;
  const int lanes = 1 << lanes_log2, j = lane & (lanes - 1), sub = lane >> lanes_log2;
  const int rows_per_wave = 64 >> lanes_log2, chunks = E >> 3;
  const long row = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rows_per_wave + sub;
  const bool in = row < N;
  unsigned long long sum = 0ull;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = j + k * lanes;
    if (in && c < chunks) {
      const float* p = rows + row * (long)E + 8 * c;
      const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + 4);
      i16x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = coreset_quantise(v0[e]);
        o[4 + e] = coreset_quantise(v1[e]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += (unsigned long long)((int)o[e] * (int)o[e]);
      *(i16x8*)(q + row * (long)E + 8 * c) = o;
    }
  }
  for (int m = lanes >> 1; m > 0; m >>= 1) sum += shfl_xor_u64(sum, m);
  if (in && j == 0) norm2[row] = coreset_norm2_saturate(sum);
}

// one wave per row, a fixed order of summation
__global__ __launch_bounds__(256) void coreset_unit_rows_kernel(const float* __restrict__ rows, long N, int E,
                                                                float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* p = rows + row * (long)E;
  float s = 0.f;
  for (int k = 4 * lane; k < E; k += 256) {
    const f32x4 v = *(const f32x4*)(p + k);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  s = wave_sum(s);
  const float scale = 1.0f / fmaxf(sqrtf(s), 1e-12f);
  float* o = out + row * (long)E;
  for (int k = 4 * lane; k < E; k += 256) {
    const f32x4 v = *(const f32x4*)(p + k);
    *(f32x4*)(o + k) = v * scale;
  }
}

size_t coreset_ws_bytes(long n) { return coreset_layout(n).bytes; }

void launch_coreset_rows(const float* rows, long N, int E, int16_t* q, int32_t* norm2, hipStream_t s) {
  const CoresetPlan p = coreset_plan(N, E);
  const long blocks = (p.groups + 3) / 4;
  hipLaunchKernelGGL(coreset_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, rows, N, E, p.lanes_log2, q, norm2);
}

void launch_coreset_select(const int16_t* q, const int32_t* norm2, long N, int E, long n, long start, int32_t* picks,
                           uint32_t* radius2, uint32_t* min_d2, void* ws, hipStream_t s) {
  const CoresetPlan p = coreset_plan(N, E);
  unsigned long long* words = (unsigned long long*)((char*)ws + coreset_layout(n).words);
  (void)hipMemsetAsync(words, 0, (size_t)(n + 1) * 8, s);
  for (long t = 0; t < n; ++t)
    hipLaunchKernelGGL(coreset_pick_kernel, dim3((unsigned)p.workgroups), dim3(CORESET_THREADS), 0, s, q, norm2, N, E,
                       p.lanes_log2, t, (uint32_t)start, words, min_d2);
  hipLaunchKernelGGL(coreset_decode_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, words, n,
                     (uint32_t)start, picks, radius2);
}

void launch_coreset_unit_rows(const float* rows, long N, int E, float* out, hipStream_t s) {
  hipLaunchKernelGGL(coreset_unit_rows_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, rows, N, E, out);
}

}  // namespace aaclip

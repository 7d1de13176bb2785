// split3 rows (bf16x3.h): fp32 [rows, K] -> bf16 [rows, 3K] = [hi | lo | hi] with hi = bf16(v), lo = bf16(v - hi), both
// conversions round-to-nearest-even (the planes equal torch's .bfloat16() bit for bit; v - hi is exact in fp32).  A
// thread takes eight consecutive values: two 16-byte loads, three 16-byte stores.  The GELU forms apply
// text_backward.hip's element-wise arithmetic (mode 0 / 1 of its ew_kernel, the same expressions) on the way, so the
// F-wide fp32 rows between the row pass and the split never exist.
#include "bf16x3.h"
#include "common.h"

namespace aaclip {

namespace {

enum { S3_COPY = 0, S3_GELU = 1, S3_GELU_BWD = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ src, const float* __restrict__ g,
                                                     bf16* __restrict__ dst, long n8, int K) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int k8 = K >> 3;
  const long row = i / k8;
  const int c = (int)(i - row * k8) * 8;
  float v[8];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f32x4 fv = *(const f32x4*)(src + i * 8 + 4 * j);
    f32x4 gv = fv;
    if (MODE == S3_GELU_BWD) gv = *(const f32x4*)(g + i * 8 + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = fv[e];
      if (MODE == S3_COPY) {
        v[4 * j + e] = x;
      } else if (MODE == S3_GELU) {
        v[4 * j + e] = gelu_erf(x);
      } else {
        const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
        const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
        v[4 * j + e] = gv[e] * (cdf + x * pdf);
      }
    }
  }
  bf16x8 hi, lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    hi[e] = (bf16)v[e];
    lo[e] = (bf16)(v[e] - (float)hi[e]);
  }
  bf16* o = dst + row * 3 * K + c;
  *(bf16x8*)o = hi;
  *(bf16x8*)(o + K) = lo;
  *(bf16x8*)(o + 2 * K) = hi;
}

template <int MODE>
void launch_split3(const float* src, const float* g, void* dst, long rows, int K, hipStream_t s) {
  const long n8 = rows * (K >> 3);
  hipLaunchKernelGGL(split3_kernel<MODE>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, src, g, (bf16*)dst, n8, K);
}

}  // namespace

void launch_split3_rows(const float* src, void* dst, long rows, int K, hipStream_t s) {
  launch_split3<S3_COPY>(src, nullptr, dst, rows, K, s);
}
void launch_gelu_forward_split3(const float* f, void* dst, long rows, int K, hipStream_t s) {
  launch_split3<S3_GELU>(f, nullptr, dst, rows, K, s);
}
void launch_gelu_backward_split3(const float* f, const float* dg, void* dst, long rows, int K, hipStream_t s) {
  launch_split3<S3_GELU_BWD>(f, dg, dst, rows, K, s);
}

}  // namespace aaclip

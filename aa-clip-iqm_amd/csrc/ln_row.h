// LayerNorm of one token row by one 64-lane wave: the row lives in registers (16-byte coalesced loads), no LDS and no
// barrier.  Shared by layernorm_kernel (rowops.hip) and the LayerNorm workers of the residual products' tail launch
// (gemm256t.hip, tail_plan.h), so both produce the same bits.
#pragma once
#include "common.h"

namespace aaclip {

template <int NCH>
AACLIP_DEV void load_row(const float* p, int lane, f32x4 (&v)[NCH]) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) v[c] = *(const f32x4*)(p + (c * 64 + lane) * 4);
}

template <typename T>
AACLIP_DEV void store4(T* p, f32x4 v);
template <>
AACLIP_DEV void store4<float>(float* p, f32x4 v) { *(f32x4*)p = v; }
template <>
AACLIP_DEV void store4<f16>(f16* p, f32x4 v) {
  f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
  *(f16x4*)p = o;
}
template <>
AACLIP_DEV void store4<bf16>(bf16* p, f32x4 v) {
  bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  *(bf16x4*)p = o;
}

// split8 row (AACLIP_F16X2, common.h): 4 values at column `col` of a row of logical width `width` starting at `row`:
// hi plane (fp16), then the lo8 and hi8 planes (e4m3, one byte per element)
// hi8 = false: the hi8 plane is not written (its only reader is the Ah8 . Wl8 correction tile, which a product whose
// weight is exact in fp16 skips)
AACLIP_DEV void store4_split(f16* row, int col, f32x4 v, int width, bool hi8 = true) {
  const float vv[4] = {v[0], v[1], v[2], v[3]};
  f16x4 hi;
  uint32_t l8, h8;
  split8x4(vv, hi, l8, h8);
  *(f16x4*)(row + col) = hi;
  uint8_t* p8 = (uint8_t*)(row + width);
  *(uint32_t*)(p8 + col) = l8;
  if (hi8) *(uint32_t*)(p8 + width + col) = h8;
}

// LayerNorm over the last dim, reference model/transformer.py:37-43 (eps 1e-5), two-pass statistics in registers, of
// the row held in v with this lane's weights g and biases bb (load_row of w and b); out_row = the row's first output
// element (SPLIT: a split8 row of 2 * D halves)
template <typename T, int NCH, bool SPLIT>
AACLIP_DEV void layernorm_row(const f32x4 (&v)[NCH], const f32x4 (&g)[NCH], const f32x4 (&bb)[NCH], T* out_row, int lane,
                              float eps, bool hi8) {
  constexpr int D = NCH * 256;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
  const float mean = wave_sum(s) * (1.0f / D);
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float d = v[c][e] - mean;
      q = fmaf(d, d, q);
    }
  const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 4;
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (v[c][e] - mean) * rstd * g[c][e] + bb[c][e];
    if constexpr (SPLIT) store4_split(out_row, col, y, D, hi8);
    else store4<T>(out_row + col, y);
  }
}

// A wave that walks rows first, first + stride, ... below `rows` (all wave-uniform) into split8 rows.  PF rows of loads
// are in flight (16 registers each at D = 1024; the GEMM side of the launch holds the register budget anyway): at the
// eight waves per CU of a workgroup that shares its launch with GEMM tiles, one or two rows do not reach the HBM rate.
// The weights stay in registers for the whole walk: loads return in order, so a load of them per row would wait for the
// row just requested and leave ONE row in flight.
template <int NCH>
AACLIP_DEV void layernorm_split_rows_strided(const float* x, const float* __restrict__ w, const float* __restrict__ b,
                                             f16* out, long first, long stride, long rows, int lane, float eps,
                                             bool hi8) {
  constexpr int D = NCH * 256, PF = 8;
  f32x4 v[PF][NCH], g[NCH], bb[NCH];
  load_row<NCH>(w, lane, g);
  load_row<NCH>(b, lane, bb);
#pragma unroll
  for (int k = 0; k < PF; ++k)
    if (first + k * stride < rows) load_row<NCH>(x + (first + k * stride) * D, lane, v[k]);
  for (long r = first; r < rows; r += PF * stride) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const long rk = r + k * stride;
      if (rk < rows) {
        layernorm_row<f16, NCH, true>(v[k], g, bb, out + rk * 2 * D, lane, eps, hi8);
        const long rn = rk + PF * stride;
        if (rn < rows) load_row<NCH>(x + rn * D, lane, v[k]);
      }
    }
  }
}

}  // namespace aaclip

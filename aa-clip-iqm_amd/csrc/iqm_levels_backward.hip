// Backward of aaclip_cross_rows_levels (iqm.hip): per image b, R effective queries over the 16-bit rows of up to four
// segments that share ONE softmax,
//   s_(r,s,j) = qt[b,r,s] . x[s][b,j],  p_r = softmax over all (s, j),  out[b,r,s] = sum_j p_(r,s,j) x[s][b,j]
// and from d_out [B, R, nseg, Dk], with g_(r,s,j) = d_out[b,r,s] . x[s][b,j] and delta_r = sum_(s,j) p g:
//   ds = p (g - delta_r),  d_qt[b,r,s] = sum_j ds_(r,s,j) x[s][b,j],
//   d_x[s][b,j] = sum_r (p_(r,s,j) d_out[b,r,s] + ds_(r,s,j) qt[b,r,s]).
// The passes are those of iqm_backward.hip (fp32 arithmetic on the row values as they are, exact-fp32
// v_mfma_f32_32x32x2_f32 products, operand maps there), with a workgroup per (image, segment, key slice):
//   clb_scores_kernel   SG[b, s, j, 0:16] = s_(., s, j) and SG[b, s, j, 16:32] = g_(., s, j)
//   crb_stats_kernel    (crb_common.h) over the nseg * Lk records of an image: one m, 1 / l and delta per (b, r)
//   clb_grad_kernel     d_x[s] tile = [P | dS] . [d_out[., s] ; qt[., s]]; dS^T X accumulates over the slice
//   clb_combine_kernel  d_qt[b, r, s] = the slices' partials of segment s added in slice order
// Rows: image b's key j of segment s is row b * rows_per_image + row0 + j of x[s] (ldx elements apart) and of d_x[s]
// (Dk floats apart); rows outside [row0, row0 + Lk) are never touched.  No atomics, every output element is written by
// one thread, every sum runs in a fixed order: two calls give the same bits.
#include "common.h"
#include "crb_common.h"
#include "kernels.h"

namespace aaclip {

struct LevelRows { const void* x[4]; float* d_x[4]; };

// grid (nseg * slices, B).  Column c of the right-hand side: qt[b, c, seg] for c < 16, d_out[b, c - 16, seg] otherwise.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void clb_scores_kernel(LevelRows lv, const float* __restrict__ qt,
                                                         const float* __restrict__ dout, float* __restrict__ sg, int R,
                                                         int nseg, int slices, int rows_per_image, int row0, int Lk,
                                                         long ldx, int per) {
  constexpr int Dk = NCH * 256, DW = NCH * 64;
  __shared__ float red[4][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, seg = blockIdx.x / slices, sl = blockIdx.x - seg * slices;
  const int j0 = sl * per, j1 = min(Lk, j0 + per);
  const int d0 = wave * DW;
  const T* x = (const T*)lv.x[seg] + ((long)b * rows_per_image + row0) * ldx;
  float* sgs = sg + ((long)b * nseg + seg) * Lk * 32;
  float qd[DW / 2];
  {
    const int q = r & 15;
    const float* src = (r < 16 ? qt : dout) + (((long)b * R + (q < R ? q : 0)) * nseg + seg) * Dk + d0 + 4 * h;
#pragma unroll
    for (int c = 0; c < DW / 8; ++c) {
      const f32x4 v = *(const f32x4*)(src + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) qd[4 * c + e] = q < R ? v[e] : 0.f;
    }
  }
  for (int t0 = j0; t0 < j1; t0 += 32) {
    int row = t0 + r;
    row = row < j1 ? row : j1 - 1;
    const T* xr = x + (long)row * ldx + d0 + 4 * h;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < DW / 8; ++c) {
      const f32x4 v = crb_ld4(xr + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[e], qd[4 * c + e], acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave][e][lane] = acc[e];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = tid + 256 * k;
      const int e = idx >> 6, ln = idx & 63;
      const float v = ((red[0][e][ln] + red[1][e][ln]) + red[2][e][ln]) + red[3][e][ln];
      const int key = t0 + crb_row(e, ln >> 5);
      if (key < j1) sgs[(long)key * 32 + (ln & 31)] = v;
    }
    __syncthreads();
  }
}

// grid (nseg * slices, B).  The d_x pointers or part may be null (not both).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void clb_grad_kernel(LevelRows lv, const float* __restrict__ qt,
                                                       const float* __restrict__ dout, const float* __restrict__ sg,
                                                       const float* __restrict__ stats, float* __restrict__ part, int R,
                                                       int nseg, int slices, int rows_per_image, int row0, int Lk,
                                                       int ldx, int per, int accumulate) {
  constexpr int Dk = NCH * 256, DW = NCH * 64, NB = DW / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, seg = blockIdx.x / slices, sl = blockIdx.x - seg * slices;
  const int j0 = sl * per, j1 = min(Lk, j0 + per);
  const int d0 = wave * DW;
  const float* st = stats + (long)b * 16 * 4;
  const T* x = (const T*)lv.x[seg] + ((long)b * rows_per_image + row0) * ldx;   // offsets inside an image: 32 bits
  float* d_x = lv.d_x[seg] ? lv.d_x[seg] + ((long)b * rows_per_image + row0) * Dk : nullptr;
  const float* sgs = sg + ((long)b * nseg + seg) * Lk * 32;

  // d_x: step i of the [P | dS] . [d_out ; qt] product is row c = 2 i + h: d_out row c for i < 8, qt row c - 16 after
  float dq[NB][16];
  float m8[8], li8[8], de8[8];
  if (d_x) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = 2 * (i & 7) + h;
      const float* src = (i < 8 ? dout : qt) + (((long)b * R + (q < R ? q : 0)) * nseg + seg) * Dk + d0 + r;
#pragma unroll
      for (int k = 0; k < NB; ++k) dq[k][i] = q < R ? src[32 * k] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = 2 * i + h;
      const bool on = q < R;
      m8[i] = on ? st[q * 4] : 0.f;
      li8[i] = on ? st[q * 4 + 1] : 0.f;
      de8[i] = on ? st[q * 4 + 2] : 0.f;
    }
  }
  // d_qt: row r of dS^T (r < R), the statistics of query r
  const bool qrow = r < R;   // R <= 16
  const float m2 = qrow ? st[r * 4] : 0.f, li2 = qrow ? st[r * 4 + 1] : 0.f, de2 = qrow ? st[r * 4 + 2] : 0.f;
  f32x16 aq[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k)
#pragma unroll
    for (int e = 0; e < 16; ++e) aq[k][e] = 0.f;

  for (int t0 = j0; t0 < j1; t0 += 32) {
    if (d_x) {
      const bool alive = t0 + r < j1;
      const float* sr = sgs + (alive ? t0 + r : j1 - 1) * 32;
      f32x4 sv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) sv[c] = *(const f32x4*)(sr + 4 * c);
      float a[16];
#pragma unroll
      for (int i = 0; i < 8; ++i) {   // query 2 i + h: element 2 (i & 1) + h of chunk i / 2 (s) and 4 + i / 2 (g)
        const float s = h ? sv[i >> 1][2 * (i & 1) + 1] : sv[i >> 1][2 * (i & 1)];
        const float g = h ? sv[4 + (i >> 1)][2 * (i & 1) + 1] : sv[4 + (i >> 1)][2 * (i & 1)];
        const float p = (alive && 2 * i + h < R) ? crb_p(s, m8[i], li8[i]) : 0.f;
        a[i] = p;
        a[8 + i] = p * (g - de8[i]);
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], dq[k][i], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = t0 + crb_row(e, h);
          if (key < j1) {
            const int o = key * Dk + d0 + 32 * k + r;
            float v = acc[e];
            if (accumulate) v = d_x[o] + v;
            d_x[o] = v;
          }
        }
      }
    }
    if (part) {
      float a2[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = t0 + 2 * i + h;
        const bool alive = key < j1 && qrow;
        const float* sr = sgs + (key < j1 ? key : j1 - 1) * 32 + (r & 15);
        const float p = alive ? crb_p(sr[0], m2, li2) : 0.f;
        a2[i] = p * (sr[16] - de2);
      }
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = t0 + 2 * i + h;
          const float xv = crb_ld1(x + (key < j1 ? key : j1 - 1) * ldx + d0 + 32 * k + r);
          aq[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[i], xv, aq[k], 0, 0, 0);
        }
    }
  }
  if (part) {
    float* pp = part + ((((long)b * nseg + seg) * slices + sl) * R) * Dk;
#pragma unroll
    for (int k = 0; k < NB; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {   // accumulator rows 0 .. 15 are elements 0 .. 7 of both halves
        const int q = crb_row(e, h);
        if (q < R) pp[(long)q * Dk + d0 + 32 * k + r] = aq[k][e];
      }
  }
}

// grid (R, nseg, B): d_qt[b, r, seg, :] = the partials of the segment's slices in slice order
__global__ __launch_bounds__(256) void clb_combine_kernel(const float* __restrict__ part, float* __restrict__ d_qt, int R,
                                                          int Dk, int nseg, int slices) {
  const int q = blockIdx.x, seg = blockIdx.y, b = blockIdx.z;
  for (int d = threadIdx.x; d < Dk; d += 256) {
    float t = 0.f;
    for (int s = 0; s < slices; ++s) t += part[((((long)b * nseg + seg) * slices + s) * R + q) * Dk + d];
    d_qt[(((long)b * R + q) * nseg + seg) * Dk + d] = t;
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The slicing of a segment's keys is cross_rows_backward's (kernels.h).  Workspace:
// partial d_qt [B, nseg, slots, R, Dk] | SG [B, nseg, Lk, 32] | statistics [B, 16, 4]; slots = min(CRB_MAX_SLICES,
// ceil(Lk / 64)) bounds the slice count and does not decrease with Lk.
static size_t clb_part_floats(int B, int R, int nseg, int Lk, int Dk) {
  const size_t slots = (size_t)((Lk + 63) / 64 < CRB_MAX_SLICES ? (Lk + 63) / 64 : CRB_MAX_SLICES);
  return ((size_t)B * nseg * slots * R * Dk + 63) & ~(size_t)63;
}
size_t cross_rows_levels_backward_ws_bytes(int B, int R, int nseg, int Lk, int Dk) {
  if (B <= 0 || R <= 0 || nseg <= 0 || Lk <= 0 || Dk <= 0) return 0;
  return (clb_part_floats(B, R, nseg, Lk, Dk) + (size_t)B * nseg * Lk * 32 + (size_t)B * 16 * 4) * 4;
}
const char* cross_rows_levels_backward_check(int x_dtype, int R, int nseg, int Lk, int Dk, long ldx) {
  if (x_dtype != AACLIP_F16 && x_dtype != AACLIP_BF16) return "cross_rows_levels_backward: rows must be fp16 or bf16";
  if (R != 4 && R != 8 && R != 12 && R != 16) return "cross_rows_levels_backward: 4, 8, 12 or 16 effective queries per image";
  if (nseg < 1 || nseg > 4) return "cross_rows_levels_backward: 1..4 segments";
  if (Lk < 1) return "cross_rows_levels_backward: no keys";
  if (Dk != 768 && Dk != 1024) return "cross_rows_levels_backward: row width must be 768 or 1024";
  if (ldx < Dk || (ldx & 7)) return "cross_rows_levels_backward: row stride must be >= the width and a multiple of 8 elements";
  return nullptr;
}

template <typename T>
static void clb_t(const float* qt, const LevelRows& lv, const float* dout, float* d_qt, int accumulate, int B, int R,
                  int nseg, int rows_per_image, int row0, int Lk, int Dk, long ldx, float* ws, hipStream_t s) {
  const int per = crb_per(Lk), slices = cross_rows_backward_slices(Lk);
  float* part = ws;
  float* sg = part + clb_part_floats(B, R, nseg, Lk, Dk);
  float* stats = sg + (size_t)B * nseg * Lk * 32;
  float* pp = d_qt ? part : nullptr;
  const dim3 g(nseg * slices, B), blk(256);
#define CLB(N)                                                                                                         \
  hipLaunchKernelGGL((clb_scores_kernel<T, N>), g, blk, 0, s, lv, qt, dout, sg, R, nseg, slices, rows_per_image, row0, \
                     Lk, ldx, per);                                                                                    \
  hipLaunchKernelGGL(crb_stats_kernel, dim3(R, B), blk, 0, s, sg, stats, nseg * Lk);                                   \
  hipLaunchKernelGGL((clb_grad_kernel<T, N>), g, blk, 0, s, lv, qt, dout, sg, stats, pp, R, nseg, slices,              \
                     rows_per_image, row0, Lk, (int)ldx, per, accumulate)
  if (Dk == 1024) { CLB(4); }
  else { CLB(3); }
#undef CLB
  if (d_qt) hipLaunchKernelGGL(clb_combine_kernel, dim3(R, nseg, B), blk, 0, s, part, d_qt, R, Dk, nseg, slices);
}

void launch_cross_rows_levels_backward(int x_dtype, const float* qt, const void* const* x, int nseg, const float* dout,
                                       float* d_qt, float* const* d_x, int accumulate, int B, int R, int rows_per_image,
                                       int row0, int Lk, int Dk, long ldx, void* ws, hipStream_t s) {
  LevelRows lv;
  for (int i = 0; i < 4; ++i) {
    lv.x[i] = x[i < nseg ? i : 0];
    lv.d_x[i] = d_x ? d_x[i < nseg ? i : 0] : nullptr;
  }
  if (x_dtype == AACLIP_F16)
    clb_t<f16>(qt, lv, dout, d_qt, accumulate, B, R, nseg, rows_per_image, row0, Lk, Dk, ldx, (float*)ws, s);
  else
    clb_t<bf16>(qt, lv, dout, d_qt, accumulate, B, R, nseg, rows_per_image, row0, Lk, Dk, ldx, (float*)ws, s);
}

}  // namespace aaclip

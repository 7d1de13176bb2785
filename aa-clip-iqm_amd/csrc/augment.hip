// Train-time input work on raw frames (reference dataset/__init__.py:37-102), one kernel family per step:
//   colour jitter   torchvision's ColorJitter(brightness) / (contrast) / (saturation) on a PIL image, i.e. Pillow's
//                   ImageEnhance.{Brightness, Contrast, Color}: Image.blend(degenerate, image, factor) on bytes
//   mask            Resize((S, S), NEAREST) -> ToTensor -> (!= 0): Pillow's nearest index map
//   geometry        RandomRotation / RandomAffine(translate) / RandomHorizontalFlip / RandomVerticalFlip on the
//                   [4, S, S] tensor of image and mask: nearest sampling, zero fill, composed into one gather
// Every random number is an INPUT: the host draws them (dataset.draw_augment_params), the kernels only apply them.
// The bicubic resize and the normalisation between the colour step and the geometry are preprocess.hip, unchanged.
#include "common.h"
#include "kernels.h"
#include <math.h>

namespace aaclip {

// ------------------------------------------------------------------------------------------- colour jitter
// The frames are one flat byte array of B*H*W pixels.  A thread owns a GROUP of 16 pixels = 48 bytes = three 16-byte
// vectors when the base pointers are 16-byte aligned and the group is whole; the last group of the array (and every
// group of an unaligned array) moves byte by byte.  A group may straddle frames (H*W is no multiple of 16 in
// general, and a 1x1 frame is shorter than a group), so the frame index is followed pixel by pixel.
static constexpr int CJ_GROUP = 16;
static constexpr int CJ_THREADS = 256;
static constexpr int CJ_MAX_BLOCKS = 64;   // workgroups per frame of the luma sum

int color_jitter_sum_blocks(long pixels) {
  const long groups = (pixels + CJ_GROUP - 1) / CJ_GROUP + 1;   // + 1: the frame's first group may start before it
  const long blocks = (groups + CJ_THREADS - 1) / CJ_THREADS;
  return (int)(blocks < CJ_MAX_BLOCKS ? blocks : CJ_MAX_BLOCKS);
}

// Pillow's L of an RGB pixel (ImagingConvert rgb2l)
AACLIP_DEV int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Pillow's ImagingBlend on one byte: fp32 d + f * (s - d), truncated toward zero; outside 0 <= f <= 1 the value is
// clipped to [0, 255] first (inside, it cannot leave that range, so the clip is applied always)
AACLIP_DEV int blend(int d, int s, float f) {
  float t = (float)d + f * (float)(s - d);
  t = fminf(fmaxf(t, 0.f), 255.f);
  return (int)t;
}

union PixelGroup {
  u32x4 v[3];
  uint8_t px[48];
};

AACLIP_DEV void load_group(const uint8_t* __restrict__ src, long byte0, long total_bytes, bool vec, PixelGroup& g) {
  if (vec && byte0 + 48 <= total_bytes) {
    const u32x4* p = (const u32x4*)(src + byte0);
    g.v[0] = p[0];
    g.v[1] = p[1];
    g.v[2] = p[2];
  } else {
#pragma unroll
    for (int j = 0; j < 48; ++j) g.px[j] = byte0 + j < total_bytes ? src[byte0 + j] : 0;
  }
}

// partial[b * nblk + blockIdx.x] = sum of L over this workgroup's share of frame b AFTER its brightness step.  Integer
// sums: any order gives the same value.  Frames whose contrast bit is clear are skipped (their partials stay unread).
__global__ __launch_bounds__(CJ_THREADS) void color_luma_sum_kernel(const uint8_t* __restrict__ src, long HW,
                                                                    long total_bytes, int vec,
                                                                    const float* __restrict__ factors,
                                                                    const int32_t* __restrict__ apply,
                                                                    unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long red[CJ_THREADS];
  const int b = blockIdx.y, nblk = gridDim.x;
  const int m = apply[b];
  if (!(m & 2)) return;
  const float fb = factors[3 * b];
  const long p_lo = (long)b * HW, p_hi = p_lo + HW;
  const long g_lo = p_lo / CJ_GROUP, g_hi = (p_hi + CJ_GROUP - 1) / CJ_GROUP;
  unsigned long long acc = 0;
  for (long g = g_lo + (long)blockIdx.x * CJ_THREADS + threadIdx.x; g < g_hi; g += (long)nblk * CJ_THREADS) {
    PixelGroup grp;
    load_group(src, g * 48, total_bytes, vec != 0, grp);
    const uint8_t* px = grp.px;
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j < CJ_GROUP; ++j) {
      const long p = g * CJ_GROUP + j;
      int r = px[3 * j], gg = px[3 * j + 1], bb = px[3 * j + 2];
      if (m & 1) {
        r = blend(0, r, fb);
        gg = blend(0, gg, fb);
        bb = blend(0, bb, fb);
      }
      if (p >= p_lo && p < p_hi) s += (unsigned)luma(r, gg, bb);
    }
    acc += s;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = CJ_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(size_t)b * nblk + blockIdx.x] = red[0];
}

// mean[b] = int(sum / count + 0.5) in integers (ImageStat mean of L, then ImageEnhance.Contrast's rounding)
__global__ void color_luma_mean_kernel(const unsigned long long* __restrict__ partial, int nblk, int B, long HW,
                                       const int32_t* __restrict__ apply, int32_t* __restrict__ mean) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  unsigned long long s = 0;
  if (apply[b] & 2)
    for (int i = 0; i < nblk; ++i) s += partial[(size_t)b * nblk + i];
  mean[b] = (int32_t)((2 * s + (unsigned long long)HW) / (2 * (unsigned long long)HW));
}

__global__ __launch_bounds__(CJ_THREADS) void color_jitter_kernel(const uint8_t* __restrict__ src,
                                                                  uint8_t* __restrict__ dst, long HW, long total_bytes,
                                                                  int vec, const float* __restrict__ factors,
                                                                  const int32_t* __restrict__ apply,
                                                                  const int32_t* __restrict__ mean) {
  const long g = (long)blockIdx.x * CJ_THREADS + threadIdx.x;
  const long byte0 = g * 48;
  if (byte0 >= total_bytes) return;
  PixelGroup grp;
  load_group(src, byte0, total_bytes, vec != 0, grp);
  uint8_t* px = grp.px;
  const long p0 = g * CJ_GROUP;
  int b = (int)(p0 / HW);
  long left = (long)(b + 1) * HW - p0;   // pixels of this group's range that still belong to frame b
  int m = 0, mu = 0;
  float fb = 1.f, fc = 1.f, fs = 1.f;
  bool fresh = true;
#pragma unroll
  for (int j = 0; j < CJ_GROUP; ++j) {
    if (byte0 + 3 * j >= total_bytes) break;
    while (left <= 0) {
      ++b;
      left += HW;
      fresh = true;
    }
    if (fresh) {
      m = apply[b];
      mu = mean[b];
      fb = factors[3 * b];
      fc = factors[3 * b + 1];
      fs = factors[3 * b + 2];
      fresh = false;
    }
    --left;
    int r = px[3 * j], gg = px[3 * j + 1], bb = px[3 * j + 2];
    if (m & 1) {
      r = blend(0, r, fb);
      gg = blend(0, gg, fb);
      bb = blend(0, bb, fb);
    }
    if (m & 2) {
      r = blend(mu, r, fc);
      gg = blend(mu, gg, fc);
      bb = blend(mu, bb, fc);
    }
    if (m & 4) {
      const int l = luma(r, gg, bb);
      r = blend(l, r, fs);
      gg = blend(l, gg, fs);
      bb = blend(l, bb, fs);
    }
    px[3 * j] = (uint8_t)r;
    px[3 * j + 1] = (uint8_t)gg;
    px[3 * j + 2] = (uint8_t)bb;
  }
  if (vec && byte0 + 48 <= total_bytes) {
    u32x4* p = (u32x4*)(dst + byte0);
    p[0] = grp.v[0];
    p[1] = grp.v[1];
    p[2] = grp.v[2];
  } else {
#pragma unroll
    for (int j = 0; j < 48; ++j)
      if (byte0 + j < total_bytes) dst[byte0 + j] = px[j];
  }
}

// ws: [B * nblk] 64-bit partials, then [B] int32 means
void launch_color_jitter(const uint8_t* src, uint8_t* dst, int B, int H, int W, const float* factors,
                         const int32_t* apply, void* ws, hipStream_t s) {
  const long HW = (long)H * W, total = HW * B * 3;
  const int nblk = color_jitter_sum_blocks(HW);
  const int vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  unsigned long long* partial = (unsigned long long*)ws;
  int32_t* mean = (int32_t*)(partial + (size_t)B * nblk);
  hipLaunchKernelGGL(color_luma_sum_kernel, dim3(nblk, B), dim3(CJ_THREADS), 0, s, src, HW, total, vec, factors, apply,
                     partial);
  hipLaunchKernelGGL(color_luma_mean_kernel, dim3((B + 63) / 64), dim3(64), 0, s, partial, nblk, B, HW, apply, mean);
  const long groups = (HW * B + CJ_GROUP - 1) / CJ_GROUP;
  hipLaunchKernelGGL(color_jitter_kernel, dim3((unsigned)((groups + CJ_THREADS - 1) / CJ_THREADS)), dim3(CJ_THREADS), 0,
                     s, src, dst, HW, total, vec, factors, apply, mean);
}

// ---------------------------------------------------------------------------------------------------- mask
// Pillow's NEAREST resize is an affine scale (Geometry.c, ImagingScaleAffine): the source coordinate starts at half a
// step and is ADVANCED by repeated addition in double, then truncated.  Equal sizes: Image.resize returns a copy.
void nearest_table(int in_size, int out_size, int32_t* idx) {
  if (in_size == out_size) {
    for (int i = 0; i < out_size; ++i) idx[i] = i;
    return;
  }
  const double step = (double)in_size / out_size;
  double pos = 0.0 + step * 0.5;
  for (int i = 0; i < out_size; ++i) {
    int v = pos < 0.0 ? -1 : (int)pos;
    idx[i] = v < 0 ? 0 : (v >= in_size ? in_size - 1 : v);
    pos += step;
  }
}

// grid (ceil(S*S / 256), B).  out[b, 0, y, x] = src[b, ymap[y], xmap[x]] != 0, or 0 for a frame flagged normal.
__global__ __launch_bounds__(256) void mask_preprocess_kernel(const uint8_t* __restrict__ src, int Hm, int Wm, int S,
                                                              const int32_t* __restrict__ xmap,
                                                              const int32_t* __restrict__ ymap,
                                                              const int32_t* __restrict__ normal,
                                                              float* __restrict__ out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S * S) return;
  float v = 0.f;
  if (!(normal && normal[b])) {
    const int y = i / S, x = i - y * S;
    const int ys = min(max(ymap[y], 0), Hm - 1), xs = min(max(xmap[x], 0), Wm - 1);   // a table is never trusted
    v = src[((size_t)b * Hm + ys) * Wm + xs] != 0 ? 1.f : 0.f;
  }
  out[(size_t)b * S * S + i] = v;
}

void launch_mask_preprocess(const uint8_t* src, int B, int Hm, int Wm, int S, const int32_t* xmap, const int32_t* ymap,
                            const int32_t* normal, float* out, hipStream_t s) {
  hipLaunchKernelGGL(mask_preprocess_kernel, dim3((S * S + 255) / 256, B), dim3(256), 0, s, src, Hm, Wm, S, xmap, ymap,
                     normal, out);
}

// ------------------------------------------------------------------------------------------------ geometry
// One gather per output pixel.  The reference applies rotation, shift, horizontal flip, vertical flip in that order,
// each a pure gather with zero fill, so the output pixel is traced back through them in reverse: undo the vertical
// flip, undo the horizontal flip, undo the shift (outside: 0), then take the rotation's source pixel (outside: 0).
// Rotation, torchvision's tensor path (affine grid about the centre, nearest, align_corners = False):
//   xs = cos(t) * xc - sin(t) * yc + S/2 - 0.5,  ys = sin(t) * xc + cos(t) * yc + S/2 - 0.5,  xc = x + 0.5 - S/2
// evaluated in fp64 (cos / sin once per workgroup), rounded to nearest: away from the half-integer boundaries this
// is the pixel torch's fp32 grid picks.
static constexpr int GEO_ROTATE = 1, GEO_SHIFT = 2, GEO_HFLIP = 4, GEO_VFLIP = 8;

__global__ __launch_bounds__(256) void augment_geometric_kernel(const float* __restrict__ image,
                                                                const float* __restrict__ mask, int S,
                                                                const float* __restrict__ angle_deg,
                                                                const int32_t* __restrict__ shift,
                                                                const int32_t* __restrict__ flags,
                                                                float* __restrict__ image_out,
                                                                float* __restrict__ mask_out) {
  __shared__ double cs[2];
  const int b = blockIdx.y;
  const int f = flags[b];
  if (threadIdx.x == 0 && (f & GEO_ROTATE)) {
    const double t = (double)angle_deg[b] * (M_PI / 180.0);
    cs[0] = cos(t);
    cs[1] = sin(t);
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  const size_t plane = (size_t)S * S;
  if ((size_t)i >= plane) return;
  int y = i / S, x = i - y * S;
  if (f & GEO_VFLIP) y = S - 1 - y;
  if (f & GEO_HFLIP) x = S - 1 - x;
  bool inside = true;
  if (f & GEO_SHIFT) {
    const long xl = (long)x - shift[2 * b], yl = (long)y - shift[2 * b + 1];   // any int32 shift, no overflow
    inside = xl >= 0 && xl < S && yl >= 0 && yl < S;
    x = inside ? (int)xl : 0;
    y = inside ? (int)yl : 0;
  }
  if (inside && (f & GEO_ROTATE)) {
    const double half = 0.5 * S;
    const double xc = x + 0.5 - half, yc = y + 0.5 - half;
    const double xs = rint(cs[0] * xc - cs[1] * yc + half - 0.5);
    const double ys = rint(cs[1] * xc + cs[0] * yc + half - 0.5);
    inside = xs >= 0.0 && xs < (double)S && ys >= 0.0 && ys < (double)S;   // false for NaN as well
    x = inside ? (int)xs : 0;
    y = inside ? (int)ys : 0;
  }
  const size_t src = (size_t)y * S + x;
  const float* ib = image + (size_t)b * 3 * plane;
  float* ob = image_out + (size_t)b * 3 * plane;
#pragma unroll
  for (int c = 0; c < 3; ++c) ob[c * plane + i] = inside ? ib[c * plane + src] : 0.f;
  mask_out[(size_t)b * plane + i] = inside ? mask[(size_t)b * plane + src] : 0.f;
}

void launch_augment_geometric(const float* image, const float* mask, int B, int S, const float* angle_deg,
                              const int32_t* shift, const int32_t* flags, float* image_out, float* mask_out,
                              hipStream_t s) {
  hipLaunchKernelGGL(augment_geometric_kernel, dim3((unsigned)(((size_t)S * S + 255) / 256), B), dim3(256), 0, s, image,
                     mask, S, angle_deg, shift, flags, image_out, mask_out);
}

}  // namespace aaclip

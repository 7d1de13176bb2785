// Heat-map overlays: the frame the model saw, the heat map blended over it and the ground truth blended over it, with
// the contours of the predicted and the true mask, as uint8 RGB panels stacked vertically (the definition and the
// tile geometry: csrc/overlay_plan.h; include/aaclip.h states it for callers).
//
// overlay_kernel is ONE launch: a gather over output pixels with no workspace, no memset and no atomics, so a second
// call gives the same bytes.  A workgroup of 256 threads renders one tile of rows x tw pixels of one image:
//   1. the colour table goes into the LDS once per workgroup, one dword per entry;
//   2. the tile of each mask goes into the LDS with a halo of T pixels (positions outside the image hold 1 and are never
//      looked at: the contour's window is cut to the image);
//   3. every pixel is computed ONCE: its three frame values, its map value and its mask bytes are read once, and the
//      bytes of all selected panels go into the LDS, laid out as the tile's byte runs of the output -- one run per
//      panel where the tile spans the image's width (the rows of a panel follow one another in memory), else one per
//      row -- each run shifted by its global address modulo 4;
//   4. the runs are written out in ALIGNED 16-byte chunks, each assembled from four aligned LDS dwords.  A row of 518
//      pixels is 1554 bytes, so rows are only 2-byte aligned and a panel is H * W * 3 bytes after the one before: no
//      mapping of threads to PIXELS gives aligned stores, a mapping of threads to aligned CHUNKS does for any output
//      pointer.  Only the first and last chunk of a run are partial; they fall back to dword, then byte stores.
// The fp32 steps are separately rounded operations (-ffp-contract=off, and the intrinsics say so again).
#include "common.h"
#include "kernels.h"
#include "metrics_records.h"
#include "overlay_plan.h"

namespace aaclip {

namespace {

AACLIP_DEV int frame_byte(float x, float sd, float mean) {
  return overlay_clamp_byte(rintf(__fmul_rn(__fadd_rn(__fmul_rn(x, sd), mean), 255.0f)));
}

// q = trunc(clamp(n, 0, 1) * 255) with the product rounded toward zero: the product of an fp32 and 255 is exact in
// fp64, and truncating the exact product equals truncating its fp32 value rounded toward zero (integers up to 255 are
// fp32 values, so the rounding never crosses one)
AACLIP_DEV int heat_byte(float x, const RangeNorm& norm) {
  const float n = range_normalised(x, norm);
  if (n != n) return 0;
  const float c = n < 0.0f ? 0.0f : (n > 1.0f ? 1.0f : n);
  return (int)((double)c * 255.0);
}

// contour(M) at tile pixel (r, i) = image pixel (y, x), for a pixel with M != 0; s is the staged tile with its halo
AACLIP_DEV bool contour_at(const unsigned char* s, int halo_w, int T, int r, int i, int y, int x, int H, int W) {
  const OverlayWindow wy = overlay_window(y, H, T), wx = overlay_window(x, W, T);
  for (int yy = wy.lo; yy <= wy.hi; ++yy) {
    const unsigned char* row = s + (yy - y + r + T) * halo_w + (i + T - x);
    for (int xx = wx.lo; xx <= wx.hi; ++xx)
      if (row[xx] == 0) return true;
  }
  return false;
}

AACLIP_DEV void stage_mask(const uint8_t* __restrict__ mask, unsigned char* s, const OverlayGeom& g, long long image, int y0,
                           int x0) {
  const int cells = g.halo_w * g.halo_h;
  for (int h = threadIdx.x; h < cells; h += OVERLAY_THREADS) {
    const int hr = h / g.halo_w, hc = h - hr * g.halo_w;
    const int y = y0 - g.T + hr, x = x0 - g.T + hc;
    s[h] = (y >= 0 && y < g.H && x >= 0 && x < g.W) ? mask[overlay_map_offset(g.H, g.W, image, y, x)] : (unsigned char)1;
  }
}

AACLIP_DEV void put3(unsigned char* p, int r, int g, int b) { p[0] = (unsigned char)r, p[1] = (unsigned char)g, p[2] = (unsigned char)b; }

}  // namespace

__global__ __launch_bounds__(OVERLAY_THREADS) void overlay_kernel(
    const float* __restrict__ frames, const float* __restrict__ maps, const RangeRecord* __restrict__ rec,
    const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, const uint8_t* __restrict__ lut,
    uint8_t* __restrict__ out, OverlayGeom g, int images) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t* s_lut = (uint32_t*)(lds + g.off_lut);
  unsigned char* s_out = lds + g.off_out;
  unsigned char* s_pred = lds + g.off_pred;
  unsigned char* s_truth = lds + g.off_truth;
  const int tid = threadIdx.x;
  for (int e = tid; e < 256; e += OVERLAY_THREADS)
    s_lut[e] = (uint32_t)lut[3 * e] | ((uint32_t)lut[3 * e + 1] << 8) | ((uint32_t)lut[3 * e + 2] << 16);
  const RangeNorm norm = range_norm(rec);
  const int H = g.H, W = g.W, T = g.T, n = g.n_panels, a = g.alpha256;
  const int slot_heat = (int)(g.panels & OVERLAY_FRAME), slot_truth = slot_heat + (int)((g.panels >> 1) & 1u);
  const long long tiles = (long long)g.tiles_x * g.tiles_y;
  const unsigned long long out_addr = (unsigned long long)out;

  for (long long image = blockIdx.y; image < images; image += gridDim.y)
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
      const int ty = (int)(tile / g.tiles_x), tx = (int)(tile - (long long)ty * g.tiles_x);
      const int y0 = ty * g.rows, x0 = tx * g.tw;
      const int nr = H - y0 < g.rows ? H - y0 : g.rows, nc = W - x0 < g.tw ? W - x0 : g.tw;
      __syncthreads();                 // the table is written; the last tile's runs have been read
      if (pred) stage_mask(pred, s_pred, g, image, y0, x0);
      if (truth) stage_mask(truth, s_truth, g, image, y0, x0);
      __syncthreads();

      // the byte offset of run 0 of each panel slot, and its address modulo 4
      long long base[3];
      int mod4[3];
      for (int p = 0; p < n; ++p) {
        base[p] = overlay_out_offset(H, W, n, image, p, y0, x0);
        mod4[p] = (int)((out_addr + (unsigned long long)base[p]) & 3);
      }
      const int row_mod4 = (W & 3) * 3;        // a run per row: the next run starts W * 3 bytes on

      for (int idx = tid; idx < nr * nc; idx += OVERLAY_THREADS) {
        const int r = idx / nc, i = idx - r * nc, y = y0 + r, x = x0 + i;
        int F[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) F[c] = frame_byte(frames[overlay_frame_offset(H, W, image, c, y, x)], g.sd[c], g.mean[c]);
        const int mp = pred ? s_pred[(r + T) * g.halo_w + i + T] : 0;
        const int mt = truth ? s_truth[(r + T) * g.halo_w + i + T] : 0;
        const bool cp = mp != 0 && T > 0 && contour_at(s_pred, g.halo_w, T, r, i, y, x, H, W);
        const int run = g.full ? 0 : r, within = g.full ? idx * 3 : i * 3;
        if (g.panels & OVERLAY_FRAME)
          put3(s_out + run * g.run_stride + ((mod4[0] + run * row_mod4) & 3) + within, F[0], F[1], F[2]);
        if (g.panels & OVERLAY_HEAT) {
          unsigned char* d = s_out + (slot_heat * g.runs + run) * g.run_stride + ((mod4[slot_heat] + run * row_mod4) & 3) + within;
          if (cp) {
            put3(d, g.pred_colour[0], g.pred_colour[1], g.pred_colour[2]);
          } else {
            const uint32_t colour = s_lut[heat_byte(maps[overlay_map_offset(H, W, image, y, x)], norm)];
            put3(d, overlay_blend(a, F[0], (int)(colour & 255)), overlay_blend(a, F[1], (int)((colour >> 8) & 255)),
                 overlay_blend(a, F[2], (int)((colour >> 16) & 255)));
          }
        }
        if (g.panels & OVERLAY_TRUTH) {
          unsigned char* d = s_out + (slot_truth * g.runs + run) * g.run_stride + ((mod4[slot_truth] + run * row_mod4) & 3) + within;
          if (cp)
            put3(d, g.pred_colour[0], g.pred_colour[1], g.pred_colour[2]);
          else if (mt != 0 && T > 0 && contour_at(s_truth, g.halo_w, T, r, i, y, x, H, W))
            put3(d, g.truth_colour[0], g.truth_colour[1], g.truth_colour[2]);
          else if (mt != 0)
            put3(d, overlay_blend(a, F[0], g.truth_colour[0]), overlay_blend(a, F[1], g.truth_colour[1]),
                 overlay_blend(a, F[2], g.truth_colour[2]));
          else
            put3(d, F[0], F[1], F[2]);
        }
      }
      __syncthreads();

      // the runs, in aligned 16-byte chunks
      const int nruns = g.full ? 1 : nr;
      const int run_len = (g.full ? nr : 1) * nc * 3;
      const int chunks = overlay_run_chunks(run_len);
      for (int c = tid; c < n * nruns * chunks; c += OVERLAY_THREADS) {
        const int pr = c / chunks, k = c - pr * chunks;
        const int p = pr / nruns, run = pr - p * nruns;
        const unsigned long long A = out_addr + (unsigned long long)base[p] + (unsigned long long)run * (unsigned long long)W * 3ull;
        const unsigned long long end = A + (unsigned long long)run_len;
        const unsigned long long ca = overlay_chunk_address(A, k);
        if (ca >= end) continue;
        // the LDS byte of global address A is the run's slot + (A & 3): a multiple of 4 in the LDS is one in memory
        const unsigned char* src = s_out + (p * g.runs + run) * g.run_stride + (int)(A & 3) + (long long)(ca - A);
        if (ca >= A && ca + 16 <= end) {
          const uint32_t* w = (const uint32_t*)src;
          *(u32x4*)ca = (u32x4){w[0], w[1], w[2], w[3]};
          continue;
        }
        for (int d = 0; d < 4; ++d) {
          const unsigned long long da = ca + 4ull * (unsigned long long)d;
          if (da >= A && da + 4 <= end) {
            *(uint32_t*)da = *(const uint32_t*)(src + 4 * d);
          } else {
            for (int b = 0; b < 4; ++b)
              if (da + b >= A && da + b < end) *(unsigned char*)(da + b) = src[4 * d + b];
          }
        }
      }
    }
}

void launch_overlay_render(const OverlayGeom& g, int images, const float* frames, const float* maps, const void* range_record,
                           const uint8_t* pred, const uint8_t* truth, const uint8_t* lut, uint8_t* out, hipStream_t s) {
  if ((size_t)g.lds_bytes > OVERLAY_LDS_LIMIT) {
    set_launch_error("overlay: the tile does not fit the LDS");
    return;
  }
  const long long tiles = (long long)g.tiles_x * g.tiles_y;
  const dim3 grid((unsigned)(tiles < (1 << 20) ? tiles : (1 << 20)), (unsigned)(images < 65535 ? images : 65535));
  hipLaunchKernelGGL(overlay_kernel, grid, dim3(OVERLAY_THREADS), (size_t)g.lds_bytes, s, frames, maps,
                     (const RangeRecord*)range_record, pred, truth, lut, out, g, images);
}

}  // namespace aaclip

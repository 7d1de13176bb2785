// Heat-map overlays (csrc/overlay.hip): what the device code, the C ABI's checks and a host program share
// (csrc/overlay_host_check.cpp replays it against brute force under a sanitizer).
//
// B images of H x W pixels.  Inputs: frames fp32 [B, 3, H, W] (the normalised model input), maps fp32 [B, H, W], the
// range record of aaclip_metrics_range or none, pred / truth uint8 [B, H, W] or none, lut uint8 [256, 3].  Output uint8
// [B, n * H, W, 3]: the n selected panels (frame, heat, truth, in that order) stacked vertically.  Per pixel, all in
// integers or in separately rounded fp32 operations (include/aaclip.h states the definition):
//   F[c]   = clamp(rint((x[c] * std[c] + mean[c]) * 255), 0, 255), NaN -> 0
//   q      = trunc(min(max(n, 0), 1) * 255), the product rounded toward zero, NaN -> 0
//   blend  = (alpha256 * u + (256 - alpha256) * v + 128) >> 8
//   contour(M) at (y, x): M != 0 and some pixel INSIDE the image with |dy| <= T, |dx| <= T has M == 0
//
// A workgroup renders one TILE of rows x tw pixels of one image: tw = min(W, OVERLAY_TILE_WIDTH) and as many rows as
// keep the tile within OVERLAY_TILE_PIXELS (at most OVERLAY_TILE_ROWS).  Where tw == W the tile's bytes are ONE
// contiguous run of every panel, otherwise one run per row.  Every offset is 64-bit.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AACLIP_OV_HD __host__ __device__ inline
#else
#define AACLIP_OV_HD inline
#endif

namespace aaclip {

static constexpr unsigned OVERLAY_FRAME = 1u, OVERLAY_HEAT = 2u, OVERLAY_TRUTH = 4u, OVERLAY_ALL = 7u;
static constexpr int OVERLAY_MAX_THICKNESS = 8;
static constexpr int OVERLAY_TILE_WIDTH = 1024, OVERLAY_TILE_PIXELS = 2048, OVERLAY_TILE_ROWS = 64;
static constexpr int OVERLAY_THREADS = 256;
static constexpr int OVERLAY_LUT_BYTES = 1024;                  // 256 entries of 4 bytes in the LDS
static constexpr size_t OVERLAY_LDS_LIMIT = 64 * 1024;
// the largest pixel count images * H * W: 12 bytes of frame per pixel stay far inside 64 bits
static constexpr long long OVERLAY_MAX_PIXELS = 1ll << 56;

AACLIP_OV_HD int overlay_panel_count(unsigned panels) { return (int)((panels & 1u) + ((panels >> 1) & 1u) + ((panels >> 2) & 1u)); }

// nullptr, or why the plan is refused.  images == 0 passes (the entry then launches nothing).
inline const char* overlay_plan_check(int images, int H, int W, unsigned panels, int alpha256, int thickness,
                                      const float* std3) {
  if (images < 0) return "images must not be negative";
  if (H < 1) return "height must be at least 1";
  if (W < 1) return "width must be at least 1";
  if (panels == 0 || (panels & ~OVERLAY_ALL)) return "panels must select at least one of frame (1), heat (2), truth (4)";
  if (alpha256 < 0 || alpha256 > 256) return "alpha256 must be in 0 .. 256";
  if (thickness < 0 || thickness > OVERLAY_MAX_THICKNESS) return "thickness must be in 0 .. 8";
  for (int c = 0; c < 3; ++c)
    if (!(std3[c] > 0.0f) || !(std3[c] <= 3.402823466e+38f)) return "std must be positive and finite";
  const long long plane = (long long)H * W;                     // below 2^62
  if (plane > OVERLAY_MAX_PIXELS || (images > 0 && plane > OVERLAY_MAX_PIXELS / images)) return "the tensors are too large";
  return nullptr;
}

struct OverlayGeom {
  int H, W, T, tw, rows;          // image, contour reach, tile width and rows
  int tiles_x, tiles_y;
  unsigned panels;
  int n_panels;
  int alpha256;
  int full;                       // tw == W: a tile's bytes are one run per panel
  int runs, run_stride;           // runs per panel of a tile, and the LDS bytes reserved for each (a multiple of 4)
  int halo_w, halo_h;             // the staged mask tile: (rows + 2T) x (tw + 2T)
  int off_lut, off_out, off_pred, off_truth, lds_bytes;
  unsigned char pred_colour[3], truth_colour[3];
  float mean[3], sd[3];         // the normalisation that the frame byte undoes
};

inline OverlayGeom overlay_geom(int H, int W, unsigned panels, int alpha256, int T, bool has_pred, bool has_truth) {
  OverlayGeom g = {};
  g.H = H, g.W = W, g.T = T, g.panels = panels, g.n_panels = overlay_panel_count(panels), g.alpha256 = alpha256;
  g.tw = W < OVERLAY_TILE_WIDTH ? W : OVERLAY_TILE_WIDTH;
  int rows = OVERLAY_TILE_PIXELS / g.tw;
  if (rows > OVERLAY_TILE_ROWS) rows = OVERLAY_TILE_ROWS;
  if (rows > H) rows = H;
  g.rows = rows;
  g.tiles_x = (int)(((long long)W + g.tw - 1) / g.tw);
  g.tiles_y = (int)(((long long)H + rows - 1) / rows);
  g.full = g.tw == W;
  g.runs = g.full ? 1 : rows;
  const int run_bytes = (g.full ? rows : 1) * g.tw * 3;
  g.run_stride = ((run_bytes + 3) & ~3) + 4;                    // + the run's address modulo 4 in front
  g.halo_w = g.tw + 2 * T, g.halo_h = rows + 2 * T;
  const int halo = (g.halo_w * g.halo_h + 3) & ~3;
  g.off_lut = 0;
  g.off_out = OVERLAY_LUT_BYTES;
  g.off_pred = g.off_out + g.n_panels * g.runs * g.run_stride;
  g.off_truth = g.off_pred + (has_pred ? halo : 0);
  g.lds_bytes = g.off_truth + (has_truth ? halo : 0);
  return g;
}

// ---- the integer pixel functions
AACLIP_OV_HD int overlay_blend(int alpha256, int u, int v) { return (alpha256 * u + (256 - alpha256) * v + 128) >> 8; }

// a rounded fp32 value -> a byte: NaN and anything below 0 give 0, anything above 255 gives 255
AACLIP_OV_HD int overlay_clamp_byte(float v) {
  if (!(v >= 0.0f)) return 0;
  return v > 255.0f ? 255 : (int)v;
}

// the window of contour(M) at coordinate p of an axis of n pixels: [lo, hi] inside the image
struct OverlayWindow {
  int lo, hi;
};
AACLIP_OV_HD OverlayWindow overlay_window(int p, int n, int T) {
  OverlayWindow w;
  w.lo = p - T < 0 ? 0 : p - T;
  w.hi = p + T > n - 1 ? n - 1 : p + T;
  return w;
}

// ---- a run of `len` output bytes at address A is written in aligned 16-byte chunks: chunk k starts at
// overlay_chunk_address(A, k), k < overlay_run_chunks(len); an unaligned run touches at most one chunk more than an
// aligned one, and a chunk that starts at or past A + len does not exist
AACLIP_OV_HD int overlay_run_chunks(int len) { return (len + 15) / 16 + 1; }
AACLIP_OV_HD unsigned long long overlay_chunk_address(unsigned long long A, int k) {
  return (A & ~15ull) + 16ull * (unsigned long long)k;
}

// ---- 64-bit offsets
AACLIP_OV_HD long long overlay_frame_offset(int H, int W, long long image, int c, int y, int x) {   // in floats
  return ((image * 3 + c) * H + y) * (long long)W + x;
}
AACLIP_OV_HD long long overlay_map_offset(int H, int W, long long image, int y, int x) {            // floats or mask bytes
  return (image * H + y) * (long long)W + x;
}
// in bytes: panel slot p (0 .. n_panels - 1) of an image
AACLIP_OV_HD long long overlay_out_offset(int H, int W, int n_panels, long long image, int p, int y, int x) {
  return (((image * n_panels + p) * H + y) * (long long)W + x) * 3;
}

#if defined(__HIPCC__)
// one launch on s; the plan has passed overlay_plan_check and images >= 1
void launch_overlay_render(const OverlayGeom& g, int images, const float* frames, const float* maps, const void* range_record,
                           const uint8_t* pred, const uint8_t* truth, const uint8_t* lut, uint8_t* out, hipStream_t s);
#endif

}  // namespace aaclip

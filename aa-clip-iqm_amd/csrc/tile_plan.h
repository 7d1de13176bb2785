// Tiled inference (csrc/tiles.hip): the geometry that the device code, the C ABI's checks and a host program share
// (csrc/tile_host_check.cpp replays it against brute force under a sanitizer).
//
// S the tile side, G >= 1 tiles per side, 0 <= O <= S / 2 pixels of overlap, stride T = S - O >= 1, canvas side
// C = S + (G - 1) * T.  Tile t = i * G + j covers canvas rows [i * T, i * T + S) and columns [j * T, j * T + S).
// Because O <= S / 2 (so 2 * T >= S) a canvas coordinate lies in at most 2 tiles per axis: tile_cover gives the first
// and the count.  The blend weight of a tile at (y, x) is w1(y) * w1(x), w1(u) = min(u + 1, S - u): across an overlap
// the two 1-D weights add up to O + 1 (a linear cross-fade).  The 1-D weights are integers; their product and the sums
// are taken in fp32, exact while S <= 4096 (4 * (S / 2)^2 < 2^24).
//
// Layouts: canvas fp32 [images, channels, C, C]; tiles fp32 [images * G * G, channels, S, S].  Every offset is 64-bit.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AACLIP_TP_HD __host__ __device__ inline
#else
#define AACLIP_TP_HD inline
#endif

namespace aaclip {

struct TileGeom {
  int S, G, O, T, C, channels;
};

// C, or -1 for a geometry that is refused (S < 1, G < 1, O outside [0, S / 2], C above INT_MAX)
inline long tile_canvas_side(int S, int G, int O) {
  if (S < 1 || G < 1 || O < 0 || O > S / 2) return -1;
  const long long c = (long long)S + (long long)(G - 1) * (long long)(S - O);
  return c > (long long)INT_MAX ? -1 : (long)c;
}

// the largest element count either tensor may have: its byte size stays far inside 64 bits
static constexpr long long TILE_MAX_ELEMENTS = 1ll << 59;
// the planes of either tensor (images * G * G * channels, images * channels) are walked with 32-bit indices
static constexpr long long TILE_MAX_PLANES = (long long)INT_MAX;

// nullptr, or why the plan is refused.  images == 0 passes (the entries then launch nothing).
inline const char* tile_plan_check(int images, int channels, int S, int G, int O) {
  if (images < 0) return "images must not be negative";
  if (channels < 1) return "channels must be at least 1";
  if (S < 1) return "tile must be at least 1";
  if (G < 1) return "grid must be at least 1";
  if (O < 0 || O > S / 2) return "overlap must be in 0 .. tile / 2";
  const long C = tile_canvas_side(S, G, O);
  if (C < 0) return "the canvas side overflows int";
  const long long g2 = (long long)G * G;                 // G < 2^31: below 2^62
  const long long img_ch = (long long)images * channels;   // below 2^62
  if (img_ch > TILE_MAX_PLANES || g2 > TILE_MAX_PLANES || img_ch * g2 > TILE_MAX_PLANES)
    return "images * grid^2 * channels must stay below 2^31";
  const long long tile_plane = (long long)S * S, canvas_plane = (long long)C * C;      // each below 2^62
  if (img_ch > 0 && (tile_plane > TILE_MAX_ELEMENTS / (img_ch * g2) || canvas_plane > TILE_MAX_ELEMENTS / img_ch))
    return "the tensors are too large";
  return nullptr;
}

inline TileGeom tile_geom(int channels, int S, int G, int O) {
  TileGeom g;
  g.S = S, g.G = G, g.O = O, g.T = S - O, g.C = (int)tile_canvas_side(S, G, O), g.channels = channels;
  return g;
}

AACLIP_TP_HD int tile_w1(int u, int S) { return u + 1 < S - u ? u + 1 : S - u; }

// the tiles i (along one axis) with i * T <= p < i * T + S, 0 <= i < G, for a canvas coordinate 0 <= p < C:
// i = lo .. lo + n - 1, n = 1 or 2
struct TileCover {
  int lo, n;
};
AACLIP_TP_HD TileCover tile_cover(int p, int S, int G, int T) {
  int hi = p / T;
  if (hi > G - 1) hi = G - 1;
  TileCover c;
  c.lo = p < S ? 0 : (p - S) / T + 1;
  c.n = hi - c.lo + 1;
  return c;
}

// element offsets (in floats)
AACLIP_TP_HD long long tile_offset(const TileGeom& g, long long image, int t, int c, int y, int x) {
  return (((image * g.G * g.G + t) * g.channels + c) * g.S + y) * (long long)g.S + x;
}
AACLIP_TP_HD long long canvas_offset(const TileGeom& g, long long image, int c, int Y, int X) {
  return ((image * g.channels + c) * g.C + Y) * (long long)g.C + X;
}

// floats per vector access: rows of both tensors start on a multiple of V floats when V divides S and T (hence C) and
// both base pointers are V * 4 byte aligned; a tile's columns then start on multiples of V in the canvas too, and the
// V pixels of a vector share their covering tiles (every cover boundary j * T, j * T + S is a multiple of V)
inline int tile_vector_width(int S, int T, const void* a, const void* b) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b;
  if (S % 4 == 0 && T % 4 == 0 && (bits & 15) == 0) return 4;
  if (S % 2 == 0 && T % 2 == 0 && (bits & 7) == 0) return 2;
  return 1;
}

#if defined(__HIPCC__)
// one launch each on s; the plan has passed tile_plan_check and images >= 1
void launch_tile_gather(const TileGeom& g, int images, const float* canvas, float* tiles, hipStream_t s);
void launch_tile_stitch(const TileGeom& g, int images, const float* tiles, float* canvas, hipStream_t s);
#endif

}  // namespace aaclip

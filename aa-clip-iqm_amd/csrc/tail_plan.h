// Split fp16 residual products (out_proj, c_proj) whose 256 x 256 tiles do not fill the last round of the walking kernel
// (gemm256t.hip): the row split that runs the LayerNorm after the product beside that partial round.  Shared by the
// launcher, the kernel and a host program (csrc/tail_host_check.cpp replays it against brute force under a sanitizer).
//
// `grid` workgroups (one per CU, a multiple of 8) walk tiles_m x tiles_n tiles.  full_rounds = tiles / grid rounds are
// full; they cover the first r0 = full_rounds * (grid / tiles_n) * 256 rows.  Launch A is the product on rows [0, r0).
// Launch B is ONE launch of `grid` workgroups: workgroup indices below `span` are tile slots, the tail tiles (rows >= r0)
// in them, every other workgroup is a LayerNorm worker on rows [0, r0), which launch A has completed.  The launch
// boundary between A and B is the only synchronisation.
//
// Slots: workgroup w runs on XCD w % 8.  The tn tiles of one row tile share their A rows, so with xs = 8 a row tile's
// tiles sit in slots of ONE XCD: slot w = xcd + xs * (k * tiles_n + tn) holds tile (row tile k * xs + xcd, tn); slots whose
// row tile does not exist are holes and run LayerNorm rows like the workgroups past `span`.  Where that span does not fit
// the grid (small planning grids), xs = 1: slot w = row tile * tiles_n + tn, no holes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AACLIP_TL_HD __host__ __device__ inline
#else
#define AACLIP_TL_HD inline
#endif

namespace aaclip {

struct TailPlan {
  int engaged;          // 0: the product keeps its single launch (the other fields then describe why not)
  int grid, tiles_n, tiles_m, full_rounds;
  long r0;              // rows of launch A (a multiple of 256)
  int tail_row_tiles;   // row tiles of rows [r0, M)
  int tail_tiles;       // tail_row_tiles * tiles_n
  int xs, span, holes;  // slot geometry (above)
  int ln_workers;       // grid - tail_tiles = (grid - span) + holes
};

// the part of the plan the kernel needs
struct TailSlots {
  int xs, tiles_n, tail_row_tiles, span, holes, grid;
};

// M rows, N columns (a multiple of 256), grid = workgroups the walking kernel is launched with
inline TailPlan tail_plan(long M, int N, int grid) {
  TailPlan t = {};
  t.grid = grid;
  if (M <= 0 || N <= 0 || N % 256 != 0 || grid < 8 || grid % 8 != 0 || M > (1L << 38)) return t;
  t.tiles_n = N / 256;
  t.tiles_m = (int)((M + 255) / 256);
  if (grid % t.tiles_n != 0) return t;   // a round must be a whole number of row tiles
  const long tiles = (long)t.tiles_m * t.tiles_n;
  t.full_rounds = (int)(tiles / grid);
  t.r0 = (long)t.full_rounds * (grid / t.tiles_n) * 256;
  t.tail_row_tiles = t.tiles_m - (int)(t.r0 / 256);
  t.tail_tiles = t.tail_row_tiles * t.tiles_n;
  if (t.full_rounds < 2 || t.tail_tiles <= 0 || t.tail_tiles > grid / 2) return t;
  const int span8 = 8 * t.tiles_n * ((t.tail_row_tiles + 7) / 8);
  t.xs = span8 <= grid ? 8 : 1;
  t.span = t.xs == 8 ? span8 : t.tail_tiles;
  t.holes = t.span - t.tail_tiles;
  t.ln_workers = grid - t.tail_tiles;
  t.engaged = 1;
  return t;
}

inline TailSlots tail_slots(const TailPlan& t) {
  TailSlots s = {t.xs, t.tiles_n, t.tail_row_tiles, t.span, t.holes, t.grid};
  return s;
}

// workgroup w < span: its tile (row tile counted from r0, column tile), or false for a hole
AACLIP_TL_HD bool tail_slot_tile(const TailSlots& s, int w, int& row_tile, int& tn) {
  const int xcd = w % s.xs, q = w / s.xs;
  tn = q % s.tiles_n;
  row_tile = (q / s.tiles_n) * s.xs + xcd;
  return row_tile < s.tail_row_tiles;
}

// the LayerNorm worker index (0 .. ln_workers - 1) of a workgroup that runs no tile: the workgroups past the span first,
// then the holes (all in the last group of xs row tiles) in slot order per column tile
AACLIP_TL_HD int tail_ln_worker(const TailSlots& s, int w) {
  if (w >= s.span) return w - s.span;
  const int rem = s.tail_row_tiles % s.xs;   // != 0 where holes exist
  const int xcd = w % s.xs, tn = (w / s.xs) % s.tiles_n;
  return (s.grid - s.span) + tn * (s.xs - rem) + (xcd - rem);
}

// byte ranges [a, a + an) and [b, b + bn)
inline bool tail_ranges_disjoint(uintptr_t a, uint64_t an, uintptr_t b, uint64_t bn) {
  return an == 0 || bn == 0 || a + an <= b || b + bn <= a;
}

// What launch B touches, as byte ranges: its LayerNorm workers READ rows [0, r0) of the product's output `out` (fp32,
// ldc floats per row) and WRITE rows [0, r0) of `ln_out` (split8 rows of 4 * D bytes); its tiles READ rows [r0, M) of A
// (lda halves per row) and of the residual, and WRITE rows [r0, M) of `out`.  True when no write meets another access.
inline bool tail_rows_disjoint(long M, long r0, int D, uintptr_t A, long lda, uintptr_t out, long ldc, uintptr_t resid,
                               uintptr_t ln_out) {
  const uint64_t ln_bytes = (uint64_t)r0 * 4 * (uint64_t)D;
  const uint64_t tail = (uint64_t)(M - r0);
  const uintptr_t a_tail = A + (uint64_t)r0 * lda * 2, o_tail = out + (uint64_t)r0 * ldc * 4;
  const uintptr_t r_tail = resid ? resid + (uint64_t)r0 * ldc * 4 : o_tail;
  return tail_ranges_disjoint(ln_out, ln_bytes, a_tail, tail * lda * 2) &&      // LayerNorm rows vs the tiles' A rows
         tail_ranges_disjoint(ln_out, ln_bytes, o_tail, tail * ldc * 4) &&      // ... vs the rows the tiles write
         tail_ranges_disjoint(ln_out, ln_bytes, r_tail, tail * ldc * 4) &&      // ... vs the residual rows they read
         tail_ranges_disjoint(ln_out, ln_bytes, out, (uint64_t)r0 * ldc * 4) && // ... vs the rows the LayerNorm reads
         tail_ranges_disjoint(out, (uint64_t)r0 * ldc * 4, o_tail, tail * ldc * 4);
}

}  // namespace aaclip

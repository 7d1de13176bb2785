// csrc/tail_plan.h as gemm256t.hip uses it, in a host program of its own (built with ASan + UBSan by
// tests/test_tail_overlap_cpu.py): r0, the tail tile count and the engagement rule against brute force over row counts,
// widths and grids; the slots of launch B as a bijection onto the tail tiles with a row tile's tiles on one XCD; the
// LayerNorm worker indices as a permutation; the row disjointness check on the block path's buffers and on overlapping
// ones.  Prints "ok <checks>" and returns 0, or says what differs and returns 1.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <vector>

#include "tail_plan.h"

using namespace aaclip;

static long g_checks = 0;
#define CHECK(cond, ...)              \
  do {                                \
    ++g_checks;                       \
    if (!(cond)) {                    \
      fprintf(stderr, __VA_ARGS__);   \
      fprintf(stderr, "\n");          \
      return 1;                       \
    }                                 \
  } while (0)

static int plan_case(long M, int N, int grid) {
  const TailPlan t = tail_plan(M, N, grid);
  const int tiles_n = N / 256;
  // brute force: deal the tiles out round by round
  long tiles = 0;
  for (long r = 0; r < M; r += 256) tiles += tiles_n;
  long left = tiles;
  int rounds = 0;
  while (left >= grid) { left -= grid; ++rounds; }
  const bool want = grid % tiles_n == 0 && rounds >= 2 && left > 0 && 2 * left <= grid;
  CHECK((t.engaged != 0) == want, "engaged(%ld, %d, %d) = %d, want %d", M, N, grid, t.engaged, (int)want);
  if (!t.engaged) return 0;
  CHECK(t.full_rounds == rounds && t.tail_tiles == left, "rounds / tail of (%ld, %d, %d): %d / %d, want %d / %ld", M, N, grid,
        t.full_rounds, t.tail_tiles, rounds, left);
  CHECK(t.r0 % 256 == 0 && t.r0 > 0 && t.r0 < M, "r0 of (%ld, %d, %d) = %ld", M, N, grid, t.r0);
  CHECK((t.r0 / 256) * tiles_n == (long)rounds * grid, "launch A of (%ld, %d, %d) is not %d full rounds", M, N, grid, rounds);
  CHECK(t.r0 + 256L * t.tail_row_tiles >= M && t.r0 + 256L * (t.tail_row_tiles - 1) < M, "tail rows of (%ld, %d, %d)", M, N, grid);
  CHECK(t.span <= grid && t.span - t.holes == t.tail_tiles && t.ln_workers == grid - t.tail_tiles && t.ln_workers >= grid / 2,
        "slot counts of (%ld, %d, %d): span %d holes %d", M, N, grid, t.span, t.holes);
  CHECK(t.xs == 8 || t.xs == 1, "xs of (%ld, %d, %d) = %d", M, N, grid, t.xs);
  const TailSlots s = tail_slots(t);
  std::vector<int> tile_seen((size_t)t.tail_tiles, 0), worker_seen((size_t)t.ln_workers, 0), xcd_of((size_t)t.tail_row_tiles, -1);
  for (int w = 0; w < grid; ++w) {
    int rt = -1, tn = -1;
    if (w < s.span && tail_slot_tile(s, w, rt, tn)) {
      CHECK(rt >= 0 && rt < t.tail_row_tiles && tn >= 0 && tn < tiles_n, "slot %d of (%ld, %d, %d): tile (%d, %d)", w, M, N, grid, rt, tn);
      CHECK(tile_seen[(size_t)rt * tiles_n + tn]++ == 0, "tile (%d, %d) of (%ld, %d, %d) twice", rt, tn, M, N, grid);
      if (t.xs == 8) {
        CHECK(xcd_of[rt] < 0 || xcd_of[rt] == w % 8, "row tile %d of (%ld, %d, %d) on two XCDs", rt, M, N, grid);
        xcd_of[rt] = w % 8;
      }
    } else {
      const int id = tail_ln_worker(s, w);
      CHECK(id >= 0 && id < t.ln_workers, "worker index %d of workgroup %d of (%ld, %d, %d)", id, w, M, N, grid);
      CHECK(worker_seen[id]++ == 0, "worker index %d of (%ld, %d, %d) twice", id, M, N, grid);
    }
  }
  for (int v : tile_seen) CHECK(v == 1, "a tail tile of (%ld, %d, %d) has no slot", M, N, grid);
  for (int v : worker_seen) CHECK(v == 1, "a worker index of (%ld, %d, %d) is unused", M, N, grid);
  return 0;
}

int main() {
  for (int grid : {8, 16, 32, 64, 104, 256, 304})
    for (int N : {256, 512, 768, 1024})
      for (long M = 1; M <= 3L * grid * 256 + 700; M += (M % 256 == 0 || M % 256 == 255 || M % 256 == 1) ? 1 : 127)
        if (plan_case(M, N, grid)) return 1;
  for (long M : {87680L, 81920L, 5760L, 4096L, 4097L, 4225L, 18480L, 1L << 26})
    for (int N : {256, 1024})
      for (int grid : {8, 256})
        if (plan_case(M, N, grid)) return 1;
  {  // the tower at batch 64: 1372 tiles on 256 CUs
    const TailPlan t = tail_plan(87680, 1024, 256);
    CHECK(t.engaged && t.full_rounds == 5 && t.r0 == 81920 && t.tail_row_tiles == 23 && t.tail_tiles == 92 && t.xs == 8 &&
              t.span == 96 && t.holes == 4 && t.ln_workers == 164, "tower plan: r0 %ld tail %d span %d", t.r0, t.tail_tiles, t.span);
  }
  {  // the test shapes on a planning grid of 8: one tail tile; a tail of grid / 2; an exact number of rounds
    TailPlan t = tail_plan(4097, 256, 8);
    CHECK(t.engaged && t.r0 == 4096 && t.tail_tiles == 1 && t.xs == 8 && t.span == 8 && t.holes == 7, "4097 x 256 on 8");
    t = tail_plan(4225, 1024, 8);
    CHECK(t.engaged && t.r0 == 4096 && t.tail_tiles == 4 && t.xs == 1 && t.span == 4 && t.holes == 0, "4225 x 1024 on 8");
    t = tail_plan(4096, 256, 8);
    CHECK(!t.engaged && t.tail_tiles == 0, "4096 x 256 on 8 engages");
    CHECK(!tail_plan(4096, 1024, 8).engaged && !tail_plan(2049, 256, 8).engaged, "exact rounds / one round engage");
    CHECK(!tail_plan(4097, 768, 8).engaged, "a grid that is no multiple of tiles_n engages");
    CHECK(!tail_plan(0, 256, 8).engaged && !tail_plan(4097, 200, 8).engaged && !tail_plan(4097, 256, 12).engaged, "bad arguments engage");
  }
  {  // disjointness on the block path's buffers (D = 1024, M = 87680, r0 = 81920): narrow holds ctx rows and takes the LayerNorm rows
    const long M = 87680, r0 = 81920;
    const int D = 1024;
    const uintptr_t narrow = 0x7f0000000000ull, big = narrow + (uintptr_t)M * 4 * D, x = 0x7e0000000000ull, x_in = 0x7d0000000000ull;
    CHECK(tail_rows_disjoint(M, r0, D, narrow, 2 * D, x, D, 0, narrow), "out_proj in place");
    CHECK(tail_rows_disjoint(M, r0, D, narrow, 2 * D, x, D, x_in, narrow), "out_proj with a residual buffer");
    CHECK(tail_rows_disjoint(M, r0, D, big, 2 * 4 * D, x, D, 0, narrow), "c_proj");
    CHECK(!tail_rows_disjoint(M, r0, D, narrow, 2 * D, x, D, 0, narrow + 4096), "LayerNorm rows shifted into the tiles' A rows");
    CHECK(!tail_rows_disjoint(M, r0, D, narrow, 2 * D, x, D, 0, x), "LayerNorm rows over the product's output");
    CHECK(!tail_rows_disjoint(M, r0, D, big, 2 * 4 * D, x, D, narrow - 4096, narrow), "LayerNorm rows over the residual rows the tiles read");
    CHECK(!tail_rows_disjoint(M, r0, D, big, 2 * 4 * D, x, D, 0, x + (uintptr_t)r0 * 4 * D - 16), "LayerNorm rows into the tail rows of x");
    CHECK(tail_ranges_disjoint(16, 16, 32, 16) && !tail_ranges_disjoint(16, 17, 32, 16) && tail_ranges_disjoint(16, 0, 0, 64), "ranges");
  }
  printf("ok %ld\n", g_checks);
  return 0;
}

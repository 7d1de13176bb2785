// csrc/tile_plan.h as tiles.hip and the C ABI use it, in a host program of its own (built with ASan + UBSan by
// tests/test_tiled_cpu.py): the canvas side, the covering tiles of every canvas coordinate, the weights and their sums,
// the offsets of both layouts at an image count whose byte offsets pass 2^32 and 2^40, the vector width, and the refusal
// of every bad plan -- each against brute force.  Prints "ok <checks>" and returns 0, or says what differs and returns 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "tile_plan.h"

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

static int geometry_case(int S, int G, int O) {
  const long side = tile_canvas_side(S, G, O);
  const int T = S - O;
  // brute force: the last tile ends where the canvas ends
  long want = 0;
  for (int i = 0; i < G; ++i) want = (long)i * T + S;
  CHECK(side == want, "canvas side of (%d, %d, %d): %ld, want %ld", S, G, O, side, want);
  CHECK(tile_plan_check(1, 1, S, G, O) == nullptr, "plan (%d, %d, %d) refused", S, G, O);
  const TileGeom g = tile_geom(3, S, G, O);
  CHECK(g.S == S && g.G == G && g.O == O && g.T == T && g.C == side && g.channels == 3, "tile_geom of (%d, %d, %d)", S, G, O);
  const int C = (int)side;
  for (int p = 0; p < C; ++p) {
    int lo = -1, n = 0;
    for (int i = 0; i < G; ++i)
      if ((long)i * T <= p && p < (long)i * T + S) {
        if (lo < 0) lo = i;
        CHECK(i == lo + n, "covering tiles of %d in (%d, %d, %d) are not consecutive", p, S, G, O);
        ++n;
      }
    const TileCover c = tile_cover(p, S, G, T);
    CHECK(c.lo == lo && c.n == n && n >= 1 && n <= 2, "cover of %d in (%d, %d, %d): (%d, %d), want (%d, %d)", p, S, G, O, c.lo,
          c.n, lo, n);
    // the weights: positive integers, symmetric, and across an overlap they add up to O + 1
    int sum = 0;
    for (int i = c.lo; i < c.lo + c.n; ++i) {
      const int u = p - i * T, w = tile_w1(u, S);
      int brute = u + 1;
      if (S - u < brute) brute = S - u;
      CHECK(w == brute && w >= 1 && w == tile_w1(S - 1 - u, S), "w1(%d) at S = %d", u, S);
      sum += w;
    }
    if (n == 2) CHECK(sum == O + 1, "overlap weights at %d in (%d, %d, %d) add up to %d, want %d", p, S, G, O, sum, O + 1);
    // 2-D: at most 4 tiles, and the largest weight sum (this 1-D sum squared) is an exact fp32 integer below 2^24
    if (S <= 4096) {
      const float f = (float)sum * (float)sum;
      CHECK((double)f == (double)sum * (double)sum && (double)sum * (double)sum < 16777216.0, "2-D weight sum at %d", p);
    }
  }
  // every tile pixel lands on the canvas exactly where the offsets say
  for (int t = 0; t < G * G; ++t) {
    const int i = t / G, j = t % G;
    for (int y : {0, S / 2, S - 1})
      for (int x : {0, S / 2, S - 1}) {
        const int Y = i * T + y, X = j * T + x;
        CHECK(Y >= 0 && Y < C && X >= 0 && X < C, "tile %d pixel (%d, %d) leaves the canvas of (%d, %d, %d)", t, y, x, S, G, O);
        const TileCover r = tile_cover(Y, S, G, T), c = tile_cover(X, S, G, T);
        CHECK(r.lo <= i && i < r.lo + r.n && c.lo <= j && j < c.lo + c.n, "tile %d is not in the cover of its own pixel", t);
      }
  }
  return 0;
}

static int offsets_case(int S, int G, int O, int channels, long long images) {
  const TileGeom g = tile_geom(channels, S, G, O);
  const long long C = g.C, G2 = (long long)G * G;
  // against the nested-array definition, in 128-bit arithmetic
  const long long b = images - 1;
  for (int t : {0, (int)G2 - 1})
    for (int c : {0, channels - 1})
      for (int y : {0, S - 1})
        for (int x : {0, S - 1}) {
          const __int128 want = ((((__int128)b * G2 + t) * channels + c) * S + y) * S + x;
          const long long got = tile_offset(g, b, t, c, y, x);
          CHECK((__int128)got == want, "tile offset of image %lld tile %d", b, t);
          CHECK(got >= 0 && (__int128)got < (__int128)images * G2 * channels * S * S, "tile offset out of the tensor");
          const int i = t / G, j = t % G, Y = i * g.T + y, X = j * g.T + x;
          const __int128 cwant = (((__int128)b * channels + c) * C + Y) * C + X;
          const long long cgot = canvas_offset(g, b, c, Y, X);
          CHECK((__int128)cgot == cwant, "canvas offset of image %lld", b);
          CHECK(cgot >= 0 && (__int128)cgot < (__int128)images * channels * C * C, "canvas offset out of the tensor");
        }
  // the last element of each tensor is the last offset
  CHECK(tile_offset(g, b, (int)G2 - 1, channels - 1, S - 1, S - 1) + 1 == images * G2 * channels * S * S, "last tile element");
  CHECK(canvas_offset(g, b, channels - 1, (int)C - 1, (int)C - 1) + 1 == images * channels * C * C, "last canvas element");
  return 0;
}

int main() {
  // geometry against brute force: no overlap, the largest overlap of odd and even sides, overlap 1, one tile, S = 1
  const int cases[][3] = {{5, 1, 0},   {5, 2, 0},   {5, 2, 2},    {5, 3, 1},     {14, 3, 7},   {37, 2, 18}, {37, 3, 1},
                          {70, 2, 14}, {1, 1, 0},   {1, 7, 0},    {2, 5, 1},     {3, 4, 1},    {518, 2, 112}, {518, 3, 112},
                          {518, 4, 259}, {64, 9, 32}, {4096, 2, 2048}};
  for (const auto& c : cases)
    if (geometry_case(c[0], c[1], c[2])) return 1;
  for (int S = 1; S <= 12; ++S)
    for (int G = 1; G <= 4; ++G)
      for (int O = 0; O <= S / 2; ++O)
        if (geometry_case(S, G, O)) return 1;
  CHECK(tile_canvas_side(518, 2, 112) == 924 && tile_canvas_side(518, 3, 112) == 1330 && tile_canvas_side(70, 2, 14) == 126,
        "canvas sides of the working sizes");

  // 64-bit offsets: 170 frames x 9 tiles x 3 channels x 518^2 x 4 bytes passes 2^32; larger counts pass 2^40 elements
  if (offsets_case(518, 3, 112, 1, 170)) return 1;
  if (offsets_case(518, 3, 112, 3, 170)) return 1;
  if (offsets_case(518, 2, 112, 3, 100000)) return 1;
  if (offsets_case(5, 3, 1, 2, 3)) return 1;
  if (offsets_case(4096, 8, 0, 1, 1 << 20)) return 1;
  CHECK((long long)170 * 9 * 3 * 518 * 518 * 4 > (1ll << 32), "the working size is past 4 GiB");
  CHECK(tile_plan_check(170, 1, 518, 3, 112) == nullptr && tile_plan_check(100000, 3, 518, 2, 112) == nullptr &&
            tile_plan_check(1 << 20, 1, 4096, 8, 0) == nullptr, "large plans refused");

  // refusals: each bad field on its own, and the sizes that would overflow
  CHECK(tile_plan_check(0, 1, 5, 2, 1) == nullptr, "images == 0 passes");
  CHECK(tile_plan_check(-1, 1, 5, 2, 1) != nullptr, "images < 0");
  CHECK(tile_plan_check(1, 0, 5, 2, 1) != nullptr && tile_plan_check(1, -3, 5, 2, 1) != nullptr, "channels < 1");
  CHECK(tile_plan_check(1, 1, 0, 2, 0) != nullptr && tile_plan_check(1, 1, -5, 2, 0) != nullptr, "tile < 1");
  CHECK(tile_plan_check(1, 1, 5, 0, 1) != nullptr && tile_plan_check(1, 1, 5, -1, 1) != nullptr, "grid < 1");
  CHECK(tile_plan_check(1, 1, 5, 2, -1) != nullptr && tile_plan_check(1, 1, 5, 2, 3) != nullptr &&
            tile_plan_check(1, 1, 6, 2, 4) != nullptr && tile_plan_check(1, 1, 6, 2, 3) == nullptr, "overlap outside 0 .. tile / 2");
  CHECK(tile_canvas_side(0, 1, 0) < 0 && tile_canvas_side(5, 0, 0) < 0 && tile_canvas_side(5, 2, -1) < 0 &&
            tile_canvas_side(5, 2, 3) < 0, "tile_canvas_side refuses what the plan check refuses");
  CHECK(tile_canvas_side(INT_MAX, 1, 0) == INT_MAX && tile_canvas_side(INT_MAX, 2, 0) < 0 &&
            tile_canvas_side(1 << 20, 1 << 11, 0) < 0 && tile_canvas_side(1 << 20, (1 << 11) - 1, 0) == 2146435072l &&
            tile_canvas_side(2, INT_MAX, 1) < 0 && tile_canvas_side(2, INT_MAX - 1, 1) == INT_MAX,
        "the canvas side at the edge of int");
  CHECK(tile_plan_check(1, 1, INT_MAX, 2, 0) != nullptr && tile_plan_check(1, 1, 2, INT_MAX, 1) != nullptr, "canvas overflow");
  CHECK(tile_plan_check(INT_MAX, 2, 5, 1, 0) != nullptr && tile_plan_check(1 << 20, 1, 5, 1 << 6, 0) != nullptr &&
            tile_plan_check(INT_MAX, 1, 5, 1, 0) == nullptr, "too many planes");
  CHECK(tile_plan_check(INT_MAX, 1, 1 << 15, 1, 0) != nullptr && tile_plan_check(1, 1, INT_MAX, 1, 0) != nullptr &&
            tile_plan_check(1 << 10, 1, 1 << 24, 1, 0) == nullptr, "tensors too large");

  // vector width: what divides S and T, limited by the pointers' alignment
  char* base = (char*)0x1000;
  CHECK(tile_vector_width(72, 56, base, base + 16) == 4 && tile_vector_width(72, 56, base, base + 8) == 2 &&
            tile_vector_width(72, 56, base + 4, base) == 1, "vector width by alignment");
  CHECK(tile_vector_width(518, 406, base, base) == 2 && tile_vector_width(70, 56, base, base) == 2 &&
            tile_vector_width(72, 58, base, base) == 2 && tile_vector_width(37, 19, base, base) == 1 &&
            tile_vector_width(14, 7, base, base) == 1 && tile_vector_width(5, 4, base, base) == 1, "vector width by the sides");
  for (const auto& c : cases) {
    const int S = c[0], G = c[1], T = c[0] - c[2], V = tile_vector_width(S, T, base, base);
    const int C = (int)tile_canvas_side(S, G, c[2]);
    CHECK(S % V == 0 && T % V == 0 && C % V == 0, "vector width %d does not divide the sides of (%d, %d, %d)", V, S, G, c[2]);
    for (int X = 0; X < C; X += V) {     // the pixels of a vector share their cover and stay inside each covering tile
      const TileCover first = tile_cover(X, S, G, T);
      for (int e = 1; e < V; ++e) {
        const TileCover other = tile_cover(X + e, S, G, T);
        CHECK(other.lo == first.lo && other.n == first.n, "a vector at %d straddles a cover boundary", X);
      }
      for (int j = first.lo; j < first.lo + first.n; ++j)
        CHECK(X - j * T >= 0 && X - j * T + V <= S && (X - j * T) % V == 0, "a vector at %d leaves tile %d", X, j);
    }
  }
  printf("ok %ld checks\n", g_checks);
  return 0;
}

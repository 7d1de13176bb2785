// Host check of bootstrap_plan.h, a program of its own (built with -fsanitize=address,undefined by
// tests/test_bootstrap_cpu.py): the decomposition that bootstrap.hip runs -- weighted sums per tile, their exclusive
// prefix, a record per (tile, replicate), the fold over the tiles -- written out per replicate with the header's own
// functions and compared with a brute-force loop over the tie groups of the whole array.
//   num, P, N must be equal; ap within 1e-10.
// Sizes around 1, 2 and 3 tiles +- 1; score kinds: every element its own group, 40 levels, one tie group longer than two
// tiles (a tile without a start), groups that straddle every tile boundary; images of weight 0 in every replicate.
#include "bootstrap_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace aaclip;

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

struct Case {
  std::vector<uint32_t> keys, payload;   // ascending keys, image << 1 | label
  long images;
};

// kind 0: distinct keys; 1: 40 levels; 2: a constant run over two and a half tiles placed across boundaries;
// 3: groups of 4096 shifted by half a tile: every group straddles a tile boundary, every tile has one start
static Case make_case(long n, int kind, long images) {
  Case c;
  c.images = images;
  c.keys.resize(n);
  c.payload.resize(n);
  for (long i = 0; i < n; ++i) {
    uint32_t k;
    if (kind == 0) k = (uint32_t)i * 3u + 7u;
    else if (kind == 1) k = (uint32_t)(i * 40 / n);
    else if (kind == 2) k = i < 1000 ? (uint32_t)i : (i < 1000 + 10240 ? 1000u : (uint32_t)(i - 10240));
    else k = (uint32_t)((i + BOOT_TILE / 2) / BOOT_TILE);
    c.keys[i] = k;
    const uint32_t image = rnd() % (uint32_t)images;
    const uint32_t label = (image & 1u) && (rnd() % 3u == 0u) ? 1u : 0u;
    c.payload[i] = (image << 1) | label;
  }
  return c;
}

static BootRecord brute(const Case& c, const std::vector<uint8_t>& w) {
  const long n = (long)c.keys.size();
  uint32_t P = 0, Mtot = 0;
  for (long i = 0; i < n; ++i) {
    const uint32_t wt = w[c.payload[i] >> 1];
    Mtot += wt;
    if (c.payload[i] & 1u) P += wt;
  }
  const uint32_t N = Mtot - P;
  if (P == 0 || N == 0) return BootRecord{0ull, P, N, 0.0};
  uint64_t num = 0;
  double ap = 0.0;
  uint32_t E = 0, M = 0;
  long i = 0;
  while (i < n) {
    long i2 = i;
    uint32_t E2 = E, M2 = M;
    while (i2 < n && c.keys[i2] == c.keys[i]) {
      const uint32_t wt = w[c.payload[i2] >> 1];
      M2 += wt;
      if (c.payload[i2] & 1u) E2 += wt;
      ++i2;
    }
    const uint64_t tp = P - E, fp = (Mtot - M) - tp, tp0 = P - E2, fp0 = (Mtot - M2) - tp0;
    num += (fp - fp0) * (tp + tp0);
    if (tp != tp0) ap += ((double)(tp - tp0) / (double)P) * ((double)tp / (double)(tp + fp));
    i = i2, E = E2, M = M2;
  }
  return BootRecord{num, P, N, ap};
}

// what the four kernels do for one replicate
static BootRecord tiled(const Case& c, const std::vector<uint8_t>& w) {
  const long n = (long)c.keys.size(), tiles = boot_tiles(n);
  std::vector<uint32_t> sumE(tiles, 0u), sumM(tiles, 0u), starts(tiles, 0u);
  for (long t = 0; t < tiles; ++t)                                   // pass 1
    for (long i = t * BOOT_TILE; i < n && i < (t + 1) * BOOT_TILE; ++i) {
      const uint32_t wt = w[c.payload[i] >> 1];
      sumM[t] += wt;
      if (c.payload[i] & 1u) sumE[t] += wt;
      if (i == 0 || c.keys[i - 1] != c.keys[i]) ++starts[t];
    }
  uint32_t P = 0, Mtot = 0;                                          // scan
  for (long t = 0; t < tiles; ++t) {
    const uint32_t e = sumE[t], m = sumM[t];
    sumE[t] = P, sumM[t] = Mtot;
    P += e, Mtot += m;
  }
  std::vector<BootTileRecord> rec(tiles);
  for (long t = 0; t < tiles; ++t) {                                 // pass 2
    uint32_t E = sumE[t], M = sumM[t], Ef = 0, Mf = 0, Ep = 0, Mp = 0;
    uint64_t num = 0;
    double ap = 0.0;
    bool have = false;
    for (long i = t * BOOT_TILE; i < n && i < (t + 1) * BOOT_TILE; ++i) {
      if (i == 0 || c.keys[i - 1] != c.keys[i]) {
        if (have) boot_close_group(P, Mtot, Ep, Mp, E, M, num, ap);   // P == 0: no group has a positive, nothing divides
        else Ef = E, Mf = M;
        have = true, Ep = E, Mp = M;
      }
      const uint32_t wt = w[c.payload[i] >> 1];
      M += wt;
      if (c.payload[i] & 1u) E += wt;
    }
    rec[t] = BootTileRecord{Ef, Mf, Ep, Mp, num, ap};
    if (have != (starts[t] != 0)) {
      printf("FAIL start count of tile %ld\n", t);
      exit(1);
    }
  }
  BootFold f = boot_fold_begin();                                    // fold
  for (long t = 0; t < tiles; ++t)
    if (starts[t]) boot_fold_tile(f, rec[t], P, Mtot);
  return boot_fold_end(f, P, Mtot);
}

int main() {
  static_assert(sizeof(BootRecord) == 32 && sizeof(BootTileRecord) == 32, "record sizes are part of the ABI / workspace");
  const long sizes[] = {1, 2, 63, BOOT_TILE - 1, BOOT_TILE, BOOT_TILE + 1, 2 * BOOT_TILE - 1, 2 * BOOT_TILE,
                        2 * BOOT_TILE + 1, 3 * BOOT_TILE - 1, 3 * BOOT_TILE, 3 * BOOT_TILE + 1, 12305};
  long checked = 0;
  double worst = 0.0;
  for (long n : sizes)
    for (int kind = 0; kind < 4; ++kind) {
      const long images = 23;
      const Case c = make_case(n, kind, images);
      for (int r = 0; r < 12; ++r) {
        std::vector<uint8_t> w(images);
        for (long i = 0; i < images; ++i) w[i] = (uint8_t)(rnd() % 4u);          // weight 0 for about a quarter
        if (r == 0) for (long i = 0; i < images; ++i) w[i] = 1;                    // the unweighted curve
        if (r == 1) for (long i = 0; i < images; ++i) w[i] = (i & 1) ? 0 : 2;      // no positive: invalid
        if (r == 2) for (long i = 0; i < images; ++i) w[i] = i == 3 ? 23 : 0;      // one image only
        if (r == 3) for (long i = 0; i < images; ++i) w[i] = i < 20 ? 0 : 255;     // the largest count
        const BootRecord a = brute(c, w), b = tiled(c, w);
        const double d = std::fabs(a.ap - b.ap);
        if (a.num != b.num || a.P != b.P || a.N != b.N || !(d <= 1e-10)) {
          printf("FAIL n %ld kind %d replicate %d: num %llu / %llu, P %llu / %llu, N %llu / %llu, ap %.17g / %.17g\n", n,
                 kind, r, (unsigned long long)a.num, (unsigned long long)b.num, (unsigned long long)a.P,
                 (unsigned long long)b.P, (unsigned long long)a.N, (unsigned long long)b.N, a.ap, b.ap);
          return 1;
        }
        worst = d > worst ? d : worst;
        ++checked;
      }
    }
  // the layout: sections in order, 256-byte aligned, no growth with R beyond the chunk
  const BootLayout l1 = boot_layout(45615080L, 1000), l2 = boot_layout(45615080L, 100000);
  if (l1.bytes != l2.bytes || l1.bytes >= ((size_t)1 << 30) || (l1.totals | l1.starts | l1.records | l1.bytes) % 256 ||
      !(l1.sums < l1.totals && l1.totals < l1.starts && l1.starts < l1.records && l1.records < l1.bytes) ||
      boot_layout(1, 1).bytes == 0 || boot_layout(12305, 65).bytes <= boot_layout(12305, 64).bytes) {
    printf("FAIL layout\n");
    return 1;
  }
  printf("ok %ld replicates, worst |d ap| %.3g, workspace at 45.6 M x 1000: %zu bytes\n", checked, worst, l1.bytes);
  return 0;
}

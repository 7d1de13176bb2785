// csrc/support_pack.h as support.hip uses it, in a host program of its own (built with ASan + UBSan by
// tests/test_support_cpu.py): candidates are packed, merged per chunk and across chunks in several chunk orders, decoded,
// and compared with a sequential scan that keeps the first of the equal maxima.  Covers negative cosines, -0.0 / +0.0,
// equal cosines at different indices, the extreme indices, the key's order and round trip, the chunk plan and the
// workspace layout.  Prints "ok <checks>" and returns 0, or says what differs and returns 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "support_pack.h"

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

static uint32_t bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

// the definition: a scan in index order, "strictly greater" replaces (so -0.0 and +0.0 tie and the first stays)
static void scan(const std::vector<float>& cosines, float* best, uint32_t* row) {
  *best = cosines[0], *row = 0;
  for (size_t j = 1; j < cosines.size(); ++j)
    if (cosines[j] > *best) *best = cosines[j], *row = (uint32_t)j;
}

static int merge_case(const std::vector<float>& cosines, uint32_t first_row, const char* what) {
  const size_t n = cosines.size();
  float want;
  uint32_t want_row;
  scan(cosines, &want, &want_row);
  if (want == 0.0f) want = 0.0f;   // the decode gives +0.0 for either zero
  for (size_t chunk : {(size_t)1, (size_t)3, (size_t)128, n}) {
    const size_t chunks = (n + chunk - 1) / chunk;
    std::vector<unsigned long long> partial(chunks, 0ull);
    for (size_t c = 0; c < chunks; ++c)
      for (size_t j = c * chunk; j < std::min(n, (c + 1) * chunk); ++j)
        partial[c] = support_merge(partial[c], support_pack(cosines[j], first_row + (uint32_t)j));
    std::vector<size_t> order(chunks);
    for (size_t c = 0; c < chunks; ++c) order[c] = c;
    for (int pass = 0; pass < 4; ++pass) {
      if (pass == 1) std::reverse(order.begin(), order.end());
      if (pass == 2) std::rotate(order.begin(), order.begin() + chunks / 2, order.end());
      if (pass == 3)
        for (size_t c = 0; c + 1 < chunks; c += 2) std::swap(order[c], order[c + 1]);
      unsigned long long word = 0ull;   // the workspace word starts at 0 = "no candidate"
      for (size_t c : order) word = support_merge(word, partial[c]);
      CHECK(word != 0ull, "%s: a merged word of 0", what);
      const float got = support_word_cos(word);
      const uint32_t got_row = support_word_row(word);
      CHECK(bits(got) == bits(want) && got_row == first_row + want_row,
            "%s chunk %zu pass %d: got (%.9g, %u), want (%.9g, %u)", what, chunk, pass, got, got_row, want,
            first_row + want_row);
    }
  }
  return 0;
}

int main() {
  // the key preserves the order of the floats, both zeros share one key, and it decodes to the float it came from
  const float ladder[] = {-INFINITY, -3.4e38f, -1.0f, -0.9f, -1e-30f, -1e-45f, -0.0f, 0.0f, 1e-45f, 1e-30f,
                          0.5f,      0.9999999f, 1.0f, 1.0000001f, 3.4e38f, INFINITY};
  const int L = (int)(sizeof(ladder) / sizeof(ladder[0]));
  for (int a = 0; a < L; ++a) {
    const uint32_t ka = support_cos_key(ladder[a]);
    CHECK(ka != 0u || ladder[a] != ladder[a], "a finite cosine with key 0");
    const float back = support_key_cos(ka);
    CHECK(back == ladder[a] && (ladder[a] == 0.0f ? bits(back) == 0u : bits(back) == bits(ladder[a])), "key round trip of %g",
          ladder[a]);
    for (int b = 0; b < L; ++b) {
      const uint32_t kb = support_cos_key(ladder[b]);
      CHECK((ladder[a] < ladder[b]) == (ka < kb) && (ladder[a] == ladder[b]) == (ka == kb), "key order of %g and %g",
            ladder[a], ladder[b]);
    }
  }
  // the extreme indices: row 0 beats row 2^32 - 2 at equal cosines, and every word of a finite cosine is non-zero
  for (float v : {-1.0f, -0.0f, 0.0f, 1.0f}) {
    const unsigned long long lo = support_pack(v, 0u), hi = support_pack(v, 0xFFFFFFFEu), top = support_pack(v, 0x7FFFFFFFu);
    CHECK(lo > top && top > hi && hi != 0ull, "index order at cosine %g", v);
    CHECK(support_word_row(lo) == 0u && support_word_row(hi) == 0xFFFFFFFEu && support_word_row(top) == 0x7FFFFFFFu, "row decode");
    CHECK(support_merge(hi, lo) == lo && support_merge(lo, hi) == lo, "merge is the maximum");
  }
  CHECK(support_pack(-0.0f, 5u) == support_pack(0.0f, 5u), "the zeros pack alike");
  CHECK(support_pack(-1.0f, 0u) < support_pack(-0.99f, 0xFFFFFFFEu), "a larger cosine beats any index");

  // merges against the scan
  uint32_t state = 12345u;
  auto rnd = [&]() {
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) / 16777216.0f;
  };
  for (size_t n : {(size_t)1, (size_t)2, (size_t)127, (size_t)130, (size_t)2738}) {
    std::vector<float> v(n);
    for (auto& x : v) x = 2.0f * rnd() - 1.0f;
    if (merge_case(v, 0u, "random")) return 1;
    for (auto& x : v) x = -0.9f - 0.05f * rnd();          // all negative: a missing candidate (0) must not win
    if (merge_case(v, 0u, "negative")) return 1;
    if (merge_case(v, 0xFFFFFFFEu - (uint32_t)n, "negative at the top of the index range")) return 1;
    for (size_t j = 0; j < n; ++j) v[j] = (j % 3 == 0) ? -0.0f : 0.0f;     // zeros of both signs: the first row wins
    if (merge_case(v, 0u, "signed zeros")) return 1;
    for (size_t j = 0; j < n; ++j) v[j] = (j % 2) ? 0.0f : -0.0f;
    if (merge_case(v, 7u, "signed zeros, -0.0 first")) return 1;
    for (size_t j = 0; j < n; ++j) v[j] = 0.25f * (float)(j % 5);          // equal maxima at several rows
    if (merge_case(v, 0u, "equal maxima")) return 1;
    for (auto& x : v) x = -0.5f;                                           // all equal
    if (merge_case(v, 3u, "all equal")) return 1;
    if (n > 8) {                                                           // duplicates j and j + 7, first and last
      for (auto& x : v) x = 2.0f * rnd() - 1.0f;
      v[0] = v[7] = v[n - 1] = 1.5f;
      if (merge_case(v, 0u, "duplicates")) return 1;
    }
  }

  // the plan covers every bank tile exactly once, and the workspace holds one word per row
  for (long M : {1L, 17L, 129L, 1369L, 87616L, 5000000L})
    for (long N : {1L, 127L, 128L, 129L, 2738L, 5476L, 43808L, 175232L}) {
      const SupportPlan p = support_plan(M, N);
      CHECK(p.row_tiles * SUPPORT_TILE >= M && (p.row_tiles - 1) * SUPPORT_TILE < M, "row tiles of M = %ld", M);
      CHECK(p.bank_tiles * SUPPORT_TILE >= N && (p.bank_tiles - 1) * SUPPORT_TILE < N, "bank tiles of N = %ld", N);
      CHECK(p.chunks >= 1 && p.tiles_per_chunk >= 1 && p.chunks * p.tiles_per_chunk >= p.bank_tiles &&
                (p.chunks - 1) * p.tiles_per_chunk < p.bank_tiles && p.chunks <= 65535,
            "chunks of M = %ld, N = %ld: %ld x %ld for %ld tiles", M, N, p.chunks, p.tiles_per_chunk, p.bank_tiles);
      const SupportLayout l = support_layout(M);
      CHECK(l.words == 0 && l.bytes >= (size_t)M * 8 && l.bytes % 256 == 0 && l.bytes < (size_t)M * 8 + 256, "layout of M = %ld", M);
    }
  printf("ok %ld checks\n", g_checks);
  return 0;
}

// csrc/coreset_pack.h as coreset.hip uses it, in a host program of its own (built with ASan + UBSan by
// tests/test_coreset_cpu.py): the quantiser against a double-precision rounding written here, the candidate word's
// order, decode and merge in shuffled orders against a sequential scan, and the whole selection replayed the way the
// device runs it -- rows dealt to workgroups by the launch plan, one candidate per workgroup, the workgroups merged in
// shuffled orders into word t + 1 -- against a plain int64 loop written here.  Also the plan and the workspace layout.
// Prints "ok <checks>" and returns 0, or says what differs and returns 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "coreset_pack.h"

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

static uint32_t g_state = 2463534242u;
static uint32_t rnd_u32() {
  g_state = g_state * 1664525u + 1013904223u;
  return g_state;
}
static float rnd_unit() { return (float)(rnd_u32() >> 8) / 8388608.0f - 1.0f; }   // [-1, 1)

// the quantiser's definition in double: v * 2^14 is exact there too, nearbyint is round-half-even
static int plain_quantise(float v) {
  if (v != v) return 0;
  double x = nearbyint((double)v * 16384.0);
  if (x > 32767.0) x = 32767.0;
  if (x < -32767.0) x = -32767.0;
  return (int)x;
}

// the selection's definition: int64 arithmetic, a scan that keeps the first of the equal maxima
static void plain_select(const std::vector<int16_t>& q, long N, int E, long n, long start, std::vector<long>& picks,
                         std::vector<long long>& radius2, std::vector<long long>& min_d2) {
  std::vector<long long> norm2(N);
  for (long i = 0; i < N; ++i) {
    long long s = 0;
    for (int k = 0; k < E; ++k) s += (long long)q[i * E + k] * q[i * E + k];
    norm2[i] = s;
  }
  min_d2.assign(N, 0xFFFFFFFFll);
  radius2.assign(n + 1, 0xFFFFFFFFll);
  picks.assign(n, start);
  long c = start;
  for (long t = 0; t < n; ++t) {
    long far = 0;
    for (long i = 0; i < N; ++i) {
      long long dot = 0;
      for (int k = 0; k < E; ++k) dot += (long long)q[i * E + k] * q[c * E + k];
      const long long d2 = norm2[i] + norm2[c] - 2 * dot;
      if (d2 < min_d2[i]) min_d2[i] = d2;
      if (min_d2[i] > min_d2[far]) far = i;
    }
    radius2[t + 1] = min_d2[far];
    if (t + 1 < n) picks[t + 1] = far;
    c = far;
  }
}

// the device's way: quantise with the header, deal the row groups to workgroups by the plan, fold each workgroup's
// rows, merge the workgroups in the order `shuffle` names, decode
static int replay_case(const std::vector<float>& rows, long N, int E, long n, long start, const char* what) {
  std::vector<int16_t> q((size_t)N * E);
  std::vector<int32_t> norm2(N);
  for (long i = 0; i < N; ++i) {
    norm2[i] = coreset_quantise_row(&rows[(size_t)i * E], E, &q[(size_t)i * E]);
    CHECK(norm2[i] >= 0 && (uint32_t)norm2[i] < CORESET_NORM2_LIMIT, "%s: norm2 of row %ld is %d", what, i, norm2[i]);
    for (int k = 0; k < E; ++k)
      CHECK(q[(size_t)i * E + k] == plain_quantise(rows[(size_t)i * E + k]), "%s: quantiser at row %ld, %d", what, i, k);
  }
  std::vector<long> want_picks;
  std::vector<long long> want_radius2, want_min;
  plain_select(q, N, E, n, start, want_picks, want_radius2, want_min);

  const CoresetPlan p = coreset_plan(N, E);
  const CoresetLayout lay = coreset_layout(n);
  CHECK(lay.bytes >= (size_t)(n + 1) * 8 && lay.words == 0, "%s: layout", what);
  for (int shuffle = 0; shuffle < 3; ++shuffle) {
    std::vector<unsigned long long> words(lay.bytes / 8, 0ull);   // the one memset
    std::vector<uint32_t> min_d2(N, 0x12345678u);                 // garbage: launch 0 must not read it
    for (long t = 0; t < n; ++t) {
      const uint32_t centre = t == 0 ? (uint32_t)start : coreset_word_row(words[t]);
      CHECK((long)centre < N, "%s: centre %u of pick %ld outside the bank", what, centre, t);
      std::vector<unsigned long long> wg(p.workgroups, 0ull);
      const long stride = p.workgroups * CORESET_WAVES;
      for (long g = 0; g < p.groups; ++g) {
        const long b = (g % stride) / CORESET_WAVES;   // the workgroup whose wave walks group g
        for (int s = 0; s < p.rows_per_wave; ++s) {
          const long i = g * p.rows_per_wave + s;
          if (i >= N) continue;
          const int32_t dot = coreset_dot(&q[(size_t)i * E], &q[(size_t)centre * E], E);
          const uint32_t d2 = coreset_d2(norm2[i], norm2[centre], dot);
          const uint32_t old = t == 0 ? CORESET_D2_INIT : min_d2[i];
          const uint32_t now = d2 < old ? d2 : old;
          min_d2[i] = now;
          wg[b] = coreset_merge(wg[b], coreset_word(now, (uint32_t)i));
        }
      }
      std::vector<long> order(p.workgroups);
      for (long b = 0; b < p.workgroups; ++b) order[b] = b;
      if (shuffle == 1) std::reverse(order.begin(), order.end());
      if (shuffle == 2)
        for (long b = p.workgroups - 1; b > 0; --b) std::swap(order[b], order[rnd_u32() % (uint32_t)(b + 1)]);
      for (long b : order) {
        CHECK(wg[b] != 0ull, "%s: workgroup %ld of %ld has no candidate", what, b, p.workgroups);
        words[t + 1] = coreset_merge(words[t + 1], wg[b]);
      }
    }
    for (long t = 0; t <= n; ++t) {
      const long long r2 = t == 0 ? (long long)CORESET_D2_INIT : (long long)coreset_word_d2(words[t]);
      CHECK(r2 == want_radius2[t], "%s shuffle %d: radius2[%ld] = %lld, want %lld", what, shuffle, t, r2, want_radius2[t]);
      if (t < n) {
        const long pk = t == 0 ? start : (long)coreset_word_row(words[t]);
        CHECK(pk == want_picks[t], "%s shuffle %d: pick[%ld] = %ld, want %ld", what, shuffle, t, pk, want_picks[t]);
      }
      CHECK(t == 0 || want_radius2[t] <= want_radius2[t - 1], "%s: radius2 increases at %ld", what, t);
    }
    for (long i = 0; i < N; ++i)
      CHECK((long long)min_d2[i] == want_min[i], "%s shuffle %d: min_d2[%ld] = %u, want %lld", what, shuffle, i, min_d2[i], want_min[i]);
  }
  return 0;
}

static void unit_rows(std::vector<float>& rows, long N, int E) {
  for (long i = 0; i < N; ++i) {
    double s = 0;
    for (int k = 0; k < E; ++k) s += (double)rows[(size_t)i * E + k] * rows[(size_t)i * E + k];
    const double r = s > 0 ? 1.0 / sqrt(s) : 0.0;
    for (int k = 0; k < E; ++k) rows[(size_t)i * E + k] = (float)(rows[(size_t)i * E + k] * r);
  }
}

int main() {
  // ---- the quantiser: half-way values of both parities, the clamp, the zeros, denormals, non-finite values
  {
    std::vector<float> v = {0.0f, -0.0f, 1.0f, -1.0f, 2.0f, -2.0f, 1.99993896484375f, -1.99993896484375f, 1e-45f, -1e-45f,
                            1e-39f, 3.4e38f, -3.4e38f, INFINITY, -INFINITY, NAN, 3.0517578125e-05f, -3.0517578125e-05f,
                            6.103515625e-05f, 0.999969482421875f};
    for (int k = -40; k <= 40; ++k) v.push_back(((float)k + 0.5f) / 16384.0f);               // k + 0.5: ties
    for (int k = 32760; k <= 32770; ++k) v.push_back(((float)k + 0.5f) / 16384.0f), v.push_back(-((float)k + 0.5f) / 16384.0f);
    for (int i = 0; i < 20000; ++i) v.push_back(2.2f * rnd_unit());
    for (float x : v) {
      const int got = coreset_quantise(x), want = plain_quantise(x);
      CHECK(got == want && got >= -32767 && got <= 32767, "quantise(%.9g) = %d, want %d", x, got, want);
    }
    CHECK(coreset_quantise(0.5f / 16384.0f) == 0 && coreset_quantise(1.5f / 16384.0f) == 2 &&
              coreset_quantise(2.5f / 16384.0f) == 2 && coreset_quantise(-0.5f / 16384.0f) == 0 &&
              coreset_quantise(-1.5f / 16384.0f) == -2,
          "ties go to the even neighbour");
    CHECK(coreset_quantise(2.0f) == 32767 && coreset_quantise(-2.0f) == -32767 && coreset_quantise(1.0f) == 16384, "clamp");
    std::vector<float> big(1024, 2.0f);
    std::vector<int16_t> qb(1024);
    CHECK(coreset_quantise_row(big.data(), 1024, qb.data()) == 0x7FFFFFFF, "norm2 saturates");
    CHECK(coreset_quantise_row(big.data(), 1, qb.data()) == 32767 * 32767, "norm2 of one clamped component");
  }

  // ---- the candidate word: order, decode, extremes
  {
    const uint32_t d2s[] = {0u, 1u, 0x3FFFFFFFu, 0x40000000u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    const uint32_t rows[] = {0u, 1u, 2737u, 0x7FFFFFFEu};
    for (uint32_t a : d2s)
      for (uint32_t ra : rows) {
        const unsigned long long wa = coreset_word(a, ra);
        CHECK(wa != 0ull && coreset_word_d2(wa) == a && coreset_word_row(wa) == ra, "word round trip of (%u, %u)", a, ra);
        for (uint32_t b : d2s)
          for (uint32_t rb : rows) {
            const unsigned long long wb = coreset_word(b, rb);
            const bool a_wins = a > b || (a == b && ra < rb);
            CHECK((wa > wb) == a_wins && (wa == wb) == (a == b && ra == rb), "word order of (%u, %u) and (%u, %u)", a, ra, b, rb);
            CHECK(coreset_merge(wa, wb) == (wa > wb ? wa : wb) && coreset_merge(wa, wb) == coreset_merge(wb, wa), "merge");
          }
      }
    // merges in shuffled orders against a scan
    for (size_t n : {(size_t)1, (size_t)2, (size_t)63, (size_t)130, (size_t)2738}) {
      std::vector<uint32_t> d(n);
      for (int kind = 0; kind < 3; ++kind) {
        for (size_t i = 0; i < n; ++i) d[i] = kind == 0 ? rnd_u32() : kind == 1 ? (uint32_t)(i % 5) * 1000u : 0u;
        size_t far = 0;
        for (size_t i = 1; i < n; ++i)
          if (d[i] > d[far]) far = i;
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; ++i) order[i] = i;
        for (int pass = 0; pass < 3; ++pass) {
          if (pass == 1) std::reverse(order.begin(), order.end());
          if (pass == 2)
            for (size_t i = n - 1; i > 0; --i) std::swap(order[i], order[rnd_u32() % (uint32_t)(i + 1)]);
          unsigned long long w = 0ull;
          for (size_t i : order) w = coreset_merge(w, coreset_word(d[i], (uint32_t)i));
          CHECK(coreset_word_d2(w) == d[far] && coreset_word_row(w) == far, "merge of %zu kind %d pass %d", n, kind, pass);
        }
      }
    }
  }

  // ---- d2 at its extremes: antipodal unit rows reach 2^30, identical rows 0
  {
    CHECK(coreset_d2(1 << 28, 1 << 28, -(1 << 28)) == (1u << 30), "antipodal d2");
    CHECK(coreset_d2(1 << 28, 1 << 28, 1 << 28) == 0u, "d2 of equal rows");
    CHECK(coreset_d2((1 << 29) - 1, (1 << 29) - 1, -((1 << 29) - 1)) == 4u * ((1u << 29) - 1u), "largest d2 under the precondition");
  }

  // ---- the whole selection
  for (int E : {32, 96, 128, 768}) {
    for (long N : {1L, 2L, 65L, 257L}) {
      if (N > 65 && E > 96) continue;   // the wide rows on the smaller banks: the program stays at a second or two
      std::vector<float> rows((size_t)N * E);
      for (auto& x : rows) x = rnd_unit();
      unit_rows(rows, N, E);
      for (long n : {1L, 2L, (N + 9) / 10, N}) {
        if (n < 1 || n > N) continue;
        if (replay_case(rows, N, E, n, 0, "random")) return 1;
        if (N > 2 && replay_case(rows, N, E, n, N / 2, "random, interior start")) return 1;
      }
    }
    // duplicates: 5 distinct rows, 4 copies of each; radius 0 after 5 picks, then row 0 again and again
    {
      const long N = 20;
      std::vector<float> base((size_t)5 * E), rows((size_t)N * E);
      for (auto& x : base) x = rnd_unit();
      unit_rows(base, 5, E);
      for (long i = 0; i < N; ++i) std::copy(base.begin() + (i % 5) * E, base.begin() + (i % 5 + 1) * E, rows.begin() + i * E);
      if (replay_case(rows, N, E, N, 0, "duplicates")) return 1;
      if (replay_case(rows, N, E, 7, 13, "duplicates, interior start")) return 1;
    }
    // ties: the signed basis vectors; antipodal pairs reach d2 = 2^30
    {
      const long N = 2 * E;
      std::vector<float> rows((size_t)N * E, 0.0f);
      for (long i = 0; i < N; ++i) rows[(size_t)i * E + i / 2] = (i % 2) ? -1.0f : 1.0f;
      if (replay_case(rows, N, E, N < 48 ? N : 48, 0, "ties")) return 1;
      if (replay_case(rows, N, E, 9, 5, "ties, interior start")) return 1;
    }
  }

  // ---- the plan covers every row once with at most two chunks per lane, and the layout holds n + 1 words
  for (int E = 32; E <= 1024; E += 32)
    for (long N : {1L, 2L, 63L, 64L, 65L, 2738L, 5476L, 286121L, 0x7FFFFFFFL}) {
      const CoresetPlan p = coreset_plan(N, E);
      const int chunks = E / 8;
      CHECK(p.lanes == (1 << p.lanes_log2) && p.lanes >= 4 && p.lanes <= 64 && p.lanes <= chunks && 2 * p.lanes >= chunks &&
                (2 * p.lanes > chunks || p.lanes == 64),
            "lanes of E = %d: %d", E, p.lanes);
      CHECK(p.rows_per_wave * p.lanes == 64 && p.groups * p.rows_per_wave >= N && (p.groups - 1) * p.rows_per_wave < N,
            "groups of N = %ld, E = %d", N, E);
      CHECK(p.workgroups >= 1 && p.workgroups <= CORESET_MAX_WORKGROUPS && p.workgroups * CORESET_WAVES * CORESET_UNROLL <= p.groups + CORESET_WAVES * CORESET_UNROLL - 1,
            "workgroups of N = %ld, E = %d: %ld", N, E, p.workgroups);
    }
  for (long n : {1L, 2L, 31L, 32L, 274L, 28613L, 0x7FFFFFFFL}) {
    const CoresetLayout l = coreset_layout(n);
    CHECK(l.words == 0 && l.bytes >= (size_t)(n + 1) * 8 && l.bytes % 256 == 0 && l.bytes < (size_t)(n + 1) * 8 + 256, "layout of n = %ld", n);
  }
  printf("ok %ld checks\n", g_checks);
  return 0;
}

// csrc/png_plan.h as png.hip and the C ABI use it, in a host program of its own (built with ASan + UBSan by
// tests/test_png_cpu.py).  encode_image below runs the header's encoder on the host, in the kernels' order of steps;
// everything it is compared with is written here a second time, naively: the filters by PNG's text, the tokens by a
// sequential parse at every run length from 1 to 600, the length symbols by the table of RFC 1951, the code builder by
// the Kraft sum and the limits, the Adler combination by the byte loop, the streams by a small inflate that decodes
// them back to the filtered bytes, the plan's refusals, geometry and 64-bit offsets by arithmetic in a wider type.
// Prints "ok <checks>" and returns 0, or says what differs and returns 1.
//   png_host_check encode H W C pixels.raw streams.bin    writes the zlib streams of the images in pixels.raw, each
//   after its length as 8 little-endian bytes (the tests compare them with forward_utils.png_encode_host)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "png_plan.h"

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

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

// ---- the header's encoder, on the host
struct Segment {
  std::vector<uint8_t> bytes;
  uint32_t s1, s2, n;
  int limited;
  bool stored;
};

static Segment encode_segment(const uint8_t* f, int n) {
  Segment out;
  std::vector<int> start(n), length(n);
  for (int i = 0; i < n; ++i) start[i] = (i == 0 || f[i] != f[i - 1]) ? i : start[i - 1];
  for (int i = n - 1; i >= 0; --i) length[i] = (i == n - 1 || f[i + 1] != f[i]) ? i + 1 - start[i] : length[i + 1];
  uint32_t hist[PNG_LITLEN] = {0};
  int has_match = 0;
  uint64_t s1 = 0, s2 = 0;
  for (int i = 0; i < n; ++i) {
    const PngRole r = png_token_role(i - start[i], length[i]);
    if (r.kind == 1) ++hist[f[i]];
    if (r.kind == 2) ++hist[png_length_symbol(r.length).symbol], has_match = 1;
    s1 += f[i], s2 += (uint64_t)(n - i) * f[i];
  }
  ++hist[256];
  static PngTree tree;
  static PngHeader header;
  uint8_t len[PNG_LITLEN + 2] = {0};
  uint16_t code[PNG_LITLEN];
  out.limited = png_build_lengths(hist, PNG_LITLEN, PNG_LIMIT, len, tree);
  png_canonical_codes(len, PNG_LITLEN, code);
  uint32_t pos = png_block_header(len, has_match, header, tree, nullptr);
  uint32_t bits = pos;
  for (int i = 0; i < n; ++i) {
    const PngRole r = png_token_role(i - start[i], length[i]);
    if (r.kind == 1) bits += len[f[i]];
    if (r.kind == 2) {
      const PngLength l = png_length_symbol(r.length);
      bits += len[l.symbol] + l.extra_bits + 1;
    }
  }
  const uint32_t body = (bits + len[256] + 3 + 7) >> 3, size = body + 4;
  out.stored = !(size < (uint32_t)(n + PNG_STORED_EXTRA));
  out.s1 = (uint32_t)s1, out.s2 = (uint32_t)(s2 % PNG_ADLER_MOD), out.n = (uint32_t)n;
  if (out.stored) {
    out.bytes = {0, (uint8_t)(n & 255), (uint8_t)(n >> 8), (uint8_t)(~n & 255), (uint8_t)((~n >> 8) & 255)};
    out.bytes.insert(out.bytes.end(), f, f + n);
    return out;
  }
  std::vector<uint32_t> words(size / 4 + 2, 0u);
  png_block_header(len, has_match, header, tree, words.data());
  for (int i = 0; i < n; ++i) {
    const PngRole r = png_token_role(i - start[i], length[i]);
    if (r.kind == 1) png_put_bits(words.data(), pos, code[f[i]], len[f[i]]), pos += len[f[i]];
    if (r.kind == 2) {
      const PngLength l = png_length_symbol(r.length);
      const int nb = len[l.symbol] + l.extra_bits + 1;
      png_put_bits(words.data(), pos, (uint32_t)code[l.symbol] | ((uint32_t)l.extra << len[l.symbol]), nb);
      pos += (uint32_t)nb;
    }
  }
  png_put_bits(words.data(), pos, code[256], len[256]);
  png_put_bits(words.data(), 8 * body + 16, 0xFFFFu, 16);
  out.bytes.resize(size);
  for (uint32_t k = 0; k < size; ++k) out.bytes[k] = (uint8_t)(words[k >> 2] >> (8 * (k & 3)));
  return out;
}

static std::vector<uint8_t> filter_image(const PngGeom& g, const uint8_t* px) {
  std::vector<uint8_t> rows((size_t)g.H * g.row_bytes);
  for (int y = 0; y < g.H; ++y) {
    const uint8_t* cur = px + png_pixel_offset(g, 0, y);
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int pass = 0, type = 0; pass < 2; ++pass) {
      for (int x = 0; x < g.R; ++x) {
        const int a = x >= g.C ? cur[x - g.C] : 0, b = y > 0 ? cur[x - g.R] : 0, c = (y > 0 && x >= g.C) ? cur[x - g.C - g.R] : 0;
        if (pass == 0)
          for (int t = 0; t < 5; ++t) cost[t] += (uint32_t)png_filter_cost(png_filter_byte(t, cur[x], a, b, c));
        else
          rows[(size_t)y * g.row_bytes + 1 + x] = (uint8_t)png_filter_byte(type, cur[x], a, b, c);
      }
      type = png_filter_choice(cost);
      rows[(size_t)y * g.row_bytes] = (uint8_t)type;
    }
  }
  return rows;
}

static std::vector<uint8_t> encode_image(const PngGeom& g, const uint8_t* px, int* limited = nullptr, int* stored = nullptr) {
  const std::vector<uint8_t> rows = filter_image(g, px);
  std::vector<uint8_t> out = {0x78, 0x01};
  uint32_t a = 1, b = 0;
  for (int s = 0; s < g.segments; ++s) {
    const int n = png_segment_rows(g, s) * g.row_bytes;
    const Segment seg = encode_segment(rows.data() + (size_t)s * g.rows_per_segment * g.row_bytes, n);
    out.insert(out.end(), seg.bytes.begin(), seg.bytes.end());
    png_adler_combine(a, b, seg.n, seg.s1, seg.s2);
    if (limited) *limited += seg.limited;
    if (stored) *stored += seg.stored ? 1 : 0;
  }
  const uint8_t tail[6] = {3, 0, (uint8_t)(b >> 8), (uint8_t)b, (uint8_t)(a >> 8), (uint8_t)a};
  out.insert(out.end(), tail, tail + 6);
  return out;
}

// ---- written a second time, naively
static int naive_filter_byte(int type, int x, int a, int b, int c) {
  int pred = 0;
  if (type == 1) pred = a;
  if (type == 2) pred = b;
  if (type == 3) pred = (a + b) / 2;
  if (type == 4) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return ((x - pred) % 256 + 256) % 256;
}

static std::vector<uint8_t> naive_filter_image(int H, int W, int C, const uint8_t* px) {
  const int R = W * C;
  std::vector<uint8_t> rows;
  for (int y = 0; y < H; ++y) {
    long best_cost = -1;
    std::vector<uint8_t> best;
    for (int t = 0; t < 5; ++t) {
      std::vector<uint8_t> row = {(uint8_t)t};
      long cost = 0;
      for (int x = 0; x < R; ++x) {
        const int a = x >= C ? px[(size_t)y * R + x - C] : 0, b = y ? px[(size_t)(y - 1) * R + x] : 0;
        const int c = (y && x >= C) ? px[(size_t)(y - 1) * R + x - C] : 0;
        const int f = naive_filter_byte(t, px[(size_t)y * R + x], a, b, c);
        row.push_back((uint8_t)f);
        cost += f < 256 - f ? f : 256 - f;
      }
      if (best_cost < 0 || cost < best_cost) best_cost = cost, best = row;
    }
    rows.insert(rows.end(), best.begin(), best.end());
  }
  return rows;
}

static const int LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const int LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const int CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// a small inflate: stored, fixed and dynamic blocks, distance 1 only (the only distance this format sends)
struct Bits {
  const uint8_t* p;
  size_t n, pos;
  bool bad;
  int get(int k) {
    int v = 0;
    for (int i = 0; i < k; ++i, ++pos) {
      if (pos >= 8 * n) {
        bad = true;
        return 0;
      }
      v |= ((p[pos >> 3] >> (pos & 7)) & 1) << i;
    }
    return v;
  }
};
struct Code {
  std::vector<int> len;
  // the symbol of the next code, read bit by bit: canonical codes, by RFC 1951's counting
  int count[16];
  std::vector<int> sorted;
  void prepare() {
    for (int& c : count) c = 0;
    for (int l : len) ++count[l];
    count[0] = 0;
    sorted.clear();
    for (int l = 1; l < 16; ++l)
      for (size_t s = 0; s < len.size(); ++s)
        if (len[s] == l) sorted.push_back((int)s);
  }
  int decode(Bits& in) const {
    int first = 0, index = 0, code = 0;
    for (int l = 1; l < 16; ++l) {
      code |= in.get(1);
      if (in.bad) return -1;
      if (code - count[l] < first) return sorted[index + (code - first)];
      index += count[l], first += count[l], first <<= 1, code <<= 1;
    }
    return -1;
  }
};
static bool naive_inflate(const uint8_t* z, size_t n, std::vector<uint8_t>& out, uint32_t* adler) {
  if (n < 8 || z[0] != 0x78 || z[1] != 0x01) return false;
  Bits in = {z + 2, n - 6, 0, false};
  for (;;) {
    const int final = in.get(1), type = in.get(2);
    if (in.bad || type == 3) return false;
    if (type == 0) {
      in.pos = (in.pos + 7) & ~(size_t)7;
      const int len = in.get(16), nlen = in.get(16);
      if (in.bad || (len ^ nlen) != 0xFFFF) return false;
      for (int i = 0; i < len; ++i) out.push_back((uint8_t)in.get(8));
    } else {
      Code lit, dist;
      if (type == 1) {
        for (int s = 0; s < 288; ++s) lit.len.push_back(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        dist.len.assign(30, 5);
      } else {
        const int hlit = in.get(5) + 257, hdist = in.get(5) + 1, hclen = in.get(4) + 4;
        Code cl;
        cl.len.assign(19, 0);
        for (int i = 0; i < hclen; ++i) cl.len[CL_ORDER[i]] = in.get(3);
        cl.prepare();
        std::vector<int> all;
        while ((int)all.size() < hlit + hdist) {
          const int s = cl.decode(in);
          if (s < 0) return false;
          if (s < 16) all.push_back(s);
          if (s == 16) {
            if (all.empty()) return false;
            all.insert(all.end(), (size_t)(3 + in.get(2)), all.back());
          }
          if (s == 17) all.insert(all.end(), (size_t)(3 + in.get(3)), 0);
          if (s == 18) all.insert(all.end(), (size_t)(11 + in.get(7)), 0);
        }
        if ((int)all.size() != hlit + hdist) return false;
        lit.len.assign(all.begin(), all.begin() + hlit);
        dist.len.assign(all.begin() + hlit, all.end());
      }
      lit.prepare(), dist.prepare();
      for (;;) {
        const int s = lit.decode(in);
        if (s < 0 || s > 285) return false;
        if (s == 256) break;
        if (s < 256) {
          out.push_back((uint8_t)s);
          continue;
        }
        const int len = LEN_BASE[s - 257] + in.get(LEN_EXTRA[s - 257]);
        if (dist.decode(in) != 0 || out.empty()) return false;
        out.insert(out.end(), (size_t)len, out.back());
      }
    }
    if (in.bad) return false;
    if (final) break;
  }
  if (((in.pos + 7) >> 3) != n - 6) return false;
  *adler = ((uint32_t)z[n - 4] << 24) | ((uint32_t)z[n - 3] << 16) | ((uint32_t)z[n - 2] << 8) | z[n - 1];
  return true;
}
static uint32_t naive_adler(const std::vector<uint8_t>& v) {
  uint32_t a = 1, b = 0;
  for (uint8_t x : v) a = (a + x) % 65521u, b = (b + a) % 65521u;
  return (b << 16) | a;
}

static int image_case(const char* what, int H, int W, int C, const std::vector<uint8_t>& px, int* limited = nullptr) {
  CHECK(png_plan_check(1, H, W, C) == nullptr, "%s: refused", what);
  const PngGeom g = png_geom(1, H, W, C);
  int stored = 0;
  const std::vector<uint8_t> z = encode_image(g, px.data(), limited, &stored);
  const std::vector<uint8_t> want = naive_filter_image(H, W, C, px.data());
  CHECK(filter_image(g, px.data()) == want, "%s: the filtered stream differs from the naive one", what);
  std::vector<uint8_t> back;
  uint32_t adler = 0;
  CHECK(naive_inflate(z.data(), z.size(), back, &adler), "%s: the stream does not inflate", what);
  CHECK(back == want, "%s: the stream inflates to other bytes", what);
  CHECK(adler == naive_adler(want), "%s: Adler-32 %08x, the byte loop gives %08x", what, adler, naive_adler(want));
  CHECK(z.size() <= png_capacity_bytes(g), "%s: %zu bytes exceed the capacity %zu", what, z.size(), png_capacity_bytes(g));
  return 0;
}

static int token_checks() {
  // a sequential parse of a run of L equal bytes: a literal, then matches of 258 while 3 or more remain
  for (int L = 1; L <= 600; ++L) {
    std::vector<int> kind(L, 0), length(L, 0);
    kind[0] = 1;
    for (int i = 1; i < L;) {
      const int left = L - i;
      if (left >= 3) {
        const int take = left < 258 ? left : 258;
        kind[i] = 2, length[i] = take;
        i += take;
      } else {
        kind[i++] = 1;
      }
    }
    for (int p = 0; p < L; ++p) {
      const PngRole r = png_token_role(p, L);
      CHECK(r.kind == kind[p] && (kind[p] != 2 || r.length == length[p]), "role of byte %d of a run of %d: kind %d length %d", p, L,
            r.kind, r.length);
    }
  }
  for (int len = 3; len <= 258; ++len) {
    int slot = 28;
    while (LEN_BASE[slot] > len) --slot;
    const PngLength l = png_length_symbol(len);
    CHECK(l.symbol == 257 + slot && l.extra_bits == LEN_EXTRA[slot] && l.extra == len - LEN_BASE[slot], "length symbol of %d", len);
  }
  for (int i = 0; i < 19; ++i) CHECK(png_cl_order(i) == CL_ORDER[i], "code-length order at %d", i);
  for (int len = 1; len <= 15; ++len)
    for (uint32_t c = 0; c < (1u << len); c += 1 + (c >> 4)) {
      uint32_t r = 0;
      for (int i = 0; i < len; ++i) r = (r << 1) | ((c >> i) & 1);
      CHECK(png_reverse_bits(c, len) == r, "bit reversal of %u at %d bits", c, len);
    }
  return 0;
}

static int builder_case(const char* what, const std::vector<uint32_t>& count, int limit, int* limited_out = nullptr) {
  static PngTree tree;
  const int nsym = (int)count.size();
  std::vector<uint8_t> len(nsym + 2, 0xAA);
  const int limited = png_build_lengths(count.data(), nsym, limit, len.data(), tree);
  if (limited_out) *limited_out = limited;
  unsigned long long kraft = 0;
  int used = 0, leaves = 0;
  for (int s = 0; s < nsym; ++s) {
    CHECK(len[s] <= limit, "%s: symbol %d has length %d", what, s, len[s]);
    CHECK(count[s] == 0 || len[s] > 0, "%s: symbol %d with a count has no code", what, s);
    if (count[s]) ++used;
    if (len[s]) ++leaves, kraft += 1ull << (limit - len[s]);
  }
  CHECK(leaves == (used < 2 ? 2 : used), "%s: %d codes for %d symbols", what, leaves, used);
  CHECK(kraft == 1ull << limit, "%s: Kraft sum %llu / %llu", what, kraft, 1ull << limit);
  CHECK(len[nsym] == 0xAA, "%s: wrote past the lengths", what);
  std::vector<uint16_t> code(nsym);
  png_canonical_codes(len.data(), nsym, code.data());
  // no code is a prefix of another: sent from the top bit, so compare the reversed codes' low bits
  for (int a = 0; a < nsym; ++a)
    for (int b = 0; b < nsym; ++b)
      if (a != b && len[a] && len[b] && len[a] <= len[b])
        CHECK((code[b] & ((1u << len[a]) - 1)) != code[a], "%s: the code of %d is a prefix of that of %d", what, a, b);
  // a rarer symbol never has the shorter code
  for (int a = 0; a < nsym; ++a)
    for (int b = 0; b < nsym; ++b)
      if (count[a] && count[b] && count[a] < count[b]) CHECK(len[a] >= len[b], "%s: the rarer symbol %d has the shorter code", what, a);
  return 0;
}

static int builder_checks() {
  for (int round = 0; round < 300; ++round) {
    const int nsym = round % 3 == 0 ? PNG_CLSYMS : PNG_LITLEN;
    std::vector<uint32_t> count(nsym, 0);
    const int shape = round % 7;
    for (int s = 0; s < nsym; ++s) {
      if (shape == 0) count[s] = rnd() % 4 ? 0 : rnd() % 1000;
      if (shape == 1) count[s] = rnd() % 50;
      if (shape == 2) count[s] = 1;
      if (shape == 3) count[s] = s < 24 ? 1u << s : 0;
      if (shape == 4) count[s] = rnd() % 3 == 0 ? 1u + rnd() % 3 : 0;
      if (shape == 5) count[s] = s == (int)(rnd() % nsym) ? 7 : 0;
      if (shape == 6) count[s] = 0;
    }
    if (shape == 5 && round % 2) count[0] = 3;
    if (builder_case("random counts", count, nsym == PNG_CLSYMS ? PNG_CL_LIMIT : PNG_LIMIT)) return 1;
  }
  // Fibonacci counts make the deepest tree: 30 of them pass the limit of 15, and 12 that of 7
  std::vector<uint32_t> fib(PNG_LITLEN, 0);
  uint32_t a = 1, b = 1;
  for (int s = 0; s < 30; ++s) {
    fib[s * 3] = a;
    const uint32_t c = a + b;
    a = b, b = c;
  }
  int limited = 0;
  if (builder_case("Fibonacci counts", fib, PNG_LIMIT, &limited)) return 1;
  CHECK(limited > 0, "Fibonacci counts did not reach the limit");
  std::vector<uint32_t> small(PNG_CLSYMS, 0);
  a = 1, b = 1;
  for (int s = 0; s < 12; ++s) {
    small[s] = a;
    const uint32_t c = a + b;
    a = b, b = c;
  }
  if (builder_case("Fibonacci counts of the code-length alphabet", small, PNG_CL_LIMIT, &limited)) return 1;
  CHECK(limited > 0, "Fibonacci counts did not reach the limit of 7");
  return 0;
}

static int adler_checks() {
  for (int round = 0; round < 40; ++round) {
    std::vector<uint8_t> all;
    uint32_t a = 1, b = 0;
    const int pieces = 1 + (int)(rnd() % 6);
    for (int k = 0; k < pieces; ++k) {
      const int n = round % 4 == 0 ? PNG_SEGMENT_BYTES : 1 + (int)(rnd() % 5000);
      uint64_t s1 = 0, s2 = 0;
      for (int i = 0; i < n; ++i) {
        const uint8_t v = round % 4 == 0 ? 255 : (uint8_t)rnd();
        all.push_back(v);
        s1 += v, s2 += (uint64_t)(n - i) * v;
      }
      CHECK(s1 <= 0xFFFFFFFFull, "the sum of a segment's bytes leaves 32 bits");
      png_adler_combine(a, b, (uint32_t)n, (uint32_t)s1, (uint32_t)(s2 % PNG_ADLER_MOD));
    }
    CHECK(((b << 16) | a) == naive_adler(all), "Adler-32 of %d pieces", pieces);
  }
  return 0;
}

static int plan_checks() {
  CHECK(png_plan_check(-1, 4, 4, 3) && png_plan_check(1, -1, 4, 3) && png_plan_check(1, 4, -1, 3), "a negative size passes");
  CHECK(png_plan_check(1, 0, 4, 3) && png_plan_check(1, 4, 0, 3), "an empty image passes");
  CHECK(!png_plan_check(0, 0, 0, 3) && !png_plan_check(0, 4, 4, 1), "images == 0 is refused");
  CHECK(png_plan_check(1, 4, 4, 0) && png_plan_check(1, 4, 4, 2) && png_plan_check(1, 4, 4, 4), "a channel count outside {1, 3} passes");
  CHECK(!png_plan_check(1, 1, 10922, 3) && png_plan_check(1, 1, 10923, 3), "the widest row at 3 channels is 10922 pixels");
  CHECK(!png_plan_check(1, 1, 32767, 1) && png_plan_check(1, 1, 32768, 1), "the widest row at 1 channel is 32767 pixels");
  CHECK(png_plan_check(1, 1, INT_MAX, 3) && png_plan_check(1, 1, INT_MAX, 1), "a width whose row overflows int passes");
  CHECK(png_plan_check(INT_MAX, INT_MAX, 10922, 3) && png_plan_check(1 << 20, INT_MAX, 32767, 1), "sizes past 2^56 bytes pass");
  CHECK(!png_plan_check(1, INT_MAX, 10922, 3), "a tall image within 2^56 bytes is refused");
  const int sizes[][3] = {{1, 1, 1}, {1, 1, 3}, {7, 5, 3}, {83, 131, 3}, {84, 131, 3}, {166, 131, 3}, {3, 10000, 3}, {518, 518, 1},
                          {1554, 518, 3}, {2772, 924, 3}, {40000, 1, 1}, {5, 10922, 3}, {100000, 32767, 1}};
  for (const auto& s : sizes)
    for (int images : {1, 3, 70000}) {
      const int H = s[0], W = s[1], C = s[2];
      CHECK(!png_plan_check(images, H, W, C), "%d x %d x %d x %d is refused", images, H, W, C);
      const PngGeom g = png_geom(images, H, W, C);
      const __int128 row = 1 + (__int128)W * C;
      CHECK(g.R == W * C && g.row_bytes == row && g.rows_per_segment >= 1, "row of %d x %d", W, C);
      CHECK((__int128)g.rows_per_segment * row <= PNG_SEGMENT_BYTES && (__int128)(g.rows_per_segment + 1) * row > PNG_SEGMENT_BYTES,
            "rows per segment of %d x %d", W, C);
      CHECK((__int128)(g.segments - 1) * g.rows_per_segment < H && (__int128)g.segments * g.rows_per_segment >= H, "segments of %d", H);
      long long rows = 0;
      for (int k : {0, g.segments / 2, g.segments - 1}) CHECK(png_segment_rows(g, k) >= 1 && png_segment_rows(g, k) <= g.rows_per_segment, "rows of segment %d", k);
      rows = (long long)(g.segments - 1) * g.rows_per_segment + png_segment_rows(g, g.segments - 1);
      CHECK(rows == H, "the segments of %d rows hold %lld", H, rows);
      CHECK(g.slot_bytes % 16 == 0 && g.slot_bytes >= g.segment_bytes + PNG_STORED_EXTRA && g.segment_bytes <= PNG_SEGMENT_BYTES, "slot of %d x %d", W, C);
      const __int128 cap = (__int128)images * (8 + (__int128)H * row + 5 * (__int128)g.segments);
      CHECK((__int128)png_capacity_bytes(g) == cap, "capacity of %d x %d x %d x %d", images, H, W, C);
      const __int128 ws = (__int128)images * g.segments * ((__int128)g.slot_bytes + 16);
      CHECK((__int128)png_workspace_bytes(g) == ws, "workspace of %d x %d x %d x %d", images, H, W, C);
      const long long image = images - 1;
      const __int128 slot = (__int128)images * g.segments * 16 + ((__int128)image * g.segments + (g.segments - 1)) * g.slot_bytes;
      CHECK((__int128)png_slot_offset(g, image, g.segments - 1) == slot && slot + g.slot_bytes == ws, "the last slot of %d x %d x %d x %d", images, H, W, C);
      CHECK((__int128)png_pixel_offset(g, image, H - 1) == ((__int128)image * H + (H - 1)) * W * C, "the last row of %d x %d x %d x %d", images, H, W, C);
    }
  return 0;
}

static int image_checks() {
  int limited = 0;
  for (int round = 0; round < 60; ++round) {
    const int C = round % 2 ? 3 : 1, H = 1 + (int)(rnd() % 40), W = 1 + (int)(rnd() % 300);
    std::vector<uint8_t> px((size_t)H * W * C);
    const int shape = round % 5;
    int walk = 128;
    for (size_t i = 0; i < px.size(); ++i) {
      walk += (int)(rnd() % 7) - 3;
      if (shape == 0) px[i] = (uint8_t)rnd();
      if (shape == 1) px[i] = (uint8_t)walk;
      if (shape == 2) px[i] = 0;
      if (shape == 3) px[i] = rnd() % 64 ? 200 : 10;
      if (shape == 4) px[i] = (uint8_t)((i / 97) * 31);
    }
    if (image_case("random image", H, W, C, px, &limited)) return 1;
  }
  {  // several segments, a short last one, one row per segment
    std::vector<uint8_t> px((size_t)700 * 700 * 3, 0);
    if (image_case("zeros", 700, 700, 3, px)) return 1;
    std::vector<uint8_t> wide((size_t)3 * 10000 * 3);
    int walk = 100;
    for (auto& v : wide) v = (uint8_t)(walk += (int)(rnd() % 5) - 2);
    if (image_case("one row per segment", 3, 10000, 3, wide)) return 1;
    std::vector<uint8_t> tall((size_t)40000, 0);
    for (size_t i = 0; i < tall.size(); ++i) tall[i] = (uint8_t)(i / 300);
    if (image_case("two bytes per row", 40000, 1, 1, tall)) return 1;
  }
  return 0;
}

static int encode_files(int argc, char** argv) {
  if (argc != 7) return 2;
  const int H = atoi(argv[2]), W = atoi(argv[3]), C = atoi(argv[4]);
  if (png_plan_check(1, H, W, C)) return 2;
  FILE* in = fopen(argv[5], "rb");
  FILE* out = fopen(argv[6], "wb");
  if (!in || !out) return 2;
  const PngGeom g = png_geom(1, H, W, C);
  std::vector<uint8_t> px((size_t)H * W * C);
  while (fread(px.data(), 1, px.size(), in) == px.size()) {
    const std::vector<uint8_t> z = encode_image(g, px.data());
    uint8_t size[8];
    for (int k = 0; k < 8; ++k) size[k] = (uint8_t)((unsigned long long)z.size() >> (8 * k));
    fwrite(size, 1, 8, out);
    fwrite(z.data(), 1, z.size(), out);
  }
  fclose(in);
  return fclose(out) ? 2 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "encode")) return encode_files(argc, argv);
  if (plan_checks() || token_checks() || builder_checks() || adler_checks() || image_checks()) return 1;
  printf("ok %ld\n", g_checks);
  return 0;
}

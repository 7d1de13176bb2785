// PNG encoding on the device (csrc/png.hip): what the kernels, the C ABI's checks and a host program share
// (csrc/png_host_check.cpp replays it against a naive implementation under a sanitizer).  The definition, byte for
// byte, is forward_utils.png_encode_host; include/aaclip.h states it for callers.
//
// pixels uint8 [images, H, W, C], C in {1, 3}; R = W * C; the FILTERED STREAM of an image is H rows of 1 + R bytes (the
// filter type, then the filtered bytes).  A SEGMENT is rows_per_segment = max(1, 32768 / (1 + R)) whole rows of it (the
// last one of an image may be shorter) and becomes one deflate block that ends byte-aligned:
//   filters   PNG's five types with bpp = C, the row above row 0 all zeros; a row takes the type with the smallest sum of
//             min(b, 256 - b) over its R filtered bytes, ties to the lowest type
//   tokens    distance-1 matches only: a maximal run of n equal bytes inside a segment is one literal, then the other
//             n - 1 bytes in pieces of 258; a last piece of 3 or more is a match, one of 1 or 2 is literals
//             (png_token_role: a byte's role follows from its position in its run and the run's length)
//   code      png_build_lengths: leaves in (count, symbol) order, two-queue Huffman merge, a leaf before an internal
//             node of equal weight.  The tree gives the NUMBER of codes of every length, a deeper leaf counted at the
//             limit; while their Kraft sum exceeds 1, one code of the limit's length goes and the longest shorter code
//             becomes two codes one bit longer; the lengths are handed out in leaf order, the longest to the rarest.
//             Literal / length limit 15, code-length alphabet limit 7; the distance alphabet is one code (HDIST = 0)
//             of length 1 if the segment has a match, else 0
//   lengths   the HLIT literal / length lengths and the distance length as ONE sequence: a non-zero length is sent as
//             itself (symbol 16 is never used); of a zero run of z, while z >= 11 one symbol 18 takes min(z, 138),
//             then one symbol 17 takes the rest if that is 3 or more, else it is sent as symbols 0
//   block     BFINAL = 0, BTYPE = 2, the header, the tokens, end-of-block, three zero bits (an empty stored block),
//             padding to the byte, 00 00 FF FF.  If that is not shorter than the stored block (00, LEN, NLEN, the
//             bytes), the stored block is taken: a segment never takes more than its length + 5 bytes
// The zlib stream of an image is 78 01, its segments, 03 00 (an empty final fixed block) and the Adler-32 of the filtered
// stream, big-endian, combined from per-segment sums in segment order (png_adler_combine).
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AACLIP_PNG_HD __host__ __device__ inline
#else
#define AACLIP_PNG_HD inline
#endif

namespace aaclip {

static constexpr int PNG_SEGMENT_BYTES = 32768;          // a segment's rows hold at most this many bytes
static constexpr int PNG_THREADS = 256;
static constexpr int PNG_CHUNK = PNG_SEGMENT_BYTES / PNG_THREADS;   // the bytes of a segment that one thread walks
static constexpr int PNG_LITLEN = 286, PNG_CLSYMS = 19;
static constexpr int PNG_LIMIT = 15, PNG_CL_LIMIT = 7;
static constexpr int PNG_MIN_MATCH = 3, PNG_MAX_MATCH = 258;
static constexpr uint32_t PNG_ADLER_MOD = 65521u;
static constexpr uint32_t PNG_NONE = 0xFFFFFFFFu;        // the key of a symbol that is no leaf
static constexpr int PNG_STREAM_EXTRA = 8;               // 78 01 ... 03 00 and four bytes of Adler-32
static constexpr int PNG_STORED_EXTRA = 5;               // 00 LEN NLEN
static constexpr int PNG_META_WORDS = 4;                 // per segment: size, sum of bytes, weighted sum mod 65521, length
static constexpr long long PNG_MAX_BYTES = 1ll << 56;    // the largest capacity or workspace
static constexpr int PNG_COPY_PARTS = 16;                // workgroups that share the copy of one image

struct PngGeom {
  int images, H, W, C;
  int R, row_bytes;               // W * C, 1 + R
  int rows_per_segment, segments; // per image
  int segment_bytes;              // of a full segment (the largest one)
  int slot_bytes;                 // a segment's slot of the workspace: segment_bytes + 5, rounded up to 16
};

// nullptr, or why the plan is refused.  images == 0 passes (the entry then launches nothing).
inline const char* png_plan_check(int images, int H, int W, int C) {
  if (images < 0) return "images must not be negative";
  if (H < 0 || W < 0) return "height and width must not be negative";
  if (C != 1 && C != 3) return "channels must be 1 or 3";
  if (images > 0 && (H == 0 || W == 0)) return "height and width must be at least 1";
  const long long row = 1 + (long long)W * C;
  if (row > PNG_SEGMENT_BYTES) return "a filtered row (1 + width * channels bytes) must not exceed 32768 bytes";
  const long long rps = PNG_SEGMENT_BYTES / row, segs = ((long long)H + rps - 1) / rps;
  // per image: the capacity 8 + H * row + 5 * segs, and the workspace below; both within PNG_MAX_BYTES / images
  const long long per_image = PNG_STREAM_EXTRA + (long long)H * row + (PNG_STORED_EXTRA + 32 + 16) * segs;   // < 2^52
  if (images > 0 && per_image > PNG_MAX_BYTES / images) return "the tensors are too large";
  return nullptr;
}

inline PngGeom png_geom(int images, int H, int W, int C) {
  PngGeom g = {};
  g.images = images, g.H = H, g.W = W, g.C = C;
  g.R = W * C, g.row_bytes = 1 + g.R;
  g.rows_per_segment = PNG_SEGMENT_BYTES / g.row_bytes;
  if (g.rows_per_segment < 1) g.rows_per_segment = 1;
  g.segments = (int)(((long long)H + g.rows_per_segment - 1) / g.rows_per_segment);
  g.segment_bytes = (H < g.rows_per_segment ? H : g.rows_per_segment) * g.row_bytes;
  g.slot_bytes = (g.segment_bytes + PNG_STORED_EXTRA + 15) & ~15;
  return g;
}

AACLIP_PNG_HD int png_segment_rows(const PngGeom& g, int seg) {
  const int left = g.H - seg * g.rows_per_segment;
  return left < g.rows_per_segment ? left : g.rows_per_segment;
}
inline size_t png_capacity_bytes(const PngGeom& g) {
  return (size_t)g.images * ((size_t)PNG_STREAM_EXTRA + (size_t)g.H * (size_t)g.row_bytes + (size_t)PNG_STORED_EXTRA * (size_t)g.segments);
}
// the workspace: PNG_META_WORDS dwords per (image, segment), then the slots; 16-byte aligned
inline size_t png_workspace_bytes(const PngGeom& g) {
  return (size_t)g.images * (size_t)g.segments * ((size_t)g.slot_bytes + 4 * PNG_META_WORDS);
}
AACLIP_PNG_HD long long png_slot_offset(const PngGeom& g, long long image, int seg) {   // in bytes from the workspace
  return (long long)g.images * g.segments * (4 * PNG_META_WORDS) + (image * g.segments + seg) * (long long)g.slot_bytes;
}
AACLIP_PNG_HD long long png_pixel_offset(const PngGeom& g, long long image, int y) { return (image * g.H + y) * (long long)g.R; }

// ---- row filters
AACLIP_PNG_HD int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// x the byte, a the byte bpp to its left, b the byte above, c the byte above a (0 outside the image)
AACLIP_PNG_HD int png_filter_byte(int type, int x, int a, int b, int c) {
  const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
  return (x - pred) & 255;
}
AACLIP_PNG_HD int png_filter_cost(int f) { return f < 256 - f ? f : 256 - f; }
AACLIP_PNG_HD int png_filter_choice(const uint32_t cost[5]) {
  int best = 0;
  for (int t = 1; t < 5; ++t)
    if (cost[t] < cost[best]) best = t;
  return best;
}

// ---- tokens
struct PngRole {
  int kind;      // 0: inside a match, 1: a literal, 2: the first byte of a match of `length`
  int length;
};
// the byte at position p (0-based) of a maximal run of L equal bytes
AACLIP_PNG_HD PngRole png_token_role(int p, int L) {
  PngRole r = {1, 0};
  if (p == 0) return r;
  const int m = L - 1, q = p - 1;
  const int piece = q / PNG_MAX_MATCH < m / PNG_MAX_MATCH ? PNG_MAX_MATCH : m % PNG_MAX_MATCH;
  if (piece < PNG_MIN_MATCH) return r;
  r.kind = q % PNG_MAX_MATCH == 0 ? 2 : 0;
  r.length = piece;
  return r;
}
struct PngLength {
  int symbol, extra_bits, extra;
};
AACLIP_PNG_HD PngLength png_length_symbol(int length) {   // 3 .. 258
  PngLength l = {0, 0, 0};
  const int x = length - 3;
  if (length == PNG_MAX_MATCH) {
    l.symbol = 285;
  } else if (x < 8) {
    l.symbol = 257 + x;
  } else {
    int e = 1;
    while ((x >> (e + 3)) != 0) ++e;               // 8 <= x >> (e - 1) ... : e = floor(log2 x) - 2
    l.symbol = 257 + 4 * e + 4 + ((x >> e) & 3);
    l.extra_bits = e;
    l.extra = x & ((1 << e) - 1);
  }
  return l;
}

// ---- the code builder.  key[s] is a leaf's count, or PNG_NONE for a symbol that is no leaf.
struct PngTree {
  uint32_t key[PNG_LITLEN];
  uint32_t weight[2 * PNG_LITLEN];
  uint16_t parent[2 * PNG_LITLEN];
  uint16_t depth[2 * PNG_LITLEN];
  uint16_t order[PNG_LITLEN];       // the leaves in (key, symbol) order
};
// the number of leaves before symbol s in (key, symbol) order
AACLIP_PNG_HD int png_rank(const uint32_t* key, int nsym, int s) {
  const uint32_t ks = key[s];
  int r = 0;
  for (int j = 0; j < nsym; ++j) {
    const uint32_t kj = key[j];
    r += (kj != PNG_NONE && (kj < ks || (kj == ks && j < s))) ? 1 : 0;
  }
  return r;
}
// the tree over the m >= 2 leaves of t.order: t.depth[k] of leaf k
AACLIP_PNG_HD void png_tree_depths(PngTree& t, int m) {
  for (int k = 0; k < m; ++k) t.weight[k] = t.key[t.order[k]];
  int leaf = 0, node = m, next = m;
  for (; next < 2 * m - 1; ++next) {
    uint32_t sum = 0;
    for (int pick = 0; pick < 2; ++pick) {
      const bool take_leaf = leaf < m && (node >= next || t.weight[leaf] <= t.weight[node]);
      const int k = take_leaf ? leaf++ : node++;
      sum += t.weight[k];
      t.parent[k] = (uint16_t)next;
    }
    t.weight[next] = sum;
  }
  t.depth[2 * m - 2] = 0;
  for (int k = 2 * m - 3; k >= 0; --k) t.depth[k] = (uint16_t)(t.depth[t.parent[k]] + 1);
}
// the limit: the number of codes of every length is taken from the tree, a deeper leaf counted at the limit; while the
// Kraft sum exceeds 1, one code of the limit's length goes, and the longest shorter code becomes two codes one bit
// longer.  The lengths are then handed out in leaf order, the longest to the rarest.  Returns how many leaves lay
// deeper than the limit.
AACLIP_PNG_HD int png_limit_lengths(const PngTree& t, int m, int limit, uint8_t* len) {
  uint32_t num[PNG_LIMIT + 1];
  for (int l = 0; l <= PNG_LIMIT; ++l) num[l] = 0;
  int over = 0;
  for (int k = 0; k < m; ++k) {
    const int d = t.depth[k];
    over += d > limit ? 1 : 0;
    ++num[d > limit ? limit : d];
  }
  uint32_t total = 0;
  for (int l = 1; l <= limit; ++l) total += num[l] << (limit - l);
  while (total > (1u << limit)) {
    --num[limit];
    for (int l = limit - 1; l > 0; --l)
      if (num[l]) {
        --num[l];
        num[l + 1] += 2;
        break;
      }
    --total;
  }
  int k = 0;
  for (int l = limit; l >= 1; --l)
    for (uint32_t c = 0; c < num[l]; ++c) len[t.order[k++]] = (uint8_t)l;
  return over;
}
// count[nsym] -> t.key: a zero count is no leaf; fewer than two leaves are filled up with the lowest other symbols at
// count 0 (a code of one length-1 symbol alone is incomplete, and zlib refuses an incomplete code-length code)
AACLIP_PNG_HD void png_keys_from_counts(const uint32_t* count, int nsym, uint32_t* key) {
  int used = 0;
  for (int s = 0; s < nsym; ++s) key[s] = count[s] ? (++used, count[s]) : PNG_NONE;
  for (int s = 0; s < nsym && used < 2; ++s)
    if (key[s] == PNG_NONE) key[s] = 0, ++used;
}
// the whole builder, serial: len[nsym] from count[nsym]; returns how many leaves the limit moved up
AACLIP_PNG_HD int png_build_lengths(const uint32_t* count, int nsym, int limit, uint8_t* len, PngTree& t) {
  png_keys_from_counts(count, nsym, t.key);
  int m = 0;
  for (int s = 0; s < nsym; ++s) {
    len[s] = 0;
    if (t.key[s] != PNG_NONE) t.order[png_rank(t.key, nsym, s)] = (uint16_t)s, ++m;
  }
  png_tree_depths(t, m);
  return png_limit_lengths(t, m, limit, len);
}

// ---- canonical codes, bit-reversed (deflate sends Huffman codes from their most significant bit)
AACLIP_PNG_HD uint32_t png_reverse_bits(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}
AACLIP_PNG_HD void png_canonical_codes(const uint8_t* len, int nsym, uint16_t* code) {
  uint32_t count[PNG_LIMIT + 1], next[PNG_LIMIT + 1];
  for (int l = 0; l <= PNG_LIMIT; ++l) count[l] = 0;
  for (int s = 0; s < nsym; ++s) ++count[len[s]];
  count[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int l = 1; l <= PNG_LIMIT; ++l) next[l] = c = (c + count[l - 1]) << 1;
  for (int s = 0; s < nsym; ++s) code[s] = len[s] ? (uint16_t)png_reverse_bits(next[len[s]]++, len[s]) : (uint16_t)0;
}

// ---- bits, least significant first, OR-ed into zeroed 32-bit words; n <= 32
AACLIP_PNG_HD void png_put_bits(uint32_t* words, uint32_t pos, uint32_t value, int n) {
  if (n == 0) return;
  const uint32_t w = pos >> 5, sh = pos & 31;
  words[w] |= value << sh;
  if (sh + (uint32_t)n > 32) words[w + 1] |= value >> (32 - sh);
}

// ---- how the code lengths are sent: f(symbol, extra_bits, extra) per code-length token of the sequence
// len[0 .. hlit), dist_len
template <class F>
AACLIP_PNG_HD void png_length_tokens(const uint8_t* len, int hlit, int dist_len, F&& f) {
  const int n = hlit + 1;
  for (int i = 0; i < n;) {
    const int v = i < hlit ? len[i] : dist_len;
    if (v != 0) {
      f(v, 0, 0);
      ++i;
      continue;
    }
    int z = 1;
    while (i + z < n && (i + z < hlit ? len[i + z] : dist_len) == 0) ++z;
    i += z;
    while (z >= 11) {
      const int take = z < 138 ? z : 138;
      f(18, 7, take - 11);
      z -= take;
    }
    if (z >= 3) {
      f(17, 3, z - 3);
    } else {
      for (; z > 0; --z) f(0, 0, 0);
    }
  }
}
AACLIP_PNG_HD int png_hlit(const uint8_t* len) {
  int h = PNG_LITLEN;
  while (h > 257 && len[h - 1] == 0) --h;
  return h;
}
AACLIP_PNG_HD int png_cl_order(int i) {
  return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2;   // 16 17 18 0 8 7 9 6 10 5 ... 1 15
}

// the header of a dynamic block: BFINAL, BTYPE, HLIT, HDIST, HCLEN, the code-length code and the coded lengths.
// Returns its bits; writes them at bit 0 of words unless words is null.  len[286] are the literal / length lengths.
struct PngHeader {
  uint32_t cl_count[PNG_CLSYMS];
  uint8_t cl_len[PNG_CLSYMS];
  uint16_t cl_code[PNG_CLSYMS];
};
AACLIP_PNG_HD uint32_t png_block_header(const uint8_t* len, int dist_len, PngHeader& h, PngTree& t, uint32_t* words) {
  const int hlit = png_hlit(len);
  for (int s = 0; s < PNG_CLSYMS; ++s) h.cl_count[s] = 0;
  uint32_t* cl_count = h.cl_count;
  png_length_tokens(len, hlit, dist_len, [cl_count](int s, int, int) { ++cl_count[s]; });
  png_build_lengths(h.cl_count, PNG_CLSYMS, PNG_CL_LIMIT, h.cl_len, t);
  png_canonical_codes(h.cl_len, PNG_CLSYMS, h.cl_code);
  int hclen = PNG_CLSYMS;
  while (hclen > 4 && h.cl_len[png_cl_order(hclen - 1)] == 0) --hclen;
  uint32_t pos = 0;
  auto put = [&pos, words](uint32_t v, int n) {
    if (words) png_put_bits(words, pos, v, n);
    pos += (uint32_t)n;
  };
  put(0, 1), put(2, 2);
  put((uint32_t)(hlit - 257), 5), put(0, 5), put((uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; ++i) put(h.cl_len[png_cl_order(i)], 3);
  const uint8_t* cl_len = h.cl_len;
  const uint16_t* cl_code = h.cl_code;
  png_length_tokens(len, hlit, dist_len, [&put, cl_len, cl_code](int s, int eb, int e) {
    put(cl_code[s], cl_len[s]);
    put((uint32_t)e, eb);
  });
  return pos;
}

// ---- Adler-32 from per-segment sums: s1 = sum of b[i], s2 = sum of (n - i) * b[i] mod 65521, in segment order
AACLIP_PNG_HD void png_adler_combine(uint32_t& a, uint32_t& b, uint32_t n, uint32_t s1, uint32_t s2) {
  b = (uint32_t)(((uint64_t)b + (uint64_t)n * a + s2) % PNG_ADLER_MOD);
  a = (uint32_t)(((uint64_t)a + s1) % PNG_ADLER_MOD);
}

#if defined(__HIPCC__)
// two launches on s; the plan has passed png_plan_check and images >= 1
void launch_png_encode(const PngGeom& g, const uint8_t* pixels, void* workspace, uint8_t* payload, int64_t* offsets,
                       hipStream_t s);
#endif

}  // namespace aaclip

// csrc/buffers.h as the C ABI uses it, in a host program of its own (built with ASan + UBSan by
// tests/test_buffer_checks_cpu.py): bufs_overlap, bufs_misaligned and bufs_clash against a set-of-bytes model.  A
// buffer of the model is a 48-bit set, bit i = byte i of a 48-byte universe that starts at `base`; two buffers overlap
// when the sets meet.  The universe is laid (a) on a 64-byte aligned address in the middle of the address space and
// (b) on the LAST 48 bytes of it, where a range ends on byte UINTPTR_MAX and `p + bytes` wraps to 0.
//   pairs    every start and length (0 included) and the null pointer, for both buffers, at byte granularity
//   triples  every written / read-only assignment: every start, length and null pointer at byte granularity in the
//            first 12 bytes, and on the 4-byte grid of the whole universe (byte granularity over all 48 bytes would be
//            1.8e9 placements times 8 assignments); every start of three buffers with every alignment of {1, 4, 8, 16}
// Prints "ok <checks>" and returns 0, or says what differs and returns 1.
#include <stdio.h>

#include <vector>

#include "buffers.h"

using namespace aaclip;

static long g_checks = 0;
#define CHECK(cond, ...)            \
  do {                              \
    ++g_checks;                     \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

static const int U = 48;
struct Place { int start, len; bool null; };   // null: the pointer is NULL, whatever the length

static uint64_t bytes_of(const Place& s) {   // the model: the set of bytes the buffer holds
  uint64_t m = 0;
  if (!s.null)
    for (int i = s.start; i < s.start + s.len; ++i) m |= 1ull << i;
  return m;
}
static Buf buf_of(uintptr_t base, const Place& s, unsigned align, bool written) {
  return Buf{s.null ? nullptr : (const void*)(base + (uintptr_t)s.start), (size_t)s.len, align, written};
}

// every placement inside [0, limit) on a grid of `step` bytes, lengths from 0, and two null pointers (no bytes, bytes)
static std::vector<Place> places(int limit, int step) {
  std::vector<Place> v;
  for (int s = 0; s < limit; s += step)
    for (int n = 0; s + n <= limit; n += step) v.push_back(Place{s, n, false});
  v.push_back(Place{0, 0, true});
  v.push_back(Place{0, step, true});
  return v;
}

static int pairs(uintptr_t base) {
  const std::vector<Place> v = places(U, 1);
  for (const Place& a : v)
    for (const Place& b : v) {
      const bool want = (bytes_of(a) & bytes_of(b)) != 0;
      const Buf x = buf_of(base, a, 1, true), y = buf_of(base, b, 1, false);
      CHECK(bufs_overlap(x, y) == want && bufs_overlap(y, x) == want, "overlap of [%d, +%d) and [%d, +%d) at base %zx: want %d",
            a.start, a.len, b.start, b.len, (size_t)base, (int)want);
      if (!a.null && !b.null)
        CHECK(ranges_overlap(x.p, x.bytes, y.p, y.bytes) == want, "ranges_overlap of [%d, +%d) and [%d, +%d) at base %zx",
              a.start, a.len, b.start, b.len, (size_t)base);
    }
  return 0;
}

static int triples(uintptr_t base, int limit, int step) {
  const std::vector<Place> v = places(limit, step);
  for (const Place& a : v)
    for (const Place& b : v)
      for (const Place& c : v) {
        const Place* s[3] = {&a, &b, &c};
        const uint64_t m[3] = {bytes_of(a), bytes_of(b), bytes_of(c)};
        for (int w = 0; w < 8; ++w) {   // bit i: buffer i is written
          Buf t[3];
          for (int i = 0; i < 3; ++i) t[i] = buf_of(base, *s[i], 1, (w >> i) & 1);
          bool want = false;
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) want = want || (i != j && ((w >> i) & 1) && (m[i] & m[j]));
          CHECK(bufs_clash(t) == want && bufs_clash(t, 3) == want, "clash of (%d,+%d) (%d,+%d) (%d,+%d) written %d at base %zx: want %d",
                a.start, a.len, b.start, b.len, c.start, c.len, w, (size_t)base, (int)want);
        }
      }
  return 0;
}

// every start (and the null pointer) of three buffers with every alignment of {1, 4, 8, 16}; the length plays no part
static int alignments(uintptr_t base) {
  const unsigned aligns[4] = {1, 4, 8, 16};
  int start[3];
  for (start[0] = -1; start[0] < U; ++start[0])   // -1: the null pointer
    for (start[1] = -1; start[1] < U; ++start[1])
      for (start[2] = -1; start[2] < U; ++start[2])
        for (int k = 0; k < 64; ++k) {   // two bits per buffer: its alignment
          Buf t[3];
          int want = -1;
          for (int i = 2; i >= 0; --i) {
            t[i] = buf_of(base, Place{start[i], i, start[i] < 0}, aligns[(k >> (2 * i)) & 3], false);
            if (start[i] >= 0 && (base + (uintptr_t)start[i]) % t[i].align != 0) want = i;
          }
          CHECK(bufs_misaligned(t) == want && bufs_misaligned(t, 3) == want, "misaligned of starts %d %d %d, alignments %d: want %d",
                start[0], start[1], start[2], k, want);
        }
  return 0;
}

int main() {
  alignas(64) static char universe[U];
  const uintptr_t bases[2] = {(uintptr_t)universe, UINTPTR_MAX - (uintptr_t)(U - 1)};
  for (const uintptr_t base : bases) {
    if (base % 16 != 0) return fprintf(stderr, "base %zx is not 16-byte aligned\n", (size_t)base), 1;
    if (pairs(base) || triples(base, 12, 1) || triples(base, U, 4) || alignments(base)) return 1;
  }
  // the ranges that end on the last byte of the address space overlap their neighbours (x + bytes wraps to 0 there)
  for (int k = 0; k < U; ++k) {
    const Buf last = wr((const void*)(UINTPTR_MAX - (uintptr_t)k), (size_t)k + 1);
    const Buf inside = rd((const void*)UINTPTR_MAX, 1), below = rd((const void*)(UINTPTR_MAX - (uintptr_t)k - 8), 9);
    const Buf apart = rd((const void*)(UINTPTR_MAX - (uintptr_t)k - 8), 8);
    CHECK(bufs_overlap(last, inside) && bufs_overlap(inside, last), "the last byte and the last %d bytes", k + 1);
    CHECK(bufs_overlap(last, below) && bufs_overlap(below, last), "a range that reaches into the last %d bytes", k + 1);
    CHECK(!bufs_overlap(last, apart) && !bufs_overlap(apart, last), "a range that ends before the last %d bytes", k + 1);
    const Buf t[3] = {apart, last, inside};
    CHECK(bufs_clash(t), "clash at the top of the address space, k = %d", k);
  }
  printf("ok %ld\n", g_checks);
  return 0;
}

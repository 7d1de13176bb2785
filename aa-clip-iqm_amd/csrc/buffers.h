// The buffers of one C ABI call (csrc/capi.hip): each data-side entry declares ONE table of them -- pointer, byte
// length, alignment, written or read-only -- and its alignment and overlap checks read that table.  Host code only,
// shared with csrc/buffers_host_check.cpp, which replays it against a set-of-bytes model under a sanitizer.
//
// The rule (include/aaclip.h, "Buffers of a call"): every buffer the call writes -- outputs, records, workspace -- is
// disjoint from every other buffer of the call; read-only buffers may alias one another.  A buffer that is absent
// (NULL, or no bytes) overlaps nothing.  A pointer that is given is aligned even where the sizes leave it no bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace aaclip {

struct Buf { const void* p; size_t bytes; unsigned align; bool written; };   // align: a power of two
inline Buf rd(const void* p, size_t bytes, unsigned align = 1) { return Buf{p, bytes, align, false}; }
inline Buf wr(const void* p, size_t bytes, unsigned align = 1) { return Buf{p, bytes, align, true}; }

// [a, a + na) and [b, b + nb) share a byte.  Only differences are formed, so a range that ends on the last byte of the
// address space is compared like any other; an empty range shares nothing.
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na && nb && (x < y ? y - x < na : x - y < nb);
}
inline bool bufs_overlap(const Buf& a, const Buf& b) { return a.p && b.p && ranges_overlap(a.p, a.bytes, b.p, b.bytes); }

// index of the first buffer whose pointer is given and not a multiple of its alignment, or -1
inline int bufs_misaligned(const Buf* b, int n) {
  for (int i = 0; i < n; ++i)
    if (b[i].p && ((uintptr_t)b[i].p & (b[i].align - 1))) return i;
  return -1;
}
// a written buffer overlaps another buffer of the table
inline bool bufs_clash(const Buf* b, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if ((b[i].written || b[j].written) && bufs_overlap(b[i], b[j])) return true;
  return false;
}
template <int N> inline int bufs_misaligned(const Buf (&b)[N]) { return bufs_misaligned(b, N); }
template <int N> inline bool bufs_clash(const Buf (&b)[N]) { return bufs_clash(b, N); }

}  // namespace aaclip

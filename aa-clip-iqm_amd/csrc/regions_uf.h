// Label-equivalence union-find of csrc/regions.hip on a 32-bit parent array, written once for the device and for a host
// program (csrc/regions_host_check.cpp runs it under a sanitizer over adversarial masks in shuffled pixel orders).
// The ACCESS policy supplies the two memory operations:
//   static uint32_t load(const uint32_t* p)          a relaxed atomic (or volatile) load: never hoisted out of a loop
//   static uint32_t min(uint32_t* p, uint32_t v)     atomic minimum, returns the value before it
// Invariant: parent[i] <= i at all times.  Every entry starts as parent[i] = i and is written by ACCESS::min alone, so
// it is only ever lowered.  Both loops below step to a strictly smaller index or stop, which bounds them by the index
// they start from even over a parent array that does not keep the invariant (`p >= i` ends a walk).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AACLIP_UF_HD __host__ __device__ inline
#else
#define AACLIP_UF_HD inline
#endif

namespace aaclip {

template <class ACCESS>
AACLIP_UF_HD uint32_t uf_find(const uint32_t* parent, uint32_t i) {
  for (;;) {
    const uint32_t p = ACCESS::load(parent + i);
    if (p >= i) return i;
    i = p;
  }
}

// The same walk, shortening the path behind it: where i has a grandparent, it takes it as its parent (path halving).
// The grandparent is an ancestor, so i stays in its set; the write is a minimum, so the invariant holds and a lower value
// that another thread has put there meanwhile is kept.  Without it a one-pixel-wide spiral leaves chains as long as the
// component, and every later find walks them.
template <class ACCESS>
AACLIP_UF_HD uint32_t uf_find_halve(uint32_t* parent, uint32_t i) {
  for (;;) {
    const uint32_t p = ACCESS::load(parent + i);
    if (p >= i) return i;
    const uint32_t gp = ACCESS::load(parent + p);
    if (gp < p) ACCESS::min(parent + i, gp);
    i = p;
  }
}

// After the call a and b have one root.  a + b falls in every round that does not return: the larger root either takes
// the smaller one as its parent, or it had been lowered by another union in the meantime (old < a), and the union goes
// on from where it points now -- whichever link the minimum dropped, old -- b is the pair that still has to be joined.
template <class ACCESS>
AACLIP_UF_HD void uf_union(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find_halve<ACCESS>(parent, a);
    b = uf_find_halve<ACCESS>(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = ACCESS::min(parent + a, b);
    if (old >= a) return;   // a was a root and points to b now
    a = old;
  }
}

// The unions of one anomalous pixel i = (img, y, x) with the neighbours that precede it in row-major order: W and N,
// and for connectivity 8 NW and NE.  Where N is set, NW and NE are already joined to it by their own W links.
template <class ACCESS>
AACLIP_UF_HD void uf_merge_pixel(const uint8_t* mask, uint32_t* parent, long i, int H, int W, int connectivity) {
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const uint32_t u = (uint32_t)i;
  if (x > 0 && mask[i - 1]) uf_union<ACCESS>(parent, u, u - 1);
  if (y == 0) return;
  if (mask[i - W]) {
    uf_union<ACCESS>(parent, u, u - (uint32_t)W);
  } else if (connectivity == 8) {
    if (x > 0 && mask[i - W - 1]) uf_union<ACCESS>(parent, u, u - (uint32_t)W - 1);
    if (x + 1 < W && mask[i - W + 1]) uf_union<ACCESS>(parent, u, u - (uint32_t)W + 1);
  }
}

}  // namespace aaclip

// The region table of csrc/region_table.hip, the parts that the device code and a host program share
// (csrc/region_table_host_check.cpp replays the construction sequentially under a sanitizer): the row, the record, the
// order-preserving score key, the packed peak word with its decode, the row's start values and its last step, and the
// workspace layout.
//
// A row is built in three steps.  (1) The root pixel of a kept region (region[p] == p + 1, area >= min_area) starts it:
// image, first, area, the GLOBAL number of the root among all roots in `label`, an empty box, a zero peak word in the
// two words (peak_x, peak_y), overlap 0.  (2) Every pixel of the region lowers x0 / y0, raises x1 / y1 and the peak
// word, adds to overlap -- integer minima, maxima and sums: any order gives the same row.  (3) The last step turns the
// label into the 1-based number within the image and the peak word into peak_x, peak_y, peak.
//
// The peak word is  score key << 32 | (0xFFFFFFFF - flat index within the image) : its maximum over the region's pixels
// is the largest compared score, and among equal scores the lowest index.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "metrics_records.h"

#if defined(__HIPCC__)
#define AACLIP_RT_HD __host__ __device__ inline
#else
#define AACLIP_RT_HD inline
#endif

namespace aaclip {

struct RegionRow {   // include/aaclip.h aaclip_region_row
  uint32_t image, label, first, area, x0, y0, x1, y1, peak_x, peak_y, peak, overlap;
};
static_assert(sizeof(RegionRow) == 48, "a region row is twelve 32-bit words");
static constexpr int REGION_ROW_PEAK_WORD = 8;   // the peak word lives in (peak_x, peak_y): byte 32 of a row, 8-byte aligned

struct RegionTableRecord {   // include/aaclip.h aaclip_region_table_record
  unsigned long long kept, regions, hit, dropped;
};

static constexpr uint32_t REGION_NO_ROW = 0x7FFFFFFFu;   // rowof[] of a root whose region is filtered out
static constexpr uint32_t REGION_HIT_BIT = 0x80000000u;  // rowof[] of a kept root beyond the capacity, once it overlaps

// the ordered image of all 32 bits of a float (metrics.hip's unpacked key): -0.0 as +0.0, the sign flipped for positive
// floats, every bit for negative ones
AACLIP_RT_HD uint32_t region_score_bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b == 0x80000000u ? 0u : b;
}
AACLIP_RT_HD uint32_t region_score_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
AACLIP_RT_HD uint32_t region_key_bits(uint32_t key) { return (key >> 31) ? key ^ 0x80000000u : ~key; }

AACLIP_RT_HD unsigned long long region_peak_pack(uint32_t key, uint32_t index_in_image) {
  return ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - index_in_image);
}
AACLIP_RT_HD uint32_t region_peak_key(unsigned long long word) { return (uint32_t)(word >> 32); }
AACLIP_RT_HD uint32_t region_peak_index(unsigned long long word) { return 0xFFFFFFFFu - (uint32_t)(word & 0xFFFFFFFFull); }

// the compared score: metrics_records.h range_normalised
AACLIP_RT_HD float region_compared(float x, bool norm, float mn, float mx) {
  return range_normalised(x, RangeNorm{norm, mn, mx});
}

AACLIP_RT_HD RegionRow region_row_start(uint32_t image, uint32_t root_number, uint32_t first, uint32_t area, int H, int W) {
  RegionRow r;
  r.image = image, r.label = root_number, r.first = first, r.area = area;
  r.x0 = (uint32_t)W, r.y0 = (uint32_t)H, r.x1 = 0, r.y1 = 0;
  r.peak_x = 0, r.peak_y = 0, r.peak = 0, r.overlap = 0;
  return r;
}

// step (3); word = the row's peak word, roots_before = the number of roots in front of the row's image
AACLIP_RT_HD void region_row_finish(RegionRow* r, unsigned long long word, uint32_t roots_before, int W) {
  const uint32_t index = region_peak_index(word);
  r->label = r->label - roots_before + 1;
  r->peak_x = index % (uint32_t)W;
  r->peak_y = index / (uint32_t)W;
  r->peak = region_key_bits(region_peak_key(word));
}

// ---- the workspace: [rowof: n x 4] [tile words: tiles x 8] [roots before every image: (images + 1) x 4] [totals: 16]
static constexpr int REGION_TABLE_THREADS = 256;
static constexpr int REGION_TABLE_ITEMS = 8;
static constexpr int REGION_TABLE_TILE = REGION_TABLE_THREADS * REGION_TABLE_ITEMS;

struct RegionTableLayout {
  size_t rowof, tile_word, roots_before, total, bytes;
  long tiles;
};
inline RegionTableLayout region_table_layout(long n, long images) {
  RegionTableLayout l;
  l.tiles = (n + REGION_TABLE_TILE - 1) / REGION_TABLE_TILE;
  l.rowof = 0;
  l.tile_word = l.rowof + up256_bytes((size_t)n * 4);
  l.roots_before = l.tile_word + up256_bytes((size_t)l.tiles * 8);
  l.total = l.roots_before + up256_bytes((size_t)(images + 1) * 4);
  l.bytes = l.total + 256;
  return l;
}

}  // namespace aaclip

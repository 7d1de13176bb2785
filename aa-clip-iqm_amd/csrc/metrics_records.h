// The device records that the evaluation entries hand to one another (include/aaclip.h documents them for callers;
// engine.py reads them as int64 words), the one normalisation rule that four kernels apply to a raw score, and the
// workspace layouts of the sort, curve, F1-max and PRO-curve entries: what metrics.hip, regions.hip, region_table.hip
// and overlay.hip share, and a host program may include (region_table_host_check.cpp does, through region_table.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AACLIP_REC_HD __host__ __device__ inline
#else
#define AACLIP_REC_HD inline
#endif

namespace aaclip {

typedef unsigned long long u64;
inline size_t up256_bytes(size_t v) { return (v + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------- records
struct RangeRecord {   // aaclip_metrics_range_record; also the per-workgroup partial of the range kernels
  float mn, mx;
  u64 bad, pos;
};
static_assert(sizeof(RangeRecord) == 24 && offsetof(RangeRecord, mx) == 4 && offsetof(RangeRecord, bad) == 8 &&
                  offsetof(RangeRecord, pos) == 16,
              "engine.metrics_range_host reads min, max in word 0 and the two counts in words 1, 2");

struct CurveRecord {   // aaclip_metrics_curve_record (the sixth word of engine.CURVE_RECORD_WORDS is the sort's)
  u64 num, P, N, groups;
  double ap;
};
static_assert(sizeof(CurveRecord) == 40 && offsetof(CurveRecord, ap) == 32, "five 64-bit words, ap the fifth");

struct F1MaxRecord {   // aaclip_metrics_f1max_record; the threshold kernel reads `threshold`
  u64 tp, fp, P, N, groups, start;
  uint32_t key;
  float threshold;
};
static_assert(sizeof(F1MaxRecord) == 56 && offsetof(F1MaxRecord, key) == 48 && offsetof(F1MaxRecord, threshold) == 52,
              "engine.F1MAX_RECORD_WORDS = 7: the key in the low half of word 6, the threshold bits in the high half");

struct ThresholdRecord {   // aaclip_metrics_threshold_record
  u64 tp, fp, fn, tn;
};
static_assert(sizeof(ThresholdRecord) == 32, "engine.THRESHOLD_RECORD_WORDS = 4");

struct RegionsRecord {   // aaclip_metrics_regions_record; the PRO curve reads `regions`
  u64 regions, anomalous, normal;
};
static_assert(sizeof(RegionsRecord) == 24 && offsetof(RegionsRecord, regions) == 0, "three 64-bit words");

struct ProRecord {   // aaclip_metrics_pro_record
  double aupro;
  u64 regions, normal, groups;
  double y_limit;
};
static_assert(sizeof(ProRecord) == 40 && offsetof(ProRecord, y_limit) == 32, "engine.PRO_RECORD_WORDS = 5");

// ------------------------------------------------------------------------------------------------ normalise
// The compared score of aaclip_metrics_normalise, _threshold, _region_table and _overlay_render: the raw one, or, iff a
// range record is given and its max != 1 (the reference's `if preds.max() != 1`), numpy's float32
// (x - min) / (max - min): one IEEE subtraction and one correctly rounded division (no file is built with contraction).
struct RangeNorm {
  bool on;
  float mn, mx;
};
AACLIP_REC_HD RangeNorm range_norm(const RangeRecord* rec) {
  RangeNorm r{false, 0.0f, 1.0f};
  if (rec) r.mn = rec->mn, r.mx = rec->mx, r.on = rec->mx != 1.0f;
  return r;
}
AACLIP_REC_HD float range_normalised(float x, const RangeNorm& r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return r.on ? __fdiv_rn(__fsub_rn(x, r.mn), __fsub_rn(r.mx, r.mn)) : x;
#else
  return r.on ? (x - r.mn) / (r.mx - r.mn) : x;
#endif
}

// ------------------------------------------------------------------------------------------------- workspaces
// Offsets in bytes from the workspace pointer, every section 256-byte aligned; `bytes` is what *_ws_bytes returns.
static constexpr int METRICS_THREADS = 256;       // threads of every workgroup of these entries (4 waves)
static constexpr int METRICS_SCAN_ITEMS = 16;     // consecutive items of one thread of a tile
static constexpr int METRICS_TILE = METRICS_THREADS * METRICS_SCAN_ITEMS;   // 4096
static constexpr int METRICS_MAX_BLOCKS = 1024;   // workgroups of a group fold = partials its last kernel folds
static constexpr int SORT_ROUNDS = 32;
static constexpr int SORT_CHUNK = 64 * SORT_ROUNDS;   // keys one wave of the sort walks
static constexpr int SCAN_SEGMENTS = 256;             // row segments of the sort's table scan at the most

inline long metrics_tiles(long n) { return (n + METRICS_TILE - 1) / METRICS_TILE; }
inline long metrics_group_blocks(long n) {
  const long b = (n + METRICS_THREADS - 1) / METRICS_THREADS;
  return b < METRICS_MAX_BLOCKS ? b : METRICS_MAX_BLOCKS;
}

// aaclip_metrics_sort (value_bytes 1: the label) and aaclip_metrics_sort_pairs (4):
// [keys B: n uint32] [values B: n values] [table: chunks x 256 uint32] [segment sums: 256 x 256 uint32]
struct SortLayout {
  size_t keys_b, values_b, table, seg_sum, bytes;
  long chunks;
};
inline SortLayout sort_layout(long n, size_t value_bytes) {
  SortLayout l;
  l.chunks = (n + SORT_CHUNK - 1) / SORT_CHUNK;
  l.keys_b = 0;
  l.values_b = l.keys_b + up256_bytes((size_t)n * 4);
  l.table = l.values_b + up256_bytes((size_t)n * value_bytes);
  l.seg_sum = l.table + (size_t)l.chunks * 1024;
  l.bytes = l.seg_sum + (size_t)SCAN_SEGMENTS * 1024;
  return l;
}

// aaclip_metrics_curve and _f1max share the front, [tile sums: tiles x 8] [total: 8] [marks: n x 8]; behind it (`end`)
// the entry's own partials, `parts` of them
struct CurveMarksLayout {
  size_t tile_sum, total, marks, end;
  long tiles;
  int parts;
};
inline CurveMarksLayout curve_marks_layout(long n) {
  CurveMarksLayout m;
  m.tiles = metrics_tiles(n);
  m.parts = (int)metrics_group_blocks(n);
  m.tile_sum = 0;
  m.total = m.tile_sum + up256_bytes((size_t)m.tiles * 8);
  m.marks = m.total + 256;
  m.end = m.marks + up256_bytes((size_t)n * 8);
  return m;
}
struct CurveLayout {   // [front] [partial numerators: parts x 8] [partial AP sums: parts x 8]
  CurveMarksLayout front;
  size_t part_num, part_ap, bytes;
};
inline CurveLayout curve_layout(long n) {
  CurveLayout l;
  l.front = curve_marks_layout(n);
  l.part_num = l.front.end;
  l.part_ap = l.part_num + up256_bytes((size_t)l.front.parts * 8);
  l.bytes = l.part_ap + up256_bytes((size_t)l.front.parts * 8);
  return l;
}
static constexpr size_t F1_CANDIDATE_BYTES = 24;
struct F1MaxLayout {   // [front] [partial candidates: parts x 24]
  CurveMarksLayout front;
  size_t partial, bytes;
};
inline F1MaxLayout f1max_layout(long n) {
  F1MaxLayout l;
  l.front = curve_marks_layout(n);
  l.partial = l.front.end;
  l.bytes = l.partial + up256_bytes((size_t)l.front.parts * F1_CANDIDATE_BYTES);
  return l;
}

// aaclip_metrics_pro_curve: [tile sums: tiles x {word, weight}] [total: 8, y at the limit: 8] [marks fp: n x 4]
// [marks S: n x 8] [partial areas: parts x 8]
struct ProLayout {
  size_t tile_sum, total, marks_fp, marks_s, part, bytes;
  long tiles;
  int parts;
};
inline ProLayout pro_curve_layout(long n) {
  ProLayout l;
  l.tiles = metrics_tiles(n);
  l.parts = (int)metrics_group_blocks(n);
  l.tile_sum = 0;
  l.total = l.tile_sum + 2 * up256_bytes((size_t)l.tiles * 8);
  l.marks_fp = l.total + 256;
  l.marks_s = l.marks_fp + up256_bytes((size_t)n * 4);
  l.part = l.marks_s + up256_bytes((size_t)n * 8);
  l.bytes = l.part + up256_bytes((size_t)l.parts * 8);
  return l;
}

}  // namespace aaclip

// Exact AUROC / average precision of one class on the device (forward_utils.metrics_eval_device), five steps:
//   range      min / max / non-finite count / positive count of the scores, and the maximum of every image
//   normalise  (x - min) / (max - min) in fp32 where max != 1, the bits numpy gives (reference forward_utils.py:246-253)
//   keys       an order-preserving uint32 image of every score; the 0 / 1 label in bit 0 where the scores lie in [0, 1]
//   sort       stable LSD radix sort, four passes of 8-bit digits
//   curve      tie groups of the sorted keys -> integer AUROC numerator and the fp64 AP sum
// and, from the same sorted keys and the curve's own first phases (forward_utils.f1max_eval_device):
//   f1max      the tie group with the largest F1, an integer argmax -> counts, start index, key and fp32 threshold
//   threshold  raw scores -> uint8 masks and tp / fp / fn / tn per image and in all at a threshold read on the device
// The numbers are sklearn's roc_auc_score / average_precision_score: the same tie groups and the same definitions.
// No floating-point atomics; every floating-point sum runs in an order fixed by n alone, so two calls give the same bits.
#include "common.h"
#include "kernels.h"
#include "metrics_records.h"
#include "tile_scan.h"
#include <math.h>

namespace aaclip {

static constexpr int MT = TILE_THREADS;   // threads of every workgroup in this file (4 waves)

// ---------------------------------------------------------------------------------------------------- range
// A SEGMENT is one image (per_image elements), or the whole array when per_image is 0.  Stage 1: blocks_per_segment
// workgroups per segment, each a strided share; stage 2: one workgroup folds the partials in index order.
static constexpr int RANGE_ITEMS = 4096;        // elements of a segment per workgroup before another one is added
static constexpr int RANGE_MAX_BLOCKS = 1024;   // workgroups per segment at the most

long metrics_range_blocks(long seg_len) {
  const long b = (seg_len + RANGE_ITEMS - 1) / RANGE_ITEMS;
  return b < 1 ? 1 : (b < RANGE_MAX_BLOCKS ? b : RANGE_MAX_BLOCKS);
}
long metrics_range_partials(long n, long per_image) {
  const long seg_len = per_image > 0 ? per_image : n;
  return (n / seg_len) * metrics_range_blocks(seg_len);
}
size_t metrics_range_ws_bytes(long n, long per_image) {
  return (size_t)metrics_range_partials(n, per_image) * sizeof(RangeRecord);
}

// min / max of the finite scores and the two counts of a and b; the per-workgroup partial is a RangeRecord itself
AACLIP_DEV RangeRecord range_merge(const RangeRecord& a, const RangeRecord& b) {
  return RangeRecord{fminf(a.mn, b.mn), fmaxf(a.mx, b.mx), a.bad + b.bad, a.pos + b.pos};
}

__global__ __launch_bounds__(MT) void metrics_range_partial_kernel(const float* __restrict__ scores,
                                                                   const uint8_t* __restrict__ labels, long seg_len,
                                                                   int blocks, RangeRecord* __restrict__ partial) {
  __shared__ RangeRecord s_r[MT];
  const long seg = blockIdx.x / blocks;
  const int blk = blockIdx.x % blocks;
  const long base = seg * seg_len;
  RangeRecord r{INFINITY, -INFINITY, 0, 0};
  for (long i = (long)blk * MT + threadIdx.x; i < seg_len; i += (long)blocks * MT) {
    const float x = scores[base + i];
    if (isfinite(x)) {
      r.mn = fminf(r.mn, x);
      r.mx = fmaxf(r.mx, x);
    } else {
      ++r.bad;
    }
    if (labels) r.pos += labels[base + i] != 0;
  }
  r = block_fold(r, s_r, range_merge);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// one workgroup: the record over all partials, then the maximum of every segment
__global__ __launch_bounds__(MT) void metrics_range_fold_kernel(const RangeRecord* __restrict__ partial, long segs,
                                                                int blocks, RangeRecord* __restrict__ rec,
                                                                float* __restrict__ image_max) {
  __shared__ RangeRecord s_r[MT];
  const int t = threadIdx.x;
  const long total = segs * blocks;
  RangeRecord r{INFINITY, -INFINITY, 0, 0};
  for (long i = t; i < total; i += MT) r = range_merge(r, partial[i]);
  r = block_fold(r, s_r, range_merge);
  if (t == 0) *rec = r;
  if (image_max)
    for (long s = t; s < segs; s += MT) {
      float m = -INFINITY;
      for (int b = 0; b < blocks; ++b) m = fmaxf(m, partial[s * blocks + b].mx);
      image_max[s] = m;
    }
}

void launch_metrics_range(const float* scores, const uint8_t* labels, long n, long per_image, float* image_max,
                          void* record, void* ws, hipStream_t s) {
  const long seg_len = per_image > 0 ? per_image : n;
  const long segs = n / seg_len;
  const int blocks = (int)metrics_range_blocks(seg_len);
  RangeRecord* partial = (RangeRecord*)ws;
  hipLaunchKernelGGL(metrics_range_partial_kernel, dim3((unsigned)(segs * blocks)), dim3(MT), 0, s, scores, labels,
                     seg_len, blocks, partial);
  hipLaunchKernelGGL(metrics_range_fold_kernel, dim3(1), dim3(MT), 0, s, partial, segs, blocks, (RangeRecord*)record,
                     image_max);
}

// ------------------------------------------------------------------------------------------------ normalise
// metrics_records.h range_normalised, the decision read from the device record
__global__ __launch_bounds__(MT) void metrics_normalise_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               long n, const RangeRecord* __restrict__ rec) {
  const long i = (long)blockIdx.x * MT + threadIdx.x;
  if (i >= n) return;
  out[i] = range_normalised(in[i], range_norm(rec));
}

void launch_metrics_normalise(const float* in, float* out, long n, const void* record, hipStream_t s) {
  hipLaunchKernelGGL(metrics_normalise_kernel, dim3((unsigned)((n + MT - 1) / MT)), dim3(MT), 0, s, in, out, n,
                     (const RangeRecord*)record);
}

// ----------------------------------------------------------------------------------------------------- keys
// -0.0 becomes +0.0 first, so that equal floats share one key.  packed: the scores lie in [0, 1], their bit pattern is
// at most 0x3F800000 < 2^30 and already ordered: key = bits << 1 | label.  A score outside [0, 1] is counted in
// *out_of_range (an integer atomic; the caller refuses the result).  Otherwise the key is the usual ordered image of
// all 32 bits (sign flipped for positive floats, every bit for negative ones) and the label travels beside it.
__global__ __launch_bounds__(MT) void metrics_keys_kernel(const float* __restrict__ scores,
                                                          const uint8_t* __restrict__ labels, long n, int packed,
                                                          uint32_t* __restrict__ keys, u64* __restrict__ out_of_range) {
  const long i = (long)blockIdx.x * MT + threadIdx.x;
  if (i >= n) return;
  uint32_t b = __float_as_uint(scores[i]);
  if (b == 0x80000000u) b = 0;
  if (packed) {
    if (b > 0x3F800000u) {
      atomicAdd(out_of_range, 1ull);
      b = 0x3F800000u;
    }
    keys[i] = (b << 1) | (labels[i] != 0 ? 1u : 0u);
  } else {
    keys[i] = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  }
}

// ----------------------------------------------------------------------------------------------------- sort
// The unit of the sort is a CHUNK: 2048 consecutive keys, walked by one wave in 32 rounds of 64.  A workgroup is four
// waves = four chunks; every chunk has its own row of the digit table [chunks][256].  Per pass:
//   histogram   digit counts of every chunk (integer LDS atomics)                             -> table
//   scan        table <- exclusive prefix in (digit, chunk) order = the first output index of every (chunk, digit):
//               column sums of row segments, one workgroup over the segment sums and the 256 digit totals, apply
//   scatter     a wave walks its chunk in index order; in a round, the lanes that hold the same digit find each other
//               with eight ballots, rank themselves by lane number, and the lowest of them advances the chunk's
//               counter of that digit: equal digits keep their input order, which makes the sort stable
static constexpr int SORT_WAVES = MT / 64;   // SORT_ROUNDS, SORT_CHUNK, SCAN_SEGMENTS: metrics_records.h

long metrics_sort_group_items() { return (long)SORT_CHUNK * SORT_WAVES; }

__global__ __launch_bounds__(MT) void sort_hist_kernel(const uint32_t* __restrict__ keys, long n, int shift,
                                                       uint32_t* __restrict__ table, long chunks) {
  __shared__ uint32_t cnt[SORT_WAVES][256];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) cnt[w][lane + 64 * k] = 0;
  __syncthreads();
  const long chunk = (long)blockIdx.x * SORT_WAVES + w;
  const long base = chunk * SORT_CHUNK;
  if (chunk < chunks) {
#pragma unroll 4
    for (int r = 0; r < SORT_ROUNDS; ++r) {
      const long i = base + r * 64 + lane;
      if (i < n) atomicAdd(&cnt[w][(keys[i] >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  if (chunk < chunks) {
#pragma unroll
    for (int k = 0; k < 4; ++k) table[chunk * 256 + lane + 64 * k] = cnt[w][lane + 64 * k];
  }
}

// grid = segments; thread d: seg_sum[s][d] = sum of column d over the segment's rows
__global__ __launch_bounds__(MT) void sort_scan_sum_kernel(const uint32_t* __restrict__ table, long chunks, long seg_len,
                                                           uint32_t* __restrict__ seg_sum) {
  const long r0 = (long)blockIdx.x * seg_len, r1 = r0 + seg_len < chunks ? r0 + seg_len : chunks;
  uint32_t acc = 0;
  for (long r = r0; r < r1; ++r) acc += table[r * 256 + threadIdx.x];
  seg_sum[(long)blockIdx.x * 256 + threadIdx.x] = acc;
}

// one workgroup; thread d: seg_sum[.][d] <- (keys with a smaller digit) + (keys of digit d in earlier segments)
__global__ __launch_bounds__(MT) void sort_scan_base_kernel(uint32_t* __restrict__ seg_sum, int segments) {
  __shared__ uint32_t base[256];
  const int d = threadIdx.x;
  uint32_t total = 0;
  for (int s = 0; s < segments; ++s) total += seg_sum[s * 256 + d];
  base[d] = total;
  __syncthreads();
  if (d == 0) {
    uint32_t run = 0;
    for (int j = 0; j < 256; ++j) {
      const uint32_t c = base[j];
      base[j] = run;
      run += c;
    }
  }
  __syncthreads();
  uint32_t run = base[d];
  for (int s = 0; s < segments; ++s) {
    const uint32_t c = seg_sum[s * 256 + d];
    seg_sum[s * 256 + d] = run;
    run += c;
  }
}

// grid = segments; thread d walks its column over the segment's rows: count -> first output index
__global__ __launch_bounds__(MT) void sort_scan_apply_kernel(uint32_t* __restrict__ table, long chunks, long seg_len,
                                                             const uint32_t* __restrict__ seg_sum) {
  const long r0 = (long)blockIdx.x * seg_len, r1 = r0 + seg_len < chunks ? r0 + seg_len : chunks;
  uint32_t run = seg_sum[(long)blockIdx.x * 256 + threadIdx.x];
  for (long r = r0; r < r1; ++r) {
    const uint32_t c = table[r * 256 + threadIdx.x];
    table[r * 256 + threadIdx.x] = run;
    run += c;
  }
}

// V: what travels beside the key -- the label byte of aaclip_metrics_sort, the 32-bit value of aaclip_metrics_sort_pairs
template <typename V>
__global__ __launch_bounds__(MT) void sort_scatter_kernel(const uint32_t* __restrict__ keys_in,
                                                          uint32_t* __restrict__ keys_out,
                                                          const V* __restrict__ lab_in,
                                                          V* __restrict__ lab_out, long n, int shift,
                                                          const uint32_t* __restrict__ table, long chunks) {
  __shared__ uint32_t first[SORT_WAVES][256];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long chunk = (long)blockIdx.x * SORT_WAVES + w;
  if (chunk < chunks) {
#pragma unroll
    for (int k = 0; k < 4; ++k) first[w][lane + 64 * k] = table[chunk * 256 + lane + 64 * k];
  }
  __syncthreads();
  if (chunk >= chunks) return;
  // from here on a wave only touches its own row of `first`: the lanes of a wave run in lockstep, the accesses are
  // volatile and separated by wave barriers, so a round reads the counters the round before it left
  volatile uint32_t* mine = first[w];
  const u64 below = (1ull << lane) - 1;
  const long base = chunk * SORT_CHUNK;
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    if (base + r * 64 >= n) break;   // the same for every lane
    const long i = base + r * 64 + lane;
    const bool valid = i < n;
    const uint32_t key = valid ? keys_in[i] : 0u;
    const uint32_t d = (key >> shift) & 255u;
    u64 same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const u64 vote = __ballot(bit);
      same &= bit ? vote : ~vote;
    }
    const uint32_t rank = (uint32_t)__popcll(same & below);
    const uint32_t start = mine[d];
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) mine[d] = start + (uint32_t)__popcll(same);
    __builtin_amdgcn_wave_barrier();
    const uint32_t pos = start + rank;
    if (valid && (long)pos < n) {   // pos < n holds whenever the table is the scan of this input's histogram
      keys_out[pos] = key;
      if (lab_in) lab_out[pos] = lab_in[i];
    }
  }
}

// The four passes: keys ping-pong between `keys` and keys_b and are back in `keys` at the end; what travels beside them
// (nothing when v_in is null) starts in v_in, ping-pongs between v_b and v_out and ends in v_out.
template <typename V>
static void sort_passes(uint32_t* keys, uint32_t* keys_b, const V* v_in, V* v_out, V* v_b, uint32_t* table,
                        uint32_t* seg_sum, long n, long chunks, hipStream_t s) {
  const long seg_len = (chunks + SCAN_SEGMENTS - 1) / SCAN_SEGMENTS;
  const int segments = (int)((chunks + seg_len - 1) / seg_len);
  const unsigned groups = (unsigned)((chunks + SORT_WAVES - 1) / SORT_WAVES);
  for (int pass = 0; pass < 4; ++pass) {
    const uint32_t* src = pass & 1 ? keys_b : keys;
    uint32_t* dst = pass & 1 ? keys : keys_b;
    const V* vsrc = !v_in ? nullptr : (pass == 0 ? v_in : (pass & 1 ? v_b : v_out));
    V* vdst = !v_in ? nullptr : (pass & 1 ? v_out : v_b);
    hipLaunchKernelGGL(sort_hist_kernel, dim3(groups), dim3(MT), 0, s, src, n, 8 * pass, table, chunks);
    hipLaunchKernelGGL(sort_scan_sum_kernel, dim3(segments), dim3(MT), 0, s, table, chunks, seg_len, seg_sum);
    hipLaunchKernelGGL(sort_scan_base_kernel, dim3(1), dim3(MT), 0, s, seg_sum, segments);
    hipLaunchKernelGGL(sort_scan_apply_kernel, dim3(segments), dim3(MT), 0, s, table, chunks, seg_len, seg_sum);
    hipLaunchKernelGGL(sort_scatter_kernel<V>, dim3(groups), dim3(MT), 0, s, src, dst, vsrc, vdst, n, 8 * pass, table,
                       chunks);
  }
}

size_t metrics_sort_ws_bytes(long n) { return sort_layout(n, 1).bytes; }

// The keys start in `keys` and are back there after the fourth pass; so are the labels in `labels_sorted`.
void launch_metrics_sort(const float* scores, const uint8_t* labels, long n, int packed, uint32_t* keys,
                         uint8_t* labels_sorted, unsigned long long* out_of_range, void* ws, hipStream_t s) {
  const SortLayout l = sort_layout(n, 1);
  char* p = (char*)ws;
  (void)hipMemsetAsync(out_of_range, 0, sizeof(u64), s);
  hipLaunchKernelGGL(metrics_keys_kernel, dim3((unsigned)((n + MT - 1) / MT)), dim3(MT), 0, s, scores, labels, n, packed,
                     keys, out_of_range);
  sort_passes<uint8_t>(keys, (uint32_t*)(p + l.keys_b), packed ? nullptr : labels, labels_sorted,
                       (uint8_t*)(p + l.values_b), (uint32_t*)(p + l.table), (uint32_t*)(p + l.seg_sum), n, l.chunks, s);
}

size_t metrics_sort_pairs_ws_bytes(long n) { return sort_layout(n, 4).bytes; }

// The same four passes with a 32-bit value beside the unpacked key.
void launch_metrics_sort_pairs(const float* scores, const uint32_t* values, long n, uint32_t* keys,
                               uint32_t* values_sorted, void* ws, hipStream_t s) {
  const SortLayout l = sort_layout(n, 4);
  char* p = (char*)ws;
  hipLaunchKernelGGL(metrics_keys_kernel, dim3((unsigned)((n + MT - 1) / MT)), dim3(MT), 0, s, scores,
                     (const uint8_t*)nullptr, n, 0, keys, (u64*)nullptr);
  sort_passes<uint32_t>(keys, (uint32_t*)(p + l.keys_b), values, values_sorted, (uint32_t*)(p + l.values_b),
                        (uint32_t*)(p + l.table), (uint32_t*)(p + l.seg_sum), n, l.chunks, s);
}

// ---------------------------------------------------------------------------------------------------- curve
// Over the ascending keys, element i STARTS a tie group when i == 0 or its score differs from that of i - 1; read from
// the top (descending thresholds, as sklearn walks them) that element is the last of its group.  One prefix sum of
// 64-bit words (start << 32 | label) gives, at every start i, the number of groups before it and E = the positives
// before it; both are below 2^31, so the halves never meet.  Three levels: sums of tiles of 4096, one workgroup over
// the tile sums, then the tiles again, which write the compact list marks[g] = i << 32 | E.
// Group g = [i, i2) with i2 the next start (n after the last one), E2 likewise (P after the last one):
//   tp = P - E, fp = (n - i) - tp at its mark; tp0 = P - E2, fp0 = (n - i2) - tp0 at the mark before it (0, 0 for the
//   top group).  num += (fp - fp0)(tp + tp0) in uint64 (at most n^2 / 2 < 2^61);
//   AP += ((tp - tp0) / P) (tp / (tp + fp)) in fp64.
static constexpr int CURVE_ITEMS = METRICS_SCAN_ITEMS;

AACLIP_DEV u64 curve_word(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ lab, long i, int packed) {
  const uint32_t k = keys[i];
  const uint32_t score = packed ? k >> 1 : k;
  const u64 label = packed ? (k & 1u) : (lab[i] != 0 ? 1u : 0u);
  bool start = i == 0;
  if (!start) {
    const uint32_t kp = keys[i - 1];
    start = (packed ? kp >> 1 : kp) != score;
  }
  return ((u64)start << 32) | label;
}

// the three levels of tile_scan.h on the words
__global__ __launch_bounds__(MT) void curve_tile_sum_kernel(const uint32_t* __restrict__ keys,
                                                            const uint8_t* __restrict__ lab, long n, int packed,
                                                            u64* __restrict__ tile_sum) {
  tile_sum_body<CURVE_ITEMS, u64>(n, tile_sum, [=](long i) { return curve_word(keys, lab, i, packed); });
}

// one workgroup: tile_sum <- its exclusive prefix, *total <- the sum of all (groups << 32 | positives)
__global__ __launch_bounds__(MT) void curve_tile_scan_kernel(u64* __restrict__ tile_sum, long tiles,
                                                             u64* __restrict__ total) {
  const u64 all = tile_scan_body(tile_sum, tiles);
  if (threadIdx.x == 0) *total = all;
}

__global__ __launch_bounds__(MT) void curve_mark_kernel(const uint32_t* __restrict__ keys,
                                                        const uint8_t* __restrict__ lab, long n, int packed,
                                                        const u64* __restrict__ tile_prefix, u64* __restrict__ marks) {
  tile_walk_body<CURVE_ITEMS, u64>(
      n, tile_prefix, [=](long i) { return curve_word(keys, lab, i, packed); },
      [=](long i, u64 word, u64 run) {
        const u64 g = run >> 32;
        if ((word >> 32) && g < (u64)n) marks[g] = ((u64)i << 32) | (run & 0xFFFFFFFFull);   // g < groups <= n
      });
}

// Workgroup b sums a contiguous share of the groups, counted from the top; a thread takes every 256th of them, the
// threads are folded by block_fold: the order depends on n and the number of groups alone.
struct CurveSums {
  u64 num;
  double ap;
};
__global__ __launch_bounds__(MT) void curve_group_kernel(const u64* __restrict__ marks, const u64* __restrict__ total,
                                                         long n, u64* __restrict__ part_num,
                                                         double* __restrict__ part_ap) {
  __shared__ CurveSums s_sum[MT];
  const u64 tot = *total;
  const long G = (long)(tot >> 32), P = (long)(tot & 0xFFFFFFFFull);
  const GroupShare share = group_share(G);
  u64 num = 0;
  double ap = 0.0;
  for (long k = share.k0 + threadIdx.x; k < share.k1; k += MT) {
    const long g = G - 1 - k;
    const u64 a = marks[g];
    const long i = (long)(a >> 32), E = (long)(a & 0xFFFFFFFFull);
    long i2 = n, E2 = P;
    if (g + 1 < G) {
      const u64 b = marks[g + 1];
      i2 = (long)(b >> 32), E2 = (long)(b & 0xFFFFFFFFull);
    }
    const long tp = P - E, fp = (n - i) - tp, tp0 = P - E2, fp0 = (n - i2) - tp0;
    num += (u64)(fp - fp0) * (u64)(tp + tp0);
    ap += ((double)(tp - tp0) / (double)P) * ((double)tp / (double)(tp + fp));
  }
  const CurveSums all = block_fold(CurveSums{num, ap}, s_sum, [](const CurveSums& a, const CurveSums& b) {
    return CurveSums{a.num + b.num, a.ap + b.ap};
  });
  if (threadIdx.x == 0) part_num[blockIdx.x] = all.num, part_ap[blockIdx.x] = all.ap;
}

// the partials in index order, by one thread
__global__ void curve_final_kernel(const u64* __restrict__ part_num, const double* __restrict__ part_ap, int parts,
                                   const u64* __restrict__ total, long n, CurveRecord* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  u64 num = 0;
  double ap = 0.0;
  for (int j = 0; j < parts; ++j) {
    num += part_num[j];
    ap += part_ap[j];
  }
  const u64 tot = *total;
  const u64 P = tot & 0xFFFFFFFFull;
  rec->num = num, rec->P = P, rec->N = (u64)n - P, rec->groups = tot >> 32, rec->ap = ap;
}

// The phases that aaclip_metrics_curve and aaclip_metrics_f1max share: tile sums, their scan, the mark list
// (total: groups << 32 | positives; marks[g] = i << 32 | E, ascending).
static void launch_curve_marks(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed,
                               const CurveMarksLayout& m, char* p, hipStream_t s) {
  u64 *tile_sum = (u64*)(p + m.tile_sum), *total = (u64*)(p + m.total), *marks = (u64*)(p + m.marks);
  const long tiles = m.tiles;
  hipLaunchKernelGGL(curve_tile_sum_kernel, dim3((unsigned)tiles), dim3(MT), 0, s, keys, labels_sorted, n, packed,
                     tile_sum);
  hipLaunchKernelGGL(curve_tile_scan_kernel, dim3(1), dim3(MT), 0, s, tile_sum, tiles, total);
  hipLaunchKernelGGL(curve_mark_kernel, dim3((unsigned)tiles), dim3(MT), 0, s, keys, labels_sorted, n, packed, tile_sum,
                     marks);
}

size_t metrics_curve_ws_bytes(long n) { return curve_layout(n).bytes; }

void launch_metrics_curve(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed, void* record, void* ws,
                          hipStream_t s) {
  const CurveLayout l = curve_layout(n);
  char* p = (char*)ws;
  const int parts = l.front.parts;
  u64 *total = (u64*)(p + l.front.total), *marks = (u64*)(p + l.front.marks), *part_num = (u64*)(p + l.part_num);
  double* part_ap = (double*)(p + l.part_ap);
  launch_curve_marks(keys, labels_sorted, n, packed, l.front, p, s);
  hipLaunchKernelGGL(curve_group_kernel, dim3(parts), dim3(MT), 0, s, marks, total, n, part_num, part_ap);
  hipLaunchKernelGGL(curve_final_kernel, dim3(1), dim3(64), 0, s, part_num, part_ap, parts, total, n,
                     (CurveRecord*)record);
}

// ---------------------------------------------------------------------------------------------------- F1-max
// After the group that starts at ascending index i (walking down from the top, everything from i on is flagged):
// tp = P - E, m = n - i, F1 = 2 tp / (m + P).  A CANDIDATE is (tp, d = m + P, i); a beats b when tp_a d_b > tp_b d_a
// -- tp < 2^31 and d < 2^32, so the products are exact in uint64 -- and, at equal products, when i_a > i_b (the higher
// score).  (ratio, i) is a strict total order over the groups: whichever way they are shared out and folded, the same
// one wins.  d = 0 marks "no candidate" (a real d is at least 1).  Integers only, no atomics.
struct F1Candidate {
  u64 tp, d, i;
};
static_assert(sizeof(F1Candidate) == F1_CANDIDATE_BYTES, "f1max_layout sizes the partials");

AACLIP_DEV bool f1_beats(const F1Candidate& a, const F1Candidate& b) {
  if (a.d == 0) return false;
  if (b.d == 0) return true;
  const u64 l = a.tp * b.d, r = b.tp * a.d;
  return l > r || (l == r && a.i > b.i);
}

// the workgroup's best candidate
AACLIP_DEV F1Candidate f1_block_best(F1Candidate best, F1Candidate* lds) {
  return block_fold(best, lds, [](const F1Candidate& mine, const F1Candidate& other) {
    return f1_beats(other, mine) ? other : mine;
  });
}

// Workgroup b takes a contiguous share of the groups, a thread every 256th of them.
__global__ __launch_bounds__(MT) void f1max_group_kernel(const u64* __restrict__ marks, const u64* __restrict__ total,
                                                         long n, F1Candidate* __restrict__ partial) {
  __shared__ F1Candidate lds[MT];
  const u64 tot = *total;
  const u64 P = tot & 0xFFFFFFFFull;
  const GroupShare share = group_share((long)(tot >> 32));
  F1Candidate best{0, 0, 0};
  for (long g = share.k0 + threadIdx.x; g < share.k1; g += MT) {
    const u64 a = marks[g];
    const u64 i = a >> 32, E = a & 0xFFFFFFFFull;
    const F1Candidate c{P - E, ((u64)n - i) + P, i};
    if (f1_beats(c, best)) best = c;
  }
  best = f1_block_best(best, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// one workgroup over the partials; thread 0 writes the record
__global__ __launch_bounds__(MT) void f1max_final_kernel(const F1Candidate* __restrict__ partial, int parts,
                                                         const u64* __restrict__ total, long n,
                                                         const uint32_t* __restrict__ keys, int packed,
                                                         F1MaxRecord* __restrict__ rec) {
  __shared__ F1Candidate lds[MT];
  F1Candidate best{0, 0, 0};
  for (int j = threadIdx.x; j < parts; j += MT) {
    const F1Candidate c = partial[j];
    if (f1_beats(c, best)) best = c;
  }
  best = f1_block_best(best, lds);
  if (threadIdx.x != 0) return;
  const u64 tot = *total;
  const u64 P = tot & 0xFFFFFFFFull;
  const u64 start = best.i < (u64)n ? best.i : 0;   // i < n whenever the marks are those of these keys
  const uint32_t k = keys[start];
  const uint32_t score = packed ? k >> 1 : k;
  const uint32_t bits = packed ? score : ((score >> 31) ? score ^ 0x80000000u : ~score);
  rec->tp = best.tp, rec->fp = (best.d - P) - best.tp, rec->P = P, rec->N = (u64)n - P, rec->groups = tot >> 32;
  rec->start = start, rec->key = score, rec->threshold = __uint_as_float(bits);
}

size_t metrics_f1max_ws_bytes(long n) { return f1max_layout(n).bytes; }

void launch_metrics_f1max(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed, void* record, void* ws,
                          hipStream_t s) {
  const F1MaxLayout l = f1max_layout(n);
  char* p = (char*)ws;
  const int parts = l.front.parts;
  u64 *total = (u64*)(p + l.front.total), *marks = (u64*)(p + l.front.marks);
  F1Candidate* partial = (F1Candidate*)(p + l.partial);
  launch_curve_marks(keys, labels_sorted, n, packed, l.front, p, s);
  hipLaunchKernelGGL(f1max_group_kernel, dim3(parts), dim3(MT), 0, s, marks, total, n, partial);
  hipLaunchKernelGGL(f1max_final_kernel, dim3(1), dim3(MT), 0, s, partial, parts, total, n, keys, packed,
                     (F1MaxRecord*)record);
}

// ------------------------------------------------------------------------------------------------- threshold
// flagged = (v >= threshold), v the raw score or, with a range record, range_normalised's.  Segments and
// workgroups per segment are those of the range kernels.  Within a segment the elements in front of the first 16-byte
// aligned score (at most 3) and behind the last whole quad (at most 3) are taken one by one by the segment's first
// workgroup; the quads in between are read with one 128-bit load each, their four mask bytes stored as one word where
// the mask's address at the quad is 4-byte aligned (the same for every quad of a segment), byte by byte otherwise; the
// labels likewise.  Counts are integers: stage 1 leaves {tp, fp, fn, tn} per workgroup, stage 2 folds them.
AACLIP_DEV void threshold_count(bool flag, bool pos, uint32_t& tp, uint32_t& fp, uint32_t& fn, uint32_t& tn) {
  tp += flag && pos, fp += flag && !pos, fn += !flag && pos, tn += !flag && !pos;
}

__global__ __launch_bounds__(MT) void metrics_threshold_kernel(const float* __restrict__ scores,
                                                               const uint8_t* __restrict__ labels, long seg_len,
                                                               int blocks, const RangeRecord* __restrict__ range,
                                                               const F1MaxRecord* __restrict__ f1,
                                                               uint8_t* __restrict__ mask, uint4* __restrict__ partial) {
  __shared__ uint4 s_c[MT];
  const long seg = blockIdx.x / blocks;
  const int blk = blockIdx.x % blocks, t = threadIdx.x;
  const long base = seg * seg_len;
  const float thr = f1->threshold;
  const RangeNorm norm = range_norm(range);
  // head: elements in front of the first 16-byte aligned score of the segment
  long head = (long)(((16 - ((uintptr_t)(scores + base) & 15)) & 15) >> 2);
  if (head > seg_len) head = seg_len;
  const long quads = (seg_len - head) >> 2;
  const long tail0 = head + 4 * quads;   // first element behind the quads
  uint32_t tp = 0, fp = 0, fn = 0, tn = 0;
  if (blk == 0) {
    long i = -1;
    if (t < head) i = t;
    else if (t - head < seg_len - tail0) i = tail0 + (t - head);
    if (i >= 0) {
      const bool flag = range_normalised(scores[base + i], norm) >= thr;
      if (mask) mask[base + i] = flag ? 1 : 0;
      threshold_count(flag, labels && labels[base + i] != 0, tp, fp, fn, tn);
    }
  }
  const float4* q4 = reinterpret_cast<const float4*>(scores + base + head);
  const bool mask_word = mask && ((uintptr_t)(mask + base + head) & 3) == 0;
  const bool label_word = labels && ((uintptr_t)(labels + base + head) & 3) == 0;
  for (long q = (long)blk * MT + t; q < quads; q += (long)blocks * MT) {
    const float4 x = q4[q];
    const long e = base + head + 4 * q;
    uint32_t lab = 0;   // the four label bytes, element 0 in the low byte
    if (label_word) {
      lab = *reinterpret_cast<const uint32_t*>(labels + e);
    } else if (labels) {
      lab = (uint32_t)labels[e] | ((uint32_t)labels[e + 1] << 8) | ((uint32_t)labels[e + 2] << 16) |
            ((uint32_t)labels[e + 3] << 24);
    }
    const bool f0 = range_normalised(x.x, norm) >= thr, f1b = range_normalised(x.y, norm) >= thr;
    const bool f2 = range_normalised(x.z, norm) >= thr, f3 = range_normalised(x.w, norm) >= thr;
    if (mask_word) {
      *reinterpret_cast<uint32_t*>(mask + e) =
          (uint32_t)f0 | ((uint32_t)f1b << 8) | ((uint32_t)f2 << 16) | ((uint32_t)f3 << 24);
    } else if (mask) {
      mask[e] = f0, mask[e + 1] = f1b, mask[e + 2] = f2, mask[e + 3] = f3;
    }
    threshold_count(f0, (lab & 0xFFu) != 0, tp, fp, fn, tn);
    threshold_count(f1b, (lab & 0xFF00u) != 0, tp, fp, fn, tn);
    threshold_count(f2, (lab & 0xFF0000u) != 0, tp, fp, fn, tn);
    threshold_count(f3, (lab & 0xFF000000u) != 0, tp, fp, fn, tn);
  }
  const uint4 all = block_fold(make_uint4(tp, fp, fn, tn), s_c, [](const uint4& a, const uint4& b) {
    return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  });
  if (t == 0) partial[blockIdx.x] = all;
}

// one workgroup: every image's counts from its workgroups in index order, and the totals over all partials
__global__ __launch_bounds__(MT) void metrics_threshold_fold_kernel(const uint4* __restrict__ partial, long segs,
                                                                    int blocks, uint32_t* __restrict__ image_counts,
                                                                    ThresholdRecord* __restrict__ totals) {
  __shared__ ThresholdRecord s_c[MT];
  const int t = threadIdx.x;
  if (image_counts)
    for (long s = t; s < segs; s += MT) {
      uint32_t tp = 0, fp = 0, fn = 0, tn = 0;
      for (int b = 0; b < blocks; ++b) {
        const uint4 p = partial[s * blocks + b];
        tp += p.x, fp += p.y, fn += p.z, tn += p.w;
      }
      uint32_t* out = image_counts + 4 * s;   // 4-byte aligned only
      out[0] = tp, out[1] = fp, out[2] = fn, out[3] = tn;
    }
  if (!totals) return;   // the same for every thread
  u64 tp = 0, fp = 0, fn = 0, tn = 0;
  const long all = segs * blocks;
  for (long j = t; j < all; j += MT) {
    const uint4 p = partial[j];
    tp += p.x, fp += p.y, fn += p.z, tn += p.w;
  }
  const ThresholdRecord sum =
      block_fold(ThresholdRecord{tp, fp, fn, tn}, s_c, [](const ThresholdRecord& a, const ThresholdRecord& b) {
        return ThresholdRecord{a.tp + b.tp, a.fp + b.fp, a.fn + b.fn, a.tn + b.tn};
      });
  if (t == 0) *totals = sum;
}

size_t metrics_threshold_ws_bytes(long n, long per_image) {
  return (size_t)metrics_range_partials(n, per_image) * sizeof(uint4);
}

// ws: [partials: segments x workgroups per segment x {tp, fp, fn, tn} uint32]
void launch_metrics_threshold(const float* scores, const uint8_t* labels, long n, long per_image,
                              const void* range_record, const void* f1max_record, uint8_t* mask,
                              uint32_t* image_counts, void* totals, void* ws, hipStream_t s) {
  const long seg_len = per_image > 0 ? per_image : n;
  const long segs = n / seg_len;
  const int blocks = (int)metrics_range_blocks(seg_len);
  uint4* partial = (uint4*)ws;
  hipLaunchKernelGGL(metrics_threshold_kernel, dim3((unsigned)(segs * blocks)), dim3(MT), 0, s, scores, labels, seg_len,
                     blocks, (const RangeRecord*)range_record, (const F1MaxRecord*)f1max_record, mask, partial);
  if (image_counts || totals)
    hipLaunchKernelGGL(metrics_threshold_fold_kernel, dim3(1), dim3(MT), 0, s, partial, segs, blocks, image_counts,
                       (ThresholdRecord*)totals);
}

}  // namespace aaclip

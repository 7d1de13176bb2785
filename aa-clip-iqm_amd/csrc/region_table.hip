// The table of the regions of aaclip_metrics_regions (forward_utils.defects_eval_device): one row per connected
// component of at least min_area pixels, in the canonical order of the region ids, with its image, scipy's label number,
// first pixel, area, bounding box, peak score and position, and its overlap with a second mask.  Five launches:
//   tile sums   roots (region[p] == p + 1) and kept roots (area >= min_area) of every tile of 2048 pixels
//   tile scan   one workgroup: exclusive prefix of the tile sums, the totals, the record
//   rows        a root's number among all roots and among the kept ones from ballots within the wave, the wave counts of
//               the tile and the tile prefix; the kept root starts its row (region_table.h) and leaves the row number in
//               rowof[root]; the first pixel of an image leaves the two counts in front of it
//   accumulate  the streaming pass over region, area, scores and the other mask: within a wave, lanes that follow one
//               another in one region and one image row form a run; the run's peak comes from a segmented 32-bit
//               maximum scan and two ballots, its box from its two ends, its overlap from a population count.  The last
//               lane of a run looks the row up and folds the run into one of 16 accumulators in the LDS (claimed by row
//               number; a run whose slot belongs to another row goes to the row itself); the workgroup then issues one
//               integer atomic per field and claimed slot.  A wave without a kept pixel leaves after its loads
//   finish     label within the image, peak word -> peak_x, peak_y, peak; the kept regions with an overlap
// Integer minima, maxima and sums only: no floating-point atomics, and no output depends on the order of execution.
#include "common.h"
#include "kernels.h"
#include "region_table.h"
#include "tile_scan.h"

namespace aaclip {

static constexpr int TT = REGION_TABLE_THREADS, TI = REGION_TABLE_ITEMS, TILE = REGION_TABLE_TILE;
static constexpr int TW = TT / 64;   // waves of a workgroup
static_assert(TT == TILE_THREADS, "the tile scan is tile_scan.h's");

AACLIP_DEV void table_flags(const uint32_t* __restrict__ region, const uint32_t* __restrict__ area, long n, long p,
                            uint32_t min_area, bool& root, bool& kept) {
  root = kept = false;
  if (p < n && region[p] == (uint32_t)p + 1u) {
    root = true;
    kept = area[p] >= min_area;
  }
}

__global__ __launch_bounds__(TT) void table_tile_sum_kernel(const uint32_t* __restrict__ region,
                                                            const uint32_t* __restrict__ area, long n, uint32_t min_area,
                                                            u64* __restrict__ tile_word) {
  __shared__ u64 s_w[TW];
  const int t = threadIdx.x;
  const long tile0 = (long)blockIdx.x * TILE;
  u64 word = 0;   // roots << 32 | kept
#pragma unroll
  for (int k = 0; k < TI; ++k) {
    bool root, kept;
    table_flags(region, area, n, tile0 + (long)k * TT + t, min_area, root, kept);
    word += ((u64)root << 32) | (u64)kept;
  }
  for (int o = 32; o > 0; o >>= 1) word += __shfl_down(word, o);
  if ((t & 63) == 0) s_w[t >> 6] = word;
  __syncthreads();
  if (t == 0) {
    u64 all = 0;
    for (int w = 0; w < TW; ++w) all += s_w[w];
    tile_word[blockIdx.x] = all;
  }
}

// one workgroup: tile sums <- their exclusive prefix; the record, the last offset and the last root count
__global__ __launch_bounds__(TT) void table_tile_scan_kernel(u64* __restrict__ tile_word, long tiles, long capacity,
                                                             long images, int32_t* __restrict__ image_offsets,
                                                             uint32_t* __restrict__ roots_before,
                                                             RegionTableRecord* __restrict__ rec) {
  const u64 all = tile_scan_body(tile_word, tiles);
  if (threadIdx.x == 0) {
    const u64 kept = all & 0xFFFFFFFFull, roots = all >> 32;
    *rec = RegionTableRecord{kept, roots, 0, kept > (u64)capacity ? kept - (u64)capacity : 0};
    image_offsets[images] = (int32_t)kept;
    roots_before[images] = (uint32_t)roots;
  }
}

__global__ __launch_bounds__(TT) void table_rows_kernel(const uint32_t* __restrict__ region,
                                                        const uint32_t* __restrict__ area, long n, uint32_t per, int H,
                                                        int W, uint32_t min_area, uint32_t capacity,
                                                        const u64* __restrict__ tile_word, RegionRow* __restrict__ rows,
                                                        int32_t* __restrict__ image_offsets,
                                                        uint32_t* __restrict__ rowof,
                                                        uint32_t* __restrict__ roots_before) {
  __shared__ u64 s_cnt[TI][TW];   // roots << 32 | kept of a wave's round; then the exclusive prefix in (round, wave) order
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long tile0 = (long)blockIdx.x * TILE;
  const u64 lt = (1ull << lane) - 1;
  uint32_t root_bits = 0, kept_bits = 0;
  uint32_t roots_in_front[TI], kept_in_front[TI];   // within the wave's round
#pragma unroll
  for (int k = 0; k < TI; ++k) {
    bool root, kept;
    table_flags(region, area, n, tile0 + (long)k * TT + t, min_area, root, kept);
    const u64 br = __ballot(root), bk = __ballot(kept);
    roots_in_front[k] = (uint32_t)__popcll(br & lt), kept_in_front[k] = (uint32_t)__popcll(bk & lt);
    root_bits |= (uint32_t)root << k, kept_bits |= (uint32_t)kept << k;
    if (lane == 0) s_cnt[k][w] = ((u64)__popcll(br) << 32) | (u64)__popcll(bk);
  }
  __syncthreads();
  if (t == 0) {
    u64 run = tile_word[blockIdx.x];
    for (int k = 0; k < TI; ++k)
      for (int v = 0; v < TW; ++v) {
        const u64 c = s_cnt[k][v];
        s_cnt[k][v] = run;
        run += c;
      }
  }
  __syncthreads();
  // the first image start at or behind the tile: the only one in it where an image is no shorter than a tile
  const long start = (tile0 + per - 1) / per * per;
#pragma unroll
  for (int k = 0; k < TI; ++k) {
    const long p = tile0 + (long)k * TT + t;
    if (p >= n) continue;
    const u64 base = s_cnt[k][w];
    const uint32_t root_number = (uint32_t)(base >> 32) + roots_in_front[k];
    const uint32_t row = (uint32_t)(base & 0xFFFFFFFFull) + kept_in_front[k];
    const bool is_start = per >= (uint32_t)TILE ? p == start : (uint32_t)p % per == 0;
    if (is_start) {
      const uint32_t image = (uint32_t)p / per;
      image_offsets[image] = (int32_t)row;
      roots_before[image] = root_number;
    }
    if ((root_bits >> k) & 1u) {
      const bool kept = (kept_bits >> k) & 1u;
      rowof[p] = kept ? row : REGION_NO_ROW;
      if (kept && row < capacity) {
        const uint32_t image = (uint32_t)p / per;
        rows[row] = region_row_start(image, root_number, (uint32_t)p - image * per, area[p], H, W);
      }
    }
  }
}

static constexpr int SLOTS = 16;
static constexpr uint32_t SLOT_FREE = 0xFFFFFFFFu;

AACLIP_DEV void table_fold_row(RegionRow* row, u64 word, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t ov) {
  atomicMax(reinterpret_cast<u64*>(&row->peak_x), word);
  atomicMin(&row->x0, x0);
  atomicMin(&row->y0, y0);
  atomicMax(&row->x1, x1);
  atomicMax(&row->y1, y1);
  if (ov) atomicAdd(&row->overlap, ov);
}

__global__ __launch_bounds__(TT) void table_accumulate_kernel(const uint32_t* __restrict__ region,
                                                              const uint32_t* __restrict__ area,
                                                              const float* __restrict__ scores,
                                                              const RangeRecord* __restrict__ range,
                                                              const uint8_t* __restrict__ other, long n, uint32_t per,
                                                              int W, uint32_t min_area, uint32_t capacity,
                                                              RegionRow* rows, uint32_t* rowof,
                                                              uint8_t* __restrict__ kept_mask, RegionTableRecord* rec) {
  __shared__ u64 s_peak[SLOTS];
  __shared__ uint32_t s_tag[SLOTS], s_x0[SLOTS], s_y0[SLOTS], s_x1[SLOTS], s_y1[SLOTS], s_ov[SLOTS];
  const int t = threadIdx.x, lane = t & 63;
  if (t < SLOTS) {
    s_peak[t] = 0, s_tag[t] = SLOT_FREE;
    s_x0[t] = s_y0[t] = 0xFFFFFFFFu;
    s_x1[t] = s_y1[t] = s_ov[t] = 0;
  }
  __syncthreads();
  const RangeNorm norm = range_norm(range);
  const long tile0 = (long)blockIdx.x * TILE;
  const u64 le = (2ull << lane) - 1, ge = ~0ull << lane;   // the lanes up to and from this one
  uint32_t regions[TI], areas[TI];   // every round's loads are issued before the first round is folded
#pragma unroll
  for (int k = 0; k < TI; ++k) {
    const long p = tile0 + (long)k * TT + t;
    regions[k] = p < n ? region[p] : 0u;
    areas[k] = p < n ? area[p] : 0u;
  }
#pragma unroll
  for (int k = 0; k < TI; ++k) {
    const long p = tile0 + (long)k * TT + t;
    const bool in = p < n;
    const uint32_t r = regions[k], a = areas[k];
    const bool kept = r != 0 && (long)r <= n && a >= min_area;
    if (kept_mask && in) kept_mask[p] = kept ? 1 : 0;
    if (__ballot(kept) == 0) continue;   // the whole wave: nothing to fold in these 64 pixels
    uint32_t rem = 0, x = 0, y = 0, key = 0;
    bool set = false;
    if (kept) {
      rem = (uint32_t)p % per;
      y = rem / (uint32_t)W;
      x = rem - y * (uint32_t)W;
      key = region_score_key(region_score_bits(range_normalised(scores[p], norm)));
      set = other && other[p] != 0;
    }
    // a run: consecutive lanes of one region in one image row; lanes that are not kept carry id 0 and belong to none
    const uint32_t id = kept ? r : 0u;
    const uint32_t before = __shfl_up(id, 1), behind = __shfl_down(id, 1);
    const bool head = kept && (lane == 0 || before != id || x == 0);
    const bool tail = kept && (lane == 63 || behind != id || x + 1 == (uint32_t)W);
    const u64 heads = __ballot(head), tails = __ballot(tail), sets = __ballot(set);
    const int first_lane = kept ? 63 - __clzll((long long)(heads & le)) : lane;
    uint32_t m = key;   // inclusive maximum over the run's lanes up to this one
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(m, d);
      if (kept && lane - d >= first_lane) m = o > m ? o : m;
    }
    const int last_lane = kept ? __ffsll((long long)(tails & ge)) - 1 : lane;
    const uint32_t run_max = __shfl(m, last_lane);
    const u64 at_max = __ballot(kept && key == run_max);
    if (tail) {
      const u64 run = le & (~0ull << first_lane);
      const int peak_lane = __ffsll((long long)(at_max & run)) - 1;   // the lowest index among equal scores
      const u64 word = region_peak_pack(m, rem - (uint32_t)(lane - peak_lane));
      const uint32_t ov = (uint32_t)__popcll(sets & run);
      const uint32_t x0 = x - (uint32_t)(lane - first_lane), x1 = x + 1, y0 = y, y1 = y + 1;
      const uint32_t entry = __hip_atomic_load(rowof + (r - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t row = entry & ~REGION_HIT_BIT;
      if (row >= capacity) {   // no row to fold into: only whether the region overlaps at all is kept, once
        if (ov && !(entry & REGION_HIT_BIT) && !(atomicOr(rowof + (r - 1), REGION_HIT_BIT) & REGION_HIT_BIT))
          atomicAdd(&rec->hit, 1ull);
      } else {
        const int slot = (int)(row & (SLOTS - 1));
        const uint32_t tag = atomicCAS(&s_tag[slot], SLOT_FREE, row);
        if (tag == SLOT_FREE || tag == row) {
          atomicMax(&s_peak[slot], word);
          atomicMin(&s_x0[slot], x0);
          atomicMin(&s_y0[slot], y0);
          atomicMax(&s_x1[slot], x1);
          atomicMax(&s_y1[slot], y1);
          if (ov) atomicAdd(&s_ov[slot], ov);
        } else {
          table_fold_row(rows + row, word, x0, y0, x1, y1, ov);
        }
      }
    }
  }
  __syncthreads();
  if (t < SLOTS && s_tag[t] != SLOT_FREE)
    table_fold_row(rows + s_tag[t], s_peak[t], s_x0[t], s_y0[t], s_x1[t], s_y1[t], s_ov[t]);
}

__global__ __launch_bounds__(TT) void table_finish_kernel(RegionRow* __restrict__ rows, long capacity,
                                                          const uint32_t* __restrict__ roots_before, int W,
                                                          RegionTableRecord* rec) {
  const long i = (long)blockIdx.x * TT + threadIdx.x;
  const u64 kept = rec->kept;
  const long limit = kept < (u64)capacity ? (long)kept : capacity;
  bool hit = false;
  if (i < limit) {
    RegionRow row = rows[i];
    const u64 word = ((u64)row.peak_y << 32) | row.peak_x;   // little-endian: the word's low half is peak_x
    region_row_finish(&row, word, roots_before[row.image], W);
    rows[i] = row;
    hit = row.overlap != 0;
  }
  const u64 hits = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && hits) atomicAdd(&rec->hit, (u64)__popcll(hits));
}

size_t region_table_ws_bytes(long n, long images) { return region_table_layout(n, images).bytes; }

void launch_region_table(const uint32_t* region, const uint32_t* area, const float* scores, const void* range_record,
                         const uint8_t* other, long images, int H, int W, long min_area, long capacity, void* rows,
                         int32_t* image_offsets, uint8_t* kept_mask, void* record, void* ws, hipStream_t s) {
  const long per = (long)H * W, n = images * per;
  const RegionTableLayout l = region_table_layout(n, images);
  uint32_t* rowof = (uint32_t*)((char*)ws + l.rowof);
  u64* tile_word = (u64*)((char*)ws + l.tile_word);
  uint32_t* roots_before = (uint32_t*)((char*)ws + l.roots_before);
  RegionTableRecord* rec = (RegionTableRecord*)record;
  const uint32_t ma = min_area > 0x7FFFFFFFL ? 0x80000000u : (uint32_t)min_area;   // areas stay below 2^31
  const long cap = capacity < n ? capacity : n;                                      // no more rows than pixels
  const dim3 grid((unsigned)l.tiles);
  hipLaunchKernelGGL(table_tile_sum_kernel, grid, dim3(TT), 0, s, region, area, n, ma, tile_word);
  hipLaunchKernelGGL(table_tile_scan_kernel, dim3(1), dim3(TT), 0, s, tile_word, l.tiles, cap, images, image_offsets,
                     roots_before, rec);
  hipLaunchKernelGGL(table_rows_kernel, grid, dim3(TT), 0, s, region, area, n, (uint32_t)per, H, W, ma, (uint32_t)cap,
                     tile_word, (RegionRow*)rows, image_offsets, rowof, roots_before);
  hipLaunchKernelGGL(table_accumulate_kernel, grid, dim3(TT), 0, s, region, area, scores,
                     (const RangeRecord*)range_record, other, n, (uint32_t)per, W, ma, (uint32_t)cap, (RegionRow*)rows,
                     rowof, kept_mask, rec);
  if (cap > 0)
    hipLaunchKernelGGL(table_finish_kernel, dim3((unsigned)((cap + TT - 1) / TT)), dim3(TT), 0, s, (RegionRow*)rows, cap,
                       roots_before, W, rec);
}

}  // namespace aaclip

// Per-region overlap (AUPRO) of one class on the device (forward_utils.pro_eval_device), beside the AUROC / AP of metrics.hip:
//   regions    connected components of the non-zero mask pixels of every image: a label-equivalence union-find on a
//              32-bit parent array (regions_uf.h), then canonical ids (1 + the smallest flat index) and areas
//   pairs      metrics.hip's stable radix sort with a 32-bit value (the area) beside the key
//   pro curve  tie groups of the sorted keys from the top -> (fp, S = sum of 1 / area) at every group, trapezoids of
//              (fp / N_ok, min(1, S / R)) up to the false-positive limit, one interpolated at the limit
// No floating-point atomics.  The labelling takes minima of indices and integer sums, so it does not depend on the order
// of execution; every floating-point sum runs in an order fixed by n and the number of groups.
#include "common.h"
#include "kernels.h"
#include "regions_uf.h"
#include <math.h>

namespace aaclip {

static constexpr int RT = 256;
typedef unsigned long long u64;
static inline size_t up256_bytes(size_t v) { return (v + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------- regions
struct DeviceAccess {
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ uint32_t min(uint32_t* p, uint32_t v) { return atomicMin(p, v); }
};

struct RegionsRecord {   // include/aaclip.h aaclip_metrics_regions_record
  u64 regions, anomalous, normal;
};

__global__ __launch_bounds__(RT) void regions_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ count,
                                                          long n, RegionsRecord* __restrict__ rec) {
  const long i = (long)blockIdx.x * RT + threadIdx.x;
  if (i == 0) *rec = RegionsRecord{0, 0, 0};
  if (i >= n) return;
  parent[i] = (uint32_t)i;
  count[i] = 0;
}

__global__ __launch_bounds__(RT) void regions_merge_kernel(const uint8_t* __restrict__ mask, uint32_t* parent, long n,
                                                           int H, int W, int connectivity) {
  const long i = (long)blockIdx.x * RT + threadIdx.x;
  if (i >= n || !mask[i]) return;
  uf_merge_pixel<DeviceAccess>(mask, parent, i, H, W, connectivity);
}

// region = 1 + root, one integer atomic per anomalous pixel on the root's counter; the three counts of the record by a
// workgroup tree and one integer atomic each
__global__ __launch_bounds__(RT) void regions_flatten_kernel(const uint8_t* __restrict__ mask,
                                                             uint32_t* parent, long n,
                                                             uint32_t* __restrict__ region, uint32_t* __restrict__ count,
                                                             RegionsRecord* __restrict__ rec) {
  __shared__ uint32_t s_roots[RT], s_anom[RT];
  const int t = threadIdx.x;
  const long i = (long)blockIdx.x * RT + t;
  uint32_t is_root = 0, anom = 0;
  if (i < n) {
    uint32_t r = 0;
    if (mask[i]) {
      const uint32_t root = uf_find_halve<DeviceAccess>(parent, (uint32_t)i);
      atomicAdd(&count[root], 1u);
      r = root + 1;
      anom = 1;
      is_root = root == (uint32_t)i;
    }
    region[i] = r;
  }
  s_roots[t] = is_root, s_anom[t] = anom;
  __syncthreads();
  for (int o = RT / 2; o > 0; o >>= 1) {
    if (t < o) s_roots[t] += s_roots[t + o], s_anom[t] += s_anom[t + o];
    __syncthreads();
  }
  if (t == 0) {
    const long here = n - (long)blockIdx.x * RT < RT ? n - (long)blockIdx.x * RT : RT;
    if (s_roots[0]) atomicAdd(&rec->regions, (u64)s_roots[0]);
    if (s_anom[0]) atomicAdd(&rec->anomalous, (u64)s_anom[0]);
    if (here > s_anom[0]) atomicAdd(&rec->normal, (u64)(here - s_anom[0]));
  }
}

__global__ __launch_bounds__(RT) void regions_area_kernel(const uint32_t* __restrict__ region,
                                                          const uint32_t* __restrict__ count, long n,
                                                          uint32_t* __restrict__ area) {
  const long i = (long)blockIdx.x * RT + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = region[i];
  area[i] = r != 0 && (long)r <= n ? count[r - 1] : 0u;
}

size_t metrics_regions_ws_bytes(long n) { return 2 * up256_bytes((size_t)n * 4); }

// ws: [parent: n uint32] [count: n uint32]
void launch_metrics_regions(const uint8_t* mask, long n, int H, int W, int connectivity, uint32_t* region,
                            uint32_t* area, void* record, void* ws, hipStream_t s) {
  uint32_t* parent = (uint32_t*)ws;
  uint32_t* count = (uint32_t*)((char*)ws + up256_bytes((size_t)n * 4));
  const dim3 grid((unsigned)((n + RT - 1) / RT));
  RegionsRecord* rec = (RegionsRecord*)record;
  hipLaunchKernelGGL(regions_init_kernel, grid, dim3(RT), 0, s, parent, count, n, rec);
  hipLaunchKernelGGL(regions_merge_kernel, grid, dim3(RT), 0, s, mask, parent, n, H, W, connectivity);
  hipLaunchKernelGGL(regions_flatten_kernel, grid, dim3(RT), 0, s, mask, parent, n, region, count, rec);
  hipLaunchKernelGGL(regions_area_kernel, grid, dim3(RT), 0, s, region, count, n, area);
}

// ------------------------------------------------------------------------------------------------ pro curve
// The keys ascend, the curve is walked from the top: position j = n - 1 - i.  Element i ENDS a tie group there when
// i == 0 or its key differs from that of i - 1.  A prefix over j of (end << 32 | normal) and of the fp64 weight
// w = 1 / area (0 for a normal pixel, area == 0) gives, at every group end, the group's number g from the top and the
// inclusive sums fp_g and S_g: marks_fp[g], marks_s[g].  Three levels like metrics.hip's curve: sums of tiles of 4096,
// one workgroup over the tile sums, the tiles again.  The fp64 prefix is the thread's own items in order, a
// Hillis-Steele scan over the workgroup's threads and the tile prefix: an order fixed by n alone.
// Group g then gives the point x = fp / N_ok, y = min(1, S / R); with (x0, y0) the point of g - 1 ((0, 0) for the top
// group) its share of the area is the trapezoid 0.5 (x - x0)(y + y0) where x <= limit, the trapezoid up to the
// interpolated point at the limit where x0 < limit < x, and nothing beyond.
static constexpr int PRO_ITEMS = 16;
static constexpr int PRO_TILE = RT * PRO_ITEMS;
static constexpr int PRO_MAX_BLOCKS = 1024;

struct ProRecord {   // include/aaclip.h aaclip_metrics_pro_record
  double aupro;
  u64 regions, normal, groups;
  double y_limit;
};

long metrics_pro_tiles(long n) { return (n + PRO_TILE - 1) / PRO_TILE; }
long metrics_pro_blocks(long n) {
  const long b = (n + RT - 1) / RT;
  return b < PRO_MAX_BLOCKS ? b : PRO_MAX_BLOCKS;
}

struct ProItem {
  u64 word;   // end << 32 | normal
  double w;
};

AACLIP_DEV ProItem pro_item(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ areas, long n, long j) {
  const long i = n - 1 - j;
  const uint32_t a = areas[i];
  const bool end = i == 0 || keys[i - 1] != keys[i];
  return ProItem{((u64)end << 32) | (a == 0 ? 1u : 0u), a == 0 ? 0.0 : 1.0 / (double)a};
}

AACLIP_DEV ProItem pro_thread_sum(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ areas, long n,
                                  long first) {
  ProItem acc{0, 0.0};
#pragma unroll 4
  for (int k = 0; k < PRO_ITEMS; ++k)
    if (first + k < n) {
      const ProItem it = pro_item(keys, areas, n, first + k);
      acc.word += it.word;
      acc.w += it.w;
    }
  return acc;
}

// exclusive prefix over the workgroup's threads, in thread order; *all <- the sum over the workgroup
AACLIP_DEV ProItem pro_block_scan(ProItem mine, u64* lds_word, double* lds_w, ProItem* all) {
  const int t = threadIdx.x;
  lds_word[t] = mine.word, lds_w[t] = mine.w;
  __syncthreads();
  for (int o = 1; o < RT; o <<= 1) {
    const u64 add_word = t >= o ? lds_word[t - o] : 0;
    const double add_w = t >= o ? lds_w[t - o] : 0.0;
    __syncthreads();
    // left operand = the earlier threads: the Hillis-Steele tree, the same for every call with one n
    if (t >= o) lds_word[t] = add_word + lds_word[t], lds_w[t] = add_w + lds_w[t];
    __syncthreads();
  }
  if (all) *all = ProItem{lds_word[RT - 1], lds_w[RT - 1]};
  ProItem ex{0, 0.0};
  if (t > 0) ex = ProItem{lds_word[t - 1], lds_w[t - 1]};
  __syncthreads();
  return ex;
}

__global__ __launch_bounds__(RT) void pro_tile_sum_kernel(const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ areas, long n,
                                                          u64* __restrict__ tile_word, double* __restrict__ tile_w) {
  __shared__ u64 lds_word[RT];
  __shared__ double lds_w[RT];
  const ProItem mine = pro_thread_sum(keys, areas, n, (long)blockIdx.x * PRO_TILE + (long)threadIdx.x * PRO_ITEMS);
  ProItem all;
  pro_block_scan(mine, lds_word, lds_w, &all);
  if (threadIdx.x == 0) tile_word[blockIdx.x] = all.word, tile_w[blockIdx.x] = all.w;
}

// one workgroup: the tile sums <- their exclusive prefix; total[0] <- groups << 32 | normal pixels
__global__ __launch_bounds__(RT) void pro_tile_scan_kernel(u64* __restrict__ tile_word, double* __restrict__ tile_w,
                                                           long tiles, u64* __restrict__ total) {
  __shared__ u64 lds_word[RT];
  __shared__ double lds_w[RT];
  const int t = threadIdx.x;
  const long per = (tiles + RT - 1) / RT;
  const long j0 = t * per < tiles ? t * per : tiles, j1 = j0 + per < tiles ? j0 + per : tiles;
  ProItem acc{0, 0.0};
  for (long j = j0; j < j1; ++j) acc.word += tile_word[j], acc.w += tile_w[j];
  ProItem all;
  ProItem run = pro_block_scan(acc, lds_word, lds_w, &all);
  if (t == 0) total[0] = all.word;
  for (long j = j0; j < j1; ++j) {
    const u64 cw = tile_word[j];
    const double cd = tile_w[j];
    tile_word[j] = run.word, tile_w[j] = run.w;
    run.word += cw, run.w += cd;
  }
}

__global__ __launch_bounds__(RT) void pro_mark_kernel(const uint32_t* __restrict__ keys,
                                                      const uint32_t* __restrict__ areas, long n,
                                                      const u64* __restrict__ tile_word,
                                                      const double* __restrict__ tile_w, uint32_t* __restrict__ marks_fp,
                                                      double* __restrict__ marks_s) {
  __shared__ u64 lds_word[RT];
  __shared__ double lds_w[RT];
  const long first = (long)blockIdx.x * PRO_TILE + (long)threadIdx.x * PRO_ITEMS;
  const ProItem mine = pro_thread_sum(keys, areas, n, first);
  const ProItem ex = pro_block_scan(mine, lds_word, lds_w, nullptr);
  u64 word = tile_word[blockIdx.x] + ex.word;
  double w = tile_w[blockIdx.x] + ex.w;
#pragma unroll 4
  for (int k = 0; k < PRO_ITEMS; ++k) {
    const long j = first + k;
    if (j >= n) break;
    const ProItem it = pro_item(keys, areas, n, j);
    const u64 g = word >> 32;
    word += it.word;
    w += it.w;
    if ((it.word >> 32) && g < (u64)n) {   // g < groups <= n
      marks_fp[g] = (uint32_t)(word & 0xFFFFFFFFull);
      marks_s[g] = w;
    }
  }
}

// Workgroup b takes a contiguous share of the groups, a thread every 256th of them, the threads are folded by a tree.
// At most one group meets the limit from below and at most one ends exactly on it as the last that does: the y there.
__global__ __launch_bounds__(RT) void pro_group_kernel(const uint32_t* __restrict__ marks_fp,
                                                       const double* __restrict__ marks_s,
                                                       const u64* __restrict__ total,
                                                       const RegionsRecord* __restrict__ regions, double limit,
                                                       double* __restrict__ part, double* __restrict__ y_limit) {
  __shared__ double s_area[RT];
  const int t = threadIdx.x;
  const long G = (long)(total[0] >> 32);
  const double n_ok = (double)(total[0] & 0xFFFFFFFFull), R = (double)regions->regions;
  const long per = (G + gridDim.x - 1) / gridDim.x;
  const long g0 = (long)blockIdx.x * per, g1 = g0 + per < G ? g0 + per : G;
  double area = 0.0;
  for (long g = g0 + t; g < g1; g += RT) {
    const double x = (double)marks_fp[g] / n_ok, y = fmin(1.0, marks_s[g] / R);
    double x0 = 0.0, y0 = 0.0;
    if (g > 0) x0 = (double)marks_fp[g - 1] / n_ok, y0 = fmin(1.0, marks_s[g - 1] / R);
    if (x <= limit) {
      area += 0.5 * (x - x0) * (y + y0);
      const bool last = g + 1 == G || (double)marks_fp[g + 1] / n_ok > limit;
      if (last && x == limit) *y_limit = y;
    } else if (x0 < limit) {
      const double yl = y0 + (y - y0) * ((limit - x0) / (x - x0));
      area += 0.5 * (limit - x0) * (yl + y0);
      *y_limit = yl;
    }
  }
  s_area[t] = area;
  __syncthreads();
  for (int o = RT / 2; o > 0; o >>= 1) {
    if (t < o) s_area[t] += s_area[t + o];
    __syncthreads();
  }
  if (t == 0) part[blockIdx.x] = s_area[0];
}

// the partials in index order, by one thread
__global__ void pro_final_kernel(const double* __restrict__ part, int parts, const u64* __restrict__ total,
                                 const RegionsRecord* __restrict__ regions, double limit,
                                 const double* __restrict__ y_limit, ProRecord* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double area = 0.0;
  for (int j = 0; j < parts; ++j) area += part[j];
  rec->aupro = area / limit;
  rec->regions = regions->regions;
  rec->normal = total[0] & 0xFFFFFFFFull;
  rec->groups = total[0] >> 32;
  rec->y_limit = *y_limit;
}

size_t metrics_pro_curve_ws_bytes(long n) {
  return 2 * up256_bytes((size_t)metrics_pro_tiles(n) * 8) + 256 + up256_bytes((size_t)n * 4) +
         up256_bytes((size_t)n * 8) + up256_bytes((size_t)metrics_pro_blocks(n) * 8);
}

// ws: [tile words] [tile weights] [total: 8, y at the limit: 8] [marks fp: n x 4] [marks S: n x 8] [partial areas]
void launch_metrics_pro_curve(const uint32_t* keys, const uint32_t* areas_sorted, long n, const void* regions_record,
                              double fpr_limit, void* record, void* ws, hipStream_t s) {
  const long tiles = metrics_pro_tiles(n);
  const int parts = (int)metrics_pro_blocks(n);
  char* p = (char*)ws;
  u64* tile_word = (u64*)p;
  p += up256_bytes((size_t)tiles * 8);
  double* tile_w = (double*)p;
  p += up256_bytes((size_t)tiles * 8);
  u64* total = (u64*)p;
  double* y_limit = (double*)(p + 8);
  p += 256;
  uint32_t* marks_fp = (uint32_t*)p;
  p += up256_bytes((size_t)n * 4);
  double* marks_s = (double*)p;
  p += up256_bytes((size_t)n * 8);
  double* part = (double*)p;
  const RegionsRecord* regions = (const RegionsRecord*)regions_record;
  (void)hipMemsetAsync(total, 0, 16, s);
  hipLaunchKernelGGL(pro_tile_sum_kernel, dim3((unsigned)tiles), dim3(RT), 0, s, keys, areas_sorted, n, tile_word,
                     tile_w);
  hipLaunchKernelGGL(pro_tile_scan_kernel, dim3(1), dim3(RT), 0, s, tile_word, tile_w, tiles, total);
  hipLaunchKernelGGL(pro_mark_kernel, dim3((unsigned)tiles), dim3(RT), 0, s, keys, areas_sorted, n, tile_word, tile_w,
                     marks_fp, marks_s);
  hipLaunchKernelGGL(pro_group_kernel, dim3(parts), dim3(RT), 0, s, marks_fp, marks_s, total, regions, fpr_limit, part,
                     y_limit);
  hipLaunchKernelGGL(pro_final_kernel, dim3(1), dim3(64), 0, s, part, parts, total, regions, fpr_limit, y_limit,
                     (ProRecord*)record);
}

}  // namespace aaclip

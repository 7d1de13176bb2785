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
#include "metrics_records.h"
#include "regions_uf.h"
#include "tile_scan.h"
#include <math.h>

namespace aaclip {

static constexpr int RT = TILE_THREADS;

// ---------------------------------------------------------------------------------------------------- regions
struct DeviceAccess {
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ uint32_t min(uint32_t* p, uint32_t v) { return atomicMin(p, v); }
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
  __shared__ uint32_t s_cnt[RT];   // roots << 16 | anomalous pixels: both at most RT
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
  const uint32_t all = block_fold((is_root << 16) | anom, s_cnt, [](uint32_t a, uint32_t b) { return a + b; });
  if (t == 0) {
    const uint32_t roots = all >> 16, anomalous = all & 0xFFFFu;
    const long here = n - (long)blockIdx.x * RT < RT ? n - (long)blockIdx.x * RT : RT;
    if (roots) atomicAdd(&rec->regions, (u64)roots);
    if (anomalous) atomicAdd(&rec->anomalous, (u64)anomalous);
    if (here > anomalous) atomicAdd(&rec->normal, (u64)(here - anomalous));
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
// inclusive sums fp_g and S_g: marks_fp[g], marks_s[g].  The prefix is tile_scan.h's, on the item {word, w}: its order
// of the fp64 sums is fixed by n alone.
// Group g then gives the point x = fp / N_ok, y = min(1, S / R); with (x0, y0) the point of g - 1 ((0, 0) for the top
// group) its share of the area is the trapezoid 0.5 (x - x0)(y + y0) where x <= limit, the trapezoid up to the
// interpolated point at the limit where x0 < limit < x, and nothing beyond.
static constexpr int PRO_ITEMS = METRICS_SCAN_ITEMS;

struct ProItem {
  u64 word;   // end << 32 | normal
  double w;
};
AACLIP_DEV ProItem operator+(const ProItem& a, const ProItem& b) { return ProItem{a.word + b.word, a.w + b.w}; }

AACLIP_DEV ProItem pro_item(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ areas, long n, long j) {
  const long i = n - 1 - j;
  const uint32_t a = areas[i];
  const bool end = i == 0 || keys[i - 1] != keys[i];
  return ProItem{((u64)end << 32) | (a == 0 ? 1u : 0u), a == 0 ? 0.0 : 1.0 / (double)a};
}

__global__ __launch_bounds__(RT) void pro_tile_sum_kernel(const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ areas, long n,
                                                          ProItem* __restrict__ tile_sum) {
  tile_sum_body<PRO_ITEMS, ProItem>(n, tile_sum, [=](long j) { return pro_item(keys, areas, n, j); });
}

// one workgroup: the tile sums <- their exclusive prefix; total[0] <- groups << 32 | normal pixels
__global__ __launch_bounds__(RT) void pro_tile_scan_kernel(ProItem* __restrict__ tile_sum, long tiles,
                                                           u64* __restrict__ total) {
  const ProItem all = tile_scan_body(tile_sum, tiles);
  if (threadIdx.x == 0) total[0] = all.word;
}

__global__ __launch_bounds__(RT) void pro_mark_kernel(const uint32_t* __restrict__ keys,
                                                      const uint32_t* __restrict__ areas, long n,
                                                      const ProItem* __restrict__ tile_prefix,
                                                      uint32_t* __restrict__ marks_fp, double* __restrict__ marks_s) {
  tile_walk_body<PRO_ITEMS, ProItem>(
      n, tile_prefix, [=](long j) { return pro_item(keys, areas, n, j); },
      [=](long, const ProItem& it, const ProItem& run) {
        const u64 g = run.word >> 32;
        if ((it.word >> 32) && g < (u64)n) {   // g < groups <= n
          const ProItem here = run + it;       // the inclusive sums at the group's end
          marks_fp[g] = (uint32_t)(here.word & 0xFFFFFFFFull);
          marks_s[g] = here.w;
        }
      });
}

// Workgroup b takes a contiguous share of the groups, a thread every 256th of them, the threads are folded by block_fold.
// At most one group meets the limit from below and at most one ends exactly on it as the last that does: the y there.
__global__ __launch_bounds__(RT) void pro_group_kernel(const uint32_t* __restrict__ marks_fp,
                                                       const double* __restrict__ marks_s,
                                                       const u64* __restrict__ total,
                                                       const RegionsRecord* __restrict__ regions, double limit,
                                                       double* __restrict__ part, double* __restrict__ y_limit) {
  __shared__ double s_area[RT];
  const long G = (long)(total[0] >> 32);
  const double n_ok = (double)(total[0] & 0xFFFFFFFFull), R = (double)regions->regions;
  const GroupShare share = group_share(G);
  double area = 0.0;
  for (long g = share.k0 + threadIdx.x; g < share.k1; g += RT) {
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
  area = block_fold(area, s_area, [](double a, double b) { return a + b; });
  if (threadIdx.x == 0) part[blockIdx.x] = area;
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

size_t metrics_pro_curve_ws_bytes(long n) { return pro_curve_layout(n).bytes; }

void launch_metrics_pro_curve(const uint32_t* keys, const uint32_t* areas_sorted, long n, const void* regions_record,
                              double fpr_limit, void* record, void* ws, hipStream_t s) {
  const ProLayout l = pro_curve_layout(n);
  char* p = (char*)ws;
  ProItem* tile_sum = (ProItem*)(p + l.tile_sum);
  u64* total = (u64*)(p + l.total);
  double* y_limit = (double*)(p + l.total + 8);
  uint32_t* marks_fp = (uint32_t*)(p + l.marks_fp);
  double *marks_s = (double*)(p + l.marks_s), *part = (double*)(p + l.part);
  const RegionsRecord* regions = (const RegionsRecord*)regions_record;
  (void)hipMemsetAsync(total, 0, 16, s);
  hipLaunchKernelGGL(pro_tile_sum_kernel, dim3((unsigned)l.tiles), dim3(RT), 0, s, keys, areas_sorted, n, tile_sum);
  hipLaunchKernelGGL(pro_tile_scan_kernel, dim3(1), dim3(RT), 0, s, tile_sum, l.tiles, total);
  hipLaunchKernelGGL(pro_mark_kernel, dim3((unsigned)l.tiles), dim3(RT), 0, s, keys, areas_sorted, n, tile_sum, marks_fp,
                     marks_s);
  hipLaunchKernelGGL(pro_group_kernel, dim3(l.parts), dim3(RT), 0, s, marks_fp, marks_s, total, regions, fpr_limit, part,
                     y_limit);
  hipLaunchKernelGGL(pro_final_kernel, dim3(1), dim3(64), 0, s, part, l.parts, total, regions, fpr_limit, y_limit,
                     (ProRecord*)record);
}

}  // namespace aaclip

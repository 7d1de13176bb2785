// Bootstrap of AUROC / AP over the images of one class (forward_utils.bootstrap_eval is the definition; the records, the
// term of a tie group and the workspace are bootstrap_plan.h).  The class is sorted ONCE (aaclip_metrics_sort_pairs with
// the payload image << 1 | label); every replicate is that order with an integer weight per image, so the bootstrap is
// a weighted curve pass:
//   pass 1   a wave owns one tile of 4096 sorted elements and one block of 64 replicates, lane = replicate.  It loads 64
//            elements at a time and walks them in order; element j's payload is made wave-uniform with v_readlane, each
//            lane reads its own weight from the block's LDS table [images][64] bytes (64 consecutive bytes per element)
//            and keeps its running (E, M) in registers  -> the weighted sums of every (tile, replicate)
//   scan     per replicate, the exclusive prefix of those sums over the tiles, and (P, Mtot)
//   pass 2   the same walk from the true prefix: at every start of a tie group the group that ENDS there is closed from
//            the state at the start before it  -> per (tile, replicate) the state at the first and the last start and
//            the sums of the groups closed inside
//   fold     per replicate, the tiles in index order: the groups across tile boundaries (a tile without a start is
//            skipped), the top group, the record
// Integers except the fp64 AP sum, whose order is fixed by n alone; no atomics, no workgroup waits for another: two
// calls give the same bytes.
#include "common.h"
#include "kernels.h"
#include "bootstrap_plan.h"

namespace aaclip {

static constexpr int BOOT_THREADS = 64 * BOOT_WAVES;

// counts [R][images] bytes -> table[image * 64 + lane] of replicates r0 .. r0 + 63; a replicate past R weighs nothing
AACLIP_DEV void boot_load_table(uint8_t* table, const uint8_t* __restrict__ counts, long images, long R, long r0) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int l = w; l < BOOT_BLOCK; l += BOOT_WAVES) {
    const long r = r0 + l;
    for (long i = lane; i < images; i += 64) table[i * BOOT_BLOCK + l] = r < R ? counts[r * images + i] : (uint8_t)0;
  }
}

// grid (ceil(tiles / 4), blocks of the chunk); dynamic LDS images * 64 bytes
template <int PASS>
__global__ __launch_bounds__(BOOT_THREADS) void bootstrap_walk_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ payload, long n, long tiles,
    const uint8_t* __restrict__ counts, long images, long R, long r_first, uint2* __restrict__ sums,
    const uint2* __restrict__ totals, uint32_t* __restrict__ tile_starts, BootTileRecord* __restrict__ records) {
  extern __shared__ uint8_t table[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long blk = blockIdx.y;
  boot_load_table(table, counts, images, R, r_first + blk * BOOT_BLOCK);
  __syncthreads();
  const long tile = (long)blockIdx.x * BOOT_WAVES + w;
  if (tile >= tiles) return;
  const size_t slot = ((size_t)blk * tiles + tile) * BOOT_BLOCK + lane;
  const uint32_t last_image = (uint32_t)images - 1;
  uint32_t E = 0, M = 0, P = 0, Mtot = 0;
  if (PASS == 2) {
    const uint2 pre = sums[slot], tot = totals[blk * BOOT_BLOCK + lane];
    E = pre.x, M = pre.y, P = tot.x, Mtot = tot.y;
  }
  bool have = false;                       // wave-uniform: a start was met in this tile
  uint32_t Ef = 0, Mf = 0, Ep = 0, Mp = 0;   // the state at the first start, at the latest start
  uint64_t num = 0;
  double ap = 0.0;
  uint32_t starts_seen = 0;
  const long base = tile * BOOT_TILE;
  for (int r = 0; r < BOOT_TILE / 64; ++r) {
    const long i0 = base + (long)r * 64;
    if (i0 >= n) break;                    // the same for every lane
    const long i = i0 + lane;
    const bool valid = i < n;
    const uint32_t key = valid ? keys[i] : 0u;
    const uint32_t pay = valid ? payload[i] : 0u;
    const bool start = valid && (i == 0 || keys[i - 1] != key);
    const uint64_t starts = __ballot(start);
    const int cnt = n - i0 < 64 ? (int)(n - i0) : 64;
    starts_seen += (uint32_t)__popcll(starts);
    for (int j = 0; j < cnt; ++j) {
      const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pay, j);   // wave-uniform
      uint32_t image = p >> 1;
      image = image < last_image ? image : last_image;   // a payload outside the table reads its last row, never past it
      const uint32_t wgt = table[image * BOOT_BLOCK + lane];
      if (PASS == 2 && ((starts >> j) & 1ull)) {
        if (have) boot_close_group(P, Mtot, Ep, Mp, E, M, num, ap);
        else Ef = E, Mf = M;
        have = true, Ep = E, Mp = M;
      }
      M += wgt;
      E += (p & 1u) ? wgt : 0u;
    }
  }
  if (PASS == 1) {
    sums[slot] = make_uint2(E, M);
    if (lane == 0 && blk == 0) tile_starts[tile] = starts_seen;
  } else {
    records[slot] = BootTileRecord{Ef, Mf, Ep, Mp, num, ap};
  }
}

// grid = blocks of the chunk, 64 threads: thread = replicate; sums <- their exclusive prefix over the tiles.
// Eight tiles are read ahead of the dependent adds.
__global__ __launch_bounds__(BOOT_BLOCK) void bootstrap_scan_kernel(uint2* __restrict__ sums, long tiles,
                                                                    uint2* __restrict__ totals) {
  const size_t blk = blockIdx.x;
  uint2* col = sums + blk * tiles * BOOT_BLOCK + threadIdx.x;
  uint32_t E = 0, M = 0;
  for (long t0 = 0; t0 < tiles; t0 += 8) {
    uint2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = t0 + k < tiles ? col[(t0 + k) * BOOT_BLOCK] : make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (t0 + k < tiles) col[(t0 + k) * BOOT_BLOCK] = make_uint2(E, M);
      E += v[k].x, M += v[k].y;
    }
  }
  totals[blk * BOOT_BLOCK + threadIdx.x] = make_uint2(E, M);
}

// grid = blocks of the chunk, 64 threads: thread = replicate; the tiles in index order
__global__ __launch_bounds__(BOOT_BLOCK) void bootstrap_fold_kernel(const BootTileRecord* __restrict__ records,
                                                                    const uint32_t* __restrict__ tile_starts, long tiles,
                                                                    const uint2* __restrict__ totals, long R, long r_first,
                                                                    BootRecord* __restrict__ out) {
  const size_t blk = blockIdx.x;
  const long r = r_first + (long)blk * BOOT_BLOCK + threadIdx.x;
  const BootTileRecord* col = records + blk * tiles * BOOT_BLOCK + threadIdx.x;
  const uint2 tot = totals[blk * BOOT_BLOCK + threadIdx.x];
  BootFold f = boot_fold_begin();
  for (long t0 = 0; t0 < tiles; t0 += 4) {
    BootTileRecord v[4];
    uint32_t s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s[k] = t0 + k < tiles ? tile_starts[t0 + k] : 0u;
      if (s[k]) v[k] = col[(t0 + k) * BOOT_BLOCK];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (s[k]) boot_fold_tile(f, v[k], tot.x, tot.y);
  }
  if (r < R) out[r] = boot_fold_end(f, tot.x, tot.y);
}

size_t bootstrap_ws_bytes(long n, long R) { return boot_layout(n, R).bytes; }
long bootstrap_max_images() { return BOOT_MAX_IMAGES; }

void launch_bootstrap_curves(const uint32_t* keys, const uint32_t* payload, long n, const uint8_t* counts, long images,
                             long R, void* records, void* ws, hipStream_t s) {
  const BootLayout l = boot_layout(n, R);
  const long tiles = boot_tiles(n), all_blocks = (R + BOOT_BLOCK - 1) / BOOT_BLOCK;
  char* p = (char*)ws;
  uint2* sums = (uint2*)(p + l.sums);
  uint2* totals = (uint2*)(p + l.totals);
  uint32_t* tile_starts = (uint32_t*)(p + l.starts);
  BootTileRecord* tile_records = (BootTileRecord*)(p + l.records);
  const size_t lds = (size_t)images * BOOT_BLOCK;
  const unsigned groups = (unsigned)((tiles + BOOT_WAVES - 1) / BOOT_WAVES);
  for (long b0 = 0; b0 < all_blocks; b0 += BOOT_CHUNK_BLOCKS) {
    const unsigned blocks = (unsigned)(all_blocks - b0 < BOOT_CHUNK_BLOCKS ? all_blocks - b0 : BOOT_CHUNK_BLOCKS);
    const long r_first = b0 * BOOT_BLOCK;
    hipLaunchKernelGGL(bootstrap_walk_kernel<1>, dim3(groups, blocks), dim3(BOOT_THREADS), lds, s, keys, payload, n, tiles,
                       counts, images, R, r_first, sums, (const uint2*)totals, tile_starts, tile_records);
    hipLaunchKernelGGL(bootstrap_scan_kernel, dim3(blocks), dim3(BOOT_BLOCK), 0, s, sums, tiles, totals);
    hipLaunchKernelGGL(bootstrap_walk_kernel<2>, dim3(groups, blocks), dim3(BOOT_THREADS), lds, s, keys, payload, n, tiles,
                       counts, images, R, r_first, sums, (const uint2*)totals, tile_starts, tile_records);
    hipLaunchKernelGGL(bootstrap_fold_kernel, dim3(blocks), dim3(BOOT_BLOCK), 0, s, (const BootTileRecord*)tile_records,
                       (const uint32_t*)tile_starts, tiles, (const uint2*)totals, R, r_first, (BootRecord*)records);
  }
}

}  // namespace aaclip

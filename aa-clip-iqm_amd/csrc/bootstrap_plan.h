// What the host and the device share of the bootstrap of AUROC / AP over images (bootstrap.hip, DESIGN.md section 6,
// "Bootstrap intervals on the device"): the records, the term of one tie group, the fold of the tile records and the
// workspace layout.  bootstrap_host_check.cpp drives the same functions against a brute-force loop.
//
// The sorted elements carry a payload image << 1 | label; replicate r gives element e the weight c[r, image(e)].  The
// STATE at index i is (E, M) = the weighted positives and the weighted elements before i; at n it is (P, Mtot).  A tie
// group [i, i2) is closed from the state at i and the state at i2.  All counts are below 2^31 (the caller checks the
// weighted total), so the unsigned 32-bit differences are exact and num stays below 2^61.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BOOT_HD __host__ __device__ inline
#else
#define BOOT_HD inline
#endif

namespace aaclip {

static constexpr int BOOT_TILE = 4096;          // consecutive sorted elements of one wave's walk (the curve tile)
static constexpr int BOOT_BLOCK = 64;           // replicates of one block: lane = replicate
static constexpr int BOOT_WAVES = 4;            // waves = tiles of a workgroup; they share the block's weight table
static constexpr int BOOT_MAX_IMAGES = 1024;    // [images][64] bytes of LDS: 64 KiB
static constexpr int BOOT_CHUNK_BLOCKS = 8;     // replicate blocks per walk of the entry: what the workspace is sized for

struct BootRecord {   // include/aaclip.h aaclip_bootstrap_record, 32 bytes
  uint64_t num, P, N;
  double ap;
};

struct BootTileRecord {   // one (tile, replicate), 32 bytes; meaningless for a tile without a start
  uint32_t Ef, Mf;        // state at the tile's first start
  uint32_t El, Ml;        // state at its last start
  uint64_t num;           // the groups closed inside the tile
  double ap;
};

// The term of the group between the state (E, M) at its start and (E2, M2) at the next start (or at n).
// A group that holds no weighted positive adds exactly 0 to ap: that is also the 0 / 0 of a top group of weight 0.
BOOT_HD void boot_close_group(uint32_t P, uint32_t Mtot, uint32_t E, uint32_t M, uint32_t E2, uint32_t M2, uint64_t& num,
                              double& ap) {
  const uint32_t tp = P - E, fp = (Mtot - M) - tp, tp0 = P - E2, fp0 = (Mtot - M2) - tp0;
  num += (uint64_t)(fp - fp0) * (uint64_t)(tp + tp0);
  const uint32_t d = tp - tp0;
  if (d != 0) ap += ((double)d / (double)P) * ((double)tp / (double)(tp + fp));
}

// One replicate's walk over the tiles in index order.
struct BootFold {
  bool have;          // a start was met: (E, M) is the state at the last one
  uint32_t E, M;
  uint64_t num;
  double ap;
};

BOOT_HD BootFold boot_fold_begin() { return BootFold{false, 0u, 0u, 0ull, 0.0}; }

// r: the record of the next tile that HAS a start.  The group that ends at its first start began at the last start of
// the nearest earlier tile that has one.
BOOT_HD void boot_fold_tile(BootFold& f, const BootTileRecord& r, uint32_t P, uint32_t Mtot) {
  if (f.have) boot_close_group(P, Mtot, f.E, f.M, r.Ef, r.Mf, f.num, f.ap);
  f.num += r.num;
  f.ap += r.ap;
  f.have = true, f.E = r.El, f.M = r.Ml;
}

// The top group ends at n, where the state is (P, Mtot).  A replicate without a weighted positive or without a
// weighted negative is invalid: num = 0, ap = 0.
BOOT_HD BootRecord boot_fold_end(BootFold f, uint32_t P, uint32_t Mtot) {
  const uint32_t N = Mtot - P;
  if (P == 0 || N == 0) return BootRecord{0ull, P, N, 0.0};
  if (f.have) boot_close_group(P, Mtot, f.E, f.M, P, Mtot, f.num, f.ap);
  return BootRecord{f.num, P, N, f.ap};
}

// ---- workspace: [sums / prefixes: blocks x tiles x 64 x {E, M}] [totals: blocks x 64 x {P, Mtot}]
//                 [starts per tile: tiles x uint32] [tile records: blocks x tiles x 64 x 32 bytes]
// blocks = min(replicate blocks, BOOT_CHUNK_BLOCKS): the entry walks the replicates in chunks of that many blocks.
inline long boot_tiles(long n) { return (n + BOOT_TILE - 1) / BOOT_TILE; }
inline long boot_ws_blocks(long R) {
  const long b = (R + BOOT_BLOCK - 1) / BOOT_BLOCK;
  return b < BOOT_CHUNK_BLOCKS ? b : BOOT_CHUNK_BLOCKS;
}
inline size_t boot_up256(size_t v) { return (v + 255) & ~(size_t)255; }
struct BootLayout {
  size_t sums, totals, starts, records, bytes;
};
inline BootLayout boot_layout(long n, long R) {
  const size_t tiles = (size_t)boot_tiles(n), blocks = (size_t)boot_ws_blocks(R);
  BootLayout l;
  l.sums = 0;
  l.totals = l.sums + boot_up256(blocks * tiles * BOOT_BLOCK * 8);
  l.starts = l.totals + boot_up256(blocks * BOOT_BLOCK * 8);
  l.records = l.starts + boot_up256(tiles * 4);
  l.bytes = l.records + boot_up256(blocks * tiles * BOOT_BLOCK * sizeof(BootTileRecord));
  return l;
}

}  // namespace aaclip

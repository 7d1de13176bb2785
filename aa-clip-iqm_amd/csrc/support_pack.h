// The nearest-patch search of csrc/support.hip, the parts that the device code and a host program share
// (csrc/support_host_check.cpp replays the merge sequentially under a sanitizer): the candidate word with its decode,
// the operand scale of the fp16 form, the tiling and the workspace layout.
//
// A candidate is one 64-bit word,  order-preserving key of the cosine << 32 | (0xFFFFFFFF - bank row) : the integer
// maximum of any set of candidates, taken in any order, is the largest cosine and among equal cosines the lowest bank
// row.  -0.0 counts as +0.0, so a zero of either sign ties with the other.  Every finite cosine packs to a non-zero
// word: a workspace word of 0 means "no candidate yet".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define AACLIP_SP_HD __host__ __device__ inline
#else
#define AACLIP_SP_HD inline
#endif

namespace aaclip {

static constexpr int SUPPORT_FP16 = 1, SUPPORT_FP32 = 0;   // include/aaclip.h AACLIP_SUPPORT_*

// fp16 form: both operands are multiplied by 2^SUPPORT_OPERAND_EXP before they are rounded to fp16 and the fp32
// accumulator by 2^-(2 * SUPPORT_OPERAND_EXP) afterwards -- both exact.  A unit row of 768 components sits near 0.036;
// times 16 even a component 400 times below that is a normal fp16 number (>= 6.1e-5), and a component of 1.0 becomes
// 16, far from fp16's 65504.
static constexpr int SUPPORT_OPERAND_EXP = 4;
static constexpr float SUPPORT_OPERAND_SCALE = (float)(1 << SUPPORT_OPERAND_EXP);
static constexpr float SUPPORT_ACC_SCALE = 1.0f / (float)(1 << (2 * SUPPORT_OPERAND_EXP));

AACLIP_SP_HD uint32_t support_cos_key(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  if (b == 0x80000000u) b = 0u;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
AACLIP_SP_HD float support_key_cos(uint32_t key) {
  const uint32_t b = (key >> 31) ? key ^ 0x80000000u : ~key;
  float v;
  memcpy(&v, &b, 4);
  return v;
}
AACLIP_SP_HD unsigned long long support_pack(float cosine, uint32_t bank_row) {
  return ((unsigned long long)support_cos_key(cosine) << 32) | (unsigned long long)(0xFFFFFFFFu - bank_row);
}
AACLIP_SP_HD float support_word_cos(unsigned long long word) { return support_key_cos((uint32_t)(word >> 32)); }
AACLIP_SP_HD uint32_t support_word_row(unsigned long long word) { return 0xFFFFFFFFu - (uint32_t)(word & 0xFFFFFFFFull); }
AACLIP_SP_HD unsigned long long support_merge(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// ---- tiling: a workgroup owns SUPPORT_TILE query rows and a chunk of whole bank tiles (SUPPORT_TILE bank rows each)
static constexpr int SUPPORT_TILE = 128;
static constexpr long SUPPORT_TARGET_WORKGROUPS = 1024;   // four per CU: what the chunk count aims at
// the grid is (row tiles, chunks): at most SUPPORT_TARGET_WORKGROUPS chunks, far below grid.y's 65535

struct SupportPlan {
  long row_tiles, bank_tiles, chunks, tiles_per_chunk;
};
inline SupportPlan support_plan(long M, long N) {
  SupportPlan p;
  p.row_tiles = (M + SUPPORT_TILE - 1) / SUPPORT_TILE;
  p.bank_tiles = (N + SUPPORT_TILE - 1) / SUPPORT_TILE;
  long want = (SUPPORT_TARGET_WORKGROUPS + p.row_tiles - 1) / p.row_tiles;
  if (want < 1) want = 1;
  if (want > p.bank_tiles) want = p.bank_tiles;
  p.tiles_per_chunk = (p.bank_tiles + want - 1) / want;
  p.chunks = (p.bank_tiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;
  return p;
}

// ---- the workspace: [best word of every query row: M x 8]
struct SupportLayout {
  size_t words, bytes;
};
inline SupportLayout support_layout(long M) {
  SupportLayout l;
  l.words = 0;
  l.bytes = (((size_t)M * 8) + 255) & ~(size_t)255;
  return l;
}

}  // namespace aaclip

// The greedy coreset selection of csrc/coreset.hip, the parts that the device code and a host program share
// (csrc/coreset_host_check.cpp replays them sequentially under a sanitizer): the quantiser, the exact integer distance,
// the candidate word with its decode, the launch plan and the workspace layout.
//
// Rows are quantised once: q_i = clamp(rint(v_i * 2^14), -32767, 32767) as int16 (the product is exact, rint is
// round-half-even, -0.0 and NaN become 0), norm2 = sum q_i^2 as int32, saturated at INT32_MAX.  The selection accepts
// norm2 < 2^29 (a norm up to about 1.41): every dot product then fits int32 by Cauchy-Schwarz, and
//   d2(x, c) = norm2_x + norm2_c - 2 <q_x, q_c>
// is the exact squared distance of the integer rows, below 2^31.  Nothing is rounded after the quantiser, so any
// order of summation and any order of merging gives the same bits.
//
// A candidate is one 64-bit word,  min_d2 << 32 | (0xFFFFFFFF - row) : the integer maximum of any set of candidates,
// taken in any order, is the largest min_d2 and among equal ones the lowest row.  Every candidate is a non-zero word
// (row < 2^31): a workspace word of 0 means "no candidate yet".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define AACLIP_CS_HD __host__ __device__ inline
#else
#define AACLIP_CS_HD inline
#endif

namespace aaclip {

static constexpr int CORESET_SCALE_EXP = 14;
static constexpr float CORESET_SCALE = (float)(1 << CORESET_SCALE_EXP);
static constexpr int CORESET_QMAX = 32767;
static constexpr uint32_t CORESET_NORM2_LIMIT = 1u << 29;   // the selection's precondition: every norm2 below it
static constexpr uint32_t CORESET_D2_INIT = 0xFFFFFFFFu;    // min_d2 before the first pick, radius2[0]

// ---- the quantiser
AACLIP_CS_HD int16_t coreset_quantise(float v) {
  float x = __builtin_rintf(v * CORESET_SCALE);   // v * 2^14 is exact (or overflows to an infinity, which is clamped)
  if (!(x == x)) x = 0.0f;
  if (x > (float)CORESET_QMAX) x = (float)CORESET_QMAX;
  if (x < -(float)CORESET_QMAX) x = -(float)CORESET_QMAX;
  return (int16_t)(int)x;
}
AACLIP_CS_HD int32_t coreset_norm2_saturate(unsigned long long sum) {
  return sum > 0x7FFFFFFFull ? (int32_t)0x7FFFFFFF : (int32_t)sum;
}
// one row on the host: the definition of what coreset_rows_kernel writes
inline int32_t coreset_quantise_row(const float* v, int E, int16_t* q) {
  unsigned long long sum = 0;
  for (int i = 0; i < E; ++i) {
    q[i] = coreset_quantise(v[i]);
    sum += (unsigned long long)((int)q[i] * (int)q[i]);
  }
  return coreset_norm2_saturate(sum);
}

// ---- the distance: modulo 2^32 every step is defined, and the true value lies in [0, 2^31)
AACLIP_CS_HD uint32_t coreset_d2(int32_t norm2_x, int32_t norm2_c, int32_t dot) {
  return (uint32_t)norm2_x + (uint32_t)norm2_c - 2u * (uint32_t)dot;
}
inline int32_t coreset_dot(const int16_t* a, const int16_t* b, int E) {
  uint32_t s = 0;   // wraps like the device's accumulator; the sum itself fits int32 under the precondition
  for (int i = 0; i < E; ++i) s += (uint32_t)((int)a[i] * (int)b[i]);
  return (int32_t)s;
}

// ---- the candidate word
AACLIP_CS_HD unsigned long long coreset_word(uint32_t min_d2, uint32_t row) {
  return ((unsigned long long)min_d2 << 32) | (unsigned long long)(0xFFFFFFFFu - row);
}
AACLIP_CS_HD uint32_t coreset_word_d2(unsigned long long word) { return (uint32_t)(word >> 32); }
AACLIP_CS_HD uint32_t coreset_word_row(unsigned long long word) { return 0xFFFFFFFFu - (uint32_t)(word & 0xFFFFFFFFull); }
AACLIP_CS_HD unsigned long long coreset_merge(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// ---- the launch plan of one pick.  A row of E int16 is E / 8 chunks of 16 bytes; `lanes` lanes of a wave share a row
// (the largest power of two <= the chunk count, at most 64), lane j reads chunk j and, where the row is longer, chunk
// j + lanes -- at most two per lane.  A wave walks groups of 64 / lanes rows, CORESET_UNROLL groups per step; a
// workgroup is CORESET_WAVES waves; the grid strides over the groups and stays at CORESET_MAX_WORKGROUPS, because every
// workgroup ends with one atomic on the same word.
static constexpr int CORESET_WAVES = 8;
static constexpr int CORESET_THREADS = 64 * CORESET_WAVES;
static constexpr int CORESET_UNROLL = 4;
static constexpr long CORESET_MAX_WORKGROUPS = 512;   // two per CU

struct CoresetPlan {
  int lanes_log2, lanes, rows_per_wave;
  long groups, workgroups;
};
inline CoresetPlan coreset_plan(long N, int E) {
  CoresetPlan p;
  const int chunks = E / 8;
  p.lanes_log2 = 2;
  while (p.lanes_log2 < 6 && (2 << p.lanes_log2) <= chunks) ++p.lanes_log2;
  p.lanes = 1 << p.lanes_log2;
  p.rows_per_wave = 64 / p.lanes;
  p.groups = (N + p.rows_per_wave - 1) / p.rows_per_wave;
  const long per_wg = (long)CORESET_WAVES * CORESET_UNROLL;
  p.workgroups = (p.groups + per_wg - 1) / per_wg;
  if (p.workgroups > CORESET_MAX_WORKGROUPS) p.workgroups = CORESET_MAX_WORKGROUPS;
  if (p.workgroups < 1) p.workgroups = 1;
  return p;
}

// ---- the workspace: [candidate word of every pick 0 .. n: (n + 1) x 8]; word 0 is never written (pick 0 is `start`)
struct CoresetLayout {
  size_t words, bytes;
};
inline CoresetLayout coreset_layout(long n) {
  CoresetLayout l;
  l.words = 0;
  l.bytes = (((size_t)(n + 1) * 8) + 255) & ~(size_t)255;
  return l;
}

}  // namespace aaclip

// Attention backward for any sequence length (the visual tower's L = 1370): dq, dk, dv of softmax(q k^T) v per (image,
// head), head dim 64.  With s_ij = q_i . k_j (q pre-scaled), p = softmax_j s, dp_ij = dctx_i . v_j and
// delta_i = sum_j p_ij dp_ij:
//   ds_ij = p_ij (dp_ij - delta_i),  dq_i = sum_j ds_ij k_j,  dk_j = sum_i ds_ij q_i,  dv_j = sum_i p_ij dctx_i.
// Nothing of size L x L leaves the chip and LDS use does not depend on L: three passes over 32-row tiles, in the economy
// of attn32m_kernel (a wave owns 32 rows, a workgroup is 4 waves = 128 rows, the other side's 32-row tiles are
// double-buffered in LDS with one barrier per tile, an accumulator element of the score MFMA is the next MFMA's operand
// as it stands).
//   attn_bwd_stats_kernel  per query row: m = max_j t_ij (t = s log2 e, the exponent domain of the later passes),
//                          1 / sum_j 2^(t_ij - m) and delta_i.  The score loop plus dctx . V^T (NOT the forward's P . V
//                          followed by dctx . ctx): delta is then a sum of the very p dp products it is subtracted from.
//   attn_bwd_dkv_kernel    a wave owns 32 keys and walks the query tiles (from the diagonal tile on, when causal); p and
//                          ds are re-formed from the saved statistics; dk, dv accumulate in registers, 32 keys x 64 dims.
//   attn_bwd_dq_kernel     a wave owns 32 queries and walks the key tiles (up to the diagonal tile, when causal).
// Both later passes form p as exp2(s * log2e - m) * linv (attn_bwd_p).  No atomics: every output element is summed by
// one wave, over the tiles in ascending order and inside a tile in the policy's fixed MFMA order, so two calls give the
// same bits.  The statistics, the exponent and ds = p (dp - delta) are fp32 in every arithmetic.
// Operand maps of a 32x32 MFMA accumulator (lane = 32 h + r): element e = D[row (e & 3) + 8 (e >> 2) + 4 h][col r]; a
// score product puts the tile's rows on the rows and the wave's own rows on the columns.
//
// This header is the skeleton: the ownership of rows, the clamped loads, the causal tile ranges, the masks, the online
// max / sum / delta recurrence, the stage walk, the statistics staging of pass 2, the statistics store and the dq store.
// The arithmetic is a policy P, one per .hip file (AttnBwdF32, AttnBwdBf16x3); a thread constructs one as its view of q,
// k, v, d_ctx of one (image, head):
//   P::Args                         the kernel argument that names the operands
//   P(args, b, head, L, H, lane)
//   P::STAGE_BYTES                  one LDS stage: a 32-row tile of each of two tensors
//   P::ENTRY_NOPS[3]                entry_nops of passes 1, 2, 3
//   P::Own   load(P, field, row)    one row in registers, the own-row operand of a score product
//   P::Tile  load(P, field a, field b, t0, L, tid), store(stage, tid)
//                                   rows t0 .. t0 + 31 (clamped to row L - 1) of two tensors, through registers
//   score(stage, which, own)        acc[tile row][own row] of tensor `which` (0: a, 1: b) of the stage
//   grad_dkv(stage, p, ds, dk, dv)  pass 2: dv += p^T dctx, dk += ds^T q over the stage's 32 queries
//   grad_dq(stage, ds, dq)          pass 3: dq^T[d][query] += sum_key k[key][d] ds[key][query]
//   store_dkv(dqkv, b, L, head, key0, dk, dv)   (the two arithmetics hold dk | dv transposed to each other)
#pragma once
#include "common.h"

namespace aaclip {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float M_START = -1e30f;             // finite: a fully masked tile must not produce inf - inf
enum { ATT_Q = 0, ATT_K = 1, ATT_V = 2, ATT_DCTX = 3 };   // the fields of a policy's view

AACLIP_DEV int mfma_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

AACLIP_DEV void xswap(float& a, float& b) { asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
AACLIP_DEV float half_sum(float v) {   // v of lane (r, 0) + v of lane (r, 1), in that order on both halves
  float a = v, c = v;
  xswap(a, c);
  return a + c;
}
AACLIP_DEV float half_max(float v) {
  float a = v, c = v;
  xswap(a, c);
  return fmaxf(a, c);
}

// the one chain both later passes form a probability with
AACLIP_DEV float attn_bwd_p(float s, float m, float linv) { return __builtin_amdgcn_exp2f(s * LOG2E - m) * linv; }

// N s_nop at a kernel's entry (executed once per wave).  The tile loops are 2 to 6 KiB of dense MFMA issue and their speed
// depends on where they start: the bf16x3 loops, instruction for instruction the same, ran 0.8 to 1.0 % slower a few
// bytes off ("Timing").  A policy names the nops per pass (P::ENTRY_NOPS) that put its loops where they were
// measured; tests/test_host_cpu.py checks the distances in the disassembly.
template <int N> AACLIP_DEV void entry_nops() {
  if constexpr (N > 0) asm volatile(".rept %0\n\ts_nop 0\n\t.endr" ::"n"(N));
}

AACLIP_DEV void zero2(f32x16 (&a)[2]) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) a[db][e] = 0.f;
}

// ------------------------------------------------------------------------------------------------ pass 1: statistics
template <class P>
__global__ __launch_bounds__(256) void attn_bwd_stats_kernel(typename P::Args args, float* __restrict__ stats, int L,
                                                             int H, int causal) {
  __shared__ __attribute__((aligned(16))) char smem[2 * P::STAGE_BYTES];
  entry_nops<P::ENTRY_NOPS[0]>();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const P pol(args, b, head, L, H, lane);
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int qi = q0 + r;
  const int qrow = qi < L ? qi : L - 1;
  typename P::Own qo, go;
  qo.load(pol, ATT_Q, qrow);
  go.load(pol, ATT_DCTX, qrow);
  float m = M_START, l = 0.f, dsum = 0.f;
  int last_q = blockIdx.x * 128 + 127;
  if (last_q > L - 1) last_q = L - 1;
  const int nkt = causal ? (last_q / 32 + 1) : ((L + 31) / 32);

  typename P::Tile tp;
  tp.load(pol, ATT_K, ATT_V, 0, L, tid);
  tp.store(smem, tid);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const char* st = smem + (kt & 1) * P::STAGE_BYTES;
    const int k0 = kt * 32;
    if (kt + 1 < nkt) tp.load(pol, ATT_K, ATT_V, k0 + 32, L, tid);
    if (q0 < L && !(causal && k0 > q0 + 31)) {
      f32x16 s = pol.score(st, 0, qo);
      const f32x16 dp = pol.score(st, 1, go);
      float mt = M_START;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = k0 + mfma_row(e, h);
        const bool dead = (key >= L) || (causal && key > qi);
        s[e] = dead ? -INFINITY : s[e] * LOG2E;
        mt = fmaxf(mt, s[e]);
      }
      const float mn = fmaxf(m, half_max(mt));
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      float rs = 0.f, rd = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float p = __builtin_amdgcn_exp2f(s[e] - mn);   // a dead key: 2^-inf = 0
        rs += p;
        rd = fmaf(p, dp[e], rd);
      }
      l = l * alpha + half_sum(rs);
      dsum = dsum * alpha + half_sum(rd);
      m = mn;
    }
    if (kt + 1 < nkt) tp.store(smem + ((kt & 1) ^ 1) * P::STAGE_BYTES, tid);   // the other stage: everyone left it one barrier ago
    __syncthreads();
  }
  if (qi < L && h == 0) {
    const size_t n = (size_t)gridDim.z * H * L;
    const size_t at = ((size_t)b * H + head) * L + qi;
    const float linv = 1.0f / l;
    stats[at] = m;
    stats[n + at] = linv;
    stats[2 * n + at] = dsum * linv;
  }
}

// ------------------------------------------------------------------------------------------------ pass 2: dk, dv
template <class P>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(typename P::Args args, const float* __restrict__ stats,
                                                           float* __restrict__ dqkv, int L, int H, int causal) {
  __shared__ __attribute__((aligned(16))) char smem[2 * P::STAGE_BYTES];
  __shared__ float St[2][3][32];
  entry_nops<P::ENTRY_NOPS[1]>();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const P pol(args, b, head, L, H, lane);
  const size_t nstat = (size_t)gridDim.z * H * L;
  const float* sbase = stats + ((size_t)b * H + head) * L;
  const int key0 = blockIdx.x * 128 + wave * 32;
  const int kj = key0 + r;
  const int krow = kj < L ? kj : L - 1;
  typename P::Own ko, vo;
  ko.load(pol, ATT_K, krow);
  vo.load(pol, ATT_V, krow);
  f32x16 dk[2], dv[2];
  zero2(dk);
  zero2(dv);
  const int nqt = (L + 31) / 32;
  const int qt0 = causal ? blockIdx.x * 4 : 0;   // the diagonal tile of this workgroup's first wave

  typename P::Tile tp;
  float sreg = 0.f;
  auto load_stats = [&](int t0) {
    if (tid < 96) {
      int row = t0 + (tid & 31);
      row = row < L ? row : L - 1;
      sreg = sbase[(size_t)(tid >> 5) * nstat + row];
    }
  };
  auto store_stats = [&](int st) {
    if (tid < 96) St[st][tid >> 5][tid & 31] = sreg;
  };
  tp.load(pol, ATT_Q, ATT_DCTX, qt0 * 32, L, tid);
  load_stats(qt0 * 32);
  tp.store(smem + (qt0 & 1) * P::STAGE_BYTES, tid);
  store_stats(qt0 & 1);
  __syncthreads();
  for (int qt = qt0; qt < nqt; ++qt) {
    const int sti = qt & 1;
    const char* st = smem + sti * P::STAGE_BYTES;
    const int t0 = qt * 32;
    if (qt + 1 < nqt) {
      tp.load(pol, ATT_Q, ATT_DCTX, t0 + 32, L, tid);
      load_stats(t0 + 32);
    }
    if (key0 < L && !(causal && t0 + 31 < key0)) {
      f32x16 p = pol.score(st, 0, ko);    // s[query (e, h)][key r]
      f32x16 ds = pol.score(st, 1, vo);   // dp
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = mfma_row(e, h);
        const int q = t0 + row;
        const bool dead = (q >= L) || (causal && kj > q);
        const float pe = dead ? 0.f : attn_bwd_p(p[e], St[sti][0][row], St[sti][1][row]);
        p[e] = pe;
        ds[e] = pe * (ds[e] - St[sti][2][row]);
      }
      pol.grad_dkv(st, p, ds, dk, dv);
    }
    if (qt + 1 < nqt) {
      tp.store(smem + (sti ^ 1) * P::STAGE_BYTES, tid);
      store_stats(sti ^ 1);
    }
    __syncthreads();
  }
  pol.store_dkv(dqkv, b, L, head, key0, dk, dv);
}

// ------------------------------------------------------------------------------------------------ pass 3: dq
template <class P>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(typename P::Args args, const float* __restrict__ stats,
                                                          float* __restrict__ dqkv, int L, int H, int causal,
                                                          float dq_scale) {
  __shared__ __attribute__((aligned(16))) char smem[2 * P::STAGE_BYTES];
  entry_nops<P::ENTRY_NOPS[2]>();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const P pol(args, b, head, L, H, lane);
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int qi = q0 + r;
  const int qrow = qi < L ? qi : L - 1;
  typename P::Own qo, go;
  qo.load(pol, ATT_Q, qrow);
  go.load(pol, ATT_DCTX, qrow);
  const size_t nstat = (size_t)gridDim.z * H * L;
  const size_t at = ((size_t)b * H + head) * L + qrow;
  const float m = stats[at], linv = stats[nstat + at], delta = stats[2 * nstat + at];
  f32x16 dq[2];
  zero2(dq);
  int last_q = blockIdx.x * 128 + 127;
  if (last_q > L - 1) last_q = L - 1;
  const int nkt = causal ? (last_q / 32 + 1) : ((L + 31) / 32);

  typename P::Tile tp;
  tp.load(pol, ATT_K, ATT_V, 0, L, tid);
  tp.store(smem, tid);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const char* st = smem + (kt & 1) * P::STAGE_BYTES;
    const int k0 = kt * 32;
    if (kt + 1 < nkt) tp.load(pol, ATT_K, ATT_V, k0 + 32, L, tid);
    if (q0 < L && !(causal && k0 > q0 + 31)) {
      f32x16 ds = pol.score(st, 0, qo);         // s[key (e, h)][query r]
      const f32x16 dp = pol.score(st, 1, go);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = k0 + mfma_row(e, h);
        const bool dead = (key >= L) || (causal && key > qi);
        const float pe = dead ? 0.f : attn_bwd_p(ds[e], m, linv);
        ds[e] = pe * (dp[e] - delta);
      }
      pol.grad_dq(st, ds, dq);
    }
    if (kt + 1 < nkt) tp.store(smem + ((kt & 1) ^ 1) * P::STAGE_BYTES, tid);
    __syncthreads();
  }
  if (qi < L) {   // dq[db][e] = dq[query r][d = 32 db + (e, h)]: registers 4 g .. 4 g + 3 are d = 32 db + 8 g + 4 h ..
    float* dst = dqkv + ((long)b * L + qi) * (3L * H * 64) + head * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = dq[db][4 * g + j] * dq_scale;
        *(f32x4*)(dst + db * 32 + 8 * g + 4 * h) = v;
      }
  }
}

}  // namespace aaclip

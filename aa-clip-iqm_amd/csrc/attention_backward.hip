// Attention backward for any sequence length (the visual tower's L = 1370): dq, dk, dv of softmax(q k^T) v per (image,
// head), head dim 64, all five products on v_mfma_f32_32x32x2_f32 (an exact fmaf chain).  With s_ij = q_i . k_j (q
// pre-scaled), p = softmax_j s, dp_ij = dctx_i . v_j and delta_i = sum_j p_ij dp_ij:
//   ds_ij = p_ij (dp_ij - delta_i),  dq_i = sum_j ds_ij k_j,  dk_j = sum_i ds_ij q_i,  dv_j = sum_i p_ij dctx_i.
// Nothing of size L x L leaves the chip and LDS use does not depend on L: three passes over 32-row tiles, in the economy
// of attn32m_kernel (a wave owns 32 rows, a workgroup is 4 waves = 128 rows, the other side's 32-row tiles are
// double-buffered in LDS, an accumulator element of the score MFMA is the next MFMA's operand as it stands).
//   attn_bwd_stats_kernel  per query row: m = max_j t_ij (t = s log2 e, the exponent domain of the later passes),
//                          1 / sum_j 2^(t_ij - m) and delta_i.  The score loop plus dctx . V^T (NOT the forward's P . V
//                          followed by dctx . ctx): delta is then a sum of the very p dp products it is subtracted from.
//   attn_bwd_dkv_kernel    a wave owns 32 keys and walks the query tiles (from the diagonal tile on, when causal); p and
//                          ds are re-formed from the saved statistics; dk, dv accumulate in registers, 32 keys x 64 dims.
//   attn_bwd_dq_kernel     a wave owns 32 queries and walks the key tiles (up to the diagonal tile, when causal).
// Both later passes form p as exp2(s * log2e - m) * linv from a score that the MFMA summed over d = 0, 1, .., 63 in that
// order (attn_bwd_p): the same bits on both sides.  No atomics: every output element is summed by one wave, over the
// tiles in ascending order and inside a tile in the MFMA's fixed order, so two calls give the same bits.
// Operand maps of the 32x32x2 MFMA (lane = 32 h + r): A[row r][k = h], B[k = h][col r], accumulator element e =
// D[row (e & 3) + 8 (e >> 2) + 4 h][col r].
// LDS: a tile is 32 rows x 64 floats at a row stride of 65 floats, which serves both operand roles without a second
// copy -- as the A operand of a score product (row r, column 2 i + h: banks r + 2 i + h) and as the transposed operand
// of a gradient product (row (i, h), column r: banks r + const).  The loops are bound by the matrix pipe (64 to 128
// MFMAs of 64 cycles per tile and wave against as many 4-byte LDS reads), so the wider reads of a de-interleaved second
// copy would buy nothing.  Two tiles per stage, two stages, plus 3 x 32 statistics in the dk / dv pass: 34 048 bytes.
#include "common.h"
#include "kernels.h"

namespace aaclip {

namespace {

constexpr int TLD = 65;                       // tile row stride in floats
constexpr float LOG2E = 1.4426950408889634f;
constexpr float M_START = -1e30f;             // finite: a fully masked tile must not produce inf - inf

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

// row `row` (clamped to the last one) of a [L, ld] matrix: this lane's 32 values d = 2 i + h, the B operand of a score MFMA
AACLIP_DEV void load_own_row(const float* __restrict__ src, long ld, int row, int h, float (&reg)[32]) {
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const f32x4 v = *(const f32x4*)(src + (long)row * ld + 4 * c);
    reg[2 * c] = h ? v[1] : v[0];
    reg[2 * c + 1] = h ? v[3] : v[2];
  }
}

// Two 32-row tiles (rows t0 .. t0 + 31 of a and of b, clamped to row L - 1) through registers into one LDS stage.
struct TilePair {
  f32x4 ra[2], rb[2];
  AACLIP_DEV void load(const float* __restrict__ a, long lda, const float* __restrict__ b, long ldb, int t0, int L,
                       int tid) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + 256 * j;
      int row = t0 + (idx >> 4);
      row = row < L ? row : L - 1;
      const int c4 = (idx & 15) * 4;
      ra[j] = *(const f32x4*)(a + (long)row * lda + c4);
      rb[j] = *(const f32x4*)(b + (long)row * ldb + c4);
    }
  }
  AACLIP_DEV void store(float* As, float* Bs, int tid) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + 256 * j;
      const int o = (idx >> 4) * TLD + (idx & 15) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        As[o + e] = ra[j][e];
        Bs[o + e] = rb[j][e];
      }
    }
  }
};

// acc[row = tile row][col = own row] += sum_d T[row][d] own[d], d ascending
AACLIP_DEV f32x16 score_product(const float* T, const float (&own)[32], int r, int h) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(T[r * TLD + 2 * i + h], own[i], acc, 0, 0, 0);
  return acc;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ pass 1: statistics
__global__ __launch_bounds__(256) void attn_bwd_stats_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                             float* __restrict__ stats, int L, int H, int causal) {
  __shared__ float Ks[2][32 * TLD];
  __shared__ float Vs[2][32 * TLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = H * 64;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * L * ld + head * 64;
  const float* dbase = dctx + (long)b * L * D + head * 64;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int qi = q0 + r;
  const int qrow = qi < L ? qi : L - 1;
  float qreg[32], dreg[32];
  load_own_row(base, ld, qrow, h, qreg);
  load_own_row(dbase, D, qrow, h, dreg);
  float m = M_START, l = 0.f, dsum = 0.f;
  int last_q = blockIdx.x * 128 + 127;
  if (last_q > L - 1) last_q = L - 1;
  const int nkt = causal ? (last_q / 32 + 1) : ((L + 31) / 32);

  TilePair tp;
  tp.load(base + D, ld, base + 2 * D, ld, 0, L, tid);
  tp.store(Ks[0], Vs[0], tid);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int st = kt & 1;
    const int k0 = kt * 32;
    if (kt + 1 < nkt) tp.load(base + D, ld, base + 2 * D, ld, k0 + 32, L, tid);
    if (q0 < L && !(causal && k0 > q0 + 31)) {
      f32x16 s = score_product(Ks[st], qreg, r, h);
      const f32x16 dp = score_product(Vs[st], dreg, r, h);
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
    if (kt + 1 < nkt) tp.store(Ks[st ^ 1], Vs[st ^ 1], tid);   // the other stage: everyone left it one barrier ago
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
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                           const float* __restrict__ stats, float* __restrict__ dqkv,
                                                           int L, int H, int causal) {
  __shared__ float Qs[2][32 * TLD];
  __shared__ float Ds[2][32 * TLD];
  __shared__ float St[2][3][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = H * 64;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * L * ld + head * 64;
  const float* dbase = dctx + (long)b * L * D + head * 64;
  const size_t nstat = (size_t)gridDim.z * H * L;
  const float* sbase = stats + ((size_t)b * H + head) * L;
  const int key0 = blockIdx.x * 128 + wave * 32;
  const int kj = key0 + r;
  const int krow = kj < L ? kj : L - 1;
  float kreg[32], vreg[32];
  load_own_row(base + D, ld, krow, h, kreg);
  load_own_row(base + 2 * D, ld, krow, h, vreg);
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) dk[db][e] = dv[db][e] = 0.f;
  const int nqt = (L + 31) / 32;
  const int qt0 = causal ? blockIdx.x * 4 : 0;   // the diagonal tile of this workgroup's first wave

  TilePair tp;
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
  tp.load(base, ld, dbase, D, qt0 * 32, L, tid);
  load_stats(qt0 * 32);
  tp.store(Qs[qt0 & 1], Ds[qt0 & 1], tid);
  store_stats(qt0 & 1);
  __syncthreads();
  for (int qt = qt0; qt < nqt; ++qt) {
    const int st = qt & 1;
    const int t0 = qt * 32;
    if (qt + 1 < nqt) {
      tp.load(base, ld, dbase, D, t0 + 32, L, tid);
      load_stats(t0 + 32);
    }
    if (key0 < L && !(causal && t0 + 31 < key0)) {
      f32x16 p = score_product(Qs[st], kreg, r, h);    // s[query (e, h)][key r]
      f32x16 ds = score_product(Ds[st], vreg, r, h);   // dp
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = mfma_row(e, h);
        const int q = t0 + row;
        const bool dead = (q >= L) || (causal && kj > q);
        const float pe = dead ? 0.f : attn_bwd_p(p[e], St[st][0][row], St[st][1][row]);
        p[e] = pe;
        ds[e] = pe * (ds[e] - St[st][2][row]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int o = mfma_row(i, h) * TLD + r;
        dv[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[i], Ds[st][o], dv[0], 0, 0, 0);
        dv[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[i], Ds[st][o + 32], dv[1], 0, 0, 0);
        dk[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[i], Qs[st][o], dk[0], 0, 0, 0);
        dk[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[i], Qs[st][o + 32], dk[1], 0, 0, 0);
      }
    }
    if (qt + 1 < nqt) {
      tp.store(Qs[st ^ 1], Ds[st ^ 1], tid);
      store_stats(st ^ 1);
    }
    __syncthreads();
  }
  // dk[key (e, h)][d = 32 db + r]
  float* out = dqkv + (long)b * L * ld + head * 64;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int key = key0 + mfma_row(e, h);
    if (key < L) {
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        out[(long)key * ld + D + db * 32 + r] = dk[db][e];
        out[(long)key * ld + 2 * D + db * 32 + r] = dv[db][e];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ pass 3: dq
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                          const float* __restrict__ stats, float* __restrict__ dqkv,
                                                          int L, int H, int causal, float dq_scale) {
  __shared__ float Ks[2][32 * TLD];
  __shared__ float Vs[2][32 * TLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = H * 64;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * L * ld + head * 64;
  const float* dbase = dctx + (long)b * L * D + head * 64;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int qi = q0 + r;
  const int qrow = qi < L ? qi : L - 1;
  float qreg[32], dreg[32];
  load_own_row(base, ld, qrow, h, qreg);
  load_own_row(dbase, D, qrow, h, dreg);
  const size_t nstat = (size_t)gridDim.z * H * L;
  const size_t at = ((size_t)b * H + head) * L + qrow;
  const float m = stats[at], linv = stats[nstat + at], delta = stats[2 * nstat + at];
  f32x16 dq[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) dq[db][e] = 0.f;
  int last_q = blockIdx.x * 128 + 127;
  if (last_q > L - 1) last_q = L - 1;
  const int nkt = causal ? (last_q / 32 + 1) : ((L + 31) / 32);

  TilePair tp;
  tp.load(base + D, ld, base + 2 * D, ld, 0, L, tid);
  tp.store(Ks[0], Vs[0], tid);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int st = kt & 1;
    const int k0 = kt * 32;
    if (kt + 1 < nkt) tp.load(base + D, ld, base + 2 * D, ld, k0 + 32, L, tid);
    if (q0 < L && !(causal && k0 > q0 + 31)) {
      f32x16 ds = score_product(Ks[st], qreg, r, h);         // s[key (e, h)][query r]
      const f32x16 dp = score_product(Vs[st], dreg, r, h);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = k0 + mfma_row(e, h);
        const bool dead = (key >= L) || (causal && key > qi);
        const float pe = dead ? 0.f : attn_bwd_p(ds[e], m, linv);
        ds[e] = pe * (dp[e] - delta);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {   // dq^T[d][query] += K^T[d][key (i, h)] ds[key][query]
        const int o = mfma_row(i, h) * TLD + r;
        dq[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[st][o], ds[i], dq[0], 0, 0, 0);
        dq[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[st][o + 32], ds[i], dq[1], 0, 0, 0);
      }
    }
    if (kt + 1 < nkt) tp.store(Ks[st ^ 1], Vs[st ^ 1], tid);
    __syncthreads();
  }
  if (qi < L) {
    float* dst = dqkv + ((long)b * L + qi) * ld + head * 64;
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

// ------------------------------------------------------------------------------------------------ host side
const char* attention_backward_long_check(int B, int L, int H) {
  if (B <= 0 || L <= 0 || H <= 0) return "attention_backward_long: empty problem";
  if (B > 65535 || H > 65535) return "attention_backward_long: grid limit";
  if ((long)B * L * 3 * 64 * H >= (1L << 40)) return "attention_backward_long: problem too large";
  return nullptr;
}

size_t attention_backward_long_ws_bytes(int B, int L, int H) {
  if (B <= 0 || L <= 0 || H <= 0) return 0;
  return ((size_t)3 * B * H * L * 4 + 255) & ~(size_t)255;
}

void launch_attention_backward_long(const float* qkv, const float* dctx, float* dqkv, int B, int L, int H, int causal,
                                    float dq_scale, void* ws, hipStream_t s) {
  float* stats = (float*)ws;
  const dim3 g((L + 127) / 128, H, B);
  hipLaunchKernelGGL(attn_bwd_stats_kernel, g, dim3(256), 0, s, qkv, dctx, stats, L, H, causal);
  hipLaunchKernelGGL(attn_bwd_dkv_kernel, g, dim3(256), 0, s, qkv, dctx, stats, dqkv, L, H, causal);
  hipLaunchKernelGGL(attn_bwd_dq_kernel, g, dim3(256), 0, s, qkv, dctx, stats, dqkv, L, H, causal, dq_scale);
}

}  // namespace aaclip

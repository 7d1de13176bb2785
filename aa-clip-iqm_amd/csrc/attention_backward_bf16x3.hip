// Attention backward for any sequence length in the three-term bf16 arithmetic (bf16x3.h): launch_attention_backward_long's
// contract and pass structure (attention_backward.hip: statistics, then dk | dv, then dq; same formulas, same masking,
// nothing of size L x L in memory, no atomics), with all five products on v_mfma_f32_32x32x16_bf16 as
//   X.Y = Xl.Yh + Xh.Yl + Xh.Yh   (hi = bf16(v), lo = bf16(v - hi); fp32 accumulation, the two small terms first).
// The statistics m, 1 / sum and delta, the exponent and ds = p (dp - delta) are fp32.
//   attn3_split_kernel  writes the hi and lo planes of q, k, v and d_ctx once, per (image, head) as [L][64] bf16 (a 32-row
//                       tile of a plane is 4 KiB of consecutive memory); the passes then never convert an input again.
//   attn3_stats_kernel  a wave owns 32 queries and walks the key tiles: s^T = K q^T and dp^T = V dctx^T, 12 MFMAs each.
//   attn3_dkv_kernel    a wave owns 32 keys and walks the query tiles: s = Q k^T, dp = Dctx v^T, then dv^T += Dctx^T p and
//                       dk^T += Q^T ds with p and ds split in registers -- an accumulator of a score MFMA has its column
//                       on the lane and its rows in the registers, so registers 8 s .. 8 s + 7 are the B fragment of k-step
//                       s of the next MFMA as they stand (rows {0..3, 8..11} + 4 h + 16 s); the A fragment for those rows
//                       comes from the same LDS tile by ds_read_b64_tr_b16, as attention.hip reads V for P.V.
//   attn3_dq_kernel     a wave owns 32 queries and walks the key tiles: s^T, dp^T as in pass 1, dq^T += K^T ds.
// Every output element is summed by one wave, over the tiles in ascending order and inside a tile in the order above:
// two calls give the same bits.  p of pass 2 and of pass 3 agree to rounding only (the small terms swap roles).
// LDS: a stage is four 32-row planes (x hi, x lo, y hi, y lo) of 128-byte rows in common.h's tile image (tile_off: both
// the row reads of a score product and the transposed reads of a gradient product are conflict-free on it), 16 KiB; two
// stages, plus 3 x 32 statistics per stage in pass 2: 33 536 bytes.  Registers (pass 2, the largest): own rows 64,
// dk | dv 64, s | dp 32, the split p and ds 32, the tile in flight 16.
// Per 32 x 32 tile a wave issues 24 (pass 1), 48 (pass 2) and 36 (pass 3) MFMAs of 32 cycles against 64, 128 and 96 of
// 64 cycles in the fp32 kernels.
#include "bf16x3.h"
#include "common.h"

namespace aaclip {

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float M_START = -1e30f;             // finite: a fully masked tile must not produce inf - inf
constexpr int PLANE = 4096;                   // bytes of a 32-row plane in LDS
constexpr int STAGE = 4 * PLANE;

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

AACLIP_DEV float attn3_p(float s, float m, float linv) { return __builtin_amdgcn_exp2f(s * LOG2E - m) * linv; }

// The eight planes of the workspace, each [B][H][L][64] bf16
struct Planes {
  const bf16* p[8];   // q hi, q lo, k hi, k lo, v hi, v lo, dctx hi, dctx lo
};

// row `row` of the hi and lo planes as the B fragments of a score product: element j of k-step ks is d = 16 ks + 8 h + j
struct OwnRow {
  bf16x8 hi[4], lo[4];
  AACLIP_DEV void load(const bf16* ph, const bf16* pl, int row, int h) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      hi[ks] = *(const bf16x8*)(ph + (long)row * 64 + 16 * ks + 8 * h);
      lo[ks] = *(const bf16x8*)(pl + (long)row * 64 + 16 * ks + 8 * h);
    }
  }
};

// Rows t0 .. t0 + 31 (clamped to row L - 1) of four planes through registers into one LDS stage: thread tid moves
// chunk tid & 7 (16 bytes) of row tid >> 3.
struct Tile4 {
  u32x4 v[4];
  AACLIP_DEV void load(const bf16* a, const bf16* b, const bf16* c, const bf16* d, int t0, int L, int tid) {
    int row = t0 + (tid >> 3);
    row = row < L ? row : L - 1;
    const long o = (long)row * 64 + (tid & 7) * 8;
    v[0] = *(const u32x4*)(a + o);
    v[1] = *(const u32x4*)(b + o);
    v[2] = *(const u32x4*)(c + o);
    v[3] = *(const u32x4*)(d + o);
  }
  AACLIP_DEV void store(char* stage, int tid) const {
    const int o = tile_off(tid >> 3, tid & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) *(u32x4*)(stage + i * PLANE + o) = v[i];
  }
};

// Per-lane byte offsets inside a plane.  row[ks]: the A fragment of k-step ks of a score product (row r, d = 16 ks +
// 8 h ..).  tr[s][db][j]: the two transposed reads of k-step s of a gradient product for columns 32 db + r -- lane
// 4 q + p of a 16-lane group g addresses row 16 s + 8 j + 4 (g >> 1) + q, columns 32 db + 16 (g & 1) + 4 p .. + 3, and
// lane i of the group receives column i of those four rows: rows {0..3} + 4 h + 8 j + 16 s of column 32 db + r.
struct Offsets {
  int row[4];
  int tr[2][2][2];
  AACLIP_DEV void init(int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) row[ks] = tile_off(r, 2 * ks + h);
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          tr[s][db][j] = tile_off(16 * s + 8 * j + 4 * (g >> 1) + q, 4 * db + 2 * (g & 1) + (p >> 1)) + 8 * (p & 1);
  }
};

// acc[row = tile row][col = own row] = sum_d T[row][d] own[d] in three terms
AACLIP_DEV f32x16 score3(const char* th, const char* tl, const Offsets& of, const OwnRow& own) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  bf16x8 a[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) acc = Elem<bf16>::mma32(*(const bf16x8*)(tl + of.row[ks]), own.hi[ks], acc);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    a[ks] = *(const bf16x8*)(th + of.row[ks]);
    acc = Elem<bf16>::mma32(a[ks], own.lo[ks], acc);
  }
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) acc = Elem<bf16>::mma32(a[ks], own.hi[ks], acc);
  return acc;
}

AACLIP_DEV bf16x8 tr_read(const char* plane, const int (&o)[2]) {
  const i16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(plane + o[0]));
  const i16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(plane + o[1]));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// acc[db][row = d 32 db + ..][col = lane's column] += sum_t T[t][d] w[t][col], w = a score accumulator, in three terms
AACLIP_DEV void grad3(const char* th, const char* tl, const Offsets& of, const f32x16& w, f32x16 (&acc)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 wh, wl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wh[j] = (bf16)w[8 * s + j];
      wl[j] = (bf16)(w[8 * s + j] - (float)wh[j]);
    }
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      const bf16x8 xh = tr_read(th, of.tr[s][db]);
      const bf16x8 xl = tr_read(tl, of.tr[s][db]);
      acc[db] = Elem<bf16>::mma32(xl, wh, acc[db]);
      acc[db] = Elem<bf16>::mma32(xh, wl, acc[db]);
      acc[db] = Elem<bf16>::mma32(xh, wh, acc[db]);
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ pre-pass: the planes
__global__ __launch_bounds__(256) void attn3_split_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                          bf16* __restrict__ planes, long n, int L, int H) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // 8 values of one (row, tensor, head)
  if (i >= n) return;
  const int per_row = 32 * H;
  const long row = i / per_row;
  const int u = (int)(i - row * per_row);
  const int t = u / (8 * H), rem = u - t * 8 * H;
  const int head = rem >> 3, c = rem & 7;
  const long D = 64L * H;
  const float* src = t < 3 ? qkv + row * 3 * D + t * D + head * 64 + c * 8 : dctx + row * D + head * 64 + c * 8;
  const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  bf16x8 hi, lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    hi[e] = (bf16)v[e];
    lo[e] = (bf16)(v[e] - (float)hi[e]);
  }
  const long bi = row / L, l = row - bi * L;
  const long plane = 2 * n;   // elements of one plane: B * L * H * 64
  bf16* dst = planes + (2 * t) * plane + ((bi * H + head) * L + l) * 64 + c * 8;
  *(bf16x8*)dst = hi;
  *(bf16x8*)(dst + plane) = lo;
}

// ------------------------------------------------------------------------------------------------ pass 1: statistics
__global__ __launch_bounds__(256) void attn3_stats_kernel(Planes pl, float* __restrict__ stats, int L, int H, int causal) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const long hb = ((long)b * H + head) * L * 64;
  const bf16 *qh = pl.p[0] + hb, *ql = pl.p[1] + hb, *kh = pl.p[2] + hb, *kl = pl.p[3] + hb;
  const bf16 *vh = pl.p[4] + hb, *vl = pl.p[5] + hb, *dh = pl.p[6] + hb, *dl = pl.p[7] + hb;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int qi = q0 + r;
  const int qrow = qi < L ? qi : L - 1;
  OwnRow qo, go;
  qo.load(qh, ql, qrow, h);
  go.load(dh, dl, qrow, h);
  Offsets of;
  of.init(lane);
  float m = M_START, l = 0.f, dsum = 0.f;
  int last_q = blockIdx.x * 128 + 127;
  if (last_q > L - 1) last_q = L - 1;
  const int nkt = causal ? (last_q / 32 + 1) : ((L + 31) / 32);

  Tile4 tp;
  tp.load(kh, kl, vh, vl, 0, L, tid);
  tp.store(smem, tid);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const char* st = smem + (kt & 1) * STAGE;
    const int k0 = kt * 32;
    if (kt + 1 < nkt) tp.load(kh, kl, vh, vl, k0 + 32, L, tid);
    if (q0 < L && !(causal && k0 > q0 + 31)) {
      f32x16 s = score3(st, st + PLANE, of, qo);
      const f32x16 dp = score3(st + 2 * PLANE, st + 3 * PLANE, of, go);
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
    if (kt + 1 < nkt) tp.store(smem + ((kt & 1) ^ 1) * STAGE, tid);   // the other stage: everyone left it one barrier ago
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
__global__ __launch_bounds__(256) void attn3_dkv_kernel(Planes pl, const float* __restrict__ stats,
                                                        float* __restrict__ dqkv, int L, int H, int causal) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  __shared__ float St[2][3][32];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = H * 64;
  const long ld = 3L * D;
  const long hb = ((long)b * H + head) * L * 64;
  const bf16 *qh = pl.p[0] + hb, *ql = pl.p[1] + hb, *kh = pl.p[2] + hb, *kl = pl.p[3] + hb;
  const bf16 *vh = pl.p[4] + hb, *vl = pl.p[5] + hb, *dh = pl.p[6] + hb, *dl = pl.p[7] + hb;
  const size_t nstat = (size_t)gridDim.z * H * L;
  const float* sbase = stats + ((size_t)b * H + head) * L;
  const int key0 = blockIdx.x * 128 + wave * 32;
  const int kj = key0 + r;
  const int krow = kj < L ? kj : L - 1;
  OwnRow ko, vo;
  ko.load(kh, kl, krow, h);
  vo.load(vh, vl, krow, h);
  Offsets of;
  of.init(lane);
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) dk[db][e] = dv[db][e] = 0.f;
  const int nqt = (L + 31) / 32;
  const int qt0 = causal ? blockIdx.x * 4 : 0;   // the diagonal tile of this workgroup's first wave

  Tile4 tp;
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
  tp.load(qh, ql, dh, dl, qt0 * 32, L, tid);
  load_stats(qt0 * 32);
  tp.store(smem + (qt0 & 1) * STAGE, tid);
  store_stats(qt0 & 1);
  __syncthreads();
  for (int qt = qt0; qt < nqt; ++qt) {
    const int sti = qt & 1;
    const char* st = smem + sti * STAGE;
    const int t0 = qt * 32;
    if (qt + 1 < nqt) {
      tp.load(qh, ql, dh, dl, t0 + 32, L, tid);
      load_stats(t0 + 32);
    }
    if (key0 < L && !(causal && t0 + 31 < key0)) {
      f32x16 p = score3(st, st + PLANE, of, ko);                      // s[query (e, h)][key r]
      f32x16 ds = score3(st + 2 * PLANE, st + 3 * PLANE, of, vo);     // dp
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = mfma_row(e, h);
        const int q = t0 + row;
        const bool dead = (q >= L) || (causal && kj > q);
        const float pe = dead ? 0.f : attn3_p(p[e], St[sti][0][row], St[sti][1][row]);
        p[e] = pe;
        ds[e] = pe * (ds[e] - St[sti][2][row]);
      }
      grad3(st + 2 * PLANE, st + 3 * PLANE, of, p, dv);   // dv^T[d][key] += sum_q dctx[q][d] p[q][key]
      grad3(st, st + PLANE, of, ds, dk);                  // dk^T[d][key] += sum_q q[q][d] ds[q][key]
    }
    if (qt + 1 < nqt) {
      tp.store(smem + (sti ^ 1) * STAGE, tid);
      store_stats(sti ^ 1);
    }
    __syncthreads();
  }
  // dk[db][e] = dk[key r][d = 32 db + (e, h)]: registers 4 g .. 4 g + 3 are d = 32 db + 8 g + 4 h ..
  if (kj < L) {
    float* out = dqkv + ((long)b * L + kj) * ld + head * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 a, c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = dk[db][4 * g + j];
          c[j] = dv[db][4 * g + j];
        }
        *(f32x4*)(out + D + db * 32 + 8 * g + 4 * h) = a;
        *(f32x4*)(out + 2 * D + db * 32 + 8 * g + 4 * h) = c;
      }
  }
}

// ------------------------------------------------------------------------------------------------ pass 3: dq
__global__ __launch_bounds__(256) void attn3_dq_kernel(Planes pl, const float* __restrict__ stats,
                                                       float* __restrict__ dqkv, int L, int H, int causal,
                                                       float dq_scale) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = H * 64;
  const long ld = 3L * D;
  const long hb = ((long)b * H + head) * L * 64;
  const bf16 *qh = pl.p[0] + hb, *ql = pl.p[1] + hb, *kh = pl.p[2] + hb, *kl = pl.p[3] + hb;
  const bf16 *vh = pl.p[4] + hb, *vl = pl.p[5] + hb, *dh = pl.p[6] + hb, *dl = pl.p[7] + hb;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const int qi = q0 + r;
  const int qrow = qi < L ? qi : L - 1;
  OwnRow qo, go;
  qo.load(qh, ql, qrow, h);
  go.load(dh, dl, qrow, h);
  Offsets of;
  of.init(lane);
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

  Tile4 tp;
  tp.load(kh, kl, vh, vl, 0, L, tid);
  tp.store(smem, tid);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const char* st = smem + (kt & 1) * STAGE;
    const int k0 = kt * 32;
    if (kt + 1 < nkt) tp.load(kh, kl, vh, vl, k0 + 32, L, tid);
    if (q0 < L && !(causal && k0 > q0 + 31)) {
      f32x16 ds = score3(st, st + PLANE, of, qo);                          // s[key (e, h)][query r]
      const f32x16 dp = score3(st + 2 * PLANE, st + 3 * PLANE, of, go);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = k0 + mfma_row(e, h);
        const bool dead = (key >= L) || (causal && key > qi);
        const float pe = dead ? 0.f : attn3_p(ds[e], m, linv);
        ds[e] = pe * (dp[e] - delta);
      }
      grad3(st, st + PLANE, of, ds, dq);   // dq^T[d][query] += sum_key k[key][d] ds[key][query]
    }
    if (kt + 1 < nkt) tp.store(smem + ((kt & 1) ^ 1) * STAGE, tid);
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
// the row statistics (3 * B * H * L floats), then the eight planes of B * H * L * 64 bf16
size_t attention_backward_long_bf16x3_ws_bytes(int B, int L, int H) {
  if (B <= 0 || L <= 0 || H <= 0) return 0;
  return attention_backward_long_ws_bytes(B, L, H) + (size_t)8 * B * H * L * 128;
}

void launch_attention_backward_long_bf16x3(const float* qkv, const float* dctx, float* dqkv, int B, int L, int H,
                                           int causal, float dq_scale, void* ws, hipStream_t s) {
  float* stats = (float*)ws;
  bf16* planes = (bf16*)((char*)ws + attention_backward_long_ws_bytes(B, L, H));
  const long plane = (long)B * H * L * 64;
  Planes pl;
  for (int i = 0; i < 8; ++i) pl.p[i] = planes + i * plane;
  const long n = (long)B * L * H * 32;
  hipLaunchKernelGGL(attn3_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, qkv, dctx, planes, n, L, H);
  const dim3 g((L + 127) / 128, H, B);
  hipLaunchKernelGGL(attn3_stats_kernel, g, dim3(256), 0, s, pl, stats, L, H, causal);
  hipLaunchKernelGGL(attn3_dkv_kernel, g, dim3(256), 0, s, pl, stats, dqkv, L, H, causal);
  hipLaunchKernelGGL(attn3_dq_kernel, g, dim3(256), 0, s, pl, stats, dqkv, L, H, causal, dq_scale);
}

}  // namespace aaclip

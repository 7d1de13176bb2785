// Attention backward for any sequence length in the three-term bf16 arithmetic (bf16x3.h): the policy of
// attention_backward_passes.h (the formulas and the three passes are there; launch_attention_backward_long's contract),
// with all five products on v_mfma_f32_32x32x16_bf16 as
//   X.Y = Xl.Yh + Xh.Yl + Xh.Yh   (hi = bf16(v), lo = bf16(v - hi); fp32 accumulation, the two small terms first).
//   attn3_split_kernel  writes the hi and lo planes of q, k, v and d_ctx once, per (image, head) as [L][64] bf16 (a 32-row
//                       tile of a plane is 4 KiB of consecutive memory); the passes then never convert an input again.
//   pass 1, pass 3      s^T = K q^T and dp^T = V dctx^T, 12 MFMAs each; pass 3 then dq^T += K^T ds.
//   pass 2              s = Q k^T, dp = Dctx v^T, then dv^T += Dctx^T p and dk^T += Q^T ds with p and ds split in
//                       registers -- an accumulator of a score MFMA has its column on the lane and its rows in the
//                       registers, so registers 8 s .. 8 s + 7 are the B fragment of k-step s of the next MFMA as they
//                       stand (rows {0..3, 8..11} + 4 h + 16 s); the A fragment for those rows comes from the same LDS
//                       tile by ds_read_b64_tr_b16, as attention.hip reads V for P.V.
// p of pass 2 and of pass 3 agree to rounding only (the small terms swap roles).
// LDS: a stage is four 32-row planes (x hi, x lo, y hi, y lo) of 128-byte rows in common.h's tile image (tile_off: both
// the row reads of a score product and the transposed reads of a gradient product are conflict-free on it), 16 KiB; two
// stages, plus 3 x 32 statistics per stage in pass 2: 33 536 bytes.  Registers (pass 2, the largest): own rows 64,
// dk | dv 64, s | dp 32, the split p and ds 32, the tile in flight 16.
// Per 32 x 32 tile a wave issues 24 (pass 1), 48 (pass 2) and 36 (pass 3) MFMAs of 32 cycles against 64, 128 and 96 of
// 64 cycles in the fp32 kernels.
#include "attention_backward_passes.h"
#include "bf16x3.h"

namespace aaclip {

namespace {

constexpr int PLANE = 4096;                   // bytes of a 32-row plane in LDS

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

struct AttnBwdBf16x3 {
  static constexpr int STAGE_BYTES = 4 * PLANE;
  static constexpr int ENTRY_NOPS[3] = {2, 63, 2};   // loops at 904, 1380 and 1656 bytes from the entry
  // The eight planes of the workspace, each [B][H][L][64] bf16: q hi, q lo, k hi, k lo, v hi, v lo, dctx hi, dctx lo
  struct Args {
    const bf16* p[8];
  };
  const bf16* pl[8];   // field f of this (image, head): hi pl[2 f], lo pl[2 f + 1]
  Offsets of;
  int D, r, h;
  AACLIP_DEV AttnBwdBf16x3(const Args& a, int b, int head, int L, int H, int lane)
      : D(H * 64), r(lane & 31), h(lane >> 5) {
    const long hb = ((long)b * H + head) * L * 64;
#pragma unroll
    for (int i = 0; i < 8; ++i) pl[i] = a.p[i] + hb;
    of.init(lane);
  }

  struct Own : OwnRow {
    AACLIP_DEV void load(const AttnBwdBf16x3& v, int f, int row) { OwnRow::load(v.pl[2 * f], v.pl[2 * f + 1], row, v.h); }
  };
  struct Tile : Tile4 {
    AACLIP_DEV void load(const AttnBwdBf16x3& v, int fa, int fb, int t0, int L, int tid) {
      Tile4::load(v.pl[2 * fa], v.pl[2 * fa + 1], v.pl[2 * fb], v.pl[2 * fb + 1], t0, L, tid);
    }
  };

  AACLIP_DEV f32x16 score(const char* st, int which, const Own& own) const {
    return score3(st + 2 * which * PLANE, st + (2 * which + 1) * PLANE, of, own);
  }
  AACLIP_DEV void grad_dkv(const char* st, const f32x16& p, const f32x16& ds, f32x16 (&dk)[2], f32x16 (&dv)[2]) const {
    grad3(st + 2 * PLANE, st + 3 * PLANE, of, p, dv);   // dv^T[d][key] += sum_q dctx[q][d] p[q][key]
    grad3(st, st + PLANE, of, ds, dk);                  // dk^T[d][key] += sum_q q[q][d] ds[q][key]
  }
  AACLIP_DEV void grad_dq(const char* st, const f32x16& ds, f32x16 (&dq)[2]) const { grad3(st, st + PLANE, of, ds, dq); }

  // dk[db][e] = dk[key r][d = 32 db + (e, h)]: registers 4 g .. 4 g + 3 are d = 32 db + 8 g + 4 h ..
  AACLIP_DEV void store_dkv(float* __restrict__ dqkv, int b, int L, int head, int key0, const f32x16 (&dk)[2],
                            const f32x16 (&dv)[2]) const {
    const int kj = key0 + r;
    if (kj < L) {
      float* out = dqkv + ((long)b * L + kj) * (3L * D) + head * 64;
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
};

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
  AttnBwdBf16x3::Args pl;
  for (int i = 0; i < 8; ++i) pl.p[i] = planes + i * plane;
  const long n = (long)B * L * H * 32;
  hipLaunchKernelGGL(attn3_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, qkv, dctx, planes, n, L, H);
  const dim3 g((L + 127) / 128, H, B);
  hipLaunchKernelGGL(attn_bwd_stats_kernel<AttnBwdBf16x3>, g, dim3(256), 0, s, pl, stats, L, H, causal);
  hipLaunchKernelGGL(attn_bwd_dkv_kernel<AttnBwdBf16x3>, g, dim3(256), 0, s, pl, stats, dqkv, L, H, causal);
  hipLaunchKernelGGL(attn_bwd_dq_kernel<AttnBwdBf16x3>, g, dim3(256), 0, s, pl, stats, dqkv, L, H, causal, dq_scale);
}

}  // namespace aaclip

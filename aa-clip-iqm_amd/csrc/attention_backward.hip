// Attention backward for any sequence length in fp32: the policy of attention_backward_passes.h (the formulas, the three
// passes and the operand maps are there) with all five products on v_mfma_f32_32x32x2_f32, an exact fmaf chain: a score
// is summed over d = 0, 1, .., 63 in that order in both later passes, so they form p from the same bits.
// Operand maps of the 32x32x2 MFMA (lane = 32 h + r): A[row r][k = h], B[k = h][col r].
// LDS: a tile is 32 rows x 64 floats at a row stride of 65 floats, which serves both operand roles without a second
// copy -- as the A operand of a score product (row r, column 2 i + h: banks r + 2 i + h) and as the transposed operand
// of a gradient product (row (i, h), column r: banks r + const).  The loops are bound by the matrix pipe (64 to 128
// MFMAs of 64 cycles per tile and wave against as many 4-byte LDS reads), so the wider reads of a de-interleaved second
// copy would buy nothing.  Two tiles per stage, two stages, plus 3 x 32 statistics in the dk / dv pass: 34 048 bytes.
#include "attention_backward_passes.h"
#include "kernels.h"

namespace aaclip {

struct AttnBwdF32 {
  static constexpr int TLD = 65;            // tile row stride in floats
  static constexpr int TILE = 32 * TLD;     // floats of a tile
  static constexpr int STAGE_BYTES = 2 * TILE * 4;
  static constexpr int ENTRY_NOPS[3] = {0, 0, 0};
  struct Args {
    const float *qkv, *dctx;
  };
  const float *base, *dbase;   // q of this (image, head) in qkv (k, v follow at D, 2 D) and its d_ctx
  long ld;
  int D, r, h;
  AACLIP_DEV AttnBwdF32(const Args& a, int b, int head, int L, int H, int lane)
      : base(a.qkv + (long)b * L * (3L * H * 64) + head * 64), dbase(a.dctx + (long)b * L * (H * 64) + head * 64),
        ld(3L * H * 64), D(H * 64), r(lane & 31), h(lane >> 5) {}
  AACLIP_DEV const float* src(int f) const { return f == ATT_DCTX ? dbase : base + f * D; }
  AACLIP_DEV long stride(int f) const { return f == ATT_DCTX ? D : ld; }

  // row `row` of a field: this lane's 32 values d = 2 i + h, the B operand of a score MFMA
  struct Own {
    float reg[32];
    AACLIP_DEV void load(const AttnBwdF32& v, int f, int row) {
      const float* __restrict__ src = v.src(f);
      const long ld = v.stride(f);
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const f32x4 x = *(const f32x4*)(src + (long)row * ld + 4 * c);
        reg[2 * c] = v.h ? x[1] : x[0];
        reg[2 * c + 1] = v.h ? x[3] : x[2];
      }
    }
  };

  struct Tile {
    f32x4 ra[2], rb[2];
    AACLIP_DEV void load(const AttnBwdF32& v, int fa, int fb, int t0, int L, int tid) {
      const float* __restrict__ a = v.src(fa);
      const float* __restrict__ b = v.src(fb);
      const long lda = v.stride(fa), ldb = v.stride(fb);
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
    AACLIP_DEV void store(char* stage, int tid) const {
      float *As = (float*)stage, *Bs = As + TILE;
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
  AACLIP_DEV f32x16 score(const char* stage, int which, const Own& own) const {
    const float* T = (const float*)stage + which * TILE;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(T[r * TLD + 2 * i + h], own.reg[i], acc, 0, 0, 0);
    return acc;
  }

  AACLIP_DEV void grad_dkv(const char* stage, const f32x16& p, const f32x16& ds, f32x16 (&dk)[2], f32x16 (&dv)[2]) const {
    const float *Qs = (const float*)stage, *Ds = Qs + TILE;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = mfma_row(i, h) * TLD + r;
      dv[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[i], Ds[o], dv[0], 0, 0, 0);
      dv[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[i], Ds[o + 32], dv[1], 0, 0, 0);
      dk[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[i], Qs[o], dk[0], 0, 0, 0);
      dk[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[i], Qs[o + 32], dk[1], 0, 0, 0);
    }
  }

  AACLIP_DEV void grad_dq(const char* stage, const f32x16& ds, f32x16 (&dq)[2]) const {
    const float* Ks = (const float*)stage;
#pragma unroll
    for (int i = 0; i < 16; ++i) {   // dq^T[d][query] += K^T[d][key (i, h)] ds[key][query]
      const int o = mfma_row(i, h) * TLD + r;
      dq[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[o], ds[i], dq[0], 0, 0, 0);
      dq[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[o + 32], ds[i], dq[1], 0, 0, 0);
    }
  }

  // dk[key (e, h)][d = 32 db + r]
  AACLIP_DEV void store_dkv(float* __restrict__ dqkv, int b, int L, int head, int key0, const f32x16 (&dk)[2],
                            const f32x16 (&dv)[2]) const {
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
};

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
  const AttnBwdF32::Args a{qkv, dctx};
  hipLaunchKernelGGL(attn_bwd_stats_kernel<AttnBwdF32>, g, dim3(256), 0, s, a, stats, L, H, causal);
  hipLaunchKernelGGL(attn_bwd_dkv_kernel<AttnBwdF32>, g, dim3(256), 0, s, a, stats, dqkv, L, H, causal);
  hipLaunchKernelGGL(attn_bwd_dq_kernel<AttnBwdF32>, g, dim3(256), 0, s, a, stats, dqkv, L, H, causal, dq_scale);
}

}  // namespace aaclip

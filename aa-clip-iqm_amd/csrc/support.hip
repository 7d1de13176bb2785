// Few-shot support bank: for every query row the largest cosine to a bank row and the lowest bank row that attains it.
//   best_cos[m] = max_j <q_m, bank_j>,  best_idx[m] = min { j : <q_m, bank_j> = best_cos[m] }
// The M x N cosine matrix never reaches HBM: a workgroup keeps a 128 x 128 tile of it in its MFMA accumulators, folds
// the tile into one running candidate per query row and lane, and walks on to the next bank tile of its chunk.  At the
// end of the chunk the candidates of a row are merged -- over the lanes that share the row, then over the workgroups
// that share it -- as 64-bit words (csrc/support_pack.h) under an INTEGER maximum: any order gives the same word, no
// float atomics, two calls give the same bytes.
//   support_fp16_kernel   both operands rounded to fp16 (after an exact scale by 2^4), v_mfma_f32_16x16x32_f16, fp32
//                         accumulator; the query rows are converted while they are staged, the bank once by
//                         support_bank_rows_kernel
//   support_fp32_kernel   exact fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per cosine): the yardstick and
//                         the form of precision="fp32" models
//   support_decode_kernel the words -> best_cos / best_idx
//   support_dist_kernel, support_add_kernel   the map stage around launch_blur_upsample: d = 1 - cos before it,
//                         out = base + weight * out after it
// The grid is (row tiles, bank chunks): at one image M = 1369 is 11 row tiles, so the chip is filled from the bank side
// (support_plan).  Padding: query rows >= M and bank rows >= N are staged as zeros; a padded bank row is never compared
// (its cosine 0 would beat an all-negative row) and a padded query row is never written.
#include "common.h"
#include "kernels.h"
#include "mma16.h"
#include "support_pack.h"

namespace aaclip {

namespace {

constexpr int T = SUPPORT_TILE;

// the running candidate of one query row in one lane: bank rows arrive in ascending order, so "strictly greater"
// keeps the lowest row among equals (and -0.0 == +0.0 in the comparison, as in the packed key)
struct Cand {
  float best;
  int row;
};
AACLIP_DEV void cand_take(Cand& c, float v, long j, long n_end) {
  if (j < n_end && v > c.best) {
    c.best = v;
    c.row = (int)j;
  }
}
AACLIP_DEV unsigned long long cand_word(const Cand& c) { return c.row >= 0 ? support_pack(c.best, (uint32_t)c.row) : 0ull; }
AACLIP_DEV unsigned long long shfl_xor_u64(unsigned long long v, int mask) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, mask, 64);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), mask, 64);
  return ((unsigned long long)hi << 32) | lo;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ fp16 form
// LDS: the query tile and the bank tile of one K step of 64, rows of 128 bytes in mma16.h's swizzled addressing.  The
// next K step's global loads are issued before the MFMAs of the current one (register prefetch, one LDS buffer).
// A wave owns 64 bank rows x 64 query rows = 4 x 4 MFMA tiles; the BANK is the MFMA's A side, so an accumulator
// register holds bank row 4 * (lane >> 4) + r of query row lane & 15: the reduction over the bank runs inside a lane
// first.
__global__ __launch_bounds__(256) void support_fp16_kernel(const float* __restrict__ q, long M, const f16* __restrict__ bank,
                                                           long N, int E, int tiles_per_chunk,
                                                           unsigned long long* __restrict__ words) {
  __shared__ __attribute__((aligned(16))) unsigned char Qs[T * 128];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[T * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int wb = wave >> 1, wq = wave & 1;
  const long m0 = (long)blockIdx.x * T;
  const long bank_tiles = (N + T - 1) / T;
  const long t_begin = (long)blockIdx.y * tiles_per_chunk;
  long t_end = t_begin + tiles_per_chunk;
  if (t_end > bank_tiles) t_end = bank_tiles;

  // staging: 1024 sixteen-byte LDS slots per tile, four per thread
  int srow[4], schunk[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int f = tid + 256 * j;
    srow[j] = f >> 3;
    schunk[j] = f & 7;
  }
  int offB[2][4], offQ[2][4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      offB[ks][i] = tile_off_id(wb * 64 + i * 16 + c16, 4 * ks + g);
      offQ[ks][i] = tile_off_id(wq * 64 + i * 16 + c16, 4 * ks + g);
    }

  Cand cand[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) cand[i].best = -__builtin_inff(), cand[i].row = -1;

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const u32x4 zero16 = {0u, 0u, 0u, 0u};
  const int ksteps = E >> 6, ktail = E & 63;   // E % 32 == 0: a last half step of 32 is staged with zeros behind it
  const int steps = ksteps + (ktail ? 1 : 0);

  for (long t = t_begin; t < t_end; ++t) {
    const long n0 = t * T;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = zero4;

    f32x4 rq[4][2];
    u32x4 rb[4];
    auto fetch = [&](int step) {
      const int k0 = step << 6;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + schunk[j] * 8;
        const long qr = m0 + srow[j], br = n0 + srow[j];
        const bool kin = k < E;
        const bool qok = kin && qr < M, bok = kin && br < N;
        const float* qp = q + qr * (long)E + k;
        rq[j][0] = qok ? *(const f32x4*)qp : zero4;
        rq[j][1] = qok ? *(const f32x4*)(qp + 4) : zero4;
        rb[j] = bok ? *(const u32x4*)(bank + br * (long)E + k) : zero16;
      }
    };
    fetch(0);
    for (int step = 0; step < steps; ++step) {
      __syncthreads();   // the previous step's fragment reads are done
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f16x8 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          h[e] = (f16)(rq[j][0][e] * SUPPORT_OPERAND_SCALE);
          h[4 + e] = (f16)(rq[j][1][e] * SUPPORT_OPERAND_SCALE);
        }
        const int off = tile_off_id(srow[j], schunk[j]);
        *(f16x8*)(Qs + off) = h;
        *(u32x4*)(Bs + off) = rb[j];
      }
      __syncthreads();
      if (step + 1 < steps) fetch(step + 1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f16x8 fb[4], fq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fb[i] = *(const f16x8*)(Bs + offB[ks][i]);
          fq[i] = *(const f16x8*)(Qs + offQ[ks][i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = Mma16<f16>::mma(fb[i], fq[j], acc[i][j]);
      }
    }
    // fold the tile: bank rows in ascending order within the lane
    const long jb = n0 + wb * 64 + 4 * g;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) cand_take(cand[j], acc[i][j][r] * SUPPORT_ACC_SCALE, jb + i * 16 + r, N);
  }

#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned long long w = cand_word(cand[j]);
    w = support_merge(w, shfl_xor_u64(w, 16));
    w = support_merge(w, shfl_xor_u64(w, 32));
    const long m = m0 + wq * 64 + j * 16 + c16;
    if (g == 0 && m < M && w != 0ull) atomicMax(words + m, w);
  }
}

// ------------------------------------------------------------------------------------------------ fp32 form
// K steps of 16; both tiles as [row][k] with a row stride of 17 floats (the 32 rows of a fragment read fall into 32
// banks).  A wave owns 64 x 64 = 2 x 2 tiles of 32 x 32; the bank is the A side again: register e of a lane is bank row
// (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) of query row lane & 31, ascending in e.
__global__ __launch_bounds__(256) void support_fp32_kernel(const float* __restrict__ q, long M, const float* __restrict__ bank,
                                                           long N, int E, int tiles_per_chunk,
                                                           unsigned long long* __restrict__ words) {
  constexpr int LD = 17;
  __shared__ float Qs[T * LD];
  __shared__ float Bs[T * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  const int wb = wave >> 1, wq = wave & 1;
  const long m0 = (long)blockIdx.x * T;
  const long bank_tiles = (N + T - 1) / T;
  const long t_begin = (long)blockIdx.y * tiles_per_chunk;
  long t_end = t_begin + tiles_per_chunk;
  if (t_end > bank_tiles) t_end = bank_tiles;

  int srow[2], scol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = tid + 256 * j;
    srow[j] = f >> 2;
    scol[j] = (f & 3) * 4;
  }
  Cand cand[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) cand[i].best = -__builtin_inff(), cand[i].row = -1;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  for (long t = t_begin; t < t_end; ++t) {
    const long n0 = t * T;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    for (int k0 = 0; k0 < E; k0 += 16) {
      f32x4 rq[2], rb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long qr = m0 + srow[j], br = n0 + srow[j];
        rq[j] = qr < M ? *(const f32x4*)(q + qr * (long)E + k0 + scol[j]) : zero4;
        rb[j] = br < N ? *(const f32x4*)(bank + br * (long)E + k0 + scol[j]) : zero4;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          Qs[srow[j] * LD + scol[j] + e] = rq[j][e];
          Bs[srow[j] * LD + scol[j] + e] = rb[j][e];
        }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const int k = 2 * ks + h;
        float b[2], a[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          b[i] = Bs[(wb * 64 + 32 * i + r32) * LD + k];
          a[i] = Qs[(wq * 64 + 32 * i + r32) * LD + k];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[i], a[j], acc[i][j], 0, 0, 0);
      }
    }
    const long jb = n0 + wb * 64 + 4 * h;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int j = 0; j < 2; ++j) cand_take(cand[j], acc[i][j][e], jb + i * 32 + (e & 3) + 8 * (e >> 2), N);
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    unsigned long long w = cand_word(cand[j]);
    w = support_merge(w, shfl_xor_u64(w, 32));
    const long m = m0 + wq * 64 + j * 32 + r32;
    if (h == 0 && m < M && w != 0ull) atomicMax(words + m, w);
  }
}

__global__ __launch_bounds__(256) void support_decode_kernel(const unsigned long long* __restrict__ words, long M,
                                                             float* __restrict__ best_cos, int* __restrict__ best_idx) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const unsigned long long w = words[m];
  best_cos[m] = support_word_cos(w);
  if (best_idx) best_idx[m] = (int)support_word_row(w);
}

// fp32 rows -> the bank of a form: fp16(v * 2^4) or a copy; n4 = N * E / 4
__global__ __launch_bounds__(256) void support_bank_rows_kernel(const float* __restrict__ rows, long n4, int form,
                                                                void* __restrict__ bank) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4 v = *(const f32x4*)(rows + i * 4);
  if (form == SUPPORT_FP16) {
    f16x4 hv;
#pragma unroll
    for (int e = 0; e < 4; ++e) hv[e] = (f16)(v[e] * SUPPORT_OPERAND_SCALE);
    *(f16x4*)((f16*)bank + i * 4) = hv;
  } else {
    *(f32x4*)((float*)bank + i * 4) = v;
  }
}

__global__ __launch_bounds__(256) void support_dist_kernel(const float* __restrict__ cosine, float* __restrict__ d, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) d[i] = 1.0f - cosine[i];
}

__global__ __launch_bounds__(256) void support_add_kernel(const float* __restrict__ base, float weight,
                                                          float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = weight * out[i];
  out[i] = base ? base[i] + v : v;
}

size_t support_ws_bytes(long M) { return support_layout(M).bytes; }

void launch_support_nearest(const float* q, long M, const void* bank, long N, int E, int form, float* best_cos,
                            int* best_idx, void* ws, hipStream_t s) {
  const SupportPlan p = support_plan(M, N);
  unsigned long long* words = (unsigned long long*)((char*)ws + support_layout(M).words);
  (void)hipMemsetAsync(words, 0, (size_t)M * 8, s);
  const dim3 grid((unsigned)p.row_tiles, (unsigned)p.chunks);
  if (form == SUPPORT_FP16)
    hipLaunchKernelGGL(support_fp16_kernel, grid, dim3(256), 0, s, q, M, (const f16*)bank, N, E, (int)p.tiles_per_chunk, words);
  else
    hipLaunchKernelGGL(support_fp32_kernel, grid, dim3(256), 0, s, q, M, (const float*)bank, N, E, (int)p.tiles_per_chunk,
                       words);
  hipLaunchKernelGGL(support_decode_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, words, M, best_cos, best_idx);
}

void launch_support_bank_rows(const float* rows, long N, int E, int form, void* bank, hipStream_t s) {
  const long n4 = N * (long)E / 4;
  hipLaunchKernelGGL(support_bank_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, rows, n4, form, bank);
}

void launch_support_dist(const float* cosine, float* d, long n, hipStream_t s) {
  hipLaunchKernelGGL(support_dist_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cosine, d, n);
}

void launch_support_add(const float* base, float weight, float* out, long n, hipStream_t s) {
  hipLaunchKernelGGL(support_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, base, weight, out, n);
}

}  // namespace aaclip

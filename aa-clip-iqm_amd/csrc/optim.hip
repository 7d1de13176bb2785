// Multi-tensor Adam / AdamW step and the gradient norm that clips it (aaclip_optim_grad_norm, aaclip_optim_adam_step).
//
// One launch serves many tensors: its table (OptimTable, under 4 KB) travels BY VALUE in the kernel arguments, so a
// step copies nothing to the device, allocates nothing and waits for nothing.  The table holds the p / g / m / v
// pointers, element counts and group indices of up to OPTIM_TABLE_TENSORS tensors and one (slot, chunk) word per
// workgroup; optim_pack.h cuts the tensor list into as many tables as it needs.
//
//   grad norm  every workgroup sums g^2 over its chunk in fp64, in an order fixed by the thread count alone, and stores
//              the sum in the workspace slot of that chunk (slot = index of the chunk in the whole list).  No atomics.
//              One workgroup then adds the slots in fp64, again in a fixed order, and writes
//              {total_norm, clip_coef = min(1, max_norm / (total_norm + 1e-6))} (torch's clip_grad_norm_ formula, in
//              fp32; a NaN norm gives a NaN coefficient).
//   adam step  per element, fp32, every operation rounded on its own (the library is built with -ffp-contract=off):
//                g' = g * coef (+ wd * p when the decay is coupled);   p' = p * (1 - lr * wd) when it is decoupled
//                m  = beta1 * m + (1 - beta1) * g';   v = beta2 * v + (1 - beta2) * g' * g'
//                p  = p' - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
//              coef is read from the device record, or is 1.  The gradients in memory are left as they are.
//
// Both kernels give thread t of a chunk the quads t, t + OPTIM_THREADS, ... of that chunk and its first len % 4 threads
// one tail element each.  A quad is one 16-byte load / store per array where every pointer the kernel uses for that
// tensor is 16-byte aligned, four 4-byte ones otherwise: the arithmetic and its order do not depend on the alignment.
#include <string.h>

#include "common.h"
#include "kernels.h"

namespace aaclip {

constexpr int OPTIM_THREADS = 512;
constexpr int OPTIM_ADAM_DEPTH = 2;   // quads per array a thread has in flight
constexpr int OPTIM_NORM_DEPTH = 4;

struct OptimTable {
  float* p[OPTIM_TABLE_TENSORS];
  const float* g[OPTIM_TABLE_TENSORS];
  float* m[OPTIM_TABLE_TENSORS];
  float* v[OPTIM_TABLE_TENSORS];
  long n[OPTIM_TABLE_TENSORS];
  uint8_t group[OPTIM_TABLE_TENSORS];
  int blocks;
  uint32_t block[OPTIM_TABLE_BLOCKS];
};
struct OptimGroups {
  OptimGroupScalars g[AACLIP_OPTIM_MAX_GROUPS];
};
static_assert(sizeof(OptimTable) + sizeof(OptimGroups) + 64 <= 4096, "the kernel arguments stay under 4 KB");

struct OptimRecord {   // include/aaclip.h aaclip_optim_record
  float total_norm, clip_coef;
};

template <bool VEC> AACLIP_DEV float4 load_quad(const float* a) {
  if (VEC) return *reinterpret_cast<const float4*>(a);
  return make_float4(a[0], a[1], a[2], a[3]);
}
template <bool VEC> AACLIP_DEV void store_quad(float* a, float4 x) {
  if (VEC) {
    *reinterpret_cast<float4*>(a) = x;
  } else {
    a[0] = x.x, a[1] = x.y, a[2] = x.z, a[3] = x.w;
  }
}

// ------------------------------------------------------------------------------------------------- gradient norm
AACLIP_DEV double add_squares(double acc, float4 x) {
  acc += (double)x.x * (double)x.x;
  acc += (double)x.y * (double)x.y;
  acc += (double)x.z * (double)x.z;
  acc += (double)x.w * (double)x.w;
  return acc;
}

template <bool VEC> AACLIP_DEV double sumsq_chunk(const float* __restrict__ g, long len, int t) {
  const long quads = len >> 2;
  double acc = 0.0;
  long q = t;
  // OPTIM_NORM_DEPTH loads in flight per thread, then their squares in quad order: the order of the sum is that of the
  // plain loop below, whatever the depth
  for (; q + (OPTIM_NORM_DEPTH - 1) * OPTIM_THREADS < quads; q += OPTIM_NORM_DEPTH * OPTIM_THREADS) {
    float4 x[OPTIM_NORM_DEPTH];
#pragma unroll
    for (int u = 0; u < OPTIM_NORM_DEPTH; ++u) x[u] = load_quad<VEC>(g + 4 * (q + u * OPTIM_THREADS));
    __builtin_amdgcn_sched_barrier(0);   // the compiler otherwise sinks every load to its use and waits for each
#pragma unroll
    for (int u = 0; u < OPTIM_NORM_DEPTH; ++u) acc = add_squares(acc, x[u]);
  }
  for (; q < quads; q += OPTIM_THREADS) acc = add_squares(acc, load_quad<VEC>(g + 4 * q));
  const long tail = 4 * quads + t;
  if (tail < len) acc += (double)g[tail] * (double)g[tail];
  return acc;
}

// the workgroup's sum in thread 0, by a tree whose shape depends on OPTIM_THREADS alone
AACLIP_DEV double block_sum(double acc, double* s_acc, int t) {
  s_acc[t] = acc;
  __syncthreads();
  for (int o = OPTIM_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) s_acc[t] += s_acc[t + o];
    __syncthreads();
  }
  return s_acc[0];
}

__global__ __launch_bounds__(OPTIM_THREADS) void optim_sumsq_kernel(const OptimTable tab, double* __restrict__ slots) {
  __shared__ double s_acc[OPTIM_THREADS];
  const uint32_t word = tab.block[blockIdx.x];
  const int slot = (int)(word >> OPTIM_SLOT_SHIFT), t = threadIdx.x;
  const long start = (long)(word & OPTIM_CHUNK_MASK) * OPTIM_CHUNK;
  const long left = tab.n[slot] - start;
  const long len = left < OPTIM_CHUNK ? left : OPTIM_CHUNK;
  const float* g = tab.g[slot] + start;
  const double acc = ((uintptr_t)g & 15) == 0 ? sumsq_chunk<true>(g, len, t) : sumsq_chunk<false>(g, len, t);
  const double sum = block_sum(acc, s_acc, t);
  if (t == 0) slots[blockIdx.x] = sum;
}

__global__ __launch_bounds__(OPTIM_THREADS) void optim_norm_finish_kernel(const double* __restrict__ slots, long count,
                                                                          float max_norm, OptimRecord* __restrict__ rec) {
  __shared__ double s_acc[OPTIM_THREADS];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (long j = t; j < count; j += OPTIM_THREADS) acc += slots[j];
  const double sum = block_sum(acc, s_acc, t);
  if (t == 0) {
    const float norm = (float)sqrt(sum);
    const float coef = __fdiv_rn(max_norm, norm + 1e-6f);
    rec->total_norm = norm;
    rec->clip_coef = coef > 1.0f ? 1.0f : coef;   // a NaN stays a NaN
  }
}

size_t optim_grad_norm_ws_bytes(long chunks) { return (size_t)(chunks > 0 ? chunks : 1) * sizeof(double); }

// ----------------------------------------------------------------------------------------------------- adam step
AACLIP_DEV void adam_element(float& p, float g, float& m, float& v, float coef, const OptimGroupScalars& h) {
  g = g * coef;
  if (h.coupled) g = g + h.weight_decay * p;
  const float p0 = p * h.decay;   // decay is exactly 1 unless the weight decay is decoupled
  m = h.beta1 * m + h.one_minus_beta1 * g;
  v = h.beta2 * v + h.one_minus_beta2 * g * g;
  const float denom = __fdiv_rn(__fsqrt_rn(v), h.sqrt_bc2) + h.eps;
  p = p0 - h.step_size * __fdiv_rn(m, denom);
}

AACLIP_DEV void adam_quad(float4& p, const float4& g, float4& m, float4& v, float coef, const OptimGroupScalars& h) {
  adam_element(p.x, g.x, m.x, v.x, coef, h);
  adam_element(p.y, g.y, m.y, v.y, coef, h);
  adam_element(p.z, g.z, m.z, v.z, coef, h);
  adam_element(p.w, g.w, m.w, v.w, coef, h);
}

template <bool VEC>
AACLIP_DEV void adam_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                           float* __restrict__ v, long len, int t, float coef, const OptimGroupScalars& h) {
  const long quads = len >> 2;
  long q = t;
  // 4 * OPTIM_ADAM_DEPTH loads in flight per thread before the first use
  for (; q + (OPTIM_ADAM_DEPTH - 1) * OPTIM_THREADS < quads; q += OPTIM_ADAM_DEPTH * OPTIM_THREADS) {
    float4 xp[OPTIM_ADAM_DEPTH], xg[OPTIM_ADAM_DEPTH], xm[OPTIM_ADAM_DEPTH], xv[OPTIM_ADAM_DEPTH];
#pragma unroll
    for (int u = 0; u < OPTIM_ADAM_DEPTH; ++u) {
      const long e = 4 * (q + u * OPTIM_THREADS);
      xp[u] = load_quad<VEC>(p + e), xg[u] = load_quad<VEC>(g + e);
      xm[u] = load_quad<VEC>(m + e), xv[u] = load_quad<VEC>(v + e);
    }
    __builtin_amdgcn_sched_barrier(0);   // the compiler otherwise sinks every load to its use and waits for each
#pragma unroll
    for (int u = 0; u < OPTIM_ADAM_DEPTH; ++u) {
      const long e = 4 * (q + u * OPTIM_THREADS);
      adam_quad(xp[u], xg[u], xm[u], xv[u], coef, h);
      store_quad<VEC>(p + e, xp[u]);
      store_quad<VEC>(m + e, xm[u]);
      store_quad<VEC>(v + e, xv[u]);
    }
  }
  for (; q < quads; q += OPTIM_THREADS) {
    float4 xp = load_quad<VEC>(p + 4 * q), xm = load_quad<VEC>(m + 4 * q), xv = load_quad<VEC>(v + 4 * q);
    adam_quad(xp, load_quad<VEC>(g + 4 * q), xm, xv, coef, h);
    store_quad<VEC>(p + 4 * q, xp);
    store_quad<VEC>(m + 4 * q, xm);
    store_quad<VEC>(v + 4 * q, xv);
  }
  const long tail = 4 * quads + t;
  if (tail < len) {
    float xp = p[tail], xm = m[tail], xv = v[tail];
    adam_element(xp, g[tail], xm, xv, coef, h);
    p[tail] = xp, m[tail] = xm, v[tail] = xv;
  }
}

__global__ __launch_bounds__(OPTIM_THREADS) void optim_adam_kernel(const OptimTable tab, const OptimGroups groups,
                                                                   const OptimRecord* __restrict__ rec) {
  const uint32_t word = tab.block[blockIdx.x];
  const int slot = (int)(word >> OPTIM_SLOT_SHIFT), t = threadIdx.x;
  const long start = (long)(word & OPTIM_CHUNK_MASK) * OPTIM_CHUNK;
  const long left = tab.n[slot] - start;
  const long len = left < OPTIM_CHUNK ? left : OPTIM_CHUNK;
  float* p = tab.p[slot] + start;
  const float* g = tab.g[slot] + start;
  float* m = tab.m[slot] + start;
  float* v = tab.v[slot] + start;
  const OptimGroupScalars h = groups.g[tab.group[slot]];
  const float coef = rec ? rec->clip_coef : 1.0f;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0)
    adam_chunk<true>(p, g, m, v, len, t, coef, h);
  else
    adam_chunk<false>(p, g, m, v, len, t, coef, h);
}

// ------------------------------------------------------------------------------------------------------ launchers
// the next table of the list; false when the list is exhausted
static bool next_table(const aaclip_optim_tensor* items, const long* counts, long tensors, OptimPackCursor& cur,
                       OptimPackLaunch& launch, OptimTable& tab) {
  if (!optim_pack_next(counts, tensors, cur, launch)) return false;
  memset(&tab, 0, sizeof(tab));
  for (int s = 0; s < launch.tensors; ++s) {
    const aaclip_optim_tensor& it = items[launch.tensor_index[s]];
    tab.p[s] = (float*)it.p, tab.g[s] = (const float*)it.g, tab.m[s] = (float*)it.m, tab.v[s] = (float*)it.v;
    tab.n[s] = it.n, tab.group[s] = (uint8_t)it.group;
  }
  tab.blocks = launch.blocks;
  memcpy(tab.block, launch.block, sizeof(uint32_t) * launch.blocks);
  return true;
}

void launch_optim_grad_norm(const aaclip_optim_tensor* items, const long* counts, long tensors, float max_norm,
                            void* record, void* ws, hipStream_t s) {
  OptimPackCursor cur = {0, 0};
  OptimPackLaunch launch;
  OptimTable tab;
  double* slots = (double*)ws;
  long done = 0;
  while (next_table(items, counts, tensors, cur, launch, tab)) {
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)tab.blocks), dim3(OPTIM_THREADS), 0, s, tab, slots + done);
    done += tab.blocks;
  }
  hipLaunchKernelGGL(optim_norm_finish_kernel, dim3(1), dim3(OPTIM_THREADS), 0, s, (const double*)slots, done, max_norm,
                     (OptimRecord*)record);
}

void launch_optim_adam_step(const aaclip_optim_tensor* items, const long* counts, long tensors,
                            const OptimGroupScalars* groups, int n_groups, const void* record, hipStream_t s) {
  OptimGroups gr;
  memset(&gr, 0, sizeof(gr));
  for (int i = 0; i < n_groups; ++i) gr.g[i] = groups[i];
  OptimPackCursor cur = {0, 0};
  OptimPackLaunch launch;
  OptimTable tab;
  while (next_table(items, counts, tensors, cur, launch, tab))
    hipLaunchKernelGGL(optim_adam_kernel, dim3((unsigned)tab.blocks), dim3(OPTIM_THREADS), 0, s, tab, gr,
                       (const OptimRecord*)record);
}

}  // namespace aaclip

// The prefix scan over sorted keys that the curve / F1-max marks (metrics.hip), the PRO curve (regions.hip) and the
// region table (region_table.hip) run, and the folds of the group, range and threshold kernels, once.
//
// An ITEM is any type I with `+` whose I() is its zero: u64 words, or {u64 word, double w}.  Three levels:
//   tile_sum_body    grid = tiles: the sum of every tile of TILE_THREADS x ITEMS consecutive items
//   tile_scan_body   one workgroup: the tile sums <- their exclusive prefix; returns the sum of all
//   tile_walk_body   grid = tiles: calls mark(i, item, prefix before i) for every i of the tile, in index order per thread
// Every sum has the accumulated value as its left operand and runs in an order fixed by n alone: a thread's own items in
// index order, a Hillis-Steele scan over the workgroup's threads, the tile prefix in front.  Callers with a double in the
// item rely on exactly that order for equal bits from call to call; integers do not care.
// Each body declares its own LDS and is meant to be the whole body of a thin __global__ wrapper of TILE_THREADS threads.
#pragma once
#include "common.h"
#include "metrics_records.h"

namespace aaclip {

static constexpr int TILE_THREADS = METRICS_THREADS;

// Exclusive prefix of `mine` over the workgroup's threads, in thread order; *all, where given, <- the sum over the
// workgroup.  The exclusive value is the inclusive value of thread t - 1, never inclusive - mine: for a double those
// are not the same bits.  lds: TILE_THREADS items, free again when the call returns.
template <typename I>
AACLIP_DEV I block_exclusive_scan(I mine, I* lds, I* all = nullptr) {
  const int t = threadIdx.x;
  lds[t] = mine;
  __syncthreads();
  for (int o = 1; o < TILE_THREADS; o <<= 1) {
    I add = I();
    if (t >= o) add = lds[t - o];
    __syncthreads();
    if (t >= o) lds[t] = add + lds[t];   // left operand = the earlier threads
    __syncthreads();
  }
  if (all) *all = lds[TILE_THREADS - 1];
  I ex = I();
  if (t > 0) ex = lds[t - 1];
  __syncthreads();
  return ex;
}

// item(first) + ... + item(first + ITEMS - 1) in index order, without the indices from n on
template <int ITEMS, typename I, typename F>
AACLIP_DEV I thread_sum(long first, long n, F item) {
  I acc = I();
#pragma unroll 4
  for (int j = 0; j < ITEMS; ++j)
    if (first + j < n) acc = acc + item(first + j);
  return acc;
}

template <int ITEMS>
AACLIP_DEV long tile_thread_first() {
  return (long)blockIdx.x * (TILE_THREADS * ITEMS) + (long)threadIdx.x * ITEMS;
}

template <int ITEMS, typename I, typename F>
AACLIP_DEV void tile_sum_body(long n, I* __restrict__ tile_sum, F item) {
  __shared__ I lds[TILE_THREADS];
  I all;
  block_exclusive_scan(thread_sum<ITEMS, I>(tile_thread_first<ITEMS>(), n, item), lds, &all);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// a thread takes `per` consecutive tiles in index order, then the scan over the threads
template <typename I>
AACLIP_DEV I tile_scan_body(I* __restrict__ tile_sum, long tiles) {
  __shared__ I lds[TILE_THREADS];
  const int t = threadIdx.x;
  const long per = (tiles + TILE_THREADS - 1) / TILE_THREADS;
  const long j0 = t * per < tiles ? t * per : tiles, j1 = j0 + per < tiles ? j0 + per : tiles;
  I acc = I();
  for (long j = j0; j < j1; ++j) acc = acc + tile_sum[j];
  I all;
  I run = block_exclusive_scan(acc, lds, &all);
  for (long j = j0; j < j1; ++j) {
    const I c = tile_sum[j];
    tile_sum[j] = run;
    run = run + c;
  }
  return all;
}

template <int ITEMS, typename I, typename F, typename M>
AACLIP_DEV void tile_walk_body(long n, const I* __restrict__ tile_prefix, F item, M mark) {
  __shared__ I lds[TILE_THREADS];
  const long first = tile_thread_first<ITEMS>();
  I run = tile_prefix[blockIdx.x] + block_exclusive_scan(thread_sum<ITEMS, I>(first, n, item), lds);
#pragma unroll 4
  for (int j = 0; j < ITEMS; ++j) {
    const long i = first + j;
    if (i >= n) break;
    const I it = item(i);
    mark(i, it, run);
    run = run + it;
  }
}

// ---- the folds.  Workgroup b of a group kernel takes the contiguous share [k0, k1) of the G groups, a thread every
// TILE_THREADS-th of them; the threads are folded by block_fold, and one last kernel folds the workgroups' partials in
// index order: an order that depends on G and the grid alone.
struct GroupShare {
  long k0, k1;
};
AACLIP_DEV GroupShare group_share(long G) {
  const long per = (G + gridDim.x - 1) / gridDim.x;
  const long k0 = (long)blockIdx.x * per;
  return GroupShare{k0, k0 + per < G ? k0 + per : G};
}

// The LDS tree: s[t] = op(s[t], s[t + o]) for t < o, o from TILE_THREADS / 2 down.  Returns s[0], the fold over the
// workgroup, to every thread.  s: TILE_THREADS values, not to be written again before a barrier.
template <typename T, typename Op>
AACLIP_DEV T block_fold(T mine, T* s, Op op) {
  const int t = threadIdx.x;
  s[t] = mine;
  __syncthreads();
  for (int o = TILE_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) s[t] = op(s[t], s[t + o]);
    __syncthreads();
  }
  return s[0];
}

}  // namespace aaclip

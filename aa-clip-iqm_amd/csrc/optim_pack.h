// How a list of tensors becomes launches of the multi-tensor optimizer kernels (optim.hip).  Plain host C++, no HIP:
// optim_host_check.cpp runs it under AddressSanitizer + UBSan.
//
// A tensor of n elements is cut into ceil(n / OPTIM_CHUNK) chunks, one workgroup each.  One launch carries up to
// OPTIM_TABLE_TENSORS tensors and up to OPTIM_TABLE_BLOCKS chunks; a tensor with more chunks than a launch has room for
// continues in the next launch, tensors of zero elements take no slot.  Chunks are issued in order, tensor by tensor,
// so the k-th chunk of the whole list is the k-th workgroup counted over the launches: that index is the chunk's
// workspace slot in the gradient norm.
#pragma once
#include <stdint.h>

namespace aaclip {

constexpr long OPTIM_CHUNK = 16384;          // elements per workgroup
constexpr int OPTIM_TABLE_TENSORS = 24;      // tensors per launch
constexpr int OPTIM_TABLE_BLOCKS = 640;      // workgroups per launch
constexpr int OPTIM_SLOT_SHIFT = 27;         // a block word: table slot << 27 | chunk index within the tensor
constexpr uint32_t OPTIM_CHUNK_MASK = (1u << OPTIM_SLOT_SHIFT) - 1;
constexpr long OPTIM_MAX_ELEMS = (long)OPTIM_CHUNK_MASK * OPTIM_CHUNK;   // per tensor: the chunk index fits its field
static_assert(OPTIM_TABLE_TENSORS <= (1 << (32 - OPTIM_SLOT_SHIFT)), "the slot must fit the block word");

inline long optim_chunks(long n) { return n <= 0 ? 0 : (n + OPTIM_CHUNK - 1) / OPTIM_CHUNK; }

// chunks of the whole list (= workspace slots of the gradient norm); counts below 0 or above OPTIM_MAX_ELEMS are the
// caller's to refuse
inline long optim_total_chunks(const long* counts, long tensors) {
  long total = 0;
  for (long i = 0; i < tensors; ++i) total += optim_chunks(counts[i]);
  return total;
}

struct OptimPackLaunch {
  int tensors, blocks;
  long tensor_index[OPTIM_TABLE_TENSORS];    // slot -> index into the caller's list
  uint32_t block[OPTIM_TABLE_BLOCKS];        // workgroup -> slot << OPTIM_SLOT_SHIFT | chunk
};

struct OptimPackCursor {   // where the next launch starts; zero-initialise
  long tensor, chunk;
};

// Fills `out` with the next launch.  false: the list is exhausted and `out` is empty.
inline bool optim_pack_next(const long* counts, long tensors, OptimPackCursor& cur, OptimPackLaunch& out) {
  out.tensors = out.blocks = 0;
  while (cur.tensor < tensors) {
    const long chunks = optim_chunks(counts[cur.tensor]);
    if (cur.chunk >= chunks) {   // done with this tensor (at once where it is empty)
      ++cur.tensor, cur.chunk = 0;
      continue;
    }
    if (out.tensors == OPTIM_TABLE_TENSORS || out.blocks == OPTIM_TABLE_BLOCKS) break;
    const uint32_t slot = (uint32_t)out.tensors++;
    out.tensor_index[slot] = cur.tensor;
    while (cur.chunk < chunks && out.blocks < OPTIM_TABLE_BLOCKS)
      out.block[out.blocks++] = slot << OPTIM_SLOT_SHIFT | (uint32_t)cur.chunk++;
  }
  return out.blocks > 0;
}

}  // namespace aaclip

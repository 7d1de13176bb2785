// Host check of the launch packing of optim.hip (optim_pack.h): the very code that cuts a list of element counts into
// launches and chunks, over adversarial lists.  For every list: every element of every tensor lies in exactly one
// chunk, no table holds more tensors or workgroups than it has room for, every block word names a slot of its own
// launch and a chunk inside its tensor, chunks come in list order (the k-th workgroup over the launches is the k-th
// chunk: the workspace slot of the gradient norm), and the launches add up to optim_total_chunks.
// Built on its own with a host compiler and -fsanitize=address,undefined (tests/test_optim_cpu.py); no GPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "optim_pack.h"

using namespace aaclip;

static int g_failures = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      printf("  FAIL: " __VA_ARGS__);   \
      printf("\n");                     \
      ++g_failures;                     \
    }                                   \
  } while (0)

static void check_list(const char* name, const std::vector<long>& counts) {
  const long tensors = (long)counts.size();
  std::vector<std::vector<uint8_t>> seen(counts.size());
  for (long i = 0; i < tensors; ++i) seen[i].assign((size_t)counts[i], 0);
  OptimPackCursor cur = {0, 0};
  OptimPackLaunch* launch = new OptimPackLaunch;   // on the heap: ASan sees an index past either array
  long launches = 0, blocks = 0, last_tensor = -1, last_chunk = -1;
  const int before = g_failures;
  while (optim_pack_next(counts.data(), tensors, cur, *launch)) {
    ++launches;
    CHECK(launch->tensors >= 1 && launch->tensors <= OPTIM_TABLE_TENSORS, "%d tensors in a launch", launch->tensors);
    CHECK(launch->blocks >= 1 && launch->blocks <= OPTIM_TABLE_BLOCKS, "%d blocks in a launch", launch->blocks);
    if (launch->tensors > OPTIM_TABLE_TENSORS || launch->blocks > OPTIM_TABLE_BLOCKS) break;
    std::vector<int> slot_used(launch->tensors, 0);
    for (int b = 0; b < launch->blocks; ++b) {
      const int slot = (int)(launch->block[b] >> OPTIM_SLOT_SHIFT);
      const long chunk = (long)(launch->block[b] & OPTIM_CHUNK_MASK);
      CHECK(slot < launch->tensors, "block %d names slot %d of %d", b, slot, launch->tensors);
      if (slot >= launch->tensors) continue;
      slot_used[slot] = 1;
      const long t = launch->tensor_index[slot];
      CHECK(t >= 0 && t < tensors, "slot %d names tensor %ld of %ld", slot, t, tensors);
      if (t < 0 || t >= tensors) continue;
      const long start = chunk * OPTIM_CHUNK;
      CHECK(start < counts[t], "chunk %ld starts past the end of tensor %ld (%ld elements)", chunk, t, counts[t]);
      CHECK(t > last_tensor || (t == last_tensor && chunk == last_chunk + 1), "chunk (%ld, %ld) follows (%ld, %ld)", t,
            chunk, last_tensor, last_chunk);
      last_tensor = t, last_chunk = chunk;
      const long end = start + OPTIM_CHUNK < counts[t] ? start + OPTIM_CHUNK : counts[t];
      for (long e = start; e < end; ++e) ++seen[t][e];
      ++blocks;
    }
    for (int s = 0; s < launch->tensors; ++s) CHECK(slot_used[s], "slot %d holds a tensor without a chunk", s);
    if (launches > optim_total_chunks(counts.data(), tensors) + 1) {
      CHECK(false, "the packing does not end");
      break;
    }
  }
  CHECK(launch->tensors == 0 && launch->blocks == 0, "the exhausted call left a table behind");
  CHECK(!optim_pack_next(counts.data(), tensors, cur, *launch), "a call after the end found work");
  delete launch;
  CHECK(blocks == optim_total_chunks(counts.data(), tensors), "%ld blocks, %ld chunks", blocks,
        optim_total_chunks(counts.data(), tensors));
  long uncovered = 0, twice = 0;
  for (long i = 0; i < tensors; ++i)
    for (uint8_t c : seen[i]) uncovered += c == 0, twice += c > 1;
  CHECK(uncovered == 0 && twice == 0, "%ld elements in no chunk, %ld in several", uncovered, twice);
  printf("%-28s %6ld tensors %5ld launches %7ld chunks %s\n", name, tensors, launches, blocks,
         g_failures == before ? "ok" : "FAILED");
}

int main() {
  const long C = OPTIM_CHUNK, T = OPTIM_TABLE_TENSORS, B = OPTIM_TABLE_BLOCKS;
  check_list("empty", {});
  check_list("zeros", std::vector<long>(3 * T + 1, 0));
  check_list("ones", std::vector<long>(5, 1));
  check_list("chunk edges", {C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 1, 0, 2 * C + 5});
  check_list("larger than a launch", {3, (B + 1) * C + 7, 5});
  check_list("exactly a launch", {B * C, 1});
  check_list("two launches and a bit", {2 * B * C + 1});
  check_list("table + 1 tensors", std::vector<long>(T + 1, 2));
  check_list("table tensors", std::vector<long>(T, 1));
  check_list("many tables", std::vector<long>(7 * T + 3, 3));
  {   // zeros between, sizes 0 .. 7 cycling, a full block list reached in the middle of the tensor list
    std::vector<long> v;
    for (long i = 0; i < 3 * T + 1; ++i) v.push_back(i % 8);
    check_list("0..7 cycling", v);
    std::vector<long> w(T - 1, 1);
    w.push_back((B - (T - 1)) * C);      // fills the block list exactly with the last slot
    w.push_back(C + 1);
    check_list("blocks and slots full", w);
    w[T - 1] += 1;                       // one element more: its last chunk opens the next launch
    check_list("blocks full, one over", w);
  }
  {   // a deterministic shuffle of sizes around every edge
    std::vector<long> v;
    uint64_t s = 12345;
    const long edges[] = {0, 1, 3, 4, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5, 37 * C + 11};
    for (int i = 0; i < 500; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      v.push_back(edges[(s >> 33) % (sizeof(edges) / sizeof(edges[0]))]);
    }
    check_list("shuffled edges", v);
  }
  printf(g_failures ? "optim_host_check: %d FAILURES\n" : "optim_host_check: all ok\n", g_failures);
  return g_failures ? 1 : 0;
}

// Host check of the union-find of regions.hip (regions_uf.h): the very find / union / merge code, with plain loads and
// a sequential minimum, over masks read from a file, in forward, reverse and shuffled pixel orders, against a flood
// fill.  Built on its own with a host compiler and -fsanitize=address,undefined (tests/test_pro_cpu.py); no GPU.
//   regions_host_check <file>      file: int32 cases, then per case int32 N, H, W, connectivity and N * H * W bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "regions_uf.h"

struct HostAccess {
  static uint32_t load(const uint32_t* p) { return *(const volatile uint32_t*)p; }
  static uint32_t min(uint32_t* p, uint32_t v) {
    const uint32_t old = *p;
    if (v < old) *p = v;
    return old;
  }
};

static void flood_fill(const std::vector<uint8_t>& mask, int N, int H, int W, int conn, std::vector<uint32_t>& region,
                       std::vector<uint32_t>& area) {
  const long n = (long)N * H * W;
  region.assign(n, 0);
  area.assign(n, 0);
  std::vector<long> stack, members;
  for (long s = 0; s < n; ++s) {
    if (!mask[s] || region[s]) continue;
    stack.assign(1, s);
    members.clear();
    region[s] = (uint32_t)s + 1;
    while (!stack.empty()) {
      const long i = stack.back();
      stack.pop_back();
      members.push_back(i);
      const int x = (int)(i % W), y = (int)((i / W) % H);
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((dy == 0 && dx == 0) || (conn == 4 && dy != 0 && dx != 0)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          const long j = i + (long)dy * W + dx;
          if (mask[j] && !region[j]) {
            region[j] = (uint32_t)s + 1;   // s is the first pixel of its component in row-major order
            stack.push_back(j);
          }
        }
    }
    for (long i : members) area[i] = (uint32_t)members.size();
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: regions_host_check <file>\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int32_t cases = 0;
  if (fread(&cases, 4, 1, f) != 1) return fprintf(stderr, "short file\n"), 2;
  uint64_t rnd = 0x9E3779B97F4A7C15ull;
  long runs = 0;
  for (int c = 0; c < cases; ++c) {
    int32_t head[4];
    if (fread(head, 4, 4, f) != 4) return fprintf(stderr, "short file\n"), 2;
    const int N = head[0], H = head[1], W = head[2], conn = head[3];
    const long n = (long)N * H * W;
    std::vector<uint8_t> mask(n);
    if ((long)fread(mask.data(), 1, n, f) != n) return fprintf(stderr, "short file\n"), 2;
    std::vector<uint32_t> want_region, want_area;
    flood_fill(mask, N, H, W, conn, want_region, want_area);
    std::vector<long> pixels;
    for (long i = 0; i < n; ++i)
      if (mask[i]) pixels.push_back(i);
    for (int order = 0; order < 5; ++order) {
      if (order == 1) std::reverse(pixels.begin(), pixels.end());
      if (order >= 2)
        for (size_t k = pixels.size(); k > 1; --k) {   // Fisher-Yates on a 64-bit LCG
          rnd = rnd * 6364136223846793005ull + 1442695040888963407ull;
          std::swap(pixels[k - 1], pixels[(size_t)((rnd >> 33) % k)]);
        }
      std::vector<uint32_t> parent(n), count(n, 0), region(n, 0);
      for (long i = 0; i < n; ++i) parent[i] = (uint32_t)i;
      for (long i : pixels) aaclip::uf_merge_pixel<HostAccess>(mask.data(), parent.data(), i, H, W, conn);
      for (long i = n - 1; i >= 0; --i) {   // from the far end: the longest walks first
        if (parent[i] > (uint32_t)i) return fprintf(stderr, "case %d: parent[%ld] was raised\n", c, i), 1;
        if (!mask[i]) continue;
        const uint32_t r = aaclip::uf_find_halve<HostAccess>(parent.data(), (uint32_t)i);   // as the flatten kernel
        if (aaclip::uf_find<HostAccess>(parent.data(), (uint32_t)i) != r)
          return fprintf(stderr, "case %d: the two finds disagree at %ld\n", c, i), 1;
        region[i] = r + 1;
        ++count[r];
      }
      for (long i = 0; i < n; ++i) {
        const uint32_t a = region[i] ? count[region[i] - 1] : 0;
        if (region[i] != want_region[i] || a != want_area[i])
          return fprintf(stderr, "case %d (%d x %d x %d, connectivity %d), order %d: pixel %ld region %u area %u, "
                                 "flood fill %u %u\n", c, N, H, W, conn, order, i, region[i], a, want_region[i],
                         want_area[i]), 1;
      }
      ++runs;
    }
  }
  fclose(f);
  printf("ok %d cases %ld runs\n", cases, runs);
  return 0;
}

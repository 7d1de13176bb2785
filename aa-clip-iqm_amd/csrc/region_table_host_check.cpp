// Host check of the region table of region_table.hip (region_table.h): the very row start, key, peak word, decode and
// workspace layout, with the table built sequentially -- the roots counted in pixel order, every pixel folded into its row
// by plain minima / maxima / sums in forward, reverse and shuffled pixel orders -- over cases read from a file, against a
// flood fill that measures every region on its own.  Built with a host compiler and -fsanitize=address,undefined
// (tests/test_defects_cpu.py); no GPU.
//   region_table_host_check <file>
//   file: int32 cases, then per case int32 N, H, W, connectivity, min_area, capacity, has_other, normalise, then
//         N * H * W mask bytes, N * H * W fp32 scores and, with has_other, N * H * W bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "region_table.h"

using aaclip::RegionRow;

struct Truth {   // one region, measured on its own
  RegionRow row;
  std::vector<long> members;
};

static void flood_fill(const std::vector<uint8_t>& mask, int N, int H, int W, int conn, std::vector<uint32_t>& region,
                       std::vector<uint32_t>& area, std::vector<Truth>& truths) {
  const long n = (long)N * H * W, per = (long)H * W;
  region.assign(n, 0);
  area.assign(n, 0);
  std::vector<long> stack;
  uint32_t label = 0;
  for (long s = 0; s < n; ++s) {
    if (s % per == 0) label = 0;
    if (!mask[s] || region[s]) continue;
    Truth t;
    stack.assign(1, s);
    region[s] = (uint32_t)s + 1;
    while (!stack.empty()) {
      const long i = stack.back();
      stack.pop_back();
      t.members.push_back(i);
      const int x = (int)(i % W), y = (int)((i / W) % H);
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((dy == 0 && dx == 0) || (conn == 4 && dy != 0 && dx != 0)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          const long j = i + (long)dy * W + dx;
          if (mask[j] && !region[j]) {
            region[j] = (uint32_t)s + 1;
            stack.push_back(j);
          }
        }
    }
    std::sort(t.members.begin(), t.members.end());
    for (long i : t.members) area[i] = (uint32_t)t.members.size();
    memset(&t.row, 0, sizeof t.row);
    t.row.image = (uint32_t)(s / per), t.row.label = ++label, t.row.first = (uint32_t)(s % per);
    t.row.area = (uint32_t)t.members.size();
    truths.push_back(t);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: region_table_host_check <file>\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int32_t cases = 0;
  if (fread(&cases, 4, 1, f) != 1) return fprintf(stderr, "short file\n"), 2;
  uint64_t rnd = 0x9E3779B97F4A7C15ull;
  long runs = 0;
  for (int c = 0; c < cases; ++c) {
    int32_t head[8];
    if (fread(head, 4, 8, f) != 8) return fprintf(stderr, "short file\n"), 2;
    const int N = head[0], H = head[1], W = head[2], conn = head[3];
    const uint32_t min_area = (uint32_t)head[4];
    const long capacity = head[5];
    const long n = (long)N * H * W, per = (long)H * W;
    std::vector<uint8_t> mask(n), other;
    std::vector<float> scores(n);
    if ((long)fread(mask.data(), 1, n, f) != n || (long)fread(scores.data(), 4, n, f) != n)
      return fprintf(stderr, "short file\n"), 2;
    if (head[6]) {
      other.resize(n);
      if ((long)fread(other.data(), 1, n, f) != n) return fprintf(stderr, "short file\n"), 2;
    }
    float mn = scores[0], mx = scores[0];
    for (float v : scores) mn = std::min(mn, v), mx = std::max(mx, v);
    const bool norm = head[7] && mx != 1.0f;

    // ---- the truth: every region measured on its own, the peak by a loop with the lowest-index rule
    std::vector<uint32_t> region, area;
    std::vector<Truth> truths;
    flood_fill(mask, N, H, W, conn, region, area, truths);
    std::vector<RegionRow> want;
    std::vector<int32_t> want_offsets(N + 1, 0);
    std::vector<uint8_t> want_kept(n, 0);
    unsigned long long want_hit = 0;
    for (Truth& t : truths) {
      if (t.row.area < min_area) continue;
      RegionRow& r = t.row;
      r.x0 = (uint32_t)W, r.y0 = (uint32_t)H;
      float best = 0.0f;
      bool have = false;
      for (long i : t.members) {
        const uint32_t rem = (uint32_t)(i % per), x = rem % (uint32_t)W, y = rem / (uint32_t)W;
        r.x0 = std::min(r.x0, x), r.y0 = std::min(r.y0, y), r.x1 = std::max(r.x1, x + 1), r.y1 = std::max(r.y1, y + 1);
        const float v = aaclip::region_compared(scores[i], norm, mn, mx) + 0.0f;   // -0.0 + 0.0 = +0.0
        if (!have || v > best) best = v, have = true, r.peak_x = x, r.peak_y = y;
        if (!other.empty() && other[i]) ++r.overlap;
        want_kept[i] = 1;
      }
      memcpy(&r.peak, &best, 4);
      want_hit += r.overlap != 0;
      want.push_back(r);
      for (int k = (int)r.image + 1; k <= N; ++k) ++want_offsets[k];
    }

    // ---- the construction, sequentially: the layout is exercised as the launcher walks it
    const aaclip::RegionTableLayout l = aaclip::region_table_layout(n, N);
    if (l.bytes < l.total + 16 || l.tile_word < (size_t)n * 4 || l.roots_before < l.tile_word + (size_t)l.tiles * 8 ||
        l.total < l.roots_before + (size_t)(N + 1) * 4 || l.tiles * aaclip::REGION_TABLE_TILE < n)
      return fprintf(stderr, "case %d: the workspace layout overlaps itself\n", c), 1;
    std::vector<uint8_t> ws(l.bytes, 0xA5);
    uint32_t* rowof = (uint32_t*)(ws.data() + l.rowof);
    uint32_t* roots_before = (uint32_t*)(ws.data() + l.roots_before);
    std::vector<long> pixels(n);
    for (long i = 0; i < n; ++i) pixels[i] = i;
    for (int order = 0; order < 4; ++order) {
      if (order == 1) std::reverse(pixels.begin(), pixels.end());
      if (order >= 2)
        for (size_t k = pixels.size(); k > 1; --k) {   // Fisher-Yates on a 64-bit LCG
          rnd = rnd * 6364136223846793005ull + 1442695040888963407ull;
          std::swap(pixels[k - 1], pixels[(size_t)((rnd >> 33) % k)]);
        }
      const long cap = std::min(capacity, n);
      std::vector<RegionRow> rows(cap);
      std::vector<int32_t> offsets(N + 1, -1);
      std::vector<uint8_t> kept_mask(n, 0xEE);
      aaclip::RegionTableRecord rec{0, 0, 0, 0};
      uint32_t roots = 0, kept = 0;
      for (long p = 0; p < n; ++p) {   // the two scans and the row starts
        if (p % per == 0) offsets[p / per] = (int32_t)kept, roots_before[p / per] = roots;
        if (region[p] != (uint32_t)p + 1) continue;
        const bool keep = area[p] >= min_area;
        rowof[p] = keep ? kept : aaclip::REGION_NO_ROW;
        if (keep && (long)kept < cap)
          rows[kept] = aaclip::region_row_start((uint32_t)(p / per), roots, (uint32_t)(p % per), area[p], H, W);
        ++roots, kept += keep;
      }
      offsets[N] = (int32_t)kept, roots_before[N] = roots;
      rec.kept = kept, rec.regions = roots, rec.dropped = (long)kept > cap ? kept - cap : 0;
      for (long p : pixels) {   // every pixel into its row, in this order
        const bool keep = region[p] != 0 && area[p] >= min_area;
        kept_mask[p] = keep;
        if (!keep) continue;
        const uint32_t rem = (uint32_t)(p % per), x = rem % (uint32_t)W, y = rem / (uint32_t)W;
        const uint32_t key = aaclip::region_score_key(aaclip::region_score_bits(aaclip::region_compared(scores[p], norm, mn, mx)));
        const unsigned long long word = aaclip::region_peak_pack(key, rem);
        const bool set = !other.empty() && other[p];
        uint32_t& entry = rowof[region[p] - 1];
        const uint32_t row = entry & ~aaclip::REGION_HIT_BIT;
        if ((long)row >= cap) {
          if (set && !(entry & aaclip::REGION_HIT_BIT)) entry |= aaclip::REGION_HIT_BIT, ++rec.hit;
          continue;
        }
        RegionRow& r = rows[row];
        unsigned long long have;
        memcpy(&have, &r.peak_x, 8);   // the peak word lives in (peak_x, peak_y)
        have = std::max(have, word);
        memcpy(&r.peak_x, &have, 8);
        r.x0 = std::min(r.x0, x), r.y0 = std::min(r.y0, y), r.x1 = std::max(r.x1, x + 1), r.y1 = std::max(r.y1, y + 1);
        r.overlap += set;
      }
      for (long i = 0; i < std::min((long)kept, cap); ++i) {   // the last step
        unsigned long long word;
        memcpy(&word, &rows[i].peak_x, 8);
        aaclip::region_row_finish(&rows[i], word, roots_before[rows[i].image], W);
        rec.hit += rows[i].overlap != 0;
      }
      if (rec.kept != want.size() || rec.regions != truths.size() || rec.hit != want_hit)
        return fprintf(stderr, "case %d order %d: record %llu %llu %llu, truth %zu %zu %llu\n", c, order, rec.kept,
                       rec.regions, rec.hit, want.size(), truths.size(), want_hit), 1;
      if (offsets != want_offsets) return fprintf(stderr, "case %d order %d: image offsets differ\n", c, order), 1;
      if (kept_mask != want_kept) return fprintf(stderr, "case %d order %d: kept mask differs\n", c, order), 1;
      for (long i = 0; i < std::min((long)kept, cap); ++i)
        if (memcmp(&rows[i], &want[i], sizeof(RegionRow)) != 0) {
          const uint32_t *g = (const uint32_t*)&rows[i], *w = (const uint32_t*)&want[i];
          fprintf(stderr, "case %d (%d x %d x %d, connectivity %d, min_area %u) order %d row %ld:\n", c, N, H, W, conn,
                  min_area, order, i);
          for (int k = 0; k < 12; ++k) fprintf(stderr, "  word %d: %u, truth %u\n", k, g[k], w[k]);
          return 1;
        }
      ++runs;
    }
  }
  fclose(f);
  printf("ok %d cases %ld runs\n", cases, runs);
  return 0;
}

// csrc/overlay_plan.h as overlay.hip and the C ABI use it, in a host program of its own (built with ASan + UBSan by
// tests/test_overlay_cpu.py): the refusal of every bad plan, the tile geometry and its LDS layout for every width, the
// 64-bit offsets at sizes whose byte offsets pass 2^32 and 2^40, the integer blend, the byte clamp and the contour's
// window -- each against brute force -- and a replay of the kernel's store phase on the host: every byte of an
// unaligned run is written exactly once, by aligned chunks.  Prints "ok <checks>" and returns 0, or says what differs
// and returns 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "overlay_plan.h"

using namespace aaclip;

static long g_checks = 0;
#define CHECK(cond, ...)              \
  do {                                \
    ++g_checks;                       \
    if (!(cond)) {                    \
      fprintf(stderr, __VA_ARGS__);   \
      fprintf(stderr, "\n");          \
      return 1;                       \
    }                                 \
  } while (0)

static const float STD_OK[3] = {0.26862954f, 0.26130258f, 0.27577711f};

static int geometry_case(int H, int W, unsigned panels, int T, bool has_pred, bool has_truth) {
  const OverlayGeom g = overlay_geom(H, W, panels, 128, T, has_pred, has_truth);
  CHECK(g.tw >= 1 && g.tw <= W && g.tw <= OVERLAY_TILE_WIDTH && g.rows >= 1 && g.rows <= H && g.rows <= OVERLAY_TILE_ROWS,
        "tile of (%d, %d): %d x %d", H, W, g.rows, g.tw);
  CHECK((long long)g.rows * g.tw <= OVERLAY_TILE_PIXELS, "tile of (%d, %d) holds %d pixels", H, W, g.rows * g.tw);
  // the tiles cover the image exactly once
  CHECK((long long)(g.tiles_x - 1) * g.tw < W && (long long)g.tiles_x * g.tw >= W, "tiles_x of width %d", W);
  CHECK((long long)(g.tiles_y - 1) * g.rows < H && (long long)g.tiles_y * g.rows >= H, "tiles_y of height %d", H);
  CHECK(g.full == (g.tiles_x == 1) && g.runs == (g.full ? 1 : g.rows), "runs of (%d, %d)", H, W);
  CHECK(g.n_panels == overlay_panel_count(panels) && g.n_panels >= 1 && g.n_panels <= 3, "panel count of %u", panels);
  // a run and its shift of up to 3 bytes fit its slot, the slots are dword aligned, the regions do not overlap
  const int run_bytes = (g.full ? g.rows : 1) * g.tw * 3;
  CHECK(g.run_stride % 4 == 0 && g.run_stride >= run_bytes + 3, "run stride of (%d, %d)", H, W);
  CHECK(g.off_lut == 0 && g.off_out >= 256 * 4 && g.off_out % 16 == 0, "table region");
  CHECK(g.off_pred == g.off_out + g.n_panels * g.runs * g.run_stride && g.off_pred % 4 == 0, "output region of (%d, %d)", H, W);
  const int halo = (g.rows + 2 * T) * (g.tw + 2 * T);
  CHECK(g.halo_w == g.tw + 2 * T && g.halo_h == g.rows + 2 * T, "halo of (%d, %d) at T = %d", H, W, T);
  CHECK(g.off_truth - g.off_pred >= (has_pred ? halo : 0) && g.lds_bytes - g.off_truth >= (has_truth ? halo : 0), "mask regions");
  CHECK((size_t)g.lds_bytes <= OVERLAY_LDS_LIMIT, "(%d, %d) at T = %d needs %d bytes of LDS", H, W, T, g.lds_bytes);
  return 0;
}

// the store phase of overlay_kernel for one run of `len` bytes at address `addr`: which bytes each aligned 16-byte chunk
// writes, and from which LDS offset (relative to the run's slot)
static int store_case(unsigned long long addr, int len) {
  std::vector<int> written(len, 0);
  const int chunks = overlay_run_chunks(len);
  const int slot_bytes = ((len + 3) & ~3) + 4;
  int wide = 0;
  for (int k = 0; k < chunks; ++k) {
    const unsigned long long A = addr, end = A + (unsigned long long)len, ca = overlay_chunk_address(A, k);
    if (ca >= end) continue;
    const long long src = (long long)(A & 3) + (long long)(ca - A);       // LDS offset of the chunk's first byte
    if (ca >= A && ca + 16 <= end) {
      CHECK(src % 4 == 0 && src >= 0 && src + 16 <= slot_bytes, "a wide chunk reads LDS offset %lld of %d", src, slot_bytes);
      for (int b = 0; b < 16; ++b) ++written[ca + b - A];
      ++wide;
      continue;
    }
    for (int d = 0; d < 4; ++d) {
      const unsigned long long da = ca + 4ull * d;
      if (da >= A && da + 4 <= end) {
        CHECK((src + 4 * d) % 4 == 0 && src + 4 * d >= 0 && src + 4 * d + 4 <= slot_bytes, "a dword reads outside its slot");
        for (int b = 0; b < 4; ++b) ++written[da + b - A];
      } else {
        for (int b = 0; b < 4; ++b)
          if (da + b >= A && da + b < end) {
            CHECK(src + 4 * d + b >= 0 && src + 4 * d + b < slot_bytes, "a byte reads outside its slot");
            ++written[da + b - A];
          }
      }
    }
  }
  for (int i = 0; i < len; ++i) CHECK(written[i] == 1, "byte %d of a run of %d at %llx is written %d times", i, len, addr, written[i]);
  // the chunks past the run's last byte, had there been more, would start at or beyond its end
  CHECK((addr & ~15ull) + 16ull * chunks >= addr + (unsigned long long)len, "too few chunks for a run of %d at %llx", len, addr);
  CHECK(wide >= (len - 30) / 16, "a run of %d bytes got %d wide stores", len, wide);
  return 0;
}

static int offsets_case(int H, int W, int n, long long images) {
  const long long b = images - 1;
  for (int y : {0, H - 1})
    for (int x : {0, W - 1}) {
      for (int c : {0, 2}) {
        const __int128 want = (((__int128)b * 3 + c) * H + y) * W + x;
        CHECK((__int128)overlay_frame_offset(H, W, b, c, y, x) == want && want < (__int128)images * 3 * H * W, "frame offset");
      }
      const __int128 mwant = ((__int128)b * H + y) * W + x;
      CHECK((__int128)overlay_map_offset(H, W, b, y, x) == mwant && mwant < (__int128)images * H * W, "map offset");
      for (int p : {0, n - 1}) {
        const __int128 owant = ((((__int128)b * n + p) * H + y) * W + x) * 3;
        CHECK((__int128)overlay_out_offset(H, W, n, b, p, y, x) == owant && owant + 3 <= (__int128)images * n * H * W * 3,
              "output offset");
      }
    }
  CHECK(overlay_out_offset(H, W, n, b, n - 1, H - 1, W - 1) + 3 == images * n * H * W * 3, "last output byte");
  CHECK(overlay_frame_offset(H, W, b, 2, H - 1, W - 1) + 1 == images * 3 * H * W, "last frame element");
  return 0;
}

int main() {
  // ---- refusals, each bad field on its own
  CHECK(overlay_plan_check(2, 70, 70, 7, 128, 1, STD_OK) == nullptr, "a good plan is refused");
  CHECK(overlay_plan_check(0, 70, 70, 7, 128, 1, STD_OK) == nullptr, "images == 0 passes");
  CHECK(overlay_plan_check(-1, 70, 70, 7, 128, 1, STD_OK) != nullptr, "images < 0");
  CHECK(overlay_plan_check(1, 0, 70, 7, 128, 1, STD_OK) != nullptr && overlay_plan_check(1, 70, -4, 7, 128, 1, STD_OK) != nullptr,
        "height or width < 1");
  CHECK(overlay_plan_check(1, 70, 70, 0, 128, 1, STD_OK) != nullptr && overlay_plan_check(1, 70, 70, 8, 128, 1, STD_OK) != nullptr,
        "no panel, unknown panel");
  CHECK(overlay_plan_check(1, 70, 70, 7, -1, 1, STD_OK) != nullptr && overlay_plan_check(1, 70, 70, 7, 257, 1, STD_OK) != nullptr &&
            overlay_plan_check(1, 70, 70, 7, 0, 1, STD_OK) == nullptr && overlay_plan_check(1, 70, 70, 7, 256, 1, STD_OK) == nullptr,
        "alpha256 outside 0 .. 256");
  CHECK(overlay_plan_check(1, 70, 70, 7, 128, -1, STD_OK) != nullptr && overlay_plan_check(1, 70, 70, 7, 128, 9, STD_OK) != nullptr &&
            overlay_plan_check(1, 70, 70, 7, 128, 0, STD_OK) == nullptr && overlay_plan_check(1, 70, 70, 7, 128, 8, STD_OK) == nullptr,
        "thickness outside 0 .. 8");
  for (float bad : {0.0f, -1.0f, (float)INFINITY, (float)NAN})
    for (int c = 0; c < 3; ++c) {
      float sd[3] = {STD_OK[0], STD_OK[1], STD_OK[2]};
      sd[c] = bad;
      CHECK(overlay_plan_check(1, 70, 70, 7, 128, 1, sd) != nullptr, "std[%d] = %f", c, bad);
    }
  CHECK(overlay_plan_check(INT_MAX, INT_MAX, INT_MAX, 7, 128, 1, STD_OK) != nullptr &&
            overlay_plan_check(1, INT_MAX, INT_MAX, 7, 128, 1, STD_OK) != nullptr &&
            overlay_plan_check(1 << 20, 1 << 18, 1 << 18, 7, 128, 1, STD_OK) == nullptr &&
            overlay_plan_check(1 << 21, 1 << 18, 1 << 18, 7, 128, 1, STD_OK) != nullptr, "sizes that overflow");

  // ---- the tile geometry and its LDS layout: every width up to past two tiles, heights around the row counts
  for (int W = 1; W <= 2 * OVERLAY_TILE_WIDTH + 3; ++W)
    for (int H : {1, 2, 3, 63, 64, 65, 518})
      for (int T : {0, 1, 8})
        if (geometry_case(H, W, 7, T, true, true)) return 1;
  for (unsigned panels = 1; panels <= 7; ++panels)
    for (int T = 0; T <= OVERLAY_MAX_THICKNESS; ++T)
      for (const auto& hw : {std::initializer_list<int>{518, 518}, {924, 924}, {1, 100000}, {100000, 1}, {70, 70}, {64, 72}}) {
        const int H = *hw.begin(), W = *(hw.begin() + 1);
        if (geometry_case(H, W, panels, T, true, true) || geometry_case(H, W, panels, T, false, true) ||
            geometry_case(H, W, panels, T, true, false) || geometry_case(H, W, panels, T, false, false))
          return 1;
      }
  CHECK(overlay_geom(518, 518, 7, 128, 1, true, true).full == 1 && overlay_geom(518, 518, 7, 128, 1, true, true).rows == 3 &&
            overlay_geom(924, 924, 7, 128, 1, true, true).rows == 2 && overlay_geom(2000, 2000, 7, 128, 1, true, true).full == 0,
        "the tiles of the working sizes");

  // ---- the store phase: every alignment, lengths from one byte to several chunks, and the working runs
  for (unsigned long long a = 0; a < 16; ++a)
    for (int len = 1; len <= 100; ++len)
      if (store_case(0x7f0000001000ull + a, len)) return 1;
  for (unsigned long long a : {0ull, 1ull, 2ull, 1554ull, 3 * 518ull * 518ull * 3ull + 1})
    for (int len : {3 * 518 * 3, 2 * 924 * 3, 1024 * 3, 37 * 37 * 3})
      if (store_case(0x7f0000001000ull + a, len)) return 1;

  // ---- 64-bit offsets: 600 frames of 924 x 924 x 3 panels pass 2^32 bytes; larger counts pass 2^40
  if (offsets_case(924, 924, 3, 600) || offsets_case(518, 518, 3, 100000) || offsets_case(5, 3, 2, 3) ||
      offsets_case(1, 1, 1, 1) || offsets_case(1 << 15, 1 << 15, 3, 1 << 20) || offsets_case(7, 100000, 1, 50000))
    return 1;
  CHECK((long long)600 * 3 * 924 * 924 * 3 > (1ll << 32), "the working size is past 4 GiB");

  // ---- the integer pixel functions against their definitions
  for (int a = 0; a <= 256; ++a)
    for (int u = 0; u <= 255; u += (a % 16 ? 5 : 1))
      for (int v = 0; v <= 255; v += (a % 16 ? 3 : 1)) {
        const int got = overlay_blend(a, u, v);
        const double exact = (a * (double)u + (256 - a) * (double)v) / 256.0;
        CHECK(got == (int)floor(exact + 0.5) && got >= 0 && got <= 255, "blend(%d, %d, %d) = %d", a, u, v, got);
        if (a == 0) CHECK(got == v, "alpha256 = 0 is the second colour");
        if (a == 256) CHECK(got == u, "alpha256 = 256 is the first colour");
      }
  CHECK(overlay_clamp_byte(NAN) == 0 && overlay_clamp_byte(-INFINITY) == 0 && overlay_clamp_byte(INFINITY) == 255 &&
            overlay_clamp_byte(-1.0f) == 0 && overlay_clamp_byte(-0.0f) == 0 && overlay_clamp_byte(0.0f) == 0 &&
            overlay_clamp_byte(255.0f) == 255 && overlay_clamp_byte(256.0f) == 255 && overlay_clamp_byte(3e38f) == 255,
        "the byte clamp at its edges");
  for (int b = 0; b <= 255; ++b) CHECK(overlay_clamp_byte((float)b) == b, "the byte clamp at %d", b);
  // the frame byte undoes the normalisation for every byte and channel: ToTensor's and Normalize's fp32 steps, back
  const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
  for (int c = 0; c < 3; ++c)
    for (int b = 0; b <= 255; ++b) {
      volatile float x = (float)b / 255.0f;
      x = x - mean[c];
      x = x / STD_OK[c];
      volatile float v = x * STD_OK[c];
      v = v + mean[c];
      v = v * 255.0f;
      CHECK(overlay_clamp_byte(rintf(v)) == b && fabs((double)v - b) < 1e-4, "byte %d of channel %d comes back as %f", b, c, (double)v);
    }
  // the contour's window: cut to the image, never empty
  for (int n = 1; n <= 20; ++n)
    for (int T = 0; T <= OVERLAY_MAX_THICKNESS; ++T)
      for (int p = 0; p < n; ++p) {
        const OverlayWindow w = overlay_window(p, n, T);
        int lo = n, hi = -1;
        for (int q = 0; q < n; ++q)
          if (abs(q - p) <= T) {
            if (q < lo) lo = q;
            if (q > hi) hi = q;
          }
        CHECK(w.lo == lo && w.hi == hi && w.lo <= p && p <= w.hi, "window of %d in %d at T = %d", p, n, T);
      }
  CHECK(overlay_panel_count(0) == 0 && overlay_panel_count(1) == 1 && overlay_panel_count(5) == 2 && overlay_panel_count(7) == 3,
        "panel counts");
  printf("ok %ld checks\n", g_checks);
  return 0;
}

// PNG encoding on the device: row filters and a segmented deflate (the format, the code builder and everything else
// that is shared with the host: csrc/png_plan.h; include/aaclip.h states the definition for callers).
//
// Two launches, no workgroup waits for another, no global atomics, integers only: a second call gives the same bytes.
//
// png_segment_kernel: one workgroup of 256 threads per (image, segment).
//   1. a wave filters a row: five cost sums over the row's bytes, a wave reduction, the chosen type's bytes into the
//      LDS.  Raw rows are read by bytes, so the pixels may stand at any alignment.
//   2. thread t walks bytes [128 t, 128 t + 128) of the segment.  The LDS image is padded by 4 bytes per 128, so that the
//      64 lanes of a wave, 128 bytes apart, read 64 different banks.  A thread notes the first and the last position in
//      its bytes where a run starts; the run that reaches into its bytes and the one that leaves them follow from its
//      neighbours' notes, and with them the role of every byte (png_token_role).
//   3. the token histogram is counted with LDS atomics; the leaves are ranked by all threads (png_rank), the tree is
//      merged by one (png_tree_depths, at most 285 merges), which also enforces the limit (png_limit_lengths).
//   4. a thread's bits are counted, the counts are summed in order, and the tokens are OR-ed into the zeroed output
//      words of the LDS with LDS atomics (neighbouring threads share a word).  Thread 0 writes the block's header, the
//      end-of-block code and the marker.
//   5. the Huffman block, or the stored block where it is not shorter, goes to the segment's slot of the workspace,
//      its size, length and Adler sums to the segment's record.
// png_gather_kernel: up to PNG_COPY_PARTS workgroups per image.  Each sums the sizes of the images before its own and
//   scans its image's segment sizes; the segments are dealt round-robin to the workgroups, which copy them to their
//   final place in aligned dwords.  The first one writes 78 01, 03 00, the combined Adler-32 and the offsets.
#include "common.h"
#include "kernels.h"
#include "png_plan.h"

namespace aaclip {

namespace {

struct PngShared {
  PngTree tree;
  PngHeader header;
  uint32_t hist[PNG_LITLEN];
  uint16_t code[PNG_LITLEN];
  uint8_t len[PNG_LITLEN + 2];
  int first_break[PNG_THREADS], last_break[PNG_THREADS];
  uint32_t bits[PNG_THREADS];
  uint32_t has_match, s1, s2, size, huffman;
};

constexpr int PNG_NO_BREAK = INT_MAX;

AACLIP_DEV int padded(int i) { return i + ((i / PNG_CHUNK) << 2); }
inline int png_lds_filt_offset() { return (int)((sizeof(PngShared) + 15) & ~(size_t)15); }
inline int png_lds_out_offset(int segment_bytes) {
  return png_lds_filt_offset() + ((segment_bytes + 4 * (segment_bytes / PNG_CHUNK + 1) + 15) & ~15);
}
// the output words hold a block of at most segment_bytes + 5 bytes; one word more takes the spill of the last token
inline int png_lds_out_words(int segment_bytes) { return (segment_bytes + PNG_STORED_EXTRA + 3) / 4 + 2; }
inline size_t png_lds_bytes(int segment_bytes) {
  return (size_t)png_lds_out_offset(segment_bytes) + 4 * (size_t)png_lds_out_words(segment_bytes);
}

AACLIP_DEV void put_bits_atomic(uint32_t* words, uint32_t pos, uint32_t value, int n) {
  const uint32_t w = pos >> 5, sh = pos & 31;
  atomicOr(&words[w], value << sh);
  if (sh + (uint32_t)n > 32) atomicOr(&words[w + 1], value >> (32 - sh));
}

// f(position, byte, role) for every byte of [c0, c1): start0 is where the run of byte c0 starts, next_after the first
// run start at or after c1 (the segment's length if there is none)
template <class F>
AACLIP_DEV void walk(const unsigned char* filt, int c0, int c1, int start0, int next_after, F&& f) {
  int i = c0, s = start0;
  while (i < c1) {
    const int v = filt[padded(i)];
    int e = i + 1;
    while (e < c1 && filt[padded(e)] == v) ++e;
    const int L = (e == c1 ? next_after : e) - s;
    for (int k = i; k < e; ++k) f(k, v, png_token_role(k - s, L));
    i = e, s = e;
  }
}

}  // namespace

__global__ __launch_bounds__(PNG_THREADS) void png_segment_kernel(const uint8_t* __restrict__ pixels, uint32_t* __restrict__ meta,
                                                                   uint8_t* __restrict__ slots, PngGeom g, int off_filt,
                                                                   int off_out, int out_words) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  PngShared& sh = *(PngShared*)lds;
  unsigned char* filt = lds + off_filt;
  uint32_t* out = (uint32_t*)(lds + off_out);
  unsigned char* out8 = lds + off_out;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int R = g.R, C = g.C;
  const long long units = (long long)g.images * g.segments;

  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const long long image = unit / g.segments;
    const int seg = (int)(unit - image * g.segments);
    const int rows = png_segment_rows(g, seg), n = rows * g.row_bytes;
    __syncthreads();                                   // the unit before this one has left the LDS
    for (int w = tid; w < out_words; w += PNG_THREADS) out[w] = 0;
    for (int s = tid; s < PNG_LITLEN; s += PNG_THREADS) sh.hist[s] = 0;
    if (tid == 0) sh.has_match = 0, sh.s1 = 0, sh.s2 = 0;

    // 1. the filters, a wave per row
    for (int r = wave; r < rows; r += PNG_THREADS / 64) {
      const int y = seg * g.rows_per_segment + r;
      const uint8_t* cur = pixels + png_pixel_offset(g, image, y);
      const bool has_up = y > 0;                      // the row above row 0 of an image is zeros
      const uint8_t* up = has_up ? cur - R : cur;
      uint32_t cost[5] = {0, 0, 0, 0, 0};
      for (int x = lane; x < R; x += 64) {
        const int X = cur[x], a = x >= C ? cur[x - C] : 0, b = has_up ? up[x] : 0, c = has_up && x >= C ? up[x - C] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) cost[t] += (uint32_t)png_filter_cost(png_filter_byte(t, X, a, b, c));
      }
#pragma unroll
      for (int t = 0; t < 5; ++t)
        for (int off = 32; off >= 1; off >>= 1) cost[t] += (uint32_t)__shfl_xor((int)cost[t], off, 64);
      const int type = png_filter_choice(cost);
      const int base = r * g.row_bytes;
      if (lane == 0) filt[padded(base)] = (unsigned char)type;
      for (int x = lane; x < R; x += 64) {
        const int X = cur[x], a = x >= C ? cur[x - C] : 0, b = has_up ? up[x] : 0, c = has_up && x >= C ? up[x - C] : 0;
        filt[padded(base + 1 + x)] = (unsigned char)png_filter_byte(type, X, a, b, c);
      }
    }
    __syncthreads();

    // 2. where runs start, and the Adler sums
    const int c0 = tid * PNG_CHUNK, c1 = n < c0 + PNG_CHUNK ? n : c0 + PNG_CHUNK;
    {
      int fb = PNG_NO_BREAK, lb = -1;
      uint32_t a1 = 0;
      uint64_t a2 = 0;
      if (c0 < n) {
        int prev = c0 > 0 ? filt[padded(c0 - 1)] : -1;
        for (int k = c0; k < c1; ++k) {
          const int v = filt[padded(k)];
          if (v != prev) {
            if (fb == PNG_NO_BREAK) fb = k;
            lb = k;
          }
          prev = v;
          a1 += (uint32_t)v;
          a2 += (uint64_t)(n - k) * (uint64_t)v;
        }
        atomicAdd(&sh.s1, a1);
        atomicAdd(&sh.s2, (uint32_t)(a2 % PNG_ADLER_MOD));       // 256 terms below 65521
      }
      sh.first_break[tid] = fb, sh.last_break[tid] = lb;
    }
    __syncthreads();
    int start0 = c0, next_after = n;
    if (c0 < n) {
      if (sh.first_break[tid] != c0)                             // byte 0 starts a run, so the search ends
        for (int t = tid - 1; t >= 0; --t)
          if (sh.last_break[t] >= 0) {
            start0 = sh.last_break[t];
            break;
          }
      for (int t = tid + 1; t < PNG_THREADS; ++t)
        if (sh.first_break[t] != PNG_NO_BREAK) {
          next_after = sh.first_break[t];
          break;
        }
    }

    // 3. the histogram and the code
    {
      uint32_t* hist = sh.hist;
      bool match = false;
      walk(filt, c0, c1, start0, next_after, [hist, &match](int, int v, PngRole role) {
        if (role.kind == 1) atomicAdd(&hist[v], 1u);
        if (role.kind == 2) atomicAdd(&hist[png_length_symbol(role.length).symbol], 1u), match = true;
      });
      if (match) atomicOr(&sh.has_match, 1u);
      if (tid == 0) atomicAdd(&hist[256], 1u);
    }
    __syncthreads();
    for (int s = tid; s < PNG_LITLEN; s += PNG_THREADS) sh.tree.key[s] = sh.hist[s] ? sh.hist[s] : PNG_NONE;
    __syncthreads();
    for (int s = tid; s < PNG_LITLEN; s += PNG_THREADS) {
      sh.len[s] = 0;
      if (sh.tree.key[s] != PNG_NONE) sh.tree.order[png_rank(sh.tree.key, PNG_LITLEN, s)] = (uint16_t)s;
    }
    __syncthreads();
    if (tid == 0) {
      int m = 0;
      for (int s = 0; s < PNG_LITLEN; ++s) m += sh.tree.key[s] != PNG_NONE ? 1 : 0;
      png_tree_depths(sh.tree, m);                     // m >= 2: a literal and end-of-block
      png_limit_lengths(sh.tree, m, PNG_LIMIT, sh.len);
    }
    __syncthreads();

    // 4. bits per thread, their places, the header
    {
      const uint8_t* len = sh.len;
      uint32_t bits = 0;
      walk(filt, c0, c1, start0, next_after, [len, &bits](int, int v, PngRole role) {
        if (role.kind == 1) bits += len[v];
        if (role.kind == 2) {
          const PngLength l = png_length_symbol(role.length);
          bits += (uint32_t)len[l.symbol] + (uint32_t)l.extra_bits + 1u;
        }
      });
      sh.bits[tid] = bits;
    }
    __syncthreads();
    if (tid == 0) {
      png_canonical_codes(sh.len, PNG_LITLEN, sh.code);
      const uint32_t header_bits = png_block_header(sh.len, (int)sh.has_match, sh.header, sh.tree, nullptr);
      uint32_t pos = header_bits;
      for (int t = 0; t < PNG_THREADS; ++t) {
        const uint32_t b = sh.bits[t];
        sh.bits[t] = pos;
        pos += b;
      }
      const uint32_t end_bits = pos + sh.len[256] + 3u;          // end-of-block, an empty stored block's header
      const uint32_t body = (end_bits + 7u) >> 3;
      const uint32_t size = body + 4u;
      sh.huffman = size < (uint32_t)(n + PNG_STORED_EXTRA) ? 1u : 0u;
      sh.size = sh.huffman ? size : (uint32_t)(n + PNG_STORED_EXTRA);
      if (sh.huffman) {
        png_block_header(sh.len, (int)sh.has_match, sh.header, sh.tree, out);
        png_put_bits(out, pos, sh.code[256], sh.len[256]);
        png_put_bits(out, 8u * body + 16u, 0xFFFFu, 16);
      } else {
        out8[0] = 0;
        out8[1] = (unsigned char)(n & 255), out8[2] = (unsigned char)(n >> 8);
        out8[3] = (unsigned char)(~n & 255), out8[4] = (unsigned char)((~n >> 8) & 255);
      }
    }
    __syncthreads();
    if (sh.huffman) {
      const uint8_t* len = sh.len;
      const uint16_t* code = sh.code;
      uint32_t pos = sh.bits[tid];
      walk(filt, c0, c1, start0, next_after, [len, code, out, &pos](int, int v, PngRole role) {
        if (role.kind == 1) {
          put_bits_atomic(out, pos, code[v], len[v]);
          pos += len[v];
        }
        if (role.kind == 2) {
          const PngLength l = png_length_symbol(role.length);
          const int nb = len[l.symbol] + l.extra_bits + 1;       // the distance code is one zero bit
          put_bits_atomic(out, pos, (uint32_t)code[l.symbol] | ((uint32_t)l.extra << len[l.symbol]), nb);
          pos += (uint32_t)nb;
        }
      });
    } else {
      for (int k = tid; k < n; k += PNG_THREADS) out8[PNG_STORED_EXTRA + k] = filt[padded(k)];
    }
    __syncthreads();

    // 5. the slot and the record
    uint32_t* slot = (uint32_t*)(slots + (unit * (long long)g.slot_bytes));
    const int words = (int)((sh.size + 3u) >> 2);                // within the slot: its bytes are a multiple of 16
    for (int w = tid; w < words; w += PNG_THREADS) slot[w] = out[w];
    if (tid == 0) {
      uint32_t* rec = meta + unit * PNG_META_WORDS;
      rec[0] = sh.size, rec[1] = sh.s1, rec[2] = sh.s2 % PNG_ADLER_MOD, rec[3] = (uint32_t)n;
    }
  }
}

__global__ __launch_bounds__(PNG_THREADS) void png_gather_kernel(const uint32_t* __restrict__ meta, const uint8_t* __restrict__ slots,
                                                                  uint8_t* __restrict__ payload, int64_t* __restrict__ offsets,
                                                                  PngGeom g) {
  __shared__ long long scan[PNG_THREADS];
  __shared__ long long seg_off[PNG_THREADS];
  __shared__ uint32_t seg_size[PNG_THREADS];
  const int tid = threadIdx.x, part = blockIdx.x, parts = gridDim.x;

  for (long long image = blockIdx.y; image < g.images; image += gridDim.y) {
    // the bytes of the images before this one
    long long acc = 0;
    for (long long u = tid; u < image * g.segments; u += PNG_THREADS) acc += meta[u * PNG_META_WORDS];
    __syncthreads();
    scan[tid] = acc;
    __syncthreads();
    for (int s = PNG_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) scan[tid] += scan[tid + s];
      __syncthreads();
    }
    const long long base = scan[0] + (long long)PNG_STREAM_EXTRA * image;
    long long carry = base + 2;
    for (int chunk0 = 0; chunk0 < g.segments; chunk0 += PNG_THREADS) {
      const int seg = chunk0 + tid;
      const uint32_t size = seg < g.segments ? meta[(image * g.segments + seg) * PNG_META_WORDS] : 0u;
      __syncthreads();                                 // scan[0] and the chunk before have been read
      scan[tid] = size;
      __syncthreads();
      for (int d = 1; d < PNG_THREADS; d <<= 1) {
        const long long add = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
      }
      seg_off[tid] = carry + scan[tid] - size;
      seg_size[tid] = size;
      __syncthreads();
      const int here = g.segments - chunk0 < PNG_THREADS ? g.segments - chunk0 : PNG_THREADS;
      // chunk0 is a multiple of 256 and parts divides nothing in particular: segment s belongs to part s % parts
      for (int j = 0; j < here; ++j) {
        if ((chunk0 + j) % parts != part) continue;
        const uint8_t* src = slots + (image * g.segments + chunk0 + j) * (long long)g.slot_bytes;
        uint8_t* dst = payload + seg_off[j];
        const int size_j = (int)seg_size[j];
        int head = (int)((4u - (unsigned)((unsigned long long)dst & 3ull)) & 3u);
        if (head > size_j) head = size_j;
        const int body = (size_j - head) >> 2;
        for (int k = tid; k < head; k += PNG_THREADS) dst[k] = src[k];
        for (int w = tid; w < body; w += PNG_THREADS) {
          const uint8_t* s4 = src + head + 4 * w;
          *(uint32_t*)(dst + head + 4 * w) = (uint32_t)s4[0] | ((uint32_t)s4[1] << 8) | ((uint32_t)s4[2] << 16) | ((uint32_t)s4[3] << 24);
        }
        for (int k = head + 4 * body + tid; k < size_j; k += PNG_THREADS) dst[k] = src[k];
      }
      carry += scan[PNG_THREADS - 1];
    }
    if (part == 0 && tid == 0) {
      uint32_t a = 1, b = 0;
      for (int s = 0; s < g.segments; ++s) {
        const uint32_t* rec = meta + (image * g.segments + s) * PNG_META_WORDS;
        png_adler_combine(a, b, rec[3], rec[1], rec[2]);
      }
      payload[base] = 0x78, payload[base + 1] = 0x01;
      payload[carry] = 0x03, payload[carry + 1] = 0x00;
      payload[carry + 2] = (uint8_t)(b >> 8), payload[carry + 3] = (uint8_t)(b & 255);
      payload[carry + 4] = (uint8_t)(a >> 8), payload[carry + 5] = (uint8_t)(a & 255);
      offsets[image] = base;
      if (image == g.images - 1) offsets[g.images] = carry + 6;
    }
    __syncthreads();
  }
}

void launch_png_encode(const PngGeom& g, const uint8_t* pixels, void* workspace, uint8_t* payload, int64_t* offsets,
                       hipStream_t s) {
  // up to 78 KiB of LDS for a full segment: above the 64 KiB a kernel gets without asking, and two workgroups still
  // fit a CU's 160 KiB.  The attribute belongs to the current device's copy of the kernel, so it is set on every call
  const size_t lds = png_lds_bytes(g.segment_bytes);
  if (hipFuncSetAttribute((const void*)png_segment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)png_lds_bytes(PNG_SEGMENT_BYTES)) != hipSuccess) {
    (void)hipGetLastError();
    set_launch_error("png_encode: the device refused the dynamic LDS of a segment");
    return;
  }
  uint32_t* meta = (uint32_t*)workspace;
  uint8_t* slots = (uint8_t*)workspace + png_slot_offset(g, 0, 0);
  const long long units = (long long)g.images * g.segments;
  const unsigned grid = (unsigned)(units < (1ll << 20) ? units : (1ll << 20));
  hipLaunchKernelGGL(png_segment_kernel, dim3(grid), dim3(PNG_THREADS), lds, s, pixels, meta, slots, g, png_lds_filt_offset(),
                     png_lds_out_offset(g.segment_bytes), png_lds_out_words(g.segment_bytes));
  const unsigned parts = (unsigned)(g.segments < PNG_COPY_PARTS ? g.segments : PNG_COPY_PARTS);
  hipLaunchKernelGGL(png_gather_kernel, dim3(parts, (unsigned)(g.images < 65535 ? g.images : 65535)), dim3(PNG_THREADS), 0, s,
                     meta, slots, payload, offsets, g);
}

}  // namespace aaclip

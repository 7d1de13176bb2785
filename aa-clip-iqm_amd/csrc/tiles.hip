// Tiled inference: a frame larger than the model's input is cut into G x G overlapping tiles of the model's size, every
// tile goes through the model, and the tile maps are blended back into one map of the frame's size (the geometry and
// the weights: csrc/tile_plan.h).
//   tile_gather_kernel   tiles[b * G^2 + t, c, y, x] = canvas[b, c, i * T + y, j * T + x]: a copy of bits
//   tile_stitch_kernel   a gather over OUTPUT pixels: a canvas pixel under one tile takes that tile's bits; under 2 or 4
//                        tiles it is (sum_t w_t * v_t) / (sum_t w_t) with the tiles in ascending t, in fp32, products and
//                        sums rounded one by one (-ffp-contract=off).  No atomics, no workspace, no memset: a second
//                        call gives the same bytes.
// Both are one launch.  A workgroup is 4 waves, each on one row of a plane (a tile's channel, or a canvas channel), its
// 64 lanes striding along the row with vectors of V floats, V = 4, 2 or 1 by what divides S and T and by the alignment of
// the pointers (tile_vector_width; at S = 518, T = 406 it is 2).  grid.x walks the rows of a plane and grid.y the
// planes, each in a stride loop where the grid is smaller than the work, so no index needs a division per element and
// every offset is formed in 64 bits.
#include "common.h"
#include "tile_plan.h"

namespace aaclip {

namespace {

constexpr int ROWS = 4;           // rows (waves) per workgroup
constexpr int LANES = 64;

template <int V>
struct Vec;
template <>
struct Vec<1> { typedef float type; };
template <>
struct Vec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <>
struct Vec<4> { typedef float type __attribute__((ext_vector_type(4))); };

template <int V>
AACLIP_DEV float lane_of(const typename Vec<V>::type& v, int e) { return v[e]; }
template <>
AACLIP_DEV float lane_of<1>(const float& v, int) { return v; }
template <int V>
AACLIP_DEV void set_lane(typename Vec<V>::type& v, int e, float x) { v[e] = x; }
template <>
AACLIP_DEV void set_lane<1>(float& v, int, float x) { v = x; }

}  // namespace

template <int V>
__global__ __launch_bounds__(ROWS * LANES) void tile_gather_kernel(const float* __restrict__ canvas,
                                                                    float* __restrict__ tiles, TileGeom g,
                                                                    unsigned planes) {
  typedef typename Vec<V>::type vec;
  const unsigned g2 = (unsigned)g.G * (unsigned)g.G;
  for (long long row = (long long)blockIdx.x * ROWS + threadIdx.y; row < g.S; row += (long long)gridDim.x * ROWS) {
    const int y = (int)row;
    for (unsigned plane = blockIdx.y; plane < planes; plane += gridDim.y) {
      const unsigned bt = plane / (unsigned)g.channels, c = plane - bt * (unsigned)g.channels;
      const unsigned b = bt / g2, t = bt - b * g2;
      const int i = (int)(t / (unsigned)g.G), j = (int)(t - (unsigned)i * (unsigned)g.G);
      const float* src = canvas + canvas_offset(g, (long long)b, (int)c, i * g.T + y, j * g.T);
      float* dst = tiles + ((long long)plane * g.S + y) * (long long)g.S;
      for (long long x = (long long)threadIdx.x * V; x < g.S; x += LANES * V) *(vec*)(dst + x) = *(const vec*)(src + x);
    }
  }
}

template <int V>
__global__ __launch_bounds__(ROWS * LANES) void tile_stitch_kernel(const float* __restrict__ tiles,
                                                                    float* __restrict__ canvas, TileGeom g,
                                                                    unsigned planes) {
  typedef typename Vec<V>::type vec;
  for (long long row = (long long)blockIdx.x * ROWS + threadIdx.y; row < g.C; row += (long long)gridDim.x * ROWS) {
    const int Y = (int)row;
    const TileCover rows = tile_cover(Y, g.S, g.G, g.T);
    for (unsigned plane = blockIdx.y; plane < planes; plane += gridDim.y) {
      const unsigned b = plane / (unsigned)g.channels, c = plane - b * (unsigned)g.channels;
      float* dst = canvas + ((long long)plane * g.C + Y) * (long long)g.C;
      for (long long col = (long long)threadIdx.x * V; col < g.C; col += LANES * V) {
        const int X = (int)col;
        const TileCover cols = tile_cover(X, g.S, g.G, g.T);    // the V pixels share it: V divides S and T
        if (rows.n == 1 && cols.n == 1) {
          const int t = rows.lo * g.G + cols.lo;
          *(vec*)(dst + X) =
              *(const vec*)(tiles + tile_offset(g, (long long)b, t, (int)c, Y - rows.lo * g.T, X - cols.lo * g.T));
          continue;
        }
        float num[V], den[V];
        bool first = true;
        for (int di = 0; di < rows.n; ++di) {
          const int i = rows.lo + di, y = Y - i * g.T;
          const float wy = (float)tile_w1(y, g.S);
          for (int dj = 0; dj < cols.n; ++dj) {
            const int j = cols.lo + dj, x = X - j * g.T;
            const vec v = *(const vec*)(tiles + tile_offset(g, (long long)b, i * g.G + j, (int)c, y, x));
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const float w = wy * (float)tile_w1(x + e, g.S);
              const float p = w * lane_of<V>(v, e);
              num[e] = first ? p : num[e] + p;
              den[e] = first ? w : den[e] + w;
            }
            first = false;
          }
        }
        vec out;
#pragma unroll
        for (int e = 0; e < V; ++e) set_lane<V>(out, e, num[e] / den[e]);
        *(vec*)(dst + X) = out;
      }
    }
  }
}

namespace {

// grid.x: the rows of one plane, ROWS per workgroup, at most 2^20 workgroups at a time; grid.y: the planes, at most
// 65535 at a time (the kernels stride over the rest)
dim3 tile_grid(int rows, long long planes) {
  const long long groups = ((long long)rows + ROWS - 1) / ROWS;
  return dim3((unsigned)(groups < (1 << 20) ? groups : (1 << 20)), (unsigned)(planes < 65535 ? planes : 65535));
}

}  // namespace

void launch_tile_gather(const TileGeom& g, int images, const float* canvas, float* tiles, hipStream_t s) {
  const long long planes = (long long)images * g.G * g.G * g.channels;
  const dim3 grid = tile_grid(g.S, planes), block(LANES, ROWS);
  switch (tile_vector_width(g.S, g.T, canvas, tiles)) {
    case 4: hipLaunchKernelGGL(tile_gather_kernel<4>, grid, block, 0, s, canvas, tiles, g, (unsigned)planes); break;
    case 2: hipLaunchKernelGGL(tile_gather_kernel<2>, grid, block, 0, s, canvas, tiles, g, (unsigned)planes); break;
    default: hipLaunchKernelGGL(tile_gather_kernel<1>, grid, block, 0, s, canvas, tiles, g, (unsigned)planes);
  }
}

void launch_tile_stitch(const TileGeom& g, int images, const float* tiles, float* canvas, hipStream_t s) {
  const long long planes = (long long)images * g.channels;
  const dim3 grid = tile_grid(g.C, planes), block(LANES, ROWS);
  switch (tile_vector_width(g.S, g.T, canvas, tiles)) {
    case 4: hipLaunchKernelGGL(tile_stitch_kernel<4>, grid, block, 0, s, tiles, canvas, g, (unsigned)planes); break;
    case 2: hipLaunchKernelGGL(tile_stitch_kernel<2>, grid, block, 0, s, tiles, canvas, g, (unsigned)planes); break;
    default: hipLaunchKernelGGL(tile_stitch_kernel<1>, grid, block, 0, s, tiles, canvas, g, (unsigned)planes);
  }
}

}  // namespace aaclip

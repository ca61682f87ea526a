// The precision-recall sweep of a class's whole-scene probabilities (rua_scene_area_open, rua_scene_sweep_hist, include/rua_hip.h;
// scenes.host_area_open / host_sweep_hist are the definitions).
//
// The opened map G of a uint8 probability map P under descending levels t_0 > t_1 > ...: G[x] is the largest level t such that x
// lies in a connected component of {P >= t} with at least min_area pixels, 0 if there is none.  The kept sets are nested, so G is
// built level by level, labelling only what is still unsettled: U_t = {P >= t and G == 0}, and a component Z of U_t is settled
// (G = t on Z) iff |Z| >= min_area or a pixel of Z has a neighbour (same connectivity) with G != 0 - such a neighbour has P > t and
// belongs to a kept component of a higher level, which Z's full component then contains.
//
// min_area == 1: G[x] is the largest level <= P[x], one streaming pass through a 256-entry table.  Otherwise G is zeroed and every
// level takes the four launches of rua_scene_regions, restated over the predicate "x in U_t" (unionfind.h holds the forest):
//   1. open_tile: a block per SW_T x SW_T tile reads P and G, leaves at once if the tile holds no pixel of U, otherwise labels U in
//      LDS (row runs, one union per pair of touching runs) and writes global parents and zeroed areas for the pixels of U only.
//      Parents of other pixels are stale and never reached: every walk starts at a pixel of U and every link joins roots of U.
//   2. open_seams: a lane per seam pixel joins it to its neighbours across the seam when both are in U.
//   3. open_flatten: per tile with U, the pixels of U are counted per slot, each occupied slot walks to its root once and adds its
//      count with one atomic; a slot any of whose pixels has a settled neighbour (G read with a one-pixel halo) also sets bit 31 of
//      areas[root].  H * W < 2^31 keeps that bit free of the sum, and an unsigned compare reads "large or touched" in one go.
//   4. open_settle: G[x] = t for x in U whose root's areas word is >= min_area, unsigned.
// The number of launches depends on T alone, no block waits for another and nothing is read back.
//
// rua_scene_sweep_hist: one pass, four consecutive pixels per lane, an LDS histogram [2][2][256] of 32-bit cells (a block sees 1024
// pixels), equal cells of a lane's four pixels merged before the LDS atomic, one 64-bit atomic per non-zero cell at the end.
#include "unionfind.h"

namespace {

// tests/test_scene_sweep_gpu.py sizes its maps by TILE, a copy of SW_T: change them together.
constexpr int SW_T = 32;                       // tile edge in pixels: a tile row is half a wave
constexpr int SW_PIX = SW_T * SW_T;            // 1024 pixels, four per lane of a 256-lane block
constexpr int SW_HALO = SW_T + 2;
constexpr int SW_CHUNK = 96;                   // scenes per launch: 40 bytes each
constexpr int SW_TCHUNK = 120;                 // ... of the table kernel and the histogram: 24 and 32 bytes each
constexpr unsigned SW_TOUCHED = 0x80000000u;   // bit 31 of an areas word
constexpr int SW_SLOT_TOUCHED = 1 << 30;       // the same mark in a tile's LDS count, which is at most 1024

struct OpenScene { const uint8_t* prob; uint8_t* open; int32_t* labels; int32_t* areas; int H, W; };
struct OpenArgs {
  OpenScene s[SW_CHUNK];
  int stride, level, conn;
  unsigned min_area;
};
static_assert(sizeof(OpenScene) == 40 && sizeof(OpenArgs) <= 4096, "kernel arguments are limited to 4 KiB");

struct TableScene { const uint8_t* prob; uint8_t* open; int H, W; };
struct TableArgs {
  TableScene s[SW_TCHUNK];
  uint8_t table[256];
  int stride, pad;
};
static_assert(sizeof(TableScene) == 24 && sizeof(TableArgs) <= 4096, "kernel arguments are limited to 4 KiB");

struct HistScene { const uint8_t* prob; const uint8_t* open; const uint8_t* cls; int H, W; };
struct HistArgs {
  HistScene s[SW_TCHUNK];
  unsigned long long* hist;
  int stride, positive, C, pad;
};
static_assert(sizeof(HistScene) == 32 && sizeof(HistArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// the tile of a block: false for the whole block when the scene has no such tile (a smaller scene of the chunk)
struct Tile { int i0, j0, th, tw; };
__device__ __forceinline__ bool tile_of(const OpenScene& sc, Tile& t) {
  const int tiles_x = (sc.W - 1) / SW_T + 1;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  if (ty > (sc.H - 1) / SW_T) return false;
  t.i0 = ty * SW_T; t.j0 = tx * SW_T;
  t.th = min(SW_T, sc.H - t.i0); t.tw = min(SW_T, sc.W - t.j0);
  return true;
}

// x, a pixel index inside the scene, is unsettled at this level
__device__ __forceinline__ bool in_u(const OpenScene& sc, const OpenArgs& a, size_t x) {
  return sc.prob[x * (size_t)a.stride] >= a.level && sc.open[x] == 0;
}

// one lane per pixel; false beyond the scene
__device__ __forceinline__ bool sw_pixel(int H, int W, long long& x) {
  x = (long long)blockIdx.x * 256 + threadIdx.x;
  return x < (long long)H * W;
}

__global__ __launch_bounds__(256) void open_table(TableArgs a) {
  const TableScene& sc = a.s[blockIdx.y];
  long long x;
  if (sw_pixel(sc.H, sc.W, x)) sc.open[x] = a.table[sc.prob[(size_t)x * a.stride]];
}

__global__ __launch_bounds__(256) void open_zero(OpenArgs a) {
  const OpenScene& sc = a.s[blockIdx.y];
  long long x;
  if (sw_pixel(sc.H, sc.W, x)) sc.open[x] = 0;
}

__global__ __launch_bounds__(256) void open_tile(OpenArgs a) {
  __shared__ uint8_t B[SW_PIX];                  // 1: the pixel is in U; 0: it is not, or lies outside the scene
  __shared__ int P[SW_PIX];                      // parents, as tile indices ly * SW_T + lx
  const OpenScene& sc = a.s[blockIdx.y];
  Tile t;
  if (!tile_of(sc, t)) return;
  const int tid = threadIdx.x, W = sc.W, lx = tid & 31;
  const bool in_x = lx < t.tw;
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    const bool u = in_x && ly < t.th && in_u(sc, a, (size_t)(t.i0 + ly) * W + t.j0 + lx);
    B[p] = u;
    any |= u;
  }
  if (!__syncthreads_or(any)) return;            // the whole block: no pixel of U, nothing to label
#pragma unroll
  for (int k = 0; k < 4; ++k) {                  // every pixel starts below the first pixel of its row run
    const int p = tid + 256 * k;
    const uint32_t bits = row_breaks(lx == 0 || B[p - 1] != B[p]);                    // bit 0 is always set
    P[p] = (p & ~31) + 31 - __clz(bits & (0xFFFFFFFFu >> (31 - lx)));
  }
  __syncthreads();
  const bool eight = a.conn == 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    if (!B[p] || ly == 0) continue;
    const int up = p - SW_T;
    const bool left = lx > 0 && B[p - 1], upleft = lx > 0 && B[up - 1], above = B[up];
    // two runs that touch share a first column: there either this run or the one above starts
    if (above && !(left && upleft)) lds_union(P, p, up);
    if (eight) {
      // a diagonal pair needs a union of its own only if neither pixel beside it joins the two runs already
      if (upleft && !above && !left) lds_union(P, p, up - 1);
      if (lx + 1 < SW_T && B[up + 1] && !above && !B[p + 1]) lds_union(P, p, up + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    if (!B[p]) continue;
    const int r = lds_find(P, p);
    const size_t at = (size_t)(t.i0 + ly) * W + t.j0 + lx;
    sc.labels[at] = (t.i0 + (r >> 5)) * W + t.j0 + (r & 31);
    sc.areas[at] = 0;
  }
}

__global__ __launch_bounds__(256) void open_seams(OpenArgs a) {
  const OpenScene& sc = a.s[blockIdx.y];
  const int H = sc.H, W = sc.W;
  const int nh = (H - 1) / SW_T, nv = (W - 1) / SW_T;                                 // seams between tile rows, between tile columns
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long across = (long long)nh * W;
  if (e >= across + (long long)nv * H) return;
  const bool eight = a.conn == 8;
  if (e < across) {                              // pixel (i, j) on the first row of a tile row: its neighbours in row i - 1
    const int i = ((int)(e / W) + 1) * SW_T, j = (int)(e % W);
    const int x = i * W + j, u = x - W;
    if (!in_u(sc, a, x)) return;
    const bool left = j > 0 && in_u(sc, a, x - 1), upleft = j > 0 && in_u(sc, a, u - 1), above = in_u(sc, a, u);
    // the run cut of open_tile, where the pixels to the left lie in the same tiles: across a tile corner the pair to the left is
    // itself a seam pair that may count on this one
    if (above && !(left && upleft && j % SW_T != 0)) g_union(sc.labels, x, u);
    if (eight) {
      if (upleft && !above && !left) g_union(sc.labels, x, u - 1);
      if (j + 1 < W && in_u(sc, a, u + 1) && !above && !in_u(sc, a, x + 1)) g_union(sc.labels, x, u + 1);
    }
  } else {                                       // pixel (i, j) on the first column of a tile column: its neighbours in column j - 1
    const long long f = e - across;
    const int j = ((int)(f / H) + 1) * SW_T, i = (int)(f % H);
    const int x = i * W + j;
    if (!in_u(sc, a, x)) return;
    const bool left = in_u(sc, a, x - 1), above = i > 0 && in_u(sc, a, x - W), upleft = i > 0 && in_u(sc, a, x - W - 1);
    if (left && !(above && upleft && i % SW_T != 0)) g_union(sc.labels, x, x - 1);
    if (eight) {
      if (upleft && !above && !left) g_union(sc.labels, x, x - W - 1);
      if (i + 1 < H && in_u(sc, a, x + W - 1) && !left && !in_u(sc, a, x + W)) g_union(sc.labels, x, x + W - 1);
    }
  }
}

__global__ __launch_bounds__(256) void open_flatten(OpenArgs a) {
  __shared__ int cnt[SW_PIX];                    // pixels of U per slot, and SW_SLOT_TOUCHED
  __shared__ int root[SW_PIX];                   // the root of an occupied slot
  __shared__ uint8_t G[SW_HALO * SW_HALO];       // the opened map of the tile and one pixel around it; 0 outside the scene
  const OpenScene& sc = a.s[blockIdx.y];
  Tile t;
  if (!tile_of(sc, t)) return;
  const int tid = threadIdx.x, H = sc.H, W = sc.W, lx = tid & 31;
  const bool in_x = lx < t.tw;
  bool u[4], any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = (tid + 256 * k) >> 5;
    u[k] = in_x && ly < t.th && in_u(sc, a, (size_t)(t.i0 + ly) * W + t.j0 + lx);
    any |= u[k];
  }
  if (!__syncthreads_or(any)) return;            // the whole block
  for (int e = tid; e < SW_HALO * SW_HALO; e += 256) {
    const int i = t.i0 + e / SW_HALO - 1, j = t.j0 + e % SW_HALO - 1;
    G[e] = (i >= 0 && i < H && j >= 0 && j < W) ? sc.open[(size_t)i * W + j] : (uint8_t)0;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) cnt[tid + 256 * k] = 0;
  __syncthreads();
  const bool eight = a.conn == 8;
  int slot[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    slot[k] = p;                                 // a tile root that was linked outside the tile stands for itself
    if (u[k]) {
      const int q = sc.labels[(size_t)(t.i0 + ly) * W + t.j0 + lx];
      const int qi = q / W - t.i0, qj = q % W - t.j0;
      if (qi >= 0 && qi < SW_T && qj >= 0 && qj < SW_T) slot[k] = qi * SW_T + qj;
    }
    // runs of one slot along the row are counted by their first lane: all 64 lanes take part in the shuffle and the ballot
    const int beside = __shfl_up(slot[k], 1);
    const uint32_t bits = row_breaks(!u[k] || lx == 0 || beside != slot[k]);
    if (u[k] && ((bits >> lx) & 1u)) {
      const uint32_t rest = (bits >> lx) >> 1;   // the run ends at the next break, or with the row
      atomicAdd(&cnt[slot[k]], rest ? __ffs(rest) : SW_T - lx);
    }
    if (u[k]) {
      const uint8_t* g = G + (ly + 1) * SW_HALO + lx + 1;
      bool touched = g[-SW_HALO] | g[SW_HALO] | g[-1] | g[1];
      if (eight) touched |= (g[-SW_HALO - 1] | g[-SW_HALO + 1] | g[SW_HALO - 1] | g[SW_HALO + 1]) != 0;
      if (touched) atomicOr(&cnt[slot[k]], SW_SLOT_TOUCHED);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = tid + 256 * k, c = cnt[s], n = c & (SW_SLOT_TOUCHED - 1);
    if (n == 0) continue;                        // an occupied slot is a pixel of U in the tile; a mark comes with a count
    const int r = g_find(sc.labels, (t.i0 + (s >> 5)) * W + t.j0 + (s & 31));
    root[s] = r;
    atomicAdd(sc.areas + r, n);                  // the sum over all tiles is at most H * W < 2^31: it never reaches bit 31
    if (c & SW_SLOT_TOUCHED) atomicOr(reinterpret_cast<unsigned*>(sc.areas + r), SW_TOUCHED);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    if (u[k]) sc.labels[(size_t)(t.i0 + ly) * W + t.j0 + lx] = root[slot[k]];
  }
}

__global__ __launch_bounds__(256) void open_settle(OpenArgs a) {
  const OpenScene& sc = a.s[blockIdx.y];
  long long x;
  if (!sw_pixel(sc.H, sc.W, x) || !in_u(sc, a, (size_t)x)) return;
  if ((unsigned)sc.areas[sc.labels[x]] >= a.min_area) sc.open[x] = (uint8_t)a.level;
}

// a lane's run of equal cells leaves with one LDS atomic
__device__ __forceinline__ void hist_put(unsigned* h, int& cur, unsigned& n, int cell) {
  if (cell == cur) { ++n; return; }
  if (n) atomicAdd(h + cur, n);
  cur = cell; n = 1u;
}

__global__ __launch_bounds__(256) void sweep_hist(HistArgs a) {
  __shared__ unsigned h[4 * 256];
  const HistScene& sc = a.s[blockIdx.y];
  const int tid = threadIdx.x;
  const long long n = (long long)sc.H * sc.W, x0 = (long long)blockIdx.x * 1024;
  if (x0 >= n) return;                           // the whole block: a smaller scene of the chunk
#pragma unroll
  for (int k = 0; k < 4; ++k) h[tid + 256 * k] = 0u;
  __syncthreads();
  int cur0 = 0, cur1 = 0;
  unsigned n0 = 0u, n1 = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long x = x0 + 4 * tid + k;
    if (x >= n) break;
    const int c = sc.cls[x];
    if (c >= a.C) continue;
    const int kind = c == a.positive ? 256 : 0;
    const int p = sc.prob[(size_t)x * a.stride], o = sc.open ? sc.open[x] : p;
    hist_put(h, cur0, n0, kind + p);
    hist_put(h, cur1, n1, 512 + kind + o);
  }
  if (n0) atomicAdd(h + cur0, n0);
  if (n1) atomicAdd(h + cur1, n1);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned v = h[tid + 256 * k];
    if (v) atomicAdd(a.hist + tid + 256 * k, (unsigned long long)v);
  }
}

int sw_check_common(const char* fn, const int32_t* scene_h, const int32_t* scene_w, int nscenes, int pix_stride) {
  RUA_CHECK_ARG(nscenes >= 1, "%s: nscenes %d (>= 1)", fn, nscenes);
  RUA_CHECK_ARG(pix_stride >= 1 && pix_stride <= 64, "%s: pix_stride %d outside 1..64", fn, pix_stride);
  for (int s = 0; s < nscenes; ++s) RG_TRY(rg_check_size(fn, s, scene_h[s], scene_w[s]));
  return RUA_OK;
}

// the bytes a channel of an [H][W][pix_stride] map spans from its first byte to its last
uint64_t sw_prob_bytes(uint64_t n, int pix_stride) { return (n - 1) * (uint64_t)pix_stride + 1; }

}  // namespace

extern "C" int rua_scene_area_open(const uint8_t* const* scene_prob, const int32_t* scene_h, const int32_t* scene_w, int nscenes,
                                   int pix_stride, const uint8_t* levels, int T, int64_t min_area, int connectivity,
                                   uint8_t* const* scene_open, int32_t* const* labels, int32_t* const* areas, void* stream) {
  static const char* const fn = "rua_scene_area_open";
  RUA_CHECK_ARG(scene_prob && scene_h && scene_w && levels && scene_open, "%s: scene_prob, scene_h, scene_w, levels and scene_open are required", fn);
  RUA_CHECK_ARG(T >= 1 && T <= 255, "%s: T %d outside 1..255", fn, T);
  for (int k = 0; k < T; ++k) {
    RUA_CHECK_ARG(levels[k] >= 1, "%s: levels[%d] = %d outside 1..255", fn, k, (int)levels[k]);
    RUA_CHECK_ARG(k == 0 || levels[k] < levels[k - 1], "%s: levels[%d] = %d is not below levels[%d] = %d (strictly descending)", fn, k,
                  (int)levels[k], k - 1, (int)levels[k - 1]);
  }
  RUA_CHECK_ARG(min_area >= 1 && min_area < ((int64_t)1 << 31), "%s: min_area %lld outside 1..2147483647", fn, (long long)min_area);
  RUA_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", fn, connectivity);
  RG_TRY(sw_check_common(fn, scene_h, scene_w, nscenes, pix_stride));
  const bool label = min_area > 1;
  RUA_CHECK_ARG(!label || (labels && areas), "%s: min_area %lld needs the labels and areas work arrays", fn, (long long)min_area);
  std::vector<RgRange> v;
  v.reserve((size_t)nscenes * 4);
  for (int s = 0; s < nscenes; ++s) {
    RUA_CHECK_ARG(scene_prob[s] && scene_open[s] && (!label || (labels[s] && areas[s])), "%s: scene %d: null pointer", fn, s);
    RUA_CHECK_ARG(!label || (((uintptr_t)labels[s] | (uintptr_t)areas[s]) & 3) == 0, "%s: scene %d: labels and areas must be 4-byte aligned", fn, s);
    const uint64_t n = (uint64_t)scene_h[s] * (uint64_t)scene_w[s];
    v.push_back({(uintptr_t)scene_prob[s], sw_prob_bytes(n, pix_stride), s, "scene_prob", false});
    v.push_back({(uintptr_t)scene_open[s], n, s, "scene_open", true});
    if (label) {
      v.push_back({(uintptr_t)labels[s], 4 * n, s, "labels", true});
      v.push_back({(uintptr_t)areas[s], 4 * n, s, "areas", true});
    }
  }
  RG_TRY(rg_check_overlap(fn, v));
  hipStream_t st = (hipStream_t)stream;
  if (!label) {                                  // the largest listed level <= the byte
    TableArgs a;
    memset(&a, 0, sizeof(a));
    a.stride = pix_stride;
    for (int k = T - 1; k >= 0; --k)             // ascending levels: a higher one overwrites from its own value upwards
      for (int b = levels[k]; b < 256; ++b) a.table[b] = levels[k];
    for (int s0 = 0; s0 < nscenes; s0 += SW_TCHUNK) {
      const int ns = nscenes - s0 < SW_TCHUNK ? nscenes - s0 : SW_TCHUNK;
      int64_t pixels = 0;
      for (int k = 0; k < ns; ++k) {
        TableScene& e = a.s[k];
        e.prob = scene_prob[s0 + k]; e.open = scene_open[s0 + k]; e.H = scene_h[s0 + k]; e.W = scene_w[s0 + k];
        pixels = std::max(pixels, (int64_t)e.H * e.W);
      }
      hipLaunchKernelGGL(open_table, dim3((unsigned)((pixels + 255) / 256), ns), dim3(256), 0, st, a);       // below 2^23 blocks
      RUA_LAUNCH_CHECK(fn);
    }
    return RUA_OK;
  }
  OpenArgs a;
  memset(&a, 0, sizeof(a));
  a.stride = pix_stride; a.conn = connectivity; a.min_area = (unsigned)min_area;
  for (int s0 = 0; s0 < nscenes; s0 += SW_CHUNK) {
    const int ns = nscenes - s0 < SW_CHUNK ? nscenes - s0 : SW_CHUNK;
    int64_t tiles = 0, seams = 0, pixels = 0;
    for (int k = 0; k < ns; ++k) {
      const int s = s0 + k;
      OpenScene& e = a.s[k];
      e.prob = scene_prob[s]; e.open = scene_open[s]; e.labels = labels[s]; e.areas = areas[s];
      e.H = scene_h[s]; e.W = scene_w[s];
      const int64_t ty = (e.H - 1) / SW_T + 1, tx = (e.W - 1) / SW_T + 1;
      tiles = std::max(tiles, ty * tx);                                               // below 2^21: H * W < 2^31
      seams = std::max(seams, (ty - 1) * e.W + (tx - 1) * e.H);                       // below 2^27: less than H * W / 16
      pixels = std::max(pixels, (int64_t)e.H * e.W);
    }
    const dim3 per_pixel((unsigned)((pixels + 255) / 256), ns), per_tile((unsigned)tiles, ns);
    hipLaunchKernelGGL(open_zero, per_pixel, dim3(256), 0, st, a);
    for (int k = 0; k < T; ++k) {
      a.level = levels[k];
      hipLaunchKernelGGL(open_tile, per_tile, dim3(256), 0, st, a);
      if (seams) hipLaunchKernelGGL(open_seams, dim3((unsigned)((seams + 255) / 256), ns), dim3(256), 0, st, a);
      hipLaunchKernelGGL(open_flatten, per_tile, dim3(256), 0, st, a);
      hipLaunchKernelGGL(open_settle, per_pixel, dim3(256), 0, st, a);
    }
    RUA_LAUNCH_CHECK(fn);
  }
  return RUA_OK;
}

extern "C" int rua_scene_sweep_hist(const uint8_t* const* scene_prob, const uint8_t* const* scene_open, const uint8_t* const* scene_cls,
                                    const int32_t* scene_h, const int32_t* scene_w, int nscenes, int pix_stride, int positive, int C,
                                    int64_t* hist, void* stream) {
  static const char* const fn = "rua_scene_sweep_hist";
  RUA_CHECK_ARG(scene_prob && scene_cls && scene_h && scene_w && hist, "%s: scene_prob, scene_cls, scene_h, scene_w and hist are required", fn);
  RUA_CHECK_ARG(C >= 1 && C <= 64, "%s: C %d outside 1..64", fn, C);
  RUA_CHECK_ARG(positive >= 0 && positive < C, "%s: positive %d outside 0..%d", fn, positive, C - 1);
  RG_TRY(sw_check_common(fn, scene_h, scene_w, nscenes, pix_stride));
  RUA_CHECK_ARG(((uintptr_t)hist & 7) == 0, "%s: hist must be 8-byte aligned", fn);
  std::vector<RgRange> v;
  v.reserve((size_t)nscenes * 3 + 1);
  for (int s = 0; s < nscenes; ++s) {
    RUA_CHECK_ARG(scene_prob[s] && scene_cls[s] && (!scene_open || scene_open[s]), "%s: scene %d: null pointer", fn, s);
    const uint64_t n = (uint64_t)scene_h[s] * (uint64_t)scene_w[s];
    v.push_back({(uintptr_t)scene_prob[s], sw_prob_bytes(n, pix_stride), s, "scene_prob", false});
    if (scene_open) v.push_back({(uintptr_t)scene_open[s], n, s, "scene_open", false});
    v.push_back({(uintptr_t)scene_cls[s], n, s, "scene_cls", false});
  }
  v.push_back({(uintptr_t)hist, (uint64_t)4 * 256 * sizeof(int64_t), -1, "hist", true});
  RG_TRY(rg_check_overlap(fn, v));
  hipStream_t st = (hipStream_t)stream;
  HistArgs a;
  memset(&a, 0, sizeof(a));
  a.hist = reinterpret_cast<unsigned long long*>(hist);
  a.stride = pix_stride; a.positive = positive; a.C = C;
  for (int s0 = 0; s0 < nscenes; s0 += SW_TCHUNK) {
    const int ns = nscenes - s0 < SW_TCHUNK ? nscenes - s0 : SW_TCHUNK;
    int64_t pixels = 0;
    for (int k = 0; k < ns; ++k) {
      const int s = s0 + k;
      HistScene& e = a.s[k];
      e.prob = scene_prob[s]; e.open = scene_open ? scene_open[s] : nullptr; e.cls = scene_cls[s];
      e.H = scene_h[s]; e.W = scene_w[s];
      pixels = std::max(pixels, (int64_t)e.H * e.W);
    }
    hipLaunchKernelGGL(sweep_hist, dim3((unsigned)((pixels + 1023) / 1024), ns), dim3(256), 0, st, a);       // below 2^21 blocks
    RUA_LAUNCH_CHECK(fn);
  }
  return RUA_OK;
}

// Connected regions of whole class maps and the sieve that removes the small ones (rua_scene_regions, rua_scene_sieve,
// include/rua_hip.h; scenes.host_regions / host_region_counts / host_sieve are the definitions).  A region is a maximal set of
// pixels of equal byte, 4- or 8-connected; its label is its smallest row-major pixel index, its area sits at that root.
//
// Everything is a union-find forest over pixel indices in which a parent is never larger than its child: parent[x] <= x, always.
// A link only ever points a root to a SMALLER index (atomicMin), so the root of a set is its smallest member - the canonical label -
// whatever the order the unions arrive in, and every walk and every retry strictly lowers an index, so it ends (the argument stands
// beside each loop).  No block waits for another: four launches per call, their number independent of the map's content.
//   1. regions_tile: a block labels one RG_T x RG_T tile in LDS.  A row is cut into runs of equal bytes with one wave ballot (a
//      tile row is half a wave), every pixel starts at its run's first pixel, and runs of neighbouring rows are joined by ONE union
//      per pair of touching runs (at the first column they share) instead of one per pixel.  The tile's forest leaves as global
//      indices into `labels`, which is the parent array of the next two launches; `areas` is zeroed.
//   2. regions_seams: a lane per pixel on a tile seam joins it to its equal neighbours across the seam with a lock-free union on
//      the int32 parents in global memory (device-scope atomicMin) - again one union per pair of touching runs along the seam.
//   3. regions_flatten: a block per tile.  Every pixel's parent is either a pixel of its own tile (its tile root, since only roots
//      were ever linked) or it is a tile root linked outside: the pixels are counted per such slot in LDS, row runs first, each
//      occupied slot walks to its root ONCE and adds its count to areas[root] with one atomic - a region that covers a whole tile
//      costs that tile one global atomic -, and every pixel of the tile receives its slot's root.
//   4. regions_count (only with `counts`): every root adds (1, area < min_area, that area) to its class's row, through an LDS
//      histogram and one 64-bit atomic per non-zero cell.
// Loads of a parent that another block may be lowering are relaxed device-scope atomics; a stale parent is still an ancestor of the
// same set (parents only ever move towards the root), so a walk that read one merely takes a step more, and the atomicMin that ends
// a union reports the truth.
//
// The sieve reads a map with its labels and areas.  A pixel is SMALL if its byte c < C, bit c of class_mask is set and
// areas[labels[x]] < min_area.  mode void: one launch, small pixels become 255.  mode fill: every small region takes the class most
// of its kept 4-neighbours have.  The votes of class c are summed per region in a uint32 slot at the region's root (work buffer:
// three uint32 planes of H * W - two vote planes used alternately and the best count so far; 12 bytes per pixel), one launch per
// class: launch c counts the votes for c into plane c & 1 and, at every small root, compares the finished count of class c - 1 in
// the other plane with the best so far (strictly more wins, so a tie stays with the lowest class), writes the winner into out[root]
// and zeroes that plane for launch c + 1.  A last launch copies out[root] to the region's pixels and counts the changed bytes.
// C + 3 launches, whatever the map holds.  A count fits 32 bits: a region with a vote has a kept neighbour region, which is larger
// than it, so it holds fewer than H * W / 2 < 2^30 pixels and casts at most four votes per pixel.
//
// The forest's walks and unions, row_breaks and the overlap check live in unionfind.h, which sweep.hip shares.
#include "unionfind.h"

namespace {

// tests/test_scene_regions_gpu.py sizes its maps by TILE, a copy of RG_T: change them together.
constexpr int RG_T = 32;                       // tile edge in pixels: a tile row is half a wave
constexpr int RG_PIX = RG_T * RG_T;            // 1024 pixels, four per lane of a 256-lane block
constexpr int RG_CHUNK = 120;                  // scenes per launch: 32 bytes each
constexpr int RG_MAXC = 64;

struct RegScene { const uint8_t* map; int32_t* labels; int32_t* areas; int H, W; };
struct RegArgs {
  RegScene s[RG_CHUNK];
  unsigned long long* counts;
  int conn, C, min_area, pad;
};
static_assert(sizeof(RegScene) == 32 && sizeof(RegArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// the tile of a block: false for the whole block when the scene has no such tile (a smaller scene of the chunk)
struct Tile { int i0, j0, th, tw; };
__device__ __forceinline__ bool tile_of(const RegScene& sc, Tile& t) {
  const int tiles_x = (sc.W - 1) / RG_T + 1;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  if (ty > (sc.H - 1) / RG_T) return false;
  t.i0 = ty * RG_T; t.j0 = tx * RG_T;
  t.th = min(RG_T, sc.H - t.i0); t.tw = min(RG_T, sc.W - t.j0);
  return true;
}

__global__ __launch_bounds__(256) void regions_tile(RegArgs a) {
  __shared__ uint8_t B[RG_PIX];                  // the tile's bytes; outside the scene: never read
  __shared__ int P[RG_PIX];                      // parents, as tile indices ly * RG_T + lx
  const RegScene& sc = a.s[blockIdx.y];
  Tile t;
  if (!tile_of(sc, t)) return;
  const int tid = threadIdx.x, W = sc.W, lx = tid & 31;
  const bool in_x = lx < t.tw;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    if (in_x && ly < t.th) B[p] = sc.map[(size_t)(t.i0 + ly) * W + t.j0 + lx];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {                  // every pixel starts below the first pixel of its row run
    const int p = tid + 256 * k, ly = p >> 5;
    const bool valid = in_x && ly < t.th;
    const uint32_t bits = row_breaks(!valid || lx == 0 || B[p - 1] != B[p]);          // bit 0 is always set
    P[p] = (p & ~31) + 31 - __clz(bits & (0xFFFFFFFFu >> (31 - lx)));
  }
  __syncthreads();
  const bool eight = a.conn == 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    if (!in_x || ly >= t.th || ly == 0) continue;
    const int v = B[p], up = p - RG_T;
    const bool left = lx > 0 && B[p - 1] == v, upleft = lx > 0 && B[up - 1] == v, above = B[up] == v;
    // two runs that touch share a first column: there either this run or the one above starts
    if (above && !(left && upleft)) lds_union(P, p, up);
    if (eight) {
      // a diagonal pair needs a union of its own only if neither pixel beside it joins the two runs already
      if (upleft && !above && !left) lds_union(P, p, up - 1);
      if (lx + 1 < t.tw && B[up + 1] == v && !above && B[p + 1] != v) lds_union(P, p, up + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    if (!in_x || ly >= t.th) continue;
    const int r = lds_find(P, p);
    const size_t at = (size_t)(t.i0 + ly) * W + t.j0 + lx;
    sc.labels[at] = (t.i0 + (r >> 5)) * W + t.j0 + (r & 31);
    if (sc.areas) sc.areas[at] = 0;
  }
}

__global__ __launch_bounds__(256) void regions_seams(RegArgs a) {
  const RegScene& sc = a.s[blockIdx.y];
  const int H = sc.H, W = sc.W;
  const int nh = (H - 1) / RG_T, nv = (W - 1) / RG_T;                                 // seams between tile rows, between tile columns
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long across = (long long)nh * W;
  if (e >= across + (long long)nv * H) return;
  const uint8_t* m = sc.map;
  const bool eight = a.conn == 8;
  if (e < across) {                              // pixel (i, j) on the first row of a tile row: its neighbours in row i - 1
    const int i = ((int)(e / W) + 1) * RG_T, j = (int)(e % W);
    const int x = i * W + j, u = x - W;
    const int v = m[x];
    const bool left = j > 0 && m[x - 1] == v, upleft = j > 0 && m[u - 1] == v, above = m[u] == v;
    // the run cut of regions_tile, where the pixels to the left lie in the same tiles: across a tile corner the pair to the left
    // is itself a seam pair that may count on this one
    if (above && !(left && upleft && j % RG_T != 0)) g_union(sc.labels, x, u);
    if (eight) {
      if (upleft && !above && !left) g_union(sc.labels, x, u - 1);
      if (j + 1 < W && m[u + 1] == v && !above && m[x + 1] != v) g_union(sc.labels, x, u + 1);
    }
  } else {                                       // pixel (i, j) on the first column of a tile column: its neighbours in column j - 1
    const long long f = e - across;
    const int j = ((int)(f / H) + 1) * RG_T, i = (int)(f % H);
    const int x = i * W + j;
    const int v = m[x];
    const bool left = m[x - 1] == v, above = i > 0 && m[x - W] == v, upleft = i > 0 && m[x - W - 1] == v;
    if (left && !(above && upleft && i % RG_T != 0)) g_union(sc.labels, x, x - 1);
    if (eight) {
      if (upleft && !above && !left) g_union(sc.labels, x, x - W - 1);
      if (i + 1 < H && m[x + W - 1] == v && !left && m[x + W] != v) g_union(sc.labels, x, x + W - 1);
    }
  }
}

__global__ __launch_bounds__(256) void regions_flatten(RegArgs a) {
  __shared__ int cnt[RG_PIX];                    // pixels of the tile per slot
  __shared__ int root[RG_PIX];                   // the root of an occupied slot
  const RegScene& sc = a.s[blockIdx.y];
  Tile t;
  if (!tile_of(sc, t)) return;
  const int tid = threadIdx.x, W = sc.W, lx = tid & 31;
  const bool in_x = lx < t.tw;
#pragma unroll
  for (int k = 0; k < 4; ++k) cnt[tid + 256 * k] = 0;
  __syncthreads();
  int slot[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    const bool valid = in_x && ly < t.th;
    slot[k] = p;                                 // a tile root that was linked outside the tile stands for itself
    if (valid) {
      const int q = sc.labels[(size_t)(t.i0 + ly) * W + t.j0 + lx];
      const int qi = q / W - t.i0, qj = q % W - t.j0;
      if (qi >= 0 && qi < RG_T && qj >= 0 && qj < RG_T) slot[k] = qi * RG_T + qj;
    }
    // runs of one slot along the row are counted by their first lane: all 64 lanes take part in the shuffle and the ballot
    const int beside = __shfl_up(slot[k], 1);
    const uint32_t bits = row_breaks(!valid || lx == 0 || beside != slot[k]);
    if (valid && ((bits >> lx) & 1u)) {
      const uint32_t rest = (bits >> lx) >> 1;   // the run ends at the next break, or with the row
      atomicAdd(&cnt[slot[k]], rest ? __ffs(rest) : RG_T - lx);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = tid + 256 * k, n = cnt[s];
    if (n == 0) continue;                        // an occupied slot is a pixel of the tile inside the scene
    const int r = g_find(sc.labels, (t.i0 + (s >> 5)) * W + t.j0 + (s & 31));
    root[s] = r;
    if (sc.areas) atomicAdd(sc.areas + r, n);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + 256 * k, ly = p >> 5;
    if (in_x && ly < t.th) sc.labels[(size_t)(t.i0 + ly) * W + t.j0 + lx] = root[slot[k]];
  }
}

__global__ __launch_bounds__(256) void regions_count(RegArgs a) {
  __shared__ unsigned long long hist[3 * RG_MAXC];
  const RegScene& sc = a.s[blockIdx.y];
  const int tid = threadIdx.x, C = a.C;
  const long long n = (long long)sc.H * sc.W, x0 = (long long)blockIdx.x * 1024;
  if (x0 >= n) return;                           // the whole block: a smaller scene of the chunk
  for (int e = tid; e < 3 * C; e += 256) hist[e] = 0ull;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long x = x0 + tid + 256 * k;
    if (x >= n || sc.labels[x] != (int)x) continue;
    const int c = sc.map[x];
    if (c >= C) continue;
    const int area = sc.areas[x];
    atomicAdd(&hist[3 * c], 1ull);
    if (area < a.min_area) {
      atomicAdd(&hist[3 * c + 1], 1ull);
      atomicAdd(&hist[3 * c + 2], (unsigned long long)area);
    }
  }
  __syncthreads();
  for (int e = tid; e < 3 * C; e += 256) {
    const unsigned long long v = hist[e];
    if (v) atomicAdd(a.counts + e, v);
  }
}

// ---- the sieve --------------------------------------------------------------------------------------------------------------------
constexpr int SV_CHUNK = 80;                   // scenes per launch: 48 bytes each

struct SieveScene { const uint8_t* map; const int32_t* labels; const int32_t* areas; uint8_t* out; uint32_t* work; int H, W; };
struct SieveArgs {
  SieveScene s[SV_CHUNK];
  unsigned long long* changed;
  unsigned long long mask;
  int C, min_area, cls, pad;                   // cls: the class whose votes this launch counts (fill)
};
static_assert(sizeof(SieveScene) == 48 && sizeof(SieveArgs) <= 4096, "kernel arguments are limited to 4 KiB");

__device__ __forceinline__ bool sv_small(const SieveScene& sc, const SieveArgs& a, long long x, int c) {
  return c < a.C && ((a.mask >> c) & 1ull) && sc.areas[sc.labels[x]] < a.min_area;
}

// one lane per pixel; false beyond the scene
__device__ __forceinline__ bool sv_pixel(const SieveScene& sc, long long& x) {
  x = (long long)blockIdx.x * 256 + threadIdx.x;
  return x < (long long)sc.H * sc.W;
}

// the block's changed pixels leave with one atomic
__device__ __forceinline__ void sv_changed(const SieveArgs& a, bool changed) {
  __shared__ unsigned int n;
  if (threadIdx.x == 0) n = 0u;
  __syncthreads();
  if (changed) atomicAdd(&n, 1u);
  __syncthreads();
  if (threadIdx.x == 0 && n && a.changed) atomicAdd(a.changed, (unsigned long long)n);
}

__global__ __launch_bounds__(256) void sieve_void(SieveArgs a) {
  const SieveScene& sc = a.s[blockIdx.y];
  long long x;
  bool changed = false;
  if (sv_pixel(sc, x)) {
    const int c = sc.map[x];
    changed = sv_small(sc, a, x, c);
    sc.out[x] = changed ? (uint8_t)255 : (uint8_t)c;
  }
  sv_changed(a, changed);
}

__global__ __launch_bounds__(256) void sieve_fill_init(SieveArgs a) {
  const SieveScene& sc = a.s[blockIdx.y];
  long long x;
  if (!sv_pixel(sc, x)) return;
  sc.out[x] = sc.map[x];
  if (sc.labels[x] != (int)x) return;            // the slots of a root: both vote planes and the best count
  const size_t n = (size_t)sc.H * sc.W;
  sc.work[x] = 0u; sc.work[n + x] = 0u; sc.work[2 * n + x] = 0u;
}

// launch cls = 0 .. C: the votes for class cls (cls < C) and the verdict on class cls - 1 (cls > 0)
__global__ __launch_bounds__(256) void sieve_fill_vote(SieveArgs a) {
  const SieveScene& sc = a.s[blockIdx.y];
  long long x;
  if (!sv_pixel(sc, x)) return;
  const int v = sc.map[x], cls = a.cls;
  if (!sv_small(sc, a, x, v)) return;
  const int r = sc.labels[x], W = sc.W;
  const size_t n = (size_t)sc.H * W;
  if (cls > 0 && r == (int)x) {
    uint32_t* done = sc.work + (size_t)((cls - 1) & 1) * n + x;
    const uint32_t votes = *done;
    if (votes) {
      if (votes > sc.work[2 * n + x]) { sc.work[2 * n + x] = votes; sc.out[x] = (uint8_t)(cls - 1); }
      *done = 0u;
    }
  }
  if (cls >= a.C || cls == v) return;            // a neighbour of the region's own byte is the region itself
  const int i = (int)(x / W), j = (int)(x - (long long)i * W);
  int k = 0;
  if (i > 0 && sc.map[x - W] == cls && !sv_small(sc, a, x - W, cls)) ++k;
  if (i + 1 < sc.H && sc.map[x + W] == cls && !sv_small(sc, a, x + W, cls)) ++k;
  if (j > 0 && sc.map[x - 1] == cls && !sv_small(sc, a, x - 1, cls)) ++k;
  if (j + 1 < W && sc.map[x + 1] == cls && !sv_small(sc, a, x + 1, cls)) ++k;
  if (k) atomicAdd(sc.work + (size_t)(cls & 1) * n + r, (uint32_t)k);
}

__global__ __launch_bounds__(256) void sieve_fill_apply(SieveArgs a) {
  const SieveScene& sc = a.s[blockIdx.y];
  long long x;
  bool changed = false;
  if (sv_pixel(sc, x)) {
    const int v = sc.map[x];
    if (sv_small(sc, a, x, v)) {                 // a root holds its region's verdict since the last vote launch and is not written here
      const int r = sc.labels[x];
      const uint8_t w = sc.out[r];
      if (r != (int)x) sc.out[x] = w;
      changed = w != v;
    }
  }
  sv_changed(a, changed);
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------
int rg_check_params(const char* fn, int connectivity, int64_t min_area, int C) {
  RUA_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", fn, connectivity);
  RUA_CHECK_ARG(min_area >= 1 && min_area < ((int64_t)1 << 31), "%s: min_area %lld outside 1..2147483647", fn, (long long)min_area);
  RUA_CHECK_ARG(C >= 1 && C <= RG_MAXC, "%s: C %d outside 1..64", fn, C);
  return RUA_OK;
}

}  // namespace

extern "C" int rua_scene_regions(const uint8_t* const* scene_map, const int32_t* scene_h, const int32_t* scene_w, int nscenes,
                                 int connectivity, int32_t* const* labels, int32_t* const* areas, int64_t min_area, int C,
                                 int64_t* counts, void* stream) {
  static const char* const fn = "rua_scene_regions";
  RUA_CHECK_ARG(scene_map && scene_h && scene_w && labels, "%s: scene_map, scene_h, scene_w and labels are required", fn);
  RUA_CHECK_ARG(nscenes >= 1, "%s: nscenes %d (>= 1)", fn, nscenes);
  RG_TRY(rg_check_params(fn, connectivity, counts ? min_area : 1, counts ? C : 1));
  RUA_CHECK_ARG(!counts || areas, "%s: counts needs areas (a region is small by its area)", fn);
  RUA_CHECK_ARG(((uintptr_t)counts & 7) == 0, "%s: counts must be 8-byte aligned", fn);
  std::vector<RgRange> v;
  v.reserve((size_t)nscenes * 3 + 1);
  for (int s = 0; s < nscenes; ++s) {
    RUA_CHECK_ARG(scene_map[s] && labels[s] && (!areas || areas[s]), "%s: scene %d: null pointer", fn, s);
    RG_TRY(rg_check_size(fn, s, scene_h[s], scene_w[s]));
    RUA_CHECK_ARG((((uintptr_t)labels[s] | (uintptr_t)(areas ? areas[s] : nullptr)) & 3) == 0, "%s: scene %d: labels and areas must be 4-byte aligned", fn, s);
    const uint64_t n = (uint64_t)scene_h[s] * (uint64_t)scene_w[s];
    v.push_back({(uintptr_t)scene_map[s], n, s, "scene_map", false});
    v.push_back({(uintptr_t)labels[s], 4 * n, s, "labels", true});
    if (areas) v.push_back({(uintptr_t)areas[s], 4 * n, s, "areas", true});
  }
  if (counts) v.push_back({(uintptr_t)counts, (uint64_t)C * 3 * sizeof(int64_t), -1, "counts", true});
  RG_TRY(rg_check_overlap(fn, v));
  hipStream_t st = (hipStream_t)stream;
  RegArgs a;
  memset(&a, 0, sizeof(a));
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.conn = connectivity; a.C = counts ? C : 0; a.min_area = counts ? (int)min_area : 0;
  for (int s0 = 0; s0 < nscenes; s0 += RG_CHUNK) {
    const int ns = nscenes - s0 < RG_CHUNK ? nscenes - s0 : RG_CHUNK;
    int64_t tiles = 0, seams = 0, pixels = 0;
    for (int k = 0; k < ns; ++k) {
      const int s = s0 + k;
      RegScene& e = a.s[k];
      e.map = scene_map[s]; e.labels = labels[s]; e.areas = areas ? areas[s] : nullptr;
      e.H = scene_h[s]; e.W = scene_w[s];
      const int64_t ty = (e.H - 1) / RG_T + 1, tx = (e.W - 1) / RG_T + 1;
      tiles = std::max(tiles, ty * tx);                                               // below 2^21: H * W < 2^31
      seams = std::max(seams, (ty - 1) * e.W + (tx - 1) * e.H);                       // below 2^27: less than H * W / 16
      pixels = std::max(pixels, (int64_t)e.H * e.W);
    }
    hipLaunchKernelGGL(regions_tile, dim3((unsigned)tiles, ns), dim3(256), 0, st, a);
    if (seams) hipLaunchKernelGGL(regions_seams, dim3((unsigned)((seams + 255) / 256), ns), dim3(256), 0, st, a);
    hipLaunchKernelGGL(regions_flatten, dim3((unsigned)tiles, ns), dim3(256), 0, st, a);
    if (counts) hipLaunchKernelGGL(regions_count, dim3((unsigned)((pixels + 1023) / 1024), ns), dim3(256), 0, st, a);
    RUA_LAUNCH_CHECK(fn);
  }
  return RUA_OK;
}

extern "C" int64_t rua_scene_sieve_work_bytes(int H, int W, int C) {
  if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || C < 1 || C > RG_MAXC) return -1;
  return (int64_t)H * W * 12;
}

extern "C" int rua_scene_sieve(const uint8_t* const* scene_map, const int32_t* scene_h, const int32_t* scene_w, int nscenes,
                               int connectivity, int64_t min_area, int C, uint64_t class_mask, int mode, const int32_t* const* labels,
                               const int32_t* const* areas, uint8_t* const* scene_out, void* work, int64_t work_bytes,
                               int64_t* changed, void* stream) {
  static const char* const fn = "rua_scene_sieve";
  RUA_CHECK_ARG(scene_map && scene_h && scene_w && labels && areas && scene_out, "%s: scene_map, scene_h, scene_w, labels, areas and scene_out are required", fn);
  RUA_CHECK_ARG(nscenes >= 1, "%s: nscenes %d (>= 1)", fn, nscenes);
  RG_TRY(rg_check_params(fn, connectivity, min_area, C));
  RUA_CHECK_ARG(mode == RUA_SIEVE_VOID || mode == RUA_SIEVE_FILL, "%s: mode %d is neither void (0) nor fill (1)", fn, mode);
  RUA_CHECK_ARG(C == 64 || (class_mask >> C) == 0, "%s: class_mask 0x%llx names a class outside 0..%d", fn, (unsigned long long)class_mask, C - 1);
  RUA_CHECK_ARG(((uintptr_t)changed & 7) == 0, "%s: changed must be 8-byte aligned", fn);
  const bool fill = mode == RUA_SIEVE_FILL;
  std::vector<RgRange> v;
  v.reserve((size_t)nscenes * 4 + 2);
  int64_t need = 0;
  for (int s = 0; s < nscenes; ++s) {
    RUA_CHECK_ARG(scene_map[s] && labels[s] && areas[s] && scene_out[s], "%s: scene %d: null pointer", fn, s);
    RG_TRY(rg_check_size(fn, s, scene_h[s], scene_w[s]));
    RUA_CHECK_ARG((((uintptr_t)labels[s] | (uintptr_t)areas[s]) & 3) == 0, "%s: scene %d: labels and areas must be 4-byte aligned", fn, s);
    const uint64_t n = (uint64_t)scene_h[s] * (uint64_t)scene_w[s];
    need += (int64_t)n * 12;
    v.push_back({(uintptr_t)scene_map[s], n, s, "scene_map", false});
    v.push_back({(uintptr_t)labels[s], 4 * n, s, "labels", false});
    v.push_back({(uintptr_t)areas[s], 4 * n, s, "areas", false});
    v.push_back({(uintptr_t)scene_out[s], n, s, "scene_out", true});
  }
  if (fill) {
    RUA_CHECK_ARG(work && ((uintptr_t)work & 3) == 0, "%s: mode fill needs a 4-byte aligned work buffer (rua_scene_sieve_work_bytes per scene)", fn);
    RUA_CHECK_ARG(work_bytes >= need, "%s: work_bytes %lld, the scenes need %lld (rua_scene_sieve_work_bytes of each, summed)", fn, (long long)work_bytes, (long long)need);
    v.push_back({(uintptr_t)work, (uint64_t)need, -1, "work", true});
  }
  if (changed) v.push_back({(uintptr_t)changed, sizeof(int64_t), -1, "changed", true});
  RG_TRY(rg_check_overlap(fn, v));
  hipStream_t st = (hipStream_t)stream;
  SieveArgs a;
  memset(&a, 0, sizeof(a));
  a.changed = reinterpret_cast<unsigned long long*>(changed);
  a.mask = class_mask; a.C = C; a.min_area = (int)min_area;
  uint32_t* wk = static_cast<uint32_t*>(work);
  for (int s0 = 0; s0 < nscenes; s0 += SV_CHUNK) {
    const int ns = nscenes - s0 < SV_CHUNK ? nscenes - s0 : SV_CHUNK;
    int64_t pixels = 0;
    for (int k = 0; k < ns; ++k) {
      const int s = s0 + k;
      SieveScene& e = a.s[k];
      e.map = scene_map[s]; e.labels = labels[s]; e.areas = areas[s]; e.out = scene_out[s];
      e.H = scene_h[s]; e.W = scene_w[s];
      const int64_t n = (int64_t)e.H * e.W;
      e.work = fill ? wk : nullptr;
      if (fill) wk += 3 * n;
      pixels = std::max(pixels, n);
    }
    const dim3 grid((unsigned)((pixels + 255) / 256), ns);                            // below 2^23 blocks
    if (!fill) {
      hipLaunchKernelGGL(sieve_void, grid, dim3(256), 0, st, a);
    } else {
      hipLaunchKernelGGL(sieve_fill_init, grid, dim3(256), 0, st, a);
      for (int c = 0; c <= C; ++c) {
        a.cls = c;
        hipLaunchKernelGGL(sieve_fill_vote, grid, dim3(256), 0, st, a);
      }
      hipLaunchKernelGGL(sieve_fill_apply, grid, dim3(256), 0, st, a);
    }
    RUA_LAUNCH_CHECK(fn);
  }
  return RUA_OK;
}

// Instances from whole-scene maps (rua_scene_seed_map, rua_scene_instances, rua_scene_instance_match, include/rua_hip.h;
// scenes.host_seed_map / host_instances / host_instance_match are the definitions).  One scene per call: ids and tables are per scene.
//
// Seed map: one streaming pass.  marker[x] = cls[x] where the class is chosen, the boundary byte of that class is below bound_below
// and its distance byte at least dist_at_least; 255 elsewhere.
//
// Instances read the marker with the labels and areas rua_scene_regions wrote for it.  A SEED is a region of the marker with a byte
// c < C and at least min_seed pixels; seeds are numbered 0..N-1 in ascending order of their root.  Four launches, their number
// independent of the map's content, no block ever waits for another:
//   1. inst_count: a block per chunk of 1024 pixels counts the chunk's qualifying roots.
//   2. inst_scan: ONE block turns the chunk counts into exclusive offsets, 256 chunks per pass with a carry (ceil(chunks / 256)
//      passes: 138 for a 6000 x 6000 scene), and writes N and a zero for `ungrown`.
//   3. inst_number: a block per chunk ranks its roots in index order (a lane holds four consecutive pixels, the lanes are scanned in
//      LDS), writes each root's id into the work plane and, for ids below max_instances, the fixed columns of its table row.
//   4. inst_grow: a block per 32 x 32 tile stages the seed ids and marker bytes of the tile and a halo of `radius` pixels in LDS -
//      (32 + 2 radius)^2 entries of 5 bytes, 46080 bytes at radius 16 - and every eligible pixel takes the exact minimum of
//      (d^2 << 32) | id over the disc (at most (2 radius + 1)^2 <= 1089 steps; a seed pixel of its own class ends at once with its
//      own id).  inst is written, the tile's unassigned eligible pixels leave with one atomic, and the table takes area and bounding
//      box per run of equal ids along a tile row (integer atomicAdd / atomicMin / atomicMax: the result does not depend on order);
//      the runs of the tile's largest id collect in LDS and reach the table once per tile, so a tile inside one large instance
//      costs that instance's row five global atomics (a 6000 x 6000 map that is one instance: 64 ms without, 2.3 ms with).
//
// Match: the exact strict majority without a hash table or a sort.  votes[P][b] counts the pixels of predicted instance P whose
// ground-truth id has bit b set; the candidate is assembled from the bits with 2 votes > area_P; a second pass counts the pixels
// of P on exactly that candidate; the last writes (cand, inter) if 2 inter > area_P.  If a strict-majority id exists, each of its
// set bits collects more than half of P's pixels and each unset bit fewer, so the candidate is that id; if none exists the
// verification rejects whatever the bits spelled.  One atomic per run of equal (P, g) along the row-major order inside a wave; the runs
// of the instance at a block's first pixel collect in LDS first.
#include "unionfind.h"
#include <climits>

namespace {

constexpr int IN_T = 32;                       // tile edge of the grow kernel: a tile row is half a wave
constexpr int IN_CHUNK = 1024;                 // pixels per chunk of the seed numbering
constexpr int IN_MAXR = 16;                    // the largest radius, as rua_scene_erode's
constexpr int IN_MAXC = 64;

struct InstArgs {
  const uint8_t* cls; const uint8_t* marker; const int32_t* labels; const int32_t* areas;
  int32_t* ids;                                // work: the seed id at every qualifying root
  int32_t* chunk;                              // work: qualifying roots per chunk, then their exclusive prefix
  int32_t* inst; int32_t* table; int32_t* n;
  unsigned long long mask;
  int H, W, C, min_seed, radius, max_instances, chunks;
};

__device__ __forceinline__ bool in_seed_root(const InstArgs& a, long long x) {
  return a.labels[x] == (int)x && a.marker[x] < a.C && a.areas[x] >= a.min_seed;
}

__global__ __launch_bounds__(256) void inst_count(InstArgs a) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const long long n = (long long)a.H * a.W, x0 = (long long)blockIdx.x * IN_CHUNK + threadIdx.x * 4;
  int k = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (x0 + e < n && in_seed_root(a, x0 + e)) ++k;
  if (k) atomicAdd(&cnt, k);
  __syncthreads();
  if (threadIdx.x == 0) a.chunk[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(256) void inst_scan(InstArgs a) {
  __shared__ int sh[256];
  int carry = 0;
  for (int c0 = 0; c0 < a.chunks; c0 += 256) {   // ceil(chunks / 256) passes
    const int c = c0 + threadIdx.x;
    const int v = c < a.chunks ? a.chunk[c] : 0;
    int total;
    const int ex = block_scan_256(sh, v, total);
    if (c < a.chunks) a.chunk[c] = carry + ex;
    carry += total;                              // below H * W < 2^31
  }
  if (threadIdx.x == 0) { a.n[0] = carry; a.n[1] = 0; }
}

__global__ __launch_bounds__(256) void inst_number(InstArgs a) {
  __shared__ int sh[256];
  const int t = threadIdx.x;
  const long long n = (long long)a.H * a.W, x0 = (long long)blockIdx.x * IN_CHUNK + t * 4;
  bool q[4];
  int k = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) { q[e] = x0 + e < n && in_seed_root(a, x0 + e); k += q[e]; }
  int total;
  int id = a.chunk[blockIdx.x] + block_scan_256(sh, k, total);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!q[e]) continue;
    const long long x = x0 + e;
    a.ids[x] = id;
    if (id < a.max_instances) {
      int32_t* row = a.table + (size_t)id * 8;
      row[0] = (int)x; row[1] = a.marker[x]; row[2] = 0; row[3] = a.areas[x];
      row[4] = a.H; row[5] = a.W; row[6] = -1; row[7] = -1;
    }
    ++id;
  }
}

__global__ __launch_bounds__(256) void inst_grow(InstArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int lim[2 * IN_MAXR + 1];           // the half-width of the disc in row dy
  __shared__ unsigned int ungrown;
  __shared__ int dom, agg[5];                    // the tile's largest id, and its area and box inside the tile
  const int r = a.radius, S = IN_T + 2 * r, H = a.H, W = a.W, tid = threadIdx.x;
  int* sid = reinterpret_cast<int*>(lds);                        // S * S seed ids, -1 where there is no seed pixel
  uint8_t* smk = lds + (size_t)S * S * 4;                        // S * S marker bytes, 255 where there is no seed pixel
  const int tiles_x = (W - 1) / IN_T + 1;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i0 = ty * IN_T, j0 = tx * IN_T;
  if (tid == 0) { ungrown = 0u; dom = -1; agg[0] = 0; agg[1] = INT_MAX; agg[2] = INT_MAX; agg[3] = -1; agg[4] = -1; }
  if (tid <= 2 * r) {
    const int dy = tid - r, rest = r * r - dy * dy;
    int l = 0;
    while ((l + 1) * (l + 1) <= rest) ++l;       // at most 16 steps
    lim[tid] = l;
  }
  for (int e = tid; e < S * S; e += 256) {       // at most 96 * 96 / 256 = 36 rounds
    const int ly = e / S, lx = e - ly * S;
    const int i = i0 - r + ly, j = j0 - r + lx;
    int id = -1, mk = 255;
    if (i >= 0 && i < H && j >= 0 && j < W) {
      const size_t y = (size_t)i * W + j;
      const int m = a.marker[y];
      if (m < a.C) {
        const int root = a.labels[y];
        if (a.areas[root] >= a.min_seed) { id = a.ids[root]; mk = m; }
      }
    }
    sid[e] = id; smk[e] = (uint8_t)mk;
  }
  __syncthreads();
  const int lx = tid & 31;
  int mine = 0, top = -1, ids4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = (tid >> 5) + 8 * k;
    const int i = i0 + ly, j = j0 + lx;
    int got = -1;
    if (i < H && j < W) {
      const size_t x = (size_t)i * W + j;
      const int c = a.cls[x];
      if (c < a.C && ((a.mask >> c) & 1ull)) {
        const int at = (ly + r) * S + lx + r;
        if (smk[at] == c) {
          got = sid[at];                         // distance 0: nothing is nearer, and one pixel holds one id
        } else {
          unsigned long long best = ~0ull;
          for (int dy = -r; dy <= r; ++dy) {     // (2 r + 1) rows of at most (2 r + 1) pixels
            const int l = lim[dy + r], base = at + dy * S;
            for (int dx = -l; dx <= l; ++dx) {
              if (smk[base + dx] != c) continue;
              const unsigned long long key = ((unsigned long long)(dy * dy + dx * dx) << 32) | (unsigned int)sid[base + dx];
              best = key < best ? key : best;
            }
          }
          if (best != ~0ull) got = (int)(unsigned int)best;
          else ++mine;
        }
      }
      a.inst[x] = got;
    }
    ids4[k] = got;
    top = got > top ? got : top;
  }
  if (top >= 0) atomicMax(&dom, top);
  __syncthreads();
  // the table: one set of atomics per run of equal ids along the tile row - into LDS for the runs of ONE id of the tile (the largest:
  // a tile inside a large instance then costs the table five global atomics, not five per row), into the table for the others.
  // All 64 lanes take part in the shuffle and the ballot.
  const int d = dom;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = (tid >> 5) + 8 * k;
    const int i = i0 + ly, j = j0 + lx, got = ids4[k];
    const bool valid = i < H && j < W;
    const int beside = __shfl_up(got, 1);
    const uint32_t bits = row_breaks(!valid || lx == 0 || beside != got);
    if (valid && got >= 0 && got < a.max_instances && ((bits >> lx) & 1u)) {
      const uint32_t rest = (bits >> lx) >> 1;
      const int len = rest ? __ffs(rest) : IN_T - lx;
      if (got == d) {
        atomicAdd(&agg[0], len);
        atomicMin(&agg[1], i); atomicMin(&agg[2], j);
        atomicMax(&agg[3], i); atomicMax(&agg[4], j + len - 1);
      } else {
        int32_t* row = a.table + (size_t)got * 8;
        atomicAdd(row + 2, len);
        atomicMin(row + 4, i); atomicMin(row + 5, j);
        atomicMax(row + 6, i); atomicMax(row + 7, j + len - 1);
      }
    }
  }
  if (mine) atomicAdd(&ungrown, (unsigned int)mine);
  __syncthreads();
  if (tid == 0 && ungrown) atomicAdd(a.n + 1, (int)ungrown);
  if (tid == 0 && agg[0] > 0) {                  // only runs below max_instances were added
    int32_t* row = a.table + (size_t)d * 8;
    atomicAdd(row + 2, agg[0]);
    atomicMin(row + 4, agg[1]); atomicMin(row + 5, agg[2]);
    atomicMax(row + 6, agg[3]); atomicMax(row + 7, agg[4]);
  }
}

__global__ __launch_bounds__(256) void seed_map_kernel(const uint8_t* cls, const uint8_t* bound, const uint8_t* dist, long long n, int C,
                                                       unsigned long long mask, int bound_below, int dist_at_least, uint8_t* marker) {
  const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  const int c = cls[x];
  bool keep = c < C && ((mask >> c) & 1ull);
  if (keep && bound) keep = bound[(size_t)x * C + c] < bound_below;
  if (keep && dist) keep = dist[(size_t)x * C + c] >= dist_at_least;
  marker[x] = keep ? (uint8_t)c : (uint8_t)255;
}

// ---- the match --------------------------------------------------------------------------------------------------------------------
struct MatchArgs {
  const int32_t* inst_p; const int32_t* inst_g; const int32_t* area_p;
  int32_t* votes; int32_t* cand; int32_t* inter; int32_t* match;
  long long n;
  int Np, Ng, bits, pad;
};

// this lane's pixel starts a run of equal (P, g) inside its wave: the run's length, 0 for every other lane.  All 64 lanes call it.
__device__ __forceinline__ int run_length(int P, int g) {
  const int lane = threadIdx.x & 63;
  const int bp = __shfl_up(P, 1), bg = __shfl_up(g, 1);
  const bool head = lane == 0 || bp != P || bg != g;
  const unsigned long long m = __ballot(head);
  if (!head) return 0;
  const unsigned long long rest = lane == 63 ? 0ull : m >> (lane + 1);
  return rest ? __ffsll(rest) : 64 - lane;
}

// the votes, candidates and intersections start at zero: a kernel, so that a captured graph would hold no memset node
__global__ __launch_bounds__(256) void match_zero(int32_t* work, long long n) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) work[e] = 0;
}

// the pair of pixel x: (-1, -1) beyond the map and where either id is no instance
__device__ __forceinline__ void match_pair(const MatchArgs& a, long long x, int& P, int& g) {
  P = -1; g = -1;
  if (x < a.n) {
    P = a.inst_p[x]; g = a.inst_g[x];
    if (P < 0 || P >= a.Np || g < 0 || g >= a.Ng) { P = -1; g = -1; }
  }
}

// A block counts MT_SPAN consecutive pixels.  The runs of ONE predicted instance - that of the block's first pixel - are summed in
// LDS and leave with one atomic per bit and block: inside a large instance a block then costs its row `bits` global atomics, not
// `bits` per run.  The runs of every other instance go to the table directly.
constexpr int MT_SPAN = 4096;

__global__ __launch_bounds__(256) void match_votes(MatchArgs a) {
  __shared__ int sum[32];
  const long long x0 = (long long)blockIdx.x * MT_SPAN;
  if (threadIdx.x < 32) sum[threadIdx.x] = 0;
  int P0, g0;
  match_pair(a, x0, P0, g0);
  __syncthreads();
  for (int it = 0; it < MT_SPAN / 256; ++it) {   // 16 rounds, every lane in each
    int P, g;
    match_pair(a, x0 + it * 256 + threadIdx.x, P, g);
    const int len = run_length(P, g);
    if (len == 0 || P < 0) continue;
    int32_t* v = P == P0 ? sum : a.votes + (size_t)P * a.bits;
    for (int b = 0; b < a.bits; ++b)             // bits <= 31
      if ((g >> b) & 1) atomicAdd(v + b, len);
  }
  __syncthreads();
  if (P0 >= 0 && threadIdx.x < a.bits && sum[threadIdx.x]) atomicAdd(a.votes + (size_t)P0 * a.bits + threadIdx.x, sum[threadIdx.x]);
}

__global__ __launch_bounds__(256) void match_cand(MatchArgs a) {
  const int P = blockIdx.x * 256 + threadIdx.x;
  if (P >= a.Np) return;
  const long long area = a.area_p[(size_t)P * 8];
  const int32_t* v = a.votes + (size_t)P * a.bits;
  int c = 0;
  for (int b = 0; b < a.bits; ++b)
    if (2ll * v[b] > area) c |= 1 << b;
  a.cand[P] = c;
}

__global__ __launch_bounds__(256) void match_inter(MatchArgs a) {
  __shared__ int sum;
  const long long x0 = (long long)blockIdx.x * MT_SPAN;
  if (threadIdx.x == 0) sum = 0;
  int P0, g0;
  match_pair(a, x0, P0, g0);
  __syncthreads();
  for (int it = 0; it < MT_SPAN / 256; ++it) {   // 16 rounds, every lane in each
    int P, g;
    match_pair(a, x0 + it * 256 + threadIdx.x, P, g);
    const int len = run_length(P, g);
    if (len == 0 || P < 0 || a.cand[P] != g) continue;
    atomicAdd(P == P0 ? &sum : a.inter + P, len);
  }
  __syncthreads();
  if (threadIdx.x == 0 && P0 >= 0 && sum) atomicAdd(a.inter + P0, sum);
}

__global__ __launch_bounds__(256) void match_write(MatchArgs a) {
  const int P = blockIdx.x * 256 + threadIdx.x;
  if (P >= a.Np) return;
  const long long area = a.area_p[(size_t)P * 8];
  const int c = a.cand[P], k = a.inter[P];
  const bool ok = c < a.Ng && 2ll * k > area;
  a.match[2 * (size_t)P] = ok ? c : -1;
  a.match[2 * (size_t)P + 1] = ok ? k : 0;
}

int bit_length(int64_t v) {                      // of v >= 0
  int b = 0;
  while (v > 0) { ++b; v >>= 1; }
  return b;
}

int in_check_map(const char* fn, int H, int W, int C, uint64_t class_mask) {
  RUA_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31), "%s: size %d x %d (H * W < 2^31: an id is an int32)", fn, H, W);
  RUA_CHECK_ARG(C >= 1 && C <= IN_MAXC, "%s: C %d outside 1..64", fn, C);
  RUA_CHECK_ARG(C == 64 || (class_mask >> C) == 0, "%s: class_mask 0x%llx names a class outside 0..%d", fn, (unsigned long long)class_mask, C - 1);
  return RUA_OK;
}

int64_t in_chunks(int H, int W) { return ((int64_t)H * W + IN_CHUNK - 1) / IN_CHUNK; }

}  // namespace

extern "C" int rua_scene_seed_map(const uint8_t* cls, const uint8_t* bound, const uint8_t* dist, int H, int W, int C, uint64_t class_mask,
                                  int bound_below, int dist_at_least, uint8_t* marker, void* stream) {
  static const char* const fn = "rua_scene_seed_map";
  RUA_CHECK_ARG(cls && marker, "%s: cls and marker are required", fn);
  RG_TRY(in_check_map(fn, H, W, C, class_mask));
  RUA_CHECK_ARG(bound_below >= 1 && bound_below <= 256, "%s: bound_below %d outside 1..256", fn, bound_below);
  RUA_CHECK_ARG(dist_at_least >= 0 && dist_at_least <= 255, "%s: dist_at_least %d outside 0..255", fn, dist_at_least);
  const uint64_t n = (uint64_t)H * (uint64_t)W;
  std::vector<RgRange> v;
  v.push_back({(uintptr_t)cls, n, -1, "cls", false});
  if (bound) v.push_back({(uintptr_t)bound, n * C, -1, "bound", false});
  if (dist) v.push_back({(uintptr_t)dist, n * C, -1, "dist", false});
  v.push_back({(uintptr_t)marker, n, -1, "marker", true});
  RG_TRY(rg_check_overlap(fn, v));
  hipLaunchKernelGGL(seed_map_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cls, bound, dist, (long long)n, C,
                     (unsigned long long)class_mask, bound_below, dist_at_least, marker);
  RUA_LAUNCH_CHECK(fn);
  return RUA_OK;
}

extern "C" int64_t rua_scene_instances_work_bytes(int H, int W) {
  if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return -1;
  return ((int64_t)H * W + in_chunks(H, W)) * 4;
}

extern "C" int rua_scene_instances(const uint8_t* cls, const uint8_t* marker, const int32_t* labels, const int32_t* areas, int H, int W, int C,
                                   uint64_t class_mask, int64_t min_seed, int radius, void* work, int64_t work_bytes, int32_t* inst,
                                   int32_t* table, int64_t max_instances, int32_t* n, void* stream) {
  static const char* const fn = "rua_scene_instances";
  RUA_CHECK_ARG(cls && marker && labels && areas && inst && table && n, "%s: cls, marker, labels, areas, inst, table and n are required", fn);
  RG_TRY(in_check_map(fn, H, W, C, class_mask));
  RUA_CHECK_ARG(min_seed >= 1 && min_seed < ((int64_t)1 << 31), "%s: min_seed %lld outside 1..2147483647", fn, (long long)min_seed);
  RUA_CHECK_ARG(radius >= 0 && radius <= IN_MAXR, "%s: radius %d outside 0..16", fn, radius);
  RUA_CHECK_ARG(max_instances >= 1 && max_instances < ((int64_t)1 << 31), "%s: max_instances %lld outside 1..2147483647", fn, (long long)max_instances);
  RUA_CHECK_ARG((((uintptr_t)labels | (uintptr_t)areas | (uintptr_t)inst | (uintptr_t)table | (uintptr_t)n) & 3) == 0,
                "%s: labels, areas, inst, table and n must be 4-byte aligned", fn);
  const int64_t need = rua_scene_instances_work_bytes(H, W);
  RUA_CHECK_ARG(work && ((uintptr_t)work & 3) == 0, "%s: a 4-byte aligned work buffer is required (rua_scene_instances_work_bytes)", fn);
  RUA_CHECK_ARG(work_bytes >= need, "%s: work_bytes %lld, the scene needs %lld (rua_scene_instances_work_bytes)", fn, (long long)work_bytes, (long long)need);
  const uint64_t px = (uint64_t)H * (uint64_t)W;
  std::vector<RgRange> v;
  v.push_back({(uintptr_t)cls, px, -1, "cls", false});
  v.push_back({(uintptr_t)marker, px, -1, "marker", false});
  v.push_back({(uintptr_t)labels, 4 * px, -1, "labels", false});
  v.push_back({(uintptr_t)areas, 4 * px, -1, "areas", false});
  v.push_back({(uintptr_t)work, (uint64_t)need, -1, "work", true});
  v.push_back({(uintptr_t)inst, 4 * px, -1, "inst", true});
  v.push_back({(uintptr_t)table, (uint64_t)max_instances * 32, -1, "table", true});
  v.push_back({(uintptr_t)n, 8, -1, "n", true});
  RG_TRY(rg_check_overlap(fn, v));
  hipStream_t st = (hipStream_t)stream;
  InstArgs a;
  memset(&a, 0, sizeof(a));
  a.cls = cls; a.marker = marker; a.labels = labels; a.areas = areas;
  a.ids = static_cast<int32_t*>(work); a.chunk = a.ids + px;
  a.inst = inst; a.table = table; a.n = n;
  a.mask = class_mask;
  a.H = H; a.W = W; a.C = C; a.min_seed = (int)min_seed; a.radius = radius; a.max_instances = (int)max_instances;
  a.chunks = (int)in_chunks(H, W);                                                     // below 2^21
  const int S = IN_T + 2 * radius;
  const unsigned tiles = (unsigned)(((H - 1) / IN_T + 1) * (int64_t)((W - 1) / IN_T + 1));  // below 2^21
  hipLaunchKernelGGL(inst_count, dim3((unsigned)a.chunks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(inst_scan, dim3(1), dim3(256), 0, st, a);
  hipLaunchKernelGGL(inst_number, dim3((unsigned)a.chunks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(inst_grow, dim3(tiles), dim3(256), (size_t)S * S * 5, st, a);
  RUA_LAUNCH_CHECK(fn);
  return RUA_OK;
}

extern "C" int64_t rua_scene_instance_match_work_bytes(int64_t Np, int64_t Ng) {
  if (Np < 0 || Ng < 0 || Np >= ((int64_t)1 << 31) || Ng >= ((int64_t)1 << 31)) return -1;
  return Np * (bit_length(Ng > 0 ? Ng - 1 : 0) + 2) * 4;
}

extern "C" int rua_scene_instance_match(const int32_t* inst_p, const int32_t* area_p, int64_t Np, const int32_t* inst_g, int64_t Ng, int H, int W,
                                        void* work, int64_t work_bytes, int32_t* match, void* stream) {
  static const char* const fn = "rua_scene_instance_match";
  RUA_CHECK_ARG(inst_p && inst_g, "%s: inst_p and inst_g are required", fn);
  RUA_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31), "%s: size %d x %d (H * W < 2^31: an id is an int32)", fn, H, W);
  RUA_CHECK_ARG(Np >= 0 && Np < ((int64_t)1 << 31), "%s: Np %lld outside 0..2147483647", fn, (long long)Np);
  RUA_CHECK_ARG(Ng >= 0 && Ng < ((int64_t)1 << 31), "%s: Ng %lld outside 0..2147483647", fn, (long long)Ng);
  RUA_CHECK_ARG((((uintptr_t)inst_p | (uintptr_t)inst_g | (uintptr_t)area_p | (uintptr_t)match | (uintptr_t)work) & 3) == 0,
                "%s: inst_p, inst_g, area_p, match and work must be 4-byte aligned", fn);
  const int64_t need = rua_scene_instance_match_work_bytes(Np, Ng);
  if (Np > 0) {
    RUA_CHECK_ARG(area_p && match && work, "%s: area_p, match and work are required with Np > 0", fn);
    RUA_CHECK_ARG(work_bytes >= need, "%s: work_bytes %lld, the tables need %lld (rua_scene_instance_match_work_bytes)", fn, (long long)work_bytes, (long long)need);
  }
  const uint64_t px = (uint64_t)H * (uint64_t)W;
  std::vector<RgRange> v;
  v.push_back({(uintptr_t)inst_p, 4 * px, -1, "inst_p", false});
  v.push_back({(uintptr_t)inst_g, 4 * px, -1, "inst_g", false});
  if (Np > 0) {
    v.push_back({(uintptr_t)area_p, (uint64_t)(Np - 1) * 32 + 4, -1, "area_p", false});
    v.push_back({(uintptr_t)work, (uint64_t)need, -1, "work", true});
    v.push_back({(uintptr_t)match, (uint64_t)Np * 8, -1, "match", true});
  }
  RG_TRY(rg_check_overlap(fn, v));
  if (Np == 0) return RUA_OK;                    // no row to write
  hipStream_t st = (hipStream_t)stream;
  MatchArgs a;
  memset(&a, 0, sizeof(a));
  a.inst_p = inst_p; a.inst_g = inst_g; a.area_p = area_p; a.match = match;
  a.n = (long long)px; a.Np = (int)Np; a.Ng = (int)Ng; a.bits = bit_length(Ng > 0 ? Ng - 1 : 0);
  a.votes = static_cast<int32_t*>(work); a.cand = a.votes + (size_t)Np * a.bits; a.inter = a.cand + Np;
  const long long cells = need / 4;                                                    // below 2^31 * 33: the grid stays below 2^31 blocks
  hipLaunchKernelGGL(match_zero, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a.votes, cells);
  const dim3 pix((unsigned)((px + MT_SPAN - 1) / MT_SPAN)), rows((unsigned)((Np + 255) / 256));
  if (a.bits) hipLaunchKernelGGL(match_votes, pix, dim3(256), 0, st, a);
  hipLaunchKernelGGL(match_cand, rows, dim3(256), 0, st, a);
  hipLaunchKernelGGL(match_inter, pix, dim3(256), 0, st, a);
  hipLaunchKernelGGL(match_write, rows, dim3(256), 0, st, a);
  RUA_LAUNCH_CHECK(fn);
  return RUA_OK;
}

// Flooding: a marker-controlled watershed of a height map in synchronous rounds (rua_scene_flood, include/rua_hip.h;
// scenes.host_flood is the definition).  One scene per call.
//
// The schedule is R = (256 - floor) J + D rounds: levels 255 .. floor, each J times, then D rounds at `floor`.  In a round at level
// t an eligible, unsettled pixel of height >= t that has a settled neighbour of its own class takes the smallest id among those
// neighbours; every decision reads the state at the start of the round (Jacobi).  After S rounds a pixel depends only on the state
// within S pixels of it (Chebyshev distance, so under both connectivities), hence S rounds per launch:
//   flood_init   zeroes the tile flags and the two counters.
//   flood_copy   only when ceil(R / S) is odd: inst -> the second map, so that the last launch writes inst.
//   flood_rounds ceil(R / S) launches.  A block per 32 x 32 tile reads ids from one map and writes its interior to the other - no
//                block reads what another block of the same launch writes.  It stages the interior (ids, class bytes, height
//                bytes) in LDS and looks at it first: a tile without an eligible unsettled pixel is FINISHED - it is copied, its
//                flag counts the copies, and from the third launch on the block leaves at once, both maps holding its final
//                interior.  A tile none of whose open pixels is high enough for the lowest level of this launch is copied too, and
//                so is one whose whole staged region holds no settled pixel.  Every other tile stages the halo of S pixels -
//                (32 + 2 S)^2 = 2304 entries of 6 bytes -, runs S rounds in LDS (a thread owns 9 entries; new ids wait in
//                registers between the two barriers of a round) and writes its interior.  The region's border lacks its outer
//                neighbours, so ring k of the region may be wrong from round k + 1 on: the interior, ring S, is exact through
//                round S.  The level of round r is computed from (r, J, floor); rounds from R on do nothing.
//   flood_table_reset, flood_table   with a table: area and box of rows below min(N, max_instances) and n[1] start over and are
//                collected from the final inst per run of equal ids along a tile row, the tile's largest id in LDS first, as
//                inst_grow does (csrc/instances.hip).
// Integer atomics only (one add per block for `settled`, one max for `last_round`), nothing is read back, no block waits for another.
#include "unionfind.h"
#include <climits>

namespace {

constexpr int FL_T = 32;                       // tile edge: a tile row is half a wave
constexpr int FL_S = 8;                        // rounds per launch = the halo
constexpr int FL_R = FL_T + 2 * FL_S;          // edge of the staged region, 48
constexpr int FL_N = FL_R * FL_R;              // 2304 entries
constexpr int FL_PER = FL_N / 256;             // 9 entries per thread
static_assert(FL_N % 256 == 0, "a thread owns a whole number of entries");
constexpr int FL_MAXC = 64;
constexpr int FL_MAXJ = 16, FL_MAXD = 4096, FL_MAXSTRIDE = 256;

struct FloodArgs {
  const uint8_t* cls; const uint8_t* height;
  const int32_t* src; int32_t* dst;
  int32_t* flags;                              // work: per tile, the copies made since the tile was found finished (0, 1, 2)
  int32_t* stats;
  unsigned long long mask;
  int H, W, C, pix_stride, per_class, conn8, J, floor_, R, r0, tiles;
};

// the level of round r < R
__device__ __forceinline__ int fl_level(const FloodArgs& a, int r) {
  const int lv = 255 - r / a.J;
  return lv > a.floor_ ? lv : a.floor_;
}

__global__ __launch_bounds__(256) void flood_init(int32_t* flags, int tiles, int32_t* stats) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < tiles) flags[e] = 0;
  if (e < 2) stats[e] = 0;
}

__global__ __launch_bounds__(256) void flood_copy(const int32_t* src, int32_t* dst, long long n) {
  const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
  if (x < n) dst[x] = src[x];
}

// one staged entry: the id, the class byte (255: not eligible, or outside the map) and the height byte of an open pixel
__device__ __forceinline__ void fl_stage(const FloodArgs& a, int i, int j, int& id, int& c, int& h) {
  id = -1; c = 255; h = 0;
  if (i < 0 || i >= a.H || j < 0 || j >= a.W) return;
  const size_t x = (size_t)i * a.W + j;
  id = a.src[x];
  const int b = a.cls[x];
  if (b < a.C && ((a.mask >> b) & 1ull)) {
    c = b;
    if (id < 0) h = a.height ? a.height[x * (size_t)a.pix_stride + (a.per_class ? b : 0)] : 255;
  }
}

__global__ __launch_bounds__(256) void flood_rounds(FloodArgs a) {
  __shared__ int sid[FL_N];
  __shared__ uint8_t scl[FL_N], shh[FL_N];
  __shared__ int open_any, live_any, seed_any, n_settled, last_round;
  const int tid = threadIdx.x, H = a.H, W = a.W;
  int32_t* flag = a.flags + blockIdx.x;
  const int done = *flag;                        // written by this tile's block of an earlier launch only
  if (done >= 2) return;                         // finished, and both maps hold the interior
  const int tiles_x = (W - 1) / FL_T + 1;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i0 = ty * FL_T, j0 = tx * FL_T;
  if (tid == 0) { open_any = 0; live_any = 0; seed_any = 0; n_settled = 0; last_round = 0; }
  __syncthreads();
  const int r_end = a.r0 + FL_S < a.R ? a.r0 + FL_S : a.R;           // this launch runs rounds r0 .. r_end - 1
  const int lowest = fl_level(a, r_end - 1);                          // levels only fall
  const int lx = tid & 31;
  {
    bool open = false, live = false, seed = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ly = (tid >> 5) + 8 * k;
      int id, c, h;
      fl_stage(a, i0 + ly, j0 + lx, id, c, h);
      const int e = (ly + FL_S) * FL_R + lx + FL_S;
      sid[e] = id; scl[e] = (uint8_t)c; shh[e] = (uint8_t)h;
      const bool o = c != 255 && id < 0;
      open |= o; live |= o && h >= lowest; seed |= id >= 0;
    }
    if (open) open_any = 1;
    if (live) live_any = 1;
    if (seed) seed_any = 1;
  }
  __syncthreads();
  bool run = live_any != 0;
  if (run) {
    // the halo: every entry of the region outside the interior
    bool seed = false;
    for (int e = tid; e < FL_N; e += 256) {      // 9 rounds
      const int ry = e / FL_R, rx = e - ry * FL_R;
      if (ry >= FL_S && ry < FL_S + FL_T && rx >= FL_S && rx < FL_S + FL_T) continue;
      int id, c, h;
      fl_stage(a, i0 - FL_S + ry, j0 - FL_S + rx, id, c, h);
      sid[e] = id; scl[e] = (uint8_t)c; shh[e] = (uint8_t)h;
      seed |= id >= 0;
    }
    if (seed) seed_any = 1;
    __syncthreads();
    run = seed_any != 0;
  }
  if (run) {
    unsigned open = 0u;                          // bit k: entry tid + 256 k is eligible and unsettled
    unsigned inner = 0u;                         // bit k: that entry is a pixel of the interior
    unsigned up = 0u, dn = 0u, lf = 0u, rt = 0u; // bit k: that entry has a neighbour above, below, left, right inside the region
#pragma unroll
    for (int k = 0; k < FL_PER; ++k) {           // row and column of an entry are taken apart once, here
      const int e = tid + 256 * k;
      const int ry = e / FL_R, rx = e - ry * FL_R;
      if (scl[e] != 255 && sid[e] < 0) open |= 1u << k;
      if (ry >= FL_S && ry < FL_S + FL_T && rx >= FL_S && rx < FL_S + FL_T) inner |= 1u << k;   // outside the map: never open
      if (ry > 0) up |= 1u << k;
      if (ry < FL_R - 1) dn |= 1u << k;
      if (rx > 0) lf |= 1u << k;
      if (rx < FL_R - 1) rt |= 1u << k;
    }
    int mine = 0, last = 0;
    for (int r = a.r0; r < r_end; ++r) {         // at most S rounds, the same for every thread
      const int t = fl_level(a, r);
      int got[FL_PER];
#pragma unroll
      for (int k = 0; k < FL_PER; ++k) {
        got[k] = INT_MAX;
        const int e = tid + 256 * k;
        if (!((open >> k) & 1u) || shh[e] < t) continue;
        const int c = scl[e];
        int best = INT_MAX;
        const bool u = (up >> k) & 1u, d = (dn >> k) & 1u, l = (lf >> k) & 1u, r1 = (rt >> k) & 1u;
#define FL_TRY(ok, off) if (ok) { const int v = sid[e + (off)]; if (v >= 0 && scl[e + (off)] == c && v < best) best = v; }
        FL_TRY(u, -FL_R) FL_TRY(d, FL_R) FL_TRY(l, -1) FL_TRY(r1, 1)
        if (a.conn8) { FL_TRY(u && l, -FL_R - 1) FL_TRY(u && r1, -FL_R + 1) FL_TRY(d && l, FL_R - 1) FL_TRY(d && r1, FL_R + 1) }
#undef FL_TRY
        got[k] = best;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < FL_PER; ++k) {
        if (got[k] == INT_MAX) continue;
        sid[tid + 256 * k] = got[k];
        open &= ~(1u << k);
        if ((inner >> k) & 1u) { ++mine; last = r + 1; }
      }
      __syncthreads();
    }
    if (mine) { atomicAdd(&n_settled, mine); atomicMax(&last_round, last); }
  }
  // the interior leaves: what the rounds made of it, or the copy
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = (tid >> 5) + 8 * k;
    const int i = i0 + ly, j = j0 + lx;
    if (i < H && j < W) a.dst[(size_t)i * W + j] = sid[(ly + FL_S) * FL_R + lx + FL_S];
  }
  __syncthreads();
  if (tid == 0) {
    if (!open_any) *flag = done + 1;
    if (n_settled) { atomicAdd(a.stats, n_settled); atomicMax(a.stats + 1, last_round); }
  }
}

struct FloodTableArgs {
  const uint8_t* cls; const int32_t* inst; int32_t* table; int32_t* n;
  unsigned long long mask;
  int H, W, C, max_instances;
};

__global__ __launch_bounds__(256) void flood_table_reset(FloodTableArgs a) {
  const int n0 = a.n[0];
  const int rows = n0 < a.max_instances ? n0 : a.max_instances;
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < rows) {
    int32_t* row = a.table + (size_t)k * 8;
    row[2] = 0; row[4] = a.H; row[5] = a.W; row[6] = -1; row[7] = -1;
  }
  if (k == 0) a.n[1] = 0;
}

__global__ __launch_bounds__(256) void flood_table(FloodTableArgs a) {
  __shared__ unsigned int ungrown;
  __shared__ int dom, agg[5];                    // the tile's largest id, and its area and box inside the tile
  const int H = a.H, W = a.W, tid = threadIdx.x;
  const int n0 = a.n[0];
  const int rows = n0 < a.max_instances ? n0 : a.max_instances;
  const int tiles_x = (W - 1) / FL_T + 1;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i0 = ty * FL_T, j0 = tx * FL_T;
  if (tid == 0) { ungrown = 0u; dom = -1; agg[0] = 0; agg[1] = INT_MAX; agg[2] = INT_MAX; agg[3] = -1; agg[4] = -1; }
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
      got = a.inst[x];
      const int c = a.cls[x];
      if (got < 0 && c < a.C && ((a.mask >> c) & 1ull)) ++mine;
      if (got < 0 || got >= rows) got = -1;      // no row
    }
    ids4[k] = got;
    top = got > top ? got : top;
  }
  if (top >= 0) atomicMax(&dom, top);
  __syncthreads();
  const int d = dom;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                  // all 64 lanes take part in the shuffle and the ballot
    const int ly = (tid >> 5) + 8 * k;
    const int i = i0 + ly, j = j0 + lx, got = ids4[k];
    const bool valid = i < H && j < W;
    const int beside = __shfl_up(got, 1);
    const uint32_t bits = row_breaks(!valid || lx == 0 || beside != got);
    if (valid && got >= 0 && ((bits >> lx) & 1u)) {
      const uint32_t rest = (bits >> lx) >> 1;
      const int len = rest ? __ffs(rest) : FL_T - lx;
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
  if (tid == 0 && agg[0] > 0) {
    int32_t* row = a.table + (size_t)d * 8;
    atomicAdd(row + 2, agg[0]);
    atomicMin(row + 4, agg[1]); atomicMin(row + 5, agg[2]);
    atomicMax(row + 6, agg[3]); atomicMax(row + 7, agg[4]);
  }
}

int64_t fl_tiles(int H, int W) { return (int64_t)((H - 1) / FL_T + 1) * ((W - 1) / FL_T + 1); }

}  // namespace

extern "C" int64_t rua_scene_flood_work_bytes(int H, int W) {
  if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return -1;
  return ((int64_t)H * W + fl_tiles(H, W)) * 4;
}

extern "C" int rua_scene_flood(const uint8_t* cls, const uint8_t* height, int pix_stride, int per_class, int H, int W, int C,
                               uint64_t class_mask, int connectivity, int rounds_per_level, int floor, int drain, void* work,
                               int64_t work_bytes, int32_t* inst, int32_t* table, int64_t max_instances, int32_t* n, int32_t* stats,
                               void* stream) {
  static const char* const fn = "rua_scene_flood";
  RUA_CHECK_ARG(cls && inst && stats, "%s: cls, inst and stats are required", fn);
  RUA_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31), "%s: size %d x %d (H * W < 2^31: an id is an int32)", fn, H, W);
  RUA_CHECK_ARG(C >= 1 && C <= FL_MAXC, "%s: C %d outside 1..64", fn, C);
  RUA_CHECK_ARG(C == 64 || (class_mask >> C) == 0, "%s: class_mask 0x%llx names a class outside 0..%d", fn, (unsigned long long)class_mask, C - 1);
  RUA_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", fn, connectivity);
  RUA_CHECK_ARG(rounds_per_level >= 1 && rounds_per_level <= FL_MAXJ, "%s: rounds_per_level %d outside 1..16", fn, rounds_per_level);
  RUA_CHECK_ARG(floor >= 0 && floor <= 255, "%s: floor %d outside 0..255", fn, floor);
  RUA_CHECK_ARG(drain >= 0 && drain <= FL_MAXD, "%s: drain %d outside 0..4096", fn, drain);
  if (height) {
    RUA_CHECK_ARG(per_class == 0 || per_class == 1, "%s: per_class %d (0 or 1)", fn, per_class);
    RUA_CHECK_ARG(pix_stride >= 1 && pix_stride <= FL_MAXSTRIDE, "%s: pix_stride %d outside 1..256", fn, pix_stride);
    RUA_CHECK_ARG(!per_class || pix_stride >= C, "%s: pix_stride %d below C %d with per_class", fn, pix_stride, C);
  }
  if (table) {
    RUA_CHECK_ARG(n != nullptr, "%s: n is required with a table", fn);
    RUA_CHECK_ARG(max_instances >= 1 && max_instances < ((int64_t)1 << 31), "%s: max_instances %lld outside 1..2147483647", fn, (long long)max_instances);
  }
  RUA_CHECK_ARG((((uintptr_t)inst | (uintptr_t)table | (uintptr_t)n | (uintptr_t)stats) & 3) == 0, "%s: inst, table, n and stats must be 4-byte aligned", fn);
  const int64_t need = rua_scene_flood_work_bytes(H, W);
  RUA_CHECK_ARG(work && ((uintptr_t)work & 3) == 0, "%s: a 4-byte aligned work buffer is required (rua_scene_flood_work_bytes)", fn);
  RUA_CHECK_ARG(work_bytes >= need, "%s: work_bytes %lld, the scene needs %lld (rua_scene_flood_work_bytes)", fn, (long long)work_bytes, (long long)need);
  const uint64_t px = (uint64_t)H * (uint64_t)W;
  std::vector<RgRange> v;
  v.push_back({(uintptr_t)cls, px, -1, "cls", false});
  if (height) v.push_back({(uintptr_t)height, px * (uint64_t)pix_stride, -1, "height", false});
  v.push_back({(uintptr_t)work, (uint64_t)need, -1, "work", true});
  v.push_back({(uintptr_t)inst, 4 * px, -1, "inst", true});
  if (table) {
    v.push_back({(uintptr_t)table, (uint64_t)max_instances * 32, -1, "table", true});
    v.push_back({(uintptr_t)n, 8, -1, "n", true});
  }
  v.push_back({(uintptr_t)stats, 8, -1, "stats", true});
  RG_TRY(rg_check_overlap(fn, v));
  hipStream_t st = (hipStream_t)stream;
  FloodArgs a;
  memset(&a, 0, sizeof(a));
  a.cls = cls; a.height = height; a.stats = stats; a.mask = class_mask;
  a.H = H; a.W = W; a.C = C; a.pix_stride = height ? pix_stride : 1; a.per_class = height ? per_class : 0;
  a.conn8 = connectivity == 8; a.J = rounds_per_level; a.floor_ = floor;
  a.R = (256 - floor) * rounds_per_level + drain;                                     // 1 .. 8192
  a.tiles = (int)fl_tiles(H, W);                                                       // below 2^21
  int32_t* other = static_cast<int32_t*>(work);
  a.flags = other + px;
  const int launches = (a.R + FL_S - 1) / FL_S;                                        // 1 .. 1024
  hipLaunchKernelGGL(flood_init, dim3((unsigned)((a.tiles + 255) / 256)), dim3(256), 0, st, a.flags, a.tiles, stats);
  int32_t* src = inst;
  int32_t* dst = other;
  if (launches & 1) {                            // an odd count would end in the work map: start from there
    hipLaunchKernelGGL(flood_copy, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, inst, other, (long long)px);
    src = other; dst = inst;
  }
  for (int l = 0; l < launches; ++l) {
    a.src = src; a.dst = dst; a.r0 = l * FL_S;
    hipLaunchKernelGGL(flood_rounds, dim3((unsigned)a.tiles), dim3(256), 0, st, a);
    int32_t* t = src; src = dst; dst = t;
  }
  if (table) {
    FloodTableArgs b;
    memset(&b, 0, sizeof(b));
    b.cls = cls; b.inst = inst; b.table = table; b.n = n; b.mask = class_mask;
    b.H = H; b.W = W; b.C = C; b.max_instances = (int)max_instances;
    hipLaunchKernelGGL(flood_table_reset, dim3((unsigned)((max_instances + 255) / 256)), dim3(256), 0, st, b);
    hipLaunchKernelGGL(flood_table, dim3((unsigned)a.tiles), dim3(256), 0, st, b);
  }
  RUA_LAUNCH_CHECK(fn);
  return RUA_OK;
}

// Outlines of whole-scene instance maps (rua_scene_outline_count, rua_scene_outline_rings, include/rua_hip.h; scenes.host_outlines is
// the definition).  One map per call.  The boundary of an id map is a set of directed unit edges, one per (pixel, side) whose
// neighbour across the side has another id; every edge has one successor, so the edges form cycles - the rings - and putting a ring's
// corners in walking order is list ranking.  An edge's key is 4 (i W + j) + side; COMPACTED index = rank among the edges in key order.
//
// rua_scene_outline_count, three launches whatever the map holds:
//   1. ol_count: a block per chunk of 1024 pixels (row-major) stages the chunk and the rows above and below it in LDS - three strips of
//      1026 ids, negative ids and pixels outside the map as -1 - and counts the chunk's edges and corner edges (both are local: the
//      successor rule reads two pixels of the 3 x 3 neighbourhood).
//   2. ol_scan: ONE block turns the chunk counts into exclusive offsets, 256 chunks per pass with a carry, and writes n = (E, V).
//   3. ol_base: as 1, then a block scan of the per-lane counts (a lane holds four consecutive pixels): base[x] = edges before pixel x.
// rua_scene_outline_rings, 2 ceil(log2 E) + 10 launches (one for E == 0), their number a function of E alone:
//   1. ol_emit: chunk and two rows either way in LDS (five strips of 1028 ids).  Edge base[p] + (rank of the side among p's edges) gets
//      its key with the corner flag in bit 31, its successor's compacted index (base of the successor's pixel + the rank there, from
//      that pixel's own four neighbours) and the first jumping record (own index, successor).
//   2. ol_jump_min, ceil(log2 E) rounds between two buffers of 8-byte records: (min, hop) -> (min(min, min[hop]), hop[hop]).  After
//      round r the record covers 2^r edges along the cycle; wrapping round it is harmless for a minimum.  Compaction keeps key order,
//      so the smallest index of a cycle is its leader - the edge of smallest key.
//   3. ol_cut: the leader replaces the successor in its array; the ranking records start as (corner flag, successor), the edge in
//      front of the leader as (corner flag, NIL): every cycle is now a list that ends there.
//   4. ol_jump_sum, ceil(log2 E) rounds: a record whose hop is not NIL adds the record at its hop and takes that hop.  A list of at
//      most E entries has every hop at NIL after ceil(log2 E) doublings: sum = corner edges from the edge to the end of its list.
//   5. ol_lead_count, ol_scan, ol_lead_number: the leaders are numbered in compacted order (chunks of 1024 edges); a leader writes its
//      ring number into the buffer the jumping left free and the row (id, key, 0, 0, 0, 0).
//   6. ol_collect: vertex count, signed area and length per ring with integer atomics - one set per run of equal rings inside a
//      wave (a segmented scan over the lanes), the runs of the ring at the block's first edge through LDS first, so a ring of
//      millions of edges costs its row three atomics per block.  Sums are taken modulo 2^32: the true values fit an int32.
//   7. ol_ring_count, ol_scan, ol_ring_offset: exclusive scan of the vertex counts over the rings (chunks of 1024 rings).
//   8. ol_scatter: verts[offset + count - sum] = end point, for every corner edge.
// No block waits for another and nothing depends on arrival order: every cell is written by one lane or by integer atomic adds.  Every
// index that came out of memory is compared with the size of what it indexes before it is used, so E and V that do not belong to
// (inst, base) give wrong rings but no access outside the buffers.  Work: 24 bytes per edge (key 4, successor / leader 4, two
// 8-byte jumping buffers) and 4 per chunk.
#include "unionfind.h"

namespace {

constexpr int OL_CHUNK = 1024;                   // pixels, edges or rings per chunk of a scan: 256 lanes of four
constexpr unsigned OL_NIL = 0xFFFFFFFFu;         // the hop of a list's last entry
constexpr int64_t OL_MAXPX = (int64_t)1 << 29;   // keys 4 (H W - 1) + 3 and areas fit an int32

// the row offset of the pixel across side s, and its column offset; the heading of side s is the offset across side s + 1
__device__ __forceinline__ int ol_ni(int s) { return (s & 1) ? 0 : s - 1; }
__device__ __forceinline__ int ol_nj(int s) { return (s & 1) ? 2 - s : 0; }

// The chunk that starts at pixel x0 and the HALO rows above and below it: strip d holds the ids of the pixels x0 + d W - HALO ..
// x0 + d W + 1023 + HALO, -1 for a negative id and beyond either end of the map.  Aligned dwords along the rows.
template <int HALO>
struct Strips {
  static constexpr int PITCH = OL_CHUNK + 2 * HALO;
  static constexpr int SIZE = (2 * HALO + 1) * PITCH;

  static __device__ __forceinline__ void stage(const int32_t* inst, long long n, long long x0, int W, int* sh) {
    for (int d = -HALO; d <= HALO; ++d) {
      const long long r0 = x0 + (long long)d * W - HALO;
      for (int t = threadIdx.x; t < PITCH; t += 256) {
        const long long x = r0 + t;
        int v = -1;
        if (x >= 0 && x < n) { v = inst[x]; v = v < 0 ? -1 : v; }
        sh[(d + HALO) * PITCH + t] = v;
      }
    }
  }
  // the id at (di, dj) from the pixel at chunk position lx in column j.  A column outside the map is no pixel; with the column inside,
  // a row outside the map lies beyond an end of the map and was staged as -1.
  static __device__ __forceinline__ int id(const int* sh, int lx, int j, int W, int di, int dj) {
    const int jj = j + dj;
    if (jj < 0 || jj >= W) return -1;
    return sh[(di + HALO) * PITCH + lx + dj + HALO];
  }
  // bit s: the pixel at (di, dj) owns an edge on side s
  static __device__ __forceinline__ int mask(const int* sh, int lx, int j, int W, int di, int dj) {
    const int k = id(sh, lx, j, W, di, dj);
    if (k < 0) return 0;
    int m = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) m |= (id(sh, lx, j, W, di + ol_ni(s), dj + ol_nj(s)) != k) << s;
    return m;
  }
  // the successor of edge (pixel, s) of an object k: the offset of its pixel and its side
  static __device__ __forceinline__ void succ(const int* sh, int lx, int j, int W, int k, int s, int conn, int& qi, int& qj, int& s2) {
    const int fi = ol_ni((s + 1) & 3), fj = ol_nj((s + 1) & 3), li = fi + ol_ni(s), lj = fj + ol_nj(s);
    const bool f = id(sh, lx, j, W, fi, fj) == k, l = id(sh, lx, j, W, li, lj) == k;
    if (l && (f || conn == 8)) { qi = li; qj = lj; s2 = (s + 3) & 3; }
    else if (f) { qi = fi; qj = fj; s2 = s; }
    else { qi = 0; qj = 0; s2 = (s + 1) & 3; }
  }
};

struct CountArgs {
  const int32_t* inst; int32_t* base; unsigned* chunk_e; unsigned* chunk_v; int64_t* n;
  long long px; int W, conn;
};

// edges and corner edges of the four pixels x .. x + 3 of a lane
__device__ __forceinline__ void ol_count4(const CountArgs& a, const int* sh, int lx, long long x, int cnt[4], int& corners) {
  typedef Strips<1> S;
  corners = 0;
  int j = (int)(x % a.W);
#pragma unroll
  for (int e = 0; e < 4; ++e, ++j) {
    cnt[e] = 0;
    if (x + e >= a.px) continue;
    if (j >= a.W) j -= a.W;                        // W >= 1: at most one row end between two neighbours
    const int k = S::id(sh, lx + e, j, a.W, 0, 0), m = S::mask(sh, lx + e, j, a.W, 0, 0);
    cnt[e] = __popc(m);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (!((m >> s) & 1)) continue;
      int qi, qj, s2;
      S::succ(sh, lx + e, j, a.W, k, s, a.conn, qi, qj, s2);
      corners += s2 != s;
    }
  }
}

__global__ __launch_bounds__(256) void ol_count(CountArgs a) {
  __shared__ int sh[Strips<1>::SIZE];
  __shared__ unsigned ce, cv;
  if (threadIdx.x == 0) { ce = 0u; cv = 0u; }
  const long long x0 = (long long)blockIdx.x * OL_CHUNK;
  Strips<1>::stage(a.inst, a.px, x0, a.W, sh);
  __syncthreads();
  int cnt[4], corners;
  ol_count4(a, sh, threadIdx.x * 4, x0 + threadIdx.x * 4, cnt, corners);
  const int edges = cnt[0] + cnt[1] + cnt[2] + cnt[3];
  if (edges) { atomicAdd(&ce, (unsigned)edges); atomicAdd(&cv, (unsigned)corners); }
  __syncthreads();
  if (threadIdx.x == 0) { a.chunk_e[blockIdx.x] = ce; a.chunk_v[blockIdx.x] = cv; }
}

// ONE block: c0 (and c1, if given) become their exclusive prefixes, 256 chunks per pass with a carry; the totals go to tot[0], tot[1]
__global__ __launch_bounds__(256) void ol_scan(unsigned* c0, unsigned* c1, long long chunks, int64_t* tot) {
  __shared__ unsigned sh[256];
  unsigned carry0 = 0u, carry1 = 0u;
  for (long long b = 0; b < chunks; b += 256) {   // ceil(chunks / 256) passes
    const long long c = b + threadIdx.x;
    unsigned total;
    const unsigned v0 = c < chunks ? c0[c] : 0u;
    const unsigned ex0 = block_scan_256(sh, v0, total);
    if (c < chunks) c0[c] = carry0 + ex0;
    carry0 += total;                               // at most 4 H W <= 2^31
    if (c1) {
      const unsigned v1 = c < chunks ? c1[c] : 0u;
      const unsigned ex1 = block_scan_256(sh, v1, total);
      if (c < chunks) c1[c] = carry1 + ex1;
      carry1 += total;
    }
  }
  if (threadIdx.x == 0) { tot[0] = (int64_t)carry0; if (c1) tot[1] = (int64_t)carry1; }
}

__global__ __launch_bounds__(256) void ol_base(CountArgs a) {
  __shared__ int sh[Strips<1>::SIZE];
  __shared__ unsigned scan[256];
  const long long x0 = (long long)blockIdx.x * OL_CHUNK, x = x0 + threadIdx.x * 4;
  Strips<1>::stage(a.inst, a.px, x0, a.W, sh);
  __syncthreads();
  int cnt[4], corners;
  ol_count4(a, sh, threadIdx.x * 4, x, cnt, corners);
  unsigned total;
  unsigned at = a.chunk_e[blockIdx.x] + block_scan_256(scan, (unsigned)(cnt[0] + cnt[1] + cnt[2] + cnt[3]), total);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (x + e < a.px) a.base[x + e] = (int32_t)at; // below 2^31: at least one pixel's edges are not counted
    at += (unsigned)cnt[e];
  }
}

struct RingArgs {
  const int32_t* inst; const int32_t* base;
  unsigned* keyc;                                // key | corner << 31
  unsigned* lead;                                // the successor until ol_cut, the leader from then on
  uint2* rec[2];                                 // the jumping records
  unsigned* chunk_e; unsigned* chunk_r;          // leaders per chunk of edges, vertices per chunk of rings; then their prefixes
  int64_t* scratch;                              // a total nobody reads
  int32_t* rings; int32_t* verts; int64_t* nr;
  long long px;
  unsigned E, V, cap;                            // cap = V / 4 ring rows
  int W, conn;
};

__global__ __launch_bounds__(256) void ol_emit(RingArgs a) {
  typedef Strips<2> S;
  __shared__ int sh[S::SIZE];
  const long long x0 = (long long)blockIdx.x * OL_CHUNK, x = x0 + threadIdx.x * 4;
  S::stage(a.inst, a.px, x0, a.W, sh);
  __syncthreads();
  int j = (int)(x % a.W);
#pragma unroll
  for (int e = 0; e < 4; ++e, ++j) {
    if (x + e >= a.px) break;
    if (j >= a.W) j -= a.W;
    const int lx = threadIdx.x * 4 + e;
    const int k = S::id(sh, lx, j, a.W, 0, 0), m = S::mask(sh, lx, j, a.W, 0, 0);
    if (!m) continue;
    unsigned at = (unsigned)a.base[x + e];
    for (int s = 0; s < 4; ++s) {
      if (!((m >> s) & 1)) continue;
      int qi, qj, s2;
      S::succ(sh, lx, j, a.W, k, s, a.conn, qi, qj, s2);
      const int mq = S::mask(sh, lx, j, a.W, qi, qj);
      unsigned nxt = (unsigned)a.base[x + e + (long long)qi * a.W + qj] + (unsigned)__popc(mq & ((1 << s2) - 1));
      const unsigned idx = at++;
      if (idx >= a.E) continue;                    // an E below the map's: nothing beyond the buffers
      if (nxt >= a.E) nxt = idx;
      a.keyc[idx] = (unsigned)(4 * (x + e) + s) | (s2 != s ? 0x80000000u : 0u);
      a.lead[idx] = nxt;
      a.rec[0][idx] = make_uint2(idx, nxt);
    }
  }
}

__global__ __launch_bounds__(256) void ol_jump_min(const uint2* in, uint2* out, unsigned E) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= E) return;
  uint2 r = in[e];
  if (r.y < E) {                                   // always, for records ol_emit wrote
    const uint2 h = in[r.y];
    r.x = h.x < r.x ? h.x : r.x;
    r.y = h.y;
  }
  out[e] = r;
}

__global__ __launch_bounds__(256) void ol_cut(const uint2* fin, uint2* out, RingArgs a) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= a.E) return;
  const unsigned leader = fin[e].x, nxt = a.lead[e];
  a.lead[e] = leader < a.E ? leader : e;
  out[e] = make_uint2(a.keyc[e] >> 31, nxt == leader ? OL_NIL : nxt);
}

__global__ __launch_bounds__(256) void ol_jump_sum(const uint2* in, uint2* out, unsigned E) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= E) return;
  uint2 r = in[e];
  if (r.y < E) {                                   // not NIL
    const uint2 h = in[r.y];
    r.x += h.x;
    r.y = h.y;
  }
  out[e] = r;
}

__global__ __launch_bounds__(256) void ol_lead_count(RingArgs a) {
  __shared__ unsigned cnt;
  if (threadIdx.x == 0) cnt = 0u;
  __syncthreads();
  const unsigned long long e0 = (unsigned long long)blockIdx.x * OL_CHUNK + threadIdx.x * 4;
  unsigned k = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (e0 + t < a.E && a.lead[e0 + t] == (unsigned)(e0 + t)) ++k;
  if (k) atomicAdd(&cnt, k);
  __syncthreads();
  if (threadIdx.x == 0) a.chunk_e[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(256) void ol_lead_number(RingArgs a, unsigned* ringno) {
  __shared__ unsigned scan[256];
  const unsigned long long e0 = (unsigned long long)blockIdx.x * OL_CHUNK + threadIdx.x * 4;
  bool q[4];
  unsigned k = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) { q[t] = e0 + t < a.E && a.lead[e0 + t] == (unsigned)(e0 + t); k += q[t]; }
  unsigned total;
  unsigned r = a.chunk_e[blockIdx.x] + block_scan_256(scan, k, total);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (!q[t]) continue;
    ringno[e0 + t] = r;
    if (r < a.cap) {                               // always, for a V that belongs to the map: a ring has at least four corners
      const unsigned key = a.keyc[e0 + t] & 0x7FFFFFFFu;
      int32_t* row = a.rings + (size_t)r * 6;
      row[0] = (key >> 2) < (unsigned long long)a.px ? a.inst[key >> 2] : -1;
      row[1] = (int32_t)key; row[2] = 0; row[3] = 0; row[4] = 0; row[5] = 0;
    }
    ++r;
  }
}

__global__ __launch_bounds__(256) void ol_collect(RingArgs a, const unsigned* ringno) {
  __shared__ unsigned agg[3];                      // vertices, area, length of the ring of the block's first edge, inside the block
  const unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 3) agg[threadIdx.x] = 0u;
  const unsigned l0 = a.lead[(unsigned long long)blockIdx.x * 256u];   // the grid holds no block without an edge
  unsigned l = OL_NIL, cl = 0u, ar = 0u;
  if (e < a.E) {
    l = a.lead[e];
    const unsigned kc = a.keyc[e], key = kc & 0x7FFFFFFFu, s = key & 3u, i = (key >> 2) / (unsigned)a.W;
    cl = (kc >> 31) | (1u << 16);                  // vertices in the low half, length in the high: at most 64 each in a wave
    ar = s == 2u ? i + 1u : s == 0u ? 0u - i : 0u; // modulo 2^32
  }
  __syncthreads();
  // the runs of equal leaders along the wave; all 64 lanes take part in every shuffle and in the ballot
  const unsigned up = __shfl_up(l, 1);
  const unsigned long long heads = __ballot(lane == 0 || up != l);
  const int hp = 63 - __clzll(heads & ((2ull << lane) - 1ull));        // the head of this lane's run (lane 63: the mask is all ones)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {               // a scan that stops at the run's head: the run's last lane ends with its sums
    const unsigned t1 = __shfl_up(cl, d), t2 = __shfl_up(ar, d);
    if (lane - d >= hp) { cl += t1; ar += t2; }
  }
  const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (last && l != OL_NIL) {
    if (l == l0) {
      atomicAdd(&agg[0], cl & 0xFFFFu); atomicAdd(&agg[1], ar); atomicAdd(&agg[2], cl >> 16);
    } else {
      const unsigned r = ringno[l];
      if (r < a.cap) {
        unsigned* row = reinterpret_cast<unsigned*>(a.rings) + (size_t)r * 6;
        if (cl & 0xFFFFu) atomicAdd(row + 3, cl & 0xFFFFu);
        if (ar) atomicAdd(row + 4, ar);
        atomicAdd(row + 5, cl >> 16);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && agg[2]) {
    const unsigned r = ringno[l0];
    if (r < a.cap) {
      unsigned* row = reinterpret_cast<unsigned*>(a.rings) + (size_t)r * 6;
      if (agg[0]) atomicAdd(row + 3, agg[0]);
      if (agg[1]) atomicAdd(row + 4, agg[1]);
      atomicAdd(row + 5, agg[2]);
    }
  }
}

// the rings in use: what the leaders' scan counted, never more than there are rows
__device__ __forceinline__ unsigned ol_rings_used(const RingArgs& a) {
  const int64_t r = a.nr[0];
  return r < (int64_t)a.cap ? (unsigned)r : a.cap;
}

__global__ __launch_bounds__(256) void ol_ring_count(RingArgs a) {
  __shared__ unsigned cnt;
  if (threadIdx.x == 0) cnt = 0u;
  __syncthreads();
  const unsigned R = ol_rings_used(a);
  const unsigned long long r0 = (unsigned long long)blockIdx.x * OL_CHUNK + threadIdx.x * 4;
  unsigned k = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (r0 + t < R) k += (unsigned)a.rings[(r0 + t) * 6 + 3];
  if (k) atomicAdd(&cnt, k);
  __syncthreads();
  if (threadIdx.x == 0) a.chunk_r[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(256) void ol_ring_offset(RingArgs a) {
  __shared__ unsigned scan[256];
  const unsigned R = ol_rings_used(a);
  const unsigned long long r0 = (unsigned long long)blockIdx.x * OL_CHUNK + threadIdx.x * 4;
  unsigned c[4], k = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) { c[t] = r0 + t < R ? (unsigned)a.rings[(r0 + t) * 6 + 3] : 0u; k += c[t]; }
  unsigned total;
  unsigned at = a.chunk_r[blockIdx.x] + block_scan_256(scan, k, total);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (r0 + t < R) a.rings[(r0 + t) * 6 + 2] = (int32_t)at;
    at += c[t];
  }
}

__global__ __launch_bounds__(256) void ol_scatter(RingArgs a, const uint2* sums, const unsigned* ringno) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= a.E) return;
  const unsigned kc = a.keyc[e];
  if (!(kc >> 31)) return;
  const unsigned r = ringno[a.lead[e]];
  if (r >= a.cap) return;
  const int32_t* row = a.rings + (size_t)r * 6;
  const unsigned long long at = (unsigned long long)(unsigned)row[2] + (unsigned)row[3] - sums[e].x;
  if (at >= a.V) return;                           // a V below the map's
  const unsigned key = kc & 0x7FFFFFFFu, s = key & 3u, p = key >> 2;
  const int i = (int)(p / (unsigned)a.W), j = (int)(p - (unsigned)i * (unsigned)a.W);
  // the end point of side s: (i, j+1), (i+1, j+1), (i+1, j), (i, j)
  reinterpret_cast<int2*>(a.verts)[at] = make_int2(i + (s == 1u || s == 2u), j + (s <= 1u));
}

__global__ void ol_no_ring(int64_t* nr) { nr[0] = 0; }

int64_t ol_chunks(int64_t n) { return (n + OL_CHUNK - 1) / OL_CHUNK; }
int64_t ol_round16(int64_t b) { return (b + 15) & ~(int64_t)15; }

int ol_check_map(const char* fn, int H, int W, int connectivity) {
  RUA_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W <= OL_MAXPX, "%s: size %d x %d (1 <= H, W and H * W <= 2^29: keys and areas are int32)", fn, H, W);
  RUA_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", fn, connectivity);
  return RUA_OK;
}

int ol_rounds(int64_t E) {                       // ceil(log2 E)
  int k = 0;
  while (((int64_t)1 << k) < E) ++k;
  return k;
}

// the sections of the rings call's work buffer, in bytes from its start
struct RingWork { int64_t chunk_e, chunk_r, keyc, lead, rec0, rec1, end; };

RingWork ol_ring_work(int64_t E) {
  RingWork w;
  w.chunk_e = 16;                                  // after the scratch total
  w.chunk_r = w.chunk_e + ol_round16(4 * ol_chunks(E));
  w.keyc = w.chunk_r + ol_round16(4 * ol_chunks(E / 4));
  w.lead = w.keyc + ol_round16(4 * E);
  w.rec0 = w.lead + ol_round16(4 * E);
  w.rec1 = w.rec0 + ol_round16(8 * E);
  w.end = w.rec1 + ol_round16(8 * E);
  return w;
}

}  // namespace

extern "C" int64_t rua_scene_outline_work_bytes(int H, int W, int64_t E) {
  if (H < 1 || W < 1 || (int64_t)H * W > OL_MAXPX || E < 0 || E > 4 * (int64_t)H * W) return -1;
  const int64_t count = 8 * ol_chunks((int64_t)H * W);
  return E == 0 ? count : std::max(count, ol_ring_work(E).end);
}

extern "C" int rua_scene_outline_count(const int32_t* inst, int H, int W, int connectivity, int32_t* base, void* work, int64_t work_bytes,
                                       int64_t* n, void* stream) {
  static const char* const fn = "rua_scene_outline_count";
  RUA_CHECK_ARG(inst && base && n, "%s: inst, base and n are required", fn);
  RG_TRY(ol_check_map(fn, H, W, connectivity));
  RUA_CHECK_ARG((((uintptr_t)inst | (uintptr_t)base) & 3) == 0, "%s: inst and base must be 4-byte aligned", fn);
  RUA_CHECK_ARG(((uintptr_t)n & 7) == 0, "%s: n must be 8-byte aligned", fn);
  const int64_t need = rua_scene_outline_work_bytes(H, W, 0);
  RUA_CHECK_ARG(work && ((uintptr_t)work & 15) == 0, "%s: a 16-byte aligned work buffer is required (rua_scene_outline_work_bytes)", fn);
  RUA_CHECK_ARG(work_bytes >= need, "%s: work_bytes %lld, the map needs %lld (rua_scene_outline_work_bytes(H, W, 0))", fn, (long long)work_bytes, (long long)need);
  const uint64_t px = (uint64_t)H * (uint64_t)W;
  std::vector<RgRange> v;
  v.push_back({(uintptr_t)inst, 4 * px, -1, "inst", false});
  v.push_back({(uintptr_t)base, 4 * px, -1, "base", true});
  v.push_back({(uintptr_t)work, (uint64_t)need, -1, "work", true});
  v.push_back({(uintptr_t)n, 16, -1, "n", true});
  RG_TRY(rg_check_overlap(fn, v));
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = ol_chunks((int64_t)px);                                       // at most 2^19
  CountArgs a;
  memset(&a, 0, sizeof(a));
  a.inst = inst; a.base = base; a.n = n;
  a.chunk_e = static_cast<unsigned*>(work); a.chunk_v = a.chunk_e + chunks;
  a.px = (long long)px; a.W = W; a.conn = connectivity;
  hipLaunchKernelGGL(ol_count, dim3((unsigned)chunks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(ol_scan, dim3(1), dim3(256), 0, st, a.chunk_e, a.chunk_v, (long long)chunks, n);
  hipLaunchKernelGGL(ol_base, dim3((unsigned)chunks), dim3(256), 0, st, a);
  RUA_LAUNCH_CHECK(fn);
  return RUA_OK;
}

extern "C" int rua_scene_outline_rings(const int32_t* inst, const int32_t* base, int H, int W, int connectivity, int64_t E, int64_t V, void* work,
                                       int64_t work_bytes, int32_t* rings, int32_t* verts, int64_t* nr, void* stream) {
  static const char* const fn = "rua_scene_outline_rings";
  RUA_CHECK_ARG(inst && base && nr, "%s: inst, base and nr are required", fn);
  RG_TRY(ol_check_map(fn, H, W, connectivity));
  const uint64_t px = (uint64_t)H * (uint64_t)W;
  RUA_CHECK_ARG(E >= 0 && E <= 4 * (int64_t)px, "%s: E %lld outside 0..4 H W = %lld", fn, (long long)E, (long long)(4 * px));
  RUA_CHECK_ARG(E == 0 ? V == 0 : V >= 4 && V <= E && V % 2 == 0,
                "%s: V %lld with E %lld (what rua_scene_outline_count wrote: even, 4 <= V <= E, or both 0)", fn, (long long)V, (long long)E);
  RUA_CHECK_ARG((((uintptr_t)inst | (uintptr_t)base | (uintptr_t)rings) & 3) == 0, "%s: inst, base and rings must be 4-byte aligned", fn);
  RUA_CHECK_ARG((((uintptr_t)verts | (uintptr_t)nr) & 7) == 0, "%s: verts and nr must be 8-byte aligned", fn);
  const int64_t need = rua_scene_outline_work_bytes(H, W, E);
  if (E > 0) {
    RUA_CHECK_ARG(rings && verts, "%s: rings and verts are required with E > 0", fn);
    RUA_CHECK_ARG(work && ((uintptr_t)work & 15) == 0, "%s: a 16-byte aligned work buffer is required (rua_scene_outline_work_bytes)", fn);
    RUA_CHECK_ARG(work_bytes >= need, "%s: work_bytes %lld, %lld edges need %lld (rua_scene_outline_work_bytes)", fn, (long long)work_bytes,
                  (long long)E, (long long)need);
  }
  std::vector<RgRange> v;
  v.push_back({(uintptr_t)inst, 4 * px, -1, "inst", false});
  v.push_back({(uintptr_t)base, 4 * px, -1, "base", false});
  v.push_back({(uintptr_t)nr, 8, -1, "nr", true});
  if (E > 0) {
    v.push_back({(uintptr_t)work, (uint64_t)need, -1, "work", true});
    v.push_back({(uintptr_t)rings, (uint64_t)(V / 4) * 24, -1, "rings", true});
    v.push_back({(uintptr_t)verts, (uint64_t)V * 8, -1, "verts", true});
  }
  RG_TRY(rg_check_overlap(fn, v));
  hipStream_t st = (hipStream_t)stream;
  if (E == 0) {
    hipLaunchKernelGGL(ol_no_ring, dim3(1), dim3(1), 0, st, nr);
    RUA_LAUNCH_CHECK(fn);
    return RUA_OK;
  }
  const RingWork w = ol_ring_work(E);
  char* wb = static_cast<char*>(work);
  RingArgs a;
  memset(&a, 0, sizeof(a));
  a.inst = inst; a.base = base; a.rings = rings; a.verts = verts; a.nr = nr;
  a.scratch = reinterpret_cast<int64_t*>(wb);
  a.chunk_e = reinterpret_cast<unsigned*>(wb + w.chunk_e); a.chunk_r = reinterpret_cast<unsigned*>(wb + w.chunk_r);
  a.keyc = reinterpret_cast<unsigned*>(wb + w.keyc); a.lead = reinterpret_cast<unsigned*>(wb + w.lead);
  a.rec[0] = reinterpret_cast<uint2*>(wb + w.rec0); a.rec[1] = reinterpret_cast<uint2*>(wb + w.rec1);
  a.px = (long long)px; a.E = (unsigned)E; a.V = (unsigned)V; a.cap = (unsigned)(V / 4); a.W = W; a.conn = connectivity;
  const int K = ol_rounds(E);                                                          // at most 31
  const dim3 pix((unsigned)ol_chunks((int64_t)px)), per_edge((unsigned)((E + 255) / 256));   // at most 2^19 and 2^23 blocks
  const int64_t ce = ol_chunks(E), cr = ol_chunks(V / 4);
  hipLaunchKernelGGL(ol_emit, pix, dim3(256), 0, st, a);
  for (int r = 0; r < K; ++r) hipLaunchKernelGGL(ol_jump_min, per_edge, dim3(256), 0, st, a.rec[r & 1], a.rec[(r + 1) & 1], a.E);
  // the leaders lie in rec[K & 1] (q1); the ranking starts in the other buffer (q0) and ends, K rounds later, in q0 or q1
  uint2* const q0 = a.rec[(K + 1) & 1];
  uint2* const q1 = a.rec[K & 1];
  hipLaunchKernelGGL(ol_cut, per_edge, dim3(256), 0, st, q1, q0, a);
  for (int r = 0; r < K; ++r) hipLaunchKernelGGL(ol_jump_sum, per_edge, dim3(256), 0, st, r & 1 ? q1 : q0, r & 1 ? q0 : q1, a.E);
  const uint2* const sums = K & 1 ? q1 : q0;
  unsigned* const ringno = reinterpret_cast<unsigned*>(K & 1 ? q0 : q1);               // the buffer the ranking left free
  hipLaunchKernelGGL(ol_lead_count, dim3((unsigned)ce), dim3(256), 0, st, a);
  hipLaunchKernelGGL(ol_scan, dim3(1), dim3(256), 0, st, a.chunk_e, (unsigned*)nullptr, (long long)ce, nr);
  hipLaunchKernelGGL(ol_lead_number, dim3((unsigned)ce), dim3(256), 0, st, a, ringno);
  hipLaunchKernelGGL(ol_collect, per_edge, dim3(256), 0, st, a, (const unsigned*)ringno);
  hipLaunchKernelGGL(ol_ring_count, dim3((unsigned)cr), dim3(256), 0, st, a);
  hipLaunchKernelGGL(ol_scan, dim3(1), dim3(256), 0, st, a.chunk_r, (unsigned*)nullptr, (long long)cr, a.scratch);
  hipLaunchKernelGGL(ol_ring_offset, dim3((unsigned)cr), dim3(256), 0, st, a);
  hipLaunchKernelGGL(ol_scatter, per_edge, dim3(256), 0, st, a, sums, (const unsigned*)ringno);
  RUA_LAUNCH_CHECK(fn);
  return RUA_OK;
}

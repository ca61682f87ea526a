// Lovasz-Softmax: the Lovasz extension of the Jaccard index over a head's probabilities (include/rua_hip.h, rua_lovasz_grad / rua_lovasz_dz; the
// package's losses.py holds the definitions, host_lovasz and host_lovasz_dz).
//
// Every class needs all valid pixels ordered by their error, descending, ties in ascending pixel index: a stable LSD radix sort of (key, pixel)
// pairs in four 8-bit digit passes, the classes batched over blockIdx.y.  A pair is one u64: the high word is ~ohem_key(e) - ascending in it is
// descending in e, a NaN (key 0xFFFFFFFF) first -, the low word is pixel | fg << 31.  A void pixel takes the high word 0xFFFFFFFF, above every
// valid one (a valid key has its top bit set), so the void pixels are the tail of the order.
//
// 18 + 1 launches, a function of (M, C) alone; no block waits for another, plain stores and integer atomics only, nothing is read back:
//   1      lovasz_zero_kernel      the counters n_valid, G[16]
//   2      lovasz_key_kernel       the pairs of every class; n_valid and G_c with integer atomics (per block through LDS)
//   3..14  four digit passes, each  lovasz_hist_kernel     per tile of LV_T pairs the 256 digit counts (LDS, one ballot-merged atomic per equal run)
//                                   lovasz_scan_kernel     per class one block: exclusive offsets in (digit, tile) order
//                                   lovasz_scatter_kernel  per tile: stable ranks from wave ballots, the tile staged in LDS in digit order so that a
//                                                          digit's run leaves as contiguous stores
//   15     lovasz_fgsum_kernel     per tile the number of foreground pairs
//   16     lovasz_fgscan_kernel    per class one block: exclusive prefix of the tile counts
//   17     lovasz_apply_kernel     F_r, w_r = J_r - J_{r-1} in fp64, dp scattered to the pixels, order_out, per-tile fp64 partials of e * w
//   18     lovasz_finish_kernel    one block: the partials in tile order, the classes in order; the result struct, loss_out[0] += loss_weight * loss
//   (+1    lovasz_dz_kernel        rua_lovasz_dz, the streaming pass from dp to d(total)/d(logits))
// The fp64 sums are deterministic: a thread adds its eight ranks in order, a fixed butterfly folds the lanes, the waves and then the tiles are added
// in order.  The equal-key hot spot (p = 1/C everywhere puts all 64 lanes on one digit) costs no serialised atomics: the histogram merges the lanes
// of the first active lane's bin by a ballot (as ohem_hist_kernel does), and the scatter ranks by ballots alone and stores one count per equal run.
#include "common.h"

#define LV_T 2048                       // pairs per tile: 256 threads x 8
#define LV_PER 8
#define LV_SEG (LV_T / 64)              // 64-pair segments of a tile, in order
typedef unsigned long long u64;

struct LvCounters { long long n_valid; long long G[RUA_LOVASZ_MAX_C]; };

static inline int64_t lv_tiles(int64_t M) { return (M + LV_T - 1) / LV_T; }
static inline int64_t lv_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
struct LvLayout { int64_t a, b, hist, tsum, part, cnt, total; };
static inline LvLayout lv_layout(int64_t M, int C) {
  const int64_t nt = lv_tiles(M);
  LvLayout l; int64_t o = 0;
  l.a = o; o += lv_align((int64_t)C * M * 8);
  l.b = o; o += lv_align((int64_t)C * M * 8);
  l.hist = o; o += lv_align((int64_t)C * nt * 256 * 4);
  l.tsum = o; o += lv_align((int64_t)C * nt * 4);
  l.part = o; o += lv_align((int64_t)C * nt * 8);
  l.cnt = o; o += lv_align((int64_t)sizeof(LvCounters));
  l.total = o;
  return l;
}

__device__ __forceinline__ unsigned lv_key(float v) {         // ohem.hip's key: order-preserving, every NaN the largest
  const unsigned b = __float_as_uint(v);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float lv_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ __launch_bounds__(64) void lovasz_zero_kernel(LvCounters* __restrict__ cnt) {
  if (threadIdx.x == 0) cnt->n_valid = 0;
  if (threadIdx.x < RUA_LOVASZ_MAX_C) cnt->G[threadIdx.x] = 0;
}

// one thread per pixel and grid step: the C pairs of the pixel (coalesced per class), the counts through LDS
__global__ __launch_bounds__(256) void lovasz_key_kernel(const float* __restrict__ p, const float* __restrict__ y, const uint8_t* __restrict__ vm,
                                                         long long M, int C, u64* __restrict__ A, LvCounters* __restrict__ cnt) {
  __shared__ unsigned sh[RUA_LOVASZ_MAX_C + 1];
  if (threadIdx.x <= RUA_LOVASZ_MAX_C) sh[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256; base < M; base += (long long)gridDim.x * 256) {       // block-uniform trip count
    const long long m = base + threadIdx.x;
    const bool in = m < M;
    const bool valid = in && (vm == nullptr || vm[m] == 0);
    const u64 nb = __ballot(valid);
    if (lane == 0 && nb != 0) atomicAdd(&sh[RUA_LOVASZ_MAX_C], (unsigned)__popcll(nb));
    for (int c = 0; c < C; ++c) {
      bool fg = false; unsigned hi = 0xffffffffu;
      if (valid) {
        fg = y[(size_t)m * C + c] > 0.5f;
        const float e = fabsf((fg ? 1.0f : 0.0f) - p[(size_t)m * C + c]);
        hi = ~lv_key(e);
      }
      if (in) A[(size_t)c * M + m] = ((u64)hi << 32) | (u64)((unsigned)m | (fg ? 0x80000000u : 0u));
      const u64 fb = __ballot(fg);
      if (lane == 0 && fb != 0) atomicAdd(&sh[c], (unsigned)__popcll(fb));
    }
  }
  __syncthreads();
  if (threadIdx.x < C && sh[threadIdx.x] != 0) atomicAdd((u64*)&cnt->G[threadIdx.x], (u64)sh[threadIdx.x]);
  if (threadIdx.x == RUA_LOVASZ_MAX_C && sh[RUA_LOVASZ_MAX_C] != 0) atomicAdd((u64*)&cnt->n_valid, (u64)sh[RUA_LOVASZ_MAX_C]);
}

// hist[c][tile][256]: the digit counts of a tile (every entry stored: the workspace needs no zeroing)
__global__ __launch_bounds__(256) void lovasz_hist_kernel(const u64* __restrict__ src, long long M, int shift, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const long long tile = blockIdx.x;
  const u64* s = src + (size_t)blockIdx.y * M;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < LV_PER; ++r) {
    const long long i = tile * LV_T + r * 256 + threadIdx.x;
    const bool act = i < M;
    unsigned bin = 0;
    if (act) bin = (unsigned)(s[i] >> shift) & 255u;
    const u64 am = __ballot(act);
    if (am != 0) {                                        // the lanes on the first active lane's bin: one atomic for all of them
      const int leader = __ffsll((long long)am) - 1;
      const unsigned fb = (unsigned)__shfl((int)bin, leader, 64);
      const u64 same = __ballot(act && bin == fb);
      if (act) {
        if (bin == fb) { if (lane == leader) atomicAdd(&h[fb], (unsigned)__popcll(same)); }
        else atomicAdd(&h[bin], 1u);
      }
    }
  }
  __syncthreads();
  hist[((size_t)blockIdx.y * gridDim.x + tile) * 256 + threadIdx.x] = h[threadIdx.x];
}

// One block of 1024 threads per class: hist[c][tile][d] becomes the exclusive offset of (d, tile) in (digit, tile) order.  Thread (g, d) walks a
// quarter of the tiles of digit d (loads coalesced over d); the 256 digit totals are scanned by the first four waves.
__global__ __launch_bounds__(1024) void lovasz_scan_kernel(unsigned* __restrict__ hist, long long ntiles) {
  __shared__ unsigned part[4][256];
  __shared__ unsigned excl[256];
  __shared__ unsigned wsum[4];
  const int g = threadIdx.x >> 8, d = threadIdx.x & 255;
  unsigned* h = hist + (size_t)blockIdx.x * ntiles * 256;
  const long long per = (ntiles + 3) / 4;
  const long long t0 = g * per, t1 = (t0 + per < ntiles) ? t0 + per : ntiles;
  unsigned s = 0;
#pragma unroll 8
  for (long long t = t0; t < t1; ++t) s += h[(size_t)t * 256 + d];
  part[g][d] = s;
  __syncthreads();
  if (g == 0) {
    const unsigned tot = ((part[0][d] + part[1][d]) + part[2][d]) + part[3][d];
    const int lane = d & 63, wave = d >> 6;
    unsigned incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = (unsigned)__shfl_up((int)incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    excl[d] = incl - tot;
  }
  __syncthreads();
  unsigned run = excl[d];
  for (int w = 0; w < (d >> 6); ++w) run += wsum[w];
  for (int q = 0; q < g; ++q) run += part[q][d];
#pragma unroll 8
  for (long long t = t0; t < t1; ++t) {
    const unsigned c = h[(size_t)t * 256 + d];
    h[(size_t)t * 256 + d] = run;
    run += c;
  }
}

// The order inside a tile is r * 256 + thread: segment (r, wave) = 64 consecutive pairs.  A pair's rank among the equal digits of its segment
// comes from eight ballots (match-any on the digit's bits); the first lane of an equal run stores the run's length: no LDS atomics at all.
__global__ __launch_bounds__(256) void lovasz_scatter_kernel(const u64* __restrict__ src, u64* __restrict__ dst, long long M, int shift,
                                                            const unsigned* __restrict__ offs) {
  __shared__ unsigned short cnt[LV_SEG][256];             // per segment and digit: first the count, then the exclusive prefix over the segments
  __shared__ unsigned dstart[256];                        // where the digit's run begins in the staged tile
  __shared__ unsigned gbase[256];                         // global offset of the digit's run minus dstart (mod 2^32)
  __shared__ unsigned wtot[4];
  __shared__ u64 stage[LV_T];
  const long long tile = blockIdx.x;
  const u64* s = src + (size_t)blockIdx.y * M;
  u64* o = dst + (size_t)blockIdx.y * M;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < LV_SEG * 256; i += 256) (&cnt[0][0])[i] = 0;
  __syncthreads();
  u64 v[LV_PER]; unsigned short lrank[LV_PER];
  const u64 below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int r = 0; r < LV_PER; ++r) {
    const long long i = tile * LV_T + r * 256 + threadIdx.x;
    const bool act = i < M;
    v[r] = act ? s[i] : 0ull;
    const unsigned dg = (unsigned)(v[r] >> shift) & 255u;
    u64 mask = __ballot(act);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const u64 bm = __ballot((dg >> b) & 1u);
      mask &= ((dg >> b) & 1u) ? bm : ~bm;
    }
    lrank[r] = (unsigned short)__popcll(mask & below);
    if (act && (mask & below) == 0) cnt[r * 4 + wave][dg] = (unsigned short)__popcll(mask);
  }
  __syncthreads();
  {
    const int d = threadIdx.x;
    unsigned run = 0;
#pragma unroll
    for (int sg = 0; sg < LV_SEG; ++sg) { const unsigned c = cnt[sg][d]; cnt[sg][d] = (unsigned short)run; run += c; }
    unsigned incl = run;                                  // exclusive scan of the 256 digit totals
#pragma unroll
    for (int of = 1; of < 64; of <<= 1) {
      const unsigned t = (unsigned)__shfl_up((int)incl, of, 64);
      if (lane >= of) incl += t;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    unsigned ex = incl - run;
    for (int w = 0; w < wave; ++w) ex += wtot[w];
    dstart[d] = ex;
    gbase[d] = offs[((size_t)blockIdx.y * gridDim.x + tile) * 256 + d] - ex;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < LV_PER; ++r) {
    const long long i = tile * LV_T + r * 256 + threadIdx.x;
    if (i < M) {
      const unsigned dg = (unsigned)(v[r] >> shift) & 255u;
      stage[dstart[dg] + cnt[r * 4 + wave][dg] + lrank[r]] = v[r];
    }
  }
  __syncthreads();
  const long long left = M - tile * LV_T;
  const int nin = left < LV_T ? (int)left : LV_T;
  for (int j = threadIdx.x; j < nin; j += 256) {
    const u64 x = stage[j];
    const unsigned dg = (unsigned)(x >> shift) & 255u;
    o[(size_t)(unsigned)(gbase[dg] + (unsigned)j)] = x;   // < M by construction: the offsets of a class add up to M
  }
}

__global__ __launch_bounds__(256) void lovasz_fgsum_kernel(const u64* __restrict__ sorted, long long M, unsigned* __restrict__ tsum) {
  __shared__ unsigned sh[4];
  const long long tile = blockIdx.x;
  const u64* s = sorted + (size_t)blockIdx.y * M;
  unsigned c = 0;
#pragma unroll
  for (int r = 0; r < LV_PER; ++r) {
    const long long i = tile * LV_T + r * 256 + threadIdx.x;
    if (i < M) c += (unsigned)(s[i] >> 31) & 1u;
  }
#pragma unroll
  for (int of = 32; of > 0; of >>= 1) c += (unsigned)__shfl_xor((int)c, of, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tsum[(size_t)blockIdx.y * gridDim.x + tile] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one block per class: tsum[c][tile] becomes the number of foreground pairs in front of the tile
__global__ __launch_bounds__(1024) void lovasz_fgscan_kernel(unsigned* __restrict__ tsum, long long ntiles) {
  __shared__ unsigned wsum[16];
  unsigned* t = tsum + (size_t)blockIdx.x * ntiles;
  const long long per = (ntiles + 1023) / 1024;
  const long long t0 = (long long)threadIdx.x * per, t1 = (t0 + per < ntiles) ? t0 + per : ntiles;
  unsigned s = 0;
  for (long long i = t0; i < t1; ++i) s += t[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = s;
#pragma unroll
  for (int of = 1; of < 64; of <<= 1) {
    const unsigned v = (unsigned)__shfl_up((int)incl, of, 64);
    if (lane >= of) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  unsigned run = incl - s;
  for (int w = 0; w < wave; ++w) run += wsum[w];
  for (long long i = t0; i < t1; ++i) { const unsigned c = t[i]; t[i] = run; run += c; }
}

__device__ __forceinline__ double lv_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// thread t owns the ranks tile * LV_T + t * 8 .. + 7: a sequential prefix in the thread, a block scan of the threads' counts
__global__ __launch_bounds__(256) void lovasz_apply_kernel(const u64* __restrict__ sorted, long long M, int C, int all_classes, const unsigned* __restrict__ tpre,
                                                          const LvCounters* __restrict__ cnt, float* __restrict__ dp, unsigned* __restrict__ order,
                                                          double* __restrict__ part) {
  __shared__ unsigned wsum[4];
  __shared__ double shs[4];
  const long long tile = blockIdx.x;
  const int c = blockIdx.y;
  const u64* s = sorted + (size_t)c * M;
  const long long n = cnt->n_valid, G = cnt->G[c];
  const bool counted = n > 0 && (all_classes || G > 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = tile * LV_T + (long long)threadIdx.x * LV_PER;
  u64 v[LV_PER]; unsigned f = 0;
#pragma unroll
  for (int j = 0; j < LV_PER; ++j) {
    v[j] = (r0 + j < M) ? s[r0 + j] : 0ull;
    f += (unsigned)(v[j] >> 31) & 1u;
  }
  unsigned incl = f;
#pragma unroll
  for (int of = 1; of < 64; of <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)incl, of, 64);
    if (lane >= of) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  long long F = (long long)tpre[(size_t)c * gridDim.x + tile] + (long long)(incl - f);      // foreground pairs in front of rank r0
  for (int w = 0; w < wave; ++w) F += wsum[w];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < LV_PER; ++j) {
    const long long r = r0 + j;
    if (r >= M) break;
    const unsigned lo = (unsigned)v[j];
    const unsigned pix = lo & 0x7fffffffu;
    const long long fg = lo >> 31;
    float g = 0.0f;
    if (counted && r < n) {
      const long long Fr = F + fg;
      const double jprev = r == 0 ? 0.0 : 1.0 - (double)(G - F) / (double)(G + r - F);
      const double jr = 1.0 - (double)(G - Fr) / (double)(G + (r + 1) - Fr);
      const double w = jr - jprev;
      const float wf = (float)w;
      g = fg ? -wf : wf;
      acc += (double)lv_unkey(~(unsigned)(v[j] >> 32)) * w;
    }
    F += fg;
    if (dp != nullptr) dp[(size_t)pix * C + c] = g;
    if (order != nullptr) order[(size_t)c * M + r] = pix;
  }
  acc = lv_wave_sum_f64(acc);
  if (lane == 0) shs[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)c * gridDim.x + tile] = ((shs[0] + shs[1]) + shs[2]) + shs[3];
}

// One block.  Wave w adds the tile partials of the classes w, w + 4, .. in tile order (lane 0 takes the 64 loaded values one by one); thread 0
// then adds the classes in order.
__global__ __launch_bounds__(256) void lovasz_finish_kernel(const double* __restrict__ part, long long ntiles, int C, int all_classes, float loss_weight,
                                                           const LvCounters* __restrict__ cnt, double* loss_out, rua_lovasz_result* __restrict__ res) {
  __shared__ double lc[RUA_LOVASZ_MAX_C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c < C; c += 4) {
    double sum = 0.0;
    for (long long base = 0; base < ntiles; base += 64) {
      const double v = (base + lane < ntiles) ? part[(size_t)c * ntiles + base + lane] : 0.0;
      const int cntl = ntiles - base < 64 ? (int)(ntiles - base) : 64;
      for (int l = 0; l < cntl; ++l) sum += __shfl(v, l, 64);
    }
    if (lane == 0) lc[c] = sum;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long n = cnt->n_valid;
  int ncls = 0; double loss = 0.0;
  for (int c = 0; c < RUA_LOVASZ_MAX_C; ++c) {
    const long long G = c < C ? cnt->G[c] : 0;
    const bool counted = c < C && n > 0 && (all_classes || G > 0);
    res->G[c] = G;
    res->loss_c[c] = counted ? lc[c] : 0.0;
    if (counted) { ++ncls; loss += lc[c]; }
  }
  loss = ncls > 0 ? loss / (double)ncls : 0.0;
  res->n_valid = n; res->n_cls = ncls;
  res->scale = ncls > 0 ? (float)((double)loss_weight / (double)ncls) : 0.0f;
  res->loss = loss;
  if (ncls > 0) {                                       // two roundings: the product passes through an empty asm statement, so the sum cannot take it as an fma
    double t = __dmul_rn((double)loss_weight, loss);
    asm volatile("" : "+v"(t));
    loss_out[0] = __dadd_rn(loss_out[0], t);
  }
}

// d(total)/d(logits) from dp: every operation rounded on its own, host_lovasz_dz's order.  __fmul_rn / __fadd_rn are plain operators in HIP's
// headers and the backend fuses a product into the sum that follows it, so the products g * p pass through an empty asm statement first (as
// ema_update in loss_optim.hip does); no other product here feeds a sum.  A pixel whose dp is +-0 in every
// class (every void pixel is one) leaves as +0.0f by a select, whatever p holds there.
template <int ACT>
__global__ __launch_bounds__(256) void lovasz_dz_kernel(const float* __restrict__ p, const float* __restrict__ dp, const float* __restrict__ scale_dev,
                                                       long long M, int C, float* __restrict__ dz) {
  const float scale = scale_dev[0];
  if (ACT == RUA_ACT_SIGMOID) {                            // per element: the flat index, fully coalesced
    const long long n = M * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
      const float g = dp[i], q = p[i];
      dz[i] = g != 0.0f ? __fmul_rn(scale, __fmul_rn(g, __fmul_rn(q, __fsub_rn(1.0f, q)))) : 0.0f;
    }
    return;
  }
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
    const float* pp = p + (size_t)m * C;
    const float* gg = dp + (size_t)m * C;
    float* out = dz + (size_t)m * C;
    float s = 0.0f; bool any = false;
    for (int c = 0; c < C; ++c) {
      float t = __fmul_rn(gg[c], pp[c]);
      asm volatile("" : "+v"(t));
      s = c == 0 ? t : __fadd_rn(s, t);
      any = any || gg[c] != 0.0f;
    }
    for (int c = 0; c < C; ++c) out[c] = any ? __fmul_rn(scale, __fmul_rn(pp[c], __fsub_rn(gg[c], s))) : 0.0f;
  }
}

static inline bool lv_shape_ok(int64_t M, int C) {
  return C >= 1 && C <= RUA_LOVASZ_MAX_C && M >= 1 && M < ((int64_t)1 << 31) && M * (int64_t)C < ((int64_t)1 << 32);
}

extern "C" int rua_lovasz_tile(void) { return LV_T; }

extern "C" int64_t rua_lovasz_workspace_bytes(int64_t M, int C) {
  if (!lv_shape_ok(M, C)) return -1;
  return lv_layout(M, C).total;
}

extern "C" int rua_lovasz_grad(const float* p, const float* y, const uint8_t* void_mask, int64_t M, int C, int all_classes, float loss_weight,
                               void* workspace, int64_t workspace_bytes, double* loss_out, float* dp, uint32_t* order_out,
                               rua_lovasz_result* result_dev, void* stream) {
  RUA_CHECK_ARG(p && y && workspace && loss_out && result_dev, "rua_lovasz_grad: null argument");
  RUA_CHECK_ARG(C >= 1 && C <= RUA_LOVASZ_MAX_C, "rua_lovasz_grad: C=%d must be in 1..%d", C, RUA_LOVASZ_MAX_C);
  RUA_CHECK_ARG(M >= 1 && M < ((int64_t)1 << 31), "rua_lovasz_grad: M=%lld must be in 1..2^31-1", (long long)M);
  RUA_CHECK_ARG(M * (int64_t)C < ((int64_t)1 << 32), "rua_lovasz_grad: M*C=%lld must be below 2^32", (long long)(M * (int64_t)C));
  RUA_CHECK_ARG(all_classes == 0 || all_classes == 1, "rua_lovasz_grad: all_classes must be 0 or 1");
  const LvLayout l = lv_layout(M, C);
  RUA_CHECK_ARG(workspace_bytes >= l.total, "rua_lovasz_grad: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)l.total);
  RUA_CHECK_ARG(((size_t)workspace & 7) == 0 && ((size_t)loss_out & 7) == 0 && ((size_t)result_dev & 7) == 0 && ((size_t)p & 3) == 0 && ((size_t)y & 3) == 0 &&
                ((size_t)dp & 3) == 0 && ((size_t)order_out & 3) == 0, "rua_lovasz_grad: misaligned buffer");
  char* ws = (char*)workspace;
  u64* A = (u64*)(ws + l.a);
  u64* B = (u64*)(ws + l.b);
  unsigned* hist = (unsigned*)(ws + l.hist);
  unsigned* tsum = (unsigned*)(ws + l.tsum);
  double* part = (double*)(ws + l.part);
  LvCounters* cnt = (LvCounters*)(ws + l.cnt);
  const long long nt = lv_tiles(M);
  const int kg = (int)((M + 255) / 256 > 2048 ? 2048 : (M + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  const dim3 tiles((unsigned)nt, (unsigned)C);
  hipLaunchKernelGGL(lovasz_zero_kernel, dim3(1), dim3(64), 0, st, cnt);
  hipLaunchKernelGGL(lovasz_key_kernel, dim3(kg), dim3(256), 0, st, p, y, void_mask, (long long)M, C, A, cnt);
  u64 *src = A, *dst = B;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 32 + 8 * pass;
    hipLaunchKernelGGL(lovasz_hist_kernel, tiles, dim3(256), 0, st, (const u64*)src, (long long)M, shift, hist);
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3(C), dim3(1024), 0, st, hist, nt);
    hipLaunchKernelGGL(lovasz_scatter_kernel, tiles, dim3(256), 0, st, (const u64*)src, dst, (long long)M, shift, (const unsigned*)hist);
    u64* t = src; src = dst; dst = t;
  }
  hipLaunchKernelGGL(lovasz_fgsum_kernel, tiles, dim3(256), 0, st, (const u64*)src, (long long)M, tsum);
  hipLaunchKernelGGL(lovasz_fgscan_kernel, dim3(C), dim3(1024), 0, st, tsum, nt);
  hipLaunchKernelGGL(lovasz_apply_kernel, tiles, dim3(256), 0, st, (const u64*)src, (long long)M, C, all_classes, (const unsigned*)tsum, (const LvCounters*)cnt,
                     dp, order_out, part);
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nt, C, all_classes, loss_weight, (const LvCounters*)cnt, loss_out, result_dev);
  RUA_LAUNCH_CHECK("rua_lovasz_grad");
  return RUA_OK;
}

extern "C" int rua_lovasz_dz(int act, const float* p, const float* dp, const float* scale_dev, int64_t M, int C, float* dz, void* stream) {
  RUA_CHECK_ARG(p && dp && scale_dev && dz, "rua_lovasz_dz: null argument");
  RUA_CHECK_ARG(act == RUA_ACT_SOFTMAX || act == RUA_ACT_SIGMOID, "rua_lovasz_dz: act=%d must be softmax or sigmoid", act);
  RUA_CHECK_ARG(lv_shape_ok(M, C), "rua_lovasz_dz: M=%lld, C=%d out of range", (long long)M, C);
  const int g = (int)((M + 255) / 256 > 4096 ? 4096 : (M + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  if (act == RUA_ACT_SOFTMAX) hipLaunchKernelGGL(lovasz_dz_kernel<RUA_ACT_SOFTMAX>, dim3(g), dim3(256), 0, st, p, dp, scale_dev, (long long)M, C, dz);
  else hipLaunchKernelGGL(lovasz_dz_kernel<RUA_ACT_SIGMOID>, dim3(g), dim3(256), 0, st, p, dp, scale_dev, (long long)M, C, dz);
  RUA_LAUNCH_CHECK("rua_lovasz_dz");
  return RUA_OK;
}

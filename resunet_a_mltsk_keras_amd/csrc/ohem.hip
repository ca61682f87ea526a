// Online hard example mining: the exact k-th-largest selection over a head's per-pixel loss map (include/rua_hip.h, rua_ohem_select; the package's
// losses.py holds the definition, host_ohem).
//
// SIX launches whatever the map holds, none waits for another, nothing is read back:
//   1  ohem_zero_kernel       the three global histograms of the workspace
//   2  ohem_hist_kernel<1>    digit 1 = key bits 31..21 (2048 bins) of every valid pixel; the bins' total is n_valid
//   3  ohem_hist_kernel<2>    digit 2 = key bits 20..10 (2048 bins) of the valid pixels whose digit 1 is the chosen one
//   4  ohem_hist_kernel<3>    digit 3 = key bits 9..0 (1024 bins) of those whose digits 1 and 2 are the chosen ones
//   5  ohem_mask_kernel       drop_mask, and per block the count and the fp64 sum of the kept pixels
//   6  ohem_finish_kernel     one block: the partials through LDS, thread 0 adds them in block order; the result struct, loss_out[0] += mean
// A pass builds its histogram in LDS with integer atomics and flushes the non-empty bins to the global one with integer atomics: integer sums are
// the same in any order.  The digit chosen so far is derived by EVERY block itself from the previous passes' global histograms (ohem_resolve: a
// block scan over 256 threads from the top bin down), so there is no pick launch and no block waits for another.  K needs n_valid, the total of
// pass 1, and t, the device's step counter: both are read on the device.
// The hot spot - a map whose values are (nearly) all equal puts every lane of a wave on ONE LDS bin - is taken out inside the wave: the lanes whose
// bin is the first active lane's are counted by a ballot and added by that lane alone; the others add for themselves.  An all-equal wave costs one
// LDS atomic instead of 64 serialised ones, a spread-out wave one ballot more than before.
// The kept sum is deterministic: the grid is a function of M alone, a thread adds its pixels in index order in fp64, the lanes of a wave are folded
// by a fixed butterfly, the four waves and then the blocks are added in order (the way rua_grad_sumsq / rua_clip_finish do it).
// Plain stores and ordinary atomics only.
#include "common.h"

#define OHEM_B1 2048
#define OHEM_B2 2048
#define OHEM_B3 1024
#define OHEM_BINS (OHEM_B1 + OHEM_B2 + OHEM_B3)
#define OHEM_MAX_BLOCKS 1024
typedef unsigned long long u64;

// workspace: u64 hist[OHEM_BINS]; OhemPartial part[blocks]; OhemHead head
struct OhemPartial { double sum; long long kept; };
struct OhemHead { long long n_valid, K; unsigned tau_key; int q16; };
static inline int ohem_blocks(int64_t M) { const int64_t g = (M + 1023) / 1024; return (int)(g < 1 ? 1 : g > OHEM_MAX_BLOCKS ? OHEM_MAX_BLOCKS : g); }
static inline int64_t ohem_ws_bytes(int64_t M) { return (int64_t)OHEM_BINS * 8 + (int64_t)ohem_blocks(M) * (int64_t)sizeof(OhemPartial) + (int64_t)sizeof(OhemHead); }

// the order-preserving key of a float32: negatives with all bits flipped, non-negatives with the sign bit set (-0 < +0), every NaN the largest key
__device__ __forceinline__ unsigned ohem_key(float v) {
  const unsigned b = __float_as_uint(v);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static inline unsigned ohem_key_host(float v) {
  unsigned b; memcpy(&b, &v, 4);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ohem_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// Block-wide: which bin holds the rank-th largest entry of hist[nbins] (nbins = 256 * PER, rank counted from the top bin down, 1-based), and the
// rank inside that bin.  rank_of(total) turns the histogram's total into the rank (pass 1 derives K from n_valid there).  sc: 258 u64 of LDS.
// A rank of 0 or beyond the total (an empty histogram: no valid pixel) chooses bin 0 with rank 0.  Ends with a block barrier.
template <int PER, typename RankOf>
__device__ __forceinline__ void ohem_pick(const u64* __restrict__ hist, u64* sc, RankOf&& rank_of, unsigned& digit, u64& rank_in, u64& total) {
  const int t = threadIdx.x;
  const int hi = 256 * PER - 1 - t * PER;               // thread t owns bins hi, hi - 1, .. hi - PER + 1: thread order = descending key order
  u64 c[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) { c[j] = hist[hi - j]; s += c[j]; }
  const int lane = t & 63, wave = t >> 6;
  u64 incl = s;                                         // inclusive scan over the threads: shuffles inside a wave, the four wave totals through LDS
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) sc[wave] = incl;
  if (t == 0) { sc[256] = 0; sc[257] = 0; }
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += sc[w];
  total = ((sc[0] + sc[1]) + sc[2]) + sc[3];
  const u64 rank = rank_of(total);
  u64 acc = incl - s;
  if (acc < rank && rank <= incl) {                     // exactly one thread for 1 <= rank <= total
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (acc < rank && rank <= acc + c[j]) { sc[256] = (u64)(hi - j); sc[257] = rank - acc; }
      acc += c[j];
    }
  }
  __syncthreads();
  digit = (unsigned)sc[256]; rank_in = sc[257];
  __syncthreads();
}

// K of the definition from n_valid, the options and the step counter; q16: the share used
__device__ __forceinline__ long long ohem_K(long long n_valid, const rua_ohem_opts& o, const double* __restrict__ step_state, int& q16) {
  q16 = o.keep_q16;
  if (o.warmup > 0 && step_state != nullptr) {
    long long t = (long long)step_state[0];
    if (t < 0) t = 0;
    if (t > o.warmup) t = o.warmup;
    q16 = 65536 - (int)(((long long)(65536 - o.keep_q16) * t) / o.warmup);
  }
  long long k = (n_valid * (long long)q16 + 65535) >> 16;
  if (k < o.min_kept) k = o.min_kept;
  return k < n_valid ? k : n_valid;
}

// What the passes 1 .. NP decided, by every block for itself: n_valid, K, and the key bits chosen so far (prefix, in key position)
template <int NP>
__device__ __forceinline__ void ohem_resolve(const u64* __restrict__ hist, u64* sc, const rua_ohem_opts& o, const double* __restrict__ step_state,
                                             long long& n_valid, long long& K, int& q16, unsigned& prefix) {
  unsigned d; u64 r, tot;
  long long k = 0; int q = o.keep_q16;
  ohem_pick<OHEM_B1 / 256>(hist, sc, [&](u64 total) { k = ohem_K((long long)total, o, step_state, q); return (u64)k; }, d, r, tot);
  n_valid = (long long)tot; K = k; q16 = q; prefix = d << 21;
  if constexpr (NP >= 2) {
    const u64 r1 = r;
    ohem_pick<OHEM_B2 / 256>(hist + OHEM_B1, sc, [&](u64) { return r1; }, d, r, tot);
    prefix |= d << 10;
  }
  if constexpr (NP >= 3) {
    const u64 r2 = r;
    ohem_pick<OHEM_B3 / 256>(hist + OHEM_B1 + OHEM_B2, sc, [&](u64) { return r2; }, d, r, tot);
    prefix |= d;
  }
}

__global__ __launch_bounds__(256) void ohem_zero_kernel(u64* __restrict__ hist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < OHEM_BINS) hist[i] = 0;
}

template <int PASS>
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ L, const uint8_t* __restrict__ vm, long long M, const rua_ohem_opts o,
                                                        const double* __restrict__ step_state, u64* __restrict__ hist) {
  constexpr int NB = PASS == 3 ? OHEM_B3 : OHEM_B1;
  __shared__ unsigned h[NB];
  __shared__ u64 sc[258];
  for (int b = threadIdx.x; b < NB; b += 256) h[b] = 0;
  unsigned prefix = 0;
  if constexpr (PASS >= 2) {
    long long nv, K; int q16;
    ohem_resolve<PASS - 1>(hist, sc, o, step_state, nv, K, q16, prefix);
    if (K == 0) return;                                 // no valid pixel (block-uniform): nothing to count
  } else {
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256; base < M; base += (long long)gridDim.x * 256) {     // block-uniform trip count
    const long long m = base + threadIdx.x;
    bool act = m < M;
    if (act && vm != nullptr) act = vm[m] == 0;
    unsigned bin = 0;
    if (act) {
      const unsigned k = ohem_key(L[m]);
      if constexpr (PASS == 1) bin = k >> 21;
      else if constexpr (PASS == 2) { act = (k >> 21) == (prefix >> 21); bin = (k >> 10) & 2047u; }
      else { act = (k >> 10) == (prefix >> 10); bin = k & 1023u; }
    }
    const u64 am = __ballot(act);
    if (am != 0) {                                      // the lanes on the first active lane's bin: one atomic for all of them
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
  u64* dst = hist + (PASS == 1 ? 0 : PASS == 2 ? OHEM_B1 : OHEM_B1 + OHEM_B2);
  for (int b = threadIdx.x; b < NB; b += 256) {
    const unsigned v = h[b];
    if (v != 0) atomicAdd(&dst[b], (u64)v);
  }
}

__device__ __forceinline__ double ohem_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long ohem_wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void ohem_mask_kernel(const float* __restrict__ L, const uint8_t* __restrict__ vm, long long M, const rua_ohem_opts o,
                                                        const double* __restrict__ step_state, const u64* __restrict__ hist, unsigned thresh_key,
                                                        uint8_t* __restrict__ drop, OhemPartial* __restrict__ part, OhemHead* __restrict__ head) {
  __shared__ u64 sc[258];
  __shared__ double shs[4];
  __shared__ long long shc[4];
  long long nv, K; int q16; unsigned tau;
  ohem_resolve<3>(hist, sc, o, step_state, nv, K, q16, tau);
  if (K == 0) tau = 0xffffffffu;                        // no valid pixel: nothing is kept whatever the threshold
  if (o.has_thresh && thresh_key < tau) tau = thresh_key;
  if (blockIdx.x == 0 && threadIdx.x == 0) { head->n_valid = nv; head->K = K; head->tau_key = tau; head->q16 = q16; }
  double acc = 0.0; long long cnt = 0;
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
    bool keep = vm == nullptr || vm[m] == 0;
    const float v = L[m];
    keep = keep && ohem_key(v) >= tau;
    drop[m] = keep ? 0 : 1;
    if (keep) { acc += (double)v; ++cnt; }
  }
  acc = ohem_wave_sum_f64(acc); cnt = ohem_wave_sum_i64(cnt);
  if ((threadIdx.x & 63) == 0) { shs[threadIdx.x >> 6] = acc; shc[threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x].sum = ((shs[0] + shs[1]) + shs[2]) + shs[3];
    part[blockIdx.x].kept = ((shc[0] + shc[1]) + shc[2]) + shc[3];
  }
}

// One block.  The partials pass through LDS (coalesced loads by all threads: a thread that walks them in global memory pays a load latency per
// block); thread 0 adds the sums in block order, the counts are integers and any order gives the same.
__global__ __launch_bounds__(256) void ohem_finish_kernel(const OhemPartial* __restrict__ part, int nblocks, const OhemHead* __restrict__ head, float loss_weight,
                                                          double* loss_out, rua_ohem_result* __restrict__ res) {
  __shared__ double ss[OHEM_MAX_BLOCKS];
  __shared__ long long sk[OHEM_MAX_BLOCKS];
  for (int b = threadIdx.x; b < nblocks; b += 256) { ss[b] = part[b].sum; sk[b] = part[b].kept; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0; long long n = 0;
  for (int b = 0; b < nblocks; ++b) { s += ss[b]; n += sk[b]; }
  res->tau_key = head->tau_key; res->tau = ohem_unkey(head->tau_key);
  res->n_valid = head->n_valid; res->n_kept = n; res->K = head->K;
  res->kept_sum = n > 0 ? s : 0.0;
  res->scale = n > 0 ? (float)((double)loss_weight / (double)n) : 0.f;
  res->q16_used = head->q16;
  if (n > 0) loss_out[0] += s / (double)n;
}

extern "C" int64_t rua_ohem_workspace_bytes(int64_t M) {
  if (M < 1 || M > ((int64_t)1 << 40)) return -1;
  return ohem_ws_bytes(M);
}

extern "C" int rua_ohem_select(const float* per_pixel, const uint8_t* void_mask, int64_t M, const rua_ohem_opts* opts, const double* step_state,
                               float loss_weight, void* workspace, int64_t workspace_bytes, uint8_t* drop_mask, double* loss_out,
                               rua_ohem_result* result_dev, void* stream) {
  RUA_CHECK_ARG(per_pixel && opts && workspace && drop_mask && loss_out && result_dev, "rua_ohem_select: null argument");
  RUA_CHECK_ARG(M >= 1 && M <= ((int64_t)1 << 40), "rua_ohem_select: M=%lld must be in 1..2^40", (long long)M);
  RUA_CHECK_ARG(opts->keep_q16 >= 1 && opts->keep_q16 <= 65536, "rua_ohem_select: keep_q16=%d must be in 1..65536", opts->keep_q16);
  RUA_CHECK_ARG(opts->min_kept >= 0, "rua_ohem_select: min_kept=%lld is negative", (long long)opts->min_kept);
  RUA_CHECK_ARG(opts->warmup >= 0, "rua_ohem_select: warmup=%d is negative", opts->warmup);
  RUA_CHECK_ARG(opts->has_thresh == 0 || opts->has_thresh == 1, "rua_ohem_select: has_thresh must be 0 or 1");
  RUA_CHECK_ARG(!opts->has_thresh || opts->thresh == opts->thresh, "rua_ohem_select: thresh is NaN");
  RUA_CHECK_ARG(workspace_bytes >= ohem_ws_bytes(M), "rua_ohem_select: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)ohem_ws_bytes(M));
  RUA_CHECK_ARG(((size_t)workspace & 7) == 0 && ((size_t)loss_out & 7) == 0 && ((size_t)result_dev & 7) == 0 && ((size_t)per_pixel & 3) == 0 &&
                (step_state == nullptr || ((size_t)step_state & 7) == 0), "rua_ohem_select: misaligned buffer");
  const int G = ohem_blocks(M);
  u64* hist = (u64*)workspace;
  OhemPartial* part = (OhemPartial*)(hist + OHEM_BINS);
  OhemHead* head = (OhemHead*)(part + G);
  const unsigned tk = opts->has_thresh ? ohem_key_host(opts->thresh) : 0u;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ohem_zero_kernel, dim3(OHEM_BINS / 256), dim3(256), 0, st, hist);
  hipLaunchKernelGGL(ohem_hist_kernel<1>, dim3(G), dim3(256), 0, st, per_pixel, void_mask, (long long)M, *opts, step_state, hist);
  hipLaunchKernelGGL(ohem_hist_kernel<2>, dim3(G), dim3(256), 0, st, per_pixel, void_mask, (long long)M, *opts, step_state, hist);
  hipLaunchKernelGGL(ohem_hist_kernel<3>, dim3(G), dim3(256), 0, st, per_pixel, void_mask, (long long)M, *opts, step_state, hist);
  hipLaunchKernelGGL(ohem_mask_kernel, dim3(G), dim3(256), 0, st, per_pixel, void_mask, (long long)M, *opts, step_state, (const u64*)hist, tk, drop_mask, part, head);
  hipLaunchKernelGGL(ohem_finish_kernel, dim3(1), dim3(256), 0, st, (const OhemPartial*)part, G, (const OhemHead*)head, loss_weight, loss_out, result_dev);
  RUA_LAUNCH_CHECK("rua_ohem_select");
  return RUA_OK;
}

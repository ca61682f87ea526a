// Loss heads, metrics and optimizers.  Everything here is fp32 on [B][HW][C] probabilities and
// labels with fp64 accumulators; per-pixel work is HBM-bound, reductions are wavefront
// shuffles + one fp64 atomic per block and value.
#include "common.h"

__device__ __forceinline__ void block_atomic_add(double* dst, float v, float* sh /*[4]*/, int slot) {
  // every thread calls; wave shuffle -> LDS -> one fp64 atomic
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) sh[slot * 4 + wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) unsafeAtomicAdd(dst, (double)sh[slot * 4 + 0] + (double)sh[slot * 4 + 1] + (double)sh[slot * 4 + 2] + (double)sh[slot * 4 + 3]);
  __syncthreads();
}

// ---- Tanimoto with complement (multitasking_utils.py:38-85) ------------------------------
// sums[n][c][6] = { sum p, sum (1-l), sum p*l, sum p^2+l^2, sum (1-p)(1-l), sum (1-p)^2+(1-l)^2 }
// VM: void_mask[n * HW + i] != 0 takes pixel i of sample n out of every sum (by select: p and y may hold anything there), as if it were cut out
// of the image; the unmasked instantiation is the code it was.
template <bool VM>
__global__ __launch_bounds__(256) void tanimoto_sums_kernel(const float* __restrict__ p, const float* __restrict__ y, long long HW, int C,
                                                            int pix_per_block, double* sums, const uint8_t* __restrict__ vm) {
  __shared__ float sh[4 * 48];
  const int n = blockIdx.y;
  float acc[8][6];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[c][k] = 0.f;
  long long i = (long long)blockIdx.x * pix_per_block + threadIdx.x;
  long long iend = (long long)(blockIdx.x + 1) * pix_per_block; if (iend > HW) iend = HW;
  for (; i < iend; i += 256) {
    if constexpr (VM) { if (vm[(size_t)n * HW + i]) continue; }
    const float* pp = p + ((size_t)n * HW + i) * C;
    const float* yy = y + ((size_t)n * HW + i) * C;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        const float a = pp[c], l = yy[c], q = 1.f - a, m = 1.f - l;
        acc[c][0] += a; acc[c][1] += m; acc[c][2] = fmaf(a, l, acc[c][2]);
        acc[c][3] += a * a + l * l; acc[c][4] = fmaf(q, m, acc[c][4]); acc[c][5] += q * q + m * m;
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const float v = wave_sum(acc[c][k]);
      if (lane == 0) sh[wid * 48 + c * 6 + k] = v;
    }
  __syncthreads();
  if (threadIdx.x < 48) {
    const int c = threadIdx.x / 6, k = threadIdx.x % 6;
    if (c < C) {
      const double t = (double)sh[threadIdx.x] + (double)sh[48 + threadIdx.x] + (double)sh[96 + threadIdx.x] + (double)sh[144 + threadIdx.x];
      unsafeAtomicAdd(&sums[((size_t)n * C + c) * 6 + k], t);
    }
  }
}

// Same sums with 16-byte loads for the class counts the reference's heads use: a thread takes G pixels (G * C floats = NV
// float4) per iteration from each tensor, all loads issued before the first use; the class of every element is a
// compile-time constant.  (The scalar kernel above streams at ~1.5 TB/s.)
template <int C, int G, bool VM>
__global__ __launch_bounds__(256) void tanimoto_sums_vec(const float* __restrict__ p, const float* __restrict__ y, long long HW,
                                                         int groups_per_block, double* sums, const uint8_t* __restrict__ vm) {
  constexpr int NV = G * C / 4;
  static_assert(G * C % 4 == 0, "group must be whole float4s");
  __shared__ float sh[4 * 48];
  const int n = blockIdx.y;
  float acc[C][6];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[c][k] = 0.f;
  const long long ngroups = HW / G;
  long long gi = (long long)blockIdx.x * groups_per_block + threadIdx.x;
  long long gend = (long long)(blockIdx.x + 1) * groups_per_block; if (gend > ngroups) gend = ngroups;
  const float4* pp = reinterpret_cast<const float4*>(p + (size_t)n * HW * C);
  const float4* yy = reinterpret_cast<const float4*>(y + (size_t)n * HW * C);
  for (; gi < gend; gi += 256) {
    float4 a4[NV], l4[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) { a4[v] = pp[gi * NV + v]; l4[v] = yy[gi * NV + v]; }
    bool vd[G];
#pragma unroll
    for (int g = 0; g < G; ++g) vd[g] = VM ? vm[(size_t)n * HW + gi * G + g] != 0 : false;      // (byte loads: the mask has no alignment)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float av[4] = {a4[v].x, a4[v].y, a4[v].z, a4[v].w}, lv[4] = {l4[v].x, l4[v].y, l4[v].z, l4[v].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (v * 4 + j) % C;
        if (VM && vd[(v * 4 + j) / C]) continue;
        const float a = av[j], l = lv[j], q = 1.f - a, m = 1.f - l;
        acc[c][0] += a; acc[c][1] += m; acc[c][2] = fmaf(a, l, acc[c][2]);
        acc[c][3] += a * a + l * l; acc[c][4] = fmaf(q, m, acc[c][4]); acc[c][5] += q * q + m * m;
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const float v = wave_sum(acc[c][k]);
      if (lane == 0) sh[wid * 48 + c * 6 + k] = v;
    }
  __syncthreads();
  if (threadIdx.x < C * 6) {
    const double t = (double)sh[threadIdx.x] + (double)sh[48 + threadIdx.x] + (double)sh[96 + threadIdx.x] + (double)sh[144 + threadIdx.x];
    unsafeAtomicAdd(&sums[(size_t)n * C * 6 + threadIdx.x], t);
  }
}

template <int C, int G>
static void launch_tanimoto_vec(const float* p, const float* y, const uint8_t* vm, int B, int64_t HW, double* sums, hipStream_t st) {
  const int64_t ngroups = HW / G;
  int64_t gpb = (ngroups + 63) / 64; if (gpb < 256) gpb = 256;         // ~64 blocks per sample
  gpb = (gpb + 255) / 256 * 256;
  const int gx = (int)((ngroups + gpb - 1) / gpb);
  if (vm) hipLaunchKernelGGL((tanimoto_sums_vec<C, G, true>), dim3(gx, B), dim3(256), 0, st, p, y, (long long)HW, (int)gpb, sums, vm);
  else hipLaunchKernelGGL((tanimoto_sums_vec<C, G, false>), dim3(gx, B), dim3(256), 0, st, p, y, (long long)HW, (int)gpb, sums, vm);
}

extern "C" int rua_tanimoto_sums_void(const float* p, const float* y, const uint8_t* void_mask, int B, int64_t HW, int C, double* sums, void* stream) {
  RUA_CHECK_ARG(p && y && sums && B > 0 && HW > 0, "rua_tanimoto_sums: bad arguments");
  RUA_CHECK_ARG(C >= 1 && C <= 8, "rua_tanimoto_sums: C=%d must be in 1..8", C);
  const int vec_on = g_tune.tani_vec;
  if (vec_on && HW % 4 == 0 && ((size_t)p & 15) == 0 && ((size_t)y & 15) == 0 && (C == 6 || C == 3 || C == 2)) {
    if (C == 6) launch_tanimoto_vec<6, 2>(p, y, void_mask, B, HW, sums, (hipStream_t)stream);
    else if (C == 3) launch_tanimoto_vec<3, 4>(p, y, void_mask, B, HW, sums, (hipStream_t)stream);
    else launch_tanimoto_vec<2, 2>(p, y, void_mask, B, HW, sums, (hipStream_t)stream);
    RUA_LAUNCH_CHECK("rua_tanimoto_sums");
    return RUA_OK;
  }
  int64_t ppb = (HW + 127) / 128; if (ppb < 1024) ppb = 1024;      // measured: 64..256 blocks per sample all ~17 us, 16: 21, 8: 35
  ppb = (ppb + 255) / 256 * 256;
  const int gx = (int)((HW + ppb - 1) / ppb);
  if (void_mask) hipLaunchKernelGGL(tanimoto_sums_kernel<true>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, p, y, (long long)HW, C, (int)ppb, sums, void_mask);
  else hipLaunchKernelGGL(tanimoto_sums_kernel<false>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, p, y, (long long)HW, C, (int)ppb, sums, void_mask);
  RUA_LAUNCH_CHECK("rua_tanimoto_sums");
  return RUA_OK;
}
extern "C" int rua_tanimoto_sums(const float* p, const float* y, int B, int64_t HW, int C, double* sums, void* stream) {
  return rua_tanimoto_sums_void(p, y, nullptr, B, HW, C, sums, stream);
}

// One block.  Follows Tanimoto_dual_loss: loss1 = T(label:=pred, pred:=label) so the class weights of
// the first term come from the PREDICTION volumes (and carry gradient); loss2 = T(1-label, 1-pred).
// single != 0: Tanimoto_loss(label, pred) itself (multitasking_utils.py:38-68) for sums taken with p := label, y := pred -
// the first term's ratio (N1 + 1e-5) / (D1 + 1e-5) with the class weights from the volumes of the FIRST argument.
__device__ __forceinline__ void tanimoto_finalize_body(const double* sums, int B, int C, float grad_scale, double* loss_out, float* coef, float* per_sample,
                                                       int single, int replicas) {
  __shared__ double w1[8], w2[8], v1[8], kap[8];
  __shared__ double E1[256], F1[256], E2[256], F2[256];
  __shared__ int inf1[8];
  const int t = threadIdx.x;
  const double smooth = 1e-5;
  if (replicas > 1) {
    // sums[replicas + 1][B][C][6]: the producers added into `replicas` copies (rua_head_fwd_loss_rep: fewer same-address atomics in a row); their sum,
    // in replica order, goes into the extra slot behind them by plain stores (idempotent: calling this twice gives the same result) and is what the
    // rest of the kernel reads
    const int ne = B * C * 6;
    double* folded = const_cast<double*>(sums) + (size_t)replicas * ne;
    for (int i = t; i < ne; i += blockDim.x) {
      double a = 0;
      for (int r = 0; r < replicas; ++r) a += sums[(size_t)r * ne + i];
      folded[i] = a;
    }
    __threadfence_block();
    __syncthreads();
    sums = folded;
  }
  if (t < C) {
    double a = 0, b = 0;
    for (int n = 0; n < B; ++n) { a += sums[((size_t)n * C + t) * 6 + 0]; b += sums[((size_t)n * C + t) * 6 + 1]; }
    a /= B; b /= B;
    // the reference squares and takes the reciprocal in float32 (multitasking_utils.py:46-53): the reciprocal overflows to inf for every
    // V^2 <= 2^-128 (V below ~5e-20), not only at V == 0 - a class whose softmax mass has died gets the largest finite weight, not 1e40 times it.
    // Infinity is decided by that float32 reciprocal of the float32 square; where it is finite the weight keeps its float64 value.
    v1[t] = a;
    const float a2 = (float)a * (float)a, b2 = (float)b * (float)b;
    w1[t] = isfinite(1.f / a2) ? 1.0 / (a * a) : INFINITY;
    w2[t] = isfinite(1.f / b2) ? 1.0 / (b * b) : INFINITY;
  }
  __syncthreads();
  if (t == 0) {
    double m1 = 0, m2 = 0;
    for (int c = 0; c < C; ++c) { if (!isinf(w1[c]) && w1[c] > m1) m1 = w1[c]; if (!isinf(w2[c]) && w2[c] > m2) m2 = w2[c]; }
    for (int c = 0; c < C; ++c) {
      inf1[c] = isinf(w1[c]);
      if (isinf(w1[c])) w1[c] = m1;
      if (isinf(w2[c])) w2[c] = m2;
    }
  }
  __syncthreads();
  double lsum = 0;
  for (int n = t; n < B; n += blockDim.x) {
    double N1 = 0, D1 = 0, N2 = 0, D2 = 0;
    for (int c = 0; c < C; ++c) {
      const double* s = &sums[((size_t)n * C + c) * 6];
      N1 += w1[c] * s[2]; D1 += w1[c] * (s[3] - s[2]);
      N2 += w2[c] * s[4]; D2 += w2[c] * (s[5] - s[4]);
    }
    E1[n] = D1 + smooth; F1[n] = N1 + smooth; E2[n] = D2 + smooth; F2[n] = N2 + smooth;
    const double ln = single ? F1[n] / E1[n] : 1.0 - 0.5 * (F1[n] / E1[n] + F2[n] / E2[n]);
    if (per_sample) per_sample[n] = (float)ln;
    lsum += ln;
  }
  // block sum of lsum (B <= 256, blockDim 64: one wave)
  for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
  if (t == 0) loss_out[0] = lsum / B;
  __syncthreads();
  if (t < C) {
    // d loss1[n] / d w1_c = [Spl (D1+e) - (N1+e)(SS - Spl)] / (D1+e)^2 ; d w1_c / d p = -2 / (V^3 B)
    double R = 0;
    for (int n = 0; n < B; ++n) {
      const double* s = &sums[((size_t)n * C + t) * 6];
      R += (s[2] * E1[n] - F1[n] * (s[3] - s[2])) / (E1[n] * E1[n]);
    }
    kap[t] = inf1[t] ? 0.0 : (-2.0 / (v1[t] * v1[t] * v1[t] * B)) * R;
  }
  __syncthreads();
  const double sc = -0.5 * (double)grad_scale;      // d(1 - .5(l1+l2)); grad_scale = loss_weight / B
  if (coef)
  for (int i = t; i < B * C; i += blockDim.x) {
    const int n = i / C, c = i - n * C;
    const double a1 = w1[c] / (E1[n] * E1[n]), a2 = w2[c] / (E2[n] * E2[n]);
    const double c0 = kap[c] + a2 * (F2[n] - E2[n]);
    const double c1 = -2.0 * a1 * F1[n] - 2.0 * a2 * F2[n];
    const double c2 = a1 * (E1[n] + F1[n]) + a2 * (E2[n] + F2[n]);
    coef[i * 3 + 0] = (float)(sc * c0); coef[i * 3 + 1] = (float)(sc * c1); coef[i * 3 + 2] = (float)(sc * c2);
  }
}
__global__ void tanimoto_finalize_kernel(const double* sums, int B, int C, float grad_scale, double* loss_out, float* coef, float* per_sample,
                                         int single, int replicas) {
  tanimoto_finalize_body(sums, B, C, grad_scale, loss_out, coef, per_sample, single, replicas);
}
// the heads of a multitask model in ONE launch (a block per head): four one-block launches of ~5 us each were ~20 us of a 7 ms step
struct TaniMulti { rua_tani_head h[RUA_MAX_HEADS]; };
__global__ void tanimoto_finalize_multi_kernel(const TaniMulti a) {
  const rua_tani_head& h = a.h[blockIdx.x];
  tanimoto_finalize_body(h.sums, h.B, h.C, h.grad_scale, h.loss_out, h.coef, h.per_sample, 0, h.replicas);
}
extern "C" int rua_tanimoto_finalize_multi(const rua_tani_head* heads, int n, void* stream) {
  RUA_CHECK_ARG(heads && n >= 1 && n <= RUA_MAX_HEADS, "rua_tanimoto_finalize_multi: 1..%d heads", RUA_MAX_HEADS);
  TaniMulti a;
  for (int i = 0; i < n; ++i) {
    const rua_tani_head& h = heads[i];
    RUA_CHECK_ARG(h.sums && h.loss_out && h.B > 0 && h.B <= 256 && h.C >= 1 && h.C <= 8 && h.replicas >= 1 && h.replicas <= 64,
                  "rua_tanimoto_finalize_multi: head %d: B must be in 1..256, C in 1..8, replicas in 1..64", i);
    a.h[i] = h;
  }
  hipLaunchKernelGGL(tanimoto_finalize_multi_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, a);
  RUA_LAUNCH_CHECK("rua_tanimoto_finalize_multi");
  return RUA_OK;
}

extern "C" int rua_tanimoto_finalize_rep(double* sums, int replicas, int B, int64_t HW, int C, float grad_scale, double* loss_out, float* coef,
                                         float* per_sample, void* stream) {
  RUA_CHECK_ARG(sums && loss_out && B > 0 && B <= 256, "rua_tanimoto_finalize: B must be in 1..256");
  RUA_CHECK_ARG(C >= 1 && C <= 8, "rua_tanimoto_finalize: C=%d must be in 1..8", C);
  RUA_CHECK_ARG(replicas >= 1 && replicas <= 64, "rua_tanimoto_finalize_rep: replicas=%d must be in 1..64", replicas);
  (void)HW;
  hipLaunchKernelGGL(tanimoto_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)sums, B, C, grad_scale, loss_out, coef, per_sample, 0, replicas);
  RUA_LAUNCH_CHECK("rua_tanimoto_finalize");
  return RUA_OK;
}
extern "C" int rua_tanimoto_finalize(const double* sums, int B, int64_t HW, int C, float grad_scale, double* loss_out, float* coef,
                                     float* per_sample, void* stream) {
  return rua_tanimoto_finalize_rep(const_cast<double*>(sums), 1, B, HW, C, grad_scale, loss_out, coef, per_sample, stream);      // one replica: sums is only read
}

extern "C" int rua_tanimoto_ratio(const double* sums, int B, int C, double* mean_out, float* per_sample, void* stream) {
  RUA_CHECK_ARG(sums && mean_out && per_sample && B > 0 && B <= 256, "rua_tanimoto_ratio: B must be in 1..256");
  RUA_CHECK_ARG(C >= 1 && C <= 8, "rua_tanimoto_ratio: C=%d must be in 1..8", C);
  hipLaunchKernelGGL(tanimoto_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, B, C, 0.f, mean_out, (float*)nullptr, per_sample, 1, 1);
  RUA_LAUNCH_CHECK("rua_tanimoto_ratio");
  return RUA_OK;
}

// ---- per-pixel losses (utils.py:481-490; Keras CategoricalCrossentropy / BinaryCrossentropy /
// MeanSquaredError as train_ISPRS.py:411-428 selects them) -----------------------------------
#define KERAS_EPS 1e-7f
// ---- the options of the rua_*_opts entries (include/rua_hip.h; losses.py holds the definitions) ----
// (q^gamma, d/dq q^gamma).  gamma == 0: factor 1 and derivative 0 by a branch, never pow(0, 0) or 0 * inf; gamma == 2: the squared form; otherwise
// gamma >= 1 (checked on the host), so q^(gamma - 1) is finite at q == 0
__device__ __forceinline__ void focal_factor(float q, float gamma, float& f, float& df) {
  if (gamma == 0.f) { f = 1.f; df = 0.f; }
  else if (gamma == 2.f) { f = q * q; df = 2.f * q; }
  else { const float r = powf(q, gamma - 1.f); f = r * q; df = gamma * r; }
}
__device__ __forceinline__ bool smooth_is_binary(int kind) { return kind == RUA_LOSS_BCE_LOGITS || kind == RUA_LOSS_FOCAL_BCE; }
// binary focal, one sigmoid channel: l = w (1 - p_t)^gamma bce with o = clip(p), bce = -(t log o + (1 - t) log(1 - o)), p_t = t p + (1 - t)(1 - p) on the
// unclipped p, w = t alpha + (1 - t)(1 - alpha) under class balancing.  (1 - p_t is held at >= 0: rounding may carry p_t an ulp past 1)
// 1 - o is taken as clip(1 - p), the same number: 1.f - (1.f - 1e-7f) is 1.19e-7, which would move log(1 - o) at the upper bound by 0.17
__device__ __forceinline__ float focal_bce_terms(float pc, float t, const rua_loss_opts& lo, float& f, float& df, float& w, float& o, float& om) {
  o = fminf(fmaxf(pc, KERAS_EPS), 1.f - KERAS_EPS);
  om = fminf(fmaxf(1.f - pc, KERAS_EPS), 1.f - KERAS_EPS);
  const float bce = -(t * logf(o) + (1.f - t) * logf(om));
  const float q = fmaxf(1.f - (t * pc + (1.f - t) * (1.f - pc)), 0.f);
  focal_factor(q, lo.gamma, f, df);
  w = lo.class_balance ? t * lo.alpha + (1.f - t) * (1.f - lo.alpha) : 1.f;
  return bce;
}
__device__ __forceinline__ float focal_bce_loss(float pc, float t, const rua_loss_opts& lo) {
  float f, df, w, o, om;
  const float bce = focal_bce_terms(pc, t, lo, f, df, w, o, om);
  return w * f * bce;
}
// dl/dp: d(1 - p_t)/dp = 1 - 2t; the clip passes bce's gradient strictly inside only
__device__ __forceinline__ float focal_bce_dp(float pc, float t, const rua_loss_opts& lo) {
  float f, df, w, o, om;
  const float bce = focal_bce_terms(pc, t, lo, f, df, w, o, om);
  const bool inside = pc >= KERAS_EPS && pc <= 1.f - KERAS_EPS;
  const float dbce = inside ? (1.f - t) / om - t / o : 0.f;
  return w * (df * (1.f - 2.f * t) * bce + f * dbce);
}
// VM: a void pixel adds nothing and its per_pixel entry is 0; the caller still divides by M, the count of ALL pixels (Keras' sample_weight rule with
// 0 / 1 weights: grad_scale = weight / M stays a host constant)
template <bool VM>
__global__ __launch_bounds__(256) void pixel_loss_kernel(int kind, const float* __restrict__ p, const float* __restrict__ z,
                                                         const float* __restrict__ y, const float* __restrict__ cw,
                                                         long long M, int C, double* out, float* per_pixel, const uint8_t* __restrict__ vm) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
    float l = 0.f;
    if constexpr (VM) {
      if (vm[m]) { if (per_pixel) per_pixel[m] = 0.f; continue; }
    }
    if (kind == RUA_LOSS_WCE) {
      float S = 0.f;
      for (int c = 0; c < C; ++c) S += p[m * C + c];
      for (int c = 0; c < C; ++c) {
        const float u = fminf(fmaxf(p[m * C + c] / S, KERAS_EPS), 1.f - KERAS_EPS);
        l -= y[m * C + c] * logf(u) * cw[c];
      }
    } else if (kind == RUA_LOSS_CE_LOGITS) {
      float mx = -INFINITY;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[m * C + c]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += expf(z[m * C + c] - mx);
      const float lse = mx + logf(s);
      for (int c = 0; c < C; ++c) l -= y[m * C + c] * (z[m * C + c] - lse);
    } else if (kind == RUA_LOSS_BCE_LOGITS) {
      for (int c = 0; c < C; ++c) {
        const float zz = z[m * C + c];
        l += fmaxf(zz, 0.f) - zz * y[m * C + c] + log1pf(expf(-fabsf(zz)));
      }
      l /= C;
    } else {
      for (int c = 0; c < C; ++c) { const float d = y[m * C + c] - p[m * C + c]; l = fmaf(d, d, l); }
      l /= C;
    }
    if (per_pixel) per_pixel[m] = l;
    acc += l;
  }
  block_atomic_add(out, acc, sh, 0);
}

extern "C" int rua_pixel_loss_void(int kind, const float* p, const float* z, const float* y, const float* class_w, const uint8_t* void_mask,
                                   int64_t M, int C, double* loss_out, float* per_pixel, void* stream) {
  RUA_CHECK_ARG(p && y && loss_out && M > 0 && C >= 1 && C <= 64, "rua_pixel_loss: bad arguments");
  RUA_CHECK_ARG(kind >= RUA_LOSS_WCE && kind <= RUA_LOSS_MSE, "rua_pixel_loss: kind %d is not a per-pixel loss", kind);
  RUA_CHECK_ARG(kind != RUA_LOSS_WCE || class_w, "rua_pixel_loss: weighted CE needs class weights");
  RUA_CHECK_ARG((kind != RUA_LOSS_CE_LOGITS && kind != RUA_LOSS_BCE_LOGITS) || z, "rua_pixel_loss: logits needed");
  int64_t g = (M + 255) / 256; if (g > 1024) g = 1024;
  if (void_mask) hipLaunchKernelGGL(pixel_loss_kernel<true>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, kind, p, z, y, class_w, (long long)M, C, loss_out, per_pixel, void_mask);
  else hipLaunchKernelGGL(pixel_loss_kernel<false>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, kind, p, z, y, class_w, (long long)M, C, loss_out, per_pixel, void_mask);
  RUA_LAUNCH_CHECK("rua_pixel_loss");
  return RUA_OK;
}
extern "C" int rua_pixel_loss(int kind, const float* p, const float* z, const float* y, const float* class_w,
                              int64_t M, int C, double* loss_out, float* per_pixel, void* stream) {
  return rua_pixel_loss_void(kind, p, z, y, class_w, nullptr, M, C, loss_out, per_pixel, stream);
}

// pixel_loss_kernel with the options: t = the smoothed label in the three cross-entropies' formulas, and the two focal kinds.  Same traversal,
// same accumulation (fp32 per thread, block_atomic_add); C <= 8.
template <bool VM>
__global__ __launch_bounds__(256) void pixel_loss_opts_kernel(int kind, const float* __restrict__ p, const float* __restrict__ z,
                                                              const float* __restrict__ y, const float* __restrict__ cw, const rua_loss_opts lo,
                                                              long long M, int C, double* out, float* per_pixel, const uint8_t* __restrict__ vm) {
  __shared__ float sh[4];
  float acc = 0.f;
  const bool smooth = lo.label_smoothing != 0.f;
  const float sa = 1.f - lo.label_smoothing, sb = lo.label_smoothing / (smooth_is_binary(kind) ? 2.f : (float)C);
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
    float l = 0.f;
    if constexpr (VM) {
      if (vm[m]) { if (per_pixel) per_pixel[m] = 0.f; continue; }
    }
    float t[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) t[c] = c < C ? y[m * C + c] : 0.f;
    if (smooth) {
#pragma unroll
      for (int c = 0; c < 8; ++c) t[c] = c < C ? fmaf(t[c], sa, sb) : 0.f;
    }
    if (kind == RUA_LOSS_WCE || kind == RUA_LOSS_FOCAL_CE) {
      float S = 0.f;
      for (int c = 0; c < C; ++c) S += p[m * C + c];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (c < C) {
          const float u = fminf(fmaxf(p[m * C + c] / S, KERAS_EPS), 1.f - KERAS_EPS);
          if (kind == RUA_LOSS_WCE) l -= t[c] * logf(u) * cw[c];
          else {
            float f, df;
            focal_factor(1.f - u, lo.gamma, f, df);
            l -= t[c] * logf(u) * cw[c] * f;
          }
        }
      }
    } else if (kind == RUA_LOSS_CE_LOGITS) {
      float mx = -INFINITY;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[m * C + c]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += expf(z[m * C + c] - mx);
      const float lse = mx + logf(s);
#pragma unroll
      for (int c = 0; c < 8; ++c) if (c < C) l -= t[c] * (z[m * C + c] - lse);
    } else if (kind == RUA_LOSS_BCE_LOGITS) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (c < C) {
          const float zz = z[m * C + c];
          l += fmaxf(zz, 0.f) - zz * t[c] + log1pf(expf(-fabsf(zz)));
        }
      }
      l /= C;
    } else {      // RUA_LOSS_FOCAL_BCE (MSE takes no option: the entry sends it to pixel_loss_kernel)
#pragma unroll
      for (int c = 0; c < 8; ++c) if (c < C) l += focal_bce_loss(p[m * C + c], t[c], lo);
      l /= C;
    }
    if (per_pixel) per_pixel[m] = l;
    acc += l;
  }
  block_atomic_add(out, acc, sh, 0);
}

// The range of the options (include/rua_hip.h), checked before any launch; why: the violated rule
static const char* loss_opts_error(int kind, const rua_loss_opts& o) {
  if (!(o.label_smoothing >= 0.f && o.label_smoothing < 1.f)) return "label_smoothing must be in [0, 1)";
  if (o.label_smoothing != 0.f && (kind == RUA_LOSS_TANIMOTO || kind == RUA_LOSS_MSE)) return "Tanimoto and MSE take no label smoothing";
  if (kind == RUA_LOSS_FOCAL_CE || kind == RUA_LOSS_FOCAL_BCE) {
    if (!(o.gamma == 0.f || (o.gamma >= 1.f && o.gamma <= 8.f))) return "gamma must be 0 or in [1, 8]";
  }
  if (kind == RUA_LOSS_FOCAL_BCE) {
    if (o.class_balance != 0 && o.class_balance != 1) return "class_balance must be 0 or 1";
    if (o.class_balance && !(o.alpha >= 0.f && o.alpha <= 1.f)) return "alpha must be in [0, 1]";
  }
  return nullptr;
}
static bool loss_needs_opts(int kind, const rua_loss_opts& o) { return kind > RUA_LOSS_MSE || o.label_smoothing != 0.f; }

extern "C" int rua_pixel_loss_opts(int kind, const float* p, const float* z, const float* y, const float* class_w, const uint8_t* void_mask,
                                   const rua_loss_opts* opts, int64_t M, int C, double* loss_out, float* per_pixel, void* stream) {
  RUA_CHECK_ARG(opts, "rua_pixel_loss_opts: null options");
  RUA_CHECK_ARG(kind >= RUA_LOSS_WCE && kind <= RUA_LOSS_FOCAL_BCE, "rua_pixel_loss_opts: kind %d is not a per-pixel loss", kind);
  const char* why = loss_opts_error(kind, *opts);
  RUA_CHECK_ARG(!why, "rua_pixel_loss_opts: kind %d: %s", kind, why);
  if (!loss_needs_opts(kind, *opts))                      // kinds 1..4 with nothing set: the kernel, and so the bytes, of rua_pixel_loss_void
    return rua_pixel_loss_void(kind, p, z, y, class_w, void_mask, M, C, loss_out, per_pixel, stream);
  RUA_CHECK_ARG(p && y && loss_out && M > 0, "rua_pixel_loss_opts: bad arguments");
  RUA_CHECK_ARG(C >= 1 && C <= 8, "rua_pixel_loss_opts: C=%d must be in 1..8", C);
  RUA_CHECK_ARG((kind != RUA_LOSS_WCE && kind != RUA_LOSS_FOCAL_CE) || class_w, "rua_pixel_loss_opts: weighted and focal CE need the per-class vector");
  RUA_CHECK_ARG((kind != RUA_LOSS_CE_LOGITS && kind != RUA_LOSS_BCE_LOGITS) || z, "rua_pixel_loss_opts: logits needed");
  int64_t g = (M + 255) / 256; if (g > 1024) g = 1024;
  if (void_mask) hipLaunchKernelGGL(pixel_loss_opts_kernel<true>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, kind, p, z, y, class_w, *opts, (long long)M, C, loss_out, per_pixel, void_mask);
  else hipLaunchKernelGGL(pixel_loss_opts_kernel<false>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, kind, p, z, y, class_w, *opts, (long long)M, C, loss_out, per_pixel, void_mask);
  RUA_LAUNCH_CHECK("rua_pixel_loss_opts");
  return RUA_OK;
}

// d(total loss)/d(logits), one thread per pixel
// CT: the class count as a template constant (6, 3; 0: runtime, <= 8) - with a runtime C every `c < C` became a branch around one scalar access
// VM: dz is +0.0f at a void pixel (written, not skipped: rua_head_bwd_sums reads every element); p and y are not read there
// OP: the rua_*_opts entries - label smoothing on the cross-entropies and the two focal kinds (focal_factor above); the instantiations without it
// are the code they were
template <int CT, bool VM, bool OP = false>
__device__ __forceinline__ void head_dz_body(int kind, int act, const float* __restrict__ p, const float* __restrict__ y,
                                             const float* __restrict__ coef, const float* __restrict__ cw, float gs,
                                             long long HW, int C_rt, float* dz, const uint8_t* __restrict__ vm,
                                             const rua_loss_opts lo = rua_loss_opts{0.f, 0.f, 0.f, 0}) {
  const int C = CT > 0 ? CT : C_rt;
  auto load_row = [&](const float* src, long long m, float* v) {
    if constexpr (CT == 6) {                              // 24-byte rows: three 8-byte accesses
      const float2* q = reinterpret_cast<const float2*>(src + m * 6);
      const float2 a = q[0], b = q[1], c = q[2];
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y; v[6] = 0.f; v[7] = 0.f;
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = c < C ? src[m * C + c] : 0.f;
    }
  };
  auto store_row = [&](long long m, const float* v) {
    if constexpr (CT == 6) {
      float2* q = reinterpret_cast<float2*>(dz + m * 6);
      q[0] = make_float2(v[0], v[1]); q[1] = make_float2(v[2], v[3]); q[2] = make_float2(v[4], v[5]);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) if (c < C) dz[m * C + c] = v[c];
    }
  };
  // blockIdx.y = sample (the Tanimoto coefficients are per sample and class: m / HW per pixel was a 64-bit division - ~100 vector instructions
  // in a pass that moves 72 bytes per pixel)
  const int n = blockIdx.y;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) {
    const long long m = (long long)n * HW + i;
    float pv[8], yv[8], g[8], o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { g[c] = 0.f; o[c] = 0.f; }
    if constexpr (VM) {
      if (vm[m]) { store_row(m, o); continue; }
    }
    load_row(p, m, pv); load_row(y, m, yv);
    if constexpr (OP) {
      if (lo.label_smoothing != 0.f) {                    // t = y (1 - e) + e / K; K = C under a softmax, 2 per sigmoid channel (a branch: e == 0 leaves y's bytes)
        const float sa = 1.f - lo.label_smoothing, sb = lo.label_smoothing / (smooth_is_binary(kind) ? 2.f : (float)C);
#pragma unroll
        for (int c = 0; c < 8; ++c) yv[c] = c < C ? fmaf(yv[c], sa, sb) : 0.f;
      }
    }
    if (kind == RUA_LOSS_CE_LOGITS) {
      float sy = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) sy += yv[c];
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = (pv[c] * sy - yv[c]) * gs;
      store_row(m, o);
      continue;
    }
    if (kind == RUA_LOSS_BCE_LOGITS) {
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = (pv[c] - yv[c]) * gs / C;
      store_row(m, o);
      continue;
    }
    if (OP && kind == RUA_LOSS_FOCAL_CE) {
      // L = - sum_c a_c t_c (1 - u_c)^gamma log u_c: dL/du_c = -a_c t_c [(1 - u)^gamma / u - gamma (1 - u)^(gamma - 1) log u] inside the clip, 0 outside;
      // gamma == 0 is weighted CE's line below, byte for byte
      float S = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) S += pv[c];
      float h[8], hu = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        h[c] = 0.f;
        if (c < C) {
          const float u = pv[c] / S;
          const bool inside = u >= KERAS_EPS && u <= 1.f - KERAS_EPS;
          float f, df;
          focal_factor(1.f - u, lo.gamma, f, df);
          h[c] = inside ? -yv[c] * cw[c] * (f - df * u * logf(u)) / u : 0.f;
          hu = fmaf(h[c], u, hu);
        }
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) g[c] = (h[c] - hu) / S * gs;
    } else if (OP && kind == RUA_LOSS_FOCAL_BCE) {
#pragma unroll
      for (int c = 0; c < 8; ++c) if (c < C) g[c] = focal_bce_dp(pv[c], yv[c], lo) * gs / C;
    } else if (kind == RUA_LOSS_TANIMOTO) {
#pragma unroll
      for (int c = 0; c < 8; ++c) if (c < C) { const float* k = coef + ((size_t)n * C + c) * 3; g[c] = fmaf(k[1], pv[c], fmaf(k[2], yv[c], k[0])); }
    } else if (kind == RUA_LOSS_WCE) {
      float S = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) S += pv[c];
      float h[8], hu = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        h[c] = 0.f;
        if (c < C) {
          const float u = pv[c] / S;
          const bool inside = u >= KERAS_EPS && u <= 1.f - KERAS_EPS;     // clip_by_value passes gradient inside only
          h[c] = inside ? -yv[c] * cw[c] / u : 0.f;
          hu = fmaf(h[c], u, hu);
        }
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) g[c] = (h[c] - hu) / S * gs;
    } else {   // MSE
#pragma unroll
      for (int c = 0; c < 8; ++c) g[c] = 2.f * (pv[c] - yv[c]) * gs / C;
    }
    if (act == RUA_ACT_SOFTMAX) {
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) dot = fmaf(g[c], pv[c], dot);
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = pv[c] * (g[c] - dot);
      store_row(m, o);
    } else if (act == RUA_ACT_SIGMOID) {
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = g[c] * pv[c] * (1.f - pv[c]);
      store_row(m, o);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = g[c];
      store_row(m, o);
    }
  }
}

template <bool VM>
__global__ __launch_bounds__(256) void head_dz_kernel(int kind, int act, const float* __restrict__ p, const float* __restrict__ y,
                                                      const float* __restrict__ coef, const float* __restrict__ cw, float gs,
                                                      long long HW, long long M, int C, float* dz, const uint8_t* __restrict__ vm) {
  (void)M;
  if (C == 6) head_dz_body<6, VM>(kind, act, p, y, coef, cw, gs, HW, C, dz, vm);
  else if (C == 3) head_dz_body<3, VM>(kind, act, p, y, coef, cw, gs, HW, C, dz, vm);
  else head_dz_body<0, VM>(kind, act, p, y, coef, cw, gs, HW, C, dz, vm);
}
// d(loss)/d(logits) of several heads in ONE launch: blockIdx.z = head (the four heads of the multitask model: four launches of 4 - 12 us)
struct DzMulti { rua_dz_head h[RUA_MAX_HEADS]; };
template <bool VM>
__global__ __launch_bounds__(256) void head_dz_multi_kernel(const DzMulti a, const uint8_t* __restrict__ vm) {
  const rua_dz_head& h = a.h[blockIdx.z];
  if ((int)blockIdx.y >= h.B) return;
  if (h.C == 6) head_dz_body<6, VM>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, h.grad_scale, (long long)h.HW, h.C, h.dz, vm);
  else if (h.C == 3) head_dz_body<3, VM>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, h.grad_scale, (long long)h.HW, h.C, h.dz, vm);
  else head_dz_body<0, VM>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, h.grad_scale, (long long)h.HW, h.C, h.dz, vm);
}
extern "C" int rua_head_dz_multi_void(const rua_dz_head* heads, int n, const uint8_t* void_mask, void* stream) {
  RUA_CHECK_ARG(heads && n >= 1 && n <= RUA_MAX_HEADS, "rua_head_dz_multi: 1..%d heads", RUA_MAX_HEADS);
  DzMulti a;
  int64_t g = 1; int Bm = 1;
  for (int i = 0; i < n; ++i) {
    const rua_dz_head& h = heads[i];
    RUA_CHECK_ARG(h.p && h.y && h.dz && h.B > 0 && h.B <= 65535 && h.HW > 0 && h.C >= 1 && h.C <= 8 && h.kind >= 0 && h.kind <= 4 && h.act >= 0 && h.act <= 2,
                  "rua_head_dz_multi: head %d: bad arguments", i);
    RUA_CHECK_ARG(h.kind != RUA_LOSS_TANIMOTO || h.coef, "rua_head_dz_multi: Tanimoto needs coefficients");
    RUA_CHECK_ARG(h.kind != RUA_LOSS_WCE || h.class_w, "rua_head_dz_multi: weighted CE needs class weights");
    // one mask [B * HW] serves every head: it is indexed by (sample, pixel), so the heads must agree in both
    RUA_CHECK_ARG(!void_mask || (h.B == heads[0].B && h.HW == heads[0].HW), "rua_head_dz_multi_void: head %d: B %d, HW %lld differ from head 0's", i, h.B, (long long)h.HW);
    a.h[i] = h;
    const int64_t gi = (h.HW + 255) / 256; if (gi > g) g = gi;
    if (h.B > Bm) Bm = h.B;
  }
  const int64_t cap = 4096 / ((int64_t)Bm * n) > 0 ? 4096 / ((int64_t)Bm * n) : 1;
  if (g > cap) g = cap;
  if (void_mask) hipLaunchKernelGGL(head_dz_multi_kernel<true>, dim3((int)g, Bm, n), dim3(256), 0, (hipStream_t)stream, a, void_mask);
  else hipLaunchKernelGGL(head_dz_multi_kernel<false>, dim3((int)g, Bm, n), dim3(256), 0, (hipStream_t)stream, a, void_mask);
  RUA_LAUNCH_CHECK("rua_head_dz_multi");
  return RUA_OK;
}
extern "C" int rua_head_dz_multi(const rua_dz_head* heads, int n, void* stream) {
  return rua_head_dz_multi_void(heads, n, nullptr, stream);
}

extern "C" int rua_head_dz_void(int kind, int act, const float* p, const float* y, const float* coef, const float* class_w,
                                float grad_scale, int B, int64_t HW, int C, const uint8_t* void_mask, float* dz, void* stream) {
  RUA_CHECK_ARG(p && y && dz && B > 0 && HW > 0, "rua_head_dz: bad arguments");
  RUA_CHECK_ARG(C >= 1 && C <= 8, "rua_head_dz: C=%d must be in 1..8", C);
  RUA_CHECK_ARG(kind >= 0 && kind <= 4 && act >= 0 && act <= 2, "rua_head_dz: bad kind/act");
  RUA_CHECK_ARG(kind != RUA_LOSS_TANIMOTO || coef, "rua_head_dz: Tanimoto needs coefficients");
  RUA_CHECK_ARG(kind != RUA_LOSS_WCE || class_w, "rua_head_dz: weighted CE needs class weights");
  const int64_t M = (int64_t)B * HW;
  int64_t g = (HW + 255) / 256;
  const int64_t cap = 4096 / B > 0 ? 4096 / B : 1;       // ~4096 blocks over the batch; blockIdx.y = sample
  if (g > cap) g = cap;
  RUA_CHECK_ARG(B <= 65535, "rua_head_dz: B=%d too large", B);
  if (void_mask) hipLaunchKernelGGL(head_dz_kernel<true>, dim3((int)g, B), dim3(256), 0, (hipStream_t)stream, kind, act, p, y, coef, class_w, grad_scale,
                                    (long long)HW, (long long)M, C, dz, void_mask);
  else hipLaunchKernelGGL(head_dz_kernel<false>, dim3((int)g, B), dim3(256), 0, (hipStream_t)stream, kind, act, p, y, coef, class_w, grad_scale,
                          (long long)HW, (long long)M, C, dz, void_mask);
  RUA_LAUNCH_CHECK("rua_head_dz");
  return RUA_OK;
}
extern "C" int rua_head_dz(int kind, int act, const float* p, const float* y, const float* coef, const float* class_w,
                           float grad_scale, int B, int64_t HW, int C, float* dz, void* stream) {
  return rua_head_dz_void(kind, act, p, y, coef, class_w, grad_scale, B, HW, C, nullptr, dz, stream);
}

// ---- the same two launches with rua_loss_opts: all seven kinds.  Same grids; a call in which no head has an option set or a new kind goes to the
// kernels above
template <bool VM>
__global__ __launch_bounds__(256) void head_dz_opts_kernel(int kind, int act, const float* __restrict__ p, const float* __restrict__ y,
                                                           const float* __restrict__ coef, const float* __restrict__ cw, float gs,
                                                           long long HW, int C, float* dz, const uint8_t* __restrict__ vm, const rua_loss_opts lo) {
  if (C == 6) head_dz_body<6, VM, true>(kind, act, p, y, coef, cw, gs, HW, C, dz, vm, lo);
  else if (C == 3) head_dz_body<3, VM, true>(kind, act, p, y, coef, cw, gs, HW, C, dz, vm, lo);
  else head_dz_body<0, VM, true>(kind, act, p, y, coef, cw, gs, HW, C, dz, vm, lo);
}
struct DzMultiOpts { rua_dz_head h[RUA_MAX_HEADS]; rua_loss_opts o[RUA_MAX_HEADS]; };
template <bool VM>
__global__ __launch_bounds__(256) void head_dz_multi_opts_kernel(const DzMultiOpts a, const uint8_t* __restrict__ vm) {
  const rua_dz_head& h = a.h[blockIdx.z];
  const rua_loss_opts lo = a.o[blockIdx.z];
  if ((int)blockIdx.y >= h.B) return;
  if (h.C == 6) head_dz_body<6, VM, true>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, h.grad_scale, (long long)h.HW, h.C, h.dz, vm, lo);
  else if (h.C == 3) head_dz_body<3, VM, true>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, h.grad_scale, (long long)h.HW, h.C, h.dz, vm, lo);
  else head_dz_body<0, VM, true>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, h.grad_scale, (long long)h.HW, h.C, h.dz, vm, lo);
}
// what a head of the opts entries must satisfy beyond rua_head_dz's own rules; NULL: fine
static const char* dz_opts_error(int kind, int act, const float* class_w, const rua_loss_opts& o) {
  if (kind == RUA_LOSS_FOCAL_CE && act != RUA_ACT_SOFTMAX) return "focal CE needs a softmax head";
  if (kind == RUA_LOSS_FOCAL_BCE && act != RUA_ACT_SIGMOID) return "binary focal needs a sigmoid head";
  if (kind == RUA_LOSS_FOCAL_CE && !class_w) return "focal CE needs the per-class alpha vector (class_w)";
  return loss_opts_error(kind, o);
}

extern "C" int rua_head_dz_multi_opts(const rua_dz_head* heads, const rua_loss_opts* opts, int n, const uint8_t* void_mask, void* stream) {
  RUA_CHECK_ARG(heads && opts && n >= 1 && n <= RUA_MAX_HEADS, "rua_head_dz_multi_opts: 1..%d heads, each with its options", RUA_MAX_HEADS);
  DzMultiOpts a;
  int64_t g = 1; int Bm = 1;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const rua_dz_head& h = heads[i];
    RUA_CHECK_ARG(h.p && h.y && h.dz && h.B > 0 && h.B <= 65535 && h.HW > 0 && h.C >= 1 && h.C <= 8 && h.kind >= 0 && h.kind <= RUA_LOSS_FOCAL_BCE && h.act >= 0 && h.act <= 2,
                  "rua_head_dz_multi_opts: head %d: bad arguments", i);
    RUA_CHECK_ARG(h.kind != RUA_LOSS_TANIMOTO || h.coef, "rua_head_dz_multi_opts: Tanimoto needs coefficients");
    RUA_CHECK_ARG(h.kind != RUA_LOSS_WCE || h.class_w, "rua_head_dz_multi_opts: weighted CE needs class weights");
    const char* why = dz_opts_error(h.kind, h.act, h.class_w, opts[i]);
    RUA_CHECK_ARG(!why, "rua_head_dz_multi_opts: head %d: %s", i, why);
    RUA_CHECK_ARG(!void_mask || (h.B == heads[0].B && h.HW == heads[0].HW), "rua_head_dz_multi_opts: head %d: B %d, HW %lld differ from head 0's", i, h.B, (long long)h.HW);
    a.h[i] = h; a.o[i] = opts[i];
    any = any || loss_needs_opts(h.kind, opts[i]);
    const int64_t gi = (h.HW + 255) / 256; if (gi > g) g = gi;
    if (h.B > Bm) Bm = h.B;
  }
  if (!any) return rua_head_dz_multi_void(heads, n, void_mask, stream);
  const int64_t cap = 4096 / ((int64_t)Bm * n) > 0 ? 4096 / ((int64_t)Bm * n) : 1;
  if (g > cap) g = cap;
  if (void_mask) hipLaunchKernelGGL(head_dz_multi_opts_kernel<true>, dim3((int)g, Bm, n), dim3(256), 0, (hipStream_t)stream, a, void_mask);
  else hipLaunchKernelGGL(head_dz_multi_opts_kernel<false>, dim3((int)g, Bm, n), dim3(256), 0, (hipStream_t)stream, a, void_mask);
  RUA_LAUNCH_CHECK("rua_head_dz_multi_opts");
  return RUA_OK;
}

extern "C" int rua_head_dz_opts(int kind, int act, const float* p, const float* y, const float* coef, const float* class_w, float grad_scale,
                                int B, int64_t HW, int C, const uint8_t* void_mask, const rua_loss_opts* opts, float* dz, void* stream) {
  RUA_CHECK_ARG(opts, "rua_head_dz_opts: null options");
  RUA_CHECK_ARG(p && y && dz && B > 0 && HW > 0, "rua_head_dz_opts: bad arguments");
  RUA_CHECK_ARG(C >= 1 && C <= 8, "rua_head_dz_opts: C=%d must be in 1..8", C);
  RUA_CHECK_ARG(kind >= 0 && kind <= RUA_LOSS_FOCAL_BCE && act >= 0 && act <= 2, "rua_head_dz_opts: bad kind/act");
  RUA_CHECK_ARG(kind != RUA_LOSS_TANIMOTO || coef, "rua_head_dz_opts: Tanimoto needs coefficients");
  RUA_CHECK_ARG(kind != RUA_LOSS_WCE || class_w, "rua_head_dz_opts: weighted CE needs class weights");
  const char* why = dz_opts_error(kind, act, class_w, *opts);
  RUA_CHECK_ARG(!why, "rua_head_dz_opts: kind %d: %s", kind, why);
  RUA_CHECK_ARG(B <= 65535, "rua_head_dz_opts: B=%d too large", B);
  if (!loss_needs_opts(kind, *opts)) return rua_head_dz_void(kind, act, p, y, coef, class_w, grad_scale, B, HW, C, void_mask, dz, stream);
  int64_t g = (HW + 255) / 256;
  const int64_t cap = 4096 / B > 0 ? 4096 / B : 1;
  if (g > cap) g = cap;
  if (void_mask) hipLaunchKernelGGL(head_dz_opts_kernel<true>, dim3((int)g, B), dim3(256), 0, (hipStream_t)stream, kind, act, p, y, coef, class_w, grad_scale,
                                    (long long)HW, C, dz, void_mask, *opts);
  else hipLaunchKernelGGL(head_dz_opts_kernel<false>, dim3((int)g, B), dim3(256), 0, (hipStream_t)stream, kind, act, p, y, coef, class_w, grad_scale,
                          (long long)HW, C, dz, void_mask, *opts);
  RUA_LAUNCH_CHECK("rua_head_dz_opts");
  return RUA_OK;
}

// ---- online hard example mining: the same launch with a head's mask and normaliser read from device memory (rua_dz_sel; csrc/ohem.hip writes them).
// A head with a selection runs the instantiation rua_head_dz_opts would run for it - its own drop_mask as the mask, scale_dev[0] as grad_scale,
// the options form only if the head needs it -, a head without one the instantiation rua_head_dz_multi_opts would: the same bytes either way.
struct DzMultiSel { rua_dz_head h[RUA_MAX_HEADS]; rua_loss_opts o[RUA_MAX_HEADS]; rua_dz_sel s[RUA_MAX_HEADS]; unsigned char op[RUA_MAX_HEADS]; };
template <bool VM, bool OP>
__device__ __forceinline__ void head_dz_sel_body(const rua_dz_head& h, const rua_loss_opts lo, float gs, const uint8_t* __restrict__ vm) {
  if (h.C == 6) head_dz_body<6, VM, OP>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, gs, (long long)h.HW, h.C, h.dz, vm, lo);
  else if (h.C == 3) head_dz_body<3, VM, OP>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, gs, (long long)h.HW, h.C, h.dz, vm, lo);
  else head_dz_body<0, VM, OP>(h.kind, h.act, h.p, h.y, h.coef, h.class_w, gs, (long long)h.HW, h.C, h.dz, vm, lo);
}
__global__ __launch_bounds__(256) void head_dz_multi_sel_kernel(const DzMultiSel a, const uint8_t* __restrict__ vm) {
  const rua_dz_head& h = a.h[blockIdx.z];
  if ((int)blockIdx.y >= h.B) return;
  const rua_loss_opts lo = a.o[blockIdx.z];
  const rua_dz_sel s = a.s[blockIdx.z];
  const uint8_t* m = s.drop_mask ? s.drop_mask : vm;
  const float gs = s.drop_mask ? s.scale_dev[0] : h.grad_scale;
  if (a.op[blockIdx.z]) {
    if (m) head_dz_sel_body<true, true>(h, lo, gs, m); else head_dz_sel_body<false, true>(h, lo, gs, m);
  } else {
    if (m) head_dz_sel_body<true, false>(h, lo, gs, m); else head_dz_sel_body<false, false>(h, lo, gs, m);
  }
}
extern "C" int rua_head_dz_multi_sel(const rua_dz_head* heads, const rua_loss_opts* opts, const rua_dz_sel* sel, int n, const uint8_t* void_mask, void* stream) {
  RUA_CHECK_ARG(heads && opts && sel && n >= 1 && n <= RUA_MAX_HEADS, "rua_head_dz_multi_sel: 1..%d heads, each with its options and its selection", RUA_MAX_HEADS);
  DzMultiSel a;
  int64_t g = 1; int Bm = 1, first_plain = -1;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const rua_dz_head& h = heads[i];
    RUA_CHECK_ARG(h.p && h.y && h.dz && h.B > 0 && h.B <= 65535 && h.HW > 0 && h.C >= 1 && h.C <= 8 && h.kind >= 0 && h.kind <= RUA_LOSS_FOCAL_BCE && h.act >= 0 && h.act <= 2,
                  "rua_head_dz_multi_sel: head %d: bad arguments", i);
    RUA_CHECK_ARG(h.kind != RUA_LOSS_TANIMOTO || h.coef, "rua_head_dz_multi_sel: Tanimoto needs coefficients");
    RUA_CHECK_ARG(h.kind != RUA_LOSS_WCE || h.class_w, "rua_head_dz_multi_sel: weighted CE needs class weights");
    const char* why = dz_opts_error(h.kind, h.act, h.class_w, opts[i]);
    RUA_CHECK_ARG(!why, "rua_head_dz_multi_sel: head %d: %s", i, why);
    RUA_CHECK_ARG((sel[i].drop_mask != nullptr) == (sel[i].scale_dev != nullptr), "rua_head_dz_multi_sel: head %d: drop_mask and scale_dev go together", i);
    RUA_CHECK_ARG(!sel[i].scale_dev || ((size_t)sel[i].scale_dev & 3) == 0, "rua_head_dz_multi_sel: head %d: misaligned scale_dev", i);
    if (!sel[i].drop_mask) {                              // the shared mask is indexed by (sample, pixel): the heads that read it must agree in both
      if (first_plain < 0) first_plain = i;
      RUA_CHECK_ARG(!void_mask || (h.B == heads[first_plain].B && h.HW == heads[first_plain].HW),
                    "rua_head_dz_multi_sel: head %d: B %d, HW %lld differ from head %d's", i, h.B, (long long)h.HW, first_plain);
    }
    a.h[i] = h; a.o[i] = opts[i]; a.s[i] = sel[i];
    any = any || loss_needs_opts(h.kind, opts[i]);
    const int64_t gi = (h.HW + 255) / 256; if (gi > g) g = gi;
    if (h.B > Bm) Bm = h.B;
  }
  for (int i = 0; i < n; ++i) a.op[i] = sel[i].drop_mask ? loss_needs_opts(heads[i].kind, opts[i]) : any;
  const int64_t cap = 4096 / ((int64_t)Bm * n) > 0 ? 4096 / ((int64_t)Bm * n) : 1;
  if (g > cap) g = cap;
  hipLaunchKernelGGL(head_dz_multi_sel_kernel, dim3((int)g, Bm, n), dim3(256), 0, (hipStream_t)stream, a, void_mask);
  RUA_LAUNCH_CHECK("rua_head_dz_multi_sel");
  return RUA_OK;
}
extern "C" int rua_head_dz_sel(int kind, int act, const float* p, const float* y, const float* coef, const float* class_w, int B, int64_t HW, int C,
                               const rua_loss_opts* opts, const uint8_t* drop_mask, const float* scale_dev, float* dz, void* stream) {
  RUA_CHECK_ARG(opts && drop_mask && scale_dev, "rua_head_dz_sel: options, drop_mask and scale_dev are required");
  rua_dz_head h;
  memset(&h, 0, sizeof(h));
  h.kind = kind; h.act = act; h.p = p; h.y = y; h.coef = coef; h.class_w = class_w; h.grad_scale = 0.f; h.B = B; h.HW = HW; h.C = C; h.dz = dz;
  const rua_dz_sel s = {drop_mask, scale_dev};
  return rua_head_dz_multi_sel(&h, opts, &s, 1, nullptr, stream);
}

// accuracy + TP/FP/TN/FN (Keras 'accuracy' = categorical accuracy; confusion counts at .5)
// VM: void pixels are counted nowhere, so (TP + FP + TN + FN) / C is the number of valid pixels
template <bool VM>
__global__ __launch_bounds__(256) void seg_metrics_kernel(const float* __restrict__ p, const float* __restrict__ y, long long M, int C, double* out,
                                                          const uint8_t* __restrict__ vm) {
  __shared__ float sh[5 * 4];
  float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
    if constexpr (VM) { if (vm[m]) continue; }
    int ip = 0, iy = 0; float bp = p[m * C], by = y[m * C];
    for (int c = 0; c < C; ++c) {
      const float pv = p[m * C + c], yv = y[m * C + c];
      if (pv > bp) { bp = pv; ip = c; }
      if (yv > by) { by = yv; iy = c; }
      const bool t = yv > 0.5f, q = pv > 0.5f;
      a[1] += (t && q); a[2] += (!t && q); a[3] += (!t && !q); a[4] += (t && !q);
    }
    a[0] += (ip == iy);
  }
  for (int k = 0; k < 5; ++k) block_atomic_add(&out[k], a[k], sh, k);
}

// 16-byte loads: G pixels (G * C floats = NV float4) per thread per iteration, element classes are compile-time constants
template <int C, int G, bool VM>
__global__ __launch_bounds__(256) void seg_metrics_vec(const float* __restrict__ p, const float* __restrict__ y, long long M, double* out,
                                                       const uint8_t* __restrict__ vm) {
  constexpr int NV = G * C / 4;
  __shared__ float sh[5 * 4];
  float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const float4* pp = reinterpret_cast<const float4*>(p);
  const float4* yy = reinterpret_cast<const float4*>(y);
  const long long ngroups = M / G;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += (long long)gridDim.x * 256) {
    float pv[NV * 4], yv[NV * 4];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float4 a4 = pp[gi * NV + v], l4 = yy[gi * NV + v];
      pv[v * 4] = a4.x; pv[v * 4 + 1] = a4.y; pv[v * 4 + 2] = a4.z; pv[v * 4 + 3] = a4.w;
      yv[v * 4] = l4.x; yv[v * 4 + 1] = l4.y; yv[v * 4 + 2] = l4.z; yv[v * 4 + 3] = l4.w;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if constexpr (VM) { if (vm[gi * G + g]) continue; }
      int ip = 0, iy = 0; float bp = pv[g * C], by = yv[g * C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float q_ = pv[g * C + c], t_ = yv[g * C + c];
        if (q_ > bp) { bp = q_; ip = c; }
        if (t_ > by) { by = t_; iy = c; }
        const bool t = t_ > 0.5f, q = q_ > 0.5f;
        a[1] += (t && q); a[2] += (!t && q); a[3] += (!t && !q); a[4] += (t && !q);
      }
      a[0] += (ip == iy);
    }
  }
  for (int k = 0; k < 5; ++k) block_atomic_add(&out[k], a[k], sh, k);
}

extern "C" int rua_seg_metrics_void(const float* p, const float* y, const uint8_t* void_mask, int64_t M, int C, double* out, void* stream) {
  RUA_CHECK_ARG(p && y && out && M > 0 && C >= 1, "rua_seg_metrics: bad arguments");
  if ((C == 6 || C == 2) && M % 2 == 0 && ((size_t)p & 15) == 0 && ((size_t)y & 15) == 0) {
    int64_t g = (M / 2 + 255) / 256; if (g > 256) g = 256;
    if (C == 6 && void_mask) hipLaunchKernelGGL((seg_metrics_vec<6, 2, true>), dim3((int)g), dim3(256), 0, (hipStream_t)stream, p, y, (long long)M, out, void_mask);
    else if (C == 6) hipLaunchKernelGGL((seg_metrics_vec<6, 2, false>), dim3((int)g), dim3(256), 0, (hipStream_t)stream, p, y, (long long)M, out, void_mask);
    else if (void_mask) hipLaunchKernelGGL((seg_metrics_vec<2, 2, true>), dim3((int)g), dim3(256), 0, (hipStream_t)stream, p, y, (long long)M, out, void_mask);
    else hipLaunchKernelGGL((seg_metrics_vec<2, 2, false>), dim3((int)g), dim3(256), 0, (hipStream_t)stream, p, y, (long long)M, out, void_mask);
    RUA_LAUNCH_CHECK("rua_seg_metrics");
    return RUA_OK;
  }
  // the five counters share one cache line and every block ends in five same-line fp64 atomics (serialised): measured
  // 64 blocks 36 us, 128: 23, 256: 24, 512: 37
  const int cap = g_tune.metrics_blocks > 0 ? g_tune.metrics_blocks : rua_cu_count() / 2;      // 128 on MI355X
  int64_t g = (M + 255) / 256; if (g > cap) g = cap;
  if (void_mask) hipLaunchKernelGGL(seg_metrics_kernel<true>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, p, y, (long long)M, C, out, void_mask);
  else hipLaunchKernelGGL(seg_metrics_kernel<false>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, p, y, (long long)M, C, out, void_mask);
  RUA_LAUNCH_CHECK("rua_seg_metrics");
  return RUA_OK;
}
extern "C" int rua_seg_metrics(const float* p, const float* y, int64_t M, int C, double* out, void* stream) {
  return rua_seg_metrics_void(p, y, nullptr, M, C, out, stream);
}

// ---- optimizers on the flat parameter buffer ---------------------------------------------------
// Four parameters per thread (16-byte accesses; every slice of the flat buffers is 64-byte aligned and n a multiple of 4 - the tail, if any, element
// by element); WC: the updated weights also leave as bf16 (wcopy: the forward-layout copy the convolutions read - its index space is the master's -, so
// rua_weight_prep has only the data-gradient layout left to build, from this copy: rua_weight_prep_dgrad).  Same arithmetic per element as before.
template <bool WC>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ th, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   long long n, float lr_t, const float* __restrict__ lr_dev, float b1, float b2, float eps, float gs, int zero,
                                                   bf16_t* __restrict__ wcopy) {
  if (lr_dev) lr_t = lr_dev[0];
  const long long n4 = n >> 2;
  auto upd = [&](float gg_, float& mm, float& vv, float& tt) {
    const float gg = gg_ * gs;
    mm = b1 * mm + (1.f - b1) * gg;
    vv = b2 * vv + (1.f - b2) * gg * gg;
    tt -= lr_t * mm / (sqrtf(vv) + eps);
  };
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 g4 = reinterpret_cast<const float4*>(g)[i];
    float4 m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i], t4 = reinterpret_cast<float4*>(th)[i];
    upd(g4.x, m4.x, v4.x, t4.x); upd(g4.y, m4.y, v4.y, t4.y); upd(g4.z, m4.z, v4.z, t4.z); upd(g4.w, m4.w, v4.w, t4.w);
    reinterpret_cast<float4*>(m)[i] = m4; reinterpret_cast<float4*>(v)[i] = v4; reinterpret_cast<float4*>(th)[i] = t4;
    if (zero) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (WC) reinterpret_cast<uint2*>(wcopy)[i] = make_uint2(ET<bf16_t>::pk(t4.x, t4.y), ET<bf16_t>::pk(t4.z, t4.w));
  }
  for (long long i = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float mm = m[i], vv = v[i], tt = th[i];
    upd(g[i], mm, vv, tt);
    m[i] = mm; v[i] = vv; th[i] = tt;
    if (zero) g[i] = 0.f;
    if constexpr (WC) wcopy[i] = (bf16_t)tt;
  }
}
template <bool WC>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ th, float* __restrict__ g, float* __restrict__ vel,
                                                  long long n, float lr, const float* __restrict__ lr_dev, float mu, float gs, int zero, bf16_t* __restrict__ wcopy) {
  if (lr_dev) lr = lr_dev[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float vv = mu * vel[i] - lr * g[i] * gs;
    vel[i] = vv;
    const float tt = th[i] + vv;
    th[i] = tt;
    if (zero) g[i] = 0.f;
    if constexpr (WC) wcopy[i] = (bf16_t)tt;
  }
}
// Step-dependent learning rate on the device, so that a captured training step needs no host-side scalar update between
// replays: state[0] = optimizer steps taken (advanced here), state[1] = base learning rate; lr_out[0] = the rate the
// optimizer kernel launched next reads (Adam: Keras' lr * sqrt(1 - beta2^t) / (1 - beta1^t), train_ISPRS.py:404-407).
// hold (NULL: never) != 0 - a hold step of gradient accumulation -: nothing is read or written (the gated entry points further down).
__global__ void lr_step_kernel(double* state, float* lr_out, int adam, double beta1, double beta2, const int32_t* hold) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && !(hold != nullptr && hold[0] != 0)) {
    const double t = state[0] + 1.0;
    state[0] = t;
    double lr = state[1];
    if (adam) lr = lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t));
    lr_out[0] = (float)lr;
  }
}
extern "C" int rua_lr_step(double* state, float* lr_out, int adam, double beta1, double beta2, void* stream) {
  RUA_CHECK_ARG(state && lr_out, "rua_lr_step: null pointer");
  hipLaunchKernelGGL(lr_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, lr_out, adam, beta1, beta2, (const int32_t*)nullptr);
  RUA_LAUNCH_CHECK("rua_lr_step");
  return RUA_OK;
}
extern "C" int rua_lr_step_gated(double* state, float* lr_out, int adam, double beta1, double beta2, const int32_t* hold, void* stream) {
  RUA_CHECK_ARG(state && lr_out && hold && ((size_t)hold & 3) == 0, "rua_lr_step_gated: null or misaligned pointer");
  hipLaunchKernelGGL(lr_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, lr_out, adam, beta1, beta2, hold);
  RUA_LAUNCH_CHECK("rua_lr_step_gated");
  return RUA_OK;
}
extern "C" int rua_adam_step_w(float* theta, float* g, float* m, float* v, int64_t n, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                               float eps, float grad_scale, int zero_grad, void* wcopy_bf16, void* stream) {
  RUA_CHECK_ARG(theta && g && m && v && n > 0, "rua_adam_step: bad arguments");
  RUA_CHECK_ARG((((size_t)theta | (size_t)g | (size_t)m | (size_t)v) & 15) == 0 && ((size_t)wcopy_bf16 & 7) == 0, "rua_adam_step: buffers must be 16-byte aligned");
  int64_t gr = (n / 4 + 255) / 256; if (gr > 4096) gr = 4096; if (gr < 1) gr = 1;
  if (wcopy_bf16) hipLaunchKernelGGL((adam_kernel<true>), dim3((int)gr), dim3(256), 0, (hipStream_t)stream, theta, g, m, v, (long long)n, lr_t, lr_t_dev, beta1, beta2, eps, grad_scale, zero_grad, (bf16_t*)wcopy_bf16);
  else hipLaunchKernelGGL((adam_kernel<false>), dim3((int)gr), dim3(256), 0, (hipStream_t)stream, theta, g, m, v, (long long)n, lr_t, lr_t_dev, beta1, beta2, eps, grad_scale, zero_grad, (bf16_t*)nullptr);
  RUA_LAUNCH_CHECK("rua_adam_step");
  return RUA_OK;
}
extern "C" int rua_adam_step(float* theta, float* g, float* m, float* v, int64_t n, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                             float eps, float grad_scale, int zero_grad, void* stream) {
  return rua_adam_step_w(theta, g, m, v, n, lr_t, lr_t_dev, beta1, beta2, eps, grad_scale, zero_grad, nullptr, stream);
}
extern "C" int rua_sgd_step_w(float* theta, float* g, float* vel, int64_t n, float lr, const float* lr_dev, float momentum, float grad_scale,
                              int zero_grad, void* wcopy_bf16, void* stream) {
  RUA_CHECK_ARG(theta && g && vel && n > 0, "rua_sgd_step: bad arguments");
  int64_t gr = (n + 255) / 256; if (gr > 4096) gr = 4096;
  if (wcopy_bf16) hipLaunchKernelGGL((sgd_kernel<true>), dim3((int)gr), dim3(256), 0, (hipStream_t)stream, theta, g, vel, (long long)n, lr, lr_dev, momentum, grad_scale, zero_grad, (bf16_t*)wcopy_bf16);
  else hipLaunchKernelGGL((sgd_kernel<false>), dim3((int)gr), dim3(256), 0, (hipStream_t)stream, theta, g, vel, (long long)n, lr, lr_dev, momentum, grad_scale, zero_grad, (bf16_t*)nullptr);
  RUA_LAUNCH_CHECK("rua_sgd_step");
  return RUA_OK;
}
extern "C" int rua_sgd_step(float* theta, float* g, float* vel, int64_t n, float lr, const float* lr_dev, float momentum, float grad_scale,
                            int zero_grad, void* stream) {
  return rua_sgd_step_w(theta, g, vel, n, lr, lr_dev, momentum, grad_scale, zero_grad, nullptr, stream);
}

// ---- clipping, decoupled decay and the non-finite step skip: the optimizers over a chunk table (include/rua_hip.h) ------------------------
// One 256-thread block per chunk of at most RUA_OPT_CHUNK elements.  Fixed reduction order, no atomics: a lane adds the squares of its
// 16-byte groups in index order (x, y, z, w), the ragged tail (len % 4 elements) goes to lanes 0 .. 2 of wave 0 after their groups, the
// lanes of a wave are folded by the xor butterfly 32, 16, .. 1, thread 0 adds the four waves in order.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const rua_opt_chunk* __restrict__ chunks, double* __restrict__ partials,
                                                         const int32_t* __restrict__ hold) {
  __shared__ double sh[4];
  if (hold != nullptr && hold[0] != 0) return;          // a hold step of gradient accumulation (uniform): the gated finisher will not look at the partials
  const rua_opt_chunk ck = chunks[blockIdx.x];
  const float* gp = g + ck.off;
  const int n4 = ck.len >> 2;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 q = reinterpret_cast<const float4*>(gp)[i];
    acc += (double)q.x * (double)q.x; acc += (double)q.y * (double)q.y; acc += (double)q.z * (double)q.z; acc += (double)q.w * (double)q.w;
  }
  const int t = (n4 << 2) + threadIdx.x;
  if (t < ck.len) { const double x = (double)gp[t]; acc += x * x; }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
extern "C" int rua_grad_sumsq(const float* g, const rua_opt_chunk* chunks, int n_chunks, double* partials, void* stream) {
  RUA_CHECK_ARG(g && chunks && partials && n_chunks > 0, "rua_grad_sumsq: bad arguments");
  RUA_CHECK_ARG(((size_t)g & 15) == 0 && ((size_t)chunks & 15) == 0 && ((size_t)partials & 7) == 0, "rua_grad_sumsq: g and the chunk table must be 16-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, g, chunks, partials, (const int32_t*)nullptr);
  RUA_LAUNCH_CHECK("rua_grad_sumsq");
  return RUA_OK;
}
extern "C" int rua_grad_sumsq_gated(const float* g, const rua_opt_chunk* chunks, int n_chunks, double* partials, const int32_t* hold, void* stream) {
  RUA_CHECK_ARG(g && chunks && partials && hold && n_chunks > 0, "rua_grad_sumsq_gated: bad arguments");
  RUA_CHECK_ARG(((size_t)g & 15) == 0 && ((size_t)chunks & 15) == 0 && ((size_t)partials & 7) == 0 && ((size_t)hold & 3) == 0,
                "rua_grad_sumsq_gated: g and the chunk table must be 16-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, g, chunks, partials, hold);
  RUA_LAUNCH_CHECK("rua_grad_sumsq_gated");
  return RUA_OK;
}

// One block.  The partials pass through LDS in tiles of FIN_TILE (coalesced loads by all threads: a thread that walked its variable's partials in
// global memory paid one exposed load latency per chunk, 105 us for the flagship table's 5519 chunks); thread v % 256 adds variable v's partials of
// the tile in chunk order onto its running sum (var_sumsq[v], which only it touches), so the order of every addition is what a serial loop's is.
// The variables' sums pass through LDS the same way and thread 0 adds them in order.  The smallest coefficient is a min: any order gives the same.
#define FIN_TILE 4096
// s + x[0] + x[1] + ... in index order; the LDS reads go out eight at a time so that their latency is paid once per eight additions
__device__ __forceinline__ double add_in_order(double s, const double* x, int n) {
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    double t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = x[k + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += t[j];
  }
  for (; k < n; ++k) s += x[k];
  return s;
}
__global__ __launch_bounds__(256) void clip_finish_kernel(const double* __restrict__ partials, int n_chunks, const rua_opt_var* __restrict__ vars, int n_vars,
                                                          int mode, double c, double gs, int skip_nonfinite, double* __restrict__ var_sumsq,
                                                          float* __restrict__ coef, int32_t* __restrict__ flag, double* __restrict__ report,
                                                          const int32_t* __restrict__ hold) {
  __shared__ double tile[FIN_TILE];
  if (hold != nullptr) {
    // gradient accumulation (rua_clip_finish_gated): flag[0] stays "this update was skipped" - what the BatchNorm restore reads -, flag[1] is
    // "hold or skipped" - what the optimizer and the moving average read.  A hold step writes the two flags and nothing else.
    if (hold[0] != 0) {                                  // uniform: the whole block leaves before the first barrier
      if (threadIdx.x == 0) { flag[0] = 0; flag[1] = 1; }
      return;
    }
  }
  __shared__ double s_total;
  __shared__ float s_coef, s_min[4];
  __shared__ int s_skip;
  const int tid = threadIdx.x;
  for (int t0 = 0; t0 < n_chunks; t0 += FIN_TILE) {
    const int tn = n_chunks - t0 < FIN_TILE ? n_chunks - t0 : FIN_TILE;
    for (int i = tid; i < tn; i += 256) tile[i] = partials[t0 + i];
    __syncthreads();
    for (int v = tid; v < n_vars; v += 256) {
      const rua_opt_var vr = vars[v];
      const int a = vr.chunk_begin > t0 ? vr.chunk_begin : t0, b = vr.chunk_end < t0 + tn ? vr.chunk_end : t0 + tn;
      if (t0 == 0 || a < b) {
        double s = vr.chunk_begin >= t0 ? 0.0 : var_sumsq[v];              // the variable's first tile starts its sum
        var_sumsq[v] = add_in_order(s, tile + (a - t0), b > a ? b - a : 0);
      }
    }
    __syncthreads();
  }
  double total = 0.0;                                                       // thread 0's
  for (int t0 = 0; t0 < n_vars; t0 += FIN_TILE) {
    const int tn = n_vars - t0 < FIN_TILE ? n_vars - t0 : FIN_TILE;
    for (int i = tid; i < tn; i += 256) tile[i] = var_sumsq[t0 + i];
    __syncthreads();
    if (tid == 0) total = add_in_order(total, tile, tn);
    __syncthreads();
  }
  if (tid == 0) {
    const double norm = gs * sqrt(total);
    s_total = norm;
    s_coef = mode == RUA_CLIP_GLOBAL_NORM ? (float)(c / fmax(norm, c)) : 1.f;
    s_skip = (skip_nonfinite && !isfinite(total)) ? 1 : 0;
  }
  __syncthreads();
  float mn = s_coef;
  for (int v = tid; v < n_vars; v += 256) {
    float cf = s_coef;
    if (mode == RUA_CLIP_NORM) cf = (float)(c / fmax(gs * sqrt(var_sumsq[v]), c));
    coef[v] = cf;
    mn = cf < mn ? cf : mn;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const float w = __shfl_xor(mn, o, 64); mn = w < mn ? w : mn; }
  if ((tid & 63) == 0) s_min[tid >> 6] = mn;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) mn = s_min[w] < mn ? s_min[w] : mn;
    const int skip = s_skip;
    flag[0] = skip;
    if (hold != nullptr) flag[1] = skip;
    report[0] = s_total;
    report[1] = (double)mn;
    report[2] += (double)skip;
    report[3] += (mn < 1.f && !skip) ? 1.0 : 0.0;
  }
}
extern "C" int rua_clip_finish(const double* partials, int n_chunks, const rua_opt_var* vars, int n_vars, int mode, double c, double grad_scale,
                               int skip_nonfinite, double* var_sumsq, float* coef, int32_t* flag, double* report, void* stream) {
  RUA_CHECK_ARG(partials && vars && var_sumsq && coef && flag && report && n_vars > 0 && n_chunks > 0, "rua_clip_finish: bad arguments");
  RUA_CHECK_ARG(mode >= RUA_CLIP_NONE && mode <= RUA_CLIP_VALUE, "rua_clip_finish: unknown mode %d", mode);
  RUA_CHECK_ARG((mode != RUA_CLIP_GLOBAL_NORM && mode != RUA_CLIP_NORM) || c > 0.0, "rua_clip_finish: the clip norm must be positive");
  RUA_CHECK_ARG((((size_t)partials | (size_t)var_sumsq | (size_t)report) & 7) == 0 && ((size_t)vars & 15) == 0 && (((size_t)coef | (size_t)flag) & 3) == 0,
                "rua_clip_finish: misaligned buffers");
  hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_chunks, vars, n_vars, mode, c, grad_scale, skip_nonfinite, var_sumsq,
                     coef, flag, report, (const int32_t*)nullptr);
  RUA_LAUNCH_CHECK("rua_clip_finish");
  return RUA_OK;
}
extern "C" int rua_clip_finish_gated(const double* partials, int n_chunks, const rua_opt_var* vars, int n_vars, int mode, double c, double grad_scale,
                                     int skip_nonfinite, double* var_sumsq, float* coef, int32_t* flag2, double* report, const int32_t* hold, void* stream) {
  RUA_CHECK_ARG(partials && vars && var_sumsq && coef && flag2 && report && hold && n_vars > 0 && n_chunks > 0, "rua_clip_finish_gated: bad arguments");
  RUA_CHECK_ARG(mode >= RUA_CLIP_NONE && mode <= RUA_CLIP_VALUE, "rua_clip_finish_gated: unknown mode %d", mode);
  RUA_CHECK_ARG((mode != RUA_CLIP_GLOBAL_NORM && mode != RUA_CLIP_NORM) || c > 0.0, "rua_clip_finish_gated: the clip norm must be positive");
  RUA_CHECK_ARG((((size_t)partials | (size_t)var_sumsq | (size_t)report) & 7) == 0 && ((size_t)vars & 15) == 0 &&
                (((size_t)coef | (size_t)flag2 | (size_t)hold) & 3) == 0 && flag2 != hold, "rua_clip_finish_gated: misaligned buffers");
  hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_chunks, vars, n_vars, mode, c, grad_scale, skip_nonfinite, var_sumsq,
                     coef, flag2, report, hold);
  RUA_LAUNCH_CHECK("rua_clip_finish_gated");
  return RUA_OK;
}

// The segmented optimizers.  ADAM: m2 is Adam's v; SGD: m is the velocity and m2 is not touched.  The element arithmetic of the flat kernels with the
// decay in front and the coefficient / clamp on the gradient; a skipped step stores only the zeroed gradient and the bf16 copy of the unchanged theta.
struct seg_args {
  float lr, b1, b2, eps, mu, gs, cv, d;
};
template <bool ADAM>
__device__ __forceinline__ void seg_update(const seg_args& a, bool dec, float cf, float g_, float& mm, float& vv, float& tt) {
  if (dec) tt = tt - tt * a.d;
  float gg = (g_ * a.gs) * cf;
  if (a.cv > 0.f) gg = gg < -a.cv ? -a.cv : (gg > a.cv ? a.cv : gg);
  if constexpr (ADAM) {
    mm = a.b1 * mm + (1.f - a.b1) * gg;
    vv = a.b2 * vv + (1.f - a.b2) * gg * gg;
    tt -= a.lr * mm / (sqrtf(vv) + a.eps);
  } else {
    mm = a.mu * mm - a.lr * gg;
    tt = tt + mm;
  }
}
template <bool ADAM, bool WC>
__global__ __launch_bounds__(256) void opt_seg_kernel(float* __restrict__ th, float* __restrict__ g, float* __restrict__ m, float* __restrict__ m2,
                                                      const rua_opt_chunk* __restrict__ chunks, const rua_opt_var* __restrict__ vars, const float* __restrict__ coef,
                                                      const int32_t* __restrict__ flag, const float* __restrict__ lr_dev, const double* __restrict__ lr_state,
                                                      seg_args a, double wd, int zero, bf16_t* __restrict__ wcopy) {
  const rua_opt_chunk ck = chunks[blockIdx.x];
  const bool skip = flag != nullptr && flag[0] != 0;
  const bool dec = wd != 0.0 && vars[ck.var].decay != 0;
  const float cf = coef[ck.var];
  a.lr = lr_dev[0];
  a.d = dec ? (float)(wd * lr_state[1]) : 0.f;
  th += ck.off; g += ck.off; m += ck.off;
  if constexpr (ADAM) m2 += ck.off;
  if constexpr (WC) wcopy += ck.off;
  const int n4 = ck.len >> 2;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 t4 = reinterpret_cast<float4*>(th)[i];
    if (!skip) {
      const float4 g4 = reinterpret_cast<const float4*>(g)[i];
      float4 m4 = reinterpret_cast<float4*>(m)[i], v4 = z4;
      if constexpr (ADAM) v4 = reinterpret_cast<float4*>(m2)[i];
      seg_update<ADAM>(a, dec, cf, g4.x, m4.x, v4.x, t4.x); seg_update<ADAM>(a, dec, cf, g4.y, m4.y, v4.y, t4.y);
      seg_update<ADAM>(a, dec, cf, g4.z, m4.z, v4.z, t4.z); seg_update<ADAM>(a, dec, cf, g4.w, m4.w, v4.w, t4.w);
      reinterpret_cast<float4*>(m)[i] = m4; reinterpret_cast<float4*>(th)[i] = t4;
      if constexpr (ADAM) reinterpret_cast<float4*>(m2)[i] = v4;
    }
    if (zero) reinterpret_cast<float4*>(g)[i] = z4;
    if constexpr (WC) reinterpret_cast<uint2*>(wcopy)[i] = make_uint2(ET<bf16_t>::pk(t4.x, t4.y), ET<bf16_t>::pk(t4.z, t4.w));
  }
  const int i = (n4 << 2) + threadIdx.x;
  if (i < ck.len) {
    float tt = th[i];
    if (!skip) {
      float mm = m[i], vv = 0.f;
      if constexpr (ADAM) vv = m2[i];
      seg_update<ADAM>(a, dec, cf, g[i], mm, vv, tt);
      m[i] = mm; th[i] = tt;
      if constexpr (ADAM) m2[i] = vv;
    }
    if (zero) g[i] = 0.f;
    if constexpr (WC) wcopy[i] = (bf16_t)tt;
  }
}
template <bool ADAM>
static int opt_seg_launch(const char* name, float* theta, float* g, float* m, float* m2, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars,
                          const float* coef, const int32_t* flag, const float* lr_dev, const double* lr_state, seg_args a, double wd, int zero,
                          void* wcopy_bf16, void* stream) {
  RUA_CHECK_ARG(theta && g && m && (m2 || !ADAM) && chunks && vars && coef && lr_dev && lr_state && n_chunks > 0, "%s: bad arguments", name);
  RUA_CHECK_ARG((((size_t)theta | (size_t)g | (size_t)m | (size_t)m2 | (size_t)chunks | (size_t)vars) & 15) == 0 && ((size_t)wcopy_bf16 & 7) == 0 &&
                (((size_t)coef | (size_t)flag | (size_t)lr_dev) & 3) == 0 && ((size_t)lr_state & 7) == 0, "%s: buffers must be 16-byte aligned", name);
  RUA_CHECK_ARG(wd >= 0.0, "%s: negative weight decay", name);
  if (wcopy_bf16) hipLaunchKernelGGL((opt_seg_kernel<ADAM, true>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, theta, g, m, m2, chunks, vars, coef, flag, lr_dev,
                                     lr_state, a, wd, zero, (bf16_t*)wcopy_bf16);
  else hipLaunchKernelGGL((opt_seg_kernel<ADAM, false>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, theta, g, m, m2, chunks, vars, coef, flag, lr_dev,
                          lr_state, a, wd, zero, (bf16_t*)nullptr);
  RUA_LAUNCH_CHECK(name);
  return RUA_OK;
}
extern "C" int rua_adam_step_seg(float* theta, float* g, float* m, float* v, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars,
                                 const float* coef, const int32_t* flag, const float* lr_dev, const double* lr_state, float beta1, float beta2, float eps,
                                 float grad_scale, float clipvalue, double weight_decay, int zero_grad, void* wcopy_bf16, void* stream) {
  seg_args a = {0.f, beta1, beta2, eps, 0.f, grad_scale, clipvalue, 0.f};
  return opt_seg_launch<true>("rua_adam_step_seg", theta, g, m, v, chunks, n_chunks, vars, coef, flag, lr_dev, lr_state, a, weight_decay, zero_grad, wcopy_bf16, stream);
}
extern "C" int rua_sgd_step_seg(float* theta, float* g, float* vel, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars,
                                const float* coef, const int32_t* flag, const float* lr_dev, const double* lr_state, float momentum,
                                float grad_scale, float clipvalue, double weight_decay, int zero_grad, void* wcopy_bf16, void* stream) {
  seg_args a = {0.f, 0.f, 0.f, 0.f, momentum, grad_scale, clipvalue, 0.f};
  return opt_seg_launch<false>("rua_sgd_step_seg", theta, g, vel, nullptr, chunks, n_chunks, vars, coef, flag, lr_dev, lr_state, a, weight_decay, zero_grad, wcopy_bf16, stream);
}

__global__ __launch_bounds__(256) void state_copy_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n, const int32_t* __restrict__ flag) {
  if (flag != nullptr && flag[0] == 0) return;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
    reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
  for (long long i = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}
extern "C" int rua_state_copy(float* dst, const float* src, int64_t n, const int32_t* flag, void* stream) {
  RUA_CHECK_ARG(dst && src && n > 0, "rua_state_copy: bad arguments");
  RUA_CHECK_ARG((((size_t)dst | (size_t)src) & 15) == 0 && ((size_t)flag & 3) == 0, "rua_state_copy: buffers must be 16-byte aligned");
  int64_t gr = (n / 4 + 255) / 256; if (gr > 1024) gr = 1024; if (gr < 1) gr = 1;
  hipLaunchKernelGGL(state_copy_kernel, dim3((int)gr), dim3(256), 0, (hipStream_t)stream, dst, src, (long long)n, flag);
  RUA_LAUNCH_CHECK("rua_state_copy");
  return RUA_OK;
}

// ---- learning-rate schedules and the weights' moving average (include/rua_hip.h; schedules.py holds the host definitions) ------------------
// schedules.host_lr in fp64, operation for operation.  Contraction is asked off; the device's pow and cos - and a multiply-add the backend
// fuses all the same - may differ from numpy's result by a few fp64 ulps.  The table look-up, the clamped tails (cos(pi) = -1 and
// 0^power = 0 are exact, and x * 0 + y is y fused or not) and the constant kind are exact.
__device__ double sched_rate(const rua_lr_schedule& k, double s) {
#pragma clang fp contract(off)
  switch (k.kind) {
    case RUA_SCHED_COSINE: {
      double base = k.initial;
      if (k.warmup) {
        if (s < k.warmup_steps) return (k.warmup_target - k.initial) * (s / k.warmup_steps) + k.initial;
        s = fmin(s, k.warmup_steps + k.decay_steps) - k.warmup_steps;
        base = k.warmup_target;
      } else {
        s = fmin(s, k.decay_steps);
      }
      const double cosine = 0.5 * (1.0 + cos(3.14159265358979323846 * (s / k.decay_steps)));
      return base * ((1.0 - k.alpha) * cosine + k.alpha);
    }
    case RUA_SCHED_EXPONENTIAL: {
      double p = s / k.decay_steps;
      if (k.staircase) p = floor(p);
      return k.initial * pow(k.decay_rate, p);
    }
    case RUA_SCHED_POLYNOMIAL: {
      double d = k.decay_steps;
      if (k.cycle) d = d * (s == 0.0 ? 1.0 : ceil(s / d));
      else s = fmin(s, d);
      return (k.initial - k.end) * pow(1.0 - s / d, k.power) + k.end;
    }
    case RUA_SCHED_PIECEWISE: {
      for (int i = 0; i < k.n_boundaries; ++i)
        if (s <= k.boundaries[i]) return k.values[i];
      return k.values[k.n_boundaries];
    }
    case RUA_SCHED_INVERSE_TIME: {
      double p = s / k.decay_steps;
      if (k.staircase) p = floor(p);
      return k.initial / (1.0 + k.decay_rate * p);
    }
    default: return k.initial;
  }
}
__global__ void lr_schedule_step_kernel(double* state, float* lr_out, const rua_lr_schedule sched, int adam, double beta1, double beta2,
                                        const int32_t* hold) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && !(hold != nullptr && hold[0] != 0)) {
    const double t = state[0] + 1.0;
    state[0] = t;
    double lr = sched_rate(sched, t - 1.0);
    state[1] = lr;                                       // the base rate the segmented optimizers' weight decay reads
    if (adam) lr = lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t));
    lr_out[0] = (float)lr;
  }
}
static int lr_schedule_launch(const char* name, double* state, float* lr_out, const rua_lr_schedule& sched, int adam, double beta1, double beta2,
                              const int32_t* hold, void* stream) {
  RUA_CHECK_ARG(state && lr_out && ((size_t)state & 7) == 0 && ((size_t)lr_out & 3) == 0, "rua_lr_schedule_step: null or misaligned pointer");
  RUA_CHECK_ARG(sched.kind >= RUA_SCHED_CONSTANT && sched.kind <= RUA_SCHED_INVERSE_TIME, "rua_lr_schedule_step: unknown kind %d", sched.kind);
  RUA_CHECK_ARG(sched.kind == RUA_SCHED_CONSTANT || sched.kind == RUA_SCHED_PIECEWISE || sched.decay_steps > 0.0, "rua_lr_schedule_step: decay_steps must be positive");
  RUA_CHECK_ARG(sched.kind != RUA_SCHED_PIECEWISE || (sched.n_boundaries >= 0 && sched.n_boundaries <= RUA_SCHED_MAX_BOUNDARIES),
                "rua_lr_schedule_step: %d boundaries (at most %d)", sched.n_boundaries, RUA_SCHED_MAX_BOUNDARIES);
  RUA_CHECK_ARG(!(sched.kind == RUA_SCHED_COSINE && sched.warmup) || sched.warmup_steps >= 0.0, "rua_lr_schedule_step: negative warmup_steps");
  hipLaunchKernelGGL(lr_schedule_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, lr_out, sched, adam, beta1, beta2, hold);
  RUA_LAUNCH_CHECK(name);
  return RUA_OK;
}
extern "C" int rua_lr_schedule_step(double* state, float* lr_out, rua_lr_schedule sched, int adam, double beta1, double beta2, void* stream) {
  return lr_schedule_launch("rua_lr_schedule_step", state, lr_out, sched, adam, beta1, beta2, nullptr, stream);
}
extern "C" int rua_lr_schedule_step_gated(double* state, float* lr_out, rua_lr_schedule sched, int adam, double beta1, double beta2, const int32_t* hold,
                                          void* stream) {
  RUA_CHECK_ARG(hold && ((size_t)hold & 3) == 0, "rua_lr_schedule_step_gated: null or misaligned hold flag");
  return lr_schedule_launch("rua_lr_schedule_step_gated", state, lr_out, sched, adam, beta1, beta2, hold, stream);
}

// Four elements per thread and stream (16-byte accesses; 8-byte for the bf16 copy), grid sized like adam_kernel's, the n % 4 tail element by
// element.  The step counter and the skip flag are read once per thread; both are uniform, so a skipped step costs an empty grid.
// __fmul_rn / __fadd_rn / __fsub_rn are plain operators in HIP's headers, and the backend fuses a product into the sum that follows it whatever
// the source says about contraction.  The two products therefore pass through an empty asm statement: no instruction, but the sum no longer
// sees where its operands came from, so each of the three operations is rounded on its own.
__device__ __forceinline__ float ema_update(bool first, float mom, float om, float e, float x) {
  float a = __fmul_rn(mom, e), b = __fmul_rn(om, x);
  asm volatile("" : "+v"(a), "+v"(b));
  return first ? x : __fadd_rn(a, b);
}
template <bool WC>
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, float* __restrict__ th, bf16_t* __restrict__ wcopy, long long n, float mom,
                                                  const double* __restrict__ lr_state, int every, const int32_t* __restrict__ flag) {
  if (flag != nullptr && flag[0] != 0) return;
  const long long t = (long long)lr_state[0];
  const bool first = t == 1;
  const bool over = every > 0 && t % every == 0;
  const float om = __fsub_rn(1.f, mom);
  auto upd = [&](float e, float x) { return ema_update(first, mom, om, e, x); };
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 t4 = reinterpret_cast<const float4*>(th)[i];
    float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!first) e4 = reinterpret_cast<const float4*>(ema)[i];
    e4.x = upd(e4.x, t4.x); e4.y = upd(e4.y, t4.y); e4.z = upd(e4.z, t4.z); e4.w = upd(e4.w, t4.w);
    reinterpret_cast<float4*>(ema)[i] = e4;
    if (over) {
      reinterpret_cast<float4*>(th)[i] = e4;
      if constexpr (WC) reinterpret_cast<uint2*>(wcopy)[i] = make_uint2(ET<bf16_t>::pk(e4.x, e4.y), ET<bf16_t>::pk(e4.z, e4.w));
    }
  }
  for (long long i = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float e = upd(first ? 0.f : ema[i], th[i]);
    ema[i] = e;
    if (over) {
      th[i] = e;
      if constexpr (WC) wcopy[i] = (bf16_t)e;
    }
  }
}
extern "C" int rua_ema_step(float* ema, float* theta, void* wcopy_bf16, int64_t n, float momentum, const double* lr_state, int overwrite_every,
                            const int32_t* flag, void* stream) {
  RUA_CHECK_ARG(ema && theta && lr_state && n > 0 && ema != theta, "rua_ema_step: bad arguments");
  RUA_CHECK_ARG((((size_t)ema | (size_t)theta) & 15) == 0 && ((size_t)wcopy_bf16 & 7) == 0 && ((size_t)lr_state & 7) == 0 && ((size_t)flag & 3) == 0,
                "rua_ema_step: buffers must be 16-byte aligned");
  RUA_CHECK_ARG(momentum >= 0.f && momentum <= 1.f && overwrite_every >= 0, "rua_ema_step: momentum in [0, 1], overwrite_every >= 0");
  int64_t gr = (n / 4 + 255) / 256; if (gr > 4096) gr = 4096; if (gr < 1) gr = 1;
  if (wcopy_bf16) hipLaunchKernelGGL((ema_kernel<true>), dim3((int)gr), dim3(256), 0, (hipStream_t)stream, ema, theta, (bf16_t*)wcopy_bf16, (long long)n, momentum, lr_state, overwrite_every, flag);
  else hipLaunchKernelGGL((ema_kernel<false>), dim3((int)gr), dim3(256), 0, (hipStream_t)stream, ema, theta, (bf16_t*)nullptr, (long long)n, momentum, lr_state, overwrite_every, flag);
  RUA_LAUNCH_CHECK("rua_ema_step");
  return RUA_OK;
}

// ---- gradient accumulation (include/rua_hip.h; accum.py holds the host definition) ----------------------------------------------------------
// The gate: one thread.  acc_state[0] = gradients of the current cycle already in the accumulator (0 .. k - 1).  Everything behind it in the step
// reads hold[0]; the decision is device state, so a captured step replays it.
__global__ void accum_gate_kernel(int32_t* acc_state, int k, int32_t* hold) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int m = acc_state[0] + 1;
    const int h = m < k ? 1 : 0;
    acc_state[0] = h ? m : 0;
    hold[0] = h;
  }
}
extern "C" int rua_accum_gate(int32_t* acc_state, int k, int32_t* hold, void* stream) {
  RUA_CHECK_ARG(acc_state && hold && (((size_t)acc_state | (size_t)hold) & 3) == 0, "rua_accum_gate: null or misaligned pointer");
  RUA_CHECK_ARG(k >= 2, "rua_accum_gate: k = %d (at least 2)", k);
  hipLaunchKernelGGL(accum_gate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc_state, k, hold);
  RUA_LAUNCH_CHECK("rua_accum_gate");
  return RUA_OK;
}
// ema_kernel's shape: four elements per thread and stream (16-byte accesses), a grid-stride loop, the n % 4 tail element by element, hold read once
// per thread (uniform).  A hold step reads g and a and writes a (12 bytes per parameter; the flagged optimizer behind it zeroes g), an update step
// reads both and writes both (16).  The quotient is an IEEE division (__fdiv_rn), not a product with 1 / k: accum.host_accumulate bit for bit.
__global__ __launch_bounds__(256) void accum_kernel(float* __restrict__ g, float* __restrict__ a, long long n, float kf, const int32_t* __restrict__ hold) {
  const bool h = hold[0] != 0;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 g4 = reinterpret_cast<const float4*>(g)[i];
    float4 a4 = reinterpret_cast<const float4*>(a)[i];
    if (h) {
      a4.x = __fadd_rn(a4.x, g4.x); a4.y = __fadd_rn(a4.y, g4.y); a4.z = __fadd_rn(a4.z, g4.z); a4.w = __fadd_rn(a4.w, g4.w);
      reinterpret_cast<float4*>(a)[i] = a4;
    } else {
      a4.x = __fdiv_rn(__fadd_rn(g4.x, a4.x), kf); a4.y = __fdiv_rn(__fadd_rn(g4.y, a4.y), kf);
      a4.z = __fdiv_rn(__fadd_rn(g4.z, a4.z), kf); a4.w = __fdiv_rn(__fadd_rn(g4.w, a4.w), kf);
      reinterpret_cast<float4*>(g)[i] = a4;
      reinterpret_cast<float4*>(a)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  for (long long i = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if (h) {
      a[i] = __fadd_rn(a[i], g[i]);
    } else {
      g[i] = __fdiv_rn(__fadd_rn(g[i], a[i]), kf);
      a[i] = 0.f;
    }
  }
}
extern "C" int rua_accum_step(float* g, float* a, int64_t n, int k, const int32_t* hold, void* stream) {
  RUA_CHECK_ARG(g && a && hold && n > 0 && g != a, "rua_accum_step: bad arguments");
  RUA_CHECK_ARG((((size_t)g | (size_t)a) & 15) == 0 && ((size_t)hold & 3) == 0, "rua_accum_step: buffers must be 16-byte aligned");
  RUA_CHECK_ARG(k >= 2 && k <= (1 << 24), "rua_accum_step: k = %d (2 .. 2^24: exact in fp32)", k);
  int64_t gr = (n / 4 + 255) / 256; if (gr > 4096) gr = 4096; if (gr < 1) gr = 1;
  hipLaunchKernelGGL(accum_kernel, dim3((int)gr), dim3(256), 0, (hipStream_t)stream, g, a, (long long)n, (float)k, hold);
  RUA_LAUNCH_CHECK("rua_accum_step");
  return RUA_OK;
}

// LAMB (You et al. 2019; keras.optimizers.Lamb) over the chunk table of the segmented optimizers (include/rua_hip.h; lamb.py holds the host
// definition).  Three launches where rua_adam_step_seg is one: the trust ratio of a variable needs the norm of ALL its Adam directions before
// the first weight moves.
//   rua_lamb_moments   one 256-thread block per chunk, grad_sumsq_kernel's shape: m', v' and the direction u (into g's slot), and the chunk's
//                      fp64 sums of th1^2 and u^2 in grad_sumsq_kernel's reduction order
//   rua_lamb_finish    one block, clip_finish_kernel's shape: per-variable sums in chunk order, ratio[v], the report
//   rua_lamb_apply     one block per chunk: theta' = th1 - (ratio * lr) * u, g zeroed, the bf16 copy
// Bytes per element: 16 read + 12 written, then 8 read + 8 (+ 2) written.
// Every fp32 operation is rounded on its own.  The backend fuses a product into the sum that follows it whatever the source says about
// contraction (see ema_update in loss_optim.hip), so every product that feeds a sum passes through an empty asm statement first.  Divisions and
// square roots are the compiler's correctly rounded expansions (__fdiv_rn is the plain operator, sqrtf the builtin - __fsqrt_rn is the NATIVE
// square root in HIP's headers and is not used), denormals included.
#include "common.h"

__device__ __forceinline__ float lamb_alone(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ double lamb_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// lamb.host_powi: b^t by binary exponentiation in a fixed order, no pow on either side.  Plain fp64 products lose about t / 4 ulp (a squaring
// doubles the error it inherits: 37 .. 209 ulp measured at t = 1000), so the running power and the result are PAIRS of doubles (value, remainder):
// a product's remainder fma(a, b, -a * b) is exact, which is what the host's Dekker product computes too - the same bits on both sides, and
// the result within one ulp of b^t.  Every product passes through an empty asm statement so that no sum absorbs it.
__device__ __forceinline__ double lamb_alone64(double x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ void lamb_dd_mul(double& xh, double& xl, double yh, double yl) {
  const double p = lamb_alone64(xh * yh);
  double e = lamb_alone64(fma(xh, yh, -p));
  const double cross = lamb_alone64(xh * yl) + lamb_alone64(xl * yh);
  e = e + cross;
  const double s = p + e;
  xl = e - (s - p);
  xh = s;
}
__device__ __forceinline__ double lamb_powi(double b, long long t) {
  double rh = 1.0, rl = 0.0, ph = b, pl = 0.0;
  while (t > 0) {
    if (t & 1) lamb_dd_mul(rh, rl, ph, pl);
    t >>= 1;
    if (t) lamb_dd_mul(ph, pl, ph, pl);
  }
  return rh;
}
struct lamb_args {
  float b1, b2, eps, gs, cv;
  float om1, om2, c1, c2, d;    // filled on the device
};
__device__ __forceinline__ float lamb_decay(bool dec, float d, float th) {
  return dec ? __fsub_rn(th, lamb_alone(__fmul_rn(th, d))) : th;
}
// m', v' in place; returns u
__device__ __forceinline__ float lamb_direction(const lamb_args& a, float cf, float g_, float& mm, float& vv) {
  float gg = __fmul_rn(__fmul_rn(g_, a.gs), cf);
  if (a.cv > 0.f) gg = gg < -a.cv ? -a.cv : (gg > a.cv ? a.cv : gg);
  mm = __fadd_rn(mm, lamb_alone(__fmul_rn(__fsub_rn(gg, mm), a.om1)));
  const float g2 = lamb_alone(__fmul_rn(gg, gg));
  vv = __fadd_rn(vv, lamb_alone(__fmul_rn(__fsub_rn(g2, vv), a.om2)));
  const float den = __fadd_rn(sqrtf(__fdiv_rn(vv, a.c2)), a.eps);
  return __fdiv_rn(__fdiv_rn(mm, a.c1), den);
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ th, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                           const rua_opt_chunk* __restrict__ chunks, const rua_opt_var* __restrict__ vars,
                                                           const float* __restrict__ coef, const int32_t* __restrict__ flag,
                                                           const double* __restrict__ lr_state, lamb_args a, double wd, double* __restrict__ pw,
                                                           double* __restrict__ pu) {
  __shared__ double sh[8];
  const rua_opt_chunk ck = chunks[blockIdx.x];
  g += ck.off;
  const int n4 = ck.len >> 2;
  const int tail = (n4 << 2) + threadIdx.x;
  if (flag != nullptr && flag[0] != 0) {                  // skipped update / hold step (uniform): the gradient is consumed, nothing else moves
    for (int i = threadIdx.x; i < n4; i += 256) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tail < ck.len) g[tail] = 0.f;
    return;
  }
  const bool dec = wd != 0.0 && vars[ck.var].decay != 0;
  const float cf = coef[ck.var];
  const long long t = (long long)lr_state[0];
  a.om1 = __fsub_rn(1.f, a.b1);
  a.om2 = __fsub_rn(1.f, a.b2);
  a.c1 = (float)(1.0 - lamb_powi((double)a.b1, t));
  a.c2 = (float)(1.0 - lamb_powi((double)a.b2, t));
  a.d = dec ? (float)(wd * lr_state[1]) : 0.f;
  th += ck.off; m += ck.off; v += ck.off;
  double aw = 0.0, au = 0.0;
  auto one = [&](float tt, float& gu, float& mm, float& vv) {
    const float t1 = lamb_decay(dec, a.d, tt);
    gu = lamb_direction(a, cf, gu, mm, vv);
    aw += (double)t1 * (double)t1;                         // squares of fp32 values are exact in fp64: fused or not, the same bits
    au += (double)gu * (double)gu;
  };
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 t4 = reinterpret_cast<const float4*>(th)[i];
    float4 g4 = reinterpret_cast<const float4*>(g)[i], m4 = reinterpret_cast<const float4*>(m)[i], v4 = reinterpret_cast<const float4*>(v)[i];
    one(t4.x, g4.x, m4.x, v4.x); one(t4.y, g4.y, m4.y, v4.y); one(t4.z, g4.z, m4.z, v4.z); one(t4.w, g4.w, m4.w, v4.w);
    reinterpret_cast<float4*>(m)[i] = m4; reinterpret_cast<float4*>(v)[i] = v4; reinterpret_cast<float4*>(g)[i] = g4;
  }
  if (tail < ck.len) {
    float gu = g[tail], mm = m[tail], vv = v[tail];
    one(th[tail], gu, mm, vv);
    m[tail] = mm; v[tail] = vv; g[tail] = gu;
  }
  aw = lamb_wave_sum(aw); au = lamb_wave_sum(au);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = aw; sh[4 + (threadIdx.x >> 6)] = au; }
  __syncthreads();
  if (threadIdx.x == 0) {
    pw[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    pu[blockIdx.x] = ((sh[4] + sh[5]) + sh[6]) + sh[7];
  }
}

static bool lamb_betas_ok(float b1, float b2, float eps) { return b1 >= 0.f && b1 < 1.f && b2 >= 0.f && b2 < 1.f && eps > 0.f && eps < INFINITY; }

extern "C" int rua_lamb_moments(const float* theta, float* g, float* m, float* v, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars,
                                const float* coef, const int32_t* flag, const double* lr_state, float beta1, float beta2, float eps, float grad_scale,
                                float clipvalue, double weight_decay, double* pw, double* pu, void* stream) {
  RUA_CHECK_ARG(theta && g && m && v && chunks && vars && coef && lr_state && pw && pu && n_chunks > 0, "rua_lamb_moments: bad arguments");
  RUA_CHECK_ARG((((size_t)theta | (size_t)g | (size_t)m | (size_t)v | (size_t)chunks | (size_t)vars) & 15) == 0 && (((size_t)coef | (size_t)flag) & 3) == 0 &&
                (((size_t)lr_state | (size_t)pw | (size_t)pu) & 7) == 0, "rua_lamb_moments: buffers must be 16-byte aligned");
  RUA_CHECK_ARG(pw != pu, "rua_lamb_moments: pw and pu are two buffers");
  RUA_CHECK_ARG(lamb_betas_ok(beta1, beta2, eps), "rua_lamb_moments: 0 <= beta < 1 and eps > 0 (got %g, %g, %g)", beta1, beta2, eps);
  RUA_CHECK_ARG(weight_decay >= 0.0, "rua_lamb_moments: negative weight decay");
  lamb_args a = {beta1, beta2, eps, grad_scale, clipvalue, 0.f, 0.f, 0.f, 0.f, 0.f};
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, theta, g, m, v, chunks, vars, coef, flag, lr_state, a, weight_decay,
                     pw, pu);
  RUA_LAUNCH_CHECK("rua_lamb_moments");
  return RUA_OK;
}

// ---- the finisher: clip_finish_kernel's staging (loss_optim.hip), once per sum ------------------------------------------------------------
#define LAMB_TILE 4096
__device__ __forceinline__ double lamb_add_in_order(double s, const double* x, int n) {
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
// sums[v] = the partials of variable v added in chunk order: the partials pass through LDS a tile at a time, thread v % 256 owns sums[v] and
// carries it from tile to tile, so a variable may span tiles and a thread may own several variables
__device__ void lamb_var_sums(const double* __restrict__ partials, int n_chunks, const rua_opt_var* __restrict__ vars, int n_vars, double* __restrict__ sums,
                              double* tile) {
  const int tid = threadIdx.x;
  for (int t0 = 0; t0 < n_chunks; t0 += LAMB_TILE) {
    const int tn = n_chunks - t0 < LAMB_TILE ? n_chunks - t0 : LAMB_TILE;
    for (int i = tid; i < tn; i += 256) tile[i] = partials[t0 + i];
    __syncthreads();
    for (int v = tid; v < n_vars; v += 256) {
      const rua_opt_var vr = vars[v];
      const int a = vr.chunk_begin > t0 ? vr.chunk_begin : t0, b = vr.chunk_end < t0 + tn ? vr.chunk_end : t0 + tn;
      if (t0 == 0 || a < b) {
        const double s = vr.chunk_begin >= t0 ? 0.0 : sums[v];
        sums[v] = lamb_add_in_order(s, tile + (a - t0), b > a ? b - a : 0);
      }
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void lamb_finish_kernel(const double* __restrict__ pw, const double* __restrict__ pu, int n_chunks,
                                                          const rua_opt_var* __restrict__ vars, int n_vars, const int32_t* __restrict__ flag,
                                                          double* __restrict__ var_wu, float* __restrict__ ratio, double* __restrict__ report) {
  __shared__ double tile[LAMB_TILE];
  __shared__ float s_min[4], s_max[4];
  __shared__ int s_forced[4];
  if (flag != nullptr && flag[0] != 0) return;            // uniform: the whole block leaves before the first barrier
  const int tid = threadIdx.x;
  lamb_var_sums(pw, n_chunks, vars, n_vars, var_wu, tile);
  lamb_var_sums(pu, n_chunks, vars, n_vars, var_wu + n_vars, tile);
  float mn = INFINITY, mx = -INFINITY;
  int forced = 0;
  for (int v = tid; v < n_vars; v += 256) {                // thread v % 256 wrote both sums itself
    const double W = var_wu[v], U = var_wu[n_vars + v];
    const bool ok = W > 0.0 && U > 0.0;                    // false for a NaN sum too: Keras' nested where
    const float r = ok ? (float)(sqrt(W) / sqrt(U)) : 1.f;
    ratio[v] = r;
    mn = fminf(mn, r); mx = fmaxf(mx, r);
    forced += ok ? 0 : 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); forced += __shfl_xor(forced, o, 64);
  }
  if ((tid & 63) == 0) { s_min[tid >> 6] = mn; s_max[tid >> 6] = mx; s_forced[tid >> 6] = forced; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) { mn = fminf(mn, s_min[w]); mx = fmaxf(mx, s_max[w]); forced += s_forced[w]; }
    report[0] = (double)mn;
    report[1] = (double)mx;
    report[2] = (double)forced;
    report[3] += 1.0;
  }
}
extern "C" int rua_lamb_finish(const double* pw, const double* pu, int n_chunks, const rua_opt_var* vars, int n_vars, const int32_t* flag, double* var_wu,
                               float* ratio, double* report, void* stream) {
  RUA_CHECK_ARG(pw && pu && vars && var_wu && ratio && report && n_chunks > 0 && n_vars > 0, "rua_lamb_finish: bad arguments");
  RUA_CHECK_ARG((((size_t)pw | (size_t)pu | (size_t)var_wu | (size_t)report) & 7) == 0 && ((size_t)vars & 15) == 0 && (((size_t)ratio | (size_t)flag) & 3) == 0,
                "rua_lamb_finish: misaligned buffers");
  hipLaunchKernelGGL(lamb_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pw, pu, n_chunks, vars, n_vars, flag, var_wu, ratio, report);
  RUA_LAUNCH_CHECK("rua_lamb_finish");
  return RUA_OK;
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------------------------------
template <bool WC>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ th, float* __restrict__ g, const rua_opt_chunk* __restrict__ chunks,
                                                         const rua_opt_var* __restrict__ vars, const float* __restrict__ ratio,
                                                         const int32_t* __restrict__ flag, const float* __restrict__ lr_dev,
                                                         const double* __restrict__ lr_state, double wd, int zero, bf16_t* __restrict__ wcopy) {
  const bool skip = flag != nullptr && flag[0] != 0;
  if (!WC && skip) return;                                 // pass 1 zeroed the gradient; without a bf16 copy nothing is left to do
  const rua_opt_chunk ck = chunks[blockIdx.x];
  const bool dec = wd != 0.0 && vars[ck.var].decay != 0;
  const float d = dec ? (float)(wd * lr_state[1]) : 0.f;
  const float step = __fmul_rn(ratio[ck.var], lr_dev[0]);
  th += ck.off; g += ck.off;
  if constexpr (WC) wcopy += ck.off;
  const int n4 = ck.len >> 2;
  auto one = [&](float tt, float u) { return __fsub_rn(lamb_decay(dec, d, tt), lamb_alone(__fmul_rn(step, u))); };
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 t4 = reinterpret_cast<const float4*>(th)[i];
    if (!skip) {
      const float4 u4 = reinterpret_cast<const float4*>(g)[i];
      t4.x = one(t4.x, u4.x); t4.y = one(t4.y, u4.y); t4.z = one(t4.z, u4.z); t4.w = one(t4.w, u4.w);
      reinterpret_cast<float4*>(th)[i] = t4;
      if (zero) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (WC) reinterpret_cast<uint2*>(wcopy)[i] = make_uint2(ET<bf16_t>::pk(t4.x, t4.y), ET<bf16_t>::pk(t4.z, t4.w));
  }
  const int i = (n4 << 2) + threadIdx.x;
  if (i < ck.len) {
    float tt = th[i];
    if (!skip) {
      tt = one(tt, g[i]);
      th[i] = tt;
      if (zero) g[i] = 0.f;
    }
    if constexpr (WC) wcopy[i] = (bf16_t)tt;
  }
}
extern "C" int rua_lamb_apply(float* theta, float* g, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars, const float* ratio,
                              const int32_t* flag, const float* lr_dev, const double* lr_state, double weight_decay, int zero_grad, void* wcopy_bf16,
                              void* stream) {
  RUA_CHECK_ARG(theta && g && chunks && vars && ratio && lr_dev && lr_state && n_chunks > 0, "rua_lamb_apply: bad arguments");
  RUA_CHECK_ARG((((size_t)theta | (size_t)g | (size_t)chunks | (size_t)vars) & 15) == 0 && ((size_t)wcopy_bf16 & 7) == 0 &&
                (((size_t)ratio | (size_t)flag | (size_t)lr_dev) & 3) == 0 && ((size_t)lr_state & 7) == 0, "rua_lamb_apply: buffers must be 16-byte aligned");
  RUA_CHECK_ARG(weight_decay >= 0.0, "rua_lamb_apply: negative weight decay");
  if (wcopy_bf16) hipLaunchKernelGGL((lamb_apply_kernel<true>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, theta, g, chunks, vars, ratio, flag, lr_dev, lr_state,
                                     weight_decay, zero_grad, (bf16_t*)wcopy_bf16);
  else hipLaunchKernelGGL((lamb_apply_kernel<false>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, theta, g, chunks, vars, ratio, flag, lr_dev, lr_state,
                          weight_decay, zero_grad, (bf16_t*)nullptr);
  RUA_LAUNCH_CHECK("rua_lamb_apply");
  return RUA_OK;
}

// Forward and data-gradient convolutions: a segmented implicit GEMM on MFMA (gfx950), channels-last.
// Kernels: conv_igemm, conv_dma, conv_dmap (+ _s / _chain), conv_halo, conv_pw, conv_img, conv_small, conv_splitk_finish.
// Host side (at the end): conv_plan_one() - descriptor -> ConvLaunch -, the kernel table and conv_issue().
// Exports: rua_conv_fwd, rua_conv_fwd_group, rua_conv_plan, rua_conv_group_plan and the rua_conv_* queries.
// The weight gradients (rua_conv_wgrad, wgrad_plan_one, ...) live in conv_wgrad.hip, the weight copies in weight_prep.hip.
//
// GEMM view: rows = output pixels (n,h,w), cols = output channels, K = (segment, tap, channel).
// A "unit" is 32 channels of one tap of one segment; a stage stages KU units of the A tile
// (128 pixels x 32 ch) and the B tile (BN couts x 32 ch) through LDS with the global loads of
// stage s+1 in flight under the MFMAs of stage s (issue-early / write-late).  Nothing is
// im2col'ed: a tap is an address offset, zero padding is a predicated load, nearest upsampling
// is a right shift of the source coordinate, channel concatenation is a list of segments.
// Epilogue: accumulators -> LDS fp32 tile -> 8-channel pieces per thread: bias, residual /
// ReLU-mask from `aux`, per-channel statistics (fp32 partials, fp64 atomics), 16-byte stores.
#include "common.h"


template <typename T> __device__ __forceinline__ void load8(const unsigned char* base, size_t elem_off, float* f) {
  if constexpr (sizeof(T) == 2) {
    ET<T>::unpack(ldg16(base + elem_off * 2), f);
  } else {
    ET<T>::unpack(ldg16(base + elem_off * 4), f);
    ET<T>::unpack(ldg16(base + elem_off * 4 + 16), f + 4);
  }
}
template <typename T> __device__ __forceinline__ void store8(unsigned char* base, size_t elem_off, const float* f) {
  if constexpr (sizeof(T) == 2) {
    stg16(base + elem_off * 2, ET<T>::pack(f));
  } else {
    stg16(base + elem_off * 4, ET<T>::pack(f));
    stg16(base + elem_off * 4 + 16, ET<T>::pack(f + 4));
  }
}

template <typename T, int BM, int BN> __host__ __device__ constexpr int conv_smem_base() {
  constexpr int ROWB = (sizeof(T) == 2) ? 80 : 132;
  constexpr int a = 2 * (BM + BN) * ROWB;
  constexpr int b = BM * (BN + 4) * 4 + 4 * (BN / 8) * 16 * 4;
  return ((a > b ? a : b) + 15) / 16 * 16;
}

// Shared epilogue of one 128 x BN output tile whose fp32 sums sit in `src` (LDS tile or split-K workspace):
// 8-channel pieces per thread: bias, accumulate, residual / ReLU mask from aux, output ReLU, per-channel
// statistics (fp32 partials -> wave shuffles -> LDS -> one fp64 atomic per channel and block), 16-byte stores.
// SLABS: `src` is the first of p.ksplit fp32 slabs (stride M*Cout floats) whose sum is the tile (split-K finisher).
#ifdef RUA_DMAP_DBG_TS                                 // (debug build: phase timestamps of block 0 / thread 0 of conv_dmap, read by rua_debug_ts)
__device__ unsigned long long g_dbg_ts[32];
#define RUA_TS(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { g_dbg_ts[i] = clock64(); g_dbg_ts[16 + (i)] = wall_clock64(); } } while (0)
extern "C" int rua_debug_ts(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_ts), sizeof(g_dbg_ts)); }
#else
#define RUA_TS(i) do { } while (0)
#endif
// KIND > 0: the descriptor's flags as COMPILE-TIME constants for the forms the LDS-DMA kernels meet on whole tiles with a dense output
// (conv_epi_kind below: every row and channel of the tile exists, out_stride 1, no output ReLU, no accumulate): KIND = 1 + aux_mode +
// 3 * stats_mode, instantiated for bias + statistics sum v / sum v^2 (a ResBlock's first convs), ReLU mask from aux + statistics sum g /
// sum g*aux (data gradients), residual add from aux (the summed second convs), plain.  The generic form spends ~5 us per 128 x 128 tile with one wave per SIMD - per-piece
// branches on kernel arguments, their scalar loads and waits (measured: rounds of tools/bench_conv_levels.py with the epilogue run 1x / 3x
// / not at all) - as much as a third of a 9.7 GFLOP convolution.
template <typename T, int BM, int BN, bool SLABS = false, int KIND = 0>
__device__ __forceinline__ void conv_epilogue(const ConvK& p, long long m0, int n0, int bm_i, const float* src, int sstride, float* sred,
                                              const int* rowtab = nullptr, int nrows = BM, float* carry = nullptr, bool last = true) {
  constexpr bool FULL = KIND > 0;
  const int aux_mode = FULL ? (KIND - 1) % 3 : p.aux_mode;
  const int stats_mode = FULL ? (KIND - 1) / 3 : p.stats_mode;
  const int accumulate = FULL ? 0 : p.accumulate;
  const int out_relu = FULL ? 0 : p.out_relu;
  constexpr int CG = BN / 8;
  constexpr int ROWS_PP = 256 / CG;
  constexpr int EP = BM / ROWS_PP;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int HW = p.H * p.W;
  const int cg = tid % CG, r0 = tid / CG;
  const int co = n0 + cg * 8;
  const bool cok = FULL || co < p.Cout;
  float s1[8], s2[8], bias8[8], ms8[8], mt8[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; bias8[j] = 0.f; ms8[j] = 1.f; mt8[j] = 0.f; }
  if (carry) {                                         // statistics partials carried over several calls of one block
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = carry[j]; s2[j] = carry[8 + j]; }
  }
  if (cok) {
    if (p.bias) {
#pragma unroll
      for (int j = 0; j < 8; ++j) bias8[j] = p.bias[co + j];
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (p.bias_more[q]) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bias8[j] += p.bias_more[q][co + j];
        }
    }
    if (aux_mode == 2) {
      if (p.mscale) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ms8[j] = p.mscale[co + j];
      }
      if (p.mshift) {
#pragma unroll
        for (int j = 0; j < 8; ++j) mt8[j] = p.mshift[co + j];
      }
    }
  }
  const bool plain_out = FULL || (p.out_stride == 1 && p.OH == p.H && p.OW == p.W);
  // pass 1: addresses, and ALL global loads of this thread's pieces (aux, old output) issued back to back - one exposed
  // memory latency per thread instead of one per piece (the pieces are independent; a load-use pair per loop iteration
  // serialised them: 4-6 dependent HBM round trips per thread)
  unsigned ooff[EP];                                 // element offsets (tensors are < 2 GiB: checked by the launcher)
  int mrow[EP];
  constexpr int NV = sizeof(T) == 2 ? 1 : 2;         // 16-byte vectors per 8-channel piece; kept RAW here so that no
  uint4 araw[EP][NV], oraw[EP][NV];                 // unpack (= use) sits between the loads
#pragma unroll
  for (int e = 0; e < EP; ++e) {
    const int row = r0 + e * ROWS_PP;
    long long m = m0 + row;
    if (rowtab) m = (row < nrows) ? (long long)rowtab[row] : -1;      // tile row -> pixel table (lattice tiles of conv_halo)
    if (!FULL && !(m >= 0 && m < p.M && cok)) m = -1;
    mrow[e] = (int)m;
    ooff[e] = 0;
    if (m >= 0) {
      if (plain_out) {
        ooff[e] = (unsigned)m * p.Cout + co;
      } else {
        const int mm = (int)m;
        const int n = mm / HW, rem = mm - n * HW, h = rem / p.W, w = rem - h * p.W;
        ooff[e] = (unsigned)(((n * p.OH + h * p.out_stride) * p.OW + w * p.out_stride) * p.Cout + co);
      }
      if (aux_mode != 0) {
#pragma unroll
        for (int v_ = 0; v_ < NV; ++v_) araw[e][v_] = ldg16(p.aux + ((size_t)m * p.Cout + co) * sizeof(T) + v_ * 16);
      }
      if (accumulate) {
#pragma unroll
        for (int v_ = 0; v_ < NV; ++v_) oraw[e][v_] = ldg16(p.y + (size_t)ooff[e] * sizeof(T) + v_ * 16);
      }
    }
  }
  RUA_TS(4);
  // pass 2: arithmetic, statistics, stores
#pragma unroll
  for (int e = 0; e < EP; ++e) {
    const int row = r0 + e * ROWS_PP;
    if (mrow[e] >= 0) {
      float v[8];
      float4 t0 = *reinterpret_cast<const float4*>(&src[(size_t)row * sstride + cg * 8]);
      float4 t1 = *reinterpret_cast<const float4*>(&src[(size_t)row * sstride + cg * 8 + 4]);
      if (SLABS) {
        const size_t slab = (size_t)p.M * p.Cout;
        for (int k = 1; k < p.ksplit; ++k) {                 // fixed order: split-K results are bit-reproducible
          const float4 u0 = *reinterpret_cast<const float4*>(&src[k * slab + (size_t)row * sstride + cg * 8]);
          const float4 u1 = *reinterpret_cast<const float4*>(&src[k * slab + (size_t)row * sstride + cg * 8 + 4]);
          t0.x += u0.x; t0.y += u0.y; t0.z += u0.z; t0.w += u0.w; t1.x += u1.x; t1.y += u1.y; t1.z += u1.z; t1.w += u1.w;
        }
      }
      v[0] = t0.x; v[1] = t0.y; v[2] = t0.z; v[3] = t0.w; v[4] = t1.x; v[5] = t1.y; v[6] = t1.z; v[7] = t1.w;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += bias8[j];
      float a8[8];
      if (accumulate) {
        float o8[8];
#pragma unroll
        for (int v_ = 0; v_ < NV; ++v_) ET<T>::unpack(oraw[e][v_], o8 + v_ * 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += o8[j];
      }
      if (aux_mode != 0) {
#pragma unroll
        for (int v_ = 0; v_ < NV; ++v_) ET<T>::unpack(araw[e][v_], a8 + v_ * 4);
      }
      if (aux_mode == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += a8[j];
      } else if (aux_mode == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (fmaf(ms8[j], a8[j], mt8[j]) > 0.f) ? v[j] : 0.f;
      }
      if (out_relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
      }
      if (stats_mode == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { s1[j] += v[j]; s2[j] = fmaf(v[j], v[j], s2[j]); }
      } else if (stats_mode == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { s1[j] += v[j]; s2[j] = fmaf(v[j], a8[j], s2[j]); }
      }
      store8<T>(p.y, ooff[e], v);
    }
  }
  RUA_TS(5);
  if (carry) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { carry[j] = s1[j]; carry[8 + j] = s2[j]; }
  }
  if (stats_mode != 0 && last) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int o = CG; o < 64; o <<= 1) { s1[j] += __shfl_xor(s1[j], o, 64); s2[j] += __shfl_xor(s2[j], o, 64); }
    }
    if (lane < CG) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { sred[(wid * CG + lane) * 16 + j] = s1[j]; sred[(wid * CG + lane) * 16 + 8 + j] = s2[j]; }
    }
    __syncthreads();
    if (tid < CG * 16) {
      const int g = tid / 16, k = tid % 16;
      const float t = sred[(0 * CG + g) * 16 + k] + sred[(1 * CG + g) * 16 + k] + sred[(2 * CG + g) * 16 + k] + sred[(3 * CG + g) * 16 + k];
      const int c = n0 + g * 8 + (k & 7);
      if (c < p.Cout) unsafeAtomicAdd(&p.stats[(size_t)(bm_i & (p.stats_R - 1)) * 2 * p.Cout + (k >> 3) * p.Cout + c], (double)t);
    }
  }
}

// which compile-time form of the epilogue serves this tile size (0: the generic one); kernel-side mirror of the host's choice
template <int BM, int BN>
__device__ __forceinline__ int conv_epi_kind(const ConvK& p) {
  if (!p.epi_fast || p.M % BM != 0 || p.Cout % BN != 0 || p.out_stride != 1 || p.OH != p.H || p.OW != p.W || p.out_relu || p.accumulate) return 0;
  if (p.aux_mode > 2 || p.stats_mode > 2 || (p.stats_mode != 0 && p.stats == nullptr)) return 0;
  return 1 + p.aux_mode + 3 * p.stats_mode;
}
// the epilogue of a whole tile through its compile-time form where one applies
template <typename T, int BM, int BN>
__device__ __forceinline__ void conv_epilogue_pick(const ConvK& p, long long m0, int n0, int bm_i, const float* src, int sstride, float* sred,
                                                   float* carry = nullptr, bool last = true) {
  const int kind = conv_epi_kind<BM, BN>(p);
  if (kind == 4) conv_epilogue<T, BM, BN, false, 4>(p, m0, n0, bm_i, src, sstride, sred, nullptr, BM, carry, last);        // bias, statistics
  else if (kind == 9) conv_epilogue<T, BM, BN, false, 9>(p, m0, n0, bm_i, src, sstride, sred, nullptr, BM, carry, last);   // mask, statistics 2
  else if (kind == 2) conv_epilogue<T, BM, BN, false, 2>(p, m0, n0, bm_i, src, sstride, sred, nullptr, BM, carry, last);   // residual
  else if (kind == 1) conv_epilogue<T, BM, BN, false, 1>(p, m0, n0, bm_i, src, sstride, sred, nullptr, BM, carry, last);   // plain
  else conv_epilogue<T, BM, BN>(p, m0, n0, bm_i, src, sstride, sred, nullptr, BM, carry, last);
}

template <typename T, int BM, int BN>
__device__ __forceinline__ void conv_igemm_body(const ConvK& p) {
  constexpr int KU = 2;
  constexpr int VEC = ET<T>::VEC, ES = sizeof(T);
  constexpr int PPR = 32 / VEC;
  constexpr int ROWB = (ES == 2) ? 80 : 132;
  constexpr int RPP = 256 / PPR;
  constexpr int APASS = BM / RPP;
  constexpr int BPIECES = BN * PPR;
  constexpr int BPASS = (BPIECES + 255) / 256;
  constexpr int WN = (BN >= 128 || (BN == 64 && BM == 128)) ? 2 : 1, WM = 4 / WN;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int CSTR = BN + 4;
  constexpr int UTAB_OFF = conv_smem_base<T, BM, BN>();     // the unit table sits behind the staging / epilogue area

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sA = smem;
  unsigned char* sB = smem + KU * BM * ROWB;
  float* sC = reinterpret_cast<float*>(smem);

  // XCD-aware, bijective remap: blocks b and b+8 share an XCD (and its L2), so give each XCD a
  // contiguous run of tiles; the BN-tiles of one pixel tile then hit the same L2.
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int vid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int bn_i = vid % p.nbn;
  const int bm_i = (vid / p.nbn) % p.nbm;
  const int ks_i = vid / (p.nbn * p.nbm);
  const long long m0 = (long long)bm_i * BM;
  const int n0 = bn_i * BN;

  const int tid = threadIdx.x;
  const int aq = tid % PPR, ar = tid / PPR;
  const int HW = p.H * p.W;
  // per-thread pixel rows of the A tile: logical source coordinates (output coordinate * stride), decoded once
  int an[APASS], ah[APASS], aw[APASS];
  bool av[APASS];
#pragma unroll
  for (int i = 0; i < APASS; ++i) {
    long long m = m0 + ar + i * RPP;
    av[i] = m < p.M;
    int mm = av[i] ? (int)m : 0;
    int n = mm / HW, rem = mm - n * HW, h = rem / p.W;
    an[i] = n; ah[i] = h * p.stride; aw[i] = (rem - h * p.W) * p.stride;
  }
  constexpr int BROWS = (BPIECES < 256) ? BPIECES : 256;
  const int bq = tid % PPR, br = tid / PPR;          // B piece column / row (pass j adds j*RPP rows)
  const bool bthread = tid < BROWS;

  uint4 ra0[KU][APASS], rb0[KU][BPASS];
  const uint4 zero4 = make_uint4(0, 0, 0, 0);

  // ---- K iteration: a per-unit table built once per block in LDS ------------------------------------------
  // entry u = { tap/chunk element offset into the source, element offset into the weights, (dh << 16) | (dw & 0xffff),
  //             segment | channels left in this chunk << 8 }.  The loader reads ONE broadcast 16-byte entry per unit
  // instead of re-deriving segment / tap / chunk with scalar code every stage (that bookkeeping was ~50 SALU + ~35
  // VALU instructions per unit and dominated the issue slots of the K loop).
  int4* utab = reinterpret_cast<int4*>(smem + UTAB_OFF);
  for (int u = tid; u < p.nunits; u += 256) {
    int sgi = 0;
    while (sgi + 1 < p.nseg && u >= p.seg[sgi + 1].ubegin) ++sgi;
    const SegK sg = p.seg[sgi];
    const int loc = u - sg.ubegin;
    const int tap = loc / sg.nchunk, chunk = loc - tap * sg.nchunk;
    int dh = 0, dw = 0;
    if (sg.taps == 9) { dh = (tap / 3 - 1) * sg.dil; dw = (tap % 3 - 1) * sg.dil; }
    int4 e;
    e.x = (dh * sg.Ws + dw) * sg.C + chunk * 32;
    e.y = tap * p.Cout * sg.C + chunk * 32;
    e.z = (dh << 16) | (dw & 0xffff);
    int left = sg.C - chunk * 32; if (left > 32) left = 32;
    e.w = sgi | (left << 8);
    utab[u] = e;
  }
  int cs = -1;                        // segment the per-thread bases below belong to
  // per-segment, per-thread precomputed element offsets (32-bit: every tensor here is < 2^31 bytes)
  int abase[APASS];                   // ((n*Hs + (hS>>up))*Ws + (wS>>up))*C + aq*VEC   (tap offset added per unit)
  int bbase[BPASS];                   // row*C + bq*VEC
  __amdgpu_buffer_rsrc_t rx = make_rsrc(p.seg[0].x, p.seg[0].xbytes), rw = make_rsrc(p.seg[0].w, p.seg[0].wbytes);
  unsigned sHL = 0, sWL = 0;

  auto enter_segment = [&](int s) {
    const SegK sg = p.seg[s];
    cs = s; rx = make_rsrc(sg.x, sg.xbytes); rw = make_rsrc(sg.w, sg.wbytes);
    sHL = (unsigned)(sg.Hs << sg.up); sWL = (unsigned)(sg.Ws << sg.up);
#pragma unroll
    for (int i = 0; i < APASS; ++i)
      abase[i] = ((an[i] * sg.Hs + (ah[i] >> sg.up)) * sg.Ws + (aw[i] >> sg.up)) * sg.C + aq * VEC;
#pragma unroll
    for (int j = 0; j < BPASS; ++j) bbase[j] = (n0 + br + j * RPP) * sg.C + bq * VEC;
  };

  auto load_stage = [&](int st, uint4 (&ra)[KU][APASS], uint4 (&rb)[KU][BPASS]) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int unit = st * KU + u;
      if (unit < p.nunits) {
        const int4 e = utab[unit];
        const int sgi = __builtin_amdgcn_readfirstlane(e.w & 0xff);
        if (sgi != cs) enter_segment(sgi);
        const int dh = e.z >> 16, dw = (int)(short)(e.z & 0xffff);
        const int left = e.w >> 8;
        const bool cok = aq * VEC < left;
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
          const bool ok = av[i] && cok && (unsigned)(ah[i] + dh) < sHL && (unsigned)(aw[i] + dw) < sWL;
          ra[u][i] = bufload16(rx, ok ? (unsigned)((abase[i] + e.x) * ES) : RUA_OOB);
        }
        const bool bcok = bq * VEC < left;
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
          const bool ok = bthread && bcok && (n0 + br + j * RPP) < p.Cout;
          rb[u][j] = bufload16(rw, ok ? (unsigned)((bbase[j] + e.y) * ES) : RUA_OOB);
        }
      } else {
#pragma unroll
        for (int i = 0; i < APASS; ++i) ra[u][i] = zero4;
#pragma unroll
        for (int j = 0; j < BPASS; ++j) rb[u][j] = zero4;
      }
    }
  };

  auto write_stage = [&](uint4 (&ra)[KU][APASS], uint4 (&rb)[KU][BPASS]) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int i = 0; i < APASS; ++i) {
        unsigned char* dst = sA + (u * BM + ar + i * RPP) * ROWB + aq * 16;
        if constexpr (ES == 2) {
          *reinterpret_cast<uint4*>(dst) = ra[u][i];
        } else {
          uint32_t* d = reinterpret_cast<uint32_t*>(dst);
          d[0] = ra[u][i].x; d[1] = ra[u][i].y; d[2] = ra[u][i].z; d[3] = ra[u][i].w;
        }
      }
#pragma unroll
      for (int j = 0; j < BPASS; ++j) {
        if (bthread) {
          unsigned char* dst = sB + (u * BN + br + j * RPP) * ROWB + bq * 16;
          if constexpr (ES == 2) {
            *reinterpret_cast<uint4*>(dst) = rb[u][j];
          } else {
            uint32_t* d = reinterpret_cast<uint32_t*>(dst);
            d[0] = rb[u][j].x; d[1] = rb[u][j].y; d[2] = rb[u][j].z; d[3] = rb[u][j].w;
          }
        }
      }
    }
  };

  const int lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int lr = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  const int nstages_all = (p.nunits + KU - 1) / KU;
  const int st_begin = ks_i * p.stages_per_split;
  int nstages = st_begin + p.stages_per_split;
  if (nstages > nstages_all) nstages = nstages_all;
  __syncthreads();                     // unit table visible
  auto mfma_stage = [&]() {
    // Branch-free MFMA section: units past the end of K were staged as zeros, so they are simply multiplied
    // (a conditional here splits the loop into blocks and makes hipcc copy every accumulator AGPR<->VGPR per stage).
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const unsigned char* pa = sA + (u * BM + wm * (BM / WM) + lr) * ROWB;
      const unsigned char* pb = sB + (u * BN + wn * (BN / WN) + lr) * ROWB;
      if constexpr (ES == 2) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          bf16x8 fa[TM], fb[TN];
#pragma unroll
          for (int a = 0; a < TM; ++a) fa[a] = *reinterpret_cast<const bf16x8*>(pa + a * 32 * ROWB + ks * 32 + lh * 16);
#pragma unroll
          for (int b = 0; b < TN; ++b) fb[b] = *reinterpret_cast<const bf16x8*>(pb + b * 32 * ROWB + ks * 32 + lh * 16);
#pragma unroll
          for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          float fa[TM], fb[TN];
#pragma unroll
          for (int a = 0; a < TM; ++a) fa[a] = *reinterpret_cast<const float*>(pa + a * 32 * ROWB + (ks * 2 + lh) * 4);
#pragma unroll
          for (int b = 0; b < TN; ++b) fb[b] = *reinterpret_cast<const float*>(pb + b * 32 * ROWB + (ks * 2 + lh) * 4);
#pragma unroll
          for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
      }
    }
  };
  // Software pipeline, depth 1: the loads of stage s+1 are in flight while stage s is multiplied.  (Depth 2 was
  // measured slower at every level: the second register set costs a wave of occupancy per SIMD.)
  load_stage(st_begin, ra0, rb0);
  for (int st = st_begin; st < nstages; ++st) {
    __syncthreads();
    write_stage(ra0, rb0);
    __syncthreads();
    if (st + 1 < nstages) load_stage(st + 1, ra0, rb0);
    mfma_stage();
  }

  // ---- epilogue -------------------------------------------------------------------------
  if (p.ksplit > 1) {
    // split-K: store the partial tile into this K slice's fp32 slab of the workspace (plain stores, 128-byte row
    // segments per wave instruction: float atomics run at ~1.3 TB/s chip-wide, stores at ~6); the slabs are summed,
    // and bias / mask / statistics / store applied, by conv_splitk_finish.
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const long long m = m0 + wm * (BM / WM) + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
          const int c = n0 + wn * (BN / WN) + b * 32 + lr;
          if (m < p.M && c < p.Cout) p.ws[((size_t)ks_i * p.M + m) * p.Cout + c] = acc[a][b][i];
        }
    return;
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = wm * (BM / WM) + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
        const int col = wn * (BN / WN) + b * 32 + lr;
        sC[row * CSTR + col] = acc[a][b][i];
      }
  __syncthreads();
  conv_epilogue<T, BM, BN>(p, m0, n0, bm_i, sC, CSTR, sC + BM * CSTR);
}

// split-K finisher: the shared epilogue over the sum of the K slices' fp32 slabs (one block per FM x 64 output tile;
// FM = 32 where 128-row tiles would leave most of the chip idle: the 8x8 level has 4 x 16 of them)
template <typename T, int BM, int BN> __global__ __launch_bounds__(256) void conv_igemm(const ConvK p) { conv_igemm_body<T, BM, BN>(p); }
// grouped launch (rua_conv_fwd_group): independent convolutions of one shape class - the dilation branches of a ResBlock - in ONE
// grid, blockIdx.y picks the member (no drain / launch gap between the branches, their tails overlap)
template <typename T, int BM, int BN> __global__ __launch_bounds__(256) void conv_igemm_g(const ConvKG g) { conv_igemm_body<T, BM, BN>(g.k[blockIdx.y]); }

template <typename T, int FM>
__global__ __launch_bounds__(256) void conv_splitk_finish(const ConvK p) {
  __shared__ float sred[4 * 8 * 16];
  const int nbn = (p.Cout + 63) / 64;
  const int bn_i = blockIdx.x % nbn, bm_i = blockIdx.x / nbn;
  const long long m0 = (long long)bm_i * FM;
  const int n0 = bn_i * 64;
  conv_epilogue<T, FM, 64, true>(p, m0, n0, bm_i, p.ws + (size_t)m0 * p.Cout + n0, p.Cout, sred);
}
template <typename T> static void launch_splitk_finish(const ConvK& k, hipStream_t st) {
  rua_record_mid_event(st);
  const int nbn = (k.Cout + 63) / 64;
  const long long t128 = ((k.M + 127) / 128) * nbn;
  if (t128 >= 512) hipLaunchKernelGGL((conv_splitk_finish<T, 128>), dim3((unsigned)t128), dim3(256), 0, st, k);
  else hipLaunchKernelGGL((conv_splitk_finish<T, 32>), dim3((unsigned)(((k.M + 31) / 32) * nbn)), dim3(256), 0, st, k);
}

// =========================================================================================
// conv_dma<BM,BN>: the bf16 production kernel.  Same GEMM view, tiles, unit table and epilogue as conv_igemm, but the
// A / B stage tiles are written by LDS-DMA (buffer_load ... lds: no VGPR staging, no ds_write; out-of-range lanes
// write zeros, which IS the zero padding) into THREE stage buffers, with the loads of two stages in flight behind a
// counted vmcnt and ONE raw barrier per stage.  LDS rows are 64 B (32 bf16 channels) unpadded, as the DMA requires
// (destination = wave-uniform base + lane*16); bank conflicts of the ds_read_b128 fragment reads are removed by an
// XOR swizzle of the 16-byte piece index, slot = piece ^ ((row >> 2) & 3), applied to the per-lane SOURCE address
// and to the fragment read address (never to the DMA destination).

template <int BM, int BN>
__global__ __launch_bounds__(256) void conv_dma(const ConvK p) {
  typedef bf16_t T;
  constexpr int KU = 2, NBUF = 3, ROWB = 64;
  constexpr int A_BYTES = KU * BM * ROWB, B_BYTES = KU * BN * ROWB;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int AI = BM / 64;                       // A DMA instructions per wave per unit (16 rows each)
  constexpr int BI = (BN + 63) / 64;                // B DMA instructions per wave per unit (BN = 32: waves 2,3 load zeros)
  constexpr int PER_STAGE = KU * (AI + BI);         // DMA instructions per wave per stage (uniform across waves)
  constexpr int WN = (BN >= 128 || (BN == 64 && BM == 128)) ? 2 : 1, WM = 4 / WN;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int CSTR = BN + 4;
  constexpr int DUMMY_OFF = NBUF * STAGE;           // 1 KiB sink for the padding instructions of BN = 32
  constexpr int EPI = BM * CSTR * 4 + 4 * (BN / 8) * 16 * 4;
  constexpr int BASE = ((NBUF * STAGE + 1024 > EPI ? NBUF * STAGE + 1024 : EPI) + 15) / 16 * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sC = reinterpret_cast<float*>(smem);

  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int vid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int bn_i = vid % p.nbn;
  const int bm_i = (vid / p.nbn) % p.nbm;
  const int ks_i = vid / (p.nbn * p.nbm);
  const long long m0 = (long long)bm_i * BM;
  const int n0 = bn_i * BN;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int HW = p.H * p.W;

  // this lane's rows: DMA instruction i of this wave covers tile rows (wid*AI + i)*16 .. +15, lane -> row lane/4,
  // LDS slot lane%4, i.e. source piece (lane%4) ^ ((row >> 2) & 3)
  const int lrow = lane >> 2, lslot = lane & 3;
  int an[AI], ah[AI], aw[AI], aqv[AI];
  bool av[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int row = (wid * AI + i) * 16 + lrow;
    const long long m = m0 + row;
    av[i] = m < p.M;
    const int mm = av[i] ? (int)m : 0;
    const int n = mm / HW, rem = mm - n * HW, h = rem / p.W;
    an[i] = n; ah[i] = h * p.stride; aw[i] = (rem - h * p.W) * p.stride;
    aqv[i] = (lslot ^ ((row >> 2) & 3)) * 8;             // first channel of the piece this lane fetches
  }
  int brow[BI], bqv[BI];
  bool bv[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int row = (wid * BI + j) * 16 + lrow;          // B tile row (output channel); rows >= BN are padding
    brow[j] = row; bv[j] = row < BN && (n0 + row) < p.Cout;
    bqv[j] = (lslot ^ ((row >> 2) & 3)) * 8;
  }

  int cs = -1;
  int abase[AI], bbase[BI];
  __amdgpu_buffer_rsrc_t rx = make_rsrc(p.seg[0].x, p.seg[0].xbytes), rw = make_rsrc(p.seg[0].w, p.seg[0].wbytes);
  unsigned sHL = 0, sWL = 0;
  auto enter_segment = [&](int s_) {
    const SegK sg = p.seg[s_];
    cs = s_; rx = make_rsrc(sg.x, sg.xbytes); rw = make_rsrc(sg.w, sg.wbytes);
    sHL = (unsigned)(sg.Hs << sg.up); sWL = (unsigned)(sg.Ws << sg.up);
#pragma unroll
    for (int i = 0; i < AI; ++i)
      abase[i] = ((an[i] * sg.Hs + (ah[i] >> sg.up)) * sg.Ws + (aw[i] >> sg.up)) * sg.C + aqv[i];
#pragma unroll
    for (int j = 0; j < BI; ++j) bbase[j] = (n0 + brow[j]) * sg.C + bqv[j];
  };

  // K iteration state (segment, tap, chunk): scalar, division-free.  (No LDS table here: hipcc puts a vmcnt(0) in
  // front of any ds_read issued while LDS-DMA writes are in flight, which would drain the pipeline every stage.)
  int u_seg = 0, u_tap = 0, u_chunk = 0, s_taps = 1, s_nchunk = 1, s_C = 0, s_Ws = 0, s_dil = 1;
  auto seek_unit = [&](int unit) {
    int sgi = 0;
    while (sgi + 1 < p.nseg && unit >= p.seg[sgi + 1].ubegin) ++sgi;
    const int loc = unit - p.seg[sgi].ubegin;
    u_seg = sgi; u_tap = loc / p.seg[sgi].nchunk; u_chunk = loc - u_tap * p.seg[sgi].nchunk;
  };
  auto issue_stage = [&](int st, int buf) {
    unsigned char* sA = smem + buf * STAGE;
    unsigned char* sB = sA + A_BYTES;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int unit = st * KU + u;
      const bool live = unit < p.nunits;
      int dh = 0, dw = 0, left = 0, ex = 0, ey = 0;
      if (live) {
        if (u_seg != cs) {
          enter_segment(u_seg);
          const SegK sg = p.seg[u_seg];
          s_taps = sg.taps; s_nchunk = sg.nchunk; s_C = sg.C; s_Ws = sg.Ws; s_dil = sg.dil;
        }
        if (s_taps == 9) {
          const int t3 = (u_tap >= 6) ? 2 : (u_tap >= 3) ? 1 : 0;
          dh = (t3 - 1) * s_dil; dw = (u_tap - 3 * t3 - 1) * s_dil;
        }
        ex = (dh * s_Ws + dw) * s_C + u_chunk * 32;
        ey = u_tap * p.Cout * s_C + u_chunk * 32;
        left = s_C - u_chunk * 32; if (left > 32) left = 32;
        if (++u_chunk == s_nchunk) { u_chunk = 0; if (++u_tap == s_taps) { u_tap = 0; ++u_seg; } }
      }
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const bool ok = live && av[i] && aqv[i] < left && (unsigned)(ah[i] + dh) < sHL && (unsigned)(aw[i] + dw) < sWL;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sA + (u * BM + (wid * AI + i) * 16) * ROWB), 16,
                                                 ok ? (unsigned)((abase[i] + ex) * 2) : RUA_OOB, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < BI; ++j) {
        const bool ok = live && bv[j] && bqv[j] < left;
        unsigned char* dst = (brow[j] - lrow < BN) ? sB + (u * BN + (wid * BI + j) * 16) * ROWB : smem + DUMMY_OFF;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_p)dst, 16, ok ? (unsigned)((bbase[j] + ey) * 2) : RUA_OOB, 0, 0, 0);
      }
    }
  };

  const int wm = wid / WN, wn = wid % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int xs = (lr >> 2) & 3;                          // swizzle term of this lane's fragment rows (tile offsets are multiples of 32)
  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  auto mfma_stage = [&](int buf) {
    const unsigned char* sA = smem + buf * STAGE;
    const unsigned char* sB = sA + A_BYTES;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const unsigned char* pa = sA + (u * BM + wm * (BM / WM) + lr) * ROWB;
      const unsigned char* pb = sB + (u * BN + wn * (BN / WN) + lr) * ROWB;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int slot = ((ks * 2 + lh) ^ xs) * 16;
        bf16x8 fa[TM], fb[TN];
#pragma unroll
        for (int a = 0; a < TM; ++a) fa[a] = *reinterpret_cast<const bf16x8*>(pa + a * 32 * ROWB + slot);
#pragma unroll
        for (int b = 0; b < TN; ++b) fb[b] = *reinterpret_cast<const bf16x8*>(pb + b * 32 * ROWB + slot);
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int b = 0; b < TN; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
    }
  };

  const int nstages_all = (p.nunits + KU - 1) / KU;
  const int st_begin = ks_i * p.stages_per_split;
  int nstages = st_begin + p.stages_per_split;
  if (nstages > nstages_all) nstages = nstages_all;
  seek_unit(st_begin * KU);
  issue_stage(st_begin, 0);
  issue_stage(st_begin + 1, 1);                          // past-the-end stages load zeros: the instruction count per stage stays uniform
  int buf = 0;
  for (int st = st_begin; st < nstages; ++st) {
    // all but the newest stage's DMAs of this wave have landed -> stage st is in LDS (this wave's part) ...
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PER_STAGE) : "memory");
    // ... and after the barrier every wave's part; every wave has also finished reading the buffer refilled next
    __builtin_amdgcn_s_barrier();
    int nb = buf + 2; if (nb >= NBUF) nb -= NBUF;
    issue_stage(st + 2, nb);
    mfma_stage(buf);
    if (++buf == NBUF) buf = 0;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // drain before the epilogue reuses the stage buffers
  __builtin_amdgcn_s_barrier();

  if (p.ksplit > 1) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const long long m = m0 + wm * (BM / WM) + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
          const int c = n0 + wn * (BN / WN) + b * 32 + lr;
          if (m < p.M && c < p.Cout) p.ws[((size_t)ks_i * p.M + m) * p.Cout + c] = acc[a][b][i];
        }
    return;
  }
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = wm * (BM / WM) + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
        const int col = wn * (BN / WN) + b * 32 + lr;
        sC[row * CSTR + col] = acc[a][b][i];
      }
  __syncthreads();
  conv_epilogue<T, BM, BN>(p, m0, n0, bm_i, sC, CSTR, sC + BM * CSTR);
}

// =========================================================================================
// conv_dmap<BM,BN>: conv_dma with (a) a K iteration whose per-stage cost is one v_add per DMA instruction - everything
// that depends on the tap (zero-padding validity, source offset) is recomputed only when the tap changes, which
// requires every segment's C to be a multiple of 64 (a stage = 2 units of 32 channels never straddles a tap) -,
// (b) 64x64 wave tiles (one LDS fragment read per MFMA instead of 1.5) and (c) a software pipeline across the stage
// barrier: the fragments of k-step 0 of stage s+1 are read while the last MFMAs of stage s execute, so with one wave
// per SIMD the LDS latency is not exposed after every barrier.  Three stage buffers:
//   iteration s, k-steps 0..2 : read fragments of k-step kk+1, MFMA k-step kk
//   k-step 3                  : vmcnt(PER_STAGE) [stage s+1 landed] ; lgkmcnt(0) [my reads of stage s done] ; s_barrier ;
//                               DMA stage s+3 into the buffer of stage s ; read fragments (s+1, 0) ; MFMA k-step 3
#ifndef RUA_DMAP_NBUF
#define RUA_DMAP_NBUF 3                                   // stage buffers of the LDS-DMA ring (NBUF - 1 stages in flight)
#endif
// CHAIN (conv_dmap_chain): the members of a grouped launch (same pixel tiles, same output channels: the dilation branches of a
// ResBlock) run BACK TO BACK inside one block - the K iteration walks member after member without ever letting the DMA ring run
// dry, and at a member boundary the accumulators leave through an epilogue of their own (LDS behind the ring, two half tiles)
// while the first stages of the next member are already in flight.  Measured motive (tools/bench_conv_levels.py, 8 x 64 x 64 x
// 128): three members as one K x 3 launch 45 - 48 us, as three blocks per CU (conv_dmap_g) 66 - 70 us - a block turnover
// (epilogue, exit, dispatch, prologue, ring refill from cold) costs ~11 us of a ~22 us member.
// SPREAD: the DMA instructions of a stage are issued a quarter per k-step BETWEEN the MFMAs instead of in one burst behind the stage barrier.
// Motive (tools/dmap_phases.py, in-kernel timestamps, 8 x 64 x 64 x 128): the K loop takes 11.96 us, without its DMA instructions 7.2 us,
// without its MFMAs 6.1 us - the two do NOT overlap: the texture path takes one 1-KiB DMA instruction per ~10.6 ns and CU, all four waves issue
// their eight right behind the barrier and sit in the issue queue ~0.3 us per stage with the MFMA pipes drained.  Four stage buffers: the
// quarters of stage s + 3 go into the buffer of stage s - 1 while stage s multiplies.
template <int BM, int BN, int ROWB, bool CHAIN = false, bool SPREAD = false>
__device__ __forceinline__ void conv_dmap_body(const ConvK* pk, int nmem) {
  static_assert(!(CHAIN && SPREAD), "conv_dmap: one issue form at a time");
  typedef bf16_t T;
  const ConvK& p = pk[0];                               // geometry (the same for every member of a chain)
  // a stage = 64 channels, 4 k-steps of 16.  ROWB = 128: one LDS image [rows][128 B], every DMA row a full line;
  // ROWB = 64: two sub-images [2][rows][64 B] (32 channels each)
  constexpr int NBUF = SPREAD ? 4 : RUA_DMAP_NBUF, KS = 4;
  constexpr int NSUB = 128 / ROWB, SPR = ROWB / 16, RPI = 1024 / ROWB;      // sub-images, 16-B slots per row, rows per DMA instruction
  constexpr int SW = (ROWB == 64) ? 2 : 1;                                  // swizzle: slot = piece ^ ((row >> SW) & (SPR - 1))
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int AI = BM / (4 * RPI), BI = BN / (4 * RPI);                   // DMA instructions per wave per sub-image
  constexpr int PER_STAGE = NSUB * (AI + BI);
  constexpr int WN = 2, WM = 2;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int CSTR = BN + 4;
  constexpr unsigned OOB = 0x80000000u;             // stays out of range after the per-stage chunk offset is added
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sC = reinterpret_cast<float*>(smem);

  RUA_TS(0);
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int vid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int bn_i = vid % p.nbn;
  const int bm_i = (vid / p.nbn) % p.nbm;
  const int ks_i = vid / (p.nbn * p.nbm);
  const long long m0 = (long long)bm_i * BM;
  const int n0 = bn_i * BN;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int HW = p.H * p.W;

  // LDS image: [row][8 slots of 16 B]; slot = piece ^ ((row >> 1) & 7) makes the ds_read_b128 fragment reads
  // conflict-free (the 16-lane groups of a read see 8 even and 8 odd rows with 8 distinct slots each); the permutation
  // is applied to the per-lane SOURCE piece within the row's own 128-byte line, so every DMA row is one full line
  const int lrow = lane / SPR, lslot = lane % SPR;
  int an[AI], ah[AI], aw[AI], aqv[AI];
  bool av[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int row = (wid * AI + i) * RPI + lrow;
    const long long m = m0 + row;
    av[i] = m < p.M;
    const int mm = av[i] ? (int)m : 0;
    const int n = mm / HW, rem = mm - n * HW, h = rem / p.W;
    an[i] = n; ah[i] = h * p.stride; aw[i] = (rem - h * p.W) * p.stride;
    aqv[i] = (lslot ^ ((row >> SW) & (SPR - 1))) * 8;
  }
  int brow[BI], bqv[BI];
  bool bv[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int row = (wid * BI + j) * RPI + lrow;
    brow[j] = row; bv[j] = (n0 + row) < p.Cout;
    bqv[j] = (lslot ^ ((row >> SW) & (SPR - 1))) * 8;
  }

  // iteration state: (segment, tap, chunk) scalars + per-tap byte offsets of this lane's DMA sources
  int u_seg = 0, u_tap = 0, u_chunk = 0;
  int s_taps = 1, s_nchunk = 1, s_C = 64, s_Ws = 1, s_dil = 1;      // s_nchunk: 64-channel stages per tap
  unsigned sHL = 0, sWL = 0;
  int abase[AI];
  unsigned atap[AI], btap[BI];
  __amdgpu_buffer_rsrc_t rx = make_rsrc(p.seg[0].x, p.seg[0].xbytes), rw = make_rsrc(p.seg[0].w, p.seg[0].wbytes);
  int im = 0;                                           // CHAIN: the member the DMA cursor is in
  auto enter_segment = [&]() {
    const SegK sg = pk[im].seg[u_seg];
    rx = make_rsrc(sg.x, sg.xbytes); rw = make_rsrc(sg.w, sg.wbytes);
    s_taps = sg.taps; s_nchunk = sg.nchunk >> 1; s_C = sg.C; s_Ws = sg.Ws; s_dil = sg.dil;
    sHL = (unsigned)(sg.Hs << sg.up); sWL = (unsigned)(sg.Ws << sg.up);
#pragma unroll
    for (int i = 0; i < AI; ++i)
      abase[i] = ((an[i] * sg.Hs + (ah[i] >> sg.up)) * sg.Ws + (aw[i] >> sg.up)) * sg.C + aqv[i];
  };
  auto enter_tap = [&]() {
    int dh = 0, dw = 0;
    if (s_taps == 9) {
      const int t3 = (u_tap >= 6) ? 2 : (u_tap >= 3) ? 1 : 0;
      dh = (t3 - 1) * s_dil; dw = (u_tap - 3 * t3 - 1) * s_dil;
    }
    const int ex = (dh * s_Ws + dw) * s_C;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      bool ok = av[i] && (unsigned)(ah[i] + dh) < sHL && (unsigned)(aw[i] + dw) < sWL;
      atap[i] = ok ? (unsigned)((abase[i] + ex) * 2) : OOB;
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      btap[j] = bv[j] ? (unsigned)(((u_tap * p.Cout + n0 + brow[j]) * s_C + bqv[j]) * 2) : OOB;
    }
  };
  int st_left = 0;                                      // real stages of this block not yet issued
  // DMA the next stage of the K range into `buf` and step the iteration state; past the end of the range the
  // instructions still issue (out-of-range source => zeros) so that the vmcnt arithmetic stays uniform
  // (the explicit (unsigned) casts on the offsets are load-bearing: without them hipcc 7.2 silently drops the HOST stub
  //  of this kernel template - the implicit unsigned->int conversion of a template-dependent array element in a builtin
  //  argument fails substitution on the host pass only)
  // part < 0: the whole stage; part 0..3 (SPREAD): that quarter of its DMA instructions, the iteration state steps behind the last one
  auto issue_next = [&](int buf, int part = -1) {
    unsigned char* sA = smem + buf * STAGE;
    unsigned char* sB = sA + A_BYTES;
    const bool live = st_left > 0;
#pragma unroll
    for (int u = 0; u < NSUB; ++u) {
      const unsigned co = (unsigned)(u_chunk * 128 + u * ROWB);            // 64 channels * 2 bytes per stage
#pragma unroll
      for (int i = 0; i < AI; ++i)
        if (part < 0 || ((u * (AI + BI) + i) * 4) / PER_STAGE == part)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sA + (u * BM + (wid * AI + i) * RPI) * ROWB), 16,
                                                   (unsigned)(live ? atap[i] + co : OOB), 0, 0, 0);
#pragma unroll
      for (int j = 0; j < BI; ++j)
        if (part < 0 || ((u * (AI + BI) + AI + j) * 4) / PER_STAGE == part)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_p)(sB + (u * BN + (wid * BI + j) * RPI) * ROWB), 16,
                                                   (unsigned)(live ? btap[j] + co : OOB), 0, 0, 0);
    }
    if (part >= 0 && part < 3) return;
    if (live && --st_left > 0) {
      u_chunk += 1;
      if (u_chunk >= s_nchunk) {
        u_chunk = 0;
        if (++u_tap == s_taps) {
          u_tap = 0; ++u_seg;
          if (CHAIN && u_seg == pk[im].nseg) { u_seg = 0; ++im; }
          enter_segment();
        }
        enter_tap();
      }
    }
  };

  const int wm = wid / WN, wn = wid % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int xs = (lr >> SW) & (SPR - 1);                          // swizzle term of this lane's fragment rows (tile offsets are multiples of 32)
  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  const unsigned fa_off = (wm * (BM / WM) + lr) * ROWB, fb_off = A_BYTES + (wn * (BN / WN) + lr) * ROWB;
  auto load_frags = [&](int buf, int kk, bf16x8* fa, bf16x8* fb) {
    const unsigned char* sS = smem + buf * STAGE;
    const int u = (ROWB == 64) ? (kk >> 1) : 0;
    const int piece = (ROWB == 64) ? ((kk & 1) * 2 + lh) : (kk * 2 + lh);
    const int slot = (piece ^ xs) * 16;
#pragma unroll
    for (int a = 0; a < TM; ++a) fa[a] = *reinterpret_cast<const bf16x8*>(sS + fa_off + (u * BM + a * 32) * ROWB + slot);
#pragma unroll
    for (int b = 0; b < TN; ++b) fb[b] = *reinterpret_cast<const bf16x8*>(sS + fb_off + (u * BN + b * 32) * ROWB + slot);
  };

  int nstages_all = p.nunits / 2;
  if (CHAIN)
    for (int m = 1; m < nmem; ++m) nstages_all += pk[m].nunits / 2;
  const int st_begin = CHAIN ? 0 : ks_i * p.stages_per_split;
  int nstages = CHAIN ? nstages_all : st_begin + p.stages_per_split;
  if (nstages > nstages_all) nstages = nstages_all;
  const int nst = nstages - st_begin;
  if (!CHAIN) {
    const int unit = st_begin * 2;
    int sgi = 0;
    while (sgi + 1 < p.nseg && unit >= p.seg[sgi + 1].ubegin) ++sgi;
    const int loc = unit - p.seg[sgi].ubegin;
    u_seg = sgi; u_tap = loc / p.seg[sgi].nchunk; u_chunk = (loc - u_tap * p.seg[sgi].nchunk) >> 1;
  }
  st_left = nst;
  enter_segment(); enter_tap();
  static_assert(!SPREAD || PER_STAGE % 4 == 0, "SPREAD: a stage's DMA instructions split into four equal parts");
#pragma unroll
  for (int b = 0; b < NBUF - 1; ++b) issue_next(b);
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NBUF - 2) * PER_STAGE) : "memory");
  __builtin_amdgcn_s_barrier();
  if (!SPREAD) issue_next(NBUF - 1);
  bf16x8 fa[2][TM], fb[2][TN];
  load_frags(0, 0, fa[0], fb[0]);
  int buf = 0;
  int cm = 0, c_left = p.nunits / 2;                    // CHAIN: the member the MFMA cursor is in, its stages left
  RUA_TS(1);
  for (int st = 0; st < nst; ++st) {
    int nxt = buf + 1; if (nxt == NBUF) nxt = 0;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int cur = kk & 1;
      if (kk < KS - 1) {
        load_frags(buf, kk + 1, fa[cur ^ 1], fb[cur ^ 1]);
      } else if (SPREAD) {                             // in flight here: stages s + 1, s + 2 and three quarters of s + 3
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)" :: "n"(2 * PER_STAGE - PER_STAGE / 4) : "memory");
        __builtin_amdgcn_s_barrier();
        load_frags(nxt, 0, fa[cur ^ 1], fb[cur ^ 1]);
      } else {
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)" :: "n"((NBUF - 2) * PER_STAGE) : "memory");
        __builtin_amdgcn_s_barrier();
        issue_next(buf);
        load_frags(nxt, 0, fa[cur ^ 1], fb[cur ^ 1]);
      }
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][a], fb[cur][b], acc[a][b], 0, 0, 0);
      if (SPREAD) issue_next(buf == 0 ? NBUF - 1 : buf - 1, kk);      // a quarter of stage s + 3 into the buffer stage s - 1 left
    }
    buf = nxt;
    if (CHAIN) {
      if (--c_left == 0) {                              // the member's last stage: its tile leaves, the ring keeps running
        const ConvK& q = pk[cm];
        float* sCh = reinterpret_cast<float*>(smem + NBUF * STAGE);
        float carry[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) carry[j] = 0.f;
#pragma unroll
        for (int h = 0; h < WM; ++h) {
          if (wm == h) {
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
              for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                  sCh[(a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh) * CSTR + wn * (BN / WN) + b * 32 + lr] = acc[a][b][i];
          }
          __syncthreads();
          conv_epilogue_pick<T, BM / WM, BN>(q, m0 + h * (BM / WM), n0, bm_i, sCh, CSTR, sCh + (BM / WM) * CSTR, carry, h == WM - 1);
          __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
        if (++cm < nmem) c_left = pk[cm].nunits / 2;
      }
    }
  }
  RUA_TS(2);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (CHAIN) return;

  if (p.ksplit > 1) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const long long m = m0 + wm * (BM / WM) + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
          const int c = n0 + wn * (BN / WN) + b * 32 + lr;
          if (m < p.M && c < p.Cout) p.ws[((size_t)ks_i * p.M + m) * p.Cout + c] = acc[a][b][i];
        }
    if (p.cnt == nullptr) return;                      // a separate conv_splitk_finish launch sums the slabs
    // In-launch reduction: the slice that arrives LAST at this tile's ticket counter sums the slabs (fixed order) and runs
    // the epilogue.  Publication: every wave's slab stores complete (vmcnt) -> block barrier -> one agent-scope release +
    // relaxed ticket; the last arriver takes one agent-scope acquire (the other XCDs' L2s are not coherent with ours)
    // before any slab load.  The ticket word lives in the kernel's one dynamic LDS array (a second __shared__ object
    // beside LDS-DMA buffers makes hipcc drain vmcnt(0) before every ds_read of the K loop).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* flag = reinterpret_cast<int*>(smem);
    int* cnt = p.cnt + (bm_i * p.nbn + bn_i);
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      *flag = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (*flag != p.ksplit - 1) return;
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    }
    __syncthreads();
    conv_epilogue<T, BM, BN, true>(p, m0, n0, bm_i, p.ws + (size_t)m0 * p.Cout + n0, p.Cout, sC + BM * CSTR);
    return;
  }
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = wm * (BM / WM) + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
        const int col = wn * (BN / WN) + b * 32 + lr;
        sC[row * CSTR + col] = acc[a][b][i];
      }
  __syncthreads();
  RUA_TS(3);
  conv_epilogue_pick<T, BM, BN>(p, m0, n0, bm_i, sC, CSTR, sC + BM * CSTR);
  RUA_TS(6);
}



template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap(const ConvK p) { conv_dmap_body<BM, BN, ROWB>(&p, 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap_g(const ConvKG g) { conv_dmap_body<BM, BN, ROWB>(&g.k[blockIdx.y], 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap_s(const ConvK p) { conv_dmap_body<BM, BN, ROWB, false, true>(&p, 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap_gs(const ConvKG g) { conv_dmap_body<BM, BN, ROWB, false, true>(&g.k[blockIdx.y], 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap_chain(const ConvKG g, int nmem) { conv_dmap_body<BM, BN, ROWB, true>(g.k, nmem); }

template <int BM, int BN, int NBUF = RUA_DMAP_NBUF> static constexpr int conv_dmap_smem() {
  constexpr int STAGE = 2 * (BM + BN) * 64;
  constexpr int EPI = BM * (BN + 4) * 4 + 4 * (BN / 8) * 16 * 4;
  return ((NBUF * STAGE > EPI ? NBUF * STAGE : EPI) + 15) / 16 * 16;
}

// conv_dmap_chain: the ring stays live during a member's epilogue, whose half tile and reduction scratch sit behind it
template <int BM, int BN> static constexpr int conv_dmap_chain_smem() {
  return (RUA_DMAP_NBUF * 2 * (BM + BN) * 64 + (BM / 2) * (BN + 4) * 4 + 4 * (BN / 8) * 16 * 4 + 15) / 16 * 16;
}

template <int BM, int BN> static constexpr int conv_dma_base() {
  constexpr int STAGE = 2 * (BM + BN) * 64;
  constexpr int EPI = BM * (BN + 4) * 4 + 4 * (BN / 8) * 16 * 4;
  return ((3 * STAGE + 1024 > EPI ? 3 * STAGE + 1024 : EPI) + 15) / 16 * 16;
}

// =========================================================================================
// conv_halo<C>: 3x3 dilated convolution with C = Cout in {32} (the top level), bf16.  The implicit-GEMM kernels re-stage the
// A tile from L2 for every tap (9 x the bytes; measured: they run at the L2 gather rate, not at MFMA or HBM rate).  Here a
// block loads the input ONCE with its halo and serves all nine taps from LDS.  Dilation d is handled by lattice
// decomposition: the pixels with y = ry (mod d), x = rx (mod d) form a dense grid on which the dilated conv IS a plain
// 3x3 conv, so a tile is a TH x TW rectangle of ONE residue class, its halo the (TH+2) x (TW+2) lattice points around it
// (64-byte pixel vectors gathered at stride d; a block takes NS such sub-tiles so that small lattices - d = 15, 31 -
// still fill 8..12 MFMA row tiles).  No barrier inside the K loop: one DMA phase, one barrier, 9 taps x C/16 k-steps of
// MFMAs whose A fragments are LDS reads at (row + tap offset) and whose B fragments (all 9 taps) live in registers.
// Overlap of load / compute / epilogue comes from 2-3 co-resident blocks per CU.
// HaloK: common.h
__device__ __forceinline__ int fdiv(int x, unsigned m, int dv) { return dv == 1 ? x : (int)__umulhi((unsigned)x, m); }

template <int C, int MAXMT>                           // MAXMT: MFMA row tiles per wave (rows <= MAXMT * 128)
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(4, MAXMT == 2 ? 6 : 4)))     // = blocks per CU the LDS footprint allows
void conv_halo(const HaloK q) {
  typedef bf16_t T;
  static_assert(C == 32, "conv_halo: C = Cout = 32");
  constexpr int ROWB = C * 2, SPR = ROWB / 16;        // bytes per LDS pixel row, 16-B slots per row
  constexpr int SW = 2;                               // swizzle: slot = piece ^ ((row >> SW) & (SPR - 1)) (conflict-free b128 reads)
  constexpr int CSTR = 32 + 4;                        // a block computes all 32 output channels
  constexpr int KST = C / 16;                         // k-steps per tap
  const ConvK& p = q.c;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sC = reinterpret_cast<float*>(smem);         // aliases the halo images after the MFMA phase
  // fixed carve-up behind the halo / epilogue area (sizes from the launcher): row->pixel table, row->LDS-row table, sub-tile records
  const int halo_b = ((q.NS * q.HP * ROWB + 1023) / 1024) * 1024;
  const int area = 128 * CSTR * 4 > halo_b ? 128 * CSTR * 4 : halo_b;       // the fp32 tile is transposed 128 rows at a time
  int* rowtab = reinterpret_cast<int*>(smem + area);
  int* subrec = rowtab + q.rows;                      // [NS][4]: n, y0, x0, valid   (halo origin in image coordinates)
  float* sred = reinterpret_cast<float*>(subrec + 4 * 12);

  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int vid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int H = p.H, W = p.W, d = q.d;

  if (tid < q.NS) {
    int t = vid * q.NS + tid;
    const int ok = t < q.total_sub;
    if (!ok) t = 0;
    const int rx = t % d; t /= d;
    const int tx = t % q.ntx; t /= q.ntx;
    const int ry = t % d; t /= d;
    const int ty = t % q.nty; const int n = t / q.nty;
    subrec[tid * 4 + 0] = n;
    subrec[tid * 4 + 1] = ry + (ty * q.TH - 1) * d;
    subrec[tid * 4 + 2] = rx + (tx * q.TW - 1) * d;
    subrec[tid * 4 + 3] = ok;
  }
  __syncthreads();

  // ---- tables: tile row m -> output pixel (or -1) and -> LDS row of its tap (0,0) ---------------------------------
  for (int m = tid; m < q.rows; m += 256) {
    const int s_ = fdiv(m, q.mPT, q.PT), qq = m - s_ * q.PT;
    const int i = fdiv(qq, q.mTW, q.TW), j = qq - i * q.TW;
    const int y = subrec[s_ * 4 + 1] + (i + 1) * d, x = subrec[s_ * 4 + 2] + (j + 1) * d;
    const bool ok = subrec[s_ * 4 + 3] && i < q.TH && y < H && x < W;
    rowtab[m] = ok ? (subrec[s_ * 4 + 0] * H + y) * W + x : -1;
  }

  // ---- weights: every wave keeps the B fragments of all 9 taps in registers -------------------------------------------
  const int lr = lane & 31, lh = lane >> 5;
  // C = 32: B fragments of ONE kernel row (3 taps) live in registers; the fragment of tap t + 3 is loaded into the
  // registers of tap t right after the MFMAs that consumed it (72 -> 24 VGPRs: one to two more blocks per CU)
  bf16x8 fb[3][KST];
  const unsigned char* wlane = p.seg[0].w + ((size_t)lr * C + lh * 8) * 2;      // this lane's (cout row, k half) in tap 0
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int ks = 0; ks < KST; ++ks)
      fb[t][ks] = *reinterpret_cast<const bf16x8*>(wlane + ((size_t)t * C * C + ks * 16) * 2);

  // ---- halo images: HBM/L2 -> LDS, one pass (lane-linear destination, swizzle on the source piece) ------------------
  {
    const __amdgpu_buffer_rsrc_t rx_ = make_rsrc(p.seg[0].x, p.seg[0].xbytes);
    const int hrows = q.NS * q.HP;
    const int ninst = (hrows * SPR + 63) / 64;                 // wave-instructions in total (64 pieces = 16 rows each)
    for (int it = wid; it < ninst; it += 4) {
      const int g = it * 64 + lane;
      const int row = g / SPR, slot = g % SPR;
      const int s_ = fdiv(row, q.mHP, q.HP), hp = row - s_ * q.HP;
      const int hi = fdiv(hp, q.mHPW, q.HPW), hj = hp - hi * q.HPW;
      unsigned off = 0x80000000u;
      if (row < hrows) {
        const int y = subrec[s_ * 4 + 1] + hi * d, x = subrec[s_ * 4 + 2] + hj * d;
        if (subrec[s_ * 4 + 3] && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
          off = (unsigned)((((subrec[s_ * 4 + 0] * H + y) * W + x) * C + ((slot ^ ((row >> SW) & (SPR - 1))) * 8)) * 2);
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx_, (lds_void_p)(smem + it * 1024), 16, off, 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- MFMA phase: this wave's row tiles wid, wid+4, wid+8 ------------------------------------------------------------
  const int mtb = q.rows >> 5;
  int r0[MAXMT];                                         // LDS row of tap (0,0) for this lane's pixel of each row tile
#pragma unroll
  for (int a = 0; a < MAXMT; ++a) {
    const int mt = wid + a * 4;
    const int m = (mt < mtb ? mt : 0) * 32 + lr;
    const int s_ = fdiv(m, q.mPT, q.PT), qq = m - s_ * q.PT;
    const int i = fdiv(qq, q.mTW, q.TW), j = qq - i * q.TW;
    r0[a] = s_ * q.HP + (i < q.TH ? i : 0) * q.HPW + j;
  }
  f32x16 acc[MAXMT];
#pragma unroll
  for (int a = 0; a < MAXMT; ++a)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int toff = (t / 3) * q.HPW + (t % 3);
#pragma unroll
    for (int ks = 0; ks < KST; ++ks) {
      bf16x8 fa[MAXMT];
#pragma unroll
      for (int a = 0; a < MAXMT; ++a) {
        const int row = r0[a] + toff;
        fa[a] = *reinterpret_cast<const bf16x8*>(smem + row * ROWB + (((ks * 2 + lh) ^ ((row >> SW) & (SPR - 1))) * 16));
      }
      const bf16x8 fbv = fb[t % 3][ks];
#pragma unroll
      for (int a = 0; a < MAXMT; ++a)          // unconditional (a branch around MFMAs makes hipcc shuttle the accumulators):
        acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fbv, acc[a], 0, 0, 0);     // a missing row tile computes garbage, never stored
      if (t < 6) fb[t % 3][ks] = *reinterpret_cast<const bf16x8*>(wlane + ((size_t)(t + 3) * C * C + ks * 16) * 2);
    }
  }
  // ---- epilogue, 128 rows (one row tile per wave) at a time: a small fp32 tile keeps LDS per block low (more blocks per CU) --
  float carry[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) carry[j] = 0.f;
#pragma unroll
  for (int a = 0; a < MAXMT; ++a) {
    __syncthreads();                                     // a == 0: every wave is done with the halo images; else: previous pass read
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = wid * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
      sC[row * CSTR + lr] = acc[a][i];
    }
    __syncthreads();
    // tile rows of pass a: row tile (wid + 4a) of wave wid sits at LDS rows wid*32.., i.e. tile row r <-> m = (a*4 + r/32)*32 + r%32
    conv_epilogue<T, 128, 32>(p, 0, 0, vid, sC, CSTR, sred, rowtab + a * 128, q.rows - a * 128, carry, a == MAXMT - 1);
  }
}

#define RUA_MAX_UNITS 1024
template <typename T, int BM, int BN> static constexpr int conv_smem() { return conv_smem_base<T, BM, BN>() + RUA_MAX_UNITS * 16; }

// split-K factor: only when the output grid cannot fill the chip and the K loop is long
static int pick_ksplit(long long tiles, int nstages, long long M, int Cout, size_t ws_bytes) {
  const long long slabs = (long long)(ws_bytes / ((size_t)M * Cout * sizeof(float)));     // one fp32 slab per K slice
  if (slabs < 2) return 1;
  if (tiles >= 256 || nstages < 8) return 1;
  long long want = (512 + tiles - 1) / tiles;
  long long cap = nstages / 4;
  if (want > cap) want = cap;
  if (want > 32) want = 32;
  if (want > slabs) want = slabs;
  return want < 2 ? 1 : (int)want;
}


static int pick_bn(const rua_conv_desc* d, long long M) {
  const int force = g_tune.conv_force_bn;          // experiments only
  if (force == 32 || force == 64 || force == 128) return (d->Cout <= 32) ? 32 : (force == 128 && d->Cout < 128) ? 64 : (force == 32 ? 64 : force);
  if (d->Cout <= 32) return 32;
  if (d->Cout <= 64) return 64;
  int units = 0;
  for (int s_ = 0; s_ < d->nseg; ++s_) units += d->seg[s_].taps * ((d->seg[s_].C + 31) / 32);
  if (d->Cout >= 256 && units >= 200) return 128;       // multi-branch 3x3 at the deep levels: A re-read dominates
  const long long nbm = (M + 127) / 128;
  if (nbm * ((d->Cout + 127) / 128) < 512) return 64;   // small maps: more, smaller tiles
  return 128;
}
// pixel-tile height: 256 only where the grid stays large (the two top levels) and the N tile is narrow
static int pick_bm(const rua_conv_desc* d, long long M, int bn) {
  const int force = g_tune.conv_force_bm;
  if (bn == 128) return 128;
  if (force == 128 || force == 256) return force;
  return (M >= 65536) ? 256 : 128;
}

static bool pick_dma(const rua_conv_desc* d, int bn) {
  const int use_dma = g_tune.conv_dma;    // 0 / 1: force (experiments)
  bool dma = d->dtype == RUA_BF16 && d->Cout >= 128 && !(bn == 128);
  if (use_dma == 0) dma = false;
  if (use_dma == 1 && d->dtype == RUA_BF16) dma = true;
  return dma;
}

// =========================================================================================
// conv_pw: the narrow 1x1 convolutions of the two top levels (Cout <= 32, K <= 96: combine / PSP / upsampling convs and their
// data gradients) are memory-bound, and on conv_igemm they streamed at ~2.8 TB/s (one 256-row tile per block: load ->
// LDS -> MFMA -> LDS -> epilogue, serial, 8-12 waves per CU).  Here every WAVE streams its own pixel range in 32-pixel
// tiles with no LDS and no barrier in the loop: the transposed product D^T[co][px] = W[co][k] * X^T[k][px] makes BOTH MFMA
// operands plain 16-byte loads (a-operand: weight rows, held in registers for the whole kernel; b-operand: lane = pixel,
// k-slice = 8 consecutive channels), the next tile's loads (input, aux, old output) are in flight while the current tile
// computes, and one 32-lane exchange per register pair turns the accumulator layout (lane = pixel, 4-channel groups
// interleaved between the wave halves) into 8-channel pieces for the shared epilogue semantics (bias, accumulate, residual /
// mask, ReLU, statistics) and 16-byte stores.  Statistics stay in registers over all tiles of a wave and leave through
// shuffles -> LDS -> one fp64 atomic per channel and block, like everywhere else.
// PwStep, PwK<KS>: common.h.  PwKG: the members of a group (rua_conv_fwd_group: the four branch convolutions of the top-level PSPPooling, the per-source data gradients of a
// concatenating 1x1 conv) as ONE grid (blockIdx.y = member, grids of unequal size) - each was a launch of 8 - 15 us, half of it ramp and drain
template <int KS> struct PwKG { PwK<KS> k[RUA_MAX_BRANCH]; };
static_assert(sizeof(PwKG<2>) <= 4096, "grouped launch: kernel arguments are limited to 4 KiB");

template <int KS, bool DENSE>
__device__ __forceinline__ void conv_pw_body(const PwK<KS>& q) {
  const ConvK& p = q.c;
  __shared__ float tab[3 * 32];                       // bias sum, mask scale, mask shift per output channel
  __shared__ float sred[4 * 64 * 33 + 4 * 64];        // statistics fold: [wave][value row][33] + [wave][64]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int pl = lane & 31, lh = lane >> 5;
  if (tid < 32) {
    float b = 0.f, ms = 1.f, mt = 0.f;
    if (tid < p.Cout) {
      if (p.bias) { b = p.bias[tid]; for (int r = 0; r < 3; ++r) if (p.bias_more[r]) b += p.bias_more[r][tid]; }
      if (p.aux_mode == 2) { if (p.mscale) ms = p.mscale[tid]; if (p.mshift) mt = p.mshift[tid]; }
    }
    tab[tid] = b; tab[32 + tid] = ms; tab[64 + tid] = mt;
  }
  __syncthreads();
  const int M = (int)p.M;
  const int gw = blockIdx.x * 4 + wid;
  const int k_begin = gw * q.px_per_wave;
  int k_end = k_begin + q.px_per_wave; if (k_end > M) k_end = M;

  // weight fragments: a-operand row = output channel pl, k-slice 8*lh of step ks
  bf16x8 wf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const PwStep& s = q.st[ks];
    const int kk = s.kofs + 8 * lh;
    const bool ok = pl < p.Cout && kk < s.C;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(s.w, s.wbytes);
    wf[ks] = __builtin_bit_cast(bf16x8, bufload16(rw, ok ? (unsigned)((pl * s.C + kk) * 2) : RUA_OOB));
  }
  const __amdgpu_buffer_rsrc_t raux = make_rsrc(p.aux ? p.aux : p.y, (unsigned)((size_t)M * p.Cout * 2));
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.y, (unsigned)((size_t)M * p.Cout * 2));
  const bool cok0 = 8 * lh < p.Cout, cok1 = 16 + 8 * lh < p.Cout;       // this lane's two 8-channel pieces exist

  struct Tile { uint4 x[KS], a[2], o[2]; };           // the loads of one 32-pixel tile: input k-steps, aux pieces, old-output pieces
  auto load_tile = [&](Tile& T, int t0) {
    const int m = t0 + pl;
    const bool in = m < k_end;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const PwStep& s = q.st[ks];
      const int kk = s.kofs + 8 * lh;
      int px = m;
      if constexpr (!DENSE) {                           // some segment is upsampled on read (power-of-two maps, checked by the launcher)
        const int w = m & (p.W - 1), h = (m >> q.wsh) & (p.H - 1), n = m >> (q.wsh + q.hsh);
        const int gen = (n * s.Hs + (h >> s.up)) * s.Ws + (w >> s.up);
        px = s.dense ? m : gen;
      }
      const __amdgpu_buffer_rsrc_t rx = make_rsrc(s.x, s.xbytes);
      T.x[ks] = bufload16(rx, (in && kk < s.C) ? (unsigned)((px * s.C + kk) * 2) : RUA_OOB);
    }
    const unsigned o0 = (unsigned)((m * p.Cout + 8 * lh) * 2), o1 = o0 + 32;
    T.a[0] = bufload16(raux, (in && cok0 && p.aux_mode != 0) ? o0 : RUA_OOB);
    T.a[1] = bufload16(raux, (in && cok1 && p.aux_mode != 0) ? o1 : RUA_OOB);
    T.o[0] = bufload16(ry, (in && cok0 && p.accumulate) ? o0 : RUA_OOB);
    T.o[1] = bufload16(ry, (in && cok1 && p.accumulate) ? o1 : RUA_OOB);
  };
  float s1[2][8], s2[2][8];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[g][j] = 0.f; s2[g][j] = 0.f; }

  auto process = [&](const Tile& T, int t0) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks], __builtin_bit_cast(bf16x8, T.x[ks]), acc, 0, 0, 0);
    // acc[r]: channel (r & 3) + 8 * (r >> 2) + 4 * lh of pixel pl.  v_permlane32_swap(A, B) exchanges the upper half of A with
    // the lower half of B: with A = group 2g and B = group 2g+1 every lane ends up with channels 16g + 8*lh .. +7 of its pixel
    // (lower half: own group 2g + the upper half's group 2g; upper half: the lower half's group 2g+1 + own group 2g+1).
    float v[2][8];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // (inline asm: the builtin form of this exchange was miscompiled here - every pair collapsed onto acc[0].  The asm
        // reads MFMA results directly, a hazard hipcc does not track for inline asm: the s_nops before the first exchange
        // cover the 19 wait states an 8/16-pass MFMA needs before a VALU read of its destination.)
        float a = acc[(2 * g) * 4 + j], b = acc[(2 * g + 1) * 4 + j];
        if (g == 0 && j == 0) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
        else asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
        v[g][j] = a;
        v[g][4 + j] = b;
      }
    const int m = t0 + pl;
    if (m < k_end) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int co = 16 * g + 8 * lh;
        if (co < p.Cout) {
          float a8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[g][j] += tab[co + j];
          if (p.accumulate) {
            float o8[8];
            ET<bf16_t>::unpack(T.o[g], o8);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[g][j] += o8[j];
          }
          if (p.aux_mode != 0) ET<bf16_t>::unpack(T.a[g], a8);
          if (p.aux_mode == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[g][j] += a8[j];
          } else if (p.aux_mode == 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[g][j] = (fmaf(tab[32 + co + j], a8[j], tab[64 + co + j]) > 0.f) ? v[g][j] : 0.f;
          }
          if (p.out_relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[g][j] = fmaxf(v[g][j], 0.f);
          }
          if (p.stats_mode == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { s1[g][j] += v[g][j]; s2[g][j] = fmaf(v[g][j], v[g][j], s2[g][j]); }
          } else if (p.stats_mode == 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { s1[g][j] += v[g][j]; s2[g][j] = fmaf(v[g][j], a8[j], s2[g][j]); }
          }
          stg16(p.y + ((size_t)m * p.Cout + co) * 2, ET<bf16_t>::pack(v[g]));
        }
      }
    }
  };
  // ping-pong: the next tile's loads are in flight while this one computes (a tile past the range loads zeros and stores
  // nothing).  Three tiles in flight were measured and are no faster (18.2 vs 17.2 us at 256x256x32->32): the loop is bound by
  // its own VALU work (address arithmetic, the half-wave exchange, unpack / pack), not by bytes in flight.
  Tile T0, T1;
  load_tile(T0, k_begin);
  for (int t0 = k_begin; t0 < k_end; t0 += 64) {
    load_tile(T1, t0 + 32); process(T0, t0);
    load_tile(T0, t0 + 64); process(T1, t0 + 32);
  }
  if (p.stats_mode != 0) {
    // fold the 32 pixel lanes of each half through LDS (every lane writes its 32 partial sums as a column, thread (wave, row)
    // adds the row; as butterfly shuffles this was 320 ds_bpermute per wave, ~2 us at the end of the launch), then the four waves
    float* sw = sred + 4 * 64 * 33;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = (lh * 16 + g * 8 + j) * 2;
        sred[(wid * 64 + row) * 33 + pl] = s1[g][j];
        sred[(wid * 64 + row + 1) * 33 + pl] = s2[g][j];
      }
    __syncthreads();
    {
      const float* rowp = sred + tid * 33;
      float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
      for (int k = 0; k < 32; k += 4) { t0 += rowp[k]; t1 += rowp[k + 1]; t2 += rowp[k + 2]; t3 += rowp[k + 3]; }
      sw[tid] = (t0 + t1) + (t2 + t3);
    }
    __syncthreads();
    if (tid < 64) {
      const int c = tid >> 1, k = tid & 1;
      const int row = (((c >> 3) & 1) * 16 + (c >> 4) * 8 + (c & 7)) * 2 + k;
      const float t = sw[row] + sw[64 + row] + sw[128 + row] + sw[192 + row];
      if (c < p.Cout) unsafeAtomicAdd(&p.stats[(size_t)(blockIdx.x & (p.stats_R - 1)) * 2 * p.Cout + k * p.Cout + c], (double)t);
    }
  }
}
template <int KS, bool DENSE>
__global__ __launch_bounds__(256, (KS <= 4 ? 3 : 2)) void conv_pw(const PwK<KS> q) { conv_pw_body<KS, DENSE>(q); }      // >= 3 waves per SIMD for K <= 64
template <int KS, bool DENSE>
__global__ __launch_bounds__(256, (KS <= 4 ? 3 : 2)) void conv_pw_g(const PwKG<KS> g) {
  const PwK<KS>& q = g.k[blockIdx.y];
  if ((int)blockIdx.x >= q.nblk) return;
  conv_pw_body<KS, DENSE>(q);
}

static int pw_steps(const rua_conv_desc* d) {             // 16-channel k-steps of all segments; 0: not a conv_pw shape
  int n = 0;
  for (int s = 0; s < d->nseg; ++s) {
    const rua_conv_seg& g = d->seg[s];
    if (g.taps != 1 || g.C % 8 != 0 || g.C > 64) return 0;
    n += (g.C + 15) / 16;
  }
  return n;
}
static bool pick_pw(const rua_conv_desc* d) {
  const int on = g_tune.conv_pw;
  const long long minm = g_tune.conv_pw_minm;
  auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
  if (!on || d->dtype != RUA_BF16 || d->Cout > 32 || d->stride != 1 || d->out_stride != 1 || d->OH != d->H || d->OW != d->W) return false;
  const long long M = (long long)d->N * d->H * d->W;
  if (M < minm || M * d->Cout * 2 >= (1ll << 31)) return false;
  const int ks = pw_steps(d);
  if (ks < 1 || ks > 6) return false;
  for (int s = 0; s < d->nseg; ++s) {
    const rua_conv_seg& g = d->seg[s];
    const bool dense = g.up_shift == 0 && g.Hs == d->H && g.Ws == d->W;
    if (!dense && !(pow2(d->H) && pow2(d->W))) return false;
  }
  return true;
}
template <int KS> static void plan_conv_pw(PwK<KS>& q, const rua_conv_desc* d, ConvLaunch* L) {       // q: the member of L->a for KS, its ConvK filled
  const ConvK& k = q.c;
  int n = 0;
  for (int s = 0; s < d->nseg; ++s) {
    const SegK& g = k.seg[s];
    for (int k0 = 0; k0 < g.C; k0 += 16) {
      PwStep& t = q.st[n++];
      t.x = g.x; t.w = g.w; t.xbytes = g.xbytes; t.wbytes = g.wbytes; t.C = g.C; t.kofs = k0; t.up = g.up; t.Hs = g.Hs; t.Ws = g.Ws;
      t.dense = (g.up == 0 && g.Hs == k.H && g.Ws == k.W) ? 1 : 0;
    }
  }
  for (; n < KS; ++n) { PwStep& t = q.st[n]; t = q.st[0]; t.C = 0; t.kofs = 0; }       // padding steps: every load out of range
  int wsh = 0, hsh = 0; while ((1 << wsh) < k.W) ++wsh; while ((1 << hsh) < k.H) ++hsh;
  q.wsh = wsh; q.hsh = hsh;
  const int target = g_tune.conv_pw_blocks > 0 ? g_tune.conv_pw_blocks : 8 * rua_cu_count();      // 2048 on MI355X
  long long waves = (long long)target * 4;
  if (waves > k.M / 128) waves = k.M / 128;                // >= 4 tiles per wave
  if (waves < 4) waves = 4;
  long long ppw = (k.M + waves - 1) / waves;
  ppw = (ppw + 31) / 32 * 32;
  q.px_per_wave = (int)ppw;
  const unsigned grid = (unsigned)((k.M + ppw * 4 - 1) / (ppw * 4));
  q.nblk = (int)grid;
  bool all_dense = true;
  for (int i = 0; i < KS; ++i) all_dense = all_dense && (q.st[i].dense || q.st[i].C == 0);
  L->kernel = (KS == 2 ? CK_PW2 : KS == 4 ? CK_PW4 : CK_PW6) + (all_dense ? 1 : 0);
  L->gx = grid; L->smem = 0;
}

// ---- conv_halo launcher -------------------------------------------------------------------------------------------------
static bool pick_halo(const rua_conv_desc* d) {
  const int mode = g_tune.conv_halo;      // 0: off (experiments)
  if (!mode || d->dtype != RUA_BF16 || d->nseg != 1) return false;
  const rua_conv_seg& g = d->seg[0];
  return g.taps == 9 && g.up_shift == 0 && g.C == 32 && d->Cout == g.C && d->stride == 1 && d->out_stride == 1 &&
         d->OH == d->H && d->OW == d->W && g.Hs == d->H && g.Ws == d->W && d->H >= 16 && d->W >= 16 &&
         (long long)d->N * d->H * d->W >= 65536;
}
static unsigned magic_div(int dv) { return dv <= 1 ? 0u : (unsigned)(((1ull << 32) + dv - 1) / dv); }

// lattice tile TH x TW (slots padded to a multiple of 32) and sub-tiles per block for an H x W map at dilation d:
// minimise padded slots (MFMA waste) with a penalty for halo bytes; at most 384 rows and 40 KiB of halo images per block
static void halo_tiling(int H, int W, int d, int rowb, int* TH_, int* TW_, int* NS_) {
  const int ny = (H + d - 1) / d, nx = (W + d - 1) / d;
  const int lim = 41 * 1024;                           // halo images per block
  double best = 1e30;
  int bth = 1, btw = 1;
  for (int th = 1; th <= ny && th <= 32; ++th)
    for (int tw = 1; tw <= nx && tw <= 32; ++tw) {
      const int pt = (th * tw + 31) / 32 * 32;
      if (pt > 384 || (th + 2) * (tw + 2) * rowb > lim) continue;
      const double slots = (double)((ny + th - 1) / th) * ((nx + tw - 1) / tw) * pt;
      const double halo = (double)(th + 2) * (tw + 2) / (th * tw);
      const double cost = slots * (1.0 + 0.35 * (halo - 1.0));
      if (cost < best) { best = cost; bth = th; btw = tw; }
    }
  const int pt = (bth * btw + 31) / 32 * 32;
  int ns = 384 / pt;
  while (ns > 1 && ns * (bth + 2) * (btw + 2) * rowb > lim) --ns;
  if (ns > 12) ns = 12;
  *TH_ = bth; *TW_ = btw; *NS_ = ns < 1 ? 1 : ns;
}

static int plan_conv_halo(int dil, ConvLaunch* L) {
  HaloK& q = L->a.h;
  const ConvK& k = q.c;
  q.d = dil;
  const int Cc = k.seg[0].C, rowb = Cc * 2;
  halo_tiling(k.H, k.W, dil, rowb, &q.TH, &q.TW, &q.NS);
  q.PT = (q.TH * q.TW + 31) / 32 * 32;
  q.HPW = q.TW + 2; q.HP = (q.TH + 2) * (q.TW + 2);
  const int ny = (k.H + dil - 1) / dil, nx = (k.W + dil - 1) / dil;
  q.nty = (ny + q.TH - 1) / q.TH; q.ntx = (nx + q.TW - 1) / q.TW;
  const long long total = (long long)k.N * dil * dil * q.nty * q.ntx;
  RUA_CHECK_ARG(total < (1ll << 30), "conv_halo: too many lattice tiles");
  q.total_sub = (int)total;
  q.rows = q.NS * q.PT;
  q.mHP = magic_div(q.HP); q.mHPW = magic_div(q.HPW); q.mPT = magic_div(q.PT); q.mTW = magic_div(q.TW);
  const int halo_bytes = (q.NS * q.HP * rowb + 1023) / 1024 * 1024;
  const int epi_bytes = 128 * 36 * 4;
  const int area = epi_bytes > halo_bytes ? epi_bytes : halo_bytes;
  L->smem = area + q.rows * 4 + 4 * 12 * 4 + 4 * 4 * 16 * 4;
  L->gx = (unsigned)((total + q.NS - 1) / q.NS);
  L->kernel = q.rows <= 256 ? CK_HALO2 : CK_HALO3;
  return RUA_OK;
}

// =========================================================================================
// conv_img<W, KS> (round 4): the 3x3 convolutions (and data gradients) of the two deepest levels - 8 x 8 x 1024 and 16 x 16 x 512 maps, dilation 1 (model2.py:109-112
// and the decoder's mirror).  On conv_dmap they are 128 x 128 tiles with 8 / 4 K slices: every block gathers its input pixels nine times (once per tap) through LDS-DMA,
// the weights are re-read by every pixel tile, the K slices leave 16.8 MB of fp32 slabs that a finisher launch reads again - 21 + 7 us for 9.66 GFLOP.  Here a block owns ONE
// WHOLE IMAGE x 32 output channels: the image's input (64 pixels x 1024 channels, or 256 pixels x 256 channels = half the channels: KS = 2) is RESIDENT in LDS (128 KB, once,
// by LDS-DMA; 16-byte chunks XOR-swizzled with the pixel index for the 2-KiB / 512-B pixel rows), a tap is a shifted read of it (border lanes read a zero slot), and the
// weights - the only stream - go from L2 straight into registers (a B fragment is 16 bytes per lane of w[tap][co][ci .. ci + 8): no LDS staging, four k-steps prefetched).
// MEASURED AND NOT THE DEFAULT (tuning key conv_img): 28 - 29 us per convolution at both levels, what conv_dmap_s + its finisher take - 45 us with four fragments in flight per
// wave, no better with 24 than with 16; a fragment gathered as 32 x 32-byte row pieces costs the texture path 32 line look-ups per KiB (the ablations below).
// Ablations at 8 x 8 x 1024 (tools/bench_conv_levels.py on builds without the weight loads / the fragment reads - compile-time switches that last existed at commit 841d62a; event pair included): 32.6 us; without the weight loads 22.6; without the fragment reads of the
// image no faster - the K loop of ONE wave per SIMD (two dependent accumulators, ~100 cycles per k-step), the cold 128 KB image and the epilogue are ~17 us before any weight
// arrives, the gathered weight fragments add ~10.  Starting each image's K quarter at another point (rot below) changed nothing: not a matter of distinct HBM streams.
// Four waves split the K range (nine taps x the block's channels) in quarters and meet once through LDS.  KS = 1: the tile leaves through the shared epilogue (bias, residual /
// mask, statistics) - no K slices, no slabs, no finisher; KS = 2: two slabs, the usual finisher.  Blocks that share weights (the eight images of an output-channel tile) sit
// on one XCD.
template <int W, int KS, int D>
__global__ __launch_bounds__(256) void conv_img(const ConvK p) {
  typedef bf16_t T;
  constexpr int HW = W * W, NT = HW / 32, CSTR = 36;
  constexpr int WSH = (W == 8) ? 3 : 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sZ = smem;                             // 1 KiB of zeros (what a tap reads across an image border)
  unsigned char* sX = smem + 1024;                      // [HW pixels][CS channels] bf16, chunk-swizzled
  const SegK& sg = p.seg[0];
  const int C = sg.C, CS = C / KS, CS2 = CS * 2;
  const int csh = 31 - __builtin_clz((unsigned)CS2);    // CS * 2 is a power of two (host)
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int vid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int nimg = (int)(p.M / HW);
  const int img = vid % nimg, rr = vid / nimg;
  const int ks_i = rr % KS, ct = rr / KS;
  const long long m0 = (long long)img * HW;
  const int n0 = ct * 32, ci0 = ks_i * CS;

  if (tid < 64) reinterpret_cast<uint4*>(sZ)[tid] = make_uint4(0, 0, 0, 0);
  {
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(sg.x, sg.xbytes);
    const int npieces = (HW * CS2) >> 10;
    for (int q = wv; q < npieces; q += 4) {
      const unsigned o = (unsigned)(q * 1024 + lane * 16);
      const unsigned P = o >> csh, sl = (o & (unsigned)(CS2 - 1)) >> 4;
      const unsigned src = ((unsigned)m0 + P) * (unsigned)(C * 2) + (unsigned)(ci0 * 2) + ((sl ^ (P & 7u)) << 4);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sX + q * 1024), 16, src, 0, 0, 0);
    }
  }
  // this wave's quarter of the K range: k-step = (tap, 16 channels), taps outermost
  const int kpt = CS >> 4, kpsh = 31 - __builtin_clz((unsigned)kpt);
  const int nk = (9 * kpt) >> 2, ks0 = wv * nk;
  const unsigned char* wb = sg.w + ((size_t)(n0 + lr) * C + ci0 + 8 * lh) * 2;        // + (tap * Cout * C + cik * 16) * 2
  const size_t wtap = (size_t)p.Cout * C * 2;
  auto bsrc = [&](int ks) { const int tap = ks >> kpsh, cik = ks & (kpt - 1); return wb + (size_t)tap * wtap + (size_t)cik * 32; };
  int ph[NT], pw[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { const int px = t * 32 + lr; ph[t] = px >> WSH; pw[t] = px & (W - 1); }
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  // D weight fragments in flight per wave (4 D KiB per CU): a block streams 590 KB (8 x 8 x 1024) or 147 KB of weights and nothing else - at 16 KiB in flight the
  // 8 x 8 level ran 45 us (8 GB/s and CU)
  // the images of an output-channel tile read the SAME weights: each starts its K quarter at another point (rot), so that at any moment the eight blocks have different lines
  // in flight - eight times the distinct HBM requests, and whoever comes second finds the line in L2
  const int rot = (int)(((long long)(img & 7) * nk) >> 3);
  auto kmap = [&](int j) { int r = j + rot; if (r >= nk) r -= nk; return ks0 + r; };
  uint4 bq[D];
#pragma unroll
  for (int u = 0; u < D; ++u) bq[u] = *reinterpret_cast<const uint4*>(bsrc(kmap(u)));
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(D) : "memory");                 // the image's DMAs (issued first) have landed; the weight fragments stay in flight
  __syncthreads();
  for (int kk = 0; kk < nk; kk += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int ks = kmap(kk + u);
      const int tap = ks >> kpsh, cik = ks & (kpt - 1);
      const int t3 = (tap >= 6) ? 2 : (tap >= 3) ? 1 : 0;
      const int dh = t3 - 1, dw = tap - 3 * t3 - 1;
      const uint4 bcur = bq[u];
      { const int jn = kk + u + D < nk ? kk + u + D : nk - 1; bq[u] = *reinterpret_cast<const uint4*>(bsrc(kmap(jn))); }      // unconditional (clamped): the compiler counts the loads in flight exactly, no branch
      const bf16x8 fb = __builtin_bit_cast(bf16x8, bcur);
      const int c16 = 2 * cik + lh;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int hh = ph[t] + dh, ww = pw[t] + dw;
        const bool ok = (unsigned)hh < (unsigned)W && (unsigned)ww < (unsigned)W;
        const int pp = (hh << WSH) + ww;
        const unsigned char* a = ok ? sX + (pp << csh) + ((c16 ^ (pp & 7)) << 4) : sZ;
        const bf16x8 fa = *reinterpret_cast<const bf16x8*>(a);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[t], 0, 0, 0);
      }
    }
  }
  // ---- the four K quarters meet: [quarter][pixel][32 co] fp32 in LDS (the image is dead), summed in place into quarter 0 ----------------
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) red[((size_t)wv * HW + t * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh) * CSTR + lr] = acc[t][i];
  __syncthreads();
  for (int e = tid; e < HW * 8; e += 256) {             // float4 columns: 8 per pixel
    const int px = e >> 3, c4 = (e & 7) * 4;
    float* d0 = red + (size_t)px * CSTR + c4;
    f32x4 v = *reinterpret_cast<const f32x4*>(d0);
#pragma unroll
    for (int q = 1; q < 4; ++q) v += *reinterpret_cast<const f32x4*>(d0 + (size_t)q * HW * CSTR);
    if constexpr (KS > 1) *reinterpret_cast<f32x4*>(p.ws + ((size_t)ks_i * p.M + m0 + px) * p.Cout + n0 + c4) = v;      // the slice's slab: conv_splitk_finish sums them
    else *reinterpret_cast<f32x4*>(d0) = v;
  }
  if constexpr (KS == 1) {
    __syncthreads();
    conv_epilogue_pick<T, HW, 32>(p, m0, n0, img, red, CSTR, red + 4 * HW * CSTR);
  }
}
template <int W, int KS> static constexpr int conv_img_smem() {
  constexpr int HW = W * W;
  constexpr int tile = 1024 + 131072, redb = 4 * HW * 36 * 4;
  return (tile > redb ? tile : redb) + 4 * 4 * 16 * 4;
}
// eligibility + K slices (0: not this kernel)
static int pick_img(const rua_conv_desc* d, bool in_group) {
  if (!g_tune.conv_img || in_group || d->dtype != RUA_BF16 || d->nseg != 1 || d->in_scale || d->in_fold) return 0;
  const rua_conv_seg& g = d->seg[0];
  if (g.taps != 9 || g.dil != 1 || d->stride != 1 || g.up_shift != 0 || g.Hs != d->H || g.Ws != d->W || d->H != d->W || (d->W != 8 && d->W != 16)) return 0;
  const int HW = d->H * d->W;
  if (g.C % 64 || d->Cout % 32) return 0;
  const int KS = ((long long)HW * g.C * 2 <= 131072) ? 1 : 2;
  const int CS = g.C / KS;
  if ((long long)HW * CS * 2 > 131072 || CS % 256 || (CS & (CS - 1))) return 0;      // 9 CS / 16 k-steps in four quarters of whole groups of four
  const long long M = (long long)d->N * HW;
  if (M * d->Cout * 4 >= (1ll << 31)) return 0;
  if ((long long)d->N * (d->Cout / 32) * KS < rua_cu_count() / 2) return 0;
  if (KS > 1) {
    const size_t ws_usable = d->workspace_bytes > 4096 ? (size_t)d->workspace_bytes - 4096 : 0;
    if (!d->workspace || ws_usable / ((size_t)M * d->Cout * sizeof(float)) < (size_t)KS) return 0;
  }
  return KS;
}
static int plan_conv_img(const rua_conv_desc* d, int KS, ConvLaunch* L) {
  ConvK& k = L->a.c;
  k.nbn = d->Cout / 32; k.nbm = d->N; k.ksplit = KS; k.stages_per_split = 0; k.ws = KS > 1 ? (float*)d->workspace : nullptr; k.cnt = nullptr;
  L->gx = (unsigned)(d->N * (d->Cout / 32) * KS);
  const int nk = 9 * (d->seg[0].C / KS / 16) / 4;        // k-steps per wave: 144 (CS = 1024), 72, 36 (CS = 256) - a multiple of the prefetch depth
  if (d->W == 8 && KS == 1 && nk % 24 == 0) L->kernel = CK_IMG8_24;
  else if (d->W == 8 && KS == 1) L->kernel = CK_IMG8_12;
  else if (d->W == 16 && KS == 1) L->kernel = CK_IMG16;
  else if (d->W == 16 && KS == 2) L->kernel = CK_IMG16_K2;
  else { rua_set_error("conv_img: no instantiation for W=%d KS=%d", d->W, KS); return RUA_ERR_ARG; }
  L->smem = d->W == 8 ? conv_img_smem<8, 1>() : KS == 1 ? conv_img_smem<16, 1>() : conv_img_smem<16, 2>();
  L->ksplit = KS; L->finisher = KS > 1 ? 1 : 0;
  return RUA_OK;
}

// conv_dmap eligibility: bf16, wide outputs, every segment a whole number of 64-channel stages
static bool pick_dmap(const rua_conv_desc* d) {
  const int mode = g_tune.conv_dmap;      // 0: off (experiments)
  if (!mode || d->dtype != RUA_BF16 || d->Cout < 128) return false;
  for (int s_ = 0; s_ < d->nseg; ++s_)
    if (d->seg[s_].C % 64 != 0) return false;
  return true;
}

// =========================================================================================
// conv_small: 1x1 convolutions over at most a few thousand output pixels, bf16 - the PSPPooling at the bottleneck (model2.py:41-79 at 8 x 8 x 1024:
// four branch convs on 8 .. 512 pixels, the fuse conv over five concatenated sources), the upsampling / stride-2 convs of the two deepest
// levels and the data gradients of all of them.  These are GEMMs of 0.03 - 2 GFLOP; on the tiled kernels they ran as 128 x 128 tiles with K split
// 8 - 32 ways plus a finisher launch: 10 - 26 us each, almost all of it fixed cost (two launches, slab round trip, an LDS-DMA ring that never
// fills).  Here a block owns 32 pixels x 64 output channels over the WHOLE K: no K split across blocks, no slabs, no finisher.  Its four
// waves take a quarter of the K range each and read their MFMA fragments STRAIGHT from global memory into registers (both operands are
// K-contiguous rows: a pixel's channels, an output channel's weights; 16-byte buffer loads, out-of-range rows read zeros), eight k-steps
// = 24 loads per wave in flight, no LDS and no barrier in the loop; the four partial tiles meet in LDS and leave through the shared epilogue.
// Concatenated sources (segments) follow one another in the K range; nearest-upsampled sources and stride 2 are address arithmetic.
template <int BNT>
__device__ __forceinline__ void conv_small_body(const ConvK& p) {
  typedef bf16_t T;
  constexpr int BM = 32, BN = 32 * BNT, CH = 8, CSTR = BN + 4;
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* part = reinterpret_cast<float*>(smem);           // [4 waves][BM][CSTR]
  float* sred = part + 4 * BM * CSTR;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int bn_i = blockIdx.x % p.nbn, bm_i = blockIdx.x / p.nbn;
  const long long m0 = (long long)bm_i * BM;
  const int n0 = bn_i * BN;
  const long long m = m0 + lr;
  const bool av = m < p.M;
  const int mm = av ? (int)m : 0, HW = p.H * p.W;
  const int n = mm / HW, rem = mm - n * HW, h = rem / p.W, w = rem - h * p.W;
  const int ah = h * p.stride, aw = w * p.stride;
  int total = 0;
  for (int s_ = 0; s_ < p.nseg; ++s_) total += p.seg[s_].C >> 4;
  const int q = (total + 3) >> 2;
  int ks = wid * q, ke = ks + q < total ? ks + q : total;
  int seg = 0, kk = ks;
  while (seg + 1 < p.nseg && kk >= (p.seg[seg].C >> 4)) { kk -= p.seg[seg].C >> 4; ++seg; }
  f32x16 acc[BNT];
#pragma unroll
  for (int t = 0; t < BNT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  __amdgpu_buffer_rsrc_t rx = make_rsrc(p.seg[0].x, p.seg[0].xbytes), rw = make_rsrc(p.seg[0].w, p.seg[0].wbytes);
  unsigned abase = OOB, bbase[BNT];
  int nk = 1;
  auto enter = [&]() {
    const SegK sg = p.seg[seg];
    rx = make_rsrc(sg.x, sg.xbytes); rw = make_rsrc(sg.w, sg.wbytes);
    nk = sg.C >> 4;
    abase = av ? (unsigned)((((n * sg.Hs + (ah >> sg.up)) * sg.Ws + (aw >> sg.up)) * sg.C + lh * 8) * 2) : OOB;
#pragma unroll
    for (int t = 0; t < BNT; ++t) bbase[t] = (n0 + t * 32 + lr) < p.Cout ? (unsigned)(((n0 + t * 32 + lr) * sg.C + lh * 8) * 2) : OOB;
  };
  if (ks < ke) enter();
  while (ks < ke) {
    int nstep = ke - ks;                                   // a chunk stays inside its segment
    if (nstep > CH) nstep = CH;
    if (nstep > nk - kk) nstep = nk - kk;
    uint4 a[CH], b[BNT][CH];
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (j < nstep) {
        a[j] = bufload16(rx, abase + (unsigned)((kk + j) * 32));
#pragma unroll
        for (int t = 0; t < BNT; ++t) b[t][j] = bufload16(rw, bbase[t] + (unsigned)((kk + j) * 32));
      }
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (j < nstep) {
#pragma unroll
        for (int t = 0; t < BNT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[j]), __builtin_bit_cast(bf16x8, b[t][j]), acc[t], 0, 0, 0);
      }
    ks += nstep; kk += nstep;
    if (kk == nk && ks < ke) { ++seg; kk = 0; enter(); }
  }
  float* mine = part + wid * BM * CSTR;
#pragma unroll
  for (int t = 0; t < BNT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) mine[((i & 3) + 8 * (i >> 2) + 4 * lh) * CSTR + t * 32 + lr] = acc[t][i];
  __syncthreads();
  for (int e = tid; e < BM * BN; e += 256) {                 // the four K quarters, in a fixed order
    const int r = e / BN, c = e - r * BN, o = r * CSTR + c;
    part[o] = ((part[o] + part[BM * CSTR + o]) + part[2 * BM * CSTR + o]) + part[3 * BM * CSTR + o];
  }
  __syncthreads();
  conv_epilogue<T, BM, BN>(p, m0, n0, bm_i, part, CSTR, sred);
}
template <int BNT> __global__ __launch_bounds__(256) void conv_small(const ConvK p) { conv_small_body<BNT>(p); }
// the members of a group (the four branch convolutions of a PSPPooling at the bottleneck - 512 / 128 / 32 / 8 pixels -, the fuse conv's data gradients towards
// them): blockIdx.y = member, grids of unequal size (a launch of 4 - 64 blocks is all latency: ~10 us each whatever its pixel count - side by side they cost one)
template <int BNT> __global__ __launch_bounds__(256) void conv_small_g(const ConvKG g) {
  const ConvK& p = g.k[blockIdx.y];
  if ((int)blockIdx.x >= p.nbm * p.nbn) return;
  conv_small_body<BNT>(p);
}

// conv_small eligibility: bf16, every source 1x1 with a multiple of 16 channels, few pixels (the K-split regime of the tiled kernels)
static bool pick_small(const rua_conv_desc* d) {
  if (!g_tune.conv_small || d->dtype != RUA_BF16 || d->in_scale || d->in_fold) return false;
  const long long M = (long long)d->N * d->H * d->W;
  if (M > g_tune.conv_small || d->Cout < 32) return false;
  for (int s_ = 0; s_ < d->nseg; ++s_)
    if (d->seg[s_].taps != 1 || d->seg[s_].C % 16 != 0) return false;
  return true;
}
static void plan_conv_small(ConvLaunch* L) {
  ConvK& k = L->a.c;
  k.nbm = (int)((k.M + 31) / 32); k.nbn = (k.Cout + 63) / 64;
  k.ksplit = 1; k.stages_per_split = 0; k.ws = nullptr; k.cnt = nullptr;
  L->kernel = CK_SMALL; L->gx = (unsigned)(k.nbm * k.nbn); L->smem = (4 * 32 * 68 + 4 * 8 * 16) * 4;
}

// =========================================================================================
// Host side: plan, then issue.  conv_plan_one() turns a descriptor into a ConvLaunch - kernel row, grid, LDS, kernel arguments, K slices, finisher - as a pure
// function of the descriptor, whether it is one of `members` convolutions of a group, g_tune and rua_cu_count(): it launches nothing and keeps no state.
// conv_pack() joins m plans on the same row into the arguments, grid and LDS of one launch, conv_issue() puts that on a stream.  Every export below is a
// composition of these, so what rua_conv_plan / rua_conv_group_plan report is what the launch does.

// which kernel serves a descriptor: the public id of rua_conv_kernel_id; *ks: the K slices of conv_img2 / conv_img
static int conv_pick(const rua_conv_desc* d, bool in_group, int* ks) {
  *ks = 1;
  if (rua_pick_strip(d)) return 5;
  if (pick_halo(d)) return 3;
  if (pick_pw(d)) return 4;
  if (pick_small(d)) return 6;
  if (const int img2_ks = rua_pick_img2(d, in_group)) { *ks = img2_ks; return 8; }      // the two deepest levels (round 5, conv_img2.hip)
  if (!in_group && rua_band128_sum_ok(d)) return 9;         // several 3x3 segments at C = 128 / 256 (the summed second convolutions of levels 3 - 4): conv_band128m, the sum on chip
  if (const int img_ks = pick_img(d, in_group)) { *ks = img_ks; return 7; }
  if (pick_dmap(d)) return 2;
  return pick_dma(d, pick_bn(d, (long long)d->N * d->H * d->W)) ? 1 : 0;
}

// tile, grid and K split of the tiled kernels (ids 0 - 2): what conv_plan_one launches and rua_conv_tile_bm / _bn report
struct ConvTiling { bool dmap; int bm, bn, nbm, nbn, ksplit, stages_per_split; };
static void conv_tiling(const rua_conv_desc* d, ConvTiling* t) {
  const long long M = (long long)d->N * d->H * d->W;
  int units = 0;
  for (int s = 0; s < d->nseg && s < RUA_MAX_SEG; ++s) units += d->seg[s].taps * ((d->seg[s].C + 31) / 32);
  const bool sized = M > 0 && d->Cout > 0;                  // (the queries answer for any descriptor)
  const size_t ws_usable = d->workspace_bytes > 4096 ? (size_t)d->workspace_bytes - 4096 : 0;
  t->dmap = pick_dmap(d);
  if (t->dmap) {
    // 128 x 128 tiles; split K until the grid covers the chip once (every level of the reference network then runs
    // 256 blocks of >= 18 stages: one block per CU, no tail)
    const int target = g_tune.dmap_target > 0 ? g_tune.dmap_target : rua_cu_count();      // one block per CU
    t->bm = 128; t->bn = 128;
    t->nbn = (d->Cout + 127) / 128;
    t->nbm = (int)((M + 127) / 128);
    const int nstages = units / 2;
    const long long tiles = (long long)t->nbm * t->nbn;
    int want = 1;
    const long long slabs = (d->workspace && sized) ? (long long)(ws_usable / ((size_t)M * d->Cout * sizeof(float))) : 0;
    if (slabs >= 2 && tiles < target) {
      want = (int)((target + tiles - 1) / tiles);
      if (want > nstages / 4) want = nstages / 4;
      if (want > 32) want = 32;
      if (want > slabs) want = (int)slabs;
      if (want < 1) want = 1;
      // half the chip busy for a short K beats two slices + slab traffic + a finisher launch
      // (measured at the 32x32 level: 28.4 vs 32.5 us for K = 36 stages; the 108-stage convs still split: 46 vs 68)
      if (tiles * 2 >= target && nstages <= 40) want = 1;
    }
    t->stages_per_split = (nstages + want - 1) / want;
    t->ksplit = t->stages_per_split > 0 ? (nstages + t->stages_per_split - 1) / t->stages_per_split : 1;
    // the unsplit half-chip case (32x32 level: 128 tiles of 128 x 128, 36 stages): 64-row tiles put a block on every CU
    // (measured there: 25.5 / 23.7 / 22.6 us vs 30.1 / 30.0 / 28.6 for d = 1 / d = 15 / plain)
    if (g_tune.dmap_bm64 && t->ksplit == 1 && tiles < target && tiles * 2 >= target) {
      t->bm = 64;
      t->nbm = (int)((M + 63) / 64);
    }
    return;
  }
  t->bn = pick_bn(d, M);
  t->bm = pick_bm(d, M, t->bn);
  t->nbn = (d->Cout + t->bn - 1) / t->bn;
  t->nbm = (int)((M + t->bm - 1) / t->bm);
  const int nstages = (units + 1) / 2;
  t->ksplit = (d->workspace && t->bm == 128 && sized) ? pick_ksplit((long long)t->nbm * t->nbn, nstages, M, d->Cout, ws_usable) : 1;
  t->stages_per_split = (nstages + t->ksplit - 1) / t->ksplit;
  t->ksplit = t->stages_per_split > 0 ? (nstages + t->stages_per_split - 1) / t->stages_per_split : 1;
}
static int tile_form(int bm, int bn) { return bn == 128 ? 4 : (bm == 256 ? 2 : 0) + (bn == 64 ? 1 : 0); }       // ConvKernel: 0 128 x 32, 1 128 x 64, 2 256 x 32, 3 256 x 64, 4 128 x 128

// one row per ConvKernel below CK_MFMA_KERNELS (conv_img2's and conv_strip's rows stand beside their kernels)
#define FN RUA_KERNEL_FN
#define RUA_TILE_ROWS(NAME, KERN, LDS, ...) \
  {NAME, FN(KERN<__VA_ARGS__ 128, 32>), nullptr, nullptr, CA_CONV, LDS<__VA_ARGS__ 128, 32>(), 0}, {NAME, FN(KERN<__VA_ARGS__ 128, 64>), nullptr, nullptr, CA_CONV, LDS<__VA_ARGS__ 128, 64>(), 0}, \
  {NAME, FN(KERN<__VA_ARGS__ 256, 32>), nullptr, nullptr, CA_CONV, LDS<__VA_ARGS__ 256, 32>(), 0}
static const ConvKernelRow CONV_ROWS[CK_MFMA_KERNELS] = {
  RUA_TILE_ROWS("conv_igemm", conv_igemm, conv_smem, bf16_t,),
  {"conv_igemm", FN(conv_igemm<bf16_t, 256, 64>), FN(conv_igemm_g<bf16_t, 256, 64>), nullptr, CA_CONV, conv_smem<bf16_t, 256, 64>(), 0},     // the C = 64 level's 3x3 convs
  {"conv_igemm", FN(conv_igemm<bf16_t, 128, 128>), nullptr, nullptr, CA_CONV, conv_smem<bf16_t, 128, 128>(), 0},
  RUA_TILE_ROWS("conv_igemm", conv_igemm, conv_smem, float,),
  {"conv_igemm", FN(conv_igemm<float, 256, 64>), nullptr, nullptr, CA_CONV, conv_smem<float, 256, 64>(), 0},
  {"conv_igemm", FN(conv_igemm<float, 128, 128>), nullptr, nullptr, CA_CONV, conv_smem<float, 128, 128>(), 0},
  RUA_TILE_ROWS("conv_dma", conv_dma, conv_dma_base,),
  {"conv_dma", FN(conv_dma<256, 64>), nullptr, nullptr, CA_CONV, conv_dma_base<256, 64>(), 0},
  {"conv_dma", FN(conv_dma<128, 128>), nullptr, nullptr, CA_CONV, conv_dma_base<128, 128>(), 0},
  {"conv_dmap", FN(conv_dmap<128, 128, 64>), FN(conv_dmap_g<128, 128, 64>), FN(conv_dmap_chain<128, 128, 64>), CA_CONV, conv_dmap_smem<128, 128>(), conv_dmap_chain_smem<128, 128>()},
  {"conv_dmap", FN(conv_dmap<128, 128, 128>), nullptr, nullptr, CA_CONV, conv_dmap_smem<128, 128>(), 0},
  {"conv_dmap", FN(conv_dmap<64, 128, 64>), FN(conv_dmap_g<64, 128, 64>), FN(conv_dmap_chain<64, 128, 64>), CA_CONV, conv_dmap_smem<64, 128>(), conv_dmap_chain_smem<64, 128>()},
  {"conv_dmap_s", FN(conv_dmap_s<128, 128, 64>), FN(conv_dmap_gs<128, 128, 64>), nullptr, CA_CONV, conv_dmap_smem<128, 128, 4>(), 0},      // DMA instructions between the MFMAs of the same waves (four stage buffers)
  {"conv_halo", FN(conv_halo<32, 2>), nullptr, nullptr, CA_HALO, 96 * 1024, 0},
  {"conv_halo", FN(conv_halo<32, 3>), nullptr, nullptr, CA_HALO, 96 * 1024, 0},
  {"conv_pw", FN(conv_pw<2, false>), FN(conv_pw_g<2, false>), nullptr, CA_PW2, 0, 0},
  {"conv_pw", FN(conv_pw<2, true>), FN(conv_pw_g<2, true>), nullptr, CA_PW2, 0, 0},
  {"conv_pw", FN(conv_pw<4, false>), nullptr, nullptr, CA_PW4, 0, 0},
  {"conv_pw", FN(conv_pw<4, true>), nullptr, nullptr, CA_PW4, 0, 0},
  {"conv_pw", FN(conv_pw<6, false>), nullptr, nullptr, CA_PW6, 0, 0},
  {"conv_pw", FN(conv_pw<6, true>), nullptr, nullptr, CA_PW6, 0, 0},
  {"conv_small", FN(conv_small<2>), FN(conv_small_g<2>), nullptr, CA_CONV, 0, 0},
  {"conv_img", FN(conv_img<8, 1, 24>), nullptr, nullptr, CA_CONV, conv_img_smem<8, 1>(), 0},
  {"conv_img", FN(conv_img<8, 1, 12>), nullptr, nullptr, CA_CONV, conv_img_smem<8, 1>(), 0},
  {"conv_img", FN(conv_img<16, 1, 12>), nullptr, nullptr, CA_CONV, conv_img_smem<16, 1>(), 0},
  {"conv_img", FN(conv_img<16, 2, 18>), nullptr, nullptr, CA_CONV, conv_img_smem<16, 2>(), 0},
};
#undef RUA_TILE_ROWS
#undef FN
static const ConvKernelRow& conv_row(int kernel) {
  return kernel >= CK_STRIP ? RUA_STRIP_ROWS[kernel - CK_STRIP] : kernel >= CK_IMG2_8 ? RUA_IMG2_ROWS[kernel - CK_IMG2_8] : CONV_ROWS[kernel];
}

// ---- planning ----------------------------------------------------------------------------------------------------------
// in_group: the convolution is one of `members` of a rua_conv_fwd_group call that groups (members >= 2, tuning key conv_group not 0); rua_conv_fwd alone is
// members = 1, in_group = false.  A group shares the chip: conv_strip sizes its round of blocks by `members`, and the kernels that want the chip to themselves
// (conv_img2, conv_img, the summed form of conv_band128m) stay out of it.
static int conv_plan_one(const rua_conv_desc* d, int members, bool in_group, ConvLaunch* L) {
  RUA_CHECK_ARG(d && d->nseg >= 1 && d->nseg <= RUA_MAX_SEG, "rua_conv_fwd: nseg out of range");
  RUA_CHECK_ARG(d->dtype == RUA_F32 || d->dtype == RUA_BF16, "rua_conv_fwd: bad dtype");
  const int vec = d->dtype == RUA_BF16 ? 8 : 4;
  RUA_CHECK_ARG(d->Cout > 0 && d->Cout % 8 == 0, "rua_conv_fwd: Cout=%d must be a multiple of 8", d->Cout);
  RUA_CHECK_ARG(d->N > 0 && d->H > 0 && d->W > 0 && d->stride >= 1, "rua_conv_fwd: bad output grid");
  RUA_CHECK_ARG(d->y != nullptr, "rua_conv_fwd: null output");
  RUA_CHECK_ARG(d->out_stride >= 1 && d->OH >= (d->H - 1) * d->out_stride + 1 && d->OW >= (d->W - 1) * d->out_stride + 1,
                "rua_conv_fwd: output tensor smaller than the strided grid");
  RUA_CHECK_ARG((long long)d->N * d->H * d->W < (1ll << 31), "rua_conv_fwd: too many pixels");
  RUA_CHECK_ARG(d->aux_mode == 0 || d->aux != nullptr, "rua_conv_fwd: aux_mode without aux");
  RUA_CHECK_ARG(d->stats_mode == 0 || d->stats != nullptr, "rua_conv_fwd: stats_mode without stats");
  RUA_CHECK_ARG(d->stats_mode != 2 || d->aux != nullptr, "rua_conv_fwd: stats_mode 2 needs aux");
  ConvK& k = L->a.c;
  k.nseg = d->nseg;
  int units = 0;
  for (int s = 0; s < d->nseg; ++s) {
    const rua_conv_seg& g = d->seg[s];
    RUA_CHECK_ARG(g.x && g.w, "rua_conv_fwd: null segment pointer");
    RUA_CHECK_ARG(g.C > 0 && g.C % vec == 0, "rua_conv_fwd: segment C=%d not a multiple of %d", g.C, vec);
    RUA_CHECK_ARG(g.taps == 1 || g.taps == 9, "rua_conv_fwd: taps must be 1 or 9");
    RUA_CHECK_ARG(g.up_shift >= 0 && g.up_shift <= 4 && g.dil >= 1, "rua_conv_fwd: bad up_shift/dil");
    // every centre-tap read must be in range: (H-1)*stride < Hs<<up
    RUA_CHECK_ARG((long long)(d->H - 1) * d->stride < ((long long)g.Hs << g.up_shift) &&
                  (long long)(d->W - 1) * d->stride < ((long long)g.Ws << g.up_shift),
                  "rua_conv_fwd: segment %d source %dx%d (up %d) too small for output %dx%d stride %d", s, g.Hs, g.Ws, g.up_shift, d->H, d->W, d->stride);
    RUA_CHECK_ARG((long long)d->N * g.Hs * g.Ws * g.C * 4 < (1ll << 31), "rua_conv_fwd: source tensor must stay below 2 GiB (32-bit offsets)");
    RUA_CHECK_ARG(g.up_shift == 0 || g.taps == 1, "rua_conv_fwd: nearest-upsampled sources are 1x1 only");
    RUA_CHECK_ARG((long long)g.taps * d->Cout * g.C * 4 < (1ll << 31), "rua_conv_fwd: weight block too large");
    SegK& o = k.seg[s];
    o.x = (const unsigned char*)g.x; o.w = (const unsigned char*)g.w;
    o.C = g.C; o.Hs = g.Hs; o.Ws = g.Ws; o.up = g.up_shift; o.dil = g.dil; o.taps = g.taps;
    o.nchunk = (g.C + 31) / 32; o.ubegin = units;
    o.xbytes = (unsigned)((size_t)d->N * g.Hs * g.Ws * g.C * (d->dtype == RUA_BF16 ? 2 : 4));
    o.wbytes = (unsigned)((size_t)g.taps * d->Cout * g.C * (d->dtype == RUA_BF16 ? 2 : 4));
    units += g.taps * o.nchunk;
  }
  k.nunits = units;
  RUA_CHECK_ARG(units <= RUA_MAX_UNITS, "rua_conv_fwd: K = %d units of 32 channels exceeds the unit-table capacity %d", units, RUA_MAX_UNITS);
  k.N = d->N; k.H = d->H; k.W = d->W; k.Cout = d->Cout; k.stride = d->stride;
  k.M = (long long)d->N * d->H * d->W;
  k.bias = d->bias; k.aux = (const unsigned char*)d->aux; k.aux_mode = d->aux_mode;
  for (int q = 0; q < 3; ++q) k.bias_more[q] = d->bias ? d->bias_more[q] : nullptr;
  k.mscale = d->mscale; k.mshift = d->mshift; k.out_relu = d->out_relu; k.accumulate = d->accumulate;
  k.y = (unsigned char*)d->y; k.out_stride = d->out_stride; k.OH = d->OH; k.OW = d->OW;
  k.stats = d->stats; k.stats_mode = d->stats_mode;
  k.stats_R = d->stats_replicas < 1 ? 1 : d->stats_replicas;
  RUA_CHECK_ARG((k.stats_R & (k.stats_R - 1)) == 0, "rua_conv_fwd: stats_replicas must be a power of two");
  k.in_scale = d->in_scale; k.in_shift = d->in_shift; k.in_relu = d->in_relu;
  k.epi_fast = g_tune.epi_fast;
  k.nbn = 1; k.nbm = 1; k.ksplit = 1; k.stages_per_split = 0; k.ws = nullptr; k.cnt = nullptr;      // the kernels without tiles or K slices leave it so
  int ks;
  L->kid = conv_pick(d, in_group, &ks);
  L->route = CONV_LAUNCH; L->kernel = -1; L->gx = 0; L->block = 256; L->smem = 0; L->bm = L->bn = 0; L->ksplit = 1; L->finisher = 0; L->groupable = false; L->per_cu = 0;
  if (L->kid == 5) return rua_plan_conv_strip(d, members, in_group, L);
  RUA_CHECK_ARG(d->in_scale == nullptr && d->in_fold == nullptr, "rua_conv_fwd: in_scale / in_shift / in_fold (normalise on load) is not available for "
                                        "this shape: ask rua_conv_fused_input_ok() first");
  switch (L->kid) {
    case 3: return plan_conv_halo(d->seg[0].dil, L);
    case 4: {
      const int steps = pw_steps(d);
      if (steps <= 2) plan_conv_pw<2>(L->a.p2, d, L); else if (steps <= 4) plan_conv_pw<4>(L->a.p4, d, L); else plan_conv_pw<6>(L->a.p6, d, L);
      L->groupable = in_group && steps <= 2 && (g_tune.conv_group & 32);
      return RUA_OK;
    }
    case 6: plan_conv_small(L); L->groupable = in_group && (g_tune.conv_group & 16); return RUA_OK;
    case 8: rua_plan_conv_img2(d, ks, L); return RUA_OK;
    case 9: L->route = CONV_ROUTE_BAND128_SUM; return RUA_OK;
    case 7: return plan_conv_img(d, ks, L);
    default: break;
  }
  ConvTiling t;
  conv_tiling(d, &t);
  k.nbn = t.nbn; k.nbm = t.nbm; k.ksplit = t.ksplit; k.stages_per_split = t.stages_per_split;
  k.ws = (float*)d->workspace;
  L->bm = t.bm; L->bn = t.bn; L->ksplit = t.ksplit;
  L->gx = (unsigned)(t.nbm * t.nbn * t.ksplit);
  if (t.dmap) {
    // the last 4 KiB of the workspace hold the tile ticket counters of the in-launch reduction (zero between launches:
    // the caller zero-fills the workspace once, every last arriver resets its counter)
    // OFF by default - measured: the single last-arriving block reads ksplit x 64 KB of slabs serially (8x8 level: 45 vs 26 us,
    // 16x16: 39 vs 28 us); the separate finisher spreads the same bytes over 1024 blocks.  Kept (and tested) as an option.
    const size_t ws_usable = d->workspace_bytes > 4096 ? (size_t)d->workspace_bytes - 4096 : 0;
    k.cnt = (g_tune.dmap_fused_finish && d->workspace && (long long)((k.M + 127) / 128) * t.nbn <= 1024) ? reinterpret_cast<int*>((char*)d->workspace + ws_usable) : nullptr;
    const bool rows64 = g_tune.dmap_rowb != 128;            // bytes per LDS row
    L->kernel = t.bm == 64 ? CK_DMAP64 : !rows64 ? CK_DMAP128_R128 : g_tune.dmap_spread == 1 ? CK_DMAP_S : CK_DMAP128;
    L->finisher = (t.ksplit > 1 && k.cnt == nullptr) ? 1 : 0;
    L->groupable = in_group && (g_tune.conv_group & (t.bm == 128 ? 4 : 8)) && t.ksplit == 1 && (rows64 || t.bm == 64);
    L->smem = conv_row(L->kernel).lds;
    return RUA_OK;
  }
  // Kernel choice (measured per level, scratch/bench_conv.py): the LDS-DMA kernel wins where K is long and the grid is
  // small (Cout >= 128: 5-12 %); the register-staged kernel wins on the two top levels (short K, occupancy-bound) and,
  // with 128-wide tiles, on the very long K of the multi-branch convs at Cout >= 256.
  // split-K invariant: the workspace is all zeros on entry (caller zero-fills it once) and the finisher writes the
  // zeros back after consuming the sums, so no memset is launched per convolution.
  L->finisher = t.ksplit > 1 ? (d->dtype == RUA_BF16 ? 1 : 2) : 0;
  if (L->kid == 1) {
    L->kernel = CK_DMA + tile_form(t.bm, t.bn);
    L->smem = conv_row(L->kernel).lds;
    return RUA_OK;
  }
  L->kernel = (d->dtype == RUA_BF16 ? CK_IGEMM_BF16 : CK_IGEMM_F32) + tile_form(t.bm, t.bn);
  L->smem = conv_row(L->kernel).lds - RUA_MAX_UNITS * 16 + ((k.nunits * 16 + 255) / 256) * 256;     // unit table sized to this launch
  L->groupable = in_group && (g_tune.conv_group & 2) && t.ksplit == 1 && L->kernel == CK_IGEMM_BF16 + 3;
  return RUA_OK;
}

// ---- issuing -----------------------------------------------------------------------------------------------------------
// One launch for m >= 1 plans on the SAME row.  One plan: the kernel itself, with the plan's own grid and LDS.  Several: its grouped form - blockIdx.y picks the
// member, the grid and the LDS are the largest member's (the others' surplus blocks leave at once; conv_strip32 rounds the grid up to a multiple
// of 8), unused slots repeat member 0 - or, chain, conv_dmap_chain: ONE grid of the members' common size, every block walking all of them.
// conv_strip32s is one grid whatever m is (rua_strip_s_pack).
struct ConvPacked {
  const ConvKernelRow* row; const void* fn; int form;   // form: 0 the kernel, 1 its grouped form, 2 its chain form
  dim3 grid; unsigned block; int smem, nmem;
  void* args[2];
  union alignas(16) { ConvKG c; PwKG<2> p; StripKG s; unsigned char raw[4096]; } many;
};
static int conv_pack(const ConvLaunch* const* L, int m, bool chain, ConvPacked* P) {
  const ConvLaunch& first = *L[0];
  const ConvKernelRow& row = conv_row(first.kernel);
  P->row = &row; P->form = chain ? 2 : m > 1 ? 1 : 0;
  P->fn = chain ? row.chain : m > 1 ? row.many : row.one;
  RUA_CHECK_ARG(P->fn && m <= RUA_MAX_BRANCH, "rua_conv_fwd_group: %d members of %s in one grid", m, row.name);
  P->grid = dim3(first.gx); P->block = first.block; P->smem = first.smem; P->nmem = m;
  P->args[0] = row.args == CA_IMG2 ? const_cast<void*>(static_cast<const void*>(&first.i2)) : const_cast<void*>(static_cast<const void*>(&first.a));
  P->args[1] = &P->nmem;
  if (row.args == CA_STRIPS) { P->args[0] = &P->many; return rua_strip_s_pack(L, m, &P->many, &P->grid.x, &P->smem); }
  if (m == 1) return RUA_OK;
  for (int i = 0; i < RUA_MAX_BRANCH; ++i) {
    const ConvLaunch& x = *L[i < m ? i : 0];
    if (x.gx > P->grid.x) P->grid.x = x.gx;
    if (x.smem > P->smem) P->smem = x.smem;
    if (row.args == CA_CONV) P->many.c.k[i] = x.a.c; else if (row.args == CA_PW2) P->many.p.k[i] = x.a.p2; else P->many.s.k[i] = x.a.s;
  }
  if (row.args == CA_STRIP) P->grid.x = (P->grid.x + 7) / 8 * 8;
  if (chain) P->smem = row.lds_chain; else P->grid.y = m;
  P->args[0] = &P->many;
  return RUA_OK;
}
static int conv_issue(const ConvLaunch* const* L, int m, bool chain, hipStream_t st) {
  ConvPacked P;
  const int rc = conv_pack(L, m, chain, &P);
  if (rc != RUA_OK) return rc;
  static RuaPerDevFlag allowed[CK_KERNELS][3];          // hipFuncSetAttribute: once per (kernel, form, device)
  bool& ok = allowed[L[0]->kernel][P.form].get();
  const int lds = chain ? P.row->lds_chain : P.row->lds;
  if (!ok && lds) (void)hipFuncSetAttribute(P.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  ok = true;
  (void)hipLaunchKernel(P.fn, P.grid, dim3(P.block), P.args, (size_t)P.smem, st);
  RUA_LAUNCH_CHECK(P.row->name);
  return RUA_OK;
}
// a plan on its own: a route's launcher, or its grid and then its finisher over the K slices' slabs
static int conv_issue_alone(const rua_conv_desc* d, const ConvLaunch& L, hipStream_t st) {
  if (L.route == CONV_ROUTE_BAND128_SUM) return rua_launch_band128_sum(d, st);
  const ConvLaunch* one = &L;
  const int rc = conv_issue(&one, 1, false, st);
  if (rc != RUA_OK || !L.finisher) return rc;
  if (L.finisher == 2) launch_splitk_finish<float>(L.a.c, st); else launch_splitk_finish<bf16_t>(L.a.c, st);
  RUA_LAUNCH_CHECK("conv_splitk_finish");
  return RUA_OK;
}

// ---- groups ------------------------------------------------------------------------------------------------------------
// rua_conv_fwd_group: n INDEPENDENT convolutions (the dilation branches of a ResBlock: model2.py:26-31).  Every member is planned as rua_conv_fwd would plan it,
// told that it shares the chip; members that land on the same kernel with the same grid are then issued as ONE grid (blockIdx.y = member), the rest one by
// one.  Results are those of n separate calls.  Nothing is launched before every member has a plan.
struct ConvBatch { int idx[RUA_MAX_BRANCH]; int m; bool chain; };                // members of one launch
struct ConvGroupPlan { ConvLaunch L[RUA_MAX_BRANCH]; ConvBatch b[RUA_MAX_BRANCH]; int nb, band, chain; };     // band: 1 conv_band64m / 2 conv_band128m takes the whole call (nb = 0)

// conv_dmap_chain wants members of one shape
static bool chain_ok(const ConvLaunch* L, const ConvBatch& b) {
  const ConvK& a = L[b.idx[0]].a.c;
  for (int i = 0; i < b.m; ++i) {
    const ConvK& k = L[b.idx[i]].a.c;
    if (k.ksplit != 1 || k.M != a.M || k.Cout != a.Cout || k.nbm != a.nbm || k.nbn != a.nbn || k.H != a.H || k.W != a.W || k.stride != a.stride) return false;
  }
  return true;
}
// The launches of a group, in issue order: (1) members that go alone, in member order; (2) the conv_pw grids, non-dense then dense (grids of unequal size: the
// largest member's); (3) the conv_strip grids, by first member - one row and one blocks-per-CU class each; (4) the other grouped kinds by first member:
// conv_small all together (unequal grids), conv_dmap / conv_igemm members of equal grid and LDS - as a chain where the tuning key dmap_chain asks for it.
static void conv_partition(ConvGroupPlan* P, int n) {
  const ConvLaunch* L = P->L;
  bool done[RUA_MAX_BRANCH] = {false};
  P->nb = 0; P->chain = 0;
  auto collect = [&](int from, auto&& same) -> ConvBatch* {          // the members from `from` on that no launch has yet and `same` accepts: one more launch, or none
    ConvBatch b;
    b.m = 0; b.chain = false;
    for (int j = from; j < n; ++j)
      if (!done[j] && same(L[j])) { b.idx[b.m++] = j; done[j] = true; }
    if (!b.m) return nullptr;
    P->b[P->nb] = b;
    return &P->b[P->nb++];
  };
  for (int i = 0; i < n; ++i)
    if (!L[i].groupable) { ConvBatch& b = P->b[P->nb++]; b.idx[0] = i; b.m = 1; b.chain = false; done[i] = true; }
  for (int kern = CK_PW2; kern <= CK_PW2_DENSE; ++kern) collect(0, [&](const ConvLaunch& x) { return x.kernel == kern; });
  for (int i = 0; i < n; ++i)
    if (!done[i] && L[i].kernel >= CK_STRIP) collect(i, [&](const ConvLaunch& x) { return x.kernel == L[i].kernel && x.per_cu == L[i].per_cu; });
  for (int i = 0; i < n; ++i) {
    if (done[i]) continue;
    if (L[i].kernel == CK_SMALL) { collect(i, [&](const ConvLaunch& x) { return x.kernel == CK_SMALL; }); continue; }
    ConvBatch& b = *collect(i, [&](const ConvLaunch& x) { return x.kernel == L[i].kernel && x.gx == L[i].gx && x.smem == L[i].smem; });      // (member i itself, at the least)
    const int bit = L[i].kernel == CK_DMAP128 ? 1 : L[i].kernel == CK_DMAP64 ? 2 : 0;
    b.chain = b.m >= 2 && (g_tune.dmap_chain & bit) && chain_ok(L, b);
    if (b.chain) P->chain = b.m;
  }
}
static int conv_plan_group(const rua_conv_desc* d, int n, ConvGroupPlan* P) {
  RUA_CHECK_ARG(d && n >= 1 && n <= RUA_MAX_BRANCH, "rua_conv_fwd_group: 1..%d members", RUA_MAX_BRANCH);
  P->nb = 0; P->chain = 0;
  P->band = (n >= 2 && rua_band128m_ok(d, n)) ? 2      // C = 128 / C = 64 on whole rows: two-row stages, weights of a kernel row in registers (conv_band128.hip)
          : rua_band64m_ok(d, n) ? 1 : 0;              // the C = 64 level, round-3 form: one row-streaming launch for all members (conv_band64.hip)
  if (P->band) return RUA_OK;
  const bool in_group = n >= 2 && g_tune.conv_group != 0;
  for (int i = 0; i < n; ++i) {
    const int rc = conv_plan_one(d + i, in_group ? n : 1, in_group, &P->L[i]);
    if (rc != RUA_OK) return rc;
  }
  conv_partition(P, n);
  return RUA_OK;
}

// ---- exports -----------------------------------------------------------------------------------------------------------
static thread_local int g_last_ksplit = 1;
static thread_local int g_group_last_grids = 0, g_group_last_band = 0, g_group_last_chain = 0;
extern "C" int rua_conv_last_ksplit(void) { return g_last_ksplit; }    // K slices of this thread's latest rua_conv_fwd launch (1: no finisher ran)
extern "C" int rua_conv_group_last_grids(void) { return g_group_last_grids; }    // grids the calling thread's latest rua_conv_fwd_group issued (1: one grid for all members)
extern "C" int rua_conv_group_last_chain(void) { return g_group_last_chain; }    // members the latest rua_conv_fwd_group ran back to back inside one conv_dmap_chain grid (0: none)
extern "C" int rua_conv_group_last_band(void) { return g_group_last_band; }      // 1: the calling thread's latest rua_conv_fwd_group ran as one conv_band64m launch, 2: conv_band128m
// would rua_conv_fwd_group run these members as one conv_band64m / conv_band128m launch (which honours in_fold / in_scale of every member)?
extern "C" int rua_conv_group_band_ok(const rua_conv_desc* d, int n) { return (d && (rua_band64m_ok(d, n) || rua_band128m_ok(d, n))) ? 1 : 0; }

extern "C" int rua_conv_fwd(const rua_conv_desc* d, void* stream) {
  ConvLaunch L;
  const int rc = conv_plan_one(d, 1, false, &L);
  if (rc != RUA_OK) return rc;
  g_last_ksplit = L.ksplit;
  return conv_issue_alone(d, L, (hipStream_t)stream);
}
extern "C" int rua_conv_fwd_group(const rua_conv_desc* d, int n, void* stream) {
  ConvGroupPlan P;
  int rc = conv_plan_group(d, n, &P);
  if (rc != RUA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  g_group_last_grids = n;
  g_group_last_band = 0;
  g_group_last_chain = P.chain;
  if (P.band) {
    rc = P.band == 2 ? rua_launch_band128m(d, n, st) : rua_launch_band64m(d, n, st);
    if (rc == RUA_OK) { g_group_last_grids = 1; g_group_last_band = P.band; }
    return rc;
  }
  for (int b = 0; b < P.nb; ++b) {
    const ConvBatch& B = P.b[b];
    const ConvLaunch* mem[RUA_MAX_BRANCH];
    for (int i = 0; i < B.m; ++i) mem[i] = &P.L[B.idx[i]];
    rc = B.m == 1 ? conv_issue_alone(d + B.idx[0], *mem[0], st) : conv_issue(mem, B.m, B.chain, st);
    if (rc != RUA_OK) return rc;
  }
  g_last_ksplit = P.L[n - 1].ksplit;
  g_group_last_grids = P.nb;
  return RUA_OK;
}

static void conv_report(const ConvLaunch& L, const ConvPacked* P, unsigned members, const ConvGroupPlan* G, rua_conv_launch_info* o) {
  memset(o, 0, sizeof(*o));
  o->kernel_id = L.kid; o->form = P ? L.kernel : -1;
  if (P) { o->grid_x = (int)P->grid.x; o->grid_y = (int)P->grid.y; o->block = (int)P->block; o->lds_bytes = P->smem; }
  o->bm = L.bm; o->bn = L.bn; o->ksplit = L.ksplit; o->finisher = L.finisher ? 1 : 0;
  o->members = (int)members;
  if (G) { o->band = G->band; o->chain = G->chain; }
}
extern "C" int rua_conv_plan(const rua_conv_desc* d, rua_conv_launch_info* out) {
  RUA_CHECK_ARG(out, "rua_conv_plan: null pointer");
  ConvLaunch L;
  ConvPacked P;
  const ConvLaunch* one = &L;
  int rc = conv_plan_one(d, 1, false, &L);
  if (rc == RUA_OK && L.route == CONV_LAUNCH) rc = conv_pack(&one, 1, false, &P);
  if (rc == RUA_OK) conv_report(L, L.route == CONV_LAUNCH ? &P : nullptr, 1u, nullptr, out);
  return rc;
}
extern "C" int rua_conv_group_plan(const rua_conv_desc* d, int n, rua_conv_launch_info* out, int* n_out) {
  RUA_CHECK_ARG(out && n_out, "rua_conv_group_plan: null pointer");
  ConvGroupPlan G;
  int rc = conv_plan_group(d, n, &G);
  if (rc != RUA_OK) return rc;
  if (G.band) {                                         // the whole call is one launch of conv_band64.hip / conv_band128.hip
    memset(out, 0, sizeof(*out));
    out->kernel_id = -1; out->form = -1; out->members = (1 << n) - 1; out->band = G.band;
    *n_out = 1;
    return RUA_OK;
  }
  for (int b = 0; b < G.nb; ++b) {
    const ConvBatch& B = G.b[b];
    const ConvLaunch* mem[RUA_MAX_BRANCH];
    unsigned mask = 0;
    for (int i = 0; i < B.m; ++i) { mem[i] = &G.L[B.idx[i]]; mask |= 1u << B.idx[i]; }
    ConvPacked P;
    const bool launch = mem[0]->route == CONV_LAUNCH;
    if (launch && (rc = conv_pack(mem, B.m, B.chain, &P)) != RUA_OK) return rc;
    conv_report(*mem[0], launch ? &P : nullptr, mask, &G, out + b);
  }
  *n_out = G.nb;
  return RUA_OK;
}

// bytes of ONE fp32 slab (M x Cout) of the split-K workspace: a workspace of k slabs + 4 KiB allows k K slices
extern "C" int64_t rua_conv_workspace_bytes(const rua_conv_desc* d) {
  if (!d) return 0;
  return (int64_t)d->N * d->H * d->W * d->Cout * (int64_t)sizeof(float);
}
// The queries below answer for any descriptor - before its buffers exist, too - from the pickers conv_plan_one itself calls.
// 0: conv_igemm (register-staged), 1: conv_dma (LDS-DMA), 2: conv_dmap (LDS-DMA, pipelined across the stage barrier),
// 3: conv_halo (input + halo resident in LDS, lattice tiles), 4: conv_pw (narrow 1x1, per-wave streaming), 5: conv_strip (conv_strip.hip),
// 6: conv_small (1x1 over few pixels, no K split), 7: conv_img (whole image resident in LDS), 8: conv_img2 (conv_img2.hip),
// 9: conv_band128m's form of several summed 3x3 segments (conv_band128.hip)
extern "C" int rua_conv_kernel_id(const rua_conv_desc* d) {
  int ks;
  return d ? conv_pick(d, false, &ks) : RUA_ERR_ARG;
}
extern "C" int rua_conv_fused_input_ok(const rua_conv_desc* d) { return (d && rua_pick_strip(d)) ? 1 : 0; }
// tile (pixel rows, output channels per block) of the tiled kernels: identifies the kernel instantiation
extern "C" int rua_conv_tile_bn(const rua_conv_desc* d) {
  if (!d) return RUA_ERR_ARG;
  ConvTiling t;
  conv_tiling(d, &t);
  return t.bn;
}
extern "C" int rua_conv_tile_bm(const rua_conv_desc* d) {
  if (!d) return RUA_ERR_ARG;
  ConvTiling t;
  conv_tiling(d, &t);
  return t.bm;
}
// LDS of the conv_igemm instantiation with the tile pick_bn / pick_bm choose (the unit table at its capacity)
extern "C" int rua_conv_smem_bytes(const rua_conv_desc* d) {
  const long long M = (long long)d->N * d->H * d->W;
  const int bn = pick_bn(d, M), bm = pick_bm(d, M, bn);
  return CONV_ROWS[(d->dtype == RUA_BF16 ? CK_IGEMM_BF16 : CK_IGEMM_F32) + tile_form(bm, bn)].lds;
}


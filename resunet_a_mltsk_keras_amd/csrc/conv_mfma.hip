// Segmented implicit-GEMM convolution on MFMA (gfx950), channels-last.
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
#ifdef RUA_EPI_DBG_NOVEC
  if (p.M < 0)
#endif
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
#ifdef RUA_EPI_DBG_NOSTORE                             // (timing experiments on the epilogue's latency chain; results are garbage)
      if (v[0] == 123.456f)
#endif
      store8<T>(p.y, ooff[e], v);
    }
  }
  RUA_TS(5);
  if (carry) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { carry[j] = s1[j]; carry[8 + j] = s2[j]; }
  }
#ifdef RUA_EPI_DBG_NOSTATS
  if (s1[0] == 123.456f)
#endif
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
// Profiling hook (bench.py): an event recorded BETWEEN the main kernel of a call and its second launch (split-K finisher,
// wgrad_taps_reduce), so that per-kernel durations can be compared with rocprofv3's per-kernel-name averages.  One shot.
static thread_local hipEvent_t g_mid_event = nullptr;
static thread_local int g_mid_fired = 0;
extern "C" void rua_profile_mid_event(void* ev) { g_mid_event = (hipEvent_t)ev; if (ev) g_mid_fired = 0; }
extern "C" int rua_profile_mid_event_fired(void) { return g_mid_fired; }     // 1: the call since the last arm had a second launch
// rua_wgrad_plan(): the launchers below run with g_wgrad_dry set - every geometry decision is taken, nothing is launched - and
// report the reduction they would leave pending through g_wgrad_pending (also filled by real deferred calls).
static thread_local bool g_wgrad_dry = false;
static thread_local rua_wgrad_pending* g_wgrad_pending = nullptr;
static inline void note_pending(int kind, int parts, long long n, const float* partials, float* dw, int CC, int blocks) {
  if (!g_wgrad_pending) return;
  g_wgrad_pending->kind = kind; g_wgrad_pending->parts = parts; g_wgrad_pending->n = n; g_wgrad_pending->partials = partials;
  g_wgrad_pending->dw = dw; g_wgrad_pending->CC = CC; g_wgrad_pending->blocks = blocks;
}
static inline void record_mid_event(hipStream_t st) {
  if (g_mid_event) { (void)hipEventRecord(g_mid_event, st); g_mid_event = nullptr; g_mid_fired = 1; }
}
template <typename T> static void launch_splitk_finish(const ConvK& k, hipStream_t st) {
  record_mid_event(st);
  const int nbn = (k.Cout + 63) / 64;
  const long long t128 = ((k.M + 127) / 128) * nbn;
  if (t128 >= 512) hipLaunchKernelGGL((conv_splitk_finish<T, 128>), dim3((unsigned)t128), dim3(256), 0, st, k);
  else hipLaunchKernelGGL((conv_splitk_finish<T, 32>), dim3((unsigned)(((k.M + 31) / 32) * nbn)), dim3(256), 0, st, k);
}

int rua_splitk_finish_bf16(const ConvK& k, hipStream_t st) {
  launch_splitk_finish<bf16_t>(k, st);
  RUA_LAUNCH_CHECK("conv_splitk_finish");
  return RUA_OK;
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
// SPEC (conv_dmap_w): 512 threads - waves 0-3 read fragments and multiply, waves 4-7 issue the DMA instructions (each the share wave
// w - 4 issues in the other forms), wait for their landing and meet the consumers at the stage barrier.  A consumer never stands in the
// texture path's issue queue, a producer never holds an MFMA back; after the K loop the producers end and the four consumer waves run
// the epilogue (a barrier counts only the waves of a workgroup that are still alive).
template <int BM, int BN, int ROWB, bool CHAIN = false, bool SPREAD = false, bool SPEC = false>
__device__ __forceinline__ void conv_dmap_body(const ConvK* pk, int nmem) {
  static_assert(!(SPEC && (CHAIN || SPREAD)), "conv_dmap: one issue form at a time");
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
#if defined(RUA_DMAP_DBG_SKIPB)                        // (timing experiments: the DMA INSTRUCTIONS of one operand left out - results are garbage)
  constexpr int PER_STAGE = NSUB * AI;
#elif defined(RUA_DMAP_DBG_SKIPA)
  constexpr int PER_STAGE = NSUB * BI;
#else
  constexpr int PER_STAGE = NSUB * (AI + BI);
#endif
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
  const int tid = threadIdx.x, lane = tid & 63, wid0 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = SPEC && wid0 >= 4;
  const int wid = SPEC ? (wid0 & 3) : wid0;             // consumer w multiplies the tile quarter of wave w, producer w + 4 issues wave w's DMA share
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
#ifdef RUA_DMAP_DBG_A3                                 // timing experiment only (wrong results): the input staged for one tap of three
      ok = ok && (s_taps != 9 || u_tap % 3 == 0);
#endif
#ifdef RUA_DMAP_DBG_A0
      ok = false;
#endif
      atap[i] = ok ? (unsigned)((abase[i] + ex) * 2) : OOB;
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      btap[j] = bv[j] ? (unsigned)(((u_tap * p.Cout + n0 + brow[j]) * s_C + bqv[j]) * 2) : OOB;
#ifdef RUA_DMAP_DBG_B0                                 // timing experiment only: no weight bytes at all
      btap[j] = OOB;
#endif
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
#ifndef RUA_DMAP_DBG_NODMA                             // (timing experiment: the kernel without its staging traffic)
#pragma unroll
    for (int u = 0; u < NSUB; ++u) {
      const unsigned co = (unsigned)(u_chunk * 128 + u * ROWB);            // 64 channels * 2 bytes per stage
#ifndef RUA_DMAP_DBG_SKIPA
#pragma unroll
      for (int i = 0; i < AI; ++i)
        if (part < 0 || ((u * (AI + BI) + i) * 4) / PER_STAGE == part)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sA + (u * BM + (wid * AI + i) * RPI) * ROWB), 16,
                                                   (unsigned)(live ? atap[i] + co : OOB), 0, 0, 0);
#endif
#ifndef RUA_DMAP_DBG_SKIPB
#pragma unroll
      for (int j = 0; j < BI; ++j)
        if (part < 0 || ((u * (AI + BI) + AI + j) * 4) / PER_STAGE == part)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_p)(sB + (u * BN + (wid * BI + j) * RPI) * ROWB), 16,
                                                   (unsigned)(live ? btap[j] + co : OOB), 0, 0, 0);
#endif
    }
#endif
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
  if (SPEC && producer) {                               // ---- the DMA waves: issue, wait for the landing, meet the consumers at the barrier
    issue_next(0);
    issue_next(1);
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PER_STAGE) : "memory");
    __builtin_amdgcn_s_barrier();                       // stage 0 is in LDS
    issue_next(2);
    int pbuf = 0;
    for (int st = 0; st < nst; ++st) {
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PER_STAGE) : "memory");     // stage st + 1 landed (st + 2 stays in flight)
      __builtin_amdgcn_s_barrier();                     // ... and every consumer has read its last fragment of stage st
      issue_next(pbuf);                                 // stage st + 3 into the buffer of stage st
      pbuf = pbuf + 1 == NBUF ? 0 : pbuf + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the zero fills issued past the end of the K range too: the epilogue reuses this LDS
    __builtin_amdgcn_s_barrier();
    return;
  }
  static_assert(!SPREAD || PER_STAGE % 4 == 0, "SPREAD: a stage's DMA instructions split into four equal parts");
  if (!SPEC) {
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b) issue_next(b);
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NBUF - 2) * PER_STAGE) : "memory");
  }
  __builtin_amdgcn_s_barrier();
  if (!SPREAD && !SPEC) issue_next(NBUF - 1);
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
      } else if (SPEC) {                               // the producers waited for stage s + 1; they refill this buffer behind the barrier
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        load_frags(nxt, 0, fa[cur ^ 1], fb[cur ^ 1]);
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
#ifndef RUA_DMAP_DBG_NOMFMA                            // (timing experiment: the staging skeleton alone)
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][a], fb[cur][b], acc[a][b], 0, 0, 0);
#endif
      if (SPREAD) issue_next(buf == 0 ? NBUF - 1 : buf - 1, kk);      // a quarter of stage s + 3 into the buffer stage s - 1 left
    }
    buf = nxt;
    if (CHAIN) {
      if (--c_left == 0) {                              // the member's last stage: its tile leaves, the ring keeps running
        const ConvK& q = pk[cm];
#ifdef RUA_DMAP_DBG_NOEPI                              // (timing experiment: no epilogue at all - results are garbage)
        if (q.M > 0) { if (acc[0][0][0] == 123.456f) q.y[0] = 1; ++cm; if (cm < nmem) c_left = pk[cm].nunits / 2; continue; }
#endif
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
  if (SPEC) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
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
#ifdef RUA_DMAP_DBG_NOEPI
  if (p.M > 0) { if (acc[0][0][0] == 123.456f) p.y[0] = 1; return; }
#endif
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
#ifdef RUA_DMAP_DBG_EPI2                               // (timing experiment: the epilogue run p.ksplit + 2 times - is its cost execution or cold instruction fetch?)
#pragma unroll 1
  for (int rep = 0; rep < p.ksplit + 1; ++rep) { conv_epilogue<T, BM, BN>(p, m0, n0, bm_i, sC, CSTR, sC + BM * CSTR); __syncthreads(); }
#endif
  conv_epilogue_pick<T, BM, BN>(p, m0, n0, bm_i, sC, CSTR, sC + BM * CSTR);
  RUA_TS(6);
}



template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap(const ConvK p) { conv_dmap_body<BM, BN, ROWB>(&p, 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap_g(const ConvKG g) { conv_dmap_body<BM, BN, ROWB>(&g.k[blockIdx.y], 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap_s(const ConvK p) { conv_dmap_body<BM, BN, ROWB, false, true>(&p, 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(256) void conv_dmap_gs(const ConvKG g) { conv_dmap_body<BM, BN, ROWB, false, true>(&g.k[blockIdx.y], 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(512) void conv_dmap_w(const ConvK p) { conv_dmap_body<BM, BN, ROWB, false, false, true>(&p, 1); }
template <int BM, int BN, int ROWB> __global__ __launch_bounds__(512) void conv_dmap_gw(const ConvKG g) { conv_dmap_body<BM, BN, ROWB, false, false, true>(&g.k[blockIdx.y], 1); }
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
struct HaloK {
  ConvK c;
  int d, TH, TW, PT, NS, HPW, HP, nty, ntx, total_sub, rows;     // PT: slots per sub-tile (multiple of 32), rows = NS * PT
  unsigned mHP, mHPW, mPT, mTW;                                  // ceil(2^32 / divisor): x / dv == umulhi(x, m) for x, dv < 2^16, dv > 1
};
__device__ __forceinline__ int fdiv(int x, unsigned m, int dv) { return dv == 1 ? x : (int)__umulhi((unsigned)x, m); }

template <int C, int MAXMT>                           // MAXMT: MFMA row tiles per wave (rows <= MAXMT * 128)
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(C == 64 ? 2 : (MAXMT == 2 ? 4 : 4), C == 64 ? 2 : (MAXMT == 2 ? 6 : 4))))     // = blocks per CU the LDS footprint allows
void conv_halo(const HaloK q) {
  typedef bf16_t T;
  static_assert(C == 32 || C == 64, "conv_halo: C = Cout in {32, 64}");
  constexpr int ROWB = C * 2, SPR = ROWB / 16;        // bytes per LDS pixel row, 16-B slots per row
  constexpr int SW = (C == 32) ? 2 : 1;               // swizzle: slot = piece ^ ((row >> SW) & (SPR - 1)) (conflict-free b128 reads)
  constexpr int CSTR = 32 + 4;                        // a block computes 32 output channels (C = 64: blockIdx.y picks the half)
  constexpr int KST = C / 16;                         // k-steps per tap
  constexpr bool BLDS = (C == 64);                    // weights of the block's 32 output channels: LDS (C = 64) or registers
  constexpr int B_BYTES = BLDS ? 9 * 32 * ROWB : 0;
  const int n0 = BLDS ? blockIdx.y * 32 : 0;
  const ConvK& p = q.c;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sC = reinterpret_cast<float*>(smem);         // aliases the halo images after the MFMA phase
  // fixed carve-up behind the halo / epilogue area (sizes from the launcher): row->pixel table, row->LDS-row table, sub-tile records
  const int halo_b = ((q.NS * q.HP * ROWB + 1023) / 1024) * 1024;
  const int area = 128 * CSTR * 4 > halo_b ? 128 * CSTR * 4 : halo_b;       // the fp32 tile is transposed 128 rows at a time
  unsigned char* sB = smem + area;                     // [9 taps * 32 output channels][C] bf16, swizzled like the halo rows
  int* rowtab = reinterpret_cast<int*>(smem + area + B_BYTES);
  int* subrec = rowtab + q.rows;                      // [NS][4]: n, y0, x0, valid   (halo origin in image coordinates)
  float* sred = reinterpret_cast<float*>(subrec + 4 * 12);

  const int nwg = gridDim.x, bid = blockIdx.x;         // (gridDim.y = output-channel halves)
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
  bf16x8 fb[BLDS ? 1 : 3][BLDS ? 1 : KST];
  const unsigned char* wlane = p.seg[0].w + ((size_t)lr * C + lh * 8) * 2;      // this lane's (cout row, k half) in tap 0
  if constexpr (!BLDS) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int ks = 0; ks < KST; ++ks)
        fb[t][ks] = *reinterpret_cast<const bf16x8*>(wlane + ((size_t)t * C * C + ks * 16) * 2);
  } else {
    // 288 rows (tap, output channel) x 128 B -> LDS by DMA, 8 rows per wave-instruction, same source-side swizzle
    const __amdgpu_buffer_rsrc_t rw_ = make_rsrc(p.seg[0].w, p.seg[0].wbytes);
    for (int it = wid; it < 9 * 32 / 8; it += 4) {
      const int row = it * 8 + (lane >> 3), slot = lane & 7;
      const int t = row >> 5, co = row & 31;
      const unsigned off = (unsigned)((((t * C + n0 + co) * C) + ((slot ^ ((row >> SW) & (SPR - 1))) * 8)) * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw_, (lds_void_p)(sB + it * 1024), 16, off, 0, 0, 0);
    }
  }

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
      bf16x8 fbv;
      if constexpr (BLDS) fbv = *reinterpret_cast<const bf16x8*>(sB + (t * 32 + lr) * ROWB + (((ks * 2 + lh) ^ ((lr >> SW) & (SPR - 1))) * 16));
      else fbv = fb[t % 3][ks];
#pragma unroll
      for (int a = 0; a < MAXMT; ++a)          // unconditional (a branch around MFMAs makes hipcc shuttle the accumulators):
        acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fbv, acc[a], 0, 0, 0);     // a missing row tile computes garbage, never stored
      if constexpr (!BLDS) {
        if (t < 6) fb[t % 3][ks] = *reinterpret_cast<const bf16x8*>(wlane + ((size_t)(t + 3) * C * C + ks * 16) * 2);
      }
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
    conv_epilogue<T, 128, 32>(p, 0, n0, vid, sC, CSTR, sred, rowtab + a * 128, q.rows - a * 128, carry, a == MAXMT - 1);
  }
}

#define RUA_MAX_UNITS 1024
template <typename T, int BM, int BN> static constexpr int conv_smem() { return conv_smem_base<T, BM, BN>() + RUA_MAX_UNITS * 16; }

template <typename T, int BM, int BN> static int launch_conv(const ConvK& k, int nbm, hipStream_t st) {
  static RuaPerDevFlag attr_set_;
  bool& attr_set = attr_set_.get();
  constexpr int smem = conv_smem<T, BM, BN>();
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm<T, BM, BN>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  // split-K invariant: the workspace is all zeros on entry (caller zero-fills it once) and the finisher writes the
  // zeros back after consuming the sums, so no memset is launched per convolution.
  const int smem_now = conv_smem_base<T, BM, BN>() + ((k.nunits * 16 + 255) / 256) * 256;     // unit table sized to this launch
  if (g_conv_group && (g_tune.conv_group & 2) && k.ksplit == 1 && sizeof(T) == 2 && BM == 256 && BN == 64) {           // the C = 64 level's 3x3 convs
    if (!g_conv_group->add(3, (unsigned)(nbm * k.nbn), smem_now, k)) { rua_set_error("rua_conv_fwd_group: more than %d captured members", RUA_MAX_BRANCH); return RUA_ERR_ARG; }
    return RUA_OK;
  }
  hipLaunchKernelGGL((conv_igemm<T, BM, BN>), dim3(nbm * k.nbn * k.ksplit), dim3(256), smem_now, st, k);
  RUA_LAUNCH_CHECK("conv_igemm");
  if (k.ksplit > 1) {
    launch_splitk_finish<T>(k, st);
    RUA_LAUNCH_CHECK("conv_splitk_finish");
  }
  return RUA_OK;
}

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

extern "C" int rua_conv_smem_bytes(const rua_conv_desc* d) {
  const long long M = (long long)d->N * d->H * d->W;
  const int bn = pick_bn(d, M), bm = pick_bm(d, M, bn);
  const bool h = d->dtype == RUA_BF16;
  if (bn == 128) return h ? conv_smem<bf16_t, 128, 128>() : conv_smem<float, 128, 128>();
  if (bm == 256) return bn == 32 ? (h ? conv_smem<bf16_t, 256, 32>() : conv_smem<float, 256, 32>()) : (h ? conv_smem<bf16_t, 256, 64>() : conv_smem<float, 256, 64>());
  return bn == 32 ? (h ? conv_smem<bf16_t, 128, 32>() : conv_smem<float, 128, 32>()) : (h ? conv_smem<bf16_t, 128, 64>() : conv_smem<float, 128, 64>());
}

template <int BM, int BN> static int launch_conv_dma(const ConvK& k, int nbm, hipStream_t st) {
  static RuaPerDevFlag attr_set_;
  bool& attr_set = attr_set_.get();
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dma<BM, BN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              conv_dma_base<BM, BN>());
    attr_set = true;
  }
  const int smem_now = conv_dma_base<BM, BN>();
  hipLaunchKernelGGL((conv_dma<BM, BN>), dim3(nbm * k.nbn * k.ksplit), dim3(256), smem_now, st, k);
  RUA_LAUNCH_CHECK("conv_dma");
  if (k.ksplit > 1) {
    launch_splitk_finish<bf16_t>(k, st);
    RUA_LAUNCH_CHECK("conv_splitk_finish");
  }
  return RUA_OK;
}

template <int BM, int BN, int ROWB> static int launch_conv_dmap(const ConvK& k, hipStream_t st) {
  static RuaPerDevFlag attr_set_;
  bool& attr_set = attr_set_.get();
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dmap<BM, BN, ROWB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              conv_dmap_smem<BM, BN>());
    if constexpr (BM == 128 && ROWB == 64)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dmap_s<BM, BN, ROWB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                conv_dmap_smem<BM, BN, 4>());
    if constexpr (ROWB == 64)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dmap_w<BM, BN, ROWB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                conv_dmap_smem<BM, BN>());
    attr_set = true;
  }
  // DMA waves beside the MFMA waves (conv_dmap_w, 512 threads): the 128-row tiles (2); the 64-row tiles run two blocks per CU that already
  // fill each other's gaps and would lose the second block to the register file (6: measured 0.39 vs 0.33 ms per step on their group launches)
  const bool spec = ROWB == 64 && (g_tune.dmap_spread & 2) && (BM == 128 || (g_tune.dmap_spread & 4));
  const bool spread = BM == 128 && ROWB == 64 && g_tune.dmap_spread == 1; // DMA instructions between the MFMAs of the same waves (four stage buffers)
  const int smem = spread ? conv_dmap_smem<BM, BN, 4>() : conv_dmap_smem<BM, BN>();
  if (g_conv_group && (g_tune.conv_group & (BM == 128 ? 4 : 8)) && k.ksplit == 1 && ROWB == 64) {
    if (!g_conv_group->add(BM == 128 ? (spec ? 4 : spread ? 6 : 1) : (spec ? 5 : 2),     /* capture kinds: 1 / 2 conv_dmap 128- / 64-row tiles, 3 conv_igemm<256,64>, 4 / 5 conv_dmap_w, 6 conv_dmap_s */ (unsigned)(k.nbm * k.nbn), smem, k)) { rua_set_error("rua_conv_fwd_group: more than %d captured members", RUA_MAX_BRANCH); return RUA_ERR_ARG; }
    return RUA_OK;
  }
  if constexpr (ROWB == 64) {
    if (spec) {
      hipLaunchKernelGGL((conv_dmap_w<BM, BN, ROWB>), dim3(k.nbm * k.nbn * k.ksplit), dim3(512), smem, st, k);
      RUA_LAUNCH_CHECK("conv_dmap_w");
      if (k.ksplit > 1 && k.cnt == nullptr) {
        launch_splitk_finish<bf16_t>(k, st);
        RUA_LAUNCH_CHECK("conv_splitk_finish");
      }
      return RUA_OK;
    }
  }
  if constexpr (BM == 128 && ROWB == 64) {
    if (spread) hipLaunchKernelGGL((conv_dmap_s<BM, BN, ROWB>), dim3(k.nbm * k.nbn * k.ksplit), dim3(256), smem, st, k);
    else hipLaunchKernelGGL((conv_dmap<BM, BN, ROWB>), dim3(k.nbm * k.nbn * k.ksplit), dim3(256), smem, st, k);
  } else {
    hipLaunchKernelGGL((conv_dmap<BM, BN, ROWB>), dim3(k.nbm * k.nbn * k.ksplit), dim3(256), smem, st, k);
  }
  RUA_LAUNCH_CHECK("conv_dmap");
  if (k.ksplit > 1 && k.cnt == nullptr) {
    launch_splitk_finish<bf16_t>(k, st);
    RUA_LAUNCH_CHECK("conv_splitk_finish");
  }
  return RUA_OK;
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
struct PwStep { const unsigned char* x; const unsigned char* w; unsigned xbytes, wbytes; int C, kofs, up, Hs, Ws, dense; };
template <int KS> struct PwK { ConvK c; PwStep st[KS]; int px_per_wave, wsh, hsh, nblk; };
// members of a group (rua_conv_fwd_group: the four branch convolutions of the top-level PSPPooling, the per-source data gradients of a concatenating 1x1
// conv): recorded by the launcher, issued as ONE grid (blockIdx.y = member, grids of unequal size) - each was a launch of 8 - 15 us, half of it ramp and drain
struct PwGroupCapture { int n; PwK<2> k[RUA_MAX_BRANCH]; bool dense[RUA_MAX_BRANCH]; };
static thread_local PwGroupCapture* g_pw_group = nullptr;
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
template <int KS> static int launch_conv_pw(const ConvK& k, const rua_conv_desc* d, hipStream_t st) {
  PwK<KS> q;
  q.c = k;
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
  if constexpr (KS == 2) {
    if (g_pw_group && g_pw_group->n < RUA_MAX_BRANCH) {      // a member of a group: recorded, issued by rua_conv_fwd_group
      g_pw_group->dense[g_pw_group->n] = all_dense; g_pw_group->k[g_pw_group->n++] = q;
      return RUA_OK;
    }
  }
  if (all_dense) hipLaunchKernelGGL((conv_pw<KS, true>), dim3(grid), dim3(256), 0, st, q);
  else hipLaunchKernelGGL((conv_pw<KS, false>), dim3(grid), dim3(256), 0, st, q);
  RUA_LAUNCH_CHECK("conv_pw");
  return RUA_OK;
}

// ---- conv_halo launcher -------------------------------------------------------------------------------------------------
static bool pick_halo(const rua_conv_desc* d) {
  const int mode = g_tune.conv_halo;      // 0: off (experiments)
  if (!mode || d->dtype != RUA_BF16 || d->nseg != 1) return false;
  const rua_conv_seg& g = d->seg[0];
  // C = 64: measured against conv_igemm<256,64> on 128x128 maps - d = 1: 28.0 vs 30.3 us, d = 15: 46 vs 29 us (the small
  // lattices leave 192-row blocks at two per CU), so only the small dilations take the halo kernel there
  const int maxd64 = g_tune.halo64_maxd;
  if (g.C == 64 && g.dil > maxd64) return false;
  return g.taps == 9 && g.up_shift == 0 && (g.C == 32 || g.C == 64) && d->Cout == g.C && d->stride == 1 && d->out_stride == 1 &&
         d->OH == d->H && d->OW == d->W && g.Hs == d->H && g.Ws == d->W && d->H >= 16 && d->W >= 16 &&
         (long long)d->N * d->H * d->W >= 65536;
}
static unsigned magic_div(int dv) { return dv <= 1 ? 0u : (unsigned)(((1ull << 32) + dv - 1) / dv); }

// lattice tile TH x TW (slots padded to a multiple of 32) and sub-tiles per block for an H x W map at dilation d:
// minimise padded slots (MFMA waste) with a penalty for halo bytes; at most 384 rows and 40 KiB of halo images per block
static void halo_tiling(int H, int W, int d, int rowb, int* TH_, int* TW_, int* NS_) {
  const int ny = (H + d - 1) / d, nx = (W + d - 1) / d;
  const int lim = 41 * 1024;                           // halo images per block (C = 64: + 36 KiB of weights = 2 blocks per CU)
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

static int launch_conv_halo(const ConvK& k, int dil, hipStream_t st) {
  HaloK q;
  q.c = k;
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
  const int smem = area + (Cc == 64 ? 9 * 32 * 128 : 0) + q.rows * 4 + 4 * 12 * 4 + 4 * 4 * 16 * 4;
  const int blocks = (int)((total + q.NS - 1) / q.NS);
  static RuaPerDevFlag attr2_, attr3_, attr642_, attr643_;
  bool &attr2 = attr2_.get(), &attr3 = attr3_.get(), &attr642 = attr642_.get(), &attr643 = attr643_.get();
  if (Cc == 64) {
    if (q.rows <= 256) {
      if (!attr642) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo<64, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); attr642 = true; }
      hipLaunchKernelGGL((conv_halo<64, 2>), dim3(blocks, 2), dim3(256), smem, st, q);
    } else {
      if (!attr643) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo<64, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); attr643 = true; }
      hipLaunchKernelGGL((conv_halo<64, 3>), dim3(blocks, 2), dim3(256), smem, st, q);
    }
  } else if (q.rows <= 256) {
    if (!attr2) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo<32, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); attr2 = true; }
    hipLaunchKernelGGL((conv_halo<32, 2>), dim3(blocks), dim3(256), smem, st, q);
  } else {
    if (!attr3) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo<32, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); attr3 = true; }
    hipLaunchKernelGGL((conv_halo<32, 3>), dim3(blocks), dim3(256), smem, st, q);
  }
  RUA_LAUNCH_CHECK("conv_halo");
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
// Ablations at 8 x 8 x 1024 (tools/bench_conv_levels.py, -DRUA_IMG_DBG_NOB / NOA; event pair included): 32.6 us; without the weight loads 22.6; without the fragment reads of the
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
#ifdef RUA_IMG_DBG_NOB                                 // (timing experiments - results are garbage: no weight loads in the loop)
      const uint4 bcur = make_uint4(ks, tap, cik, 1);
#else
      const uint4 bcur = bq[u];
#endif
#ifndef RUA_IMG_DBG_NOB
      { const int jn = kk + u + D < nk ? kk + u + D : nk - 1; bq[u] = *reinterpret_cast<const uint4*>(bsrc(kmap(jn))); }
#endif      // unconditional (clamped): the compiler counts the loads in flight exactly, no branch
      const bf16x8 fb = __builtin_bit_cast(bf16x8, bcur);
      const int c16 = 2 * cik + lh;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int hh = ph[t] + dh, ww = pw[t] + dw;
        const bool ok = (unsigned)hh < (unsigned)W && (unsigned)ww < (unsigned)W;
        const int pp = (hh << WSH) + ww;
        const unsigned char* a = ok ? sX + (pp << csh) + ((c16 ^ (pp & 7)) << 4) : sZ;
#ifdef RUA_IMG_DBG_NOA                                 // (no fragment reads from the resident image)
        const bf16x8 fa = __builtin_bit_cast(bf16x8, make_uint4((unsigned)(size_t)a, ok, pp, 3));
#else
        const bf16x8 fa = *reinterpret_cast<const bf16x8*>(a);
#endif
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
static int pick_img(const rua_conv_desc* d) {
  if (!g_tune.conv_img || g_conv_group || d->dtype != RUA_BF16 || d->nseg != 1 || d->in_scale || d->in_fold) return 0;
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
static int launch_conv_img(ConvK& k, const rua_conv_desc* d, int KS, hipStream_t st) {
  k.nbn = d->Cout / 32; k.nbm = d->N; k.ksplit = KS; k.stages_per_split = 0; k.ws = KS > 1 ? (float*)d->workspace : nullptr; k.cnt = nullptr;
  const unsigned grid = (unsigned)(d->N * (d->Cout / 32) * KS);
  static RuaPerDevFlag attr_;
  bool& attr = attr_.get();
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_img<8, 1, 24>), hipFuncAttributeMaxDynamicSharedMemorySize, conv_img_smem<8, 1>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_img<8, 1, 12>), hipFuncAttributeMaxDynamicSharedMemorySize, conv_img_smem<8, 1>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_img<16, 1, 12>), hipFuncAttributeMaxDynamicSharedMemorySize, conv_img_smem<16, 1>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_img<16, 2, 18>), hipFuncAttributeMaxDynamicSharedMemorySize, conv_img_smem<16, 2>());
    attr = true;
  }
  constexpr int s81 = conv_img_smem<8, 1>(), s161 = conv_img_smem<16, 1>(), s162 = conv_img_smem<16, 2>();
  const int nk = 9 * (d->seg[0].C / KS / 16) / 4;        // k-steps per wave: 144 (CS = 1024), 72, 36 (CS = 256) - a multiple of the prefetch depth
  if (d->W == 8 && KS == 1 && nk % 24 == 0) hipLaunchKernelGGL((conv_img<8, 1, 24>), dim3(grid), dim3(256), s81, st, k);
  else if (d->W == 8 && KS == 1) hipLaunchKernelGGL((conv_img<8, 1, 12>), dim3(grid), dim3(256), s81, st, k);
  else if (d->W == 16 && KS == 1) hipLaunchKernelGGL((conv_img<16, 1, 12>), dim3(grid), dim3(256), s161, st, k);
  else if (d->W == 16 && KS == 2) hipLaunchKernelGGL((conv_img<16, 2, 18>), dim3(grid), dim3(256), s162, st, k);
  else { rua_set_error("conv_img: no instantiation for W=%d KS=%d", d->W, KS); return RUA_ERR_ARG; }
  RUA_LAUNCH_CHECK("conv_img");
  if (KS > 1) { launch_splitk_finish<bf16_t>(k, st); RUA_LAUNCH_CHECK("conv_splitk_finish"); }
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

static int dispatch_conv_dma(const ConvK& k, int bm, int bn, int nbm, hipStream_t st) {
  if (bn == 128) return launch_conv_dma<128, 128>(k, nbm, st);
  if (bm == 256) return bn == 32 ? launch_conv_dma<256, 32>(k, nbm, st) : launch_conv_dma<256, 64>(k, nbm, st);
  return bn == 32 ? launch_conv_dma<128, 32>(k, nbm, st) : launch_conv_dma<128, 64>(k, nbm, st);
}

template <typename T> static int dispatch_conv(const ConvK& k, int bm, int bn, int nbm, hipStream_t st) {
  if (bn == 128) return launch_conv<T, 128, 128>(k, nbm, st);
  if (bm == 256) return bn == 32 ? launch_conv<T, 256, 32>(k, nbm, st) : launch_conv<T, 256, 64>(k, nbm, st);
  return bn == 32 ? launch_conv<T, 128, 32>(k, nbm, st) : launch_conv<T, 128, 64>(k, nbm, st);
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
static int launch_conv_small(ConvK& k, hipStream_t st) {
  k.nbm = (int)((k.M + 31) / 32); k.nbn = (k.Cout + 63) / 64;
  k.ksplit = 1; k.stages_per_split = 0; k.ws = nullptr; k.cnt = nullptr;
  constexpr int smem = (4 * 32 * 68 + 4 * 8 * 16) * 4;
  if (g_conv_group && (g_tune.conv_group & 16)) {       // capture mode: issued by rua_conv_fwd_group, side by side with its siblings
    if (!g_conv_group->add(7, (unsigned)(k.nbm * k.nbn), smem, k)) { rua_set_error("rua_conv_fwd_group: more than %d captured members", RUA_MAX_BRANCH); return RUA_ERR_ARG; }
    return RUA_OK;
  }
  hipLaunchKernelGGL((conv_small<2>), dim3(k.nbm * k.nbn), dim3(256), smem, st, k);
  RUA_LAUNCH_CHECK("conv_small");
  return RUA_OK;
}

static thread_local int g_last_ksplit = 1;
extern "C" int rua_conv_last_ksplit(void) { return g_last_ksplit; }    // K slices of this thread's latest rua_conv_fwd launch (1: no finisher ran)

extern "C" int rua_conv_fwd(const rua_conv_desc* d, void* stream) {
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
  ConvK k;
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
  hipStream_t st = (hipStream_t)stream;
  if (rua_pick_strip(d)) {
    k.nbn = 1; k.nbm = 1; k.ksplit = 1; k.stages_per_split = 0; k.ws = nullptr; k.cnt = nullptr;
    g_last_ksplit = 1;
    return rua_launch_conv_strip(k, d, st);
  }
  RUA_CHECK_ARG(d->in_scale == nullptr && d->in_fold == nullptr, "rua_conv_fwd: in_scale / in_shift / in_fold (normalise on load) is not available for "
                                        "this shape: ask rua_conv_fused_input_ok() first");
  if (pick_halo(d)) {
    k.nbn = 1; k.nbm = 1; k.ksplit = 1; k.stages_per_split = 0; k.ws = nullptr; k.cnt = nullptr;
    g_last_ksplit = 1;
    return launch_conv_halo(k, d->seg[0].dil, st);
  }
  if (pick_pw(d)) {
    k.nbn = 1; k.nbm = 1; k.ksplit = 1; k.stages_per_split = 0; k.ws = nullptr; k.cnt = nullptr;
    g_last_ksplit = 1;
    const int ks = pw_steps(d);
    return ks <= 2 ? launch_conv_pw<2>(k, d, st) : ks <= 4 ? launch_conv_pw<4>(k, d, st) : launch_conv_pw<6>(k, d, st);
  }
  if (pick_small(d)) {
    g_last_ksplit = 1;
    return launch_conv_small(k, st);
  }
  if (const int img2_ks = rua_pick_img2(d)) {                // the two deepest levels (round 5, conv_img2.hip)
    g_last_ksplit = img2_ks;
    return rua_launch_conv_img2(k, d, img2_ks, st);
  }
  if (!g_conv_group && rua_band128_sum_ok(d)) {              // several 3x3 segments at C = 128 / 256 (the summed second convolutions of levels 3 - 4): conv_band128m, the sum on chip
    g_last_ksplit = 1;
    return rua_launch_band128_sum(d, st);
  }
  if (const int img_ks = pick_img(d)) {
    g_last_ksplit = img_ks;
    return launch_conv_img(k, d, img_ks, st);
  }
  if (pick_dmap(d)) {
    // 128 x 128 tiles; split K until the grid covers the chip once (every level of the reference network then runs
    // 256 blocks of >= 18 stages: one block per CU, no tail)
    const int target = g_tune.dmap_target > 0 ? g_tune.dmap_target : rua_cu_count();      // one block per CU
    k.nbn = (d->Cout + 127) / 128;
    k.nbm = (int)((k.M + 127) / 128);
    const int nstages = units / 2;
    const long long tiles = (long long)k.nbm * k.nbn;
    int want = 1;
    // the last 4 KiB of the workspace hold the tile ticket counters of the in-launch reduction (zero between launches:
    // the caller zero-fills the workspace once, every last arriver resets its counter)
    // OFF by default - measured: the single last-arriving block reads ksplit x 64 KB of slabs serially (8x8 level: 45 vs 26 us,
    // 16x16: 39 vs 28 us); the separate finisher spreads the same bytes over 1024 blocks.  Kept (and tested) as an option.
    const int fused = g_tune.dmap_fused_finish;
    const size_t ws_usable = d->workspace_bytes > 4096 ? (size_t)d->workspace_bytes - 4096 : 0;
    const long long slabs = d->workspace ? (long long)(ws_usable / ((size_t)k.M * d->Cout * sizeof(float))) : 0;
    k.cnt = (fused && d->workspace && tiles <= 1024) ? reinterpret_cast<int*>((char*)d->workspace + ws_usable) : nullptr;
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
    k.ws = (float*)d->workspace;
    k.stages_per_split = (nstages + want - 1) / want;
    k.ksplit = (nstages + k.stages_per_split - 1) / k.stages_per_split;
    g_last_ksplit = k.ksplit;
    const int rowb = g_tune.dmap_rowb == 128 ? 128 : 64;
    // the unsplit half-chip case (32x32 level: 128 tiles of 128 x 128, 36 stages): 64-row tiles put a block on every CU
    // (measured there: 25.5 / 23.7 / 22.6 us vs 30.1 / 30.0 / 28.6 for d = 1 / d = 15 / plain)
    const int bm64 = g_tune.dmap_bm64;
    // (the members of a grouped launch fill the chip together: 3 x 128 tiles of 128 x 128 need no 64-row tiles, which stage
    //  50 % more bytes per FLOP; tuning key dmap_group_bm128)
    const bool group_fills = g_tune.dmap_group_bm128 && g_conv_group && (g_tune.conv_group & 4) && (long long)g_conv_group->members * tiles >= target;
    // (dmap_bm64 & 2, experiment: the members of a group whose 128-row tiles fill the chip exactly once take 64-row tiles too - two blocks
    //  per CU, one in its epilogue while the other multiplies)
    const bool group64 = (bm64 & 2) && g_conv_group && k.ksplit == 1 && tiles == target;
    if (((bm64 & 1) && k.ksplit == 1 && tiles < target && tiles * 2 >= target && !group_fills) || group64) {
      k.nbm = (int)((k.M + 63) / 64);
      return launch_conv_dmap<64, 128, 64>(k, st);
    }
    return rowb == 128 ? launch_conv_dmap<128, 128, 128>(k, st) : launch_conv_dmap<128, 128, 64>(k, st);
  }
  const int bn = pick_bn(d, k.M);
  int bm = pick_bm(d, k.M, bn);
  k.nbn = (d->Cout + bn - 1) / bn;
  int nbm = (int)((k.M + bm - 1) / bm);
  k.nbm = nbm;
  const int nstages = (units + 1) / 2;
  k.ws = (float*)d->workspace;
  k.cnt = nullptr;
  k.ksplit = (d->workspace && bm == 128) ? pick_ksplit((long long)nbm * k.nbn, nstages, k.M, d->Cout,
                                                       d->workspace_bytes > 4096 ? (size_t)d->workspace_bytes - 4096 : 0) : 1;
  k.stages_per_split = (nstages + k.ksplit - 1) / k.ksplit;
  k.ksplit = (nstages + k.stages_per_split - 1) / k.stages_per_split;
  g_last_ksplit = k.ksplit;
  // Kernel choice (measured per level, scratch/bench_conv.py): the LDS-DMA kernel wins where K is long and the grid is
  // small (Cout >= 128: 5-12 %); the register-staged kernel wins on the two top levels (short K, occupancy-bound) and,
  // with 128-wide tiles, on the very long K of the multi-branch convs at Cout >= 256.
  if (pick_dma(d, bn)) return dispatch_conv_dma(k, bm, bn, nbm, st);
  if (d->dtype == RUA_BF16) return dispatch_conv<bf16_t>(k, bm, bn, nbm, st);
  return dispatch_conv<float>(k, bm, bn, nbm, st);
}

// ---- grouped launch --------------------------------------------------------------------------------------------------
// rua_conv_fwd_group: n INDEPENDENT convolutions (the dilation branches of a ResBlock: model2.py:26-31).  Every member goes
// through rua_conv_fwd's own dispatch with the launchers in capture mode; members that land on the same kernel with the same
// grid are then issued as ONE grid (blockIdx.y = member), the rest one by one.  Results are those of n separate calls.
thread_local ConvGroupCapture* g_conv_group = nullptr;
static thread_local int g_group_last_grids = 0;
static thread_local int g_group_last_band = 0;
extern "C" int rua_conv_group_last_grids(void) { return g_group_last_grids; }
static thread_local int g_group_last_chain = 0;
extern "C" int rua_conv_group_last_chain(void) { return g_group_last_chain; }    // members the latest rua_conv_fwd_group ran back to back inside one conv_dmap_chain grid (0: none)
extern "C" int rua_conv_group_last_band(void) { return g_group_last_band; }      // 1: the calling thread's latest rua_conv_fwd_group ran as one conv_band64m launch
// would rua_conv_fwd_group run these members as one conv_band64m launch (which honours in_fold / in_scale of every member)?
extern "C" int rua_conv_group_band_ok(const rua_conv_desc* d, int n) { return (d && (rua_band64m_ok(d, n) || rua_band128m_ok(d, n))) ? 1 : 0; }   // grids the calling thread's latest rua_conv_fwd_group issued (1: one grid for all members)

template <typename KG, typename F1, typename FG>
static int issue_group(const ConvGroupCapture& c, const int* idx, int m, F1 single, FG grouped, int smem_attr, hipStream_t st, const char* what, int threads = 256) {
  if (m == 1) {
    hipLaunchKernelGGL(single, dim3(c.grid[idx[0]]), dim3(threads), c.smem[idx[0]], st, c.k[idx[0]]);
  } else {
    static RuaPerDevFlag attr[8];                        // per device, not per thread (the instantiations of this template are per kernel pair)
    const int slot = c.kind[idx[0]];
    if (!attr[slot].get()) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(grouped), hipFuncAttributeMaxDynamicSharedMemorySize, smem_attr); attr[slot].get() = true; }
    KG g;
    for (int i = 0; i < m; ++i) g.k[i] = c.k[idx[i]];
    hipLaunchKernelGGL(grouped, dim3(c.grid[idx[0]], m), dim3(threads), c.smem[idx[0]], st, g);
  }
  RUA_LAUNCH_CHECK(what);
  return RUA_OK;
}

// conv_dmap_chain: the captured conv_dmap members as ONE grid of the members' common size, every block walking all of them
static bool chain_ok(const ConvGroupCapture& c, const int* idx, int m) {
  const ConvK& a = c.k[idx[0]];
  for (int i = 0; i < m; ++i) {
    const ConvK& k = c.k[idx[i]];
    if (k.ksplit != 1 || k.M != a.M || k.Cout != a.Cout || k.nbm != a.nbm || k.nbn != a.nbn || k.H != a.H || k.W != a.W || k.stride != a.stride) return false;
  }
  return true;
}
template <typename FC>
static int issue_chain(const ConvGroupCapture& c, const int* idx, int m, FC kern, int smem, int slot, hipStream_t st) {
  static RuaPerDevFlag attr[2];
  if (!attr[slot].get()) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem); attr[slot].get() = true; }
  ConvKG g;
  for (int i = 0; i < m; ++i) g.k[i] = c.k[idx[i]];
  hipLaunchKernelGGL(kern, dim3(c.grid[idx[0]]), dim3(256), smem, st, g, m);
  RUA_LAUNCH_CHECK("conv_dmap_chain");
  return RUA_OK;
}

extern "C" int rua_conv_fwd_group(const rua_conv_desc* d, int n, void* stream) {
  RUA_CHECK_ARG(d && n >= 1 && n <= RUA_MAX_BRANCH, "rua_conv_fwd_group: 1..%d members", RUA_MAX_BRANCH);
  hipStream_t st = (hipStream_t)stream;
  g_group_last_grids = n;
  g_group_last_band = 0;
  g_group_last_chain = 0;
  if (n >= 2 && rua_band128m_ok(d, n)) {                    // C = 128 / C = 64 on whole rows: two-row stages, weights of a kernel row in registers (conv_band128.hip)
    const int rc = rua_launch_band128m(d, n, st);
    if (rc == RUA_OK) { g_group_last_grids = 1; g_group_last_band = 2; }
    return rc;
  }
  if (rua_band64m_ok(d, n)) {                               // the C = 64 level, round-3 form: one row-streaming launch for all members (conv_band64.hip)
    const int rc = rua_launch_band64m(d, n, st);
    if (rc == RUA_OK) { g_group_last_grids = 1; g_group_last_band = 1; }
    return rc;
  }
  if (n == 1 || !g_tune.conv_group) {
    for (int i = 0; i < n; ++i) { const int rc = rua_conv_fwd(d + i, stream); if (rc != RUA_OK) return rc; }
    return RUA_OK;
  }
  ConvGroupCapture cap;
  cap.n = 0;
  cap.members = n;
  PwGroupCapture pwc;
  pwc.n = 0;
  rua_strip_group_reset();                                  // nothing stale from a group that failed half-way
  g_conv_group = &cap;
  g_pw_group = (g_tune.conv_group & 32) ? &pwc : nullptr;
  int rc = RUA_OK;
  for (int i = 0; i < n && rc == RUA_OK; ++i) rc = rua_conv_fwd(d + i, stream);      // non-groupable members launch right here
  g_conv_group = nullptr;
  g_pw_group = nullptr;
  if (rc != RUA_OK) { rua_strip_group_reset(); return rc; }  // captured members are dropped, not issued by the next group
  int grids = n - cap.n - pwc.n - rua_strip_group_pending();        // members no launcher captured were launched one by one above
  for (int dense = 0; dense < 2; ++dense) {                 // conv_pw members: one grid per addressing form
    PwKG<2> g; int m = 0; unsigned gx = 0;
    for (int i = 0; i < pwc.n; ++i) if ((int)pwc.dense[i] == dense) { g.k[m++] = pwc.k[i]; if ((unsigned)pwc.k[i].nblk > gx) gx = (unsigned)pwc.k[i].nblk; }
    if (m == 0) continue;
    for (int i = m; i < RUA_MAX_BRANCH; ++i) g.k[i] = g.k[0];
    if (m == 1) { if (dense) hipLaunchKernelGGL((conv_pw<2, true>), dim3(gx), dim3(256), 0, st, g.k[0]); else hipLaunchKernelGGL((conv_pw<2, false>), dim3(gx), dim3(256), 0, st, g.k[0]); }
    else if (dense) hipLaunchKernelGGL((conv_pw_g<2, true>), dim3(gx, m), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((conv_pw_g<2, false>), dim3(gx, m), dim3(256), 0, st, g);
    RUA_LAUNCH_CHECK("conv_pw (group)");
    ++grids;
  }
  rc = rua_strip_group_flush(st, &grids);
  if (rc != RUA_OK) return rc;
  bool done[RUA_MAX_BRANCH] = {false};
  for (int i = 0; i < cap.n; ++i) {
    if (done[i]) continue;
    int idx[RUA_MAX_BRANCH], m = 0;
    if (cap.kind[i] == 7) {                                 // conv_small: members of unequal grids share one launch (the grid of the largest)
      unsigned gmax = 0;
      for (int j = i; j < cap.n; ++j)
        if (!done[j] && cap.kind[j] == 7) { idx[m++] = j; done[j] = true; if (cap.grid[j] > gmax) gmax = cap.grid[j]; }
      if (m == 1) hipLaunchKernelGGL((conv_small<2>), dim3(cap.grid[idx[0]]), dim3(256), cap.smem[idx[0]], st, cap.k[idx[0]]);
      else { ConvKG g; for (int q = 0; q < m; ++q) g.k[q] = cap.k[idx[q]]; hipLaunchKernelGGL((conv_small_g<2>), dim3(gmax, m), dim3(256), cap.smem[idx[0]], st, g); }
      RUA_LAUNCH_CHECK("conv_small (group)");
      ++grids;
      continue;
    }
    for (int j = i; j < cap.n; ++j)
      if (!done[j] && cap.kind[j] == cap.kind[i] && cap.grid[j] == cap.grid[i] && cap.smem[j] == cap.smem[i]) { idx[m++] = j; done[j] = true; }
    const bool chain = m >= 2 && (cap.kind[i] == 1 || cap.kind[i] == 2) && (g_tune.dmap_chain & cap.kind[i]) && chain_ok(cap, idx, m);
    if (chain) g_group_last_chain = m;
    if (chain && cap.kind[i] == 1) rc = issue_chain(cap, idx, m, conv_dmap_chain<128, 128, 64>, conv_dmap_chain_smem<128, 128>(), 0, st);
    else if (chain) rc = issue_chain(cap, idx, m, conv_dmap_chain<64, 128, 64>, conv_dmap_chain_smem<64, 128>(), 1, st);
    else if (cap.kind[i] == 1) rc = issue_group<ConvKG>(cap, idx, m, conv_dmap<128, 128, 64>, conv_dmap_g<128, 128, 64>, conv_dmap_smem<128, 128>(), st, "conv_dmap (group)");
    else if (cap.kind[i] == 4) rc = issue_group<ConvKG>(cap, idx, m, conv_dmap_w<128, 128, 64>, conv_dmap_gw<128, 128, 64>, conv_dmap_smem<128, 128>(), st, "conv_dmap_w (group)", 512);
    else if (cap.kind[i] == 5) rc = issue_group<ConvKG>(cap, idx, m, conv_dmap_w<64, 128, 64>, conv_dmap_gw<64, 128, 64>, conv_dmap_smem<64, 128>(), st, "conv_dmap_w (group)", 512);
    else if (cap.kind[i] == 6) rc = issue_group<ConvKG>(cap, idx, m, conv_dmap_s<128, 128, 64>, conv_dmap_gs<128, 128, 64>, conv_dmap_smem<128, 128, 4>(), st, "conv_dmap_s (group)");
    else if (cap.kind[i] == 2) rc = issue_group<ConvKG>(cap, idx, m, conv_dmap<64, 128, 64>, conv_dmap_g<64, 128, 64>, conv_dmap_smem<64, 128>(), st, "conv_dmap (group)");
    else rc = issue_group<ConvKG>(cap, idx, m, conv_igemm<bf16_t, 256, 64>, conv_igemm_g<bf16_t, 256, 64>, conv_smem<bf16_t, 256, 64>(), st, "conv_igemm (group)");
    if (rc != RUA_OK) return rc;
    ++grids;
  }
  g_group_last_grids = grids;
  return RUA_OK;
}

// =========================================================================================
// Weight gradient: dW[t][co][c] += sum_pix dy[pix][co] * a[src(pix,t)][c]
// GEMM rows = co, cols = c, K = pixels.  Both operands are pixel-major in HBM, so the K index is
// the LDS row: bf16 fragments are gathered with the transposing LDS read (ds_read_b64_tr_b16),
// fp32 fragments (32x32x2 MFMA) are single dwords.  Split over pixels across blocks, fp32 atomics.
struct WgK {
  const unsigned char* a; const unsigned char* dy; float* dw;
  int C, Hs, Ws, Cout, H, W, N, stride, dil, taps;
  long long M; int pix_per_block, ntc, nti, ksplit;
  int wshift, hshift;      // log2(W), log2(H) when both are powers of two, else -1 (generic division path)
  float* slabs;            // K split: slice ks stores its partial dW into slabs[ks * taps * Cout * C ..] (plain stores; summed in a
                           // fixed order by wgrad_slab_reduce: bit-reproducible); null: fp32 atomics into dw
  const int* overwrite;    // ksplit == 1: a device flag - non-zero: dw = acc instead of dw += acc (rua_wgrad_desc.overwrite_dev: dw is zero and has no other writer)
};

template <typename T>
__device__ __forceinline__ void wgrad_kernel_body(const WgK& p, int b) {
  constexpr int VEC = ET<T>::VEC, ES = sizeof(T);
  constexpr int TP = 64;                         // pixels per stage
  constexpr int PPR = 64 / VEC;                  // pieces per 64-channel row
  constexpr int ROWB = (ES == 2) ? 192 : 260;    // 64 ch + pad (bank-conflict-free tr reads / b32 reads)
  constexpr int PASS = TP * PPR / 256;           // bf16: 2, f32: 4
  __shared__ __attribute__((aligned(16))) unsigned char sD[TP * ROWB];   // dy tile  [pix][co]
  __shared__ __attribute__((aligned(16))) unsigned char sX[TP * ROWB];   // a  tile  [pix][ci]

  const int ks = b % p.ksplit; b /= p.ksplit;
  const int ti = b % p.nti; b /= p.nti;
  const int tc = b % p.ntc; b /= p.ntc;
  const int tap = b;
  const int co0 = tc * 64, ci0 = ti * 64;
  int dh = 0, dw = 0;
  if (p.taps == 9) { dh = (tap / 3 - 1) * p.dil; dw = (tap % 3 - 1) * p.dil; }

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int pq = tid % PPR, pr = tid / PPR;      // piece column / row within pass
  constexpr int RPP = 256 / PPR;
  const int HW = p.H * p.W;
  const long long k_begin = (long long)ks * p.pix_per_block;
  long long k_end = k_begin + p.pix_per_block;
  if (k_end > p.M) k_end = p.M;

  const int wr = wid >> 1, wc = wid & 1;         // wave -> 32x32 tile (co half, ci half)
  const bool active = (co0 + wr * 32 < p.Cout) && (ci0 + wc * 32 < p.C);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  const int lr = lane & 31, lh = lane >> 5;

  uint4 rd[PASS], rx[PASS];
  const int co_t = co0 + pq * VEC, ci_t = ci0 + pq * VEC;
  const bool cok = co_t < p.Cout, xok = ci_t < p.C;
  const int kend32 = (int)k_end;
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(p.dy, (unsigned)((size_t)p.M * p.Cout * ES));
  const __amdgpu_buffer_rsrc_t rxa = make_rsrc(p.a, (unsigned)((size_t)p.N * p.Hs * p.Ws * p.C * ES));
  auto load_stage = [&](long long k0) {
#pragma unroll
    for (int i = 0; i < PASS; ++i) {
      const int mm = (int)k0 + pr + i * RPP;
      const bool in = mm < kend32;
      int n, h, w;
      if (p.wshift >= 0) { w = mm & (p.W - 1); h = (mm >> p.wshift) & (p.H - 1); n = mm >> (p.wshift + p.hshift); }
      else { n = mm / HW; const int rem = mm - n * HW; h = rem / p.W; w = rem - h * p.W; }
      const int hs = h * p.stride + dh, ws = w * p.stride + dw;
      const bool inx = in && xok && (unsigned)hs < (unsigned)p.Hs && (unsigned)ws < (unsigned)p.Ws;
      rd[i] = bufload16(rdy, (in && cok) ? (unsigned)((mm * p.Cout + co_t) * ES) : RUA_OOB);
      rx[i] = bufload16(rxa, inx ? (unsigned)((((n * p.Hs + hs) * p.Ws + ws) * p.C + ci_t) * ES) : RUA_OOB);
    }
  };
  auto write_stage = [&]() {
#pragma unroll
    for (int i = 0; i < PASS; ++i) {
      const int row = pr + i * RPP;
      if constexpr (ES == 2) {
        *reinterpret_cast<uint4*>(sD + row * ROWB + pq * 16) = rd[i];
        *reinterpret_cast<uint4*>(sX + row * ROWB + pq * 16) = rx[i];
      } else {
        uint32_t* d = reinterpret_cast<uint32_t*>(sD + row * ROWB + pq * 16);
        d[0] = rd[i].x; d[1] = rd[i].y; d[2] = rd[i].z; d[3] = rd[i].w;
        uint32_t* x = reinterpret_cast<uint32_t*>(sX + row * ROWB + pq * 16);
        x[0] = rx[i].x; x[1] = rx[i].y; x[2] = rx[i].z; x[3] = rx[i].w;
      }
    }
  };

  if (k_begin < k_end) load_stage(k_begin);
  for (long long k0 = k_begin; k0 < k_end; k0 += TP) {
    __syncthreads();
    write_stage();
    __syncthreads();
    if (k0 + TP < k_end) load_stage(k0 + TP);
    if (active) {
      if constexpr (ES == 2) {
        // transposing read: 16-lane group g reads a 4(pixel) x 16(channel) block; lane 4q+p of the
        // group addresses row q, channels 4p..4p+3; lane i receives channel i of the 4 pixels.
        const int li = lane & 15, g = lane >> 4;
        const int q = li >> 2, pp = li & 3;
        const int chan = 16 * (g & 1) + 4 * pp;        // channel offset inside the wave's 32
        const int hrow = 8 * (g >> 1) + q;             // pixel row inside the 16-pixel k-step
#pragma unroll
        for (int kk = 0; kk < TP / 16; ++kk) {
          const unsigned char* ad = sD + (kk * 16 + hrow) * ROWB + (wr * 32 + chan) * 2;
          const unsigned char* ax = sX + (kk * 16 + hrow) * ROWB + (wc * 32 + chan) * 2;
          typedef s16x4 __attribute__((address_space(3))) * lds4;
          const s16x4 d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ad));
          const s16x4 d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ad + 4 * ROWB));
          const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ax));
          const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ax + 4 * ROWB));
          typedef __attribute__((ext_vector_type(8))) short s16x8;
          const s16x8 fa = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
          const s16x8 fb = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa), __builtin_bit_cast(bf16x8, fb), acc, 0, 0, 0);
        }
      } else {
#pragma unroll 8
        for (int kk = 0; kk < TP / 2; ++kk) {
          const float fa = *reinterpret_cast<const float*>(sD + (kk * 2 + lh) * ROWB + (wr * 32 + lr) * 4);
          const float fb = *reinterpret_cast<const float*>(sX + (kk * 2 + lh) * ROWB + (wc * 32 + lr) * 4);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc, 0, 0, 0);
        }
      }
    }
  }
  if (active) {
    const int ci = ci0 + wc * 32 + lr;
    const bool ow = p.ksplit == 1 && p.overwrite && *p.overwrite != 0;
    if (ci < p.C) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = co0 + wr * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
        if (co < p.Cout) {
          float* dst = &p.dw[((size_t)tap * p.Cout + co) * p.C + ci];
          // one K slice = one writer per element: a plain read-modify-write (float atomics run at ~1.3 TB/s chip-wide,
          // plain traffic at ~6; the 8x8 level writes its whole 37.7 MB gradient this way)
          if (p.ksplit == 1) { if (ow) *dst = acc[i]; else *dst += acc[i]; }
          else if (p.slabs) p.slabs[(size_t)ks * p.taps * p.Cout * p.C + ((size_t)tap * p.Cout + co) * p.C + ci] = acc[i];
          else unsafeAtomicAdd(dst, acc[i]);
        }
      }
    }
  }
}
template <typename T> __global__ __launch_bounds__(256) void wgrad_kernel(const WgK p) { wgrad_kernel_body<T>(p, (int)blockIdx.x); }
// grouped launch (rua_conv_wgrad_group): the weight gradients of the dilation branches of a ResBlock in ONE grid; blockIdx.y picks
// the member, blocks beyond a member's own grid leave at once
struct WgKG { WgK k[RUA_MAX_WGRAD_GROUP]; };
static_assert(sizeof(WgKG) <= 4096, "grouped launch: kernel arguments are limited to 4 KiB");
__global__ __launch_bounds__(256) void wgrad_kernel_g(const WgKG g) {
  const WgK& p = g.k[blockIdx.y];
  if ((long long)blockIdx.x >= (long long)p.ntc * p.nti * p.taps * p.ksplit) return;
  wgrad_kernel_body<bf16_t>(p, (int)blockIdx.x);
}
// batched launch (rua_conv_wgrad_group, members with rua_wgrad_desc.batch set that all land on this kernel): UNEQUAL weight gradients - a step's wide 1x1 convolutions on
// small maps - in one COMPACT grid: exactly the sum of the members' blocks, longest blocks first.  end[i] = first block behind member i (prefix sums, in the
// kernel arguments): a block finds its member by scalar compares, no division
struct WgKB { WgK k[RUA_MAX_WGRAD_BATCH]; unsigned end[RUA_MAX_WGRAD_BATCH]; int n; };
static_assert(sizeof(WgKB) <= 4096, "batched launch: kernel arguments are limited to 4 KiB");
__global__ __launch_bounds__(256) void wgrad_kernel_b(const WgKB g) {
  const unsigned b = blockIdx.x;
  int m = 0;
  for (int i = 0; i + 1 < g.n; ++i) m += (b >= g.end[i]) ? 1 : 0;
  const unsigned first = m ? g.end[m - 1] : 0u;
  wgrad_kernel_body<bf16_t>(g.k[m], (int)(b - first));
}

// dw += sum of the K slices' slabs, in a FIXED order (bit-reproducible).  A thread owns one float4 column and walks the slices
// eight loads at a time: a wave reads 1 KiB runs of every slab, nothing is exchanged.  (Before: 16 columns x 16 slice lanes per
// block folded through LDS - 256-byte runs and 40x the blocks; the batched reduction of a step took 287 us for 1.04 GB.)
constexpr int SLAB_RED_COLS = 256;                      // float4 columns per block
__device__ __forceinline__ void wgrad_slab_reduce_body(const float* __restrict__ slabs, float* __restrict__ dw, long long n4, int ksplit, int vblock, int overwrite = 0) {
  const long long i = (long long)vblock * SLAB_RED_COLS + threadIdx.x;
  if (i >= n4) return;
  const float4* s = reinterpret_cast<const float4*>(slabs) + i;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  auto add4 = [](float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; };
  int k = 0;
  for (; k + 8 <= ksplit; k += 8) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = s[(size_t)(k + u) * n4];
    float4 a = v[0], b = v[4];
    add4(a, v[1]); add4(b, v[5]); add4(a, v[2]); add4(b, v[6]); add4(a, v[3]); add4(b, v[7]);
    add4(a, b); add4(t, a);
  }
  for (; k < ksplit; ++k) add4(t, s[(size_t)k * n4]);
  float4* d = reinterpret_cast<float4*>(dw) + i;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!overwrite) o = *d;                               // (overwrite: dw holds zeros and has no other writer - the read is spared, the sum the same)
  add4(o, t);
  *d = o;
}
__global__ __launch_bounds__(256) void wgrad_slab_reduce(const float* __restrict__ slabs, float* __restrict__ dw, long long n4, int ksplit) {
  wgrad_slab_reduce_body(slabs, dw, n4, ksplit, (int)blockIdx.x);
}
static int launch_slab_reduce(const float* slabs, float* dw, long long n, int ksplit, hipStream_t st) {
  const long long n4 = n / 4;
  hipLaunchKernelGGL(wgrad_slab_reduce, dim3((unsigned)((n4 + SLAB_RED_COLS - 1) / SLAB_RED_COLS)), dim3(256), 0, st, slabs, dw, n4, ksplit);
  RUA_LAUNCH_CHECK("wgrad_slab_reduce");
  return RUA_OK;
}
// K slices that fit the caller's workspace as fp32 slabs (the last WG_PW_TAIL bytes belong to wgrad_pw); 1: no room
static int slab_capacity(const rua_wgrad_desc* d, long long ndw);

// =========================================================================================
// wgrad_dmap: the weight gradient of the wide levels (C, Cout multiples of 128, bf16, stride 1, power-of-two maps) on the
// conv_dmap structure.  wgrad_kernel's 64x64 tiles (32x32 per wave: four LDS reads per MFMA, 0.031 staged bytes per FLOP,
// one barrier per 4 MFMAs) are bound by the L2->LDS staging rate like every implicit GEMM here; this one uses 128 (co) x
// 128 (ci) tiles with 64x64 wave tiles (two transposing LDS reads per MFMA, half the staged bytes), 64-pixel stages filled
// by LDS-DMA into three buffers with a counted vmcnt and ONE barrier per 16 MFMAs, and the fragment prefetch across the
// barrier.  LDS image of a stage: [64 pixels][256 B = 128 channels] for dy and for the (tap-shifted, zero-padded) input; the
// 64-byte quarter of a row is XOR-swizzled with (pixel & 3) - applied to the per-lane SOURCE chunk of the DMA - so that the
// ds_read_b64_tr_b16 fragment reads (4 pixel rows x 64 B per 32-lane group) hit four different bank quarters.
struct WgdK {
  const unsigned char* a; const unsigned char* dy; float* dw;
  int C, Cout, H, W, dil, taps, wsh;
  long long M;
  int ntc, nti, ksplit, stages_per_split;
  unsigned abytes, dybytes;
  float* slabs;            // as in WgK
  int ks_slow;             // block -> (K slice, tap, tile) order, see the kernel
};

// Transposing LDS read that hipcc's wait insertion cannot see (it puts s_waitcnt vmcnt(0) in front of a ds_read_b64_tr_b16
// builtin whenever an LDS-DMA is in flight, which would drain the stage pipeline at every k-step): the caller orders these
// reads itself with counted lgkmcnt waits that name the destination registers.
__device__ __forceinline__ s16x4 lds_tr_raw(const unsigned char* p) {
  s16x4 v;
  const unsigned a = (unsigned)(size_t)(lds_void_p)const_cast<unsigned char*>(p);
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(a) : "memory");
  return v;
}

__device__ __forceinline__ void wgrad_dmap_body(const WgdK& p, const int nwg) {
  constexpr int NBUF = 3, PX = 64, ROWB = 256, KS = 4;
  constexpr int D_BYTES = PX * ROWB, STAGE = 2 * D_BYTES;
  constexpr int PER_STAGE = 8;                                      // DMA instructions per wave per stage (4 dy + 4 a)
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int bid = blockIdx.x;                          // nwg: this weight gradient's own block count (a grouped grid is padded)
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  int vid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  // K slice slowest: the taps x tiles blocks that read the SAME pixels of dy and of the input are neighbours in vid, i.e. run on one
  // XCD and share its L2 (K slice fastest spread them over all eight: every XCD fetched every slice - 94 MB per launch for
  // 8-17 MB of tensors)
  const int ncombo = p.nti * p.ntc * p.taps;
  const int ks_i = p.ks_slow ? vid / ncombo : vid % p.ksplit;
  vid = p.ks_slow ? vid - ks_i * ncombo : vid / p.ksplit;
  const int ti = vid % p.nti; vid /= p.nti;
  const int tc = vid % p.ntc;
  const int tap = vid / p.ntc;
  const int co0 = tc * 128, ci0 = ti * 128;
  int dh = 0, dw_ = 0;
  if (p.taps == 9) { dh = (tap / 3 - 1) * p.dil; dw_ = (tap % 3 - 1) * p.dil; }
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int H = p.H, W = p.W;

  const int st_begin = ks_i * p.stages_per_split;
  const int k_begin = st_begin * PX;                               // pixel indices fit 32 bits (checked by the launcher)
  int k_end = k_begin + p.stages_per_split * PX;
  if (k_end > (int)p.M) k_end = (int)p.M;
  const int nst = k_end > k_begin ? (k_end - k_begin + PX - 1) / PX : 0;

  // DMA geometry of this lane: instruction j of this wave covers pixel rows (wid*4 + j)*4 .. +3 of the stage
  const int rl = lane >> 4, c16 = lane & 15;
  int drow[4], dchan[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    drow[j] = (wid * 4 + j) * 4 + rl;
    dchan[j] = (c16 ^ ((drow[j] & 3) << 2)) * 8;                   // source chunk that lands in LDS slot c16
  }
  const __amdgpu_buffer_rsrc_t rd_ = make_rsrc(p.dy, p.dybytes), ra_ = make_rsrc(p.a, p.abytes);
  const int shift_px = dh * W + dw_;
  int st_next = 0;                                                  // next stage of this block to issue
  auto issue_next = [&](int buf) {
    unsigned char* sD = smem + buf * STAGE;
    unsigned char* sA = sD + D_BYTES;
    const int p0 = k_begin + st_next * PX;                          // past the end of the K range: every pixel >= k_end => zeros
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // branch-free: offsets are computed for every lane and replaced by the out-of-range offset where invalid (a branch
      // here would execute the DMA under a partial exec mask and leave stale LDS bytes instead of zeros)
      const int pi = p0 + drow[j];
      const unsigned offd = (unsigned)((pi * p.Cout + co0 + dchan[j]) * 2);
      const unsigned okd = (unsigned)(pi < k_end);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rd_, (lds_void_p)(sD + (wid * 4 + j) * 1024), 16, okd ? offd : OOB, 0, 0, 0);
      const int w = pi & (W - 1), h = (pi >> p.wsh) & (H - 1);
      const unsigned oka = okd & (unsigned)((unsigned)(h + dh) < (unsigned)H) & (unsigned)((unsigned)(w + dw_) < (unsigned)W);
      const unsigned offa = (unsigned)(((pi + shift_px) * p.C + ci0 + dchan[j]) * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (lds_void_p)(sA + (wid * 4 + j) * 1024), 16, oka ? offa : OOB, 0, 0, 0);
    }
    ++st_next;
  };

  // fragment geometry (transposing reads, see wgrad_kernel): a 32-channel x 16-pixel fragment = two ds_read_b64_tr_b16
  const int wm = wid >> 1, wn = wid & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int li = lane & 15, g = lane >> 4;
  const int q4 = li >> 2, pp = li & 3;
  const int chan = 16 * (g & 1) + 4 * pp;
  const int hrow = 8 * (g >> 1) + q4;
  typedef s16x4 __attribute__((address_space(3))) * lds4;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  unsigned fa_off[2], fb_off[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    fa_off[t] = hrow * ROWB + (((wm * 2 + t) ^ q4) * 64) + chan * 2;             // (row & 3) == q4 for every row this lane reads
    fb_off[t] = D_BYTES + hrow * ROWB + (((wn * 2 + t) ^ q4) * 64) + chan * 2;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  // a fragment set = 8 raw transposing reads (2 co blocks + 2 ci blocks, two 4-pixel-row halves each), in flight until
  // the caller's counted wait
  struct Frags { s16x4 a[2][2], b[2][2]; };
  auto load_frags = [&](int buf, int kk, Frags& f) {
    const unsigned char* sS = smem + buf * STAGE + kk * 16 * ROWB;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f.a[t][0] = lds_tr_raw(sS + fa_off[t]);
      f.a[t][1] = lds_tr_raw(sS + fa_off[t] + 4 * ROWB);
      f.b[t][0] = lds_tr_raw(sS + fb_off[t]);
      f.b[t][1] = lds_tr_raw(sS + fb_off[t] + 4 * ROWB);
    }
  };
#define RUA_FRAG_OPS(f) "+v"(f.a[0][0]), "+v"(f.a[0][1]), "+v"(f.a[1][0]), "+v"(f.a[1][1]), "+v"(f.b[0][0]), "+v"(f.b[0][1]), "+v"(f.b[1][0]), "+v"(f.b[1][1])
  auto mfma_set = [&](const Frags& f) {
#pragma unroll
    for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
      for (int b_ = 0; b_ < 2; ++b_) {
        const s16x8 va = {f.a[a_][0][0], f.a[a_][0][1], f.a[a_][0][2], f.a[a_][0][3], f.a[a_][1][0], f.a[a_][1][1], f.a[a_][1][2], f.a[a_][1][3]};
        const s16x8 vb = {f.b[b_][0][0], f.b[b_][0][1], f.b[b_][0][2], f.b[b_][0][3], f.b[b_][1][0], f.b[b_][1][1], f.b[b_][1][2], f.b[b_][1][3]};
        acc[a_][b_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va), __builtin_bit_cast(bf16x8, vb), acc[a_][b_], 0, 0, 0);
      }
  };

  issue_next(0);
  issue_next(1);
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PER_STAGE) : "memory");
  __builtin_amdgcn_s_barrier();
  issue_next(2);
  Frags f0, f1;
  load_frags(0, 0, f0);
  int buf = 0;
  for (int st = 0; st < nst; ++st) {
    int nxt = buf + 1; if (nxt == NBUF) nxt = 0;
    // k-steps 0..3 alternate between the two fragment sets; the set of k-step kk+1 is requested before the MFMAs of kk
    load_frags(buf, 1, f1);
    asm volatile("s_waitcnt lgkmcnt(8)" : RUA_FRAG_OPS(f0) :: "memory");      // the 8 older reads (f0) have landed
    mfma_set(f0);
    load_frags(buf, 2, f0);
    asm volatile("s_waitcnt lgkmcnt(8)" : RUA_FRAG_OPS(f1) :: "memory");
    mfma_set(f1);
    load_frags(buf, 3, f1);
    asm volatile("s_waitcnt lgkmcnt(8)" : RUA_FRAG_OPS(f0) :: "memory");
    mfma_set(f0);
    // stage st+1 landed (this wave's part), every read of this stage's buffer is complete -> barrier -> refill it
    asm volatile("s_waitcnt vmcnt(%[ps])\n\ts_waitcnt lgkmcnt(0)" : RUA_FRAG_OPS(f1) : [ps] "n"(PER_STAGE) : "memory");
    __builtin_amdgcn_s_barrier();
    issue_next(buf);
    load_frags(nxt, 0, f0);
    mfma_set(f1);
    buf = nxt;
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" : RUA_FRAG_OPS(f0) :: "memory");
#undef RUA_FRAG_OPS
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = co0 + wm * 64 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
        const int ci = ci0 + wn * 64 + b * 32 + lr;
        float* dst = &p.dw[((size_t)tap * p.Cout + co) * p.C + ci];
        // K slices add with float atomics: per-slice partial tiles in a workspace + a reduce launch were measured and are no
        // faster (64x64x128 level 32.8 vs 35.6 us, still behind wgrad_kernel's 33.7; 32x32x256 level 27.9 vs 27.0)
        if (p.ksplit == 1) *dst += acc[a][b][i];
        else if (p.slabs) p.slabs[(size_t)ks_i * p.taps * p.Cout * p.C + ((size_t)tap * p.Cout + co) * p.C + ci] = acc[a][b][i];
        else unsafeAtomicAdd(dst, acc[a][b][i]);
      }
}
__global__ __launch_bounds__(256) void wgrad_dmap(const WgdK p) { wgrad_dmap_body(p, (int)gridDim.x); }
struct WgdKG { WgdK k[RUA_MAX_WGRAD_GROUP]; };
static_assert(sizeof(WgdKG) <= 4096, "grouped launch: kernel arguments are limited to 4 KiB");
__global__ __launch_bounds__(256) void wgrad_dmap_g(const WgdKG g) {
  const WgdK& p = g.k[blockIdx.y];
  const int nwg = p.ntc * p.nti * p.taps * p.ksplit;   // gridDim.x is a multiple of 8: member y's block x runs on XCD x & 7, as ungrouped
  if ((int)blockIdx.x >= nwg) return;
  wgrad_dmap_body(p, nwg);
}

// =========================================================================================
// All-taps weight gradient for the two top levels (Cin = Cout = CC in {32, 64}, 3x3, stride 1, W % 64 == 0; bf16).
// A stage is a run of 64 consecutive pixels of one image row.  A pixel group (3 waves x CC/32) walks a CHAIN of stages
// down the image: same 64-pixel column strip, rows h, h+d, h+2d, .. (one residue class mod d), so the conv-input rows
// h-d, h, h+d it needs are a sliding window: per stage it loads ONE new halo row a[64+2d][CC] into a 3-slot LDS ring plus
// dy[64][32], instead of three rows (measured before chaining: 132 MB fetched for 67 MB of tensors; the window makes the
// nine taps cost ~1.3x the pixel traffic).  Wave `tr` computes the three taps of kernel row tr (dh = (tr-1)*d) for
// every 16-pixel k-step from shifted views of ring slot (it + tr) % 3.  Chains are cut into segments so that ~1024
// groups are busy; a segment pays two extra row loads to fill its window.  NPG pixel groups per block are summed in LDS;
// the block writes ONE fp32 partial (plain coalesced stores); wgrad_taps_reduce adds the partials into dW in a fixed
// order (deterministic, no atomics).  blockIdx.y selects the 32-wide output-channel half (CC = 64).
struct WgtK {
  const unsigned char* a; const unsigned char* dy; float* scratch; float* dw;
  int H, W, N, dil, NPG, halo, halo4, group_bytes, gx;
  int strips, spc, seglen, nchains;        // 64-pixel column strips per row, segments per chain, lattice rows per segment
  int njobs, nworkers, jpw;                // (chain, segment) jobs, pixel groups in the grid, jobs per group
  unsigned abytes, dybytes;
  const float* in_scale; const float* in_shift; int in_relu;      // a is read as [relu](in_scale * a + in_shift) (zero padding stays zero)
  int sx;                                  // wgrad_rows32 / wgrad_rows64: the rows as ONE stream of slots (WgSlots) instead of (chain, segment) jobs
};

template <int CC>
__device__ __forceinline__ void wgrad_taps_body(const WgtK& p) {
  constexpr int NH = CC / 32;             // 32-wide input-channel halves = waves per kernel row
  constexpr int GW = 3 * NH;              // waves per pixel group
  constexpr int GT = GW * 64;             // threads per pixel group
  constexpr int PP = CC / 8;              // 16-byte pieces per pixel of the a image
  constexpr int AROWB = CC * 2;           // a image row bytes (CC = 64: 16-byte chunks XOR-swizzled, see swz())
  constexpr int DROWB = 64;               // dy image: this block's 32 output channels
  constexpr int MAXP = (126 * PP + GT - 1) / GT;       // pieces of one halo row per thread (d <= 31)
  constexpr int DP = (256 + GT - 1) / GT; // dy piece passes
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pg = wv / GW, rr = wv - pg * GW;
  const int tr = rr / NH, cih = rr - tr * NH;
  const int gt = tid - pg * GT;
  unsigned char* sD = smem + pg * p.group_bytes;
  unsigned char* sA = sD + 64 * DROWB;
  const int halo = p.halo, d = p.dil, W = p.W, H = p.H;
  const int co0 = blockIdx.y * 32;
  const __amdgpu_buffer_rsrc_t ra_ = make_rsrc(p.a, p.abytes), rd_ = make_rsrc(p.dy, p.dybytes);

  auto swz = [](int row, int chunk) { return (CC == 64) ? (chunk ^ (((row >> 1) & 1) << 2)) : chunk; };

  const int worker = blockIdx.x * p.NPG + pg;

  // ---- stage-invariant per-thread data: halo-row pieces (offset relative to the row's pixel x0, LDS offset inside a ring
  // slot, border flags: bit2 left of the image, bit3 right of it) and dy pieces
  int prel[MAXP], plds[MAXP], pneed[MAXP];
  const int total = halo * PP;
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int i = gt + k * GT;
    const int j = i / PP, q = i - j * PP;
    prel[k] = ((j - d) * CC + q * 8) * 2;
    plds[k] = (i < total) ? j * AROWB + swz(j, q) * 16 : -1;
    pneed[k] = (j < d ? 4 : 0) | (j >= 64 + d ? 8 : 0) | (i < total ? 0 : 16);
  }
  // normalise on load: GT is a multiple of PP, so every halo-row piece of this thread holds the same 8 input channels
  const bool bn = p.in_scale != nullptr;
  float sc8[8], sh8[8];
  {
    const int q = gt % PP;
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc8[j] = bn ? p.in_scale[q * 8 + j] : 1.f; sh8[j] = (bn && p.in_shift) ? p.in_shift[q * 8 + j] : 0.f; }
  }
  int drel[DP], dlds[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const int i = gt + k * GT;
    drel[k] = ((i >> 2) * CC + co0 + (i & 3) * 8) * 2;
    dlds[k] = (i < 256) ? (i >> 2) * DROWB + (i & 3) * 16 : -1;
  }
  // transposing-read lane geometry (see wgrad_kernel) and the stage-invariant fragment addresses (inside a ring slot)
  const int li = lane & 15, g = lane >> 4;
  const int q4 = li >> 2, pp = li & 3;
  const int chan = 16 * (g & 1) + 4 * pp;
  const int hrow = 8 * (g >> 1) + q4;
  typedef s16x4 __attribute__((address_space(3))) * lds4;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const unsigned char* dybase = sD + hrow * DROWB + chan * 2;
  int aoff[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int row = j * d + hrow;                        // ring slots start at multiples of 4 rows: the swizzle bit is slot-independent
    const int ch = cih * 32 + chan;
    aoff[j] = row * AROWB + swz(row, ch >> 3) * 16 + (ch & 7) * 2;     // +16 rows / +4 rows never flip the swizzle bit
  }
  const int slot_bytes = p.halo4 * AROWB;

  // the current job of this group: image n_, column strip x0, rows h = r_ + i*d for i in [i0, i0 + nit)
  int n_ = 0, x0 = 0, r_ = 0, i0 = 0, nit = 0, bad_lr = 31;
  auto enter_job = [&](int job) {
    n_ = 0; x0 = 0; r_ = 0; i0 = 0; nit = 0;
    if (job < p.njobs) {
      const int chain = job / p.spc, seg = job - chain * p.spc;
      r_ = chain % d; const int t = chain / d;
      x0 = (t % p.strips) * 64; n_ = t / p.strips;
      const int ny = (H - r_ + d - 1) / d;
      i0 = seg * p.seglen;
      int i1 = i0 + p.seglen; if (i1 > ny) i1 = ny;
      nit = i1 > i0 ? i1 - i0 : 0;
    }
    bad_lr = (x0 == 0 ? 4 : 0) | (x0 + 64 == W ? 8 : 0) | 16;
  };

  // lattice row j (relative to i0; j = -1 .. nit) of the conv input -> registers; dy of stage jd (0 .. nit-1) -> registers.
  // TWO register sets: a load has two stages to land (one block per CU: the only latency hiding is this depth)
  uint4 va0[MAXP], vd0[DP], va1[MAXP], vd1[DP];
  int vm0 = 0, vm1 = 0;                                  // which pieces of a register set are real pixels (not zero padding)
  auto load_rows = [&](uint4* va, uint4* vd, int& vm, int j, int jd) {
    const int h = r_ + (i0 + j) * d;
    const bool rowok = nit > 0 && j <= nit && h >= 0 && h < H;
    const int segb = ((n_ * H + h) * W + x0) * CC * 2;
    vm = 0;
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
      const bool ok = rowok && (pneed[k] & bad_lr) == 0;
      vm |= ok ? (1 << k) : 0;
      va[k] = bufload16(ra_, ok ? (unsigned)(segb + prel[k]) : RUA_OOB);
    }
    const int hd = r_ + (i0 + jd) * d;
    const bool dok = jd >= 0 && jd < nit;
    const int dyb = ((n_ * H + hd) * W + x0) * CC * 2;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      vd[k] = bufload16(rd_, (dok && dlds[k] >= 0) ? (unsigned)(dyb + drel[k]) : RUA_OOB);
  };
  auto write_rows = [&](const uint4* va, const uint4* vd, int vm, int slot, bool with_dy) {
    unsigned char* dst = sA + slot * slot_bytes;
#pragma unroll
    for (int k = 0; k < MAXP; ++k)
      if (plds[k] >= 0) {
        uint4 v = va[k];
        if (bn && ((vm >> k) & 1)) {                     // BatchNorm (+ ReLU) of the conv input as it enters LDS (model2.py:17-24)
          float f[8];
          ET<bf16_t>::unpack(v, f);
#pragma unroll
          for (int j = 0; j < 8; ++j) { f[j] = fmaf(sc8[j], f[j], sh8[j]); if (p.in_relu) f[j] = fmaxf(f[j], 0.f); }
          v = ET<bf16_t>::pack(f);
        }
        *reinterpret_cast<uint4*>(dst + plds[k]) = v;
      }
    if (with_dy) {
#pragma unroll
      for (int k = 0; k < DP; ++k)
        if (dlds[k] >= 0) *reinterpret_cast<uint4*>(sD + dlds[k]) = vd[k];
    }
  };
  auto compute = [&](f32x16* acc, int it) {
    const unsigned char* ar = sA + ((it + tr) % 3) * slot_bytes;      // row it + tr - 1
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const s16x4 d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(dybase + ks * 16 * DROWB));
      const s16x4 d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(dybase + ks * 16 * DROWB + 4 * DROWB));
      const s16x8 fd = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const s16x4 x0_ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ar + aoff[j] + ks * 16 * AROWB));
        const s16x4 x1_ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ar + aoff[j] + ks * 16 * AROWB + 4 * AROWB));
        const s16x8 fx = {x0_[0], x0_[1], x0_[2], x0_[3], x1_[0], x1_[1], x1_[2], x1_[3]};
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fd), __builtin_bit_cast(bf16x8, fx), acc[j], 0, 0, 0);
      }
    }
  };

  f32x16 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  for (int jb = 0; jb < p.jpw; ++jb) {
    enter_job(worker + jb * p.nworkers);
    __syncthreads();                                     // the previous job's last stage is done with the ring
    // window fill: rows -1 and 0 into slots 0 and 1 (row j lives in slot (j + 1) % 3), both loads in flight together;
    // then set 0 <- (row 1, dy 0), set 1 <- (row 2, dy 1)
    load_rows(va0, vd0, vm0, -1, -1); load_rows(va1, vd1, vm1, 0, -1);
    write_rows(va0, vd0, vm0, 0, false); write_rows(va1, vd1, vm1, 1, false);
    load_rows(va0, vd0, vm0, 1, 0); load_rows(va1, vd1, vm1, 2, 1);
    for (int it = 0; it < p.seglen; it += 2) {
      __syncthreads();                                   // everyone is done reading slot (it + 2) % 3 (row it - 1) and sD
      write_rows(va0, vd0, vm0, (it + 2) % 3, true);     // row it + 1, dy of stage it
      __syncthreads();
      load_rows(va0, vd0, vm0, it + 3, it + 2);
      compute(acc, it);
      if (it + 1 < p.seglen) {
        __syncthreads();
        write_rows(va1, vd1, vm1, (it + 3) % 3, true);   // row it + 2, dy of stage it + 1
        __syncthreads();
        load_rows(va1, vd1, vm1, it + 4, it + 3);
        compute(acc, it + 1);
      }
    }
  }
  // ---- reduce the pixel groups through LDS, then one partial per block -------------------------
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
  if (pg > 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) red[((((pg - 1) * GW + rr) * 3 + j) * 16 + i) * 64 + lane] = acc[j][i];
  }
  __syncthreads();
  if (pg == 0) {
    float* part = p.scratch + (size_t)(blockIdx.y * p.gx + blockIdx.x) * 9 * 32 * CC;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = acc[j][i];
        for (int gg = 1; gg < p.NPG; ++gg) v += red[((((gg - 1) * GW + rr) * 3 + j) * 16 + i) * 64 + lane];
        const int co = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        part[((tr * 3 + j) * 32 + co) * CC + cih * 32 + (lane & 31)] = v;
      }
  }
}
template <int CC> __global__ __launch_bounds__(768) void wgrad_taps_kernel(const WgtK p) { wgrad_taps_body<CC>(p); }
struct WgtKG { WgtK k[RUA_MAX_WGRAD_GROUP]; };
static_assert(sizeof(WgtKG) <= 4096, "grouped launch: kernel arguments are limited to 4 KiB");
template <int CC> __global__ __launch_bounds__(768) void wgrad_taps_kernel_g(const WgtKG g) {      // blockIdx.z = member
  const WgtK& p = g.k[blockIdx.z];
  if ((int)blockIdx.x >= p.gx) return;
  wgrad_taps_body<CC>(p);
}

// The rows of all images and dilation chains (h = r, r + d, ... of one image) as ONE sequence of slots: a chain's rows followed by one separator (a row of zeros: the
// lower neighbour of the chain's last row and the upper neighbour of the next chain's first).  A block that owns slots [u0, u1) streams them through its ring
// without draining it between chains; a (chain, segment) job refilled the window per job - at d = 31 a chain of a 256-row image has 8 rows, the fill three.
// (wgrad_rowsx.inc has the same machinery inline, for image pairs.)  All of it wave-uniform: scalar registers.
struct SlotCur { int p, r, i; };             // image, chain, position in the chain (i == rows of the chain: its separator)
struct WgSlots {
  int H, d, NP, nyb, R1, per;
  __device__ __forceinline__ void init(int H_, int d_, int NP_) { H = H_; d = d_; NP = NP_; nyb = (H + d - 1) / d; R1 = H - (nyb - 1) * d; per = H + d; }
  __device__ __forceinline__ int rows_of(int r) const { return nyb - (r >= R1 ? 1 : 0); }      // chains r < R1 have nyb rows, the others nyb - 1
  __device__ __forceinline__ SlotCur decode(int u) const {
    SlotCur c;
    if (u < 0) { c.p = -1; c.r = d - 1; c.i = rows_of(d - 1); return c; }      // the separator in front of slot 0
    c.p = u / per;
    int rem = u - c.p * per;
    const int big = R1 * (nyb + 1);
    if (rem < big) { c.r = rem / (nyb + 1); c.i = rem - c.r * (nyb + 1); }
    else { rem -= big; const int q = rem / nyb; c.r = R1 + q; c.i = rem - q * nyb; }
    return c;
  }
  __device__ __forceinline__ void adv(SlotCur& c) const { if (++c.i > rows_of(c.r)) { c.i = 0; if (++c.r == d) { c.r = 0; ++c.p; } } }
  __device__ __forceinline__ bool is_row(const SlotCur& c) const { return c.p >= 0 && c.p < NP && c.i < rows_of(c.r); }
  __device__ __forceinline__ int grow(const SlotCur& c) const { return c.p * H + c.r + c.i * d; }      // row index over all images
};

// wgrad_rows32<NPG, BN> (round 4): the all-taps weight gradient at C = Cout = 32 for rows that are exactly 64 * NPG pixels wide (the
// d6 residual atrous block at 256 x 256: NPG = 4; 128 x 128: NPG = 2), rebuilt like conv_strip32s around what the round-3 census of
// wgrad_taps_kernel<32> showed - 190 - 300 instructions per wave and 64-pixel stage around its 12 MFMAs, three waves per SIMD:
//   * the block works on WHOLE rows: its NPG pixel groups (3 waves each: kernel rows) share one ring of full-width input rows
//     instead of walking NPG chains with private rings - a halo row is loaded once, not per 64-pixel strip with 2 d halo pixels;
//   * rows enter LDS by LDS-DMA (no registers: wgrad_taps_kernel staged every row through VGPRs and C++ LDS stores), waited for
//     with counted vmcnt; the BatchNorm + ReLU of the conv input is applied in place ONE row ahead of its first use, each wave on
//     its own DMA pieces, coefficients read with the pieces, a row outside the image normalised with zeros (no branch);
//   * ONE barrier per stage (wgrad_taps_kernel: two); the slot layout [row | 32 zero pixels] makes the zero padding of a row's
//     left edge the pad of the slot before it: 18 KB per slot, six slots + three dy slots in 160 KB;
//   * fragments by raw ds_read_b64_tr_b16 (hipcc drains the DMA ring in front of the builtin), the reads of k-step k + 1 issued
//     under the MFMAs of k-step k.
// Same jobs (chain segments, several per block), same block partial and deterministic reduction as wgrad_taps_kernel.
// vmcnt: every wave issues exactly KDMA vector-memory operations per stage (row pieces, dy pieces, dummy stores).
template <int NPG, bool BN, bool SX>
__device__ __forceinline__ void wgrad_rows32_body(const WgtK& p) {
  constexpr int C = 32, NW = 3 * NPG, NT = NW * 64, SW = 64 * NPG, PADPX = 32;
  constexpr int SLOT = (SW + PADPX) * 64, DSLOT = SW * 64, R = 6, RD = 3;
  constexpr int NPS = SW / 16;                          // 1-KiB DMA pieces per row
  constexpr int KDMA = (2 * NPS + NW - 1) / NW;         // operations per wave and stage
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sX = smem + PADPX * 64;                // slot 0 (the 2 KiB in front of it: the zero pad of row pixels < 0)
  unsigned char* sDy = sX + R * SLOT;
  float* tab = reinterpret_cast<float*>(sDy + RD * DSLOT);            // [32] scale, [32] shift, [64] zeros
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pgx = wv / 3, ty = wv - 3 * pgx;
  const int H = p.H, d = p.dil;
  const unsigned rowbytes = (unsigned)(SW * C * 2);

  if (tid < 32) {
    tab[tid] = BN ? p.in_scale[tid] : 1.f; tab[32 + tid] = (BN && p.in_shift) ? p.in_shift[tid] : 0.f;
    tab[64 + tid] = 0.f; tab[96 + tid] = 0.f;
  }
  // zero pads: the front pad and the 32 pixels behind every row slot (never written again: the row DMAs cover the SW row pixels only)
  for (int i = tid; i < (R + 1) * (PADPX * 64 / 16); i += NT) {
    const int sl = i / (PADPX * 4), k = i - sl * (PADPX * 4);
    unsigned char* z = (sl == 0 ? smem : sX + (sl - 1) * SLOT + SW * 64) + k * 16;
    *reinterpret_cast<uint4*>(z) = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.a, p.abytes), rd = make_rsrc(p.dy, p.dybytes);
  const unsigned sx_a = (unsigned)(size_t)(lds_void_p)sX, sd_a = (unsigned)(size_t)(lds_void_p)sDy;
  const unsigned tab_a = (unsigned)(size_t)(lds_void_p)tab;
  const unsigned lrel = (unsigned)(lane * 16);
  // transposing-read lane geometry (wgrad_kernel): a 32-channel x 16-pixel fragment = two ds_read_b64_tr_b16, 4 pixel rows apart
  const int li = lane & 15, g = lane >> 4;
  const int q4 = li >> 2, pp = li & 3;
  const int chan = 16 * (g & 1) + 4 * pp;
  const int hrow = 8 * (g >> 1) + q4;
  const unsigned fbase = (unsigned)((64 * pgx + hrow) * 64 + chan * 2);       // pixel 64 pgx + hrow of a slot row, channel chan
  const int tapoff = d * 64;                            // one tap column = d pixels

  int n_ = 0, r_ = 0, i0 = 0, nit = 0;
  auto enter_job = [&](int job) {
    n_ = 0; r_ = 0; i0 = 0; nit = 0;
    if (job < p.njobs) {
      const int chain = job / p.spc, seg = job - chain * p.spc;
      r_ = chain % d; n_ = chain / d;
      const int ny = (H - r_ + d - 1) / d;
      i0 = seg * p.seglen;
      int i1 = i0 + p.seglen; if (i1 > ny) i1 = ny;
      nit = i1 > i0 ? i1 - i0 : 0;
    }
  };
  auto xrow_ok = [&](int rho) { const int h = r_ + (i0 + rho) * d; return nit > 0 && rho <= nit && h >= 0 && h < H; };
  WgSlots G; SlotCur cxi = {0, 0, 0}, cdi = {0, 0, 0}, ctr = {0, 0, 0}, ccm = {0, 0, 0}; int sn = 0;      // SX: the slot cursors of the four streams - row fetched, dy row fetched, row normalised, row multiplied
  if constexpr (SX) {
    G.init(H, d, p.N);
    const long long U = (long long)p.N * G.per;
    const int u0 = (int)(U * (long long)blockIdx.x / p.gx), u1 = (int)(U * (long long)(blockIdx.x + 1) / p.gx);
    sn = u1 - u0;
    cxi = G.decode(u0 - 1); ctr = cxi; cdi = G.decode(u0); ccm = cdi;
  }
  auto xslot = [&](int rho) { return (unsigned)(((rho + 1 + R) % R) * SLOT); };
  auto dslot = [&](int j) { return (unsigned)(((j + RD) % RD) * DSLOT); };
  // the stage's DMA operations of this wave: piece pi = k NW + wv: < NPS a piece of input row xr, < 2 NPS a piece of dy row dr, else a dummy
  auto issue = [&](int xr, int dr) {
    const bool xok_ = SX ? (xr <= sn && G.is_row(cxi)) : xrow_ok(xr);
    const bool dok_ = SX ? (dr >= 0 && dr < sn && G.is_row(cdi)) : (dr >= 0 && dr < nit);
    const unsigned xbase = xok_ ? (unsigned)(SX ? G.grow(cxi) : n_ * H + r_ + (i0 + xr) * d) * rowbytes : OOB;
    const unsigned dbase = dok_ ? (unsigned)(SX ? G.grow(cdi) : n_ * H + r_ + (i0 + dr) * d) * rowbytes : OOB;
    if constexpr (SX) { G.adv(cxi); if (dr >= 0) G.adv(cdi); }      // (the streams are visited in order: every call is the next row of its stream)
    const unsigned xs = xslot(xr), ds = dslot(dr);
#pragma unroll
    for (int k = 0; k < KDMA; ++k) {
      const int pi = k * NW + wv;
      if (pi < NPS) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sX + xs + pi * 1024), 16, (xbase + (unsigned)(pi * 1024)) + lrel, 0, 0, 0);
      else if (pi < 2 * NPS) __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_void_p)(sDy + ds + (pi - NPS) * 1024), 16, (dbase + (unsigned)((pi - NPS) * 1024)) + lrel, 0, 0, 0);
      else { const unsigned z = 0u, off = OOB; asm volatile("buffer_store_dword %0, %1, %2, 0 offen" :: "v"(z), "v"(off), "s"(rd) : "memory"); }
    }
  };
  // BatchNorm + ReLU of input row rho in place, on this wave's own pieces of it (piece pi = k NW + wv < NPS)
  auto transform = [&](int rho) {
    if constexpr (BN) {
      const bool tok_ = SX ? (rho <= sn && G.is_row(ctr)) : xrow_ok(rho);
      if constexpr (SX) G.adv(ctr);
      const unsigned ca = (tab_a + (tok_ ? 0u : 64u * 4u)) + (unsigned)((lane & 3) * 32);
      const unsigned xs = sx_a + xslot(rho) + lrel;
#pragma unroll
      for (int k = 0; k < KDMA; ++k) {
        const int pi = k * NW + wv;
        if (pi < NPS) {                                 // wave-uniform
          u32x4_t rw; f32x4 sa, sb, ha, hb;
          const unsigned a = xs + (unsigned)(pi * 1024);
          asm volatile("ds_read_b128 %0, %5\n\tds_read_b128 %1, %6\n\tds_read_b128 %2, %6 offset:16\n\tds_read_b128 %3, %6 offset:128\n\tds_read_b128 %4, %6 offset:144\n\t"
                       "s_waitcnt lgkmcnt(0)" : "=&v"(rw), "=&v"(sa), "=&v"(sb), "=&v"(ha), "=&v"(hb) : "v"(a), "v"(ca) : "memory");
          float f[8];
          ET<bf16_t>::unpack(make_uint4(rw[0], rw[1], rw[2], rw[3]), f);
#pragma unroll
          for (int j = 0; j < 4; ++j) { f[j] = fmaf(sa[j], f[j], ha[j]); f[4 + j] = fmaf(sb[j], f[4 + j], hb[j]); }
          typedef __attribute__((ext_vector_type(2))) short s16x2;
          typedef __attribute__((ext_vector_type(2))) float f32x2_t;
          typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
          const s16x2 z = {0, 0};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x2_t p2 = {f[2 * j], f[2 * j + 1]};
            const bf16x2_t b2 = __builtin_convertvector(p2, bf16x2_t);
            rw[j] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, b2), z));
          }
          asm volatile("ds_write_b128 %0, %1" :: "v"(a), "v"(rw) : "memory");
        }
      }
    }
  };

  f32x16 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  // fragments of k-step ks of the stage (16 pixels): dy (the a-operand) and the three tap columns of input row `it + ty - 1`
  struct Frags { s16x4 d0, d1, x0[3], x1[3]; };
  auto read_frags = [&](unsigned da, unsigned xa, int ks, Frags& f) {
    const unsigned dk = da + (unsigned)(ks * 1024), xk = xa + (unsigned)(ks * 1024);
    const unsigned xl = xk - (unsigned)tapoff, xr_ = xk + (unsigned)tapoff;
    asm volatile("ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %8 offset:256\n\t"
                 "ds_read_b64_tr_b16 %2, %9\n\tds_read_b64_tr_b16 %3, %9 offset:256\n\t"
                 "ds_read_b64_tr_b16 %4, %10\n\tds_read_b64_tr_b16 %5, %10 offset:256\n\t"
                 "ds_read_b64_tr_b16 %6, %11\n\tds_read_b64_tr_b16 %7, %11 offset:256"
                 : "=&v"(f.d0), "=&v"(f.d1), "=&v"(f.x0[0]), "=&v"(f.x1[0]), "=&v"(f.x0[1]), "=&v"(f.x1[1]), "=&v"(f.x0[2]), "=&v"(f.x1[2])
                 : "v"(dk), "v"(xl), "v"(xk), "v"(xr_) : "memory");
  };
  auto wait_frags = [&](Frags& f, int pending) {
    if (pending) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f.d0), "+v"(f.d1), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.d0), "+v"(f.d1), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
  };
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  auto mfma3 = [&](const Frags& f) {
    const s16x8 fd = {f.d0[0], f.d0[1], f.d0[2], f.d0[3], f.d1[0], f.d1[1], f.d1[2], f.d1[3]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const s16x8 fx = {f.x0[j][0], f.x0[j][1], f.x0[j][2], f.x0[j][3], f.x1[j][0], f.x1[j][1], f.x1[j][2], f.x1[j][3]};
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fd), __builtin_bit_cast(bf16x8, fx), acc[j], 0, 0, 0);
    }
  };

  const int njb_ = SX ? 1 : p.jpw;
  for (int jb = 0; jb < njb_; ++jb) {
    if constexpr (SX) nit = sn; else enter_job((int)blockIdx.x + jb * p.gx);
    // ---- window fill: input rows -1 .. 3 and dy rows 0, 1 in flight, all landed; rows -1, 0, 1 normalised -------------------------
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // the previous job's last stage is done with the rings
    issue(-1, -1); issue(0, 0); issue(1, 1); issue(2, -1); issue(3, -1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    transform(-1); transform(0); transform(1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int it = 0; it < nit; ++it) {
      __builtin_amdgcn_s_barrier();                     // input row it + 1 is normalised and dy row it has landed, for everyone
      issue(it + 4, it + 2);                            // input row it + 4 into the slot of row it - 2, dy row it + 2 into the slot of dy row it - 1
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * KDMA) : "memory");      // the operations of stage it - 2 (input row it + 2) are done
      const unsigned da = sd_a + dslot(it) + fbase;
      const unsigned xa = sx_a + xslot(it + ty - 1) + fbase;
      const bool mul_ = !SX || G.is_row(ccm);             // (SX: a separator slot has nothing to multiply)
      if constexpr (SX) G.adv(ccm);
      if (mul_) {
      Frags fa, fb;
      read_frags(da, xa, 0, fa);
      read_frags(da, xa, 1, fb);
      wait_frags(fa, 1); mfma3(fa);
      read_frags(da, xa, 2, fa);
      wait_frags(fb, 1); mfma3(fb);
      read_frags(da, xa, 3, fb);
      wait_frags(fa, 1); mfma3(fa);
      wait_frags(fb, 0); mfma3(fb);
      }
      transform(it + 2);
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)" :: "n"(KDMA) : "memory");   // stage it - 1's operations (dy row it + 1) are done; this wave's LDS writes too
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
  // ---- reduce the pixel groups through LDS, then one partial per block (wgrad_taps_kernel's layout) -------------------------------
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
  const int lane_ = lane;
  if (pgx > 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) red[((((pgx - 1) * 3 + ty) * 3 + j) * 16 + i) * 64 + lane_] = acc[j][i];
  }
  __syncthreads();
  if (pgx == 0) {
    float* part = p.scratch + (size_t)blockIdx.x * 9 * 32 * C;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = acc[j][i];
        for (int gg = 1; gg < NPG; ++gg) v += red[((((gg - 1) * 3 + ty) * 3 + j) * 16 + i) * 64 + lane_];
        const int co = (i & 3) + 8 * (i >> 2) + 4 * (lane_ >> 5);
        part[((ty * 3 + j) * 32 + co) * C + (lane_ & 31)] = v;
      }
  }
}
template <int NPG, bool BN> __global__ __launch_bounds__(NPG * 192) void wgrad_rows32(const WgtK p) { if (p.sx) wgrad_rows32_body<NPG, BN, true>(p); else wgrad_rows32_body<NPG, BN, false>(p); }
template <int NPG, bool BN> __global__ __launch_bounds__(NPG * 192) void wgrad_rows32_g(const WgtKG g) {       // blockIdx.z = member
  const WgtK& p = g.k[blockIdx.z];
  if ((int)blockIdx.x >= p.gx) return;
  if (p.sx) wgrad_rows32_body<NPG, BN, true>(p); else wgrad_rows32_body<NPG, BN, false>(p);
}

// wgrad_rows64<BN> (round 4): wgrad_rows32's scheme at C = Cout = 64 for rows of exactly 128 pixels (the level-2 ResBlock at 128 x 128, model2.py:15-34,104).
// wgrad_taps_kernel<64> runs one block per output-channel HALF (both halves load, stage through registers and normalise the same input rows), two barriers and
// 12 MFMAs per wave and 64-pixel stage.  Here a block owns WHOLE rows and all 64 output channels: 12 waves = 2 pixel groups x 3 kernel rows x 2 input-channel
// halves, six accumulators (2 output-channel halves x 3 tap columns) and 24 MFMAs per wave and stage; rows by LDS-DMA into one shared ring (five input slots of
// [128 pixels | 32 zero pixels] x 128 B + three dy slots: 153 KB), BatchNorm + ReLU in place one row ahead, ONE barrier per stage.  128-byte pixel rows would put
// the four pixel rows of a transposing read on two banks: the 16-byte chunks of a pixel are XOR-swizzled with bit 1 of the pixel index (chunk ^ 4), applied on
// the DMA's SOURCE side (the LDS destination of a DMA is lane-linear) and in the fragment / coefficient addresses.
// Same jobs, same block partials (one per output-channel half) and deterministic reduction as wgrad_taps_kernel<64>.
template <bool BN, bool SX>
__device__ __forceinline__ void wgrad_rows64_body(const WgtK& p) {
  constexpr int C = 64, NPG = 2, NW = 6 * NPG, NT = NW * 64, SW = 64 * NPG, PADPX = 32, PXB = C * 2;
  constexpr int SLOT = (SW + PADPX) * PXB, DSLOT = SW * PXB, R = 5, RD = 3;
  constexpr int NPS = SW * PXB / 1024;                  // 1-KiB DMA pieces per row (8 pixels each)
  constexpr int KDMA = (2 * NPS + NW - 1) / NW;         // operations per wave and stage
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sX = smem + PADPX * PXB;               // slot 0 (the 4 KiB in front of it: the zero pad of row pixels < 0)
  unsigned char* sDy = sX + R * SLOT;
  float* tab = reinterpret_cast<float*>(sDy + RD * DSLOT);            // [64] scale, [64] shift, [128] zeros
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pgx = wv / 6, rem = wv - 6 * pgx, ty = rem >> 1, cih = rem & 1;
  const int H = p.H, d = p.dil;
  const unsigned rowbytes = (unsigned)(SW * PXB);

  if (tid < 64) {
    tab[tid] = BN ? p.in_scale[tid] : 1.f; tab[64 + tid] = (BN && p.in_shift) ? p.in_shift[tid] : 0.f;
    tab[128 + tid] = 0.f; tab[192 + tid] = 0.f;
  }
  for (int i = tid; i < (R + 1) * (PADPX * PXB / 16); i += NT) {       // zero pads: the front pad and the 32 pixels behind every row slot
    const int sl = i / (PADPX * PXB / 16), k = i - sl * (PADPX * PXB / 16);
    unsigned char* z = (sl == 0 ? smem : sX + (sl - 1) * SLOT + SW * PXB) + k * 16;
    *reinterpret_cast<uint4*>(z) = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.a, p.abytes), rd = make_rsrc(p.dy, p.dybytes);
  const unsigned sx_a = (unsigned)(size_t)(lds_void_p)sX, sd_a = (unsigned)(size_t)(lds_void_p)sDy;
  const unsigned tab_a = (unsigned)(size_t)(lds_void_p)tab;
  // lane l of a DMA piece: LDS position = pixel (l >> 3), chunk (l & 7); it fetches the chunk (l & 7) ^ (bit 1 of the pixel << 2) of that pixel
  const int gchunk = (lane & 7) ^ (((lane >> 4) & 1) << 2);
  const unsigned srel = (unsigned)((lane >> 3) * PXB + gchunk * 16);
  const unsigned lrel = (unsigned)(lane * 16);
  // transposing-read lane geometry (wgrad_kernel): a 32-channel x 16-pixel fragment = two ds_read_b64_tr_b16, 4 pixel rows apart
  const int li = lane & 15, g = lane >> 4;
  const int q4 = li >> 2, pp = li & 3;
  const int chan = 16 * (g & 1) + 4 * pp;
  const int hrow = 8 * (g >> 1) + q4;
  auto frag_off = [&](int pix_rel, int ch) {             // byte offset of channel ch of slot pixel 64 pgx + hrow + pix_rel (its swizzle bit: bit 1 of hrow + pix_rel)
    const int v = hrow + pix_rel;
    const int sb = (v >> 1) & 1;
    return (64 * pgx + v) * PXB + (((ch >> 3) ^ (sb << 2)) * 16) + (ch & 7) * 2;
  };
  const int dyo0 = frag_off(0, chan);                    // dy: output-channel half 0; half 1 is 32 channels = 4 chunks further: the chunk index ^ 4, i.e. the address ^ 64
  const int xo0 = frag_off(-d, cih * 32 + chan), xo1 = frag_off(0, cih * 32 + chan), xo2 = frag_off(d, cih * 32 + chan);   // x: tap columns, this wave's ci half

  int n_ = 0, r_ = 0, i0 = 0, nit = 0;
  auto enter_job = [&](int job) {
    n_ = 0; r_ = 0; i0 = 0; nit = 0;
    if (job < p.njobs) {
      const int chain = job / p.spc, seg = job - chain * p.spc;
      r_ = chain % d; n_ = chain / d;
      const int ny = (H - r_ + d - 1) / d;
      i0 = seg * p.seglen;
      int i1 = i0 + p.seglen; if (i1 > ny) i1 = ny;
      nit = i1 > i0 ? i1 - i0 : 0;
    }
  };
  auto xrow_ok = [&](int rho) { const int h = r_ + (i0 + rho) * d; return nit > 0 && rho <= nit && h >= 0 && h < H; };
  WgSlots G; SlotCur cxi = {0, 0, 0}, cdi = {0, 0, 0}, ctr = {0, 0, 0}, ccm = {0, 0, 0}; int sn = 0;      // SX: the slot cursors of the four streams - row fetched, dy row fetched, row normalised, row multiplied
  if constexpr (SX) {
    G.init(H, d, p.N);
    const long long U = (long long)p.N * G.per;
    const int u0 = (int)(U * (long long)blockIdx.x / p.gx), u1 = (int)(U * (long long)(blockIdx.x + 1) / p.gx);
    sn = u1 - u0;
    cxi = G.decode(u0 - 1); ctr = cxi; cdi = G.decode(u0); ccm = cdi;
  }
  auto xslot = [&](int rho) { return (unsigned)(((rho + 1 + R) % R) * SLOT); };
  auto dslot = [&](int j) { return (unsigned)(((j + RD) % RD) * DSLOT); };
  auto issue = [&](int xr, int dr) {
    const bool xok_ = SX ? (xr <= sn && G.is_row(cxi)) : xrow_ok(xr);
    const bool dok_ = SX ? (dr >= 0 && dr < sn && G.is_row(cdi)) : (dr >= 0 && dr < nit);
    const unsigned xbase = xok_ ? (unsigned)(SX ? G.grow(cxi) : n_ * H + r_ + (i0 + xr) * d) * rowbytes : OOB;
    const unsigned dbase = dok_ ? (unsigned)(SX ? G.grow(cdi) : n_ * H + r_ + (i0 + dr) * d) * rowbytes : OOB;
    if constexpr (SX) { G.adv(cxi); if (dr >= 0) G.adv(cdi); }      // (the streams are visited in order: every call is the next row of its stream)
    const unsigned xs = xslot(xr), ds = dslot(dr);
#pragma unroll
    for (int k = 0; k < KDMA; ++k) {
      const int pi = k * NW + wv;
      if (pi < NPS) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sX + xs + pi * 1024), 16, (xbase + (unsigned)(pi * 1024)) + srel, 0, 0, 0);
      else if (pi < 2 * NPS) __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_void_p)(sDy + ds + (pi - NPS) * 1024), 16, (dbase + (unsigned)((pi - NPS) * 1024)) + srel, 0, 0, 0);
      else { const unsigned z = 0u, off = OOB; asm volatile("buffer_store_dword %0, %1, %2, 0 offen" :: "v"(z), "v"(off), "s"(rd) : "memory"); }
    }
  };
  // BatchNorm + ReLU of input row rho in place, on this wave's own pieces of it (piece pi = k NW + wv < NPS); the piece of lane l holds the channels of chunk gchunk
  auto transform = [&](int rho) {
    if constexpr (BN) {
      const bool tok_ = SX ? (rho <= sn && G.is_row(ctr)) : xrow_ok(rho);
      if constexpr (SX) G.adv(ctr);
      const unsigned ca = (tab_a + (tok_ ? 0u : 128u * 4u)) + (unsigned)(gchunk * 32);
      const unsigned xs = sx_a + xslot(rho) + lrel;
#pragma unroll
      for (int k = 0; k < KDMA; ++k) {
        const int pi = k * NW + wv;
        if (pi < NPS) {                                 // wave-uniform
          u32x4_t rw; f32x4 sa, sb, ha, hb;
          const unsigned a = xs + (unsigned)(pi * 1024);
          asm volatile("ds_read_b128 %0, %5\n\tds_read_b128 %1, %6\n\tds_read_b128 %2, %6 offset:16\n\tds_read_b128 %3, %6 offset:256\n\tds_read_b128 %4, %6 offset:272\n\t"
                       "s_waitcnt lgkmcnt(0)" : "=&v"(rw), "=&v"(sa), "=&v"(sb), "=&v"(ha), "=&v"(hb) : "v"(a), "v"(ca) : "memory");
          float f[8];
          ET<bf16_t>::unpack(make_uint4(rw[0], rw[1], rw[2], rw[3]), f);
#pragma unroll
          for (int j = 0; j < 4; ++j) { f[j] = fmaf(sa[j], f[j], ha[j]); f[4 + j] = fmaf(sb[j], f[4 + j], hb[j]); }
          typedef __attribute__((ext_vector_type(2))) short s16x2;
          typedef __attribute__((ext_vector_type(2))) float f32x2_t;
          typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
          const s16x2 z = {0, 0};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x2_t p2 = {f[2 * j], f[2 * j + 1]};
            const bf16x2_t b2 = __builtin_convertvector(p2, bf16x2_t);
            rw[j] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, b2), z));
          }
          asm volatile("ds_write_b128 %0, %1" :: "v"(a), "v"(rw) : "memory");
        }
      }
    }
  };

  f32x16 acc[6];                                         // [output-channel half][tap column]
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  // fragments of k-step ks of the stage (16 pixels): dy (the a-operand) of both output-channel halves and the three tap columns of input row `it + ty - 1`
  struct Frags { s16x4 d0[2], d1[2], x0[3], x1[3]; };
  auto read_frags = [&](unsigned da, unsigned xa, int ks, Frags& f) {
    const unsigned dk0 = da + (unsigned)(dyo0 + ks * 16 * PXB), dk1 = dk0 ^ 64u;
    const unsigned xk0 = (unsigned)((int)xa + xo0 + ks * 16 * PXB), xk1 = (unsigned)((int)xa + xo1 + ks * 16 * PXB), xk2 = (unsigned)((int)xa + xo2 + ks * 16 * PXB);
    asm volatile("ds_read_b64_tr_b16 %0, %10\n\tds_read_b64_tr_b16 %1, %10 offset:512\n\t"
                 "ds_read_b64_tr_b16 %2, %11\n\tds_read_b64_tr_b16 %3, %11 offset:512\n\t"
                 "ds_read_b64_tr_b16 %4, %12\n\tds_read_b64_tr_b16 %5, %12 offset:512\n\t"
                 "ds_read_b64_tr_b16 %6, %13\n\tds_read_b64_tr_b16 %7, %13 offset:512\n\t"
                 "ds_read_b64_tr_b16 %8, %14\n\tds_read_b64_tr_b16 %9, %14 offset:512"
                 : "=&v"(f.d0[0]), "=&v"(f.d1[0]), "=&v"(f.d0[1]), "=&v"(f.d1[1]), "=&v"(f.x0[0]), "=&v"(f.x1[0]), "=&v"(f.x0[1]), "=&v"(f.x1[1]), "=&v"(f.x0[2]), "=&v"(f.x1[2])
                 : "v"(dk0), "v"(dk1), "v"(xk0), "v"(xk1), "v"(xk2) : "memory");
  };
  auto wait_frags = [&](Frags& f, int pending) {
    if (pending) asm volatile("s_waitcnt lgkmcnt(10)" : "+v"(f.d0[0]), "+v"(f.d1[0]), "+v"(f.d0[1]), "+v"(f.d1[1]), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.d0[0]), "+v"(f.d1[0]), "+v"(f.d0[1]), "+v"(f.d1[1]), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
  };
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  auto mfma6 = [&](const Frags& f) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const s16x8 fd = {f.d0[h][0], f.d0[h][1], f.d0[h][2], f.d0[h][3], f.d1[h][0], f.d1[h][1], f.d1[h][2], f.d1[h][3]};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const s16x8 fx = {f.x0[j][0], f.x0[j][1], f.x0[j][2], f.x0[j][3], f.x1[j][0], f.x1[j][1], f.x1[j][2], f.x1[j][3]};
        acc[h * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fd), __builtin_bit_cast(bf16x8, fx), acc[h * 3 + j], 0, 0, 0);
      }
    }
  };

  const int njb_ = SX ? 1 : p.jpw;
  for (int jb = 0; jb < njb_; ++jb) {
    if constexpr (SX) nit = sn; else enter_job((int)blockIdx.x + jb * p.gx);
    // ---- window fill: input rows -1 .. 2 and dy rows 0, 1 in flight, all landed; rows -1, 0, 1 normalised ---------------------------
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // the previous job's last stage is done with the rings
    issue(-1, -1); issue(0, 0); issue(1, 1); issue(2, -1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    transform(-1); transform(0); transform(1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int it = 0; it < nit; ++it) {
      __builtin_amdgcn_s_barrier();                     // input row it + 1 is normalised and dy row it has landed, for everyone
      issue(it + 3, it + 2);                            // input row it + 3 into the slot of row it - 2, dy row it + 2 into the slot of dy row it - 1
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KDMA) : "memory");          // the operations of stage it - 1 (input row it + 2, dy row it + 1) are done
      const unsigned da = sd_a + dslot(it);
      const unsigned xa = sx_a + xslot(it + ty - 1);
      const bool mul_ = !SX || G.is_row(ccm);             // (SX: a separator slot has nothing to multiply)
      if constexpr (SX) G.adv(ccm);
      if (mul_) {
      Frags fa, fb;
      read_frags(da, xa, 0, fa);
      read_frags(da, xa, 1, fb);
      wait_frags(fa, 1); mfma6(fa);
      read_frags(da, xa, 2, fa);
      wait_frags(fb, 1); mfma6(fb);
      read_frags(da, xa, 3, fb);
      wait_frags(fa, 1); mfma6(fa);
      wait_frags(fb, 0); mfma6(fb);
      }
      transform(it + 2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                    // this wave's LDS writes are done before the barrier publishes them
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
  // ---- reduce the pixel groups through LDS, then one partial per block and output-channel half (wgrad_taps_kernel<64>'s layout) -------
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
  if (pgx > 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) red[((rem * 6 + j) * 16 + i) * 64 + lane] = acc[j][i];
  }
  __syncthreads();
  if (pgx == 0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float* part = p.scratch + (size_t)(h * p.gx + (int)blockIdx.x) * 9 * 32 * C;
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc[h * 3 + j][i] + red[((rem * 6 + h * 3 + j) * 16 + i) * 64 + lane];
          const int co = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
          part[((ty * 3 + j) * 32 + co) * C + cih * 32 + (lane & 31)] = v;
        }
    }
  }
}
template <bool BN> __global__ __launch_bounds__(768) void wgrad_rows64(const WgtK p) { if (p.sx) wgrad_rows64_body<BN, true>(p); else wgrad_rows64_body<BN, false>(p); }
template <bool BN> __global__ __launch_bounds__(768) void wgrad_rows64_g(const WgtKG g) {       // blockIdx.z = member
  const WgtK& p = g.k[blockIdx.z];
  if ((int)blockIdx.x >= p.gx) return;
  if (p.sx) wgrad_rows64_body<BN, true>(p); else wgrad_rows64_body<BN, false>(p);
}

// wgrad_rows128 (round 4): the same scheme one level down - C = Cout = 128 on 64-pixel rows (the level-3 ResBlock at 64 x 64, model2.py:105-106; its input is a
// materialised BatchNorm output: no normalise-on-load).  The generic wgrad_kernel runs this level on 64 x 64 tiles with two barriers per 64-pixel stage and 4 MFMAs per
// wave (PMC: matrix pipe 5 % busy).  Here a block owns whole rows, ALL 128 input channels and a SLICE of 64 output channels (blockIdx.y): 12 waves = 3 kernel rows x 4
// input-channel quarters, six accumulators (2 output-channel halves x 3 tap columns), 24 MFMAs per wave and stage; the input rows (64 pixels x 256 B) and the slice of
// the dy rows (64 x 128 B, gathered from 256-byte pixels by the DMA's per-lane source address) stream through one shared ring, one barrier per stage.  256-byte pixels
// put all four pixel rows of a transposing read on ONE bank group: the 16-byte chunks are XOR-swizzled with bits 0 - 1 of the pixel index (chunk ^ (p & 3) << 2), the
// 128-byte dy pixels with bit 1 (as wgrad_rows64).  Block partials [output-channel quarter][block][9][32][128] and the deterministic reduction of wgrad_taps_kernel.
__device__ __forceinline__ void wgrad_rows128_body(const WgtK& p, int slice) {
  constexpr int C = 128, NW = 12, SW = 64, PADPX = 32, PXB = C * 2, DPB = 128;
  constexpr int SLOT = (SW + PADPX) * PXB, DSLOT = SW * DPB, R = 5, RD = 3;
  constexpr int NPX = SW * PXB / 1024, NPD = DSLOT / 1024;             // 1-KiB DMA pieces per input row (4 pixels each) / per dy slice row (8 pixels each)
  constexpr int KDMA = (NPX + NPD) / NW;                // operations per wave and stage: exactly 2
  static_assert((NPX + NPD) % NW == 0, "every wave issues the same number of DMA operations per stage");
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sX = smem + PADPX * PXB;               // slot 0 (the 8 KiB in front of it: the zero pad of row pixels < 0)
  unsigned char* sDy = sX + R * SLOT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = wv >> 2, ciq = wv & 3;
  const int H = p.H, d = p.dil;
  const unsigned rowbytes = (unsigned)(SW * PXB);

  for (int i = tid; i < (R + 1) * (PADPX * PXB / 16); i += NW * 64) {  // zero pads: the front pad and the 32 pixels behind every row slot
    const int sl = i / (PADPX * PXB / 16), k = i - sl * (PADPX * PXB / 16);
    unsigned char* z = (sl == 0 ? smem : sX + (sl - 1) * SLOT + SW * PXB) + k * 16;
    *reinterpret_cast<uint4*>(z) = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.a, p.abytes), rd = make_rsrc(p.dy, p.dybytes);
  const unsigned sx_a = (unsigned)(size_t)(lds_void_p)sX, sd_a = (unsigned)(size_t)(lds_void_p)sDy;
  // x piece: lane l sits at pixel (l >> 4), chunk (l & 15) of the piece's four pixels and fetches chunk (l & 15) ^ ((pixel & 3) << 2) of that pixel
  const unsigned srel_x = (unsigned)((lane >> 4) * PXB + (((lane & 15) ^ ((lane >> 4) << 2)) * 16));
  // dy piece: lane l sits at pixel (l >> 3), chunk (l & 7) of the piece's eight 128-byte slice pixels; the source pixels are 256 bytes apart
  const unsigned srel_d = (unsigned)((lane >> 3) * PXB + slice * DPB + (((lane & 7) ^ (((lane >> 4) & 1) << 2)) * 16));
  const int li = lane & 15, g = lane >> 4;
  const int q4 = li >> 2, pp = li & 3;
  const int chan = 16 * (g & 1) + 4 * pp;
  const int hrow = 8 * (g >> 1) + q4;
  auto x_off = [&](int pix_rel) {                        // channel ciq * 32 + chan of slot pixel hrow + pix_rel
    const int v = hrow + pix_rel, ch = ciq * 32 + chan;
    return v * PXB + (((ch >> 3) ^ ((v & 3) << 2)) * 16) + (ch & 7) * 2;
  };
  const int dyo0 = hrow * DPB + (((chan >> 3) ^ (((hrow >> 1) & 1) << 2)) * 16) + (chan & 7) * 2;      // output-channel half 0 of the slice; half 1: ^ 64
  const int xo0 = x_off(-d), xo1 = x_off(0), xo2 = x_off(d);

  int n_ = 0, r_ = 0, i0 = 0, nit = 0;
  auto enter_job = [&](int job) {
    n_ = 0; r_ = 0; i0 = 0; nit = 0;
    if (job < p.njobs) {
      const int chain = job / p.spc, seg = job - chain * p.spc;
      r_ = chain % d; n_ = chain / d;
      const int ny = (H - r_ + d - 1) / d;
      i0 = seg * p.seglen;
      int i1 = i0 + p.seglen; if (i1 > ny) i1 = ny;
      nit = i1 > i0 ? i1 - i0 : 0;
    }
  };
  auto xrow_ok = [&](int rho) { const int h = r_ + (i0 + rho) * d; return nit > 0 && rho <= nit && h >= 0 && h < H; };
  auto xslot = [&](int rho) { return (unsigned)(((rho + 1 + R) % R) * SLOT); };
  auto dslot = [&](int j) { return (unsigned)(((j + RD) % RD) * DSLOT); };
  auto issue = [&](int xr, int dr) {
    const unsigned xbase = xrow_ok(xr) ? (unsigned)(n_ * H + r_ + (i0 + xr) * d) * rowbytes : OOB;
    const unsigned dbase = (dr >= 0 && dr < nit) ? (unsigned)(n_ * H + r_ + (i0 + dr) * d) * rowbytes : OOB;
    const unsigned xs = xslot(xr), ds = dslot(dr);
#pragma unroll
    for (int k = 0; k < KDMA; ++k) {
      const int pi = k * NW + wv;
      if (pi < NPX) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sX + xs + pi * 1024), 16, (xbase + (unsigned)(pi * 1024)) + srel_x, 0, 0, 0);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_void_p)(sDy + ds + (pi - NPX) * 1024), 16, (dbase + (unsigned)((pi - NPX) * 8 * PXB)) + srel_d, 0, 0, 0);
    }
  };

  f32x16 acc[6];                                         // [output-channel half of the slice][tap column]
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  struct Frags { s16x4 d0[2], d1[2], x0[3], x1[3]; };
  auto read_frags = [&](unsigned da, unsigned xa, int ks, Frags& f) {
    const unsigned dk0 = da + (unsigned)(dyo0 + ks * 16 * DPB), dk1 = dk0 ^ 64u;
    const unsigned xk0 = (unsigned)((int)xa + xo0 + ks * 16 * PXB), xk1 = (unsigned)((int)xa + xo1 + ks * 16 * PXB), xk2 = (unsigned)((int)xa + xo2 + ks * 16 * PXB);
    asm volatile("ds_read_b64_tr_b16 %0, %10\n\tds_read_b64_tr_b16 %1, %10 offset:512\n\t"
                 "ds_read_b64_tr_b16 %2, %11\n\tds_read_b64_tr_b16 %3, %11 offset:512\n\t"
                 "ds_read_b64_tr_b16 %4, %12\n\tds_read_b64_tr_b16 %5, %12 offset:1024\n\t"
                 "ds_read_b64_tr_b16 %6, %13\n\tds_read_b64_tr_b16 %7, %13 offset:1024\n\t"
                 "ds_read_b64_tr_b16 %8, %14\n\tds_read_b64_tr_b16 %9, %14 offset:1024"
                 : "=&v"(f.d0[0]), "=&v"(f.d1[0]), "=&v"(f.d0[1]), "=&v"(f.d1[1]), "=&v"(f.x0[0]), "=&v"(f.x1[0]), "=&v"(f.x0[1]), "=&v"(f.x1[1]), "=&v"(f.x0[2]), "=&v"(f.x1[2])
                 : "v"(dk0), "v"(dk1), "v"(xk0), "v"(xk1), "v"(xk2) : "memory");
  };
  auto wait_frags = [&](Frags& f, int pending) {
    if (pending) asm volatile("s_waitcnt lgkmcnt(10)" : "+v"(f.d0[0]), "+v"(f.d1[0]), "+v"(f.d0[1]), "+v"(f.d1[1]), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.d0[0]), "+v"(f.d1[0]), "+v"(f.d0[1]), "+v"(f.d1[1]), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
  };
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  auto mfma6 = [&](const Frags& f) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const s16x8 fd = {f.d0[h][0], f.d0[h][1], f.d0[h][2], f.d0[h][3], f.d1[h][0], f.d1[h][1], f.d1[h][2], f.d1[h][3]};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const s16x8 fx = {f.x0[j][0], f.x0[j][1], f.x0[j][2], f.x0[j][3], f.x1[j][0], f.x1[j][1], f.x1[j][2], f.x1[j][3]};
        acc[h * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fd), __builtin_bit_cast(bf16x8, fx), acc[h * 3 + j], 0, 0, 0);
      }
    }
  };

  for (int jb = 0; jb < p.jpw; ++jb) {
    enter_job((int)blockIdx.x + jb * p.gx);
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // the previous job's last stage is done with the rings
    issue(-1, -1); issue(0, 0); issue(1, 1); issue(2, -1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int it = 0; it < nit; ++it) {
      __builtin_amdgcn_s_barrier();                     // input row it + 1 and dy row it have landed, for everyone
      issue(it + 3, it + 2);                            // input row it + 3 into the slot of row it - 2, dy row it + 2 into the slot of dy row it - 1
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KDMA) : "memory");          // the operations of stage it - 1 (input row it + 2, dy row it + 1) are done
      const unsigned da = sd_a + dslot(it);
      const unsigned xa = sx_a + xslot(it + ty - 1);
      Frags fa, fb;
      read_frags(da, xa, 0, fa);
      read_frags(da, xa, 1, fb);
      wait_frags(fa, 1); mfma6(fa);
      read_frags(da, xa, 2, fa);
      wait_frags(fb, 1); mfma6(fb);
      read_frags(da, xa, 3, fb);
      wait_frags(fa, 1); mfma6(fa);
      wait_frags(fb, 0); mfma6(fb);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float* part = p.scratch + (size_t)((2 * slice + h) * p.gx + (int)blockIdx.x) * 9 * 32 * C;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        part[((ty * 3 + j) * 32 + co) * C + ciq * 32 + (lane & 31)] = acc[h * 3 + j][i];
      }
  }
}
__global__ __launch_bounds__(768) void wgrad_rows128(const WgtK p) { wgrad_rows128_body(p, (int)blockIdx.y); }
__global__ __launch_bounds__(768) void wgrad_rows128_g(const WgtKG g) {       // blockIdx.z = member, blockIdx.y = output-channel slice
  const WgtK& p = g.k[blockIdx.z];
  if ((int)blockIdx.x >= p.gx) return;
  wgrad_rows128_body(p, (int)blockIdx.y);
}

#include "wgrad_rowsx.inc"

// wgrad_img<W> (round 4): the 3x3 weight gradients of the two deepest levels (16 x 16 x 512 and 8 x 8 x 1024, dilation 1: model2.py:109-112 and their decoder mirror).  The generic
// wgrad_kernel cuts dW into 64 x 64 tiles per TAP - 2 304 blocks at 8 x 8 x 1024, each staging all 512 pixels of its two operand slices through registers and LDS again, 64 pixels
// and two barriers at a time: ~0.3 GB of L2 -> LDS traffic per launch, 22 - 28 us for 9.66 GFLOP.  Here a block owns a 64 x 64 tile of dW for ALL NINE taps over a chunk of 512
// pixels (8 images of 8 x 8, or 2 of 16 x 16: whole images): its slices of dy and of the input - 512 pixels x 64 channels each, 64 KB + 64 KB - enter LDS ONCE by LDS-DMA
// (per-lane source addresses gather the 128-byte slices out of the C-channel pixels, chunks XOR-swizzled with bit 1 of the pixel index as in wgrad_rows64), then 12 waves =
// 3 kernel rows x 2 output-channel halves x 2 input-channel halves run 32 k-steps of three MFMAs with NO barrier: a tap is a shift of the input pixels by (dh W + dw), read
// straight from the resident tile; pixels the shift carries across an image border are zeroed in the fragment (their position inside a transposed fragment is fixed per tap column;
// the rows are a per-k-step predicate) - the tile has a slack of 18 pixels at either end for the shifted addresses.  256 blocks = one per CU at both levels (16 x 16: four
// pixel chunks, i.e. four K slices through the deterministic slab reduction).
template <int W>
__global__ __launch_bounds__(768) void wgrad_img(const WgK p) {
  constexpr int PC = 512, PXB = 128, SLACK = 18 * PXB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sX = smem + SLACK;                     // [512 pixels][64 ci] + slack either side
  unsigned char* sD = sX + PC * PXB + SLACK;            // [512 pixels][64 co]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = wv >> 2, coh = (wv >> 1) & 1, cih = wv & 1;
  int b = blockIdx.x;
  const int ti = b % p.nti; b /= p.nti;
  const int tc = b % p.ntc; b /= p.ntc;
  const int chunk = b;                                  // pixel chunk = K slice
  const int co0 = tc * 64, ci0 = ti * 64;
  const unsigned cbytes = (unsigned)(p.C * 2), obytes = (unsigned)(p.Cout * 2);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.a, (unsigned)((size_t)p.M * p.C * 2)), rd = make_rsrc(p.dy, (unsigned)((size_t)p.M * p.Cout * 2));
  {
    // piece = 8 pixels x 128 bytes; lane l sits at pixel (l >> 3), chunk (l & 7) and fetches chunk (l & 7) ^ (bit 1 of the pixel << 2) of that pixel's slice
    const unsigned gch = (unsigned)(((lane & 7) ^ (((lane >> 4) & 1) << 2)) * 16);
    const unsigned pix0 = (unsigned)(chunk * PC + (lane >> 3));
    // 128 pieces in pixel order, the two operands alternating; wave wv issues pieces wv, wv + 12, ...: eleven operations each (the last four waves end with a dummy), so that
    // "operation k of every wave is done" means "the first 48 (k + 1) pixels of both tiles have landed" and the k-steps start while the rest is in flight
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const int q = k * 12 + wv, pb = q >> 1;
      if (q >= 2 * (PC / 8)) { const unsigned z = 0u, off = 0x80000000u; asm volatile("buffer_store_dword %0, %1, %2, 0 offen" :: "v"(z), "v"(off), "s"(rd) : "memory"); }
      else if (!(q & 1)) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sX + pb * 1024), 16, (pix0 + (unsigned)(pb * 8)) * cbytes + (unsigned)(ci0 * 2) + gch, 0, 0, 0);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_void_p)(sD + pb * 1024), 16, (pix0 + (unsigned)(pb * 8)) * obytes + (unsigned)(co0 * 2) + gch, 0, 0, 0);
    }
  }
  const unsigned sx_a = (unsigned)(size_t)(lds_void_p)sX, sd_a = (unsigned)(size_t)(lds_void_p)sD;
  const int li = lane & 15, g = lane >> 4;
  const int q4 = li >> 2, pp = li & 3;
  const int chan = 16 * (g & 1) + 4 * pp;
  const int kh = g >> 1;                                // which 8 pixels of the 16-pixel k-step this lane's fragment elements come from
  const int hrow = 8 * kh + q4;
  auto off_of = [&](int pix, int ch) {                   // byte offset of channel ch (of the 64-channel slice) of tile pixel `pix` (may be negative: slack)
    return pix * PXB + ((((ch >> 3)) ^ (((pix >> 1) & 1) << 2)) * 16) + (ch & 7) * 2;
  };
  const unsigned dyo = sd_a + (unsigned)off_of(hrow, coh * 32 + chan);
  unsigned xo[3];
#pragma unroll
  for (int tx = 0; tx < 3; ++tx) xo[tx] = (unsigned)((int)sx_a + off_of(hrow + (ty - 1) * W + (tx - 1), cih * 32 + chan));
  // fragment element masks: a transposed read returns, per lane, its channel of the four pixels 8 kh + {0..3} (second read: + 4).  Tap column 0 reads pixel w - 1: invalid at
  // w = 0 (element 0 of the first read where the group starts a row); tap column 2 reads w + 1: invalid at w = W - 1 (element 3 of the second read where the group ends a row)
  const bool row_start = (W == 8) || kh == 0, row_end = (W == 8) || kh == 1;
  const unsigned m_l = row_start ? 0xffff0000u : 0xffffffffu;      // first read, low dword (elements 0, 1): element 0 off
  const unsigned m_r = row_end ? 0x0000ffffu : 0xffffffffu;        // second read, high dword (elements 2, 3): element 3 off

  f32x16 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  struct Frags { s16x4 d0, d1, x0[3], x1[3]; };
  auto read_frags = [&](int ks, Frags& f) {
    const unsigned dk = dyo + (unsigned)(ks * 16 * PXB);
    const unsigned x0a = xo[0] + (unsigned)(ks * 16 * PXB), x1a = xo[1] + (unsigned)(ks * 16 * PXB), x2a = xo[2] + (unsigned)(ks * 16 * PXB);
    asm volatile("ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %8 offset:512\n\t"
                 "ds_read_b64_tr_b16 %2, %9\n\tds_read_b64_tr_b16 %3, %9 offset:512\n\t"
                 "ds_read_b64_tr_b16 %4, %10\n\tds_read_b64_tr_b16 %5, %10 offset:512\n\t"
                 "ds_read_b64_tr_b16 %6, %11\n\tds_read_b64_tr_b16 %7, %11 offset:512"
                 : "=&v"(f.d0), "=&v"(f.d1), "=&v"(f.x0[0]), "=&v"(f.x1[0]), "=&v"(f.x0[1]), "=&v"(f.x1[1]), "=&v"(f.x0[2]), "=&v"(f.x1[2])
                 : "v"(dk), "v"(x0a), "v"(x1a), "v"(x2a) : "memory");
  };
  auto wait_frags = [&](Frags& f, int pending) {
    if (pending) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f.d0), "+v"(f.d1), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.d0), "+v"(f.d1), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
  };
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  auto mfma3 = [&](const Frags& f, int ks) {
    // the image row of this lane's pixels: W = 8: row (2 ks + kh) & 7 (a k-step spans two rows); W = 16: row ks & 15 (one row).  Kernel row 0 reads row h - 1, kernel row 2 row h + 1
    const int h = (W == 8) ? ((2 * ks + kh) & 7) : (ks & 15);
    const bool rows_ok = !((ty == 0 && h == 0) || (ty == 2 && h == W - 1));
    const unsigned rm = rows_ok ? 0xffffffffu : 0u;
    const s16x8 fd = {f.d0[0], f.d0[1], f.d0[2], f.d0[3], f.d1[0], f.d1[1], f.d1[2], f.d1[3]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      u32x2 a = __builtin_bit_cast(u32x2, f.x0[j]), c = __builtin_bit_cast(u32x2, f.x1[j]);
      a[0] &= rm & (j == 0 ? m_l : 0xffffffffu); a[1] &= rm;
      c[0] &= rm; c[1] &= rm & (j == 2 ? m_r : 0xffffffffu);
      const s16x4 xa = __builtin_bit_cast(s16x4, a), xc = __builtin_bit_cast(s16x4, c);
      const s16x8 fx = {xa[0], xa[1], xa[2], xa[3], xc[0], xc[1], xc[2], xc[3]};
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fd), __builtin_bit_cast(bf16x8, fx), acc[j], 0, 0, 0);
    }
  };
  // four stages of eight k-steps (128 pixels); a stage reads input pixels up to 17 beyond its own: it starts once 146 / 274 / 402 / 512 pixels have landed = operation 3 / 5 / 8 / 10 of every wave
#pragma unroll
  for (int sg = 0; sg < 4; ++sg) {
    if (sg == 0) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if (sg == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if (sg == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    Frags fa, fb;
    read_frags(8 * sg, fa);
#pragma unroll
    for (int k2 = 0; k2 < 8; k2 += 2) {
      const int ks = 8 * sg + k2;
      read_frags(ks + 1, fb);
      wait_frags(fa, 1); mfma3(fa, ks);
      if (k2 + 2 < 8) read_frags(ks + 2, fa);
      if (k2 + 2 < 8) wait_frags(fb, 1); else wait_frags(fb, 0);
      mfma3(fb, ks + 1);
    }
  }
  // ---- the 64 x 64 x 9 tile of dW: one writer per element (K slices: slabs summed in a fixed order) ---------------------------------
  const bool ow = p.ksplit == 1 && p.overwrite && *p.overwrite != 0;
  const int ci = ci0 + cih * 32 + (lane & 31);
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = co0 + coh * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
      const size_t idx = ((size_t)(ty * 3 + j) * p.Cout + co) * p.C + ci;
      if (p.ksplit > 1) p.slabs[(size_t)chunk * 9 * p.Cout * p.C + idx] = acc[j][i];
      else if (ow) p.dw[idx] = acc[j][i];
      else p.dw[idx] += acc[j][i];
    }
}

// wgrad_imgs<W> (round 4): wgrad_img for MORE than 512 pixels (8 x 16 x 16 x 512: four chunks; the 8 x 8 level at batches above 8) WITHOUT K slices.  wgrad_img's 64 x 64 tiles need the
// four chunks as four K slices to fill the chip - 37.7 MB of fp32 slabs written per launch and read again by the batched reduction (151 MB per step at this level).  Here a block
// owns a 32 x 32 tile of dW for all nine taps (256 blocks at 512 x 512) and STREAMS the chunks through a two-stage LDS ring (512 pixels x 32 channels x 2 operands per stage:
// 64-byte pixel rows, the four pixel rows of a transposing read are one contiguous 256 bytes - no swizzle): chunk c + 1 lands while chunk c multiplies.  12 waves = 3 kernel
// rows x 4 k-quarters of a chunk (8 k-steps each, 3 MFMAs per k-step, fragment reads pipelined as in wgrad_img); the quarters meet once, at the end, through LDS; dW is written
// once (stored under the first-writer flag, added otherwise): no slabs, no reduction.
template <int W>
__global__ __launch_bounds__(768) void wgrad_imgs(const WgK p) {
  constexpr int PC = 512, PXB = 64, SLACK = 18 * PXB, TILE = PC * PXB, STAGE = 2 * SLACK + 2 * TILE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = wv >> 2, kq = wv & 3;
  const int ti = (int)blockIdx.x % p.nti, tc = (int)blockIdx.x / p.nti;
  const int co0 = tc * 32, ci0 = ti * 32;
  const int nch = p.ksplit;                             // chunks of 512 pixels (host: M / 512; NOT K slices here)
  const unsigned cbytes = (unsigned)(p.C * 2), obytes = (unsigned)(p.Cout * 2);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.a, (unsigned)((size_t)p.M * p.C * 2)), rd = make_rsrc(p.dy, (unsigned)((size_t)p.M * p.Cout * 2));
  // a DMA piece = 16 pixels x 64 bytes: lane l -> pixel (l >> 2), 16-byte chunk (l & 3)
  const unsigned srcx = (unsigned)(lane >> 2) * cbytes + (unsigned)(ci0 * 2 + (lane & 3) * 16);
  const unsigned srcd = (unsigned)(lane >> 2) * obytes + (unsigned)(co0 * 2 + (lane & 3) * 16);
  auto issue = [&](int c, int st) {                     // chunk c into stage st: 64 pieces, six operations per wave (the last eight slots: dummies)
    unsigned char* sX = smem + st * STAGE + SLACK;
    unsigned char* sD = sX + TILE + SLACK;
    const unsigned pix0 = (unsigned)(c * PC);
#ifdef RUA_IMGS_DBG_NODMA                               // (timing experiments only - results are garbage)
    return;
#endif
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int q = k * 12 + wv, pb = q >> 1;
      if (q >= 2 * (PC / 16)) { const unsigned z = 0u, off = 0x80000000u; asm volatile("buffer_store_dword %0, %1, %2, 0 offen" :: "v"(z), "v"(off), "s"(rd) : "memory"); }
      else if (!(q & 1)) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(sX + pb * 1024), 16, (pix0 + (unsigned)(pb * 16)) * cbytes + srcx, 0, 0, 0);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_void_p)(sD + pb * 1024), 16, (pix0 + (unsigned)(pb * 16)) * obytes + srcd, 0, 0, 0);
    }
  };
  issue(0, 0);
  if (nch > 1) issue(1, 1);

  const unsigned s_a = (unsigned)(size_t)(lds_void_p)smem;
  const int li = lane & 15, g = lane >> 4;
  const int q4 = li >> 2, pp = li & 3;
  const int kh = g >> 1;
  const int hrow = 8 * kh + q4;
  const int chb = 32 * (g & 1) + 8 * pp;                // byte offset of this lane's four channels inside the 64-byte pixel row
  const unsigned dyo = (unsigned)(2 * SLACK + TILE + (kq * 128 + hrow) * PXB + chb);
  unsigned xo[3];
#pragma unroll
  for (int tx = 0; tx < 3; ++tx) xo[tx] = (unsigned)(SLACK + (kq * 128 + hrow + (ty - 1) * W + (tx - 1)) * PXB + chb);
  // tap column 0 reads pixel w - 1: off at w = 0 (element 0 of the first read where the lane's eight pixels start a row); tap column 2 reads w + 1: off at w = W - 1 (element 3 of the
  // second read where they end one) - W = 16: the first / second half of the k-step, W = 8: both (a k-step is two rows)
  const unsigned m_l = (W == 8 || kh == 0) ? 0xffff0000u : 0xffffffffu;
  const unsigned m_r = (W == 8 || kh == 1) ? 0x0000ffffu : 0xffffffffu;

  f32x16 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  struct Frags { s16x4 d0, d1, x0[3], x1[3]; };
  auto read_frags = [&](unsigned base, int k, Frags& f) {
    const unsigned dk = base + dyo + (unsigned)(k * 16 * PXB);
    const unsigned x0a = base + xo[0] + (unsigned)(k * 16 * PXB), x1a = base + xo[1] + (unsigned)(k * 16 * PXB), x2a = base + xo[2] + (unsigned)(k * 16 * PXB);
    asm volatile("ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %8 offset:256\n\t"
                 "ds_read_b64_tr_b16 %2, %9\n\tds_read_b64_tr_b16 %3, %9 offset:256\n\t"
                 "ds_read_b64_tr_b16 %4, %10\n\tds_read_b64_tr_b16 %5, %10 offset:256\n\t"
                 "ds_read_b64_tr_b16 %6, %11\n\tds_read_b64_tr_b16 %7, %11 offset:256"
                 : "=&v"(f.d0), "=&v"(f.d1), "=&v"(f.x0[0]), "=&v"(f.x1[0]), "=&v"(f.x0[1]), "=&v"(f.x1[1]), "=&v"(f.x0[2]), "=&v"(f.x1[2])
                 : "v"(dk), "v"(x0a), "v"(x1a), "v"(x2a) : "memory");
  };
  auto wait_frags = [&](Frags& f, int pending) {
    if (pending) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f.d0), "+v"(f.d1), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.d0), "+v"(f.d1), "+v"(f.x0[0]), "+v"(f.x1[0]), "+v"(f.x0[1]), "+v"(f.x1[1]), "+v"(f.x0[2]), "+v"(f.x1[2]) :: "memory");
  };
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  auto mfma3 = [&](const Frags& f, int k) {             // k-step 8 kq + k of the chunk = image row (8 kq + k) & 15 (W = 16: two images per chunk), rows 2 (8 kq + k) + {0, 1} (W = 8)
    const int h = (W == 8) ? ((2 * (8 * kq + k) + kh) & 7) : ((8 * kq + k) & 15);
    const bool rows_ok = !((ty == 0 && h == 0) || (ty == 2 && h == W - 1));
    const unsigned rm = rows_ok ? 0xffffffffu : 0u;
    const s16x8 fd = {f.d0[0], f.d0[1], f.d0[2], f.d0[3], f.d1[0], f.d1[1], f.d1[2], f.d1[3]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      u32x2 a = __builtin_bit_cast(u32x2, f.x0[j]), c = __builtin_bit_cast(u32x2, f.x1[j]);
      a[0] &= rm & (j == 0 ? m_l : 0xffffffffu); a[1] &= rm;
      c[0] &= rm; c[1] &= rm & (j == 2 ? m_r : 0xffffffffu);
      const s16x4 xa = __builtin_bit_cast(s16x4, a), xc = __builtin_bit_cast(s16x4, c);
      const s16x8 fx = {xa[0], xa[1], xa[2], xa[3], xc[0], xc[1], xc[2], xc[3]};
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fd), __builtin_bit_cast(bf16x8, fx), acc[j], 0, 0, 0);
    }
  };

  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");       // chunk c has landed (chunk c + 1 stays in flight)
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const unsigned base = s_a + (unsigned)((c & 1) * STAGE);
    Frags fa, fb;
#ifdef RUA_IMGS_DBG_NOMFMA
    if (p.M > 0) continue;
#endif
    read_frags(base, 0, fa);
#pragma unroll
    for (int k2 = 0; k2 < 8; k2 += 2) {
      read_frags(base, k2 + 1, fb);
      wait_frags(fa, 1); mfma3(fa, k2);
      if (k2 + 2 < 8) read_frags(base, k2 + 2, fa);
      if (k2 + 2 < 8) wait_frags(fb, 1); else wait_frags(fb, 0);
      mfma3(fb, k2 + 1);
    }
    if (c + 2 < nch) {
      __builtin_amdgcn_s_barrier();                     // every wave is done with this stage
      issue(c + 2, c & 1);
    }
  }
  // ---- the k-quarters meet in LDS (the ring is free), quarter 0 writes the 32 x 32 x 9 tile -----------------------------------------
  __syncthreads();
#ifdef RUA_IMGS_DBG_NOEPI
  if (p.M > 0) { if (acc[0][0] == 123.456f) p.dw[0] = 1; return; }
#endif
  // every wave leaves its three accumulators in LDS ([k-quarter][tap][register][lane]: 144 KB, the ring is free); then all 768 threads sum the four quarters of three float4
  // each - four consecutive input channels of one (tap, output channel) = four consecutive lanes of one register - and write dW in 128-byte row segments
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) red[(((kq * 3 + ty) * 3 + j) * 16 + i) * 64 + lane] = acc[j][i];
  __syncthreads();
  const bool ow = p.overwrite && *p.overwrite != 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int o4 = tid + 768 * r;                       // float4 index in [tap][32 co][8 x 4 ci]
    const int tap = o4 >> 8, col = (o4 >> 3) & 31, c4 = (o4 & 7) * 4;
    const int i = (col & 3) + 4 * (col >> 3), lh = (col >> 2) & 1;
    const float* src = red + (tap * 16 + i) * 64 + lh * 32 + c4;
    f32x4 v = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
    for (int q = 1; q < 4; ++q) v += *reinterpret_cast<const f32x4*>(src + q * 9 * 16 * 64);
    float* dst = p.dw + ((size_t)tap * p.Cout + co0 + col) * p.C + ci0 + c4;
    if (!ow) v += *reinterpret_cast<const f32x4*>(dst);
    *reinterpret_cast<f32x4*>(dst) = v;
  }
}

// dw[tap][co][ci] += sum over the gx partials of its output-channel half.  256 threads = 64 float4 columns x 4 slice lanes: a wave
// reads 1 KiB runs of a partial, eight loads in flight per thread, the four lanes are folded through LDS in a fixed order
// (deterministic).  (Before: 16 columns x 16 lanes - 256-byte runs, four loads in flight, 4x the blocks.)
constexpr int TAPS_RED_COLS = 64;
__device__ __forceinline__ void wgrad_taps_reduce_body(const float* __restrict__ scratch, float* __restrict__ dw, int CC, int gx, int vblock, int overwrite = 0) {
  __shared__ float4 sh[256];
  const int total4 = 9 * CC * CC / 4;
  const int el = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int e4 = vblock * TAPS_RED_COLS + el;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  auto add4 = [](float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; };
  if (e4 < total4) {
    const int e = e4 * 4;
    const int tap = e / (CC * CC), r = e - tap * CC * CC, co = r / CC, ci = r - co * CC;
    const float* src = scratch + ((size_t)(co >> 5) * gx * 9 + tap) * 32 * CC + (co & 31) * CC + ci;
    const size_t pstride = (size_t)9 * 32 * CC;
    int b = sl;
    for (; b + 28 < gx; b += 32) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(src + (size_t)(b + 4 * u) * pstride);
      float4 a = v[0], c = v[4];
      add4(a, v[1]); add4(c, v[5]); add4(a, v[2]); add4(c, v[6]); add4(a, v[3]); add4(c, v[7]);
      add4(a, c); add4(s, a);
    }
    for (; b < gx; b += 4) add4(s, *reinterpret_cast<const float4*>(src + (size_t)b * pstride));
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  if (sl == 0 && e4 < total4) {
    float4 t = sh[el];
    add4(t, sh[64 + el]); add4(t, sh[128 + el]); add4(t, sh[192 + el]);
    float4* d = reinterpret_cast<float4*>(dw + (size_t)e4 * 4);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!overwrite) o = *d;
    add4(o, t);
    *d = o;
  }
}

__global__ __launch_bounds__(256) void wgrad_taps_reduce(const float* __restrict__ scratch, float* __restrict__ dw, int CC, int gx) {
  wgrad_taps_reduce_body(scratch, dw, CC, gx, (int)blockIdx.x);
}

// rua_conv_wgrad_group: the launchers below record instead of launching while g_wg_group is set
struct WgGroupCapture {
  int n;
  int kind[RUA_MAX_WGRAD_GROUP];                 // 0 wgrad_kernel<bf16>, 1 wgrad_taps<32>, 2 wgrad_taps<64>, 3 wgrad_dmap
  unsigned gx[RUA_MAX_WGRAD_GROUP]; int smem[RUA_MAX_WGRAD_GROUP];
  WgK g[RUA_MAX_WGRAD_GROUP]; WgdK d[RUA_MAX_WGRAD_GROUP]; WgtK t[RUA_MAX_WGRAD_GROUP];
  int post[RUA_MAX_WGRAD_GROUP];                 // reduction the member wants right after its grid (not deferred): 0 none, 1 block partials, 2 slabs
  const float* part[RUA_MAX_WGRAD_GROUP]; float* dw[RUA_MAX_WGRAD_GROUP]; long long ndw[RUA_MAX_WGRAD_GROUP]; int parts[RUA_MAX_WGRAD_GROUP], CC[RUA_MAX_WGRAD_GROUP], rblocks[RUA_MAX_WGRAD_GROUP];
};
static thread_local WgGroupCapture* g_wg_group = nullptr;

// wgrad_rows32 variants: kind 4 + 2 * (NPG == 2) + (no BatchNorm on load)
static void launch_rows32(int kind, bool grouped, dim3 grid, int smem, hipStream_t st, const WgtK* one, const WgtKG* many) {
  static RuaPerDevFlag attr_[18];
  bool& attr = attr_[(kind - 4) * 2 + (grouped ? 1 : 0)].get();
#define RUA_ROWS_GO(NPG_, BN_) do { \
    if (grouped) { if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_rows32_g<NPG_, BN_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
                   hipLaunchKernelGGL((wgrad_rows32_g<NPG_, BN_>), grid, dim3(NPG_ * 192), smem, st, *many); } \
    else { if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_rows32<NPG_, BN_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
           hipLaunchKernelGGL((wgrad_rows32<NPG_, BN_>), grid, dim3(NPG_ * 192), smem, st, *one); } } while (0)
#define RUA_ROWS64_GO(BN_) do { \
    if (grouped) { if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_rows64_g<BN_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
                   hipLaunchKernelGGL((wgrad_rows64_g<BN_>), grid, dim3(768), smem, st, *many); } \
    else { if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_rows64<BN_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
           hipLaunchKernelGGL((wgrad_rows64<BN_>), grid, dim3(768), smem, st, *one); } } while (0)
#define RUA_ROWSX_GO(MODE_) do { \
    if (grouped) { if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_rowsx_g<MODE_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
                   hipLaunchKernelGGL((wgrad_rowsx_g<MODE_>), grid, dim3(768), smem, st, *many); } \
    else { if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_rowsx<MODE_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
           hipLaunchKernelGGL((wgrad_rowsx<MODE_>), grid, dim3(768), smem, st, *one); } } while (0)
  switch (kind) {
    case 4: RUA_ROWS_GO(4, true); break;
    case 5: RUA_ROWS_GO(4, false); break;
    case 6: RUA_ROWS_GO(2, true); break;
    case 7: RUA_ROWS_GO(2, false); break;
    case 8: RUA_ROWS64_GO(true); break;                  // C = 64, 128-pixel rows
    case 9: RUA_ROWS64_GO(false); break;
    case 11: RUA_ROWSX_GO(0); break;                     // the slot-stream form (wgrad_rowsx.inc): C = 128 on 64-pixel rows (grid.y = 2) ...
    case 12: RUA_ROWSX_GO(1); break;                     // ... and C = 256 on 32-pixel rows, two images per stage (grid.y = 4 output-channel slices x 2 input-channel halves)
    default:                                             // 10: C = 128, 64-pixel rows (grid.y = output-channel slice)
      if (grouped) { if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_rows128_g), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; }
                     hipLaunchKernelGGL(wgrad_rows128_g, grid, dim3(768), smem, st, *many); }
      else { if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_rows128), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; }
             hipLaunchKernelGGL(wgrad_rows128, grid, dim3(768), smem, st, *one); }
      break;
  }
#undef RUA_ROWSX_GO
#undef RUA_ROWS64_GO
#undef RUA_ROWS_GO
}

static int launch_wgrad_taps(const rua_wgrad_desc* d, hipStream_t st) {
  const int CC = d->C;
  WgtK k;
  k.a = (const unsigned char*)d->a; k.dy = (const unsigned char*)d->dy; k.scratch = (float*)d->workspace; k.dw = d->dw;
  k.H = d->H; k.W = d->W; k.N = d->N; k.dil = d->dil;
  k.in_scale = d->in_scale; k.in_shift = d->in_shift; k.in_relu = d->in_relu; k.sx = 0;
  const long long M = (long long)d->N * d->H * d->W;
  if (CC == 256 || (CC == 128 && (g_tune.wgrad_rows & 64))) {
    // wgrad_rowsx: gx blocks per grid row share the slot stream of the member evenly; grid.y = (output-channel slice, input-channel half); a block leaves two
    // partials [9][32][C] (or its 128 columns of them), so C / 32 x gx of them <= one per CU - the workspace contract of the all-taps kernels
    const int ncu_ = rua_cu_count();
    const int gy_ = CC == 256 ? 8 : 2;
    const int share_ = (g_tune.wgrad_taps_share && d->group_members > 1) ? d->group_members : 1;
    int gx_ = ncu_ / share_ / gy_;
    if (gx_ > ncu_ / (CC / 32)) gx_ = ncu_ / (CC / 32);
    const long long U_ = (long long)(CC == 256 ? d->N / 2 : d->N) * (d->H + d->dil);
    if (gx_ > U_ / 4) gx_ = (int)(U_ / 4);               // >= 4 slots behind a block's three-row fill
    if (gx_ < 1) gx_ = 1;
    k.NPG = 1; k.strips = 1; k.halo = 0; k.halo4 = 0; k.group_bytes = 0; k.nchains = 0; k.spc = 0; k.seglen = 0; k.njobs = 0; k.jpw = 0;
    k.gx = gx_; k.nworkers = gx_;
    k.abytes = (unsigned)((size_t)M * CC * 2); k.dybytes = k.abytes;
    const size_t smem_ = (size_t)32 * 256 + 5 * (size_t)96 * 256 + 3 * (size_t)64 * 128;
    const int rblocks_ = rua_div_up(9 * CC * CC / 4, TAPS_RED_COLS);
    const int kd_ = CC == 256 ? 12 : 11;
    note_pending(1, gx_, (long long)9 * CC * CC, (const float*)k.scratch, d->dw, CC, rblocks_);
    if (g_wgrad_dry) return RUA_OK;
    if (g_wg_group && (g_tune.wgrad_group & 4) && g_wg_group->n < RUA_MAX_WGRAD_GROUP) {
      WgGroupCapture& c = *g_wg_group; const int i = c.n++;
      c.kind[i] = kd_; c.gx[i] = gx_; c.smem[i] = (int)smem_; c.t[i] = k;
      c.post[i] = d->defer ? 0 : 1; c.part[i] = k.scratch; c.dw[i] = d->dw; c.CC[i] = CC; c.parts[i] = gx_; c.rblocks[i] = rblocks_; c.ndw[i] = 0;
      return RUA_OK;
    }
    launch_rows32(kd_, false, dim3(gx_, gy_), (int)smem_, st, &k, nullptr);
    RUA_LAUNCH_CHECK("wgrad_rowsx");
    if (d->defer) return RUA_OK;
    record_mid_event(st);
    hipLaunchKernelGGL(wgrad_taps_reduce, dim3(rblocks_), dim3(256), 0, st, (const float*)k.scratch, d->dw, CC, gx_);
    RUA_LAUNCH_CHECK("wgrad_taps_reduce");
    return RUA_OK;
  }
  if (CC == 128) {
    // wgrad_rows128: blocks (x) per output-channel slice (y = 2); a block leaves two partials (the halves of its slice), the scratch holds ncu of them
    const int ncu_ = rua_cu_count();
    const int share_ = (g_tune.wgrad_taps_share && d->group_members > 1) ? d->group_members : 1;
    int blocks = ncu_ / share_ / 2 > 0 ? ncu_ / share_ / 2 : 1;
    if (blocks > ncu_ / 4) blocks = ncu_ / 4;
    const int ny_ = (d->H + d->dil - 1) / d->dil;
    k.NPG = 1; k.strips = 1; k.halo = 0; k.halo4 = 0; k.group_bytes = 0;
    k.nchains = d->N * d->dil;
    int spc2 = blocks / k.nchains;
    if (spc2 < 1) spc2 = 1;
    if (spc2 > (ny_ + 3) / 4) spc2 = (ny_ + 3) / 4;
    if (spc2 < 1) spc2 = 1;
    k.seglen = (ny_ + spc2 - 1) / spc2;
    k.spc = (ny_ + k.seglen - 1) / k.seglen;
    k.njobs = k.nchains * k.spc;
    const int gx_ = k.njobs < blocks ? k.njobs : blocks;
    k.gx = gx_; k.nworkers = gx_;
    k.jpw = (k.njobs + gx_ - 1) / gx_;
    k.abytes = (unsigned)((size_t)M * CC * 2); k.dybytes = k.abytes;
    const size_t smem_ = (size_t)32 * 256 + 5 * (size_t)(64 + 32) * 256 + 3 * (size_t)64 * 128;
    const int rblocks_ = rua_div_up(9 * CC * CC / 4, TAPS_RED_COLS);
    note_pending(1, gx_, (long long)9 * CC * CC, (const float*)k.scratch, d->dw, CC, rblocks_);
    if (g_wgrad_dry) return RUA_OK;
    if (g_wg_group && (g_tune.wgrad_group & 4) && g_wg_group->n < RUA_MAX_WGRAD_GROUP) {
      WgGroupCapture& c = *g_wg_group; const int i = c.n++;
      c.kind[i] = 10; c.gx[i] = gx_; c.smem[i] = (int)smem_; c.t[i] = k;
      c.post[i] = d->defer ? 0 : 1; c.part[i] = k.scratch; c.dw[i] = d->dw; c.CC[i] = CC; c.parts[i] = gx_; c.rblocks[i] = rblocks_; c.ndw[i] = 0;
      return RUA_OK;
    }
    launch_rows32(10, false, dim3(gx_, 2), (int)smem_, st, &k, nullptr);
    RUA_LAUNCH_CHECK("wgrad_rows128");
    if (d->defer) return RUA_OK;
    record_mid_event(st);
    hipLaunchKernelGGL(wgrad_taps_reduce, dim3(rblocks_), dim3(256), 0, st, (const float*)k.scratch, d->dw, CC, gx_);
    RUA_LAUNCH_CHECK("wgrad_taps_reduce");
    return RUA_OK;
  }
  k.halo = 64 + 2 * d->dil;
  k.halo4 = (k.halo + 3) / 4 * 4;
  k.group_bytes = 64 * 64 + 3 * k.halo4 * CC * 2;
  k.NPG = (CC == 32) ? 4 : 2;                          // 12 waves per block either way (3 kernel rows x CC/32 halves per group)
  const int gy = CC / 32;
  const int ncu = rua_cu_count();
  // the members of a grouped launch share ONE round of blocks (four members of 256 blocks each ran four rounds, every block with
  // its own prologue and 36 - 74 KB of partials to write and to reduce): tuning key wgrad_taps_share
  const int share = (g_tune.wgrad_taps_share && (g_tune.wgrad_group & (CC == 32 ? 2 : 4)) && d->group_members > 1) ? d->group_members : 1;
  const int target = (ncu / gy) * k.NPG / share;       // pixel groups wanted: one block per CU and output-channel half
  k.strips = d->W / 64;
  k.nchains = d->N * k.strips * d->dil;
  const int ny = (d->H + d->dil - 1) / d->dil;         // lattice rows of the longest chain
  int spc = target / k.nchains;                        // segments per chain (jobs <= groups where possible: one round)
  if (spc < 1) spc = 1;
  if (spc > ny) spc = ny;
  k.seglen = (ny + spc - 1) / spc;
  k.spc = (ny + k.seglen - 1) / k.seglen;
  k.njobs = k.nchains * k.spc;
  int gx = (k.njobs + k.NPG - 1) / k.NPG;
  if (gx > ncu / gy / share) gx = ncu / gy / share;    // one block per CU and output-channel half (of this member's share); extra jobs are queued
  if (gx < 1) gx = 1;
  k.gx = gx;
  k.nworkers = gx * k.NPG;
  k.jpw = (k.njobs + k.nworkers - 1) / k.nworkers;
  k.abytes = (unsigned)((size_t)M * CC * 2); k.dybytes = k.abytes;
  size_t smem = (size_t)k.group_bytes * k.NPG;
  const size_t red = (size_t)(k.NPG - 1) * 3 * (CC / 32) * 3 * 16 * 64 * 4;
  if (red > smem) smem = red;
  // full-width rows at C = 32: wgrad_rows32 (tuning key wgrad_rows) - the block's pixel groups share ONE ring of whole rows; a worker is a block
  int rows_kind = 0;
  if (g_tune.wgrad_rows && CC == 32 && (d->W == 256 || d->W == 128) && d->dil <= 31 && (!d->in_scale || d->in_relu) && (size_t)M * CC * 2 < 0x80000000ull) {
    const int npg = d->W / 64;
    rows_kind = 4 + (npg == 2 ? 2 : 0) + (d->in_scale ? 0 : 1);
    k.NPG = npg; k.strips = 1;
    k.nchains = d->N * d->dil;
    const int blocks = ncu / share > 0 ? ncu / share : 1;
    int spc2 = blocks / k.nchains;
    if (spc2 < 1) spc2 = 1;
    if (spc2 > (ny + 3) / 4) spc2 = (ny + 3) / 4;       // >= 4 rows per segment (a segment re-reads two window rows)
    if (spc2 < 1) spc2 = 1;
    k.seglen = (ny + spc2 - 1) / spc2;
    k.spc = (ny + k.seglen - 1) / k.seglen;
    k.njobs = k.nchains * k.spc;
    gx = k.njobs < blocks ? k.njobs : blocks;
    if (g_tune.wgrad_rows & 128) {                       // the slot stream (WgSlots): every block an equal share of the rows + separators
      const long long U_ = (long long)d->N * (d->H + d->dil);
      k.sx = 1; gx = (int)(U_ / 4 < blocks ? (U_ / 4 > 0 ? U_ / 4 : 1) : blocks);
    }
    k.gx = gx; k.nworkers = gx;
    k.jpw = (k.njobs + gx - 1) / gx;
    smem = (size_t)32 * 64 + 6 * (size_t)(d->W + 32) * 64 + 3 * (size_t)d->W * 64 + 128 * 4;
    const size_t red2 = (size_t)(npg - 1) * 3 * 3 * 16 * 64 * 4;
    if (red2 > smem) smem = red2;
  }
  // C = 64 on 128-pixel rows (the level-2 ResBlock): wgrad_rows64 - a block owns whole rows and BOTH output-channel halves (tuning key wgrad_rows & 2)
  if ((g_tune.wgrad_rows & 2) && CC == 64 && d->W == 128 && d->dil <= 31 && (!d->in_scale || d->in_relu) && (size_t)M * CC * 2 < 0x80000000ull) {
    rows_kind = 8 + (d->in_scale ? 0 : 1);
    k.NPG = 2; k.strips = 1;
    k.nchains = d->N * d->dil;
    int blocks = ncu / share > 0 ? ncu / share : 1;     // one round of blocks for the group; a block leaves TWO partials (one per output-channel half) and the
    if (blocks > ncu / 2) blocks = ncu / 2;             // scratch of wgrad_taps_kernel<64> holds ncu of them per weight gradient
    int spc2 = blocks / k.nchains;
    if (spc2 < 1) spc2 = 1;
    if (spc2 > (ny + 3) / 4) spc2 = (ny + 3) / 4;       // >= 4 rows per segment (a segment re-reads two window rows)
    if (spc2 < 1) spc2 = 1;
    k.seglen = (ny + spc2 - 1) / spc2;
    k.spc = (ny + k.seglen - 1) / k.seglen;
    k.njobs = k.nchains * k.spc;
    gx = k.njobs < blocks ? k.njobs : blocks;
    if (g_tune.wgrad_rows & 128) {
      const long long U_ = (long long)d->N * (d->H + d->dil);
      k.sx = 1; gx = (int)(U_ / 4 < blocks ? (U_ / 4 > 0 ? U_ / 4 : 1) : blocks);
    }
    k.gx = gx; k.nworkers = gx;
    k.jpw = (k.njobs + gx - 1) / gx;
    smem = (size_t)32 * 128 + 5 * (size_t)(128 + 32) * 128 + 3 * (size_t)128 * 128 + 256 * 4;
  }
  const int rblocks = rua_div_up(9 * CC * CC / 4, TAPS_RED_COLS);
  note_pending(1, gx, (long long)9 * CC * CC, (const float*)k.scratch, d->dw, CC, rblocks);
  if (g_wgrad_dry) return RUA_OK;
  if (g_wg_group && (g_tune.wgrad_group & (CC == 32 ? 2 : 4)) && g_wg_group->n < RUA_MAX_WGRAD_GROUP) {
    WgGroupCapture& c = *g_wg_group; const int i = c.n++;
    c.kind[i] = rows_kind ? rows_kind : (CC == 32 ? 1 : 2); c.gx[i] = gx; c.smem[i] = (int)smem; c.t[i] = k;
    c.post[i] = d->defer ? 0 : 1; c.part[i] = k.scratch; c.dw[i] = d->dw; c.CC[i] = CC; c.parts[i] = gx; c.rblocks[i] = rblocks; c.ndw[i] = 0;
    return RUA_OK;
  }
  static RuaPerDevFlag attr32f, attr64f;
  bool& attr32 = attr32f.get(); bool& attr64 = attr64f.get();
  if (rows_kind) launch_rows32(rows_kind, false, dim3(gx), (int)smem, st, &k, nullptr);
  else if (CC == 32) {
    if (!attr32) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_taps_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr32 = true; }
    hipLaunchKernelGGL((wgrad_taps_kernel<32>), dim3(gx, gy), dim3(768), smem, st, k);
  } else {
    if (!attr64) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_taps_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr64 = true; }
    hipLaunchKernelGGL((wgrad_taps_kernel<64>), dim3(gx, gy), dim3(768), smem, st, k);
  }
  RUA_LAUNCH_CHECK("wgrad_taps_kernel");
  if (d->defer) return RUA_OK;                         // the caller sums the block partials later (rua_wgrad_reduce_batch)
  record_mid_event(st);
  hipLaunchKernelGGL(wgrad_taps_reduce, dim3(rblocks), dim3(256), 0, st, (const float*)k.scratch, d->dw, CC, gx);
  RUA_LAUNCH_CHECK("wgrad_taps_reduce");
  return RUA_OK;
}

// =========================================================================================
// wgrad_pw: the weight gradient of the narrow 1x1 convolutions (C, Cout <= 64: stem, PSP branches, combine / upsampling
// convs of the top levels).  These are memory-bound (67 MB in for a 4 KB..16 KB dW at 256x256x32) and were slow on
// wgrad_kernel for two reasons: one 64x64 tile per block with two block barriers per 64 pixels, and up to 512 blocks
// adding the SAME few hundred dW addresses with float atomics (same-address atomics serialise at ~25 ns: 13 us).
// Here every WAVE streams its own pixel range with no block barrier at all: 16-byte coalesced loads (two iterations
// in flight in registers) -> the wave's private LDS tile -> transposing fragment reads -> MFMA 32x32x16; LDS operations
// of one wave execute in order, so write -> read -> next write needs no barrier.  The four waves of a block add their
// accumulators in LDS, the block adds the result into one of R replica buffers (atomic chain nblocks / R long), and the
// block that draws the last ticket sums the replicas into dW (one writer, plain +=) and leaves replicas and ticket
// zero for the next launch.
struct WgpK {
  const unsigned char* a; const unsigned char* dy; float* dw; float* rep; int* cnt;
  int C, Cout, Hs, Ws, H, W, stride, wshift, hshift, dense, R;
  int M, px_per_wave;
  unsigned abytes, dybytes;
  int nblk;                         // blocks of this member (= gridDim.x of a launch of its own; a grouped launch has the grid of its largest member)
  float* slabs;                     // round 5: block b stores its sum as partial [b][Cout][C] here (summed in a fixed order by wgrad_slab_reduce / rua_wgrad_reduce_batch); null: replicas + tickets
};
struct WgpKG { WgpK k[RUA_MAX_BRANCH]; };
// rua_conv_wgrad_group: wgrad_pw members (own workspaces: own replicas and tickets) are recorded here and issued as ONE grid per (NCO, NCI) form
struct WgPwCapture { int n; WgpK k[RUA_MAX_BRANCH]; int form[RUA_MAX_BRANCH]; int post[RUA_MAX_BRANCH]; };      // post: the member's partials are summed right behind the grid (not deferred)
static thread_local WgPwCapture* g_wg_pw = nullptr;
constexpr int WG_PW_REPLICAS = 16;
constexpr int64_t WG_PW_TAIL = (int64_t)WG_PW_REPLICAS * 64 * 64 * 4 + 8192;   // replicas + two ticket pages at the end of the workspace

template <int NCO, int NCI> static constexpr int wgrad_pw_smem() {
  constexpr int PXW = (NCO + NCI <= 2) ? 32 : 16;
  constexpr int WAVE_LDS = PXW * ((NCO == 2 ? 192 : 64) + (NCI == 2 ? 192 : 64));
  constexpr int RED = 4 * NCO * 32 * (NCI * 32 + 1) * 4;
  return (16 * WAVE_LDS > RED ? 16 * WAVE_LDS : RED) + 16;
}

template <int NCO, int NCI>
__device__ __forceinline__ void wgrad_pw_body(const WgpK& p) {
  constexpr int NW = 16, NT = NW * 64;                           // waves / threads per block
  constexpr int PXW = (NCO + NCI <= 2) ? 32 : 16;                  // pixels per wave iteration
  constexpr int ROWB_D = NCO == 2 ? 192 : 64, ROWB_A = NCI == 2 ? 192 : 64;   // 64 ch + pad / 32 ch: conflict-free tr reads
  constexpr int WAVE_LDS = PXW * (ROWB_D + ROWB_A);
  constexpr int NLD = PXW * NCO * 4 / 64, NLA = PXW * NCI * 4 / 64;          // 16-byte pieces per lane per iteration
  constexpr int RED = 4 * NCO * 32 * (NCI * 32 + 1) * 4;            // four padded fp32 slots for the block sum
  constexpr int SMEM = wgrad_pw_smem<NCO, NCI>() - 16;
  static_assert(SMEM >= NW * WAVE_LDS && SMEM >= RED, "LDS size");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int& s_ticket = *reinterpret_cast<int*>(smem + SMEM);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  unsigned char* sD = smem + wid * WAVE_LDS;
  unsigned char* sA = sD + PXW * ROWB_D;

  const int gw = blockIdx.x * NW + wid;
  const int k_begin = gw * p.px_per_wave;
  int k_end = k_begin + p.px_per_wave; if (k_end > p.M) k_end = p.M;

  // loop-invariant piece geometry of this lane
  const int PD = p.Cout >> 3, PA = p.C >> 3;
  int dpx[NLD], doff[NLD], dlds[NLD], apx[NLA], apc[NLA], alds[NLA];
#pragma unroll
  for (int j = 0; j < NLD; ++j) {
    const int e = lane + 64 * j, px = e / PD, pc = e - px * PD;
    dpx[j] = px < PXW ? px : (1 << 30);                            // idle lane: never in range
    doff[j] = (px * p.Cout + pc * 8) * 2; dlds[j] = px * ROWB_D + pc * 16;
  }
#pragma unroll
  for (int j = 0; j < NLA; ++j) {
    const int e = lane + 64 * j, px = e / PA, pc = e - px * PA;
    apx[j] = px < PXW ? px : (1 << 30);
    apc[j] = pc * 8; alds[j] = px * ROWB_A + pc * 16;
  }
  const __amdgpu_buffer_rsrc_t rd_ = make_rsrc(p.dy, p.dybytes), ra_ = make_rsrc(p.a, p.abytes);
  uint4 rd[2][NLD], rx[2][NLA];
  auto load = [&](int set, int k0) {
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const bool in = (long long)k0 + dpx[j] < k_end;
      rd[set][j] = bufload16(rd_, in ? (unsigned)(k0 * p.Cout * 2 + doff[j]) : RUA_OOB);
    }
#pragma unroll
    for (int j = 0; j < NLA; ++j) {
      const bool in = (long long)k0 + apx[j] < k_end;
      const int mm = k0 + (apx[j] & 31);
      const int w = mm & (p.W - 1), h = (mm >> p.wshift) & (p.H - 1), n = mm >> (p.wshift + p.hshift);
      const int gen = ((n * p.Hs + h * p.stride) * p.Ws + w * p.stride) * p.C;   // only meaningful when !dense (power-of-two maps)
      const int pix = p.dense ? mm * p.C : gen;
      rx[set][j] = bufload16(ra_, in ? (unsigned)((pix + apc[j]) * 2) : RUA_OOB);
    }
  };
  f32x16 acc[NCO][NCI];
#pragma unroll
  for (int a = 0; a < NCO; ++a)
#pragma unroll
    for (int b = 0; b < NCI; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
  const int li = lane & 15, g = lane >> 4;
  const int chan = 16 * (g & 1) + 4 * (li & 3), hrow = 8 * (g >> 1) + (li >> 2);
  typedef s16x4 __attribute__((address_space(3))) * lds4;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  auto consume = [&](int set) {
#pragma unroll
    for (int j = 0; j < NLD; ++j)
      if (dpx[j] < PXW) *reinterpret_cast<uint4*>(sD + dlds[j]) = rd[set][j];
#pragma unroll
    for (int j = 0; j < NLA; ++j)
      if (apx[j] < PXW) *reinterpret_cast<uint4*>(sA + alds[j]) = rx[set][j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int kk = 0; kk < PXW / 16; ++kk) {
      bf16x8 fa[NCO], fb[NCI];
#pragma unroll
      for (int a = 0; a < NCO; ++a) {
        const unsigned char* ad = sD + (kk * 16 + hrow) * ROWB_D + (a * 32 + chan) * 2;
        const s16x4 d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ad));
        const s16x4 d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ad + 4 * ROWB_D));
        const s16x8 f = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
        fa[a] = __builtin_bit_cast(bf16x8, f);
      }
#pragma unroll
      for (int b = 0; b < NCI; ++b) {
        const unsigned char* ax = sA + (kk * 16 + hrow) * ROWB_A + (b * 32 + chan) * 2;
        const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ax));
        const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(ax + 4 * ROWB_A));
        const s16x8 f = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        fb[b] = __builtin_bit_cast(bf16x8, f);
      }
#pragma unroll
      for (int a = 0; a < NCO; ++a)
#pragma unroll
        for (int b = 0; b < NCI; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  // channels beyond C / Cout of a 32-wide MFMA tile read LDS bytes no load ever wrote: zero the wave's tile once so that
  // they are zeros (a NaN pattern there would only reach output elements that are never stored, but zeros cost nothing)
  for (int o = lane * 16; o < WAVE_LDS; o += 64 * 16) *reinterpret_cast<uint4*>(sD + o) = make_uint4(0, 0, 0, 0);
  __builtin_amdgcn_wave_barrier();
  // two iterations in flight; out-of-range iterations load zeros (range-checked offsets), so the loop needs no tail
  load(0, k_begin);
  load(1, k_begin + PXW);
  for (int k0 = k_begin; k0 < k_end; k0 += 2 * PXW) {
    consume(0);
    load(0, k0 + 2 * PXW);
    consume(1);
    load(1, k0 + 3 * PXW);
  }
  // Block sum of the 16 waves' accumulators through four LDS slots with plain stores (ds_add_f32 from several waves on the
  // same words took ~20 us per launch): wave w uses slot w & 3 in round w >> 2 (round 0 stores, rounds 1-3 add); every
  // thread then sums the four slots of its elements.
  __syncthreads();
  constexpr int RW = NCI * 32 + 1;                                 // padded row
  constexpr int SLOT = NCO * 32 * RW;
  float* slot = reinterpret_cast<float*>(smem) + (wid & 3) * SLOT;
  const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int round = 0; round < NW / 4; ++round) {
    if ((wid >> 2) == round) {
#pragma unroll
      for (int a = 0; a < NCO; ++a)
#pragma unroll
        for (int b = 0; b < NCI; ++b)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float* q = &slot[(a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh) * RW + b * 32 + lr];
            *q = round == 0 ? acc[a][b][i] : *q + acc[a][b][i];
          }
    }
    __syncthreads();
  }
  const int nel = p.Cout * p.C;
  // The block adds its sum into replica (block % R) with RETURNING atomics: when the old values are back the adds have
  // been performed at the device's coherence point, so the ticket below needs no release fence (an agent-scope release
  // would write back this XCD's whole L2), and the last block reads the replicas with atomic exchanges (read and reset
  // in one round trip, all R in flight), which needs no acquire fence either.
  const float* s0 = reinterpret_cast<const float*>(smem);
  constexpr int NPT = NCO * NCI;                                   // elements per thread at the full tile width
  if (p.slabs) {
    // Round 5: the block's sum leaves as ONE partial with plain stores and the kernel ends here - the atomics, the two ticket round trips and the finishing
    // block below were 5 - 8 us of dependent latency behind 6 - 11 us of streaming; the partials (<= 16 KB a block) are summed with every other pending
    // weight gradient by rua_wgrad_reduce_batch, in a fixed order: the narrow 1x1 weight gradients are bit-reproducible now as well.
    float* part = p.slabs + (size_t)blockIdx.x * nel;
#pragma unroll
    for (int e = 0; e < NPT; ++e) {
      const int o = tid + e * NT;
      const int co = o / p.C, ci = o - co * p.C;
      if (o < nel) { const float* q = s0 + co * RW + ci; part[o] = (q[0] + q[SLOT]) + (q[2 * SLOT] + q[3 * SLOT]); }
    }
    return;
  }
  float* rep = p.rep + (size_t)(blockIdx.x % p.R) * nel;
  float olds[NPT];
#pragma unroll
  for (int e = 0; e < NPT; ++e) {                                  // unrolled: all of a thread's adds are in flight together
    const int o = tid + e * NT;
    const int co = o / p.C, ci = o - co * p.C;
    olds[e] = 0.f;
    if (o < nel) { const float* q = s0 + co * RW + ci; olds[e] = unsafeAtomicAdd(rep + o, (q[0] + q[SLOT]) + (q[2 * SLOT] + q[3 * SLOT])); }
  }
#pragma unroll
  for (int e = 0; e < NPT; ++e) asm volatile("" : "+v"(olds[e]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // Two-level ticket (one counter for all blocks is a same-address chain of ~13 ns per block: 13 us at 1024 blocks, and so
  // are 16 counters in one cache line): the group counters sit 256 B apart, the last block of each replica group draws
  // from the top counter (its own page), the last of those finishes.
  if (tid == 0) {
    const int G = p.nblk < p.R ? p.nblk : p.R;
    const int g = blockIdx.x % p.R;
    const int gsize = (p.nblk - g + p.R - 1) / p.R;
    int last = 0;
    int* cg = p.cnt + g * 64;
    int* ctop = p.cnt + WG_PW_REPLICAS * 64;
    if (__hip_atomic_fetch_add(cg, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1) {
      __hip_atomic_store(cg, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__hip_atomic_fetch_add(ctop, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) {
        __hip_atomic_store(ctop, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = 1;
      }
    }
    s_ticket = last;
  }
  __syncthreads();
  if (!s_ticket) return;
  constexpr int OB = 2;                                            // elements per thread per round: 2 x R exchanges in flight
  for (int o0 = tid; o0 < nel; o0 += NT * OB) {
    float v[OB][WG_PW_REPLICAS];
#pragma unroll
    for (int e = 0; e < OB; ++e)
#pragma unroll
      for (int r = 0; r < WG_PW_REPLICAS; ++r) {
        const int o = o0 + e * NT;
        v[e][r] = 0.f;
        if (o < nel && r < p.R) v[e][r] = __hip_atomic_exchange(p.rep + (size_t)r * nel + o, 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
    for (int e = 0; e < OB; ++e) {
      const int o = o0 + e * NT;
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < WG_PW_REPLICAS; ++r) sum += v[e][r];
      if (o < nel) p.dw[o] += sum;
    }
  }
}
template <int NCO, int NCI> __global__ __launch_bounds__(1024) void wgrad_pw(const WgpK p) { wgrad_pw_body<NCO, NCI>(p); }
// members of unequal size in one grid (blockIdx.y = member): the narrow 1x1 weight gradients of a composite - the sources of a concatenating conv, the
// branch convs of a PSPPooling - are 2 - 15 us of mostly launch ramp and drain apiece when launched one by one
template <int NCO, int NCI> __global__ __launch_bounds__(1024) void wgrad_pw_g(const WgpKG g) {
  const WgpK& p = g.k[blockIdx.y];
  if ((int)blockIdx.x >= p.nblk) return;
  wgrad_pw_body<NCO, NCI>(p);
}

static int64_t wg_taps_bytes(const rua_wgrad_desc* d) { return (int64_t)rua_cu_count() * 9 * 32 * (int64_t)d->C * 4; }   // one block partial of [9][32][C] fp32 per CU

static bool pick_wgrad_pw(const rua_wgrad_desc* d) {
  const int on = g_tune.wgrad_pw;
  auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
  const long long M = (long long)d->N * d->H * d->W;
  const bool dense = d->stride == 1 && d->Hs == d->H && d->Ws == d->W;
  return on && d->dtype == RUA_BF16 && d->taps == 1 && d->C <= 64 && d->Cout <= 64 && d->C % 8 == 0 && d->Cout % 8 == 0 &&
         (dense || (pow2(d->H) && pow2(d->W))) && M >= 2048 && d->workspace &&
         d->workspace_bytes >= WG_PW_TAIL && M * d->Cout * 2 < (1ll << 31) &&
         (long long)d->N * d->Hs * d->Ws * d->C * 2 < (1ll << 31) &&
         (long long)(d->H - 1) * d->stride < d->Hs && (long long)(d->W - 1) * d->stride < d->Ws;
}

static int launch_wgrad_pw(const rua_wgrad_desc* d, hipStream_t st) {
  WgpK k;
  k.a = (const unsigned char*)d->a; k.dy = (const unsigned char*)d->dy; k.dw = d->dw;
  char* tail = (char*)d->workspace + d->workspace_bytes - WG_PW_TAIL;
  k.rep = (float*)tail; k.cnt = (int*)(tail + WG_PW_TAIL - 8192);
  k.C = d->C; k.Cout = d->Cout; k.Hs = d->Hs; k.Ws = d->Ws; k.H = d->H; k.W = d->W; k.stride = d->stride;
  k.dense = (d->stride == 1 && d->Hs == d->H && d->Ws == d->W) ? 1 : 0;
  int ws = 0, hs = 0; while ((1 << ws) < d->W) ++ws; while ((1 << hs) < d->H) ++hs;
  k.wshift = ws; k.hshift = hs;
  k.M = (int)((long long)d->N * d->H * d->W);
  k.abytes = (unsigned)((size_t)d->N * d->Hs * d->Ws * d->C * 2); k.dybytes = (unsigned)((size_t)k.M * d->Cout * 2);
  const int nco = d->Cout > 32 ? 2 : 1, nci = d->C > 32 ? 2 : 1;
  const int pxw = (nco + nci <= 2) ? 32 : 16;
  const int target = g_tune.wgpw_blocks > 0 ? g_tune.wgpw_blocks : rua_cu_count();    // blocks of 16 waves, one per CU
  long long waves = (long long)target * 16;
  if (waves > k.M / 128) waves = k.M / 128;                // >= 128 pixels per wave
  if (waves < 16) waves = 16;
  long long ppw = (k.M + waves - 1) / waves;
  ppw = (ppw + 2 * pxw - 1) / (2 * pxw) * (2 * pxw);       // whole double iterations
  k.px_per_wave = (int)ppw;
  {   // replicas: atomic chains of ~64 blocks per address; fewer replicas = fewer exchanges for the finishing block
    const long long nblk = (k.M + ppw * 16 - 1) / (ppw * 16);
    k.R = (int)(nblk / 32); if (k.R < 1) k.R = 1; if (k.R > WG_PW_REPLICAS) k.R = WG_PW_REPLICAS;
    if (g_tune.wgpw_r > 0) k.R = g_tune.wgpw_r > WG_PW_REPLICAS ? WG_PW_REPLICAS : g_tune.wgpw_r;
  }
  const unsigned grid = (unsigned)((k.M + ppw * 16 - 1) / (ppw * 16));
  k.nblk = (int)grid;
  // block partials in front of the tail (tuning key wgrad_pw, bit 1) where the workspace holds one per block; else replicas + tickets (nothing pending)
  const long long nel = (long long)d->Cout * d->C;
  // (a call that reduces right away keeps the replicas unless bit 2 is set: one block walking 256 partials of a 2 KB dW - the stem's - takes 10 us longer than the tickets)
  const bool slab = (g_tune.wgrad_pw & 2) && (d->defer || (g_tune.wgrad_pw & 4)) && (long long)grid * nel * 4 <= (long long)d->workspace_bytes - WG_PW_TAIL;
  k.slabs = slab ? (float*)d->workspace : nullptr;
  if (slab) note_pending(2, (int)grid, nel, k.slabs, d->dw, 0, (int)((nel / 4 + SLAB_RED_COLS - 1) / SLAB_RED_COLS));
  if (g_wgrad_dry) return RUA_OK;
  if (g_wg_pw && g_wg_pw->n < RUA_MAX_BRANCH) {            // a member of a group: recorded, issued by rua_conv_wgrad_group
    WgPwCapture& c = *g_wg_pw; const int i = c.n++;
    c.k[i] = k; c.form[i] = (nco - 1) * 2 + (nci - 1); c.post[i] = (slab && !d->defer) ? 1 : 0;
    return RUA_OK;
  }
  constexpr int s11 = wgrad_pw_smem<1, 1>(), s21 = wgrad_pw_smem<2, 1>(), s12 = wgrad_pw_smem<1, 2>(), s22 = wgrad_pw_smem<2, 2>();
  static RuaPerDevFlag attr_;
  bool& attr = attr_.get();
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_pw<2, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, s21);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_pw<1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, s12);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_pw<2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, s22);
    attr = true;
  }
  if (nco == 1 && nci == 1) hipLaunchKernelGGL((wgrad_pw<1, 1>), dim3(grid), dim3(1024), s11, st, k);
  else if (nco == 2 && nci == 1) hipLaunchKernelGGL((wgrad_pw<2, 1>), dim3(grid), dim3(1024), s21, st, k);
  else if (nco == 1 && nci == 2) hipLaunchKernelGGL((wgrad_pw<1, 2>), dim3(grid), dim3(1024), s12, st, k);
  else hipLaunchKernelGGL((wgrad_pw<2, 2>), dim3(grid), dim3(1024), s22, st, k);
  RUA_LAUNCH_CHECK("wgrad_pw");
  if (slab && !d->defer) { record_mid_event(st); return launch_slab_reduce(k.slabs, d->dw, nel, (int)grid, st); }
  return RUA_OK;
}

extern "C" int64_t rua_wgrad_workspace_bytes(const rua_wgrad_desc* d) {
  if (!d) return 0;
  // all-taps block partials, or 64 K-slice slabs of dW (capped at 64 MiB: the launchers split K no further than the slabs that
  // fit), + wgrad_pw's replicas and ticket (the tail)
  int64_t slabs = (int64_t)64 * d->taps * d->Cout * d->C * 4;
  if (slabs > (64ll << 20)) slabs = 64ll << 20;
  const int64_t taps = wg_taps_bytes(d);
  return (taps > slabs ? taps : slabs) + WG_PW_TAIL;
}

static int slab_capacity(const rua_wgrad_desc* d, long long ndw) {
  if (!d->workspace || d->workspace_bytes <= WG_PW_TAIL) return 1;
  const long long n = (d->workspace_bytes - WG_PW_TAIL) / (ndw * 4);
  return n > 64 ? 64 : (int)n;
}

// which kernel a descriptor launches: 1 = all-taps (top levels), 0 = generic tiled
static int launch_wgrad_dmap(const rua_wgrad_desc* d, hipStream_t st) {
  WgdK k;
  k.a = (const unsigned char*)d->a; k.dy = (const unsigned char*)d->dy; k.dw = d->dw;
  k.C = d->C; k.Cout = d->Cout; k.H = d->H; k.W = d->W; k.dil = d->dil; k.taps = d->taps;
  k.M = (long long)d->N * d->H * d->W;
  int wsh = 0; while ((1 << wsh) < d->W) ++wsh;
  k.wsh = wsh;
  k.ntc = d->Cout / 128; k.nti = d->C / 128;
  const long long tiles = (long long)k.ntc * k.nti * d->taps;
  const int stages = (int)((k.M + 63) / 64);
  const int target = g_tune.wgd_blocks > 0 ? g_tune.wgd_blocks : rua_cu_count();
  long long want = target / tiles; if (want < 1) want = 1;
  if (want > stages / 4) want = stages / 4;             // >= 4 stages per K slice
  if (want < 1) want = 1;
  const long long ndw = (long long)d->taps * d->Cout * d->C;
  const int cap = g_tune.wgrad_slabs ? slab_capacity(d, ndw) : 0;
  if (cap >= 2 && want > cap) want = cap;               // deterministic K split: one fp32 slab per slice must fit the workspace
  k.stages_per_split = (int)((stages + want - 1) / want);
  k.ksplit = (stages + k.stages_per_split - 1) / k.stages_per_split;
  k.slabs = (cap >= 2 && k.ksplit > 1) ? (float*)d->workspace : nullptr;
  k.abytes = (unsigned)((size_t)k.M * d->C * 2); k.dybytes = (unsigned)((size_t)k.M * d->Cout * 2);
  k.ks_slow = g_tune.wgd_ks_slow;
  if (k.slabs) note_pending(2, k.ksplit, ndw, k.slabs, d->dw, 0, (int)((ndw / 4 + SLAB_RED_COLS - 1) / SLAB_RED_COLS));
  if (g_wgrad_dry) return RUA_OK;
  if (g_wg_group && (g_tune.wgrad_group & 8) && g_wg_group->n < RUA_MAX_WGRAD_GROUP) {
    WgGroupCapture& c = *g_wg_group; const int i = c.n++;
    c.kind[i] = 3; c.gx[i] = (unsigned)(tiles * k.ksplit); c.smem[i] = 96 * 1024; c.d[i] = k;
    c.post[i] = (k.slabs && !d->defer) ? 2 : 0; c.part[i] = k.slabs; c.dw[i] = d->dw; c.ndw[i] = ndw; c.parts[i] = k.ksplit; c.CC[i] = 0; c.rblocks[i] = 0;
    return RUA_OK;
  }
  static RuaPerDevFlag attr_;
  bool& attr = attr_.get();
  if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_dmap), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); attr = true; }
  hipLaunchKernelGGL(wgrad_dmap, dim3((unsigned)(tiles * k.ksplit)), dim3(256), 96 * 1024, st, k);
  RUA_LAUNCH_CHECK("wgrad_dmap");
  if (k.slabs && !d->defer) { record_mid_event(st); return launch_slab_reduce(k.slabs, d->dw, ndw, k.ksplit, st); }
  return RUA_OK;
}

// wgrad_rowsx<1>: C = Cout = 256 on 32-pixel rows, an even number of images (the level-4 ResBlock), dilation <= 16 (the zeros between the two rows of a slot)
static bool wgrad_rows256_ok(const rua_wgrad_desc* d) {
  return (g_tune.wgrad_rows & 32) && d->dtype == RUA_BF16 && d->taps == 9 && d->stride == 1 && d->C == 256 && d->Cout == 256 && d->W == 32 && d->N % 2 == 0 && d->N >= 2 &&
         d->Hs == d->H && d->Ws == d->W && d->dil >= 1 && d->dil <= 16 && !d->in_scale && d->workspace && d->workspace_bytes >= wg_taps_bytes(d) &&
         (long long)d->N * d->H * d->W * d->C * 2 < (1ll << 31);
}
extern "C" int rua_wgrad_kind(const rua_wgrad_desc* d) {
  if (!d) return RUA_ERR_ARG;
  if (pick_wgrad_pw(d)) return 3;
  {
    const int on = g_tune.wgrad_dmap;
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    if (on && !wgrad_rows256_ok(d) && d->dtype == RUA_BF16 && (d->taps == 9 || d->taps == 1) && d->stride == 1 && d->C % 128 == 0 && d->Cout % 128 == 0 &&
        d->Hs == d->H && d->Ws == d->W && pow2(d->H) && pow2(d->W) && d->dil >= 1 &&
        ((long long)d->N * d->H * d->W + 64 * 64) * (d->C > d->Cout ? d->C : d->Cout) * 2 < (1ll << 31)) {
      // measured per level of the reference network (us, wgrad_dmap vs wgrad_kernel): 64x64x128 33.1 / 32.5 (9 tiles: the
      // 28 K slices pay 16 MB of float atomics), 32x32x256 25.9 / 35.1, 16x16x512 41.9 / 33.3 (144 tiles: no K split, half
      // the CUs idle), 8x8x1024 75 / 32 (576 short-K blocks at one per CU).  So: a few dozen tiles and a long K.
      const long long tiles = (long long)d->taps * (d->Cout / 128) * (d->C / 128);
      const long long stages = ((long long)d->N * d->H * d->W + 63) / 64;
      const int mint = g_tune.wgd_mintiles;    // 9: the 64x64x128 level too (A/B in the step: -0.03 ms)
      if (on == 2 || (tiles >= mint && tiles <= 64 && stages >= 64)) return 2;
    }
  }
  const bool rows128 = (g_tune.wgrad_rows & 4) && d->C == 128 && d->W == 64 && !d->in_scale;      // wgrad_rows128 (the level-3 ResBlock)
  if (wgrad_rows256_ok(d)) return 1;
  const bool ok = d->dtype == RUA_BF16 && d->taps == 9 && d->stride == 1 && d->C == d->Cout && (d->C == 32 || d->C == 64 || rows128) &&
                  d->W % 64 == 0 && d->Hs == d->H && d->Ws == d->W && d->dil >= 1 && d->dil <= 31 && d->workspace &&
                  d->workspace_bytes >= wg_taps_bytes(d) && (long long)d->N * d->H * d->W * d->C * 2 < (1ll << 31);
  return ok ? 1 : 0;
}

// the whole-image kernels of the deepest levels (kind 0 of rua_wgrad_kind): 0 none (generic tiles), 1 wgrad_img (64 x 64 tiles, 512-pixel chunks as K slices through slabs),
// 2 wgrad_imgs (more than 512 pixels: 32 x 32 tiles, chunks streamed - when those tiles fill at least half the chip)
static int wgrad_img_pick(const rua_wgrad_desc* d) {
  const long long M = (long long)d->N * d->H * d->W;
  if (!((g_tune.wgrad_rows & 8) && d->dtype == RUA_BF16 && d->taps == 9 && d->stride == 1 && d->dil == 1 && d->Hs == d->H && d->Ws == d->W && d->H == d->W &&
        (d->W == 8 || d->W == 16) && d->C % 32 == 0 && d->Cout % 32 == 0 && M % 512 == 0 && !d->in_scale)) return 0;
  if ((g_tune.wgrad_rows & 16) && M >= 1024 && (long long)(d->C / 32) * (d->Cout / 32) >= rua_cu_count() / 2) return 2;
  if (d->C % 64 || d->Cout % 64) return 0;
  if (M == 512 || (g_tune.wgrad_slabs && slab_capacity(d, (long long)9 * d->Cout * d->C) >= (int)(M / 512))) return 1;
  return 0;
}
extern "C" int rua_wgrad_img_kind(const rua_wgrad_desc* d) { return (d && rua_wgrad_kind(d) == 0) ? wgrad_img_pick(d) : 0; }

// a member of a batched launch (wgrad_batch_launch / rua_wgrad_group_plan): rua_conv_wgrad takes the K split from here and hands its kernel arguments back
struct WgBatchMember { long long want; WgK k; unsigned grid; long long ndw; };
static thread_local WgBatchMember* g_wg_batch = nullptr;

extern "C" int rua_conv_wgrad(const rua_wgrad_desc* d, void* stream) {
  RUA_CHECK_ARG(d && d->a && d->dy && d->dw, "rua_conv_wgrad: null pointer");
  RUA_CHECK_ARG(d->dtype == RUA_F32 || d->dtype == RUA_BF16, "rua_conv_wgrad: bad dtype");
  const int vec = d->dtype == RUA_BF16 ? 8 : 4;
  RUA_CHECK_ARG(d->C % vec == 0 && d->Cout % vec == 0, "rua_conv_wgrad: C=%d Cout=%d must be multiples of %d", d->C, d->Cout, vec);
  RUA_CHECK_ARG(d->taps == 1 || d->taps == 9, "rua_conv_wgrad: taps must be 1 or 9");
  if (rua_wgrad_kind(d) == 1) return launch_wgrad_taps(d, (hipStream_t)stream);
  RUA_CHECK_ARG(d->in_scale == nullptr, "rua_conv_wgrad: in_scale / in_shift (normalise on load) needs the all-taps kernel (rua_wgrad_kind() == 1)");
  if (rua_wgrad_kind(d) == 2) return launch_wgrad_dmap(d, (hipStream_t)stream);
  if (rua_wgrad_kind(d) == 3) return launch_wgrad_pw(d, (hipStream_t)stream);
  RUA_CHECK_ARG((long long)(d->H - 1) * d->stride < d->Hs && (long long)(d->W - 1) * d->stride < d->Ws,
                "rua_conv_wgrad: input %dx%d too small for gradient %dx%d stride %d", d->Hs, d->Ws, d->H, d->W, d->stride);
  WgK k;
  k.a = (const unsigned char*)d->a; k.dy = (const unsigned char*)d->dy; k.dw = d->dw; k.overwrite = d->overwrite_dev;
  k.C = d->C; k.Hs = d->Hs; k.Ws = d->Ws; k.Cout = d->Cout; k.H = d->H; k.W = d->W; k.N = d->N;
  k.stride = d->stride; k.dil = d->dil; k.taps = d->taps;
  k.M = (long long)d->N * d->H * d->W;
  RUA_CHECK_ARG(k.M * d->Cout * 4 < (1ll << 31) && (long long)d->N * d->Hs * d->Ws * d->C * 4 < (1ll << 31),
                "rua_conv_wgrad: tensors must stay below 2 GiB (32-bit offsets)");
  auto lg2 = [](int v) { int s = 0; while ((1 << s) < v) ++s; return (1 << s) == v ? s : -1; };
  k.wshift = lg2(d->W); k.hshift = lg2(d->H);
  if (k.wshift < 0 || k.hshift < 0) k.wshift = k.hshift = -1;
  k.ntc = (d->Cout + 63) / 64; k.nti = (d->C + 63) / 64;
  const int img_kind = wgrad_img_pick(d);
  if (img_kind) {
    // wgrad_img: whole images resident in LDS, a 64 x 64 tile of dW for all nine taps per block, 512-pixel chunks as K slices
    hipStream_t st_ = (hipStream_t)stream;
    const long long ndw_ = (long long)9 * d->Cout * d->C;
    if (img_kind == 2) {
      // wgrad_imgs: 32 x 32 tiles, the chunks streamed through a two-stage ring - no K slices, no slabs
      if (g_wgrad_dry) return RUA_OK;
      k.ksplit = (int)(k.M / 512); k.pix_per_block = 512; k.slabs = nullptr;
      k.nti = d->C / 32; k.ntc = d->Cout / 32;
      constexpr int smems_ = 4 * 9 * 16 * 64 * 4;             // the ring (2 x 67 840 B) and, after it, the four k-quarters' accumulators (147 456 B)
      static RuaPerDevFlag attrs_;
      bool& attrs = attrs_.get();
      if (!attrs) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_imgs<8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_imgs<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attrs = true;
      }
      if (d->W == 8) hipLaunchKernelGGL(wgrad_imgs<8>, dim3((unsigned)(k.nti * k.ntc)), dim3(768), smems_, st_, k);
      else hipLaunchKernelGGL(wgrad_imgs<16>, dim3((unsigned)(k.nti * k.ntc)), dim3(768), smems_, st_, k);
      RUA_LAUNCH_CHECK("wgrad_imgs");
      return RUA_OK;
    }
    k.ksplit = (int)(k.M / 512);
    k.pix_per_block = 512;
    k.slabs = k.ksplit > 1 ? (float*)d->workspace : nullptr;
    if (k.slabs) note_pending(2, k.ksplit, ndw_, k.slabs, d->dw, 0, (int)((ndw_ / 4 + SLAB_RED_COLS - 1) / SLAB_RED_COLS));
    if (g_wgrad_dry) return RUA_OK;
    const unsigned grid_ = (unsigned)(k.ntc * k.nti * k.ksplit);
    constexpr int smem_ = 2 * 512 * 128 + 2 * 18 * 128;
    static RuaPerDevFlag attr_;
    bool& attr = attr_.get();
    if (!attr) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_img<8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_img<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      attr = true;
    }
    if (d->W == 8) hipLaunchKernelGGL(wgrad_img<8>, dim3(grid_), dim3(768), smem_, st_, k);
    else hipLaunchKernelGGL(wgrad_img<16>, dim3(grid_), dim3(768), smem_, st_, k);
    RUA_LAUNCH_CHECK("wgrad_img");
    if (k.slabs && !d->defer) { record_mid_event(st_); return launch_slab_reduce(k.slabs, d->dw, ndw_, k.ksplit, st_); }
    return RUA_OK;
  }
  const long long tiles = (long long)k.ntc * k.nti * d->taps;
  // K split: every slice adds the whole dW tile with fp32 atomics (~1.3 TB/s chip-wide), so slices x |dW| must stay
  // small: ~512 blocks fill the chip; 2048 blocks meant 33 MB of atomics (~25 us) per launch.
  // (the members of a grouped launch share the ~512 blocks: a third / quarter of the K slices and of their slabs each)
  const int wshare = (g_tune.wgrad_kernel_share && (g_tune.wgrad_group & 1) && d->group_members > 1 && d->dtype == RUA_BF16) ? d->group_members : 1;
  const int target = (g_tune.wgrad_blocks > 0 ? g_tune.wgrad_blocks : 2 * rua_cu_count()) / wshare;      // 512 on MI355X
  long long want = target / tiles; if (want < 1) want = 1;
  long long stages = (k.M + 63) / 64;
  if (g_wg_batch && g_wg_batch->want > 0) want = g_wg_batch->want;      // a member of a batched launch: its share of the batch's blocks (wgrad_batch_split)
  if (want > stages) want = stages;
  const long long ndw = (long long)d->taps * d->Cout * d->C;
  const int cap = (g_tune.wgrad_slabs && ndw % 4 == 0) ? slab_capacity(d, ndw) : 0;
  if (cap >= 2 && want > cap) want = cap;              // deterministic K split: one fp32 slab per slice must fit the workspace
  long long spb = (stages + want - 1) / want;          // stages per block
  k.pix_per_block = (int)(spb * 64);
  k.ksplit = (int)((k.M + k.pix_per_block - 1) / k.pix_per_block);
  k.slabs = (cap >= 2 && k.ksplit > 1) ? (float*)d->workspace : nullptr;
  const long long grid = tiles * k.ksplit;
  RUA_CHECK_ARG(grid < (1ll << 31), "rua_conv_wgrad: grid too large");
  hipStream_t st = (hipStream_t)stream;
  if (k.slabs) note_pending(2, k.ksplit, ndw, k.slabs, d->dw, 0, (int)((ndw / 4 + SLAB_RED_COLS - 1) / SLAB_RED_COLS));
  if (g_wgrad_dry) return RUA_OK;
  if (g_wg_batch) { g_wg_batch->k = k; g_wg_batch->grid = (unsigned)grid; g_wg_batch->ndw = ndw; return RUA_OK; }      // issued by wgrad_batch_launch
  if (g_wg_group && (g_tune.wgrad_group & 1) && g_wg_group->n < RUA_MAX_WGRAD_GROUP && d->dtype == RUA_BF16) {
    WgGroupCapture& c = *g_wg_group; const int i = c.n++;
    c.kind[i] = 0; c.gx[i] = (unsigned)grid; c.smem[i] = 0; c.g[i] = k;
    c.post[i] = (k.slabs && !d->defer) ? 2 : 0; c.part[i] = k.slabs; c.dw[i] = d->dw; c.ndw[i] = ndw; c.parts[i] = k.ksplit; c.CC[i] = 0; c.rblocks[i] = 0;
    return RUA_OK;
  }
  if (d->dtype == RUA_BF16) hipLaunchKernelGGL((wgrad_kernel<bf16_t>), dim3((unsigned)grid), dim3(256), 0, st, k);
  else hipLaunchKernelGGL((wgrad_kernel<float>), dim3((unsigned)grid), dim3(256), 0, st, k);
  RUA_LAUNCH_CHECK("wgrad_kernel");
  if (k.slabs && !d->defer) { record_mid_event(st); return launch_slab_reduce(k.slabs, d->dw, ndw, k.ksplit, st); }
  return RUA_OK;
}

// rua_conv_wgrad_group: n INDEPENDENT weight gradients (the dilation branches of a ResBlock) with the results of n rua_conv_wgrad
// calls.  Members that land on the same kernel go out as ONE grid (blockIdx.y / .z = member; the grid is the largest member's,
// the others' surplus blocks leave at once), the rest one by one.  Members that share partial-sum workspace cannot overlap:
// such a group runs member by member.
static thread_local int g_wg_group_last_grids = 0;
extern "C" int rua_wgrad_group_last_grids(void) { return g_wg_group_last_grids; }

// The batched form: every member lands on the generic bf16 tile kernel (rua_wgrad_kind() == 0, no whole-image kernel) and asks for it
// (rua_wgrad_desc.batch).  Any number of members; RUA_MAX_WGRAD_BATCH per grid (the kernel arguments), so ceil(n / RUA_MAX_WGRAD_BATCH) grids.
constexpr int WG_BATCH_MAX_MEMBERS = 4 * RUA_MAX_WGRAD_BATCH;
static bool wgrad_batch_ok(const rua_wgrad_desc* d, int n) {
  if (!(g_tune.wgrad_group & 1) || n > WG_BATCH_MAX_MEMBERS) return false;
  for (int i = 0; i < n; ++i) {
    if (!d[i].a || !d[i].dy || !d[i].dw || d[i].dtype != RUA_BF16 || !d[i].batch || d[i].in_scale) return false;
    if (d[i].C <= 0 || d[i].Cout <= 0 || d[i].C % 8 || d[i].Cout % 8 || (d[i].taps != 1 && d[i].taps != 9)) return false;
    if (rua_wgrad_kind(d + i) != 0 || wgrad_img_pick(d + i) != 0) return false;
  }
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) if (d[i].dw == d[j].dw) return false;
  return true;
}
// One block budget for the members [0, n) of ONE grid, dealt by work (a pure function of the descriptors): a member's work is stages x tiles (64-pixel stages of
// its K range, 64 x 64 tiles of its dW), and it gets that share of the budget as blocks - so every block of the grid runs about work / budget stages, whichever
// member it belongs to.  want[i] = K slices asked for (rua_conv_wgrad bounds it by the member's stages and slab capacity); 0: the split it would take alone
// (bit 5 of wgrad_group: the batch is then bit-identical to the single launches).
static void wgrad_batch_split(const rua_wgrad_desc* d, int n, long long* want) {
  long long work = 0;
  for (int i = 0; i < n; ++i)
    work += (((long long)d[i].N * d[i].H * d[i].W + 63) / 64) * ((d[i].Cout + 63) / 64) * ((d[i].C + 63) / 64) * d[i].taps;
  const long long budget = g_tune.wgrad_batch_blocks > 0 ? g_tune.wgrad_batch_blocks : 4ll * rua_cu_count();
  for (int i = 0; i < n; ++i) {
    const long long stages = ((long long)d[i].N * d[i].H * d[i].W + 63) / 64;
    long long w = work > 0 ? (budget * stages + work / 2) / work : 1;           // blocks of the member / its tiles
    want[i] = (g_tune.wgrad_group & 32) ? 0 : (w < 1 ? 1 : w);
  }
}
// geometry of the members of one grid: kernel arguments, grid and (through g_wgrad_pending, one record per member) the partials each leaves
static int wgrad_batch_members(const rua_wgrad_desc* d, int n, WgBatchMember* mem, rua_wgrad_pending* recs, bool dry) {
  long long want[RUA_MAX_WGRAD_BATCH];
  wgrad_batch_split(d, n, want);
  int rc = RUA_OK;
  for (int i = 0; i < n && rc == RUA_OK; ++i) {
    mem[i].want = want[i]; mem[i].grid = 0;
    if (recs) { memset(recs + i, 0, sizeof(*recs)); g_wgrad_pending = recs + i; }
    g_wg_batch = mem + i; g_wgrad_dry = dry;
    rc = rua_conv_wgrad(d + i, nullptr);
    g_wg_batch = nullptr; g_wgrad_dry = false; g_wgrad_pending = nullptr;
    if (recs) recs[i].overwrite_dev = d[i].overwrite_dev;
  }
  return rc;
}
static int wgrad_batch_launch(const rua_wgrad_desc* d, int n, hipStream_t st) {
  int grids = 0;
  for (int base = 0; base < n; base += RUA_MAX_WGRAD_BATCH) {
    const int m = n - base < RUA_MAX_WGRAD_BATCH ? n - base : RUA_MAX_WGRAD_BATCH;
    WgBatchMember mem[RUA_MAX_WGRAD_BATCH];
    const int rc = wgrad_batch_members(d + base, m, mem, nullptr, false);
    if (rc != RUA_OK) return rc;
    int order[RUA_MAX_WGRAD_BATCH];
    for (int i = 0; i < m; ++i) order[i] = i;
    for (int i = 1; i < m; ++i) {                          // longest blocks first (stable: equal members keep the caller's order)
      const int o = order[i]; int j = i;
      while (j > 0 && mem[order[j - 1]].k.pix_per_block < mem[o].k.pix_per_block) { order[j] = order[j - 1]; --j; }
      order[j] = o;
    }
    WgKB g;
    unsigned long long total = 0;
    for (int i = 0; i < m; ++i) { g.k[i] = mem[order[i]].k; total += mem[order[i]].grid; g.end[i] = (unsigned)total; }
    for (int i = m; i < RUA_MAX_WGRAD_BATCH; ++i) { g.k[i] = g.k[0]; g.end[i] = (unsigned)total; }
    g.n = m;
    RUA_CHECK_ARG(total >= 1 && total < (1ull << 31), "rua_conv_wgrad_group: grid too large");
    hipLaunchKernelGGL(wgrad_kernel_b, dim3((unsigned)total), dim3(256), 0, st, g);
    RUA_LAUNCH_CHECK("wgrad_kernel_b");
    ++grids;
    for (int i = 0; i < m; ++i)                            // members that did not defer their reduction
      if (mem[i].k.slabs && !d[base + i].defer) { const int rr = launch_slab_reduce(mem[i].k.slabs, mem[i].k.dw, mem[i].ndw, mem[i].k.ksplit, st); if (rr != RUA_OK) return rr; }
  }
  g_wg_group_last_grids = grids;
  return RUA_OK;
}
extern "C" int rua_wgrad_group_plan(const rua_wgrad_desc* d, int n, rua_wgrad_pending* out) {
  RUA_CHECK_ARG(d && out && n >= 1, "rua_wgrad_group_plan: bad arguments");
  if (!wgrad_batch_ok(d, n)) {
    for (int i = 0; i < n; ++i) { const int rc = rua_wgrad_plan(d + i, out + i); if (rc != RUA_OK) return rc; }
    return RUA_OK;
  }
  for (int base = 0; base < n; base += RUA_MAX_WGRAD_BATCH) {
    const int m = n - base < RUA_MAX_WGRAD_BATCH ? n - base : RUA_MAX_WGRAD_BATCH;
    WgBatchMember mem[RUA_MAX_WGRAD_BATCH];
    const int rc = wgrad_batch_members(d + base, m, mem, out + base, true);
    if (rc != RUA_OK) return rc;
  }
  return RUA_OK;
}
extern "C" int rua_conv_wgrad_group(const rua_wgrad_desc* d, int n, void* stream) {
  RUA_CHECK_ARG(d && n >= 1, "rua_conv_wgrad_group: no members");
  hipStream_t st = (hipStream_t)stream;
  if (wgrad_batch_ok(d, n)) {
    // members whose slabs overlap (a shared workspace) cannot run at once: member by member, as any group that shares workspace
    static thread_local rua_wgrad_pending recs[WG_BATCH_MAX_MEMBERS];
    const int rp = rua_wgrad_group_plan(d, n, recs);
    if (rp != RUA_OK) return rp;
    bool overlap = false;
    for (int i = 0; i < n && !overlap; ++i)
      for (int j = i + 1; j < n && !overlap; ++j) {
        if (recs[i].kind != 2 || recs[j].kind != 2) continue;
        const float* a0 = recs[i].partials; const float* b0 = recs[j].partials;
        overlap = a0 < b0 + (long long)recs[j].parts * recs[j].n && b0 < a0 + (long long)recs[i].parts * recs[i].n;
      }
    if (!overlap) return wgrad_batch_launch(d, n, st);
    g_wg_group_last_grids = n;
    for (int i = 0; i < n; ++i) { const int rc = rua_conv_wgrad(d + i, stream); if (rc != RUA_OK) return rc; }
    return RUA_OK;
  }
  RUA_CHECK_ARG(n <= RUA_MAX_WGRAD_GROUP, "rua_conv_wgrad_group: 1..%d members (more only in the batched form)", RUA_MAX_WGRAD_GROUP);
  bool shared = false;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const char* a0 = (const char*)d[i].workspace; const char* b0 = (const char*)d[j].workspace;
      if (a0 && b0 && a0 < b0 + d[j].workspace_bytes && b0 < a0 + d[i].workspace_bytes) shared = true;
      if (d[i].dw == d[j].dw) shared = true;
    }
  g_wg_group_last_grids = n;
  {
    // all members narrow 1x1 weight gradients (wgrad_pw) with replicas / tickets of their own: one grid per (NCO, NCI) form
    bool allpw = n >= 2 && (g_tune.wgrad_group & 16);
    for (int i = 0; i < n && allpw; ++i) allpw = rua_wgrad_kind(d + i) == 3;
    for (int i = 0; i < n && allpw; ++i)
      for (int j = i + 1; j < n; ++j) {
        const char* ti = (const char*)d[i].workspace + d[i].workspace_bytes - WG_PW_TAIL; const char* tj = (const char*)d[j].workspace + d[j].workspace_bytes - WG_PW_TAIL;
        if (ti < tj + WG_PW_TAIL && tj < ti + WG_PW_TAIL) allpw = false;        // shared replicas: one by one
        if (d[i].dw == d[j].dw) allpw = false;
      }
    if (allpw) {
      WgPwCapture cap;
      cap.n = 0;
      g_wg_pw = &cap;
      int rc = RUA_OK;
      for (int i = 0; i < n && rc == RUA_OK; ++i) rc = rua_conv_wgrad(d + i, stream);
      g_wg_pw = nullptr;
      if (rc != RUA_OK) return rc;
      int grids = n - cap.n;
      constexpr int s11 = wgrad_pw_smem<1, 1>(), s21 = wgrad_pw_smem<2, 1>(), s12 = wgrad_pw_smem<1, 2>(), s22 = wgrad_pw_smem<2, 2>();
      static RuaPerDevFlag attr_;
      if (!attr_.get()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_pw_g<2, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, s21);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_pw_g<1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, s12);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_pw_g<2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, s22);
        attr_.get() = true;
      }
      for (int form = 0; form < 4; ++form) {
        WgpKG g; int m = 0; unsigned gx = 0;
        for (int i = 0; i < cap.n; ++i) if (cap.form[i] == form) { g.k[m++] = cap.k[i]; if ((unsigned)cap.k[i].nblk > gx) gx = (unsigned)cap.k[i].nblk; }
        if (m == 0) continue;
        for (int i = m; i < RUA_MAX_BRANCH; ++i) g.k[i] = g.k[0];
        if (form == 0) hipLaunchKernelGGL((wgrad_pw_g<1, 1>), dim3(gx, m), dim3(1024), s11, st, g);
        else if (form == 1) hipLaunchKernelGGL((wgrad_pw_g<1, 2>), dim3(gx, m), dim3(1024), s12, st, g);
        else if (form == 2) hipLaunchKernelGGL((wgrad_pw_g<2, 1>), dim3(gx, m), dim3(1024), s21, st, g);
        else hipLaunchKernelGGL((wgrad_pw_g<2, 2>), dim3(gx, m), dim3(1024), s22, st, g);
        RUA_LAUNCH_CHECK("wgrad_pw (group)");
        ++grids;
      }
      g_wg_group_last_grids = grids;
      for (int i = 0; i < cap.n; ++i)
        if (cap.post[i]) { rc = launch_slab_reduce(cap.k[i].slabs, cap.k[i].dw, (long long)cap.k[i].Cout * cap.k[i].C, cap.k[i].nblk, st); if (rc != RUA_OK) return rc; }
      return RUA_OK;
    }
  }
  if (n == 1 || shared || !g_tune.wgrad_group) {
    for (int i = 0; i < n; ++i) { const int rc = rua_conv_wgrad(d + i, stream); if (rc != RUA_OK) return rc; }
    return RUA_OK;
  }
  WgGroupCapture cap;
  cap.n = 0;
  g_wg_group = &cap;
  int rc = RUA_OK;
  for (int i = 0; i < n && rc == RUA_OK; ++i) rc = rua_conv_wgrad(d + i, stream);      // members no launcher captures launch right here
  g_wg_group = nullptr;
  if (rc != RUA_OK) return rc;
  int grids = n - cap.n;
  bool done[RUA_MAX_WGRAD_GROUP] = {false};
  for (int i = 0; i < cap.n; ++i) {
    if (done[i]) continue;
    int idx[RUA_MAX_WGRAD_GROUP], m = 0; unsigned gx = 0; int smem = 0;
    for (int j = i; j < cap.n; ++j)
      if (!done[j] && cap.kind[j] == cap.kind[i]) { idx[m++] = j; done[j] = true; if (cap.gx[j] > gx) gx = cap.gx[j]; if (cap.smem[j] > smem) smem = cap.smem[j]; }
    static RuaPerDevFlag attrf[4];
    bool* attr[4] = {&attrf[0].get(), &attrf[1].get(), &attrf[2].get(), &attrf[3].get()};
    const int kd = cap.kind[i];
    if (kd == 0) {
      if (m == 1) hipLaunchKernelGGL((wgrad_kernel<bf16_t>), dim3(gx), dim3(256), 0, st, cap.g[idx[0]]);
      else { WgKG g; for (int q = 0; q < m; ++q) g.k[q] = cap.g[idx[q]]; hipLaunchKernelGGL(wgrad_kernel_g, dim3(gx, m), dim3(256), 0, st, g); }
    } else if (kd == 3) {
      if (!*attr[3]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_dmap), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_dmap_g), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); *attr[3] = true;
      }
      if (m == 1) hipLaunchKernelGGL(wgrad_dmap, dim3(gx), dim3(256), smem, st, cap.d[idx[0]]);
      else { WgdKG g; for (int q = 0; q < m; ++q) g.k[q] = cap.d[idx[q]]; hipLaunchKernelGGL(wgrad_dmap_g, dim3((gx + 7) / 8 * 8, m), dim3(256), smem, st, g); }
    } else if (kd >= 4) {
      WgtKG g; for (int q = 0; q < m; ++q) g.k[q] = cap.t[idx[q]];
      const unsigned gyr = kd == 12 ? 8u : (kd == 10 || kd == 11) ? 2u : 1u;     // wgrad_rows128 / wgrad_rowsx: grid.y = output-channel slice (x input-channel half)
      if (m == 1) launch_rows32(kd, false, dim3(gx, gyr), smem, st, &g.k[0], nullptr);
      else launch_rows32(kd, true, dim3(gx, gyr, m), smem, st, nullptr, &g);
    } else {
      const int gy = kd == 1 ? 1 : 2;
      if (!*attr[kd]) {
        if (kd == 1) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_taps_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                       (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_taps_kernel_g<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
        else { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_taps_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
               (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_taps_kernel_g<64>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
        *attr[kd] = true;
      }
      WgtKG g; for (int q = 0; q < m; ++q) g.k[q] = cap.t[idx[q]];
      if (m == 1) { if (kd == 1) hipLaunchKernelGGL((wgrad_taps_kernel<32>), dim3(gx, gy), dim3(768), smem, st, g.k[0]);
                    else hipLaunchKernelGGL((wgrad_taps_kernel<64>), dim3(gx, gy), dim3(768), smem, st, g.k[0]); }
      else if (kd == 1) hipLaunchKernelGGL((wgrad_taps_kernel_g<32>), dim3(gx, gy, m), dim3(768), smem, st, g);
      else hipLaunchKernelGGL((wgrad_taps_kernel_g<64>), dim3(gx, gy, m), dim3(768), smem, st, g);
    }
    RUA_LAUNCH_CHECK("rua_conv_wgrad_group");
    ++grids;
  }
  g_wg_group_last_grids = grids;
  for (int i = 0; i < cap.n; ++i) {                      // members that did not defer their reduction
    if (cap.post[i] == 1) { hipLaunchKernelGGL(wgrad_taps_reduce, dim3(cap.rblocks[i]), dim3(256), 0, st, cap.part[i], cap.dw[i], cap.CC[i], cap.parts[i]); RUA_LAUNCH_CHECK("wgrad_taps_reduce"); }
    else if (cap.post[i] == 2) { rc = launch_slab_reduce(cap.part[i], cap.dw[i], cap.ndw[i], cap.parts[i], st); if (rc != RUA_OK) return rc; }
  }
  return RUA_OK;
}

extern "C" int rua_wgrad_plan(const rua_wgrad_desc* d, rua_wgrad_pending* out) {
  RUA_CHECK_ARG(d && out, "rua_wgrad_plan: null pointer");
  memset(out, 0, sizeof(*out));
  g_wgrad_pending = out; g_wgrad_dry = true;
  const int rc = rua_conv_wgrad(d, nullptr);
  g_wgrad_pending = nullptr; g_wgrad_dry = false;
  out->overwrite_dev = d->overwrite_dev;
  return rc;
}

// One launch for any number of pending weight-gradient reductions: block -> record by binary search over block_begin, then the
// record's own reduction (same arithmetic and order as wgrad_taps_reduce / wgrad_slab_reduce: bit-reproducible).
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const rua_wgrad_pending* __restrict__ items, int n_items) {
  int lo = 0, hi = n_items - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].block_begin <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
  const rua_wgrad_pending it = items[lo];
  const int vb = (int)blockIdx.x - it.block_begin;
  if (vb >= it.blocks) return;
  const int ow = (it.overwrite_dev && *it.overwrite_dev != 0) ? 1 : 0;
  if (it.kind == 1) wgrad_taps_reduce_body(it.partials, it.dw, it.CC, it.parts, vb, ow);
  else if (it.kind == 2) wgrad_slab_reduce_body(it.partials, it.dw, it.n / 4, it.parts, vb, ow);
  else if (it.kind == 3) {                             // per-channel fp64 sums (replicated statistics) -> += an fp32 vector (bias gradients)
    const int c = vb * 256 + (int)threadIdx.x;
    if (c < (int)it.n) {
      double a, unused;
      replica_sum(reinterpret_cast<const double*>(it.partials), it.parts, (int)it.n, c, a, unused);
      it.dw[c] += (float)a;
    }
  }
}
extern "C" int rua_wgrad_reduce_batch(const rua_wgrad_pending* items_dev, int n_items, int total_blocks, void* stream) {
  RUA_CHECK_ARG(items_dev && n_items >= 1 && total_blocks >= 1, "rua_wgrad_reduce_batch: bad arguments");
  hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, items_dev, n_items);
  RUA_LAUNCH_CHECK("rua_wgrad_reduce_batch");
  return RUA_OK;
}

// =========================================================================================
// Weight preparation: fp32 master [taps][Cout][C] -> dtype copies (forward layout, dgrad layout).
template <typename T>
__global__ __launch_bounds__(256) void wprep_kernel(const float* __restrict__ master, T* __restrict__ wf, T* __restrict__ wd,
                                                    const rua_wprep_item* __restrict__ items) {
  // one 64(co) x 64(ci) tile of one tap per block iteration: 16-byte fp32 reads along ci, 4-element writes of the forward
  // copy (same layout) and, through an LDS transpose, of the data-gradient copy [taps reversed][ci][co].  Every slice of
  // the flat buffers is 64-byte aligned and C, Cout are multiples of 4 wherever the fast path is taken.
  __shared__ float tile[64][65];
  const rua_wprep_item it = items[blockIdx.y];
  const int tco = (it.Cout + 63) / 64, tci = (it.C + 63) / 64;
  const int ntiles = it.taps * tco * tci;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;          // 16 x 16: 4 elements per thread and pass
  const bool vec = (it.C % 4 == 0) && (it.Cout % 4 == 0);
  auto put4 = [](T* dst, const float* v) {
    if constexpr (sizeof(T) == 2) {
      const uint2 q = make_uint2(ET<bf16_t>::pk(v[0], v[1]), ET<bf16_t>::pk(v[2], v[3]));
      *reinterpret_cast<uint2*>(dst) = q;
    } else {
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    }
  };
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int tap = t / (tco * tci), r = t - tap * tco * tci;
    const int co0 = (r / tci) * 64, ci0 = (r % tci) * 64;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int co = co0 + ty + k * 16, ci = ci0 + tx * 4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (co < it.Cout) {
        const size_t o = (size_t)tap * it.Cout * it.C + (size_t)co * it.C + ci;
        if (vec && ci + 3 < it.C) {
          const float4 q = *reinterpret_cast<const float4*>(master + it.src_off + o);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
          put4(wf + it.dst_off + o, v);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (ci + j < it.C) { v[j] = master[it.src_off + o + j]; wf[it.dst_off + o + j] = (T)v[j]; }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[ty + k * 16][tx * 4 + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ci = ci0 + ty + k * 16, co = co0 + tx * 4;
      if (ci < it.C) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = tile[tx * 4 + j][ty + k * 16];
        T* dst = wd + it.dst_off + (size_t)(it.taps - 1 - tap) * it.Cout * it.C + (size_t)ci * it.Cout + co;
        if (vec && co + 3 < it.Cout) put4(dst, v);
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (co + j < it.Cout) dst[j] = (T)v[j];
        }
      }
    }
    __syncthreads();
  }
}

extern "C" int rua_weight_prep(const float* master, void* w_fwd, void* w_dgrad, const rua_wprep_item* items_dev,
                               int n_items, int max_elems, int dtype, void* stream) {
  RUA_CHECK_ARG(master && w_fwd && w_dgrad && items_dev && n_items > 0, "rua_weight_prep: bad arguments");
  int gx = rua_div_up(max_elems, 4096 * 4); if (gx < 1) gx = 1; if (gx > 256) gx = 256;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == RUA_BF16) hipLaunchKernelGGL((wprep_kernel<bf16_t>), dim3(gx, n_items), dim3(256), 0, st, master, (bf16_t*)w_fwd, (bf16_t*)w_dgrad, items_dev);
  else hipLaunchKernelGGL((wprep_kernel<float>), dim3(gx, n_items), dim3(256), 0, st, master, (float*)w_fwd, (float*)w_dgrad, items_dev);
  RUA_LAUNCH_CHECK("wprep_kernel");
  return RUA_OK;
}

constexpr int RUA_WPREP_TPB = 8;                      // 64 x 64 tiles a block of the block map takes (two per wave)
// The data-gradient layout alone, from the forward-layout bf16 copy the optimizer already wrote (rua_adam_step_w / rua_sgd_step_w): wd[taps reversed][ci][co]
// = wf[tap][co][ci].  A block moves 64 (co) x 64 (ci) tiles of one tap through a 2-byte LDS tile: 8-byte reads along ci, 8-byte writes along co - half the
// bytes of rua_weight_prep (no fp32 master read, no forward copy written).
// blockmap (optional): [blocks][2] = (item, first tile) - a block takes RUA_WPREP_TPB tiles of ONE item, the grid is as long as the tensors ask (a (256, items)
// grid launched 26 000 blocks for ~100 convolutions of which a dozen hold 90 % of the bytes: most blocks fetched their item and left - 60 us for 170 MB)
__global__ __launch_bounds__(256) void wprep_dgrad_kernel(const bf16_t* __restrict__ wf, bf16_t* __restrict__ wd, const rua_wprep_item* __restrict__ items,
                                                          const int* __restrict__ blockmap) {
  __shared__ unsigned short tile[64][66];
  const int item = blockmap ? blockmap[2 * blockIdx.x] : (int)blockIdx.y;
  const rua_wprep_item it = items[item];
  const int tco = (it.Cout + 63) / 64, tci = (it.C + 63) / 64;
  const int ntiles = it.taps * tco * tci;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const bool vec = (it.C % 4 == 0) && (it.Cout % 4 == 0);
  const unsigned short* src = reinterpret_cast<const unsigned short*>(wf) + it.dst_off;
  unsigned short* dst = reinterpret_cast<unsigned short*>(wd) + it.dst_off;
  if ((it.C & 7) == 0 && (it.Cout & 7) == 0) {
    // Fast path, no LDS: a wave owns a 64 x 64 tile, lane (cg, pg) its 8 (co) x 8 (ci) block - eight 16-byte loads (lanes pg = 0 .. 7 read 128 contiguous
    // bytes of a row), the block transposed in registers, eight 16-byte stores (lanes cg = 0 .. 7 write 128 contiguous bytes of a [ci] row).  (The LDS
    // tile below moved 4 elements per access through 2-byte cells with a 0.40 bank-conflict share: 2.9 TB/s.)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cg = lane >> 3, pg = lane & 7;
    const int t0 = blockmap ? blockmap[2 * blockIdx.x + 1] : (int)blockIdx.x * 4;
    const int tend = blockmap ? (t0 + RUA_WPREP_TPB < ntiles ? t0 + RUA_WPREP_TPB : ntiles) : ntiles;
    const int tstep = blockmap ? 4 : (int)gridDim.x * 4;
    for (int t = t0 + wv; t < tend; t += tstep) {
      const int tap = t / (tco * tci), r = t - tap * tco * tci;
      const int co = (r / tci) * 64 + cg * 8, ci = (r % tci) * 64 + pg * 8;
      if (co < it.Cout && ci < it.C) {
        const unsigned short* sp = src + (size_t)tap * it.Cout * it.C + (size_t)co * it.C + ci;
        uint4 in[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) in[j] = *reinterpret_cast<const uint4*>(sp + (size_t)j * it.C);
        unsigned short* dp = dst + (size_t)(it.taps - 1 - tap) * it.Cout * it.C + (size_t)ci * it.Cout + co;
#pragma unroll
        for (int i = 0; i < 8; ++i) {                     // output row ci + i: element i of the eight input rows
          unsigned e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const unsigned w = (i >> 1) == 0 ? in[j].x : (i >> 1) == 1 ? in[j].y : (i >> 1) == 2 ? in[j].z : in[j].w;
            e[j] = (i & 1) ? (w >> 16) : (w & 0xffffu);
          }
          *reinterpret_cast<uint4*>(dp + (size_t)i * it.Cout) = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
        }
      }
    }
    return;
  }
  const int s0 = blockmap ? blockmap[2 * blockIdx.x + 1] : (int)blockIdx.x;
  const int send = blockmap ? (s0 + RUA_WPREP_TPB < ntiles ? s0 + RUA_WPREP_TPB : ntiles) : ntiles;
  for (int t = s0; t < send; t += blockmap ? 1 : (int)gridDim.x) {
    const int tap = t / (tco * tci), r = t - tap * tco * tci;
    const int co0 = (r / tci) * 64, ci0 = (r % tci) * 64;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int co = co0 + ty + k * 16, ci = ci0 + tx * 4;
      unsigned short v[4] = {0, 0, 0, 0};
      if (co < it.Cout) {
        const size_t o = (size_t)tap * it.Cout * it.C + (size_t)co * it.C + ci;
        if (vec && ci + 3 < it.C) {
          const uint2 q = *reinterpret_cast<const uint2*>(src + o);
          v[0] = (unsigned short)(q.x & 0xffffu); v[1] = (unsigned short)(q.x >> 16); v[2] = (unsigned short)(q.y & 0xffffu); v[3] = (unsigned short)(q.y >> 16);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (ci + j < it.C) v[j] = src[o + j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[ty + k * 16][tx * 4 + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ci = ci0 + ty + k * 16, co = co0 + tx * 4;
      if (ci < it.C) {
        unsigned short v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = tile[tx * 4 + j][ty + k * 16];
        unsigned short* d = dst + (size_t)(it.taps - 1 - tap) * it.Cout * it.C + (size_t)ci * it.Cout + co;
        if (vec && co + 3 < it.Cout) *reinterpret_cast<uint2*>(d) = make_uint2((unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16));
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (co + j < it.Cout) d[j] = v[j];
        }
      }
    }
    __syncthreads();
  }
}
extern "C" int rua_wprep_blocks(int taps, int Cout, int C) {           // blocks of the block map a [taps][Cout][C] item takes
  const int ntiles = taps * ((Cout + 63) / 64) * ((C + 63) / 64);
  return (ntiles + RUA_WPREP_TPB - 1) / RUA_WPREP_TPB;
}
extern "C" int rua_weight_prep_dgrad(const void* w_fwd, void* w_dgrad, const rua_wprep_item* items_dev, int n_items, int max_elems, const int32_t* blockmap_dev,
                                     int n_blocks, int dtype, void* stream) {
  RUA_CHECK_ARG(w_fwd && w_dgrad && items_dev && n_items > 0, "rua_weight_prep_dgrad: bad arguments");
  RUA_CHECK_ARG(dtype == RUA_BF16, "rua_weight_prep_dgrad: bf16 copies only (the fp32 path keeps rua_weight_prep)");
  RUA_CHECK_ARG(!blockmap_dev || n_blocks >= 1, "rua_weight_prep_dgrad: a block map needs its length");
  if (blockmap_dev) {
    hipLaunchKernelGGL(wprep_dgrad_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w_fwd, (bf16_t*)w_dgrad, items_dev, (const int*)blockmap_dev);
  } else {
    int gx = rua_div_up(max_elems, 4096 * 4); if (gx < 1) gx = 1; if (gx > 256) gx = 256;
    hipLaunchKernelGGL(wprep_dgrad_kernel, dim3(gx, n_items), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w_fwd, (bf16_t*)w_dgrad, items_dev, (const int*)nullptr);
  }
  RUA_LAUNCH_CHECK("wprep_dgrad_kernel");
  return RUA_OK;
}

// tile width (output channels per block) the launcher picks for a descriptor: identifies the kernel instantiation
extern "C" int64_t rua_conv_workspace_bytes(const rua_conv_desc* d) {
  if (!d) return 0;
  return (int64_t)d->N * d->H * d->W * d->Cout * (int64_t)sizeof(float);
}

extern "C" int rua_conv_tile_bn(const rua_conv_desc* d) {
  if (!d) return RUA_ERR_ARG;
  if (pick_dmap(d)) return 128;
  return pick_bn(d, (long long)d->N * d->H * d->W);
}
// 0: conv_igemm (register-staged), 1: conv_dma (LDS-DMA), 2: conv_dmap (LDS-DMA, pipelined across the stage barrier),
// 3: conv_halo (input + halo resident in LDS, lattice tiles)
extern "C" int rua_conv_fused_input_ok(const rua_conv_desc* d) { return (d && rua_pick_strip(d)) ? 1 : 0; }

extern "C" int rua_conv_kernel_id(const rua_conv_desc* d) {
  if (!d) return RUA_ERR_ARG;
  if (rua_pick_strip(d)) return 5;
  if (pick_halo(d)) return 3;
  if (pick_pw(d)) return 4;
  if (pick_small(d)) return 6;
  if (rua_pick_img2(d)) return 8;
  if (!g_conv_group && rua_band128_sum_ok(d)) return 9;
  if (pick_img(d)) return 7;
  if (pick_dmap(d)) return 2;
  return pick_dma(d, pick_bn(d, (long long)d->N * d->H * d->W)) ? 1 : 0;
}
extern "C" int rua_conv_tile_bm(const rua_conv_desc* d) {
  if (!d) return RUA_ERR_ARG;
  const long long M = (long long)d->N * d->H * d->W;
  if (pick_dmap(d)) {                                   // mirrors the launcher: 64-row tiles in the unsplit half-chip case
    const int target = g_tune.dmap_target > 0 ? g_tune.dmap_target : rua_cu_count();
    const int bm64 = g_tune.dmap_bm64;
    const long long tiles = ((M + 127) / 128) * ((d->Cout + 127) / 128);
    int units = 0;
    for (int i = 0; i < d->nseg; ++i) units += d->seg[i].taps * (d->seg[i].C / 32);
    const bool split = d->workspace && d->workspace_bytes > 4096 &&
                       (size_t)(d->workspace_bytes - 4096) / ((size_t)M * d->Cout * sizeof(float)) >= 2 && units / 2 > 40;
    return (bm64 && !split && tiles < target && tiles * 2 >= target) ? 64 : 128;
  }
  return pick_bm(d, M, pick_bn(d, M));
}

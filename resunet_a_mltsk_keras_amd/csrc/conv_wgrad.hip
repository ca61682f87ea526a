// Weight gradients of the convolutions on MFMA (gfx950): dW[t][co][c] += sum_pix dy[pix][co] * a[src(pix,t)][c].
// Kernels: wgrad_kernel (generic, K split over pixels), wgrad_dmap (LDS-DMA), wgrad_taps (all taps per block), wgrad_rows32 / 64 and
// wgrad_rowsx (wgrad_rowsx.inc: whole rows in one LDS-DMA ring), wgrad_img / wgrad_imgs (whole images resident), wgrad_pw (1x1), the
// deterministic reductions of their partials.
// Host side (behind the kernels): wgrad_plan_one() - descriptor -> WgLaunch, a pure function of descriptor, tuning and CU count - and wgrad_issue() /
// wgrad_reduce(), which launch plans through one table of kernels (WG_KERNEL).
// Exports, each a composition of those: rua_conv_wgrad, rua_conv_wgrad_group, rua_wgrad_kind, rua_wgrad_plan and the other rua_wgrad_* queries, rua_wgrad_reduce_batch.
#include "common.h"

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

// =========================================================================================
// Host side: plan, then issue.  wgrad_plan_one() turns a descriptor into a WgLaunch - kernel, grid, LDS, kernel arguments, the reduction it leaves
// pending - as a pure function of the descriptor, g_tune and rua_cu_count(): it launches nothing and keeps no state.  wgrad_issue() puts plans of
// one kernel on a stream (one: the kernel itself; several: its grouped form), wgrad_reduce() a plan's reduction.  Every export below is a composition
// of these, so what rua_wgrad_plan / rua_wgrad_group_plan report is what the launch does.
enum WgKernel {
  WG_TILES_BF16, WG_TILES_F32, WG_TAPS32, WG_TAPS64,
  WG_ROWS32_N4_BN, WG_ROWS32_N4, WG_ROWS32_N2_BN, WG_ROWS32_N2, WG_ROWS64_BN, WG_ROWS64, WG_ROWSX0, WG_ROWSX1,      // rows32: + 2 (two pixel groups) + 1 (no BatchNorm on load)
  WG_DMAP, WG_IMG8, WG_IMG16, WG_IMGS8, WG_IMGS16,
  WG_PW11, WG_PW12, WG_PW21, WG_PW22,                                                                                // + 2 (Cout > 32) + 1 (C > 32)
  WG_KERNELS
};
enum WgArgs { WG_ARGS_K, WG_ARGS_D, WG_ARGS_T, WG_ARGS_P };      // WgK, WgdK, WgtK, WgpK
struct WgLaunch {
  int kernel;                                  // WgKernel
  unsigned gx, gy, block; int smem;            // grid of a launch of its own, threads per block, dynamic LDS bytes
  union { WgK g; WgdK d; WgtK t; WgpK p; } k;  // the member of WgKernelRow.args
  rua_wgrad_pending pending;                   // the reduction the kernel leaves behind (kind 0: none)
  bool defer;                                  // rua_wgrad_desc.defer: the caller runs that reduction (rua_wgrad_reduce_batch)
  bool groupable;                              // rua_conv_wgrad_group may put it into a grid shared with other members on the same kernel (tuning key wgrad_group)
};

// one row per WgKernel: the kernel, its grouped form (null: none), which arguments they take, the dynamic LDS to allow through hipFuncSetAttribute (0: the default will do)
struct WgKernelRow { const char* name; const void* one; const void* many; int args; int lds; };
#define WG_FN(...) reinterpret_cast<const void*>(&__VA_ARGS__)
static const WgKernelRow WG_KERNEL[WG_KERNELS] = {
  {"wgrad_kernel", WG_FN(wgrad_kernel<bf16_t>), WG_FN(wgrad_kernel_g), WG_ARGS_K, 0},
  {"wgrad_kernel", WG_FN(wgrad_kernel<float>), nullptr, WG_ARGS_K, 0},
  {"wgrad_taps_kernel", WG_FN(wgrad_taps_kernel<32>), WG_FN(wgrad_taps_kernel_g<32>), WG_ARGS_T, 160 * 1024},
  {"wgrad_taps_kernel", WG_FN(wgrad_taps_kernel<64>), WG_FN(wgrad_taps_kernel_g<64>), WG_ARGS_T, 160 * 1024},
  {"wgrad_rows32", WG_FN(wgrad_rows32<4, true>), WG_FN(wgrad_rows32_g<4, true>), WG_ARGS_T, 160 * 1024},
  {"wgrad_rows32", WG_FN(wgrad_rows32<4, false>), WG_FN(wgrad_rows32_g<4, false>), WG_ARGS_T, 160 * 1024},
  {"wgrad_rows32", WG_FN(wgrad_rows32<2, true>), WG_FN(wgrad_rows32_g<2, true>), WG_ARGS_T, 160 * 1024},
  {"wgrad_rows32", WG_FN(wgrad_rows32<2, false>), WG_FN(wgrad_rows32_g<2, false>), WG_ARGS_T, 160 * 1024},
  {"wgrad_rows64", WG_FN(wgrad_rows64<true>), WG_FN(wgrad_rows64_g<true>), WG_ARGS_T, 160 * 1024},
  {"wgrad_rows64", WG_FN(wgrad_rows64<false>), WG_FN(wgrad_rows64_g<false>), WG_ARGS_T, 160 * 1024},
  {"wgrad_rowsx", WG_FN(wgrad_rowsx<0>), WG_FN(wgrad_rowsx_g<0>), WG_ARGS_T, 160 * 1024},
  {"wgrad_rowsx", WG_FN(wgrad_rowsx<1>), WG_FN(wgrad_rowsx_g<1>), WG_ARGS_T, 160 * 1024},
  {"wgrad_dmap", WG_FN(wgrad_dmap), WG_FN(wgrad_dmap_g), WG_ARGS_D, 96 * 1024},
  {"wgrad_img", WG_FN(wgrad_img<8>), nullptr, WG_ARGS_K, 160 * 1024},
  {"wgrad_img", WG_FN(wgrad_img<16>), nullptr, WG_ARGS_K, 160 * 1024},
  {"wgrad_imgs", WG_FN(wgrad_imgs<8>), nullptr, WG_ARGS_K, 160 * 1024},
  {"wgrad_imgs", WG_FN(wgrad_imgs<16>), nullptr, WG_ARGS_K, 160 * 1024},
  {"wgrad_pw", WG_FN(wgrad_pw<1, 1>), WG_FN(wgrad_pw_g<1, 1>), WG_ARGS_P, 0},
  {"wgrad_pw", WG_FN(wgrad_pw<1, 2>), WG_FN(wgrad_pw_g<1, 2>), WG_ARGS_P, wgrad_pw_smem<1, 2>()},
  {"wgrad_pw", WG_FN(wgrad_pw<2, 1>), WG_FN(wgrad_pw_g<2, 1>), WG_ARGS_P, wgrad_pw_smem<2, 1>()},
  {"wgrad_pw", WG_FN(wgrad_pw<2, 2>), WG_FN(wgrad_pw_g<2, 2>), WG_ARGS_P, wgrad_pw_smem<2, 2>()},
};
#undef WG_FN

static int64_t wg_taps_bytes(const rua_wgrad_desc* d) { return (int64_t)rua_cu_count() * 9 * 32 * (int64_t)d->C * 4; }   // one block partial of [9][32][C] fp32 per CU

extern "C" int64_t rua_wgrad_workspace_bytes(const rua_wgrad_desc* d) {
  if (!d) return 0;
  // all-taps block partials, or 64 K-slice slabs of dW (capped at 64 MiB: the planner splits K no further than the slabs that
  // fit), + wgrad_pw's replicas and ticket (the tail)
  int64_t slabs = (int64_t)64 * d->taps * d->Cout * d->C * 4;
  if (slabs > (64ll << 20)) slabs = 64ll << 20;
  const int64_t taps = wg_taps_bytes(d);
  return (taps > slabs ? taps : slabs) + WG_PW_TAIL;
}

// K slices that fit the caller's workspace as fp32 slabs (the last WG_PW_TAIL bytes belong to wgrad_pw); 1: no room
static int slab_capacity(const rua_wgrad_desc* d, long long ndw) {
  if (!d->workspace || d->workspace_bytes <= WG_PW_TAIL) return 1;
  const long long n = (d->workspace_bytes - WG_PW_TAIL) / (ndw * 4);
  return n > 64 ? 64 : (int)n;
}

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
// wgrad_rowsx<1>: C = Cout = 256 on 32-pixel rows, an even number of images (the level-4 ResBlock), dilation <= 16 (the zeros between the two rows of a slot)
static bool wgrad_rows256_ok(const rua_wgrad_desc* d) {
  return (g_tune.wgrad_rows & 32) && d->dtype == RUA_BF16 && d->taps == 9 && d->stride == 1 && d->C == 256 && d->Cout == 256 && d->W == 32 && d->N % 2 == 0 && d->N >= 2 &&
         d->Hs == d->H && d->Ws == d->W && d->dil >= 1 && d->dil <= 16 && !d->in_scale && d->workspace && d->workspace_bytes >= wg_taps_bytes(d) &&
         (long long)d->N * d->H * d->W * d->C * 2 < (1ll << 31);
}
// which kernel family a descriptor lands on: 0 generic tiles (or a whole-image kernel: wgrad_img_pick), 1 all-taps, 2 wgrad_dmap, 3 wgrad_pw
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
  const bool rows128 = (g_tune.wgrad_rows & 4) && d->C == 128 && d->W == 64 && !d->in_scale;      // wgrad_rowsx<0> (the level-3 ResBlock)
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

// ---- planning ----------------------------------------------------------------------------------------------------------
static void wgrad_plan_grid(WgLaunch* L, int kernel, unsigned gx, unsigned gy, unsigned block, size_t smem, int group_bit) {
  L->kernel = kernel; L->gx = gx; L->gy = gy; L->block = block; L->smem = (int)smem; L->groupable = (g_tune.wgrad_group & group_bit) != 0;
}
static void wgrad_plan_pending(WgLaunch* L, int kind, int parts, long long n, const float* partials, float* dw, int CC) {
  rua_wgrad_pending& r = L->pending;
  r.kind = kind; r.parts = parts; r.n = n; r.partials = partials; r.dw = dw; r.CC = CC;
  r.blocks = kind == 1 ? rua_div_up((int)(n / 4), TAPS_RED_COLS) : (int)((n / 4 + SLAB_RED_COLS - 1) / SLAB_RED_COLS);
}

// wgrad_rows32 / wgrad_rows64: a worker is a block that owns whole rows.  The N x dil chains are cut into segments of >= 4 lattice rows (a segment re-reads two
// window rows) for `blocks` blocks - one round for the members that share the chip, at most `most`: the workspace holds one partial per CU, and a block that owns
// both output-channel halves leaves two.  Returns grid.x.
static int wgrad_rows_split(const rua_wgrad_desc* d, WgtK& k, int npg, int blocks, int most) {
  if (blocks < 1) blocks = 1;
  if (blocks > most) blocks = most;
  const int ny = (d->H + d->dil - 1) / d->dil;         // lattice rows of the longest chain
  k.NPG = npg; k.strips = 1;
  k.nchains = d->N * d->dil;
  int spc = blocks / k.nchains;
  if (spc < 1) spc = 1;
  if (spc > (ny + 3) / 4) spc = (ny + 3) / 4;
  if (spc < 1) spc = 1;
  k.seglen = (ny + spc - 1) / spc;
  k.spc = (ny + k.seglen - 1) / k.seglen;
  k.njobs = k.nchains * k.spc;
  int gx = k.njobs < blocks ? k.njobs : blocks;
  if (g_tune.wgrad_rows & 128) {                       // the slot stream (WgSlots): every block an equal share of the rows + separators
    const long long U = (long long)d->N * (d->H + d->dil);
    k.sx = 1; gx = (int)(U / 4 < blocks ? (U / 4 > 0 ? U / 4 : 1) : blocks);
  }
  k.gx = gx; k.nworkers = gx;
  k.jpw = (k.njobs + gx - 1) / gx;
  return gx;
}

// rua_wgrad_kind() == 1: the all-taps kernels and the row kernels that took over most of their shapes
static void wgrad_plan_taps(const rua_wgrad_desc* d, WgLaunch* L) {
  const int CC = d->C, ncu = rua_cu_count();
  WgtK& k = L->k.t;
  k.a = (const unsigned char*)d->a; k.dy = (const unsigned char*)d->dy; k.scratch = (float*)d->workspace; k.dw = d->dw;
  k.H = d->H; k.W = d->W; k.N = d->N; k.dil = d->dil;
  k.in_scale = d->in_scale; k.in_shift = d->in_shift; k.in_relu = d->in_relu; k.sx = 0;
  const long long M = (long long)d->N * d->H * d->W;
  k.abytes = (unsigned)((size_t)M * CC * 2); k.dybytes = k.abytes;
  if (CC == 256 || CC == 128) {
    // wgrad_rowsx: gx blocks per grid row share the slot stream of the member evenly; grid.y = (output-channel slice, input-channel half); a block leaves two
    // partials [9][32][C] (or its 128 columns of them), so C / 32 x gx of them <= one per CU - the workspace contract of the all-taps kernels
    const int gy = CC == 256 ? 8 : 2;
    const int share = (g_tune.wgrad_taps_share && d->group_members > 1) ? d->group_members : 1;
    int gx = ncu / share / gy;
    if (gx > ncu / (CC / 32)) gx = ncu / (CC / 32);
    const long long U = (long long)(CC == 256 ? d->N / 2 : d->N) * (d->H + d->dil);
    if (gx > U / 4) gx = (int)(U / 4);                 // >= 4 slots behind a block's three-row fill
    if (gx < 1) gx = 1;
    k.NPG = 1; k.strips = 1; k.halo = 0; k.halo4 = 0; k.group_bytes = 0; k.nchains = 0; k.spc = 0; k.seglen = 0; k.njobs = 0; k.jpw = 0;
    k.gx = gx; k.nworkers = gx;
    wgrad_plan_grid(L, CC == 256 ? WG_ROWSX1 : WG_ROWSX0, gx, gy, 768, (size_t)32 * 256 + 5 * (size_t)96 * 256 + 3 * (size_t)64 * 128, 4);
    wgrad_plan_pending(L, 1, gx, (long long)9 * CC * CC, k.scratch, d->dw, CC);
    return;
  }
  k.halo = 64 + 2 * d->dil;
  k.halo4 = (k.halo + 3) / 4 * 4;
  k.group_bytes = 64 * 64 + 3 * k.halo4 * CC * 2;
  k.NPG = (CC == 32) ? 4 : 2;                          // 12 waves per block either way (3 kernel rows x CC/32 halves per group)
  const int gy = CC / 32, group_bit = CC == 32 ? 2 : 4;
  // the members of a grouped launch share ONE round of blocks (four members of 256 blocks each ran four rounds, every block with
  // its own prologue and 36 - 74 KB of partials to write and to reduce): tuning key wgrad_taps_share
  const int share = (g_tune.wgrad_taps_share && (g_tune.wgrad_group & group_bit) && d->group_members > 1) ? d->group_members : 1;
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
  size_t smem = (size_t)k.group_bytes * k.NPG;
  const size_t red = (size_t)(k.NPG - 1) * 3 * (CC / 32) * 3 * 16 * 64 * 4;
  if (red > smem) smem = red;
  wgrad_plan_grid(L, CC == 32 ? WG_TAPS32 : WG_TAPS64, gx, gy, 768, smem, group_bit);
  const bool rows_ok = d->dil <= 31 && (!d->in_scale || d->in_relu) && (size_t)M * CC * 2 < 0x80000000ull;
  if (g_tune.wgrad_rows && CC == 32 && (d->W == 256 || d->W == 128) && rows_ok) {
    // full-width rows at C = 32: wgrad_rows32 (tuning key wgrad_rows) - the block's pixel groups share ONE ring of whole rows
    const int npg = d->W / 64;
    gx = wgrad_rows_split(d, k, npg, ncu / share, ncu);
    smem = (size_t)32 * 64 + 6 * (size_t)(d->W + 32) * 64 + 3 * (size_t)d->W * 64 + 128 * 4;
    const size_t red2 = (size_t)(npg - 1) * 3 * 3 * 16 * 64 * 4;
    if (red2 > smem) smem = red2;
    wgrad_plan_grid(L, WG_ROWS32_N4_BN + (npg == 2 ? 2 : 0) + (d->in_scale ? 0 : 1), gx, 1, npg * 192, smem, group_bit);
  } else if ((g_tune.wgrad_rows & 2) && CC == 64 && d->W == 128 && rows_ok) {
    // C = 64 on 128-pixel rows (the level-2 ResBlock): wgrad_rows64 - a block owns whole rows and BOTH output-channel halves (tuning key wgrad_rows & 2)
    gx = wgrad_rows_split(d, k, 2, ncu / share, ncu / 2);
    wgrad_plan_grid(L, d->in_scale ? WG_ROWS64_BN : WG_ROWS64, gx, 1, 768, (size_t)32 * 128 + 5 * (size_t)(128 + 32) * 128 + 3 * (size_t)128 * 128 + 256 * 4, group_bit);
  }
  wgrad_plan_pending(L, 1, gx, (long long)9 * CC * CC, k.scratch, d->dw, CC);
}

// rua_wgrad_kind() == 3: every wave streams a pixel range of its own
static void wgrad_plan_pw(const rua_wgrad_desc* d, WgLaunch* L) {
  WgpK& k = L->k.p;
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
  const unsigned grid = (unsigned)((k.M + ppw * 16 - 1) / (ppw * 16));
  k.nblk = (int)grid;
  // replicas: atomic chains of ~64 blocks per address; fewer replicas = fewer exchanges for the finishing block
  k.R = k.nblk / 32; if (k.R < 1) k.R = 1; if (k.R > WG_PW_REPLICAS) k.R = WG_PW_REPLICAS;
  if (g_tune.wgpw_r > 0) k.R = g_tune.wgpw_r > WG_PW_REPLICAS ? WG_PW_REPLICAS : g_tune.wgpw_r;
  // block partials in front of the tail (tuning key wgrad_pw, bit 1) where the workspace holds one per block; else replicas + tickets (nothing pending)
  const long long nel = (long long)d->Cout * d->C;
  // (a call that reduces right away keeps the replicas unless bit 2 is set: one block walking 256 partials of a 2 KB dW - the stem's - takes 10 us longer than the tickets)
  const bool slab = (g_tune.wgrad_pw & 2) && (d->defer || (g_tune.wgrad_pw & 4)) && (long long)grid * nel * 4 <= (long long)d->workspace_bytes - WG_PW_TAIL;
  k.slabs = slab ? (float*)d->workspace : nullptr;
  constexpr int lds[4] = {wgrad_pw_smem<1, 1>(), wgrad_pw_smem<1, 2>(), wgrad_pw_smem<2, 1>(), wgrad_pw_smem<2, 2>()};
  const int form = (nco - 1) * 2 + (nci - 1);
  wgrad_plan_grid(L, WG_PW11 + form, grid, 1, 1024, lds[form], 16);      // (bit 16: only a group of nothing but wgrad_pw members shares grids)
  if (slab) wgrad_plan_pending(L, 2, (int)grid, nel, k.slabs, d->dw, 0);
}

// rua_wgrad_kind() == 2
static void wgrad_plan_dmap(const rua_wgrad_desc* d, WgLaunch* L) {
  WgdK& k = L->k.d;
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
  wgrad_plan_grid(L, WG_DMAP, (unsigned)(tiles * k.ksplit), 1, 256, 96 * 1024, 8);
  if (k.slabs) wgrad_plan_pending(L, 2, k.ksplit, ndw, k.slabs, d->dw, 0);
}

// The plan of one weight gradient.  want: K slices a batched launch asks this member to take (wgrad_batch_split; only the generic tile kernel listens), 0: its own split.
static int wgrad_plan_one(const rua_wgrad_desc* d, long long want_hint, WgLaunch* L) {
  memset(L, 0, sizeof(*L));
  RUA_CHECK_ARG(d && d->a && d->dy && d->dw, "rua_conv_wgrad: null pointer");
  RUA_CHECK_ARG(d->dtype == RUA_F32 || d->dtype == RUA_BF16, "rua_conv_wgrad: bad dtype");
  const int vec = d->dtype == RUA_BF16 ? 8 : 4;
  RUA_CHECK_ARG(d->C % vec == 0 && d->Cout % vec == 0, "rua_conv_wgrad: C=%d Cout=%d must be multiples of %d", d->C, d->Cout, vec);
  RUA_CHECK_ARG(d->taps == 1 || d->taps == 9, "rua_conv_wgrad: taps must be 1 or 9");
  L->defer = d->defer != 0;
  const int kind = rua_wgrad_kind(d);
  if (kind == 1) { wgrad_plan_taps(d, L); return RUA_OK; }
  RUA_CHECK_ARG(d->in_scale == nullptr, "rua_conv_wgrad: in_scale / in_shift (normalise on load) needs the all-taps kernel (rua_wgrad_kind() == 1)");
  if (kind == 2) { wgrad_plan_dmap(d, L); return RUA_OK; }
  if (kind == 3) { wgrad_plan_pw(d, L); return RUA_OK; }
  RUA_CHECK_ARG((long long)(d->H - 1) * d->stride < d->Hs && (long long)(d->W - 1) * d->stride < d->Ws,
                "rua_conv_wgrad: input %dx%d too small for gradient %dx%d stride %d", d->Hs, d->Ws, d->H, d->W, d->stride);
  WgK& k = L->k.g;
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
  const long long ndw = (long long)d->taps * d->Cout * d->C;
  const int img_kind = wgrad_img_pick(d);
  if (img_kind == 2) {
    // wgrad_imgs: whole images resident in LDS, 32 x 32 tiles of dW for all nine taps, the 512-pixel chunks streamed through a two-stage ring - no K slices, no slabs
    k.ksplit = (int)(k.M / 512); k.pix_per_block = 512; k.slabs = nullptr;
    k.nti = d->C / 32; k.ntc = d->Cout / 32;
    // LDS: the ring (2 x 67 840 B) and, after it, the four k-quarters' accumulators (147 456 B)
    wgrad_plan_grid(L, d->W == 8 ? WG_IMGS8 : WG_IMGS16, (unsigned)(k.nti * k.ntc), 1, 768, 4 * 9 * 16 * 64 * 4, 0);
    return RUA_OK;
  }
  if (img_kind == 1) {
    // wgrad_img: a 64 x 64 tile of dW for all nine taps per block, 512-pixel chunks as K slices
    k.ksplit = (int)(k.M / 512);
    k.pix_per_block = 512;
    k.slabs = k.ksplit > 1 ? (float*)d->workspace : nullptr;
    wgrad_plan_grid(L, d->W == 8 ? WG_IMG8 : WG_IMG16, (unsigned)(k.ntc * k.nti * k.ksplit), 1, 768, 2 * 512 * 128 + 2 * 18 * 128, 0);
    if (k.slabs) wgrad_plan_pending(L, 2, k.ksplit, ndw, k.slabs, d->dw, 0);
    return RUA_OK;
  }
  const long long tiles = (long long)k.ntc * k.nti * d->taps;
  // K split: every slice adds the whole dW tile with fp32 atomics (~1.3 TB/s chip-wide), so slices x |dW| must stay
  // small: ~512 blocks fill the chip; 2048 blocks meant 33 MB of atomics (~25 us) per launch.
  const int target = (g_tune.wgrad_blocks > 0 ? g_tune.wgrad_blocks : 2 * rua_cu_count());      // 512 on MI355X
  long long want = target / tiles; if (want < 1) want = 1;
  long long stages = (k.M + 63) / 64;
  if (want_hint > 0) want = want_hint;                 // a member of a batched launch: its share of the batch's blocks
  if (want > stages) want = stages;
  const int cap = (g_tune.wgrad_slabs && ndw % 4 == 0) ? slab_capacity(d, ndw) : 0;
  if (cap >= 2 && want > cap) want = cap;              // deterministic K split: one fp32 slab per slice must fit the workspace
  long long spb = (stages + want - 1) / want;          // stages per block
  k.pix_per_block = (int)(spb * 64);
  k.ksplit = (int)((k.M + k.pix_per_block - 1) / k.pix_per_block);
  k.slabs = (cap >= 2 && k.ksplit > 1) ? (float*)d->workspace : nullptr;
  const long long grid = tiles * k.ksplit;
  RUA_CHECK_ARG(grid < (1ll << 31), "rua_conv_wgrad: grid too large");
  wgrad_plan_grid(L, d->dtype == RUA_BF16 ? WG_TILES_BF16 : WG_TILES_F32, (unsigned)grid, 1, 256, 0, d->dtype == RUA_BF16 ? 1 : 0);
  if (k.slabs) wgrad_plan_pending(L, 2, k.ksplit, ndw, k.slabs, d->dw, 0);
  return RUA_OK;
}
// plan + the record the call leaves for rua_wgrad_reduce_batch
static int wgrad_plan_record(const rua_wgrad_desc* d, long long want, WgLaunch* L, rua_wgrad_pending* out) {
  const int rc = wgrad_plan_one(d, want, L);
  *out = L->pending;
  out->overwrite_dev = d->overwrite_dev;
  return rc;
}

// ---- issuing -----------------------------------------------------------------------------------------------------------
// One grid for m >= 1 plans of the SAME kernel.  One plan: the kernel itself.  Several: its grouped form - blockIdx.y picks the member (blockIdx.z in the all-taps
// family, whose grid.y is the output-channel slice); the grid and the LDS are the largest member's, the others' surplus blocks leave at once.  always_grouped: the
// grouped form for a single member too (the wgrad_pw forms of an all-wgrad_pw group, as they always went out).
static int wgrad_issue(const WgLaunch* const* L, int m, hipStream_t st, bool always_grouped = false) {
  const WgLaunch& first = *L[0];
  const WgKernelRow& row = WG_KERNEL[first.kernel];
  const bool grouped = m > 1 || always_grouped;
  const void* fn = grouped ? row.many : row.one;
  const int slots = row.args == WG_ARGS_P ? RUA_MAX_BRANCH : RUA_MAX_WGRAD_GROUP;
  RUA_CHECK_ARG(fn && m <= slots, "rua_conv_wgrad_group: %d members of %s in one grid", m, row.name);
  static RuaPerDevFlag allowed[WG_KERNELS][2];        // hipFuncSetAttribute: once per (kernel, device)
  bool& ok = allowed[first.kernel][grouped].get();
  if (!ok && row.lds) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, row.lds);
  ok = true;
  dim3 grid(first.gx, first.gy);
  int smem = first.smem;
  union { WgKG g; WgdKG d; WgtKG t; WgpKG p; } many;
  void* args[1] = {const_cast<void*>(static_cast<const void*>(&first.k))};
  if (grouped) {
    for (int i = 0; i < slots; ++i) {                  // (unused slots repeat member 0)
      const WgLaunch& x = *L[i < m ? i : 0];
      if (x.gx > grid.x) grid.x = x.gx;
      if (x.smem > smem) smem = x.smem;
      switch (row.args) {
        case WG_ARGS_K: many.g.k[i] = x.k.g; break;
        case WG_ARGS_D: many.d.k[i] = x.k.d; break;
        case WG_ARGS_T: many.t.k[i] = x.k.t; break;
        default: many.p.k[i] = x.k.p; break;
      }
    }
    if (first.kernel == WG_DMAP) grid.x = (grid.x + 7) / 8 * 8;
    if (row.args == WG_ARGS_T) grid.z = m; else grid.y = m;
    args[0] = &many;
  }
  (void)hipLaunchKernel(fn, grid, dim3(first.block), args, (size_t)smem, st);
  RUA_LAUNCH_CHECK(row.name);
  return RUA_OK;
}
// the reduction a plan leaves pending, as a launch of its own (deferred ones go through rua_wgrad_reduce_batch instead)
static int wgrad_reduce(const rua_wgrad_pending& r, hipStream_t st) {
  if (r.kind == 1) {
    hipLaunchKernelGGL(wgrad_taps_reduce, dim3(r.blocks), dim3(256), 0, st, r.partials, r.dw, r.CC, r.parts);
    RUA_LAUNCH_CHECK("wgrad_taps_reduce");
  } else if (r.kind == 2) {
    hipLaunchKernelGGL(wgrad_slab_reduce, dim3(r.blocks), dim3(256), 0, st, r.partials, r.dw, r.n / 4, r.parts);
    RUA_LAUNCH_CHECK("wgrad_slab_reduce");
  }
  return RUA_OK;
}
// a plan on its own: its grid, then - unless deferred - the mid event and its reduction
static int wgrad_issue_alone(const WgLaunch& L, hipStream_t st) {
  const WgLaunch* one = &L;
  const int rc = wgrad_issue(&one, 1, st);
  if (rc != RUA_OK || L.defer || !L.pending.kind) return rc;
  rua_record_mid_event(st);
  return wgrad_reduce(L.pending, st);
}

// ---- exports -----------------------------------------------------------------------------------------------------------
extern "C" int rua_wgrad_plan(const rua_wgrad_desc* d, rua_wgrad_pending* out) {
  RUA_CHECK_ARG(d && out, "rua_wgrad_plan: null pointer");
  WgLaunch L;
  return wgrad_plan_record(d, 0, &L, out);
}
extern "C" int rua_conv_wgrad(const rua_wgrad_desc* d, void* stream) {
  WgLaunch L;
  const int rc = wgrad_plan_one(d, 0, &L);
  return rc != RUA_OK ? rc : wgrad_issue_alone(L, (hipStream_t)stream);
}

// rua_conv_wgrad_group: n INDEPENDENT weight gradients (the dilation branches of a ResBlock) with the results of n rua_conv_wgrad
// calls.  Members that land on the same kernel go out as ONE grid, the rest one by one.  Members that share partial-sum workspace
// cannot overlap: such a group runs member by member.
static thread_local int g_wg_group_last_grids = 0;     // per calling thread: rua_hip.h promises the count of the thread's own latest call
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
// member it belongs to.  want[i] = K slices asked for (wgrad_plan_one bounds it by the member's stages and slab capacity); 0: the split it would take alone
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
// the plans and records of a batched call (wgrad_batch_ok): consecutive runs of RUA_MAX_WGRAD_BATCH members share a grid and its block budget
static int wgrad_batch_plan(const rua_wgrad_desc* d, int n, WgLaunch* L, rua_wgrad_pending* out) {
  for (int base = 0; base < n; base += RUA_MAX_WGRAD_BATCH) {
    const int m = n - base < RUA_MAX_WGRAD_BATCH ? n - base : RUA_MAX_WGRAD_BATCH;
    long long want[RUA_MAX_WGRAD_BATCH];
    wgrad_batch_split(d + base, m, want);
    for (int i = base; i < base + m; ++i) { const int rc = wgrad_plan_record(d + i, want[i - base], L + i, out + i); if (rc != RUA_OK) return rc; }
  }
  return RUA_OK;
}
extern "C" int rua_wgrad_group_plan(const rua_wgrad_desc* d, int n, rua_wgrad_pending* out) {
  RUA_CHECK_ARG(d && out && n >= 1, "rua_wgrad_group_plan: bad arguments");
  WgLaunch L[WG_BATCH_MAX_MEMBERS];
  if (wgrad_batch_ok(d, n)) return wgrad_batch_plan(d, n, L, out);
  for (int i = 0; i < n; ++i) { const int rc = wgrad_plan_record(d + i, 0, L, out + i); if (rc != RUA_OK) return rc; }
  return RUA_OK;
}
static int wgrad_batch_launch(const rua_wgrad_desc* d, int n, hipStream_t st) {
  WgLaunch L[WG_BATCH_MAX_MEMBERS];
  rua_wgrad_pending recs[WG_BATCH_MAX_MEMBERS];
  const int rp = wgrad_batch_plan(d, n, L, recs);
  if (rp != RUA_OK) return rp;
  // members whose slabs overlap (a shared workspace) cannot run at once: member by member, as any group that shares workspace
  bool overlap = false;
  for (int i = 0; i < n && !overlap; ++i)
    for (int j = i + 1; j < n && !overlap; ++j) {
      if (recs[i].kind != 2 || recs[j].kind != 2) continue;
      const float* a0 = recs[i].partials; const float* b0 = recs[j].partials;
      overlap = a0 < b0 + (long long)recs[j].parts * recs[j].n && b0 < a0 + (long long)recs[i].parts * recs[i].n;
    }
  if (overlap) {
    g_wg_group_last_grids = n;
    for (int i = 0; i < n; ++i) { const int rc = rua_conv_wgrad(d + i, st); if (rc != RUA_OK) return rc; }
    return RUA_OK;
  }
  int grids = 0;
  for (int base = 0; base < n; base += RUA_MAX_WGRAD_BATCH) {
    const int m = n - base < RUA_MAX_WGRAD_BATCH ? n - base : RUA_MAX_WGRAD_BATCH;
    const WgLaunch* mem = L + base;
    int order[RUA_MAX_WGRAD_BATCH];
    for (int i = 0; i < m; ++i) order[i] = i;
    for (int i = 1; i < m; ++i) {                          // longest blocks first (stable: equal members keep the caller's order)
      const int o = order[i]; int j = i;
      while (j > 0 && mem[order[j - 1]].k.g.pix_per_block < mem[o].k.g.pix_per_block) { order[j] = order[j - 1]; --j; }
      order[j] = o;
    }
    WgKB g;
    unsigned long long total = 0;
    for (int i = 0; i < m; ++i) { g.k[i] = mem[order[i]].k.g; total += mem[order[i]].gx; g.end[i] = (unsigned)total; }
    for (int i = m; i < RUA_MAX_WGRAD_BATCH; ++i) { g.k[i] = g.k[0]; g.end[i] = (unsigned)total; }
    g.n = m;
    RUA_CHECK_ARG(total >= 1 && total < (1ull << 31), "rua_conv_wgrad_group: grid too large");
    hipLaunchKernelGGL(wgrad_kernel_b, dim3((unsigned)total), dim3(256), 0, st, g);
    RUA_LAUNCH_CHECK("wgrad_kernel_b");
    ++grids;
    for (int i = 0; i < m; ++i)                            // members that did not defer their reduction
      if (!mem[i].defer) { const int rr = wgrad_reduce(mem[i].pending, st); if (rr != RUA_OK) return rr; }
  }
  g_wg_group_last_grids = grids;
  return RUA_OK;
}
extern "C" int rua_conv_wgrad_group(const rua_wgrad_desc* d, int n, void* stream) {
  RUA_CHECK_ARG(d && n >= 1, "rua_conv_wgrad_group: no members");
  hipStream_t st = (hipStream_t)stream;
  if (wgrad_batch_ok(d, n)) return wgrad_batch_launch(d, n, st);
  RUA_CHECK_ARG(n <= RUA_MAX_WGRAD_GROUP, "rua_conv_wgrad_group: 1..%d members (more only in the batched form)", RUA_MAX_WGRAD_GROUP);
  WgLaunch L[RUA_MAX_WGRAD_GROUP];
  for (int i = 0; i < n; ++i) { const int rc = wgrad_plan_one(d + i, 0, L + i); if (rc != RUA_OK) return rc; }
  // which members go into shared grids
  bool shared = false;                                 // partial-sum workspace or dw in common: one by one
  bool allpw = n >= 2;                                 // nothing but wgrad_pw members with replicas / tickets (the workspace tails) of their own: one grid per (NCO, NCI) form
  for (int i = 0; i < n; ++i) {
    allpw = allpw && WG_KERNEL[L[i].kernel].args == WG_ARGS_P && L[i].groupable;
    for (int j = i + 1; j < n; ++j) {
      const char* a0 = (const char*)d[i].workspace; const char* b0 = (const char*)d[j].workspace;
      if (a0 && b0 && a0 < b0 + d[j].workspace_bytes && b0 < a0 + d[i].workspace_bytes) shared = true;
      if (d[i].dw == d[j].dw) shared = true;
    }
  }
  for (int i = 0; i < n && allpw; ++i)
    for (int j = i + 1; j < n; ++j) {
      const char* ti = (const char*)d[i].workspace + d[i].workspace_bytes - WG_PW_TAIL; const char* tj = (const char*)d[j].workspace + d[j].workspace_bytes - WG_PW_TAIL;
      if ((ti < tj + WG_PW_TAIL && tj < ti + WG_PW_TAIL) || d[i].dw == d[j].dw) allpw = false;
    }
  bool grouped[RUA_MAX_WGRAD_GROUP];
  for (int i = 0; i < n; ++i) {
    if (allpw) grouped[i] = i < RUA_MAX_BRANCH;                                    // (the slots of wgrad_pw_g)
    else grouped[i] = n > 1 && !shared && L[i].groupable && WG_KERNEL[L[i].kernel].args != WG_ARGS_P;
  }
  // the others first, in member order, each followed at once by its own reduction
  int grids = 0;
  for (int i = 0; i < n; ++i)
    if (!grouped[i]) { const int rc = wgrad_issue_alone(L[i], st); if (rc != RUA_OK) return rc; ++grids; }
  // then one grid per kernel: in order of first appearance (the wgrad_pw forms: in order of the form)
  bool done[RUA_MAX_WGRAD_GROUP] = {false};
  auto issue_kernel = [&](int kernel) {                // (all of wgrad_pw: the grouped kernel even for a form with one member)
    const WgLaunch* same[RUA_MAX_WGRAD_GROUP]; int m = 0;
    for (int j = 0; j < n; ++j)
      if (grouped[j] && !done[j] && L[j].kernel == kernel) { same[m++] = L + j; done[j] = true; }
    if (m == 0) return (int)RUA_OK;
    ++grids;
    return wgrad_issue(same, m, st, allpw);
  };
  if (allpw) {
    for (int kernel = WG_PW11; kernel <= WG_PW22; ++kernel) { const int rc = issue_kernel(kernel); if (rc != RUA_OK) return rc; }
  } else {
    for (int i = 0; i < n; ++i)
      if (grouped[i] && !done[i]) { const int rc = issue_kernel(L[i].kernel); if (rc != RUA_OK) return rc; }
  }
  g_wg_group_last_grids = grids;
  // then the reductions of the grouped members that did not defer theirs, in member order
  for (int i = 0; i < n; ++i)
    if (grouped[i] && !L[i].defer) { const int rc = wgrad_reduce(L[i].pending, st); if (rc != RUA_OK) return rc; }
  return RUA_OK;
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

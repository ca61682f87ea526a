// Weight preparation: the dtype copies of the fp32 master weights [taps][Cout][C] - forward layout and data-gradient layout
// [taps reversed][C][Cout] (wprep_kernel), or the data-gradient layout alone from the bf16 forward copy the optimizer wrote (wprep_dgrad_kernel).
// Exports: rua_weight_prep, rua_weight_prep_dgrad, rua_wprep_blocks.
#include "common.h"

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

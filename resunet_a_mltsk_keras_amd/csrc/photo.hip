// Photometric jitter of staged training windows (rua_window_photometric, include/rua_hip.h): a colour matrix with offsets, a tone
// curve and hashed noise applied to the uint8 windows [N][PH][PW][Cin] the cutting kernels left, before rua_multitask_targets
// reads them - so the network input and the colour head's HSV target are made from the same jittered bytes.  Integers only;
// scenes.host_photometric is the numpy definition and gives the same bytes.
//
// Per window an int32 row R[16] (Q16): M = R[0..8] (row-major 3 x 3), b = R[9..11], t = R[12], A = R[13], seed = R[14], R[15] = 0.
// For source byte p[c] of pixel (i, j), with >> arithmetic and clamp to [0, 255]:
//   colour  Cin == 3:  u[c] = clamp((M[c][0] p[0] + M[c][1] p[1] + M[c][2] p[2] + b[c] + 32768) >> 16)
//           Cin != 3:  u[c] = clamp((M[0][0] p[c] + b[0] + 32768) >> 16)                       (the host insists on a scalar row)
//   tone               v[c] = clamp(u[c] + ((t u[c] (255 - u[c]) + 2^23) >> 24))
//   noise   A != 0:    idx = (i PW + j) Cin + c;  x = seed + (idx + 1) 0x9E3779B9 (mod 2^32);  x ^= x >> 16;  x *= 0x7feb352d;
//                      x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16;  z = (sum of the four bytes of x) - 510;
//                      out[c] = clamp(v[c] + ((A z + 32768) >> 16))
// Under the host's limits |M| <= 2^20, |b| <= 2^29, |t| <= 65536, 0 <= A <= 65536 every intermediate fits in 32 bits:
//   3 * 2^20 * 255 + 2^29 + 2^15 < 2^31,   65536 * 127 * 128 + 2^23 < 2^31,   65536 * 510 + 2^15 < 2^31.
//
// A byte stream bound by memory and launch overhead.  The grid is laid out per window (blockIdx.y), so a lane never crosses from
// one row of the table into the next and the row is read through a block-uniform index of the kernel arguments.  Inside a window
// a lane owns runs of four units - a unit is a whole pixel at Cin == 3 (12 bytes, three dwords) and a single byte otherwise (one
// dword: no channel reads another there) - loaded and stored as aligned dwords.  A window starts at any byte when PH * PW * Cin
// is odd: the units in front of the first dword boundary (at Cin == 3: `start & 3` pixels, since 3 h = -start mod 4 has the
// solution h = start) and the up to three units behind the last whole run go bytewise, as rua_scene_stitch_maps treats its ragged
// ends.  Every byte is read and written by the same lane, loads before stores, so in place is safe.
//
// The rows travel as kernel arguments, PHO_CHUNK per launch; no device-side table, no copy, no synchronisation.
#include "common.h"

namespace {

constexpr int PHO_CHUNK = 48;                  // windows per launch: 64 bytes each
constexpr int PHO_MAXP = 512, PHO_MAXC = 16;
constexpr int PHO_MAXM = 1 << 20, PHO_MAXB = 1 << 29, PHO_MAXT = 65536, PHO_MAXA = 65536;
constexpr int PHO_RUNS = 4;                    // runs per lane the grid is sized for

struct PhotoArgs {
  int32_t row[PHO_CHUNK][16];                  // word 15 (reserved, 0 from the caller): 1 = leave this window alone
  const uint8_t* in; uint8_t* out;             // of the chunk's first window
  uint32_t wbytes;                             // PH * PW * Cin
  int pad;
};
static_assert(sizeof(PhotoArgs) <= 4096, "kernel arguments are limited to 4 KiB");

__device__ __forceinline__ int pho_clamp(int v) { return min(max(v, 0), 255); }

// tone and noise of one colour-mapped byte u at position idx of its window
__device__ __forceinline__ uint32_t pho_finish(int u, int t, int A, uint32_t seed, uint32_t idx) {
  int v = pho_clamp(u + ((t * (u * (255 - u)) + (1 << 23)) >> 24));
  if (A) {
    uint32_t x = seed + (idx + 1u) * 0x9E3779B9u;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    const int z = (int)((x & 255u) + ((x >> 8) & 255u) + ((x >> 16) & 255u) + (x >> 24)) - 510;
    v = pho_clamp(v + ((A * z + 32768) >> 16));
  }
  return (uint32_t)v;
}

// one unit bytewise: pixel `unit` (RGB) or byte `unit` of the window
template <bool RGB>
__device__ __forceinline__ void pho_unit(const uint8_t* in, uint8_t* out, const int32_t* R, uint32_t unit) {
  const int t = R[12], A = R[13];
  const uint32_t seed = (uint32_t)R[14];
  if (RGB) {
    const uint32_t o = unit * 3u;
    const int p0 = in[o], p1 = in[o + 1], p2 = in[o + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int u = pho_clamp((R[3 * c] * p0 + R[3 * c + 1] * p1 + R[3 * c + 2] * p2 + R[9 + c] + 32768) >> 16);
      out[o + c] = (uint8_t)pho_finish(u, t, A, seed, o + c);
    }
  } else {
    const int u = pho_clamp((R[0] * (int)in[unit] + R[9] + 32768) >> 16);
    out[unit] = (uint8_t)pho_finish(u, t, A, seed, unit);
  }
}

template <bool RGB>
__global__ __launch_bounds__(256) void window_photometric(PhotoArgs a) {
  const int n = blockIdx.y, tid = threadIdx.x;
  const int32_t* R = a.row[n];
  if (R[15]) return;
  constexpr uint32_t U = RGB ? 3 : 1;          // bytes per unit
  const uint32_t WB = a.wbytes, units = WB / U;
  const uint8_t* in = a.in + (size_t)n * WB;
  uint8_t* out = a.out + (size_t)n * WB;       // both bases are 4-byte aligned: in and out share their byte phase
  const uint32_t mis = (uint32_t)((uintptr_t)in & 3);
  const uint32_t head = min(RGB ? mis : ((4u - mis) & 3u), units);
  const uint32_t runs = (units - head) / 4u, tail = units - head - 4u * runs;
  const int t = R[12], A = R[13];
  const uint32_t seed = (uint32_t)R[14];
  for (uint32_t g = blockIdx.x * 256u + tid; g < runs; g += gridDim.x * 256u) {
    const uint32_t o = (head + 4u * g) * U;    // a multiple of 4 past the window's first dword boundary; o + 4 U <= WB
    const uint32_t* src = reinterpret_cast<const uint32_t*>(in + o);
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + o);
    if (RGB) {
      const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
      uint32_t r[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {            // pixel k: bytes 3 k .. 3 k + 2 of the twelve
        int p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int q = 3 * k + c;
          p[c] = (int)(((q < 4 ? w0 : q < 8 ? w1 : w2) >> (8 * (q & 3))) & 255u);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int q = 3 * k + c;
          const int u = pho_clamp((R[3 * c] * p[0] + R[3 * c + 1] * p[1] + R[3 * c + 2] * p[2] + R[9 + c] + 32768) >> 16);
          r[q >> 2] |= pho_finish(u, t, A, seed, o + q) << (8 * (q & 3));
        }
      }
      dst[0] = r[0]; dst[1] = r[1]; dst[2] = r[2];
    } else {
      const uint32_t w = src[0];
      uint32_t r = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int u = pho_clamp((R[0] * (int)((w >> (8 * q)) & 255u) + R[9] + 32768) >> 16);
        r |= pho_finish(u, t, A, seed, o + q) << (8 * q);
      }
      dst[0] = r;
    }
  }
  if (blockIdx.x == 0) {                       // the ragged ends: at most three units each
    if ((uint32_t)tid < head) pho_unit<RGB>(in, out, R, tid);
    else if (tid >= 64 && (uint32_t)(tid - 64) < tail) pho_unit<RGB>(in, out, R, head + 4u * runs + (tid - 64));
  }
}

bool pho_identity(const int32_t* r) {
  for (int q = 0; q < 15; ++q)
    if (r[q] != (q == 0 || q == 4 || q == 8 ? 65536 : 0) && q != 14) return false;
  return true;
}

}  // namespace

extern "C" int rua_window_photometric(const uint8_t* img_in, uint8_t* img_out, int N, int PH, int PW, int Cin, const int32_t* photo,
                                      void* stream) {
  RUA_CHECK_ARG(img_in && img_out && photo, "rua_window_photometric: img_in, img_out and photo are required");
  RUA_CHECK_ARG(N >= 1, "rua_window_photometric: N %d (>= 1)", N);
  RUA_CHECK_ARG(Cin >= 1 && Cin <= PHO_MAXC, "rua_window_photometric: Cin %d outside 1..16", Cin);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= PHO_MAXP && PW <= PHO_MAXP, "rua_window_photometric: PH %d, PW %d (1 <= PH, PW <= 512)", PH, PW);
  const int64_t wbytes = (int64_t)PH * PW * Cin, total = wbytes * N;
  RUA_CHECK_ARG(total < ((int64_t)1 << 31), "rua_window_photometric: N*PH*PW*Cin is %lld (must stay below 2^31)", (long long)total);
  RUA_CHECK_ARG(((uintptr_t)img_in & 3) == 0 && ((uintptr_t)img_out & 3) == 0, "rua_window_photometric: img_in and img_out must be 4-byte aligned");
  const uintptr_t pi = (uintptr_t)img_in, po = (uintptr_t)img_out;
  RUA_CHECK_ARG(pi == po || (pi < po ? po - pi : pi - po) >= (uintptr_t)total,
                "rua_window_photometric: img_in and img_out overlap in part (in place is the same pointer; otherwise their %lld bytes lie apart)", (long long)total);
  for (int k = 0; k < N; ++k) {
    const int32_t* r = photo + 16 * (size_t)k;
    for (int q = 0; q < 9; ++q)
      RUA_CHECK_ARG(r[q] >= -PHO_MAXM && r[q] <= PHO_MAXM,
                    "rua_window_photometric: row %d: word %d: matrix entry %d outside -1048576..1048576 (16 in Q16)", k, q, r[q]);
    for (int q = 9; q < 12; ++q)
      RUA_CHECK_ARG(r[q] >= -PHO_MAXB && r[q] <= PHO_MAXB,
                    "rua_window_photometric: row %d: word %d: offset %d outside -536870912..536870912 (8192 levels in Q16)", k, q, r[q]);
    RUA_CHECK_ARG(r[12] >= -PHO_MAXT && r[12] <= PHO_MAXT, "rua_window_photometric: row %d: word 12: tone %d outside -65536..65536 (1 in Q16)", k, r[12]);
    RUA_CHECK_ARG(r[13] >= 0 && r[13] <= PHO_MAXA, "rua_window_photometric: row %d: word 13: noise amplitude %d outside 0..65536", k, r[13]);
    RUA_CHECK_ARG(r[15] == 0, "rua_window_photometric: row %d: word 15: reserved, must be 0, got %d", k, r[15]);
    if (Cin != 3) {
      static const int like[12] = {0, -1, -1, -1, 0, -1, -1, -1, 0, 9, 9, 9};       // the word each must equal; -1: zero
      for (int q = 0; q < 12; ++q)
        RUA_CHECK_ARG(r[q] == (like[q] < 0 ? 0 : r[like[q]]),
                      "rua_window_photometric: row %d: word %d: %d, but Cin %d != 3 takes scalar rows (off-diagonals 0, one gain, one offset)", k, q, r[q], Cin);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const bool in_place = img_in == img_out;
  const uint32_t runs = (uint32_t)(wbytes / (Cin == 3 ? 12 : 4));
  const uint32_t per_block = 256u * PHO_RUNS;
  uint32_t gx = (runs + per_block - 1) / per_block;
  gx = gx < 1 ? 1 : gx > 1024 ? 1024 : gx;
  PhotoArgs a;
  memset(&a, 0, sizeof(a));
  a.wbytes = (uint32_t)wbytes;
  for (int k0 = 0; k0 < N; k0 += PHO_CHUNK) {
    const int nk = N - k0 < PHO_CHUNK ? N - k0 : PHO_CHUNK;
    int work = 0;
    for (int k = 0; k < nk; ++k) {
      const int32_t* r = photo + 16 * (size_t)(k0 + k);
      memcpy(a.row[k], r, 64);
      a.row[k][15] = in_place && pho_identity(r);             // an identity row in place: nothing to do; out of place it copies
      work += !a.row[k][15];
    }
    if (!work) continue;
    a.in = img_in + (size_t)k0 * wbytes;
    a.out = img_out + (size_t)k0 * wbytes;
    if (Cin == 3) hipLaunchKernelGGL(window_photometric<true>, dim3(gx, nk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(window_photometric<false>, dim3(gx, nk), dim3(256), 0, st, a);
    RUA_LAUNCH_CHECK("rua_window_photometric");
  }
  return RUA_OK;
}

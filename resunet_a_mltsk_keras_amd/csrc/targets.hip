// Multitask training targets from uint8 patches and uint8 class maps (rua_multitask_targets, include/rua_hip.h).
//
// Every output equals the host definition in labels.py bit for bit:
//   x      float32(u8) / 255 (norm_type 1) or / 126.5 (norm_type 2), correctly rounded f32 division
//   seg    onehot(cls): an all-zero row for a class value >= C
//   bound  get_boundary_label(seg): Canny(0, 1) of every class mask + 3x3 cross dilation.  Sobel dx and dy of a 0/1 mask are
//          congruent mod 2, so every non-maximum-suppression survivor has |dx|+|dy| >= 2 > high: hysteresis keeps them all and the
//          target is a local 7x7 stencil (tests/test_targets_host.py pins this against labels.canny_u8)
//   dist   get_distance_label(seg): the classes partition the pixels, so dist[p, c] is nonzero only for c = cls(p) and equals
//          d(p) / max{d(q) : cls(q) = c}, d = Euclidean distance to the nearest in-image pixel of another class value
//   color  color_label(rgb, norm_type): OpenCV's 8-bit RGB->HSV fixed point, then the normalisation
// Four launches: column distances -> row distances (+ per-(sample, class) max) -> per-pixel pass -> boundary tiles.
#include "common.h"

namespace {

constexpr int TGT_MAXHW = 512;
constexpr int TGT_INFG = 1023;            // "no other class in this column" (real column distances are <= 512)
constexpr int TGT_BIG = 1 << 28;          // its square; + 511^2 still fits an int

// The column distances and then the distances live in the first N*H*W words of `bound` (an int, then a float's bits, per pixel):
// the boundary pass, the last launch, overwrites it.

// ---- pass 1: per pixel the distance along its column to the nearest pixel of another class value (searched outwards in LDS;
// TGT_INFG if the whole column is one class).  A block: 32 columns x 32 rows of output, with the columns' whole height in LDS.
constexpr int CS = 32, CR = 32;
__global__ __launch_bounds__(256) void tgt_columns(const uint8_t* __restrict__ cls, int H, int W, uint32_t* __restrict__ mid,
                                                   uint32_t* __restrict__ cmax, int NC) {
  __shared__ uint8_t T[TGT_MAXHW * CS];
  const int tid = threadIdx.x, j0 = blockIdx.x * CS, i0 = blockIdx.y * CR, n = blockIdx.z;
  const int flat = ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 256 + tid;   // >= N * 256 >= N * C threads
  if (flat < NC) cmax[flat] = 0u;
  const uint8_t* src = cls + (size_t)n * H * W;
  if ((W & 3) == 0) {
    for (int e = tid; e < H * (CS / 4); e += 256) {
      const int i = e / (CS / 4), q = e % (CS / 4), j = j0 + 4 * q;
      *reinterpret_cast<uint32_t*>(&T[i * CS + 4 * q]) = j < W ? *reinterpret_cast<const uint32_t*>(src + (size_t)i * W + j) : 0u;
    }
  } else {
    for (int e = tid; e < H * CS; e += 256) {
      const int i = e / CS, l = e % CS;
      T[e] = j0 + l < W ? src[(size_t)i * W + j0 + l] : 0;
    }
  }
  __syncthreads();
  const int l = tid % CS, j = j0 + l;
  if (j >= W) return;
  for (int i = i0 + tid / CS; i < min(i0 + CR, H); i += 256 / CS) {
    const int c = T[i * CS + l];
    int g = TGT_INFG;
    const int reach = max(i, H - 1 - i);
    for (int t = 1; t <= reach; ++t) {
      if ((i - t >= 0 && T[(i - t) * CS + l] != c) || (i + t < H && T[(i + t) * CS + l] != c)) { g = t; break; }
    }
    mid[((size_t)n * H + i) * W + j] = (uint32_t)g;
  }
}

// ---- pass 2: per (sample, row) the exact squared distance, min over columns k of (j-k)^2 + g_c(k)^2 where g_c(k) is the column
// distance if pixel (i, k) has the same class as (i, j), else 0.  Searched outwards from j, stopping once (j-k)^2 reaches the best
// so far (O(W) per pixel at worst).  d = float(sqrt(double(d2))) is scipy's float64 distance cast to float32.  The per-(sample,
// class) maximum goes through an LDS max per row and one integer atomicMax on the float's bits (d >= 0): exact, order-independent.
__global__ __launch_bounds__(256) void tgt_rows(const uint8_t* __restrict__ cls, int H, int W, int C, uint32_t* __restrict__ mid,
                                               uint32_t* __restrict__ cmax) {
  __shared__ uint32_t R[TGT_MAXHW];       // column distance << 8 | class
  __shared__ uint32_t bmax[64];
  const int tid = threadIdx.x, i = blockIdx.x, n = blockIdx.y;
  const size_t row = ((size_t)n * H + i) * W;
  if (tid < 64) bmax[tid] = 0u;
  for (int k = tid; k < W; k += 256) R[k] = (mid[row + k] << 8) | cls[row + k];
  __syncthreads();
  for (int j = tid; j < W; j += 256) {
    const int c = R[j] & 255;
    float d = 0.f;
    if (c < C) {
      int best = TGT_BIG;
      const int reach = j > W - 1 - j ? j : W - 1 - j;
      for (int t = 0; t <= reach; ++t) {
        const int tt = t * t;
        if (tt >= best) break;
        if (j - t >= 0) {
          const uint32_t w = R[j - t];
          const int g = (int)(w >> 8);
          const int v = (int)(w & 255) == c ? (g == TGT_INFG ? TGT_BIG : g * g) : 0;
          best = min(best, tt + v);
        }
        if (t > 0 && j + t < W) {
          const uint32_t w = R[j + t];
          const int g = (int)(w >> 8);
          const int v = (int)(w & 255) == c ? (g == TGT_INFG ? TGT_BIG : g * g) : 0;
          best = min(best, tt + v);
        }
      }
      if (best < TGT_BIG) {               // else the class fills the patch: zeros
        d = (float)sqrt((double)best);
        atomicMax(&bmax[c], __float_as_uint(d));
      }
    }
    mid[row + j] = __float_as_uint(d);
  }
  __syncthreads();
  if (tid < C && bmax[tid] != 0u) atomicMax(&cmax[n * C + tid], bmax[tid]);
}

// ---- pass 3: x, seg, dist (normalised) and color of 1024 consecutive pixels per block.  x comes straight from the image words;
// the pixels' class, distance value and colour go through LDS so that every store instruction of a wave writes one contiguous
// run of 16-byte pieces (a block's outputs are contiguous: NHWC). ------------------------------------------------------------
constexpr int PB = 1024;
__device__ __forceinline__ int rdiv(int a, int b) {      // np.rint(a / b) for a, b > 0 (half to even)
  const int q = a / b, r = a - q * b;
  return 2 * r > b ? q + 1 : (2 * r == b ? q + (q & 1) : q);
}
__device__ __forceinline__ void hsv_u8(int r, int g, int b, int& h, int& s, int& v) {   // labels.rgb_to_hsv_u8
  v = max(max(r, g), b);
  const int diff = v - min(min(r, g), b);
  s = v ? (diff * rdiv(255 << 12, v) + (1 << 11)) >> 12 : 0;
  int hh = v == r ? g - b : (v == g ? (b - r) + 2 * diff : (r - g) + 4 * diff);
  hh = diff ? (hh * rdiv(180 << 12, 6 * diff) + (1 << 11)) >> 12 : 0;
  h = hh < 0 ? hh + 180 : hh;
}
__device__ __forceinline__ void st4(float* p, float a, float b, float c, float d) {
  stg16(p, make_uint4(__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d)));
}

struct PixArgs {
  const uint8_t* img; const uint8_t* cls; const uint32_t* mid; const uint32_t* cmax; int NP, HW, Cin, C; float xdiv, hdiv, sdiv;
  float* x; float* seg; float* dist; float* color;
};

// MODE 0: x only; 1: x + seg; 2: x, seg, dist, color
template <int MODE>
__global__ __launch_bounds__(256) void tgt_pixels(PixArgs a) {
  __shared__ uint8_t scl[PB];
  __shared__ float sdv[MODE == 2 ? PB : 1];
  __shared__ float shsv[MODE == 2 ? 3 * PB : 1];
  const int tid = threadIdx.x, base = blockIdx.x * PB, np = min(PB, a.NP - base);
  {
    const int ne = np * a.Cin;
    const uint8_t* ib = a.img + (size_t)base * a.Cin;
    const uint32_t* iw = reinterpret_cast<const uint32_t*>(ib);
    float* xo = a.x + (size_t)base * a.Cin;
    for (int k = tid; k < ne / 4; k += 256) {
      const uint32_t w = iw[k];
      st4(xo + 4 * k, (float)(w & 255) / a.xdiv, (float)((w >> 8) & 255) / a.xdiv, (float)((w >> 16) & 255) / a.xdiv, (float)(w >> 24) / a.xdiv);
    }
    for (int e = (ne & ~3) + tid; e < ne; e += 256) xo[e] = (float)ib[e] / a.xdiv;
  }
  if (MODE == 0) return;
  for (int p = tid; p < np; p += 256) {
    const int gp = base + p, cl = a.cls[gp];
    scl[p] = (uint8_t)cl;
    if (MODE == 2) {
      float dv = 0.f;
      if (cl < a.C) {
        const uint32_t m = a.cmax[(gp / a.HW) * a.C + cl];
        if (m) dv = __uint_as_float(a.mid[gp]) / __uint_as_float(m);
      }
      sdv[p] = dv;
      int h, s, v;
      hsv_u8(a.img[3 * (size_t)gp], a.img[3 * (size_t)gp + 1], a.img[3 * (size_t)gp + 2], h, s, v);
      shsv[3 * p] = (float)h / a.hdiv; shsv[3 * p + 1] = (float)s / a.sdiv; shsv[3 * p + 2] = (float)v / a.xdiv;
    }
  }
  __syncthreads();
  const int C = a.C, ne = np * C;
  float* so = a.seg + (size_t)base * C;
  float* dout = MODE == 2 ? a.dist + (size_t)base * C : nullptr;
  for (int k = tid; k < ne / 4; k += 256) {
    int px = (4 * k) / C, c = 4 * k - px * C;
    float sv[4], dv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool on = scl[px] == c;
      sv[q] = on ? 1.f : 0.f;
      if (MODE == 2) dv[q] = on ? sdv[px] : 0.f;
      if (++c == C) { c = 0; ++px; }
    }
    st4(so + 4 * k, sv[0], sv[1], sv[2], sv[3]);
    if (MODE == 2) st4(dout + 4 * k, dv[0], dv[1], dv[2], dv[3]);
  }
  for (int e = (ne & ~3) + tid; e < ne; e += 256) {
    const int px = e / C, c = e - px * C;
    so[e] = scl[px] == c ? 1.f : 0.f;
    if (MODE == 2) dout[e] = scl[px] == c ? sdv[px] : 0.f;
  }
  if (MODE == 2) {
    const int nc = np * 3;
    float* co = a.color + (size_t)base * 3;
    for (int k = tid; k < nc / 4; k += 256) st4(co + 4 * k, shsv[4 * k], shsv[4 * k + 1], shsv[4 * k + 2], shsv[4 * k + 3]);
    for (int e = (nc & ~3) + tid; e < nc; e += 256) co[e] = shsv[e];
  }
}

// ---- pass 4: boundary tiles.  A 16 x 64 output tile with the class map around it (3-pixel halo, replicated borders) in LDS; for
// every class value below C present in that window: the mask's Sobel magnitude and direction on the 2-pixel halo (zero outside the
// image), the NMS survivors on the 1-pixel halo (none outside the image), their cross dilation on the tile.  A window of a single
// class value has no edges.  The tile's C bits per pixel leave as coalesced rows of floats. --------------------------------
constexpr int BTH = 16, BTW = 64;
constexpr int BH3 = BTH + 6, BW3 = BTW + 6, BH2 = BTH + 4, BW2 = BTW + 4, BH1 = BTH + 2, BW1 = BTW + 2;
__global__ __launch_bounds__(256) void tgt_bound(const uint8_t* __restrict__ cls, int H, int W, int C, float* __restrict__ bound) {
  __shared__ uint8_t T[BH3 * BW3];
  __shared__ uint8_t M[BH2 * BW2];       // |dx| + |dy| (0..8) | direction << 4
  __shared__ uint8_t E[BH1 * BW1];
  __shared__ unsigned long long bits[BTH * BTW];
  __shared__ unsigned long long present;
  __shared__ int mixed;
  const int tid = threadIdx.x, j0 = blockIdx.x * BTW, i0 = blockIdx.y * BTH, n = blockIdx.z;
  const uint8_t* src = cls + (size_t)n * H * W;
  if (tid == 0) { present = 0ull; mixed = 0; }
  __syncthreads();
  const int first = src[(size_t)min(max(i0 - 3, 0), H - 1) * W + min(max(j0 - 3, 0), W - 1)];
  unsigned long long mine = 0ull;
  int diff = 0;
  for (int e = tid; e < BH3 * BW3; e += 256) {
    const int r = e / BW3, q = e % BW3;
    const int gi = min(max(i0 - 3 + r, 0), H - 1), gj = min(max(j0 - 3 + q, 0), W - 1);
    const int v = src[(size_t)gi * W + gj];
    T[e] = (uint8_t)v;
    if (v < C) mine |= 1ull << v;
    diff |= v != first;
  }
  if (mine) atomicOr(&present, mine);
  if (diff) atomicOr(&mixed, 1);
  unsigned long long b0 = 0ull, b1 = 0ull, b2 = 0ull, b3 = 0ull;     // output pixels tid + 256 m
  __syncthreads();
  unsigned long long todo = mixed ? present : 0ull;
  while (todo) {
    const int c = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    for (int e = tid; e < BH2 * BW2; e += 256) {
      const int r = e / BW2, q = e % BW2, gi = i0 - 2 + r, gj = j0 - 2 + q;
      int val = 0;
      if (gi >= 0 && gi < H && gj >= 0 && gj < W) {
        const uint8_t* t = &T[(r + 1) * BW3 + q + 1];        // the window centre in T
        const int a00 = t[-BW3 - 1] == c, a01 = t[-BW3] == c, a02 = t[-BW3 + 1] == c;
        const int a10 = t[-1] == c, a12 = t[1] == c;
        const int a20 = t[BW3 - 1] == c, a21 = t[BW3] == c, a22 = t[BW3 + 1] == c;
        const int dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
        const int dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
        const int ax = abs(dx), ay = abs(dy) << 15, tg22 = ax * 13573, tg67 = tg22 + (ax << 16);
        const int dir = ay < tg22 ? 0 : ay > tg67 ? 1 : ((dx ^ dy) < 0 ? 3 : 2);
        val = (abs(dx) + abs(dy)) | (dir << 4);
      }
      M[e] = (uint8_t)val;
    }
    __syncthreads();
    for (int e = tid; e < BH1 * BW1; e += 256) {
      const int r = e / BW1, q = e % BW1;
      const uint8_t* mp = &M[(r + 1) * BW2 + q + 1];
      const int m = mp[0] & 15, dir = mp[0] >> 4;
      int edge = 0;
      if (m) {                         // outside the image M is 0: no edge there
        if (dir == 0) edge = m > (mp[-1] & 15) && m >= (mp[1] & 15);
        else if (dir == 1) edge = m > (mp[-BW2] & 15) && m >= (mp[BW2] & 15);
        else if (dir == 2) edge = m > (mp[-BW2 - 1] & 15) && m > (mp[BW2 + 1] & 15);
        else edge = m > (mp[-BW2 + 1] & 15) && m > (mp[BW2 - 1] & 15);
      }
      E[e] = (uint8_t)edge;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = tid + 256 * m, r = k / BTW, q = k % BTW;
      const uint8_t* ep = &E[(r + 1) * BW1 + q + 1];
      const unsigned long long b = (unsigned long long)(ep[0] | ep[-1] | ep[1] | ep[-BW1] | ep[BW1]) << c;
      if (m == 0) b0 |= b; else if (m == 1) b1 |= b; else if (m == 2) b2 |= b; else b3 |= b;
    }
  }
  bits[tid] = b0; bits[tid + 256] = b1; bits[tid + 512] = b2; bits[tid + 768] = b3;
  __syncthreads();
  // a tile row is tw * C contiguous floats; element e is pixel e / C (as (e * ceil(2^20 / C)) >> 20: exact for e < 4096, C <= 64)
  const int th = min(BTH, H - i0), tw = min(BTW, W - j0), rowf = tw * C;
  const uint32_t m20 = ((1u << 20) + C - 1) / C;
  for (int r = 0; r < th; ++r) {
    float* out = bound + (((size_t)n * H + i0 + r) * W + j0) * C;
    const unsigned long long* br = &bits[r * BTW];
    for (int e = tid; e < rowf; e += 256) {
      const int px = (int)(((uint32_t)e * m20) >> 20), c = e - px * C;
      out[e] = (br[px] >> c) & 1ull ? 1.f : 0.f;
    }
  }
}

// ---- void mask: square dilation (radius mg) of cls >= C inside each patch.  A 32 x 64 output tile with the flags of its halo in LDS (zero outside
// the patch), ORed along the rows, then along the columns; a thread finishes four neighbouring pixels and stores them as one dword where the address
// allows it (the mask has no alignment of its own: a row of odd width starts anywhere), byte by byte at ragged ends. ------------------------------
constexpr int VTH = 32, VTW = 64, VMG = 16;
__global__ __launch_bounds__(256) void void_mask_kernel(const uint8_t* __restrict__ cls, int H, int W, int C, int mg, uint8_t* __restrict__ mask) {
  __shared__ uint8_t F[(VTH + 2 * VMG) * (VTW + 2 * VMG)];
  __shared__ uint8_t R[(VTH + 2 * VMG) * VTW];
  const int tid = threadIdx.x, j0 = blockIdx.x * VTW, i0 = blockIdx.y * VTH, n = blockIdx.z;
  const int fh = VTH + 2 * mg, fw = VTW + 2 * mg;
  const uint8_t* src = cls + (size_t)n * H * W;
  for (int e = tid; e < fh * fw; e += 256) {
    const int r = e / fw, q = e - r * fw, gi = i0 - mg + r, gj = j0 - mg + q;
    F[e] = (gi >= 0 && gi < H && gj >= 0 && gj < W && src[(size_t)gi * W + gj] >= C) ? 1 : 0;
  }
  __syncthreads();
  for (int e = tid; e < fh * VTW; e += 256) {
    const int r = e / VTW, q = e % VTW;
    int v = 0;
    for (int t = 0; t <= 2 * mg; ++t) v |= F[r * fw + q + t];
    R[e] = (uint8_t)v;
  }
  __syncthreads();
  for (int e = tid; e < VTH * (VTW / 4); e += 256) {
    const int r = e / (VTW / 4), q4 = (e % (VTW / 4)) * 4, i = i0 + r, j = j0 + q4;
    if (i >= H || j >= W) continue;
    uint32_t word = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int v = 0;
      for (int t = 0; t <= 2 * mg; ++t) v |= R[(r + t) * VTW + q4 + k];
      word |= (v ? 255u : 0u) << (8 * k);
    }
    uint8_t* out = mask + (size_t)n * H * W + (size_t)i * W + j;
    if (j + 3 < W && ((uintptr_t)out & 3) == 0) {
      *reinterpret_cast<uint32_t*>(out) = word;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (j + k < W) out[k] = (uint8_t)(word >> (8 * k));
    }
  }
}

}  // namespace

extern "C" int rua_void_mask(const uint8_t* cls, int N, int H, int W, int num_classes, int margin, uint8_t* mask, void* stream) {
  RUA_CHECK_ARG(cls && mask, "rua_void_mask: cls and mask are required");
  RUA_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= TGT_MAXHW && W <= TGT_MAXHW, "rua_void_mask: N %d, H %d, W %d (1 <= N <= 65535, 1 <= H, W <= 512)", N, H, W);
  RUA_CHECK_ARG(num_classes >= 1 && num_classes <= 255, "rua_void_mask: num_classes %d outside 1..255", num_classes);
  RUA_CHECK_ARG(margin >= 0 && margin <= VMG, "rua_void_mask: margin %d outside 0..%d", margin, VMG);
  RUA_CHECK_ARG((int64_t)N * H * W < ((int64_t)1 << 31), "rua_void_mask: N*H*W must stay below 2^31");
  hipLaunchKernelGGL(void_mask_kernel, dim3((W + VTW - 1) / VTW, (H + VTH - 1) / VTH, N), dim3(256), 0, (hipStream_t)stream, cls, H, W, num_classes, margin, mask);
  RUA_LAUNCH_CHECK("rua_void_mask");
  return RUA_OK;
}

extern "C" int64_t rua_targets_scratch_bytes(int N, int num_classes) {
  return N > 0 && num_classes > 0 ? (int64_t)N * num_classes * 4 : 0;
}

extern "C" int rua_multitask_targets(const uint8_t* img, const uint8_t* cls, int N, int H, int W, int Cin, int num_classes, int norm_type,
                                     float* x, float* seg, float* bound, float* dist, float* color, void* scratch, int64_t scratch_bytes,
                                     void* stream) {
  const int C = num_classes;
  const bool mt = bound || dist || color;
  RUA_CHECK_ARG(img && x, "rua_multitask_targets: img and x are required");
  RUA_CHECK_ARG(!cls == !seg, "rua_multitask_targets: cls and seg go together");
  RUA_CHECK_ARG(!mt || (bound && dist && color && cls), "rua_multitask_targets: bound, dist and color are all given (with cls) or all null");
  RUA_CHECK_ARG(norm_type == 1 || norm_type == 2, "rua_multitask_targets: norm_type %d (1: /255, 2: /126.5)", norm_type);
  RUA_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && H <= TGT_MAXHW && W <= TGT_MAXHW, "rua_multitask_targets: N %d, H %d, W %d (1 <= H, W <= 512)", N, H, W);
  RUA_CHECK_ARG(C >= 1 && C <= 64, "rua_multitask_targets: num_classes %d outside 1..64", C);
  RUA_CHECK_ARG(Cin >= 1 && Cin <= 16, "rua_multitask_targets: Cin %d outside 1..16", Cin);
  RUA_CHECK_ARG(!color || Cin == 3, "rua_multitask_targets: color needs Cin = 3 (got %d)", Cin);
  const int64_t NP = (int64_t)N * H * W;
  const int64_t widest = C > Cin ? (C > 4 ? C : 4) : (Cin > 4 ? Cin : 4);
  RUA_CHECK_ARG(NP * widest < ((int64_t)1 << 31), "rua_multitask_targets: N*H*W*max(C, Cin, 4) must stay below 2^31");
  RUA_CHECK_ARG(((uintptr_t)img & 3) == 0 && ((uintptr_t)cls & 3) == 0, "rua_multitask_targets: img and cls must be 4-byte aligned");
  RUA_CHECK_ARG((((uintptr_t)x | (uintptr_t)seg | (uintptr_t)bound | (uintptr_t)dist | (uintptr_t)color) & 15) == 0,
                "rua_multitask_targets: x, seg, bound, dist and color must be 16-byte aligned");
  RUA_CHECK_ARG(!dist || (scratch && ((uintptr_t)scratch & 3) == 0 && scratch_bytes >= rua_targets_scratch_bytes(N, C)),
                "rua_multitask_targets: scratch needs %lld bytes, 4-byte aligned (got %lld)", (long long)rua_targets_scratch_bytes(N, C),
                (long long)scratch_bytes);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* cmax = (uint32_t*)scratch;
  uint32_t* mid = (uint32_t*)bound;                   // N*H*W words of intermediate; the boundary pass overwrites them
  if (mt) {
    hipLaunchKernelGGL(tgt_columns, dim3((W + CS - 1) / CS, (H + CR - 1) / CR, N), dim3(256), 0, st, cls, H, W, mid, cmax, N * C);
    RUA_LAUNCH_CHECK("rua_multitask_targets (columns)");
    hipLaunchKernelGGL(tgt_rows, dim3(H, N), dim3(256), 0, st, cls, H, W, C, mid, cmax);
    RUA_LAUNCH_CHECK("rua_multitask_targets (rows)");
  }
  PixArgs a;
  a.img = img; a.cls = cls; a.NP = (int)NP; a.HW = H * W; a.Cin = Cin; a.C = C;
  a.xdiv = norm_type == 1 ? 255.f : 126.5f;           // the reference's `img /= 127.5 - 1.` (test_ISPRS.py normalize_rgb)
  a.hdiv = norm_type == 1 ? 179.f : 88.5f;            // labels.color_label / normalize_hsv, precedence quirk included
  a.sdiv = a.xdiv;
  a.x = x; a.seg = seg; a.dist = dist; a.color = color; a.cmax = cmax; a.mid = mid;
  const unsigned blocks = (unsigned)((NP + PB - 1) / PB);
  if (mt) hipLaunchKernelGGL(tgt_pixels<2>, dim3(blocks), dim3(256), 0, st, a);
  else if (cls) hipLaunchKernelGGL(tgt_pixels<1>, dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(tgt_pixels<0>, dim3(blocks), dim3(256), 0, st, a);
  RUA_LAUNCH_CHECK("rua_multitask_targets (pixels)");
  if (mt) {
    hipLaunchKernelGGL(tgt_bound, dim3((W + BTW - 1) / BTW, (H + BTH - 1) / BTH, N), dim3(256), 0, st, cls, H, W, C, bound);
    RUA_LAUNCH_CHECK("rua_multitask_targets (bound)");
  }
  return RUA_OK;
}

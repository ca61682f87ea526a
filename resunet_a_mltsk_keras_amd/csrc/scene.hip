// Training windows cut out of resident scenes and augmented on the way (rua_scene_windows, include/rua_hip.h): the uint8 image
// [N][PH][PW][Cin] and class map [N][PH][PW] that rua_multitask_targets reads, written from uint8 scenes [H][W][Cin] / [H][W]
// and a table of (scene, row, col, code) rows.  code is one of the eight symmetries of the square (scenes.py, host_windows):
//   0 w   1 rot90   2 rot180   3 flip rows   4 flip columns   5 rot270   6 transpose   7 anti-transpose
// Every code is "transpose or not, then flip rows and / or columns":  out[i][j] = w[fr ? n-1-a : a][fc ? m-1-b : b] with
// (a, b) = (i, j), or (j, i) for the transposing codes 1, 5, 6, 7.
//
// A block moves one 32 x 32-pixel tile of one plane (image or class map) of one window.  The source tile is read ALONG SOURCE
// ROWS into LDS - aligned dwords where a whole one lies inside the row, single bytes at its ragged ends, so a window row may
// start at any byte - and leaves ALONG DESTINATION ROWS in 16-byte pieces (4-byte pieces or bytes where PW * Cin does not
// allow more).  The transposition happens between the two, in the LDS read: both global sides stay row-contiguous for every
// code.  An LDS row keeps the byte phase of its global row (no shifting on the way in) and the row pitch is an odd number of
// dwords, so the 32 LDS rows a transposed read walks through start in 32 different banks.
//
// The host resolves and checks every table row; the kernel receives, per window, the address of its first pixel in either
// plane, the scene width and the code - as kernel arguments, up to SW_CHUNK windows per launch.
#include "common.h"

namespace {

constexpr int SW_T = 32;                       // tile edge in pixels
constexpr int SW_MAXPIX = 16;                  // bytes per pixel
constexpr int SW_LPD = 133;                    // LDS row pitch in dwords: >= (3 + 32 * 16 + 3) / 4 = 129, odd
constexpr int SW_CHUNK = 128;                  // windows per launch
constexpr int SW_MAXP = 512;

struct SceneWin { const uint8_t* img; const uint8_t* cls; int W; int code; };
struct SceneArgs {
  SceneWin w[SW_CHUNK];
  uint8_t* img_out; uint8_t* cls_out;          // of the chunk's first window
  int PH, PW, Cin, img_unit, cls_unit, planes;
};
static_assert(sizeof(SceneArgs) <= 4096, "kernel arguments are limited to 4 KiB");

template <int U> struct StoreUnit;
template <> struct StoreUnit<16> { static __device__ __forceinline__ void st(uint8_t* p, const uint32_t* v) { stg16(p, make_uint4(v[0], v[1], v[2], v[3])); } };
template <> struct StoreUnit<4> { static __device__ __forceinline__ void st(uint8_t* p, const uint32_t* v) { *reinterpret_cast<uint32_t*>(p) = v[0]; } };
template <> struct StoreUnit<1> { static __device__ __forceinline__ void st(uint8_t* p, const uint32_t* v) { *p = (uint8_t)v[0]; } };

// the write side: unit e of the tile is U bytes of destination row i0 + e / upr, gathered byte by byte from the LDS tile
template <int U>
__device__ __forceinline__ void sw_write(const uint8_t* T, const int* phase, uint8_t* out, int PW, int cb, int i0, int j0, int th, int tw,
                                         bool tr, int ra, int rs, int ca, int cs, int tid) {
  const int upr = tw * cb / U, total = th * upr;
  for (int e = tid; e < total; e += 256) {
    const int ti = e / upr, v = e - ti * upr;
    uint32_t word[U >= 4 ? U / 4 : 1] = {};
    int tj = (v * U) / cb, ch = v * U - tj * cb;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      // LDS row / column of destination pixel (ti, tj): r = ra + rs * (tr ? tj : ti), c = ca + cs * (tr ? ti : tj)
      const int rr = ra + rs * (tr ? tj : ti), cc = ca + cs * (tr ? ti : tj);
      const uint32_t b = T[rr * (SW_LPD * 4) + phase[rr] + cc * cb + ch];
      word[k / 4] |= b << (8 * (k & 3));
      if (++ch == cb) { ch = 0; ++tj; }
    }
    StoreUnit<U>::st(out + ((size_t)(i0 + ti) * PW + j0) * cb + (size_t)v * U, word);
  }
}

__global__ __launch_bounds__(256) void scene_windows(SceneArgs a) {
  __shared__ uint32_t Td[SW_T * SW_LPD];
  __shared__ int phase[SW_T];
  uint8_t* T = reinterpret_cast<uint8_t*>(Td);
  const int tid = threadIdx.x, n = blockIdx.y, plane = blockIdx.z;
  const int PH = a.PH, PW = a.PW;
  const int tiles_x = (PW + SW_T - 1) / SW_T;
  const int i0 = (blockIdx.x / tiles_x) * SW_T, j0 = (blockIdx.x % tiles_x) * SW_T;
  const int th = min(SW_T, PH - i0), tw = min(SW_T, PW - j0);
  const SceneWin& w = a.w[n];
  const int cb = plane ? 1 : a.Cin, unit = plane ? a.cls_unit : a.img_unit;
  const uint8_t* src = plane ? w.cls : w.img;
  uint8_t* out = (plane ? a.cls_out : a.img_out) + (size_t)n * PH * PW * cb;
  const size_t pitch = (size_t)w.W * cb;
  const int code = w.code;
  const bool tr = code == 1 || code == 5 || code == 6 || code == 7;
  const bool fr = code == 2 || code == 3 || code == 5 || code == 7;     // source row runs against its destination index
  const bool fc = code == 1 || code == 2 || code == 4 || code == 7;     // source column likewise
  // source tile: sh rows x sw pixels at (r0, c0) of the window.  Transposing codes have PH == PW (checked on the host).
  const int a0 = tr ? j0 : i0, an = tr ? tw : th, A = tr ? PW : PH;     // destination index range the source ROW follows
  const int b0 = tr ? i0 : j0, bn = tr ? th : tw, Bn = tr ? PH : PW;    // ... the source COLUMN follows
  const int r0 = fr ? A - a0 - an : a0, c0 = fc ? Bn - b0 - bn : b0, sh = an, sw = bn;
  const int nb = sw * cb, ndmax = (nb + 6) / 4;
  const uint8_t* first = src + (size_t)r0 * pitch + (size_t)c0 * cb;
  for (int e = tid; e < sh * ndmax; e += 256) {
    const int rr = e / ndmax, q = e - rr * ndmax;
    const uint8_t* row = first + (size_t)rr * pitch;
    const int s = (int)((uintptr_t)row & 3);
    if (q == 0) phase[rr] = s;
    const int lo = max(4 * q, s), hi = min(4 * q + 4, s + nb);
    const uint8_t* al = row - s;                                        // the row's bytes sit at al + [s, s + nb)
    if (hi - lo == 4) Td[rr * SW_LPD + q] = *reinterpret_cast<const uint32_t*>(al + 4 * q);
    else for (int k = lo; k < hi; ++k) T[rr * (SW_LPD * 4) + k] = al[k];
  }
  __syncthreads();
  // LDS row / column of destination pixel (ti, tj) of the tile
  const int ra = fr ? an - 1 : 0, rs = fr ? -1 : 1, ca = fc ? bn - 1 : 0, cs = fc ? -1 : 1;
  if (unit == 16) sw_write<16>(T, phase, out, PW, cb, i0, j0, th, tw, tr, ra, rs, ca, cs, tid);
  else if (unit == 4) sw_write<4>(T, phase, out, PW, cb, i0, j0, th, tw, tr, ra, rs, ca, cs, tid);
  else sw_write<1>(T, phase, out, PW, cb, i0, j0, th, tw, tr, ra, rs, ca, cs, tid);
}

// widest store a plane's rows allow: every tile row starts a multiple of 32 * cb bytes into a row of PW * cb bytes
int store_unit(const void* out, int row_bytes) {
  const uintptr_t p = (uintptr_t)out;
  if ((p & 15) == 0 && row_bytes % 16 == 0) return 16;
  if ((p & 3) == 0 && row_bytes % 4 == 0) return 4;
  return 1;
}

}  // namespace

extern "C" int rua_scene_windows(const uint8_t* const* scene_img, const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w,
                                 int nscenes, const int32_t* windows, int N, int PH, int PW, int Cin,
                                 uint8_t* img_out, uint8_t* cls_out, void* stream) {
  RUA_CHECK_ARG(scene_img && scene_h && scene_w && windows && img_out, "rua_scene_windows: scene_img, scene_h, scene_w, windows and img_out are required");
  RUA_CHECK_ARG(!scene_cls == !cls_out, "rua_scene_windows: scene_cls and cls_out go together");
  RUA_CHECK_ARG(nscenes >= 1 && N >= 1, "rua_scene_windows: nscenes %d, N %d (both >= 1)", nscenes, N);
  RUA_CHECK_ARG(Cin >= 1 && Cin <= SW_MAXPIX, "rua_scene_windows: Cin %d outside 1..16", Cin);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= SW_MAXP && PW <= SW_MAXP, "rua_scene_windows: PH %d, PW %d (1 <= PH, PW <= 512)", PH, PW);
  RUA_CHECK_ARG(((uintptr_t)img_out & 3) == 0 && ((uintptr_t)cls_out & 3) == 0, "rua_scene_windows: img_out and cls_out must be 4-byte aligned");
  for (int s = 0; s < nscenes; ++s) {
    RUA_CHECK_ARG(scene_img[s] && (!scene_cls || scene_cls[s]), "rua_scene_windows: scene %d: null pointer", s);
    RUA_CHECK_ARG(scene_h[s] >= 1 && scene_w[s] >= 1 && (int64_t)scene_h[s] * scene_w[s] * Cin < ((int64_t)1 << 40),
                  "rua_scene_windows: scene %d: size %d x %d", s, scene_h[s], scene_w[s]);
  }
  for (int k = 0; k < N; ++k) {
    const int32_t* t = windows + 4 * (size_t)k;
    const int s = t[0], r = t[1], c = t[2], code = t[3];
    RUA_CHECK_ARG(s >= 0 && s < nscenes, "rua_scene_windows: row %d: scene %d outside 0..%d", k, s, nscenes - 1);
    RUA_CHECK_ARG(r >= 0 && c >= 0 && (int64_t)r + PH <= scene_h[s] && (int64_t)c + PW <= scene_w[s],
                  "rua_scene_windows: row %d: window (%d, %d) + %d x %d leaves its %d x %d scene", k, r, c, PH, PW, scene_h[s], scene_w[s]);
    RUA_CHECK_ARG(code >= 0 && code <= 7, "rua_scene_windows: row %d: code %d outside 0..7", k, code);
    RUA_CHECK_ARG(PH == PW || !(code == 1 || code >= 5), "rua_scene_windows: row %d: code %d transposes and needs a square patch (got %d x %d)",
                  k, code, PH, PW);
  }
  hipStream_t st = (hipStream_t)stream;
  const int tiles = ((PH + SW_T - 1) / SW_T) * ((PW + SW_T - 1) / SW_T);
  SceneArgs a;
  memset(&a, 0, sizeof(a));
  a.PH = PH; a.PW = PW; a.Cin = Cin; a.planes = cls_out ? 2 : 1;
  a.img_unit = store_unit(img_out, PW * Cin);
  a.cls_unit = store_unit(cls_out, PW);
  for (int k0 = 0; k0 < N; k0 += SW_CHUNK) {
    const int nk = N - k0 < SW_CHUNK ? N - k0 : SW_CHUNK;
    for (int k = 0; k < nk; ++k) {
      const int32_t* t = windows + 4 * (size_t)(k0 + k);
      const int s = t[0];
      const size_t px = (size_t)t[1] * scene_w[s] + t[2];
      a.w[k].img = scene_img[s] + px * Cin;
      a.w[k].cls = scene_cls ? scene_cls[s] + px : nullptr;
      a.w[k].W = scene_w[s];
      a.w[k].code = t[3];
    }
    a.img_out = img_out + (size_t)k0 * PH * PW * Cin;          // a window is a whole number of rows, a row a whole number of store units
    a.cls_out = cls_out ? cls_out + (size_t)k0 * PH * PW : nullptr;
    hipLaunchKernelGGL(scene_windows, dim3(tiles, nk, a.planes), dim3(256), 0, st, a);
    RUA_LAUNCH_CHECK("rua_scene_windows");
  }
  return RUA_OK;
}

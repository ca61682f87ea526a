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
#include <algorithm>
#include <vector>

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

// a symmetry code as "transpose or not, then flip": the source row (column) runs against its destination index under fr (fc)
struct Sym {
  int code;
  __device__ __forceinline__ bool tr() const { return code == 1 || code == 5 || code == 6 || code == 7; }
  __device__ __forceinline__ bool fr() const { return code == 2 || code == 3 || code == 5 || code == 7; }
  __device__ __forceinline__ bool fc() const { return code == 1 || code == 2 || code == 4 || code == 7; }
};

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
  const Sym y{w.code};
  const bool tr = y.tr(), fr = y.fr(), fc = y.fc();
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

// ---- the argument checks the entry points share: each speaks under the name `fn` of the entry point that called it ---------------
#define SC_TRY(call) do { const int rc_ = (call); if (rc_ != RUA_OK) return rc_; } while (0)

// scene s of a call: its pointers (ptrs: all that the call needs are there), and h * w * bpp bytes below 2^40
int check_scene(const char* fn, int s, bool ptrs, int h, int w, int bpp, bool say_bpp = false) {
  RUA_CHECK_ARG(ptrs, "%s: scene %d: null pointer", fn, s);
  if (h >= 1 && w >= 1 && (int64_t)h * w * bpp < ((int64_t)1 << 40)) return RUA_OK;
  if (say_bpp) rua_set_error("%s: scene %d: size %d x %d x %d", fn, s, h, w, bpp);
  else rua_set_error("%s: scene %d: size %d x %d", fn, s, h, w);
  return RUA_ERR_ARG;
}

// every scene of a call: `must` holds a pointer per scene, `may` is either absent or holds one per scene too
int check_scene_list(const char* fn, const uint8_t* const* must, const uint8_t* const* may, const int32_t* scene_h, const int32_t* scene_w,
                     int nscenes, int bpp, bool say_bpp = false) {
  for (int s = 0; s < nscenes; ++s) SC_TRY(check_scene(fn, s, must[s] && (!may || may[s]), scene_h[s], scene_w[s], bpp, say_bpp));
  return RUA_OK;
}

// table row k = (scene, row, col, code): the scene exists and the PH x PW window lies inside it ...
int check_row_place(const char* fn, int k, const int32_t* t, int PH, int PW, const int32_t* scene_h, const int32_t* scene_w, int nscenes) {
  const int s = t[0], r = t[1], c = t[2];
  RUA_CHECK_ARG(s >= 0 && s < nscenes, "%s: row %d: scene %d outside 0..%d", fn, k, s, nscenes - 1);
  RUA_CHECK_ARG(r >= 0 && c >= 0 && (int64_t)r + PH <= scene_h[s] && (int64_t)c + PW <= scene_w[s],
                "%s: row %d: window (%d, %d) + %d x %d leaves its %d x %d scene", fn, k, r, c, PH, PW, scene_h[s], scene_w[s]);
  return RUA_OK;
}

// ... and its code is one of the eight symmetries, a transposing one only on a square patch
int check_row_code(const char* fn, int k, int code, int PH, int PW) {
  RUA_CHECK_ARG(code >= 0 && code <= 7, "%s: row %d: code %d outside 0..7", fn, k, code);
  RUA_CHECK_ARG(PH == PW || !(code == 1 || code >= 5), "%s: row %d: code %d transposes and needs a square patch (got %d x %d)", fn, k, code, PH, PW);
  return RUA_OK;
}

// an ownership row (r0, r1, c0, c1) of the `what` ("row" or "group") with index k
int check_owned(const char* fn, const char* what, int k, const int32_t* o, int PH, int PW) {
  RUA_CHECK_ARG(0 <= o[0] && o[0] <= o[1] && o[1] <= PH && 0 <= o[2] && o[2] <= o[3] && o[3] <= PW,
                "%s: %s %d: owned rows %d..%d, columns %d..%d outside the %d x %d window", fn, what, k, o[0], o[1], o[2], o[3], PH, PW);
  return RUA_OK;
}

// a window table [N][4] whose codes matter
int check_window_rows(const char* fn, const int32_t* windows, int N, int PH, int PW, const int32_t* scene_h, const int32_t* scene_w, int nscenes) {
  for (int k = 0; k < N; ++k) {
    const int32_t* t = windows + 4 * (size_t)k;
    SC_TRY(check_row_place(fn, k, t, PH, PW, scene_h, scene_w, nscenes));
    SC_TRY(check_row_code(fn, k, t[3], PH, PW));
  }
  return RUA_OK;
}

// G groups of K views: rows g K .. g K + K - 1 of windows [G*K][4] are one window under K codes, own [G][4] its owned rectangle
int check_groups(const char* fn, const int32_t* windows, const int32_t* own, int G, int K, int PH, int PW, const int32_t* scene_h,
                 const int32_t* scene_w, int nscenes) {
  for (int g = 0; g < G; ++g) {
    const int32_t* t0 = windows + 4 * (size_t)g * K;
    for (int v = 0; v < K; ++v) {
      const int32_t* t = t0 + 4 * v;
      const int k = g * K + v;
      SC_TRY(check_row_place(fn, k, t, PH, PW, scene_h, scene_w, nscenes));
      RUA_CHECK_ARG(t[0] == t0[0] && t[1] == t0[1] && t[2] == t0[2], "%s: row %d: scene %d, window (%d, %d), but its group %d is scene %d, window (%d, %d)",
                    fn, k, t[0], t[1], t[2], g, t0[0], t0[1], t0[2]);
      SC_TRY(check_row_code(fn, k, t[3], PH, PW));
    }
    SC_TRY(check_owned(fn, "group", g, own + 4 * (size_t)g, PH, PW));
  }
  return RUA_OK;
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
  SC_TRY(check_scene_list("rua_scene_windows", scene_img, scene_cls, scene_h, scene_w, nscenes, Cin));
  SC_TRY(check_window_rows("rua_scene_windows", windows, N, PH, PW, scene_h, scene_w, nscenes));
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

// ---- rua_scene_windows_affine: the same outputs under a free affine map (rotation, zoom, shift), reflect-padded ------------------
// Destination pixel (i, j) samples its scene at sy = y0 + i * a_yy + j * a_yx, sx = x0 + i * a_xy + j * a_xx (Q16, pixel centres
// on integers): the image bilinearly with 8-bit fractions, the class map at the nearest pixel, indices folded into the scene by
// numpy's 'reflect' rule (include/rua_hip.h spells the arithmetic out; scenes.host_windows_affine is its numpy twin).
//
// One form: a direct gather.  A block owns one 32 x 32 destination tile of one plane; a thread resolves a destination pixel once
// (two reflections per axis, four tap offsets, the weights), reads its taps through L1 / L2 - neighbouring lanes are neighbouring
// destination columns, so their taps are neighbours along the map's x direction - and puts the result bytes into an LDS image of
// the DESTINATION tile.  After the barrier the tile leaves along destination rows in 16-byte pieces (4 bytes or single bytes where
// PW * Cin does not allow more), exactly as sw_write stores.  Staging the SOURCE bounding box in LDS instead was not built: at
// zoom-out 4 under 45 degrees a tile's box is about 181 x 181 pixels (512 KiB at Cin = 16), so that form needs this gather as its
// other branch anyway, and the gather alone already runs far below the copy it replaces.
namespace {

constexpr int SA_CHUNK = 80;                   // windows per launch: 48 bytes each
constexpr int SA_PITCH = SW_T * SW_MAXPIX + 16;  // LDS row pitch in bytes: a multiple of 16, 132 dwords (rows 4 banks apart)
constexpr int SA_MAXDIM = 16384, SA_MAXCOEF = 4 << 16, SA_MAXORG = 1 << 30;

struct AffineWin { const uint8_t* img; const uint8_t* cls; int H, W, y0, x0, ayy, ayx, axy, axx; };
struct AffineArgs {
  AffineWin w[SA_CHUNK];
  uint8_t* img_out; uint8_t* cls_out;          // of the chunk's first window
  int PH, PW, Cin, img_unit, cls_unit, planes;
};
static_assert(sizeof(AffineArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// numpy 'reflect' (no edge repeat, any number of reflections): t mod 2 (n - 1), folded.  m = 2 (n - 1) >= 2.
__device__ __forceinline__ int sa_mod(int t, int m) { const int u = t % m; return u < 0 ? u + m : u; }
__device__ __forceinline__ int sa_fold(int u, int n, int m) { return u < n ? u : m - u; }

template <int U>
__device__ __forceinline__ void sa_write(const uint8_t* T, uint8_t* out, int PW, int cb, int i0, int j0, int th, int tw, int tid) {
  const int upr = tw * cb / U, total = th * upr;
  for (int e = tid; e < total; e += 256) {
    const int ti = e / upr, v = e - ti * upr;
    const uint8_t* s = T + ti * SA_PITCH + v * U;                       // 16-byte aligned for U = 16, 4-byte for U = 4
    uint32_t word[U >= 4 ? U / 4 : 1];
    if (U == 1) word[0] = *s;
    else {
#pragma unroll
      for (int k = 0; k < U / 4; ++k) word[k] = reinterpret_cast<const uint32_t*>(s)[k];
    }
    StoreUnit<U>::st(out + ((size_t)(i0 + ti) * PW + j0) * cb + (size_t)v * U, word);
  }
}

__global__ __launch_bounds__(256) void scene_windows_affine(AffineArgs a) {
  __shared__ uint4 Tq[SW_T * SA_PITCH / 16];
  uint8_t* T = reinterpret_cast<uint8_t*>(Tq);
  const int tid = threadIdx.x, n = blockIdx.y, plane = blockIdx.z;
  const int PH = a.PH, PW = a.PW;
  const int tiles_x = (PW + SW_T - 1) / SW_T;
  const int i0 = (blockIdx.x / tiles_x) * SW_T, j0 = (blockIdx.x % tiles_x) * SW_T;
  const int th = min(SW_T, PH - i0), tw = min(SW_T, PW - j0);
  const AffineWin& w = a.w[n];
  const int H = w.H, W = w.W, mh = 2 * (H - 1), mw = 2 * (W - 1);
  const int cb = plane ? 1 : a.Cin, unit = plane ? a.cls_unit : a.img_unit;
  uint8_t* out = (plane ? a.cls_out : a.img_out) + (size_t)n * PH * PW * cb;
  for (int e = tid; e < th * SW_T; e += 256) {
    const int ti = e / SW_T, tj = e % SW_T;
    if (tj >= tw) continue;
    const int i = i0 + ti, j = j0 + tj;
    // 32-bit throughout: |y0|, |x0| <= 2^30, |a| <= 2^18 and i, j <= 511 give |i * a + j * a'| < 2^28, so |sy|, |sx| < 2^30 + 2^28,
    // and the + 32768 of the nearest rule stays below 2^31 (the host refuses anything beyond these limits)
    const int sy = w.y0 + i * w.ayy + j * w.ayx, sx = w.x0 + i * w.axy + j * w.axx;
    uint8_t* d = T + ti * SA_PITCH + tj * cb;
    if (plane) {
      const int r = sa_fold(sa_mod((sy + 32768) >> 16, mh), H, mh), c = sa_fold(sa_mod((sx + 32768) >> 16, mw), W, mw);
      *d = w.cls[(size_t)r * W + c];
    } else {
      const int uy = sa_mod(sy >> 16, mh), ux = sa_mod(sx >> 16, mw);   // of iy, ix; iy + 1 and ix + 1 are one step on in the cycle
      const int r0 = sa_fold(uy, H, mh), r1 = sa_fold(uy + 1 == mh ? 0 : uy + 1, H, mh);
      const int c0 = sa_fold(ux, W, mw), c1 = sa_fold(ux + 1 == mw ? 0 : ux + 1, W, mw);
      const uint32_t fy = (uint32_t)(sy & 0xFFFF) >> 8, fx = (uint32_t)(sx & 0xFFFF) >> 8;
      const uint8_t* p00 = w.img + ((size_t)r0 * W + c0) * cb;
      const uint8_t* p01 = w.img + ((size_t)r0 * W + c1) * cb;
      const uint8_t* p10 = w.img + ((size_t)r1 * W + c0) * cb;
      const uint8_t* p11 = w.img + ((size_t)r1 * W + c1) * cb;
      for (int ch = 0; ch < cb; ++ch) {
        // at most 256 * 256 * 255 + 32768 < 2^25
        const uint32_t top = (256 - fx) * p00[ch] + fx * p01[ch], bot = (256 - fx) * p10[ch] + fx * p11[ch];
        d[ch] = (uint8_t)(((256 - fy) * top + fy * bot + 32768) >> 16);
      }
    }
  }
  __syncthreads();
  if (unit == 16) sa_write<16>(T, out, PW, cb, i0, j0, th, tw, tid);
  else if (unit == 4) sa_write<4>(T, out, PW, cb, i0, j0, th, tw, tid);
  else sa_write<1>(T, out, PW, cb, i0, j0, th, tw, tid);
}

}  // namespace

extern "C" int rua_scene_windows_affine(const uint8_t* const* scene_img, const uint8_t* const* scene_cls, const int32_t* scene_h,
                                        const int32_t* scene_w, int nscenes, const int32_t* windows, int N, int PH, int PW, int Cin,
                                        uint8_t* img_out, uint8_t* cls_out, void* stream) {
  RUA_CHECK_ARG(scene_img && scene_h && scene_w && windows && img_out,
                "rua_scene_windows_affine: scene_img, scene_h, scene_w, windows and img_out are required");
  RUA_CHECK_ARG(!scene_cls == !cls_out, "rua_scene_windows_affine: scene_cls and cls_out go together");
  RUA_CHECK_ARG(nscenes >= 1 && N >= 1, "rua_scene_windows_affine: nscenes %d, N %d (both >= 1)", nscenes, N);
  RUA_CHECK_ARG(Cin >= 1 && Cin <= SW_MAXPIX, "rua_scene_windows_affine: Cin %d outside 1..16", Cin);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= SW_MAXP && PW <= SW_MAXP, "rua_scene_windows_affine: PH %d, PW %d (1 <= PH, PW <= 512)", PH, PW);
  RUA_CHECK_ARG(((uintptr_t)img_out & 3) == 0 && ((uintptr_t)cls_out & 3) == 0, "rua_scene_windows_affine: img_out and cls_out must be 4-byte aligned");
  for (int s = 0; s < nscenes; ++s) {
    RUA_CHECK_ARG(scene_img[s] && (!scene_cls || scene_cls[s]), "rua_scene_windows_affine: scene %d: null pointer", s);
    RUA_CHECK_ARG(scene_h[s] >= 2 && scene_w[s] >= 2 && scene_h[s] <= SA_MAXDIM && scene_w[s] <= SA_MAXDIM,
                  "rua_scene_windows_affine: scene %d: size %d x %d (2 <= H, W <= 16384)", s, scene_h[s], scene_w[s]);
  }
  for (int k = 0; k < N; ++k) {
    const int32_t* t = windows + 7 * (size_t)k;
    const int s = t[0];
    RUA_CHECK_ARG(s >= 0 && s < nscenes, "rua_scene_windows_affine: row %d: scene %d outside 0..%d", k, s, nscenes - 1);
    RUA_CHECK_ARG(t[1] >= -SA_MAXORG && t[1] <= SA_MAXORG && t[2] >= -SA_MAXORG && t[2] <= SA_MAXORG,
                  "rua_scene_windows_affine: row %d: origin (%d, %d) outside -2^30..2^30 (Q16)", k, t[1], t[2]);
    for (int q = 3; q < 7; ++q)
      RUA_CHECK_ARG(t[q] >= -SA_MAXCOEF && t[q] <= SA_MAXCOEF,
                    "rua_scene_windows_affine: row %d: coefficient %d outside -262144..262144 (4 in Q16)", k, t[q]);
  }
  hipStream_t st = (hipStream_t)stream;
  const int tiles = ((PH + SW_T - 1) / SW_T) * ((PW + SW_T - 1) / SW_T);
  AffineArgs a;
  memset(&a, 0, sizeof(a));
  a.PH = PH; a.PW = PW; a.Cin = Cin; a.planes = cls_out ? 2 : 1;
  a.img_unit = store_unit(img_out, PW * Cin);
  a.cls_unit = store_unit(cls_out, PW);
  for (int k0 = 0; k0 < N; k0 += SA_CHUNK) {
    const int nk = N - k0 < SA_CHUNK ? N - k0 : SA_CHUNK;
    for (int k = 0; k < nk; ++k) {
      const int32_t* t = windows + 7 * (size_t)(k0 + k);
      const int s = t[0];
      AffineWin& w = a.w[k];
      w.img = scene_img[s];
      w.cls = scene_cls ? scene_cls[s] : nullptr;
      w.H = scene_h[s]; w.W = scene_w[s];
      w.y0 = t[1]; w.x0 = t[2]; w.ayy = t[3]; w.ayx = t[4]; w.axy = t[5]; w.axx = t[6];
    }
    a.img_out = img_out + (size_t)k0 * PH * PW * Cin;          // a window is a whole number of rows, a row a whole number of store units
    a.cls_out = cls_out ? cls_out + (size_t)k0 * PH * PW : nullptr;
    hipLaunchKernelGGL(scene_windows_affine, dim3(tiles, nk, a.planes), dim3(256), 0, st, a);
    RUA_LAUNCH_CHECK("rua_scene_windows_affine");
  }
  return RUA_OK;
}

// ---- rua_scene_stitch: class probabilities of prediction windows -> a uint8 class map per scene and a confusion matrix -----------
// Window n of p [N][PH][PW][C] (fp32, what the seg head leaves) owns the rectangle [r0, r1) x [c0, c1) of itself (scenes.py,
// predict_table: every scene pixel belongs to exactly one window); each owned pixel's arg-max (first index of the maximum, a strict
// > scan from class 0) goes into its scene's map and, with a class map t there, into confusion[t][pred].  Integers out of one
// probability vector each: no float sum, no dependence on order; scenes.host_stitch gives the same bytes.
//
// The kernel is bound by reading p.  A block owns up to SS_BAND rows x tw columns of one window's rectangle (tw * C <= SS_ROWF
// floats, at most 256 columns) and walks it in passes of as many rows as fit into LDS.  An owned row is one contiguous run of
// (c1 - c0) * C floats that may start at any dword (C = 5: every pixel 20 bytes), so it comes in as the ALIGNED 16-byte pieces
// that cover it - whole pieces straight into LDS at the same dword phase, single dwords only where a piece would reach past the end
// of p - and then one lane takes the arg-max of one pixel out of LDS (stride C dwords: free of conflicts for odd C, two-way for
// C = 6).  Lanes of a wave are neighbouring pixels of a scene row: the class map is read and the prediction written as contiguous
// bytes.  Counts collect in an LDS histogram of C * C cells (a block holds at most 8 * 256 pixels: 32 bits are plenty; ss_score, ss_flush).
namespace {

constexpr int SS_CHUNK = 120;                  // windows per launch: 32 bytes each
constexpr int SS_BAND = 8;                     // rows of a window per block
constexpr int SS_ROWF = 4096;                  // floats of one staged row run at most (C = 64: 64 pixels)
constexpr int SS_LDSF = 4608;                  // LDS floats: >= one row's pitch (SS_ROWF + 6) / 4 * 4 = 4100
constexpr int SS_MAXC = 64;

// One window of a stitching launch, or one group of K views of it (the three stitch kernels).  out, cls: at the window's origin in
// its scene's map (cls: null where nothing is counted); W: the scene's width; codes: 3 bits per view, view 0 lowest.
struct StitchGroup { uint8_t* out; const uint8_t* cls; int W; uint16_t r0, r1, c0, c1; uint32_t codes; };
struct StitchArgs {
  StitchGroup w[SS_CHUNK];
  const float* p; unsigned long long* confusion;
  long long total;                             // floats in p: nothing beyond is read
  int first, PH, PW, C, tw;                    // first: table row of w[0]; tw: columns per block
};
static_assert(sizeof(StitchGroup) == 32 && sizeof(StitchArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// group g of a launch from rows t (its K table rows) and o (its ownership row); the maps hold bpp bytes per pixel
void fill_group(StitchGroup& w, const int32_t* t, const int32_t* o, int K, uint8_t* out, const uint8_t* cls, int W, int bpp) {
  const size_t px = (size_t)t[1] * W + t[2];
  w.out = out + px * bpp;
  w.cls = cls ? cls + px : nullptr;
  w.W = W;
  w.r0 = (uint16_t)o[0]; w.r1 = (uint16_t)o[1]; w.c0 = (uint16_t)o[2]; w.c1 = (uint16_t)o[3];
  w.codes = 0;
  for (int v = 0; v < K; ++v) w.codes |= (uint32_t)t[4 * v + 3] << (3 * v);
}

// The scoring tail of a stitched pixel: the arg-max of its C values at v (first index of the maximum, a strict > scan from class
// 0) goes to window pixel (i, j) of the scene's map and, with a class map, into the block's histogram cell [t][pred] ...
__device__ __forceinline__ void ss_score(const float* v, int C, const StitchGroup& w, int i, int j, bool count, uint32_t* hist) {
  float best = v[0];
  int pred = 0;
  for (int c = 1; c < C; ++c) {
    const float x = v[c];
    if (x > best) { best = x; pred = c; }
  }
  const size_t at = (size_t)i * w.W + j;
  w.out[at] = (uint8_t)pred;
  if (count) {
    const int t = w.cls[at];
    if (t < C) atomicAdd(&hist[t * C + pred], 1u);
  }
}

// ... and at the end of the block (after a barrier) every non-zero cell leaves with one 64-bit atomicAdd
__device__ __forceinline__ void ss_flush(const uint32_t* hist, int C, unsigned long long* confusion, int tid) {
  for (int e = tid; e < C * C; e += 256) {
    const uint32_t n = hist[e];
    if (n) atomicAdd(confusion + e, (unsigned long long)n);
  }
}

__global__ __launch_bounds__(256) void scene_stitch(StitchArgs a) {
  __shared__ uint4 Sq[SS_LDSF / 4];
  extern __shared__ uint32_t hist[];             // C * C cells (dynamic: 144 bytes at C = 6, not the 16 KiB of C = 64)
  float* S = reinterpret_cast<float*>(Sq);
  const int tid = threadIdx.x, C = a.C, PW = a.PW;
  const StitchGroup& w = a.w[blockIdx.y];
  const int chunks = (PW + a.tw - 1) / a.tw;
  const int band = blockIdx.x / chunks, chunk = blockIdx.x - band * chunks;
  const int i0 = w.r0 + band * SS_BAND, j0 = w.c0 + chunk * a.tw;
  if (i0 >= w.r1 || j0 >= w.c1) return;        // the whole block: nothing of the rectangle lies here (an empty rectangle: every block)
  const int th = min(SS_BAND, w.r1 - i0), tw = min(a.tw, w.c1 - j0);
  const bool count = w.cls != nullptr;
  if (count)
    for (int e = tid; e < C * C; e += 256) hist[e] = 0u;
  const int ne = tw * C, maxp = (ne + 6) / 4, pitch = maxp * 4;        // pieces that cover a run at any phase; LDS row pitch in floats
  const int R = min(th, SS_LDSF / pitch);
  const long long wbase = ((long long)(a.first + blockIdx.y) * a.PH) * PW;   // pixel index of the window in p
  for (int ib = 0; ib < th; ib += R) {
    const int nr = min(R, th - ib);
    __syncthreads();                           // the last pass' reads of S (and the zeroing of hist) are done
    for (int e = tid; e < nr * maxp; e += 256) {
      const int rr = e / maxp, q = e - rr * maxp;
      const long long e0 = (wbase + (long long)(i0 + ib + rr) * PW + j0) * C, a0 = e0 & ~3LL;   // the run is floats [e0, e0 + ne) of p
      const long long lo = a0 + 4 * q;
      if (lo >= e0 + ne) continue;
      if (lo + 4 <= a.total) Sq[rr * maxp + q] = ldg16(a.p + lo);
      else for (long long k = lo; k < a.total; ++k) S[rr * pitch + (int)(k - a0)] = a.p[k];
    }
    __syncthreads();
    for (int e = tid; e < nr * tw; e += 256) {
      const int rr = e / tw, tj = e - rr * tw, i = i0 + ib + rr, j = j0 + tj;
      const int phase = (int)(((wbase + (long long)i * PW + j0) * C) & 3);
      const float* v = S + rr * pitch + phase + tj * C;              // ss_score, written out: see DESIGN.md
      float best = v[0];
      int pred = 0;
      for (int c = 1; c < C; ++c) {
        const float x = v[c];
        if (x > best) { best = x; pred = c; }
      }
      const size_t at = (size_t)i * w.W + j;
      w.out[at] = (uint8_t)pred;
      if (count) {
        const int t = w.cls[at];
        if (t < C) atomicAdd(&hist[t * C + pred], 1u);
      }
    }
  }
  if (!count) return;
  __syncthreads();
  for (int e = tid; e < C * C; e += 256) {     // ss_flush, written out
    const uint32_t n = hist[e];
    if (n) atomicAdd(a.confusion + e, (unsigned long long)n);
  }
}

}  // namespace

extern "C" int rua_scene_stitch(const float* p, int N, int PH, int PW, int C, const int32_t* windows, const int32_t* own,
                                uint8_t* const* scene_pred, const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w,
                                int nscenes, int64_t* confusion, void* stream) {
  RUA_CHECK_ARG(p && windows && own && scene_pred && scene_h && scene_w, "rua_scene_stitch: p, windows, own, scene_pred, scene_h and scene_w are required");
  RUA_CHECK_ARG(!scene_cls == !confusion, "rua_scene_stitch: scene_cls and confusion go together");
  RUA_CHECK_ARG(nscenes >= 1 && N >= 1, "rua_scene_stitch: nscenes %d, N %d (both >= 1)", nscenes, N);
  RUA_CHECK_ARG(C >= 1 && C <= SS_MAXC, "rua_scene_stitch: C %d outside 1..64", C);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= SW_MAXP && PW <= SW_MAXP, "rua_scene_stitch: PH %d, PW %d (1 <= PH, PW <= 512)", PH, PW);
  RUA_CHECK_ARG(((uintptr_t)p & 15) == 0 && ((uintptr_t)confusion & 7) == 0, "rua_scene_stitch: p must be 16-byte, confusion 8-byte aligned");
  SC_TRY(check_scene_list("rua_scene_stitch", scene_pred, scene_cls, scene_h, scene_w, nscenes, 1));
  for (int k = 0; k < N; ++k) {                  // check_groups' order for K = 1, with this entry point's own rule for the code
    const int32_t* t = windows + 4 * (size_t)k;
    SC_TRY(check_row_place("rua_scene_stitch", k, t, PH, PW, scene_h, scene_w, nscenes));
    RUA_CHECK_ARG(t[3] == 0, "rua_scene_stitch: row %d: code %d (a prediction window is cut as it is: code 0)", k, t[3]);
    SC_TRY(check_owned("rua_scene_stitch", "row", k, own + 4 * (size_t)k, PH, PW));
  }
  hipStream_t st = (hipStream_t)stream;
  StitchArgs a;
  memset(&a, 0, sizeof(a));
  a.p = p; a.confusion = reinterpret_cast<unsigned long long*>(confusion);
  a.total = (long long)N * PH * PW * C;
  a.PH = PH; a.PW = PW; a.C = C;
  a.tw = SS_ROWF / C < 256 ? SS_ROWF / C : 256;
  if (a.tw > PW) a.tw = PW;
  const int blocks = ((PH + SS_BAND - 1) / SS_BAND) * ((PW + a.tw - 1) / a.tw);
  for (int k0 = 0; k0 < N; k0 += SS_CHUNK) {
    const int nk = N - k0 < SS_CHUNK ? N - k0 : SS_CHUNK;
    for (int k = 0; k < nk; ++k) {
      const int32_t* t = windows + 4 * (size_t)(k0 + k);
      const int s = t[0];
      fill_group(a.w[k], t, own + 4 * (size_t)(k0 + k), 1, scene_pred[s], scene_cls ? scene_cls[s] : nullptr, scene_w[s], 1);
    }
    a.first = k0;
    hipLaunchKernelGGL(scene_stitch, dim3(blocks, nk), dim3(256), scene_cls ? (size_t)C * C * sizeof(uint32_t) : 0, st, a);
    RUA_LAUNCH_CHECK("rua_scene_stitch");
  }
  return RUA_OK;
}

// ---- rua_scene_stitch_views: test-time augmentation - K views of every window summed, then the arg-max, map and matrix --------
// Group g of p [G*K][PH][PW][C] holds K views of ONE window: view k is the network's answer to the window under symmetry code_k
// (rua_scene_windows cut it so).  Turned back (scenes.INVERSE), the K probability vectors of a window pixel are summed per class by
// sequential fp32 adds in view order, s = q_0, s = s + q_k - no tree, no atomics, no wider accumulator - and the arg-max of s goes
// where rua_scene_stitch puts the arg-max of p.  scenes.host_stitch_views gives the same bytes.
//
// A block owns a T x T tile of a group's owned rectangle (clipped to it); T, a multiple of 4 up to 32, is the largest with
// T * T * C <= SV_ACCF (tile_of), so a thread holds at most SV_SLOTS = 16 (pixel, class) sums in registers, the same ones under
// every view: the order of a sum is the order of the view loop.  Under any of the eight symmetries the tile is a (transposed,
// mirrored) rectangle of the view (view_tile), so every view is read ALONG ITS OWN ROWS (sv_stage); the turn back happens in the
// LDS read (sv_at), whose row pitch is an odd number of 16-byte pieces so that the rows a transposed read walks start in different
// banks.  A barrier on either side of the staging separates the views.  At the end the sums go to LDS (over the staging area) and
// one lane scores one pixel as in scene_stitch (ss_score, ss_flush), lanes along scene rows.
namespace {

constexpr int SV_CHUNK = 120;                  // groups per launch: 32 bytes each
constexpr int SV_MAXK = 8;
constexpr int SV_ACCF = 4096;                  // sums of one tile at most: T * T * C
constexpr int SV_SLOTS = SV_ACCF / 256;        // ... and of one thread

struct ViewArgs {
  StitchGroup g[SV_CHUNK];
  const float* p; unsigned long long* confusion;
  long long total;                             // floats in p: nothing beyond is read
  int first, PH, PW, C, K, T, maxp;            // first: group of g[0]; maxp: LDS row pitch in 16-byte pieces (odd)
};
static_assert(sizeof(ViewArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// the tile edge T and the LDS row pitch maxp (pieces that cover a run of T * C floats at any phase, made odd) for C values a pixel
void tile_of(int C, int& T, int& maxp) {
  T = 32;
  while (T * T * C > SV_ACCF) T -= 4;                          // C = 64: 8
  maxp = ((T * C + 6) / 4) | 1;
}

// The tile [i0, i0 + th) x [j0, j0 + tw) of a PH x PW window under a view: window pixel (i, j) sits at view (tr ? (y, x) : (x, y))
// with x = fr ? PH-1-i : i, y = fc ? PW-1-j : j (PH == PW when tr), so the tile is va rows of vb pixels at (a0, b0) of the view.
struct ViewTile { int a0, b0, va, vb; };
__device__ __forceinline__ ViewTile view_tile(bool tr, bool fr, bool fc, int PH, int PW, int i0, int j0, int th, int tw) {
  const int x0 = fr ? PH - i0 - th : i0, y0 = fc ? PW - j0 - tw : j0;
  return {tr ? y0 : x0, tr ? x0 : y0, tr ? tw : th, tr ? th : tw};
}

// the read side of a view: va rows of ne floats, row rr the run that starts at pixel vbase + (a0 + rr) * PW + b0 of p, as the aligned
// 16-byte pieces that cover it (single dwords only where a piece would reach past the end of p) into LDS rows of maxp pieces at the
// run's own dword phase
__device__ __forceinline__ void sv_stage(uint4* Vq, const float* p, long long total, long long vbase, int a0, int b0, int va, int ne,
                                         int PW, int C, int maxp, int tid) {
  float* S = reinterpret_cast<float*>(Vq);
  const int pitch = maxp * 4;
  for (int e = tid; e < va * maxp; e += 256) {
    const int rr = e / maxp, q = e - rr * maxp;
    const long long e0 = (vbase + (long long)(a0 + rr) * PW + b0) * C, al = e0 & ~3LL;   // the run is floats [e0, e0 + ne) of p
    const long long lo = al + 4 * q;
    if (lo >= e0 + ne) continue;
    if (lo + 4 <= total) Vq[rr * maxp + q] = ldg16(p + lo);
    else for (long long x = lo; x < total; ++x) S[rr * pitch + (int)(x - al)] = p[x];
  }
}

// item e of a tile of tw columns and C values a pixel, e = (ti * tw + tj) * C + c, kept as one register over the view loop
struct TileItem { int ti, tj, c; };
__device__ __forceinline__ int sv_pack(int e, int C, int tw) {
  const int px = e / C, c = e - px * C, ti = px / tw, tj = px - ti * tw;
  return (ti << 16) | (tj << 8) | c;
}
__device__ __forceinline__ TileItem sv_unpack(int pk) { return {pk >> 16, (pk >> 8) & 255, pk & 255}; }

// the turn back: the LDS float of a tile item in the staged view.  pb: the low bits of the pixel index of the view tile's first
// pixel, of which a row's dword phase follows
__device__ __forceinline__ int sv_at(bool tr, bool fr, bool fc, const TileItem& it, int th, int tw, unsigned pb, int PW, int C, int pitch) {
  const int xl = fr ? th - 1 - it.ti : it.ti, yl = fc ? tw - 1 - it.tj : it.tj;
  const int ra = tr ? yl : xl, cb = tr ? xl : yl;
  const int phase = (int)(((pb + (unsigned)(ra * PW)) * (unsigned)C) & 3u);
  return ra * pitch + phase + cb * C + it.c;
}

__global__ __launch_bounds__(256) void scene_stitch_views(ViewArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 Vq[];      // T * maxp pieces of staging, then C * C histogram cells
  float* S = reinterpret_cast<float*>(Vq);
  const int tid = threadIdx.x, C = a.C, PH = a.PH, PW = a.PW, T = a.T, maxp = a.maxp, pitch = maxp * 4;
  uint32_t* hist = reinterpret_cast<uint32_t*>(Vq + T * maxp);
  const StitchGroup& w = a.g[blockIdx.y];
  const int tiles_x = (PW + T - 1) / T;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i0 = w.r0 + ty * T, j0 = w.c0 + tx * T;
  if (i0 >= w.r1 || j0 >= w.c1) return;        // the whole block: nothing of the rectangle lies here (an empty rectangle: every block)
  const int th = min(T, w.r1 - i0), tw = min(T, w.c1 - j0), ne_tile = th * tw * C;
  const bool count = w.cls != nullptr;
  if (count)
    for (int e = tid; e < C * C; e += 256) hist[e] = 0u;            // the view loop's barriers come before any use
  // this thread's sums: element e = (ti * tw + tj) * C + c of the tile for e = tid + 256 m
  int pk[SV_SLOTS];
  float acc[SV_SLOTS];
#pragma unroll
  for (int m = 0; m < SV_SLOTS; ++m) {
    const int e = tid + 256 * m;
    pk[m] = 0;
    acc[m] = 0.f;
    if (e < ne_tile) pk[m] = sv_pack(e, C, tw);
  }
  const long long group = a.first + (long long)blockIdx.y;
  for (int k = 0; k < a.K; ++k) {
    const Sym y{(int)(w.codes >> (3 * k)) & 7};
    const bool tr = y.tr(), fr = y.fr(), fc = y.fc();
    const ViewTile vt = view_tile(tr, fr, fc, PH, PW, i0, j0, th, tw);
    const long long vbase = (group * a.K + k) * PH * PW;            // pixel index of the view in p
    __syncthreads();                           // the last view's reads of S are done
    sv_stage(Vq, a.p, a.total, vbase, vt.a0, vt.b0, vt.va, vt.vb * C, PW, C, maxp, tid);
    __syncthreads();
    const unsigned pb = (unsigned)vbase + (unsigned)(vt.a0 * PW + vt.b0);
#pragma unroll
    for (int m = 0; m < SV_SLOTS; ++m) {
      if (tid + 256 * m < ne_tile) {
        const float v = S[sv_at(tr, fr, fc, sv_unpack(pk[m]), th, tw, pb, PW, C, pitch)];
        acc[m] = k == 0 ? v : acc[m] + v;      // sequential fp32 adds in view order
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < SV_SLOTS; ++m)
    if (tid + 256 * m < ne_tile) S[tid + 256 * m] = acc[m];
  __syncthreads();
  for (int e = tid; e < th * tw; e += 256) {
    const int ti = e / tw, tj = e - ti * tw;
    ss_score(S + e * C, C, w, i0 + ti, j0 + tj, count, hist);
  }
  if (!count) return;
  __syncthreads();
  ss_flush(hist, C, a.confusion, tid);
}

}  // namespace

extern "C" int rua_scene_stitch_views(const float* p, int G, int K, int PH, int PW, int C, const int32_t* windows, const int32_t* own,
                                      uint8_t* const* scene_pred, const uint8_t* const* scene_cls, const int32_t* scene_h,
                                      const int32_t* scene_w, int nscenes, int64_t* confusion, void* stream) {
  RUA_CHECK_ARG(p && windows && own && scene_pred && scene_h && scene_w,
                "rua_scene_stitch_views: p, windows, own, scene_pred, scene_h and scene_w are required");
  RUA_CHECK_ARG(!scene_cls == !confusion, "rua_scene_stitch_views: scene_cls and confusion go together");
  RUA_CHECK_ARG(nscenes >= 1 && G >= 1, "rua_scene_stitch_views: nscenes %d, G %d (both >= 1)", nscenes, G);
  RUA_CHECK_ARG(K >= 1 && K <= SV_MAXK, "rua_scene_stitch_views: K %d outside 1..8", K);
  RUA_CHECK_ARG(C >= 1 && C <= SS_MAXC, "rua_scene_stitch_views: C %d outside 1..64", C);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= SW_MAXP && PW <= SW_MAXP, "rua_scene_stitch_views: PH %d, PW %d (1 <= PH, PW <= 512)", PH, PW);
  RUA_CHECK_ARG(((uintptr_t)p & 15) == 0 && ((uintptr_t)confusion & 7) == 0, "rua_scene_stitch_views: p must be 16-byte, confusion 8-byte aligned");
  SC_TRY(check_scene_list("rua_scene_stitch_views", scene_pred, scene_cls, scene_h, scene_w, nscenes, 1));
  SC_TRY(check_groups("rua_scene_stitch_views", windows, own, G, K, PH, PW, scene_h, scene_w, nscenes));
  hipStream_t st = (hipStream_t)stream;
  ViewArgs a;
  memset(&a, 0, sizeof(a));
  a.p = p; a.confusion = reinterpret_cast<unsigned long long*>(confusion);
  a.total = (long long)G * K * PH * PW * C;
  a.PH = PH; a.PW = PW; a.C = C; a.K = K;
  tile_of(C, a.T, a.maxp);
  const int blocks = ((PH + a.T - 1) / a.T) * ((PW + a.T - 1) / a.T);
  const size_t lds = (size_t)a.T * a.maxp * 16 + (scene_cls ? (size_t)C * C * sizeof(uint32_t) : 0);   // 33 KiB at most (C = 64)
  for (int g0 = 0; g0 < G; g0 += SV_CHUNK) {
    const int ng = G - g0 < SV_CHUNK ? G - g0 : SV_CHUNK;
    for (int g = 0; g < ng; ++g) {
      const int32_t* t = windows + 4 * (size_t)(g0 + g) * K;
      const int s = t[0];
      fill_group(a.g[g], t, own + 4 * (size_t)(g0 + g), K, scene_pred[s], scene_cls ? scene_cls[s] : nullptr, scene_w[s], 1);
    }
    a.first = g0;
    hipLaunchKernelGGL(scene_stitch_views, dim3(blocks, ng), dim3(256), lds, st, a);
    RUA_LAUNCH_CHECK("rua_scene_stitch_views");
  }
  return RUA_OK;
}

// ---- rua_scene_stitch_maps: any head's window outputs under K views -> a uint8 scene map of Ch interleaved channels -------------
// The same groups, ownership and view codes as rua_scene_stitch_views, but the map keeps every channel: a float becomes the integer
// a = rint(clamp(x, 0, 1) * 65536) the moment it leaves LDS (sm_q16: a multiply by a power of two, so contraction cannot matter), and
// everything after is integer arithmetic - the order of the views, of the launches and of the lanes cannot change a byte, and
// scenes.host_stitch_maps gives the same ones.  Mode 0 (plain): A = sum of a_k, out = (255 A + K 32768) / (K 65536), the rounded
// mean.  Mode 1 (hsv_rgb, Ch = 3): every view's (h, s, v) = (179 a_0 >> 16, 255 a_1 >> 16, 255 a_2 >> 16) goes through sm_hsv_rgb
// and the views are averaged in RGB, out = (2 sum + K) / (2 K): hue is circular, its mean is not a hue.
//
// The read side is scene_stitch_views': a block owns a T x T tile of a group's rectangle, each view comes in along its own rows
// (sv_stage), the turn back happens in the LDS read (sv_at) and the sums stay in registers over the view loop - in mode 0 a thread holds
// (pixel, channel) elements tid + 256 m, consecutive lanes consecutive floats of a window row (free of bank conflicts under a
// code that keeps rows, stride Ch dwords under a transposing one: odd pitch, so 2-way at most for even Ch); in mode 1 it holds
// whole pixels tid + 256 m (T = 32: four of them), three floats at a stride of 3 dwords between lanes, conflict-free.
//
// The write side: a tile row is tw * Ch bytes of a scene row at ANY byte phase (W * Ch is odd as often as not), and its
// neighbours in the same dword belong to other blocks.  The finished bytes go into an LDS image of the tile, row ti at the byte
// phase of its scene row, and leave as the aligned dwords that lie wholly inside the row plus single bytes at its two ragged ends,
// lanes along the row - what scene_windows does on its read side, mirrored.  No lane stores a byte outside its rectangle.
namespace {

constexpr int SM_CHUNK = 120;                  // groups per launch: 32 bytes each
constexpr int SM_PIX = 4;                      // pixels of one thread in mode 1: 32 * 32 / 256

struct MapArgs {
  StitchGroup g[SM_CHUNK];                     // out: the Ch-channel map; cls unused
  const float* p;
  long long total;                             // floats in p: nothing beyond is read
  int first, PH, PW, Ch, K, T, maxp;           // as ViewArgs
};
static_assert(sizeof(MapArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// NaN and everything <= 0 give 0, everything >= 1 (+inf too) 65536; ties to even
__device__ __forceinline__ uint32_t sm_q16(float x) {
  const float y = x > 0.f ? fminf(x, 1.f) : 0.f;
  return (uint32_t)__float2int_rn(y * 65536.f);
}

// scenes.hsv_to_rgb_u8: the textbook sector formula rounded exactly, h in 0..179 (30 per sector), s and v in 0..255
__device__ __forceinline__ void sm_hsv_rgb(uint32_t h, uint32_t s, uint32_t v, uint32_t& r, uint32_t& g, uint32_t& b) {
  const uint32_t sec = h / 30u, f = h - sec * 30u;
  const uint32_t p = (v * (255u - s) + 127u) / 255u;
  const uint32_t q = (v * (7650u - s * f) + 3825u) / 7650u;
  const uint32_t t = (v * (7650u - s * (30u - f)) + 3825u) / 7650u;
  r = sec == 0 || sec == 5 ? v : sec == 1 ? q : sec == 4 ? t : p;
  g = sec == 1 || sec == 2 ? v : sec == 0 ? t : sec == 3 ? q : p;
  b = sec == 3 || sec == 4 ? v : sec == 2 ? t : sec == 5 ? q : p;
}

template <int MODE>
__global__ __launch_bounds__(256) void scene_stitch_maps(MapArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 Mq[];      // T * maxp pieces of staging; the byte image of the tile lies over it at the end
  const float* S = reinterpret_cast<const float*>(Mq);
  const int tid = threadIdx.x, Ch = a.Ch, PH = a.PH, PW = a.PW, T = a.T, maxp = a.maxp, pitch = maxp * 4;
  const StitchGroup& w = a.g[blockIdx.y];
  const int tiles_x = (PW + T - 1) / T;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i0 = w.r0 + ty * T, j0 = w.c0 + tx * T;
  if (i0 >= w.r1 || j0 >= w.c1) return;        // the whole block: nothing of the rectangle lies here (an empty rectangle: every block)
  const int th = min(T, w.r1 - i0), tw = min(T, w.c1 - j0);
  // this thread's items: mode 0 element e = (ti * tw + tj) * Ch + c of the tile, mode 1 pixel e = ti * tw + tj, for e = tid + 256 m
  constexpr int NS = MODE ? SM_PIX : SV_SLOTS, NA = MODE ? 3 : 1;
  const int items = MODE ? th * tw : th * tw * Ch;
  int pk[NS];
  uint32_t acc[NS][NA];
#pragma unroll
  for (int m = 0; m < NS; ++m) {
    const int e = tid + 256 * m;
    pk[m] = 0;
#pragma unroll
    for (int n = 0; n < NA; ++n) acc[m][n] = 0u;
    if (e < items) pk[m] = sv_pack(e, MODE ? 1 : Ch, tw);      // mode 1: c = 0, the pixel's first channel
  }
  const long long group = a.first + (long long)blockIdx.y;
  for (int k = 0; k < a.K; ++k) {
    const Sym y{(int)(w.codes >> (3 * k)) & 7};
    const bool tr = y.tr(), fr = y.fr(), fc = y.fc();
    const ViewTile vt = view_tile(tr, fr, fc, PH, PW, i0, j0, th, tw);
    const long long vbase = (group * a.K + k) * PH * PW;
    __syncthreads();                           // the last view's reads of S are done
    sv_stage(Mq, a.p, a.total, vbase, vt.a0, vt.b0, vt.va, vt.vb * Ch, PW, Ch, maxp, tid);
    __syncthreads();
    const unsigned pb = (unsigned)vbase + (unsigned)(vt.a0 * PW + vt.b0);
#pragma unroll
    for (int m = 0; m < NS; ++m) {
      if (tid + 256 * m < items) {
        const float* v = S + sv_at(tr, fr, fc, sv_unpack(pk[m]), th, tw, pb, PW, Ch, pitch);
        if (MODE == 0) {
          acc[m][0] += sm_q16(v[0]);           // at most 8 * 65536
        } else {
          uint32_t r, g, b;                    // truncation, as the reference's astype(uint8)
          sm_hsv_rgb((179u * sm_q16(v[0])) >> 16, (255u * sm_q16(v[1])) >> 16, (255u * sm_q16(v[2])) >> 16, r, g, b);
          acc[m][0] += r; acc[m][1] += g; acc[m][2] += b;
        }
      }
    }
  }
  __syncthreads();
  // the tile's bytes: row ti at the byte phase of its scene row, pitch a whole number of dwords
  uint8_t* B = reinterpret_cast<uint8_t*>(Mq);
  const int nb = tw * Ch, nd = (nb + 6) / 4, bp = nd * 4;
  const unsigned K = (unsigned)a.K;
  const unsigned o0 = (unsigned)(uintptr_t)w.out + ((unsigned)i0 * (unsigned)w.W + (unsigned)j0) * (unsigned)Ch;   // low address bits of tile row 0
  const unsigned ostep = (unsigned)w.W * (unsigned)Ch;
#pragma unroll
  for (int m = 0; m < NS; ++m) {
    if (tid + 256 * m < items) {
      const TileItem it = sv_unpack(pk[m]);
      uint8_t* d = B + it.ti * bp + (int)((o0 + (unsigned)it.ti * ostep) & 3u) + it.tj * Ch + it.c;
      if (MODE == 0) {
        d[0] = (uint8_t)((255u * acc[m][0] + K * 32768u) / (K * 65536u));   // below 2^27 + 2^18
      } else {
#pragma unroll
        for (int n = 0; n < 3; ++n) d[n] = (uint8_t)((2u * acc[m][n] + K) / (2u * K));
      }
    }
  }
  __syncthreads();
  const uint32_t* Bd = reinterpret_cast<const uint32_t*>(Mq);
  for (int e = tid; e < th * nd; e += 256) {
    const int ti = e / nd, q = e - ti * nd;
    uint8_t* row = w.out + ((size_t)(i0 + ti) * w.W + j0) * Ch;
    const int s = (int)((uintptr_t)row & 3);
    const int lo = max(4 * q, s), hi = min(4 * q + 4, s + nb);
    uint8_t* al = row - s;                     // the row's bytes go to al + [s, s + nb)
    if (hi - lo == 4) *reinterpret_cast<uint32_t*>(al + 4 * q) = Bd[ti * nd + q];
    else for (int x = lo; x < hi; ++x) al[x] = B[ti * bp + x];
  }
}

}  // namespace

extern "C" int rua_scene_stitch_maps(const float* p, int G, int K, int PH, int PW, int Ch, const int32_t* windows, const int32_t* own,
                                     uint8_t* const* scene_out, const int32_t* scene_h, const int32_t* scene_w, int nscenes, int mode,
                                     void* stream) {
  RUA_CHECK_ARG(p && windows && own && scene_out && scene_h && scene_w,
                "rua_scene_stitch_maps: p, windows, own, scene_out, scene_h and scene_w are required");
  RUA_CHECK_ARG(nscenes >= 1 && G >= 1, "rua_scene_stitch_maps: nscenes %d, G %d (both >= 1)", nscenes, G);
  RUA_CHECK_ARG(K >= 1 && K <= SV_MAXK, "rua_scene_stitch_maps: K %d outside 1..8", K);
  RUA_CHECK_ARG(Ch >= 1 && Ch <= SS_MAXC, "rua_scene_stitch_maps: Ch %d outside 1..64", Ch);
  RUA_CHECK_ARG(mode == 0 || mode == 1, "rua_scene_stitch_maps: mode %d (0 plain, 1 hsv_rgb)", mode);
  RUA_CHECK_ARG(mode == 0 || Ch == 3, "rua_scene_stitch_maps: mode 1 (hsv_rgb) reads H, S, V: Ch 3, got %d", Ch);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= SW_MAXP && PW <= SW_MAXP, "rua_scene_stitch_maps: PH %d, PW %d (1 <= PH, PW <= 512)", PH, PW);
  RUA_CHECK_ARG(((uintptr_t)p & 15) == 0, "rua_scene_stitch_maps: p must be 16-byte aligned");
  SC_TRY(check_scene_list("rua_scene_stitch_maps", scene_out, nullptr, scene_h, scene_w, nscenes, Ch, true));
  SC_TRY(check_groups("rua_scene_stitch_maps", windows, own, G, K, PH, PW, scene_h, scene_w, nscenes));
  hipStream_t st = (hipStream_t)stream;
  MapArgs a;
  memset(&a, 0, sizeof(a));
  a.p = p;
  a.total = (long long)G * K * PH * PW * Ch;
  a.PH = PH; a.PW = PW; a.Ch = Ch; a.K = K;
  tile_of(Ch, a.T, a.maxp);                                    // Ch = 3 (mode 1): 32
  const int blocks = ((PH + a.T - 1) / a.T) * ((PW + a.T - 1) / a.T);
  const size_t lds = (size_t)a.T * a.maxp * 16;                // 17 KiB at most (Ch = 4: 32 x 33 pieces); the byte image, T rows of at most T * Ch + 6 bytes, fits in it
  for (int g0 = 0; g0 < G; g0 += SM_CHUNK) {
    const int ng = G - g0 < SM_CHUNK ? G - g0 : SM_CHUNK;
    for (int g = 0; g < ng; ++g) {
      const int32_t* t = windows + 4 * (size_t)(g0 + g) * K;
      const int s = t[0];
      fill_group(a.g[g], t, own + 4 * (size_t)(g0 + g), K, scene_out[s], nullptr, scene_w[s], Ch);
    }
    a.first = g0;
    if (mode) hipLaunchKernelGGL(scene_stitch_maps<1>, dim3(blocks, ng), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(scene_stitch_maps<0>, dim3(blocks, ng), dim3(256), lds, st, a);
    RUA_LAUNCH_CHECK("rua_scene_stitch_maps");
  }
  return RUA_OK;
}

// ---- rua_scene_accumulate: the way back of a zoomed window - K views resampled onto the scene grid and added to an int32 accumulator --
// Multi-scale test-time augmentation (scenes.py, scale_table): a pass covers the scene with footprints of FH x FW scene pixels, each
// cut into a PH x PW window by rua_scene_windows_affine under K view codes (an axis-aligned matrix: a zoom per axis, flips, maybe a
// transposition).  Group g of p [G*K][PH][PW][C] holds the network's answers to those K windows, own[g] the rectangle of SCENE pixels
// the footprint owns.  For each owned pixel, each view and channel the window is sampled bilinearly at the pixel's window coordinate
// - in 1/256 pixels, an exact 64-bit floor division - from the quantised values sm_q16(p), and the K results are summed in a register
// and added to scene_acc[y][x][c] with one plain read-add-write: the groups of a call own disjoint pixels, passes are ordered by the
// stream, so there are no atomics.  Integers from the first step on; scenes.host_accumulate gives the same numbers.
//
// A block owns a SQ_TH x SQ_TW tile of one group's rectangle.  First its threads work out, per view, the taps of the tile's rows and
// columns (index pair and weight, one division each: SQ_TH + SQ_TW per view, not one per pixel and channel) into LDS; then thread e
// walks the elements (row, column, channel) e = tid + 256 m of the tile, channel fastest: consecutive lanes are consecutive int32 of
// an accumulator row - the 2 x 4 C bytes of accumulator traffic per pixel are coalesced - and read the four taps of their channel,
// neighbouring lanes neighbouring floats of p wherever the view keeps rows (a gather served by the caches: p of a batch is a few MB).
namespace {

constexpr int SQ_CHUNK = 24;                   // groups per launch: 160 bytes each
constexpr int SQ_TH = 16, SQ_TW = 64;          // tile of scene pixels per block

// one axis of one view: scene coordinate s -> window coordinate in 1/256 pixels, w = floor((256 (65536 s - o) + (|a| >> 1)) / |a|), mirrored for a < 0
struct AccAxis { int o, a; };
struct AccGroup {
  int32_t* acc;                                // the scene's accumulator [H][W][C]
  int W, r0, r1, c0, c1;
  uint32_t turns;                              // bit k: view k transposes (y feeds the column index, x the row index)
  AccAxis y[SV_MAXK], x[SV_MAXK];
};
struct AccArgs {
  AccGroup g[SQ_CHUNK];
  const float* p;
  int first, PH, PW, C, K;
};
static_assert(sizeof(AccGroup) == 160 && sizeof(AccArgs) <= 4096, "kernel arguments are limited to 4 KiB");

__host__ __device__ __forceinline__ long long sq_floordiv(long long n, long long d) {      // d > 0
  const long long q = n / d;
  return (n % d != 0 && n < 0) ? q - 1 : q;
}

// the unclamped window coordinate of scene coordinate s, in 1/256 pixels (|256 t| < 2^41, a != 0)
__host__ __device__ __forceinline__ long long sq_coord(int s, AccAxis ax) {
  long long t = (long long)s * 65536 - ax.o, a = ax.a;
  if (a < 0) { t = -t; a = -a; }
  return sq_floordiv(t * 256 + (a >> 1), a);
}

// taps of scene coordinate s along an index of n window pixels, packed: i0 | i1 << 10 | f << 20
__device__ __forceinline__ uint32_t sq_taps(int s, AccAxis ax, int n) {
  long long w = sq_coord(s, ax);
  const long long hi = (long long)(n - 1) * 256;
  w = w < 0 ? 0 : w > hi ? hi : w;
  const uint32_t i0 = (uint32_t)(w >> 8), f = (uint32_t)(w & 255);
  const uint32_t i1 = i0 + 1 < (uint32_t)n ? i0 + 1 : (uint32_t)(n - 1);
  return i0 | (i1 << 10) | (f << 20);
}

__global__ __launch_bounds__(256) void scene_accumulate(AccArgs a) {
  __shared__ uint32_t ytab[SV_MAXK][SQ_TH], xtab[SV_MAXK][SQ_TW];
  const int tid = threadIdx.x, C = a.C, PH = a.PH, PW = a.PW, K = a.K;
  const AccGroup& w = a.g[blockIdx.y];
  const int tiles_x = (w.c1 - w.c0 + SQ_TW - 1) / SQ_TW;
  if (tiles_x <= 0) return;                    // an empty rectangle: every block
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = w.r0 + ty * SQ_TH, x0 = w.c0 + tx * SQ_TW;
  if (y0 >= w.r1) return;                      // the whole block: the grid is sized for the launch's largest rectangle
  const int th = min(SQ_TH, w.r1 - y0), tw = min(SQ_TW, w.c1 - x0);
  for (int e = tid; e < K * (SQ_TH + SQ_TW); e += 256) {
    const int k = e / (SQ_TH + SQ_TW), r = e - k * (SQ_TH + SQ_TW);
    const bool turns = (w.turns >> k) & 1u;
    if (r < SQ_TH) {
      if (r < th) ytab[k][r] = sq_taps(y0 + r, w.y[k], turns ? PW : PH);
    } else if (r - SQ_TH < tw) {
      xtab[k][r - SQ_TH] = sq_taps(x0 + r - SQ_TH, w.x[k], turns ? PH : PW);
    }
  }
  __syncthreads();
  const int rowe = tw * C, items = th * rowe;
  const size_t vsize = (size_t)PH * PW * C;
  const float* pg = a.p + (size_t)(a.first + blockIdx.y) * K * vsize;
  for (int e = tid; e < items; e += 256) {
    const int r = e / rowe, rem = e - r * rowe, j = rem / C, c = rem - j * C;
    uint32_t sum = 0u;                         // at most 8 * 65536
    for (int k = 0; k < K; ++k) {
      const uint32_t ty_ = ytab[k][r], tx_ = xtab[k][j];
      const uint32_t u0 = ty_ & 1023u, u1 = (ty_ >> 10) & 1023u, fy = ty_ >> 20;
      const uint32_t v0 = tx_ & 1023u, v1 = (tx_ >> 10) & 1023u, fx = tx_ >> 20;
      const float* v = pg + (size_t)k * vsize + c;
      // window pixel (row, column) of tap (u, v): (u, v) where the view keeps rows, (v, u) where it transposes
      const bool turns = (w.turns >> k) & 1u;
      const uint32_t su = turns ? (uint32_t)C : (uint32_t)(PW * C), sv = turns ? (uint32_t)(PW * C) : (uint32_t)C;
      const uint32_t q00 = sm_q16(v[u0 * su + v0 * sv]), q01 = sm_q16(v[u0 * su + v1 * sv]);
      const uint32_t q10 = sm_q16(v[u1 * su + v0 * sv]), q11 = sm_q16(v[u1 * su + v1 * sv]);
      const uint32_t top = (256u - fx) * q00 + fx * q01, bot = (256u - fx) * q10 + fx * q11;      // at most 2^24
      sum += (uint32_t)(((unsigned long long)(256u - fy) * top + (unsigned long long)fy * bot + 32768ull) >> 16);   // the sum reaches 2^32
    }
    int32_t* d = w.acc + ((size_t)(y0 + r) * w.W + x0) * C + rem;
    *d += (int32_t)sum;
  }
}

// ---- rua_scene_accumulate_blend: scene_accumulate for OVERLAPPING footprints, each under a linear taper ------------------------------
// scenes.py, blend_table / host_accumulate_blend: a group's rectangle is its whole footprint, the footprints of a call overlap, and
// the K views' sum v of a pixel enters the accumulator as (wy wx v + 32768) >> 16 with wy, wx = blend_weight of the pixel's row and
// column inside the footprint (out of 256: a linear taper, flat towards a scene border, never below 16).  Everything up to the sum
// is scene_accumulate's - structs, tap helpers, tile, channel-fastest walk; three things differ: the weights of the tile's rows and
// columns are worked out once per tile into LDS next to the taps, the weight is applied once to the views' sum with a 64-bit
// product, and the add is an integer atomicAdd whose value nobody reads (the returnless vector atomic): two groups of a call, in
// one launch or in two, may hold the same pixel.  Integer addition commutes, so the accumulator is the same in any order; a wave's
// atomics are consecutive dwords of an accumulator row.
constexpr int SL_CHUNK = 24;                   // groups per launch: 168 bytes each
struct BlendGroup {
  AccGroup g;                                  // r0..r1, c0..c1: the full footprint
  uint32_t flat;                               // bit 0: r0 == 0, bit 1: r1 == H, bit 2: c0 == 0, bit 3: c1 == W
};
struct BlendArgs {
  BlendGroup g[SL_CHUNK];
  const float* p;
  int first, PH, PW, C, K;
};
static_assert(sizeof(BlendGroup) == 168 && sizeof(BlendArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// scenes.blend_weight: position t of a footprint of F pixels along one axis (256 (2 t + 1) < 2^24: F is a few window sizes at most)
__host__ __device__ __forceinline__ uint32_t sl_weight(int t, int F, bool flat_lo, bool flat_hi) {
  if ((flat_lo && 2 * t + 1 <= F) || (flat_hi && 2 * t + 1 >= F)) return 256u;
  const int m = t < F - 1 - t ? t : F - 1 - t;
  const int w = (256 * (2 * m + 1)) / F;
  return (uint32_t)(w < 16 ? 16 : w);
}

__global__ __launch_bounds__(256) void scene_accumulate_blend(BlendArgs a) {
  __shared__ uint32_t ytab[SV_MAXK][SQ_TH], xtab[SV_MAXK][SQ_TW], wytab[SQ_TH], wxtab[SQ_TW];
  const int tid = threadIdx.x, C = a.C, PH = a.PH, PW = a.PW, K = a.K;
  const AccGroup& w = a.g[blockIdx.y].g;
  const uint32_t flat = a.g[blockIdx.y].flat;
  const int tiles_x = (w.c1 - w.c0 + SQ_TW - 1) / SQ_TW;
  if (tiles_x <= 0) return;                    // an empty rectangle: every block
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = w.r0 + ty * SQ_TH, x0 = w.c0 + tx * SQ_TW;
  if (y0 >= w.r1) return;                      // the whole block: the grid is sized for the launch's largest rectangle
  const int th = min(SQ_TH, w.r1 - y0), tw = min(SQ_TW, w.c1 - x0);
  for (int e = tid; e < (K + 1) * (SQ_TH + SQ_TW); e += 256) {      // row K of the table: the weights
    const int k = e / (SQ_TH + SQ_TW), r = e - k * (SQ_TH + SQ_TW);
    if (k == K) {
      if (r < SQ_TH) {
        if (r < th) wytab[r] = sl_weight(y0 + r - w.r0, w.r1 - w.r0, flat & 1u, flat & 2u);
      } else if (r - SQ_TH < tw) {
        wxtab[r - SQ_TH] = sl_weight(x0 + r - SQ_TH - w.c0, w.c1 - w.c0, flat & 4u, flat & 8u);
      }
      continue;
    }
    const bool turns = (w.turns >> k) & 1u;
    if (r < SQ_TH) {
      if (r < th) ytab[k][r] = sq_taps(y0 + r, w.y[k], turns ? PW : PH);
    } else if (r - SQ_TH < tw) {
      xtab[k][r - SQ_TH] = sq_taps(x0 + r - SQ_TH, w.x[k], turns ? PH : PW);
    }
  }
  __syncthreads();
  const int rowe = tw * C, items = th * rowe;
  const size_t vsize = (size_t)PH * PW * C;
  const float* pg = a.p + (size_t)(a.first + blockIdx.y) * K * vsize;
  for (int e = tid; e < items; e += 256) {
    const int r = e / rowe, rem = e - r * rowe, j = rem / C, c = rem - j * C;
    uint32_t sum = 0u;                         // at most 8 * 65536
    for (int k = 0; k < K; ++k) {
      const uint32_t ty_ = ytab[k][r], tx_ = xtab[k][j];
      const uint32_t u0 = ty_ & 1023u, u1 = (ty_ >> 10) & 1023u, fy = ty_ >> 20;
      const uint32_t v0 = tx_ & 1023u, v1 = (tx_ >> 10) & 1023u, fx = tx_ >> 20;
      const float* v = pg + (size_t)k * vsize + c;
      const bool turns = (w.turns >> k) & 1u;
      const uint32_t su = turns ? (uint32_t)C : (uint32_t)(PW * C), sv = turns ? (uint32_t)(PW * C) : (uint32_t)C;
      const uint32_t q00 = sm_q16(v[u0 * su + v0 * sv]), q01 = sm_q16(v[u0 * su + v1 * sv]);
      const uint32_t q10 = sm_q16(v[u1 * su + v0 * sv]), q11 = sm_q16(v[u1 * su + v1 * sv]);
      const uint32_t top = (256u - fx) * q00 + fx * q01, bot = (256u - fx) * q10 + fx * q11;      // at most 2^24
      sum += (uint32_t)(((unsigned long long)(256u - fy) * top + (unsigned long long)fy * bot + 32768ull) >> 16);   // the sum reaches 2^32
    }
    const uint32_t wgt = wytab[r] * wxtab[j];  // at most 2^16
    const int32_t add = (int32_t)(((unsigned long long)wgt * sum + 32768ull) >> 16);              // the product reaches 2^35; add <= K * 65536
    atomicAdd(w.acc + ((size_t)(y0 + r) * w.W + x0) * C + rem, add);                               // the value is not read: no return
  }
}

// ---- rua_scene_argmax: the finished accumulators -> a uint8 class map per scene and a confusion matrix ----------------------------
// A block owns `np` neighbouring pixels of one scene (256, fewer where 256 C sums would not fit: np C <= SX_LDSW): their np C int32
// sums are one contiguous run of the accumulator and come in with consecutive lanes on consecutive dwords, into LDS at a pixel pitch
// of C | 1 dwords; then one lane per pixel scans its C sums out of LDS (first index of the maximum, a strict > scan from class 0; the
// odd pitch keeps the lanes on different banks), lanes along the scene row: the map is written and the class map read as contiguous
// bytes.  Counts collect in the block's LDS histogram as in scene_stitch; a launch has at most SX_BLOCKS blocks per scene and a block
// sweeps through its scene in steps of the grid, so a 6000 x 6000 scene ends in 1024 x C x C atomic adds on the C x C counters, not
// in 140 000 x C x C (a scene holds fewer than 2^38 pixels, a block sees 2^28 of them at most: 32-bit cells are plenty).
constexpr int SX_CHUNK = 100;                  // scenes per launch: 32 bytes each
constexpr int SX_LDSW = 4096;                  // int32 sums a block stages (C = 64: 64 pixels)
constexpr int SX_BLOCKS = 1024;                // blocks per scene at most: four for each of 256 compute units
struct ArgmaxScene { const int32_t* acc; uint8_t* pred; const uint8_t* cls; long long npix; };
struct ArgmaxArgs {
  ArgmaxScene s[SX_CHUNK];
  unsigned long long* confusion;
  int C, np;                                   // np: pixels per block, at most 256
};
static_assert(sizeof(ArgmaxArgs) <= 4096, "kernel arguments are limited to 4 KiB");

__global__ __launch_bounds__(256) void scene_argmax(ArgmaxArgs a) {
  __shared__ int32_t S[SX_LDSW + 256];         // np pixels at a pitch of C | 1
  extern __shared__ uint32_t hist[];             // C * C cells, only with class maps
  const int tid = threadIdx.x, C = a.C, pitch = C | 1;
  const ArgmaxScene& s = a.s[blockIdx.y];
  const long long step = (long long)gridDim.x * a.np;
  if ((long long)blockIdx.x * a.np >= s.npix) return;       // the whole block: the grid is sized for the launch's largest scene
  const bool count = s.cls != nullptr;
  if (count)
    for (int e = tid; e < C * C; e += 256) hist[e] = 0u;
  for (long long first = (long long)blockIdx.x * a.np; first < s.npix; first += step) {      // the same trips for every thread of the block
    const int n = (int)min((long long)a.np, s.npix - first);
    const int32_t* run = s.acc + (size_t)first * C;
    __syncthreads();                           // the last sweep's reads of S (and the zeroing of hist) are done
    for (int e = tid; e < n * C; e += 256) {
      const int px = e / C;
      S[px * pitch + (e - px * C)] = run[e];
    }
    __syncthreads();
    if (tid < n) {
      const int32_t* v = S + tid * pitch;
      int32_t best = v[0];
      int pred = 0;
      for (int c = 1; c < C; ++c) {
        const int32_t x = v[c];
        if (x > best) { best = x; pred = c; }
      }
      s.pred[first + tid] = (uint8_t)pred;
      if (count) {
        const int t = s.cls[first + tid];
        if (t < C) atomicAdd(&hist[t * C + pred], 1u);
      }
    }
  }
  if (!count) return;
  __syncthreads();
  ss_flush(hist, C, a.confusion, tid);
}

}  // namespace

namespace {

// the argument checks of rua_scene_accumulate and rua_scene_accumulate_blend under the caller's name, in scenes._check_accumulate's
// order and words; one_size: the non-empty rectangles of the call have one size (a blended call is one pass)
int check_accumulate(const char* fn, const float* p, int G, int K, int PH, int PW, int C, const int32_t* windows7, const int32_t* own,
                     int32_t* const* scene_acc, const int32_t* scene_h, const int32_t* scene_w, int nscenes, bool one_size) {
  RUA_CHECK_ARG(p && windows7 && own && scene_acc && scene_h && scene_w, "%s: p, windows7, own, scene_acc, scene_h and scene_w are required", fn);
  RUA_CHECK_ARG(nscenes >= 1 && G >= 1, "%s: nscenes %d, G %d (both >= 1)", fn, nscenes, G);
  RUA_CHECK_ARG(K >= 1 && K <= SV_MAXK, "%s: K %d outside 1..8", fn, K);
  RUA_CHECK_ARG(C >= 1 && C <= SS_MAXC, "%s: C %d outside 1..64", fn, C);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= SW_MAXP && PW <= SW_MAXP, "%s: PH %d, PW %d (1 <= PH, PW <= 512)", fn, PH, PW);
  RUA_CHECK_ARG(((uintptr_t)p & 15) == 0, "%s: p must be 16-byte aligned", fn);
  for (int s = 0; s < nscenes; ++s) {
    RUA_CHECK_ARG(scene_h[s] >= 1 && scene_w[s] >= 1 && scene_h[s] <= SA_MAXDIM && scene_w[s] <= SA_MAXDIM,
                  "%s: scene %d: size %d x %d (1 <= H, W <= 16384)", fn, s, scene_h[s], scene_w[s]);
    RUA_CHECK_ARG(scene_acc[s] && ((uintptr_t)scene_acc[s] & 3) == 0, "%s: scene %d: null or misaligned accumulator", fn, s);
  }
  int first = -1, fh = 0, fw = 0;               // the first non-empty rectangle and its size
  for (int g = 0; g < G; ++g) {
    const int32_t* t0 = windows7 + 7 * (size_t)g * K;
    for (int v = 0; v < K; ++v) {
      const int32_t* t = t0 + 7 * v;
      const int k = g * K + v;
      RUA_CHECK_ARG(t[0] >= 0 && t[0] < nscenes, "%s: row %d: scene %d outside 0..%d", fn, k, t[0], nscenes - 1);
      RUA_CHECK_ARG(t[0] == t0[0], "%s: row %d: scene %d, but its group %d is scene %d", fn, k, t[0], g, t0[0]);
      const bool keeps = t[4] == 0 && t[5] == 0 && t[3] != 0 && t[6] != 0, turns = t[3] == 0 && t[6] == 0 && t[4] != 0 && t[5] != 0;
      RUA_CHECK_ARG(keeps || turns, "%s: row %d: matrix (%d, %d, %d, %d) is not axis-aligned (a_yx = a_xy = 0 or a_yy = a_xx = 0, the other two nonzero)",
                    fn, k, t[3], t[4], t[5], t[6]);
      RUA_CHECK_ARG(!turns || PH == PW, "%s: row %d: matrix (%d, %d, %d, %d) transposes and needs a square patch (got %d x %d)",
                    fn, k, t[3], t[4], t[5], t[6], PH, PW);
    }
    const int H = scene_h[t0[0]], W = scene_w[t0[0]];
    const int32_t* o = own + 4 * (size_t)g;
    RUA_CHECK_ARG(0 <= o[0] && o[0] <= o[1] && o[1] <= H && 0 <= o[2] && o[2] <= o[3] && o[3] <= W,
                  "%s: group %d: rectangle rows %d..%d, columns %d..%d outside its %d x %d scene", fn, g, o[0], o[1], o[2], o[3], H, W);
    if (o[0] == o[1] || o[2] == o[3]) continue;
    if (one_size && first < 0) { first = g; fh = o[1] - o[0]; fw = o[3] - o[2]; }
    RUA_CHECK_ARG(!one_size || (o[1] - o[0] == fh && o[3] - o[2] == fw),
                  "%s: group %d: rectangle of %d x %d, but group %d has %d x %d (the footprints of one call have one size)", fn, g, o[1] - o[0],
                  o[3] - o[2], first, fh, fw);
    for (int v = 0; v < K; ++v) {
      const int32_t* t = t0 + 7 * v;
      const bool turns = t[3] == 0;
      const AccAxis ay{t[1], turns ? t[4] : t[3]}, ax{t[2], turns ? t[5] : t[6]};
      const long long ny = 256LL * (turns ? PW : PH), nx = 256LL * (turns ? PH : PW);
      const long long wy0 = sq_coord(o[0], ay), wy1 = sq_coord(o[1] - 1, ay), wx0 = sq_coord(o[2], ax), wx1 = sq_coord(o[3] - 1, ax);
      RUA_CHECK_ARG(wy0 >= -256 && wy0 <= ny && wy1 >= -256 && wy1 <= ny && wx0 >= -256 && wx0 <= nx && wx1 >= -256 && wx1 <= nx,
                    "%s: row %d: rectangle rows %d..%d, columns %d..%d of group %d leaves the window's footprint", fn, g * K + v, o[0], o[1], o[2], o[3], g);
    }
  }
  return RUA_OK;
}

// group g of a checked call as a kernel argument; returns the blocks its rectangle takes
int fill_acc_group(AccGroup& w, const int32_t* t0, const int32_t* o, int K, int32_t* const* scene_acc, const int32_t* scene_w) {
  w.acc = scene_acc[t0[0]]; w.W = scene_w[t0[0]];
  w.r0 = o[0]; w.r1 = o[1]; w.c0 = o[2]; w.c1 = o[3];
  if (w.r0 == w.r1) w.c1 = w.c0;               // empty either way: the kernel tests the columns
  w.turns = 0;
  for (int v = 0; v < K; ++v) {
    const int32_t* t = t0 + 7 * v;
    const bool turns = t[3] == 0;
    if (turns) w.turns |= 1u << v;
    w.y[v] = AccAxis{t[1], turns ? t[4] : t[3]};
    w.x[v] = AccAxis{t[2], turns ? t[5] : t[6]};
  }
  return ((w.r1 - w.r0 + SQ_TH - 1) / SQ_TH) * ((w.c1 - w.c0 + SQ_TW - 1) / SQ_TW);
}

}  // namespace

extern "C" int rua_scene_accumulate(const float* p, int G, int K, int PH, int PW, int C, const int32_t* windows7, const int32_t* own,
                                    int32_t* const* scene_acc, const int32_t* scene_h, const int32_t* scene_w, int nscenes, void* stream) {
  // every row and rectangle before anything is launched, in scenes.check_accumulate's order and words
  SC_TRY(check_accumulate("rua_scene_accumulate", p, G, K, PH, PW, C, windows7, own, scene_acc, scene_h, scene_w, nscenes, false));
  hipStream_t st = (hipStream_t)stream;
  AccArgs a;
  memset(&a, 0, sizeof(a));
  a.p = p; a.PH = PH; a.PW = PW; a.C = C; a.K = K;
  for (int g0 = 0; g0 < G; g0 += SQ_CHUNK) {
    const int ng = G - g0 < SQ_CHUNK ? G - g0 : SQ_CHUNK;
    int blocks = 0;
    for (int g = 0; g < ng; ++g) {
      const int nb = fill_acc_group(a.g[g], windows7 + 7 * (size_t)(g0 + g) * K, own + 4 * (size_t)(g0 + g), K, scene_acc, scene_w);
      if (nb > blocks) blocks = nb;
    }
    if (blocks == 0) continue;                 // nothing but empty rectangles
    a.first = g0;
    hipLaunchKernelGGL(scene_accumulate, dim3(blocks, ng), dim3(256), 0, st, a);
    RUA_LAUNCH_CHECK("rua_scene_accumulate");
  }
  return RUA_OK;
}

extern "C" int rua_scene_accumulate_blend(const float* p, int G, int K, int PH, int PW, int C, const int32_t* windows7, const int32_t* foot,
                                          int32_t* const* scene_acc, const int32_t* scene_h, const int32_t* scene_w, int nscenes, void* stream) {
  // scenes.check_accumulate_blend's order and words; nothing is launched before every group has passed
  SC_TRY(check_accumulate("rua_scene_accumulate_blend", p, G, K, PH, PW, C, windows7, foot, scene_acc, scene_h, scene_w, nscenes, true));
  hipStream_t st = (hipStream_t)stream;
  BlendArgs a;
  memset(&a, 0, sizeof(a));
  a.p = p; a.PH = PH; a.PW = PW; a.C = C; a.K = K;
  for (int g0 = 0; g0 < G; g0 += SL_CHUNK) {
    const int ng = G - g0 < SL_CHUNK ? G - g0 : SL_CHUNK;
    int blocks = 0;
    for (int g = 0; g < ng; ++g) {
      const int32_t* t0 = windows7 + 7 * (size_t)(g0 + g) * K;
      const int32_t* o = foot + 4 * (size_t)(g0 + g);
      const int nb = fill_acc_group(a.g[g].g, t0, o, K, scene_acc, scene_w);
      a.g[g].flat = (o[0] == 0 ? 1u : 0u) | (o[1] == scene_h[t0[0]] ? 2u : 0u) | (o[2] == 0 ? 4u : 0u) | (o[3] == scene_w[t0[0]] ? 8u : 0u);
      if (nb > blocks) blocks = nb;
    }
    if (blocks == 0) continue;                 // nothing but empty rectangles
    a.first = g0;
    hipLaunchKernelGGL(scene_accumulate_blend, dim3(blocks, ng), dim3(256), 0, st, a);
    RUA_LAUNCH_CHECK("rua_scene_accumulate_blend");
  }
  return RUA_OK;
}

extern "C" int rua_scene_argmax(const int32_t* const* scene_acc, uint8_t* const* scene_pred, const uint8_t* const* scene_cls,
                                const int32_t* scene_h, const int32_t* scene_w, int nscenes, int C, int64_t* confusion, void* stream) {
  const char* fn = "rua_scene_argmax";
  RUA_CHECK_ARG(scene_acc && scene_pred && scene_h && scene_w, "%s: scene_acc, scene_pred, scene_h and scene_w are required", fn);
  RUA_CHECK_ARG(!scene_cls == !confusion, "%s: scene_cls and confusion go together", fn);
  RUA_CHECK_ARG(nscenes >= 1, "%s: nscenes %d (>= 1)", fn, nscenes);
  RUA_CHECK_ARG(C >= 1 && C <= SS_MAXC, "%s: C %d outside 1..64", fn, C);
  RUA_CHECK_ARG(((uintptr_t)confusion & 7) == 0, "%s: confusion must be 8-byte aligned", fn);
  for (int s = 0; s < nscenes; ++s) {
    SC_TRY(check_scene(fn, s, scene_acc[s] && scene_pred[s] && (!scene_cls || scene_cls[s]), scene_h[s], scene_w[s], 4 * C, true));
    RUA_CHECK_ARG(((uintptr_t)scene_acc[s] & 3) == 0, "%s: scene %d: misaligned accumulator", fn, s);
  }
  hipStream_t st = (hipStream_t)stream;
  ArgmaxArgs a;
  memset(&a, 0, sizeof(a));
  a.confusion = reinterpret_cast<unsigned long long*>(confusion);
  a.C = C;
  a.np = SX_LDSW / C < 256 ? SX_LDSW / C : 256;
  for (int s0 = 0; s0 < nscenes; s0 += SX_CHUNK) {
    const int ns = nscenes - s0 < SX_CHUNK ? nscenes - s0 : SX_CHUNK;
    long long most = 0;
    for (int s = 0; s < ns; ++s) {
      a.s[s] = ArgmaxScene{scene_acc[s0 + s], scene_pred[s0 + s], scene_cls ? scene_cls[s0 + s] : nullptr, (long long)scene_h[s0 + s] * scene_w[s0 + s]};
      if (a.s[s].npix > most) most = a.s[s].npix;
    }
    const long long sweeps = (most + a.np - 1) / a.np;
    hipLaunchKernelGGL(scene_argmax, dim3((unsigned)(sweeps < SX_BLOCKS ? sweeps : SX_BLOCKS), ns), dim3(256), scene_cls ? (size_t)C * C * sizeof(uint32_t) : 0, st, a);
    RUA_LAUNCH_CHECK("rua_scene_argmax");
  }
  return RUA_OK;
}

// ---- rua_scene_class_counts: how many pixels of each class lie in each window of a table ------------------------------------------
// counts[n][c] for c < C is the number of pixels equal to c in window n of the class map, counts[n][C] the number of pixels >= C
// (scenes.host_class_counts is the definition).  A symmetry code permutes pixels, so it is checked and otherwise ignored.
//
// A block owns a band of R rows of one window, R the largest with R * np <= 512 where np = (PW + 30) / 16 aligned 16-byte pieces
// cover a row at any byte phase: a lane holds at most SC_KP = 2 pieces, 32 bytes, in registers.  Piece e = tid + 256 m is piece
// e % np of band row e / np, so neighbouring lanes read neighbouring pieces of a scene row (a wave crosses a row end every np
// lanes, never a pitch per lane).  A piece that lies wholly inside the row is one 16-byte load; at the ragged ends a dword that
// lies wholly inside is a dword load and what remains single bytes - nothing outside the window's rows is touched.  Bytes outside
// the row are 0xFF in the register, which equals no class below 64.
//
// Counting is byte-parallel and independent of the content: for a class c the lane XORs its eight dwords with c in every byte
// and counts the NON-zero bytes (((x & 0x7F7F7F7F) + 0x7F7F7F7F) | x has bit 7 of a byte set exactly when the byte is non-zero;
// one popcount per dword), so its matches are 32 minus that.  Two classes share one wave reduction, 16 bits each: a lane has at
// most 32 matches, a wave 2048, so a half cannot carry into the other.  Lane 0 of each wave puts the wave's count into LDS (a cell
// of its own: no LDS atomics), and after one barrier wave 0 adds the four waves' cells - lane c class c -, takes the >= C count as
// the band's pixels minus the sum over the classes, and leaves with at most one 32-bit atomicAdd per (window, class) and block.
// counts is zeroed by a fill launch on the same stream first; the sums are integers, so the order of arrival does not matter.
namespace {

constexpr int SC_CHUNK = 250;                  // windows per launch: 16 bytes each
constexpr int SC_KP = 2;                       // 16-byte pieces per lane
constexpr int SC_MAXC = 64;

struct CountWin { const uint8_t* cls; int W; int pad; };      // cls: at the window's origin
struct CountArgs {
  CountWin w[SC_CHUNK];
  int32_t* counts;                             // of the chunk's first window
  int PH, PW, C, R, np;                        // R: rows per block; np: pieces per row
};
static_assert(sizeof(CountWin) == 16 && sizeof(CountArgs) <= 4096, "kernel arguments are limited to 4 KiB");

__device__ __forceinline__ int sc_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void scene_class_counts(CountArgs a) {
  __shared__ uint32_t part[4 * SC_MAXC];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int PW = a.PW, C = a.C, np = a.np;
  const CountWin& w = a.w[blockIdx.y];
  const int i0 = blockIdx.x * a.R, th = min(a.R, a.PH - i0);
  uint32_t v[SC_KP][4];
#pragma unroll
  for (int m = 0; m < SC_KP; ++m) {
    v[m][0] = v[m][1] = v[m][2] = v[m][3] = 0xFFFFFFFFu;
    const int e = tid + 256 * m, rr = e / np, q = e - rr * np;
    if (rr >= th) continue;
    const uint8_t* row = w.cls + (size_t)(i0 + rr) * w.W;
    const int s = (int)((uintptr_t)row & 15), end = s + PW;             // the row's bytes sit at al + [s, end)
    const uint8_t* al = row - s;
    const int p0 = 16 * q;
    if (p0 >= s && p0 + 16 <= end) {
      const uint4 x = ldg16(al + p0);
      v[m][0] = x.x; v[m][1] = x.y; v[m][2] = x.z; v[m][3] = x.w;
    } else if (p0 + 16 > s && p0 < end) {
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int d0 = p0 + 4 * d, lo = max(d0, s), hi = min(d0 + 4, end);
        if (hi - lo == 4) v[m][d] = *reinterpret_cast<const uint32_t*>(al + d0);
        else for (int k = lo; k < hi; ++k) v[m][d] = (v[m][d] & ~(0xFFu << (8 * (k - d0)))) | ((uint32_t)al[k] << (8 * (k - d0)));
      }
    }
  }
  for (int c = 0; c < C; c += 2) {
    const uint32_t k0 = (uint32_t)c * 0x01010101u, k1 = k0 + 0x01010101u;
    int n0 = 0, n1 = 0;                        // non-zero bytes of v ^ k: the bytes that are NOT the class
#pragma unroll
    for (int m = 0; m < SC_KP; ++m)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t x0 = v[m][d] ^ k0, x1 = v[m][d] ^ k1;
        n0 += __popc((((x0 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x0) & 0x80808080u);
        n1 += __popc((((x1 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x1) & 0x80808080u);
      }
    const int both = sc_wave_sum((16 * SC_KP - n0) | ((16 * SC_KP - n1) << 16));   // a wave: at most 64 * 32 = 2048 per half
    if (lane == 0) {
      part[wv * SC_MAXC + c] = (uint32_t)both & 0xFFFFu;
      if (c + 1 < C) part[wv * SC_MAXC + c + 1] = (uint32_t)both >> 16;
    }
  }
  __syncthreads();
  if (wv == 0) {
    const int t = lane < C ? (int)(part[lane] + part[SC_MAXC + lane] + part[2 * SC_MAXC + lane] + part[3 * SC_MAXC + lane]) : 0;
    const int rest = th * PW - sc_wave_sum(t);                         // the band's pixels with a value >= C
    int32_t* out = a.counts + (size_t)blockIdx.y * (C + 1);
    if (lane < C && t) atomicAdd(out + lane, t);
    if (lane == 0 && rest) atomicAdd(out + C, rest);
  }
}

}  // namespace

extern "C" int rua_scene_class_counts(const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w, int nscenes,
                                      const int32_t* windows, int N, int PH, int PW, int C, int32_t* counts, void* stream) {
  RUA_CHECK_ARG(scene_cls && scene_h && scene_w && windows && counts, "rua_scene_class_counts: scene_cls, scene_h, scene_w, windows and counts are required");
  RUA_CHECK_ARG(nscenes >= 1 && N >= 1, "rua_scene_class_counts: nscenes %d, N %d (both >= 1)", nscenes, N);
  RUA_CHECK_ARG(C >= 1 && C <= SC_MAXC, "rua_scene_class_counts: C %d outside 1..64", C);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= SW_MAXP && PW <= SW_MAXP, "rua_scene_class_counts: PH %d, PW %d (1 <= PH, PW <= 512)", PH, PW);
  RUA_CHECK_ARG(((uintptr_t)counts & 3) == 0, "rua_scene_class_counts: counts must be 4-byte aligned");
  SC_TRY(check_scene_list("rua_scene_class_counts", scene_cls, nullptr, scene_h, scene_w, nscenes, 1));
  SC_TRY(check_window_rows("rua_scene_class_counts", windows, N, PH, PW, scene_h, scene_w, nscenes));
  // the bands add into their window's cells: zeroed here, on the same stream, so the call overwrites
  const int rc = rua_fill_zero(counts, (int64_t)N * (C + 1) * (int64_t)sizeof(int32_t), stream);
  if (rc != RUA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  CountArgs a;
  memset(&a, 0, sizeof(a));
  a.PH = PH; a.PW = PW; a.C = C;
  a.np = (PW + 30) / 16;                                       // pieces that cover a row at any phase: 33 at most
  a.R = 256 * SC_KP / a.np < PH ? 256 * SC_KP / a.np : PH;     // 15 rows at least
  const int bands = (PH + a.R - 1) / a.R;
  for (int k0 = 0; k0 < N; k0 += SC_CHUNK) {
    const int nk = N - k0 < SC_CHUNK ? N - k0 : SC_CHUNK;
    for (int k = 0; k < nk; ++k) {
      const int32_t* t = windows + 4 * (size_t)(k0 + k);
      const int s = t[0];
      a.w[k].cls = scene_cls[s] + (size_t)t[1] * scene_w[s] + t[2];
      a.w[k].W = scene_w[s];
    }
    a.counts = counts + (size_t)k0 * (C + 1);
    hipLaunchKernelGGL(scene_class_counts, dim3(bands, nk), dim3(256), 0, st, a);
    RUA_LAUNCH_CHECK("rua_scene_class_counts");
  }
  return RUA_OK;
}

// ---- rua_scene_erode: the eroded ground truth of whole class maps, and the confusion matrix of a prediction against it -----------
// out[i][j] = 255 if some (dy, dx) with dy^2 + dx^2 <= radius^2 has (i + dy, j + dx) inside the map and a byte there other than
// cls[i][j], else cls[i][j] (scenes.host_erode is the definition; bytes are compared raw and the scene border is no boundary).
// With a prediction map, every pixel whose eroded value t < C and whose pred < C counts into confusion[t][pred].
//
// The disc is scanned in its O(radius) form.  hd(i, j) is the distance along row i to the nearest byte other than cls[i][j]
// (127: none within radius); pixel (i, j) erodes iff for some |dy| <= radius, rows clamped into the map - a clamped row is a row of
// the disc, so clamping adds nothing -, cls[i + dy][j] != cls[i][j] or hd(i + dy, j) <= isqrt(radius^2 - dy^2).
//
// A block owns a tile of SE_TH rows x SE_TW columns of one scene.  It stages the tile's rows plus `radius` rows above and below
// and `radius` columns left and right, as far as they exist, into LDS as bytes: a staged row run may start at any byte (scene
// widths are arbitrary), so it comes in as the ALIGNED 16-byte pieces that cover it, at the same byte phase - single bytes only
// where a piece would reach outside the map.  Columns beyond the scene's left or right border are then filled with the border byte
// (clamping moves an offset towards the centre, so it stays in the disc): the passes below need no border case.
// Both passes work on FOUR neighbouring pixels of a row at once, bytes of one dword.  A dword at any byte of LDS is two aligned
// dwords and a v_alignbyte; "which bytes differ" is an XOR and the carry trick of scene_class_counts; "hd <= limit" is one add
// that carries into bit 7 of a byte.  Pass A: a lane takes four pixels of a staged row and, for d = radius down to 1, the dwords d
// bytes to the left and to the right, and leaves the four hd bytes in a second LDS image.  Pass B: a lane takes four pixels of a
// tile row and walks the 2 radius + 1 rows of its columns through both images; lanes run along a scene row, so pred is read and out
// written as contiguous dwords (single bytes in the ragged last group of a row).  Counts collect in an LDS histogram (a block holds
// SE_TH * SE_TW = 8192 pixels: 32 bits are plenty) and leave with one 64-bit atomicAdd per non-zero cell.
namespace {

constexpr int SE_TH = 32, SE_TW = 256;         // tile: rows x columns
constexpr int SE_MAXR = 16;
constexpr int SE_ROWS = SE_TH + 2 * SE_MAXR;   // staged rows at most
constexpr int SE_LEFT = 16;                    // bytes in front of a row's first piece: room for the left border fill at phase 0
constexpr int SE_NP = (15 + SE_TW + 2 * SE_MAXR + 15) / 16;   // 16-byte pieces that cover a staged run at any phase: 19
constexpr int SE_PITCH = SE_LEFT + SE_NP * 16; // LDS row pitch in bytes: 320
constexpr int SE_NONE = 127;                   // hd of a pixel with no other value within radius
constexpr int SE_CHUNK = 120;                  // scenes per launch: 32 bytes each
constexpr int SE_MAXC = 64;

struct ErodeScene { const uint8_t* cls; const uint8_t* pred; uint8_t* out; int H, W; };
struct ErodeArgs {
  ErodeScene s[SE_CHUNK];
  unsigned long long* confusion;
  int radius, C;
};
static_assert(sizeof(ErodeScene) == 32 && sizeof(ErodeArgs) <= 4096, "kernel arguments are limited to 4 KiB");

typedef uint32_t __attribute__((aligned(1))) se_u32u;           // a dword of four pixels at any byte of a global row

// the four bytes at byte address `at` of an LDS image, `at` of any phase: two aligned dwords, funnelled
__device__ __forceinline__ uint32_t se_ld4(const uint32_t* Td, int at) {
  return __builtin_amdgcn_alignbyte(Td[(at >> 2) + 1], Td[at >> 2], (uint32_t)at & 3u);
}
// bit 7 of every byte of x that is not zero
__device__ __forceinline__ uint32_t se_nz(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
// 0xFF in every byte whose bit 7 is set in m (m has no other bits)
__device__ __forceinline__ uint32_t se_bytes(uint32_t m) { return (m >> 7) * 255u; }

__global__ __launch_bounds__(256) void scene_erode(ErodeArgs a) {
  __shared__ uint4 Tq[SE_ROWS * SE_PITCH / 16 + 1];   // the staged bytes: column jlo of row rr at rr * SE_PITCH + SE_LEFT + phase(rr); one piece of slack
  __shared__ uint32_t Hd[SE_ROWS * SE_TW / 4];        // hd of the staged rows over the tile's columns, four pixels a dword
  __shared__ uint32_t limk[SE_MAXR + 1];              // (127 - isqrt(r^2 - dy^2)) in every byte: hd + limk carries into bit 7 iff hd > limit
  extern __shared__ uint32_t ehist[];                 // C * C cells, only when counting
  uint8_t* Tb = reinterpret_cast<uint8_t*>(Tq);
  const uint32_t* Td = reinterpret_cast<const uint32_t*>(Tq);
  const ErodeScene& sc = a.s[blockIdx.y];
  const int tid = threadIdx.x, r = a.radius, C = a.C, H = sc.H, W = sc.W;
  const int tiles_x = (W + SE_TW - 1) / SE_TW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  if (ty * SE_TH >= H) return;                   // the whole block: a smaller scene of the chunk
  const int i0 = ty * SE_TH, j0 = tx * SE_TW;
  const int th = min(SE_TH, H - i0), tw = min(SE_TW, W - j0), ng = (tw + 3) >> 2;     // ng: groups of four pixels in a tile row
  const int ilo = max(i0 - r, 0), ihi = min(i0 + th + r, H), nrows = ihi - ilo;      // staged rows [ilo, ihi): at most SE_ROWS
  const int jlo = max(j0 - r, 0), jhi = min(j0 + tw + r, W), ncols = jhi - jlo;      // staged columns: at most SE_TW + 2 SE_MAXR
  const bool count = sc.pred != nullptr;
  if (count)
    for (int e = tid; e < C * C; e += 256) ehist[e] = 0u;
  if (tid <= r) {
    int l = 0;
    while ((l + 1) * (l + 1) <= r * r - tid * tid) ++l;
    limk[tid] = (uint32_t)(SE_NONE - l) * 0x01010101u;
  }
  const uint8_t* mend = sc.cls + (size_t)H * W;
  // byte phase of staged row rr, the low four bits of its run's address: (ph0 + rr * W) mod 16
  const int ph0 = (int)(((uintptr_t)sc.cls + (size_t)ilo * W + jlo) & 15), wl = W & 15;
#define SE_COL0(rr) ((rr) * SE_PITCH + SE_LEFT + ((ph0 + (rr) * wl) & 15))     // LDS byte of column jlo of staged row rr
#pragma unroll 1
  for (int e = tid; e < nrows * SE_NP; e += 256) {
    const int rr = e / SE_NP, q = e - rr * SE_NP;
    const uint8_t* row = sc.cls + (size_t)(ilo + rr) * W + jlo;         // the run is bytes [row, row + ncols)
    const int s = (ph0 + rr * wl) & 15;
    if (16 * q >= s + ncols) continue;
    const uint8_t* p = row - s + 16 * q;
    if (p >= sc.cls && p + 16 <= mend) Tq[rr * (SE_PITCH / 16) + 1 + q] = ldg16(p);   // what lies beside the run is the map's own: read, never used
    else for (int k = max(16 * q, s); k < min(16 * q + 16, s + ncols); ++k) Tb[rr * SE_PITCH + SE_LEFT + k] = row[k - s];
  }
  __syncthreads();
  if (jlo == 0 || jhi == W) {                    // the whole block: a tile on the scene's left or right border (r >= 1 inside)
    for (int e = tid; e < nrows * r; e += 256) {
      const int rr = e / r, d = e - rr * r + 1, c0 = SE_COL0(rr);
      if (jlo == 0) Tb[c0 - d] = Tb[c0];
      if (d <= j0 + tw + r - W) Tb[c0 + ncols - 1 + d] = Tb[c0 + ncols - 1];     // the tile's own halo only: at most byte 318 of the row
    }
    __syncthreads();
  }
#pragma unroll 1
  for (int e = tid; e < nrows * ng; e += 256) {
    const int rr = e / ng, k = e - rr * ng;
    const int at = SE_COL0(rr) + (j0 - jlo) + 4 * k;                    // columns j0 + 4k .. + 3; beyond tw: staged bytes of no meaning, never used
    const uint32_t v = se_ld4(Td, at);
    uint32_t h = SE_NONE * 0x01010101u;
#pragma unroll 4
    for (int d = r; d >= 1; --d) {                                      // downwards: the smallest distance is written last
      const uint32_t m = se_bytes(se_nz((se_ld4(Td, at - d) ^ v) | (se_ld4(Td, at + d) ^ v)));
      h = (h & ~m) | (((uint32_t)d * 0x01010101u) & m);
    }
    Hd[rr * (SE_TW / 4) + k] = h;
  }
  __syncthreads();
#pragma unroll 1
  for (int e = tid; e < th * ng; e += 256) {
    const int ti = e / ng, k = e - ti * ng, i = i0 + ti, j = j0 + 4 * k;
    const int off = (j0 - jlo) + 4 * k;
    const uint32_t v = se_ld4(Td, SE_COL0(i - ilo) + off);
    uint32_t er = 0u;                            // bit 7 of a byte: that pixel erodes
#pragma unroll 4
    for (int dy = -r; dy <= r; ++dy) {
      const int rr = min(max(i + dy, 0), H - 1) - ilo;
      const uint32_t u = se_ld4(Td, SE_COL0(rr) + off), h = Hd[rr * (SE_TW / 4) + k];
      er |= se_nz(u ^ v) | (~(h + limk[dy < 0 ? -dy : dy]) & 0x80808080u);
    }
    const uint32_t t4 = v | se_bytes(er);
    const size_t at = (size_t)i * W + j;
    const int np = min(4, tw - 4 * k);           // pixels of this group inside the tile
    uint32_t p4 = 0xFFFFFFFFu;
    if (np == 4) {
      if (sc.out) *reinterpret_cast<se_u32u*>(sc.out + at) = t4;
      if (count) p4 = *reinterpret_cast<const se_u32u*>(sc.pred + at);
    } else {
      for (int b = 0; b < np; ++b) {
        if (sc.out) sc.out[at + b] = (uint8_t)(t4 >> (8 * b));
        if (count) p4 = (p4 & ~(0xFFu << (8 * b))) | ((uint32_t)sc.pred[at + b] << (8 * b));
      }
    }
    if (count) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int t = (t4 >> (8 * b)) & 255, p = (p4 >> (8 * b)) & 255;             // outside the tile: p = 255, no class
        if (t < C && p < C) atomicAdd(&ehist[t * C + p], 1u);
      }
    }
  }
  if (!count) return;
  __syncthreads();
  for (int e = tid; e < C * C; e += 256) {
    const uint32_t n = ehist[e];
    if (n) atomicAdd(a.confusion + e, (unsigned long long)n);
  }
#undef SE_COL0
}

}  // namespace

extern "C" int rua_scene_erode(const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w, int nscenes, int radius,
                               uint8_t* const* scene_out, const uint8_t* const* scene_pred, int C, int64_t* confusion, void* stream) {
  RUA_CHECK_ARG(scene_cls && scene_h && scene_w, "rua_scene_erode: scene_cls, scene_h and scene_w are required");
  RUA_CHECK_ARG(radius >= 0 && radius <= SE_MAXR, "rua_scene_erode: radius %d outside 0..16", radius);
  RUA_CHECK_ARG(nscenes >= 1, "rua_scene_erode: nscenes %d (>= 1)", nscenes);
  RUA_CHECK_ARG(!scene_pred == !confusion, "rua_scene_erode: scene_pred and confusion go together");
  RUA_CHECK_ARG(scene_out || scene_pred, "rua_scene_erode: nothing to do: give scene_out, or scene_pred and confusion, or both");
  if (scene_pred) {
    RUA_CHECK_ARG(C >= 1 && C <= SE_MAXC, "rua_scene_erode: C %d outside 1..64", C);
    RUA_CHECK_ARG(((uintptr_t)confusion & 7) == 0, "rua_scene_erode: confusion must be 8-byte aligned");
  }
  for (int s = 0; s < nscenes; ++s) {
    SC_TRY(check_scene("rua_scene_erode", s, scene_cls[s] && (!scene_out || scene_out[s]) && (!scene_pred || scene_pred[s]), scene_h[s], scene_w[s], 1));
    RUA_CHECK_ARG(!scene_out || scene_out[s] != scene_cls[s], "rua_scene_erode: scene %d: scene_out is scene_cls (an erosion in place would read its own output)", s);
  }
  hipStream_t st = (hipStream_t)stream;
  ErodeArgs a;
  memset(&a, 0, sizeof(a));
  a.confusion = reinterpret_cast<unsigned long long*>(confusion);
  a.radius = radius; a.C = scene_pred ? C : 0;
  for (int s0 = 0; s0 < nscenes; s0 += SE_CHUNK) {
    const int ns = nscenes - s0 < SE_CHUNK ? nscenes - s0 : SE_CHUNK;
    int most = 0;
    for (int k = 0; k < ns; ++k) {
      const int s = s0 + k;
      ErodeScene& e = a.s[k];
      e.cls = scene_cls[s];
      e.pred = scene_pred ? scene_pred[s] : nullptr;
      e.out = scene_out ? scene_out[s] : nullptr;
      e.H = scene_h[s]; e.W = scene_w[s];
      const int tiles = ((e.H + SE_TH - 1) / SE_TH) * ((e.W + SE_TW - 1) / SE_TW);   // below 2^28: H * W < 2^40 and a tile holds 2^13 pixels
      if (tiles > most) most = tiles;
    }
    hipLaunchKernelGGL(scene_erode, dim3(most, ns), dim3(256), scene_pred ? (size_t)C * C * sizeof(uint32_t) : 0, st, a);
    RUA_LAUNCH_CHECK("rua_scene_erode");
  }
  return RUA_OK;
}

// ---- rua_scene_boundary: the boundary pixels of a class map and of a prediction map, and how many of each lie near the other's ---
// bound[i][j] = m[i][j] if m[i][j] < C and a 4-neighbour inside the map holds another byte, else 255 (scenes.host_boundaries): the
// inner boundary of every class, B_c(m) the pixels where it equals c.  counts[c] += (|B_c(pred)|, the pixels of B_c(pred) with a
// pixel of B_c(cls) within `radius`, |B_c(cls)|, the pixels of B_c(cls) with one of B_c(pred) within `radius`): what the boundary
// F1 is a ratio of (scenes.host_boundary_counts is the definition).
//
// A block owns a tile of SB_TH rows x SB_TW columns of one scene and stages both maps with a halo of radius + 1 into LDS, four
// pixels a dword: an unaligned global dword where the four columns lie inside the row, clamped single bytes at the scene's border -
// a clamped neighbour equals its centre, so "outside the map does not exist" needs no case in pass A.  Pass A turns the staged
// bytes into the two boundary images over the tile plus a halo of `radius` (a dword at any byte of LDS is se_ld4; "< C" is one add
// that carries into bit 7); positions outside the map become 255 there, so they match nothing.  Pass B: a lane takes four pixels
// of a tile row as one dword of either boundary image and, row by row outwards (dy = 0, +-1, ..) through the lattice disc, XORs it
// with the OTHER image's dword at that offset; a zero byte under a boundary byte is a match (255 never equals a class byte).  A lane
// leaves the disc as soon as all its boundary pixels are matched - a lane without any never enters it, and a wave of such lanes
// skips it.  Counts collect in an LDS histogram of 4 C cells (a block holds 4096 pixels: 32 bits are plenty) and leave with one
// 64-bit atomicAdd per non-zero cell.  Lanes run along a scene row: the boundary maps leave as contiguous dwords (single bytes in
// the ragged last group of a row).
namespace {

// tests/test_scene_boundary_gpu.py places its class edges, halo matches and scene counts by TILE_H, TILE_W and CHUNK, copies of
// SB_TH, SB_TW and SB_CHUNK: change them together, or those tests stop probing the real tile borders without failing.
constexpr int SB_TH = 32, SB_TW = 128;         // tile: rows x columns
constexpr int SB_MAXR = 16;
constexpr int SB_MAXC = 64;
constexpr int SB_CHUNK = 96;                   // scenes per launch: 40 bytes each

struct BoundScene { const uint8_t* cls; const uint8_t* pred; uint8_t* bcls; uint8_t* bpred; int H, W; };
struct BoundArgs {
  BoundScene s[SB_CHUNK];
  unsigned long long* counts;
  int radius, C;
};
static_assert(sizeof(BoundScene) == 40 && sizeof(BoundArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// LDS row pitch in dwords: the tile's columns plus the halo of radius + 1 on either side, and one dword that se_ld4 may read past a row
__host__ __device__ constexpr int sb_pitch(int r) { return (SB_TW + 2 * (r + 1) + 3) / 4 + 1; }
// dwords of one staged image (one of slack), and of everything: two raw images, two boundary images, the histogram, the disc's half widths
__host__ __device__ constexpr int sb_image(int r) { return (SB_TH + 2 * (r + 1)) * sb_pitch(r) + 1; }
__host__ __device__ constexpr int sb_lds_dwords(int r) { return 4 * sb_image(r) + 4 * SB_MAXC + SB_MAXR + 1; }
static_assert(sb_lds_dwords(SB_MAXR) * 4 <= 65536, "the staged images must fit the LDS a block may have");

// bit 7 of every byte of x that is below c (1 <= c <= 64)
__device__ __forceinline__ uint32_t sb_lt(uint32_t x, int c) { return ~(((x & 0x7F7F7F7Fu) + (uint32_t)(128 - c) * 0x01010101u) | x) & 0x80808080u; }

__global__ __launch_bounds__(256) void scene_boundary(BoundArgs a) {
  extern __shared__ uint32_t bsh[];
  const BoundScene& sc = a.s[blockIdx.y];
  const int tid = threadIdx.x, r = a.radius, R1 = r + 1, C = a.C, H = sc.H, W = sc.W;
  const int tiles_x = (W - 1) / SB_TW + 1;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  if (ty > (H - 1) / SB_TH) return;              // the whole block: a smaller scene of the chunk
  const int i0 = ty * SB_TH, j0 = tx * SB_TW;
  const int th = min(SB_TH, H - i0), tw = min(SB_TW, W - j0), ng = (tw + 3) >> 2;     // ng: groups of four pixels in a tile row
  const int PD = sb_pitch(r), IMG = sb_image(r);
  const int nrows = th + 2 * R1, ncd = (tw + 2 * R1 + 3) >> 2;                        // staged rows, staged dwords of a row (< PD)
  uint32_t* raw[2] = {bsh, bsh + IMG};           // 0: the class map, 1: the prediction; staged (y, x) is scene (i0 - R1 + y, j0 - R1 + x)
  uint32_t* bnd[2] = {bsh + 2 * IMG, bsh + 3 * IMG};
  uint32_t* hist = bsh + 4 * IMG;
  uint32_t* lim = hist + 4 * SB_MAXC;            // lim[d] = isqrt(r^2 - d^2): the disc's half width d rows from its centre
  const bool count = a.counts != nullptr;
  const uint8_t* src[2] = {sc.cls, sc.pred};
  uint8_t* dst[2] = {sc.bcls, sc.bpred};
  const bool need[2] = {count || sc.bcls != nullptr, count || sc.bpred != nullptr};
  if (count) {
    for (int e = tid; e < 4 * C; e += 256) hist[e] = 0u;
    if (tid <= r) {
      int l = 0;
      while ((l + 1) * (l + 1) <= r * r - tid * tid) ++l;
      lim[tid] = (uint32_t)l;
    }
  }
#pragma unroll 1
  for (int e = tid; e < nrows * ncd; e += 256) {
    const int y = e / ncd, xd = e - y * ncd;
    const int i = min(max(i0 - R1 + y, 0), H - 1), jr = 4 * xd - R1;                  // jr: the dword's first column, from j0
    const bool whole = jr >= -j0 && jr + 3 < W - j0;                                  // its four columns exist
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      if (!need[m]) continue;
      const uint8_t* row = src[m] + (size_t)i * W + j0;
      uint32_t v;
      if (whole) v = *reinterpret_cast<const se_u32u*>(row + jr);
      else {
        v = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= (uint32_t)row[min(max(jr + b, -j0), W - 1 - j0)] << (8 * b);
      }
      raw[m][y * PD + xd] = v;
    }
  }
  __syncthreads();
  // Pass A.  The left neighbours of a row's first dword (xd = 0) and the right ones of its last (xd = ncd - 1) come from LDS that
  // nobody staged (the dword before the row, dword ncd <= PD - 1 of it): in bounds, but garbage.  It reaches only the boundary
  // image's byte at staged column 0, R1 left of the tile, and bytes from staged column 4 ncd - 1 >= tw + 2 R1 - 1 on, R1 or more
  // right of it.  Pass B reads columns within r = R1 - 1 of the tile's pixels; the bytes a ragged last group reads beyond that sit
  // under lanes masked to 255, which count nothing.
#pragma unroll 1
  for (int e = tid; e < (nrows - 2) * ncd; e += 256) {
    const int y = 1 + e / ncd, xd = e - (y - 1) * ncd, idx = y * PD + xd;
    const int ir = y - R1, jr = 4 * xd - R1;
    uint32_t exist = 0u;                         // bit 7 of a byte: that position lies inside the map
    if (ir >= -i0 && ir < H - i0) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (jr + b >= -j0 && jr + b < W - j0) exist |= 0x80u << (8 * b);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      if (!need[m]) continue;
      const uint32_t* T = raw[m];
      const uint32_t v = T[idx];
      const uint32_t d = (T[idx - PD] ^ v) | (T[idx + PD] ^ v) | (se_ld4(T, 4 * idx - 1) ^ v) | (se_ld4(T, 4 * idx + 1) ^ v);
      bnd[m][idx] = v | se_bytes(~(se_nz(d) & sb_lt(v, C) & exist) & 0x80808080u);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int e = tid; e < th * ng; e += 256) {
    const int ti = e / ng, k = e - ti * ng;
    const int at0 = 4 * (R1 + ti) * PD + R1 + 4 * k;                                  // LDS byte of the group's first pixel
    const int np = min(4, tw - 4 * k);           // pixels of this group inside the tile
    const size_t at = (size_t)(i0 + ti) * W + j0 + 4 * k;
    uint32_t own[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      if (!need[m]) continue;
      own[m] = se_ld4(bnd[m], at0);
      if (np < 4) own[m] |= 0xFFFFFFFFu << (8 * np);                                  // a ragged group ends at the scene's border: 255 beyond it
      if (dst[m]) {
        if (np == 4) *reinterpret_cast<se_u32u*>(dst[m] + at) = own[m];
        else for (int b = 0; b < np; ++b) dst[m][at + b] = (uint8_t)(own[m] >> (8 * b));
      }
    }
    if (!count) continue;
    const uint32_t isb0 = ~own[0] & 0x80808080u, isb1 = ~own[1] & 0x80808080u;       // bit 7 of a byte: a boundary pixel (a class byte is < 64)
    uint32_t pend0 = isb0, pend1 = isb1;         // ... that has found no match yet
    for (int d = 0; d <= r && (pend0 | pend1); ++d) {
      const int l = (int)lim[d];
      for (int sgn = 0; sgn < (d ? 2 : 1); ++sgn) {
        const int base = at0 + (sgn ? -d : d) * 4 * PD;
        for (int dx = -l; dx <= l; ++dx) {
          pend0 &= se_nz(own[0] ^ se_ld4(bnd[1], base + dx));
          pend1 &= se_nz(own[1] ^ se_ld4(bnd[0], base + dx));
        }
      }
    }
    const uint32_t hit0 = isb0 & ~pend0, hit1 = isb1 & ~pend1;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t bit = 0x80u << (8 * b);
      if (isb1 & bit) {                          // columns of counts: n_pred, m_pred, n_true, m_true
        const int c = (own[1] >> (8 * b)) & 255;
        atomicAdd(&hist[4 * c], 1u);
        if (hit1 & bit) atomicAdd(&hist[4 * c + 1], 1u);
      }
      if (isb0 & bit) {
        const int c = (own[0] >> (8 * b)) & 255;
        atomicAdd(&hist[4 * c + 2], 1u);
        if (hit0 & bit) atomicAdd(&hist[4 * c + 3], 1u);
      }
    }
  }
  if (!count) return;
  __syncthreads();
  for (int e = tid; e < 4 * C; e += 256) {
    const uint32_t n = hist[e];
    if (n) atomicAdd(a.counts + e, (unsigned long long)n);
  }
}

// do the n bytes at p and the n bytes at q share one?
inline bool sb_overlap(const uint8_t* p, const uint8_t* q, int64_t n) {
  return p && q && (uintptr_t)p < (uintptr_t)q + (uint64_t)n && (uintptr_t)q < (uintptr_t)p + (uint64_t)n;
}

// a byte range that a call reads or writes: kind 0 scene_cls, 1 scene_pred, 2 bound_cls, 3 bound_pred (of scene `scene`), 4 counts
struct SbRange { uintptr_t at; uint64_t n; int scene, kind; };
inline void sb_name(char* to, size_t len, const SbRange& x) {
  static const char* const names[] = {"scene_cls", "scene_pred", "bound_cls", "bound_pred"};
  if (x.kind == 4) snprintf(to, len, "counts");
  else snprintf(to, len, "scene %d: %s", x.scene, names[x.kind]);
}

}  // namespace

extern "C" int rua_scene_boundary(const uint8_t* const* scene_cls, const uint8_t* const* scene_pred, const int32_t* scene_h,
                                  const int32_t* scene_w, int nscenes, int radius, int C, uint8_t* const* bound_cls,
                                  uint8_t* const* bound_pred, int64_t* counts, void* stream) {
  RUA_CHECK_ARG(scene_cls && scene_pred && scene_h && scene_w, "rua_scene_boundary: scene_cls, scene_pred, scene_h and scene_w are required");
  RUA_CHECK_ARG(radius >= 0 && radius <= SB_MAXR, "rua_scene_boundary: radius %d outside 0..16", radius);
  RUA_CHECK_ARG(C >= 1 && C <= SB_MAXC, "rua_scene_boundary: C %d outside 1..64", C);
  RUA_CHECK_ARG(nscenes >= 1, "rua_scene_boundary: nscenes %d (>= 1)", nscenes);
  RUA_CHECK_ARG(bound_cls || bound_pred || counts, "rua_scene_boundary: nothing to do: give bound_cls, bound_pred or counts");
  RUA_CHECK_ARG(((uintptr_t)counts & 7) == 0, "rua_scene_boundary: counts must be 8-byte aligned");
  for (int s = 0; s < nscenes; ++s) {
    SC_TRY(check_scene("rua_scene_boundary", s, scene_cls[s] && scene_pred[s] && (!bound_cls || bound_cls[s]) && (!bound_pred || bound_pred[s]),
                       scene_h[s], scene_w[s], 1));
    const int64_t n = (int64_t)scene_h[s] * scene_w[s];
    uint8_t* const bc = bound_cls ? bound_cls[s] : nullptr;
    uint8_t* const bp = bound_pred ? bound_pred[s] : nullptr;
    RUA_CHECK_ARG(!sb_overlap(bc, scene_cls[s], n) && !sb_overlap(bc, scene_pred[s], n), "rua_scene_boundary: scene %d: bound_cls overlaps an input map (the neighbours are read while it is written)", s);
    RUA_CHECK_ARG(!sb_overlap(bp, scene_cls[s], n) && !sb_overlap(bp, scene_pred[s], n), "rua_scene_boundary: scene %d: bound_pred overlaps an input map (the neighbours are read while it is written)", s);
    RUA_CHECK_ARG(!sb_overlap(bc, bp, n), "rua_scene_boundary: scene %d: bound_cls overlaps bound_pred", s);
  }
  // ... and across the scenes of the call: no output (a boundary map, the counts) may share a byte with any input or with another
  // output; inputs may share (one map scored against several).  One sweep over the ranges in address order: a range that starts
  // before the furthest end so far of the other kind - or, for an output, of any kind - overlaps the range that set that end.
  {
    std::vector<SbRange> v;
    v.reserve((size_t)nscenes * 4 + 1);
    for (int s = 0; s < nscenes; ++s) {
      const uint64_t n = (uint64_t)scene_h[s] * (uint64_t)scene_w[s];
      v.push_back({(uintptr_t)scene_cls[s], n, s, 0});
      if (scene_pred[s] != scene_cls[s]) v.push_back({(uintptr_t)scene_pred[s], n, s, 1});
      if (bound_cls) v.push_back({(uintptr_t)bound_cls[s], n, s, 2});
      if (bound_pred) v.push_back({(uintptr_t)bound_pred[s], n, s, 3});
    }
    if (counts) v.push_back({(uintptr_t)counts, (uint64_t)C * 4 * sizeof(int64_t), -1, 4});
    std::sort(v.begin(), v.end(), [](const SbRange& x, const SbRange& y) { return x.at < y.at; });
    const SbRange* far[2] = {nullptr, nullptr};    // the range that ends furthest so far: [0] among the inputs, [1] among the outputs
    for (const SbRange& x : v) {
      const int out = x.kind >= 2;
      for (int k = out ? 0 : 1; k < 2; ++k) {
        const SbRange* f = far[k];
        if (!f || x.at >= f->at + f->n) continue;
        char xs[48], fs[48];
        sb_name(xs, sizeof(xs), x);
        sb_name(fs, sizeof(fs), *f);
        RUA_CHECK_ARG(false, "rua_scene_boundary: %s overlaps %s (an output may share no byte with an input or another output of the call)", xs, fs);
      }
      if (!far[out] || x.at + x.n > far[out]->at + far[out]->n) far[out] = &x;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  BoundArgs a;
  memset(&a, 0, sizeof(a));
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.radius = radius; a.C = C;
  for (int s0 = 0; s0 < nscenes; s0 += SB_CHUNK) {
    const int ns = nscenes - s0 < SB_CHUNK ? nscenes - s0 : SB_CHUNK;
    int most = 0;
    for (int k = 0; k < ns; ++k) {
      const int s = s0 + k;
      BoundScene& e = a.s[k];
      e.cls = scene_cls[s]; e.pred = scene_pred[s];
      e.bcls = bound_cls ? bound_cls[s] : nullptr;
      e.bpred = bound_pred ? bound_pred[s] : nullptr;
      e.H = scene_h[s]; e.W = scene_w[s];
      const int tiles = ((e.H - 1) / SB_TH + 1) * ((e.W - 1) / SB_TW + 1);           // below 2^29: H * W < 2^40 and a tile holds 2^12 pixels
      if (tiles > most) most = tiles;
    }
    hipLaunchKernelGGL(scene_boundary, dim3(most, ns), dim3(256), (size_t)sb_lds_dwords(radius) * sizeof(uint32_t), st, a);
    RUA_LAUNCH_CHECK("rua_scene_boundary");
  }
  return RUA_OK;
}

// Copy-paste augmentation of staged training windows (rua_window_paste, include/rua_hip.h): labelled objects of the resident scenes
// are dropped, hard mask and label together, into the uint8 windows [N][PH][PW][Cin] and class maps [N][PH][PW] the cutting kernels
// left, before rua_window_photometric and rua_multitask_targets read them - so the input and all four heads' targets move together.
// scenes.host_paste is the numpy definition and gives the same bytes.
//
// A paste row R[16] names a window, a scene, an object id of that scene's int32 id map, a symmetry code, the place (top, left) of
// the transformed crop T in the window, the crop rectangle (i0, j0, h, w) of the scene, a 64-bit mask of the destination classes it
// may cover (`onto`, two words) and a flag for destinations that hold no class.  Destination pixel (y, x) inside T has the source
// pixel (i, j) = (i0 + (fr ? h-1-a : a), j0 + (fc ? w-1-b : b)) with (a, b) = (y - top, x - left), swapped under the transposing
// codes 1, 5, 6, 7 (fr, fc: the flips of csrc/scene.hip's Sym); it is pasted iff inst[i][j] == id and its CURRENT class byte d
// - after every earlier row - is allowed: d < C ? bit d of onto : flags & 1.  Rows apply in table order.
//
// One thread owns one destination pixel through ALL rows of its window in a launch: it keeps the class byte in a register, walks
// the rows in order, remembers the source pixel of the last row that pasted and stores once at the end - the image bytes of
// earlier pastes are never needed, only their class bytes are.  Overlapping pastes so need no atomics and no order among blocks.
// A block is one 32 x 32 destination tile of a window that has rows in this launch and skips the rows whose clipped rectangle
// misses its tile; a tile no row reaches ends at once.  A window's rows may straddle two launches: the stream orders them.
//
// The source is gathered directly, under the transposing codes too: a 32 x 32 tile touches at most 32 source rows of 128 bytes of
// ids, every one of them by all 32 lanes of a destination column, so the lines stay in L1 / L2 while the tile is walked, and an
// object is a few thousand pixels - tools/bench_scene_paste.py measures plain against transposing codes (DESIGN.md has the numbers).
//
// The rows travel resolved as kernel arguments, PA_CHUNK per launch; no device-side table, no copy, no synchronisation.
#include "common.h"

namespace {

constexpr int PA_T = 32;                       // tile edge in pixels
constexpr int PA_CHUNK = 48;                   // rows per launch: 64 bytes each, and 8 bytes per window that has some
constexpr int PA_MAXP = 512, PA_MAXC = 16, PA_MAXCLS = 64, PA_MAXOFF = 1024;

struct PasteRow {
  const uint8_t* img; const uint8_t* cls; const int32_t* inst;      // pixel (i0, j0) of the scene: the crop's first
  uint64_t onto;
  int32_t W, id;                               // scene width in pixels; the object
  int16_t top, left, h, w;                     // where T lies in the window; the crop's size
  int16_t y0, y1, x0, x1;                      // T clipped to the window: never empty
  int16_t code, flags;
  int32_t pad;
};
static_assert(sizeof(PasteRow) == 64, "a resolved row is 64 bytes");
struct PasteWin { int32_t window; int16_t first, count; };           // rows first .. first + count - 1 of the launch
struct PasteArgs {
  PasteRow row[PA_CHUNK];
  PasteWin win[PA_CHUNK];
  uint8_t* img; uint8_t* cls;
  int PH, PW, Cin, C;
};
static_assert(sizeof(PasteArgs) <= 4096, "kernel arguments are limited to 4 KiB");

__global__ __launch_bounds__(256) void window_paste(PasteArgs a) {
  const PasteWin wn = a.win[blockIdx.y];
  const int PH = a.PH, PW = a.PW, Cin = a.Cin;
  const int tiles_x = (PW + PA_T - 1) / PA_T;
  const int ty0 = (blockIdx.x / tiles_x) * PA_T, tx0 = (blockIdx.x % tiles_x) * PA_T;
  uint64_t live = 0;                           // the window's rows that reach this tile: block-uniform
  for (int k = 0; k < wn.count; ++k) {
    const PasteRow& r = a.row[wn.first + k];
    if (r.y0 < ty0 + PA_T && r.y1 > ty0 && r.x0 < tx0 + PA_T && r.x1 > tx0) live |= 1ull << k;
  }
  if (!live) return;
  const int x = tx0 + (threadIdx.x & 31);
  if (x >= PW) return;
  const size_t wpix = (size_t)wn.window * PH * PW;
  uint8_t* wimg = a.img + wpix * Cin;
  uint8_t* wcls = a.cls + wpix;
  const int yend = min(ty0 + PA_T, PH);
  for (int y = ty0 + (threadIdx.x >> 5); y < yend; y += 8) {
    const size_t px = (size_t)y * PW + x;
    int d = wcls[px];
    const uint8_t* from = nullptr;
    for (uint64_t m = live; m; m &= m - 1) {
      const PasteRow& r = a.row[wn.first + __builtin_ctzll(m)];
      if (y < r.y0 || y >= r.y1 || x < r.x0 || x >= r.x1) continue;
      const bool allowed = d < a.C ? (r.onto >> d) & 1 : r.flags & 1;
      if (!allowed) continue;
      const int code = r.code, u = y - r.top, v = x - r.left;
      const bool tr = code == 1 || code >= 5, fr = code == 2 || code == 3 || code == 5 || code == 7,
                 fc = code == 1 || code == 2 || code == 4 || code == 7;
      const int sa = tr ? v : u, sb = tr ? u : v;
      const size_t sp = (size_t)(fr ? r.h - 1 - sa : sa) * r.W + (fc ? r.w - 1 - sb : sb);
      if (r.inst[sp] != r.id) continue;
      d = r.cls[sp];
      from = r.img + sp * Cin;
    }
    if (from) {
      uint8_t* to = wimg + px * Cin;
      for (int c = 0; c < Cin; ++c) to[c] = from[c];
      wcls[px] = (uint8_t)d;
    }
  }
}

}  // namespace

extern "C" int rua_window_paste(uint8_t* img, uint8_t* cls, int N, int PH, int PW, int Cin, int num_classes,
                                const uint8_t* const* scene_img, const uint8_t* const* scene_cls, const int32_t* const* scene_inst,
                                const int32_t* scene_h, const int32_t* scene_w, int nscenes, const int32_t* pastes, int M, void* stream) {
  const char* fn = "rua_window_paste";
  RUA_CHECK_ARG(img && cls, "%s: img and cls are required", fn);
  RUA_CHECK_ARG(N >= 1, "%s: N %d (>= 1)", fn, N);
  RUA_CHECK_ARG(Cin >= 1 && Cin <= PA_MAXC, "%s: Cin %d outside 1..16", fn, Cin);
  RUA_CHECK_ARG(PH >= 1 && PW >= 1 && PH <= PA_MAXP && PW <= PA_MAXP, "%s: PH %d, PW %d (1 <= PH, PW <= 512)", fn, PH, PW);
  RUA_CHECK_ARG(num_classes >= 1 && num_classes <= PA_MAXCLS, "%s: C %d outside 1..64", fn, num_classes);
  const int64_t total = (int64_t)PH * PW * Cin * N;
  RUA_CHECK_ARG(total < ((int64_t)1 << 31), "%s: N*PH*PW*Cin is %lld (must stay below 2^31)", fn, (long long)total);
  RUA_CHECK_ARG(M >= 0, "%s: M %d (>= 0)", fn, M);
  if (M == 0) return RUA_OK;
  RUA_CHECK_ARG(scene_img && scene_cls && scene_inst && scene_h && scene_w && pastes,
                "%s: scene_img, scene_cls, scene_inst, scene_h, scene_w and pastes are required", fn);
  RUA_CHECK_ARG(nscenes >= 1, "%s: nscenes %d (>= 1)", fn, nscenes);
  for (int s = 0; s < nscenes; ++s) {
    RUA_CHECK_ARG(scene_img[s] && scene_cls[s] && scene_inst[s], "%s: scene %d: null pointer", fn, s);
    RUA_CHECK_ARG(scene_h[s] >= 1 && scene_w[s] >= 1 && (int64_t)scene_h[s] * scene_w[s] * Cin < ((int64_t)1 << 40),
                  "%s: scene %d: size %d x %d", fn, s, scene_h[s], scene_w[s]);
  }
  for (int k = 0; k < M; ++k) {
    const int32_t* R = pastes + 16 * (size_t)k;
    RUA_CHECK_ARG(R[0] >= 0 && R[0] < N, "%s: row %d: word 0: window %d outside 0..%d", fn, k, R[0], N - 1);
    RUA_CHECK_ARG(k == 0 || R[0] >= R[-16], "%s: row %d: word 0: window %d after window %d (rows are sorted by window)", fn, k, R[0], k ? R[-16] : 0);
    RUA_CHECK_ARG(R[1] >= 0 && R[1] < nscenes, "%s: row %d: word 1: scene %d outside 0..%d", fn, k, R[1], nscenes - 1);
    RUA_CHECK_ARG(R[2] >= 0, "%s: row %d: word 2: id %d is negative", fn, k, R[2]);
    RUA_CHECK_ARG(R[3] >= 0 && R[3] <= 7, "%s: row %d: word 3: code %d outside 0..7", fn, k, R[3]);
    RUA_CHECK_ARG(R[4] >= -PA_MAXOFF && R[4] <= PA_MAXOFF, "%s: row %d: word 4: top %d outside -1024..1024", fn, k, R[4]);
    RUA_CHECK_ARG(R[5] >= -PA_MAXOFF && R[5] <= PA_MAXOFF, "%s: row %d: word 5: left %d outside -1024..1024", fn, k, R[5]);
    RUA_CHECK_ARG(R[8] >= 1 && R[8] <= PA_MAXP, "%s: row %d: word 8: h %d outside 1..512", fn, k, R[8]);
    RUA_CHECK_ARG(R[9] >= 1 && R[9] <= PA_MAXP, "%s: row %d: word 9: w %d outside 1..512", fn, k, R[9]);
    const int H = scene_h[R[1]], W = scene_w[R[1]];
    RUA_CHECK_ARG(R[6] >= 0 && (int64_t)R[6] + R[8] <= H, "%s: row %d: word 6: rows %d + %d leave the %d x %d scene", fn, k, R[6], R[8], H, W);
    RUA_CHECK_ARG(R[7] >= 0 && (int64_t)R[7] + R[9] <= W, "%s: row %d: word 7: columns %d + %d leave the %d x %d scene", fn, k, R[7], R[9], H, W);
    RUA_CHECK_ARG(R[12] == 0 || R[12] == 1, "%s: row %d: word 12: flags %d (0, or 1: paste over pixels of no class)", fn, k, R[12]);
    for (int q = 13; q < 16; ++q) RUA_CHECK_ARG(R[q] == 0, "%s: row %d: word %d: reserved, must be 0, got %d", fn, k, q, R[q]);
  }
  hipStream_t st = (hipStream_t)stream;
  const int tiles = ((PH + PA_T - 1) / PA_T) * ((PW + PA_T - 1) / PA_T);
  PasteArgs a;
  memset(&a, 0, sizeof(a));
  a.img = img; a.cls = cls; a.PH = PH; a.PW = PW; a.Cin = Cin; a.C = num_classes;
  int nr = 0, nw = 0;
  for (int k = 0; k <= M; ++k) {
    if (k == M || nr == PA_CHUNK) {            // a full launch, or the last one
      if (nr) {
        hipLaunchKernelGGL(window_paste, dim3(tiles, nw), dim3(256), 0, st, a);
        RUA_LAUNCH_CHECK(fn);
      }
      nr = nw = 0;
      if (k == M) break;
    }
    const int32_t* R = pastes + 16 * (size_t)k;
    const bool tr = R[3] == 1 || R[3] >= 5;
    const int th = tr ? R[9] : R[8], tw = tr ? R[8] : R[9];
    const int y0 = R[4] > 0 ? R[4] : 0, y1 = R[4] + th < PH ? R[4] + th : PH;
    const int x0 = R[5] > 0 ? R[5] : 0, x1 = R[5] + tw < PW ? R[5] + tw : PW;
    if (y0 >= y1 || x0 >= x1) continue;        // wholly outside its window: nothing to do
    PasteRow& r = a.row[nr];
    const int s = R[1];
    const size_t px = (size_t)R[6] * scene_w[s] + R[7];
    r.img = scene_img[s] + px * Cin; r.cls = scene_cls[s] + px; r.inst = scene_inst[s] + px;
    r.onto = (uint64_t)(uint32_t)R[10] | ((uint64_t)(uint32_t)R[11] << 32);
    r.W = scene_w[s]; r.id = R[2];
    r.top = (int16_t)R[4]; r.left = (int16_t)R[5]; r.h = (int16_t)R[8]; r.w = (int16_t)R[9];
    r.y0 = (int16_t)y0; r.y1 = (int16_t)y1; r.x0 = (int16_t)x0; r.x1 = (int16_t)x1;
    r.code = (int16_t)R[3]; r.flags = (int16_t)R[12]; r.pad = 0;
    if (nw && a.win[nw - 1].window == R[0]) ++a.win[nw - 1].count;
    else { a.win[nw].window = R[0]; a.win[nw].first = (int16_t)nr; a.win[nw].count = 1; ++nw; }
    ++nr;
  }
  return RUA_OK;
}

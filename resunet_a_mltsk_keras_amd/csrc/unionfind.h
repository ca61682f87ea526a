// The union-find forest of regions.hip and sweep.hip, and the argument checks both share.  A forest over pixel indices in which a
// parent is never larger than its child: parent[x] <= x, always.  A link only ever points a root to a SMALLER index (atomicMin), so
// the root of a set is its smallest member whatever the order the unions arrive in, and every walk and every retry strictly lowers
// an index, so it ends (the argument stands beside each loop).  Loads of a parent that another block may be lowering are relaxed
// device-scope atomics; a stale parent is still an ancestor of the same set (parents only ever move towards the root), so a walk
// that read one merely takes a step more, and the atomicMin that ends a union reports the truth.
#pragma once
#include "common.h"
#include <algorithm>
#include <vector>

namespace {

// ---- the forest in LDS (a tile) ---------------------------------------------------------------------------------------------------
// The root of x.  P[y] <= y for every y, so each step goes to a strictly smaller index: at most x steps.
__device__ __forceinline__ int lds_find(const int* P, int x) {
  for (;;) {
    const int q = __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (q == x) return x;
    x = q;
  }
}
// Join the sets of a and b.  With a > b the two roots, atomicMin(P[a], b) links a below b if a still was a root (it returns a); if
// not, a had meanwhile been given the parent `old` < a and now points to min(old, b), and what remains is to join old and b.  The
// larger of the two indices in hand is strictly smaller in every retry (old < a and b < a), so the loop ends.
__device__ __forceinline__ void lds_union(int* P, int a, int b) {
  for (;;) {
    a = lds_find(P, a);
    b = lds_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b);
    if (old == a) return;
    a = old;
  }
}

// ---- the same forest in global memory (a scene) -----------------------------------------------------------------------------------
__device__ __forceinline__ int g_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// parent[y] <= y for every y - the tile kernels write it so and atomicMin only lowers -, so each step goes to a strictly smaller
// index: at most x steps.  A stale parent is an earlier one: larger, and still above the root.
__device__ __forceinline__ int g_find(const int32_t* P, int x) {
  for (;;) {
    const int q = g_load(P + x);
    if (q == x) return x;
    x = q;
  }
}
// as lds_union: the larger index in hand strictly falls with every retry
__device__ __forceinline__ void g_union(int32_t* P, int a, int b) {
  for (;;) {
    a = g_find(P, a);
    b = g_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b);
    if (old == a) return;
    a = old;
  }
}

// Bit x of the result: column x of this lane's tile row starts a run (brk of the lane that holds it).  All 64 lanes call it; a
// wave holds two tile rows of 32 pixels, the lane's own is the half its bit 5 names.
__device__ __forceinline__ uint32_t row_breaks(bool brk) {
  const unsigned long long m = __ballot(brk);
  return (uint32_t)(m >> (threadIdx.x & 32));
}

// ---- a block scan ------------------------------------------------------------------------------------------------------------------
// exclusive prefix of v over the 256 lanes of the block (sh: 256 cells), and the total; every lane calls it
template <typename T>
__device__ __forceinline__ T block_scan_256(T* sh, T v, T& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {            // eight doubling steps
    const T u = t >= d ? sh[t - d] : T(0);
    __syncthreads();
    sh[t] += u;
    __syncthreads();
  }
  total = sh[255];
  const T incl = sh[t];
  __syncthreads();
  return incl - v;
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------
#define RG_TRY(call) do { const int rc_ = (call); if (rc_ != RUA_OK) return rc_; } while (0)

int rg_check_size(const char* fn, int s, int h, int w) {
  RUA_CHECK_ARG(h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31),
                "%s: scene %d: size %d x %d (H * W < 2^31: a label is an int32 pixel index)", fn, s, h, w);
  return RUA_OK;
}

// a byte range that a call reads (out == false) or writes
struct RgRange { uintptr_t at; uint64_t n; int scene; const char* name; bool out; };

// No output may share a byte with an input or with another output; inputs may share.  One sweep over the ranges in address order:
// a range that starts before the furthest end so far of the other kind - or, for an output, of either kind - overlaps the range
// that set that end.
int rg_check_overlap(const char* fn, std::vector<RgRange>& v) {
  std::sort(v.begin(), v.end(), [](const RgRange& x, const RgRange& y) { return x.at < y.at; });
  const RgRange* far[2] = {nullptr, nullptr};    // the range that ends furthest so far: [0] among the inputs, [1] among the outputs
  for (const RgRange& x : v) {
    for (int k = x.out ? 0 : 1; k < 2; ++k) {
      const RgRange* f = far[k];
      if (!f || x.at >= f->at + f->n) continue;
      char xs[48], fs[48];
      if (x.scene < 0) snprintf(xs, sizeof(xs), "%s", x.name); else snprintf(xs, sizeof(xs), "scene %d: %s", x.scene, x.name);
      if (f->scene < 0) snprintf(fs, sizeof(fs), "%s", f->name); else snprintf(fs, sizeof(fs), "scene %d: %s", f->scene, f->name);
      RUA_CHECK_ARG(false, "%s: %s overlaps %s (an output may share no byte with an input or another output of the call)", fn, xs, fs);
    }
    if (!far[x.out] || x.at + x.n > far[x.out]->at + far[x.out]->n) far[x.out] = &x;
  }
  return RUA_OK;
}

}  // namespace

// wgrad_rowsx<MODE> (round 5; included by conv_wgrad.hip): the whole-row all-taps weight gradient with its rows dealt as ONE stream.
//   MODE 0: C = Cout = 128 on 64-pixel rows (the level-3 ResBlock, model2.py:105-106; its input is a materialised BatchNorm output: no normalise-on-load);
//   MODE 1: C = Cout = 256 on 32-pixel rows (the level-4 ResBlock at 32 x 32, model2.py:107-108; was wgrad_dmap: 128 x 128 tiles per TAP, 22 - 26 us per 9.66 GFLOP).
// A block owns whole rows, 128 input channels and a SLICE of 64 output channels: 12 waves = 3 kernel rows x 4 input-channel quarters, six accumulators (2 output-channel
// halves x 3 tap columns), 24 MFMAs per wave and stage; the input rows (64 pixels x 256 B) and the slice of the dy rows (64 x 128 B, gathered from the wider pixels by
// the DMA's per-lane source address) stream through one shared ring, one barrier per stage.  256-byte pixels put all four pixel rows of a transposing read on ONE bank
// group: the 16-byte chunks are XOR-swizzled with bits 0 - 1 of the pixel index (chunk ^ (p & 3) << 2), the 128-byte dy pixels with bit 1 (as wgrad_rows64).
// The round-4 form of MODE 0 walked (chain, segment) JOBS: a chain is the rows h = r, r + d, ... of one image (there the dilated 3x3 is a plain 3x3 over a sliding window
// of three rows), and every job drained the ring, refilled three rows and started again.  At d = 15 a chain of a 64-row image has 4 - 5 rows, of a 32-row image 2 - 3: the
// fill costs more than the work, and whole chains dealt to blocks do not divide evenly (d = 3 at level 3: 24 chains for 42 blocks).  Here the rows of all images
// and chains form one sequence of SLOTS - per chain its rows and one separator (a row of zeros: the bottom neighbour of the chain's last row and the top
// neighbour of the next chain's first) -, block b of gx owns slots [U b / gx, U (b + 1) / gx) and streams them through the ring without ever draining it: one
// barrier per slot, a separator costs a barrier and its (out-of-range, zero-filling) DMA issue and no MFMA.  Three cursors (row being fetched, dy row being
// fetched, row being multiplied) step through (image, chain, position) with scalar compares; the two divisions of a slot -> cursor decode run once per block.
// MODE 1: a stage is the same row of TWO images (n, n + N / 2; the K dimension of the product is pixels, so the two rows are just 64 pixels of K): slot layout
// [32 pixels of A | 16 zero | 32 pixels of B | 16 zero] - the 96 pixels of a MODE 0 slot (64 + the 32-pixel zero pad), shifts up to 16 pixels stay inside the zeros - and a block owns
// 64 output channels x 128 INPUT channels (grid.y = 4 slices x 2 halves; the 256-byte half pixels are gathered from the 512-byte pixels by the DMA's per-lane source
// address, like the 128-byte dy slices): 24 MFMAs per wave and stage on 10 transposing reads per six, as at level 3.  Partials [output-channel 32][block][9][32][C]
// (the two input-channel halves fill disjoint columns of the same partial) and wgrad_taps_reduce, unchanged.
template <int MODE>
__device__ __forceinline__ void wgrad_rowsx_body(const WgtK& p, int ysel) {
  constexpr int CC = MODE ? 256 : 128;                  // channels of both operands
  constexpr int NW = 12, PXB = 256, DPB = 128;          // LDS: 128 input channels and 64 output channels per pixel
  constexpr int SRCPX = CC * 2;                         // bytes per pixel in HBM
  constexpr int RW = MODE ? 32 : 64;                    // pixels per image row
  constexpr int BOFF = 48;                              // MODE 1: slot pixel of the second image's row
  constexpr int SLOT = 96 * PXB, DSLOT = 64 * DPB, R = 5, RD = 3, PADPX = 32;
  constexpr int NPX = 16, KDMA = 2;                     // 1-KiB DMA pieces: 16 of the input row(s) (4 pixels each), 8 of the dy slice row(s) (8 pixels each); 2 per wave
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sX = smem + PADPX * PXB;               // slot 0 (the 8 KiB in front of it: zeros for row pixels < 0)
  unsigned char* sDy = sX + R * SLOT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = wv >> 2, ciq = wv & 3;
  const int slice = MODE ? (ysel >> 1) : ysel, cih = MODE ? (ysel & 1) : 0;
  const int H = p.H, d = p.dil;
  const int NP = MODE ? (p.N >> 1) : p.N;               // units of the slot stream: images (MODE 0) or pairs of images
  const int nyb = (H + d - 1) / d, R1 = H - (nyb - 1) * d;     // chains r < R1 have nyb rows, the others nyb - 1
  const int per = H + d;                                // slots per unit: its rows + one separator per chain
  const long long U = (long long)NP * per;
  const int u0 = (int)(U * (long long)blockIdx.x / p.gx), u1 = (int)(U * (long long)(blockIdx.x + 1) / p.gx);
  const int n = u1 - u0;

  for (int i = tid; i < (PADPX * PXB + R * SLOT) / 16; i += NW * 64)      // every pad is zero and stays zero: the DMAs write row pixels only
    *reinterpret_cast<uint4*>(smem + (size_t)i * 16) = make_uint4(0, 0, 0, 0);
  __syncthreads();

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.a, p.abytes), rd = make_rsrc(p.dy, p.dybytes);
  const unsigned sx_a = (unsigned)(size_t)(lds_void_p)sX, sd_a = (unsigned)(size_t)(lds_void_p)sDy;
  // x piece: lane l sits at pixel (l >> 4), chunk (l & 15) of the piece's four pixels and fetches chunk (l & 15) ^ ((pixel & 3) << 2) of that pixel's 256-byte half
  const unsigned srel_x = (unsigned)((lane >> 4) * SRCPX + cih * PXB + (((lane & 15) ^ ((lane >> 4) << 2)) * 16));
  // dy piece: lane l sits at pixel (l >> 3), chunk (l & 7) of the piece's eight 128-byte slice pixels
  const unsigned srel_d = (unsigned)((lane >> 3) * SRCPX + slice * DPB + (((lane & 7) ^ (((lane >> 4) & 1) << 2)) * 16));
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

  struct Cur { int p, r, i; };                           // unit, chain, position in the chain (i == rows of the chain: its separator)
  auto rows_of = [&](int r) { return nyb - (r >= R1 ? 1 : 0); };
  auto decode = [&](int u) {
    Cur c;
    if (u < 0) { c.p = -1; c.r = d - 1; c.i = rows_of(d - 1); return c; }      // the separator in front of slot 0
    c.p = u / per;
    int rem = u - c.p * per;
    const int big = R1 * (nyb + 1);
    if (rem < big) { c.r = rem / (nyb + 1); c.i = rem - c.r * (nyb + 1); }
    else { rem -= big; const int q = rem / nyb; c.r = R1 + q; c.i = rem - q * nyb; }
    return c;
  };
  auto adv = [&](Cur& c) { if (++c.i > rows_of(c.r)) { c.i = 0; if (++c.r == d) { c.r = 0; ++c.p; } } };
  auto is_row = [&](const Cur& c) { return c.p >= 0 && c.p < NP && c.i < rows_of(c.r); };
  const unsigned rowbytes = (unsigned)(RW * SRCPX);
  auto issue = [&](const Cur& cx, bool xen, int xring, const Cur& cd, bool den, int dring) {
    const bool xv = xen && is_row(cx), dv = den && is_row(cd);
    const unsigned xa_ = xv ? (unsigned)(cx.p * H + cx.r + cx.i * d) * rowbytes : OOB;
    const unsigned da_ = dv ? (unsigned)(cd.p * H + cd.r + cd.i * d) * rowbytes : OOB;
    const unsigned xb_ = (MODE && xv) ? (unsigned)((cx.p + NP) * H + cx.r + cx.i * d) * rowbytes : OOB;
    const unsigned db_ = (MODE && dv) ? (unsigned)((cd.p + NP) * H + cd.r + cd.i * d) * rowbytes : OOB;
    unsigned char* xs = sX + xring * SLOT;
    unsigned char* ds = sDy + dring * DSLOT;
#pragma unroll
    for (int k = 0; k < KDMA; ++k) {
      const int pi = k * NW + wv;                        // k = 0: input pieces 0 .. 11; k = 1: input pieces 12 .. 15 (waves 0 - 3), dy pieces 0 .. 7 (waves 4 - 11)
      if (pi < NPX) {
        if constexpr (MODE) {
          const int half = pi >> 3, q = pi & 7;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(xs + half * BOFF * PXB + q * 1024), 16, ((half ? xb_ : xa_) + (unsigned)(q * 4 * SRCPX)) + srel_x, 0, 0, 0);
        } else {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_p)(xs + pi * 1024), 16, (xa_ + (unsigned)(pi * 4 * SRCPX)) + srel_x, 0, 0, 0);
        }
      } else {
        const int pj = pi - NPX;
        if constexpr (MODE) {
          const int half = pj >> 2, q = pj & 3;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_void_p)(ds + pj * 1024), 16, ((half ? db_ : da_) + (unsigned)(q * 8 * SRCPX)) + srel_d, 0, 0, 0);
        } else {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_void_p)(ds + pj * 1024), 16, (da_ + (unsigned)(pj * 8 * SRCPX)) + srel_d, 0, 0, 0);
        }
      }
    }
  };

  f32x16 acc[6];                                         // [output-channel half of the slice][tap column]
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  struct Frags { s16x4 d0[2], d1[2], x0[3], x1[3]; };
  auto read_frags = [&](unsigned da, unsigned xa, int ks, Frags& f) {
    const int xk = ks * 16 * PXB + ((MODE && ks >= 2) ? (BOFF - 32) * PXB : 0);      // k-steps 2, 3: the second image's pixels
    const unsigned dk0 = da + (unsigned)(dyo0 + ks * 16 * DPB), dk1 = dk0 ^ 64u;
    const unsigned xk0 = (unsigned)((int)xa + xo0 + xk), xk1 = (unsigned)((int)xa + xo1 + xk), xk2 = (unsigned)((int)xa + xo2 + xk);
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

  if (n > 0) {
    Cur cx = decode(u0 - 1), cd = decode(u0), cc = cd;
    // input rows u0 - 1 .. u0 + 2 into ring slots 0 .. 3, dy rows u0, u0 + 1 into dy slots 0, 1 (rows behind the block's range are not fetched: slot u's product
    // reads input rows u - 1 .. u + 1 and dy row u)
    // (every wave issues KDMA pieces per call, so that one counted wait serves every stage: a call without a dy row zero-fills dy slot 2, which is first filled in stage 0)
    issue(cx, true, 0, cd, false, 2); adv(cx);
    issue(cx, true, 1, cd, true, 0); adv(cx); adv(cd);
    issue(cx, 1 <= n, 2, cd, 1 < n, 1); adv(cx); adv(cd);
    issue(cx, 2 <= n, 3, cd, false, 2); adv(cx);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int xi = 4, di = 2, xc = ty, dc = 0;                 // ring positions: next input slot / dy slot to fill, this wave's input slot (row it - 1 + ty) / the dy slot of row it
    for (int it = 0; it < n; ++it) {
      __builtin_amdgcn_s_barrier();                     // input row it + 1 and dy row it have landed, for everyone; everyone is done with row it - 2 and dy row it - 1
      issue(cx, it + 3 <= n, xi, cd, it + 2 < n, di); adv(cx); adv(cd);
      xi = xi == R - 1 ? 0 : xi + 1; di = di == RD - 1 ? 0 : di + 1;
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KDMA) : "memory");          // this wave's pieces of input row it + 2 and dy row it + 1 are done
      // this wave's kernel row reads input row (slot - 1 + ty): the chain's first row has no upper neighbour, its last no lower one - those products are zeros
      // (at d = 15 a third of a level-4 member's), and a wave that skips them leaves its SIMD to the two waves of the other kernel rows
      const bool mine = ty == 1 || (ty == 0 ? cc.i > 0 : cc.i + 1 < rows_of(cc.r));
      if (is_row(cc) && mine) {
        const unsigned da = sd_a + (unsigned)(dc * DSLOT);
        const unsigned xa = sx_a + (unsigned)(xc * SLOT);
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
      adv(cc);
      xc = xc == R - 1 ? 0 : xc + 1; dc = dc == RD - 1 ? 0 : dc + 1;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float* part = p.scratch + (size_t)((2 * slice + h) * p.gx + (int)blockIdx.x) * 9 * 32 * CC;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        part[((ty * 3 + j) * 32 + co) * CC + cih * 128 + ciq * 32 + (lane & 31)] = acc[h * 3 + j][i];
      }
  }
}
template <int MODE> __global__ __launch_bounds__(768) void wgrad_rowsx(const WgtK p) { wgrad_rowsx_body<MODE>(p, (int)blockIdx.y); }
template <int MODE> __global__ __launch_bounds__(768) void wgrad_rowsx_g(const WgtKG g) {       // blockIdx.z = member, blockIdx.y = (output-channel slice, input-channel half)
  const WgtK& p = g.k[blockIdx.z];
  if ((int)blockIdx.x >= p.gx) return;
  wgrad_rowsx_body<MODE>(p, (int)blockIdx.y);
}

/* librua_hip.so — C ABI of the MI355X (gfx950) ResUnet-a training-path kernels.
 *
 * The reference (thimabru1010/ResUnet-a_mltsk_keras) has NO native/FFI interface: its hot
 * path is the list of Keras layer call sites that TensorFlow executes.  Every entry point
 * below therefore cites the reference call site(s) (file:line under /root/reference) whose
 * arithmetic it replaces.  All tensors are channels-last (NHWC, the reference's own layout,
 * train_ISPRS.py:73-92) in device memory owned by the caller; `dtype` selects the storage
 * type of activations (RUA_F32 or RUA_BF16); accumulation is always fp32 (statistics fp64).
 * Every function returns 0 on success or a negative code (text via rua_last_error()), takes
 * the HIP stream as its last argument (`void*` = hipStream_t), allocates nothing and keeps no
 * global state besides the opt-in tuning switches (rua_set_tuning).  Nothing here depends on PyTorch.
 */
#ifndef RUA_HIP_H
#define RUA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RUA_F32 0
#define RUA_BF16 1
#define RUA_MAX_SEG 6
#define RUA_MAX_BRANCH 4
#define RUA_MAX_WGRAD_BATCH 32  /* members of one grid of the batched form of rua_conv_wgrad_group (rua_wgrad_desc.batch): a whole step's small weight gradients */
#define RUA_MAX_WGRAD_GROUP 8   /* members of one rua_conv_wgrad_group call (both convolutions of every branch of a ResBlock) */

#define RUA_OK 0
#define RUA_ERR_ARG (-1)      /* shape/alignment precondition violated */
#define RUA_ERR_LAUNCH (-2)   /* HIP launch error */

int rua_version(void);
const char* rua_last_error(void);
int rua_device_info(int* cu_count, int* lds_bytes, char* arch, int arch_len);

/* ---- segmented implicit-GEMM convolution (MFMA) --------------------------------------
 * y[n,h,w,co] = sum over segments s, taps t, channels c of
 *               src_s[n, (h*stride+dy_t*dil_s)>>up_s, (w*stride+dx_t*dil_s)>>up_s, c] * w_s[t][co][c]
 * Replaces: KL.Conv2D 3x3 dilated 'same' (model2.py:19-24), 1x1 / strided 1x1 (:101-111),
 * Concatenate+Conv2D of PSPPooling/combine (:73-78,:83-85) with the concat never
 * materialised, UpSampling2D-nearest folded into the read (:55-60,:91), the n-ary Add of the
 * ResBlock (:27-31) as the `aux` residual, and — with transposed/flipped weights — the
 * data-gradient of all of them.  Channel counts must be multiples of 8 (bf16) / 4 (f32). */
typedef struct rua_conv_seg {
  const void* x;       /* source activations [N][Hs][Ws][C] */
  const void* w;       /* weights [taps][Cout][C], same dtype as activations */
  int32_t C, Hs, Ws;
  int32_t up_shift;    /* nearest upsample by 2^up_shift folded into the read */
  int32_t dil;         /* dilation of the 3x3 taps */
  int32_t taps;        /* 1 or 9 */
} rua_conv_seg;

/* model2.py:17-24 BatchNormalization in training mode, folded into the consuming convolution (rua_conv_desc.in_fold) */
typedef struct rua_bn_fold {
  const double* stats;          /* [replicas][2][C] fp64: sum x, sum x^2 of the conv input, complete when the conv starts */
  int32_t replicas, pad;
  double count, bessel_n;       /* elements per channel; count for the unbiased moving variance (count if no replication) */
  float eps, momentum;
  const float* gamma; const float* beta;
  float* moving_mean; float* moving_var;         /* updated once per call (NULL: not) */
  float* scale; float* shift; float* mean; float* rstd;   /* published by one workgroup for later kernels (NULL mean / rstd: not) */
} rua_bn_fold;

typedef struct rua_conv_desc {
  rua_conv_seg seg[RUA_MAX_SEG];
  int32_t nseg;
  int32_t N, H, W, Cout;       /* logical output grid (GEMM rows = N*H*W) */
  int32_t stride;              /* input coordinate = output coordinate * stride */
  int32_t dtype;
  const float* bias;           /* [Cout] or NULL */
  const void* aux;             /* [N][H][W][Cout] or NULL */
  int32_t aux_mode;            /* 0 none, 1 y += aux (residual), 2 y *= (mscale*aux+mshift > 0) (ReLU mask), 3 statistics only */
  const float* mscale;         /* per-channel, NULL => 1 */
  const float* mshift;         /* per-channel, NULL => 0 */
  int32_t out_relu;
  int32_t accumulate;          /* y += result instead of y = result */
  void* y;                     /* [N][OH][OW][Cout], written at (h*out_stride, w*out_stride) */
  int32_t out_stride, OH, OW;
  double* stats;               /* [stats_replicas][2][Cout] atomically accumulated, or NULL */
  int32_t stats_mode;          /* 1: sum v, sum v^2   2: sum v, sum v*aux */
  void* workspace;             /* optional fp32 scratch, >= 2 * rua_conv_workspace_bytes() + 4096: enables split-K for small
                                  output grids (one N*H*W*Cout slab per K slice, plain stores, summed in a fixed order:
                                  deterministic).  The LAST 4096 bytes are reserved for the tile ticket counters of the
                                  optional in-launch reduction (RUA_DMAP_FUSED_FINISH=1): zero them once (e.g. allocate
                                  the workspace zero-filled); every call leaves them zero.  The rest: contents on entry
                                  irrelevant, undefined on return */
  int64_t workspace_bytes;
  int32_t stats_replicas;      /* power of two >= 1: block b adds into replica b % R (spreads atomic contention);
                                  the finalize kernels sum the replicas */
  const float* bias_more[3];   /* further [Cout] bias vectors (or NULL) added after `bias`, in this order: the branch-final convs
                                  of a ResBlock run as ONE concatenated conv whose bias is the sum of the branches' biases */
  /* Normalise on load (model2.py:17-24: BatchNormalization -> ReLU -> Conv2D): segment 0 is read as
   * [relu](in_scale[c] * x + in_shift[c]) - applied as the tile lands in LDS, zero padding stays zero - so the normalised
   * copy of the conv input never exists in HBM.  NULL: plain read.  Only where rua_conv_fused_input_ok() says 1. */
  const float* in_scale;
  const float* in_shift;
  int32_t in_relu;
  int32_t pad_fold;
  /* Training-mode BatchNorm whose coefficients the CONSUMER derives itself (no coefficient launch between the producer of the
   * statistics and this convolution): every workgroup sums the replicated fp64 statistics of the input in its prologue, one
   * designated workgroup publishes scale / shift / mean / rstd (ReLU masks, backward) and updates the moving statistics.
   * Non-NULL: in_scale / in_shift must be NULL; in_relu applies.  Same shapes as in_scale (rua_conv_fused_input_ok). */
  const struct rua_bn_fold* in_fold;
} rua_conv_desc;
int rua_conv_fwd(const rua_conv_desc* d, void* stream);
/* n (<= RUA_MAX_BRANCH) INDEPENDENT convolutions - the dilation branches of a ResBlock (model2.py:26-31) - with the results of n
 * rua_conv_fwd calls; members that land on the same kernel are issued as ONE grid (no drain / launch gap between the branches).
 * Every member is planned before anything is launched: a group with a rejected member returns its error, launches nothing and
 * leaves nothing behind (the thread's ..._last_* values keep what the call before left). */
int rua_conv_fwd_group(const rua_conv_desc* d, int n, void* stream);
int rua_conv_group_last_grids(void);             /* grids the calling thread's latest rua_conv_fwd_group issued (1: all members in one) */
/* C = Cout = 64, 3x3, bf16, W % 128 == 0, H % 4 == 0: the members run as ONE conv_band64m launch (row streaming, 4-row bands, every
 * member normalised on load by its own in_fold / in_scale, its own bias / ReLU mask / statistics epilogue) - the only path on which
 * normalise-on-load is served at 64 channels.  rua_conv_group_band_ok asks without launching; ..._last_band reports the last call. */
int rua_conv_group_band_ok(const rua_conv_desc* d, int n);
int rua_conv_group_last_band(void);
/* Members on conv_dmap (bf16, Cout >= 128, C % 64 == 0, no K split) with the same tiles run BACK TO BACK inside one grid (conv_dmap_chain:
 * a block walks every member over its pixel tile, the LDS-DMA ring never drains between members); ..._last_chain = how many did (0: none). */
int rua_conv_group_last_chain(void);
/* The n-ary Add of a ResBlock (model2.py:26-31: out = x_input + sum of the branches) with the sum kept ON CHIP: n (<= RUA_MAX_BRANCH)
 * single-segment convolutions into the SAME output y = aux_0 + sum_i conv_i - the results of n rua_conv_fwd calls of which member 0
 * writes (accumulate 0, optional residual aux_mode 1) and members i > 0 accumulate (accumulate 1, no aux).  Every member carries its
 * own normalise-on-load (in_fold, or in_scale / in_shift, + in_relu: the same kind for all members) and bias.  Where the shape allows
 * (bf16, C = Cout = 32, 3x3, dilation <= 32, W % 128 == 0, H % 8 == 0, >= 65536 pixels, no statistics / output ReLU) this is ONE
 * launch of conv_band32 that writes y once; otherwise the members are launched one by one (same results). */
int rua_conv_fwd_sum(const rua_conv_desc* d, int n, void* stream);
int rua_conv_sum_last_kernel(void);              /* the calling thread's latest rua_conv_fwd_sum: 1 one conv_band32 launch, 2 one conv_band64 launch (C = Cout = 64,
                                                    W % 128 == 0, H % 4 == 0), 0 member by member */
int rua_conv_sum_kernel(const rua_conv_desc* d, int n);   /* the same answer for a set of members, without launching anything */
int rua_conv_smem_bytes(const rua_conv_desc* d);
int64_t rua_conv_workspace_bytes(const rua_conv_desc* d);   /* bytes of ONE slab (N*H*W*Cout fp32); split-K uses up to 32 */
/* profiling only (bench.py): timing events without the system-scope release a default event performs when recorded */
void* rua_prof_event_create(void);
int rua_prof_event_record(void* ev, void* hip_stream);
int rua_prof_event_elapsed_us(void* start, void* stop, double* us);   /* waits for `stop` */
void rua_prof_event_destroy(void* ev);
void rua_profile_mid_event(void* hip_event);
int rua_profile_mid_event_fired(void);          /* 1 if the call made since the event was armed recorded it (had a second launch) */    /* profiling only: the calling thread's NEXT two-launch call (split-K conv, all-taps weight
                                                   gradient) records this hipEvent_t between its main kernel and its second launch; one shot */
int rua_conv_last_ksplit(void);                  /* K slices of the calling thread's latest rua_conv_fwd (1: single pass, no finisher) */
int rua_conv_tile_bn(const rua_conv_desc* d);   /* 32 / 64 / 128 and */
int rua_conv_kernel_id(const rua_conv_desc* d); /* 0: conv_igemm (register-staged), 1: conv_dma (LDS-DMA, bf16), 2: conv_dmap (LDS-DMA, pipelined across the stage barrier),
                                                   3: conv_halo (input + halo resident in LDS), 4: conv_pw (narrow 1x1, per-wave streaming),
                                                   5: conv_strip (row-streaming 3x3 at C = Cout = 32, BatchNorm + ReLU applied on load) */
int rua_conv_fused_input_ok(const rua_conv_desc* d);   /* 1: this shape runs on a kernel that honours in_scale / in_shift / in_relu */
int rua_conv_tile_bm(const rua_conv_desc* d);   /* 128 / 256: which conv_igemm<T,BM,BN> instantiation a descriptor launches */
/* What rua_conv_fwd(d) / rua_conv_fwd_group(d, n) would launch, computed by the planner the launch itself runs - nothing is launched, no pointer is followed
 * (but in_fold, which is part of the descriptor), no device is needed (the chip then counts as 256 CUs).  The descriptors are validated as for the launch. */
typedef struct rua_conv_launch_info {
  int32_t kernel_id;    /* rua_conv_kernel_id of the first member (-1: the whole group is one conv_band64m / conv_band128m launch, see band) */
  int32_t form;         /* which instantiation of that kernel: its row in the library's kernel table (-1: a launcher of conv_band*.hip takes the call) */
  int32_t grid_x, grid_y, block, lds_bytes;   /* blocks (grid_y: members side by side in a grouped grid), threads per block, dynamic LDS */
  int32_t bm, bn;       /* tile of kernel ids 0 - 2 (pixel rows x output channels; rua_conv_tile_bm / _bn), else 0 */
  int32_t ksplit;       /* K slices (rua_conv_last_ksplit after the launch) */
  int32_t finisher;     /* 1: a conv_splitk_finish launch follows */
  int32_t members;      /* bit i: member i of the group is in this launch (rua_conv_plan: 1) */
  int32_t band, chain;  /* rua_conv_group_plan: what rua_conv_group_last_band / _last_chain report after the call, in every entry */
} rua_conv_launch_info;
int rua_conv_plan(const rua_conv_desc* d, rua_conv_launch_info* out);
/* the launches of rua_conv_fwd_group(d, n) in issue order: out[0 .. *n_out - 1] (room for n entries); *n_out = rua_conv_group_last_grids after the call */
int rua_conv_group_plan(const rua_conv_desc* d, int n, rua_conv_launch_info* out, int* n_out);

/* ---- weight gradient (MFMA, split over pixels, fp32 atomic accumulation) ----------------
 * dW[t][co][c] += sum_pixels dy[n,h,w,co] * a[n, h*stride+dy_t*dil, w*stride+dx_t*dil, c]
 * Replaces the kernel-gradient of every KL.Conv2D above (Keras autodiff inside
 * train_on_batch, train_ISPRS.py:131,148). */
typedef struct rua_wgrad_desc {
  const void* a;  int32_t C, Hs, Ws;        /* conv input  [N][Hs][Ws][C]  */
  const void* dy; int32_t Cout, H, W;       /* out-gradient [N][H][W][Cout] */
  int32_t N, stride, dil, taps, dtype;
  float* dw;                                /* [taps][Cout][C] fp32, accumulated */
  void* workspace;                          /* optional fp32 scratch of rua_wgrad_workspace_bytes(): enables the all-taps kernel of */
  int64_t workspace_bytes;                  /* the two top levels (C = Cout in {32,64}, 3x3, W % 64 == 0, bf16; uses the front of it,
                                               contents on entry irrelevant) and the per-wave kernel of the narrow 1x1 convolutions
                                               (taps 1, C * Cout <= 4096, bf16), whose replica accumulators and ticket counters are the
                                               LAST 264 KiB (16 * 16 KiB + 8 KiB): zero them once before the first call, every call
                                               leaves them zero.  One workspace per concurrently running stream. */
  /* Normalise on load, as in rua_conv_desc: a is read as [relu](in_scale[c] * a + in_shift[c]), zero padding stays zero.
   * Only the all-taps kernel honours it (rua_wgrad_kind() == 1); other shapes reject a non-NULL in_scale. */
  const float* in_scale;
  const float* in_shift;
  int32_t in_relu;
  /* Deferred reduction: with defer != 0 a call whose kernel leaves partial sums (the all-taps block partials, the K slices'
   * slabs) does NOT launch its reduction; `workspace` must then stay untouched until rua_wgrad_reduce_batch has consumed the
   * record rua_wgrad_plan() returns for this descriptor (one workspace per deferred call; size: rua_wgrad_workspace_bytes). */
  int32_t defer;
  /* Members of a rua_conv_wgrad_group call: how many weight gradients share the launch (0 / 1: this one alone).  The all-taps
   * kernel sizes its persistent grid for a share of the chip - one round of blocks for the whole group, 1 / group_members of the
   * block partials to write and to reduce.  Set it on every member (rua_wgrad_plan must see the same value as the launch). */
  int32_t group_members;
  /* batch != 0: a member of the BATCHED form of rua_conv_wgrad_group - unequal weight gradients of the generic bf16 tile kernel (rua_wgrad_kind() == 0,
   * rua_wgrad_img_kind() == 0) in one compact grid that shares ONE block budget: the member's K split depends on the whole call, so its pending record comes
   * from rua_wgrad_group_plan over the same descriptors, not from rua_wgrad_plan.  Ignored by rua_conv_wgrad and by groups with other members. */
  int32_t batch;
  /* overwrite_dev (optional): a DEVICE int32 read when the kernel runs.  Non-zero: the caller guarantees that dw holds zeros and that this call is its only
   * writer before it is read (the step's gradient arena: zeroed by the optimizer, every weight has one producer) - kernels that end in a read-modify-write of dw
   * (one K slice per element, the slab / block-partial reductions) then STORE instead: dw = sum, one pass over dw spared.  Zero / NULL: dw += sum (gradient
   * accumulation over several backward passes).  A device flag, so that a captured step and an eager accumulating pass can share one recorded plan.  Kernels that
   * add with atomics or replicas ignore it; the result is the same either way. */
  const int32_t* overwrite_dev;
} rua_wgrad_desc;
typedef struct rua_wgrad_pending {
  int32_t kind;                /* 0: nothing to reduce (single writer / wgrad_pw), 1: all-taps partials, 2: K-slice slabs,
                                  3 (built by the caller): partials = replicated fp64 statistics [parts][2][n], dw[c] += sum of slot 0
                                  (what rua_stats_to_f32 does: bias gradients), blocks = ceil(n / 256) */
  int32_t parts;               /* partial buffers to sum (blocks of the all-taps kernel per output-channel half / K slices) */
  int64_t n;                   /* elements of dW */
  const float* partials;
  float* dw;
  int32_t CC;                  /* kind 1: channels */
  int32_t blocks;              /* 256-thread blocks the reduction of this record takes */
  int32_t block_begin, pad;    /* filled by the caller: first block of this record in the batched launch (prefix sum of `blocks`) */
  const int32_t* overwrite_dev; /* as rua_wgrad_desc.overwrite_dev (copied from the descriptor by rua_wgrad_plan) */
} rua_wgrad_pending;
/* the record a deferred rua_conv_wgrad(d) leaves behind - computed without launching anything */
int rua_wgrad_plan(const rua_wgrad_desc* d, rua_wgrad_pending* out);
/* dw += partial sums for every record, in ONE launch, each in its fixed order (bit-reproducible): items in device memory, sorted by
 * block_begin, total_blocks = sum of their `blocks` */
int rua_wgrad_reduce_batch(const rua_wgrad_pending* items_dev, int n_items, int total_blocks, void* stream);
int rua_conv_wgrad(const rua_wgrad_desc* d, void* stream);
/* n (<= RUA_MAX_WGRAD_GROUP; the batched form below: more) INDEPENDENT weight gradients - the dilation branches of a ResBlock (model2.py:26-31), first and second convolutions - with the results of n
 * rua_conv_wgrad calls; members on the same kernel run as ONE grid.  Members must not share dw or partial-sum workspace (a group
 * that does runs member by member). */
int rua_conv_wgrad_group(const rua_wgrad_desc* d, int n, void* stream);
int rua_wgrad_group_last_grids(void);            /* grids the calling thread's latest rua_conv_wgrad_group issued */
/* The batched form: when EVERY member has rua_wgrad_desc.batch set, is bf16 and lands on the generic tile kernel, the call takes any number of members (up to
 * 4 * RUA_MAX_WGRAD_BATCH) and issues ceil(n / RUA_MAX_WGRAD_BATCH) grids (consecutive members, in the caller's order, share a grid).  A grid is exactly the sum
 * of its members' blocks, the longest blocks first; a block finds its member from prefix sums in the kernel arguments.  The grid has one block budget (tuning
 * key wgrad_batch_blocks, 0 = 4 per CU) dealt by work: member i asks for budget * stages_i / sum_j(stages_j * tiles_j) K slices (stages: 64-pixel steps of its K
 * range, tiles: 64 x 64 tiles of its dW), at least 1, at most its stages and the fp32 slabs its workspace holds.  A member left with one slice writes dW itself
 * (honouring overwrite_dev); the others leave slabs: summed by the call, or - defer - by rua_wgrad_reduce_batch from the records of rua_wgrad_group_plan.
 * Bit 5 of the tuning key wgrad_group: every member keeps the K split it would take alone - the batch is then bit-identical to n rua_conv_wgrad calls; without
 * it (the default) the results differ by the order of the fp32 sums only, and stay deterministic.  Members whose slabs overlap run one by one.
 * rua_wgrad_group_plan: out[i] = the record member i of rua_conv_wgrad_group(d, n) leaves (kind 0: none); for calls that do not take the batched form it is
 * rua_wgrad_plan per member. */
int rua_wgrad_group_plan(const rua_wgrad_desc* d, int n, rua_wgrad_pending* out);
int64_t rua_wgrad_workspace_bytes(const rua_wgrad_desc* d);
int rua_wgrad_kind(const rua_wgrad_desc* d);   /* 0: generic tiled kernel, 1: all-taps kernel + deterministic partial reduce,
                                                  2: wgrad_dmap (wide levels), 3: wgrad_pw (narrow 1x1) */
int rua_wgrad_img_kind(const rua_wgrad_desc* d);   /* within kind 0: the whole-image kernels of the 8 x 8 / 16 x 16 levels (3x3, dilation 1, bf16, channels % 64 == 0 - % 32 for wgrad_imgs -,
                                                      N H W % 512 == 0): 1 wgrad_img (64 x 64 tiles of dW, 512-pixel chunks as K slices), 2 wgrad_imgs (more than 512 pixels and at
                                                      least half as many 32 x 32 tiles as CUs: the chunks streamed by one block, no K slices), 0 the generic tiles */

/* Master fp32 weights [taps][Cout][C] -> activation-dtype copies: forward layout (same) and
 * data-gradient layout [taps reversed][C][Cout].  One launch for the whole parameter table. */
typedef struct rua_wprep_item { int64_t src_off, dst_off; int32_t taps, Cout, C, pad; } rua_wprep_item;
int rua_weight_prep(const float* master, void* w_fwd, void* w_dgrad, const rua_wprep_item* items_dev,
                    int n_items, int max_elems, int dtype, void* stream);
/* The data-gradient layout alone from the forward-layout bf16 copy (dtype must be RUA_BF16; items as for rua_weight_prep, dst_off = the offset in both copies):
 * used when the optimizer has just written that copy itself (rua_adam_step_w / rua_sgd_step_w with wcopy_bf16 = the forward copy, whose index space
 * must then be the master's: dst_off == src_off). */
int rua_weight_prep_dgrad(const void* w_fwd, void* w_dgrad, const rua_wprep_item* items_dev, int n_items, int max_elems, const int32_t* blockmap_dev,
                          int n_blocks, int dtype, void* stream);
/* blockmap_dev (optional, NULL: a (<= 256, n_items) grid like rua_weight_prep's): int32 [n_blocks][2] = (item, first tile) - item i contributes
 * rua_wprep_blocks(taps, Cout, C) consecutive entries whose first tiles are 0, 8, 16, ...: the grid is as long as the tensors are large. */
int rua_wprep_blocks(int taps, int Cout, int C);

/* ---- few-channel 1x1 convolutions (VALU; the stem and the heads) -------------------------
 * stem: KL.Conv2D(32,(1,1)) on the 3/6/7-band input (model2.py:101).  x fp32 [M][Cin<=16]. */
int rua_stem_fwd(const float* x, const float* w, const float* b, void* y, int64_t M, int Cin, int Cout, int dtype, void* stream);
/* rua_stem_fwd with the per-channel statistics of its output in the epilogue: stats [replicas][2][Cout] fp64 (sum, sum of squares of y as stored;
 * zeroed by the caller) - what rua_col_stats would compute from y in a pass of its own (the first BatchNorm of the encoder, model2.py:102-103). */
int rua_stem_fwd_stats(const float* x, const float* w, const float* b, void* y, int64_t M, int Cin, int Cout, int dtype, double* stats, int replicas, void* stream);
int rua_stem_bwd(const float* x, const void* dy, float* dw, float* db, int64_t M, int Cin, int Cout, int dtype, void* stream);
/* rua_stem_fwd(_stats) that also writes the input once more as bf16 xpack [M][16] = { hi(x_0..x_7) | lo(x_0..x_6), 1 } (hi = bf16(x), lo = bf16(x - hi); Cin <= 7;
 * stats may be NULL): with it the stem's weight gradient is a 1x1 weight gradient on the matrix pipe - rua_conv_wgrad(a = xpack, C = 16, dy, dw = tmp [Cout][16],
 * tmp zero) - followed by rua_stem_bwd_fold: dW[co][c] += tmp[co][c] + tmp[co][8 + c], db[co] += tmp[co][15] (NULL: not), tmp := 0.  The vector form
 * (rua_stem_bwd) keeps 72 partial sums per thread and ended every block in their butterflies and 288 same-address atomics: 38 us for a 46 MB pass. */
int rua_stem_fwd_pack(const float* x, const float* w, const float* b, void* y, int64_t M, int Cin, int Cout, int dtype, double* stats, int replicas,
                      void* xpack, void* stream);
int rua_stem_bwd_fold(float* tmp, float* dw, float* db, int Cin, int Cout, void* stream);
/* heads: Conv2D(num_classes,(1,1)) + softmax / sigmoid (model2.py:145-146,160-162,169-171,181-183,186-188).
 * act: 0 none, 1 softmax over channels, 2 sigmoid.  z (logits) and p are fp32 [M][Cout<=8]. */
int rua_head_fwd(const void* x, const float* w, const float* b, float* z, float* p, int64_t M, int Cin, int Cout, int act, int dtype, void* stream);
/* rua_head_fwd with the loss moments of its output in the epilogue (the probabilities are in registers): tanimoto_sums
 * [B][Cout][6] fp64 as rua_tanimoto_sums accumulates them against the labels y [B*HW][Cout] (NULL: not), metrics[5] fp64 as
 * rua_seg_metrics (NULL: not); both zeroed by the caller.  Replaces those passes over p (train_ISPRS.py:456-461). */
int rua_head_fwd_loss(const void* x, const float* w, const float* b, float* z, float* p, const float* y, double* tanimoto_sums,
                      double* metrics, int B, int64_t HW, int Cin, int Cout, int act, int dtype, void* stream);
/* the same with tanimoto_sums kept in sums_replicas (1..64) copies, [sums_replicas][B][Cout][6]: a block adds into ONE of them, so ~64 blocks of a sample
 * do not queue up on the same 36 addresses at the end of the launch; rua_tanimoto_finalize_rep adds the copies. */
int rua_head_fwd_loss_rep(const void* x, const float* w, const float* b, float* z, float* p, const float* y, double* tanimoto_sums,
                          int sums_replicas, double* metrics, int B, int64_t HW, int Cin, int Cout, int act, int dtype, void* stream);
/* scratch (optional, >= 1024*(Cout*Cin+Cout)*4 bytes): per-block partials + fixed-order reduce instead of fp32 atomics.
 * mask_dx: x is the output of a fused ReLU (the heads' 3x3 conv + relu, model2.py:153-158): dx *= (x > 0), i.e. the ReLU's
 * backward is applied here instead of in a pass of its own */
int rua_head_bwd(const void* x, const float* dz, const float* w, void* dx, int accumulate_dx, float* dw, float* db,
                 float* scratch, int64_t scratch_bytes, int64_t M, int Cin, int Cout, int dtype, int mask_dx, void* stream);
/* the same with dxsum (fp32 [Cin], +=, optional): the per-channel sums of the values written to dx - the bias gradient of the convolution that produced x
 * where dx is its output's complete gradient (the 3x3 + ReLU convs in front of the heads: model2.py:153-171) - taken in the same pass */
int rua_head_bwd_sums(const void* x, const float* dz, const float* w, void* dx, int accumulate_dx, float* dw, float* db, float* dxsum,
                      float* scratch, int64_t scratch_bytes, int64_t M, int Cin, int Cout, int dtype, int mask_dx, void* stream);

/* ---- BatchNormalization (model2.py:17,21,38,86,93; Keras eps 1e-3, momentum .99) -------- */
/* per-channel sum / sum of squares over all rows of x [M][C] -> stats[R][2][C] (fp64, accumulated over R replicas) */
int rua_col_stats(const void* x, int64_t M, int C, double* stats, int replicas, int dtype, void* stream);
/* replicas to use for a statistics buffer fed by a kernel of `blocks` workgroups */
int rua_stats_replicas(int64_t blocks);
/* sum g*m and sum g*m*x with m = (mscale*x+mshift > 0) when masked, else 1 */
int rua_col_stats2(const void* g, const void* x, const float* mscale, const float* mshift, int masked,
                   int64_t M, int C, double* stats, int replicas, int dtype, void* stream);
/* training: stats -> scale/shift (+ mean, rstd, moving-stat update with the Bessel factor
 * bessel_n/(bessel_n-1), bessel_n = element count Keras sees, i.e. after nearest upsampling);
 * inference: moving stats -> scale/shift */
int rua_bn_finalize(const double* stats, int replicas, double count, double bessel_n, const float* gamma, const float* beta,
                    float* moving_mean, float* moving_var, float momentum, float eps, int training,
                    float* scale, float* shift, float* mean, float* rstd, int C, void* stream);
/* dst_i[c] += (float)stats[c] for n (<=4) fp32 vectors: bias gradients from per-channel sums of dy */
int rua_stats_to_f32(const double* stats, int replicas, int C, float* const* dst, int n, void* stream);
/* out_b = [relu](scale_b * x + shift_b) for b < nb (all branches of a ResBlock read x once) */
int rua_bn_apply(const void* x, int nb, const float* const* scale, const float* const* shift, int relu,
                 void* const* out, int64_t M, int C, int dtype, void* stream);
/* backward statistics -> dgamma += , dbeta += , and the coefficients A,B,Cc of dx = A*g + B*x + Cc */
int rua_bn_bwd_finalize(const double* stats2, int replicas, double count, const float* gamma, const float* mean, const float* rstd,
                        float* dgamma, float* dbeta, float* coefA, float* coefB, float* coefC, int C, void* stream);
/* dx (=|+=) [dskip] + sum_b (A_b * g_b * m_b + B_b * x + C_b),  m_b = ReLU mask of branch b (or 1) */
int rua_bn_bwd_apply(int nb, const void* const* g, const float* const* coefA, const float* const* coefB,
                     const float* const* coefC, const float* const* mscale, const float* const* mshift, int masked,
                     const void* x, const void* dskip, void* dx, int accumulate, int64_t M, int C, int dtype, void* stream);

/* Fused forms (one launch each; the engine uses these): statistics -> coefficients in every block's prologue, block 0
 * publishes scale/shift/mean/rstd, updates the moving statistics (forward) or adds dgamma/dbeta (backward). */
typedef struct rua_bn_branch {
  const float* gamma; const float* beta; float* moving_mean; float* moving_var;   /* [C] */
  float* scale; float* shift; float* mean; float* rstd;                           /* [C] published coefficients */
  void* out;                                                                      /* [M][C]; NULL in EVERY branch: coefficients only
                                                                                     (one block, nothing applied: the consumer
                                                                                     normalises on load, rua_conv_desc.in_scale) */
  const double* stats; int32_t replicas, pad;                                     /* this branch's own statistics (else the shared ones) */
  double* out_stats;   /* optional [2][C] (training, relu == 0 only): per-channel sum / sum of squares of THIS BatchNorm's output, written by block 0 from the
                          coefficients - sum = count * beta, sum of squares = count * (beta^2 + gamma^2 var / (var + eps)) exactly, so a BatchNorm that
                          follows (the first BatchNorms of the next ResBlock: model2.py:17 behind model2.py:86) needs no statistics pass over the tensor */
} rua_bn_branch;
typedef struct rua_bn_fwd_desc {
  const void* x; int64_t M; int32_t C, dtype, nb, relu, training, replicas;
  const double* stats;                       /* [replicas][2][C], shared by all branches (they normalise the same x) */
  double count, bessel_n; float momentum, eps;
  rua_bn_branch br[RUA_MAX_BRANCH];
} rua_bn_fwd_desc;
int rua_bn_fwd(const rua_bn_fwd_desc* d, void* stream);
/* n (<= RUA_MAX_BRANCH) independent one-branch BatchNorm applications of equal channel count (any pixel counts) as ONE grid (the results of n rua_bn_fwd calls; members that
 * cannot share a grid are launched one by one).  Tuning key bn_bwd_group switches both this and rua_bn_bwd_group. */
int rua_bn_fwd_group(const rua_bn_fwd_desc* d, int n, void* stream);
int rua_bn_fwd_group_last_grids(void);
typedef struct rua_bn_bwd_branch {
  const void* g; const double* stats2; int32_t replicas;
  int32_t stats2_out;   /* 1: slot 1 of stats2 is sum g * OUT (this BatchNorm's output, no ReLU: what rua_bn_bwd_desc.dx_stats of the launch that wrote g
                           provides) instead of sum g * x; the kernel converts with x = (out - shift) / scale (scale, shift must be set) */
  const float* gamma; const float* mean; const float* rstd; const float* scale; const float* shift;
  float* dgamma; float* dbeta;
} rua_bn_bwd_branch;
typedef struct rua_bn_bwd_desc {
  const void* x; const void* dskip; void* dx; int64_t M; int32_t C, dtype, nb, masked, accumulate, pad; double count;
  rua_bn_bwd_branch br[RUA_MAX_BRANCH];
  double* skip_stats;          /* optional [skip_replicas][2][C]: per-channel sum of dskip added into slot 0 (the bias gradient of */
  int32_t skip_replicas, pad2; /* the convs whose output the skip tensor is the gradient of: model2.py:27-31) - saves a pass over dskip */
  double* dx_stats;            /* optional [dx_replicas][2][C]: per-channel sum of the values written to dx added into slot 0 - the bias gradient of the */
  int32_t dx_replicas, pad3;   /* convolution that produced x (the stride-2 1x1 convs in front of the encoder ResBlocks: model2.py:103-111), without a pass over dx;
                                  slot 1 += sum dx * x: with stats2_out the statistics of the BatchNorm backward of the BatchNorm that produced x (model2.py:86) */
} rua_bn_bwd_desc;
int rua_bn_bwd(const rua_bn_bwd_desc* d, void* stream);
/* n (<= RUA_MAX_BRANCH) independent one-branch BatchNorm backwards of equal channel count (any pixel counts) - the second BatchNorms of a
 * ResBlock's dilation branches (model2.py:21-22), the branch BatchNorms of a PSPPooling (model2.py:56-66), each with its own gradient, input and output - as ONE grid (the results of n rua_bn_bwd calls; members
 * that cannot share a grid - several branches, skip statistics, unequal shapes - are launched one by one).  ..._last_grids: 1 or n. */
int rua_bn_bwd_group(const rua_bn_bwd_desc* d, int n, void* stream);
int rua_bn_bwd_group_last_grids(void);
/* The form a fused BatchNorm launch takes, from the descriptor alone (no device needed, nothing launched): 0 = pixel-major (blocks cut the tensor along
 * pixels, every block derives every channel's coefficients), else S | P << 8 = channel-sliced (small maps: a block owns S 16-byte pieces per pixel - S = 8 is one
 * 128-byte line - of one of P contiguous pixel parts, rua_bn_part_range, and derives its own S * 8 bf16 / S * 4 fp32 channels only).  P never exceeds the replica
 * count of a statistics output (skip_stats, dx_stats), so each address receives one add and the sums are reproducible bit for bit.  out and dx are bit-identical
 * between the forms; tuning key bn_sliced = 0 keeps every launch pixel-major.  A group is sliced when every member's own route is; each member keeps its own P. */
int rua_bn_fwd_route(const rua_bn_fwd_desc* d);
int rua_bn_bwd_route(const rua_bn_bwd_desc* d);
int rua_bn_part_range(int64_t M, int P, int part, int64_t* begin, int64_t* end);   /* pixels [begin, end) of part 0 <= part < P <= M */

/* ---- pooling / resampling (PSPPooling model2.py:47-60; decoder model2.py:91) ---------- */
/* The max-pool (rua_maxpool_fwd, and rua_maxpool_derive with the same results) scans its window row-major with `v > best` from -inf: the FIRST maximum wins
 * (-0.0 and +0.0 tie), NaN never wins, and a window that holds only NaN and / or -inf yields -inf with argmax byte 0 - so rua_maxpool_bwd / _bwd_multi route
 * the gradient of such a window to its position 0. */
int rua_maxpool_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, int k, int dtype, void* stream);
int rua_maxpool_bwd(const void* dy, const uint8_t* idx, void* dx, int accumulate, int N, int H, int W, int C, int k, int dtype, void* stream);
/* y[n,h,w,c] = sum over the k x k block (adjoint of nearest upsampling) */
int rua_sumpool(const void* x, void* y, int N, int H, int W, int C, int k, int dtype, void* stream);
/* The 2 / 4 / 8 pyramid of one PSPPooling: the max-pool with window 2k from the max-pool with window k and its argmax bytes
 * (values and argmax bytes of a direct rua_maxpool_fwd with 2k; y_half is [N][H_half][W_half][C]: x is read once, by the k = 2
 * pass), the scatter of up to three pooled gradients into dx (one read-modify-write of dx), and the three window sums in one pass
 * (fp32 partial sums carried up the pyramid). */
int rua_maxpool_derive(const void* y_half, const uint8_t* idx_half, void* y, uint8_t* idx, int N, int H_half, int W_half, int C,
                       int k_half, int dtype, void* stream);
int rua_maxpool_bwd_multi(int n, const void* const* dy, const uint8_t* const* idx, const int* ks, void* dx, int accumulate,
                          int N, int H, int W, int C, int dtype, void* stream);
int rua_sumpool_pyramid(const void* x, void* y2, void* y4, void* y8, int N, int H, int W, int C, int dtype, void* stream);
int rua_upsample_nearest(const void* x, void* y, int N, int H, int W, int C, int k, int dtype, void* stream);

/* ---- elementwise ------------------------------------------------------------------------- */
int rua_add_n(int n, const void* const* in, void* out, int accumulate, int64_t elems, int dtype, void* stream);
int rua_relu_mask(void* dy, const void* y, int64_t elems, int dtype, void* stream);   /* dy = y > 0 ? dy : +0 - a select, not a product: an Inf or NaN in dy leaves as +0 where y <= 0 */
int rua_relu(const void* x, void* y, int64_t elems, int dtype, void* stream);
int rua_cast_f32_to(const float* x, void* y, int64_t elems, int dtype, void* stream);
int rua_cast_to_f32(const void* x, float* y, int64_t elems, int dtype, void* stream);
int rua_fill_zero(void* p, int64_t bytes, void* stream);

/* ---- losses and metrics (multitasking_utils.py:38-85, utils.py:466-491, train_ISPRS.py:411-461)
 * p, y, z, dz are fp32 [B][HW][C]. */
#define RUA_LOSS_TANIMOTO 0
#define RUA_LOSS_WCE 1
#define RUA_LOSS_CE_LOGITS 2
#define RUA_LOSS_BCE_LOGITS 3
#define RUA_LOSS_MSE 4
#define RUA_ACT_NONE 0
#define RUA_ACT_SOFTMAX 1
#define RUA_ACT_SIGMOID 2
/* six moments per (sample, class): sum p, sum (1-l), sum p*l, sum p^2+l^2, sum (1-p)(1-l), sum (1-p)^2+(1-l)^2 */
int rua_tanimoto_sums(const float* p, const float* y, int B, int64_t HW, int C, double* sums, void* stream);
/* loss_out[0] = mean_n Tanimoto_dual ; coef[B][C][3] (optional): dLoss/dp = c0 + c1*p + c2*l (already * grad_scale);
 * per_sample[B] (optional): the (B,) vector the reference's loss function returns (multitasking_utils.py:84) */
int rua_tanimoto_finalize(const double* sums, int B, int64_t HW, int C, float grad_scale, double* loss_out, float* coef,
                          float* per_sample, void* stream);
#define RUA_MAX_HEADS 8
typedef struct rua_tani_head {
  double* sums; int32_t replicas, B, C; float grad_scale; double* loss_out; float* coef; float* per_sample;   /* as rua_tanimoto_finalize_rep */
} rua_tani_head;
/* rua_tanimoto_finalize_rep for n (<= RUA_MAX_HEADS) heads in ONE launch (the seg / bound / dist / color heads of the multitask model, train_ISPRS.py:417-421) */
int rua_tanimoto_finalize_multi(const rua_tani_head* heads, int n, void* stream);
typedef struct rua_dz_head {
  int32_t kind, act; const float* p; const float* y; const float* coef; const float* class_w; float grad_scale; int32_t B; int64_t HW; int32_t C, pad; float* dz;
} rua_dz_head;
/* rua_head_dz for n (<= RUA_MAX_HEADS) heads in ONE launch */
int rua_head_dz_multi(const rua_dz_head* heads, int n, void* stream);
/* sums [replicas + 1][B][C][6]: `replicas` copies filled by rua_head_fwd_loss_rep; their sum is stored into the extra slot behind them (plain stores:
 * idempotent) and finalised as above. */
int rua_tanimoto_finalize_rep(double* sums, int replicas, int B, int64_t HW, int C, float grad_scale, double* loss_out, float* coef,
                              float* per_sample, void* stream);
/* Tanimoto_loss(label, pred) itself (multitasking_utils.py:38-68), shape (B,): take the sums with p := label, y := pred
 * (rua_tanimoto_sums(label, pred, ...)), then per_sample[n] = (sum_c w_c*Spl + 1e-5) / (sum_c w_c*(Ssq - Spl) + 1e-5) with
 * w_c = 1 / (mean_n volume of the FIRST argument)^2, inf -> largest finite weight (:46-53); mean_out[0] = mean_n.
 * "inf" is the reference's float32 outcome - the float32 reciprocal of the float32 square overflows, for every V^2 <= 2^-128 and not only at V == 0 -
 * here and in both terms of rua_tanimoto_finalize; a finite weight keeps its float64 value. */
int rua_tanimoto_ratio(const double* sums, int B, int C, double* mean_out, float* per_sample, void* stream);
/* loss_out[0] += sum over pixels of the per-pixel loss of kind 1..4 (caller divides);
 * per_pixel[M] (optional): the (B,H,W) map the reference's loss function returns (utils.py:486) */
int rua_pixel_loss(int kind, const float* p, const float* z, const float* y, const float* class_w,
                   int64_t M, int C, double* loss_out, float* per_pixel, void* stream);
/* dz = d(total)/d(logits) for every loss kind; coef only for Tanimoto; grad_scale = loss_weight/denominator */
int rua_head_dz(int kind, int act, const float* p, const float* y, const float* coef, const float* class_w,
                float grad_scale, int B, int64_t HW, int C, float* dz, void* stream);
/* out[5] += {#argmax matches, TP, FP, TN, FN at threshold .5} */
int rua_seg_metrics(const float* p, const float* y, int64_t M, int C, double* out, void* stream);

/* ---- void pixels: training on partly labelled patches -------------------------------------------------------------------------
 * void_mask is a device uint8 [B*HW] array (one byte per sample and pixel, any alignment); a NON-ZERO byte marks a void pixel, one
 * that is outside the training data.  void_mask == NULL: exactly the entry point without the suffix.  A void pixel is left out by
 * select, never by a multiplication: p, z and y may hold NaN or Inf there and every result stays finite.
 *   rua_tanimoto_sums_void   the six moments over the valid pixels of a sample, as if the void ones were cut out of the image;
 *                            the finalisers need only the sums and are used unchanged
 *   rua_head_fwd_loss_void   rua_head_fwd_loss_rep whose moments and counts leave the void pixels out; z and p are stored for every pixel
 *   rua_pixel_loss_void      loss_out[0] += the sum over the VALID pixels; the caller still divides by M, the count of all pixels
 *                            (Keras' sample_weight rule with 0 / 1 weights); per_pixel is 0 at a void pixel
 *   rua_head_dz_void         dz is +0.0f in every class of a void pixel (written, not skipped); grad_scale as without the mask
 *   rua_head_dz_multi_void   the same for n heads and ONE mask: the heads must agree in B and HW (RUA_ERR_ARG otherwise)
 *   rua_seg_metrics_void     matches and TP / FP / TN / FN over the valid pixels: (TP + FP + TN + FN) / C is their number */
int rua_tanimoto_sums_void(const float* p, const float* y, const uint8_t* void_mask, int B, int64_t HW, int C, double* sums, void* stream);
int rua_head_fwd_loss_void(const void* x, const float* w, const float* b, float* z, float* p, const float* y, double* tanimoto_sums,
                           int sums_replicas, double* metrics, int B, int64_t HW, int Cin, int Cout, int act, int dtype,
                           const uint8_t* void_mask, void* stream);
int rua_pixel_loss_void(int kind, const float* p, const float* z, const float* y, const float* class_w, const uint8_t* void_mask,
                        int64_t M, int C, double* loss_out, float* per_pixel, void* stream);
int rua_head_dz_void(int kind, int act, const float* p, const float* y, const float* coef, const float* class_w,
                     float grad_scale, int B, int64_t HW, int C, const uint8_t* void_mask, float* dz, void* stream);
int rua_head_dz_multi_void(const rua_dz_head* heads, int n, const uint8_t* void_mask, void* stream);
int rua_seg_metrics_void(const float* p, const float* y, const uint8_t* void_mask, int64_t M, int C, double* out, void* stream);

/* ---- focal losses and label smoothing (Keras' CategoricalFocalCrossentropy / BinaryFocalCrossentropy and label_smoothing=; the package's
 * losses.py holds the definitions as fp64 functions).  Two more kinds and one struct of options; the entries above and rua_dz_head are unchanged.
 * With e = label_smoothing, g = gamma, C classes and the clip bounds 1e-7, 1 - 1e-7:
 *   smoothing        t = y (1 - e) + e / C under a softmax (kinds 1, 2, 5), t = y (1 - e) + e / 2 per sigmoid channel (kinds 3, 6); kinds 1, 2, 3
 *                    keep their formula with t in place of y; kinds 0 and 4 take none (RUA_ERR_ARG)
 *   RUA_LOSS_FOCAL_CE   u_c = clip(p_c / sum_k p_k); L = - sum_c a_c t_c (1 - u_c)^g log u_c; a = class_w[C], required; act must be softmax
 *   RUA_LOSS_FOCAL_BCE  per channel o = clip(p), bce = -(t log o + (1 - t) log(1 - o)), p_t = t p + (1 - t)(1 - p) on the unclipped p,
 *                       l_c = w_c (1 - p_t)^g bce, w_c = t alpha + (1 - t)(1 - alpha) if class_balance else 1; L = mean_c l_c; act must be sigmoid
 * The gradient passes a clip strictly inside it only.  Range: g = 0 or 1 <= g <= 8 (0 < g < 1 has no finite derivative at p_t = 1), 0 <= e < 1,
 * 0 <= alpha <= 1, C <= 8; violations are RUA_ERR_ARG before any launch.  g = 0 gives factor 1 and derivative term 0 by a branch.
 * void_mask (optional) as in the _void entries.  Kinds 0..4 with zeroed options run the kernels of the entries above: the same bytes. */
#define RUA_LOSS_FOCAL_CE 5
#define RUA_LOSS_FOCAL_BCE 6
typedef struct rua_loss_opts { float gamma, label_smoothing, alpha; int32_t class_balance; } rua_loss_opts;
/* kinds 1..6 (Tanimoto is no per-pixel loss): loss_out[0] += the sum over the valid pixels, per_pixel[M] optional */
int rua_pixel_loss_opts(int kind, const float* p, const float* z, const float* y, const float* class_w, const uint8_t* void_mask,
                        const rua_loss_opts* opts, int64_t M, int C, double* loss_out, float* per_pixel, void* stream);
/* kinds 0..6 */
int rua_head_dz_opts(int kind, int act, const float* p, const float* y, const float* coef, const float* class_w, float grad_scale,
                     int B, int64_t HW, int C, const uint8_t* void_mask, const rua_loss_opts* opts, float* dz, void* stream);
/* n heads of mixed kinds in ONE launch, opts[i] belongs to heads[i] */
int rua_head_dz_multi_opts(const rua_dz_head* heads, const rua_loss_opts* opts, int n, const uint8_t* void_mask, void* stream);

/* ---- online hard example mining (OHEM, bootstrapped cross-entropy): per step and per head only the hardest pixels contribute - those whose
 * loss lies above a threshold, but never fewer than a floor.  The package's losses.py holds the definition as a host function, host_ohem; the
 * kernels are csrc/ohem.hip.  For one head and one batch, with L[M] the per_pixel map of a loss entry above (kinds 1..6) and valid = every pixel,
 * or byte == 0 of void_mask:
 *   key        the float32 bit pattern as an order-preserving uint32: all bits of a negative flipped, the sign bit of a non-negative set
 *              (-0 < +0); every NaN is 0xFFFFFFFF, the hardest key (always kept, so a non-finite step skip still sees it)
 *   n_valid    = sum(valid)
 *   q          = keep_q16 (1..65536: the kept share of the valid pixels in Q16), or under a warm-up of `warmup` > 0 optimizer updates
 *              65536 - ((65536 - keep_q16) * min(t, warmup)) / warmup in integers, t = (int64)step_state[0] (the device's step counter;
 *              step_state NULL: no warm-up)
 *   K          = min(n_valid, max(min_kept, (n_valid * q + 65535) >> 16))
 *   tau_key    = the K-th largest valid key; with has_thresh: min(that, key(thresh)); no valid pixel: 0xFFFFFFFF in place of the K-th key
 *   kept       = valid and key(L) >= tau_key: ties at the threshold are all kept, n_kept >= K, no order enters
 *   loss       = (fp64 sum of L over the kept pixels) / n_kept, 0 for n_kept = 0;  scale = (float)((double)loss_weight / (double)n_kept), or 0
 * rua_ohem_select writes drop_mask[M] (0 kept, 1 dropped or void; every byte, always), adds the kept mean into loss_out[0] (the fp64 slot
 * contract of rua_pixel_loss; unchanged for n_kept = 0) and fills result_dev.  An exact radix select over the key in three digit passes of
 * 11 / 11 / 10 bits: per-block LDS histograms, flushed to global ones with integer atomics; every block derives the digit chosen so far from the
 * previous passes' histograms itself.  SIX launches whatever the map holds (zero, three histogram passes, the mask pass, a one-block finisher),
 * no block waits for another, no host readback; all sums are integers but the kept sum, which is added in a fixed order (per thread in index
 * order, a fixed butterfly per wave, waves and blocks in order): the same bits on every run and every replay.  workspace: at least
 * rua_ohem_workspace_bytes of M, 8-byte aligned, contents irrelevant.  RUA_ERR_ARG before any launch: M < 1 (or > 2^40), keep_q16 outside
 * 1..65536, min_kept < 0, warmup < 0, a NaN thresh with has_thresh, a workspace that is too small, a null or misaligned buffer. */
typedef struct rua_ohem_opts { int64_t min_kept; int32_t keep_q16, warmup; float thresh; int32_t has_thresh; } rua_ohem_opts;
typedef struct rua_ohem_result { uint32_t tau_key; float tau; int64_t n_valid, n_kept, K; double kept_sum; float scale; int32_t q16_used; } rua_ohem_result;
int64_t rua_ohem_workspace_bytes(int64_t M);
int rua_ohem_select(const float* per_pixel, const uint8_t* void_mask, int64_t M, const rua_ohem_opts* opts, const double* step_state,
                    float loss_weight, void* workspace, int64_t workspace_bytes, uint8_t* drop_mask, double* loss_out,
                    rua_ohem_result* result_dev, void* stream);
/* d(total)/d(logits) with the mask and the normaliser taken from device memory, per head: the bytes of rua_head_dz_opts called with
 * grad_scale = scale_dev[0] and void_mask = drop_mask (which already holds the void pixels).  rua_head_dz_multi_sel: n heads in ONE launch;
 * a head whose sel entry is zeroed behaves exactly as in rua_head_dz_multi_opts (its host grad_scale, the shared void_mask), a head with a
 * selection ignores both.  drop_mask and scale_dev of a head are both set or both NULL (RUA_ERR_ARG otherwise). */
typedef struct rua_dz_sel { const uint8_t* drop_mask; const float* scale_dev; } rua_dz_sel;
int rua_head_dz_sel(int kind, int act, const float* p, const float* y, const float* coef, const float* class_w, int B, int64_t HW, int C,
                    const rua_loss_opts* opts, const uint8_t* drop_mask, const float* scale_dev, float* dz, void* stream);
int rua_head_dz_multi_sel(const rua_dz_head* heads, const rua_loss_opts* opts, const rua_dz_sel* sel, int n, const uint8_t* void_mask, void* stream);

/* ---- Lovasz-Softmax (Berman, Triki, Blaschko, CVPR 2018): the Lovasz extension of the Jaccard index over a head's probabilities.  The package's
 * losses.py holds the definitions as host functions, host_lovasz and host_lovasz_dz; the kernels are csrc/lovasz.hip.  p[M][C], y[M][C] fp32,
 * void_mask[M] optional (non-zero = void).  Per class c over the n valid pixels: fg = y > 0.5, e = |fg - p| (one fp32 subtraction), G_c = sum fg;
 * the pixels ordered by ohem's key of e DESCENDING (NaN first), ties in ascending pixel index; F_r the foreground count of ranks 0..r;
 * J_r = 1 - (G_c - F_r) / (G_c + (r + 1) - F_r) in fp64, J_-1 = 0; w_r = J_r - J_{r-1}; loss_c = sum_r (double)e_(r) * w_r;
 * dp[pixel][c] = (float)w_r for a background pixel, -(float)w_r for a foreground one, +0.0f for void pixels and for classes that are not counted.
 * Counted: G_c > 0, or every class with all_classes.  loss = sum_counted loss_c / n_cls; scale = (float)((double)loss_weight / n_cls); n = 0 or
 * n_cls = 0: loss 0, scale 0, dp all zero, the slot unchanged.
 * rua_lovasz_grad adds loss_weight * loss into loss_out[0] (an fp64 slot), writes dp[M][C] (NULL: the value only), order_out[C][M] (NULL: not; the
 * sorted pixel indices, entries from n on unspecified) and fills result_dev.  A stable LSD radix sort of (key, pixel) pairs in four 8-bit passes
 * (histogram, scan, scatter as separate launches), a tile-wise prefix count and a one-block finisher: 18 launches whatever the maps hold, no block
 * waits for another, plain stores and integer atomics, no host readback; the fp64 sums are added in a fixed order: the same bits on every run
 * and replay.  rua_lovasz_tile: the sort's tile size in pairs.  workspace: at least rua_lovasz_workspace_bytes(M, C) (-1 for a shape out of
 * range), 8-byte aligned, contents irrelevant.  RUA_ERR_ARG before any launch: C outside 1..16, M < 1 or >= 2^31, M * C >= 2^32, a workspace
 * that is too small, a null or misaligned buffer.
 * rua_lovasz_dz: dz[M][C] = d(total)/d(logits) from dp in one streaming pass, every fp32 operation rounded on its own:
 *   softmax  s = ((g_0 p_0 + g_1 p_1) + ..), dz_k = scale * (p_k * (g_k - s));   sigmoid  dz_c = scale * (g_c * (p_c * (1 - p_c)))
 * with scale = scale_dev[0] (rua_lovasz_result.scale: a replayed graph needs no host scalar).  A softmax pixel whose dp is zero in every class
 * and a sigmoid element whose dp is zero (every void pixel) leave as +0.0f by a select: p may hold anything there. */
#define RUA_LOSS_LOVASZ 7
#define RUA_LOVASZ_MAX_C 16
typedef struct rua_lovasz_result {
  int64_t n_valid; int32_t n_cls; float scale; int64_t G[RUA_LOVASZ_MAX_C]; double loss_c[RUA_LOVASZ_MAX_C]; double loss;
} rua_lovasz_result;
int rua_lovasz_tile(void);
int64_t rua_lovasz_workspace_bytes(int64_t M, int C);
int rua_lovasz_grad(const float* p, const float* y, const uint8_t* void_mask, int64_t M, int C, int all_classes, float loss_weight,
                    void* workspace, int64_t workspace_bytes, double* loss_out, float* dp, uint32_t* order_out,
                    rua_lovasz_result* result_dev, void* stream);
int rua_lovasz_dz(int act, const float* p, const float* dp, const float* scale_dev, int64_t M, int C, float* dz, void* stream);

/* ---- optimizers on the flat parameter buffer (train_ISPRS.py:404-407) --------------------- */
/* Keras Adam: theta -= lr_t * m / (sqrt(v) + eps); g is read as g*grad_scale and zeroed if zero_grad.
 * lr_t_dev (optional): device scalar overriding lr_t, so a captured HIP graph can be replayed every step */
/* state[0] += 1 (optimizer steps taken), lr_out[0] = state[1] (base rate) [* sqrt(1 - beta2^t) / (1 - beta1^t) for Adam]:
 * the step-dependent rate is produced on the device so that a captured step replays without host-side scalar updates */
int rua_lr_step(double* state, float* lr_out, int adam, double beta1, double beta2, void* stream);
int rua_adam_step(float* theta, float* g, float* m, float* v, int64_t n, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                  float eps, float grad_scale, int zero_grad, void* stream);
int rua_sgd_step(float* theta, float* g, float* vel, int64_t n, float lr, const float* lr_dev, float momentum, float grad_scale,
                 int zero_grad, void* stream);
/* rua_adam_step / rua_sgd_step that also store the updated parameters as bf16 into wcopy_bf16[i] (NULL: not) - the convolutions' forward-layout weight copy */
int rua_adam_step_w(float* theta, float* g, float* m, float* v, int64_t n, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                    float eps, float grad_scale, int zero_grad, void* wcopy_bf16, void* stream);
int rua_sgd_step_w(float* theta, float* g, float* vel, int64_t n, float lr, const float* lr_dev, float momentum, float grad_scale,
                   int zero_grad, void* wcopy_bf16, void* stream);

/* ---- gradient clipping, decoupled weight decay and the non-finite step skip (clip.py holds the host definitions) ----------------
 * The flat parameter buffer is described by a CHUNK TABLE built once on the host (clip.build_chunk_table): every entry of the parameter
 * store is cut into chunks of at most RUA_OPT_CHUNK elements; off is a multiple of 16 elements (slices are 64-byte aligned), a chunk never
 * spans entries and the padding between slices belongs to no chunk.  A VARIABLE is one Keras name (the cin segments of a split kernel are
 * one variable): rows chunk_begin <= k < chunk_end of the chunk table, and a decay flag.
 * RUA_OPT_CHUNK = 8192: one chunk is one 256-thread block, eight 16-byte accesses per thread and stream - enough loads in flight per
 * thread to cover HBM latency without a grid-stride loop - while the partial count stays small: the largest kernel of the flagship graph
 * (3x3x1024x1024, 9.4 M elements) is 1152 chunks, which ONE thread of the finisher adds in order (the price of a fixed summation order). */
#define RUA_OPT_CHUNK 8192
typedef struct rua_opt_chunk { int64_t off; int32_t len; int32_t var; } rua_opt_chunk;
typedef struct rua_opt_var { int32_t chunk_begin, chunk_end, decay, pad; } rua_opt_var;
#define RUA_CLIP_NONE 0
#define RUA_CLIP_GLOBAL_NORM 1
#define RUA_CLIP_NORM 2
#define RUA_CLIP_VALUE 3
/* partials[k] = sum of (double)g[i]^2 over chunk k, one block per chunk, no atomics: a lane adds its elements in index order, the 64 lanes
 * of a wave are folded by a fixed butterfly, the four waves are added in order.  The square of an fp32 value is exact in fp64, so the
 * result is the same bits on every run and every replay.  g 16-byte aligned; 0 < len <= RUA_OPT_CHUNK and off % 4 == 0 are the caller's
 * contract (the table is built by clip.build_chunk_table, which checks them). */
int rua_grad_sumsq(const float* g, const rua_opt_chunk* chunks, int n_chunks, double* partials, void* stream);
/* One block.  var_sumsq[v] = partials of variable v added in chunk order; total = var_sumsq added in variable order.
 *   norm        = grad_scale * sqrt(total)                       (per variable: grad_scale * sqrt(var_sumsq[v]))
 *   coef[v]     = (float)(c / max(norm, c))                      RUA_CLIP_GLOBAL_NORM: the same value for every v; RUA_CLIP_NORM: from the
 *                                                                variable's own norm; RUA_CLIP_NONE / RUA_CLIP_VALUE: 1.  A zero norm gives 1.
 *   flag[0]     = skip_nonfinite && !isfinite(total)             (int32: 1 = the optimizer launched next leaves theta and the moments alone)
 *   report[0]   = this step's global norm, report[1] = the smallest coefficient of this step,
 *   report[2]  += flag[0] (steps skipped), report[3] += (report[1] < 1 && !flag[0]) (steps clipped by a norm; clipvalue does not count)
 * c > 0 is required in the two norm modes and ignored otherwise.  n_chunks: the rows of the chunk table (the partials); the variables'
 * chunk ranges must tile [0, n_chunks) in order, as clip.build_chunk_table leaves them. */
int rua_clip_finish(const double* partials, int n_chunks, const rua_opt_var* vars, int n_vars, int mode, double c, double grad_scale,
                    int skip_nonfinite, double* var_sumsq, float* coef, int32_t* flag, double* report, void* stream);
/* The optimizers over the chunk table instead of the flat range; padding is never read or written.  Per element of a chunk of variable v:
 *   th1 = vars[v].decay && weight_decay != 0 ? th - th * d : th,      d = (float)(weight_decay * lr_state[1])   (decoupled decay; lr_state
 *                                                                      is the device pair of the rate kernel: [1] = the BASE rate)
 *   gg  = clampv((g * grad_scale) * coef[v]),                          clampv(x) = x < -c ? -c : x > c ? c : x for clipvalue = c > 0 (a NaN
 *                                                                      stays a NaN), the identity for clipvalue <= 0
 *   Adam: m, v, theta as the flat kernel computes them, on th1 and gg;  SGD: vel = momentum * vel - lr * gg, theta = th1 + vel
 * flag (NULL: never) != 0 skips the step: theta, the moments keep their bits, no decay; g is still zeroed (zero_grad) and wcopy_bf16 (NULL:
 * none) still receives bf16(theta).  lr_dev: the device rate of the rate kernel (required).  Buffers 16-byte aligned, wcopy 8-byte. */
int rua_adam_step_seg(float* theta, float* g, float* m, float* v, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars,
                      const float* coef, const int32_t* flag, const float* lr_dev, const double* lr_state, float beta1, float beta2, float eps,
                      float grad_scale, float clipvalue, double weight_decay, int zero_grad, void* wcopy_bf16, void* stream);
int rua_sgd_step_seg(float* theta, float* g, float* vel, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars,
                     const float* coef, const int32_t* flag, const float* lr_dev, const double* lr_state, float momentum,
                     float grad_scale, float clipvalue, double weight_decay, int zero_grad, void* wcopy_bf16, void* stream);
/* dst[0 .. n) = src[0 .. n) if flag is NULL or flag[0] != 0, nothing otherwise: the BatchNorm moving statistics' backup when a step begins
 * (flag NULL) and their restore behind a skipped step (flag = the finisher's).  A kernel, not a copy node: a captured step holds kernels only. */
int rua_state_copy(float* dst, const float* src, int64_t n, const int32_t* flag, void* stream);

/* ---- learning-rate schedules and the weights' moving average (schedules.py holds the host definitions) -----------------------------
 * A schedule travels to the rate kernel BY VALUE: its constants are kernel arguments, so a captured step replays them and the device
 * state stays the pair of rua_lr_step - state[0] = optimizer steps taken, state[1] = the BASE rate of the current step, which this
 * kernel now WRITES (rua_lr_step only reads it).  Fields a kind does not use are ignored.
 *   RUA_SCHED_CONSTANT      initial
 *   RUA_SCHED_COSINE        initial, decay_steps, alpha; warmup != 0: warmup_target, warmup_steps (linear from initial to the target,
 *                           then the cosine from the target)
 *   RUA_SCHED_EXPONENTIAL   initial * decay_rate ^ (step / decay_steps)            staircase != 0: floor of the exponent
 *   RUA_SCHED_POLYNOMIAL    (initial - end) * (1 - step / decay_steps) ^ power + end, step clamped to decay_steps; cycle != 0: decay_steps
 *                           times ceil(step / decay_steps) instead of the clamp
 *   RUA_SCHED_PIECEWISE     values[i] for the first i < n_boundaries with step <= boundaries[i], values[n_boundaries] beyond
 *   RUA_SCHED_INVERSE_TIME  initial / (1 + decay_rate * step / decay_steps)        staircase != 0: floor of the quotient */
#define RUA_SCHED_CONSTANT 0
#define RUA_SCHED_COSINE 1
#define RUA_SCHED_EXPONENTIAL 2
#define RUA_SCHED_POLYNOMIAL 3
#define RUA_SCHED_PIECEWISE 4
#define RUA_SCHED_INVERSE_TIME 5
#define RUA_SCHED_MAX_BOUNDARIES 16
typedef struct rua_lr_schedule {
  int32_t kind, staircase, cycle, warmup, n_boundaries, pad;
  double initial, decay_steps, decay_rate, alpha, end, power, warmup_target, warmup_steps;
  double boundaries[RUA_SCHED_MAX_BOUNDARIES];
  double values[RUA_SCHED_MAX_BOUNDARIES + 1];
} rua_lr_schedule;
/* rua_lr_step under a schedule, launch for launch (one thread): t = state[0] + 1 is stored to state[0]; r = schedules.host_lr(sched,
 * t - 1) in fp64 is stored to state[1], where rua_adam_step_seg / rua_sgd_step_seg read the base rate of the decoupled weight decay (the
 * decay follows the schedule); lr_out[0] = (float)r, for adam != 0 (float)(r * sqrt(1 - beta2^t) / (1 - beta1^t)).  A step the optimizer
 * skips (skip_nonfinite) has advanced t all the same.  decay_steps > 0, 0 <= n_boundaries <= RUA_SCHED_MAX_BOUNDARIES and a known kind
 * are checked; state 8-byte aligned. */
int rua_lr_schedule_step(double* state, float* lr_out, rua_lr_schedule sched, int adam, double beta1, double beta2, void* stream);
/* The exponential moving average of the weights, launched right behind the optimizer kernel of the same step.  One streaming pass, 16-byte
 * accesses.  t = (int64)lr_state[0], the counter the rate kernel of THIS step has advanced.  flag (NULL: never) != 0 - a skipped step -:
 * nothing is read or written.  Otherwise per element
 *   e' = theta                                                                        t == 1 (Keras 3: the average starts as a copy)
 *   e' = fadd(fmul(momentum, ema), fmul(fsub(1, momentum), theta))                    each operation rounded on its own, no contraction:
 *                                                                                      bit for bit schedules.host_ema
 *   ema = e';  overwrite_every > 0 && t % overwrite_every == 0: theta = e' and wcopy_bf16 (NULL: none) = bf16(e') - the forward-layout
 *   copy the optimizer left fresh stays fresh.  The optimizer's moments are not touched.
 * ema, theta 16-byte aligned, wcopy 8-byte; 0 <= momentum <= 1; n > 0. */
int rua_ema_step(float* ema, float* theta, void* wcopy_bf16, int64_t n, float momentum, const double* lr_state, int overwrite_every,
                 const int32_t* flag, void* stream);

/* ---- gradient accumulation inside the step (accum.py holds the host definition; Keras 3's gradient_accumulation_steps) ---------------------
 * With K steps the optimizer applies the mean of K consecutive gradients once every K calls.  Per call the step issues, behind the backward (and
 * the all-reduce) and in front of everything else of the optimizer tail:
 *   rua_accum_gate        one thread: m = acc_state[0] + 1; hold[0] = m < k (1: a HOLD step, 0: an UPDATE step); acc_state[0] = hold ? m : 0.
 *                         acc_state[0] - the gradients of this cycle already accumulated, 0 .. k - 1 - is device state: a captured step replays
 *                         the decision.  The host pushes it only when it changed outside (a checkpoint, a re-compile).
 *   rua_accum_step        one streaming pass, 16-byte accesses, no atomics, every operation rounded on its own in fp32, Inf / NaN propagate:
 *                           hold[0] != 0:  a = fadd(a, g)                                 (g is left as it is: the flagged optimizer zeroes it)
 *                           hold[0] == 0:  g = fdiv(fadd(g, a), (float)k) - a correctly rounded division -, a = 0
 *                         g and a 16-byte aligned and distinct, n > 0, 2 <= k <= 2^24.
 *   the *_gated forms     of rua_lr_step, rua_lr_schedule_step, rua_grad_sumsq and rua_clip_finish: the same kernels with hold (not NULL) as
 *                         a last argument.  hold[0] != 0: state, rate, partials, per-variable sums, coefficients and report keep their bits.
 *                         hold[0] == 0: exactly the ungated entry point.  rua_clip_finish_gated writes TWO flags: flag2[0] = this update was
 *                         skipped (skip_nonfinite; 0 on a hold step) - rua_state_copy's restore of the BatchNorm statistics reads this one, so
 *                         it never fires on a hold step -, flag2[1] = hold or skipped - rua_adam_step_seg / rua_sgd_step_seg (which then only
 *                         zero g and rewrite the bf16 copy of the unchanged weights) and rua_ema_step read this one. */
int rua_accum_gate(int32_t* acc_state, int k, int32_t* hold, void* stream);
int rua_accum_step(float* g, float* a, int64_t n, int k, const int32_t* hold, void* stream);
int rua_lr_step_gated(double* state, float* lr_out, int adam, double beta1, double beta2, const int32_t* hold, void* stream);
int rua_lr_schedule_step_gated(double* state, float* lr_out, rua_lr_schedule sched, int adam, double beta1, double beta2, const int32_t* hold,
                               void* stream);
int rua_grad_sumsq_gated(const float* g, const rua_opt_chunk* chunks, int n_chunks, double* partials, const int32_t* hold, void* stream);
int rua_clip_finish_gated(const double* partials, int n_chunks, const rua_opt_var* vars, int n_vars, int mode, double c, double grad_scale,
                          int skip_nonfinite, double* var_sumsq, float* coef, int32_t* flag2, double* report, const int32_t* hold, void* stream);

/* ---- LAMB: Adam's direction scaled per variable by ||w|| / ||update|| (lamb.py holds the host definition; You et al. 2019, Keras 3's Lamb) ----
 * Three launches over the chunk table where rua_adam_step_seg is one.  The rate kernel in front of them runs with adam = 0: the bias
 * correction is applied per element here.  Every fp32 operation is rounded on its own (no contraction), divisions and square roots are IEEE,
 * so m', v', u and theta' are bit for bit lamb.host_lamb_step's.  Padding is never read or written.
 *   t = (int64)lr_state[0], the update count the rate kernel of THIS step has advanced; c1 = (float)(1 - beta1^t), c2 = (float)(1 - beta2^t)
 *   with beta^t = lamb.host_powi: binary exponentiation on fp64 (value, remainder) pairs in a fixed order - within one ulp of beta^t, the
 *   same bits on both sides, no pow on either.
 *
 * rua_lamb_moments - pass 1, one block per chunk.  Per element of a chunk of variable var:
 *   th1 = vars[var].decay && weight_decay != 0 ? th - th * d : th,     d = (float)(weight_decay * lr_state[1])      (as rua_adam_step_seg)
 *   gg  = clampv((g * grad_scale) * coef[var])                                                                      (as rua_adam_step_seg)
 *   m'  = m + (gg - m) * (1 - beta1),   v' = v + (gg * gg - v) * (1 - beta2)                                        (Keras' form)
 *   u   = (m' / c1) / (sqrt(v' / c2) + eps)
 * m and v receive m' and v'; g RECEIVES u (the gradient is consumed; pass 2 reads u there and zeroes the slot); theta is only read.
 * pw[k] = sum of (double)th1^2, pu[k] = sum of (double)u^2 over chunk k, in rua_grad_sumsq's reduction order (a lane adds its elements in
 * index order, a fixed butterfly over the wave, the four waves in order, no atomics): the same bits on every run and every replay.
 *
 * rua_lamb_finish - one block.  W[v], U[v] = the partials of variable v added in chunk order (var_wu[v] and var_wu[n_vars + v], scratch of
 * 2 * n_vars doubles; the variables' chunk ranges tile [0, n_chunks) in order);
 *   ratio[v] = (W > 0 && U > 0) ? (float)(sqrt(W) / sqrt(U)) : 1        (a zero or NaN sum gives 1, as Keras' nested where does)
 *   report[0] = the smallest, report[1] = the largest ratio of this update, report[2] = the variables of this update whose ratio the rule
 *   forced to 1, report[3] += 1 (updates taken).
 *
 * rua_lamb_apply - pass 2, one block per chunk:  theta' = th1 - (ratio[var] * lr_dev[0]) * u, with th1 recomputed as above and u read from
 * g's slot; g = 0 when zero_grad is set; wcopy_bf16 (NULL: none) receives bf16(theta').
 *
 * flag (NULL: never) != 0 - a skipped update (skip_nonfinite) or a hold step of gradient accumulation, the flags rua_adam_step_seg takes -:
 * theta, m, v, pw, pu, var_wu, ratio and report keep their bits; pass 1 only zeroes g, pass 2 only rewrites wcopy_bf16 from the unchanged theta.
 * 0 <= beta < 1, eps > 0, weight_decay >= 0, n_chunks > 0, n_vars > 0; float buffers and tables 16-byte aligned, doubles 8-byte, wcopy 8-byte,
 * coef / ratio / flag / lr_dev 4-byte; pw != pu.  A violation is RUA_ERR_ARG before anything is launched. */
int rua_lamb_moments(const float* theta, float* g, float* m, float* v, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars,
                     const float* coef, const int32_t* flag, const double* lr_state, float beta1, float beta2, float eps, float grad_scale,
                     float clipvalue, double weight_decay, double* pw, double* pu, void* stream);
int rua_lamb_finish(const double* pw, const double* pu, int n_chunks, const rua_opt_var* vars, int n_vars, const int32_t* flag, double* var_wu,
                    float* ratio, double* report, void* stream);
int rua_lamb_apply(float* theta, float* g, const rua_opt_chunk* chunks, int n_chunks, const rua_opt_var* vars, const float* ratio,
                   const int32_t* flag, const float* lr_dev, const double* lr_state, double weight_decay, int zero_grad, void* wcopy_bf16,
                   void* stream);

/* ---- multitask training targets from uint8 patches (labels.py; the reference's preprocess_save_patches_ISPRS.py:206-228,
 * multitasking_utils.py:6-35) ------------------------------------------------------------------------------------------------
 * img [N][H][W][Cin] and cls [N][H][W] are uint8 (4-byte aligned); x [N][H][W][Cin], seg / bound / dist [N][H][W][C] and
 * color [N][H][W][3] are fp32 (16-byte aligned).  Bit for bit the host definitions:
 *   x = float(img) / 255 (norm_type 1) or / 126.5 (norm_type 2: `img /= 127.5 - 1.`), seg = onehot(cls) (a class value >= C: all zero),
 *   bound = get_boundary_label(seg), dist = get_distance_label(seg), color = color_label(img, norm_type).
 * cls and seg are null together (x only: inference); bound, dist and color are null together (single task: x and seg only), color needs
 * Cin = 3.  scratch: rua_targets_scratch_bytes(N, C) bytes (only with dist).  Limits: 1 <= H, W <= 512, 1 <= C <= 64, 1 <= Cin <= 16,
 * N*H*W*max(C, Cin, 4) < 2^31.  Four launches (one without dist); the results do not depend on launch order or timing. */
int64_t rua_targets_scratch_bytes(int N, int num_classes);
int rua_multitask_targets(const uint8_t* img, const uint8_t* cls, int N, int H, int W, int Cin, int num_classes, int norm_type,
                          float* x, float* seg, float* bound, float* dist, float* color, void* scratch, int64_t scratch_bytes, void* stream);
/* The void mask of class-map patches (labels.host_void_mask, bit for bit): mask[n][i][j] = 255 if a pixel of patch n within Chebyshev
 * distance `margin` of (i, j) has a class value >= num_classes, else 0.  Pixels outside the patch are not void and patches never leak
 * into each other.  margin 0: mask = 255 * (cls >= num_classes).  cls and mask are device uint8 [N][H][W], any alignment, not overlapping.
 * Limits: 1 <= H, W <= 512, 1 <= num_classes <= 255, 0 <= margin <= 16, 1 <= N <= 65535, N*H*W < 2^31 (RUA_ERR_ARG before any launch).
 * One launch. */
int rua_void_mask(const uint8_t* cls, int N, int H, int W, int num_classes, int margin, uint8_t* mask, void* stream);

/* ---- training windows cut and augmented from resident scenes (scenes.py; the reference's preprocess_save_patches_ISPRS.py:28-48,
 * utils.py:69-95 done per step on the device) ------------------------------------------------------------------------------------
 * All array arguments are HOST arrays.  scene_img[s] / scene_cls[s] are device pointers to a uint8 [scene_h[s]][scene_w[s]][Cin]
 * image and its uint8 [scene_h[s]][scene_w[s]] class map; windows is int32 [N][4], rows (scene, row, col, code): the window
 * scene[row : row + PH, col : col + PW] transformed by code - 0 as it is, 1 rot90, 2 rot180, 3 rows flipped, 4 columns flipped,
 * 5 rot270, 6 transposed, 7 anti-transposed (1, 5, 6, 7 need PH == PW).  img_out [N][PH][PW][Cin] and cls_out [N][PH][PW] are
 * device memory, 4-byte aligned (what the targets call above reads); scene_cls and cls_out are null together (images only).
 * Every row is checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the row); the
 * resolved windows travel as kernel arguments, 128 per launch, image and class map in the same launch: no device-side table,
 * no copy, no synchronisation.  Limits: 1 <= PH, PW <= 512, 1 <= Cin <= 16. */
int rua_scene_windows(const uint8_t* const* scene_img, const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w,
                      int nscenes, const int32_t* windows, int N, int PH, int PW, int Cin,
                      uint8_t* img_out, uint8_t* cls_out, void* stream);

/* ---- the same outputs under a free affine map: random rotation, zoom and shift with reflect padding (scenes.py,
 * host_windows_affine / affine_rows) ------------------------------------------------------------------------------------------
 * Arguments as for rua_scene_windows, but windows is int32 [N][7], rows (scene, y0, x0, a_yy, a_yx, a_xy, a_xx), all but scene
 * in Q16 fixed point.  Destination pixel (i, j) samples the scene at
 *   sy = y0 + i * a_yy + j * a_yx      sx = x0 + i * a_xy + j * a_xx      (exact integers; pixel centres on integers).
 * A scene index t is folded into [0, n) by numpy's 'reflect' rule (no edge repeat, any number of reflections):
 *   refl(t, n):  m = 2 * (n - 1);  u = t mod m (non-negative);  u < n ? u : m - u.
 * Image, per channel, bilinear with 8-bit fractions:  iy = sy >> 16 (arithmetic), fy = (sy & 0xFFFF) >> 8, the same in x;
 *   p00 = img[refl(iy, H)][refl(ix, W)], p01 at ix + 1, p10 at iy + 1, p11 at both;
 *   out = ((256 - fy) * ((256 - fx) * p00 + fx * p01) + fy * ((256 - fx) * p10 + fx * p11) + 32768) >> 16.
 * Class map, nearest:  cls[refl((sy + 32768) >> 16, H)][refl((sx + 32768) >> 16, W)].
 * Integers only, so scenes.host_windows_affine gives the same bytes.  Limits, all checked on the host before anything is launched
 * (a violation: RUA_ERR_ARG, the message names the scene or the row): 0 <= scene < nscenes, 2 <= H, W <= 16384 for every scene,
 * |a| <= 4 * 65536 for every coefficient, |y0|, |x0| <= 2^30, 1 <= PH, PW <= 512, 1 <= Cin <= 16 - under them every sum above
 * fits in 32 bits.  The windows travel as kernel arguments, 80 per launch, image and class map in the same launch: no
 * device-side table, no copy, no synchronisation. */
int rua_scene_windows_affine(const uint8_t* const* scene_img, const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w,
                             int nscenes, const int32_t* windows /* [N][7] */, int N, int PH, int PW, int Cin,
                             uint8_t* img_out, uint8_t* cls_out, void* stream);

/* ---- colour, tone and noise jitter of the staged windows (scenes.py, host_photometric / photo_rows) ---------------------------
 * img_in and img_out are DEVICE memory, uint8 [N][PH][PW][Cin] with a 4-byte aligned base - what the two calls above write and the
 * targets call reads -, either the same pointer (in place) or ranges that do not overlap; photo is a HOST array, int32 [N][16], one
 * row R per window in Q16:  M[c][d] = R[3 c + d] (colour matrix),  b[c] = R[9 + c] (offsets, in levels),  t = R[12] (tone),
 * A = R[13] (noise amplitude),  R[14] the noise seed read as uint32,  R[15] reserved, 0.  For source byte p[c] of pixel (i, j), every
 * >> arithmetic and clamp to [0, 255]:
 *   colour, Cin == 3:  u[c] = clamp((M[c][0] * p[0] + M[c][1] * p[1] + M[c][2] * p[2] + b[c] + 32768) >> 16)
 *           Cin != 3:  u[c] = clamp((M[0][0] * p[c] + b[0] + 32768) >> 16)  - the row must be scalar: off-diagonals 0, the three
 *                      diagonal entries equal, the three offsets equal
 *   tone:              v[c] = clamp(u[c] + ((t * u[c] * (255 - u[c]) + (1 << 23)) >> 24))   (fixes 0 and 255, monotone for |t| <= 65536)
 *   noise, A != 0:     idx = (i * PW + j) * Cin + c - the position inside the window, not in the batch;
 *                      x = uint32(R[14]) + (idx + 1) * 0x9E3779B9 (mod 2^32);  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;
 *                      x *= 0x846ca68b;  x ^= x >> 16;  z = (x & 255) + ((x >> 8) & 255) + ((x >> 16) & 255) + (x >> 24) - 510;
 *                      out[c] = clamp(v[c] + ((A * z + 32768) >> 16))      (z in -510..510, standard deviation sqrt((256^2 - 1) / 3))
 * The row M = 65536 * I, zeros elsewhere, returns the input bytes.  Integers only, so scenes.host_photometric gives the same bytes.
 * Limits, all checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the row and the word):
 * |M| <= 2^20, |b| <= 2^29, |t| <= 65536, 0 <= A <= 65536, R[15] == 0, 1 <= PH, PW <= 512, 1 <= Cin <= 16, N >= 1,
 * N*PH*PW*Cin < 2^31 - under them every intermediate fits in 32 bits:  3 * 2^20 * 255 + 2^29 + 2^15 < 2^31,
 * 65536 * 127 * 128 + 2^23 < 2^31,  65536 * 510 + 2^15 < 2^31.  The rows travel as kernel arguments, 48 per launch: no
 * device-side table, no copy, no synchronisation.  In place, a window whose row is the identity is left alone. */
int rua_window_photometric(const uint8_t* img_in, uint8_t* img_out, int N, int PH, int PW, int Cin,
                           const int32_t* photo /* HOST, [N][16] */, void* stream);

/* ---- copy-paste augmentation of the staged windows (scenes.py, host_paste / paste_rows / CopyPaste) ----------------------------
 * img [N][PH][PW][Cin] and cls [N][PH][PW] are DEVICE memory, the staged windows the cutting calls above write and the targets call
 * reads; both are required and changed in place.  scene_img[s], scene_cls[s] are laid out as in rua_scene_windows, scene_inst[s] is
 * a DEVICE int32 [H][W] object-id map of scene s, -1 meaning no object (rua_scene_instances at radius 0 leaves one).  pastes is a
 * HOST array, int32 [M][16], applied IN TABLE ORDER; row R:
 *   R[0] window   R[1] scene   R[2] id   R[3] code   R[4] top   R[5] left   R[6] i0   R[7] j0   R[8] h   R[9] w
 *   R[10], R[11] the low and high word of the 64-bit `onto` mask   R[12] flags   R[13..15] reserved, 0
 * The crop is the scene rectangle [i0, i0 + h) x [j0, j0 + w); T is the crop under the symmetry `code` (the table of
 * rua_scene_windows; h x w for codes 0, 2, 3, 4 and w x h for 1, 5, 6, 7 - a non-square crop is legal under every code) placed with
 * its first pixel at (top, left) of window R[0].  For a destination pixel (y, x) of that window inside T, with source scene pixel
 * (i, j): it is pasted iff scene_inst[s][i][j] == id and d, the destination's CURRENT class byte (after all earlier rows), satisfies
 * d < num_classes ? bit d of onto : flags & 1.  A pasted pixel takes the Cin image bytes and the class byte of its source.  Parts of
 * T outside the window are clipped, a row wholly outside is a no-op; windows without a row and every byte not pasted keep their bits.
 * Integers only, so scenes.host_paste gives the same bytes.  Limits, all checked on the host before anything is launched (a
 * violation: RUA_ERR_ARG, the message names the row and the word): R[0] non-decreasing and in 0..N-1, 0 <= scene < nscenes, id >= 0,
 * code in 0..7, |top|, |left| <= 1024, 1 <= h, w <= 512 and the rectangle inside its scene, flags 0 or 1, reserved words 0,
 * 1 <= PH, PW <= 512, 1 <= Cin <= 16, 1 <= num_classes <= 64, N*PH*PW*Cin < 2^31, M >= 0; M == 0 launches nothing.  The rows
 * travel resolved as kernel arguments, 48 per launch (a window's rows may straddle two launches: the stream orders them): no
 * device-side table, no copy, no synchronisation. */
int rua_window_paste(uint8_t* img, uint8_t* cls, int N, int PH, int PW, int Cin, int num_classes,
                     const uint8_t* const* scene_img, const uint8_t* const* scene_cls, const int32_t* const* scene_inst,
                     const int32_t* scene_h, const int32_t* scene_w, int nscenes,
                     const int32_t* pastes /* HOST, [M][16] */, int M, void* stream);

/* ---- whole-scene evaluation: window probabilities -> a uint8 class map per scene and a confusion matrix (scenes.py, predict_table /
 * host_stitch; the reference's test_ISPRS.py:26-87 arg-max, mosaic and confusion_matrix done on the device) ----------------------
 * p is DEVICE memory, fp32 [N][PH][PW][C], 16-byte aligned: the class probabilities of N windows (the seg head's output).  windows
 * and own are HOST arrays, int32 [N][4]: rows (scene, row, col, 0) as rua_scene_windows reads them, and (r0, r1, c0, c1), the
 * rectangle of window coordinates [r0, r1) x [c0, c1) this window is responsible for.  scene_pred / scene_cls / scene_h / scene_w are
 * HOST arrays of nscenes entries: device pointers to a uint8 [scene_h[s]][scene_w[s]] prediction map and class map, and the sizes.
 * For every window n and every (i, j) of its rectangle:
 *   pred = first index of the maximum of p[n][i][j][0..C) (a strict > scan from 0: np.argmax on finite input);
 *   scene_pred[s][row + i][col + j] = pred;  with class maps and t = scene_cls[s][row + i][col + j] < C:  confusion[t][pred] += 1.
 * confusion is DEVICE memory, int64 [C][C], and is ACCUMULATED into (zero it first); scene_cls and confusion are null together (maps
 * only).  Nothing outside the rectangles is written; an empty rectangle (r0 == r1 or c0 == c1) writes nothing - a padded batch.
 * Rectangles that overlap in a scene are the caller's mistake: the map then holds one of the predictions, the matrix counts both.
 * Integers only, so scenes.host_stitch gives the same bytes and counts whatever the launch order.  Every row is checked on the host
 * before anything is launched (a violation: RUA_ERR_ARG, the message names the row): 0 <= scene < nscenes, the window inside its
 * scene, code == 0, 0 <= r0 <= r1 <= PH, 0 <= c0 <= c1 <= PW.  The resolved windows travel as kernel arguments, 120 per launch: no
 * device-side table, no copy, no synchronisation.  Limits: 1 <= PH, PW <= 512, 1 <= C <= 64. */
int rua_scene_stitch(const float* p, int N, int PH, int PW, int C, const int32_t* windows, const int32_t* own,
                     uint8_t* const* scene_pred, const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w,
                     int nscenes, int64_t* confusion, void* stream);

/* Test-time augmentation: the same map and matrix from K views of every window, summed (scenes.py, view_rows / host_stitch_views).
 * p is fp32 [G*K][PH][PW][C]: rows g*K .. g*K+K-1 of `windows` (HOST, int32 [G*K][4]) name ONE window - the same scene, row and col -
 * under K symmetry codes (rua_scene_windows' codes 0..7), and p[g*K+k] is the network's answer to that window cut under code_k.
 * own is HOST int32 [G][4], one rectangle per group, in the window's own (code 0) coordinates.  For every group g and (i, j) of its
 * rectangle, with q_k = p[g*K+k] turned back into the window's orientation (the inverse symmetry: codes 1 and 5 undo each other,
 * every other code itself):
 *   s[c] = q_0[i][j][c];  s[c] = s[c] + q_k[i][j][c] for k = 1 .. K-1   (fp32 adds, strictly in this order; no division)
 *   pred = first index of the maximum of s;  map and confusion as rua_scene_stitch.
 * The order is fixed, so scenes.host_stitch_views gives the same bytes and counts whatever the launch order.  Everything else is
 * rua_scene_stitch's: confusion is accumulated into, scene_cls and confusion are null together, an empty rectangle writes nothing,
 * every row is checked on the host before anything is launched (RUA_ERR_ARG, the message names the row or the group): 1 <= K <= 8,
 * 0 <= scene < nscenes, the window inside its scene, every row of a group at the group's scene, row and col, 0 <= code <= 7, a
 * transposing code (1, 5, 6, 7) only with PH == PW, the rectangle inside the window.  With K = 1 and code 0 the result is
 * rua_scene_stitch's.  The resolved groups travel as kernel arguments, 120 per launch (the K codes of a group three bits each in one
 * word): no device-side table, no copy, no synchronisation.  Limits: 1 <= PH, PW <= 512, 1 <= C <= 64; p 16-byte aligned. */
int rua_scene_stitch_views(const float* p, int G, int K, int PH, int PW, int C, const int32_t* windows /* [G*K][4] */,
                           const int32_t* own /* [G][4] */, uint8_t* const* scene_pred, const uint8_t* const* scene_cls,
                           const int32_t* scene_h, const int32_t* scene_w, int nscenes, int64_t* confusion, void* stream);

/* Whole-scene maps of any head: fp32 window outputs under K views -> uint8 maps of Ch interleaved channels (scenes.py,
 * host_stitch_maps; what the reference's test_ISPRS.py:285-414 shows of the boundary, distance and colour heads and of the seg
 * head's per-class probability).  p, G, K, PH, PW, windows and own are rua_scene_stitch_views': p is DEVICE fp32 [G*K][PH][PW][Ch],
 * 16-byte aligned, any head's output; windows (HOST int32 [G*K][4]) and own (HOST int32 [G][4]) name the groups, their view codes and
 * the rectangle each group owns.  scene_out / scene_h / scene_w are HOST arrays of nscenes entries: scene_out[s] is a device pointer
 * to uint8 [scene_h[s]][scene_w[s]][Ch].  For every group g, every (i, j) of its rectangle and every channel c, with q_k = p[g*K+k]
 * turned back into the window's orientation and
 *   a_k = rint(y * 65536), y = q_k[i][j][c] > 0 ? min(q_k[i][j][c], 1) : 0   (fp32, ties to even; NaN and -inf give 0, +inf 65536;
 *                                                                              the multiply by a power of two is exact)
 * mode 0 (plain):    A = a_0 + .. + a_{K-1};  out[row + i][col + j][c] = (255 A + K 32768) / (K 65536)   - the rounded mean, 0..255;
 * mode 1 (hsv_rgb):  Ch = 3.  Per view h = 179 a_k[0] >> 16, s = 255 a_k[1] >> 16, v = 255 a_k[2] >> 16 (truncation), then with
 *   sec = h / 30, f = h % 30, p = (v (255 - s) + 127) / 255, q = (v (7650 - s f) + 3825) / 7650, t = (v (7650 - s (30 - f)) + 3825) / 7650:
 *   rgb_k = (v,t,p), (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q) for sec = 0..5;  out = (2 (rgb_0 + .. + rgb_{K-1}) + K) / (2 K).
 *   The views are averaged in RGB because hue is circular.
 * All divisions are integer divisions of non-negative numbers, every intermediate stays below 2^28: integers from the first step
 * on, so scenes.host_stitch_maps gives the same bytes whatever the order of views, launches or lanes.  Nothing outside the owned
 * rectangles is written - a tile row leaves as the aligned dwords wholly inside it and single bytes at its ragged ends -, an empty
 * rectangle writes nothing, rectangles that overlap in a scene are the caller's mistake.  Everything is checked on the host before
 * anything is launched (a violation: RUA_ERR_ARG, the message names the row, the group or the scene, nothing is written):
 * 1 <= K <= 8, 1 <= Ch <= 64, mode 0 or 1 and mode 1 only with Ch == 3, 1 <= PH, PW <= 512, p 16-byte aligned, no null entry in
 * scene_out, 1 <= H, W and H * W * Ch < 2^40, 0 <= scene < nscenes, the window inside its scene, every row of a group at the group's
 * scene, row and col, 0 <= code <= 7, a transposing code only with PH == PW, the rectangle inside the window.  The resolved groups
 * travel as kernel arguments, 120 per launch: no device-side table, no copy, no synchronisation. */
int rua_scene_stitch_maps(const float* p, int G, int K, int PH, int PW, int Ch, const int32_t* windows /* [G*K][4] */,
                          const int32_t* own /* [G][4] */, uint8_t* const* scene_out, const int32_t* scene_h,
                          const int32_t* scene_w, int nscenes, int mode /* 0 plain, 1 hsv_rgb */, void* stream);

/* Multi-scale test-time augmentation, the way back (scenes.py, scale_table / host_accumulate / host_argmax): the class
 * probabilities of windows that were cut ZOOMED out of a scene (rua_scene_windows_affine under an axis-aligned matrix) are resampled
 * onto the scene grid and added to a scene-sized int32 accumulator, pass after pass; one arg-max at the end gives the class map.
 * p is DEVICE fp32 [G*K][PH][PW][C], 16-byte aligned: group g holds K views of one footprint.  windows7 (HOST int32 [G*K][7], rows
 * (scene, y0, x0, a_yy, a_yx, a_xy, a_xx) in Q16 exactly as rua_scene_windows_affine read them: window pixel (i, j) sampled the scene at
 * sy = y0 + i a_yy + j a_yx, sx = x0 + i a_xy + j a_xx) and own (HOST int32 [G][4], the rectangle (r0, r1, c0, c1) of SCENE pixels the
 * group owns) name the groups.  scene_acc / scene_h / scene_w are HOST arrays of nscenes entries; scene_acc[s] is a device pointer to
 * int32 [scene_h[s]][scene_w[s]][C].  Every row is axis-aligned: either a_yx = a_xy = 0 (y follows the row index i through a_yy, x
 * the column index j through a_xx) or a_yy = a_xx = 0 (y follows j through a_yx, x follows i through a_xy; PH == PW only); the other
 * two entries are nonzero.  For a scene coordinate s on an axis with origin o, coefficient a and n window pixels along its index:
 *   t = 65536 s - o;  if a < 0: t = -t, a = -a;   w = floor((256 t + (a >> 1)) / a)     (64 bit; the window coordinate in 1/256 pixels)
 *   w = min(max(w, 0), 256 (n - 1));  i0 = w >> 8;  f = w & 255;  i1 = min(i0 + 1, n - 1)
 * and with q = rint(min(max(p, 0), 1) * 65536) as rua_scene_stitch_maps quantises (NaN gives 0), read at the four index pairs, fy and
 * fx the weights of the y and the x axis:
 *   val = ((256 - fy) ((256 - fx) q00 + fx q01) + fy ((256 - fx) q10 + fx q11) + 32768) >> 16     (the sum reaches 2^32: 64 bit)
 *   scene_acc[scene][y][x][c] += val_0 + .. + val_{K-1}          for every (y, x) of the rectangle and every channel c.
 * The K views are summed in a register, the update is one plain read-add-write: the groups of ONE call must own disjoint pixels
 * (scenes.scale_table guarantees it), calls on one stream are ordered - no atomics.  Integers from the first step on: the order of
 * views, groups and passes cannot change a bit, scenes.host_accumulate gives the same numbers.  An empty rectangle adds nothing.
 * Everything is checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the row, the group or
 * the scene, nothing is written): 1 <= K <= 8, 1 <= C <= 64, 1 <= PH, PW <= 512, p 16-byte aligned, 1 <= H, W <= 16384, no null entry in
 * scene_acc, 0 <= scene < nscenes, the K rows of a group at one scene, axis-aligned matrices, a transposing one only with PH == PW,
 * the rectangle inside its scene, and - unless empty - inside every view's footprint: the unclamped w of its first and last row and of
 * its first and last column lies in [-256, 256 n].  The resolved groups travel as kernel arguments, 24 per launch: no device-side
 * table, no copy, no synchronisation. */
int rua_scene_accumulate(const float* p, int G, int K, int PH, int PW, int C, const int32_t* windows7 /* [G*K][7] */,
                         const int32_t* own /* [G][4], scene coordinates */, int32_t* const* scene_acc, const int32_t* scene_h,
                         const int32_t* scene_w, int nscenes, void* stream);

/* Blended whole-scene prediction (scenes.py, blend_table / blend_weight / host_accumulate_blend): rua_scene_accumulate for footprints
 * that OVERLAP, each under a linear taper.  The arguments are rua_scene_accumulate's, but foot (HOST int32 [G][4]) holds each group's
 * FULL footprint (r0, r1, c0, c1) in scene pixels, and the rectangles of a call may share pixels.  With FH = r1 - r0, FW = c1 - c0 and,
 * along an axis of F pixels, for position t (0 <= t < F)
 *   w(t) = 256                                        where the footprint touches the scene's low border and 2 t + 1 <= F,
 *                                                     or its high border and 2 t + 1 >= F,
 *   w(t) = max(16, (256 (2 min(t, F - 1 - t) + 1)) / F)   otherwise                                  (integer division),
 * the K views' sum v = val_0 + .. + val_{K-1} of rua_scene_accumulate enters as
 *   scene_acc[scene][y][x][c] += (w(y - r0) w(x - c0) v + 32768) >> 16            (64 bit; at most K 65536)
 * with an integer atomic add whose value is not read, so the groups of a call - and of calls on different streams - may overlap and
 * the sums are the same in any order.  The weight lives in scene space: the K views of a group share it.  The caller keeps K times
 * the number of footprints over one pixel, summed over all calls, below 32768 (scenes.check_blend_budget): the sums are int32.
 * Checked on the host before anything is launched, nothing written on a refusal: everything rua_scene_accumulate checks, under this
 * function's name, and every non-empty rectangle of a call has the size of the first one (a call is one pass).  The resolved groups
 * travel as kernel arguments, 24 per launch.  scenes.host_accumulate_blend gives the same numbers. */
int rua_scene_accumulate_blend(const float* p, int G, int K, int PH, int PW, int C, const int32_t* windows7 /* [G*K][7] */,
                               const int32_t* foot /* [G][4], scene coordinates */, int32_t* const* scene_acc, const int32_t* scene_h,
                               const int32_t* scene_w, int nscenes, void* stream);

/* The class map of finished accumulators: scene_pred[s][y][x] = the first index of the maximum of scene_acc[s][y][x][0..C-1], and,
 * with class maps, confusion[t][pred] += 1 for the label t = scene_cls[s][y][x] < C - accumulated into, as rua_scene_stitch does;
 * scene_cls and confusion are null together.  All array arguments but confusion are HOST arrays of nscenes entries of device
 * pointers (int32 [H][W][C], uint8 [H][W], uint8 [H][W]) and sizes; 1 <= C <= 64, H * W * C * 4 < 2^40; the scenes travel as kernel
 * arguments, 100 per launch.  scenes.host_argmax gives the same bytes and counts. */
int rua_scene_argmax(const int32_t* const* scene_acc, uint8_t* const* scene_pred, const uint8_t* const* scene_cls,
                     const int32_t* scene_h, const int32_t* scene_w, int nscenes, int C, int64_t* confusion, void* stream);

/* ---- class counts of scene windows (scenes.py, host_class_counts / class_weights / balance_rows; what the reference's class weights,
 * train_ISPRS.py:424, and its balance filter, utils.py:383, are functions of) ------------------------------------------------------
 * Array arguments other than counts are HOST arrays: scene_cls / scene_h / scene_w and windows, int32 [N][4] rows (scene, row, col,
 * code), as rua_scene_windows reads them.  counts is DEVICE memory, int32 [N][C + 1], 4-byte aligned.  For window n, the PH x PW
 * pixels scene_cls[scene][row : row + PH, col : col + PW]:
 *   counts[n][c] = pixels equal to c, for c < C;   counts[n][C] = pixels with a value >= C (the "no class" pixels that
 *   rua_multitask_targets turns into an all-zero seg row and rua_scene_stitch leaves out of the matrix).
 * Every row of counts sums to PH * PW.  A symmetry code permutes pixels: it is checked as rua_scene_windows checks it and does not
 * change the counts.  counts is OVERWRITTEN, not accumulated into: what it held before does not matter (a window is split into row
 * bands over blocks that add with integer atomics; the zeroing is part of the call, on the same stream).  Integers only, so
 * scenes.host_class_counts gives the same numbers whatever the launch or arrival order.  Every row is checked on the host before
 * anything is launched (a violation: RUA_ERR_ARG, the message names the row, nothing is written): 0 <= scene < nscenes, the window
 * inside its scene, 0 <= code <= 7, a transposing code only with PH == PW.  The resolved windows travel as kernel arguments, 250
 * per launch (16 bytes each): no device-side table, no copy, no synchronisation.  Limits: 1 <= PH, PW <= 512, 1 <= C <= 64, N >= 1. */
int rua_scene_class_counts(const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w, int nscenes,
                           const int32_t* windows, int N, int PH, int PW, int C, int32_t* counts, void* stream);

/* ---- the eroded ground truth (scenes.py, host_erode / host_erode_confusion; the ISPRS benchmark scores on reference maps from which
 * every pixel within a disc of radius 3 of a class boundary is left out) ---------------------------------------------------------
 * scene_cls / scene_h / scene_w are HOST arrays of nscenes entries, as the calls above read them; scene_out and scene_pred are HOST
 * arrays of nscenes device pointers to uint8 [scene_h[s]][scene_w[s]] maps.  For every pixel (i, j) of every scene:
 *   out[i][j] = 255 if some offset (dy, dx) with dy * dy + dx * dx <= radius * radius has (i + dy, j + dx) inside the map and
 *   cls[i + dy][j + dx] != cls[i][j];  otherwise out[i][j] = cls[i][j].
 * Bytes are compared raw: a "no class" byte (>= C) beside a class pixel erodes that pixel, and stays no class itself; pixels outside
 * the map do not exist, so the scene border is no boundary; radius 0 is the identity.  255 is no class for every C <= 64: the eroded
 * map feeds the t < C rule of rua_scene_stitch and rua_scene_class_counts as it is.  scene_out (nullable) receives these bytes.
 * With scene_pred and confusion (null together; confusion DEVICE memory, int64 [C][C], 8-byte aligned), every pixel with
 * t = out[i][j] < C and p = scene_pred[s][i][j] < C adds one to confusion[t][p], which is ACCUMULATED into, as rua_scene_stitch does
 * (zero it first); C is read only then.  One pass over each scene does both.  Integers only, so scenes.host_erode and
 * scenes.host_erode_confusion give the same bytes and counts whatever the launch or arrival order.  Everything is checked on the host
 * before anything is launched (a violation: RUA_ERR_ARG, the message names the offender, nothing is written): 0 <= radius <= 16,
 * nscenes >= 1, at least one of scene_out and (scene_pred, confusion), 1 <= C <= 64 when counting, no null entry in a pointer
 * array, 1 <= H, W and H * W < 2^40, scene_out[s] != scene_cls[s] (an erosion in place would read its own output).  The scenes
 * travel as kernel arguments, 120 per launch (32 bytes each): no device-side table, no copy, no synchronisation. */
int rua_scene_erode(const uint8_t* const* scene_cls, const int32_t* scene_h, const int32_t* scene_w, int nscenes, int radius,
                    uint8_t* const* scene_out, const uint8_t* const* scene_pred, int C, int64_t* confusion, void* stream);

/* ---- boundary F1 of a prediction map (scenes.py, host_boundaries / host_boundary_counts / boundary_scores; the BF score of Csurka
 * et al. 2013: per class, precision and recall of boundary pixels matched within a distance tolerance) ---------------------------
 * scene_cls / scene_pred / scene_h / scene_w are HOST arrays of nscenes entries, as rua_scene_erode reads them: device pointers to
 * uint8 [scene_h[s]][scene_w[s]] maps, the ground truth and the prediction; both are only read and scene_pred[s] == scene_cls[s] is
 * allowed.  bound_cls and bound_pred (each nullable on its own) are HOST arrays of nscenes device pointers to maps of the same size.
 * The boundary image of a map m, for every pixel (i, j):
 *   bound[i][j] = m[i][j] if m[i][j] < C and one of the four neighbours (i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1) that lie
 *   inside the map holds a byte other than m[i][j];  otherwise bound[i][j] = 255.
 * Bytes are compared raw: a "no class" byte (>= C) is never a boundary pixel and makes its class neighbours boundary pixels; pixels
 * outside the map do not exist, so the scene border is no boundary.  B_c(m), the pixels where bound equals c, is the inner boundary
 * of class c with 4-connectivity.  bound_cls receives the image of scene_cls, bound_pred that of scene_pred.
 * counts (nullable; DEVICE memory, int64 [C][4], 8-byte aligned) is ACCUMULATED into, as the confusion matrices are (zero it first):
 *   counts[c][0] += |B_c(pred)|     counts[c][1] += the x in B_c(pred) with some y in B_c(cls), (x - y) . (x - y) <= radius * radius
 *   counts[c][2] += |B_c(cls)|      counts[c][3] += the x in B_c(cls)  with some y in B_c(pred) within the same distance
 * summed over the scenes; radius 0 is exact coincidence.  One pass over each scene does all three.  Integers only, so
 * scenes.host_boundaries and scenes.host_boundary_counts give the same bytes and counts whatever the launch or arrival order.
 * Everything is checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the offender, nothing is
 * written): 0 <= radius <= 16, 1 <= C <= 64, nscenes >= 1, at least one of bound_cls, bound_pred and counts, no null entry in a
 * given pointer array, 1 <= H, W and H * W < 2^40, no output (a boundary map of any scene, the counts) sharing a byte with an
 * input of any scene of the call or with another output; inputs may share (one map scored against several).  The scenes travel as kernel arguments, 96 per launch (40 bytes each): no device-side table, no copy, no synchronisation. */
int rua_scene_boundary(const uint8_t* const* scene_cls, const uint8_t* const* scene_pred, const int32_t* scene_h, const int32_t* scene_w,
                       int nscenes, int radius, int C, uint8_t* const* bound_cls, uint8_t* const* bound_pred, int64_t* counts,
                       void* stream);

/* ---- connected regions of a class map and the sieve that removes the small ones (scenes.py, host_regions / host_region_counts /
 * host_sieve; the reference's utils.prediction cleans a prediction with an area opening before it scores it) -----------------------
 * scene_map / scene_h / scene_w are HOST arrays of nscenes entries, as rua_scene_erode reads them: device pointers to uint8
 * [scene_h[s]][scene_w[s]] maps.  A region is a maximal set of pixels of equal byte value connected through 4-neighbours
 * (connectivity 4) or 8-neighbours (8).  Bytes are compared raw, so "no class" bytes (>= C) form regions like any other; pixels
 * outside the map do not exist.  labels and areas (nullable) are HOST arrays of nscenes device pointers to int32 [H][W] arrays:
 *   labels[i][j] = the smallest row-major index i' * W + j' of the region of (i, j) - its root, canonical;
 *   areas[i][j]  = the pixel count of the region if (i, j) is its root (labels[i][j] == i * W + j), otherwise 0.
 * counts (nullable, needs areas; DEVICE memory, int64 [C][3], 8-byte aligned) is ACCUMULATED into, as the confusion matrices are
 * (zero it first), over the regions of every scene whose byte c is < C:
 *   counts[c][0] += 1     counts[c][1] += 1 if area < min_area     counts[c][2] += area if area < min_area
 * min_area and C are read only with counts.  Four launches per chunk of scenes whatever the maps hold (label each 32 x 32 tile in
 * LDS, join across tile seams with atomicMin on the int32 parents, flatten and sum the areas per tile, count): no block waits for
 * another, nothing is read back, and every walk through the forest strictly lowers an index.  Integers only, and a root is the
 * smallest index of its set, so scenes.host_regions and scenes.host_region_counts give the same bytes and counts whatever the launch
 * or arrival order.  Everything is checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the
 * offender, nothing is written): connectivity 4 or 8, nscenes >= 1, no null entry in a given pointer array, 1 <= H, W and
 * H * W < 2^31 (a label is an int32), labels and areas 4-byte aligned, with counts 1 <= min_area < 2^31 and 1 <= C <= 64, no output
 * (labels, areas, counts) sharing a byte with a map of the call or with another output.  The scenes travel as kernel arguments, 120
 * per launch (32 bytes each): no device-side table, no copy, no synchronisation. */
int rua_scene_regions(const uint8_t* const* scene_map, const int32_t* scene_h, const int32_t* scene_w, int nscenes, int connectivity,
                      int32_t* const* labels, int32_t* const* areas, int64_t min_area, int C, int64_t* counts, void* stream);

/* One round of scenes.host_sieve on maps whose labels and areas rua_scene_regions produced (same maps, same connectivity, earlier on
 * the same stream).  A region is SMALL if its byte c is < C, bit c of class_mask is set and its area is < min_area (min_area 1: none
 * is); every other region with a byte < C is KEPT; regions of bytes >= C are never changed and never donate.  scene_out is a HOST
 * array of nscenes device pointers to uint8 [H][W] maps:
 *   mode RUA_SIEVE_VOID: out = 255 on the pixels of small regions, the map's byte elsewhere;
 *   mode RUA_SIEVE_FILL: every small region takes one class for all its pixels.  One vote is cast for the byte of y per ordered
 *     pair (x in the region, y a 4-neighbour of x inside the map and in a kept region) - 4-neighbours also under connectivity 8 -;
 *     the class with the most votes wins, a tie goes to the lowest class, a region with no vote stays as it is.  All small regions
 *     decide at once, from the input map.
 * changed (nullable; DEVICE memory, one int64, 8-byte aligned) is ACCUMULATED into: the pixels whose byte changed.
 * work (mode fill; DEVICE memory, 4-byte aligned, work_bytes >= the sum over the scenes of rua_scene_sieve_work_bytes(H, W, C))
 * holds the votes: 12 bytes per pixel - at every region's root two uint32 vote counters, used alternately class after class, and
 * the best count so far; the winner itself collects in scene_out at the root.  Fill takes C + 3 launches per chunk of scenes, void
 * one, whatever the maps hold; the result does not depend on how the votes are kept.  Integers only: scenes.host_sieve gives the same
 * bytes whatever the launch or arrival order.  Everything is checked on the host before anything is launched (RUA_ERR_ARG, the
 * message names the offender, nothing is written): connectivity 4 or 8, 1 <= min_area < 2^31, 1 <= C <= 64, no bit >= C in
 * class_mask, mode 0 or 1, nscenes >= 1, no null entry in a pointer array, 1 <= H, W and H * W < 2^31, the work buffer in mode fill,
 * no output (scene_out, work, changed) sharing a byte with an input of any scene or with another output.  The scenes travel as
 * kernel arguments, 80 per launch (48 bytes each): no device-side table, no copy, no synchronisation. */
#define RUA_SIEVE_VOID 0
#define RUA_SIEVE_FILL 1
int rua_scene_sieve(const uint8_t* const* scene_map, const int32_t* scene_h, const int32_t* scene_w, int nscenes, int connectivity,
                    int64_t min_area, int C, uint64_t class_mask, int mode, const int32_t* const* labels, const int32_t* const* areas,
                    uint8_t* const* scene_out, void* work, int64_t work_bytes, int64_t* changed, void* stream);
/* bytes of work one H x W scene needs in mode fill (12 H W; -1 for sizes or a C the call would refuse) */
int64_t rua_scene_sieve_work_bytes(int H, int W, int C);

/* ---- the precision-recall sweep of one class's probabilities (scenes.py, sweep_levels / host_area_open / host_sweep_hist /
 * sweep_scores; the reference's matrics_AA_recall binarises at about 50 thresholds and area-opens each binary map) -----------------
 * scene_prob / scene_h / scene_w are HOST arrays of nscenes entries.  scene_prob[s] is a device pointer to the first byte of ONE
 * channel of a uint8 [H][W][pix_stride] map (1 <= pix_stride <= 64): pixel (i, j) is read at scene_prob[s][(i * W + j) * pix_stride],
 * so the seg map of rua_scene_stitch_maps is read where it lies; pix_stride 1 is a dense [H][W] map.  levels is a HOST array of T
 * bytes, strictly descending, each in 1..255; level t stands for "byte >= t".
 * rua_scene_area_open writes the OPENED map into scene_open (HOST array of device pointers to dense uint8 [H][W] maps):
 *   open[x] = the largest listed level t such that x lies in a connected component (connectivity 4 or 8) of {prob >= t} that has at
 *             least min_area pixels; 0 if there is none.
 * Thresholding commutes with the area opening and the kept sets are nested, so {open >= t} IS the area opening of {prob >= t} at
 * every listed t: one map serves the whole curve.  min_area 1: one streaming pass through a 256-entry table (the largest listed
 * level <= the byte), labels and areas are not read and may be null.  min_area > 1: labels and areas are work arrays (HOST arrays of
 * nscenes device pointers to int32 [H][W], 4-byte aligned, contents undefined afterwards); open is zeroed and, level after level, only
 * the still unsettled pixels U = {prob >= t and open == 0} are labelled: a block per 32 x 32 tile leaves at once if the tile holds
 * none, otherwise labels U in LDS; tile seams are joined with atomicMin on the int32 parents; a flatten pass sums the areas per tile
 * and marks (bit 31 of the areas word) the roots of components that touch a settled pixel; a last pass writes t on the pixels of U
 * whose component has min_area pixels or the mark.  One launch to zero and four per level and chunk of scenes, whatever the maps
 * hold; no block waits for another, nothing is read back, every walk through the forest strictly lowers an index.
 * rua_scene_sweep_hist ACCUMULATES into hist (DEVICE memory, int64 [2][2][256], 8-byte aligned; zero it first), over the pixels x of
 * every scene with scene_cls[s][x] < C (scene_cls: HOST array of device pointers to dense uint8 [H][W] class maps):
 *   hist[0][k][prob[x]] += 1      hist[1][k][open[x]] += 1      k = 1 if cls[x] == positive, else 0
 * scene_open null stands for prob itself (no area opening).  Suffix sums over the last index give TP, FP, FN and the pixels the
 * opening removed at every threshold at once (scenes.sweep_scores).  Integers only: scenes.host_area_open and scenes.host_sweep_hist
 * give the same bytes and counts whatever the launch or arrival order.
 * Everything is checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the offender, nothing is
 * written): 1 <= T <= 255 and the levels as above, 1 <= min_area < 2^31, connectivity 4 or 8, 1 <= pix_stride <= 64, 1 <= C <= 64,
 * 0 <= positive < C, nscenes >= 1, no null entry in a required array, 1 <= H, W and H * W < 2^31, the work arrays when min_area > 1,
 * hist's alignment, no output (open, labels, areas, hist) sharing a byte with an input of any scene or with another output.  The
 * footprint of scene_prob[s] runs from its first byte to the byte of its last pixel, (H * W - 1) * pix_stride + 1 bytes: the other
 * channels' bytes beyond it belong to the map, not to this channel.  The scenes travel as kernel arguments, 96 per launch of the
 * labelling kernels (40 bytes each), 120 of the table and histogram kernels: no device-side table, no copy, no synchronisation. */
int rua_scene_area_open(const uint8_t* const* scene_prob, const int32_t* scene_h, const int32_t* scene_w, int nscenes, int pix_stride,
                        const uint8_t* levels, int T, int64_t min_area, int connectivity, uint8_t* const* scene_open,
                        int32_t* const* labels, int32_t* const* areas, void* stream);
int rua_scene_sweep_hist(const uint8_t* const* scene_prob, const uint8_t* const* scene_open, const uint8_t* const* scene_cls,
                         const int32_t* scene_h, const int32_t* scene_w, int nscenes, int pix_stride, int positive, int C,
                         int64_t* hist, void* stream);

/* ---- instances from whole-scene maps: seeds, grow and the object match (scenes.py, host_seed_map / host_instances /
 * host_instance_match / instance_scores; the boundary and distance heads exist to tell touching objects of one class apart) ---------
 * One scene per call: ids and tables are per scene.  Every pointer is DEVICE memory.
 * rua_scene_seed_map: cls is a uint8 [H][W] class map, bound and dist (each nullable) uint8 [H][W][C] maps as rua_scene_stitch_maps
 * writes them, marker a uint8 [H][W] map:
 *   marker[x] = c = cls[x]  if c < C, bit c of class_mask is set, (bound null or bound[x][c] < bound_below) and
 *                              (dist null or dist[x][c] >= dist_at_least);      255 otherwise.
 * bound_below 1..256 (256 switches the test off), dist_at_least 0..255.  One streaming pass.
 * rua_scene_instances: labels and areas are what rua_scene_regions wrote for `marker` (same connectivity, earlier on the same
 * stream).  A SEED is a region of marker with a byte c < C and at least min_seed pixels; seeds are numbered 0..N-1 in ascending order
 * of their root.  inst is int32 [H][W]: a pixel x is ELIGIBLE if c = cls[x] < C and bit c of class_mask is set; its candidates are
 * the seed pixels y with marker[y] == c and (x - y) . (x - y) <= radius^2 (Euclidean, not geodesic; pixels outside the map do not
 * exist); inst[x] = the id of the candidate that minimises (squared distance, id) lexicographically, -1 if there is none and on every
 * pixel that is not eligible.  table is int32 [max_instances][8]; row k < min(N, max_instances) is written:
 *   root, class, area, seed_area, i_min, j_min, i_max, j_max     area and box over the pixels with inst == k
 * (an instance without a pixel: area 0, box H, W, -1, -1); rows from N on are not touched, inst always holds the true ids.
 * n is int32 [2]: n[0] = N, the uncapped seed count, n[1] = the eligible pixels with inst == -1.  work: 4-byte aligned, work_bytes >=
 * rua_scene_instances_work_bytes(H, W) (4 bytes per pixel and per chunk of 1024 pixels; -1 for sizes the call would refuse).
 * Four launches whatever the map holds: count the qualifying roots per chunk of 1024 pixels; ONE block scans the chunk counts (256
 * per pass, ceil(chunks / 256) passes) and writes N; every root takes its id and the fixed columns of its row; a block per
 * 32 x 32 tile stages ids and marker bytes of the tile and a halo of `radius` in LDS ((32 + 2 radius)^2 entries of 5 bytes), takes
 * the exact minimum of (d^2 << 32) | id over the disc - at most (2 radius + 1)^2 steps - for every eligible pixel and adds area and
 * box to the table per run of equal ids along a tile row.  No block waits for another, nothing is read back, integer atomics only:
 * scenes.host_instances gives the same bytes whatever the launch or arrival order.
 * rua_scene_instance_match: inst_p and inst_g are int32 [H][W] instance maps, area_p points to the area cell of row 0 of the
 * predicted table (row P's area is area_p[8 P]), match is int32 [Np][2]:
 *   match[P] = (g, inter)  if 2 |{x : inst_p[x] == P and inst_g[x] == g}| > area_P for some 0 <= g < Ng, inter being that count;
 *              (-1, 0)     otherwise.
 * Ids outside 0..Np-1 and 0..Ng-1 are no instance, so Np and Ng may be upper bounds of the true counts if the rows beyond hold
 * area 0.  The exact strict majority without a hash table or a sort: votes[P][b] counts the pixels of P whose ground-truth id has
 * bit b set (b < bit_length(Ng - 1)), the candidate is assembled from the bits with 2 votes > area_P, a second pass counts the pixels
 * of P on exactly that candidate, the last writes the row.  A strict-majority id collects more than half of P's pixels on each of its
 * set bits and fewer on every other, so the candidate is that id; without one the verification rejects whatever the bits spelled.
 * work: 4-byte aligned, work_bytes >= rua_scene_instance_match_work_bytes(Np, Ng) = 4 Np (bit_length(Ng - 1) + 2).  Five
 * launches (four when Ng <= 1, none when Np == 0), one atomic per run of equal (P, g) inside a wave.
 * Everything is checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the offender, nothing is
 * written): the required pointers, 1 <= H, W and H * W < 2^31, 1 <= C <= 64, no bit >= C in class_mask, bound_below, dist_at_least,
 * 1 <= min_seed < 2^31, 0 <= radius <= 16, 1 <= max_instances < 2^31, 0 <= Np, Ng < 2^31, 4-byte alignment of every int32 array,
 * the work buffers, no output sharing a byte with an input or with another output of the call. */
int rua_scene_seed_map(const uint8_t* cls, const uint8_t* bound, const uint8_t* dist, int H, int W, int C, uint64_t class_mask,
                       int bound_below, int dist_at_least, uint8_t* marker, void* stream);
int64_t rua_scene_instances_work_bytes(int H, int W);
int rua_scene_instances(const uint8_t* cls, const uint8_t* marker, const int32_t* labels, const int32_t* areas, int H, int W, int C,
                        uint64_t class_mask, int64_t min_seed, int radius, void* work, int64_t work_bytes, int32_t* inst, int32_t* table,
                        int64_t max_instances, int32_t* n /* device int32[2]: N, ungrown */, void* stream);
int64_t rua_scene_instance_match_work_bytes(int64_t Np, int64_t Ng);
int rua_scene_instance_match(const int32_t* inst_p, const int32_t* area_p /* table_p, column 2 */, int64_t Np, const int32_t* inst_g,
                             int64_t Ng, int H, int W, void* work, int64_t work_bytes, int32_t* match, void* stream);

/* ---- flooding: a bounded, marker-controlled watershed of a height map in synchronous rounds (scenes.py, host_flood) ----------------
 * One scene per call.  Every pointer is DEVICE memory.  cls is the uint8 [H][W] class map, inst the int32 [H][W] id map that
 * rua_scene_instances left (any radius), changed in place: a pixel with inst >= 0 is SETTLED and never changes; a pixel is ELIGIBLE
 * if c = cls[x] < C and bit c of class_mask is set.  The height of pixel x is 255 with height == NULL, else the byte
 * height[x * pix_stride + (per_class ? cls[x] : 0)]: pix_stride 1 for a [H][W] map, C with per_class 1 for the [H][W][C] maps
 * rua_scene_stitch_maps writes.  The schedule is R = (256 - floor) * rounds_per_level + drain rounds: the levels t = 255, 254, ..,
 * floor, each rounds_per_level times, then `drain` more rounds at level floor.  One round at level t, every decision reading the
 * state at the start of the round: an eligible, unsettled pixel x with height(x) >= t that has at least one settled neighbour y
 * (under `connectivity`; pixels outside the map do not exist) with cls[y] == cls[x] takes the smallest id among those neighbours.
 * Nothing else changes.  stats is int32 [2]: the pixels the flood settled, and 1 + the index of the last round that settled one (0
 * if none did; equal to R, the schedule may have cut the flood short).
 * With a table (int32 [max_instances][8], rua_scene_instances' own, n its int32 [2]): after the last round the columns area and
 * i_min, j_min, i_max, j_max of the rows below min(n[0], max_instances) are rewritten from the final inst (ids from there on have no
 * row), and n[1] is recounted: the eligible pixels with inst < 0.  Root, class and seed area stay.  table == NULL skips that pass;
 * n may then be NULL and is not touched.
 * work: 4-byte aligned, work_bytes >= rua_scene_flood_work_bytes(H, W): a second int32 map and a flag per 32 x 32 tile (-1 for sizes
 * the call would refuse).  A launch runs 8 rounds: a block per tile stages ids, class bytes and height bytes of the tile and a halo
 * of 8 pixels in LDS, runs the rounds there and writes its interior to the OTHER id map - the maps alternate, the result ends in
 * inst, and no block reads what another block of the same launch writes.  A tile without an eligible unsettled pixel costs a copy,
 * and nothing once both maps hold it.  ceil(R / 8) launches plus at most four, whatever the map holds; nothing is read back, no block
 * waits for another, integer atomics only: scenes.host_flood gives the same bytes.
 * Everything is checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the offender, nothing is
 * written): the required pointers, 1 <= H, W and H * W < 2^31, 1 <= C <= 64, no bit >= C in class_mask, connectivity 4 or 8,
 * 1 <= rounds_per_level <= 16, 0 <= floor <= 255, 0 <= drain <= 4096, with a height per_class 0 or 1 and 1 <= pix_stride <= 256
 * (>= C with per_class), with a table 1 <= max_instances < 2^31, 4-byte alignment of every int32 array, the work buffer, no output
 * sharing a byte with an input or with another output of the call. */
int64_t rua_scene_flood_work_bytes(int H, int W);
int rua_scene_flood(const uint8_t* cls, const uint8_t* height /* or NULL */, int pix_stride, int per_class,
                    int H, int W, int C, uint64_t class_mask, int connectivity, int rounds_per_level, int floor, int drain,
                    void* work, int64_t work_bytes, int32_t* inst /* in, out */, int32_t* table /* or NULL */, int64_t max_instances,
                    int32_t* n /* device int32[2] of rua_scene_instances: n[1] (ungrown) is rewritten */,
                    int32_t* stats /* device int32[2]: settled, last_round */, void* stream);

/* ---- outlines of whole-scene instance maps: one closed ring of grid corners per object piece and per hole (scenes.py, host_outlines /
 * outline_polygons / write_geojson) ------------------------------------------------------------------------------------------------
 * One map per call.  Every pointer is DEVICE memory.  inst is an int32 [H][W] id map (rua_scene_instances' inst, or any other): an id
 * >= 0 is an object, a negative id is none.  A vertex is a grid corner (y, x), 0 <= y <= H, 0 <= x <= W; pixel (i, j) is the square
 * between (i, j) and (i+1, j+1).  Pixel p = (i, j) with id k >= 0 owns a directed EDGE on side s (0 top, 1 right, 2 bottom, 3 left) if
 * the pixel across that side lies outside the map or has another id; the pixel is on the right of the direction of travel:
 *   s = 0: (i, j) -> (i, j+1)    s = 1: (i, j+1) -> (i+1, j+1)    s = 2: (i+1, j+1) -> (i+1, j)    s = 3: (i+1, j) -> (i, j)
 * Its key is 4 (i W + j) + s.  With F the pixel one step along the heading from p and L the pixel across side s from F, the
 * SUCCESSOR of (p, s) is (L, s+3 mod 4) if F and L have id k; else (F, s) if F has; else (L, s+3 mod 4) if connectivity is 8 and L
 * has; else (p, s+1 mod 4).  The cycles of the successor are the RINGS.  A CORNER edge is one whose successor has another side; its
 * vertex is its end point.  A ring's leader is its edge of smallest key; its vertices are those of its corner edges in walking order
 * from the leader; rings are ordered by leader key.
 * rua_scene_outline_count writes base int32 [H][W], base[p] = the number of edges of all pixels before p in row-major order, and
 * n int64 [2] = (E, V): the edges and the corner edges of the map.  Three launches.
 * rua_scene_outline_rings takes the same inst and connectivity, that base, and E and V as the host read them from n.  It writes
 *   rings int32 [V / 4][6]: rows 0..R-1 = (id, leader key, vertex offset, vertex count, area, length); rows from R on are not touched
 *   verts int32 [V][2]:     the rings' vertices (y, x), ring after ring
 *   nr    int64 [1]:        R
 * length is the ring's number of edges; area its signed enclosed area in pixels - the sum of (i + 1) over its side-2 edges minus the
 * sum of i over its side-0 edges -, positive for an outer ring (clockwise with rows pointing down), negative for a hole.  A ring has an
 * even number of at least 4 vertices, none of them collinear with its neighbours.  With E == 0 only nr = 0 is written (one launch;
 * work, rings and verts may be null); otherwise 2 ceil(log2 E) + 10 launches: the edges are compacted in key order, the leader of
 * every cycle is found by pointer jumping on (min, hop) records, the cycles are cut in front of their leaders and ranked by the same
 * jumping on (sum, hop) records, the leaders are numbered with a chunk scan, counts, areas and lengths are added with integer
 * atomics, and the corner edges scatter their end points.  scenes.host_outlines gives the same bytes whatever the launch or arrival
 * order.  E and V that do not belong to (inst, base) give meaningless rings, but nothing outside the buffers is read or written.
 * work: 16-byte aligned, work_bytes >= rua_scene_outline_work_bytes(H, W, E) - E = 0 for the count: 8 bytes per chunk of 1024 pixels;
 * for the rings 24 bytes per edge (key, successor / leader, two 8-byte jumping records) and 5 per 1024 edges; -1 for sizes the calls
 * would refuse.
 * Everything is checked on the host before anything is launched (a violation: RUA_ERR_ARG, the message names the offender, nothing is
 * written): the required pointers, 1 <= H, W and H * W <= 2^29 (keys and areas fit an int32), connectivity 4 or 8, 0 <= E <= 4 H W,
 * V even and 4 <= V <= E (V == 0 with E == 0), 4-byte alignment of inst, base and rings, 8-byte alignment of verts, n and nr, the work
 * buffer, no output sharing a byte with an input or with another output of the call. */
int64_t rua_scene_outline_work_bytes(int H, int W, int64_t E);
int rua_scene_outline_count(const int32_t* inst, int H, int W, int connectivity, int32_t* base, void* work, int64_t work_bytes,
                            int64_t* n /* device int64[2]: E, V */, void* stream);
int rua_scene_outline_rings(const int32_t* inst, const int32_t* base, int H, int W, int connectivity, int64_t E, int64_t V, void* work,
                            int64_t work_bytes, int32_t* rings, int32_t* verts, int64_t* nr /* device int64[1]: R */, void* stream);

/* ---- data parallel (train_ISPRS.py:347,432: the implicit NCCL all-reduce of tf.distribute.MirroredStrategy).  The library exports
 * no collective: gradients live in ONE flat fp32 buffer in parameter order, so the all-reduce is ncclAllReduce (RCCL) on contiguous
 * slices of it, issued by the host as the backward completes them (the Python engine: torch.distributed, dist.py; a C embedder:
 * INTEGRATION.md section 2).  rua_adam_step / rua_sgd_step take grad_scale = 1 / replicas. */

/* kernel nodes / all nodes of a captured hipGraph_t (diagnostics: dispatches per whole-step graph) */
int rua_graph_kernel_nodes(void* graph, int* kernels, int* total);

/* ---- tuning switches (experiments, A/B runs).  The launchers never read the environment and keep no other global
 * state: a heuristic changes only through this call.  Keys: rua_tuning_key(0..) until NULL.  Grid-size keys
 * ("*_blocks", "*_target", "*_grid") default to 0 = derived from the device's compute-unit count.
 * The keys (meaning and default of each: struct RuaTuning, csrc/common.h; any other name is RUA_ERR_ARG):
 *   conv_force_bn, conv_force_bm, conv_dma, conv_pw, conv_pw_minm, conv_pw_blocks, conv_halo, conv_dmap,
 *   dmap_target, dmap_fused_finish, dmap_rowb, dmap_bm64, wgrad_pw, wgpw_blocks, wgpw_r, wgd_blocks,
 *   wgrad_dmap, wgd_mintiles, wgrad_blocks, bn_grid, tani_vec, metrics_blocks, stem_blocks, head_blocks,
 *   conv_img, conv_strip, wgrad_slabs, strip_narrow_maxd, conv_group, wgrad_group, wgrad_batch_blocks,
 *   wgd_ks_slow, head_fwd2, head_fwd3, head_fwd3_bpc, stem_reg, stats_blocks, conv_band, conv_band64,
 *   conv_band64m, strip_group_share, band_dbg, fill_kernel, bn_regs, wgrad_taps_share, dmap_chain, epi_fast,
 *   dmap_spread, bn_bwd_group, conv_small, strip_stag, cu_reserve, wgrad_rows, strip_seglen, band_stag,
 *   conv_band128m, conv_img2, bn_sliced, bn_sliced_parts, bn_sliced_s, dbg_ptr */
int rua_set_tuning(const char* key, int64_t value);
int rua_get_tuning(const char* key, int64_t* value);
const char* rua_tuning_key(int index);

#ifdef __cplusplus
}
#endif
#endif

/*
 * dmc.h — C ABI of libdmc.so, the MI355X (gfx950) kernels behind the diffusion hot path.
 *
 * The reference (sunyzhi55/Diffusion_Models_Collection) is pure Python over PyTorch and has no
 * FFI layer of its own; every entry point below replaces a group of PyTorch eager
 * ops that the reference calls at the cited file:line. The Python host side
 * (diffusion_models_collection_amd/_lib.py) binds these with ctypes.
 *
 * Conventions
 *   - All pointers are device pointers unless stated; `stream` is a hipStream_t (NULL = default).
 *   - The library never allocates and never synchronises: callers pass every output and workspace
 *     buffer. Its only mutable global state is the launch-option table below (read from the
 *     environment once, then changed only by dmc_set_option). Calls are graph-capturable.
 *   - Return 0 on success, nonzero on a bad descriptor or launch error; dmc_last_error() explains.
 *   - Activations are NHWC (pixel rows, channel pitch `ld`); dtype is DMC_F32 (parity mode) or
 *     DMC_BF16 (perf mode). Statistics, biases, gradients of weights and reductions are fp32.
 */
#ifndef DMC_H
#define DMC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { DMC_F32 = 0, DMC_BF16 = 1 };
enum { DMC_MODE_NORMAL = 0, DMC_MODE_UPSAMPLE = 1, DMC_MODE_DILATE = 2 };
enum { DMC_PRO_NONE = 0, DMC_PRO_AFFINE_SILU = 1, DMC_PRO_SILU = 2, DMC_PRO_AFFINE = 3, DMC_PRO_GN_SILU = 4 };
/* DMC_PRO_GN_SILU (round 6): SiLU(GroupNorm(x)) with the GroupNorm statistics computed inside the conv from the
 * source images themselves (models/unet.py:35-36 / :51-52 at inference): pro_scale = gamma [C], pro_shift = beta [C],
 * pro_groups = G, pro_eps = eps; no dropout. Only the whole-image small-map conv (4x4 / 8x8 maps) takes it:
 * dmc_conv_halo_prologue() says whether a descriptor can be run this way, dmc_conv2d fails otherwise. */
enum { DMC_LOSS_L1 = 0, DMC_LOSS_L2 = 1, DMC_LOSS_HUBER = 2 };
enum { DMC_PRED_EPS = 0, DMC_PRED_V = 1 };   /* what the network predicts: the noise, or v = alpha*eps - sigma*x0 */
#define DMC_OBJECTIVE_MAX_BLOCKS 64          /* dmc_objective: partial sums per sample, at most */
#define DMC_VLB_MAX_BLOCKS 64                /* dmc_vlb_step: blocks per sample, at most (four partial sums each) */
#define DMC_VLB_WORKSPACE_FLOATS(N) (4 * DMC_VLB_MAX_BLOCKS * (size_t)(N))   /* dmc_vlb_step's workspace */
enum { DMC_PACK_FWD = 0, DMC_PACK_DGRAD = 1, DMC_PACK_UPDGRAD = 2, DMC_PACK_UPFOLD = 3, DMC_PACK_DOWNDGRAD = 4 };
/* Output-parity folds of the two resampling convs (dmc_conv_desc.fold, see dmc_conv_resample_fold). */
enum { DMC_FOLD_NONE = 0, DMC_FOLD_UP = 1, DMC_FOLD_DOWN_DGRAD = 2 };

int dmc_version(void);
const char* dmc_last_error(void);

/* Launch-plan options (A/B switches for measurement and tests, e.g. "DMC_NO_HALO"). The table is read once
 * per process from the environment variables of the same names; afterwards only these calls change it.
 * dmc_set_option returns nonzero for an unknown name; dmc_get_option returns -1 for one. */
int dmc_set_option(const char* name, long value);
long dmc_get_option(const char* name);
void dmc_reset_options(int from_env);

/* Implicit-GEMM convolution descriptor. Replaces nn.Conv2d / nn.Linear forward and input-gradient
 * of models/unet.py:34-60 (ResidualBlock), :81-82 (qkv/proj), :106 (Downsample), :116 (Upsample +
 * F.interpolate nearest), :167-172 (time_embed Linears), :188 (input_conv), :237-241 (output), and
 * the torch.cat skip concatenation of :284 (two sources = virtual concat).
 * Input coordinate of output pixel (oy,ox) and tap t: (oy*stride + tap_dy[t], ox*stride + tap_dx[t]),
 * then mode UPSAMPLE: valid in [0,2H) and >>1 (nearest x2); DILATE: valid iff even, /2 (the
 * transposed stride-2 conv of a dgrad); NORMAL: valid in [0,H). Invalid taps read zero.
 */
typedef struct dmc_conv_desc {
  int dtype;
  int N, H, W;               /* source batch and spatial size */
  int C1, C2, ld1, ld2;      /* channels [0,C1) from x1, [C1,C1+C2) from x2 (virtual concat) */
  int Kc;                    /* packed K per tap: >= C1+C2, multiple of 32 (fp32) / 64 (bf16) */
  int OH, OW, Cout;
  int ntaps, mode, stride;
  int tap_dy[16], tap_dx[16];
  int prologue;              /* DMC_PRO_*: applied to the sources while staging (never to padding) */
  const float* pro_scale;    /* [N][ld_pro] per-(n,c): a = x*scale + shift (GroupNorm folded) */
  const float* pro_shift;
  int ld_pro;
  uint32_t drop_seed;        /* dropout after SiLU: keep iff hash(seed, pix*C + c) >= drop_thresh */
  uint32_t drop_thresh;      /* 0 = no dropout */
  float drop_scale;          /* 1/(1-p) */
  int drop_ld;               /* channel count used in the dropout element index */
  const uint32_t* drop_seed_base; /* device word added to drop_seed when not NULL (seed varies per graph replay) */
  const float* bias;         /* [Cout] or NULL */
  const float* addvec;       /* [N][ld_add] added per (n, co) (time/label embedding) or NULL */
  int ld_add;
  const void* resid;         /* residual [pix][ld_res] in the output dtype (with out_nchw: fp32 NCHW, laid out as y1),
                              * or NULL. Added last before `act`: out = (acc + bias + addvec) * silu'(silu_pre) + resid */
  int ld_res;
  const float* silu_pre;     /* if set, (acc + bias + addvec) *= silu'(silu_pre[pix][ld_silu]) (fp32), before the
                              * residual is added: a gradient accumulated in `resid` is not scaled by this SiLU */
  int ld_silu;
  int Csplit;                /* co < Csplit -> y1[pix*ldy1 + co], else y2[pix*ldy2 + co - Csplit] */
  int ldy1, ldy2;
  int out_f32;               /* output stored fp32 even in bf16 mode */
  int out_nchw;              /* y1 is NCHW fp32 [N][Cout][OH][OW] */
  int act;                   /* DMC_ACT_*: activation applied last (after bias / addvec / resid) */
  void* y_pre;               /* with act: the pre-activation value is also stored here ([pix][ld_pre], output dtype) */
  int ld_pre;
  float* gn_part;            /* if set: GroupNorm partial statistics of the stored output y1 (the input of the next
                              * GroupNorm, models/unet.py:34/:84), [M/64][Cout/8][2] = (mean, M2) over 64 pixels x 8
                              * channels, from the kernel's epilogue where it can, else one pass over y1. Needs
                              * OH*OW % 64 == 0, Cout % 8 == 0, one NHWC output. Finalised by dmc_gn_finalize. */
  float* wg_bias;            /* dmc_conv2d_wgrad only: if set, also the bias gradient wg_bias[co] = scale * sum over
                              * pixels of dy[pix][co] (nn.Conv2d bias), from the same pass over dy */
  int pro_groups;            /* DMC_PRO_GN_SILU: GroupNorm groups G (C / G channels per group) */
  float pro_eps;             /* DMC_PRO_GN_SILU: GroupNorm eps */
  int fold;                  /* DMC_FOLD_*: w is the class-ordered pack (DMC_PACK_UPFOLD / DMC_PACK_DOWNDGRAD) and the conv
                              * runs as four output-parity classes in one launch. Set it only to what
                              * dmc_conv_resample_fold() answered for the same descriptor; dmc_conv2d fails otherwise. */
} dmc_conv_desc;
enum { DMC_ACT_NONE = 0, DMC_ACT_GELU = 1, DMC_ACT_GELU_DROP = 2, DMC_ACT_DGELU = 3 };
/* DGELU: the backward of GELU_DROP / GELU on an input-gradient conv: out = round(acc) * mask * scale * gelu'(u) with
 * u = y_pre[pix][ld_pre] READ (the stored pre-activation), the mask from the drop_* fields as for GELU_DROP (none if
 * drop_thresh == 0) -- bitwise dmc_gelu_bwd of the conv's stored output.
 * GELU (exact): the DiT MLP (dit.py:98-99). GELU_DROP: GELU, then the MLP's Dropout with the descriptor's drop_*
 * fields (prologue must be DMC_PRO_NONE): element (pix, co) kept iff hash(seed, pix*Cout + co) >= drop_thresh, kept
 * values scaled by drop_scale -- bitwise dmc_gelu_fwd with the same dropout of the stored pre-activation. */

/* y = conv(x) with fused prologue/epilogue. w = packed [Cout][ntaps][Kc] (dtype).
 * workspace (dmc_conv2d_workspace() bytes, may be 0) enables split-K for small-M shapes; with a NULL
 * or too small workspace the call still succeeds without split-K. */
size_t dmc_conv2d_workspace(const dmc_conv_desc* d);
/* 1 when dmc_conv2d runs `d` (bf16 3x3 stride-1, prologue DMC_PRO_AFFINE_SILU, no dropout) on the halo kernel
 * with SiLU(x*scale+shift) applied to the LDS-resident activation halo, so the caller need not materialise the
 * GroupNorm output first (inference; replaces the GroupNorm -> SiLU -> Conv2d chain of models/unet.py:34-37,
 * :55-60 without the intermediate tensor). 0 otherwise (dmc_conv2d then uses the register-staged kernel).
 * Default since round 2 (DMC_HALO_PRO=0 turns it off): with the GroupNorm statistics from the producing conv's
 * epilogue the activation is not read before this conv at all. With prologue DMC_PRO_GN_SILU (round 6): 1 when the
 * small-map conv takes `d` with the GroupNorm statistics computed in the conv itself (no statistics, finalize or
 * apply launch before it), 0 when dmc_conv2d would reject it. */
int dmc_conv_halo_prologue(const dmc_conv_desc* d);
/* Which of the optional outputs dmc_conv2d(d, ..., ws_bytes) produces inside its kernel's epilogue (bit mask), as
 * opposed to one extra pass over the stored output: DMC_FUSED_GN_STATS (gn_part). */
int dmc_conv2d_fused_epilogue(const dmc_conv_desc* d, size_t ws_bytes);
enum { DMC_FUSED_GN_STATS = 1 };
/* The launch plan dmc_conv2d(d, ..., ws_bytes) follows, computed on the host without touching a device (d->gn_part
 * != NULL is the request for the GroupNorm partials, as in dmc_conv2d). The three queries above report fields of
 * the same plan. Returns nonzero (dmc_last_error) where dmc_conv2d would reject the descriptor. */
enum { DMC_CONV_NONE = 0,        /* empty problem: nothing is launched */
       DMC_CONV_NIN_HALO = 1,    /* halo'd narrow-input 3x3 */
       DMC_CONV_NOUT_HALO = 2,   /* halo'd narrow-output 3x3 */
       DMC_CONV_NARROW_IN = 3,   /* generic narrow-input */
       DMC_CONV_NARROW_OUT = 4,  /* generic narrow-output */
       DMC_CONV_IMG = 5,         /* whole-image small-map 3x3 (4x4 / 8x8) */
       DMC_CONV_GEMM1X1 = 6,     /* 1x1 GEMM: persistent, or whole-K (dmc_conv_plan.whole_k) */
       DMC_CONV_HALO = 7,        /* 128-pixel halo 3x3 */
       DMC_CONV_GLDS = 8,        /* LDS-DMA implicit GEMM */
       DMC_CONV_REG = 9 };       /* register-staged implicit GEMM */
enum { DMC_GN_PART_NONE = 0,     /* not requested */
       DMC_GN_PART_KERNEL = 1,   /* the conv kernel's epilogue (DMC_FUSED_GN_STATS) */
       DMC_GN_PART_SPLITK = 2,   /* the split-K reduction's epilogue */
       DMC_GN_PART_PASS = 3 };   /* a separate pass over the stored output */
typedef struct dmc_conv_plan {
  int family;                /* DMC_CONV_* */
  unsigned grid[3];          /* grid (blocks) and block size (threads) of the main launch */
  int block;
  int splits;                /* split-K factor (1: none; > 1: a reduction launch follows) */
  int gn_part;               /* DMC_GN_PART_* */
  int fused_prologue;        /* what dmc_conv_halo_prologue answers */
  size_t ws_bytes;           /* what dmc_conv2d_workspace answers */
  int whole_k;               /* DMC_CONV_GEMM1X1: DMC_WK_* when the whole-K form runs (one tile per block, its whole K in
                              * LDS; with `block` > the tile's 64 threads per 64x64 wave tile: one wave per run of
                              * the split-K plan it replaces), 0 for the persistent GEMM and every other family */
} dmc_conv_plan;
enum { DMC_WK_64X128 = 1, DMC_WK_64X64 = 2 };   /* pixels x channels of the whole-K form's tile */
int dmc_conv2d_plan(const dmc_conv_desc* d, size_t ws_bytes, dmc_conv_plan* out);
/* Which output-parity fold (DMC_FOLD_*) dmc_conv2d(d, ..., ws_bytes) can run `d` (written with fold = 0) as:
 *   DMC_FOLD_UP          the forward of models/unet.py:116 (nearest x2, then 3x3 pad 1; mode UPSAMPLE, 9 forward taps):
 *                        output pixel (2i+a, 2j+b) is a 2x2-tap stride-1 conv of the low-resolution input with the 3x3
 *                        weights that read the same low-resolution pixel summed (DMC_PACK_UPFOLD);
 *   DMC_FOLD_DOWN_DGRAD  the input gradient of the stride-2 3x3 conv of models/unet.py:106 (mode DILATE, 9 flipped taps):
 *                        dx(2i+a, 2j+b) takes only the 1, 2, 2 or 4 taps that meet a non-zero of the zero-stuffed dy
 *                        (DMC_PACK_DOWNDGRAD), in the original tap order: the same bits as the dilated form.
 * 0 where the conv keeps its plain form: DMC_RESAMPLE_FOLD = 0 (default 1: both; 2: UP only; 3: DOWN_DGRAD only), fp32, channel
 * counts that are no multiple of 64, odd sizes, a split-K plan, outputs other than one bf16 NHWC tensor, and for UP a
 * low-resolution image that is no multiple of 64 pixels (the GroupNorm partials keep 64-pixel segments per image).
 * The caller then sets d->fold to the answer and passes the matching pack. Host only. */
int dmc_conv_resample_fold(const dmc_conv_desc* d, size_t ws_bytes);
int dmc_conv2d(const dmc_conv_desc* d, const void* x1, const void* x2, const void* w,
               void* y1, void* y2, void* workspace, size_t ws_bytes, void* stream);

/* Weight gradient of the same convolution: dw[co][c][t] (fp32, reference nn.Conv2d layout,
 * multiplied by `scale`) = sum over pixels of dy[pix][co] * prologue(x)[coord(pix,t)][c].
 * dy: [N*OH*OW][ld_dy] dtype. workspace: dmc_conv2d_wgrad_workspace() bytes. */
size_t dmc_conv2d_wgrad_workspace(const dmc_conv_desc* d);
int dmc_conv2d_wgrad(const dmc_conv_desc* d, const void* dy, int ld_dy, const void* x1,
                     const void* x2, void* workspace, float* dw, float scale, void* stream);
/* The same weight gradient in two parts: dmc_conv2d_wgrad_partial launches only the kernel that writes the per-split
 * fp32 partial sums into `workspace` and fills *job (a HOST struct) with the reduction that finishes dw (and
 * d->wg_bias); dmc_wgrad_reduce_batch then runs up to 32 such reductions in ONE launch (jobs: HOST array; each
 * job's workspace must stay untouched until it ran). Bitwise what dmc_conv2d_wgrad computes -- which is exactly
 * partial + a one-job batch. The executor batches a backward segment's weight gradients this way (the per-layer
 * reduce launches of the CIFAR step: 90 -> 3). */
typedef struct dmc_wgrad_job {
  const float* slab;         /* layout 0: [splits][KK][Cpad] partial sums; layout 1: [splits][Cout][Ctot][ntaps] */
  const float* bslab;        /* [splits][Cpad] bias partials (NULL: no bias gradient) */
  float* dw;                 /* fp32 [Cout][Ctot][ntaps] */
  float* dbias;              /* fp32 [Cout] or NULL */
  int splits, KK, Cpad, Cout, Ctot, ntaps, Kc;
  float scale;
  int layout;                /* the slab layout the weight-gradient kernel wrote (library-internal choice) */
} dmc_wgrad_job;
int dmc_conv2d_wgrad_partial(const dmc_conv_desc* d, const void* dy, int ld_dy, const void* x1, const void* x2,
                             void* workspace, float* dw, float scale, dmc_wgrad_job* job, void* stream);
int dmc_wgrad_reduce_batch(const dmc_wgrad_job* jobs, int njobs, void* stream);
/* The launch plan dmc_conv2d_wgrad / dmc_conv2d_wgrad_partial(d, dy, ld_dy, ...) follow, computed on the host without
 * touching a device: the kernel kind, the main launch, the split count (0: the kernel reduces itself, the returned job
 * is empty) and the slab layout of the returned job. group_kind is what dmc_conv2d_wgrad_group_ok(d, ld_dy) answers,
 * ws_bytes what dmc_conv2d_wgrad_workspace(d) answers: reads of the same plan. Returns nonzero (dmc_last_error) where
 * dmc_conv2d_wgrad would reject the descriptor or ld_dy. */
enum { DMC_WGRAD_IMG4 = 1,       /* whole-image 4x4 3x3: no slab, no reduction */
       DMC_WGRAD_PIPE = 2,       /* pipelined 3x3 on 32 / 16 / 8 / 4-wide maps */
       DMC_WGRAD_HALO = 3,       /* 256-pixel halo 3x3 */
       DMC_WGRAD_GEMM1X1 = 4,    /* LDS-DMA 1x1 / Linear */
       DMC_WGRAD_GENERIC = 5 };  /* register-staged, everything else */
typedef struct dmc_wgrad_plan {
  int kind;                  /* DMC_WGRAD_* */
  unsigned grid[3];          /* grid (blocks) and block size (threads) of the partial-sum launch */
  int block;
  int splits;
  int layout;                /* dmc_wgrad_job.layout */
  int group_kind;
  size_t ws_bytes;
} dmc_wgrad_plan;
int dmc_conv2d_wgrad_plan(const dmc_conv_desc* d, int ld_dy, dmc_wgrad_plan* out);

/* Grouped weight gradients: the partial-sum kernels of up to DMC_WGRAD_GROUP_MAX convs in shared launches. Every
 * job must be one dmc_conv2d_wgrad_group_ok accepts: bf16, and either 3x3 stride 1 with the forward taps, maps 32, 16
 * or 8 wide, 64-aligned channel sources, ld_dy % 8 == 0 (returns the map width), or 1x1 stride 1 with N*H*W % 64 == 0,
 * 8-aligned channels and pitches and a second source only behind a 128-aligned first one (returns 1); 0 otherwise.
 * All jobs of a call share that return value (1x1 jobs of different map sizes do);
 * N, C1 / C2, Cout (ragged and narrow in a padded pitch included) and d->wg_bias may differ. With the block count of
 * one conv's launch spread over the group, each conv is split 1 / njobs as often over its pixels: its slab, its share
 * of the reduction and its store burst shrink by that factor. The summation order is fixed (bitwise reproducible), and
 * a launch of one job (3x3 or 1x1) has the single-layer plan: bitwise dmc_conv2d_wgrad_partial of it. jobs[i] (HOST
 * array of njobs) receives job i's reduction for dmc_wgrad_reduce_batch; items[i].workspace needs bytes[i] of dmc_conv2d_wgrad_group_workspace (which
 * returns their sum, 0 if the items are no valid group) and must stay untouched until that reduction ran. */
#define DMC_WGRAD_GROUP_MAX 8
typedef struct dmc_wgrad_group_item {
  const dmc_conv_desc* d;
  const void* dy;
  int ld_dy;
  const void* x1;
  const void* x2;
  void* workspace;
  float* dw;
  float scale;
} dmc_wgrad_group_item;
int dmc_conv2d_wgrad_group_ok(const dmc_conv_desc* d, int ld_dy);
size_t dmc_conv2d_wgrad_group_workspace(const dmc_wgrad_group_item* items, int njobs, size_t* bytes);
int dmc_conv2d_wgrad_group(const dmc_wgrad_group_item* items, int njobs, dmc_wgrad_job* jobs, void* stream);
/* Bytes of split partial sums (the fp32 weight slabs) the weight-gradient launches of this process have planned
 * since the last reset; reset != 0 returns the count and clears it. Host-side bookkeeping, no GPU work. */
long dmc_wgrad_slab_bytes(int reset);

/* Repack an fp32 nn.Conv2d / nn.Linear weight [Cout][Cin][kh][kw] into the kernel layout:
 * FWD [Cout][t][Kc], DGRAD [Cin][t][Kc>=Cout], UPDGRAD [Cin][16][Kc] (nearest-x2 + 3x3 folded
 * into a 4x4 stride-2 kernel). Padding is zero-filled. */
/* DMC_PACK_UPFOLD: [class a*2+b][Cout][4 taps r*2+c][Kc], each the fp32 sum (ascending 3x3 tap order) of the weights
 * whose tap reads low-resolution offset (a-1+r, b-1+c), rounded once. DMC_PACK_DOWNDGRAD: [class][Cin][taps][Kc] with
 * 1, 2, 2, 4 taps for classes 0..3 (class bases 0, 1, 3, 5 x Cin x Kc), the class's 3x3 taps in ky-major order. */
int dmc_pack_weight(int pack_mode, int dtype, const float* w, int Cout, int Cin, int kh, int kw,
                    int Kc, void* dst, void* stream);
/* Batched repack of every stale weight in one launch (the per-step refresh after optimizer.step;
 * replaces one dmc_pack_weight per conv and mode). Each job is cut into tiles on the host
 * (dmc_pack_tiles: {job index, a, b} int triples); `jobs` and `tiles` are DEVICE arrays.
 * koff < 0: the job writes its whole rows including the zero padding of Kc; koff >= 0 (a DGRAD of a
 * row-concatenation, e.g. the 22 time_mlp weights of models/unet.py:40-43 as one GEMM, or a Kc = 1
 * FWD "pack" = copy into a concatenated bias): only its own column block [koff, koff + extent). */
typedef struct dmc_pack_job {
  const float* w;            /* fp32 master weight [Cout][Cin][kh][kw] */
  void* dst;                 /* packed [rows][ntaps][Kc] of dtype */
  int dtype, mode, Cout, Cin, kh, kw, Kc, koff;
} dmc_pack_job;
int dmc_pack_tiles(const dmc_pack_job* job, int job_index, int* tiles, int cap);   /* HOST pointers */
int dmc_pack_weights(const dmc_pack_job* jobs, const int* tiles, int ntiles, void* stream);

/* GroupNorm statistics (models/unet.py:35,51,80,238; eps 1e-5) over the virtual concat of x1/x2:
 * mean_rstd [N][G][2]; scale/shift [N][C] = folded affine for the consumer's prologue.
 * workspace: dmc_gn_workspace() bytes. */
size_t dmc_gn_workspace(int N, int C, int G, int HW);
int dmc_gn_stats(int dtype, const void* x1, const void* x2, int N, int HW, int C1, int C2, int ld1,
                 int ld2, int G, float eps, const float* gamma, const float* beta, void* workspace,
                 float* mean_rstd, float* scale, float* shift, void* stream);

/* The same statistics from the GroupNorm partials of the convs that produced x1 / x2 (dmc_conv_desc.gn_part,
 * [N*HW/64][C/8][2]): one tiny launch instead of a pass over the activation. Needs HW % 64 == 0 and groups made of
 * whole 8-channel chunks; the partials are folded in a fixed order (deterministic). */
int dmc_gn_finalize(const float* part1, int C1, const float* part2, int C2, int N, int HW, int G, float eps,
                    const float* gamma, const float* beta, float* mean_rstd, float* scale, float* shift,
                    void* stream);

/* a = dropout(SiLU(x*scale[n,c] + shift[n,c])) (silu=1) or the affine alone (silu=0), materialised once
 * (dtype, [pix][ld_out]); dropout keeps element (pix, c) iff hash(seed, pix*C + c) >= drop_thresh. */
int dmc_gn_apply(int dtype, const void* x1, const void* x2, int N, int HW, int C1, int C2, int ld1,
                 int ld2, const float* scale, const float* shift, int silu, uint32_t drop_seed,
                 const uint32_t* drop_seed_base, uint32_t drop_thresh, float drop_scale, void* out, int ld_out,
                 void* stream);

/* dmc_gn_stats then dmc_gn_apply in ONE launch, bitwise the pair: one block per sample computes the statistics
 * (mean_rstd / scale / shift as dmc_gn_stats writes them) and then writes the sample's a. Only for small samples
 * (bf16, N >= 64, HW * C <= 8192: the UNet's 4x4 levels); dmc_gn_stats_apply_ok() says whether a shape qualifies. */
int dmc_gn_stats_apply_ok(int dtype, int N, int HW, int C1, int C2, int G);
int dmc_gn_stats_apply(int dtype, const void* x1, const void* x2, int N, int HW, int C1, int C2, int ld1, int ld2,
                       int G, float eps, const float* gamma, const float* beta, float* mean_rstd, float* scale,
                       float* shift, int silu, uint32_t drop_seed, const uint32_t* drop_seed_base,
                       uint32_t drop_thresh, float drop_scale, void* out, int ld_out, void* stream);

/* Backward of a = dropout(SiLU(GroupNorm(x))) (silu=1) or a = GroupNorm(x) (silu=0, AttentionBlock
 * norm :80): g = dL/da (dtype, [pix][ld_g]); writes
 * dx (split into dx1/dx2 by channel like the sources; accumulate_k: add into existing),
 * dgamma/dbeta (fp32 [C], overwritten) and, if dx_sum_nc / dx_sum_c are not NULL (single source
 * only), the pixel sums of the stored dx per (n,c) ([N][ld_sum_nc]) / per c -- the bias and
 * time-embedding gradients of the layer that produced x (models/unet.py:64), fused into the dx pass.
 * part (may be NULL): the per-(64-pixel segment, channel) sums (sum dz, sum dz * xhat) [N*HW/64][C][2] from an
 * earlier pass; the call then skips its own reduction over (g, x). */
int dmc_gn_silu_bwd(int dtype, const void* g, int ld_g, const void* x1, const void* x2, int N,
                    int HW, int C1, int C2, int ld1, int ld2, int G, const float* mean_rstd,
                    const float* gamma, const float* beta, int silu, uint32_t drop_seed,
                    const uint32_t* drop_seed_base, uint32_t drop_thresh, float drop_scale, void* dx1, void* dx2,
                    int ld_dx1,
                    int ld_dx2, int accumulate1, int accumulate2, float* dgamma, float* dbeta,
                    float* dx_sum_nc, int ld_sum_nc, float* dx_sum_c, const float* part, void* workspace,
                    void* stream);

/* dmc_gn_silu_bwd with its column sums deferred: when the one-pass kernel takes the call (*deferred = 1), the
 * per-(n, c) sums A = (sum dz, sum dz*xhat) go to A_keep ([N][C][2]) and the per-(n, c) dx pixel sums to sums_keep
 * ([N][C], needed when dx_sum_c is set), and dgamma / dbeta / dx_sum_c are NOT written: the caller adds them to a
 * dmc_colsum_batch (the column sums over n). Otherwise (*deferred = 0) the call is dmc_gn_silu_bwd.
 * add1 (may be NULL; single source, accumulate1 set, no dx pixel sums): a second operand [pix][ld_add1] added too --
 * dx1 += dx + add1: a ResBlock's identity-shortcut gradient folded into the GroupNorm backward that writes the block
 * input's gradient (models/unet.py:64, round 6); in the one-pass kernel's dx pass (one bf16 rounding), otherwise
 * as an add into dx1 before the accumulation. */
int dmc_gn_silu_bwd_deferred(int dtype, const void* g, int ld_g, const void* x1, const void* x2, int N, int HW,
                             int C1, int C2, int ld1, int ld2, int G, const float* mean_rstd, const float* gamma,
                             const float* beta, int silu, uint32_t drop_seed, const uint32_t* drop_seed_base,
                             uint32_t drop_thresh, float drop_scale, void* dx1, void* dx2, int ld_dx1, int ld_dx2,
                             int accumulate1, int accumulate2, float* dgamma, float* dbeta, float* dx_sum_nc,
                             int ld_sum_nc, float* dx_sum_c, const float* part, void* workspace, float* A_keep,
                             float* sums_keep, int* deferred, const void* add1, int ld_add1, void* stream);

/* Column sums of up to 56 fp32 matrices in one launch: out0[c] = scale * sum_r in[r*ld + c*stride], out1 likewise
 * at +1 (may be NULL) -- the deferred GroupNorm-backward parameter sums (bitwise the immediate ones). */
typedef struct dmc_colsum_job {
  const float* in; int R; int C; long ld; int stride; float* out0; float* out1; float scale;
} dmc_colsum_job;
int dmc_colsum_batch(const dmc_colsum_job* jobs, int njobs, void* stream);

/* Per-(n,c) pixel sums of dy [N][HW][ld] -> out_nc [N][ld_out] (may be NULL) and per-c
 * sums over n -> out_c [C] (may be NULL); both fp32, scaled by `scale`. Bias / embedding grads. */
size_t dmc_channel_sum_workspace(int N, int HW, int C);
int dmc_channel_sum(int dtype, const void* dy, int N, int HW, int C, int ld, float* out_nc,
                    int ld_out, float* out_c, float scale, void* workspace, void* stream);

/* Self-attention of AttentionBlock (models/unet.py:84-99): qkv [N][L][ld_qkv] with channel
 * which*C + head*hd + d (reshape(B,3,heads,hd,HW)), softmax(QK^T/sqrt(hd))V -> out [N][L][ld_out]
 * channel head*hd + d; lse [N][heads][L] fp32 saved for backward.
 * hd <= 64: a multiple of the 16-byte chunk (4 fp32 / 8 bf16); 64 < hd <= 128: a multiple of 8 in both dtypes
 * (72, 80, ..., 128). ld_qkv >= 3*heads*hd and ld_out >= heads*hd are multiples of the 16-byte chunk;
 * ld_dqkv >= 3*heads*hd, a multiple of 4. Anything else is refused before a launch. */
int dmc_attn_fwd(int dtype, const void* qkv, int ld_qkv, int N, int L, int heads, int hd, void* out,
                 int ld_out, float* lse, uint32_t drop_seed, const uint32_t* drop_seed_base,
                 uint32_t drop_thresh, float drop_scale, void* stream);
/* dqkv [N][L][ld_dqkv] (overwritten). workspace: dmc_attn_workspace() bytes.
 * Attention-probability dropout (nn.MultiheadAttention(dropout=p) in training; the DiT blocks, dit.py:94):
 * drop_thresh != 0 keeps P[n,h][q][key] iff hash(seed, ((n*heads + h)*L + q)*L + key) >= drop_thresh and scales it
 * by drop_scale = 1/(1-p) in O = P V (lse stays that of the undropped softmax); the backward takes the same
 * arguments and recomputes the mask. drop_thresh = 0: no dropout (the UNet). */
size_t dmc_attn_workspace(int N, int L, int heads);
int dmc_attn_bwd(int dtype, const void* qkv, int ld_qkv, const void* out, const void* dout,
                 int ld_out, const float* lse, int N, int L, int heads, int hd, void* dqkv,
                 int ld_dqkv, void* workspace, uint32_t drop_seed, const uint32_t* drop_seed_base,
                 uint32_t drop_thresh, float drop_scale, void* stream);

/* Sinusoidal TimeEmbedding (models/unet.py:18-25): out [B][dim] fp32 = [sin(t f_i) | cos(t f_i)]. */
int dmc_time_embed(const int64_t* t, int B, int dim, float* out, void* stream);
/* Label embedding gather with clamp(y, 0, num_classes) (models/unet.py:256-258) and its backward
 * (padding_idx 0 receives no gradient; deterministic per-row sums). */
int dmc_embed_fwd(const int64_t* y, int B, int num_rows, const float* table, int dim, float* out,
                  void* stream);
int dmc_embed_bwd(const int64_t* y, int B, int num_rows, const float* dout, int dim, float* dtable,
                  void* stream);

/* NCHW fp32 -> NHWC dtype with channel pitch ld (zero pad channels C..ld). If t != NULL, fuses
 * DDPM.q_sample (diffusion/ddpm.py:84-104): x = a[t]*x + b[t]*noise. */
int dmc_pack_input(int dtype, const float* x, const float* noise, const int64_t* t, const float* a,
                   const float* b, int N, int C, int H, int W, void* dst, int ld, void* stream);
/* q_sample alone, NCHW fp32 (diffusion/ddpm.py:84-104). */
int dmc_q_sample(const float* x0, const float* noise, const int64_t* t, const float* a,
                 const float* b, int N, int per_sample, float* out, void* stream);

/* p_losses loss (diffusion/ddpm.py:130-139): loss = mean(f(noise - pred)); deterministic.
 * workspace: >= 4096 floats. dmc_loss_bwd: dpred = dloss[0] * df/dpred / n. */
int dmc_loss_fwd(int loss_type, const float* pred, const float* target, long n, float* loss,
                 float* workspace, void* stream);
int dmc_loss_bwd(int loss_type, const float* pred, const float* target, long n, const float* dloss,
                 float* dpred, void* stream);
/* Training objective with a prediction type and a per-sample weight, loss and gradient in ONE pass; not in the
 * reference. v-prediction (Salimans & Ho 2022, arXiv:2202.00512): target = sa[t]*noise - s1[t]*x0 with
 * sa = sqrt_alphas_cumprod, s1 = sqrt_one_minus_alphas_cumprod; DMC_PRED_EPS: target = noise (x0, sa, s1 unread).
 * w: [T] per-timestep weight, e.g. min-SNR-gamma (Hang et al. 2023, arXiv:2303.09556; diffusion/_objective.py), or
 * NULL for 1. pred, x0, noise: [N][per_sample] fp32; t: [N], clamped into [0, T).
 *   loss[0] = (1/N) sum_n w[t_n] * (1/per_sample) * sum_i f(target - pred), f as dmc_loss_fwd; fixed order
 *             (block partials per sample, samples in index order), no atomics: deterministic.
 *   dpred   = df/dpred * (dloss[0] / (float)(N*per_sample)) * w[t_n]; NULL: forward only (dloss unread). With
 *             DMC_PRED_EPS and w == NULL the bits of dmc_loss_bwd.
 * Every mul/add/sub is a separate rounding. workspace: >= DMC_OBJECTIVE_MAX_BLOCKS * N floats. 16-byte accesses
 * when per_sample % 4 == 0 and every pointer read or written is 16-byte aligned, element-wise otherwise. */
int dmc_objective(int pred_type, int loss_type, const float* pred, const float* x0, const float* noise,
                  const int64_t* t, const float* sa, const float* s1, const float* w, int T, int N,
                  int per_sample, const float* dloss, float* loss, float* dpred, float* workspace,
                  void* stream);
/* dmc_objective under importance-sampled timesteps (dmc_ts_sample below): iw: [T] importance weights or NULL for 1,
 * row_loss: [N] or NULL. The same kernels as dmc_objective, which passes NULL for both.
 *   row_loss[n] = w[t_n] * (1/per_sample) * sum_i f(target - pred): sample n's own loss BEFORE the importance weight,
 *                 the value dmc_ts_history_update takes
 *   loss[0]     = (1/N) sum_n iw[t_n] * row_loss[n], samples in index order
 *   dpred       = (df/dpred * ((dloss[0] / (float)(N*per_sample)) * w[t_n])) * iw[t_n]: iw is the LAST factor, so dpred
 *                 is iw[t_n] times dmc_objective's dpred rounded once
 * iw == NULL or all ones: loss and dpred have dmc_objective's bits. Workspace, determinism and access widths as
 * dmc_objective; row_loss and iw are accessed element-wise. */
int dmc_objective_is(int pred_type, int loss_type, const float* pred, const float* x0, const float* noise,
                     const int64_t* t, const float* sa, const float* s1, const float* w, const float* iw, int T,
                     int N, int per_sample, const float* dloss, float* loss, float* row_loss, float* dpred,
                     float* workspace, void* stream);
/* v-prediction model output -> what the step kernels consume (arXiv:2202.00512 appendix D):
 * eps = s1[t]*x + sa[t]*pred, x0 = sa[t]*x - s1[t]*pred (formed directly: no division by alpha). pred, eps_out,
 * x0_out: [reps*N][per_sample]; row r*N + n pairs with x[n], t[n] (reps = 2: the batched cond / uncond forward of
 * CFG). x0_out may be NULL. pred_type must be DMC_PRED_V: eps output needs no conversion and is refused. t is
 * clamped into [0, T); access widths as dmc_objective. */
int dmc_pred_convert(int pred_type, const float* x, const int64_t* t, const float* sa, const float* s1,
                     int T, const float* pred, int reps, int N, int per_sample, float* eps_out,
                     float* x0_out, void* stream);
/* One timestep of the variational bound on the log-likelihood, in bits per dimension, and the next step's x_t in
 * ONE pass; not in the reference (Ho et al. 2020, arXiv:2006.11239 §3-4; Nichol & Dhariwal 2021, arXiv:2102.09672
 * §2-3). coef: [T][6] fp32 rows {c_x, c_p, kprec, kvar, keps, isig} (diffusion/_vlb.py); t[n], clamped into [0, T),
 * picks sample n's row. x0, x_t, pred, z_next, x_next: [N][per_sample] fp32. Per element of sample n:
 *   u  = c_x*x_t - c_p*pred                 -- the x0 prediction, unclipped ('eps' and 'v' differ in the table only)
 *   xp = clip ? clamp(u, -1, 1) : u;   d = x0 - xp;   du = x0 - u
 *   du (and d where the clip does not act) is formed without u's rounding, as (x0 - c_x*x_t) + c_p*pred plus the two
 *   products' rounding errors (fma): a good prediction's small error keeps its digits instead of an ulp of x0
 *   t > 0:   term = kvar + kprec*d*d        -- KL(q(x_{t-1}|x_t,x0) || p(x_{t-1}|x_t)): the two means differ by
 *                                              c1*(x0 - xp) exactly and are never formed, so nothing cancels
 *   t == 0:  term = -lp, the decoder's Gaussian discretised on the 8-bit grid with the EXACT normal CDF
 *            Phi(z) = 0.5*erfc(-z/sqrt 2), deliberately not the tanh approximation of some public implementations:
 *              zp = (d + 1/255)*isig;  zm = (d - 1/255)*isig
 *              lp = log(max(Phi(zp), 1e-12))            if x0 < -0.999
 *                   log(max(Phi(-zm), 1e-12))           if x0 >  0.999
 *                   log(max(Phi(a) - Phi(b), 1e-12))    otherwise, (a, b) = (zp, zm) if zm <= 0, (-zm, -zp) if not:
 *                                                       the difference is taken where both values are small
 * Per-sample outputs, [N] fp32 each: vb = mean(term)/ln 2, xstart_mse = mean(d*d), eps_mse = keps*mean(du*du),
 * x0_sq = mean(x0*x0). At most DMC_VLB_MAX_BLOCKS blocks per sample leave partial sums in workspace
 * (>= DMC_VLB_WORKSPACE_FLOATS(N) floats), added in block order: a fixed order, no atomics, deterministic.
 * x_next != NULL: sample n with t_next[n] >= 0 gets x_next = sa[t_next]*x0 + s1[t_next]*z_next (sa, s1: [T];
 * each op rounded once, no fma: the bits of dmc_q_sample); a sample with t_next[n] < 0 is not written. x_next == NULL:
 * z_next, t_next, sa, s1 are unread. 16-byte accesses when per_sample % 4 == 0 and every pointer read or written is
 * 16-byte aligned, element-wise otherwise. */
int dmc_vlb_step(const float* x0, const float* x_t, const float* pred, const int64_t* t, const float* coef, int T,
                 int clip, const float* z_next, const int64_t* t_next, const float* sa, const float* s1,
                 int N, int per_sample, float* x_next, float* vb, float* xstart_mse, float* eps_mse,
                 float* x0_sq, float* workspace, void* stream);

/* Learned variances (Nichol & Dhariwal 2021, arXiv:2102.09672 §3.1); not in the reference. The model returns
 * [N][2][per_sample]: the prediction (eps or v), then v, the interpolation of the log-variance between the posterior's
 * and beta's. coef: [T][DMC_LVAR_COLS] fp32 rows {c_x, c_p, c1, lv_min, R, kmin, keps, lv_max}
 * (diffusion/_vlb.py learned_coefficients); t[n], clamped into [0, T), picks sample n's row. Per element
 *   d = (v + 1)/2 * R  (not clamped);   lv_p = lv_min + d;   delta = x0 - x0_pred
 *   t > 0:   term = 0.5*(d + expm1(-d)) + kmin*exp(-d)*delta^2       -- KL against the true posterior, nats
 *            d term / d v = (-0.5*expm1(-d) - kmin*exp(-d)*delta^2) * 0.5*R
 *   t == 0:  term = dmc_vlb_step's decoder -log p with isig = exp(-0.5*lv_p) per element
 *            d term / d v = 0.5*(zp*phi(zp) - zm*phi(zm)) / p * 0.5*R, an absent edge's z dropped; 0 on the 1e-12 floor
 * One device function computes the term for all three entries. 16-byte accesses when per_sample % 4 == 0, every row
 * stride is a multiple of 4 and every pointer read or written (the v half's base included) is 16-byte aligned,
 * element-wise otherwise.
 *
 * dmc_hybrid_objective: L_hybrid = L_simple + vlb_weight * mean_n vb_n and its gradient in ONE pass. out, dout:
 * [N][2][per_sample]; x0, noise: [N][per_sample]. L_simple is dmc_objective on the prediction half (pred_type,
 * loss_type, w as there; with vlb_weight == 0 loss[1] and dout's prediction half have dmc_objective's bits). vb_n is the
 * per-sample mean of the term / ln 2 with delta = c_p*(pred - target), so x_t is not needed. The term sends no gradient
 * to the prediction half (the paper's stop-gradient): dout's v half = dloss[0] * vlb_weight / (N*per_sample*ln 2) *
 * d term / d v. loss[3] = {simple + vlb, simple, vlb_weight * mean_n vb_n}. dout == NULL: forward only.
 * workspace: >= DMC_HYBRID_WORKSPACE_FLOATS(N) floats; block partials per sample added in block order, samples in
 * index order: no atomics, deterministic. sa, s1 are read for DMC_PRED_V only. */
#define DMC_LVAR_COLS 8
#define DMC_HYBRID_WORKSPACE_FLOATS(N) (2 * DMC_OBJECTIVE_MAX_BLOCKS * (size_t)(N))
int dmc_hybrid_objective(int pred_type, int loss_type, const float* out, const float* x0, const float* noise,
                         const int64_t* t, const float* sa, const float* s1, const float* w, const float* coef,
                         int T, int N, int per_sample, float vlb_weight, const float* dloss, float* loss,
                         float* dout, float* workspace, void* stream);
/* dmc_hybrid_objective under importance-sampled timesteps, as dmc_objective_is: iw: [T] or NULL for 1, row_loss: [N] or
 * NULL. With simple_n and vb_n sample n's terms of L_simple and of mean_n vb_n:
 *   row_loss[n] = simple_n + vlb_weight * vb_n          -- before the importance weight
 *   loss[3]     = {loss[1] + loss[2], (1/N) sum_n iw[t_n]*simple_n, vlb_weight * (1/N) sum_n iw[t_n]*vb_n}
 *   dout        = dmc_hybrid_objective's dout times iw[t_n] as the last factor, in both halves
 * iw == NULL or all ones: loss and dout have dmc_hybrid_objective's bits. Workspace and determinism as there. */
int dmc_hybrid_objective_is(int pred_type, int loss_type, const float* out, const float* x0, const float* noise,
                            const int64_t* t, const float* sa, const float* s1, const float* w, const float* iw,
                            const float* coef, int T, int N, int per_sample, float vlb_weight, const float* dloss,
                            float* loss, float* row_loss, float* dout, float* workspace, void* stream);
/* dmc_vlb_step with the learned term: pred and v are given as a base pointer and a row stride in floats (the two halves
 * of the model output, read in place). Outputs, the x_next contract, clip and the workspace as dmc_vlb_step. */
int dmc_vlb_step_learned(const float* x0, const float* x_t, const float* pred, long pred_stride, const float* v,
                         long v_stride, const int64_t* t, const float* coef, int T, int clip, const float* z_next,
                         const int64_t* t_next, const float* sa, const float* s1, int N, int per_sample,
                         float* x_next, float* vb, float* xstart_mse, float* eps_mse, float* x0_sq,
                         float* workspace, void* stream);
/* dmc_ddpm_step with the learned variance: out = mean + [t != 0] exp(0.5*(lv_min + d)) * z, the mean by dmc_ddpm_step's
 * ops from the same four [T] tables (z == NULL: its bits; v is then unread). eps and v: base pointer and row stride in
 * floats. eps may be NULL with x0_in. t is clamped into [0, T). */
int dmc_ddpm_step_learned(const float* x, const float* eps, long eps_stride, const float* v, long v_stride,
                          const float* x0_in, const int64_t* t, const float* sqrt_recip_ac,
                          const float* sqrt_recipm1_ac, const float* coef1, const float* coef2, const float* coef,
                          int T, int N, int per_sample, int clip, const float* z, float* out, void* stream);

/* Loss-aware timestep sampling (Nichol & Dhariwal 2021, arXiv:2102.09672 §3.3); not in the reference. The last K losses
 * seen at each timestep, hist: [T][K] fp32, and the number ever seen, count: [T] int32, live on the device; nothing is
 * read back. Host restatement: diffusion/_resample.py.
 *
 * dmc_ts_history_update: for n = 0..N-1 in index order, tt = t[n] clamped into [0, T):
 *   hist[tt][count[tt] % K] = loss[n];  ++count[tt]
 * A ring: row tt holds the multiset of the paper's shift-left buffer once count[tt] >= K ("warm"), and only the multiset
 * enters the weights. One thread per timestep scans the batch, staged in LDS in chunks (any N), and writes its own row
 * alone: samples sharing a t land exactly as the sequential loop has them. No atomics, deterministic, no workspace.
 *
 * dmc_ts_sample, ONE launch (a single block striding over T; any T >= 1, N >= 1):
 *   warm = all_t(count[t] >= K);  r_t = sqrt(mean_k hist[t][k]^2);  S = sum_t r_t
 *   !warm, or S not a positive finite number:  p_t = 1/T, iw_t = 1 exactly, cdf[i] = (i+1)/T
 *   otherwise  q_t = r_t/S*(1 - uniform_prob) + uniform_prob/T;  p_t = q_t / sum_t q_t;  iw_t = 1/(T*p_t)
 *   cdf = inclusive prefix sum of p, cdf[T-1] stored as exactly 1
 *   t_out[n] = the smallest i with cdf[i] > u[n], searched in the fp32 cdf as stored (T-1 if there is none)
 * u: [N] in [0, 1), the caller's draw (torch.rand): no RNG in the kernel. Squares, means, sqrt, both sums, the
 * divisions and the scan run in double in a fixed order (per-thread partial sums in index order, then a fixed tree;
 * every op a separate rounding); p, iw and cdf are each rounded to fp32 once. uniform_prob in [0, 1); with 0 a warm row of
 * zeros has p_t = 0 and iw_t = +inf, and the strict '>' never draws it except as the fallback T-1. Deterministic, no
 * atomics, no workspace. */
int dmc_ts_history_update(const int64_t* t, const float* loss, int N, int T, int K, float* hist, int32_t* count,
                          void* stream);
int dmc_ts_sample(const float* hist, const int32_t* count, int T, int K, float uniform_prob, const float* u, int N,
                  int64_t* t_out, float* p, float* iw, float* cdf, void* stream);

/* DDIM.p_sample update (diffusion/ddim.py:154-208), fused; alpha gathers on device; if any
 * t_next < 0 the reference uses alpha_next = 1 for the whole batch (:176-179), so does this.
 * x0_in (optional) replaces the x0 prediction; z (optional) is the eta>0 noise. */
int dmc_ddim_step(const float* x, const float* eps, const float* x0_in, const int64_t* t,
                  const int64_t* t_next, const float* alphas_cumprod, int N, int per_sample,
                  float eta, int clip, const float* z, float* out, void* stream);
/* DDPM.p_sample (diffusion/ddpm.py:151-220), fused. */
int dmc_ddpm_step(const float* x, const float* eps, const float* x0_in, const int64_t* t,
                  const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* coef1,
                  const float* coef2, const float* logvar, int N, int per_sample, int clip,
                  const float* z, float* out, void* stream);
/* DPM-Solver++ multistep update in data-prediction form, orders 1 and 2.
 * coef: [S][5] fp32 rows {sa, s1, cx, c0, c1}; step[n] in [0,S) picks sample n's row (an index
 * outside is clamped into the table).
 *   x0  = x0_in ? x0_in[i] : (x[i] - s1*eps[i]) / sa;   if (clip) x0 = clamp(x0, -1, 1)
 *   out = (cx*x[i] + c0*x0) + (c1 != 0 ? c1*x0_prev[i] : nothing)   -- each op rounded once, no fma
 *   x0_out[i] = x0                                    -- x0_out may be the same buffer as x0_prev
 * A row with c1 == 0 never reads x0_prev (it may be NULL or hold NaN); a row with c1 != 0 and
 * x0_prev == NULL gives NaN. eps may be NULL when x0_in is given. 16-byte accesses when
 * per_sample % 4 == 0 and every pointer is 16-byte aligned, element-wise otherwise. */
int dmc_dpm_step(const float* x, const float* eps, const float* x0_in, const float* x0_prev,
                 const int64_t* step, const float* coef, int S, int N, int per_sample, int clip,
                 float* out, float* x0_out, void* stream);
/* Known-region blend of the editing samplers (not in the reference): inpainting as RePaint (Lugmayr et
 * al. 2022, arXiv:2201.09865) and SDEdit's image-to-image (Meng et al. 2021, arXiv:2108.01073).
 * coef: [R][4] fp32 rows {ka, kb, ra, rb} (diffusion/_edit.py); row[n] in [0,R) picks sample n's row (an
 * index outside is clamped into the table). mask: [N][mask_per], mask_per == per_sample or a divisor of it
 * (a per-pixel mask shared by the channels of NCHW); element j of sample n reads
 * m = mask[n*mask_per + j % mask_per], 1 keeps the given image x0.
 *   known = kb != 0 ? ka*x0[i] + kb*z[i] : ka*x0[i]     -- x0 noised to the step's target level
 *   b     = m*known + (1 - m)*x[i]
 *   out   = rb != 0 ? ra*b + rb*z2[i] : b               -- the forward jump of a resampling repetition
 * Each op rounded once, no fma. A row with kb == 0 never reads z, one with rb == 0 never reads z2 (either
 * may be NULL or hold NaN); a row with kb != 0 and z == NULL, or rb != 0 and z2 == NULL, gives NaN. out may
 * be the same buffer as x. 16-byte accesses when per_sample % 4 == 0, mask_per % 4 == 0 and every pointer
 * read or written is 16-byte aligned, element-wise otherwise. */
int dmc_known_blend(const float* x, const float* x0, const float* mask, int mask_per, const float* z,
                    const float* z2, const int64_t* row, const float* coef, int R, int N, int per_sample,
                    float* out, void* stream);
/* CFG + x0 prediction + dynamic threshold (diffusion/ddim.py:300-325, ddpm.py:284-303):
 * eps = eu + s*(ec - eu) -> eps_out; x0 = mode 0: (x - sqrt(1-a)eps)/sqrt(a) [DDIM]
 * mode 1: sra*x - srm1*eps [DDPM]; threshold: p in (0,1): per-row quantile of |x0| (linear
 * interpolation, as torch.quantile), s = max(s,1), x0 = clamp(x0,-s,s)/s; p <= 0: clamp +-1. */
int dmc_cfg_x0(const float* x, const float* ec, const float* eu, float scale, const int64_t* t,
               const float* tab_a, const float* tab_b, int mode, int N, int per_sample,
               float p_threshold, float* eps_out, float* x0_out, void* stream);
/* Guidance on the model's own output, optional guidance rescale, eps and x0 for the step kernels and the dynamic
 * threshold in ONE launch between the 2B forward and the step; not in the reference (Lin et al. 2023,
 * arXiv:2305.08891 §3.4). It stands where dmc_pred_convert + dmc_cfg_x0 stand, and unlike them represents
 * alphas_cumprod[t] = 0 for DMC_PRED_V (nothing divides). pc / pu: the conditional / unconditional rows, row n at
 * pc + n*pc_stride (strides in floats, >= per_sample: the prediction half of a 2C-channel output is read in place);
 * x, eps_out, x0_out: [N][per_sample]; sa = sqrt_alphas_cumprod, s1 = sqrt_one_minus_alphas_cumprod, [T]; t is clamped
 * into [0, T). One block per sample; per element, each op rounded once, no fma:
 *   d = pc - pu;  g = pu + scale*d                             -- dmc_cfg_x0's two roundings
 *   rescale > 0:  g = g*f,  f = (float)(rescale*sqrt(M2_c/M2_g) + (1 - rescale)) in double, M2 = sum (v - mean)^2
 *                 over the sample's pc (c) and g (g): two-pass double sums in a fixed order, no atomics. The ratio is
 *                 std(pc)/std(g) under either normalisation. M2_g == 0: f = 1 (the public implementations give NaN)
 *   DMC_PRED_V:   eps = s1*x + sa*g;  x0 = sa*x - s1*g         -- dmc_pred_convert's ops
 *   DMC_PRED_EPS: eps = g;  x0 = (x - s1*g) / sa               -- dmc_cfg_x0 mode 0 with the tables' square roots
 *   threshold on x0 as dmc_cfg_x0 (p_threshold < 1; <= 0: clamp +-1)
 * rescale must lie in [0, 1]; 0 skips the reduction passes. eps_out may be NULL. per_sample > 16384 is refused before
 * the launch. Accesses are element-wise. */
int dmc_cfg_guide(int pred_type, const float* x, const float* pc, long pc_stride, const float* pu, long pu_stride,
                  float scale, float rescale, const int64_t* t, const float* sa, const float* s1, int T, int N,
                  int per_sample, float p_threshold, float* eps_out, float* x0_out, void* stream);
/* Rectified-flow ODE step (not in the reference; Liu et al. 2022, arXiv:2209.03003, Heun's scheme as Karras et al. 2022,
 * arXiv:2206.00364 alg. 1): guidance, update and history in ONE launch beside the model. coef: [R][4] fp32 rows
 * {sigma, h, hh, kind} (diffusion/_flow.py: h = sigma_next - sigma, hh = h/2); step[n] in [0,R) picks sample n's row (an
 * index outside is clamped into the table); a kind other than 1 or 2 is 0. pc / pu: the conditional / unconditional
 * velocity rows, row n at pc + n*pc_stride (strides in floats, >= per_sample: the halves of a 2N-row model output are
 * read in place); pu NULL: no guidance. Per element, each op rounded once, no fma:
 *   g = pu ? pu + scale*(pc - pu) : pc                          -- dmc_cfg_x0's two roundings
 *   kind 0 (Euler):      out = x + h*g
 *   kind 1 (predictor):  out = x + h*g;  xb_out = x;  d_out = g -- each written only if its pointer is given
 *   kind 2 (corrector):  out = xb + hh*(dprev + g)              -- x is not read
 * Rows of kind 0 or 1 never read xb or dprev (either may be NULL or hold NaN), rows of kind 0 or 2 never write xb_out or
 * d_out; a kind-2 row with xb or dprev NULL gives NaN. out may be the same buffer as x, xb_out as xb, d_out as dprev.
 * 16-byte accesses when per_sample and both strides are multiples of 4 and every pointer is 16-byte aligned,
 * element-wise otherwise. */
int dmc_flow_step(const float* x, const float* pc, long pc_stride, const float* pu, long pu_stride, float scale,
                  const float* xb, const float* dprev, const int64_t* step, const float* coef, int R, int N,
                  int per_sample, float* out, float* xb_out, float* d_out, void* stream);
/* Guided velocity of a rectified flow when the guidance is rescaled or the data prediction thresholded (otherwise
 * dmc_flow_step guides by itself); g_out feeds dmc_flow_step as pc with pu NULL. One block per sample, dmc_cfg_guide's
 * launch shape, sums and threshold; operands and row choice as dmc_flow_step. Per element, each op rounded once:
 *   g = pu + scale*(pc - pu);  rescale > 0: g = g*f, f exactly as dmc_cfg_guide forms it
 *   threshold == 0:  g_out = g                                  -- x is not read
 *   threshold != 0:  x0 = x - sigma*g;  the threshold of dmc_cfg_x0 on x0 (p_threshold in (0,1): quantile; <= 0: clamp
 *                    +-1);  g_out = (x - x0) / sigma            -- sigma of the sample's row; g_out must not be x
 * rescale must lie in [0, 1]. per_sample > 16384 is refused before the launch. Accesses are element-wise. */
int dmc_flow_guide(const float* x, const float* pc, long pc_stride, const float* pu, long pu_stride, float scale,
                   float rescale, const int64_t* step, const float* coef, int R, int N, int per_sample, int threshold,
                   float p_threshold, float* g_out, void* stream);

/* Multi-tensor ops over a device array of descriptors {dst, src, n} (utils/trainer.py:187-202
 * EMA; :259 clip_grad_norm_). */
typedef struct dmc_tensor_ref {
  float* a;
  const float* b;
  long n;
} dmc_tensor_ref;
int dmc_ema_update(const dmc_tensor_ref* refs, int count, float decay, void* stream);
/* total_norm (fp32 scalar) = ||(||g_i||)||; g *= min(1, max_norm/(total_norm+1e-6)).
 */
int dmc_clip_grad_norm(const dmc_tensor_ref* refs, int count, float max_norm, float* total_norm,
                       float* workspace, void* stream);   /* workspace >= 16*count + 16 floats */
/* Flat-buffer optimizer step (parameters, gradients, moments and EMA share one fp32 layout).
 * dmc_grad_norm_flat: total_norm = ||g||_2, coef = min(1, max_norm/(total_norm+1e-6)) (max_norm <= 0:
 * coef = 1) -- torch.nn.utils.clip_grad_norm_ of utils/trainer.py:259, with the scaling deferred to
 * the consumer. workspace >= 1024 floats.
 * dmc_adamw_flat: g *= coef[0] (coef may be NULL), then torch.optim.AdamW.step (train.py:142-146;
 * foreach path, amsgrad=False) in torch's operation order: p *= wd_mul; m = lerp(m, g, lerp_w);
 * v = v*beta2 + one_minus_beta2*g*g; p += neg_step_size * m / (sqrt(v)/bc2_sqrt + eps). The host
 * computes the scalars in double like torch (wd_mul = 1-lr*wd, lerp_w = 1-beta1, neg_step_size =
 * -lr/(1-beta1^t), bc2_sqrt = sqrt(1-beta2^t)). Then, if ema != NULL, ema = ema*ema_decay +
 * ema_one_minus*p (utils/trainer.py:187-202). */
int dmc_grad_norm_flat(const float* g, long n, float max_norm, float* total_norm, float* coef,
                       float* workspace, void* stream);
int dmc_adamw_flat(float* p, const float* g, float* m, float* v, float* ema, long n, const float* coef,
                   float wd_mul, float lerp_w, float beta2, float one_minus_beta2, float eps,
                   float neg_step_size, float bc2_sqrt, float ema_decay, float ema_one_minus, void* stream);

/* dmc_adamw_flat with the nine step scalars read from device memory (hyper[0..8] = wd_mul, lerp_w, beta2,
 * one_minus_beta2, eps, neg_step_size, bc2_sqrt, ema_decay, ema_one_minus), so a captured HIP graph of
 * the training step replays with the current learning rate and bias corrections (one H2D copy per step). */
int dmc_adamw_flat_dev(float* p, const float* g, float* m, float* v, float* ema, long n, const float* coef,
                       const float* hyper, void* stream);
/* y[n][2h+i][2w+j][c] = x[n][h][w][c] (i, j in {0,1}): nearest x2 upsample of an NHWC activation
 * (models/unet.py:118 F.interpolate(scale_factor=2, mode='nearest')), materialised as the operand of the
 * Upsample conv's weight gradient. C*esize, ld*esize and ldy*esize must be multiples of 16 bytes. */
int dmc_upsample2x_nhwc(int dtype, const void* x, int N, int H, int W, int C, int ld, void* y, int ldy,
                        void* stream);
/* y = silu(x) (fp32); NHWC dtype -> NCHW fp32 (the inverse of dmc_pack_input); y += x (dtype). */
int dmc_silu_fwd(const float* x, float* y, long n, void* stream);
int dmc_unpack_output(int dtype, const void* src, int ld, int N, int C, int H, int W, float* dst,
                      void* stream);
int dmc_add(int dtype, void* y, const void* x, long n, void* stream);


/* ---- DiT backbone (models/dit.py of the reference; dmc_dit.hip) ----------------------------------------------
 * Token rows [T = B*L][C]; the residual stream x is fp32, GEMM operands (h, branch) are in `dtype`.
 * Modulation vectors (shift / scale / gate) are rows of the stacked adaLN GEMM output [B][ld_mod].
 * C % 4 == 0, C <= 2048, T % L == 0 and every pitch (ld_br, ld_h, ld_dh, ld_dbr, ld_mod) a multiple of 4 (8- and 16-byte
 * accesses), in the forward and the backward entry points alike: anything else is refused before a launch.
 * ln_mod_fwd: DiTBlock.forward (dit.py:113-130): x_new = x + gate * dropout(br) when br != NULL (x_out = x_new),
 *   then h = LayerNorm(x_new; eps, no affine) * (1 + scale) + shift; saves the row mean / rstd.
 * ln_mod_bwd: dx += d/dx of that LayerNorm + modulation for upstream dh; dscale / dshift = sums over each image's
 *   L rows (written).  gate_bwd: dbr = dy * gate (* dropout mask); dgate = per-image row sums of dy * dropout(br).
 * gelu_fwd / gelu_bwd: nn.GELU() (erf) + nn.Dropout between the MLP Linears (dit.py:100-104).
 * timestep_embedding: TimestepEmbedder.timestep_embedding (dit.py:38-47) -> [B][dim] = [cos | sin].
 * unpatchify: DiT.unpatchify (dit.py:248-261) [B*ht*wt][ld_src >= p*p*C] -> NCHW; patchify_grad is its adjoint.
 * add_bcast: x[r][i] += v[i] (pos_embed broadcast over the batch, dit.py:274). */
int dmc_ln_mod_fwd(int dtype, const float* x, const void* br, int ld_br, const float* gate, const float* shift,
                   const float* scale, int ld_mod, int T, int C, int L, float eps, uint32_t drop_seed,
                   const uint32_t* drop_seed_base, uint32_t drop_thresh, float drop_scale, float* x_out, void* h,
                   int ld_h, float* mean, float* rstd, void* stream);
/* workspace (dmc_dit_rowsum_workspace bytes, may be NULL = one block per image): the image's rows are split over
 * several blocks whose per-image channel sums are added in split order (deterministic). */
size_t dmc_dit_rowsum_workspace(int B, int C, int L);
int dmc_ln_mod_bwd(int dtype, const void* dh, int ld_dh, const float* x, const float* mean, const float* rstd,
                   const float* scale, int ld_mod, int T, int C, int L, float* dx, float* dscale, float* dshift,
                   void* workspace, void* stream);
int dmc_gate_bwd(int dtype, const float* dy, const void* br, int ld_br, const float* gate, int ld_mod, int T, int C,
                 int L, uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_thresh, float drop_scale,
                 void* dbr, int ld_dbr, float* dgate, void* workspace, void* stream);
int dmc_gelu_fwd(int dtype, const void* u, long rows, int C, int ld, uint32_t drop_seed, const uint32_t* drop_seed_base,
                 uint32_t drop_thresh, float drop_scale, void* a, void* stream);
int dmc_gelu_bwd(int dtype, const void* da, const void* u, long rows, int C, int ld, uint32_t drop_seed,
                 const uint32_t* drop_seed_base, uint32_t drop_thresh, float drop_scale, void* du, void* stream);
int dmc_timestep_embedding(const int64_t* t, int B, int dim, float max_period, float* out, void* stream);
int dmc_unpatchify(const float* src, int ld_src, int B, int ht, int wt, int p, int C, float* dst, void* stream);
int dmc_patchify_grad(int dtype, const float* dout, int B, int ht, int wt, int p, int C, void* dst, int ld_dst,
                      void* stream);
int dmc_add_bcast(float* x, const float* v, long rows, long n, void* stream);
/* batch_sum: out[i] = sum_r x[r][i] (fp32, rows summed in order): the pos_embed gradient.
 * patch_dgrad: input gradient of the patch embedding Conv2d(k=p, s=p) (dit.py:21): dx[B][C][ht*p][wt*p] from the
 * fp32 token gradient dtok[B*ht*wt][ld] and the fp32 weight [H][C][p][p]. */
int dmc_batch_sum(const float* x, long rows, long n, float* out, void* stream);
int dmc_patch_dgrad(const float* dtok, int ld, const float* w, int B, int ht, int wt, int p, int C, int H, float* dx,
                    void* stream);

/* ---- DiM backbone (models/dim.py of the reference; dmc_dit.hip, dmc_mamba.hip) ---------------------------------
 * ln_affine_mod_fwd / bwd: MambaBlock / FeedForward / FinalLayer.forward (dim.py:131-134, :166-169, :201-203) with
 *   nn.LayerNorm(hidden, eps=1e-6) (:101, :150, :193, elementwise affine): dmc_ln_mod_fwd / bwd with
 *   h = (xhat * gamma + beta) * (1 + scale) + shift; the backward also writes dgamma / dbeta [C], the sums over all
 *   T rows (per image in row order, then images in order). With gamma = 1, beta = 0 both equal the plain kernels
 *   bitwise. */
/* gate_bwd_bias: dmc_gate_bwd, plus dbias [C] = sum over all T rows of dy * gate * mask taken in fp32: the gradient
 * of the bias of the branch's last Linear (FeedForward.mlp[3], dim.py:156; the attention fallback's out_proj, :112),
 * which the weight-gradient kernel would otherwise sum from the rounded dbr rows. dsum: [B][ld_mod] scratch rows
 * (the per-image sums of dy * mask). The workspace of dmc_dit_rowsum_workspace serves (two sums per split). */
int dmc_gate_bwd_bias(int dtype, const float* dy, const void* br, int ld_br, const float* gate, int ld_mod, int T, int C,
                      int L, uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_thresh,
                      float drop_scale, void* dbr, int ld_dbr, float* dgate, float* dsum, float* dbias, void* workspace,
                      void* stream);
/* gelu_bwd_f32in: dmc_gelu_bwd with da given as fp32 rows (pitch ld) whatever `dtype` is: the input-gradient GEMM of
 * FeedForward.mlp[3] (dim.py:156) stores them unrounded, so du (and the mlp[0] bias gradient summed from it) carries
 * one rounding, not two. u and du are in `dtype`. */
int dmc_gelu_bwd_f32in(int dtype, const float* da, const void* u, long rows, int C, int ld, uint32_t drop_seed,
                       const uint32_t* drop_seed_base, uint32_t drop_thresh, float drop_scale, void* du, void* stream);
int dmc_ln_affine_mod_fwd(int dtype, const float* x, const void* br, int ld_br, const float* gate, const float* shift,
                          const float* scale, int ld_mod, int T, int C, int L, float eps, const float* gamma,
                          const float* beta, uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_thresh,
                          float drop_scale, float* x_out, void* h, int ld_h, float* mean, float* rstd, void* stream);
int dmc_ln_affine_mod_bwd(int dtype, const void* dh, int ld_dh, const float* x, const float* mean, const float* rstd,
                          const float* scale, int ld_mod, int T, int C, int L, const float* gamma, const float* beta,
                          float* dx, float* dscale, float* dshift, float* dgamma, float* dbeta, void* workspace,
                          void* stream);
/* The token mixer mamba_ssm.Mamba(d_model, d_state=16, d_conv=4, expand=2) of MambaBlock (dim.py:104-109, :137),
 * E = 2 * d_model inner channels, token rows [T = B*L][E] in `dtype` with the given pitches, parameters fp32.
 * causal_conv_silu_fwd: Mamba's conv1d (Conv1d(E, E, 4, groups=E, padding=3), cut to L) + SiLU over the tokens of
 *   each image: u[b,l,c] = SiLU(bias[c] + sum_k w[c][k] * x[b,l-3+k,c]), x[b,<0] = 0; w is [E][4].
 * causal_conv_silu_bwd: dx rows, dw [E][4] and dbias [E] (sums over images and tokens in a fixed order) from du;
 *   workspace: dmc_causal_conv_workspace bytes.
 * selective_scan_fwd: Mamba's selective_scan_fn with delta_softplus, D and the z gate:
 *   delta = softplus(dpre + dt_bias) (torch threshold 20), A = -exp(A_log) [E][N],
 *   s_t = exp(delta_t * A) * s_{t-1} + delta_t * Bm_t * u_t (s_{-1} = 0 per image, fp32 state),
 *   y_t = (sum_n Cm_t[n] * s_t[n] + D * u_t) * SiLU(z_t). Bm / Cm are [T][N] at pitch ld_bc. N must be 16.
 *   dpre, Bm and Cm are fp32 rows whatever `dtype` is (u, z, y and the gradient rows are in `dtype`).
 *   The token axis is cut into chunks of dmc_scan_chunk() tokens; states [B][chunks][E][N] receives the state at
 *   the start of every chunk (all the backward keeps of the states); with more than one chunk states and workspace
 *   (dmc_selective_scan_workspace(.., 0) bytes) are required.
 * selective_scan_bwd: from dy: du, dz, ddpre (the gradient of the delta pre-activation) rows; dBm / dCm (sums over
 *   the channels) as columns bc_col .. bc_col + 2N of the rows dbc (pitch ld_dbc; the columns behind them up to the
 *   pitch are zeroed); dA_log [E][N] and dD [E] (sums over images and tokens). No atomics: every sum has a fixed
 *   order. workspace: dmc_selective_scan_workspace(.., 1) bytes. The dt_proj bias gradient is the column sum of
 *   ddpre (the weight-gradient kernel's wg_bias).
 * Scan orders (the _ord entry points): the tokens of an image are the h x w patch grid in row-major rows, and the
 *   recurrence walks them in another order -- "permute the tokens, run the op, un-permute", done by address arithmetic
 *   inside the kernels. order is a 3-bit code: bit 0 reverse, bit 1 column-major, bit 2 snake (every other line
 *   walked backwards). dmc_scan_order_token(order, h, w, p) is the token (row index within the image) at logical
 *   position p of the walk: q = reverse ? h*w-1-p : p; inner = column ? h : w; a = q / inner, b = q % inner;
 *   snake and a odd: b = inner-1-b; (i, j) = column ? (b, a) : (a, b); token = i*w + j. -1 for arguments out of
 *   range. Order 0 is the identity. The _ord entry points take (h, w, order) in place of L = h*w; every other
 *   argument, the workspaces and `states` (sized for L = h*w) are those of the plain entry points, which stay the
 *   order-0 code path. */
int dmc_causal_conv_silu_fwd(int dtype, const void* x, int ld_x, const float* w, const float* bias, int B, int L, int E,
                             void* u, int ld_u, void* stream);
size_t dmc_causal_conv_workspace(int B, int L, int E);
int dmc_causal_conv_silu_bwd(int dtype, const void* du, int ld_du, const void* x, int ld_x, const float* w,
                             const float* bias, int B, int L, int E, void* dx, int ld_dx, float* dw, float* dbias,
                             void* workspace, void* stream);
int dmc_causal_conv_silu_fwd_ord(int dtype, const void* x, int ld_x, const float* w, const float* bias, int B, int h,
                                 int wt, int order, int E, void* u, int ld_u, void* stream);
int dmc_causal_conv_silu_bwd_ord(int dtype, const void* du, int ld_du, const void* x, int ld_x, const float* w,
                                 const float* bias, int B, int h, int wt, int order, int E, void* dx, int ld_dx,
                                 float* dw, float* dbias, void* workspace, void* stream);
int dmc_scan_chunk(void);
int dmc_scan_order_token(int order, int h, int w, int p);
size_t dmc_selective_scan_workspace(int B, int L, int E, int N, int backward);
int dmc_selective_scan_fwd(int dtype, const void* u, int ld_u, const void* z, int ld_z, const float* dpre, int ld_dp,
                           const float* Bm, const float* Cm, int ld_bc, const float* A_log, const float* D,
                           const float* dt_bias, int B, int L, int E, int N, float* states, void* workspace, void* y,
                           int ld_y, void* stream);
int dmc_selective_scan_bwd(int dtype, const void* dy, int ld_dy, const void* u, int ld_u, const void* z, int ld_z,
                           const float* dpre, int ld_dp, const float* Bm, const float* Cm, int ld_bc, const float* A_log,
                           const float* D, const float* dt_bias, int B, int L, int E, int N, const float* states,
                           void* workspace, void* du, int ld_du, void* dz, int ld_dz, void* ddpre, int ld_ddp,
                           void* dbc, int ld_dbc, int bc_col, float* dA_log, float* dD, void* stream);
int dmc_selective_scan_fwd_ord(int dtype, const void* u, int ld_u, const void* z, int ld_z, const float* dpre,
                               int ld_dp, const float* Bm, const float* Cm, int ld_bc, const float* A_log,
                               const float* D, const float* dt_bias, int B, int h, int w, int order, int E, int N,
                               float* states, void* workspace, void* y, int ld_y, void* stream);
int dmc_selective_scan_bwd_ord(int dtype, const void* dy, int ld_dy, const void* u, int ld_u, const void* z, int ld_z,
                               const float* dpre, int ld_dp, const float* Bm, const float* Cm, int ld_bc,
                               const float* A_log, const float* D, const float* dt_bias, int B, int h, int w, int order,
                               int E, int N, const float* states, void* workspace, void* du, int ld_du, void* dz,
                               int ld_dz, void* ddpre, int ld_ddp, void* dbc, int ld_dbc, int bc_col, float* dA_log,
                               float* dD, void* stream);

/* ---- Device-resident data path (datasets/base_dataset.py:96-128, train.py:107-128) ----
 * One training batch from a uint8 image bank [n_images][H][W][C] resident in device memory: out[b] =
 * Normalize(ToTensor(RandomHorizontalFlip(bank[idx[b]]))) as NCHW fp32 [B][C][H][W], i.e.
 * ((float)u / 255 - mean[c]) / std[c] with torchvision's op order (bit-exact). idx: device int32 [B], every entry
 * in [0, n_images) (the caller validates: the kernel does not). Flip of sample b: flips[b] != 0 if flips (device
 * uint8 [B]) is given, else hash(pos0 + b, flip_seed) < flip_thresh (flip_thresh = p * 2^32; 0 = no flip).
 * mean/std: HOST arrays of C floats, C <= 4. labels_in (device int64 [n_images]) / labels_out (device int64 [B]):
 * both NULL or both set; labels_out[b] = labels_in[idx[b]]. */
int dmc_load_batch(const uint8_t* bank, long n_images, int H, int W, int C, const int32_t* idx, int B,
                   const uint8_t* flips, uint32_t flip_seed, uint32_t flip_thresh, long pos0, const float* mean,
                   const float* std, float* out, const int64_t* labels_in, int64_t* labels_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/*
 * wavelets_mi355x.h -- C ABI of libwavelets_mi355x.so
 *
 * MI355X-native (CDNA4 / gfx950, hand-written HIP) backend for the one data-parallel
 * hot path of JuliaDSP/Wavelets.jl v0.10.1: the periodic orthogonal filter-bank
 * DWT/IDWT and the lifting DWT/IDWT behind dwt / idwt / dwt! / idwt! / wpt! / iwpt!,
 * plus the callers on either side of that path: modwt / imodwt,
 * threshold!, the median / mad! noise estimate and the array helpers of denoise.
 *
 * The reference has NO native interface (it is 100 % Julia): the seam this ABI
 * plugs into is the internal `_dwt!` / `_wpt!` method table that the public API
 * ends in (src/Transforms/transforms_main.jl:105-130, 134-176) -- exactly the seam
 * the reference's own KernelAbstractions extension uses
 * (ext/WaveletsGPUExt/filter_transforms_gpu.jl:171-214, lifting_transforms_gpu.jl:171).
 * A Julia maintainer adds `_dwt!(y::ROCArray, x::ROCArray, filter::OrthoFilter, L, fw)`
 * methods that `ccall` the entry points below (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - All array pointers are DEVICE pointers (HBM) owned by the caller.  Arrays are in
 *    Julia layout: column-major, dims[0] fastest, dense (no padding) unless an `ld`
 *    argument says otherwise.
 *  - dtype: WL_F32 (Float32) or WL_F64 (Float64).  Taps / lifting coefficients are
 *    passed as Float64 exactly as the reference stores them (OrthoFilter.qmf,
 *    LSStep.param.coef) and are converted to the element type before use, as
 *    WT.makereverseqmfpair / makescheme do (wt_main.jl:172-183,
 *    transforms_lifting.jl:13-25).  They are copied at call time; no host pointer
 *    is retained.
 *  - Every call is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream) and returns without synchronising.  A wl_ctx owns a grow-only
 *    device workspace and is NOT thread-safe: use one context per stream.  Calls run on
 *    the context's device and leave the caller's current HIP device unchanged.
 *  - Return value: 0 (WL_OK) or a negative wl_status.  Nothing throws or aborts.
 *    The Julia glue maps the codes to the exceptions the reference throws
 *    (transforms_filter.jl:25-34): WL_EDIMS -> DimensionMismatch, WL_EINVAL_* /
 *    WL_EALIAS -> ArgumentError.
 *  - Arithmetic: sums are evaluated in the reference's order with separate multiply
 *    and add roundings (no FMA contraction), so Float32/Float64 results are
 *    bit-identical to the reference CPU loops on the same taps.  A second library
 *    with the same ABI, libwavelets_mi355x_fma.so (the same sources built with FMA
 *    contraction allowed, `make FMA=1`), is the opt-in "fused" arithmetic mode: it
 *    agrees with the reference to ||y - ref||_2 / ||ref||_2 <= 1e-6 sqrt(L) (Float32),
 *    1e-13 sqrt(L) (Float64) instead of bit for bit.  A host selects it by loading
 *    that file; neither library ever falls back on the other.
 *    Special values follow the reference too (subnormals are kept, Inf and NaN appear
 *    where its summation order puts them), with two exemptions: NaN payloads are not
 *    preserved by the transforms, and the sign of a zero result is unspecified for the
 *    inverse filter-bank kernels and wl_modwt_mra_batch (they may give -0 where the
 *    reference's up-sampling loop gives +0; the kernels are listed in DESIGN.md
 *    section 23).
 *  - There is no CPU fallback: without a gfx950 device every entry point that needs
 *    one returns WL_EHIP / WL_ENODEVICE.
 */
#ifndef WAVELETS_MI355X_H
#define WAVELETS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WL_VERSION 100 /* 0.1.0 */

#if defined(WL_BUILDING_LIB)
#define WL_API __attribute__((visibility("default")))
#else
#define WL_API
#endif

enum wl_dtype { WL_F32 = 0, WL_F64 = 1 };

typedef enum wl_status {
    WL_OK = 0,
    WL_EINVAL_SIZE = -1,   /* "size must have a sufficient power of 2 factor" (transforms_filter.jl:29-30) */
    WL_EINVAL_L = -2,      /* "L must be positive" (transforms_filter.jl:27-28)                          */
    WL_EALIAS = -3,        /* "in array is out array" (transforms_filter.jl:31-32)                       */
    WL_EDIMS = -4,         /* ndims not in 1..3 / non-positive extent / bad ld (DimensionMismatch)        */
    WL_EINVAL_CUBE = -5,   /* "array must be square/cube" (transforms_lifting.jl:131-132)                */
    WL_EINVAL_TREE = -6,   /* "invalid tree" (transforms_filter.jl:315-316)                              */
    WL_EINVAL_SCHEME = -7, /* lifting step list malformed (nsteps, ncoef out of range)                   */
    WL_EINVAL_DTYPE = -8,
    WL_EINVAL_FILTER = -9, /* flen < 2 or flen > WL_MAX_FLEN                                             */
    WL_EINVAL_ARG = -10,   /* NULL pointer etc.                                                          */
    WL_ENOMEM = -11,       /* device workspace allocation failed                                         */
    WL_EHIP = -12,         /* a HIP runtime call failed (wl_last_hip_error gives the hipError_t)         */
    WL_ENODEVICE = -13     /* no HIP device / device is not gfx950                                       */
} wl_status;

#define WL_MAX_FLEN 64     /* longest OrthoFilter supported (batt6 has 59 taps)   */
#define WL_MAX_STEPS 16    /* lifting steps per scheme                            */
#define WL_MAX_NCOEF 3     /* coefficients per lifting step (reference supports 1..3,
                              transforms_lifting.jl:455-483)                       */

typedef struct wl_ctx wl_ctx;

/* ---- sharding a batch of independent units over GPUs (dwtc columns, images) --------------------------------- */
/* Contiguous block partition: rank r of `world` owns units [*lo, *hi).  The path has no exchange step: one process
 * (or Julia task) per GPU calls wl_dwtc_* on its own column block with its own context; only the wavelet description travels
 * between ranks.  Host-side arithmetic only: usable without a device.  (replaces: nothing -- the reference has no dwtc,
 * transforms_main.jl:179-181; north_star defines the multi-GPU batch)                                               */
WL_API int wl_shard_range(int64_t nunits, int rank, int world, int64_t *lo, int64_t *hi);

/* ---- context -------------------------------------------------------------------- */
/* Create a context on HIP device `device` (>= 0).  Fails with WL_ENODEVICE when there is
 * no such device or it is not gfx950.  (replaces: nothing -- Julia allocates scratch
 * vectors per call, transforms_filter.jl:16-23,117-119)                                */
WL_API int wl_ctx_create(int device, wl_ctx **out);
WL_API int wl_ctx_destroy(wl_ctx *ctx);
/* Device workspace of the fast filter-bank paths for dwt / idwt of this shape: the
 * approximation ping-pong, 2 * (N / 2^ndims) elements (N = number of samples; for dwtc pass
 * ndims = 1 and dims[0] = len * nsignals).  wl_ctx_reserve grows the context's workspace
 * once so that later calls of that kind never allocate.  Lifting transforms, long (> 10 taps
 * in 2-D) / odd-length filters, 3-D boxes and the generic kernel family use up to 4 N more
 * elements: the context grows to that on their first call.  Growth inside a transform call is STREAM-ORDERED (hipFreeAsync /
 * hipMallocAsync on the call's stream: the old block is released behind the work already queued, nothing waits on the host and
 * the device is not synchronised); wl_ctx_reserve itself, which takes no stream, synchronises the device when it has to grow.
 * wl_ctx_workspace_held reports the current size.                                                                          */
WL_API size_t wl_workspace_bytes(int dtype, int ndims, const int64_t *dims, int L);
/* Upper bound for every TRANSFORM entry point on this shape (wl_dwt_*, wl_dwtc_*, wl_wpt_*: lifting, long / odd filters,
 * 3-D, the generic kernel family): reserve this much and no later transform of that shape allocates or synchronises,
 * whatever path it takes.  NOT covered: wl_denoise_ti_filter, whose batch of shifted copies needs about
 * (6.5 * prod(nspin) + nspin[0]) N elements (capped, see WL_TI_WS_CAP_MB) -- a plain one-spin denoise about 5.5 N -- and grows
 * the workspace (synchronising) on its first call like any other path; wl_modwt / wl_imodwt allocate nothing here.      */
WL_API size_t wl_workspace_bytes_full(int dtype, int ndims, const int64_t *dims, int L);
/* wl_bestbasistree_filter of an n-sample vector holds more than that bound: the packet region of wl_workspace_bytes_full(dtype, 1,
 * {n}, L), rounded up to 256 bytes, then two packet buffers of n elements (each rounded up to 256 bytes), the node entropies
 * (ntree + 2^(Lmax-1) doubles, unless the caller passes node_entropy), the best-subtree values (ntree doubles), the reduction
 * partials (n / 1024 + 64 doubles), the norm (256 bytes) and three node byte vectors (3 ntree bytes, each rounded up to 256):
 * about (ws_elems + 2) n elements + 2.1 n doubles + 3 n bytes.  wl_coefentropy holds (n / 1024 + 72) doubles.
 * wl_bestbasistree_filter_batch holds that per group of G units, with N = G * n in place of n in the packet region and
 * the two packet buffers and G times the entropies, best-subtree values, partials and split bytes: the exact formula is in the
 * comment of that entry point.                                                                                             */
WL_API int wl_ctx_reserve(wl_ctx *ctx, size_t bytes);
WL_API size_t wl_ctx_workspace_held(const wl_ctx *ctx);
/* hipStreamSynchronize for hosts without their own HIP binding.                        */
WL_API int wl_stream_sync(wl_ctx *ctx, void *stream);
WL_API const char *wl_strerror(int status);
WL_API int wl_last_hip_error(const wl_ctx *ctx);
WL_API int wl_version(void);

/* ---- helpers mirroring src/Util -------------------------------------------------- */
/* maxtransformlevels(n) (non_dyadic.jl:14-23)                                          */
WL_API int wl_maxtransformlevels(int64_t n);

/* ---- filter-bank DWT / IDWT ------------------------------------------------------- */
/* y = dwt(x, OrthoFilter(qmf), L) (fw != 0) or idwt (fw == 0); 1-D, 2-D or 3-D.
 * replaces _dwt!(y, x, filter::OrthoFilter, L, fw) -- transforms_filter.jl:13-62 (1-D),
 * :113-188 (2-D), :192-294 (3-D).  y and x must not alias; sizes need a 2^L factor in
 * every dimension; L == 0 copies.  Output layout [s_L ; d_L ; ... ; d_1] (1-D) /
 * Mallat quadrants (2-D/3-D) exactly as the reference.                                 */
WL_API int wl_dwt_filter(wl_ctx *ctx, int dtype, void *y, const void *x,
                  int ndims, const int64_t *dims,
                  const double *qmf, int flen, int L, int fw, void *stream);

/* ---- lifting DWT / IDWT ------------------------------------------------------------ */
/* In place on y: dwt!(y, scheme::GLS, L) / idwt!(y, scheme, L).
 * replaces _dwt!(y, scheme::GLS, L, fw) -- transforms_lifting.jl:30-76 (1-D), :128-194
 * (2-D, square only), :200-278 (3-D, cube only).  The scheme is passed flattened in table
 * order (wt_main.jl:451-480): step i has type step_is_update[i] (0 = WT.Predict: updates
 * the first/approximation half, 1 = WT.Update: updates the second/detail half), ncoef[i]
 * coefficients and shift step_shift[i]; coefs_flat holds the coefficients back to back.
 * Sign/order/reciprocal adjustments for the direction are done inside (makescheme).     */
WL_API int wl_dwt_lifting(wl_ctx *ctx, int dtype, void *y,
                   int ndims, const int64_t *dims,
                   int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                   const int32_t *step_shift, const double *coefs_flat,
                   double norm1, double norm2, int L, int fw, void *stream);
/* Out-of-place variant: y = dwt(x, scheme, L) without the reference's copyto!(y, x)
 * (transforms_main.jl:119-124); same result as copy + in place.  y == x is allowed.    */
WL_API int wl_dwt_lifting_oop(wl_ctx *ctx, int dtype, void *y, const void *x,
                       int ndims, const int64_t *dims,
                       int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                       const int32_t *step_shift, const double *coefs_flat,
                       double norm1, double norm2, int L, int fw, void *stream);

/* ---- batched column-wise DWT ("dwtc") ------------------------------------------------ */
/* 1-D transform of every column of a len x nsignals column-major matrix with leading
 * dimension ld >= len.  The reference names dwtc/idwtc (transforms_main.jl:179-181,188)
 * but never implements them; this build defines them as the 1-D _dwt! per column.       */
WL_API int wl_dwtc_filter(wl_ctx *ctx, int dtype, void *y, const void *x,
                   int64_t len, int64_t nsignals, int64_t ld,
                   const double *qmf, int flen, int L, int fw, void *stream);
WL_API int wl_dwtc_lifting(wl_ctx *ctx, int dtype, void *y,
                    int64_t len, int64_t nsignals, int64_t ld,
                    int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                    const int32_t *step_shift, const double *coefs_flat,
                    double norm1, double norm2, int L, int fw, void *stream);
/* Out-of-place variant (x -> y, same shapes and ld): saves the copy a caller would otherwise make before the in-place call and
 * the staging copy the in-place first level needs (y == x is allowed and is the in-place call).                              */
WL_API int wl_dwtc_lifting_oop(wl_ctx *ctx, int dtype, void *y, const void *x,
                        int64_t len, int64_t nsignals, int64_t ld,
                        int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                        const int32_t *step_shift, const double *coefs_flat,
                        double norm1, double norm2, int L, int fw, void *stream);

/* ---- a batch of independent 2-D transforms ----------------------------------------------- */
/* y[:, :, i] = dwt(x[:, :, i], filter, L) (fw = 0: idwt) for i = 0 .. nimages-1: nimages images of dims[0] x dims[1]
 * (column-major, dense), image i at element offset i * image_stride of x and of y (image_stride >= dims[0] * dims[1]).
 * The same results as nimages calls of wl_dwt_filter with ndims = 2 -- the reference has no batched form
 * (transforms_filter.jl:113-188 is the per-image loop) -- but every level is ONE launch over all images: mid-size images,
 * whose single transform is launch latency rather than bandwidth, fill the chip together.  Workspace:
 * wl_workspace_bytes(dtype, 1, {nimages * image_stride}, L) is an upper bound for the fast paths.                          */
WL_API int wl_dwt_filter_batch(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, int64_t nimages,
                        int64_t image_stride, const double *qmf, int flen, int L, int fw, void *stream);

/* ---- a batch of independent 3-D transforms ----------------------------------------------- */
/* y[:, :, :, i] = dwt(x[:, :, :, i], filter, L) (fw = 0: idwt) for nvolumes boxes of dims[0] x dims[1] x dims[2]
 * (column-major, dense), volume i at element offset i * volume_stride (>= dims[0]*dims[1]*dims[2]) of x and of y.
 * The same results, bit for bit, as nvolumes calls of wl_dwt_filter with ndims = 3 (transforms_filter.jl:192-294 per volume;
 * any box with a 2^L factor per dimension, not only cubes), but every level that one of the one-launch 3-D kernels takes --
 * boxes of <= 4096 elements (all remaining levels), the LDS blocks up to 2^18 elements, the one-pass kernels above -- is ONE
 * launch over all volumes (groups of 65535): patches of a CT / MRI volume, video blocks, whose single transform is launch latency.
 * Other levels (the axis-pass, any-extent and generic families), odd or > 10-tap filters, wl_ctx_set_path(ctx, 1) and a
 * volume_stride that leaves a volume base off a 16-byte boundary run volume after volume.  L = 0 copies the volumes; the padding
 * between volumes is never written at any L.  The call only enqueues (capturable in a hipGraph).  Status codes in this order:
 * WL_EINVAL_ARG, WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS, WL_EINVAL_L, WL_EINVAL_SIZE, WL_EALIAS (y == x).
 * Workspace, with N = dims[0]*dims[1]*dims[2] and G = min(nvolumes, 65535): the approximation ping-pong of every volume of a
 * group plus one volume's inter-pass buffers, 2 * (G * (N / 8) + 64) + 3 N + 64 elements; nothing is allocated once
 * wl_workspace_bytes_full(dtype, 1, {nvolumes * volume_stride}, L) bytes are reserved.  Lifting schemes on a batch of
 * volumes: wl_dwt_lifting_batch3.                                                                                          */
WL_API int wl_dwt_filter_batch3(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, int64_t nvolumes,
                         int64_t volume_stride, const double *qmf, int flen, int L, int fw, void *stream);

/* y[:, :, i] = dwt(x[:, :, i], scheme, L) (fw = 0: idwt) for nimages SQUARE images of dims[0] x dims[1], laid out as for
 * wl_dwt_filter_batch; the scheme is passed as for wl_dwt_lifting.  The same results, bit for bit, as nimages calls of
 * wl_dwt_lifting_oop with ndims = 2 (transforms_lifting.jl:128-196 per image), but every level is ONE launch over all images
 * (groups of 65535) and the deepest levels of every image finish in one launch, a workgroup per image.  y == x is allowed and is
 * dwt!(y, scheme, L) of every image; L = 0 copies the images and leaves the padding between them alone.  Status codes in this
 * order: WL_EINVAL_ARG, WL_EINVAL_DTYPE, WL_EINVAL_CUBE (dims[0] != dims[1]), WL_EDIMS, WL_EINVAL_L, WL_EINVAL_SIZE,
 * WL_EINVAL_SCHEME.  Workspace: nothing is allocated once wl_workspace_bytes_full(dtype, 1, {nimages * image_stride}, L)
 * bytes are reserved.  What the tile and tail tiers really hold is the approximation ping-pong of every image of a group,
 * 2 * (min(nimages, 65535) * dims[0]^2 / 2 + 64) elements; an in-place batch of images of more than 64 rows adds a dense copy
 * of the group, and schemes or alignments the fast tiers refuse use the full amount.                                       */
WL_API int wl_dwt_lifting_batch(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, int64_t nimages,
                         int64_t image_stride, int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                         const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2, int L, int fw,
                         void *stream);

/* y[:, :, :, i] = dwt(x[:, :, :, i], scheme, L) (fw = 0: idwt) for nvolumes CUBES of dims[0..2], volume i at element offset
 * i * volume_stride (>= dims[0]^3) of x and of y; the scheme is passed as for wl_dwt_lifting.  The same results, bit for bit, as
 * nvolumes calls of wl_dwt_lifting_oop with ndims = 3 (transforms_lifting.jl:200-272 per volume), but every launch of the single
 * cube's level loop is ONE launch over all volumes (groups of 65535): the plane, row and column passes, the fused plane kernel
 * from 128 per side, and the deepest levels (<= 32^3 Float32, 16^3 Float64) in one launch, a workgroup per volume.  Batched are
 * the cubes the single call has fast kernels for -- the cdf9/7-, db2- and haar-shaped schemes, a power-of-two side of 8 .. 512,
 * 16-byte aligned x and y -- with a volume_stride that keeps every volume base 16-byte aligned; every other scheme, side or
 * stride, wl_ctx_set_path(ctx, 1) and the context option WL_LIFT_BATCH3_LOOP = 1 run volume after volume.  y == x is allowed and
 * is dwt!(y, scheme, L) of every volume; L = 0 copies the volumes; the padding between volumes is never written at any L.  The
 * call only enqueues (capturable in a hipGraph).  Status codes in this order: WL_EINVAL_ARG, WL_EINVAL_DTYPE, WL_EINVAL_CUBE (the
 * extents are not all equal), WL_EDIMS (an extent or nvolumes < 1, volume_stride < dims[0]^3), WL_EINVAL_L, WL_EINVAL_SIZE,
 * WL_EINVAL_SCHEME.  Workspace: nothing is allocated once wl_workspace_bytes_full(dtype, 1, {nvolumes * volume_stride}, L)
 * bytes are reserved.  What the batched tiers really hold, with N = dims[0]^3 and G = min(nvolumes, 65535): nothing when the
 * one-workgroup tail is the whole transform (side <= 32 Float32, 16 Float64); else the approximation ping-pong and the two dense
 * inter-pass buffers of a group, 2 * (G * (N / 8) + 64) + 2 G N + 64 elements.  The volume-after-volume loop holds one volume's
 * full workspace.                                                                                                          */
WL_API int wl_dwt_lifting_batch3(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, int64_t nvolumes,
                          int64_t volume_stride, int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                          const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2, int L, int fw,
                          void *stream);

/* ---- wavelet packet transform (1-D) --------------------------------------------------- */
/* y = wpt(x, filter, tree) / iwpt.  tree: one byte per node of the BitVector
 * (length 2^maxtransformlevels(n) - 1, util_main.jl:301-344), HOST pointer; it is copied before the call returns (the node
 * bits of partially split depths travel through a pinned staging buffer of the context) and the stream is NOT synchronised.
 * A call with a partially split tree is not capturable in a hipGraph (its staging copy would be replayed with stale bits).
 * replaces _wpt!(y, x, filter, tree, fw) -- transforms_filter.jl:301-359.               */
WL_API int wl_wpt_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n,
                  const double *qmf, int flen,
                  const uint8_t *tree, int64_t ntree, int fw, void *stream);
/* In place: wpt!(y, scheme, tree).  replaces _wpt!(y, scheme::GLS, tree, fw) --
 * transforms_lifting.jl:283-319.                                                        */
WL_API int wl_wpt_lifting(wl_ctx *ctx, int dtype, void *y, int64_t n,
                   int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                   const int32_t *step_shift, const double *coefs_flat,
                   double norm1, double norm2,
                   const uint8_t *tree, int64_t ntree, int fw, void *stream);

/* wpt(x, wt, L::Integer) / iwpt(x, wt, L) / wpt!(y, x, filter, L) / wpt!(y, scheme, L): the FULL tree of depth L
 * (= maketree(length(x), L, :full), transforms_main.jl:134-176) without a tree vector.  A tree of an n-sample signal has
 * n - 1 nodes; building, validating and scanning it on the host costs more than the transform itself from a few 10^5
 * samples on, and these entry points never look at one.  0 <= L <= maxtransformlevels(n), else WL_EINVAL_L.
 * Same results as the tree forms with the full tree; no stream synchronisation; capturable in a hipGraph.              */
WL_API int wl_wpt_filter_full(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n,
                       const double *qmf, int flen, int L, int fw, void *stream);
WL_API int wl_wpt_lifting_full(wl_ctx *ctx, int dtype, void *y, int64_t n,
                        int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                        const int32_t *step_shift, const double *coefs_flat,
                        double norm1, double norm2, int L, int fw, void *stream);

/* ---- wavelet packet transform (2-D) --------------------------------------------------- */
/* y = wpt2(x, filter, tree) / iwpt2 of a dims[0] x dims[1] column-major image over a quadtree.  The reference has no such
 * transform (WPTArray = AbstractVector); the definition is DESIGN.md section 22: the node at depth d with block coordinates
 * (bi, bj) is the sub-block of rows bi dims[0] / 2^d ... and columns bj dims[1] / 2^d ...; splitting it replaces the block by its
 * one-level 2-D dwt, periodic within the block, whose quadrants [[ss, sd], [ds, dd]] are the children c = ci + 2 cj (ci = 1: the
 * lower half of dimension 0, cj = 1: the right half of dimension 1).  tree: one byte per node in breadth-first order, node k has
 * the children 4k + 1 + c, depth d starts at (4^d - 1) / 3 and is ordered by the Morton code of (bi, bj) with bi in the even bits;
 * ntree = (4^L - 1) / 3 for an L >= 0 with dims[i] % 2^L == 0, and no set node below a clear one -- otherwise WL_EINVAL_TREE.  A
 * tree whose root is clear (and ntree == 0) is a copy.  iwpt2 (fw == 0) undoes the splits, children before parents.
 * tree is a HOST pointer; it is copied before the call returns (through a pinned staging buffer of the context) and the stream is
 * NOT synchronised.  A call with a partially split tree is not capturable in a hipGraph (its staging copy would be replayed with
 * stale bits).  Out of place only.  Two kernels, named by wl_last_kernel: "k_wpt2_level" (one depth per pass over the image) and
 * "k_wpt2_tail" (every depth from the first whose nodes hold at most "WL_WPT2_TAIL_MAX" elements, in one launch; the option is
 * clamped to 1 .. 4096, the default is 256, and 1 means the tail is never used); "copy" when nothing splits.  Workspace: one plane of the
 * image (when two or more passes run) plus the tree.
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / y / x / dims / qmf, NULL tree with ntree > 0), WL_EINVAL_DTYPE,
 * WL_EINVAL_FILTER, WL_EDIMS (an extent < 1 or >= 2^31), WL_EALIAS (y == x), WL_EINVAL_TREE.                                  */
WL_API int wl_wpt2_filter(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims,
                          const double *qmf, int flen, const uint8_t *tree, int64_t ntree, int fw, void *stream);
/* The FULL quadtree of depth L without a tree vector: never sees a tree, no stream synchronisation, capturable in a hipGraph
 * once the workspace is held.  Same results as wl_wpt2_filter with the full tree of depth L; L == 0 is a copy.
 * Status codes in this order: WL_EINVAL_ARG, WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS, WL_EINVAL_L (L < 0), WL_EINVAL_SIZE
 * (dims[i] % 2^L != 0), WL_EALIAS (y == x).                                                                                  */
WL_API int wl_wpt2_filter_full(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims,
                               const double *qmf, int flen, int L, int fw, void *stream);

/* ---- maximal-overlap DWT, 1-D -------------------------- */
/* floor(log2(n)) -- replaces maxmodwttransformlevels, src/Util/non_dyadic.jl:24-25.        */
WL_API int wl_maxmodwttransformlevels(int64_t n);
/* W = modwt(x, filter, L): `out` is the n x (L+1) matrix (column-major, leading dimension
 * ldo >= n): column j-1 = level-j detail coefficients, column L = level-L scaling
 * coefficients.  Taps are used in Float64 (divided by sqrt 2) and every partial sum is
 * rounded to the element type, exactly as the reference's `w1[t] += h[n] * v[k]` does.
 * Errors: L > floor(log2 n) -> WL_EINVAL_SIZE ("Too many transform levels"), L < 1 ->
 * WL_EINVAL_L.  replaces modwt + modwt_step, src/Transforms/transforms_maximal_overlap.jl:10-63. */
WL_API int wl_modwt(wl_ctx *ctx, int dtype, void *out, int64_t ldo, const void *x, int64_t n,
             const double *qmf, int flen, int L, void *stream);
/* x = imodwt(xw, filter): xw is n x ncols (leading dimension ldw), x must not alias it.
 * replaces imodwt + imodwt_step, transforms_maximal_overlap.jl:72-107.                     */
WL_API int wl_imodwt(wl_ctx *ctx, int dtype, void *x, const void *xw, int64_t ldw, int64_t n, int ncols,
              const double *qmf, int flen, void *stream);
/* ---- maximal-overlap DWT of a batch ------------------------------------------------------------------- */
/* out_u = modwt(x_u, filter, L) of nunits independent vectors: unit u of x is the n elements at element offset u * unit_stride
 * (>= n); unit u of out is the column-major n x (L+1) matrix at u * out_unit_stride, leading dimension ldo >= n,
 * out_unit_stride >= ldo * (L+1); columns as wl_modwt lays them out (column j-1 = level-j details, column L = level-L scaling
 * coefficients).  The reference has no batched form; the result is BIT FOR BIT what nunits calls of wl_modwt give (the arithmetic
 * is the one of wl_modwt on every path: Float64 taps / sqrt 2, tap order, every partial sum rounded to the element type).  In the
 * fused library the batch meets the tolerance contract of wl_modwt there; bit equality between the tiers is not claimed in it.
 * Nothing outside [0, n) of any column of any unit is written: not the rows n .. ldo-1, not the columns behind L, not the padding
 * between units.  The call only enqueues on `stream`, never synchronises, and is capturable in a hipGraph once the workspace is
 * held.  Two tiers, named by wl_last_kernel:
 *  - "k_modwt_lds": units with 2 * n * sizeof(T) <= 64 KB (n <= 8192 Float32, n <= 4096 Float64): ONE launch runs all L levels,
 *    the scaling coefficients ping-ponged in LDS; each unit is read once and each output column written once.  No limit on nunits.
 *  - "k_modwt_step_b": longer units, or every batch after wl_ctx_set_option(ctx, "WL_MODWT_FUSED", 0): one launch per level over
 *    all units of a group (the kernels of wl_modwt with the unit in the grid's y).  16-byte accesses need every unit base on a
 *    16-byte boundary (n, ldo and, for nunits > 1, the two unit strides multiples of 16 bytes, x and out aligned); any other
 *    batch takes the element-wise kernel, as wl_modwt does.
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / out / x / qmf), WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS (n < 1,
 * nunits < 1, unit_stride < n, ldo < n, out_unit_stride < ldo * (L+1), a product that no int64 holds or nunits * stride >= 2^60),
 * WL_EALIAS (the units of out and of x overlap), WL_EINVAL_SIZE (L > floor(log2 n)), WL_EINVAL_L (L < 1).
 * Workspace: the LDS tier holds nothing.  The per-level tier takes the units in groups of G -- all of them, at most 65535 (context
 * option WL_MODWT_BATCH_GROUP lowers it), halved until the group's two scaling buffers, 2 * G * n elements, are below the
 * context's cap (option WL_TI_WS_CAP_MB, default 8192) -- and holds those 2 * G * n elements; groups change no bit.              */
WL_API int wl_modwt_batch(wl_ctx *ctx, int dtype, void *out, int64_t ldo, int64_t out_unit_stride, const void *x, int64_t n,
                          int64_t nunits, int64_t unit_stride, const double *qmf, int flen, int L, void *stream);
/* x_u = imodwt(xw_u, filter) of nunits coefficient matrices laid out as wl_modwt_batch writes them (n x ncols, leading dimension
 * ldw >= n, unit u at u * xw_unit_stride >= ldw * ncols); x_u is the n elements at u * unit_stride (>= n).  BIT FOR BIT nunits calls
 * of wl_imodwt; ncols == 1 copies the column, as wl_imodwt does ("copy").  Tiers "k_imodwt_lds" / "k_imodwt_step_b", padding,
 * stream and workspace rules as above.  Status codes in this order: WL_EINVAL_ARG (NULL ctx / x / xw / qmf), WL_EINVAL_DTYPE,
 * WL_EINVAL_FILTER, WL_EDIMS (as above, with ldw, xw_unit_stride and ncols), WL_EALIAS, WL_EINVAL_L (ncols < 1, ncols - 1 > 62).  */
WL_API int wl_imodwt_batch(wl_ctx *ctx, int dtype, void *x, int64_t unit_stride, const void *xw, int64_t ldw, int64_t xw_unit_stride,
                           int64_t n, int ncols, int64_t nunits, const double *qmf, int flen, void *stream);
/* ---- MODWT multiresolution analysis of a batch --------------------------------------------------------- */
/* out_u = mra(xw_u, filter): the details D_1 .. D_L and the smooth S_L of nunits coefficient matrices (L = ncols - 1).  xw and out
 * are laid out as wl_modwt_batch writes its result: unit u is the column-major n x ncols matrix at u * unit stride, leading
 * dimension >= n, unit stride >= ld * ncols.  Column c of out_u is imodwt(Z_c, filter), Z_c = xw_u with every column but c set to
 * +0: columns 0 .. L-1 are D_1 .. D_L, column L is S_L; they are aligned with x and add up to it for an orthogonal filter.  The
 * reference has no such function; it is defined by that loop of its own imodwt.  The device computes column c without the zero
 * terms: one one-sided step with h at level c+1 (the smooth: with g at level L), then one-sided steps with g down to level 1, each
 * with the tap order, the per-tap rounding to the element type and the wrap-around of wl_imodwt.  For finite input the result is
 * == the loop's, element for element; the sign of a zero is not part of the contract (dropping `h * 0 +` can turn -0 into +0).
 * For non-finite input the loop turns a column into NaN wherever 0 * Inf reaches it from the zeroed columns; this call propagates
 * only what is in the column's own cascade.  ncols is not bounded by log2 n (strides are reduced mod n once per level);
 * ncols == 1 copies the column ("copy").  In the fused library the call meets the tolerance contract of wl_modwt there.
 * Nothing outside [0, n) of a column of a unit of out is written.  The call only enqueues on `stream`, never synchronises, and is
 * capturable in a hipGraph once the workspace is held.  There is no in-place form.  Two tiers, named by wl_last_kernel:
 *  - "k_modwt_mra_lds": units with 2 * n * sizeof(T) <= 64 KB: ONE launch; a workgroup owns whole planes (unit, column), loads the
 *    column into LDS, runs the plane's cascade there and stores the last step to out: each coefficient column is read once and each
 *    column of out written once.  No limit on nunits * ncols.
 *  - "k_modwt_mra_step_b": longer units, or every batch after wl_ctx_set_option(ctx, "WL_MODWT_FUSED", 0): for level s = L .. 1 two
 *    launches over the planes active at that level (column s-1 takes h from xw; the columns behind it take g from their buffer).
 *    16-byte accesses under the rule of wl_modwt_batch, applied to both tensors.
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / out / xw / qmf), WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS (n < 1,
 * nunits < 1, ldo < n, ldw < n, a unit stride below ld * ncols, a product that no int64 holds or nunits * stride >= 2^60),
 * WL_EALIAS (the byte ranges of out and xw overlap), WL_EINVAL_L (ncols < 1, ncols - 1 > 62).
 * Workspace: the LDS tier and the copy hold nothing.  The per-level tier takes the units in groups of G -- all of them, at most
 * 65535 / ncols (option WL_MODWT_BATCH_GROUP lowers it), halved until the group's two plane buffers are below the context's cap
 * (option WL_TI_WS_CAP_MB) -- and holds 2 * G * ncols * n elements; groups change no bit.                                       */
WL_API int wl_modwt_mra_batch(wl_ctx *ctx, int dtype, void *out, int64_t ldo, int64_t out_unit_stride, const void *xw, int64_t ldw,
                              int64_t xw_unit_stride, int64_t n, int ncols, int64_t nunits, const double *qmf, int flen, void *stream);

/* ---- thresholding and noise estimate -------------------- */
/* THType of src/Threshold/threshold_main.jl:8-15 (BiggestTH has its own entry point).      */
enum wl_thtype { WL_TH_HARD = 0, WL_TH_SOFT = 1, WL_TH_SEMISOFT = 2, WL_TH_STEIN = 3, WL_TH_POS = 4, WL_TH_NEG = 5 };
/* threshold!(x, TH, t) in place on n elements.  t_is_f64 selects the arithmetic type Julia's
 * promotion gives `x[i] op t`: 0 = the element type (t is an Integer or has the element
 * type), 1 = Float64 (t::Float64, e.g. sigma*dnt.t in denoise), result rounded to the
 * element type on store.  t is ignored for WL_TH_POS / WL_TH_NEG; t < 0 -> WL_EINVAL_ARG
 * (the reference's @assert).  replaces threshold!, threshold_main.jl:37-122.               */
WL_API int wl_threshold(wl_ctx *ctx, int dtype, void *x, int64_t n, int th, double t, int t_is_f64, void *stream);
/* threshold!(x, BiggestTH(), m): keep the m entries of largest magnitude, zero the rest
 * (exact order-statistic selection on device; ties at the cut are cleared in index order --
 * the reference's QuickSort leaves that order unspecified).  Synchronises `stream` once.
 * replaces threshold_main.jl:22-34.                                                        */
WL_API int wl_threshold_biggest(wl_ctx *ctx, int dtype, void *x, int64_t n, int64_t m, void *stream);
/* threshold!(x_u, TH, t_u) in place on every unit x_u = x[u * unit_stride .. + n), u < nunits, in one launch ("k_threshold_batch",
 * one launch per 65535 units; "k_threshold_batch_wave", a wave per unit, for units of at most 256 elements): the arithmetic of
 * wl_threshold on every unit, so each unit has the bits of wl_threshold on that
 * unit.  th: wl_thtype, all six kinds.  t_dev == NULL: the scalar t serves every unit; otherwise t_dev is a DEVICE array of nunits
 * doubles, one threshold per unit (t is ignored).  t_is_f64 as in wl_threshold; with 0 every threshold is converted to the element
 * type before the arithmetic.  A host t < 0 (or NaN) -> WL_EINVAL_ARG for Hard / Soft / Semisoft / Stein; device thresholds are
 * NOT validated (that would need a synchronisation): a negative or NaN entry yields whatever the reference's arithmetic yields
 * without its @assert (Hard with t < 0 keeps everything, NaN compares false throughout).  The padding between units is never read
 * or written.  No workspace.  Enqueues only: no synchronisation, capturable in a hipGraph.  Status codes in this order:
 * WL_EINVAL_ARG (NULL ctx / x), WL_EINVAL_DTYPE, WL_EDIMS (n < 1, nunits < 1, unit_stride < n, nunits * unit_stride overflows or
 * reaches 2^60), WL_EINVAL_ARG (th not a wl_thtype; host t < 0).                                                              */
WL_API int wl_threshold_batch(wl_ctx *ctx, int dtype, void *x, int64_t n, int64_t nunits, int64_t unit_stride, int th, double t,
                              const double *t_dev, int t_is_f64, void *stream);
/* threshold!(x_u, BiggestTH(), m_u) in place on every unit: the m_u entries of largest magnitude of unit u keep their bits, the
 * others become +0; ties at the cut are cleared in index order, lower index first, and NaNs order above every finite magnitude
 * -- unit for unit the bits of wl_threshold_biggest.  m_dev == NULL: the scalar m serves every unit (m > n is n); otherwise m_dev
 * is a DEVICE array of nunits int64, each entry clamped on the device to [0, n] (m is ignored).  Only cleared entries are written,
 * a unit with m_u >= n is not even read; the padding between units is never read or written.  Three tiers, chosen from n and
 * nunits alone: "k_thbig_lds" (a workgroup per unit, keys in LDS: units of up to 8192 Float32 / 4096 Float64 values; context
 * option WL_THB_LDS_MAX lowers the limit, 0 = never), "k_thbig_stream" (a workgroup per unit streams it from memory), and
 * "k_thbig_split" (several workgroups per unit, a fixed number of launches whatever nunits: units of at least WL_THB_SPLIT_N
 * elements in batches of at most WL_THB_SPLIT_UNITS units, and every unit of 2^31 elements or more; WL_THB_CHUNK = elements per
 * workgroup).  Only the split tier takes workspace (a state block per unit and a counter per chunk; units in groups under the
 * context's cap).  Enqueues only: never synchronises, no counter comes back to the host, capturable in a hipGraph once the
 * workspace is reserved.  Status codes in this order: WL_EINVAL_ARG (NULL ctx / x), WL_EINVAL_DTYPE, WL_EDIMS (as above),
 * WL_EINVAL_ARG (host m < 0), then WL_ENOMEM / WL_EHIP.                                                                         */
WL_API int wl_threshold_biggest_batch(wl_ctx *ctx, int dtype, void *x, int64_t n, int64_t nunits, int64_t unit_stride, int64_t m,
                                      const int64_t *m_dev, void *stream);
/* *result = median(v) (Statistics.median!: middle order statistic, or a/2 + b/2 of the two
 * middle ones; NaN if any NaN), computed in the element type and widened to double.  `v` is
 * not modified.  Synchronises `stream` (the result is a host scalar, as in the reference).  */
WL_API int wl_median(wl_ctx *ctx, int dtype, const void *v, int64_t n, double *result, void *stream);
/* *result = mad!(y): m = median!(y); y[i] = abs(y[i] - m); median!(y).  y is overwritten by
 * the absolute deviations.  replaces mad!, src/Threshold/denoising.jl:103-110 (noisest :92-101
 * = dwt level 1 + this on the level-1 detail range, divided by 0.6745 on the host).        */
WL_API int wl_mad(wl_ctx *ctx, int dtype, void *y, int64_t n, double *result, void *stream);
/* b[i] = a[i - shift] (periodic, every dimension; dims/shift have ndims entries, b != a).
 * replaces Util.circshift! (src/Util/util_main.jl:105-130) and Base.circshift as used by the
 * translation-invariant branch of denoise (denoising.jl:44-64).                            */
WL_API int wl_circshift(wl_ctx *ctx, int dtype, void *b, const void *a, int ndims, const int64_t *dims,
                 const int64_t *shift, void *stream);
/* y[i] += z[i] -- arrayadd!, denoising.jl:82-88.                                           */
WL_API int wl_arrayadd(wl_ctx *ctx, int dtype, void *y, const void *z, int64_t n, void *stream);
/* y[i] = T(y[i] * s) with s::Float64 -- rmul!(y, 1/pns), denoising.jl:66.                  */
WL_API int wl_rmul(wl_ctx *ctx, int dtype, void *y, int64_t n, double s, void *stream);

/* denoise(x, wt::OrthoFilter; L, dnt, TI = true, nspin) fused on the device (denoising.jl:21-67), 1-D vectors, square
 * matrices and cubes (WL_EINVAL_CUBE unless all extents are equal; nspin has ndims entries, spin i shifts by
 * nspin2circ(nspin, i), first dimension fastest; cubes of up to 2^20 - 1 per side, WL_EINVAL_SIZE beyond): the spins of a cube
 * run as a batch of volumes (the level loops of wl_dwt_filter_batch3), and prod(nspin) == 1 is the plain denoise of the array
 * with sigma kept on the device.  All prod(nspin) circularly shifted copies are transformed, thresholded and transformed back as ONE batch
 * (in groups when the buffers would exceed the context's cap), then un-shifted and summed in spin order -- the summation
 * order of the reference, so the result carries the same roundings -- and scaled by 1/prod(nspin).  The noise estimate
 * sigma = noisest(x, wt) = mad!(level-1 detail range) / 0.6745 is computed on the device and consumed there (no host
 * round trip) unless sigma_host >= 0 supplies it (a custom estnoise).  th: wl_thtype, t_unit: dnt.t (threshold =
 * sigma * t_unit in Float64).  y must not alias x.  Nothing is allocated per spin; the call only enqueues.            */
WL_API int wl_denoise_ti_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                         const double *qmf, int flen, int L, int th, double t_unit, const int64_t *nspin,
                         double sigma_host, void *stream);
/* The same for a lifting scheme (wt::GLS; scheme arguments as wl_dwt_lifting), vectors, square matrices and cubes (the rules of
 * wl_denoise_ti_filter: WL_EINVAL_CUBE unless all extents are equal, WL_EINVAL_SIZE from 2^20 per side): shifted signals run as
 * one batched-lines transform, shifted images one batched 2-D lifting transform, shifted cubes one batched 3-D lifting transform
 * (the level loop of wl_dwt_lifting_batch3; a scheme it has no kernels for runs cube after cube) per group of spins; sigma and
 * everything else stay on the device.
 * replaces the translation-invariant branch of denoise(x, wt::GLS; TI=true), denoising.jl:36-67 (round 4).               */
WL_API int wl_denoise_ti_lifting(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                          int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                          const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2,
                          int L, int th, double t_unit, const int64_t *nspin, double sigma_host, void *stream);

/* ---- denoise of a batch of independent units: per-unit noise estimates and thresholds on the device ---------------------- */
/* result[i] = mad!(y[i*stride .. i*stride + n)) for i < nunits: per-unit Statistics.median!, abs deviations, median! again
 * (denoising.jl:103-110), each in the element type and widened to double.  y is overwritten by the absolute deviations of its
 * unit, the padding between units is never written.  result: DEVICE pointer, nunits doubles.  NaN in a unit -> NaN for that
 * unit only.  One workgroup per unit: the keys of a unit of up to 8192 Float32 / 4096 Float64 values (context option
 * WL_MAD_LDS_MAX lowers the limit; 0 = never) live in LDS (k_mad_units_lds); a longer unit is streamed from memory once per radix
 * byte with the histograms in LDS (k_mad_units_stream).  No workspace.  Enqueues only: no synchronisation, capturable in a
 * hipGraph.  Status codes in this order: WL_EINVAL_ARG (NULL pointers), WL_EINVAL_DTYPE, WL_EDIMS (n < 1, nunits < 1,
 * stride < n), WL_EINVAL_SIZE (n >= 2^31: the per-unit counters are 32-bit).                                                */
WL_API int wl_mad_batch(wl_ctx *ctx, int dtype, void *y, int64_t n, int64_t nunits, int64_t stride, double *result, void *stream);

/* y[.., i] = denoise(x[.., i], OrthoFilter(qmf); L, dnt = (th, t_unit), TI = false) for nunits independent units:
 * ndims = 1 signals of dims[0] samples, 2 square images, 3 cubes (WL_EINVAL_CUBE otherwise), unit i at element offset
 * i * unit_stride (>= prod(dims)) of x and of y.  Per unit, the reference's own sequence (denoising.jl:30, 69-78):
 * sigma_i = noisest(x_i, wt) = mad!(level-1 detail range, linear indexing: rows [n0/2, n0) of the first column) / 0.6745,
 * c = dwt(x_i, wt, L); threshold!(c, th, sigma_i * t_unit) with the product in Float64; y_i = idwt(c, wt, L).
 * Same bits as nunits single calls.  ONE forward transform per unit: for L >= 1 the level-1 detail range of the L-level
 * coefficients is final after level 1 (deeper levels touch only the low corner), so sigma_i is read from the coefficients the
 * denoise needs anyway; L = 0 with sigma_in == NULL runs a level-1 batch for the estimate alone (dwt / idwt are copies then).
 * The transforms are the level loops of wl_dwtc_filter / wl_dwt_filter_batch / wl_dwt_filter_batch3 over all units of a group, the
 * noise estimate one launch (the kernels of wl_mad_batch, reading the coefficients without overwriting them), the threshold one
 * launch with t read per unit.  Where those level loops run every level over all units at once (lines and images; cubes with
 * filters of up to 10 taps; the lifting schemes the fast tiers accept) the number of launches does not depend on nunits within a
 * group; cubes with longer filters, the generic lifting fallback and the cube-after-cube fallback of wl_dwt_lifting_batch3
 * transform unit after unit, as they do in those entry points, and only the estimate and the threshold are one launch each
 * there.  x is not modified; the padding
 * between units of y is never written.
 * sigma_in: optional DEVICE array of nunits doubles used instead of the estimate (a custom estnoise; not validated);
 * sigma_out: optional DEVICE array that receives the sigma used for each unit.
 * th: WL_TH_HARD..WL_TH_STEIN; t_unit >= 0.  Enqueues only: no synchronisation, capturable in a hipGraph once the workspace is
 * held.  Status codes in this order: WL_EINVAL_ARG (NULL ctx / y / x / dims / qmf, th outside 0..3, t_unit negative or NaN),
 * WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EINVAL_CUBE, WL_EDIMS (ndims outside 1..3, an extent or nunits < 1, unit_stride <
 * prod(dims), an extent whose unit no int64 stride holds), WL_EINVAL_L, WL_EINVAL_SIZE (no 2^L factor, or an odd extent when the
 * estimate is needed -- sigma_in == NULL -- because noisest needs level 1), WL_EALIAS (y == x).
 * Workspace (wl_workspace_bytes_full does not cover it), with N = prod(dims), S = unit_stride and G units per group -- all
 * nunits, halved until the sum is below the context's cap (option WL_TI_WS_CAP_MB, default 8192) and at most 65535; groups
 * change no bit --, each part rounded up to 256 bytes:
 *   the transform workspace of a group    signals / images: 2 * (G N / 2^ndims + 64) + 3 G N + 64 elements,
 *                                         cubes: 2 * (G * (N / 8) + 64) + 3 N + 64 elements
 * + the coefficients C of the group       G * S elements (the caller's stride)
 * + the sigmas of the group               G doubles.                                                                          */
WL_API int wl_denoise_batch_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                                   int64_t nunits, int64_t unit_stride, const double *qmf, int flen, int L, int th,
                                   double t_unit, const double *sigma_in, double *sigma_out, void *stream);
/* The same for a GLS (scheme arguments as wl_dwt_lifting): out-of-place forward x -> y (the level loops of wl_dwtc_lifting_oop /
 * wl_dwt_lifting_batch / wl_dwt_lifting_batch3 with their fallbacks for schemes and strides the fast tiers refuse), the estimate and
 * the threshold on y, the inverse in place on y.  y == x is allowed.  Status codes in the order above with WL_EINVAL_SCHEME in the
 * place of WL_EINVAL_FILTER and no WL_EALIAS.  Workspace: the lifting transform workspace of a group -- signals / images
 * 2 * (G N / 2 + 64) + 3 G N + 64 elements; cubes the larger of 2 * (G * (N / 8) + 64) + 2 G N + 64 and one cube's
 * 2 * (N / 2 + 64) + 3 N + 64 -- + G doubles, + G * S elements only for L = 0 with sigma_in == NULL (the level-1 coefficients
 * of the estimate).                                                                                                           */
WL_API int wl_denoise_batch_lifting(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                                    int64_t nunits, int64_t unit_stride, int nsteps, const int32_t *step_is_update,
                                    const int32_t *step_ncoef, const int32_t *step_shift, const double *coefs_flat,
                                    double norm1, double norm2, int L, int th, double t_unit,
                                    const double *sigma_in, double *sigma_out, void *stream);

/* y[.., i] = denoise(x[.., i], OrthoFilter(qmf); L, dnt = (th, t_unit), TI = true, nspin) for nunits independent units, bit for
 * bit: units, layout and unit_stride as wl_denoise_batch_filter, nspin (ndims entries) and the shift of a spin as
 * wl_denoise_ti_filter -- spin s (0-based) shifts dimension d by nspin2circ with the first dimension fastest, vectors by s mod n.
 * Every unit gets its own sigma_i = noisest(x_i, wt), estimated from the unshifted unit and consumed on the device; sigma_in /
 * sigma_out as wl_denoise_batch_filter.  A plane is one shifted copy of one unit: plane p = u * prod(nspin) + s, unit-major.
 * Sequence: (1) unless sigma_in, a level-1 forward batch of the unshifted units into workspace, in groups of units, the per-unit MAD
 * of rows [n0/2, n0) of the first column (the kernels of wl_mad_batch) and sigma = mad / 0.6745, for all units first; (2) the planes
 * G at a time -- a group may begin and end inside a unit --: shift (k_ti_shift_units), forward batch (the level loops
 * wl_denoise_ti_filter runs for its spins; L = 0 thresholds the shifted copy), one threshold launch with
 * t = sigma[p / prod(nspin)] * t_unit in Float64 (k_threshold_planes), inverse batch, one un-shift / accumulate launch
 * (k_ti_accumulate_units) that adds a unit's planes in ascending spin order -- from (T)0 when the group holds the unit's spin 0,
 * from the stored y_u otherwise: the reference's arrayadd! order -- and scales the rounded sum by 1 / prod(nspin) when the group
 * holds the unit's last spin (rmul!).  prod(nspin) == 1 takes the same path: (0 + z) * 1, a -0.0 comes back +0.0, as in the
 * reference's TI branch.  x is not modified, the padding between units of y is never written.  Enqueues only: no synchronisation,
 * capturable in a hipGraph once the workspace is held.  wl_last_kernel: "denoise_ti_units+k_mad_units_lds", "...+k_mad_units_stream"
 * or "...+sigma_in".
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / y / x / dims / qmf / nspin, th outside 0..3, t_unit negative or NaN),
 * WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EINVAL_CUBE, WL_EDIMS (the rules of wl_denoise_batch_filter; an nspin[d] < 1; a product
 * nunits * prod(nspin) that no int64 holds), WL_EINVAL_L, WL_EINVAL_SIZE (the rules of wl_denoise_batch_filter; images of more than
 * 65535 columns, cubes from 2^20 per side), WL_EALIAS (y == x).
 * Workspace (wl_workspace_bytes_full does not cover it), with N = prod(dims), S = unit_stride and G planes per group -- all
 * nunits * prod(nspin), halved until the sum is below the context's cap (option WL_TI_WS_CAP_MB) and at most 65535; context option
 * WL_TI_BATCH_GROUP (0 = automatic) lowers G after the workspace is sized; groups change no bit --, each part rounded up to 256 bytes:
 *   the transform workspace of G planes   as wl_denoise_batch_filter's for G units
 * + the planes Z and their coefficients   max(2 G N, min(G, nunits) * S without sigma_in) elements (the level-1 coefficients of
 *                                         the estimate, at the caller's stride, live here before the first group)
 * + the sigmas                            nunits doubles, for the whole call.                                                      */
WL_API int wl_denoise_ti_batch_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                                      int64_t nunits, int64_t unit_stride, const double *qmf, int flen, int L, int th,
                                      double t_unit, const int64_t *nspin, const double *sigma_in, double *sigma_out, void *stream);
/* The same for a GLS (scheme arguments as wl_dwt_lifting): the transforms are those wl_denoise_ti_lifting runs for its spins (a
 * batched-lines call, one batched 2-D or one batched 3-D lifting transform per group, with their fallbacks; L = 0 copies).  Status
 * codes in the order above with WL_EINVAL_SCHEME in the place of WL_EINVAL_FILTER; y == x is WL_EALIAS here as well, because x is
 * re-read for every group of spins.  Workspace: as above with the lifting transform workspace of wl_denoise_batch_lifting for G
 * units in the first part.                                                                                                     */
WL_API int wl_denoise_ti_batch_lifting(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                                       int64_t nunits, int64_t unit_stride, int nsteps, const int32_t *step_is_update,
                                       const int32_t *step_ncoef, const int32_t *step_shift, const double *coefs_flat,
                                       double norm1, double norm2, int L, int th, double t_unit, const int64_t *nspin,
                                       const double *sigma_in, double *sigma_out, void *stream);

/* ---- best-basis search of packet trees (src/Threshold/entropy.jl) ----------------------- */
/* Entropy measures: ShannonEntropy (-s log s) and LogEnergyEntropy (-log s) of s = (x / nrm)^2; s == 0 contributes -0.0.    */
enum wl_entropy { WL_ENTROPY_SHANNON = 0, WL_ENTROPY_LOGENERGY = 1 };
/* Accuracy contract (the one exception to "bit-identical"): the reference's log is Julia's, its norm BLAS
 * nrm2 and its sums sequential in T, which no parallel reduction reproduces.  Here nrm = T(sqrt(Float64 sum of squares)) (about
 * 1 ulp of T from the reference's), s is computed exactly as the reference does (in T, IEEE division, no contraction), the log and
 * every sum are Float64 in a fixed order -- deterministic, the same bits call after call.  Against the exact entropy of the same T
 * coefficients: <= 1e-12 sum|term| (Float64), <= 4e-7 sum|term| (Float32).  nrm == 0 gives exactly 0; an all-zero node gives
 * exactly 0, so exact ties do not split.                                                                                   */
/* *result = coefentropy(x, et, nrm) (have_nrm != 0) or coefentropy(x, et) with nrm = norm(x) (entropy.jl:31-40), rounded to the
 * element type and widened to double.  nrm < 0 (or NaN) -> WL_EINVAL_ARG (the reference's @assert nrm >= 0); n == 0 gives 0.
 * Synchronises `stream` (the result is a host scalar), like wl_median.                                                    */
WL_API int wl_coefentropy(wl_ctx *ctx, int dtype, const void *x, int64_t n, int et, int have_nrm, double nrm, double *result,
                          void *stream);
/* tree_out = bestbasistree(x, OrthoFilter(qmf), tree, et) (entropy.jl:47-111): the best subtree of `tree` (one byte per node,
 * ntree = 2^maxtransformlevels(n) - 1 nodes, HOST pointers for tree and tree_out).  Every depth 0 .. Lmax of the full packet
 * decomposition comes from the packet transform (bit-identical to wl_wpt_filter), whatever `tree` is; node k's entropy entr_bf[k]
 * is taken over its segment before it splits, entr_af[j] over the two children of bottom node j together.  Then
 * best(k) = min(entr_bf[k], best(left) + best(right)) over the full tree (Julia's min: NaN propagates) and node k is split iff
 * tree[k], its parent is split and !(entr_bf[k] <= best(k)): exact ties do not split, a NaN splits every node of `tree` under
 * split parents.  node_entropy: optional DEVICE array (NULL allowed) of ntree + 2^(Lmax-1) doubles that receives
 * [entr_bf ; entr_af].  Errors: WL_EINVAL_SIZE when maxtransformlevels(n) == 0 (odd n), WL_EINVAL_TREE for an invalid tree.
 * Synchronises `stream` once to return the tree: not capturable in a hipGraph.  The workspace grows as noted at
 * wl_workspace_bytes_full.                                                                                                 */
WL_API int wl_bestbasistree_filter(wl_ctx *ctx, int dtype, const void *x, int64_t n, const double *qmf, int flen,
                                   const uint8_t *tree, int64_t ntree, int et, uint8_t *tree_out, double *node_entropy,
                                   void *stream);

/* ---- complex-valued transforms (ComplexF32 / ComplexF64) --------------------------------------------------------------------- */
/* The reference's transforms accept complex arrays (ValueType = Union{AbstractFloat, Complex}, transforms_main.jl:7).  Complex{T}
 * is (re, im) interleaved and the taps are real, so the result is defined as re(y) = transform(re(x)), im(y) = transform(im(x)),
 * each BIT FOR BIT what the real entry point returns for that component (for finite input equal under == to the reference's
 * complex arithmetic with taps a + 0i, which can differ in the sign of a zero only).  In this section
 * dtype stays the COMPONENT type (WL_F32: ComplexF32 data, WL_F64: ComplexF64), every pointer is a device pointer to interleaved
 * data, dims / n / unit_stride count COMPLEX elements, and nunits >= 1 independent arrays sit at complex-element offset
 * u * unit_stride (>= prod(dims)) of x and of y; nunits = 1 is the single transform.  All six calls only enqueue on `stream`.
 *
 * planes[(2u + c) * plane_stride + i] = component c (0 = re, 1 = im) of z[u * unit_stride + i], i < n, u < nunits: 2 * nunits planar
 * real planes of plane_stride (>= n, in real elements) from nunits interleaved units, and back.  16-byte accesses on both sides when
 * z, planes and every unit / plane base are 16-byte aligned (else, and for the n mod (16 / sizeof(T)) tail, an element per lane);
 * nothing outside [0, n) of a unit or of a plane is written.  No workspace.  Status codes in this order: WL_EINVAL_ARG,
 * WL_EINVAL_DTYPE, WL_EDIMS (n < 1, nunits < 1, unit_stride < n, plane_stride < n).                                            */
WL_API int wl_complex_split(wl_ctx *ctx, int dtype, void *planes, int64_t plane_stride, const void *z, int64_t n, int64_t nunits,
                            int64_t unit_stride, void *stream);
WL_API int wl_complex_merge(wl_ctx *ctx, int dtype, void *z, const void *planes, int64_t plane_stride, int64_t n, int64_t nunits,
                            int64_t unit_stride, void *stream);
/* y_u = dwt(x_u, OrthoFilter(qmf), L) (fw = 0: idwt) of nunits complex arrays of ndims = 1..3 dimensions (any box with a 2^L
 * factor per dimension).  replaces _dwt!(y, x, filter, L, fw) for Complex element types (transforms_filter.jl:13-294 with complex
 * taps).  Per group of G units: split x into 2 G planes P, run the batched level loop of the real entry point on them -- ndims = 1
 * wl_dwtc_filter with ld = plane_stride, 2 wl_dwt_filter_batch, 3 wl_dwt_filter_batch3, with their own fallbacks -- from P to Q,
 * merge Q into y.  plane_stride = prod(dims) rounded up to 16 bytes, so every plane base is 16-byte aligned.  L = 0 copies the
 * units without staging; the padding between units of y is never written.  Capturable in a hipGraph once the workspace is held.
 * wl_last_kernel reports the inner transform's kernel.  Status codes in this order: WL_EINVAL_ARG (NULL ctx / y / x / dims / qmf),
 * WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS (ndims outside 1..3, an extent or nunits < 1, unit_stride < prod(dims)), WL_EINVAL_L,
 * WL_EINVAL_SIZE, WL_EALIAS (y == x).
 * Workspace (wl_workspace_bytes_full does not cover it), with N = prod(dims), ps = plane_stride and G units per group -- all
 * nunits, halved until the sum is below the context's cap (option WL_TI_WS_CAP_MB, default 8192) and at most 32767; groups change
 * no bit --, each part rounded up to 256 bytes:
 *   the transform workspace of 2 G planes   signals / images: 2 * (2 G N / 2^ndims + 64) + 6 G N + 64 elements,
 *                                           volumes: 2 * (2 G * (N / 8) + 64) + 3 N + 64 elements
 * + the planes P and Q                      2 * (2 G ps) elements.                                                              */
WL_API int wl_dwt_filter_complex(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, int64_t nunits,
                                 int64_t unit_stride, const double *qmf, int flen, int L, int fw, void *stream);
/* The same for a GLS (scheme arguments as wl_dwt_lifting): vectors, SQUARE images and CUBES; y == x is allowed and is
 * dwt!(y, scheme, L).  Split x into P, run the lifting batch loop in place on P (wl_dwtc_lifting / wl_dwt_lifting_batch /
 * wl_dwt_lifting_batch3 with their fallbacks), merge P into y.  Status codes in this order: WL_EINVAL_ARG, WL_EINVAL_DTYPE,
 * WL_EINVAL_SCHEME, WL_EINVAL_CUBE, WL_EDIMS, WL_EINVAL_L, WL_EINVAL_SIZE.  Workspace: the lifting workspace of 2 G planes --
 * signals / images 2 * (G N + 64) + 6 G N + 64 elements; cubes the larger of 2 * (2 G * (N / 8) + 64) + 4 G N + 64 and one cube's
 * 2 * (N / 2 + 64) + 3 N + 64 -- + the planes P, 2 G ps elements.                                                                 */
WL_API int wl_dwt_lifting_complex(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, int64_t nunits,
                                  int64_t unit_stride, int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                                  const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2, int L, int fw,
                                  void *stream);
/* y = wpt(x, filter, tree) / iwpt of ONE complex signal of n values: split, the packet transform of wl_wpt_filter on the two
 * planes as one batch of two units of stride ps (the level loop of wl_wpt_filter_batch), merge.  tree == NULL: the full tree of depth L (wl_wpt_filter_full;
 * 0 <= L <= maxtransformlevels(n), else WL_EINVAL_L; capturable in a hipGraph).  Otherwise tree / ntree as wl_wpt_filter (HOST
 * pointer, copied before the call returns; not capturable for a partially split tree) and L is ignored.  y must not alias x.
 * Status codes in this order: WL_EINVAL_ARG, WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS, WL_EALIAS, WL_EINVAL_L / WL_EINVAL_TREE.
 * Workspace: the packet region of the two planes (wl_workspace_bytes_full(dtype, 1, {2 ps}, L)) rounded up to 256 bytes + the
 * planes P and Q, 2 * (2 ps) elements.                                                                                          */
WL_API int wl_wpt_filter_complex(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, const double *qmf, int flen,
                                 const uint8_t *tree, int64_t ntree, int L, int fw, void *stream);
/* The same for a GLS: wpt!(y, scheme, tree) of the copy of x (y == x allowed), the packet transform of wl_wpt_lifting in place on
 * each plane.  Workspace: the packet region + the planes P, 2 ps elements.                                                       */
WL_API int wl_wpt_lifting_complex(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, int nsteps,
                                  const int32_t *step_is_update, const int32_t *step_ncoef, const int32_t *step_shift,
                                  const double *coefs_flat, double norm1, double norm2, const uint8_t *tree, int64_t ntree, int L,
                                  int fw, void *stream);

/* ---- batched wavelet packet transforms ----------------------------------------------------------------------------------------- */
/* y_i = wpt(x_i, filter, tree) (fw = 0: iwpt) of nunits independent signals of n values that share ONE tree: unit i is the n
 * elements at element offset i * unit_stride (>= n) of x and of y.  The reference has no batched form; the result is BIT FOR BIT
 * what nunits calls of wl_wpt_filter / wl_wpt_filter_full on the units give, in one chain of launches over all units (the launch
 * plan is the one of a single unit of length n).  tree == NULL: the full tree of depth L (0 <= L <= maxtransformlevels(n), else
 * WL_EINVAL_L; capturable in a hipGraph once the workspace is held).  Otherwise tree is the HOST byte-per-node vector of
 * ntree = 2^maxtransformlevels(n) - 1 nodes, validated and staged as wl_wpt_filter does it (copied before the call returns; a
 * partially split tree is not capturable) and L is ignored.  Depth 0, an empty tree or an unset root copies the units.  The padding
 * between units of y is never written.  The call only enqueues on `stream`.
 * The packet kernels take a batch whose unit bases of x, y and the work buffer are all 16-byte aligned (x and y aligned and, for
 * nunits > 1, unit_stride * sizeof(T) a multiple of 16); any other batch, odd or > 10-tap filters, segments that are no power of
 * two and wl_ctx_set_path(ctx, 1) take the per-depth kernels with the unit as a third extent -- one launch per depth over all units
 * either way, never a loop over the units.  wl_last_kernel reports the kernel name of the single-unit transform: the batch runs
 * the same kernel instances (the single transform is their batch of one), in the fused library too.
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / y / x / qmf), WL_EINVAL_DTYPE,
 * WL_EINVAL_FILTER, WL_EDIMS (n < 1, nunits < 1, unit_stride < n, nunits * unit_stride >= 2^61), WL_EALIAS (y == x), WL_EINVAL_L
 * (tree == NULL), WL_EINVAL_TREE.
 * Workspace: units are taken in groups of G -- all of them, at most 65535 (context option WL_WPT_BATCH_GROUP lowers it), halved
 * until the work buffer G * unit_stride * sizeof(T) is below the context's cap (option WL_TI_WS_CAP_MB, default 8192); groups
 * change no bit.  With N = G * unit_stride the call holds 2 * (N / 2 + 64) + 3 N + 64 elements + the staged node bits (< n bytes,
 * partially split trees only) + 256 bytes: nothing is allocated once wl_workspace_bytes_full(dtype, 1, {nunits * unit_stride}, L)
 * bytes are reserved.                                                                                                            */
WL_API int wl_wpt_filter_batch(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, int64_t nunits, int64_t unit_stride,
                               const double *qmf, int flen, const uint8_t *tree, int64_t ntree, int L, int fw, void *stream);
/* The same for a GLS (scheme arguments as wl_dwt_lifting): y == x is the in-place wpt!(y, scheme, tree) of every unit, y != x
 * leaves x untouched (the first pass reads x and writes y).  Bit for bit nunits calls of wl_wpt_lifting / wl_wpt_lifting_full.
 * Fully split depths of a dense batch (unit_stride == n) are one launch of the fused line kernels over all segments of all units;
 * partially split depths and padded batches take the per-depth lifting passes with the unit as a third extent.  Status codes in
 * this order: WL_EINVAL_ARG, WL_EINVAL_DTYPE, WL_EINVAL_SCHEME, WL_EDIMS, WL_EINVAL_L, WL_EINVAL_TREE.  Workspace as above.       */
WL_API int wl_wpt_lifting_batch(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, int64_t nunits, int64_t unit_stride,
                                int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef, const int32_t *step_shift,
                                const double *coefs_flat, double norm1, double norm2, const uint8_t *tree, int64_t ntree, int L,
                                int fw, void *stream);

/* ---- per-unit trees: the batched best-basis search and the packet transforms of its result -------------- */
/* trees_out_u = bestbasistree(x_u, filter, tree, et) of nunits independent signals: unit u is the n elements at element offset
 * u * unit_stride (>= n) of x, its result the ntree = 2^maxtransformlevels(n) - 1 bytes at trees_out + u * tree_stride
 * (tree_stride >= ntree) in DEVICE memory; with node_entropy (DEVICE, or NULL) its [entr_bf ; entr_af] doubles (ntree + 2^(Lmax-1))
 * go to node_entropy + u * entropy_stride.  Padding between units of trees_out and node_entropy is never written.
 * Input tree: tree == NULL is maketree(n, L, :full) with 0 <= L <= Lmax (else WL_EINVAL_L; ntree is ignored, nothing is staged,
 * and the call is capturable in a hipGraph once the workspace is held); otherwise ONE HOST tree of ntree nodes shared by all
 * units, validated and staged as wl_wpt_filter_batch does it (L is ignored).  Per-unit input trees are not supported.
 * The result IS the loop of wl_bestbasistree_filter over the units, bit for bit -- tree bytes and node-entropy bits, in the exact and
 * in the fused library (a padded batch, unit_stride > n, is first copied into a dense work buffer, so that every depth runs the
 * kernels the single search runs) -- in one chain of launches over all units: per depth one packet
 * launch plus the reductions, then ceil(Lmax / 9) + 1 launches for the decision.  The accuracy contract of wl_bestbasistree_filter
 * applies unchanged.  The call only enqueues on `stream`; it never synchronises.
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / x / qmf / trees_out, unknown et), WL_EINVAL_DTYPE, WL_EINVAL_FILTER,
 * WL_EDIMS (n < 1, nunits < 1, unit_stride < n, tree_stride < ntree, entropy_stride < ntree + 2^(Lmax-1), products >= 2^61),
 * WL_EINVAL_SIZE (odd n), WL_EINVAL_L (tree == NULL), WL_EINVAL_TREE.
 * Workspace: units are taken in groups of G -- all of them, at most 65535 (context option WL_WPT_BATCH_GROUP lowers it), halved
 * until the group's workspace is below the context's cap (option WL_TI_WS_CAP_MB); groups change no bit.  With N = G * n,
 * up256(b) = b rounded up to 256 and P = (2 (N / 2 + 64) + 3 N + 64) sizeof(T) the packet region, a group holds
 *   up256(P + 256) + 2 up256(N sizeof(T)) + up256(G (ntree + 2^(Lmax-1)) 8) [absent with node_entropy] + up256(G ntree 8)
 *   + up256(G (n / 1024 + 64) 8) + up256(8 G) + up256(G ntree) + 2 up256(ntree)   bytes;
 * wl_bestbasistree_filter is G = 1 of the same formula.                                                                           */
WL_API int wl_bestbasistree_filter_batch(wl_ctx *ctx, int dtype, const void *x, int64_t n, int64_t nunits, int64_t unit_stride,
                                         const double *qmf, int flen, const uint8_t *tree, int64_t ntree, int L, int et,
                                         uint8_t *trees_out, int64_t tree_stride, double *node_entropy, int64_t entropy_stride,
                                         void *stream);
/* y_u = wpt(x_u, filter, trees_u) (fw = 0: iwpt) with ONE TREE PER UNIT in DEVICE memory: unit u's byte-per-node tree is at
 * trees + u * tree_stride (tree_stride >= 2^maxtransformlevels(n) - 1) -- what wl_bestbasistree_filter_batch leaves behind.  Layout
 * and aliasing rules of x and y are those of wl_wpt_filter_batch.  Nodes at depth >= L are ignored (0 <= L <= Lmax, else
 * WL_EINVAL_L; callers default to Lmax).  A device tree cannot be validated on the host: one launch closes every tree into the
 * workspace first -- a node counts iff it and every ancestor is set -- so an INVALID tree means its largest valid subtree.
 * Per unit the result equals wl_wpt_filter with that unit's (closed) tree bit for bit.  The launch plan is the one of a single
 * unit whose every depth < L is partially split; leaves pass through inside the launches.  The call only enqueues and is
 * capturable in a hipGraph once the workspace is held.
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / y / x / qmf / trees), WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS (as
 * wl_wpt_filter_batch, and tree_stride too small), WL_EALIAS, WL_EINVAL_L.
 * Workspace: units are taken in groups of G as wl_wpt_filter_batch takes them -- halved until the work buffer plus the closed trees,
 * G * (unit_stride * sizeof(T) + 2^L - 1) bytes, is below the cap, not the whole workspace -- and a group holds that call's bytes
 * (2 * (N / 2 + 64) + 3 N + 64 elements, N = G * unit_stride, + 256 bytes) with G (2^L - 1) bytes of closed trees in place of the
 * staged node bits.                                                                                                               */
WL_API int wl_wpt_filter_batch_trees(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, int64_t nunits, int64_t unit_stride,
                                     const double *qmf, int flen, const uint8_t *trees, int64_t tree_stride, int L, int fw,
                                     void *stream);

/* ---- matching pursuit (src/Threshold/basis_functions.jl:8-55) ---------------------------------------------------------------
 *   r = x; y = 0; it = 0; cap = (nmax == -1 ? N : nmax)
 *   while nrm(r) > tol && it < cap:  ftr = ft(r); i = findmaxabs(ftr); aphi = f(ftr[i] e_i); r = T(r - aphi); y[i] = T(y[i] + ftr[i]); it += 1
 * findmaxabs(v) is the FIRST index whose magnitude is strictly greater than every earlier one: v[0] NaN gives 0, a NaN anywhere else
 * never wins, an all-zero or all-equal vector gives 0, -0.0 and +0.0 tie.  nrm(r) = (double)(T)sqrt(s) with s the Float64 sum of
 * squares in a fixed order (same input, same bits; about 1 ulp of T from BLAS nrm2): the only place where the loop is not the
 * reference bit for bit, and it only gates termination.  A NaN norm ends the loop.
 * Option "WL_MP_MAX_BLOCKS" (wl_ctx_set_option; default 4 workgroups per CU, at most 65536) caps the grid of the two reductions: it
 * changes the order of the Float64 sum, never an index.
 *
 * *idx_dev = findmaxabs(v[0 .. len)), a 0-based index in DEVICE memory.  Enqueues only; capturable in a hipGraph once the workspace
 * is held (len > 4096 takes a few KiB of it).
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / v / idx_dev), WL_EINVAL_DTYPE, WL_EDIMS (len < 1).                        */
WL_API int wl_findmaxabs(wl_ctx *ctx, int dtype, const void *v, int64_t len, int64_t *idx_dev, void *stream);
/* The select of one atom, i = *idx_dev (device memory): spat[i % n] = ftr[i]; y[i] = T(y[i] + ftr[i]).  ftr and y hold ncoef
 * coefficients, spat holds n (a union of ncoef / n bases of n: the atom's position inside its base; a dense dictionary passes
 * n = ncoef).  An index outside [0, ncoef) selects nothing.  Enqueues only; capturable in a hipGraph.
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / spat / y / ftr / idx_dev), WL_EINVAL_DTYPE, WL_EDIMS (n < 1, ncoef < 1,
 * ncoef % n != 0).                                                                                                                 */
WL_API int wl_mp_select(wl_ctx *ctx, int dtype, void *spat, int64_t n, void *y, const void *ftr, int64_t ncoef,
                        const int64_t *idx_dev, void *stream);
/* r[t] = T(r[t] - aphi[t]) for t < n (one rounding per element), then *nrm = nrm(r).  aphi == NULL: r is left alone and only the
 * norm is formed.  spat != NULL (then spat_len == n and idx_dev != NULL): spat[*idx_dev % n] = 0, the spike wl_mp_select set.
 * Synchronises `stream` (the norm is a host scalar, as in the reference).
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / r / nrm, spat without idx_dev), WL_EINVAL_DTYPE, WL_EDIMS (n < 1, spat_len
 * neither 0 nor n, spat with spat_len 0).                                                                                          */
WL_API int wl_mp_residual(wl_ctx *ctx, int dtype, void *r, const void *aphi, int64_t n, void *spat, int64_t spat_len,
                          const int64_t *idx_dev, double *nrm, void *stream);
/* matchingpursuit over a union of `nbases` orthonormal wavelet bases of a vector of n (N = nbases * n coefficients):
 * ft(r)[k n + p] = dwt(r, filter k, Ls[k])[p], f of a spike in block k = idwt(that block, filter k, Ls[k]); the all-zero blocks are
 * not transformed, so for finite input the atom is == the literal sum and the sign of a zero is not part of the contract.  Ls[k] = 0
 * is the identity (the Dirac basis).  qmfs: the host concatenation of the flens[k] taps.  r holds the signal on entry and the
 * residual on exit (the reference's r = x overwrites x); y receives the N coefficients; *niter (atoms taken) and *nrm (the last
 * norm) are host outputs.  Per atom: nbases forward transforms, arg-max + select, ONE 24-byte read-back of {index, norm} behind a
 * stream synchronisation (the host must know which base to invert and whether to stop), one inverse transform, residual + norm.
 * wl_last_kernel: "matchingpursuit+<forward kernel of base 0>".
 * Status codes in this order: WL_EINVAL_ARG (NULL ctx / y / r / qmfs / flens / Ls / niter / nrm, nbases < 1, !(tol > 0), nmax < -1),
 * WL_EINVAL_DTYPE, WL_EINVAL_FILTER (any flens[k]), WL_EDIMS (n < 1, nbases * n beyond 2^60), WL_EALIAS (the byte ranges of y and r
 * overlap), then base by base what wl_dwt_filter returns for a vector of n with Ls[k] (WL_EINVAL_L, WL_EINVAL_SIZE).
 * Workspace: one transform's own (2 * (n / 2 + 64) + 3 n + 64 elements) + (nbases + 2) * n elements + a few KiB of partials.        */
WL_API int wl_matchingpursuit_filter(wl_ctx *ctx, int dtype, void *y, void *r, int64_t n, int nbases, const double *qmfs,
                                     const int *flens, const int *Ls, double tol, int64_t nmax,
                                     int64_t *niter, double *nrm, void *stream);

/* ---- introspection (tests / bench) ---------------------------------------------------- */
/* Select the kernel family: 0 = auto (fast paths where they apply), 1 = generic kernels
 * only.  Both produce bit-identical results; the switch exists so tests can prove it.   */
WL_API int wl_ctx_set_path(wl_ctx *ctx, int path);
/* Name of the dominant kernel used by the last transform call on this context.          */
WL_API const char *wl_last_kernel(const wl_ctx *ctx);
/* Tuning / test switches of this context (the library reads no environment variable).
 * key: e.g. "WL_FUSE2_MIN", "WL_TJ", "WL_NO_INV2D" (DESIGN.md section 5 lists them with their
 * defaults); keys shorter than 32 characters, at most 32 per context; unknown keys are stored
 * and ignored.  No option changes a result: they pick between kernel families that are
 * bit-identical by construction, which is what the tests use them to prove.                */
WL_API int wl_ctx_set_option(wl_ctx *ctx, const char *key, int64_t value);
WL_API int wl_ctx_clear_options(wl_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* WAVELETS_MI355X_H */

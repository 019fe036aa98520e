// wl_api.hip -- the C ABI of libwavelets_mi355x.so (include/wavelets_mi355x.h):
// argument contract of the reference's _dwt!/_wpt! methods, workspace management, and
// the host-side level loops that sequence the HIP kernels on the caller's stream.
#include "wl_internal.h"
#include "wl_fast.h"

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

using namespace wl;

#include "wl_entry.h"

thread_local const wl::Opts *wl::tl_opts = nullptr;
thread_local unsigned *wl::tl_sync = nullptr;

int wl_ensure_ws(wl_ctx *ctx, size_t bytes, hipStream_t st, bool ordered)
{
    if (bytes <= ctx->ws_bytes) return WL_OK;
    // Grow-only.  The old block may still be in use by kernels queued on the caller's stream.
    //  * ordered (growth inside a transform call, round 4): STREAM-ORDERED -- the old block is released and the new one allocated
    //    in the order of the call's stream (hipFreeAsync / hipMallocAsync), nothing waits on the host, the device is not
    //    synchronised.  A context belongs to one stream (header), so every user of the old block is ahead of the release.
    //  * otherwise (wl_ctx_reserve, which takes no stream): device synchronisation, then the same pool on the null stream,
    //    synchronised before returning so that the block is usable from any stream.
    const size_t want = (bytes + 255) & ~(size_t)255;
    const bool pool = wl::opt("WL_WS_SYNC_ALLOC", 0) == 0;
    void *p = nullptr;
    if (ordered) {
        // A growth while the call's stream is being captured into a hipGraph would record alloc / free nodes and leave the context
        // pointing at graph-owned memory that later eager calls use: refuse (reserve wl_workspace_bytes_full before capturing).
        // A query that itself fails (e.g. hipErrorStreamCaptureImplicit: the legacy stream while another stream captures) is treated as
        // "capturing", and its error is cleared so that a later launch's hipGetLastError() cannot report it.
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const hipError_t qe = hipStreamIsCapturing(st, &cs);
        if (qe != hipSuccess) (void)hipGetLastError();
        if (qe != hipSuccess || cs != hipStreamCaptureStatusNone) { ctx->last_hip = (int)hipErrorStreamCaptureUnsupported; return WL_EHIP; }
    } else {
        // wl_ctx_reserve (no stream argument): it synchronises the device, which is illegal while ANY stream of this thread's capture
        // mode is capturing -- refuse before touching anything (the legacy-stream query reports an ongoing capture as an error)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const hipError_t qe = hipStreamIsCapturing(nullptr, &cs);
        if (qe != hipSuccess) (void)hipGetLastError();
        if (qe != hipSuccess || cs != hipStreamCaptureStatusNone) { ctx->last_hip = (int)hipErrorStreamCaptureUnsupported; return WL_EHIP; }
    }
    if (ordered && pool && (ctx->ws == nullptr || ctx->ws_pooled)) {
        if (ctx->ws) { WL_HIP(ctx, hipFreeAsync(ctx->ws, st)); ctx->ws = nullptr; ctx->ws_bytes = 0; }
        hipError_t e = hipMallocAsync(&p, want, st);
        if (e == hipSuccess) {
            ctx->ws = p; ctx->ws_bytes = want; ctx->ws_pooled = true;
            return WL_OK;
        }
        // The released block cannot be reused by the pool before the stream reaches the release, so old + new had to fit.  Fall
        // through to the synchronising path (device sync, pool trimmed, retry) before reporting WL_ENOMEM.
        (void)hipGetLastError();
        hipMemPool_t mp = nullptr;
        int dev = 0;
        if (hipDeviceSynchronize() == hipSuccess && hipGetDevice(&dev) == hipSuccess && hipDeviceGetDefaultMemPool(&mp, dev) == hipSuccess && mp)
            (void)hipMemPoolTrimTo(mp, 0);
        (void)hipGetLastError();
    }
    WL_HIP(ctx, hipDeviceSynchronize());
    if (ctx->ws) {
        if (ctx->ws_pooled) { WL_HIP(ctx, hipFreeAsync(ctx->ws, nullptr)); WL_HIP(ctx, hipStreamSynchronize(nullptr)); }
        else WL_HIP(ctx, hipFree(ctx->ws));
        ctx->ws = nullptr; ctx->ws_bytes = 0;
    }
    hipError_t e;
    if (pool) {
        e = hipMallocAsync(&p, want, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    } else {
        e = hipMalloc(&p, want);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); ctx->last_hip = (int)e; return WL_ENOMEM; }
    ctx->ws = p;
    ctx->ws_bytes = want;
    ctx->ws_pooled = pool;
    return WL_OK;
}

int wl_stage_to_device(wl_ctx *ctx, void *dst, const void *host, size_t bytes, hipStream_t st)
{
    const int k = ctx->stage_next;
    ctx->stage_next = (k + 1) % wl_ctx::kStage;
    if (ctx->stage_ev[k]) WL_HIP(ctx, hipEventSynchronize(ctx->stage_ev[k]));      // the copy that last used this slot
    else WL_HIP(ctx, hipEventCreateWithFlags(&ctx->stage_ev[k], hipEventDisableTiming));
    if (ctx->stage_bytes[k] < bytes) {
        if (ctx->stage[k]) { WL_HIP(ctx, hipHostFree(ctx->stage[k])); ctx->stage[k] = nullptr; ctx->stage_bytes[k] = 0; }
        const size_t want = (bytes + 4095) & ~(size_t)4095;
        if (hipHostMalloc(&ctx->stage[k], want, hipHostMallocDefault) != hipSuccess) { ctx->stage[k] = nullptr; return WL_ENOMEM; }
        ctx->stage_bytes[k] = want;
    }
    std::memcpy(ctx->stage[k], host, bytes);
    WL_HIP(ctx, hipMemcpyAsync(dst, ctx->stage[k], bytes, hipMemcpyHostToDevice, st));
    WL_HIP(ctx, hipEventRecord(ctx->stage_ev[k], st));
    return WL_OK;
}

namespace {

inline bool sufficientpoweroftwo(int64_t n, int L) { return L < 62 && (n % ((int64_t)1 << L)) == 0; }

inline int ensure_ws(wl_ctx *ctx, size_t bytes) { return wl_ensure_ws(ctx, bytes); }
inline int ensure_ws(wl_ctx *ctx, size_t bytes, hipStream_t st) { return wl_ensure_ws(ctx, bytes, st, true); }

// ---- generic lifting level loops -----------------------------------------------------------
template <typename T>
int generic_lifting_fwd(wl_ctx *ctx, hipStream_t st, const BoxSpec &b, T *y, const T *x,
                        const LiftScheme<T> &sc, int L)
{
    int64_t N = b.dims[0] * b.dims[1] * b.dims[2];
    Work<T> w = carve<T>(ctx->ws, N);
    const T *cur = x;
    Strides3 cur_st = b.full;
    int pp = 0;
    for (int l = 1; l <= L; ++l) {
        int64_t n[3];
        level_box(b, l, n);
        Extent3 ext = {{n[0], n[1], n[2]}};
        Extent3 lo = low_corner(b, n);
        const bool last = (l == L);
        T *llbuf = pp ? w.B : w.A;
        int64_t hn[3] = {lo.n[0], lo.n[1], lo.n[2]};
        Strides3 ll_st = dense_strides(hn);
        Strides3 box_st = dense_strides(n);
        const T *in = cur;
        Strides3 in_st = cur_st;
        int tog = 0;
        for (int a = b.nt - 1; a >= 0; --a) {
            // known scheme shapes: the whole pass (split, steps, normalize) in one launch (k_lift_any, wl_lift.hip) unless the
            // pass would read and write the same array (in-place 1-D level 1)
            {
                T *out = (a != 0) ? (tog ? w.T1 : w.T0) : y;
                hipError_t ea = hipSuccess;
                if (ctx->path == 0 && (const T *)out != in &&
                    lift_any_pass<T>(st, sc, 1, in, in_st, out, a != 0 ? box_st : b.full, (a != 0 || last) ? (T *)nullptr : llbuf, ll_st, ext, a,
                                     lo, &ea)) {
                    WL_HIP(ctx, ea);
                    ctx->last_kernel = "k_lift_any";
                    if (a != 0) { in = out; in_st = box_st; tog ^= 1; }
                    continue;
                }
            }
            WL_HIP(ctx, generic_lift_split<T>(st, in, in_st, w.W, box_st, ext, a));
            for (int s = 0; s < sc.nsteps; ++s)
                WL_HIP(ctx, generic_lift_step<T>(st, sc.step[s], w.W, box_st, ext, a));
            if (a != 0) {
                T *out = tog ? w.T1 : w.T0;
                WL_HIP(ctx, generic_lift_finish_fwd<T>(st, sc.norm1, sc.norm2, w.W, box_st, out, box_st,
                                                       (T *)nullptr, box_st, ext, a, lo));
                in = out; in_st = box_st; tog ^= 1;
            } else {
                WL_HIP(ctx, generic_lift_finish_fwd<T>(st, sc.norm1, sc.norm2, w.W, box_st, y, b.full,
                                                       last ? (T *)nullptr : llbuf, ll_st, ext, a, lo));
            }
        }
        cur = llbuf; cur_st = ll_st; pp ^= 1;
    }
    return WL_OK;
}

template <typename T>
int generic_lifting_inv(wl_ctx *ctx, hipStream_t st, const BoxSpec &b, T *y, const T *x,
                        const LiftScheme<T> &sc, int L)
{
    int64_t N = b.dims[0] * b.dims[1] * b.dims[2];
    Work<T> w = carve<T>(ctx->ws, N);
    int pp = 0;
    const T *llsrc = nullptr;
    Strides3 llsrc_st = {{0, 0, 0}};
    for (int l = L; l >= 1; --l) {
        int64_t n[3];
        level_box(b, l, n);
        Extent3 ext = {{n[0], n[1], n[2]}};
        Extent3 lo = low_corner(b, n);
        Strides3 box_st = dense_strides(n);
        const T *in = x;
        Strides3 in_st = b.full;
        int tog = 0;
        T *res = nullptr;
        for (int a = 0; a < b.nt; ++a) {
            const bool firstp = (a == 0), lastp = (a == b.nt - 1);
            T *out; Strides3 out_st;
            if (lastp) {
                if (l == 1) { out = y; out_st = b.full; }
                else { out = pp ? w.B : w.A; out_st = box_st; }
                res = out;
            } else { out = tog ? w.T1 : w.T0; out_st = box_st; tog ^= 1; }
            hipError_t ea = hipSuccess;
            if (ctx->path == 0 && (const T *)out != in &&
                lift_any_pass<T>(st, sc, 0, in, in_st, out, out_st, firstp ? const_cast<T *>(llsrc) : (T *)nullptr, llsrc_st, ext, a, lo, &ea)) {
                WL_HIP(ctx, ea);                         // normalize, steps and merge of the pass in one launch (k_lift_any)
                ctx->last_kernel = "k_lift_any";
            } else {
                WL_HIP(ctx, generic_lift_norm_inv<T>(st, sc.norm1, sc.norm2, in, in_st,
                                                     firstp ? llsrc : (const T *)nullptr, llsrc_st, w.W, box_st, ext, a, lo));
                for (int s = 0; s < sc.nsteps; ++s)
                    WL_HIP(ctx, generic_lift_step<T>(st, sc.step[s], w.W, box_st, ext, a));
                WL_HIP(ctx, generic_lift_merge<T>(st, w.W, box_st, out, out_st, ext, a));
            }
            in = out; in_st = out_st;
        }
        llsrc = res; llsrc_st = box_st; pp ^= 1;
    }
    return WL_OK;
}

// ---- argument contract (transforms_filter.jl:24-38, transforms_lifting.jl:33-43,131-143) ----
int check_box(int ndims, const int64_t *dims, int L, BoxSpec &b)
{
    if (!dims) return WL_EINVAL_ARG;
    if (ndims < 1 || ndims > 3) return WL_EDIMS;
    b.nd = ndims; b.nt = ndims;
    for (int d = 0; d < 3; ++d) b.dims[d] = (d < ndims) ? dims[d] : 1;
    for (int d = 0; d < ndims; ++d)
        if (b.dims[d] < 1) return WL_EDIMS;
    if (L < 0) return WL_EINVAL_L;
    for (int d = 0; d < ndims; ++d)
        if (!sufficientpoweroftwo(b.dims[d], L)) return WL_EINVAL_SIZE;
    b.full = dense_strides(b.dims);
    return WL_OK;
}

template <typename T>
int dwt_filter_impl(wl_ctx *ctx, hipStream_t st, const BoxSpec &b, T *y, const T *x,
                    const double *qmf, int flen, int L, int fw)
{
    const int64_t N = b.dims[0] * b.dims[1] * b.dims[2];
    if (L == 0) {
        Extent3 ext = {{b.dims[0], b.dims[1], b.dims[2]}};
        WL_HIP(ctx, generic_copy_box<T>(st, x, b.full, y, b.full, ext));
        ctx->last_kernel = "copy";
        return WL_OK;
    }
    // The fast paths need the approximation ping-pong only (2 * (N >> nt) elements); the generic / long-filter / 3-D families
    // also want three N-element buffers.  Start with whichever the context already holds (at least the ping-pong); a level
    // that finds the big buffers missing reports WL_RETRY_GEN, the workspace grows once, and the call is repeated -- x is
    // never modified by a filter transform, so repeating is harmless.
    const size_t ab_bytes = ws_ab_elems(N, b.nt) * sizeof(T), full_bytes = ws_elems(N, b.nt) * sizeof(T);
    const bool want_gen = (ctx->path != 0) || (b.nd == 3) || (flen % 2 != 0) || (flen > 10 && b.nt > 1);
    int rc = ensure_ws(ctx, want_gen ? full_bytes : ab_bytes, st);
    if (rc) return rc;
    const Taps<T> taps = taps_of<T>(qmf, flen);
    for (int attempt = 0; attempt < 2; ++attempt) {
        const bool have_gen = ctx->ws_bytes >= full_bytes;
        rc = fw ? filter_fwd_levels<T>(ctx->ws, have_gen, ctx->cu_count, ctx->path, st, b, y, x, taps, L, &ctx->last_kernel, &ctx->last_hip)
                : filter_inv_levels<T>(ctx->ws, have_gen, ctx->cu_count, ctx->path, st, b, y, x, taps, L, &ctx->last_kernel, &ctx->last_hip);
        if (rc != WL_RETRY_GEN) return rc;
        rc = ensure_ws(ctx, full_bytes, st);
        if (rc) return rc;
    }
    return WL_EINVAL_ARG;
}

template <typename T>
int dwt_lifting_impl(wl_ctx *ctx, hipStream_t st, const BoxSpec &b, T *y, const T *x,
                     const SchemeArgs &s, int L, int fw)
{
    WL_TRY(s.check());
    return wl_lifting_box<T>(ctx, st, b, y, x, s.build<T>(fw), L, fw);
}

// nunits dense units of N elements, unit i at element offset i * stride of x and of y: one copy of an N x nunits matrix with leading
// dimension stride per 65535 units (the padding is not touched)
template <typename T>
int copy_units(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int64_t N, int64_t nunits, int64_t stride)
{
    const Strides3 s = {{1, stride, 0}};
    ctx->last_kernel = "copy";
    return for_groups(nunits, 65535, [&](int64_t i0, int64_t nu) -> int {
        const Extent3 ext = {{N, nu, 1}};
        WL_HIP(ctx, generic_copy_box<T>(st, x + i0 * stride, s, y + i0 * stride, s, ext));
        return WL_OK;
    });
}

// a batch of square images: the box of wl_dwt_filter_batch (third extent = images), images in groups of at most 65535
template <typename T>
int lifting_batch_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int64_t n, int64_t nimages, int64_t image_stride,
                       const LiftScheme<T> &sc, int L, int fw)
{
    BoxSpec b;
    b.nd = 3; b.nt = 2;
    b.dims[0] = n; b.dims[1] = n;
    b.full.s[0] = 1; b.full.s[1] = n; b.full.s[2] = image_stride;
    // images in groups of at most 65535 (one grid plane / workgroup per image in the batched kernels)
    return for_groups(nimages, 65535, [&](int64_t i0, int64_t ni) {
        b.dims[2] = ni;
        return wl_lifting_box<T>(ctx, st, b, y + i0 * image_stride, x + i0 * image_stride, sc, L, fw);
    });
}

// a batch of volumes (wl_dwt_filter_batch3): volumes in groups of at most 65535, the level loops of wl_batch3d.hip
template <typename T>
int dwt_filter_batch3_impl(wl_ctx *ctx, hipStream_t st, const int64_t dims[3], int64_t nvol, int64_t vs, T *y, const T *x, const double *qmf,
                           int flen, int L, int fw)
{
    const int64_t N = dims[0] * dims[1] * dims[2];
    if (L == 0) return copy_units<T>(ctx, st, y, x, N, nvol, vs);              // (every volume is dense)
    const Taps<T> taps = taps_of<T>(qmf, flen);
    const int64_t gmax = nvol < 65535 ? nvol : 65535;
    // 3-D levels outside the tail want one volume's T0 / T1 (as dwt_filter_impl does for a 3-D box): ask for them up front
    const size_t full_bytes = ws_vols_elems(N, gmax) * sizeof(T);
    int rc = ensure_ws(ctx, full_bytes, st);
    if (rc) return rc;
    return for_groups(nvol, 65535, [&](int64_t i0, int64_t nv) {
        rc = fw ? filter_fwd_levels_vols<T>(ctx->ws, true, ctx->cu_count, ctx->path, st, dims, nv, vs, vs, y + i0 * vs, x + i0 * vs, taps, L,
                                            &ctx->last_kernel, &ctx->last_hip)
                : filter_inv_levels_vols<T>(ctx->ws, true, ctx->cu_count, ctx->path, st, dims, nv, vs, vs, y + i0 * vs, x + i0 * vs, taps, L,
                                            &ctx->last_kernel, &ctx->last_hip);
        return rc == WL_RETRY_GEN ? WL_EINVAL_ARG : rc;        // (the full workspace is held: no level can ask for more)
    });
}

}  // namespace

// the lifting transform of a box with a direction-adjusted scheme (shared with wl_ext.hip: the translation-invariant denoise)
template <typename T>
int wl_lifting_box(wl_ctx *ctx, hipStream_t st, const BoxSpec &b, T *y, const T *x, const LiftScheme<T> &sc, int L, int fw)
{
    const int64_t N = b.dims[0] * b.dims[1] * b.dims[2];
    int rc = WL_OK;
    if (L == 0) {
        if (y != x) {
            Extent3 ext = {{b.dims[0], b.dims[1], b.dims[2]}};
            WL_HIP(ctx, generic_copy_box<T>(st, x, b.full, y, b.full, ext));
        }
        ctx->last_kernel = "copy";
        return WL_OK;
    }
    rc = ensure_ws(ctx, ws_elems(N) * sizeof(T), st);
    if (rc) return rc;
    if (ctx->path == 0 && b.nt == 1 && b.full.s[0] == 1) {
        int handled = 0;
        rc = lifting_lines_fast<T>(ctx->ws, ctx->cu_count, st, b.dims[0], b.nd == 1 ? 1 : b.dims[1], b.full.s[1],
                                   y, x, sc, L, fw, &handled, &ctx->last_kernel, &ctx->last_hip);
        if (rc) return rc;
        if (handled) return WL_OK;
    }
    if (ctx->path == 0 && b.nd == 2 && b.nt == 2 && b.full.s[0] == 1) {
        int handled = 0;
        rc = lifting_2d_fast<T>(ctx->ws, ctx->cu_count, st, b.dims[0], b.full.s[1], y, x, sc, L, fw, &handled,
                                &ctx->last_kernel, &ctx->last_hip);
        if (rc) return rc;
        if (handled) return WL_OK;
    }
    // a batch of square images (third extent = images, any image stride): every level one launch over all of them
    if (ctx->path == 0 && b.nd == 3 && b.nt == 2 && b.full.s[0] == 1 && b.dims[0] == b.dims[1] && b.dims[2] <= 65535) {
        int handled = 0;
        rc = lifting_2d_fast<T>(ctx->ws, ctx->cu_count, st, b.dims[0], b.full.s[1], y, x, sc, L, fw, &handled,
                                &ctx->last_kernel, &ctx->last_hip, b.dims[2], b.full.s[2]);
        if (rc) return rc;
        if (handled) return WL_OK;
    }
    if (ctx->path == 0 && b.nd == 3 && b.nt == 3 && b.full.s[0] == 1 && b.dims[0] == b.dims[1] && b.dims[1] == b.dims[2] &&
        b.full.s[1] == b.dims[0] && b.full.s[2] == b.dims[0] * b.dims[1]) {
        int handled = 0;
        rc = lifting_3d_fast<T>(ctx->ws, ctx->cu_count, st, b.dims[0], y, x, sc, L, fw, &handled, &ctx->last_kernel, &ctx->last_hip);
        if (rc) return rc;
        if (handled) return WL_OK;
    }
    ctx->last_kernel = fw ? "k_generic_lift_fwd" : "k_generic_lift_inv";
    return fw ? generic_lifting_fwd<T>(ctx, st, b, y, x, sc, L) : generic_lifting_inv<T>(ctx, st, b, y, x, sc, L);
}
template int wl_lifting_box<float>(wl_ctx *, hipStream_t, const BoxSpec &, float *, const float *, const LiftScheme<float> &, int, int);
template int wl_lifting_box<double>(wl_ctx *, hipStream_t, const BoxSpec &, double *, const double *, const LiftScheme<double> &, int, int);

// the lifting transform of a batch of cubes of side n, cube i at element offset i * vs of x and of y (wl_dwt_lifting_batch3; the spins
// of a cube in wl_ext.hip): groups of at most 65535 cubes through the batched level loop of lifting_3d_fast where it is eligible,
// else (option WL_LIFT_BATCH3_LOOP, path 1, one cube, and whatever lifting_3d_fast declines) cube after cube through wl_lifting_box
template <typename T>
int wl_lifting_vols(wl_ctx *ctx, hipStream_t st, int64_t n, int64_t nvol, int64_t vs, T *y, const T *x, const LiftScheme<T> &sc, int L, int fw)
{
    const int64_t N = n * n * n;
    if (L == 0) return copy_units<T>(ctx, st, y, x, N, y != x ? nvol : 0, vs);  // (every cube is dense; in place: nothing to copy)
    const int64_t gmax = nvol < 65535 ? nvol : 65535;
    // (every group starts a multiple of vs from x: one answer for all of them; the last, shorter group needs no more than the first)
    const int64_t need = (opt("WL_LIFT_BATCH3_LOOP", 0) != 0 || ctx->path != 0 || nvol == 1) ? -1 : lifting_3d_fast_ws<T>(sc, n, L, fw, x, y, gmax, vs, vs);
    if (need >= 0) {
        int rc = ensure_ws(ctx, (size_t)need * sizeof(T), st);
        if (rc) return rc;
        WL_TRY(for_groups(nvol, 65535, [&](int64_t i0, int64_t nv) {
            int handled = 0;
            rc = lifting_3d_fast<T>(ctx->ws, ctx->cu_count, st, n, y + i0 * vs, x + i0 * vs, sc, L, fw, &handled, &ctx->last_kernel, &ctx->last_hip,
                                    nv, vs, vs);
            return (rc || handled) ? rc : WL_EINVAL_ARG;       // (lifting_3d_fast_ws said eligible: not reached)
        }));
        ctx->last_kernel = "k_lift_axis_stream+k_lift_short_lines_batch";      // (whatever the size of the last group)
        return WL_OK;
    }
    BoxSpec b;
    b.nd = 3; b.nt = 3;
    b.dims[0] = b.dims[1] = b.dims[2] = n;
    b.full = dense_strides(b.dims);
    for (int64_t i = 0; i < nvol; ++i) {
        int rc = wl_lifting_box<T>(ctx, st, b, y + i * vs, x + i * vs, sc, L, fw);
        if (rc) return rc;
    }
    return WL_OK;
}
template int wl_lifting_vols<float>(wl_ctx *, hipStream_t, int64_t, int64_t, int64_t, float *, const float *, const LiftScheme<float> &, int, int);
template int wl_lifting_vols<double>(wl_ctx *, hipStream_t, int64_t, int64_t, int64_t, double *, const double *, const LiftScheme<double> &, int, int);

// ==========================================================================================
extern "C" {

int wl_version(void) { return WL_VERSION; }

const char *wl_strerror(int status)
{
    switch (status) {
    case WL_OK: return "ok";
    case WL_EINVAL_SIZE: return "size must have a sufficient power of 2 factor";
    case WL_EINVAL_L: return "L must be positive";
    case WL_EALIAS: return "in array is out array";
    case WL_EDIMS: return "in and out array size must match / bad dimensions";
    case WL_EINVAL_CUBE: return "array must be square/cube";
    case WL_EINVAL_TREE: return "invalid tree";
    case WL_EINVAL_SCHEME: return "invalid lifting scheme";
    case WL_EINVAL_DTYPE: return "unsupported element type";
    case WL_EINVAL_FILTER: return "unsupported filter length";
    case WL_EINVAL_ARG: return "invalid argument";
    case WL_ENOMEM: return "device workspace allocation failed";
    case WL_EHIP: return "HIP runtime error";
    case WL_ENODEVICE: return "no gfx950 HIP device";
    default: return "unknown status";
    }
}

int wl_maxtransformlevels(int64_t n)
{
    if (n <= 1) return 0;
    int tl = 0;
    while (sufficientpoweroftwo(n, tl)) tl += 1;
    return tl - 1;
}

int wl_ctx_create(int device, wl_ctx **out)
{
    if (!out) return WL_EINVAL_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return WL_ENODEVICE;
    if (device < 0 || device >= count) return WL_ENODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return WL_ENODEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return WL_ENODEVICE;
    wl_ctx *c = new (std::nothrow) wl_ctx();
    if (!c) return WL_ENOMEM;
    c->device = device;
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        // the hand-over block of the launches whose workgroups signal one another: zeroed once here, left zero by every launch
        int prev = -1;
        (void)hipGetDevice(&prev);
        hipError_t e = (prev == device) ? hipSuccess : hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc(&c->sync, wl::kSyncWords * sizeof(unsigned));
        if (e == hipSuccess) e = hipMemset(c->sync, 0, wl::kSyncWords * sizeof(unsigned));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
        if (e != hipSuccess) {
            if (c->sync) (void)hipFree(c->sync);
            delete c;
            (void)hipGetLastError();
            return WL_ENOMEM;
        }
    }
    *out = c;
    return WL_OK;
}

int wl_ctx_destroy(wl_ctx *ctx)
{
    if (!ctx) return WL_EINVAL_ARG;
    {
        CallScope scope(ctx);                  // free on the context's device, leave the caller's device current
        (void)hipDeviceSynchronize();
        if (ctx->ws) { if (ctx->ws_pooled) { (void)hipFreeAsync(ctx->ws, nullptr); (void)hipStreamSynchronize(nullptr); } else (void)hipFree(ctx->ws); }
        if (ctx->aux) (void)hipFree(ctx->aux);
        if (ctx->sync) (void)hipFree(ctx->sync);
        for (int k = 0; k < wl_ctx::kStage; ++k) {
            if (ctx->stage_ev[k]) (void)hipEventDestroy(ctx->stage_ev[k]);
            if (ctx->stage[k]) (void)hipHostFree(ctx->stage[k]);
        }
    }
    delete ctx;
    return WL_OK;
}

int wl_shard_range(int64_t nunits, int rank, int world, int64_t *lo, int64_t *hi)
{
    if (!lo || !hi || nunits < 0 || world < 1 || rank < 0 || rank >= world) return WL_EINVAL_ARG;
    const int64_t base = nunits / world, rem = nunits % world;
    *lo = rank * base + (rank < rem ? rank : rem);
    *hi = *lo + base + (rank < rem ? 1 : 0);
    return WL_OK;
}

size_t wl_workspace_bytes(int dtype, int ndims, const int64_t *dims, int L)
{
    (void)L;
    if (!dims || ndims < 1 || ndims > 3) return 0;
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    // what the fast filter-bank paths of dwt / idwt on this box use: the approximation ping-pong, 2 * (N / 2^ndims) elements.
    // (dwtc: pass ndims = 1 with dims[0] = len * nsignals.)  Lifting, long / odd filters, 3-D boxes and the generic
    // family use up to 4 N elements more; the context grows to that on their first call.
    return ws_ab_elems(N, ndims) * (dtype == WL_F64 ? 8 : 4);
}
size_t wl_workspace_bytes_full(int dtype, int ndims, const int64_t *dims, int L)
{
    (void)L;
    if (!dims || ndims < 1 || ndims > 3) return 0;
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    // ping-pong + T0 / T1 / W of the general families (ws_elems); the packet transforms add a depth table of N bytes
    return ws_elems(N, 1) * (dtype == WL_F64 ? 8 : 4) + (size_t)N + 256;
}
size_t wl_ctx_workspace_held(const wl_ctx *ctx) { return ctx ? ctx->ws_bytes : 0; }

int wl_ctx_reserve(wl_ctx *ctx, size_t bytes)
{
    if (!ctx) return WL_EINVAL_ARG;
    WL_SCOPE(ctx);
    return ensure_ws(ctx, bytes);
}

int wl_stream_sync(wl_ctx *ctx, void *stream)
{
    if (!ctx) return WL_EINVAL_ARG;
    WL_SCOPE(ctx);
    WL_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    return WL_OK;
}

int wl_last_hip_error(const wl_ctx *ctx) { return ctx ? ctx->last_hip : 0; }
int wl_ctx_set_path(wl_ctx *ctx, int path)
{
    if (!ctx || path < 0 || path > 1) return WL_EINVAL_ARG;
    ctx->path = path;
    return WL_OK;
}
const char *wl_last_kernel(const wl_ctx *ctx) { return ctx ? ctx->last_kernel : "none"; }

int wl_ctx_set_option(wl_ctx *ctx, const char *key, int64_t value)
{
    if (!ctx || !key || !*key || strlen(key) >= (size_t)Opts::kKeyLen) return WL_EINVAL_ARG;
    Opts &o = ctx->opts;
    for (int i = 0; i < o.n; ++i)
        if (strcmp(o.key[i], key) == 0) { o.val[i] = (long long)value; return WL_OK; }
    if (o.n >= Opts::kMax) return WL_EINVAL_ARG;
    strcpy(o.key[o.n], key);
    o.val[o.n] = (long long)value;
    ++o.n;
    return WL_OK;
}
int wl_ctx_clear_options(wl_ctx *ctx)
{
    if (!ctx) return WL_EINVAL_ARG;
    ctx->opts.n = 0;
    return WL_OK;
}

int wl_dwt_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                  const double *qmf, int flen, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    BoxSpec b;
    WL_TRY(check_box(ndims, dims, L, b));
    if (y == x) return WL_EALIAS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return dwt_filter_impl<T>(ctx, st, b, (T *)y, (const T *)x, qmf, flen, L, fw);
    });
}

// the lifting entry points on a box: the scope, then the scheme's rules, then the transform
static int lifting_scoped(wl_ctx *ctx, int dtype, const BoxSpec &b, void *y, const void *x, const SchemeArgs &s, int L, int fw, void *stream)
{
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return dwt_lifting_impl<T>(ctx, st, b, (T *)y, (const T *)x, s, L, fw);
    });
}

static int lifting_common(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, const SchemeArgs &s, int L, int fw,
                          void *stream)
{
    if (!ctx || !y || !x) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    BoxSpec b;
    // iscube check comes first in the reference (transforms_lifting.jl:131-136)
    if (dims && ndims >= 2 && ndims <= 3)
        for (int d = 1; d < ndims; ++d)
            if (dims[d] != dims[0]) return WL_EINVAL_CUBE;
    WL_TRY(check_box(ndims, dims, L, b));
    return lifting_scoped(ctx, dtype, b, y, x, s, L, fw, stream);
}

int wl_dwt_lifting(wl_ctx *ctx, int dtype, void *y, int ndims, const int64_t *dims,
                   int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                   const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2,
                   int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    return lifting_common(ctx, dtype, y, y, ndims, dims, s, L, fw, stream);
}

int wl_dwt_lifting_oop(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                       int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                       const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2,
                       int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    return lifting_common(ctx, dtype, y, x, ndims, dims, s, L, fw, stream);
}

// ---- batched column-wise --------------------------------------------------------------------
static int check_dwtc(int64_t len, int64_t nsignals, int64_t ld, int L, BoxSpec &b)
{
    if (len < 1 || nsignals < 1 || ld < len) return WL_EDIMS;
    if (L < 0) return WL_EINVAL_L;
    if (!sufficientpoweroftwo(len, L)) return WL_EINVAL_SIZE;
    b.nd = 2; b.nt = 1;
    b.dims[0] = len; b.dims[1] = nsignals; b.dims[2] = 1;
    b.full.s[0] = 1; b.full.s[1] = ld; b.full.s[2] = ld * nsignals;
    return WL_OK;
}

int wl_dwtc_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t len, int64_t nsignals, int64_t ld,
                   const double *qmf, int flen, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    BoxSpec b;
    WL_TRY(check_dwtc(len, nsignals, ld, L, b));
    if (y == x) return WL_EALIAS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return dwt_filter_impl<T>(ctx, st, b, (T *)y, (const T *)x, qmf, flen, L, fw);
    });
}

int wl_dwtc_lifting_oop(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t len, int64_t nsignals, int64_t ld,
                        int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                        const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2,
                        int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || !x) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    BoxSpec b;
    WL_TRY(check_dwtc(len, nsignals, ld, L, b));
    return lifting_scoped(ctx, dtype, b, y, x, s, L, fw, stream);
}

int wl_dwtc_lifting(wl_ctx *ctx, int dtype, void *y, int64_t len, int64_t nsignals, int64_t ld,
                    int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                    const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2,
                    int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    BoxSpec b;
    WL_TRY(check_dwtc(len, nsignals, ld, L, b));
    return lifting_scoped(ctx, dtype, b, y, y, s, L, fw, stream);
}

}  // extern "C"

// ---- wavelet packet transforms (1-D) -------------------------------------------------------------
// The reference walks the tree one depth at a time (transforms_filter.jl:325-356,
// transforms_lifting.jl:297-316): at depth d the vector is 2^d segments of length n/2^d, and
// every segment whose node bit is set gets one [s ; d] level.  Here one depth = one launch over
// the box (n/2^d, 2^d) with the node bits as a per-segment mask (unset segments are copied
// through), ping-ponging between y and a work buffer so that the last launch lands in y.
// index of the last set node (-1: none); the tail of a tree vector is normally one long run of zeros
static int64_t last_set_node(const uint8_t *b, int64_t nb)
{
    int64_t i = nb;
    while (i > 0 && (reinterpret_cast<uintptr_t>(b + i) & 7) != 0) { if (b[i - 1]) return i - 1; --i; }
    while (i >= 64) {                                   // 64 bytes per iteration, independent loads
        uint64_t w[8];
        std::memcpy(w, b + i - 64, 64);
        if ((w[0] | w[1] | w[2] | w[3]) | (w[4] | w[5] | w[6] | w[7])) break;
        i -= 64;
    }
    while (i > 0) { if (b[i - 1]) return i - 1; --i; }
    return -1;
}
// isvalidtree (util_main.jl:301-314): the length matches and no node is set below an unset node.  Equivalent
// statement checked here: every set node other than the root has its parent set -- O(last set node), not O(2^ns).
static bool isvalidtree(int64_t n, const uint8_t *b, int64_t nb, int64_t *last_set)
{
    int ns = wl_maxtransformlevels(n);
    *last_set = -1;
    if (nb != ((int64_t)1 << ns) - 1) return false;
    if (ns == 0) return true;
    const int64_t hi = last_set_node(b, nb);
    *last_set = hi;
    for (int64_t j = 1; j <= hi; ++j)
        if (b[j] && !b[(j - 1) >> 1]) return false;
    return true;
}

// the tree rule of the entry points that take either: tree == NULL is the full tree of depth L
static int check_tree_or_depth(int64_t n, const uint8_t *tree, int64_t ntree, int L, int64_t *last_set)
{
    *last_set = -1;
    if (!tree) return (L < 0 || L > wl_maxtransformlevels(n)) ? WL_EINVAL_L : WL_OK;
    return isvalidtree(n, tree, ntree, last_set) ? WL_OK : WL_EINVAL_TREE;
}

// one packet transform of nunits signals of length n (wpt_impl)
template <typename T>
struct WptCall {
    int64_t n = 0;
    const Taps<T> *taps = nullptr;      // a filter bank, or
    const LiftScheme<T> *sc = nullptr;  // a lifting scheme (direction-adjusted)
    const uint8_t *tree = nullptr;      // HOST node bits (isvalidtree), ntree of them, the last set one at last_set
    int64_t ntree = 0;
    int64_t last_set = -1;
    int fw = 1;
    // full_depth >= 0: the full tree of that depth, no tree vector (tree == nullptr); only its depths >= first_depth are applied
    // (x already holds the depth-first_depth content: the best-basis search steps one depth at a time)
    int full_depth = -1;
    int first_depth = 0;
    // nunits > 1 (wl_wpt_*_batch): nunits signals of length n that share the tree, unit u at element offset u * ustride of x, of y and
    // of the work buffers.  The plan is made for ONE unit of length n -- the batch takes the same kernels, every launch over all
    // units, the packet kernels being the very instances the single unit runs -- and lifting may then run out of place (x != y: the
    // first pass reads x, x stays untouched).
    int64_t nunits = 1;
    int64_t ustride = 0;
    // utrees != nullptr (wl_wpt_filter_batch_trees; filter banks only): one DEVICE tree per unit, unit u's node bits at utrees +
    // u * utstride, depths < utL.  Nothing of them is known on the host, so the plan is the partial-tree plan of one unit with every
    // depth < utL present; one launch closes the trees into the workspace (a node counts iff it and every ancestor is set) and the
    // kernels read those bits with a per-unit stride.  Leaves pass through inside the launches.
    const uint8_t *utrees = nullptr;
    int64_t utstride = 0;
    int utL = 0;
};

template <typename T>
static int wpt_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, const WptCall<T> &c)
{
    const int64_t n = c.n, ntree = c.ntree, last_set = c.last_set, nunits = c.nunits, utstride = c.utstride;
    const Taps<T> *taps = c.taps;
    const LiftScheme<T> *sc = c.sc;
    const uint8_t *tree = c.tree, *utrees = c.utrees;
    const int fw = c.fw, first_depth = c.first_depth, utL = c.utL;
    int full_depth = c.full_depth;
    int64_t ustride = c.ustride;
    const bool lifting = (sc != nullptr);
    if (utrees) full_depth = -1;
    if (nunits == 1) ustride = n;
    const bool dense = (ustride == n);
    Extent3 full = {{n, 1, nunits}};
    Strides3 fst = {{1, n, ustride}};
    if (utrees ? utL == 0 : full_depth >= 0 ? full_depth == 0 : (ntree == 0 || !tree[0])) {
        if (y != x) WL_HIP(ctx, generic_copy_box<T>(st, x, fst, y, fst, full));
        ctx->last_kernel = "copy";
        return WL_OK;
    }
    const int Lmax = wl_maxtransformlevels(n);
    // depths in processing order, skipping depths where no node is set (pure copy-through); kind 2: every segment splits
    std::vector<int> depths, kind;
    bool any_partial = false;
    for (int L = Lmax; L > 0; --L) {
        int d = fw ? Lmax - L : L - 1;
        if (utrees) {
            if (d < utL) { depths.push_back(d); kind.push_back(1); any_partial = true; }
            continue;
        }
        if (full_depth >= 0) {
            if (d >= first_depth && d < full_depth) { depths.push_back(d); kind.push_back(2); }
            continue;
        }
        int64_t first = ((int64_t)1 << d) - 1, cnt = (int64_t)1 << d;
        int64_t nset = 0;
        if (first <= last_set)
            for (int64_t k = 0; k < cnt; ++k) nset += tree[first + k] != 0;
        if (nset) { depths.push_back(d); kind.push_back(nset == cnt ? 2 : 1); any_partial = any_partial || nset != cnt; }
    }
    const int K = (int)depths.size();
    // only the nodes up to the last set one are ever looked at on the device (whole depths: round up to 2^(d+1) - 1), and only
    // when some depth is PARTIALLY split: the kernels of fully split depths take no mask.  The bits travel through the
    // context's pinned staging ring -- the caller's (pageable) buffer is not referenced after this call returns and the stream
    // is not synchronised (round 3 did hipStreamSynchronize here, against the header's contract).
    int64_t ncopy = 1;
    while (ncopy - 1 <= last_set && ncopy - 1 < ntree) ncopy <<= 1;
    ncopy = (ncopy - 1 < ntree) ? ncopy - 1 : ntree;
    if (full_depth >= 0) ncopy = 0;
    const int64_t mstride = utrees ? ((int64_t)1 << utL) - 1 : 0;       // closed per-unit trees: the nodes of the depths < utL, dense
    if (utrees) ncopy = nunits * mstride;
    const int64_t NW = nunits * ustride;                // the work buffers mirror the layout of x and y
    int rc = ensure_ws(ctx, ws_elems(NW) * sizeof(T) + (size_t)(any_partial ? ncopy : 0) + 256, st);
    if (rc) return rc;
    Work<T> w = carve<T>(ctx->ws, NW);
    uint8_t *dtree = (uint8_t *)ctx->ws + ws_elems(NW) * sizeof(T);
    if (utrees) {
        WL_HIP(ctx, tree_close(st, utrees, utstride, mstride, dtree, mstride, nunits));
    } else if (any_partial) {
        rc = wl_stage_to_device(ctx, dtree, tree, (size_t)ncopy, st);
        if (rc) return rc;
    }
    // the packet kernels (k_wpt_fwd_multi / _inv_multi / _tail) move 16-byte vectors straight on x, y and the work buffer: a view that
    // starts 4 or 8 bytes off the grid (buf[1:1+n]) takes the per-depth kernels, which gate on alignment themselves
    const bool fast_any = (ctx->path == 0) && opt("WL_WPT_FAST", 1) != 0;          // the lifting line kernels check alignment themselves
    // (a batch: every unit base, that is the stride too -- NW is then a multiple of 16 bytes and so is T0's offset in the workspace)
    const bool fast = fast_any && al16(x) && al16(y) && al16(w.T0) && (nunits == 1 || (ustride * sizeof(T)) % 16 == 0);   // the filter-bank packet kernels

    if (lifting) {
        // wpt!(y, scheme, ...) is in place for the caller.  A fused lifting level cannot run in place (its [s ; d] outputs land
        // where other waves still read interleaved input; lifting_lines_fast would stage and copy back: three launches), so fully
        // split depths ping-pong between y and a work buffer -- one launch per depth -- and an odd count ends with one copy.
        const char *name = "k_generic_lift_wpt";
        const T *cur = x;
        for (int i = 0; i < K; ++i) {
            const int d = depths[i];
            const int64_t nj = n >> d, nseg = (int64_t)1 << d;
            // fully split depth: one lifting level (all steps fused) of nseg lines of length nj (a dense batch: nseg * nunits lines)
            if (kind[i] == 2 && fast_any && dense) {
                int handled = 0, herr = 0;
                const char *kn = nullptr;
                T *out = (cur == y) ? w.T0 : y;
                rc = lifting_lines_fast<T>(ctx->ws, ctx->cu_count, st, nj, nseg * nunits, nj, out, cur, *sc, 1, fw, &handled, &kn, &herr);
                if (rc) { ctx->last_hip = herr; return rc; }
                if (handled) { name = kn ? kn : "k_lift1d_stream"; cur = out; continue; }
            }
            if (cur != y) { WL_HIP(ctx, generic_copy_box<T>(st, cur, fst, y, fst, full)); cur = y; }
            Extent3 ext = {{nj, nseg, nunits}};
            Strides3 bst = {{1, nj, ustride}};
            Extent3 lo = {{nj >> 1, nseg, nunits}};
            const uint8_t *mask = (kind[i] == 2) ? nullptr : dtree + (((int64_t)1 << d) - 1);
            // reads of y all happen in the first kernel, so in place is safe
            if (fw) {
                WL_HIP(ctx, generic_lift_split<T>(st, y, bst, w.W, bst, ext, 0, mask));
                for (int s = 0; s < sc->nsteps; ++s)
                    WL_HIP(ctx, generic_lift_step<T>(st, sc->step[s], w.W, bst, ext, 0, mask));
                WL_HIP(ctx, generic_lift_finish_fwd<T>(st, sc->norm1, sc->norm2, w.W, bst, y, bst, (T *)nullptr, bst, ext, 0, lo, mask));
            } else {
                WL_HIP(ctx, generic_lift_norm_inv<T>(st, sc->norm1, sc->norm2, y, bst, (const T *)nullptr, bst, w.W, bst, ext, 0, lo, mask));
                for (int s = 0; s < sc->nsteps; ++s)
                    WL_HIP(ctx, generic_lift_step<T>(st, sc->step[s], w.W, bst, ext, 0, mask));
                WL_HIP(ctx, generic_lift_merge<T>(st, w.W, bst, y, bst, ext, 0, mask));
            }
        }
        if (cur != y) WL_HIP(ctx, generic_copy_box<T>(st, cur, fst, y, fst, full));
        ctx->last_kernel = name;
        return WL_OK;
    }

    // ---- filter bank: plan the launches first (the output ping-pongs between y and a work buffer and must end in y) ----
    struct Step { int kindk; int d; int nd; };          // 0 generic / line kernel (one depth), 1 / 3 forward / inverse multi (nd fused depths from depth d), 2 tail (nd depths)
    std::vector<Step> plan;
    const int F = taps->F;
    const int TSw = wpt_tile_samples<T>();
    // round 5: the packet kernels take the node bits (per-segment split mask), so partially split depths (a dwt-shaped tree, a best-basis
    // tree) ride the same fused passes -- leaves are passed through inside the launch -- instead of one generic launch per depth
    const uint8_t *pmask = any_partial ? dtree : nullptr;
    for (int i = 0; i < K;) {
        const int d = depths[i];
        int run = 0;                                     // consecutive depths d, d +- 1, ... in processing order (fully or partially split)
        while (fast && i + run < K && depths[i + run] == (fw ? d + run : d - run)) ++run;
        bool run_partial = false;
        for (int k = 0; k < run; ++k) run_partial = run_partial || kind[i + k] != 2;
        if (run >= 1 && fw) {
            const int64_t nj = n >> d;
            if (wpt_tail_ok<T>(F, n, nj, run)) { plan.push_back({2, d, run}); i += run; continue; }
            int to_tail = 0;                             // depths until the segments fit a workgroup
            while ((nj >> to_tail) > TSw) ++to_tail;
            int lim = run < to_tail ? run : to_tail;
            if (lim < 1) lim = 1;
            const int stages = (lim + 2) / 3;
            int NL = (lim + stages - 1) / stages;
            while (NL >= 1 && !wpt_fwd_multi_ok<T>(F, n, nj, NL)) --NL;
            if (NL >= 1 && (NL > 1 || run_partial || opt("WL_WPT_MULTI1", 0))) { plan.push_back({1, d, NL}); i += NL; continue; }
        } else if (run >= 1 && !fw) {
            // deepest first: take every depth of the run whose segments still fit a workgroup
            int nd = 0;
            while (nd < run && wpt_tail_ok<T>(F, n, n >> (d - nd), nd + 1)) ++nd;
            if (nd >= 1) { plan.push_back({2, d - nd + 1, nd}); i += nd; continue; }
            // big segments: up to three depths per pass (k_wpt_inv_multi), the run split evenly over the fewest launches
            const int stages = (run + 2) / 3;
            int NL = (run + stages - 1) / stages;
            const int nlmin = run_partial ? 1 : 2;
            while (NL >= nlmin && !wpt_inv_multi_ok<T>(F, n, n >> (d - NL + 1), NL)) --NL;
            if (NL >= nlmin) { plan.push_back({3, d - NL + 1, NL}); i += NL; continue; }
        }
        plan.push_back({0, d, 1});
        ++i;
    }
    const int P = (int)plan.size();
    const T *cur = x;
    const char *name = "k_generic_filter_wpt";
    for (int i = 0; i < P; ++i) {
        const Step &sp = plan[i];
        const int d = sp.d;
        T *out = ((P - 1 - i) % 2 == 0) ? y : w.T0;
        if (sp.kindk == 1) {
            WL_HIP(ctx, wpt_fwd_multi_launch<T>(st, *taps, cur, out, n, n >> d, sp.nd, pmask, nunits, ustride, mstride));
            name = "k_wpt_fwd_multi";
        } else if (sp.kindk == 3) {
            WL_HIP(ctx, wpt_inv_multi_launch<T>(st, *taps, cur, out, n, n >> d, sp.nd, pmask, nunits, ustride, mstride));
            name = "k_wpt_inv_multi";
        } else if (sp.kindk == 2) {
            WL_HIP(ctx, wpt_tail_launch<T>(st, *taps, fw, cur, out, n, n >> d, sp.nd, pmask, nunits, ustride, mstride));
            if (std::strncmp(name, "k_wpt", 5) != 0) name = fw ? "k_wpt_fwd_tail" : "k_wpt_inv_tail";
        } else {
            const int64_t nj = n >> d, nseg = (int64_t)1 << d;
            Extent3 ext = {{nj, nseg, nunits}};
            Strides3 bst = {{1, nj, ustride}};
            Extent3 lo = {{nj >> 1, nseg, nunits}};
            int ki = 0;
            while (depths[ki] != d) ++ki;
            const bool all_set = kind[ki] == 2;
            bool done = false;
            if (all_set && ctx->path == 0 && dense) {    // fully split depth: every segment (of every unit of a dense batch) is a line of the streaming kernels
                hipError_t he = hipSuccess;
                done = fw ? fast_lines_fwd_level<T>(st, *taps, cur, nj, out, nj, out + (nj >> 1), nj, nj, nseg * nunits, ctx->cu_count, &he)
                          : fast_lines_inv_level<T>(st, *taps, cur, nj, cur + (nj >> 1), nj, out, nj, nj, nseg * nunits, ctx->cu_count, &he);
                if (he != hipSuccess) return hip_fail(ctx, he);
                if (done && std::strncmp(name, "k_wpt", 5) != 0) name = fw ? "k_fwd1d_stream" : "k_inv1d_stream";
            }
            if (!done) {
                const uint8_t *mask = all_set ? nullptr : dtree + (((int64_t)1 << d) - 1);
                if (fw)
                    WL_HIP(ctx, generic_fwd_filter_pass<T>(st, *taps, cur, bst, out, bst, (T *)nullptr, bst, ext, 0, lo, mask, mstride));
                else
                    WL_HIP(ctx, generic_inv_filter_pass<T>(st, *taps, cur, bst, (const T *)nullptr, bst, out, bst, ext, 0, lo, mask, mstride));
            }
        }
        cur = out;
    }
    ctx->last_kernel = name;
    return WL_OK;
}

// ---- best-basis search (bestbasistree, entropy.jl:47-111) -----------------------------------------------------------------------
// The reference decomposes the signal to the full depth Lmax one dwt! level per node and takes each node's entropy before its split.
// Here depth d + 1 comes from depth d by one full-depth packet step (wpt_impl, first_depth = d: the packet kernels, bit-identical to
// wpt), ping-ponging between two buffers, and every depth is reduced to its node entropies by the segmented kernel (wl_entropy.hip);
// depth Lmax is reduced over the pairs of siblings only (entr_af).  The decision runs on the device.
//
// A group of G units (wl_bestbasistree_filter_batch; the single search is the group of one): every launch
// above goes over all units of the group -- unit u at x + u * S -- and the trees are written to device memory, unit u's at
// tree_out + u * tstride.  The packet buffers are DENSE (unit u at u * n): a padded batch (S > n) is copied into one first, so that
// every depth runs the plan of a dense batch -- the kernels the single search runs, which is what makes batch = loop hold in the
// fused library too (a padded batch would take the per-depth kernels where a single unit takes the streaming line kernels).
// Workspace layout of a group (bytes, every part rounded up to 256):
//   [wpt_impl's region of G n elements + 256 | A, B: G n elements each | entropies G (ntree + naf) doubles, unless the caller's |
//    best G ntree doubles | partials G (n / 1024 + 64) doubles | norms G doubles | split G ntree bytes | tree ntree | out ntree]
// (tree: the staged input tree, when there is one; out: the single search's result before its one copy to the host)
struct BBLayout { size_t oA, oB, oE, oBest, oP, oN, oS, oT, oO, total; };
static BBLayout bb_layout(int64_t n, int64_t G, size_t es, bool own_ent)
{
    const int Lmax = wl_maxtransformlevels(n);
    const int64_t ntree = ((int64_t)1 << Lmax) - 1, naf = (int64_t)1 << (Lmax - 1);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const int64_t NW = G * n;
    BBLayout l;
    size_t off = up(ws_elems(NW) * es + 256);
    l.oA = off; off += up((size_t)NW * es);
    l.oB = off; off += up((size_t)NW * es);
    l.oE = off; off += own_ent ? up((size_t)G * (size_t)(ntree + naf) * sizeof(double)) : 0;
    l.oBest = off; off += up((size_t)G * (size_t)ntree * sizeof(double));
    l.oP = off; off += up((size_t)G * entropy_partials(n) * sizeof(double));
    l.oN = off; off += up((size_t)G * sizeof(double));
    l.oS = off; off += up((size_t)G * (size_t)ntree);
    l.oT = off; off += up((size_t)ntree);
    l.oO = off; off += up((size_t)ntree);
    l.total = off;
    return l;
}

// tree: the HOST input tree (staged here) or nullptr for the full tree of depth Lfull.  tree_out: DEVICE, or nullptr for the `out`
// part of the workspace (the single search copies it to the host itself).
template <typename T>
static int bestbasis_group(wl_ctx *ctx, hipStream_t st, const T *x, int64_t n, int64_t G, int64_t S, const Taps<T> &taps, const uint8_t *tree,
                           int Lfull, int et, uint8_t *tree_out, int64_t tstride, double *node_entropy, int64_t estride, uint8_t **ws_out)
{
    const int Lmax = wl_maxtransformlevels(n);
    const int64_t ntree = ((int64_t)1 << Lmax) - 1, naf = (int64_t)1 << (Lmax - 1);
    if (G == 1) S = n;
    const BBLayout l = bb_layout(n, G, sizeof(T), node_entropy == nullptr);
    int rc = ensure_ws(ctx, l.total, st);
    if (rc) return rc;
    char *ws = (char *)ctx->ws;
    T *A = (T *)(ws + l.oA), *B = (T *)(ws + l.oB);
    double *ent = node_entropy ? node_entropy : (double *)(ws + l.oE);
    const int64_t uent = node_entropy ? estride : ntree + naf;
    double *best = (double *)(ws + l.oBest), *part = (double *)(ws + l.oP), *nrm = (double *)(ws + l.oN);
    uint8_t *split = (uint8_t *)(ws + l.oS), *dtree = (uint8_t *)(ws + l.oT), *dout = (uint8_t *)(ws + l.oO);
    if (tree) {
        rc = wl_stage_to_device(ctx, dtree, tree, (size_t)ntree, st);
        if (rc) return rc;
    }
    const int64_t np = (int64_t)entropy_partials(n);
    const T *cur = x;
    if (S != n) {                                        // a padded batch: from here on a dense one
        Extent3 full = {{n, 1, G}};
        Strides3 sst = {{1, n, S}}, dst = {{1, n, n}};
        WL_HIP(ctx, generic_copy_box<T>(st, x, sst, A, dst, full));
        cur = A;
        S = n;
    }
    EntBatch bu = {G, S, np, uent};
    WL_HIP(ctx, entropy_norm<T>(st, cur, n, part, nrm, bu));
    for (int d = 0; d <= Lmax; ++d) {
        if (d > 0) {
            T *out = (cur == A) ? B : A;
            WptCall<T> c;
            c.n = n; c.taps = &taps;
            c.full_depth = d; c.first_depth = d - 1;
            c.nunits = G; c.ustride = S;
            rc = wpt_impl<T>(ctx, st, out, cur, c);
            if (rc) return rc;
            cur = out;
        }
        if (d < Lmax) WL_HIP(ctx, entropy_segments<T>(st, et, cur, n >> d, (int64_t)1 << d, nrm, 0.0, part, ent + ((int64_t)1 << d) - 1, bu));
        else WL_HIP(ctx, entropy_segments<T>(st, et, cur, n >> (Lmax - 1), naf, nrm, 0.0, part, ent + ntree, bu));
    }
    WL_HIP(ctx, bestbasis_decide(st, ent, ntree, Lmax, best, split, tree ? dtree : nullptr, Lfull, tree_out ? tree_out : dout, G, uent,
                                 tree_out ? tstride : ntree));
    if (ws_out) *ws_out = dout;
    ctx->last_kernel = "k_entropy_seg";
    return WL_OK;
}

template <typename T>
static int bestbasis_impl(wl_ctx *ctx, hipStream_t st, const T *x, int64_t n, const Taps<T> &taps, const uint8_t *tree, int64_t ntree,
                          int et, uint8_t *tree_out, double *node_entropy)
{
    uint8_t *dout = nullptr;
    int rc = bestbasis_group<T>(ctx, st, x, n, 1, n, taps, tree, 0, et, nullptr, ntree, node_entropy, 0, &dout);
    if (rc) return rc;
    WL_HIP(ctx, hipMemcpyAsync(tree_out, dout, (size_t)ntree, hipMemcpyDeviceToHost, st));
    WL_HIP(ctx, hipStreamSynchronize(st));
    return WL_OK;
}

// units in groups of G, as wpt_batch_impl; one workspace size for every group (the last one may be shorter): nothing grows between groups
template <typename T>
static int bestbasis_batch_impl(wl_ctx *ctx, hipStream_t st, const T *x, int64_t n, int64_t nunits, int64_t S, const Taps<T> &taps,
                                const uint8_t *tree, int Lfull, int et, uint8_t *trees_out, int64_t tstride, double *node_entropy, int64_t estride)
{
    auto bytes = [&](int64_t G) { return bb_layout(n, G, sizeof(T), node_entropy == nullptr).total; };
    const int64_t G = group_size(nunits, 65535, opt("WL_WPT_BATCH_GROUP", 0), true, group_cap(), bytes);
    WL_TRY(ensure_ws(ctx, bytes(G), st));
    return for_groups(nunits, G, [&](int64_t u0, int64_t nb) {
        return bestbasis_group<T>(ctx, st, x + u0 * S, n, nb, S, taps, tree, Lfull, et, trees_out + u0 * tstride, tstride,
                                  node_entropy ? node_entropy + u0 * estride : nullptr, estride, nullptr);
    });
}

// ---- batched packet transforms (wl_wpt_*_batch) --------------------------------------------------------------------------------
// c.nunits signals of stride c.ustride in groups of G units: all of them, at most 65535 (option WL_WPT_BATCH_GROUP lowers it),
// halved while the buffers of a group -- its work buffer and tree_bytes per unit -- exceed the context's cap (group_size).  65535
// is what the second grid dimension of the packet kernels takes.  A group is ONE wpt_impl call over all its units.
template <typename T>
static int wpt_batch_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, const WptCall<T> &c, size_t tree_bytes = 0)
{
    const int64_t G = group_size(c.nunits, 65535, opt("WL_WPT_BATCH_GROUP", 0), true, group_cap(),
                                 [&](int64_t g) { return (size_t)g * ((size_t)c.ustride * sizeof(T) + tree_bytes); });
    return for_groups(c.nunits, G, [&](int64_t u0, int64_t nb) {
        WptCall<T> g = c;
        g.nunits = nb;
        if (c.utrees) g.utrees = c.utrees + u0 * c.utstride;
        return wpt_impl<T>(ctx, st, y + u0 * c.ustride, x + u0 * c.ustride, g);
    });
}

// what the two entry points share after their pointer / dtype / wavelet rules
static int wpt_batch_check(int64_t n, int64_t nunits, int64_t unit_stride, const void *y, const void *x, bool alias_ok, const uint8_t *tree,
                           int64_t ntree, int L, int64_t *last_set)
{
    if (n < 1 || nunits < 1 || unit_stride < n || unit_stride >= ((int64_t)1 << 61) / nunits) return WL_EDIMS;
    if (!alias_ok && y == x) return WL_EALIAS;
    return check_tree_or_depth(n, tree, ntree, L, last_set);
}

// the call of the entry points that take a HOST tree or, with tree == NULL, the full tree of depth L
template <typename T>
static WptCall<T> wpt_call(int64_t n, const Taps<T> *taps, const LiftScheme<T> *sc, const uint8_t *tree, int64_t ntree, int64_t last_set, int L,
                           int fw)
{
    WptCall<T> c;
    c.n = n; c.taps = taps; c.sc = sc; c.fw = fw;
    if (tree) { c.tree = tree; c.ntree = ntree; c.last_set = last_set; }
    else c.full_depth = L;
    return c;
}

// ---- complex-valued transforms (wl_*_complex) ----------------------------------------------------------------------------------
// Complex{T} data is (re, im) interleaved and the taps are real: re(y) = transform(re(x)), im(y) = transform(im(x)).  A group of G
// complex units is split into 2 G planar real planes P (k_cplx_split, wl_complex.hip), the batched level loops of the real entry
// points run on the planes as a batch of 2 G units of stride ps -- the same bits as the real transform of each component --, and
// the result is merged back interleaved (k_cplx_merge).  ps = the unit's element count rounded up to 16 bytes, so that every plane
// base is 16-byte aligned (what the batched tiers ask for).  Workspace layout (bytes): [the inner level loop's region | P | Q].
namespace {

template <typename T>
inline int64_t plane_stride_of(int64_t N)
{
    const int64_t E = 16 / (int64_t)sizeof(T);
    return (N + E - 1) / E * E;
}

// (groups: group_reserve with a limit of 32767 units -- 2 G planes, a grid row / plane / workgroup per plane in the batched kernels;
// the planes of a group are one batch for filter_levels_planes / lifting_levels_planes, wl_entry.h)

template <typename T>
int dwt_filter_complex_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, int64_t nunits, int64_t S,
                            const double *qmf, int flen, int L, int fw)
{
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    if (L == 0) return copy_units<T>(ctx, st, y, x, 2 * N, y != x ? nunits : 0, 2 * S);      // (a unit: 2 N reals)
    const int64_t ps = plane_stride_of<T>(N);
    const Taps<T> taps = taps_of<T>(qmf, flen);
    auto tw_bytes = [&](int64_t G) { return up256(ws_filter_planes_elems(ndims, N, 2 * G) * sizeof(T)); };
    auto pl_bytes = [&](int64_t G) { return up256((size_t)(2 * G * ps) * sizeof(T)); };
    auto need = [&](int64_t G) { return tw_bytes(G) + 2 * pl_bytes(G); };
    int64_t G = 1;
    int rc = group_reserve(ctx, st, nunits, 32767, need, G);
    if (rc != WL_OK) return rc;
    char *wsb = (char *)ctx->ws;
    T *P = (T *)(wsb + tw_bytes(G)), *Q = (T *)(wsb + tw_bytes(G) + pl_bytes(G));
    const char *kn = ctx->last_kernel;
    WL_TRY(for_groups(nunits, G, [&](int64_t u0, int64_t nb) -> int {
        WL_HIP(ctx, complex_split<T>(st, ctx->cu_count, P, ps, x + 2 * u0 * S, N, nb, S));
        rc = filter_levels_planes<T>(ctx, st, fw, ndims, dims, 2 * nb, ps, Q, P, taps, L, &kn);
        if (rc == WL_RETRY_GEN) rc = WL_EINVAL_ARG;          // (the full workspace is held: no level can ask for more)
        if (rc != WL_OK) return rc;
        WL_HIP(ctx, complex_merge<T>(st, ctx->cu_count, y + 2 * u0 * S, Q, ps, N, nb, S));
        return WL_OK;
    }));
    ctx->last_kernel = kn;
    return WL_OK;
}

template <typename T>
int dwt_lifting_complex_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, int64_t nunits, int64_t S,
                             const LiftScheme<T> &sc, int L, int fw)
{
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    if (L == 0) return copy_units<T>(ctx, st, y, x, 2 * N, y != x ? nunits : 0, 2 * S);      // (a unit: 2 N reals)
    const int64_t ps = plane_stride_of<T>(N);
    // the lifting workspace of the planes of a group, as wl_denoise_batch_lifting sizes it (the loops below ask for no more)
    auto tw_bytes = [&](int64_t G) { return up256(ws_lifting_planes_elems(ndims, N, 2 * G) * sizeof(T)); };
    auto need = [&](int64_t G) { return tw_bytes(G) + up256((size_t)(2 * G * ps) * sizeof(T)); };
    int64_t G = 1;
    int rc = group_reserve(ctx, st, nunits, 32767, need, G);
    if (rc != WL_OK) return rc;
    const void *held = ctx->ws;
    T *P = (T *)((char *)ctx->ws + tw_bytes(G));
    return for_groups(nunits, G, [&](int64_t u0, int64_t nb) -> int {
        WL_HIP(ctx, complex_split<T>(st, ctx->cu_count, P, ps, x + 2 * u0 * S, N, nb, S));
        rc = lifting_levels_planes<T>(ctx, st, ndims, dims[0], 2 * nb, ps, P, P, sc, L, fw);
        if (rc != WL_OK) return rc;
        if (ctx->ws != held) return WL_ENOMEM;               // (a loop that outgrew the reservation would have moved P: not reached)
        WL_HIP(ctx, complex_merge<T>(st, ctx->cu_count, y + 2 * u0 * S, P, ps, N, nb, S));
        return WL_OK;
    });
}

// the argument contract the two complex dwt entry points share after their pointer / dtype / wavelet rules (the order of the real
// batch entry points): WL_EINVAL_CUBE (lifting only), WL_EDIMS, WL_EINVAL_L, WL_EINVAL_SIZE
int complex_check(int ndims, const int64_t *dims, int64_t nunits, int64_t unit_stride, int L, bool cube)
{
    if (cube && ndims >= 2 && ndims <= 3)
        for (int d = 1; d < ndims; ++d)
            if (dims[d] != dims[0]) return WL_EINVAL_CUBE;
    if (ndims < 1 || ndims > 3 || nunits < 1) return WL_EDIMS;
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) {
        // (a unit of 2^61 values or more: above every stride in reals an int64 holds)
        if (dims[d] < 1 || dims[d] >= ((int64_t)1 << 61) / N) return WL_EDIMS;
        N *= dims[d];
    }
    if (unit_stride < N) return WL_EDIMS;
    if (L < 0) return WL_EINVAL_L;
    for (int d = 0; d < ndims; ++d)
        if (!sufficientpoweroftwo(dims[d], L)) return WL_EINVAL_SIZE;
    return WL_OK;
}

// one complex signal through the packet transform: split, wpt_impl on the two planes as one batch of two units of stride ps
// (filters: P -> Q; lifting: in place on P), merge
template <typename T>
int wpt_complex_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, WptCall<T> c)
{
    const int64_t n = c.n, ps = plane_stride_of<T>(n);
    const size_t inner = up256(ws_elems(2 * ps) * sizeof(T) + (size_t)c.ntree + 256), pl = up256((size_t)(2 * ps) * sizeof(T));
    int rc = ensure_ws(ctx, inner + (c.taps ? 2 : 1) * pl, st);
    if (rc != WL_OK) return rc;
    const void *held = ctx->ws;
    T *P = (T *)((char *)ctx->ws + inner), *Q = c.taps ? (T *)((char *)ctx->ws + inner + pl) : P;
    WL_HIP(ctx, complex_split<T>(st, ctx->cu_count, P, ps, x, n, 1, n));
    c.nunits = 2; c.ustride = ps;
    rc = wpt_impl<T>(ctx, st, Q, P, c);
    if (rc != WL_OK) return rc;
    if (ctx->ws != held) return WL_ENOMEM;                   // (not reached: wpt_impl asks for no more than `inner`)
    WL_HIP(ctx, complex_merge<T>(st, ctx->cu_count, y, Q, ps, n, 1, n));
    return WL_OK;
}

}  // namespace

// ==========================================================================================
extern "C" {

int wl_bestbasistree_filter(wl_ctx *ctx, int dtype, const void *x, int64_t n, const double *qmf, int flen, const uint8_t *tree,
                            int64_t ntree, int et, uint8_t *tree_out, double *node_entropy, void *stream)
{
    if (!ctx || !x || !qmf || !tree || !tree_out) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (et != WL_ENTROPY_SHANNON && et != WL_ENTROPY_LOGENERGY) return WL_EINVAL_ARG;
    WL_TRY(check_flen(flen));
    if (n < 1) return WL_EDIMS;
    if (wl_maxtransformlevels(n) == 0) return WL_EINVAL_SIZE;        // the reference fails on 2^(Lmax - 1) (entropy.jl:85)
    int64_t last_set = -1;
    if (!isvalidtree(n, tree, ntree, &last_set)) return WL_EINVAL_TREE;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return bestbasis_impl<T>(ctx, st, (const T *)x, n, taps_of<T>(qmf, flen), tree, ntree, et, tree_out, node_entropy);
    });
}

int wl_wpt_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, const double *qmf, int flen,
                  const uint8_t *tree, int64_t ntree, int fw, void *stream)
{
    if (!ctx || !y || !x || !qmf || (!tree && ntree > 0)) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    if (n < 1) return WL_EDIMS;
    if (y == x) return WL_EALIAS;
    int64_t last_set = -1;
    if (!isvalidtree(n, tree, ntree, &last_set)) return WL_EINVAL_TREE;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const Taps<T> taps = taps_of<T>(qmf, flen);
        WptCall<T> c;
        c.n = n; c.taps = &taps; c.fw = fw;
        c.tree = tree; c.ntree = ntree; c.last_set = last_set;
        return wpt_impl<T>(ctx, st, (T *)y, (const T *)x, c);
    });
}

int wl_wpt_lifting(wl_ctx *ctx, int dtype, void *y, int64_t n,
                   int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                   const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2,
                   const uint8_t *tree, int64_t ntree, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || (!tree && ntree > 0)) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (n < 1) return WL_EDIMS;
    int64_t last_set = -1;
    if (!isvalidtree(n, tree, ntree, &last_set)) return WL_EINVAL_TREE;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        WL_TRY(s.check());
        const LiftScheme<T> sc = s.build<T>(fw);
        WptCall<T> c;
        c.n = n; c.sc = &sc; c.fw = fw;
        c.tree = tree; c.ntree = ntree; c.last_set = last_set;
        return wpt_impl<T>(ctx, st, (T *)y, (const T *)y, c);
    });
}

int wl_dwt_filter_batch(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, int64_t nimages, int64_t image_stride,
                        const double *qmf, int flen, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !dims || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    if (dims[0] < 1 || dims[1] < 1 || nimages < 1 || image_stride < dims[0] * dims[1]) return WL_EDIMS;
    if (L < 0) return WL_EINVAL_L;
    if (!sufficientpoweroftwo(dims[0], L) || !sufficientpoweroftwo(dims[1], L)) return WL_EINVAL_SIZE;
    if (y == x) return WL_EALIAS;
    BoxSpec b;
    b.nd = 3; b.nt = 2;
    b.dims[0] = dims[0]; b.dims[1] = dims[1]; b.dims[2] = nimages;
    b.full.s[0] = 1; b.full.s[1] = dims[0]; b.full.s[2] = image_stride;
    // images in groups of at most 65535 (one grid row / plane per image in the batched kernels)
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return for_groups(nimages, 65535, [&](int64_t i0, int64_t ni) {
            b.dims[2] = ni;
            return dwt_filter_impl<T>(ctx, st, b, (T *)y + i0 * image_stride, (const T *)x + i0 * image_stride, qmf, flen, L, fw);
        });
    });
}

int wl_dwt_filter_batch3(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, int64_t nvolumes, int64_t volume_stride,
                         const double *qmf, int flen, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !dims || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || nvolumes < 1 || volume_stride < dims[0] * dims[1] * dims[2]) return WL_EDIMS;
    if (L < 0) return WL_EINVAL_L;
    if (!sufficientpoweroftwo(dims[0], L) || !sufficientpoweroftwo(dims[1], L) || !sufficientpoweroftwo(dims[2], L)) return WL_EINVAL_SIZE;
    if (y == x) return WL_EALIAS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return dwt_filter_batch3_impl<T>(ctx, st, dims, nvolumes, volume_stride, (T *)y, (const T *)x, qmf, flen, L, fw);
    });
}

int wl_dwt_lifting_batch(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, int64_t nimages, int64_t image_stride,
                         int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef, const int32_t *step_shift,
                         const double *coefs_flat, double norm1, double norm2, int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || !x || !dims) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (dims[0] != dims[1]) return WL_EINVAL_CUBE;           // the square rule comes first in the reference (transforms_lifting.jl:131-132)
    if (dims[0] < 1 || nimages < 1 || image_stride < dims[0] * dims[1]) return WL_EDIMS;
    if (L < 0) return WL_EINVAL_L;
    if (!sufficientpoweroftwo(dims[0], L)) return WL_EINVAL_SIZE;
    WL_TRY(s.check());
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const LiftScheme<T> sc = s.build<T>(fw);
        return lifting_batch_impl<T>(ctx, st, (T *)y, (const T *)x, dims[0], nimages, image_stride, sc, L, fw);
    });
}

int wl_dwt_lifting_batch3(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, int64_t nvolumes, int64_t volume_stride,
                          int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef, const int32_t *step_shift,
                          const double *coefs_flat, double norm1, double norm2, int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || !x || !dims) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (dims[0] != dims[1] || dims[0] != dims[2]) return WL_EINVAL_CUBE;     // the cube rule comes first in the reference (transforms_lifting.jl:203)
    // (a side of 2^21 or more: the volume has 2^63 elements or more, above every stride an int64 holds)
    if (dims[0] < 1 || nvolumes < 1 || dims[0] >= ((int64_t)1 << 21) || volume_stride < dims[0] * dims[1] * dims[2]) return WL_EDIMS;
    if (L < 0) return WL_EINVAL_L;
    if (!sufficientpoweroftwo(dims[0], L)) return WL_EINVAL_SIZE;
    WL_TRY(s.check());
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const LiftScheme<T> sc = s.build<T>(fw);
        return wl_lifting_vols<T>(ctx, st, dims[0], nvolumes, volume_stride, (T *)y, (const T *)x, sc, L, fw);
    });
}

int wl_wpt_filter_full(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, const double *qmf, int flen, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    if (n < 1) return WL_EDIMS;
    if (y == x) return WL_EALIAS;
    if (L < 0 || L > wl_maxtransformlevels(n)) return WL_EINVAL_L;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const Taps<T> taps = taps_of<T>(qmf, flen);
        WptCall<T> c;
        c.n = n; c.taps = &taps; c.fw = fw;
        c.full_depth = L;
        return wpt_impl<T>(ctx, st, (T *)y, (const T *)x, c);
    });
}

int wl_wpt_lifting_full(wl_ctx *ctx, int dtype, void *y, int64_t n,
                        int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                        const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2,
                        int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (n < 1) return WL_EDIMS;
    if (L < 0 || L > wl_maxtransformlevels(n)) return WL_EINVAL_L;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        WL_TRY(s.check());
        const LiftScheme<T> sc = s.build<T>(fw);
        WptCall<T> c;
        c.n = n; c.sc = &sc; c.fw = fw;
        c.full_depth = L;
        return wpt_impl<T>(ctx, st, (T *)y, (const T *)y, c);
    });
}

// ---- batched packet transforms ---------------------------------------------------------------------------------------------------
int wl_wpt_filter_batch(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, int64_t nunits, int64_t unit_stride,
                        const double *qmf, int flen, const uint8_t *tree, int64_t ntree, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    int64_t last_set = -1;
    WL_TRY(wpt_batch_check(n, nunits, unit_stride, y, x, false, tree, ntree, L, &last_set));
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const Taps<T> taps = taps_of<T>(qmf, flen);
        WptCall<T> c = wpt_call<T>(n, &taps, nullptr, tree, ntree, last_set, L, fw);
        c.nunits = nunits; c.ustride = unit_stride;
        return wpt_batch_impl<T>(ctx, st, (T *)y, (const T *)x, c);
    });
}

int wl_wpt_lifting_batch(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, int64_t nunits, int64_t unit_stride, int nsteps,
                         const int32_t *step_is_update, const int32_t *step_ncoef, const int32_t *step_shift, const double *coefs_flat,
                         double norm1, double norm2, const uint8_t *tree, int64_t ntree, int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || !x) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(s.check());
    int64_t last_set = -1;
    WL_TRY(wpt_batch_check(n, nunits, unit_stride, y, x, true, tree, ntree, L, &last_set));
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const LiftScheme<T> sc = s.build<T>(fw);
        WptCall<T> c = wpt_call<T>(n, nullptr, &sc, tree, ntree, last_set, L, fw);
        c.nunits = nunits; c.ustride = unit_stride;
        return wpt_batch_impl<T>(ctx, st, (T *)y, (const T *)x, c);
    });
}

// ---- per-unit trees: the batched best-basis search and the packet transforms that take its result --------
int wl_bestbasistree_filter_batch(wl_ctx *ctx, int dtype, const void *x, int64_t n, int64_t nunits, int64_t unit_stride, const double *qmf,
                                  int flen, const uint8_t *tree, int64_t ntree, int L, int et, uint8_t *trees_out, int64_t tree_stride,
                                  double *node_entropy, int64_t entropy_stride, void *stream)
{
    if (!ctx || !x || !qmf || !trees_out) return WL_EINVAL_ARG;
    if (et != WL_ENTROPY_SHANNON && et != WL_ENTROPY_LOGENERGY) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    if (n < 1 || nunits < 1 || unit_stride < n || unit_stride >= ((int64_t)1 << 61) / nunits) return WL_EDIMS;
    const int Lmax = wl_maxtransformlevels(n);
    const int64_t nt = ((int64_t)1 << Lmax) - 1;
    if (tree_stride < nt || tree_stride >= ((int64_t)1 << 61) / nunits) return WL_EDIMS;
    if (node_entropy && Lmax > 0 && (entropy_stride < nt + ((int64_t)1 << (Lmax - 1)) || entropy_stride >= ((int64_t)1 << 58) / nunits))
        return WL_EDIMS;
    if (Lmax == 0) return WL_EINVAL_SIZE;                                // the reference fails on 2^(Lmax - 1) (entropy.jl:85)
    int64_t last_set = -1;
    WL_TRY(check_tree_or_depth(n, tree, ntree, L, &last_set));
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return bestbasis_batch_impl<T>(ctx, st, (const T *)x, n, nunits, unit_stride, taps_of<T>(qmf, flen), tree, L, et, trees_out, tree_stride,
                                       node_entropy, entropy_stride);
    });
}

int wl_wpt_filter_batch_trees(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, int64_t nunits, int64_t unit_stride, const double *qmf,
                              int flen, const uint8_t *trees, int64_t tree_stride, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !qmf || !trees) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    if (n < 1 || nunits < 1 || unit_stride < n || unit_stride >= ((int64_t)1 << 61) / nunits) return WL_EDIMS;
    const int Lmax = wl_maxtransformlevels(n);
    if (tree_stride < ((int64_t)1 << Lmax) - 1 || tree_stride >= ((int64_t)1 << 61) / nunits) return WL_EDIMS;
    if (y == x) return WL_EALIAS;
    if (L < 0 || L > Lmax) return WL_EINVAL_L;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const Taps<T> taps = taps_of<T>(qmf, flen);
        WptCall<T> c;
        c.n = n; c.taps = &taps; c.fw = fw;
        c.nunits = nunits; c.ustride = unit_stride;
        c.utrees = trees; c.utstride = tree_stride; c.utL = L;
        // the closed trees of a group (G (2^L - 1) bytes) ride on top of its work buffer
        return wpt_batch_impl<T>(ctx, st, (T *)y, (const T *)x, c, ((size_t)1 << L) - 1);
    });
}

// ---- complex-valued transforms ---------------------------------------------------------------------------------------------------
int wl_complex_split(wl_ctx *ctx, int dtype, void *planes, int64_t plane_stride, const void *z, int64_t n, int64_t nunits,
                     int64_t unit_stride, void *stream)
{
    if (!ctx || !planes || !z) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (n < 1 || nunits < 1 || unit_stride < n || plane_stride < n) return WL_EDIMS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) -> int {
        using T = decltype(t);
        WL_HIP(ctx, complex_split<T>(st, ctx->cu_count, (T *)planes, plane_stride, (const T *)z, n, nunits, unit_stride));
        return WL_OK;
    });
}

int wl_complex_merge(wl_ctx *ctx, int dtype, void *z, const void *planes, int64_t plane_stride, int64_t n, int64_t nunits,
                     int64_t unit_stride, void *stream)
{
    if (!ctx || !planes || !z) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (n < 1 || nunits < 1 || unit_stride < n || plane_stride < n) return WL_EDIMS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) -> int {
        using T = decltype(t);
        WL_HIP(ctx, complex_merge<T>(st, ctx->cu_count, (T *)z, (const T *)planes, plane_stride, n, nunits, unit_stride));
        return WL_OK;
    });
}

int wl_dwt_filter_complex(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, int64_t nunits,
                          int64_t unit_stride, const double *qmf, int flen, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !dims || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    WL_TRY(complex_check(ndims, dims, nunits, unit_stride, L, false));
    if (y == x) return WL_EALIAS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return dwt_filter_complex_impl<T>(ctx, st, (T *)y, (const T *)x, ndims, dims, nunits, unit_stride, qmf, flen, L, fw);
    });
}

int wl_dwt_lifting_complex(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, int64_t nunits,
                           int64_t unit_stride, int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                           const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2, int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || !x || !dims) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(s.check());
    WL_TRY(complex_check(ndims, dims, nunits, unit_stride, L, true));
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const LiftScheme<T> sc = s.build<T>(fw);
        return dwt_lifting_complex_impl<T>(ctx, st, (T *)y, (const T *)x, ndims, dims, nunits, unit_stride, sc, L, fw);
    });
}

int wl_wpt_filter_complex(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, const double *qmf, int flen, const uint8_t *tree,
                          int64_t ntree, int L, int fw, void *stream)
{
    if (!ctx || !y || !x || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    if (n < 1 || n >= ((int64_t)1 << 61)) return WL_EDIMS;
    if (y == x) return WL_EALIAS;
    int64_t last_set = -1;
    WL_TRY(check_tree_or_depth(n, tree, ntree, L, &last_set));
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const Taps<T> taps = taps_of<T>(qmf, flen);
        return wpt_complex_impl<T>(ctx, st, (T *)y, (const T *)x, wpt_call<T>(n, &taps, nullptr, tree, ntree, last_set, L, fw));
    });
}

int wl_wpt_lifting_complex(wl_ctx *ctx, int dtype, void *y, const void *x, int64_t n, int nsteps, const int32_t *step_is_update,
                           const int32_t *step_ncoef, const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2,
                           const uint8_t *tree, int64_t ntree, int L, int fw, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || !x) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (n < 1 || n >= ((int64_t)1 << 61)) return WL_EDIMS;
    int64_t last_set = -1;
    WL_TRY(check_tree_or_depth(n, tree, ntree, L, &last_set));
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        WL_TRY(s.check());
        const LiftScheme<T> sc = s.build<T>(fw);
        return wpt_complex_impl<T>(ctx, st, (T *)y, (const T *)x, wpt_call<T>(n, nullptr, &sc, tree, ntree, last_set, L, fw));
    });
}

}  // extern "C"

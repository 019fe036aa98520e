// wl_entry.h -- what the extern "C" entry points (wl_api.hip, wl_ext.hip, wl_modwt.hip, wl_thbatch.hip) share: the element-type
// dispatch, the dtype / filter length rules, the lifting scheme as the ABI passes it, the grouping of a batch's units and the level
// loops of a batch of planes.  Every entry point applies its rules in the order the header documents for it, then dispatches once
// through by_dtype.
#pragma once
#include "wl_ctx.h"
#include "wl_fast.h"

// return a status that is not WL_OK
#define WL_TRY(expr)                \
    do {                            \
        const int rc__ = (expr);    \
        if (rc__ != WL_OK) return rc__; \
    } while (0)

// f(float()) or f(double()): the one place where an entry point's dtype becomes a type.  Callers write
//     return by_dtype(dtype, [&](auto t) { using T = decltype(t); return impl<T>(ctx, st, (T *)y, (const T *)x, ...); });
template <typename F>
inline auto by_dtype(int dtype, F f)
{
    return dtype == WL_F32 ? f(float()) : f(double());
}

// the entry points whose last rule is behind them: the context's device made current, then f(T(), stream) for the element type
template <typename F>
inline int scoped_by_dtype(wl_ctx *ctx, int dtype, void *stream, F f)
{
    WL_SCOPE(ctx);
    return by_dtype(dtype, [&](auto t) { return f(t, (hipStream_t)stream); });
}

inline int check_dtype(int dtype) { return (dtype != WL_F32 && dtype != WL_F64) ? WL_EINVAL_DTYPE : WL_OK; }
// the first two rules of the older entry points, which enter the scope right behind them
inline int ext_enter(wl_ctx *ctx, int dtype)
{
    if (!ctx) return WL_EINVAL_ARG;
    return check_dtype(dtype);
}
// min: 2 for the transforms, 1 for modwt / imodwt
inline int check_flen(int flen, int min = 2) { return (flen < min || flen > WL_MAX_FLEN) ? WL_EINVAL_FILTER : WL_OK; }

template <typename T>
inline wl::Taps<T> taps_of(const double *qmf, int flen)
{
    wl::Taps<T> t;
    wl::make_taps<T>(qmf, flen, t);
    return t;
}

// the lifting scheme as every lifting entry point takes it: makescheme (transforms_lifting.jl:13-25)
struct SchemeArgs {
    int nsteps;
    const int32_t *is_update, *ncoef, *shift;
    const double *coefs;
    double norm1, norm2;

    int check() const
    {
        if (nsteps < 0 || nsteps > WL_MAX_STEPS) return WL_EINVAL_SCHEME;
        if (nsteps > 0 && (!is_update || !ncoef || !shift || !coefs)) return WL_EINVAL_ARG;
        for (int i = 0; i < nsteps; ++i)
            if (ncoef[i] < 1 || ncoef[i] > WL_MAX_NCOEF) return WL_EINVAL_SCHEME;
        return WL_OK;
    }
    // the direction-adjusted scheme of a checked argument set (what the kernels' comments call make_scheme)
    template <typename T>
    wl::LiftScheme<T> build(int fw) const
    {
        wl::LiftScheme<T> sc;
        int off[WL_MAX_STEPS];
        int o = 0;
        for (int i = 0; i < nsteps; ++i) {
            off[i] = o;
            o += ncoef[i];
        }
        sc.nsteps = nsteps;
        for (int i = 0; i < nsteps; ++i) {
            int j = fw ? i : nsteps - 1 - i;
            wl::LiftStep<T> &st = sc.step[i];
            st.is_update = is_update[j] ? 1 : 0;
            st.nc = ncoef[j];
            st.shift = shift[j];
            for (int k = 0; k < WL_MAX_NCOEF; ++k) st.c[k] = (T)0;
            for (int k = 0; k < st.nc; ++k) st.c[k] = (T)(coefs[off[j] + k] * (fw ? -1.0 : 1.0));
        }
        sc.norm1 = (T)(fw ? norm1 : 1.0 / norm1);
        sc.norm2 = (T)(fw ? norm2 : 1.0 / norm2);
        return sc;
    }
};

// ---- the units of a batch in groups of G -------------------------------------------------------------------------------------
// the cap on a group's buffers (option WL_TI_WS_CAP_MB), in bytes
inline size_t group_cap() { return (size_t)wl::opt("WL_TI_WS_CAP_MB", 8192) << 20; }

// G, from bytes(G) = the size of a group's buffers.  limit: what a grid dimension of the batched kernels takes (65535; 32767 for
// the two planes of a complex unit).
//  * limit_first (the packet batches): min(nunits, limit), lowered to `lower` when 1 <= lower (option WL_WPT_BATCH_GROUP: tests
//    reach the group boundary with a handful of units), then halved while the group exceeds the cap;
//  * otherwise (the denoise, complex and translation-invariant batches; lower = 0): nunits halved while the group exceeds the
//    cap, then cut to the limit.
template <typename F>
inline int64_t group_size(int64_t nunits, int64_t limit, long long lower, bool limit_first, size_t cap, F bytes)
{
    int64_t G = nunits;
    if (limit_first && G > limit) G = limit;
    if (lower >= 1 && lower < G) G = lower;
    while (G > 1 && bytes(G) > cap) G = (G + 1) / 2;
    if (G > limit) G = limit;
    return G;
}

// group_size(.., 0, false, ..), then the workspace is grown once to bytes(G) -- with smaller groups when that allocation fails
// (another allocator may own most of the HBM)
template <typename F>
inline int group_reserve(wl_ctx *ctx, hipStream_t st, int64_t nunits, int64_t limit, F bytes, int64_t &G)
{
    G = group_size(nunits, limit, 0, false, group_cap(), bytes);
    int rc = wl_ensure_ws(ctx, bytes(G), st, true);
    while (rc == WL_ENOMEM && G > 1) {
        G = (G + 1) / 2;
        rc = wl_ensure_ws(ctx, bytes(G), st, true);
    }
    return rc;
}

// f(u0, nb) for every group of at most G units, until one returns a status that is not WL_OK
template <typename F>
inline int for_groups(int64_t nunits, int64_t G, F f)
{
    for (int64_t u0 = 0; u0 < nunits; u0 += G) WL_TRY(f(u0, (nunits - u0 < G) ? (nunits - u0) : G));
    return WL_OK;
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- all `lev` levels on nb planes of stride ps (planes_box, wl_fast.h; cubes: a batch of volumes) in the context's workspace ---------
// The status of the level loop comes back untranslated (WL_RETRY_GEN, WL_RETRY_NOVIEW: the caller's business); *kn = the kernel's name.
template <typename T>
inline int filter_levels_planes(wl_ctx *ctx, hipStream_t st, int fw, int ndims, const int64_t *dims, int64_t nb, int64_t ps, T *dst, const T *src,
                                const wl::Taps<T> &taps, int lev, const char **kn)
{
    if (ndims == 3)
        return fw ? wl::filter_fwd_levels_vols<T>(ctx->ws, true, ctx->cu_count, ctx->path, st, dims, nb, ps, ps, dst, src, taps, lev, kn, &ctx->last_hip)
                  : wl::filter_inv_levels_vols<T>(ctx->ws, true, ctx->cu_count, ctx->path, st, dims, nb, ps, ps, dst, src, taps, lev, kn, &ctx->last_hip);
    const wl::BoxSpec b = wl::planes_box(ndims, dims, nb, ps);
    return fw ? wl::filter_fwd_levels<T>(ctx->ws, true, ctx->cu_count, ctx->path, st, b, dst, src, taps, lev, kn, &ctx->last_hip)
              : wl::filter_inv_levels<T>(ctx->ws, true, ctx->cu_count, ctx->path, st, b, dst, src, taps, lev, kn, &ctx->last_hip);
}
// the same with a direction-adjusted lifting scheme on lines / squares / cubes of side n0
template <typename T>
inline int lifting_levels_planes(wl_ctx *ctx, hipStream_t st, int ndims, int64_t n0, int64_t nb, int64_t ps, T *dst, const T *src,
                                 const wl::LiftScheme<T> &sc, int lev, int fw)
{
    if (ndims == 3) return wl_lifting_vols<T>(ctx, st, n0, nb, ps, dst, src, sc, lev, fw);
    const int64_t dims[2] = {n0, n0};
    return wl_lifting_box<T>(ctx, st, wl::planes_box(ndims, dims, nb, ps), dst, src, sc, lev, fw);
}

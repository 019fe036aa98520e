// wl_modwt.hip -- the maximal-overlap transforms:
//   modwt / imodwt                       transforms_maximal_overlap.jl:10-107
// their batched forms (wl_modwt_batch / wl_imodwt_batch) and the multiresolution analysis built from one-sided
// inverse steps (wl_modwt_mra_batch).  HBM-bound gather work; the arithmetic follows
// Julia's promotion rules literally (Float32 data with Float64 taps: compute in Float64, round on every store) so the results are
// bit-identical to the reference loops.
#include "wl_entry.h"
#include "wl_select.h"

#include <cmath>

using namespace wl;

namespace {

// ---- MODWT -----------------------------------------------------------------------------------------
struct ModwtTaps { int F; double h[WL_MAX_FLEN]; double g[WL_MAX_FLEN]; };   // h: detail, g: scaling (both / sqrt 2)

// WT.makereverseqmfpair(wt) (fw, Float64: g = reverse(qmf), h = mirror(qmf)) then `/= sqrt(2)`, :50-52
void make_modwt_taps(const double *qmf, int F, ModwtTaps &t)
{
    const double r2 = std::sqrt(2.0);
    t.F = F;
    for (int i = 0; i < WL_MAX_FLEN; ++i) { t.h[i] = 0.0; t.g[i] = 0.0; }
    for (int i = 0; i < F; ++i) {
        t.g[i] = qmf[F - 1 - i] / r2;
        t.h[i] = ((i & 1) ? -qmf[i] : qmf[i]) / r2;
    }
}

// a 16-byte vector of T
template <typename T>
using Vec16 = T __attribute__((ext_vector_type(16 / sizeof(T))));

// modwt_step (:10-31): w1[t] = sum_n h[n] v[t - n*stride], v1[t] = sum_n g[n] v[...], accumulated in tap order,
// every partial sum rounded to T (Julia: `w1[t] += h[n] * v[k]` with w1::Vector{T}, h::Vector{Float64}).
// The arithmetic of one output (or of the V outputs of one 16-byte chunk) lives in the device functions below: the single-unit
// kernels, the batched per-level kernels and the LDS kernels all call them, so every tier rounds alike.  I is the index type:
// int64_t over global memory, int inside a workgroup's LDS copy of a unit.
template <typename T, typename I>
__device__ __forceinline__ void modwt_point(const T *v, I N, I t, I stride, const ModwtTaps &tp, T &w, T &s)
{
    I k = t;
    double x = (double)v[k];
    w = (T)(tp.h[0] * x);
    s = (T)(tp.g[0] * x);
    for (int n = 1; n < tp.F; ++n) {
        k -= stride;
        if (k < 0) { k += N; if (k < 0) { k %= N; if (k < 0) k += N; } }   // one add unless the stride exceeds N (tiny signals)
        x = (double)v[k];
        w = (T)((double)w + tp.h[n] * x);
        s = (T)((double)s + tp.g[n] * x);
    }
}
// imodwt_step (:72-93): v0[t] = sum_n (h[n] w[t + n*stride] + g[n] v[t + n*stride])
template <typename T, typename I>
__device__ __forceinline__ T imodwt_point(const T *v, const T *w, I N, I t, I stride, const ModwtTaps &tp)
{
    I k = t;
    T acc = (T)(tp.h[0] * (double)w[k] + tp.g[0] * (double)v[k]);
    for (int n = 1; n < tp.F; ++n) {
        k += stride;
        if (k >= N) { k -= N; if (k >= N) k %= N; }
        acc = (T)((double)acc + (tp.h[n] * (double)w[k] + tp.g[n] * (double)v[k]));
    }
    return acc;
}

// the same for strides that are multiples of the 16-byte vector width (levels >= 3 for Float32, >= 2 for Float64) and N a
// multiple of it: every tap of V consecutive outputs is one aligned vector load.  t, NV and strideV count vectors.
template <typename T, typename I>
__device__ __forceinline__ void modwt_chunk_v(const T *v, I NV, I t, I strideV, const ModwtTaps &tp,
                                              Vec16<T> &w,
                                              Vec16<T> &s)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    const VT *vv = reinterpret_cast<const VT *>(v);
    I k = t;
    VT x = vv[k];
#pragma unroll
    for (int e = 0; e < V; ++e) { const double xd = (double)x[e]; w[e] = (T)(tp.h[0] * xd); s[e] = (T)(tp.g[0] * xd); }
    for (int n = 1; n < tp.F; ++n) {
        k -= strideV;
        if (k < 0) { k += NV; if (k < 0) { k %= NV; if (k < 0) k += NV; } }
        x = vv[k];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const double xd = (double)x[e];
            w[e] = (T)((double)w[e] + tp.h[n] * xd);
            s[e] = (T)((double)s[e] + tp.g[n] * xd);
        }
    }
}
template <typename T, typename I>
__device__ __forceinline__ Vec16<T> imodwt_chunk_v(const T *v, const T *w, I NV, I t, I strideV, const ModwtTaps &tp)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    const VT *vv = reinterpret_cast<const VT *>(v), *wv = reinterpret_cast<const VT *>(w);
    I k = t;
    VT a = vv[k], b = wv[k], acc;
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = (T)(tp.h[0] * (double)b[e] + tp.g[0] * (double)a[e]);
    for (int n = 1; n < tp.F; ++n) {
        k += strideV;
        if (k >= NV) { k -= NV; if (k >= NV) k %= NV; }
        a = vv[k];
        b = wv[k];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = (T)((double)acc[e] + (tp.h[n] * (double)b[e] + tp.g[n] * (double)a[e]));
    }
    return acc;
}

// strides below the vector width (levels 1-2 for Float32, level 1 for Float64; S divides V): a thread still produces V
// consecutive outputs from aligned 16-byte loads -- the V/S taps that fall into one vector step are served from the register
// pair [previous chunk | current chunk] with compile-time offsets, then the pair slides by one chunk.  Same tap order and
// per-tap rounding as modwt_point (a scalar kernel issues one 4-byte load per lane and tap: 1.2 TB/s of level traffic).
// NV >= 2.
template <typename T, int S, typename I>
__device__ __forceinline__ void modwt_chunk_s(const T *v, I NV, I t, const ModwtTaps &tp,
                                              Vec16<T> &w,
                                              Vec16<T> &s)
{
    constexpr int V = 16 / sizeof(T), G = V / S;
    typedef T VT __attribute__((ext_vector_type(V)));
    const VT *vv = reinterpret_cast<const VT *>(v);
    I k = t;
    VT c = vv[k];
    I kp = (k == 0) ? NV - 1 : k - 1;
    VT p = vv[kp];
    for (int n0 = 0; n0 < tp.F; n0 += G) {
        T win[2 * V];
#pragma unroll
        for (int e = 0; e < V; ++e) { win[e] = p[e]; win[V + e] = c[e]; }
        c = p;                                         // slide: the next group of taps starts one chunk back
        kp = (kp == 0) ? NV - 1 : kp - 1;
        p = vv[kp];
#pragma unroll
        for (int r = 0; r < G; ++r) {
            const int n = n0 + r;
            if (n < tp.F) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const double xd = (double)win[V + e - r * S];
                    if (n == 0) { w[e] = (T)(tp.h[0] * xd); s[e] = (T)(tp.g[0] * xd); }
                    else { w[e] = (T)((double)w[e] + tp.h[n] * xd); s[e] = (T)((double)s[e] + tp.g[n] * xd); }
                }
            }
        }
    }
}
template <typename T, int S, typename I>
__device__ __forceinline__ Vec16<T> imodwt_chunk_s(const T *v, const T *w, I NV, I t, const ModwtTaps &tp)
{
    constexpr int V = 16 / sizeof(T), G = V / S;
    typedef T VT __attribute__((ext_vector_type(V)));
    const VT *vv = reinterpret_cast<const VT *>(v), *wv = reinterpret_cast<const VT *>(w);
    I kn = (t + 1 == NV) ? 0 : t + 1;
    VT ca = vv[t], cb = wv[t], na = vv[kn], nb = wv[kn], acc;
    for (int n0 = 0; n0 < tp.F; n0 += G) {
        T wa[2 * V], wb[2 * V];
#pragma unroll
        for (int e = 0; e < V; ++e) { wa[e] = ca[e]; wa[V + e] = na[e]; wb[e] = cb[e]; wb[V + e] = nb[e]; }
        ca = na; cb = nb;
        kn = (kn + 1 == NV) ? 0 : kn + 1;
        na = vv[kn]; nb = wv[kn];
#pragma unroll
        for (int r = 0; r < G; ++r) {
            const int n = n0 + r;
            if (n < tp.F) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const double term = tp.h[n] * (double)wb[e + r * S] + tp.g[n] * (double)wa[e + r * S];
                    acc[e] = (n == 0) ? (T)term : (T)((double)acc[e] + term);
                }
            }
        }
    }
    return acc;
}

// ---- one-sided synthesis steps (the multiresolution analysis) -----------------------------------------------
// imodwt_step with one of its two inputs all zero: v0[t] = sum_n c[n] s[t + n*stride], c = tp.h (s holds details) or tp.g (s holds
// scaling coefficients).  Tap order, per-tap rounding and wrap-around of imodwt_point / imodwt_chunk_v / imodwt_chunk_s, restricted
// to the non-zero side: `c[n] * s + 0` is `c[n] * s` in Float64 up to the sign of a zero.
template <typename T, typename I>
__device__ __forceinline__ T imodwt1_point(const T *s, I N, I t, I stride, const double *c, int F)
{
    I k = t;
    T acc = (T)(c[0] * (double)s[k]);
    for (int n = 1; n < F; ++n) {
        k += stride;
        if (k >= N) { k -= N; if (k >= N) k %= N; }
        acc = (T)((double)acc + c[n] * (double)s[k]);
    }
    return acc;
}
template <typename T, typename I>
__device__ __forceinline__ Vec16<T> imodwt1_chunk_v(const T *s, I NV, I t, I strideV, const double *c, int F)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    const VT *sv = reinterpret_cast<const VT *>(s);
    I k = t;
    VT a = sv[k], acc;
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = (T)(c[0] * (double)a[e]);
    for (int n = 1; n < F; ++n) {
        k += strideV;
        if (k >= NV) { k -= NV; if (k >= NV) k %= NV; }
        a = sv[k];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = (T)((double)acc[e] + c[n] * (double)a[e]);
    }
    return acc;
}
// (S divides V, NV >= 2: the register pair [current chunk | next chunk] slides forward by one chunk per V / S taps)
template <typename T, int S, typename I>
__device__ __forceinline__ Vec16<T> imodwt1_chunk_s(const T *s, I NV, I t, const double *c, int F)
{
    constexpr int V = 16 / sizeof(T), G = V / S;
    typedef T VT __attribute__((ext_vector_type(V)));
    const VT *sv = reinterpret_cast<const VT *>(s);
    I kn = (t + 1 == NV) ? 0 : t + 1;
    VT ca = sv[t], na = sv[kn], acc;
    for (int n0 = 0; n0 < F; n0 += G) {
        T wa[2 * V];
#pragma unroll
        for (int e = 0; e < V; ++e) { wa[e] = ca[e]; wa[V + e] = na[e]; }
        ca = na;
        kn = (kn + 1 == NV) ? 0 : kn + 1;
        na = sv[kn];
#pragma unroll
        for (int r = 0; r < G; ++r) {
            const int n = n0 + r;
            if (n < F) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const double term = c[n] * (double)wa[e + r * S];
                    acc[e] = (n == 0) ? (T)term : (T)((double)acc[e] + term);
                }
            }
        }
    }
    return acc;
}

// the first index and the step of a grid-stride loop in x (taken in the kernel itself, where the block size is known to be uniform)
#define GRID_X_FIRST ((int64_t)blockIdx.x * blockDim.x + threadIdx.x)
#define GRID_X_THREADS ((int64_t)gridDim.x * blockDim.x)

// one level of one unit, grid-stride in x from t0 in steps of nthr: the bodies of the single-unit kernels and of their batched twins
// (k_*_b: the unit is blockIdx.y, the pointers are moved to it, nothing else differs)
template <typename T>
__device__ __forceinline__ void modwt_step_body(const T *__restrict__ v, T *__restrict__ v1, T *__restrict__ w1, int64_t N, int64_t stride,
                                                const ModwtTaps &tp, int64_t t0, int64_t nthr)
{
    for (int64_t t = t0; t < N; t += nthr) {
        T w, s;
        modwt_point<T, int64_t>(v, N, t, stride, tp, w, s);
        w1[t] = w;
        v1[t] = s;
    }
}
template <typename T>
__device__ __forceinline__ void imodwt_step_body(const T *__restrict__ v, const T *__restrict__ w, T *__restrict__ v0, int64_t N,
                                                 int64_t stride, const ModwtTaps &tp, int64_t t0, int64_t nthr)
{
    for (int64_t t = t0; t < N; t += nthr) v0[t] = imodwt_point<T, int64_t>(v, w, N, t, stride, tp);
}
template <typename T>
__device__ __forceinline__ void modwt_step_v_body(const T *__restrict__ v, T *__restrict__ v1, T *__restrict__ w1, int64_t NV,
                                                  int64_t strideV, const ModwtTaps &tp, int64_t t0, int64_t nthr)
{
    typedef Vec16<T> VT;
    for (int64_t t = t0; t < NV; t += nthr) {
        VT w, s;
        modwt_chunk_v<T, int64_t>(v, NV, t, strideV, tp, w, s);
        reinterpret_cast<VT *>(w1)[t] = w;
        reinterpret_cast<VT *>(v1)[t] = s;
    }
}
template <typename T>
__device__ __forceinline__ void imodwt_step_v_body(const T *__restrict__ v, const T *__restrict__ w, T *__restrict__ v0, int64_t NV,
                                                   int64_t strideV, const ModwtTaps &tp, int64_t t0, int64_t nthr)
{
    typedef Vec16<T> VT;
    for (int64_t t = t0; t < NV; t += nthr)
        reinterpret_cast<VT *>(v0)[t] = imodwt_chunk_v<T, int64_t>(v, w, NV, t, strideV, tp);
}
template <typename T, int S>
__device__ __forceinline__ void modwt_step_s_body(const T *__restrict__ v, T *__restrict__ v1, T *__restrict__ w1, int64_t NV,
                                                  const ModwtTaps &tp, int64_t t0, int64_t nthr)
{
    typedef Vec16<T> VT;
    for (int64_t t = t0; t < NV; t += nthr) {
        VT w, s;
        modwt_chunk_s<T, S, int64_t>(v, NV, t, tp, w, s);
        reinterpret_cast<VT *>(w1)[t] = w;
        reinterpret_cast<VT *>(v1)[t] = s;
    }
}
template <typename T, int S>
__device__ __forceinline__ void imodwt_step_s_body(const T *__restrict__ v, const T *__restrict__ w, T *__restrict__ v0, int64_t NV,
                                                   const ModwtTaps &tp, int64_t t0, int64_t nthr)
{
    typedef Vec16<T> VT;
    for (int64_t t = t0; t < NV; t += nthr)
        reinterpret_cast<VT *>(v0)[t] = imodwt_chunk_s<T, S, int64_t>(v, w, NV, t, tp);
}

template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_modwt_step(const T *__restrict__ v, T *__restrict__ v1, T *__restrict__ w1,
                                                            int64_t N, int64_t stride, ModwtTaps tp)
{
    modwt_step_body<T>(v, v1, w1, N, stride, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_imodwt_step(const T *__restrict__ v, const T *__restrict__ w, T *__restrict__ v0,
                                                             int64_t N, int64_t stride, ModwtTaps tp)
{
    imodwt_step_body<T>(v, w, v0, N, stride, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_modwt_step_v(const T *__restrict__ v, T *__restrict__ v1, T *__restrict__ w1,
                                                              int64_t NV, int64_t strideV, ModwtTaps tp)
{
    modwt_step_v_body<T>(v, v1, w1, NV, strideV, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_imodwt_step_v(const T *__restrict__ v, const T *__restrict__ w, T *__restrict__ v0,
                                                               int64_t NV, int64_t strideV, ModwtTaps tp)
{
    imodwt_step_v_body<T>(v, w, v0, NV, strideV, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T, int S>
__global__ void __launch_bounds__(EXT_THREADS) k_modwt_step_s(const T *__restrict__ v, T *__restrict__ v1, T *__restrict__ w1,
                                                              int64_t NV, ModwtTaps tp)
{
    modwt_step_s_body<T, S>(v, v1, w1, NV, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T, int S>
__global__ void __launch_bounds__(EXT_THREADS) k_imodwt_step_s(const T *__restrict__ v, const T *__restrict__ w, T *__restrict__ v0,
                                                               int64_t NV, ModwtTaps tp)
{
    imodwt_step_s_body<T, S>(v, w, v0, NV, tp, GRID_X_FIRST, GRID_X_THREADS);
}

// ---- the batched per-level tier: one launch per level over the units of a group, unit blockIdx.y at v + y * vs (and so on) ------
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_modwt_step_b(const T *__restrict__ v, int64_t vs, T *__restrict__ v1, int64_t v1s,
                                                              T *__restrict__ w1, int64_t w1s, int64_t N, int64_t stride, ModwtTaps tp)
{
    const int64_t u = blockIdx.y;
    modwt_step_body<T>(v + u * vs, v1 + u * v1s, w1 + u * w1s, N, stride, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_imodwt_step_b(const T *__restrict__ v, int64_t vs, const T *__restrict__ w, int64_t ws,
                                                               T *__restrict__ v0, int64_t v0s, int64_t N, int64_t stride, ModwtTaps tp)
{
    const int64_t u = blockIdx.y;
    imodwt_step_body<T>(v + u * vs, w + u * ws, v0 + u * v0s, N, stride, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_modwt_step_v_b(const T *__restrict__ v, int64_t vs, T *__restrict__ v1, int64_t v1s,
                                                                T *__restrict__ w1, int64_t w1s, int64_t NV, int64_t strideV, ModwtTaps tp)
{
    const int64_t u = blockIdx.y;
    modwt_step_v_body<T>(v + u * vs, v1 + u * v1s, w1 + u * w1s, NV, strideV, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_imodwt_step_v_b(const T *__restrict__ v, int64_t vs, const T *__restrict__ w, int64_t ws,
                                                                 T *__restrict__ v0, int64_t v0s, int64_t NV, int64_t strideV, ModwtTaps tp)
{
    const int64_t u = blockIdx.y;
    imodwt_step_v_body<T>(v + u * vs, w + u * ws, v0 + u * v0s, NV, strideV, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T, int S>
__global__ void __launch_bounds__(EXT_THREADS) k_modwt_step_s_b(const T *__restrict__ v, int64_t vs, T *__restrict__ v1, int64_t v1s,
                                                                T *__restrict__ w1, int64_t w1s, int64_t NV, ModwtTaps tp)
{
    const int64_t u = blockIdx.y;
    modwt_step_s_body<T, S>(v + u * vs, v1 + u * v1s, w1 + u * w1s, NV, tp, GRID_X_FIRST, GRID_X_THREADS);
}
template <typename T, int S>
__global__ void __launch_bounds__(EXT_THREADS) k_imodwt_step_s_b(const T *__restrict__ v, int64_t vs, const T *__restrict__ w, int64_t ws,
                                                                 T *__restrict__ v0, int64_t v0s, int64_t NV, ModwtTaps tp)
{
    const int64_t u = blockIdx.y;
    imodwt_step_s_body<T, S>(v + u * vs, w + u * ws, v0 + u * v0s, NV, tp, GRID_X_FIRST, GRID_X_THREADS);
}

// ---- the per-level tier of the multiresolution analysis: one one-sided step of the planes (unit, column) of
// a group.  Plane blockIdx.y is column c0 + y % ncnt of unit y / ncnt; it reads src + unit * sus + column * sld and writes dst
// likewise.  KIND: the function of modwt_lds_kind's numbering (0 point, 1 chunk_v, 2 chunk_s<1>, 3 chunk_s<2>); N counts elements,
// stride elements (KIND 0) or 16-byte chunks (KIND 1), already reduced mod the unit.
template <typename T, int KIND>
__global__ void __launch_bounds__(EXT_THREADS) k_modwt_mra_step_b(const T *__restrict__ src, int64_t sld, int64_t sus, T *__restrict__ dst,
                                                                  int64_t dld, int64_t dus, int c0, int ncnt, int64_t N, int64_t stride,
                                                                  int useh, ModwtTaps tp)
{
    constexpr int V = 16 / sizeof(T);
    typedef Vec16<T> VT;
    const unsigned y = blockIdx.y;
    const int64_t u = y / (unsigned)ncnt, c = c0 + (int64_t)(y % (unsigned)ncnt);
    const T *s = src + u * sus + c * sld;
    T *d = dst + u * dus + c * dld;
    const double *taps = useh ? tp.h : tp.g;
    const int64_t t0 = GRID_X_FIRST, nthr = GRID_X_THREADS;
    if (KIND == 0) {
        for (int64_t t = t0; t < N; t += nthr) d[t] = imodwt1_point<T, int64_t>(s, N, t, stride, taps, tp.F);
    } else {
        const int64_t NV = N / V;
        for (int64_t t = t0; t < NV; t += nthr) {
            if (KIND == 1) reinterpret_cast<VT *>(d)[t] = imodwt1_chunk_v<T, int64_t>(s, NV, t, stride, taps, tp.F);
            else if (KIND == 2) reinterpret_cast<VT *>(d)[t] = imodwt1_chunk_s<T, 1, int64_t>(s, NV, t, taps, tp.F);
            else reinterpret_cast<VT *>(d)[t] = imodwt1_chunk_s<T, (V == 4 ? 2 : 1), int64_t>(s, NV, t, taps, tp.F);
        }
    }
}

// ---- the LDS tier of the batch: every level of a short unit in one launch ------------------------------------
// which function a level of the LDS kernels takes, by the rules of the per-level dispatch (modwt_level): 1 chunk_v, 2 chunk_s<1>, 3 chunk_s<2>
// (Float32 only), 0 the point function (an unaligned batch, or a unit of one chunk)
template <typename T>
__device__ __forceinline__ int modwt_lds_kind(int vec, int64_t stride, int n)
{
    constexpr int V = 16 / sizeof(T);
    if (!vec) return 0;
    if ((stride % V) == 0) return 1;
    if (stride == 1 && n >= 2 * V) return 2;
    return (stride == 2 && V == 4 && n >= 2 * V) ? 3 : 0;
}
// A workgroup owns `upw` whole units at a time (more than one when a unit has fewer work items than the workgroup has threads)
// and walks the batch with a grid-stride loop.  The units are loaded into LDS buffer A; level j reads V from the current buffer
// with the wrap-around index of modwt_point / modwt_chunk_*, stores W to its global column and V to the other buffer (level L:
// to column L); one barrier between levels.  vec != 0: n, ldo, the unit strides and the bases are multiples of 16 bytes -- a
// work item is one 16-byte chunk (aligned 16-byte LDS reads of consecutive lanes, 16-byte global loads and stores) and the level
// takes the chunk function the per-level dispatch takes at that stride; otherwise a work item is one element.
constexpr int MODWT_LDS_BYTES = 65536;         // two buffers of one unit: n <= 8192 (Float32) / 4096 (Float64)
constexpr int MODWT_LDS_THREADS = 1024;

template <typename T>
__global__ void __launch_bounds__(MODWT_LDS_THREADS) k_modwt_lds(T *__restrict__ out, int64_t ldo, int64_t ous, const T *__restrict__ x,
                                                                 int64_t xs, int n, int64_t nunits, int L, int upw, int vec, ModwtTaps tp)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    extern __shared__ __attribute__((aligned(16))) char modwt_lds_mem[];
    T *bufA = reinterpret_cast<T *>(modwt_lds_mem), *bufB = bufA + (size_t)upw * n;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int ipu = vec ? n / V : n;                   // work items of one unit
    for (int64_t u0 = (int64_t)blockIdx.x * upw; u0 < nunits; u0 += (int64_t)gridDim.x * upw) {
        const int nu = (nunits - u0 < upw) ? (int)(nunits - u0) : upw;
        for (int i = tid; i < nu * ipu; i += nthr) {
            int slot = 0, c = i;
            if (upw > 1) { slot = i / ipu; c = i - slot * ipu; }
            const T *xu = x + (u0 + slot) * xs;
            if (vec) reinterpret_cast<VT *>(bufA + (size_t)slot * n)[c] = reinterpret_cast<const VT *>(xu)[c];
            else bufA[(size_t)slot * n + c] = xu[c];
        }
        __syncthreads();
        T *cur = bufA, *nxt = bufB;
        for (int j = 1; j <= L; ++j) {
            const int stride = 1 << (j - 1);           // < n: L <= floor(log2 n)
            const int kind = modwt_lds_kind<T>(vec, stride, n);
            // (vec with kind 0, n == V: the items of this level are elements)
            const int ipl = kind ? n / V : n;
            for (int i = tid; i < nu * ipl; i += nthr) {
                int slot = 0, c = i;
                if (upw > 1) { slot = i / ipl; c = i - slot * ipl; }
                const T *vsrc = cur + (size_t)slot * n;
                T *ou = out + (u0 + slot) * ous;
                T *vdst = (j == L) ? ou + (int64_t)L * ldo : nxt + (size_t)slot * n;
                T *wdst = ou + (int64_t)(j - 1) * ldo;
                if (kind == 0) {
                    T w, s;
                    modwt_point<T, int>(vsrc, n, c, stride, tp, w, s);
                    wdst[c] = w;
                    vdst[c] = s;
                } else {
                    VT w, s;
                    if (kind == 1) modwt_chunk_v<T, int>(vsrc, n / V, c, stride / V, tp, w, s);
                    else if (kind == 2) modwt_chunk_s<T, 1, int>(vsrc, n / V, c, tp, w, s);
                    else modwt_chunk_s<T, (V == 4 ? 2 : 1), int>(vsrc, n / V, c, tp, w, s);
                    reinterpret_cast<VT *>(wdst)[c] = w;
                    reinterpret_cast<VT *>(vdst)[c] = s;
                }
            }
            __syncthreads();
            T *sw = cur; cur = nxt; nxt = sw;
        }
    }
}
// the mirror image: column ncols - 1 of every unit into LDS; level j reads W's column from global memory and V from LDS and
// writes V of level j - 1 to the other buffer -- level 1 writes x.  ncols >= 2.  A stride 2^(j-1) may exceed n many times over
// (ncols is not bounded by n): it is reduced mod n once, which leaves every index what imodwt_point computes.
template <typename T>
__global__ void __launch_bounds__(MODWT_LDS_THREADS) k_imodwt_lds(T *__restrict__ x, int64_t xs, const T *__restrict__ xw, int64_t ldw,
                                                                  int64_t ws, int n, int64_t nunits, int ncols, int upw, int vec, ModwtTaps tp)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    extern __shared__ __attribute__((aligned(16))) char modwt_lds_mem[];
    T *bufA = reinterpret_cast<T *>(modwt_lds_mem), *bufB = bufA + (size_t)upw * n;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int ipu = vec ? n / V : n;
    for (int64_t u0 = (int64_t)blockIdx.x * upw; u0 < nunits; u0 += (int64_t)gridDim.x * upw) {
        const int nu = (nunits - u0 < upw) ? (int)(nunits - u0) : upw;
        for (int i = tid; i < nu * ipu; i += nthr) {
            int slot = 0, c = i;
            if (upw > 1) { slot = i / ipu; c = i - slot * ipu; }
            const T *vu = xw + (u0 + slot) * ws + (int64_t)(ncols - 1) * ldw;
            if (vec) reinterpret_cast<VT *>(bufA + (size_t)slot * n)[c] = reinterpret_cast<const VT *>(vu)[c];
            else bufA[(size_t)slot * n + c] = vu[c];
        }
        __syncthreads();
        T *cur = bufA, *nxt = bufB;
        for (int j = ncols - 1; j >= 1; --j) {
            const int64_t stride = (int64_t)1 << (j - 1);
            const int kind = modwt_lds_kind<T>(vec, stride, n);
            const int ipl = kind ? n / V : n;
            const int sred = (kind == 1) ? (int)((stride / V) % (n / V)) : (int)(stride % n);
            for (int i = tid; i < nu * ipl; i += nthr) {
                int slot = 0, c = i;
                if (upw > 1) { slot = i / ipl; c = i - slot * ipl; }
                const T *vsrc = cur + (size_t)slot * n;
                const T *wsrc = xw + (u0 + slot) * ws + (int64_t)(j - 1) * ldw;
                T *dst = (j == 1) ? x + (u0 + slot) * xs : nxt + (size_t)slot * n;
                if (kind == 0) dst[c] = imodwt_point<T, int>(vsrc, wsrc, n, c, sred, tp);
                else if (kind == 1) reinterpret_cast<VT *>(dst)[c] = imodwt_chunk_v<T, int>(vsrc, wsrc, n / V, c, sred, tp);
                else if (kind == 2) reinterpret_cast<VT *>(dst)[c] = imodwt_chunk_s<T, 1, int>(vsrc, wsrc, n / V, c, tp);
                else reinterpret_cast<VT *>(dst)[c] = imodwt_chunk_s<T, (V == 4 ? 2 : 1), int>(vsrc, wsrc, n / V, c, tp);
            }
            __syncthreads();
            T *sw = cur; cur = nxt; nxt = sw;
        }
    }
}

// ---- the LDS tier of the multiresolution analysis -------------------------------------------------------------
// A work unit is a plane (unit u, column c): column c of xw, one step with h at level c + 1 (the smooth, c = L: with g at level L),
// then steps with g down to level 1, which stores column c of out.  Planes are numbered p = q * nunits + u with q the column's rank
// by depth, column L - q: the smooth and D_L (L steps each) first, D_1 (one step) last.  A workgroup takes `ppw` consecutive planes
// at a time (modwt_lds_shape) and walks the planes with a grid-stride loop.  It runs levels s = first .. 1 of its pack, `first` the
// level its first (deepest) slot starts at, one barrier per level; a slot whose column starts below `first` (a pack that straddles a
// column boundary) is loaded into the buffer that is the source at its own first level and waits.  The slots are sorted by depth, so
// at level s those on g, those on h and those still waiting are three consecutive ranges with workgroup-uniform bounds: the taps stay
// a uniform (scalar) operand.  Access widths and chunk functions as in k_imodwt_lds.
// plane p0 + slot of the pack that starts at rank q0, unit u0 (slot < 1024)
__device__ __forceinline__ void mra_plane(int q0, int64_t u0, int slot, int64_t nunits, int &q, int64_t &u)
{
    q = q0;
    u = u0 + slot;
    if (u >= nunits) {
        u -= nunits;
        ++q;
        if (u >= nunits) { const int d = (int)u, nn = (int)nunits; q += d / nn; u = d % nn; }     // (nunits <= u < 1024 here)
    }
}
template <typename T>
__global__ void __launch_bounds__(MODWT_LDS_THREADS) k_modwt_mra_lds(T *__restrict__ out, int64_t ldo, int64_t ous, const T *__restrict__ xw,
                                                                     int64_t ldw, int64_t ws, int n, int64_t nunits, int ncols, int ppw, int vec,
                                                                     ModwtTaps tp)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    extern __shared__ __attribute__((aligned(16))) char modwt_lds_mem[];
    T *bufA = reinterpret_cast<T *>(modwt_lds_mem), *bufB = bufA + (size_t)ppw * n;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int L = ncols - 1;                           // >= 1
    const int64_t nplanes = nunits * ncols;
    const int ipu = vec ? n / V : n;                   // work items of one plane
    for (int64_t p0 = (int64_t)blockIdx.x * ppw; p0 < nplanes; p0 += (int64_t)gridDim.x * ppw) {
        const int np = (nplanes - p0 < ppw) ? (int)(nplanes - p0) : ppw;
        const int q0 = (int)(p0 / nunits);
        const int64_t u0 = p0 - (int64_t)q0 * nunits;
        const int first = (q0 == 0) ? L : L - q0 + 1;
        for (int i = tid; i < np * ipu; i += nthr) {
            int slot = 0, e = i;
            if (ppw > 1) { slot = i / ipu; e = i - slot * ipu; }
            int q;
            int64_t u;
            mra_plane(q0, u0, slot, nunits, q, u);
            const int start = (q == 0) ? L : L - q + 1;
            T *b = (((first - start) & 1) ? bufB : bufA) + (size_t)slot * n;
            const T *src = xw + u * ws + (int64_t)(L - q) * ldw;
            if (vec) reinterpret_cast<VT *>(b)[e] = reinterpret_cast<const VT *>(src)[e];
            else b[e] = src[e];
        }
        __syncthreads();
        T *cur = bufA, *nxt = bufB;
        for (int s = first; s >= 1; --s) {
            const int64_t stride = (int64_t)1 << (s - 1);
            const int kind = modwt_lds_kind<T>(vec, stride, n);
            // (vec with kind 0, n == V: the items of this level are elements)
            const int ipl = kind ? n / V : n;
            const int sred = (kind == 1) ? (int)((stride / V) % (n / V)) : (int)(stride % n);
            // slots [0, a): ranks below L - s + 1, on g; [a, b): rank L - s + 1, the column that enters at this level, on h
            const int64_t ra = (int64_t)(L - s + 1) * nunits - p0, rb = ra + nunits;
            const int a = ra < 0 ? 0 : (ra > np ? np : (int)ra), b = rb < 0 ? 0 : (rb > np ? np : (int)rb);
            auto items = [&](int i0, int i1, const double *taps) {
                for (int i = i0 + tid; i < i1; i += nthr) {
                    int slot = 0, e = i;
                    if (ppw > 1) { slot = i / ipl; e = i - slot * ipl; }
                    const T *src = cur + (size_t)slot * n;
                    T *dst = nxt + (size_t)slot * n;
                    if (s == 1) {
                        int q;
                        int64_t u;
                        mra_plane(q0, u0, slot, nunits, q, u);
                        dst = out + u * ous + (int64_t)(L - q) * ldo;
                    }
                    if (kind == 0) dst[e] = imodwt1_point<T, int>(src, n, e, sred, taps, tp.F);
                    else if (kind == 1) reinterpret_cast<VT *>(dst)[e] = imodwt1_chunk_v<T, int>(src, n / V, e, sred, taps, tp.F);
                    else if (kind == 2) reinterpret_cast<VT *>(dst)[e] = imodwt1_chunk_s<T, 1, int>(src, n / V, e, taps, tp.F);
                    else reinterpret_cast<VT *>(dst)[e] = imodwt1_chunk_s<T, (V == 4 ? 2 : 1), int>(src, n / V, e, taps, tp.F);
                }
            };
            items(0, a * ipl, tp.g);
            items(a * ipl, b * ipl, tp.h);
            __syncthreads();
            T *sw = cur; cur = nxt; nxt = sw;
        }
    }
}

// ---- the level loops -------------------------------------------------------------------------------------------------------
// every unit base of a group on a 16-byte boundary: what the chunk functions need (one unit: its strides do not matter)
template <typename T>
bool modwt_batch_vec(const T *x, int64_t xs, const T *m, int64_t ld, int64_t ms, int64_t N, int64_t nunits)
{
    constexpr int V = 16 / sizeof(T);
    return (N % V) == 0 && (ld % V) == 0 && vec_ok16(x) && vec_ok16(m) && (nunits == 1 || ((xs % V) == 0 && (ms % V) == 0));
}

// One level of nb units: the step kernel of a stride.  vec: modwt_batch_vec; small: option WL_MODWT_SMALL (the chunk_s kernels);
// single: the one unit of wl_modwt / wl_imodwt, on the kernels without a unit index (the k_*_b kernels at gridDim.y == 1 measured 1 %
// behind them on a Float32 imodwt of 2^22 samples, profiles/ext_drivers_refactor.md).
template <typename T>
void modwt_level(hipStream_t st, int cu_count, bool vec, bool small, bool single, int64_t nb, const T *v, int64_t vs, T *v1, int64_t v1s, T *w1,
                 int64_t w1s, int64_t N, int64_t stride, const ModwtTaps &tp)
{
    constexpr int V = 16 / sizeof(T), S2 = (sizeof(T) == 4 ? 2 : 1);
    const dim3 gv(ext_blocks(N / V, 1, cu_count), (unsigned)nb), gs(ext_blocks(N, 1, cu_count), (unsigned)nb), th(EXT_THREADS);
    auto launch = [&](auto k1, auto kb, dim3 grid, auto... extents) {
        if (single) hipLaunchKernelGGL(k1, grid, th, 0, st, v, v1, w1, extents..., tp);
        else hipLaunchKernelGGL(kb, grid, th, 0, st, v, vs, v1, v1s, w1, w1s, extents..., tp);
    };
    if (vec && (stride % V) == 0) launch(k_modwt_step_v<T>, k_modwt_step_v_b<T>, gv, N / V, stride / V);
    else if (vec && stride == 1 && N >= 2 * V && small) launch(k_modwt_step_s<T, 1>, k_modwt_step_s_b<T, 1>, gv, N / V);
    else if (vec && stride == 2 && V == 4 && N >= 2 * V && small) launch(k_modwt_step_s<T, S2>, k_modwt_step_s_b<T, S2>, gv, N / V);
    else launch(k_modwt_step<T>, k_modwt_step_b<T>, gs, N, stride);
}
template <typename T>
void imodwt_level(hipStream_t st, int cu_count, bool vec, bool small, bool single, int64_t nb, const T *v, int64_t vs, const T *w, int64_t ws, T *v0,
                  int64_t v0s, int64_t N, int64_t stride, const ModwtTaps &tp)
{
    constexpr int V = 16 / sizeof(T), S2 = (sizeof(T) == 4 ? 2 : 1);
    const dim3 gv(ext_blocks(N / V, 1, cu_count), (unsigned)nb), gs(ext_blocks(N, 1, cu_count), (unsigned)nb), th(EXT_THREADS);
    auto launch = [&](auto k1, auto kb, dim3 grid, auto... extents) {
        if (single) hipLaunchKernelGGL(k1, grid, th, 0, st, v, w, v0, extents..., tp);
        else hipLaunchKernelGGL(kb, grid, th, 0, st, v, vs, w, ws, v0, v0s, extents..., tp);
    };
    if (vec && (stride % V) == 0) launch(k_imodwt_step_v<T>, k_imodwt_step_v_b<T>, gv, N / V, stride / V);
    else if (vec && stride == 1 && N >= 2 * V && small) launch(k_imodwt_step_s<T, 1>, k_imodwt_step_s_b<T, 1>, gv, N / V);
    else if (vec && stride == 2 && V == 4 && N >= 2 * V && small) launch(k_imodwt_step_s<T, S2>, k_imodwt_step_s_b<T, S2>, gv, N / V);
    else launch(k_imodwt_step<T>, k_imodwt_step_b<T>, gs, N, stride);
}

// All L levels of the nb units of a group (unit u of x at u * xs, of out at u * ous): level j reads V from the previous level's buffer,
// stores W to column j - 1 and V to the other of the ping-pong buffers A / B (nb dense units each) -- level L: to column L.
template <typename T>
int modwt_levels(wl_ctx *ctx, hipStream_t st, bool vec, bool single, int64_t nb, T *out, int64_t ldo, int64_t ous, const T *x, int64_t xs, int64_t N, int L,
                 T *A, T *B, const ModwtTaps &tp)
{
    const bool small = opt("WL_MODWT_SMALL", 1) != 0;
    const T *cur = x;
    int64_t cs = xs;
    for (int j = 1; j <= L; ++j) {
        T *vdst = (j == L) ? out + (int64_t)L * ldo : ((j & 1) ? A : B);
        const int64_t vds = (j == L) ? ous : N;
        modwt_level<T>(st, ctx->cu_count, vec, small, single, nb, cur, cs, vdst, vds, out + (int64_t)(j - 1) * ldo, ous, N, (int64_t)1 << (j - 1), tp);
        WL_HIP(ctx, hipGetLastError());
        cur = vdst;
        cs = vds;
    }
    return WL_OK;
}
// the mirror image: V of column ncols - 1 and W of column j - 1 give V of level j - 1 -- level 1 writes x.  2 <= ncols <= 63.
template <typename T>
int imodwt_levels(wl_ctx *ctx, hipStream_t st, bool vec, bool single, int64_t nb, T *x, int64_t xs, const T *xw, int64_t ldw, int64_t ws, int64_t N, int ncols,
                  T *A, T *B, const ModwtTaps &tp)
{
    const bool small = opt("WL_MODWT_SMALL", 1) != 0;
    const T *cur = xw + (int64_t)(ncols - 1) * ldw;
    int64_t cs = ws;
    for (int j = ncols - 1; j >= 1; --j) {
        T *dst = (j == 1) ? x : ((j & 1) ? A : B);
        const int64_t ds = (j == 1) ? xs : N;
        imodwt_level<T>(st, ctx->cu_count, vec, small, single, nb, cur, cs, xw + (int64_t)(j - 1) * ldw, ws, dst, ds, N, (int64_t)1 << (j - 1), tp);
        WL_HIP(ctx, hipGetLastError());
        cur = dst;
        cs = ds;
    }
    return WL_OK;
}

// ---- modwt / imodwt of one vector: a group of one unit on the per-level tier, whatever its length (the options of the batch do not
// apply), with the single-unit kernels ----
template <typename T>
int modwt_impl(wl_ctx *ctx, hipStream_t st, T *out, int64_t ldo, const T *x, int64_t N, const double *qmf, int flen, int L)
{
    WL_TRY(wl_ensure_ws(ctx, (size_t)2 * N * sizeof(T), st, true));
    ModwtTaps tp;
    make_modwt_taps(qmf, flen, tp);
    T *A = (T *)ctx->ws;
    WL_TRY(modwt_levels<T>(ctx, st, modwt_batch_vec<T>(x, 0, out, ldo, 0, N, 1), true, 1, out, ldo, 0, x, 0, N, L, A, A + N, tp));
    ctx->last_kernel = "k_modwt_step";
    return WL_OK;
}
template <typename T>
int imodwt_impl(wl_ctx *ctx, hipStream_t st, T *x, const T *xw, int64_t ldw, int64_t N, int ncols, const double *qmf, int flen)
{
    WL_TRY(wl_ensure_ws(ctx, (size_t)2 * N * sizeof(T), st, true));
    ModwtTaps tp;
    make_modwt_taps(qmf, flen, tp);
    if (ncols == 1) {                                        // no level: the scaling column is the signal
        WL_HIP(ctx, hipMemcpyAsync(x, xw, (size_t)N * sizeof(T), hipMemcpyDeviceToDevice, st));
        return WL_OK;
    }
    if (ncols - 2 >= 62) return WL_EINVAL_L;                 // (the stride of the first level must fit an int64)
    T *A = (T *)ctx->ws;
    WL_TRY(imodwt_levels<T>(ctx, st, modwt_batch_vec<T>(x, 0, xw, ldw, 0, N, 1), true, 1, x, 0, xw, ldw, 0, N, ncols, A, A + N, tp));
    ctx->last_kernel = "k_imodwt_step";
    return WL_OK;
}

// ---- modwt / imodwt of a batch (wl_modwt_batch / wl_imodwt_batch) ------------------------------------------
// The launch shape of the LDS tier.  A unit has `items` work items per level (16-byte chunks, or elements); the workgroup has that
// many threads, at least EXT_THREADS and at most MODWT_LDS_THREADS, and takes threads / items whole units when a unit has fewer
// items than that, so that no lane idles on a panel of tiny units.
struct ModwtLdsShape { unsigned threads, grid; int upw; size_t lds; };
template <typename T>
ModwtLdsShape modwt_lds_shape(int64_t n, int64_t nunits, bool vec, int cu_count)
{
    const int64_t items = vec ? n / (int64_t)(16 / sizeof(T)) : n;
    int64_t threads = (items + 63) / 64 * 64;
    if (threads < EXT_THREADS) threads = EXT_THREADS;
    if (threads > MODWT_LDS_THREADS) threads = MODWT_LDS_THREADS;
    int64_t upw = items < threads ? threads / items : 1;
    if (upw > nunits) upw = nunits;
    int64_t grid = (nunits + upw - 1) / upw;
    if (grid > (int64_t)cu_count * 8) grid = (int64_t)cu_count * 8;        // the rest by the grid-stride loop
    return {(unsigned)threads, (unsigned)grid, (int)upw, (size_t)2 * upw * n * sizeof(T)};
}
template <typename T>
int modwt_batch_impl(wl_ctx *ctx, hipStream_t st, T *out, int64_t ldo, int64_t ous, const T *x, int64_t N, int64_t nunits, int64_t xs,
                     const double *qmf, int flen, int L)
{
    ModwtTaps tp;
    make_modwt_taps(qmf, flen, tp);
    const bool vec = modwt_batch_vec<T>(x, xs, out, ldo, ous, N, nunits);
    if (opt("WL_MODWT_FUSED", 1) != 0 && (size_t)2 * N * sizeof(T) <= (size_t)MODWT_LDS_BYTES) {
        const ModwtLdsShape sh = modwt_lds_shape<T>(N, nunits, vec, ctx->cu_count);
        hipLaunchKernelGGL((k_modwt_lds<T>), dim3(sh.grid), dim3(sh.threads), sh.lds, st, out, ldo, ous, x, xs, (int)N, nunits, L, sh.upw,
                           vec ? 1 : 0, tp);
        WL_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "k_modwt_lds";
        return WL_OK;
    }
    auto bytes = [&](int64_t G) { return (size_t)2 * G * N * sizeof(T); };
    const int64_t G = group_size(nunits, 65535, opt("WL_MODWT_BATCH_GROUP", 0), true, group_cap(), bytes);
    WL_TRY(wl_ensure_ws(ctx, bytes(G), st, true));
    T *A = (T *)ctx->ws, *B = A + G * N;
    WL_TRY(for_groups(nunits, G, [&](int64_t u0, int64_t nb) -> int {
        return modwt_levels<T>(ctx, st, vec, false, nb, out + u0 * ous, ldo, ous, x + u0 * xs, xs, N, L, A, B, tp);
    }));
    ctx->last_kernel = "k_modwt_step_b";
    return WL_OK;
}
template <typename T>
int imodwt_batch_impl(wl_ctx *ctx, hipStream_t st, T *x, int64_t xs, const T *xw, int64_t ldw, int64_t ws, int64_t N, int ncols,
                      int64_t nunits, const double *qmf, int flen)
{
    if (ncols == 1) {                                        // no level: the scaling column is the signal
        WL_HIP(ctx, hipMemcpy2DAsync(x, (size_t)xs * sizeof(T), xw, (size_t)ws * sizeof(T), (size_t)N * sizeof(T), (size_t)nunits,
                                     hipMemcpyDeviceToDevice, st));
        ctx->last_kernel = "copy";
        return WL_OK;
    }
    ModwtTaps tp;
    make_modwt_taps(qmf, flen, tp);
    const bool vec = modwt_batch_vec<T>(x, xs, xw, ldw, ws, N, nunits);
    if (opt("WL_MODWT_FUSED", 1) != 0 && (size_t)2 * N * sizeof(T) <= (size_t)MODWT_LDS_BYTES) {
        const ModwtLdsShape sh = modwt_lds_shape<T>(N, nunits, vec, ctx->cu_count);
        hipLaunchKernelGGL((k_imodwt_lds<T>), dim3(sh.grid), dim3(sh.threads), sh.lds, st, x, xs, xw, ldw, ws, (int)N, nunits, ncols, sh.upw,
                           vec ? 1 : 0, tp);
        WL_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "k_imodwt_lds";
        return WL_OK;
    }
    auto bytes = [&](int64_t G) { return (size_t)2 * G * N * sizeof(T); };
    const int64_t G = group_size(nunits, 65535, opt("WL_MODWT_BATCH_GROUP", 0), true, group_cap(), bytes);
    WL_TRY(wl_ensure_ws(ctx, bytes(G), st, true));
    T *A = (T *)ctx->ws, *B = A + G * N;
    WL_TRY(for_groups(nunits, G, [&](int64_t u0, int64_t nb) -> int {
        return imodwt_levels<T>(ctx, st, vec, false, nb, x + u0 * xs, xs, xw + u0 * ws, ldw, ws, N, ncols, A, B, tp);
    }));
    ctx->last_kernel = "k_imodwt_step_b";
    return WL_OK;
}

// the extent rules the two batch entry points share: unit u of the vectors at u * xs (>= n), of the matrices at u * ms, leading
// dimension ld (>= n), ms >= ld * cols; every product must fit an int64.  cols < 1 breaks a later rule, not this one.
int modwt_batch_dims(int64_t n, int64_t nunits, int64_t xs, int64_t ld, int64_t ms, int64_t cols)
{
    if (n < 1 || nunits < 1 || xs < n || ld < n) return WL_EDIMS;
    int64_t need = 0, tot = 0;
    if (cols >= 1 && (__builtin_mul_overflow(ld, cols, &need) || ms < need)) return WL_EDIMS;
    if (__builtin_mul_overflow(nunits, xs, &tot) || __builtin_mul_overflow(nunits, ms, &tot) || tot >= ((int64_t)1 << 60)) return WL_EDIMS;
    return WL_OK;
}
// the units of the vectors against the units of the matrices, as byte ranges (cols clamped to what the dims rule has seen)
bool modwt_batch_overlap(const void *x, int64_t xs, const void *m, int64_t ld, int64_t ms, int64_t n, int64_t nunits, int64_t cols, size_t sz)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(x), b0 = reinterpret_cast<uintptr_t>(m);
    const uintptr_t a1 = a0 + (uintptr_t)((nunits - 1) * xs + n) * sz;
    const uintptr_t b1 = b0 + (uintptr_t)((nunits - 1) * ms + (cols >= 1 ? cols - 1 : 0) * ld + n) * sz;
    return a0 < b1 && b0 < a1;
}

// ---- the multiresolution analysis of a batch (wl_modwt_mra_batch) ------------------------------------------
// One one-sided step of nb * ncnt planes on the per-level tier: columns c0 .. c0 + ncnt - 1 of nb units, by the rules of imodwt_level.
template <typename T>
void modwt_mra_level(hipStream_t st, int cu_count, bool vec, bool small, int64_t nb, const T *src, int64_t sld, int64_t sus, T *dst, int64_t dld,
                     int64_t dus, int c0, int ncnt, int64_t N, int64_t stride, bool useh, const ModwtTaps &tp)
{
    constexpr int V = 16 / sizeof(T);
    const unsigned ny = (unsigned)(nb * ncnt);
    const dim3 gv(ext_blocks(N / V, 1, cu_count), ny), gs(ext_blocks(N, 1, cu_count), ny), th(EXT_THREADS);
    auto launch = [&](auto k, dim3 grid, int64_t sred) {
        hipLaunchKernelGGL(k, grid, th, 0, st, src, sld, sus, dst, dld, dus, c0, ncnt, N, sred, useh ? 1 : 0, tp);
    };
    if (vec && (stride % V) == 0) launch(k_modwt_mra_step_b<T, 1>, gv, (stride / V) % (N / V));
    else if (vec && stride == 1 && N >= 2 * V && small) launch(k_modwt_mra_step_b<T, 2>, gv, 1);
    else if (vec && stride == 2 && V == 4 && N >= 2 * V && small) launch(k_modwt_mra_step_b<T, 3>, gv, 2);
    else launch(k_modwt_mra_step_b<T, 0>, gs, stride % N);
}
// Levels L .. 1 of the nb units of a group.  At level s column s - 1 enters with h from xw, and the columns s .. L that are under way
// (the smooth among them) take g from the buffer level s + 1 wrote -- at level L the smooth alone, from xw.  Level s writes buffer
// A (s odd) or B, plane (unit, column) at (unit * ncols + column) * N; level 1 writes out.
template <typename T>
int modwt_mra_levels(wl_ctx *ctx, hipStream_t st, bool vec, int64_t nb, T *out, int64_t ldo, int64_t ous, const T *xw, int64_t ldw, int64_t ws,
                     int64_t N, int ncols, T *A, T *B, const ModwtTaps &tp)
{
    const bool small = opt("WL_MODWT_SMALL", 1) != 0;
    const int L = ncols - 1;
    const int64_t pus = (int64_t)ncols * N;
    for (int s = L; s >= 1; --s) {
        const int64_t stride = (int64_t)1 << (s - 1);
        T *dst = (s == 1) ? out : ((s & 1) ? A : B);
        const T *prev = (s & 1) ? B : A;
        const int64_t dld = (s == 1) ? ldo : N, dus = (s == 1) ? ous : pus;
        modwt_mra_level<T>(st, ctx->cu_count, vec, small, nb, xw, ldw, ws, dst, dld, dus, s - 1, 1, N, stride, true, tp);
        WL_HIP(ctx, hipGetLastError());
        if (s == L) modwt_mra_level<T>(st, ctx->cu_count, vec, small, nb, xw, ldw, ws, dst, dld, dus, L, 1, N, stride, false, tp);
        else modwt_mra_level<T>(st, ctx->cu_count, vec, small, nb, prev, N, pus, dst, dld, dus, s, L - s + 1, N, stride, false, tp);
        WL_HIP(ctx, hipGetLastError());
    }
    return WL_OK;
}
template <typename T>
int modwt_mra_batch_impl(wl_ctx *ctx, hipStream_t st, T *out, int64_t ldo, int64_t ous, const T *xw, int64_t ldw, int64_t ws, int64_t N,
                         int ncols, int64_t nunits, const double *qmf, int flen)
{
    if (ncols == 1) {                                        // no level: the smooth is the scaling column
        WL_HIP(ctx, hipMemcpy2DAsync(out, (size_t)ous * sizeof(T), xw, (size_t)ws * sizeof(T), (size_t)N * sizeof(T), (size_t)nunits,
                                     hipMemcpyDeviceToDevice, st));
        ctx->last_kernel = "copy";
        return WL_OK;
    }
    ModwtTaps tp;
    make_modwt_taps(qmf, flen, tp);
    const bool vec = modwt_batch_vec<T>(out, ous, xw, ldw, ws, N, nunits) && (ldo % (int64_t)(16 / sizeof(T))) == 0;
    if (opt("WL_MODWT_FUSED", 1) != 0 && (size_t)2 * N * sizeof(T) <= (size_t)MODWT_LDS_BYTES) {
        const ModwtLdsShape sh = modwt_lds_shape<T>(N, nunits * ncols, vec, ctx->cu_count);
        hipLaunchKernelGGL((k_modwt_mra_lds<T>), dim3(sh.grid), dim3(sh.threads), sh.lds, st, out, ldo, ous, xw, ldw, ws, (int)N, nunits, ncols,
                           sh.upw, vec ? 1 : 0, tp);
        WL_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "k_modwt_mra_lds";
        return WL_OK;
    }
    auto bytes = [&](int64_t G) { return (size_t)2 * G * ncols * N * sizeof(T); };
    const int64_t G = group_size(nunits, 65535 / ncols, opt("WL_MODWT_BATCH_GROUP", 0), true, group_cap(), bytes);
    WL_TRY(wl_ensure_ws(ctx, bytes(G), st, true));
    T *A = (T *)ctx->ws, *B = A + G * ncols * N;
    WL_TRY(for_groups(nunits, G, [&](int64_t u0, int64_t nb) -> int {
        return modwt_mra_levels<T>(ctx, st, vec, nb, out + u0 * ous, ldo, ous, xw + u0 * ws, ldw, ws, N, ncols, A, B, tp);
    }));
    ctx->last_kernel = "k_modwt_mra_step_b";
    return WL_OK;
}
// the units of two coefficient tensors as byte ranges (cols clamped to what the dims rule has seen)
bool modwt_mats_overlap(const void *a, int64_t lda, int64_t as, const void *b, int64_t ldb, int64_t bs, int64_t n, int64_t nunits, int64_t cols,
                        size_t sz)
{
    const int64_t lastc = cols >= 1 ? cols - 1 : 0;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t a1 = a0 + (uintptr_t)((nunits - 1) * as + lastc * lda + n) * sz;
    const uintptr_t b1 = b0 + (uintptr_t)((nunits - 1) * bs + lastc * ldb + n) * sz;
    return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" {

int wl_maxmodwttransformlevels(int64_t n)
{
    int l = 0;
    while (n > 1) { n >>= 1; ++l; }
    return l;
}

int wl_modwt(wl_ctx *ctx, int dtype, void *out, int64_t ldo, const void *x, int64_t n, const double *qmf, int flen, int L,
             void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!out || !x || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_flen(flen, 1));
    if (n < 1 || ldo < n) return WL_EDIMS;
    if (L > wl_maxmodwttransformlevels(n)) return WL_EINVAL_SIZE;      // "Too many transform levels (length(x) < 2^L)"
    if (L < 1) return WL_EINVAL_L;                                       // "L must be >= 1"
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return modwt_impl<T>(ctx, st, (T *)out, ldo, (const T *)x, n, qmf, flen, L);
    });
}

int wl_imodwt(wl_ctx *ctx, int dtype, void *x, const void *xw, int64_t ldw, int64_t n, int ncols, const double *qmf, int flen,
              void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!x || !xw || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_flen(flen, 1));
    if (n < 1 || ncols < 1 || ldw < n) return WL_EDIMS;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return imodwt_impl<T>(ctx, st, (T *)x, (const T *)xw, ldw, n, ncols, qmf, flen);
    });
}

int wl_modwt_batch(wl_ctx *ctx, int dtype, void *out, int64_t ldo, int64_t out_unit_stride, const void *x, int64_t n, int64_t nunits,
                   int64_t unit_stride, const double *qmf, int flen, int L, void *stream)
{
    if (!ctx || !out || !x || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen, 1));
    WL_TRY(modwt_batch_dims(n, nunits, unit_stride, ldo, out_unit_stride, (int64_t)L + 1));
    if (modwt_batch_overlap(x, unit_stride, out, ldo, out_unit_stride, n, nunits, (int64_t)L + 1, dtype == WL_F32 ? 4 : 8)) return WL_EALIAS;
    if (L > wl_maxmodwttransformlevels(n)) return WL_EINVAL_SIZE;      // "Too many transform levels (length(x) < 2^L)"
    if (L < 1) return WL_EINVAL_L;                                       // "L must be >= 1"
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return modwt_batch_impl<T>(ctx, st, (T *)out, ldo, out_unit_stride, (const T *)x, n, nunits, unit_stride, qmf, flen, L);
    });
}

int wl_imodwt_batch(wl_ctx *ctx, int dtype, void *x, int64_t unit_stride, const void *xw, int64_t ldw, int64_t xw_unit_stride, int64_t n,
                    int ncols, int64_t nunits, const double *qmf, int flen, void *stream)
{
    if (!ctx || !x || !xw || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen, 1));
    WL_TRY(modwt_batch_dims(n, nunits, unit_stride, ldw, xw_unit_stride, ncols));
    if (modwt_batch_overlap(x, unit_stride, xw, ldw, xw_unit_stride, n, nunits, ncols, dtype == WL_F32 ? 4 : 8)) return WL_EALIAS;
    if (ncols < 1 || ncols - 1 > 62) return WL_EINVAL_L;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return imodwt_batch_impl<T>(ctx, st, (T *)x, unit_stride, (const T *)xw, ldw, xw_unit_stride, n, ncols, nunits, qmf, flen);
    });
}

int wl_modwt_mra_batch(wl_ctx *ctx, int dtype, void *out, int64_t ldo, int64_t out_unit_stride, const void *xw, int64_t ldw,
                       int64_t xw_unit_stride, int64_t n, int ncols, int64_t nunits, const double *qmf, int flen, void *stream)
{
    if (!ctx || !out || !xw || !qmf) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen, 1));
    WL_TRY(modwt_batch_dims(n, nunits, n, ldo, out_unit_stride, ncols));
    WL_TRY(modwt_batch_dims(n, nunits, n, ldw, xw_unit_stride, ncols));
    if (modwt_mats_overlap(out, ldo, out_unit_stride, xw, ldw, xw_unit_stride, n, nunits, ncols, dtype == WL_F32 ? 4 : 8)) return WL_EALIAS;
    if (ncols < 1 || ncols - 1 > 62) return WL_EINVAL_L;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return modwt_mra_batch_impl<T>(ctx, st, (T *)out, ldo, out_unit_stride, (const T *)xw, ldw, xw_unit_stride, n, ncols, nunits, qmf, flen);
    });
}

}  // extern "C"

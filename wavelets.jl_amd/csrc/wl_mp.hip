// wl_mp.hip -- matchingpursuit (src/Threshold/basis_functions.jl:8-55): greedy pursuit over a finite dictionary, and the three
// primitives every pursuit loop is made of.
//
//   r = x;  y = 0;  while nrm(r) > tol && it < cap:  ftr = ft(r);  i = findmaxabs(ftr);  aphi = f(ftr[i] e_i);  r = T(r - aphi);
//                                                    y[i] = T(y[i] + ftr[i]);  it += 1
//
// findmaxabs is the reference's loop: the first index whose magnitude is strictly greater than every earlier one.  Here every
// element gets the key |v| (a NaN: -1, below every magnitude) and candidates are ordered by (key descending, index ascending) -- a
// total order, so the answer does not depend on how lanes, waves and workgroups combine.  v[0] NaN gives 0 (nothing compares
// greater than NaN), as does an all-NaN vector.
//
// nrm(r) = (double)(T)sqrt(s), s the Float64 sum of squares in a fixed order (lane-strided partials, a fixed butterfly, workgroup
// partials folded lane-strided by one wave): the accuracy contract of DESIGN.md section 11, deterministic for a given grid.  It is
// the one place where the loop is not the reference bit for bit, and it only gates termination.
//
// Workgroups combine at launch boundaries only: a part kernel writes one partial per workgroup, a one-workgroup fold kernel reads
// them.  A vector of at most MP_ONE elements takes the fold launch alone.
//
// The fast path of wl_matchingpursuit_filter is a union of orthonormal wavelet bases: ft = the forward transforms of the level
// loops every filter entry point runs (filter_fwd_levels, wl_fast.h), f = the one inverse transform of the base the atom is in.
#include "wl_entry.h"

#include <cmath>
#include <mutex>
#include <set>
#include <string>
#include <vector>

using namespace wl;

namespace {

constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / 64;
constexpr int64_t MP_ONE = 4096;         // elements one workgroup takes in the fold launch alone (16 per lane)
constexpr int64_t MP_PER_LANE = 16;      // elements per lane the grid is sized for
constexpr int64_t MP_GRID_MAX = 65536;   // upper end of option WL_MP_MAX_BLOCKS

// {idx, sumsq, nrm}: what the host reads back once per atom
struct MPState { long long idx; double sumsq, nrm; };

template <typename T>
struct MPBest { T key; long long idx; };

template <typename T>
__device__ __forceinline__ T mp_key(T v) { return v != v ? T(-1) : (v < T(0) ? -v : v); }

// a strictly greater key replaces; an equal key keeps the lower index
template <typename T>
__device__ __forceinline__ void mp_take(MPBest<T> &b, T k, long long i)
{
    if (k > b.key || (k == b.key && i < b.idx)) { b.key = k; b.idx = i; }
}

// the workgroup's best in thread 0: shuffles across the wave, the wave partials through LDS
template <typename T>
__device__ __forceinline__ MPBest<T> mp_block_best(MPBest<T> b)
{
    __shared__ T skey[MP_WAVES];
    __shared__ long long sidx[MP_WAVES];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T k = __shfl_xor(b.key, o, 64);
        const long long i = __shfl_xor(b.idx, o, 64);
        mp_take(b, k, i);
    }
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) { skey[wave] = b.key; sidx[wave] = b.idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < MP_WAVES; ++w) mp_take(b, skey[w], sidx[w]);
    return b;
}

// the workgroup's sum in thread 0: a fixed butterfly across the wave, the wave partials added in wave order
__device__ __forceinline__ double mp_block_sum(double acc)
{
    __shared__ double ssum[MP_WAVES];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) ssum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        acc = ssum[0];
        for (int w = 1; w < MP_WAVES; ++w) acc += ssum[w];
    }
    return acc;
}

// One (key, idx) pair per workgroup.  A lane meets its elements in ascending index order -- the `head` elements in front of the
// first 16-byte boundary, then 16-byte vectors, then the tail -- so "strictly greater replaces" leaves it the lowest index of
// its greatest key.
template <typename T>
__global__ __launch_bounds__(MP_THREADS) void k_mp_absmax_part(const T *__restrict__ v, int64_t len, int64_t head, double *__restrict__ pkey,
                                                               long long *__restrict__ pidx)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    const int64_t nthr = (int64_t)gridDim.x * MP_THREADS, gid = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
    MPBest<T> b = {T(-2), INT64_MAX};
    if (gid < head) {
        const T k = mp_key(v[gid]);
        if (k > b.key) { b.key = k; b.idx = gid; }
    }
    const int64_t nvec = (len - head) / V;
    const VT *vb = reinterpret_cast<const VT *>(v + head);
    for (int64_t q = gid; q < nvec; q += nthr) {
        const VT x = vb[q];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const T k = mp_key(x[j]);
            if (k > b.key) { b.key = k; b.idx = head + q * V + j; }
        }
    }
    for (int64_t t = head + nvec * V + gid; t < len; t += nthr) {
        const T k = mp_key(v[t]);
        if (k > b.key) { b.key = k; b.idx = t; }
    }
    b = mp_block_best(b);
    if (threadIdx.x == 0) { pkey[blockIdx.x] = (double)b.key; pidx[blockIdx.x] = b.idx; }
}

// One workgroup: the best of the nparts partials (nparts == 0: of v itself, len <= MP_ONE), v[0] NaN -> 0, *idx_out = the index.
// With spat / y (v is then ftr) the select follows: spat[idx % n] = ftr[idx], y[idx] = T(y[idx] + ftr[idx]) -- unless gate is
// given and !(gate->nrm > tol): the loop has ended, the index is written and nothing else.
template <typename T>
__global__ __launch_bounds__(MP_THREADS) void k_mp_absmax_fold(const T *__restrict__ v, int64_t len, const double *__restrict__ pkey,
                                                               const long long *__restrict__ pidx, int64_t nparts, long long *idx_out,
                                                               T *__restrict__ spat, int64_t n, T *__restrict__ y, const MPState *gate, double tol)
{
    MPBest<double> b = {-2.0, INT64_MAX};
    if (nparts == 0) {
        for (int64_t t = threadIdx.x; t < len; t += MP_THREADS) mp_take(b, (double)mp_key(v[t]), (long long)t);
    } else {
        for (int64_t p = threadIdx.x; p < nparts; p += MP_THREADS) mp_take(b, pkey[p], pidx[p]);
    }
    b = mp_block_best(b);
    if (threadIdx.x == 0) {
        const T v0 = v[0];
        const long long i = (v0 != v0) ? 0 : b.idx;
        *idx_out = i;
        if (spat && (!gate || gate->nrm > tol)) {
            const T c = v[i];
            spat[i % n] = c;
            y[i] = (T)(y[i] + c);
        }
    }
}

// the select alone, from an index in device memory (wl_mp_select); an index outside [0, ncoef) selects nothing
template <typename T>
__global__ void k_mp_select(T *__restrict__ spat, int64_t n, T *__restrict__ y, const T *__restrict__ ftr, int64_t ncoef,
                            const long long *__restrict__ idx_dev)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long i = *idx_dev;
    if (i < 0 || i >= ncoef) return;
    const T c = ftr[i];
    spat[i % n] = c;
    y[i] = (T)(y[i] + c);
}

// r[t] = T(r[t] - aphi[t]) (aphi == nullptr: r is only read) and the workgroup's Float64 sum of r[t]^2; one workgroup: the
// state is written here.  Thread 0 of workgroup 0 clears the spike spat[*idx_dev % spat_len] (its reader, the inverse transform,
// is an earlier launch).
template <typename T>
__global__ __launch_bounds__(MP_THREADS) void k_mp_residual_part(T *__restrict__ r, const T *__restrict__ aphi, int64_t n, int vec,
                                                                 T *__restrict__ spat, int64_t spat_len, const long long *__restrict__ idx_dev,
                                                                 double *__restrict__ part, MPState *__restrict__ state)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    const int64_t nthr = (int64_t)gridDim.x * MP_THREADS, gid = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
    double acc = 0.0;
    const int64_t nvec = vec ? n / V : 0;
    VT *rv = reinterpret_cast<VT *>(r);
    const VT *av = reinterpret_cast<const VT *>(aphi);
    for (int64_t q = gid; q < nvec; q += nthr) {
        VT x = rv[q];
        if (aphi) {
            const VT a = av[q];
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = (T)(x[j] - a[j]);
            rv[q] = x;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) acc += (double)x[j] * (double)x[j];
    }
    for (int64_t t = nvec * V + gid; t < n; t += nthr) {
        T x = r[t];
        if (aphi) {
            x = (T)(x - aphi[t]);
            r[t] = x;
        }
        acc += (double)x * (double)x;
    }
    if (gid == 0 && spat && idx_dev) {
        const long long i = *idx_dev;
        if (i >= 0) spat[i % spat_len] = T(0);
    }
    acc = mp_block_sum(acc);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) { state->sumsq = acc; state->nrm = (double)(T)sqrt(acc); }
        else part[blockIdx.x] = acc;
    }
}

// one wave: the partials lane-strided in index order, a fixed butterfly; {sumsq, nrm} with the norm rounded to the element type
__global__ __launch_bounds__(64) void k_mp_residual_fold(const double *__restrict__ part, int64_t nparts, int f32, MPState *__restrict__ state)
{
    double acc = 0.0;
    for (int64_t p = threadIdx.x; p < nparts; p += 64) acc += part[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (threadIdx.x == 0) {
        state->sumsq = acc;
        state->nrm = f32 ? (double)(float)sqrt(acc) : sqrt(acc);
    }
}

// ---- launch geometry --------------------------------------------------------------------------------------------------------
// the cap on a part kernel's grid: option WL_MP_MAX_BLOCKS, default 4 workgroups per CU
inline int64_t mp_grid_cap(const wl_ctx *ctx)
{
    int64_t cap = (int64_t)opt("WL_MP_MAX_BLOCKS", (long long)ctx->cu_count * 4);
    if (cap < 1) cap = 1;
    return cap > MP_GRID_MAX ? MP_GRID_MAX : cap;
}
inline int64_t mp_blocks(int64_t len, int64_t cap)
{
    const int64_t per = (int64_t)MP_THREADS * MP_PER_LANE;
    const int64_t b = (len + per - 1) / per;
    return b < 1 ? 1 : (b > cap ? cap : b);
}

// the scratch of the reductions, carved from 256-byte aligned memory: cap partial keys, indices and sums, and the state
struct MPScratch {
    double *pkey;
    long long *pidx;
    double *psum;
    MPState *state;
};
inline size_t mp_scratch_bytes(int64_t cap) { return up256((size_t)cap * 8) * 3 + 256; }
inline MPScratch mp_scratch(void *base, int64_t cap)
{
    char *p = (char *)base;
    const size_t each = up256((size_t)cap * 8);
    return {(double *)p, (long long *)(p + each), (double *)(p + 2 * each), (MPState *)(p + 3 * each)};
}

// idx_out = findmaxabs(v) (and the select when spat is given): one launch up to MP_ONE elements, else part + fold
template <typename T>
hipError_t mp_absmax(hipStream_t st, const T *v, int64_t len, const MPScratch &s, int64_t cap, long long *idx_out, T *spat, int64_t n, T *y,
                     const MPState *gate, double tol)
{
    if (len <= MP_ONE) {
        hipLaunchKernelGGL((k_mp_absmax_fold<T>), dim3(1), dim3(MP_THREADS), 0, st, v, len, (const double *)nullptr, (const long long *)nullptr,
                           (int64_t)0, idx_out, spat, n, y, gate, tol);
        return hipGetLastError();
    }
    const int64_t nb = mp_blocks(len, cap);
    const uintptr_t mis = (uintptr_t)v % 16;
    // (a pointer that is no multiple of the element size never reaches a 16-byte boundary: elements only)
    int64_t head = (mis % sizeof(T)) ? len : (int64_t)(((16 - mis) % 16) / sizeof(T));
    if (head > len) head = len;
    hipLaunchKernelGGL((k_mp_absmax_part<T>), dim3((unsigned)nb), dim3(MP_THREADS), 0, st, v, len, head, s.pkey, s.pidx);
    hipLaunchKernelGGL((k_mp_absmax_fold<T>), dim3(1), dim3(MP_THREADS), 0, st, v, len, (const double *)s.pkey, (const long long *)s.pidx, nb, idx_out,
                       spat, n, y, gate, tol);
    return hipGetLastError();
}

// r -= aphi (aphi == nullptr: nothing is written), state = {sum of r^2, nrm}, the spike of spat cleared
template <typename T>
hipError_t mp_residual(hipStream_t st, T *r, const T *aphi, int64_t n, T *spat, int64_t spat_len, const long long *idx_dev, const MPScratch &s,
                       int64_t cap)
{
    const int64_t nb = mp_blocks(n, cap);
    const int vec = ((uintptr_t)r % 16 == 0) && (!aphi || (uintptr_t)aphi % 16 == 0);
    hipLaunchKernelGGL((k_mp_residual_part<T>), dim3((unsigned)nb), dim3(MP_THREADS), 0, st, r, aphi, n, vec, spat, spat_len, idx_dev, s.psum, s.state);
    if (nb > 1) hipLaunchKernelGGL(k_mp_residual_fold, dim3(1), dim3(64), 0, st, (const double *)s.psum, nb, sizeof(T) == 4 ? 1 : 0, s.state);
    return hipGetLastError();
}

// one base of the dictionary: the transform of a vector of n with the level loops of the filter entry points (L == 0: a copy)
template <typename T>
int mp_transform(wl_ctx *ctx, hipStream_t st, int64_t n, T *y, const T *x, const Taps<T> &taps, int L, int fw, const char **kn)
{
    BoxSpec b;
    b.nd = 1; b.nt = 1;
    b.dims[0] = n; b.dims[1] = 1; b.dims[2] = 1;
    b.full = dense_strides(b.dims);
    if (L == 0) {
        const Extent3 ext = {{n, 1, 1}};
        WL_HIP(ctx, generic_copy_box<T>(st, x, b.full, y, b.full, ext));
        *kn = "copy";
        return WL_OK;
    }
    // (the whole transform workspace is held: no level can ask for more)
    const int rc = fw ? filter_fwd_levels<T>(ctx->ws, true, ctx->cu_count, ctx->path, st, b, y, x, taps, L, kn, &ctx->last_hip)
                      : filter_inv_levels<T>(ctx->ws, true, ctx->cu_count, ctx->path, st, b, y, x, taps, L, kn, &ctx->last_hip);
    return rc == WL_RETRY_GEN ? WL_EINVAL_ARG : rc;
}

// "matchingpursuit+<inner forward kernel>": wl_last_kernel hands out pointers that must outlive the call, so each distinct name
// (one per forward kernel family) is kept for the life of the library
inline const char *mp_kernel_name(const char *inner)
{
    static std::mutex mu;
    static std::set<std::string> names;
    std::lock_guard<std::mutex> lock(mu);
    return names.insert(std::string("matchingpursuit+") + (inner ? inner : "none")).first->c_str();
}

template <typename T>
int matchingpursuit_impl(wl_ctx *ctx, hipStream_t st, T *y, T *r, int64_t n, int nbases, const double *qmfs, const int *flens, const int *Ls,
                         double tol, int64_t nmax, int64_t *niter, double *nrm)
{
    const int64_t N = (int64_t)nbases * n;
    const int64_t gcap = mp_grid_cap(ctx);
    // workspace: the transforms' own region | ftr (N) | spat (n) | aphi (n) | the reductions' scratch
    const size_t tw = up256(ws_elems(n, 1) * sizeof(T)), fb = up256((size_t)N * sizeof(T)), vb = up256((size_t)n * sizeof(T));
    WL_TRY(wl_ensure_ws(ctx, tw + fb + 2 * vb + mp_scratch_bytes(gcap), st, true));
    char *base = (char *)ctx->ws;
    T *ftr = (T *)(base + tw), *spat = (T *)(base + tw + fb), *aphi = (T *)(base + tw + fb + vb);
    const MPScratch s = mp_scratch(base + tw + fb + 2 * vb, gcap);

    std::vector<Taps<T>> taps((size_t)nbases);
    {
        const double *q = qmfs;
        for (int k = 0; k < nbases; ++k) {
            make_taps<T>(q, flens[k], taps[(size_t)k]);
            q += flens[k];
        }
    }
    WL_HIP(ctx, hipMemsetAsync(y, 0, (size_t)N * sizeof(T), st));
    WL_HIP(ctx, hipMemsetAsync(spat, 0, (size_t)n * sizeof(T), st));
    WL_HIP(ctx, mp_residual<T>(st, r, (const T *)nullptr, n, (T *)nullptr, 0, nullptr, s, gcap));

    const int64_t cap = (nmax == -1) ? N : nmax;
    const char *kn = "none";
    MPState h = {0, 0.0, 0.0};
    int64_t it = 0;
    bool fresh = false;                                     // h holds the state behind the last residual update
    while (it < cap) {
        for (int k = 0; k < nbases; ++k) {
            const char *k1 = nullptr;
            WL_TRY(mp_transform<T>(ctx, st, n, ftr + (int64_t)k * n, r, taps[(size_t)k], Ls[k], 1, &k1));
            if (k == 0 && k1) kn = k1;
        }
        // the arg-max and the select, the latter only if the loop goes on (the norm of the previous update, on the device)
        WL_HIP(ctx, mp_absmax<T>(st, ftr, N, s, gcap, &s.state->idx, spat, n, y, s.state, tol));
        WL_HIP(ctx, hipMemcpyAsync(&h, s.state, sizeof(MPState), hipMemcpyDeviceToHost, st));
        WL_HIP(ctx, hipStreamSynchronize(st));
        fresh = true;
        if (!(h.nrm > tol)) break;                          // (a NaN norm ends the loop)
        if (h.idx < 0 || h.idx >= N) return WL_EINVAL_ARG;  // (not reached: the arg-max of N elements)
        const int kb = (int)(h.idx / n);
        const char *k2 = nullptr;
        WL_TRY(mp_transform<T>(ctx, st, n, aphi, spat, taps[(size_t)kb], Ls[kb], 0, &k2));
        WL_HIP(ctx, mp_residual<T>(st, r, aphi, n, spat, n, &s.state->idx, s, gcap));
        ++it;
        fresh = false;
    }
    if (!fresh) {
        WL_HIP(ctx, hipMemcpyAsync(&h, s.state, sizeof(MPState), hipMemcpyDeviceToHost, st));
        WL_HIP(ctx, hipStreamSynchronize(st));
    }
    *niter = it;
    *nrm = h.nrm;
    ctx->last_kernel = mp_kernel_name(kn);
    return WL_OK;
}

// the scratch of a primitive: the head of the workspace
inline int mp_primitive_scratch(wl_ctx *ctx, hipStream_t st, int64_t gcap, MPScratch &s)
{
    WL_TRY(wl_ensure_ws(ctx, mp_scratch_bytes(gcap), st, true));
    s = mp_scratch(ctx->ws, gcap);
    return WL_OK;
}

inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" {

int wl_findmaxabs(wl_ctx *ctx, int dtype, const void *v, int64_t len, int64_t *idx_dev, void *stream)
{
    if (!ctx || !v || !idx_dev) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (len < 1) return WL_EDIMS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const int64_t gcap = mp_grid_cap(ctx);
        MPScratch s = {};
        if (len > MP_ONE) WL_TRY(mp_primitive_scratch(ctx, st, gcap, s));
        WL_HIP(ctx, mp_absmax<T>(st, (const T *)v, len, s, gcap, (long long *)idx_dev, (T *)nullptr, 1, (T *)nullptr, nullptr, 0.0));
        ctx->last_kernel = len > MP_ONE ? "k_mp_absmax_part" : "k_mp_absmax_fold";
        return (int)WL_OK;
    });
}

int wl_mp_select(wl_ctx *ctx, int dtype, void *spat, int64_t n, void *y, const void *ftr, int64_t ncoef, const int64_t *idx_dev, void *stream)
{
    if (!ctx || !spat || !y || !ftr || !idx_dev) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (n < 1 || ncoef < 1 || ncoef % n != 0) return WL_EDIMS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_mp_select<T>), dim3(1), dim3(64), 0, st, (T *)spat, n, (T *)y, (const T *)ftr, ncoef, (const long long *)idx_dev);
        WL_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "k_mp_select";
        return (int)WL_OK;
    });
}

int wl_mp_residual(wl_ctx *ctx, int dtype, void *r, const void *aphi, int64_t n, void *spat, int64_t spat_len, const int64_t *idx_dev, double *nrm,
                   void *stream)
{
    if (!ctx || !r || !nrm || (spat && !idx_dev)) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (n < 1 || (spat_len != 0 && spat_len != n) || (spat && spat_len == 0)) return WL_EDIMS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        const int64_t gcap = mp_grid_cap(ctx);
        MPScratch s = {};
        WL_TRY(mp_primitive_scratch(ctx, st, gcap, s));
        WL_HIP(ctx, mp_residual<T>(st, (T *)r, (const T *)aphi, n, (T *)spat, spat_len, (const long long *)idx_dev, s, gcap));
        MPState h = {0, 0.0, 0.0};
        WL_HIP(ctx, hipMemcpyAsync(&h, s.state, sizeof(MPState), hipMemcpyDeviceToHost, st));
        WL_HIP(ctx, hipStreamSynchronize(st));
        *nrm = h.nrm;
        ctx->last_kernel = "k_mp_residual_part";
        return (int)WL_OK;
    });
}

int wl_matchingpursuit_filter(wl_ctx *ctx, int dtype, void *y, void *r, int64_t n, int nbases, const double *qmfs, const int *flens, const int *Ls,
                              double tol, int64_t nmax, int64_t *niter, double *nrm, void *stream)
{
    if (!ctx || !y || !r || !qmfs || !flens || !Ls || !niter || !nrm || nbases < 1 || !(tol > 0) || nmax < -1) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    for (int k = 0; k < nbases; ++k) WL_TRY(check_flen(flens[k]));
    if (n < 1 || n > (((int64_t)1 << 60) / nbases)) return WL_EDIMS;
    const size_t es = dtype == WL_F64 ? 8 : 4;
    if (ranges_overlap(y, (size_t)nbases * (size_t)n * es, r, (size_t)n * es)) return WL_EALIAS;
    // base by base, what wl_dwt_filter returns for a vector of n with Ls[k]
    for (int k = 0; k < nbases; ++k) {
        if (Ls[k] < 0) return WL_EINVAL_L;
        if (Ls[k] >= 62 || (n % ((int64_t)1 << Ls[k])) != 0) return WL_EINVAL_SIZE;
    }
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return matchingpursuit_impl<T>(ctx, st, (T *)y, (T *)r, n, nbases, qmfs, flens, Ls, tol, nmax, niter, nrm);
    });
}

}  // extern "C"

// wl_ext.hip -- the callers around the hot path (row 4, modwt / imodwt: wl_modwt.hip):
//   threshold! (all THTypes)             threshold_main.jl:21-117
//   median! / mad! (noise estimate)      denoising.jl:92-110 (+ Statistics.median!)
//   circshift / arrayadd! / rmul!        util_main.jl:105-130, denoising.jl:82-88 (translation-invariant denoising)
// All of it is HBM-bound element-wise or gather work; the arithmetic follows Julia's promotion rules
// literally (Float32 data with a Float64 threshold: compute in Float64, round on every store) so the
// results are bit-identical to the reference loops.
#include "wl_entry.h"
#include "wl_fast.h"
#include "wl_dev.h"
#include "wl_select.h"

#include <cmath>
#include <cstring>

using namespace wl;

namespace {

// ---- threshold! ------------------------------------------------------------------------------------
// (threshold_one: wl_dev.h -- the level-1 kernel of the translation-invariant batch applies it at its stores)
template <typename T, typename C>
__global__ void __launch_bounds__(EXT_THREADS) k_threshold(T *__restrict__ x, int64_t n, int th, C t, int vec_ok)
{
    ew_inplace<T>(x, n, vec_ok, [=](T v, int64_t) { return threshold_one<T, C>(v, th, t); });
}

// ---- order statistics: MSB-first radix select on monotone integer keys (KeyOf, lds_select, wave_pick_bin: wl_select.h) ------
// Two ranks are resolved together (the two middle order statistics of an even-length median).
struct SelState {
    unsigned long long prefix[2];
    unsigned long long k[2];            // remaining 0-based rank inside the current prefix class
    unsigned int hist[2][256];
    unsigned int nan_count;
    unsigned int pad;
    double result;                      // median / order statistic as Float64
    double value[2];                    // the two selected values
    unsigned long long less, equal;     // counts relative to value[0] (threshold_biggest)
};

__global__ void k_sel_init(SelState *s, unsigned long long k0, unsigned long long k1)
{
    const int t = threadIdx.x;
    if (t < 256) { s->hist[0][t] = 0; s->hist[1][t] = 0; }
    if (t == 0) {
        s->prefix[0] = s->prefix[1] = 0; s->k[0] = k0; s->k[1] = k1; s->nan_count = 0; s->result = 0.0;
        s->value[0] = s->value[1] = 0.0; s->less = s->equal = 0;
    }
}
// histogram of byte `pass` (0 = most significant) among keys whose higher bytes equal the rank's prefix
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_sel_hist(const T *__restrict__ v, int64_t n, int pass, int absmode, SelState *s)
{
    typedef typename KeyOf<T>::U U;
    constexpr int NB = KeyOf<T>::BYTES;
    __shared__ unsigned int lh[2][256];
    lh[0][threadIdx.x] = 0;
    lh[1][threadIdx.x] = 0;
    __syncthreads();
    const int shift = 8 * (NB - 1 - pass);
    const U p0 = (U)s->prefix[0], p1 = (U)s->prefix[1];
    const bool same = (p0 == p1);
    unsigned int nans = 0;
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthr) {
        const T x = v[i];
        if (pass == 0 && x != x) ++nans;
        const U key = KeyOf<T>::key(x, absmode);
        const U hi = (pass == 0) ? (U)0 : (key >> (shift + 8));
        const unsigned b = (unsigned)((key >> shift) & 0xff);
        if (pass == 0 || hi == (p0 >> (shift + 8))) atomicAdd(&lh[0][b], 1u);
        if (!same && hi == (p1 >> (shift + 8))) atomicAdd(&lh[1][b], 1u);
    }
    __syncthreads();
    if (lh[0][threadIdx.x]) atomicAdd(&s->hist[0][threadIdx.x], lh[0][threadIdx.x]);
    if (!same && lh[1][threadIdx.x]) atomicAdd(&s->hist[1][threadIdx.x], lh[1][threadIdx.x]);
    if (nans) atomicAdd(&s->nan_count, nans);
}
// pick the bucket holding each rank, extend the prefix, clear the histograms
template <typename T>
__global__ void k_sel_scan(int pass, SelState *s)
{
    constexpr int NB = KeyOf<T>::BYTES;
    const int shift = 8 * (NB - 1 - pass);
    if (threadIdx.x == 0) {
        const bool same = (s->prefix[0] == s->prefix[1]);
        for (int r = 0; r < 2; ++r) {
            const unsigned int *h = s->hist[(same && r == 1) ? 0 : r];
            unsigned long long k = s->k[r], cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (k < cum + h[b]) break;
                cum += h[b];
            }
            s->k[r] = k - cum;
            s->prefix[r] |= ((unsigned long long)b) << shift;
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) { s->hist[0][threadIdx.x] = 0; s->hist[1][threadIdx.x] = 0; }
}
// median!: odd n -> the middle order statistic, even n -> middle(a, b) = a/2 + b/2; NaN anywhere -> NaN
template <typename T>
__global__ void k_sel_finish(SelState *s, int absmode, int is_median, T *result_t)
{
    typedef typename KeyOf<T>::U U;
    const T a = KeyOf<T>::val((U)s->prefix[0], absmode), b = KeyOf<T>::val((U)s->prefix[1], absmode);
    s->value[0] = (double)a;
    s->value[1] = (double)b;
    T m = a;
    if (is_median) {
        if (s->prefix[0] != s->prefix[1]) m = a / 2 + b / 2;
        if (s->nan_count) m = (T)NAN;
    }
    s->result = (double)m;
    if (result_t) *result_t = m;
}
// mad!: y[i] = abs(y[i] - m)
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_absdev(T *__restrict__ y, int64_t n, const T *m, int vec_ok)
{
    const T mm = *m;
    ew_inplace<T>(y, n, vec_ok, [=](T v, int64_t) { const T d = v - mm; return d < 0 ? -d : d; });
}
// BiggestTH: counts of |x| below / equal to the cut, then the zeroing passes
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_count_cut(const T *__restrict__ x, int64_t n, SelState *s)
{
    const T a = (T)s->value[0];
    unsigned long long less = 0, eq = 0;
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthr) {
        const T v = x[i] < 0 ? -x[i] : x[i];
        less += (v < a);
        eq += (v == a);
    }
    if (less) atomicAdd(&s->less, less);
    if (eq) atomicAdd(&s->equal, eq);
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_zero_below(T *__restrict__ x, int64_t n, const SelState *s, int inclusive)
{
    const T a = (T)s->value[0];
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthr) {
        const T v = x[i] < 0 ? -x[i] : x[i];
        if (v < a || (inclusive && v == a)) x[i] = (T)0;
    }
}
// ties at the cut: zero the first `need` entries (index order) whose magnitude equals the cut; one wave, ordered
template <typename T>
__global__ void __launch_bounds__(64) k_zero_ties(T *__restrict__ x, int64_t n, const SelState *s, unsigned long long need)
{
    const T a = (T)s->value[0];
    const int lane = threadIdx.x;
    unsigned long long done = 0;
    for (int64_t base = 0; base < n && done < need; base += 64) {
        const int64_t i = base + lane;
        const T v = (i < n) ? (x[i] < 0 ? -x[i] : x[i]) : (T)-1;
        const bool tie = (i < n) && (v == a);
        const unsigned long long mask = __ballot(tie);
        const unsigned long long before = mask & ((1ull << lane) - 1ull);
        if (tie && done + (unsigned long long)__popcll(before) < need) x[i] = (T)0;
        done += (unsigned long long)__popcll(mask);
    }
}

int ensure_aux(wl_ctx *ctx)
{
    if (ctx->aux) return WL_OK;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, 8192);
    if (e != hipSuccess) { ctx->last_hip = (int)e; return WL_ENOMEM; }
    ctx->aux = p;
    return WL_OK;
}

// Small arrays (<= 8192 elements, e.g. the noise estimate of a 2-D array: the lower half of one column): the whole
// median / mad! in ONE workgroup with the keys in LDS -- the multi-launch radix select above is launch-bound there.
template <typename T, int INST = 0>
__device__ T lds_median(typename KeyOf<T>::U *keys, int n, unsigned int *hist, unsigned long long *sh, unsigned int nan_count)
{
    typedef typename KeyOf<T>::U U;
    const unsigned long long k1 = (unsigned long long)(n / 2), k0 = (n & 1) ? k1 : k1 - 1;
    const U p0 = lds_select<T, INST>(keys, n, k0, hist, sh);
    const U p1 = (k1 == k0) ? p0 : lds_select<T, INST>(keys, n, k1, hist, sh);
    const T a = KeyOf<T>::val(p0, 0), b = KeyOf<T>::val(p1, 0);
    T m = (p0 != p1) ? (a / 2 + b / 2) : a;
    if (nan_count) m = (T)NAN;
    return m;
}
// do_mad = 0: result = median(v) (v untouched);  1: mad!(v): v[i] = abs(v[i] - median(v)), result = median of that
template <typename T>
__global__ void __launch_bounds__(1024) k_mad_lds(T *v, int n, int do_mad, SelState *s)
{
    typedef typename KeyOf<T>::U U;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    U *keys = reinterpret_cast<U *>(smem_raw);
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long sh[2];
    __shared__ unsigned int nans;
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (tid == 0) nans = 0;
    __syncthreads();
    unsigned int mynan = 0;
    for (int i = tid; i < n; i += nthr) {
        const T x = v[i];
        if (x != x) ++mynan;
        keys[i] = KeyOf<T>::key(x, 0);
    }
    if (mynan) atomicAdd(&nans, mynan);
    __syncthreads();
    T m = lds_median<T>(keys, n, hist, sh, nans);
    if (do_mad) {
        __syncthreads();
        for (int i = tid; i < n; i += nthr) {
            const T d = KeyOf<T>::val(keys[i], 0) - m;
            const T ad = d < 0 ? -d : d;
            v[i] = ad;
            keys[i] = KeyOf<T>::key(ad, 0);
        }
        __syncthreads();
        m = lds_median<T>(keys, n, hist, sh, nans);
    }
    if (tid == 0) s->result = (double)m;
}
template <typename T>
int mad_small(wl_ctx *ctx, hipStream_t st, T *v, int64_t n, int do_mad, double *result_host)
{
    int rc = ensure_aux(ctx);
    if (rc != WL_OK) return rc;
    SelState *s = (SelState *)ctx->aux;
    const int threads = n >= 2048 ? 1024 : (n >= 256 ? 256 : 64);
    hipLaunchKernelGGL((k_mad_lds<T>), dim3(1), dim3(threads), (size_t)n * sizeof(typename KeyOf<T>::U), st, v, (int)n, do_mad, s);
    WL_HIP(ctx, hipGetLastError());
    if (result_host) {              // (nullptr: the result stays in the selection state on the device, nobody waits)
        WL_HIP(ctx, hipMemcpyAsync(result_host, &s->result, sizeof(double), hipMemcpyDeviceToHost, st));
        WL_HIP(ctx, hipStreamSynchronize(st));
    }
    return WL_OK;
}

// enqueue the selection of ranks k0 <= k1 (0-based) of v[0..n); leaves prefix[] resolved in the state
template <typename T>
int select_ranks(wl_ctx *ctx, hipStream_t st, const T *v, int64_t n, unsigned long long k0, unsigned long long k1, int absmode)
{
    SelState *s = (SelState *)ctx->aux;
    hipLaunchKernelGGL(k_sel_init, dim3(1), dim3(256), 0, st, s, k0, k1);
    const unsigned nb = ext_blocks(n, 8, ctx->cu_count);
    for (int pass = 0; pass < KeyOf<T>::BYTES; ++pass) {
        hipLaunchKernelGGL((k_sel_hist<T>), dim3(nb), dim3(EXT_THREADS), 0, st, v, n, pass, absmode, s);
        hipLaunchKernelGGL((k_sel_scan<T>), dim3(1), dim3(256), 0, st, pass, s);
    }
    WL_HIP(ctx, hipGetLastError());
    return WL_OK;
}

template <typename T>
int median_impl(wl_ctx *ctx, hipStream_t st, const T *v, int64_t n, double *result_host, T *result_dev)
{
    int rc = ensure_aux(ctx);
    if (rc != WL_OK) return rc;
    SelState *s = (SelState *)ctx->aux;
    const unsigned long long k1 = (unsigned long long)(n / 2), k0 = (n & 1) ? k1 : k1 - 1;
    rc = select_ranks<T>(ctx, st, v, n, k0, k1, 0);
    if (rc != WL_OK) return rc;
    hipLaunchKernelGGL((k_sel_finish<T>), dim3(1), dim3(1), 0, st, s, 0, 1, result_dev);
    WL_HIP(ctx, hipGetLastError());
    if (result_host) {
        WL_HIP(ctx, hipMemcpyAsync(result_host, &s->result, sizeof(double), hipMemcpyDeviceToHost, st));
        WL_HIP(ctx, hipStreamSynchronize(st));
    }
    return WL_OK;
}

// mad!(v): v[i] = abs(v[i] - median(v)) and the median of that -- in the selection state on the device, and in *result_host when
// that is not nullptr (the call then waits for it).  One workgroup with the keys in LDS where they fit, else the radix select twice.
template <typename T>
int mad_one(wl_ctx *ctx, hipStream_t st, T *v, int64_t n, double *result_host)
{
    if (n <= mad_lds_max<T>()) return mad_small<T>(ctx, st, v, n, 1, result_host);
    WL_TRY(ensure_aux(ctx));
    T *mdev = (T *)((char *)ctx->aux + 4096);              // the first median, in the element type
    WL_TRY(median_impl<T>(ctx, st, v, n, nullptr, mdev));
    hipLaunchKernelGGL((k_absdev<T>), dim3(ext_blocks(n, 4, ctx->cu_count)), dim3(EXT_THREADS), 0, st, v, n, (const T *)mdev, vec_ok16(v));
    return median_impl<T>(ctx, st, v, n, result_host, (T *)nullptr);
}

template <typename T>
int biggest_impl(wl_ctx *ctx, hipStream_t st, T *x, int64_t n, int64_t m)
{
    if (m > n) m = n;
    const int64_t nz = n - m;                      // entries to clear
    if (nz <= 0) return WL_OK;
    int rc = ensure_aux(ctx);
    if (rc != WL_OK) return rc;
    SelState *s = (SelState *)ctx->aux;
    rc = select_ranks<T>(ctx, st, x, n, (unsigned long long)(nz - 1), (unsigned long long)(nz - 1), 1);
    if (rc != WL_OK) return rc;
    hipLaunchKernelGGL((k_sel_finish<T>), dim3(1), dim3(1), 0, st, s, 1, 0, (T *)nullptr);
    const unsigned nb = ext_blocks(n, 4, ctx->cu_count);
    hipLaunchKernelGGL((k_count_cut<T>), dim3(nb), dim3(EXT_THREADS), 0, st, x, n, s);
    WL_HIP(ctx, hipGetLastError());
    unsigned long long cnt[2] = {0, 0};
    WL_HIP(ctx, hipMemcpyAsync(cnt, &s->less, sizeof(cnt), hipMemcpyDeviceToHost, st));
    WL_HIP(ctx, hipStreamSynchronize(st));
    const unsigned long long need = (unsigned long long)nz - cnt[0];       // ties at the cut that must go
    if (need >= cnt[1]) {
        hipLaunchKernelGGL((k_zero_below<T>), dim3(nb), dim3(EXT_THREADS), 0, st, x, n, s, 1);
    } else {
        hipLaunchKernelGGL((k_zero_ties<T>), dim3(1), dim3(64), 0, st, x, n, s, need);
        hipLaunchKernelGGL((k_zero_below<T>), dim3(nb), dim3(EXT_THREADS), 0, st, x, n, s, 0);
    }
    WL_HIP(ctx, hipGetLastError());
    return WL_OK;
}

// ---- circshift / arrayadd! / rmul! -------------------------------------------------------------------
struct Shift3 { int64_t d[3]; int64_t s[3]; };
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_circshift(T *__restrict__ b, const T *__restrict__ a, int64_t n, Shift3 p)
{
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += nthr) {
        const int64_t i0 = e % p.d[0], r = e / p.d[0], i1 = r % p.d[1], i2 = r / p.d[1];
        int64_t j0 = i0 - p.s[0], j1 = i1 - p.s[1], j2 = i2 - p.s[2];
        if (j0 < 0) j0 += p.d[0];
        if (j1 < 0) j1 += p.d[1];
        if (j2 < 0) j2 += p.d[2];
        b[e] = a[j0 + p.d[0] * (j1 + p.d[1] * j2)];
    }
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_arrayadd(T *__restrict__ y, const T *__restrict__ z, int64_t n, int vec_ok)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    const VT *zv = reinterpret_cast<const VT *>(z);
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nv = vec_ok ? n / V : 0;
    VT *yv = reinterpret_cast<VT *>(y);
    for (int64_t i = gid; i < nv; i += nthr) {
        VT a = yv[i];
        const VT b = zv[i];
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] = a[e] + b[e];
        yv[i] = a;
    }
    for (int64_t i = nv * V + gid; i < n; i += nthr) y[i] = y[i] + z[i];
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_rmul(T *__restrict__ y, int64_t n, double s, int vec_ok)
{
    ew_inplace<T>(y, n, vec_ok, [=](T v, int64_t) { return (T)((double)v * s); });
}


// ---- translation-invariant denoising as ONE batch (denoising.jl:36-67) ---------------------------------------------------
// spin i (1-based) shifts dimension d by nspin2circ(nspin, i)[d] (denoising.jl:112-121: first dimension fastest)
// (vectors: n1 = n2 = 1; matrices: n2 = 1; nsp of an absent dimension = 1)
struct TiGeom { int64_t n0, n1, n2, N; int64_t nsp0, nsp1, nsp2; int64_t b0; };
__device__ __forceinline__ void ti_shift_of(const TiGeom &g, int64_t spin0, int64_t &s0, int64_t &s1, int64_t &s2)
{
    s0 = (spin0 % g.nsp0) % g.n0;
    s1 = ((spin0 / g.nsp0) % g.nsp1) % g.n1;
    s2 = ((spin0 / (g.nsp0 * g.nsp1)) % g.nsp2) % g.n2;
}
// Z[b] = circshift(x, +shift(b0 + b)): z[i] = x[i - shift] (Util.circshift!, util_main.jl:105-130).
// grid: x = groups of 4 rows, y = groups of 8 columns (a column = one (i1, i2) of a cube: n1 * n2 of them, walked with a grid
// stride so that the grid stays within 65535), z = spin (no integer division per element; 16-byte stores, the shifted reads are
// four scalar loads from a contiguous run)
template <typename T>
__global__ void __launch_bounds__(256) k_ti_shift(T *__restrict__ Z, const T *__restrict__ x, TiGeom g)
{
    typedef T V4 __attribute__((ext_vector_type(4)));
    const int64_t b = blockIdx.z;
    int64_t s0, s1, s2;
    ti_shift_of(g, g.b0 + b, s0, s1, s2);
    const int n0 = (int)g.n0, sh = (int)s0;
    const int64_t ncol = g.n1 * g.n2;
    const bool vec = (n0 & 3) == 0 && (reinterpret_cast<uintptr_t>(Z) % (4 * sizeof(T))) == 0;
    // eight columns per workgroup (a workgroup per column is a single 16-byte store per thread: launch-rate bound)
    for (int64_t c0 = (int64_t)blockIdx.y * 8; c0 < ncol; c0 += (int64_t)gridDim.y * 8)
    for (int64_t c = c0; c < ncol && c < c0 + 8; ++c) {
        const int64_t i2 = c / g.n1, i1 = c - i2 * g.n1;
        int64_t j1 = i1 - s1, j2 = i2 - s2;
        if (j1 < 0) j1 += g.n1;
        if (j2 < 0) j2 += g.n2;
        const T *src = x + g.n0 * (j1 + g.n1 * j2);
        T *dst = Z + b * g.N + g.n0 * c;
        for (int i0 = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x); i0 < n0; i0 += 4 * (int)(gridDim.x * blockDim.x)) {
            T v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int j0 = i0 + e - sh;
                if (j0 < 0) j0 += n0;
                v[e] = (i0 + e < n0) ? src[j0] : (T)0;
            }
            if (vec) {
                *reinterpret_cast<V4 *>(dst + i0) = V4{v[0], v[1], v[2], v[3]};
            } else {
                for (int e = 0; e < 4 && i0 + e < n0; ++e) dst[i0 + e] = v[e];
            }
        }
    }
}
// y += circshift(Z[b], -shift(b0 + b)) for b = 0 .. nb-1 IN THAT ORDER (arrayadd! once per spin: the summation order
// of the reference, so the sums carry the same roundings).  grid: x = groups of 4 rows, y = column ((i1, i2) of a cube, grid
// stride: at most 65535 workgroups along y).  The shifts of the
// batch sit in LDS (no integer division per spin and lane); the spins are read eight at a time, loads before the adds.
template <typename T>
__global__ void __launch_bounds__(256) k_ti_accumulate(T *__restrict__ y, const T *__restrict__ Z, TiGeom g, int64_t nb, int first)
{
    __shared__ int sh0[256], sh1[256], sh2[256];
    const int n0 = (int)g.n0, n1 = (int)g.n1, n2 = (int)g.n2;
    const int64_t ncol = g.n1 * g.n2;
    for (int64_t bb0 = 0; bb0 < nb; bb0 += 256) {
        const int nbb = (int)((nb - bb0 < 256) ? (nb - bb0) : 256);
        __syncthreads();
        if ((int)threadIdx.x < nbb) {
            int64_t s0, s1, s2;
            ti_shift_of(g, g.b0 + bb0 + threadIdx.x, s0, s1, s2);
            sh0[threadIdx.x] = (int)s0;
            sh1[threadIdx.x] = (int)s1;
            sh2[threadIdx.x] = (int)s2;
        }
        __syncthreads();
        for (int64_t col = blockIdx.y; col < ncol; col += gridDim.y) {
        const int i2 = (int)(col / n1), i1 = (int)(col - (int64_t)i2 * n1);
        // a thread owns rows ib + tid + 256 e (e < 4): consecutive lanes read consecutive addresses of every shifted plane (the
        // shifts are arbitrary, so 16-byte loads are out; four rows per lane side by side cost four partial lines per load)
        for (int ib = 4 * (int)(blockIdx.x * blockDim.x); ib < n0; ib += 4 * (int)(gridDim.x * blockDim.x)) {
            const int ibt = ib + (int)threadIdx.x;
            T acc[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = ((first && bb0 == 0) || ibt + 256 * e >= n0) ? (T)0 : y[ibt + 256 * e + (int64_t)n0 * col];
            for (int b8 = 0; b8 < nbb; b8 += 8) {
                T v[8][4];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (b8 + u < nbb) {
                        int j1 = i1 + sh1[b8 + u], j2 = i2 + sh2[b8 + u];
                        if (j1 >= n1) j1 -= n1;
                        if (j2 >= n2) j2 -= n2;
                        const T *zp = Z + (bb0 + b8 + u) * g.N + (int64_t)n0 * (j1 + (int64_t)n1 * j2);
                        const int s = sh0[b8 + u];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            int j0 = ibt + 256 * e + s;
                            if (j0 >= n0) j0 -= n0;
                            v[u][e] = (ibt + 256 * e < n0) ? zp[j0] : (T)0;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (b8 + u < nbb) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = acc[e] + v[u][e];
                    }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ibt + 256 * e < n0) y[ibt + 256 * e + (int64_t)n0 * col] = acc[e];
        }
        }
    }
}
// threshold!(x, TH, sigma * t_unit) with sigma = mad / 0.6745 read from the device (noisest, denoising.jl:92-101): the
// product is formed in Float64 exactly as Julia does for a Float64 dnt.t, whatever the element type
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_threshold_dev(T *__restrict__ x, int64_t n, int th, const double *__restrict__ mad_dev,
                                                               double t_unit, double sigma_host, int vec_ok)
{
    const double sigma = (sigma_host >= 0) ? sigma_host : (*mad_dev / 0.6745);
    const double t = sigma * t_unit;
    ew_inplace<T>(x, n, vec_ok, [=](T v, int64_t) { return threshold_one<T, double>(v, th, t); });
}
// the same on the approximation quadrant [0, h0) x [0, h1) of every plane of a batch (leading dimension n0, plane stride N): the
// details of level 1 were thresholded by the kernel that produced them (SrcView::th)
template <typename T>
__global__ void __launch_bounds__(256) k_threshold_dev_quadrant(T *__restrict__ x, int64_t n0, int64_t N, int64_t h0, int th,
                                                                const double *__restrict__ mad_dev, double t_unit, double sigma_host)
{
    const double sigma = (sigma_host >= 0) ? sigma_host : (*mad_dev / 0.6745);
    const double t = sigma * t_unit;
    T *col = x + (int64_t)blockIdx.z * N + (int64_t)blockIdx.y * n0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < h0; i += (int64_t)gridDim.x * blockDim.x)
        col[i] = threshold_one<T, double>(col[i], th, t);
}
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_copy_range(T *__restrict__ dst, const T *__restrict__ src, int64_t n)
{
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += nthr) dst[e] = src[e];
}

// The noise estimate of one array from its level-1 coefficients c1 (noisest, denoising.jl:92-101): mad! of c1[detailrange(c1, 1)]
// (linear indexing: the upper half of the first column) on a copy dr of those n0 / 2 samples.  Nobody waits: the MAD stays in the
// selection state, where k_threshold_dev reads it.
template <typename T>
int sigma_of_detail(wl_ctx *ctx, hipStream_t st, T *dr, const T *c1, int64_t n0)
{
    const int64_t lo = (int64_t)llround((double)n0 / 2 + 1) - 1, nd = n0 - lo;        // detailrange(n0, 1), 0-based half open
    hipLaunchKernelGGL((k_copy_range<T>), dim3(ext_blocks(nd, 1, ctx->cu_count)), dim3(EXT_THREADS), 0, st, dr, c1 + lo, nd);
    return mad_one<T>(ctx, st, dr, nd, nullptr);
}
// the launches of k_ti_shift / k_ti_accumulate on the nb spins from g.b0: x = groups of 4 rows (at most 64 workgroups), y = the
// columns (i1, i2), eight per workgroup of the shift, with a grid stride beyond 65535 workgroups
inline unsigned ti_grid_x(int64_t n0)
{
    const int64_t gx = (n0 / 4 + 255) / 256;
    return (unsigned)(gx > 64 ? 64 : (gx > 0 ? gx : 1));
}
template <typename T>
void ti_shift(hipStream_t st, T *Z, const T *x, const TiGeom &g, int64_t nb)
{
    const int64_t gy = (g.n1 * g.n2 + 7) / 8;
    hipLaunchKernelGGL((k_ti_shift<T>), dim3(ti_grid_x(g.n0), (unsigned)(gy > 65535 ? 65535 : gy), (unsigned)nb), dim3(256), 0, st, Z, x, g);
}
template <typename T>
void ti_accumulate(hipStream_t st, T *y, const T *Z, const TiGeom &g, int64_t nb, int first)
{
    const int64_t gy = g.n1 * g.n2;
    hipLaunchKernelGGL((k_ti_accumulate<T>), dim3(ti_grid_x(g.n0), (unsigned)(gy > 65535 ? 65535 : gy)), dim3(256), 0, st, y, Z, g, nb, first);
}

template <typename T>
int denoise_ti_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, const double *qmf, int flen, int L,
                    int th, double t_unit, const int64_t *nspin, double sigma_host)
{
    const int64_t n0 = dims[0], n1 = (ndims >= 2) ? dims[1] : 1, n2 = (ndims == 3) ? dims[2] : 1, N = n0 * n1 * n2;
    const int64_t nsp0 = nspin[0], nsp1 = (ndims >= 2) ? nspin[1] : 1, nsp2 = (ndims == 3) ? nspin[2] : 1, pns = nsp0 * nsp1 * nsp2;
    Taps<T> taps;
    make_taps<T>(qmf, flen, taps);
    int rc = ensure_aux(ctx);
    if (rc != WL_OK) return rc;
    SelState *sel = (SelState *)ctx->aux;
    // cubes: the spins of a group are a batch of volumes (filter_*_levels_vols, wl_batch3d.hip: every level of the one-launch 3-D
    // kernels one launch over all spins); its workspace is the approximation ping-pong per spin + one volume's generic buffers
    auto tw_elems = [&](int64_t B) { return ws_filter_planes_elems(ndims, N, B); };
    // spins per batch: the whole set unless the buffers (2 N B for the shifted copies and their coefficients, plus the
    // transform workspace of the batch box) would pass the cap
    // Virtual shifts (Float32 square images on the LDS-exchange level kernel): a circular shift along dim 2 is an offset of the
    // column index inside the level-1 kernel, so only the nsp0 row-shifted copies of x are materialised (ZR) instead of
    // nsp0 * nsp1 shifted planes -- for 8 x 8 spins of a 2048^2 image 128 MiB written instead of 1 GiB (265 us of 2.4 ms).
    bool virt = false;
    if constexpr (sizeof(T) == 4) {
        virt = ndims == 2 && L >= 1 && ctx->path == 0 && (flen % 2) == 0 && flen <= 10 && opt("WL_TI_VIRTSHIFT", 1) != 0 &&
               fwd2d_lds_ok(flen, 1, n0, n1) && (n0 % 4) == 0 && nsp1 <= n1 && nsp0 <= n0 && nsp0 < (1 << 20);
    }
    const size_t zr_elems = virt ? (size_t)N * (size_t)nsp0 : 0;
    // (one spin: no shifted copy Z, see below)
    const size_t ncopies = (pns == 1) ? 1 : 2;
    auto need = [&](int64_t B) { return (tw_elems(B) + ncopies * (size_t)N * B + zr_elems + (size_t)n0 + 64) * sizeof(T); };
    int64_t B = 1;
    rc = group_reserve(ctx, st, pns, 65535, need, B);
    if (rc != WL_OK) return rc;
    T *tw = (T *)ctx->ws;                                   // transform workspace of the batch box (with the generic buffers)
    T *Z = tw + tw_elems(B);
    T *XT = Z + (pns == 1 ? 0 : N * B);
    T *ZR = XT + N * B;                                     // row-shifted copies (virtual shifts only)
    T *dr = ZR + zr_elems;                                  // detail range of the noise estimate (n0/2 samples)
    const unsigned nbk = ext_blocks(N * B, 4, ctx->cu_count);

    BoxSpec b1;                                             // the array itself
    b1.nd = ndims; b1.nt = ndims;
    b1.dims[0] = n0; b1.dims[1] = n1; b1.dims[2] = n2;
    b1.full = dense_strides(b1.dims);
    // ---- sigma = noisest(x, wt): level-1 transform, MAD of y1[detailrange(y1, 1)] (linear indexing: first column) ----
    if (!(sigma_host >= 0)) {
        if (n0 < 2 || (n0 % 2) != 0 || (ndims >= 2 && (n1 % 2) != 0) || (ndims == 3 && (n2 % 2) != 0)) return WL_EINVAL_SIZE;
        rc = filter_fwd_levels<T>(tw, true, ctx->cu_count, ctx->path, st, b1, XT, x, taps, 1, &ctx->last_kernel, &ctx->last_hip);
        if (rc != WL_OK) return rc;
        WL_TRY(sigma_of_detail<T>(ctx, st, dr, XT, n0));
    }
    // ---- one spin of shift zero (the plain, not translation-invariant denoise routed here so that sigma stays on the device):
    //      y = idwt(threshold!(dwt(x))) with no shifted copy, no accumulation and no scaling -- the reference's own sequence
    //      (denoising.jl:69-80), signed zeros included, and a quarter of the batch path's memory ----
    if (pns == 1) {
        const T *coef_src = x;
        if (L > 0) {
            rc = filter_fwd_levels<T>(tw, true, ctx->cu_count, ctx->path, st, b1, XT, x, taps, L, &ctx->last_kernel, &ctx->last_hip);
            if (rc != WL_OK) return rc;
            coef_src = XT;
        } else {
            hipLaunchKernelGGL((k_copy_range<T>), dim3(ext_blocks(N, 1, ctx->cu_count)), dim3(EXT_THREADS), 0, st, XT, x, N);
            coef_src = XT;
        }
        hipLaunchKernelGGL((k_threshold_dev<T>), dim3(ext_blocks(N, 4, ctx->cu_count)), dim3(EXT_THREADS), 0, st, XT, N, th, &sel->result, t_unit,
                           sigma_host, vec_ok16(XT));
        if (L > 0) {
            const char *kn = nullptr;
            rc = filter_inv_levels<T>(tw, true, ctx->cu_count, ctx->path, st, b1, y, coef_src, taps, L, &kn, &ctx->last_hip);
            if (rc != WL_OK) return rc;
        } else {
            hipLaunchKernelGGL((k_copy_range<T>), dim3(ext_blocks(N, 1, ctx->cu_count)), dim3(EXT_THREADS), 0, st, y, coef_src, N);
        }
        ctx->last_kernel = "denoise_one_spin";
        WL_HIP(ctx, hipGetLastError());
        return WL_OK;
    }
    // ---- the spins, B at a time ----
    TiGeom g;
    g.n0 = n0; g.n1 = n1; g.n2 = n2; g.N = N; g.nsp0 = nsp0; g.nsp1 = nsp1; g.nsp2 = nsp2;
    if (virt) {
        TiGeom gr = g;                                      // spins 0 .. nsp0-1 shift dim 1 only
        gr.nsp1 = 1; gr.b0 = 0;
        ti_shift<T>(st, ZR, x, gr, nsp0);
    }
    for (int64_t b0 = 0; b0 < pns; b0 += B) {
        const int64_t nb = (pns - b0 < B) ? (pns - b0) : B;
        g.b0 = b0;
        bool shifted = false, thresholded_l1 = false;
        int64_t th_c0 = n0, th_c1 = n1;                      // what the level kernels left unthresholded: the low corner of every plane
        if (virt) {
            // plane p of this group = copy (b0 + p) % nsp0 of ZR with its columns rotated by (b0 + p) / nsp0
            tl_srcview.mod = (int)nsp0; tl_srcview.spin0 = b0; tl_srcview.used = 0; tl_srcview.corner0 = n0; tl_srcview.corner1 = n1;
            // ... and that launch thresholds the level-1 details as it stores them (3/4 of all coefficients)
            // (hard: one Float32 compare; soft / semisoft / Stein: the same cut, Float64 only for the survivors -- ThCut, wl_dev.h)
            const bool fuse_th = opt("WL_TI_FUSE_TH", 1) != 0 && th >= WL_TH_HARD && th <= WL_TH_STEIN &&
                                 (th == WL_TH_HARD || opt("WL_TI_FUSE_SOFT", 1) != 0);
            tl_srcview.th = fuse_th ? th : -1; tl_srcview.t_unit = t_unit; tl_srcview.sigma_host = sigma_host; tl_srcview.mad_dev = &sel->result;
            rc = filter_fwd_levels<T>(tw, true, ctx->cu_count, ctx->path, st, planes_box(ndims, dims, nb, N), XT, ZR, taps, L, &ctx->last_kernel,
                                      &ctx->last_hip);
            shifted = tl_srcview.used != 0;
            th_c0 = tl_srcview.corner0; th_c1 = tl_srcview.corner1;
            tl_srcview.mod = 0; tl_srcview.th = -1;
            // WL_RETRY_NOVIEW: no view-aware tier took level 1 -- nothing was enqueued (and nothing read from ZR): materialise below
            if (rc == WL_RETRY_NOVIEW) { rc = WL_OK; shifted = false; }
            if (rc != WL_OK) return rc;
            thresholded_l1 = shifted && fuse_th;
        }
        if (!shifted) {                                     // (materialised shifted planes: every other case)
            ti_shift<T>(st, Z, x, g, nb);
            if (L > 0) WL_TRY(filter_levels_planes<T>(ctx, st, 1, ndims, dims, nb, N, XT, Z, taps, L, &ctx->last_kernel));
        }
        // L == 0: dwt / idwt are copies (transforms_filter.jl:36-38), so the shifted signal itself is thresholded
        T *const coef = (L == 0) ? Z : XT;
        if (thresholded_l1) {
            const int64_t h0 = th_c0, h1 = th_c1;
            if (h0 > 0 && h1 > 0)
                hipLaunchKernelGGL((k_threshold_dev_quadrant<T>), dim3((unsigned)((h0 + 255) / 256 > 8 ? 8 : (h0 + 255) / 256), (unsigned)h1, (unsigned)nb),
                                   dim3(256), 0, st, coef, n0, N, h0, th, &sel->result, t_unit, sigma_host);
        } else {
            hipLaunchKernelGGL((k_threshold_dev<T>), dim3(nbk), dim3(EXT_THREADS), 0, st, coef, N * nb, th, &sel->result, t_unit, sigma_host,
                               vec_ok16(coef));
        }
        if (L > 0) {
            const char *kn = nullptr;
            WL_TRY(filter_levels_planes<T>(ctx, st, 0, ndims, dims, nb, N, Z, XT, taps, L, &kn));
        }
        ti_accumulate<T>(st, y, Z, g, nb, b0 == 0 ? 1 : 0);
    }
    hipLaunchKernelGGL((k_rmul<T>), dim3(ext_blocks(N, 4, ctx->cu_count)), dim3(EXT_THREADS), 0, st, y, N, 1.0 / (double)pns, vec_ok16(y));
    WL_HIP(ctx, hipGetLastError());
    return WL_OK;
}

// ---- translation-invariant denoise with a lifting scheme (denoising.jl:36-67 with wt::GLS) --------------------------------
// The same device-resident sequence as denoise_ti_impl -- sigma from the level-1 transform without a host round trip, the spins
// shifted / transformed / thresholded / inverted / un-shifted / accumulated B at a time -- with the lifting transforms of the
// library: a batch of shifted SIGNALS is one batched-lines call (the fused line kernels over all spins), a batch of shifted
// IMAGES is one batched 2-D lifting transform (every level one launch over all spins of the group, as wl_dwt_lifting_batch), a batch
// of shifted CUBES one batched 3-D lifting transform (wl_lifting_vols, as wl_dwt_lifting_batch3; a scheme of no known shape runs
// cube after cube inside it).
template <typename T>
int denoise_ti_lifting_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, const SchemeArgs &s, int L, int th,
                            double t_unit, const int64_t *nspin, double sigma_host)
{
    const LiftScheme<T> scf = s.build<T>(1), sci = s.build<T>(0);           // the forward and the inverse scheme
    const int64_t n0 = dims[0], n1 = (ndims >= 2) ? dims[1] : 1, n2 = (ndims == 3) ? dims[2] : 1, N = n0 * n1 * n2;
    const int64_t nsp0 = nspin[0], nsp1 = (ndims >= 2) ? nspin[1] : 1, nsp2 = (ndims == 3) ? nspin[2] : 1, pns = nsp0 * nsp1 * nsp2;
    int rc = ensure_aux(ctx);
    if (rc != WL_OK) return rc;
    SelState *sel = (SelState *)ctx->aux;
    // transform workspace of the batched box (B lines, or B images: the approximation ping-pong of every image; B cubes: the ping-pong
    // and the two dense inter-pass buffers of the batched 3-D level loop, and no less than one cube's own), then the shifted copies Z
    // and their coefficients XT
    auto tws = [&](int64_t B) { return ws_lifting_planes_elems(ndims, N, B); };
    auto need = [&](int64_t B) { return (tws(B) + (size_t)2 * N * B + (size_t)n0 + 64) * sizeof(T); };
    int64_t B = 1;
    rc = group_reserve(ctx, st, pns, 65535, need, B);
    if (rc != WL_OK) return rc;
    T *tw = (T *)ctx->ws;
    T *Z = tw + tws(B);
    T *XT = Z + N * B;
    T *dr = XT + N * B;
    BoxSpec b1;                                              // one signal / image
    b1.nd = ndims; b1.nt = ndims;
    b1.dims[0] = n0; b1.dims[1] = n1; b1.dims[2] = n2;
    b1.full = dense_strides(b1.dims);
    // ---- sigma = noisest(x, wt): level-1 transform, MAD of y1[detailrange(y1, 1)] (linear indexing with size(x, 1)) ----
    if (!(sigma_host >= 0)) {
        if (n0 < 2 || (n0 % 2) != 0 || (ndims >= 2 && (n1 % 2) != 0) || (ndims == 3 && (n2 % 2) != 0)) return WL_EINVAL_SIZE;
        WL_TRY(wl_lifting_box<T>(ctx, st, b1, XT, x, scf, 1, 1));
        WL_TRY(sigma_of_detail<T>(ctx, st, dr, XT, n0));
    }
    TiGeom g;
    g.n0 = n0; g.n1 = n1; g.n2 = n2; g.N = N; g.nsp0 = nsp0; g.nsp1 = nsp1; g.nsp2 = nsp2;
    // nb shifted signals are the lines of one batched call, nb images the third extent of one, nb cubes one batch of volumes
    for (int64_t b0 = 0; b0 < pns; b0 += B) {
        const int64_t nb = (pns - b0 < B) ? (pns - b0) : B;
        g.b0 = b0;
        ti_shift<T>(st, Z, x, g, nb);
        WL_TRY(lifting_levels_planes<T>(ctx, st, ndims, n0, nb, N, XT, Z, scf, L, 1));       // (L = 0: a copy, as the reference's dwt is)
        hipLaunchKernelGGL((k_threshold_dev<T>), dim3(ext_blocks(N * nb, 4, ctx->cu_count)), dim3(EXT_THREADS), 0, st, XT, N * nb, th, &sel->result,
                           t_unit, sigma_host, vec_ok16(XT));
        WL_TRY(lifting_levels_planes<T>(ctx, st, ndims, n0, nb, N, Z, XT, sci, L, 0));
        ti_accumulate<T>(st, y, Z, g, nb, b0 == 0 ? 1 : 0);
    }
    hipLaunchKernelGGL((k_rmul<T>), dim3(ext_blocks(N, 4, ctx->cu_count)), dim3(EXT_THREADS), 0, st, y, N, 1.0 / (double)pns, vec_ok16(y));
    WL_HIP(ctx, hipGetLastError());
    return WL_OK;
}

// ---- denoise of a batch of independent units (wl_mad_batch, wl_denoise_batch_filter, wl_denoise_batch_lifting) --------------
// Per-unit noise estimate: k_mad_lds with blockIdx.x = unit, a strided source and result[unit].  write_back = 0 leaves the source
// alone (the coefficients of a denoise are read, never overwritten by mad!: the deviations only ever exist as LDS keys).
template <typename T>
__global__ void __launch_bounds__(1024) k_mad_units_lds(T *v0, int n, int64_t stride, int write_back, double *__restrict__ result)
{
    typedef typename KeyOf<T>::U U;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    U *keys = reinterpret_cast<U *>(smem_raw);
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long sh[2];
    __shared__ unsigned int nans;
    T *v = v0 + (int64_t)blockIdx.x * stride;
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (tid == 0) nans = 0;
    __syncthreads();
    unsigned int mynan = 0;
    for (int i = tid; i < n; i += nthr) {
        const T x = v[i];
        if (x != x) ++mynan;
        keys[i] = KeyOf<T>::key(x, 0);
    }
    if (mynan) atomicAdd(&nans, mynan);
    __syncthreads();
    T m = lds_median<T, 1>(keys, n, hist, sh, nans);
    __syncthreads();
    for (int i = tid; i < n; i += nthr) {
        const T d = KeyOf<T>::val(keys[i], 0) - m;
        const T ad = d < 0 ? -d : d;
        if (write_back) v[i] = ad;
        keys[i] = KeyOf<T>::key(ad, 0);
    }
    __syncthreads();
    m = lds_median<T, 1>(keys, n, hist, sh, nans);
    if (tid == 0) result[blockIdx.x] = (double)m;
}

// Units too long for LDS keys: a workgroup per unit streams its n values from memory once per radix byte (the unit stays in L2 between
// passes), the two histograms in LDS, both middle ranks resolved per pass (k_sel_hist / k_sel_scan without a selection state in
// HBM and without global atomics).  The second median runs the same passes on |v - m| computed on the fly; the deviations are
// stored only when write_back (wl_mad_batch).  Counters are 32-bit: n < 2^31.  blockDim.x >= 128 (a wave per rank picks its bin).
template <typename T>
__global__ void __launch_bounds__(1024) k_mad_units_stream(T *v0, int64_t n, int64_t stride, int write_back, double *__restrict__ result)
{
    typedef typename KeyOf<T>::U U;
    constexpr int NB = KeyOf<T>::BYTES;
    __shared__ unsigned int hist[2][256];
    __shared__ unsigned long long pre[2], rk[2];
    __shared__ unsigned int nans;
    T *v = v0 + (int64_t)blockIdx.x * stride;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const unsigned long long k1 = (unsigned long long)(n / 2), k0 = (n & 1) ? k1 : k1 - 1;
    T m0 = (T)0, m = (T)0;                      // median of the unit, then of its absolute deviations
    for (int phase = 0; phase < 2; ++phase) {
        __syncthreads();                        // (everybody has read pre[] of the first median)
        if (tid == 0) {
            pre[0] = pre[1] = 0; rk[0] = k0; rk[1] = k1;
            if (phase == 0) nans = 0;
        }
        for (int pass = 0; pass < NB; ++pass) {
            const int shift = 8 * (NB - 1 - pass);
            for (int b = tid; b < 512; b += nthr) (&hist[0][0])[b] = 0;
            __syncthreads();
            const U p0 = (U)pre[0], p1 = (U)pre[1];
            const bool same = (p0 == p1);
            const U q0 = (pass == 0) ? (U)0 : (U)(p0 >> (shift + 8)), q1 = (pass == 0) ? (U)0 : (U)(p1 >> (shift + 8));
            unsigned int mynan = 0;
            for (int64_t i = tid; i < n; i += nthr) {
                T x = v[i];
                if (phase == 1) { const T d = x - m0; x = d < 0 ? -d : d; }
                else if (pass == 0 && x != x) ++mynan;
                const U key = KeyOf<T>::key(x, 0);
                const U hi = (pass == 0) ? (U)0 : (U)(key >> (shift + 8));
                const unsigned b = (unsigned)((key >> shift) & 0xff);
                if (hi == q0) atomicAdd(&hist[0][b], 1u);
                if (!same && hi == q1) atomicAdd(&hist[1][b], 1u);
            }
            if (mynan) atomicAdd(&nans, mynan);
            __syncthreads();
            const int w = tid >> 6;
            if (w < 2) wave_pick_bin(hist[(same || w == 0) ? 0 : 1], tid & 63, shift, &pre[w], &rk[w]);
            __syncthreads();
        }
        const U f0 = (U)pre[0], f1 = (U)pre[1];
        const T a = KeyOf<T>::val(f0, 0), b = KeyOf<T>::val(f1, 0);
        m = (f0 != f1) ? (a / 2 + b / 2) : a;
        if (nans) m = (T)NAN;
        if (phase == 0) m0 = m;
    }
    if (write_back)
        for (int64_t i = tid; i < n; i += nthr) {
            const T d = v[i] - m0;
            v[i] = d < 0 ? -d : d;
        }
    if (tid == 0) result[blockIdx.x] = (double)m;
}

// result[u] = mad!(v[u * stride .. u * stride + n)) for u < nunits; *name = the kernel that ran
template <typename T>
int mad_units(wl_ctx *ctx, hipStream_t st, T *v, int64_t n, int64_t nunits, int64_t stride, int write_back, double *result, const char **name)
{
    int64_t lim = (int64_t)opt("WL_MAD_LDS_MAX", (long long)mad_lds_max<T>());
    if (lim > mad_lds_max<T>()) lim = mad_lds_max<T>();       // (the keys must fit the 64 KiB of LDS a kernel gets)
    const bool lds = n <= lim;
    const int64_t chunk = (int64_t)1 << 20;                    // (grid size * block size stays below 2^32)
    for (int64_t u0 = 0; u0 < nunits; u0 += chunk) {
        const unsigned nb = (unsigned)((nunits - u0 < chunk) ? (nunits - u0) : chunk);
        if (lds) {
            const int threads = n >= 2048 ? 1024 : (n >= 256 ? 256 : 64);
            hipLaunchKernelGGL((k_mad_units_lds<T>), dim3(nb), dim3(threads), (size_t)n * sizeof(typename KeyOf<T>::U), st, v + u0 * stride, (int)n,
                               stride, write_back, result + u0);
        } else {
            const int threads = n >= 4096 ? 1024 : 256;
            hipLaunchKernelGGL((k_mad_units_stream<T>), dim3(nb), dim3(threads), 0, st, v + u0 * stride, n, stride, write_back, result + u0);
        }
    }
    WL_HIP(ctx, hipGetLastError());
    *name = lds ? "k_mad_units_lds" : "k_mad_units_stream";
    return WL_OK;
}

// sg[u] = the sigma of unit u: the caller's (a custom estnoise), or mad / 0.6745 of the estimate that sits in sg (noisest,
// denoising.jl:100); sigma_out receives it
__global__ void __launch_bounds__(EXT_THREADS) k_sigma_units(double *__restrict__ sg, int64_t nb, const double *__restrict__ sigma_in,
                                                            double *__restrict__ sigma_out)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nb) return;
    const double s = sigma_in ? sigma_in[u] : sg[u] / 0.6745;
    sg[u] = s;
    if (sigma_out) sigma_out[u] = s;
}
// threshold!(c_u, th, sigma[u] * t_unit) on the N elements of every unit u = blockIdx.y (unit stride `stride`; the padding between
// units is not touched); the product in Float64 as k_threshold_dev forms it.  16-byte accesses where the unit's base allows them.
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_threshold_units(T *__restrict__ x, int64_t N, int64_t stride, int th, const double *__restrict__ sigma,
                                                                 double t_unit)
{
    T *xu = x + (int64_t)blockIdx.y * stride;
    const double t = sigma[blockIdx.y] * t_unit;
    const int vec_ok = (reinterpret_cast<uintptr_t>(xu) & 15) == 0 ? 1 : 0;
    ew_inplace<T>(xu, N, vec_ok, [=](T v, int64_t) { return threshold_one<T, double>(v, th, t); });
}

// last_kernel of the batch denoises: the family and the kernel of the noise estimate that mad_units / batch_sigma named
const char *denoise_label(bool ti, const char *madk)
{
    static const char *const names[2][3] = {
        {"denoise_batch+k_mad_units_lds", "denoise_batch+k_mad_units_stream", "denoise_batch+sigma_in"},
        {"denoise_ti_units+k_mad_units_lds", "denoise_ti_units+k_mad_units_stream", "denoise_ti_units+sigma_in"}};
    return names[ti ? 1 : 0][strcmp(madk, "k_mad_units_lds") == 0 ? 0 : (strcmp(madk, "k_mad_units_stream") == 0 ? 1 : 2)];
}
// estimate (or take) and publish the sigmas of one group of at most 65535 * 256 units: src = where the level-1 detail range of every
// unit is read from (not read with sigma_in)
template <typename T>
int batch_sigma(wl_ctx *ctx, hipStream_t st, const T *src, int64_t n0, int64_t nb, int64_t S, double *sg, const double *sigma_in,
                double *sigma_out, const char **madk)
{
    if (!sigma_in) {
        const int64_t lo = (int64_t)llround((double)n0 / 2 + 1) - 1, nd = n0 - lo;        // detailrange(n0, 1), 0-based half open
        int rc = mad_units<T>(ctx, st, const_cast<T *>(src) + lo, nd, nb, S, 0, sg, madk);
        if (rc != WL_OK) return rc;
    } else {
        *madk = "sigma_in";
    }
    hipLaunchKernelGGL(k_sigma_units, dim3((unsigned)((nb + EXT_THREADS - 1) / EXT_THREADS)), dim3(EXT_THREADS), 0, st, sg, nb, sigma_in, sigma_out);
    return WL_OK;
}
// ... and apply them: coef = the coefficients that are thresholded
template <typename T>
int batch_sigma_threshold(wl_ctx *ctx, hipStream_t st, const T *src, T *coef, int64_t n0, int64_t N, int64_t nb, int64_t S, double *sg,
                          const double *sigma_in, double *sigma_out, int th, double t_unit, const char **madk)
{
    WL_TRY(batch_sigma<T>(ctx, st, src, n0, nb, S, sg, sigma_in, sigma_out, madk));
    hipLaunchKernelGGL((k_threshold_units<T>), dim3(ext_blocks(N, 4, ctx->cu_count), (unsigned)nb), dim3(EXT_THREADS), 0, st, coef, N, S, th, sg, t_unit);
    WL_HIP(ctx, hipGetLastError());
    return WL_OK;
}

// denoise(x_i, OrthoFilter; L, dnt, TI = false) of nunits units, unit i at element offset i * S: forward batch x -> C (workspace,
// the caller's stride: a box shares its strides between source and destination), per-unit MAD read from C, per-unit threshold on C,
// inverse batch C -> y.  For L >= 1 the level-1 detail range of the L-level coefficients is final after level 1 (later levels
// touch only the low corner), so the one transform serves the estimate and the denoise; L = 0 with an estimate runs a level-1
// batch for it alone and thresholds a copy of x (dwt and idwt are copies then, transforms_filter.jl:36-38).
template <typename T>
int denoise_batch_filter_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, int64_t nunits, int64_t S,
                              const double *qmf, int flen, int L, int th, double t_unit, const double *sigma_in, double *sigma_out)
{
    const int64_t n0 = dims[0];
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    const Taps<T> taps = taps_of<T>(qmf, flen);
    auto tw_elems = [&](int64_t G) { return ws_filter_planes_elems(ndims, N, G); };
    auto need = [&](int64_t G) { return up256(tw_elems(G) * sizeof(T)) + up256((size_t)G * S * sizeof(T)) + up256((size_t)G * sizeof(double)); };
    int64_t G = 1;
    int rc = group_reserve(ctx, st, nunits, 65535, need, G);
    if (rc != WL_OK) return rc;
    char *wsb = (char *)ctx->ws;
    T *Cb = (T *)(wsb + up256(tw_elems(G) * sizeof(T)));
    double *sg = (double *)(wsb + up256(tw_elems(G) * sizeof(T)) + up256((size_t)G * S * sizeof(T)));
    const char *madk = "none", *kn = nullptr;
    WL_TRY(for_groups(nunits, G, [&](int64_t u0, int64_t nb) -> int {
        const T *xg = x + u0 * S;
        T *yg = y + u0 * S;
        if (L > 0 || !sigma_in) {
            rc = filter_levels_planes<T>(ctx, st, 1, ndims, dims, nb, S, Cb, xg, taps, L > 0 ? L : 1, &kn);
            if (rc == WL_RETRY_GEN) rc = WL_EINVAL_ARG;      // (the full workspace is held: no level can ask for more)
            if (rc != WL_OK) return rc;
        }
        T *coef = Cb;
        if (L == 0) {                                        // every unit is dense: one copy of an N x nb matrix with leading dimension S
            const Strides3 s = {{1, S, 0}};
            const Extent3 ext = {{N, nb, 1}};
            WL_HIP(ctx, generic_copy_box<T>(st, xg, s, yg, s, ext));
            coef = yg;
        }
        rc = batch_sigma_threshold<T>(ctx, st, Cb, coef, n0, N, nb, S, sg, sigma_in ? sigma_in + u0 : nullptr, sigma_out ? sigma_out + u0 : nullptr,
                                      th, t_unit, &madk);
        if (rc != WL_OK) return rc;
        if (L > 0) {
            rc = filter_levels_planes<T>(ctx, st, 0, ndims, dims, nb, S, yg, Cb, taps, L, &kn);
            if (rc == WL_RETRY_GEN) rc = WL_EINVAL_ARG;
            if (rc != WL_OK) return rc;
        }
        return WL_OK;
    }));
    WL_HIP(ctx, hipGetLastError());
    ctx->last_kernel = denoise_label(false, madk);
    return WL_OK;
}

// the same for a lifting scheme: out-of-place forward x -> y, estimate and threshold on y, inverse in place on y (y == x allowed).
// The transforms are those of wl_dwtc_lifting_oop (signals), wl_dwt_lifting_batch (images) and wl_dwt_lifting_batch3 (cubes) with
// their own fallbacks for schemes and strides the fast tiers refuse.  L = 0 with an estimate: the level-1 coefficients of the
// estimate go to a workspace buffer, y is the copy of x.
template <typename T>
int denoise_batch_lifting_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, int64_t nunits, int64_t S,
                               const SchemeArgs &s, int L, int th, double t_unit, const double *sigma_in, double *sigma_out)
{
    const LiftScheme<T> scf = s.build<T>(1), sci = s.build<T>(0);           // the forward and the inverse scheme
    const int64_t n0 = dims[0];
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    const bool est0 = (L == 0 && !sigma_in);
    auto tw_elems = [&](int64_t G) { return ws_lifting_planes_elems(ndims, N, G); };
    auto need = [&](int64_t G) {
        return up256(tw_elems(G) * sizeof(T)) + up256(est0 ? (size_t)G * S * sizeof(T) : 0) + up256((size_t)G * sizeof(double));
    };
    int64_t G = 1;
    int rc = group_reserve(ctx, st, nunits, 65535, need, G);
    if (rc != WL_OK) return rc;
    char *wsb = (char *)ctx->ws;
    T *Cb = (T *)(wsb + up256(tw_elems(G) * sizeof(T)));
    double *sg = (double *)(wsb + up256(tw_elems(G) * sizeof(T)) + up256(est0 ? (size_t)G * S * sizeof(T) : 0));
    const char *madk = "none";
    WL_TRY(for_groups(nunits, G, [&](int64_t u0, int64_t nb) -> int {
        const T *xg = x + u0 * S;
        T *yg = y + u0 * S;
        auto transform = [&](T *dst, const T *src, const LiftScheme<T> &sc, int lev, int fw) {
            return lifting_levels_planes<T>(ctx, st, ndims, n0, nb, S, dst, src, sc, lev, fw);
        };
        if (est0) {
            rc = transform(Cb, xg, scf, 1, 1);
            if (rc != WL_OK) return rc;
        }
        rc = transform(yg, xg, scf, L, 1);                   // (L = 0: a copy unless y == x, as the reference's dwt is)
        if (rc != WL_OK) return rc;
        rc = batch_sigma_threshold<T>(ctx, st, est0 ? Cb : yg, yg, n0, N, nb, S, sg, sigma_in ? sigma_in + u0 : nullptr,
                                      sigma_out ? sigma_out + u0 : nullptr, th, t_unit, &madk);
        if (rc != WL_OK) return rc;
        if (L > 0) {
            rc = transform(yg, yg, sci, L, 0);
            if (rc != WL_OK) return rc;
        }
        return WL_OK;
    }));
    WL_HIP(ctx, hipGetLastError());
    ctx->last_kernel = denoise_label(false, madk);
    return WL_OK;
}

// the argument contract the two denoise_batch entry points share after their pointer / th / t_unit / dtype / wavelet rules
int denoise_batch_check(int ndims, const int64_t *dims, int64_t nunits, int64_t unit_stride, int L, bool estimate)
{
    if (ndims >= 2 && ndims <= 3)
        for (int d = 1; d < ndims; ++d)
            if (dims[d] != dims[0]) return WL_EINVAL_CUBE;   // iscube(x) (denoising.jl:29)
    if (ndims < 1 || ndims > 3 || dims[0] < 1 || nunits < 1) return WL_EDIMS;
    // (a unit of 2^62 elements or more: above every stride an int64 holds)
    if ((ndims == 2 && dims[0] >= ((int64_t)1 << 31)) || (ndims == 3 && dims[0] >= ((int64_t)1 << 21))) return WL_EDIMS;
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    if (unit_stride < N) return WL_EDIMS;
    if (L < 0) return WL_EINVAL_L;
    if (L >= 62 || (dims[0] % ((int64_t)1 << L)) != 0) return WL_EINVAL_SIZE;
    if (estimate && (dims[0] % 2) != 0) return WL_EINVAL_SIZE;                 // noisest needs level 1
    if (estimate && dims[0] >= ((int64_t)1 << 32)) return WL_EINVAL_SIZE;      // (32-bit counters of the per-unit selection)
    return WL_OK;
}

// ---- translation-invariant denoise of a batch of units (wl_denoise_ti_batch_filter / _lifting) ------------
// A plane is one shifted copy of one unit: plane p = u * pns + s is spin s of unit u (unit-major).  A group is the nb planes
// p0 .. p0 + nb - 1, dense in Z (plane stride N); it may begin and end in the middle of a unit.  Unit u sits at x + u * S.
struct TibGeom { int64_t n0, n1, n2, N; int64_t nsp0, nsp1, nsp2, pns; int64_t S, p0, nb; };
// a / b for a >= 0, b > 0: one 32-bit division where both fit (every shape these kernels exist for)
__device__ __forceinline__ int64_t tib_div(int64_t a, int64_t b)
{
    return (((uint64_t)a | (uint64_t)b) >> 32) == 0 ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}
// ti_shift_of for spin s < pns
__device__ __forceinline__ void tib_shift_of(const TibGeom &g, int64_t s, int64_t &s0, int64_t &s1, int64_t &s2)
{
    const int64_t q0 = tib_div(s, g.nsp0), r0 = s - q0 * g.nsp0;
    const int64_t q1 = tib_div(q0, g.nsp1), r1 = q0 - q1 * g.nsp1;
    s0 = r0 - tib_div(r0, g.n0) * g.n0;
    s1 = r1 - tib_div(r1, g.n1) * g.n1;
    s2 = q1 - tib_div(q1, g.n2) * g.n2;
}
// Z[z] = circshift(x_u, +shift(s)) for the planes z < nb of a group, p0 + z = u * pns + s.  The work of the whole group is indexed
// flat -- item = four consecutive rows of one column of one plane, consecutive lanes take consecutive items across columns and
// planes -- so a 64-sample plane costs 16 lanes, not a workgroup.  16-byte stores where n0 % 4 == 0 and Z's base allows them, the
// shifted reads are four scalar loads from a contiguous run (k_ti_shift).
template <typename T>
__global__ void __launch_bounds__(256) k_ti_shift_units(T *__restrict__ Z, const T *__restrict__ x, TibGeom g)
{
    typedef T V4 __attribute__((ext_vector_type(4)));
    const int64_t ipc = (g.n0 + 3) >> 2, ncol = g.n1 * g.n2, ipp = ipc * ncol, total = ipp * g.nb;
    const bool vec = (g.n0 & 3) == 0 && (reinterpret_cast<uintptr_t>(Z) % (4 * sizeof(T))) == 0;
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += nthr) {
        const int64_t z = tib_div(it, ipp), r = it - z * ipp;
        const int64_t c = (ncol == 1) ? 0 : tib_div(r, ipc), i0 = 4 * (r - c * ipc);
        const int64_t p = g.p0 + z, u = tib_div(p, g.pns);
        int64_t s0, s1, s2;
        tib_shift_of(g, p - u * g.pns, s0, s1, s2);
        const int64_t i2 = (ncol == 1) ? 0 : tib_div(c, g.n1), i1 = c - i2 * g.n1;
        int64_t j1 = i1 - s1, j2 = i2 - s2;
        if (j1 < 0) j1 += g.n1;
        if (j2 < 0) j2 += g.n2;
        const T *src = x + u * g.S + g.n0 * (j1 + g.n1 * j2);
        T *dst = Z + z * g.N + g.n0 * c + i0;
        T v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int64_t j0 = i0 + e - s0;
            if (j0 < 0) j0 += g.n0;
            v[e] = (i0 + e < g.n0) ? src[j0] : (T)0;
        }
        if (vec) {
            *reinterpret_cast<V4 *>(dst) = V4{v[0], v[1], v[2], v[3]};
        } else {
            for (int e = 0; e < 4 && i0 + e < g.n0; ++e) dst[e] = v[e];
        }
    }
}
// threshold!(c_z, th, sigma[(p0 + z) / pns] * t_unit) on the nb dense planes of a group: the product in Float64 as k_threshold_units
// forms it, the group indexed flat.  vec_ok: N is a multiple of the 16-byte vector and c is aligned, so no vector straddles two planes.
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_threshold_planes(T *__restrict__ c, int64_t N, int64_t nb, int64_t p0, int64_t pns, int th,
                                                                  const double *__restrict__ sigma, double t_unit, int vec_ok)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec_ok) {
        VT *cv = reinterpret_cast<VT *>(c);
        const int64_t vpp = N / V, nv = vpp * nb;
        for (int64_t i = gid; i < nv; i += nthr) {
            const double t = sigma[tib_div(p0 + tib_div(i, vpp), pns)] * t_unit;
            VT v = cv[i];
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = threshold_one<T, double>(v[e], th, t);
            cv[i] = v;
        }
    } else {
        const int64_t n = N * nb;
        for (int64_t i = gid; i < n; i += nthr) {
            const double t = sigma[tib_div(p0 + tib_div(i, N), pns)] * t_unit;
            c[i] = threshold_one<T, double>(c[i], th, t);
        }
    }
}
// For every unit u the group touches: y_u (+)= circshift(Z[z], -shift(s)) over the unit's planes of the group IN ASCENDING SPIN ORDER
// (arrayadd! once per spin, the reference's summation order), starting from (T)0 when the group holds the unit's spin 0 and from the
// stored y_u otherwise (k_ti_accumulate's rule); when the group holds the unit's last spin the rounded sum is scaled by inv = 1 / pns
// (k_rmul's expression on the value k_rmul would read).  Flat over the elements of the touched units: consecutive lanes own
// consecutive elements, so every shifted plane is read along contiguous runs and a 64-sample unit costs one wave.  The shifts depend
// on the spin alone: they sit in LDS, 256 spins at a time (a unit may have more), the planes are read eight at a time, loads before
// the adds.  Every loop with a barrier has a trip count that is uniform in the workgroup.
template <typename T>
__global__ void __launch_bounds__(256) k_ti_accumulate_units(T *__restrict__ y, const T *__restrict__ Z, TibGeom g, double inv)
{
    __shared__ int sh0[256], sh1[256], sh2[256];
    const int64_t u_lo = g.p0 / g.pns, u_hi = (g.p0 + g.nb - 1) / g.pns, pend = g.p0 + g.nb;
    const int64_t total = (u_hi - u_lo + 1) * g.N, ncol = g.n1 * g.n2;
    const bool one_table = g.pns <= 256;
    auto fill = [&](int64_t sb) {
        const int64_t s = sb + threadIdx.x;
        if (s < g.pns) {
            int64_t s0, s1, s2;
            tib_shift_of(g, s, s0, s1, s2);
            sh0[threadIdx.x] = (int)s0;
            sh1[threadIdx.x] = (int)s1;
            sh2[threadIdx.x] = (int)s2;
        }
    };
    if (one_table) {
        fill(0);
        __syncthreads();
    }
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = base + threadIdx.x;
        const bool live = e < total;
        int64_t i0 = 0, i1 = 0, i2 = 0, pu = 0, slo = 0, shi = 0;
        T *yp = y;
        T acc = (T)0;
        if (live) {
            const int64_t ul = tib_div(e, g.N), r = e - ul * g.N, u = u_lo + ul;
            const int64_t c = (ncol == 1) ? 0 : tib_div(r, g.n0);
            i0 = r - c * g.n0;
            i2 = (ncol == 1) ? 0 : tib_div(c, g.n1);
            i1 = c - i2 * g.n1;
            pu = u * g.pns;
            slo = (g.p0 > pu ? g.p0 : pu) - pu;
            shi = (pend < pu + g.pns ? pend : pu + g.pns) - pu;
            yp = y + u * g.S + r;
            if (slo != 0) acc = *yp;
        }
        for (int64_t sb = 0; sb < g.pns; sb += 256) {
            if (!one_table) {
                __syncthreads();
                fill(sb);
                __syncthreads();
            }
            if (!live) continue;
            const int64_t a = slo > sb ? slo : sb, b = shi < sb + 256 ? shi : sb + 256;
            for (int64_t s8 = a; s8 < b; s8 += 8) {
                T v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (s8 + k < b) {
                        const int t = (int)(s8 + k - sb);
                        int64_t j0 = i0 + sh0[t], j1 = i1 + sh1[t], j2 = i2 + sh2[t];
                        if (j0 >= g.n0) j0 -= g.n0;
                        if (j1 >= g.n1) j1 -= g.n1;
                        if (j2 >= g.n2) j2 -= g.n2;
                        v[k] = Z[(pu + s8 + k - g.p0) * g.N + g.n0 * (j1 + g.n1 * j2) + j0];
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (s8 + k < b) acc = acc + v[k];
            }
        }
        if (live) {
            if (shi == g.pns) acc = (T)((double)acc * inv);
            *yp = acc;
        }
    }
}

// The sequence the two entry points share.  tw_elems(G): the transform workspace of G planes (and of up to G unshifted units of the
// estimate); est(C, xg, nu): level-1 forward of nu units at stride S, xg -> C; fwd / inv(dst, src, nb): all L levels of nb dense planes.
// l0_copies: the transforms are called at L = 0 too (the lifting transforms copy then, as the single call's do); otherwise L = 0
// thresholds the shifted copy itself (denoise_ti_impl).
template <typename T, typename TW, typename Est, typename Fwd, typename Inv>
int denoise_ti_batch_run(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, int64_t nunits, int64_t S, int L, int th,
                         double t_unit, const int64_t *nspin, const double *sigma_in, double *sigma_out, bool l0_copies, TW tw_elems, Est est,
                         Fwd fwd, Inv inv)
{
    TibGeom g;
    g.n0 = dims[0]; g.n1 = (ndims >= 2) ? dims[1] : 1; g.n2 = (ndims == 3) ? dims[2] : 1; g.N = g.n0 * g.n1 * g.n2;
    g.nsp0 = nspin[0]; g.nsp1 = (ndims >= 2) ? nspin[1] : 1; g.nsp2 = (ndims == 3) ? nspin[2] : 1; g.pns = g.nsp0 * g.nsp1 * g.nsp2;
    g.S = S;
    const int64_t N = g.N, pns = g.pns, nplanes = nunits * pns;
    // units per group of the estimate: as many as a group has planes; their level-1 coefficients (stride S) share the planes' buffers
    auto est_units = [&](int64_t G) { return G < nunits ? G : nunits; };
    auto zx_elems = [&](int64_t G) {
        const size_t a = (size_t)2 * N * G, b = sigma_in ? 0 : (size_t)est_units(G) * S;
        return a > b ? a : b;
    };
    auto need = [&](int64_t G) { return up256(tw_elems(G) * sizeof(T)) + up256(zx_elems(G) * sizeof(T)) + up256((size_t)nunits * sizeof(double)); };
    int64_t G = 1;
    int rc = group_reserve(ctx, st, nplanes, 65535, need, G);
    if (rc != WL_OK) return rc;
    double *sg = (double *)((char *)ctx->ws + up256(tw_elems(G) * sizeof(T)) + up256(zx_elems(G) * sizeof(T)));     // (where the held G puts it)
    T *Z = (T *)((char *)ctx->ws + up256(tw_elems(G) * sizeof(T)));
    const long long lower = opt("WL_TI_BATCH_GROUP", 0);
    if (lower >= 1 && lower < G) G = lower;                  // (the buffers stay carved for the G that was reserved)
    else G = (nplanes + (nplanes + G - 1) / G - 1) / ((nplanes + G - 1) / G);     // the same number of groups, of even size
    T *XT = Z + N * G;
    // ---- the sigmas of all units ----
    const char *madk = "none";
    if (sigma_in) {
        const int64_t chunk = (int64_t)65535 * EXT_THREADS;
        for (int64_t u0 = 0; u0 < nunits; u0 += chunk)
            WL_TRY(batch_sigma<T>(ctx, st, nullptr, g.n0, (nunits - u0 < chunk) ? (nunits - u0) : chunk, S, sg + u0, sigma_in + u0,
                                  sigma_out ? sigma_out + u0 : nullptr, &madk));
    } else {
        WL_TRY(for_groups(nunits, est_units(G), [&](int64_t u0, int64_t nu) -> int {
            WL_TRY(est(Z, x + u0 * S, nu));
            return batch_sigma<T>(ctx, st, Z, g.n0, nu, S, sg + u0, nullptr, sigma_out ? sigma_out + u0 : nullptr, &madk);
        }));
    }
    // ---- the planes, G at a time ----
    const bool transforms = L > 0 || l0_copies;
    const int vec_th = ((N * sizeof(T)) % 16) == 0 ? 1 : 0;
    WL_TRY(for_groups(nplanes, G, [&](int64_t p0, int64_t nb) -> int {
        g.p0 = p0; g.nb = nb;
        const int64_t items = ((g.n0 + 3) >> 2) * g.n1 * g.n2 * nb;
        hipLaunchKernelGGL((k_ti_shift_units<T>), dim3(ext_blocks(items, 1, ctx->cu_count)), dim3(256), 0, st, Z, x, g);
        if (transforms) WL_TRY(fwd(XT, Z, nb));
        T *const coef = transforms ? XT : Z;
        hipLaunchKernelGGL((k_threshold_planes<T>), dim3(ext_blocks(N * nb, 16 / sizeof(T), ctx->cu_count)), dim3(EXT_THREADS), 0, st, coef, N, nb, p0,
                           pns, th, sg, t_unit, vec_th & vec_ok16(coef));
        if (transforms) WL_TRY(inv(Z, XT, nb));
        const int64_t touched = ((p0 + nb - 1) / pns - p0 / pns + 1) * N;
        hipLaunchKernelGGL((k_ti_accumulate_units<T>), dim3(ext_blocks(touched, 1, ctx->cu_count)), dim3(256), 0, st, y, Z, g, 1.0 / (double)pns);
        return WL_OK;
    }));
    WL_HIP(ctx, hipGetLastError());
    ctx->last_kernel = denoise_label(true, madk);
    return WL_OK;
}

template <typename T>
int denoise_ti_batch_filter_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, int64_t nunits, int64_t S,
                                 const double *qmf, int flen, int L, int th, double t_unit, const int64_t *nspin, const double *sigma_in,
                                 double *sigma_out)
{
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    const Taps<T> taps = taps_of<T>(qmf, flen);
    const char *kn = nullptr;
    auto tw_elems = [&](int64_t G) { return ws_filter_planes_elems(ndims, N, G); };
    // all `lev` levels of nb lines / images / cubes with plane stride ps
    auto levels = [&](bool fw, T *dst, const T *src, int64_t nb, int64_t ps, int lev) {
        const int rc = filter_levels_planes<T>(ctx, st, fw ? 1 : 0, ndims, dims, nb, ps, dst, src, taps, lev, &kn);
        return rc == WL_RETRY_GEN ? WL_EINVAL_ARG : rc;      // (the full workspace is held: no level can ask for more)
    };
    return denoise_ti_batch_run<T>(ctx, st, y, x, ndims, dims, nunits, S, L, th, t_unit, nspin, sigma_in, sigma_out, false, tw_elems,
                                   [&](T *C, const T *xg, int64_t nu) { return levels(true, C, xg, nu, S, 1); },
                                   [&](T *dst, const T *src, int64_t nb) { return levels(true, dst, src, nb, N, L); },
                                   [&](T *dst, const T *src, int64_t nb) { return levels(false, dst, src, nb, N, L); });
}

template <typename T>
int denoise_ti_batch_lifting_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int ndims, const int64_t *dims, int64_t nunits, int64_t S,
                                  const SchemeArgs &s, int L, int th, double t_unit, const int64_t *nspin, const double *sigma_in,
                                  double *sigma_out)
{
    const LiftScheme<T> scf = s.build<T>(1), sci = s.build<T>(0);           // the forward and the inverse scheme
    const int64_t n0 = dims[0];
    int64_t N = 1;
    for (int d = 0; d < ndims; ++d) N *= dims[d];
    auto tw_elems = [&](int64_t G) { return ws_lifting_planes_elems(ndims, N, G); };
    // nb lines of one batched call / nb images as the third extent / nb cubes as one batch of volumes, plane stride ps
    auto transform = [&](T *dst, const T *src, int64_t nb, int64_t ps, const LiftScheme<T> &sc, int lev, int fw) {
        return lifting_levels_planes<T>(ctx, st, ndims, n0, nb, ps, dst, src, sc, lev, fw);
    };
    return denoise_ti_batch_run<T>(ctx, st, y, x, ndims, dims, nunits, S, L, th, t_unit, nspin, sigma_in, sigma_out, true, tw_elems,
                                   [&](T *C, const T *xg, int64_t nu) { return transform(C, xg, nu, S, scf, 1, 1); },
                                   [&](T *dst, const T *src, int64_t nb) { return transform(dst, src, nb, N, scf, L, 1); },
                                   [&](T *dst, const T *src, int64_t nb) { return transform(dst, src, nb, N, sci, L, 0); });
}

// the rules the two denoise_ti_batch entry points share after their pointer / th / t_unit / dtype / wavelet rules: those of
// denoise_batch_check with nspin in the WL_EDIMS group and the extent limits of denoise_ti_check in the WL_EINVAL_SIZE group
int denoise_ti_batch_check(int ndims, const int64_t *dims, int64_t nunits, int64_t unit_stride, int L, bool estimate, const int64_t *nspin)
{
    const int rc = denoise_batch_check(ndims, dims, nunits, unit_stride, L, estimate);
    if (rc == WL_EINVAL_CUBE || rc == WL_EDIMS) return rc;
    int64_t planes = nunits;
    for (int d = 0; d < ndims; ++d)
        if (nspin[d] < 1 || __builtin_mul_overflow(planes, nspin[d], &planes)) return WL_EDIMS;
    if (rc != WL_OK) return rc;
    if (ndims == 3 && dims[0] >= ((int64_t)1 << 20)) return WL_EINVAL_SIZE;
    if (ndims == 2 && dims[1] > 65535) return WL_EINVAL_SIZE;
    return WL_OK;
}

}  // namespace

extern "C" {

int wl_threshold(wl_ctx *ctx, int dtype, void *x, int64_t n, int th, double t, int t_is_f64, void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!x && n > 0) return WL_EINVAL_ARG;
    if (th < WL_TH_HARD || th > WL_TH_NEG) return WL_EINVAL_ARG;
    if (th <= WL_TH_STEIN && !(t >= 0)) return WL_EINVAL_ARG;           // @assert t >= 0
    if (n <= 0) return WL_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = ext_blocks(n, 4, ctx->cu_count);
    // the threshold is a Float64 for Float64 data; for Float32 data it is what the caller holds (t_is_f64)
    by_dtype(dtype, [&](auto e) {
        using T = decltype(e);
        if (sizeof(T) == 8 || t_is_f64) hipLaunchKernelGGL((k_threshold<T, double>), dim3(nb), dim3(EXT_THREADS), 0, st, (T *)x, n, th, t, vec_ok16(x));
        else hipLaunchKernelGGL((k_threshold<T, T>), dim3(nb), dim3(EXT_THREADS), 0, st, (T *)x, n, th, (T)t, vec_ok16(x));
    });
    WL_HIP(ctx, hipGetLastError());
    ctx->last_kernel = "k_threshold";
    return WL_OK;
}

int wl_threshold_biggest(wl_ctx *ctx, int dtype, void *x, int64_t n, int64_t m, void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if ((!x && n > 0) || m < 0) return WL_EINVAL_ARG;
    if (n <= 0) return WL_OK;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return biggest_impl<T>(ctx, st, (T *)x, n, m);
    });
}

int wl_median(wl_ctx *ctx, int dtype, const void *v, int64_t n, double *result, void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!v || !result) return WL_EINVAL_ARG;
    if (n < 1) return WL_EDIMS;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (n <= mad_lds_max<T>()) return mad_small<T>(ctx, st, (T *)const_cast<void *>(v), n, 0, result);    // (does not write v when do_mad == 0)
        return median_impl<T>(ctx, st, (const T *)v, n, result, (T *)nullptr);
    });
}

int wl_mad(wl_ctx *ctx, int dtype, void *y, int64_t n, double *result, void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!y || !result) return WL_EINVAL_ARG;
    if (n < 1) return WL_EDIMS;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return mad_one<T>(ctx, st, (T *)y, n, result);
    });
}

// the rules wl_denoise_ti_* share behind their pointer / ndims (/ filter length) rules, in their order
static int denoise_ti_check(const void *y, const void *x, int ndims, const int64_t *dims, int L, int th, double t_unit, const int64_t *nspin,
                            double sigma_host)
{
    // threshold!(xt, dnt.th, sigma*t) (denoising.jl:58) has methods for Hard / Soft / Semisoft / Stein only (threshold_main.jl:21-80)
    if (th < WL_TH_HARD || th > WL_TH_STEIN) return WL_EINVAL_ARG;
    // a custom estimator's value: NaN trips the reference's `@assert t >= 0` (threshold_main.jl:24) and so does Inf * 0; +Inf
    // alone passes it -- every coefficient is thresholded -- and is accepted here as well (negative = "estimate on the device")
    if (sigma_host != sigma_host || (sigma_host >= 0 && !(sigma_host * t_unit >= 0))) return WL_EINVAL_ARG;
    for (int d = 0; d < ndims; ++d)
        if (dims[d] < 1 || nspin[d] < 1) return WL_EDIMS;
    if (ndims >= 2 && dims[0] != dims[1]) return WL_EINVAL_CUBE;            // iscube(x) (denoising.jl:29)
    if (ndims == 3 && dims[0] != dims[2]) return WL_EINVAL_CUBE;
    if (ndims == 3 && dims[0] >= ((int64_t)1 << 20)) return WL_EINVAL_SIZE; // (32-bit extents and column counts in the shift kernels)
    if (ndims == 2 && dims[1] > 65535) return WL_EINVAL_SIZE;               // (one grid row per column in the shift kernels)
    if (L < 0) return WL_EINVAL_L;
    for (int d = 0; d < ndims; ++d)
        if (L >= 62 || (dims[d] % ((int64_t)1 << L)) != 0) return WL_EINVAL_SIZE;
    if (y == x) return WL_EALIAS;
    if (!(t_unit >= 0)) return WL_EINVAL_ARG;
    return WL_OK;
}

int wl_denoise_ti_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, const double *qmf, int flen,
                         int L, int th, double t_unit, const int64_t *nspin, double sigma_host, void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!y || !x || !dims || !qmf || !nspin) return WL_EINVAL_ARG;
    if (ndims < 1 || ndims > 3) return WL_EDIMS;
    WL_TRY(check_flen(flen));
    WL_TRY(denoise_ti_check(y, x, ndims, dims, L, th, t_unit, nspin, sigma_host));
    hipStream_t st = (hipStream_t)stream;
    const int rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return denoise_ti_impl<T>(ctx, st, (T *)y, (const T *)x, ndims, dims, qmf, flen, L, th, t_unit, nspin, sigma_host);
    });
    int64_t pns = 1;
    for (int d = 0; d < ndims; ++d) pns *= nspin[d];
    if (rc == WL_OK && pns > 1) ctx->last_kernel = "denoise_ti_batch";       // (one spin: "denoise_one_spin", set by the branch that ran)
    return rc;
}

int wl_denoise_ti_lifting(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims,
                          int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef, const int32_t *step_shift,
                          const double *coefs_flat, double norm1, double norm2,
                          int L, int th, double t_unit, const int64_t *nspin, double sigma_host, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!y || !x || !dims || !nspin) return WL_EINVAL_ARG;
    if (ndims < 1 || ndims > 3) return WL_EDIMS;
    WL_TRY(denoise_ti_check(y, x, ndims, dims, L, th, t_unit, nspin, sigma_host));
    WL_TRY(s.check());
    hipStream_t st = (hipStream_t)stream;
    WL_TRY(by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return denoise_ti_lifting_impl<T>(ctx, st, (T *)y, (const T *)x, ndims, dims, s, L, th, t_unit, nspin, sigma_host);
    }));
    ctx->last_kernel = "denoise_ti_lifting";
    return WL_OK;
}

int wl_mad_batch(wl_ctx *ctx, int dtype, void *y, int64_t n, int64_t nunits, int64_t stride, double *result, void *stream)
{
    if (!ctx || !y || !result) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    if (n < 1 || nunits < 1 || stride < n) return WL_EDIMS;
    if (n >= ((int64_t)1 << 31)) return WL_EINVAL_SIZE;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return mad_units<T>(ctx, st, (T *)y, n, nunits, stride, 1, result, &ctx->last_kernel);
    });
}

int wl_denoise_batch_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, int64_t nunits,
                            int64_t unit_stride, const double *qmf, int flen, int L, int th, double t_unit, const double *sigma_in,
                            double *sigma_out, void *stream)
{
    if (!ctx || !y || !x || !dims || !qmf) return WL_EINVAL_ARG;
    // threshold!(c, dnt.th, sigma * t) (denoising.jl:74) has methods for Hard / Soft / Semisoft / Stein only; @assert t >= 0
    if (th < WL_TH_HARD || th > WL_TH_STEIN || !(t_unit >= 0)) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    WL_TRY(denoise_batch_check(ndims, dims, nunits, unit_stride, L, sigma_in == nullptr));
    if (y == x) return WL_EALIAS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return denoise_batch_filter_impl<T>(ctx, st, (T *)y, (const T *)x, ndims, dims, nunits, unit_stride, qmf, flen, L, th, t_unit, sigma_in,
                                            sigma_out);
    });
}

int wl_denoise_batch_lifting(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, int64_t nunits,
                             int64_t unit_stride, int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                             const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2, int L, int th, double t_unit,
                             const double *sigma_in, double *sigma_out, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || !x || !dims) return WL_EINVAL_ARG;
    if (th < WL_TH_HARD || th > WL_TH_STEIN || !(t_unit >= 0)) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(s.check());
    WL_TRY(denoise_batch_check(ndims, dims, nunits, unit_stride, L, sigma_in == nullptr));
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return denoise_batch_lifting_impl<T>(ctx, st, (T *)y, (const T *)x, ndims, dims, nunits, unit_stride, s, L, th, t_unit, sigma_in, sigma_out);
    });
}

int wl_denoise_ti_batch_filter(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, int64_t nunits,
                               int64_t unit_stride, const double *qmf, int flen, int L, int th, double t_unit, const int64_t *nspin,
                               const double *sigma_in, double *sigma_out, void *stream)
{
    if (!ctx || !y || !x || !dims || !qmf || !nspin) return WL_EINVAL_ARG;
    if (th < WL_TH_HARD || th > WL_TH_STEIN || !(t_unit >= 0)) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    WL_TRY(denoise_ti_batch_check(ndims, dims, nunits, unit_stride, L, sigma_in == nullptr, nspin));
    if (y == x) return WL_EALIAS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return denoise_ti_batch_filter_impl<T>(ctx, st, (T *)y, (const T *)x, ndims, dims, nunits, unit_stride, qmf, flen, L, th, t_unit, nspin,
                                               sigma_in, sigma_out);
    });
}

int wl_denoise_ti_batch_lifting(wl_ctx *ctx, int dtype, void *y, const void *x, int ndims, const int64_t *dims, int64_t nunits,
                                int64_t unit_stride, int nsteps, const int32_t *step_is_update, const int32_t *step_ncoef,
                                const int32_t *step_shift, const double *coefs_flat, double norm1, double norm2, int L, int th, double t_unit,
                                const int64_t *nspin, const double *sigma_in, double *sigma_out, void *stream)
{
    const SchemeArgs s = {nsteps, step_is_update, step_ncoef, step_shift, coefs_flat, norm1, norm2};
    if (!ctx || !y || !x || !dims || !nspin) return WL_EINVAL_ARG;
    if (th < WL_TH_HARD || th > WL_TH_STEIN || !(t_unit >= 0)) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(s.check());
    WL_TRY(denoise_ti_batch_check(ndims, dims, nunits, unit_stride, L, sigma_in == nullptr, nspin));
    if (y == x) return WL_EALIAS;                            // (x is re-read for every group of spins)
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return denoise_ti_batch_lifting_impl<T>(ctx, st, (T *)y, (const T *)x, ndims, dims, nunits, unit_stride, s, L, th, t_unit, nspin, sigma_in,
                                                sigma_out);
    });
}

int wl_circshift(wl_ctx *ctx, int dtype, void *b, const void *a, int ndims, const int64_t *dims, const int64_t *shift, void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!b || !a || !dims || !shift) return WL_EINVAL_ARG;
    if (ndims < 1 || ndims > 3) return WL_EDIMS;
    if (b == a) return WL_EALIAS;
    Shift3 p = {{1, 1, 1}, {0, 0, 0}};
    int64_t n = 1;
    for (int k = 0; k < ndims; ++k) {
        if (dims[k] < 1) return (dims[k] == 0) ? WL_OK : WL_EDIMS;
        p.d[k] = dims[k];
        p.s[k] = ((shift[k] % dims[k]) + dims[k]) % dims[k];
        n *= dims[k];
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = ext_blocks(n, 4, ctx->cu_count);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_circshift<T>), dim3(nb), dim3(EXT_THREADS), 0, st, (T *)b, (const T *)a, n, p);
    });
    WL_HIP(ctx, hipGetLastError());
    return WL_OK;
}

int wl_arrayadd(wl_ctx *ctx, int dtype, void *y, const void *z, int64_t n, void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if ((!y || !z) && n > 0) return WL_EINVAL_ARG;
    if (n <= 0) return WL_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = ext_blocks(n, 4, ctx->cu_count);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_arrayadd<T>), dim3(nb), dim3(EXT_THREADS), 0, st, (T *)y, (const T *)z, n, vec_ok16(y) & vec_ok16(z));
    });
    WL_HIP(ctx, hipGetLastError());
    return WL_OK;
}

int wl_rmul(wl_ctx *ctx, int dtype, void *y, int64_t n, double s, void *stream)
{
    WL_TRY(ext_enter(ctx, dtype));
    WL_SCOPE(ctx);
    if (!y && n > 0) return WL_EINVAL_ARG;
    if (n <= 0) return WL_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = ext_blocks(n, 4, ctx->cu_count);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_rmul<T>), dim3(nb), dim3(EXT_THREADS), 0, st, (T *)y, n, s, vec_ok16(y));
    });
    WL_HIP(ctx, hipGetLastError());
    return WL_OK;
}

}  // extern "C"

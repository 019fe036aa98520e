// wl_thbatch.hip -- threshold! of a batch of independent units, everything on the device:
//   wl_threshold_batch           threshold!(x_u, TH, t_u), the six element-wise kinds, one launch over all units (a workgroup row per
//                                unit, or a wave per unit of at most 256 elements)
//   wl_threshold_biggest_batch   threshold!(x_u, BiggestTH(), m_u): the best m-term approximation of every unit
// Unit u is x[u * unit_stride .. + n); the padding between units is never read or written.  Neither call synchronises or brings a
// counter back to the host.  The single calls (wl_threshold, wl_threshold_biggest: wl_ext.hip) launch none of these kernels.
//
// BiggestTH of one unit, as wl_threshold_biggest computes it: a = the (n - m)-th smallest |x| (radix select on the abs-mode keys:
// NaN above every finite magnitude), less / equal = the counts of |x| < a and |x| == a (floating-point compares, so nothing
// compares against a NaN cut), then every |x| < a is cleared, and so are the first need = (n - m) - less ties |x| == a in index
// order.  Cleared entries are stored as +0, nothing else is written.  Three tiers by n and nunits:
//   k_thbig_lds      a workgroup per unit, the keys of the unit in LDS: one read of the unit from memory
//   k_thbig_stream   a workgroup per unit, the unit streamed once per radix byte, once for the counts, once for the clear
//   k_thbig_split    several workgroups per unit (few long units), a state block per unit in the workspace, a fixed number of launches
#include "wl_entry.h"
#include "wl_select.h"
#include "wl_dev.h"

using namespace wl;

namespace {

// ---- the element-wise kinds ------------------------------------------------------------------------------------------------
// threshold!(x_u, th, t_u) for unit u = blockIdx.y: t_u = t_dev[u] converted to C (the type the reference's promotion computes in),
// or the scalar t.  16-byte accesses where the unit's base allows them.
template <typename T, typename C>
__global__ void __launch_bounds__(EXT_THREADS) k_threshold_batch(T *__restrict__ x, int64_t n, int64_t stride, int th, C t,
                                                                 const double *__restrict__ t_dev)
{
    T *xu = x + (int64_t)blockIdx.y * stride;
    const C tu = t_dev ? (C)t_dev[blockIdx.y] : t;
    const int vec_ok = (reinterpret_cast<uintptr_t>(xu) & 15) == 0 ? 1 : 0;
    ew_inplace<T>(xu, n, vec_ok, [=](T v, int64_t) { return threshold_one<T, C>(v, th, tu); });
}

// short units (n <= kWaveUnitMax): a wave per unit, four units per workgroup -- a workgroup per unit would leave most of its lanes
// idle and need a launch per 65535 units.  Scalar accesses: a unit of 64 Float32 values is one 256-byte row of the wave.
constexpr int64_t kWaveUnitMax = 256;
template <typename T, typename C>
__global__ void __launch_bounds__(EXT_THREADS) k_threshold_batch_wave(T *__restrict__ x, int n, int64_t nunits, int64_t stride, int th, C t,
                                                                      const double *__restrict__ t_dev)
{
    const int64_t u = (int64_t)blockIdx.x * (EXT_THREADS / 64) + (threadIdx.x >> 6);
    if (u >= nunits) return;
    T *xu = x + u * stride;
    const C tu = t_dev ? (C)t_dev[u] : t;
    for (int i = threadIdx.x & 63; i < n; i += 64) xu[i] = threshold_one<T, C>(xu[i], th, tu);
}

// ---- BiggestTH: what the three tiers share -----------------------------------------------------------------------------------
// the number of entries unit u clears: n - m_u, m_u clamped to [0, n]
__device__ __forceinline__ long long thb_nz(long long n, long long m, const long long *m_dev, long long u)
{
    long long mu = m_dev ? m_dev[u] : m;
    if (mu < 0) mu = 0;
    if (mu > n) mu = n;
    return n - mu;
}

template <typename T>
__device__ __forceinline__ T abs_of(T v) { return v < 0 ? -v : v; }

// one radix byte of the keys of |v[i0 .. i1)| into the 256 LDS bins h: the keys whose higher bytes equal those of prefix.  A lane
// adds a run of equal bins with one atomic (the leading byte of a magnitude is its exponent: a few bins take nearly every element).
template <typename T>
__device__ __forceinline__ void thb_hist_pass(const T *__restrict__ v, int64_t i0, int64_t i1, int pass, typename KeyOf<T>::U prefix,
                                              unsigned int *h)
{
    typedef typename KeyOf<T>::U U;
    constexpr int NB = KeyOf<T>::BYTES;
    const int shift = 8 * (NB - 1 - pass);
    const U q = (pass == 0) ? (U)0 : (U)(prefix >> (shift + 8));
    unsigned cur = 0, run = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const U key = KeyOf<T>::key(v[i], 1);
        const U hi = (pass == 0) ? (U)0 : (U)(key >> (shift + 8));
        if (hi != q) continue;
        const unsigned b = (unsigned)((key >> shift) & 0xff);
        if (b != cur) {
            if (run) atomicAdd(&h[cur], run);
            cur = b;
            run = 0;
        }
        ++run;
    }
    if (run) atomicAdd(&h[cur], run);
}

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// counts of |v| < a and |v| == a over [i0, i1), summed over the wave
template <typename T>
__device__ __forceinline__ void thb_count(const T *__restrict__ v, int64_t i0, int64_t i1, T a, unsigned &less, unsigned &eq)
{
    unsigned l = 0, e = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const T av = abs_of(v[i]);
        l += (av < a);
        e += (av == a);
    }
    less = wave_sum(l);
    eq = wave_sum(e);
}

// The clear of [0, n) by one workgroup: mag(i) = |element i|, zero(i) stores +0 there.  Everything below the cut goes; a tie goes
// when all ties go, or when its index among the unit's ties, in element order, is below need -- `before` ties precede this range.
// The index of a tie: the ties of the sweeps so far (the same number in every thread), those of the lower waves of this sweep
// (wcnt, two sets so that a sweep needs one barrier) and those of the lower lanes (ballot and popcount).  Once need ties are
// behind, the remaining sweeps neither count nor wait.
template <typename T, typename I, typename Mag, typename Zero>
__device__ __forceinline__ void thb_clear(I n, T a, bool all_ties, unsigned long long before, unsigned long long need, unsigned int (*wcnt)[16],
                                          Mag mag, Zero zero)
{
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, w = tid >> 6, nw = nthr >> 6;
    unsigned long long run = before;
    int par = 0;
    for (I base = 0; base < n; base += nthr) {
        const I i = base + tid;
        const bool in = i < n;
        const T av = in ? mag(i) : (T)0;
        const bool tie = in && av == a;
        if (all_ties || run >= need) {
            if (in && (av < a || (all_ties && tie))) zero(i);
            continue;
        }
        const unsigned long long mask = __ballot(tie);
        if (lane == 0) wcnt[par][w] = (unsigned)__popcll(mask);
        __syncthreads();
        unsigned pre = 0, tot = 0;
        for (int k = 0; k < nw; ++k) {
            const unsigned c = wcnt[par][k];
            tot += c;
            if (k < w) pre += c;
        }
        const unsigned long long idx = run + pre + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
        if (in && (av < a || (tie && idx < need))) zero(i);
        run += tot;
        par ^= 1;
    }
}

// ---- the LDS tier: a workgroup per unit, the keys of |x_u| in LDS ---------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(1024) k_thbig_lds(T *x0, int n, int64_t stride, long long m, const long long *__restrict__ m_dev)
{
    typedef typename KeyOf<T>::U U;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    U *keys = reinterpret_cast<U *>(smem_raw);
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long sh[2];
    __shared__ unsigned int cnt[2];
    __shared__ unsigned int wcnt[2][16];
    const long long nz = thb_nz(n, m, m_dev, blockIdx.x);
    if (nz <= 0) return;                                     // (the whole workgroup: nothing of the unit is loaded)
    T *v = x0 + (int64_t)blockIdx.x * stride;
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (tid == 0) cnt[0] = cnt[1] = 0;
    for (int i = tid; i < n; i += nthr) keys[i] = KeyOf<T>::key(v[i], 1);
    __syncthreads();
    const T a = KeyOf<T>::val(lds_select<T, 2>(keys, n, (unsigned long long)(nz - 1), hist, sh), 1);
    unsigned l = 0, e = 0;
    for (int i = tid; i < n; i += nthr) {
        const T av = KeyOf<T>::val(keys[i], 1);
        l += (av < a);
        e += (av == a);
    }
    l = wave_sum(l);
    e = wave_sum(e);
    if ((tid & 63) == 0) {
        if (l) atomicAdd(&cnt[0], l);
        if (e) atomicAdd(&cnt[1], e);
    }
    __syncthreads();
    const unsigned long long need = (unsigned long long)nz - cnt[0];
    thb_clear<T, int>(n, a, need >= cnt[1], 0ull, need, wcnt, [&](int i) { return KeyOf<T>::val(keys[i], 1); }, [&](int i) { v[i] = (T)0; });
}

// ---- the stream tier: a workgroup per unit, the unit read from memory (L2 after the first pass) --------------------------------
// 32-bit counters: n < 2^31.
template <typename T>
__global__ void __launch_bounds__(1024) k_thbig_stream(T *x0, int64_t n, int64_t stride, long long m, const long long *__restrict__ m_dev)
{
    typedef typename KeyOf<T>::U U;
    constexpr int NB = KeyOf<T>::BYTES;
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long pre, rk;
    __shared__ unsigned int cnt[2];
    __shared__ unsigned int wcnt[2][16];
    const long long nz = thb_nz(n, m, m_dev, blockIdx.x);
    if (nz <= 0) return;
    T *v = x0 + (int64_t)blockIdx.x * stride;
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (tid == 0) { pre = 0; rk = (unsigned long long)(nz - 1); cnt[0] = cnt[1] = 0; }
    for (int pass = 0; pass < NB; ++pass) {
        for (int b = tid; b < 256; b += nthr) hist[b] = 0;
        __syncthreads();
        thb_hist_pass<T>(v, 0, n, pass, (U)pre, hist);
        __syncthreads();
        if (tid < 64) wave_pick_bin(hist, tid, 8 * (NB - 1 - pass), &pre, &rk);
        __syncthreads();
    }
    const T a = KeyOf<T>::val((U)pre, 1);
    unsigned l, e;
    thb_count<T>(v, 0, n, a, l, e);
    if ((tid & 63) == 0) {
        if (l) atomicAdd(&cnt[0], l);
        if (e) atomicAdd(&cnt[1], e);
    }
    __syncthreads();
    const unsigned long long need = (unsigned long long)nz - cnt[0];
    thb_clear<T, int64_t>(n, a, need >= cnt[1], 0ull, need, wcnt, [&](int64_t i) { return abs_of(v[i]); }, [&](int64_t i) { v[i] = (T)0; });
}

// ---- the split tier: chunks of a unit to workgroups, the selection state of a unit in the workspace ------------------------------
struct ThbUnit {
    unsigned long long prefix, rank;    // the key bytes resolved so far; the 0-based rank left inside that prefix class
    unsigned long long less, eq;        // counts of |x| < cut and |x| == cut over the unit
    long long nz;                       // entries to clear (0: the unit is skipped by every launch)
    unsigned long long pad[3];
    unsigned long long hist[256];       // the radix byte in flight, zero between launches
};

__global__ void __launch_bounds__(256) k_thb_init(ThbUnit *s, long long n, long long m, const long long *__restrict__ m_dev)
{
    ThbUnit &su = s[blockIdx.x];
    su.hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        const long long nz = thb_nz(n, m, m_dev, blockIdx.x);
        su.prefix = 0; su.rank = (unsigned long long)(nz > 0 ? nz - 1 : 0); su.less = su.eq = 0; su.nz = nz;
    }
}
// grid (chunks, units): the histogram of one radix byte over one chunk, added to the unit's
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_thb_hist(const T *__restrict__ x, int64_t n, int64_t stride, int64_t chunk, int pass, ThbUnit *s)
{
    typedef typename KeyOf<T>::U U;
    __shared__ unsigned int lh[256];
    ThbUnit &su = s[blockIdx.y];
    if (su.nz <= 0) return;
    lh[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = (i0 + chunk < n) ? i0 + chunk : n;
    thb_hist_pass<T>(x + (int64_t)blockIdx.y * stride, i0, i1, pass, (U)su.prefix, lh);
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&su.hist[threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}
// a wave per unit: the bin that holds the rank (wave_pick_bin on 64-bit counts), the prefix extended, the histogram cleared
template <typename T>
__global__ void __launch_bounds__(64) k_thb_scan(int pass, ThbUnit *s)
{
    constexpr int NB = KeyOf<T>::BYTES;
    ThbUnit &su = s[blockIdx.x];
    if (su.nz <= 0) return;
    const int lane = threadIdx.x, shift = 8 * (NB - 1 - pass);
    unsigned long long *h = su.hist;
    const unsigned long long h0 = h[4 * lane], h1 = h[4 * lane + 1], h2 = h[4 * lane + 2], h3 = h[4 * lane + 3];
    h[4 * lane] = h[4 * lane + 1] = h[4 * lane + 2] = h[4 * lane + 3] = 0;
    const unsigned long long mine = h0 + h1 + h2 + h3;
    unsigned long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    const unsigned long long kk = su.rank, excl = incl - mine;
    const unsigned long long hit = __ballot(kk < incl);
    const int first = hit ? (__ffsll((long long)hit) - 1) : 63;      // (no hit cannot happen for a rank below the class size)
    if (lane == first) {
        int b = 4 * lane;
        unsigned long long cum = excl;
        if (kk >= cum + h0) { cum += h0; ++b; if (kk >= cum + h1) { cum += h1; ++b; if (kk >= cum + h2) { cum += h2; ++b; } } }
        su.rank = kk - cum;
        su.prefix = su.prefix | (((unsigned long long)b) << shift);
    }
}
// grid (chunks, units): the chunk's counts against the cut added to the unit's, its ties recorded for the clear
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_thb_count(const T *__restrict__ x, int64_t n, int64_t stride, int64_t chunk, ThbUnit *s,
                                                           unsigned int *__restrict__ ties)
{
    typedef typename KeyOf<T>::U U;
    __shared__ unsigned int cnt[2];
    ThbUnit &su = s[blockIdx.y];
    if (su.nz <= 0) return;
    if (threadIdx.x == 0) cnt[0] = cnt[1] = 0;
    __syncthreads();
    const T a = KeyOf<T>::val((U)su.prefix, 1);
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = (i0 + chunk < n) ? i0 + chunk : n;
    unsigned l, e;
    thb_count<T>(x + (int64_t)blockIdx.y * stride, i0, i1, a, l, e);
    if ((threadIdx.x & 63) == 0) {
        if (l) atomicAdd(&cnt[0], l);
        if (e) atomicAdd(&cnt[1], e);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (cnt[0]) atomicAdd(&su.less, (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(&su.eq, (unsigned long long)cnt[1]);
        ties[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = cnt[1];
    }
}
// grid (chunks, units): the clear of one chunk; the ties ahead of it = the sum of the lower chunks' tie counts
template <typename T>
__global__ void __launch_bounds__(EXT_THREADS) k_thb_clear(T *__restrict__ x, int64_t n, int64_t stride, int64_t chunk, const ThbUnit *__restrict__ s,
                                                           const unsigned int *__restrict__ ties)
{
    typedef typename KeyOf<T>::U U;
    __shared__ unsigned long long before_s;
    __shared__ unsigned int wcnt[2][16];
    const ThbUnit &su = s[blockIdx.y];
    if (su.nz <= 0) return;
    const T a = KeyOf<T>::val((U)su.prefix, 1);
    const unsigned long long need = (unsigned long long)su.nz - su.less;
    const bool all_ties = need >= su.eq;
    unsigned long long before = 0;
    if (!all_ties) {
        if (threadIdx.x == 0) before_s = 0;
        __syncthreads();
        const unsigned int *tu = ties + (int64_t)blockIdx.y * gridDim.x;
        unsigned long long part = 0;
        for (unsigned c = threadIdx.x; c < blockIdx.x; c += blockDim.x) part += tu[c];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
        if ((threadIdx.x & 63) == 0 && part) atomicAdd(&before_s, part);
        __syncthreads();
        before = before_s;
    }
    const int64_t i0 = (int64_t)blockIdx.x * chunk, len = ((i0 + chunk < n) ? i0 + chunk : n) - i0;
    T *v = x + (int64_t)blockIdx.y * stride + i0;
    thb_clear<T, int64_t>(len, a, all_ties, before, need, wcnt, [&](int64_t i) { return abs_of(v[i]); }, [&](int64_t i) { v[i] = (T)0; });
}

// ---- hosts --------------------------------------------------------------------------------------------------------------------
template <typename T>
int threshold_batch_impl(wl_ctx *ctx, hipStream_t st, T *x, int64_t n, int64_t nunits, int64_t stride, int th, double t, const double *t_dev,
                         int t_is_f64)
{
    if (!t_dev && stride == n) {                            // one threshold, no padding: one unit of n * nunits elements
        n *= nunits;
        stride = n;
        nunits = 1;
    }
    // the threshold is a Float64 for Float64 data; for Float32 data it is what the caller holds (t_is_f64)
    const bool wide = sizeof(T) == 8 || t_is_f64;
    if (nunits > 1 && n <= kWaveUnitMax) {
        const int64_t per = (int64_t)1 << 30;               // units per launch (gridDim.x)
        for (int64_t u0 = 0; u0 < nunits; u0 += per) {
            const int64_t nb = (nunits - u0 < per) ? (nunits - u0) : per;
            const dim3 grid((unsigned)((nb + EXT_THREADS / 64 - 1) / (EXT_THREADS / 64)));
            if (wide)
                hipLaunchKernelGGL((k_threshold_batch_wave<T, double>), grid, dim3(EXT_THREADS), 0, st, x + u0 * stride, (int)n, nb, stride, th, t,
                                   t_dev ? t_dev + u0 : nullptr);
            else
                hipLaunchKernelGGL((k_threshold_batch_wave<T, T>), grid, dim3(EXT_THREADS), 0, st, x + u0 * stride, (int)n, nb, stride, th, (T)t,
                                   t_dev ? t_dev + u0 : nullptr);
        }
        WL_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "k_threshold_batch_wave";
        return WL_OK;
    }
    const int64_t lim = 65535;                               // (gridDim.y)
    for (int64_t u0 = 0; u0 < nunits; u0 += lim) {
        const int64_t nb = (nunits - u0 < lim) ? (nunits - u0) : lim;
        int64_t bx = ext_blocks(n, 4, ctx->cu_count);
        const int64_t cap = (int64_t)ctx->cu_count * 64;
        if (bx * nb > cap) bx = (cap / nb > 1) ? cap / nb : 1;
        const dim3 grid((unsigned)bx, (unsigned)nb);
        if (wide)
            hipLaunchKernelGGL((k_threshold_batch<T, double>), grid, dim3(EXT_THREADS), 0, st, x + u0 * stride, n, stride, th, t,
                               t_dev ? t_dev + u0 : nullptr);
        else
            hipLaunchKernelGGL((k_threshold_batch<T, T>), grid, dim3(EXT_THREADS), 0, st, x + u0 * stride, n, stride, th, (T)t,
                               t_dev ? t_dev + u0 : nullptr);
    }
    WL_HIP(ctx, hipGetLastError());
    ctx->last_kernel = "k_threshold_batch";
    return WL_OK;
}

// The tier of a batch depends on n and nunits only.  Options: WL_THB_LDS_MAX (the longest unit of the LDS tier, at most and by
// default mad_lds_max; 0 = never), WL_THB_SPLIT_N / WL_THB_SPLIT_UNITS (the split tier takes units of at least SPLIT_N elements
// in batches of at most SPLIT_UNITS units), WL_THB_CHUNK (elements per workgroup of the split tier).
template <typename T>
int biggest_batch_impl(wl_ctx *ctx, hipStream_t st, T *x, int64_t n, int64_t nunits, int64_t stride, int64_t m, const int64_t *m_dev)
{
    const long long *md = reinterpret_cast<const long long *>(m_dev);
    int64_t lim = (int64_t)opt("WL_THB_LDS_MAX", (long long)mad_lds_max<T>());
    if (lim > mad_lds_max<T>()) lim = mad_lds_max<T>();       // (the keys must fit the 64 KiB of LDS a kernel gets)
    // defaults: where the two tiers cross in profiles/threshold_batch.md (between 2^16 and 2^17 elements for 1, 16 and 256 units;
    // larger batches were not measured and stay on the stream tier, which then has several workgroups per CU)
    const int64_t split_n = (int64_t)opt("WL_THB_SPLIT_N", (long long)1 << 17), split_units = (int64_t)opt("WL_THB_SPLIT_UNITS", 256);
    const bool lds = n <= lim;
    const bool split = !lds && (n >= ((int64_t)1 << 31) || (n >= split_n && nunits <= split_units));
    if (!split) {
        const int64_t per = (int64_t)1 << 20;               // (grid size * block size stays below 2^32)
        for (int64_t u0 = 0; u0 < nunits; u0 += per) {
            const unsigned nb = (unsigned)((nunits - u0 < per) ? (nunits - u0) : per);
            if (lds) {
                const int threads = n >= 2048 ? 1024 : (n >= 256 ? 256 : 64);
                hipLaunchKernelGGL((k_thbig_lds<T>), dim3(nb), dim3(threads), (size_t)n * sizeof(typename KeyOf<T>::U), st, x + u0 * stride, (int)n,
                                   stride, (long long)m, md ? md + u0 : nullptr);
            } else {
                const int threads = n >= 4096 ? 1024 : 256;
                hipLaunchKernelGGL((k_thbig_stream<T>), dim3(nb), dim3(threads), 0, st, x + u0 * stride, n, stride, (long long)m,
                                   md ? md + u0 : nullptr);
            }
        }
        WL_HIP(ctx, hipGetLastError());
        ctx->last_kernel = lds ? "k_thbig_lds" : "k_thbig_stream";
        return WL_OK;
    }
    int64_t chunk = (int64_t)opt("WL_THB_CHUNK", 16384);
    if (chunk < 64) chunk = 64;
    if (chunk > ((int64_t)1 << 30)) chunk = (int64_t)1 << 30;
    while ((n + chunk - 1) / chunk > 0x7fffffff) chunk *= 2;  // (gridDim.x)
    const int64_t nch = (n + chunk - 1) / chunk;
    auto bytes = [&](int64_t G) { return up256((size_t)G * sizeof(ThbUnit)) + up256((size_t)G * nch * sizeof(unsigned int)); };
    int64_t G = 1;
    WL_TRY(group_reserve(ctx, st, nunits, 65535, bytes, G));
    ThbUnit *s = (ThbUnit *)ctx->ws;
    unsigned int *ties = (unsigned int *)((char *)ctx->ws + up256((size_t)G * sizeof(ThbUnit)));
    WL_TRY(for_groups(nunits, G, [&](int64_t u0, int64_t nb) -> int {
        T *xg = x + u0 * stride;
        const dim3 grid((unsigned)nch, (unsigned)nb);
        hipLaunchKernelGGL(k_thb_init, dim3((unsigned)nb), dim3(256), 0, st, s, (long long)n, (long long)m, md ? md + u0 : nullptr);
        for (int pass = 0; pass < KeyOf<T>::BYTES; ++pass) {
            hipLaunchKernelGGL((k_thb_hist<T>), grid, dim3(EXT_THREADS), 0, st, xg, n, stride, chunk, pass, s);
            hipLaunchKernelGGL((k_thb_scan<T>), dim3((unsigned)nb), dim3(64), 0, st, pass, s);
        }
        hipLaunchKernelGGL((k_thb_count<T>), grid, dim3(EXT_THREADS), 0, st, xg, n, stride, chunk, s, ties);
        hipLaunchKernelGGL((k_thb_clear<T>), grid, dim3(EXT_THREADS), 0, st, xg, n, stride, chunk, s, ties);
        WL_HIP(ctx, hipGetLastError());
        return WL_OK;
    }));
    ctx->last_kernel = "k_thbig_split";
    return WL_OK;
}

// the rules the two entry points share behind their pointer and dtype rules
inline int thb_dims(int64_t n, int64_t nunits, int64_t unit_stride)
{
    int64_t tot = 0;
    if (n < 1 || nunits < 1 || unit_stride < n) return WL_EDIMS;
    if (__builtin_mul_overflow(nunits, unit_stride, &tot) || tot >= ((int64_t)1 << 60)) return WL_EDIMS;
    return WL_OK;
}

}  // namespace

extern "C" {

int wl_threshold_batch(wl_ctx *ctx, int dtype, void *x, int64_t n, int64_t nunits, int64_t unit_stride, int th, double t,
                       const double *t_dev, int t_is_f64, void *stream)
{
    if (!ctx || !x) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(thb_dims(n, nunits, unit_stride));
    if (th < WL_TH_HARD || th > WL_TH_NEG) return WL_EINVAL_ARG;
    if (!t_dev && th <= WL_TH_STEIN && !(t >= 0)) return WL_EINVAL_ARG;      // @assert t >= 0 (a host threshold only)
    return scoped_by_dtype(ctx, dtype, stream, [&](auto e, hipStream_t st) {
        using T = decltype(e);
        return threshold_batch_impl<T>(ctx, st, (T *)x, n, nunits, unit_stride, th, t, t_dev, t_is_f64);
    });
}

int wl_threshold_biggest_batch(wl_ctx *ctx, int dtype, void *x, int64_t n, int64_t nunits, int64_t unit_stride, int64_t m,
                               const int64_t *m_dev, void *stream)
{
    if (!ctx || !x) return WL_EINVAL_ARG;
    WL_TRY(check_dtype(dtype));
    WL_TRY(thb_dims(n, nunits, unit_stride));
    if (!m_dev && m < 0) return WL_EINVAL_ARG;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto e, hipStream_t st) {
        using T = decltype(e);
        return biggest_batch_impl<T>(ctx, st, (T *)x, n, nunits, unit_stride, m, m_dev);
    });
}

}  // extern "C"

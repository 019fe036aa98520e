// wl_select.h -- the device primitives that the order-statistic kernels of wl_ext.hip (median!, mad!, threshold_biggest and the
// per-unit noise estimates) and of wl_thbatch.hip (threshold! of a batch) share: the element-wise in-place pass, the monotone
// integer keys, the radix select over keys in LDS and the one-wave bin pick of a 256-bin histogram.  wl_modwt.hip takes the launch
// geometry of the element-wise kernels (EXT_THREADS, ext_blocks, vec_ok16) from here.
// Everything here has internal linkage: each translation unit instantiates its own copies, and a kernel that must not share an
// instantiation with another one (its inlining, its register allocation) asks for its own through INST.
#pragma once
#include "wl_internal.h"

#include <cstdint>

namespace {

constexpr int EXT_THREADS = 256;
inline unsigned ext_blocks(int64_t n, int per_thread, int cu_count)
{
    int64_t b = (n + (int64_t)EXT_THREADS * per_thread - 1) / ((int64_t)EXT_THREADS * per_thread);
    const int64_t cap = (int64_t)cu_count * 16;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}


// element-wise in-place pass: 16-byte vectors when the pointer is aligned, scalar tail
template <typename T, typename F>
__device__ __forceinline__ void ew_inplace(T *__restrict__ x, int64_t n, int vec_ok, F f)
{
    constexpr int V = 16 / sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    constexpr int U = 4;                      // independent 16-byte accesses in flight per lane
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nv = vec_ok ? n / V : 0;
    VT *xv = reinterpret_cast<VT *>(x);
    const int64_t tile = (int64_t)U * blockDim.x, ntiles = nv / tile;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int64_t base = tl * tile + threadIdx.x;
        VT v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = xv[base + (int64_t)u * blockDim.x];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int e = 0; e < V; ++e) v[u][e] = f(v[u][e], (base + (int64_t)u * blockDim.x) * V + e);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) xv[base + (int64_t)u * blockDim.x] = v[u];
    }
    for (int64_t i = ntiles * tile + gid; i < nv; i += nthr) {
        VT v = xv[i];
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = f(v[e], i * V + e);
        xv[i] = v;
    }
    for (int64_t i = nv * V + gid; i < n; i += nthr) x[i] = f(x[i], i);
}
inline int vec_ok16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 ? 1 : 0; }

// ---- order statistics: MSB-first radix select on monotone integer keys -------------------------------
template <typename T> struct KeyOf;
template <> struct KeyOf<float> {
    typedef unsigned int U;
    static constexpr int BYTES = 4;
    __device__ static U key(float v, int absmode)
    {
        U b = __float_as_uint(v);
        if (absmode) return b & 0x7fffffffu;
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    __device__ static float val(U k, int absmode)
    {
        if (absmode) return __uint_as_float(k);
        return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
    }
};
template <> struct KeyOf<double> {
    typedef unsigned long long U;
    static constexpr int BYTES = 8;
    __device__ static U key(double v, int absmode)
    {
        U b = (U)__double_as_longlong(v);
        if (absmode) return b & 0x7fffffffffffffffull;
        return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
    }
    __device__ static double val(U k, int absmode)
    {
        if (absmode) return __longlong_as_double((long long)k);
        return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k));
    }
};

// rank k (0-based) among n keys in LDS: one workgroup, one 256-bin histogram per radix byte
// (INST: a caller that must not share the instantiation of k_mad_lds -- and with it that kernel's inlining and register allocation --
// asks for its own)
template <typename T, int INST = 0>
__device__ typename KeyOf<T>::U lds_select(const typename KeyOf<T>::U *keys, int n, unsigned long long k, unsigned int *hist,
                                             unsigned long long *sh)
{
    typedef typename KeyOf<T>::U U;
    constexpr int NB = KeyOf<T>::BYTES;
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (tid == 0) { sh[0] = 0; sh[1] = k; }
    for (int pass = 0; pass < NB; ++pass) {
        const int shift = 8 * (NB - 1 - pass);
        for (int b = tid; b < 256; b += nthr) hist[b] = 0;
        __syncthreads();
        const U prefix = (U)sh[0];
        for (int i = tid; i < n; i += nthr) {
            const U key = keys[i];
            if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)((key >> shift) & 0xff)], 1u);
        }
        __syncthreads();
        // the bin that holds rank kk: first b with kk < hist[0] + ... + hist[b] (255 when none).  One wave scans the 256 bins, four
        // per lane (thread 0 walking them one dependent LDS read at a time cost ~8 us per pass: 16 passes per mad!)
        if (tid < 64) {
            const unsigned int h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            const unsigned int mine = h0 + h1 + h2 + h3;
            unsigned int incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned int o = __shfl_up(incl, d, 64);
                if (tid >= d) incl += o;
            }
            const unsigned long long kk = sh[1];
            const unsigned long long excl = incl - mine;
            const bool hit = kk < (unsigned long long)incl;
            const unsigned long long m = __ballot(hit);
            const int first = m ? (__ffsll((long long)m) - 1) : 64;
            if (tid == first) {
                int b = 4 * tid;
                unsigned long long cum = excl;
                if (kk >= cum + h0) { cum += h0; ++b; if (kk >= cum + h1) { cum += h1; ++b; if (kk >= cum + h2) { cum += h2; ++b; } } }
                sh[1] = kk - cum;
                sh[0] = sh[0] | (((unsigned long long)b) << shift);
            } else if (first == 64 && tid == 63) {       // (cannot happen for kk < n; mirrors the serial walk: bin 255, all lower bins skipped)
                sh[1] = kk - (excl + h0 + h1 + h2);
                sh[0] = sh[0] | (255ull << shift);
            }
        }
        __syncthreads();
    }
    const U r = (U)sh[0];
    __syncthreads();                // the next call re-initialises sh
    return r;
}

// keys of n elements in dynamic LDS next to ~1 KiB of static LDS: stay under the 64 KiB a kernel gets without
// hipFuncSetAttribute (Float64 keys are 8 bytes)
template <typename T>
constexpr int64_t mad_lds_max() { return sizeof(T) == 4 ? 8192 : 4096; }

// the bin that holds rank kk among the 256 counts h[] -- first b with kk < h[0] + ... + h[b], 255 when none -- and the rank left
// inside it: one wave, four bins per lane (the scan of lds_select)
__device__ __forceinline__ void wave_pick_bin(const unsigned int *h, int lane, int shift, unsigned long long *prefix, unsigned long long *rank)
{
    const unsigned int h0 = h[4 * lane], h1 = h[4 * lane + 1], h2 = h[4 * lane + 2], h3 = h[4 * lane + 3];
    const unsigned int mine = h0 + h1 + h2 + h3;
    unsigned int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    const unsigned long long kk = *rank;
    const unsigned long long excl = incl - mine;
    const unsigned long long m = __ballot(kk < (unsigned long long)incl);
    const int first = m ? (__ffsll((long long)m) - 1) : 64;
    if (lane == first) {
        int b = 4 * lane;
        unsigned long long cum = excl;
        if (kk >= cum + h0) { cum += h0; ++b; if (kk >= cum + h1) { cum += h1; ++b; if (kk >= cum + h2) { cum += h2; ++b; } } }
        *rank = kk - cum;
        *prefix = *prefix | (((unsigned long long)b) << shift);
    } else if (first == 64 && lane == 63) {          // (cannot happen for kk < n; mirrors the serial walk of k_sel_scan)
        *rank = kk - (excl + h0 + h1 + h2);
        *prefix = *prefix | (255ull << shift);
    }
}

}  // namespace

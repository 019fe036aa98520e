// wl_complex.hip -- staging kernels of the complex-valued transforms (wl_*_complex, wl_api.hip): interleaved Complex{T} units
// <-> planar real planes.  The taps are real, so a complex transform is the real transform of the real parts and of the imaginary
// parts: a unit of n complex values becomes two planes of n reals (k_cplx_split), the existing batched level loops run on the
// planes as a batch of 2 * nunits real units, and the planes go back interleaved (k_cplx_merge).  Both kernels only move bits
// (a -0.0 or a NaN payload arrives as it left) and are bandwidth-bound: 2 n T read and 2 n T written per unit.
//
// Layout:  planes[(2u + c) * plane_stride + i] = component c (0 = re, 1 = im) of z[u * unit_stride + i],  i < n, u < nunits;
// unit_stride counts complex elements, plane_stride real elements.
//
// Vector path (16-byte unit and plane bases): the data is cut into 16-byte PIECES -- on the interleaved side piece p holds
// complex values [p E/2, (p + 1) E/2), on a plane piece k holds reals [k E, (k + 1) E), E = 16 / sizeof(T) (4 Float32, 2 Float64).
// Plane piece k of re and of im is made of the interleaved pieces 2k and 2k + 1.  A wave takes 64 plane pieces = 128 interleaved
// pieces per step; every global instruction moves 16 bytes per lane with lane l on piece base + l:
//     interleaved side   instruction A: piece 2 kb + l          instruction B: piece 2 kb + 64 + l
//     planes             re: piece kb + l                       im: piece kb + l
// and the pieces change lanes in between through ds_bpermute (__shfl; the crossbar of the LDS, no LDS allocation): 16 dword
// shuffles per lane and step, about a tenth of the time the step's 4 KiB take at the HBM rate of a CU.
// Element path: one complex value per lane -- the n mod E tail of the vector path, and whole units when a base is not 16-byte
// aligned (a ComplexF32 view that starts at an odd element, an odd unit_stride in Float32, planes of a caller's own stride).
// Nothing outside [u * unit_stride, u * unit_stride + n) of a unit or [.., + n) of a plane is written.
#include "wl_internal.h"

namespace wl {
namespace {

constexpr int CPLX_THREADS = 256;
// a 16-byte piece as the compiler's own vector type: one global_load / global_store_dwordx4 per access
typedef unsigned int piece_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ piece_t mk(unsigned x, unsigned y, unsigned z, unsigned w)
{
    piece_t p = {x, y, z, w};
    return p;
}

// the two interleaved pieces of a plane piece <-> its re piece and its im piece
template <typename T>
__device__ __forceinline__ void deinterleave(const piece_t &p0, const piece_t &p1, piece_t &re, piece_t &im);
template <>
__device__ __forceinline__ void deinterleave<float>(const piece_t &p0, const piece_t &p1, piece_t &re, piece_t &im)
{
    re = mk(p0.x, p0.z, p1.x, p1.z);            // (r0 i0 r1 i1) (r2 i2 r3 i3) -> (r0 r1 r2 r3), (i0 i1 i2 i3)
    im = mk(p0.y, p0.w, p1.y, p1.w);
}
template <>
__device__ __forceinline__ void deinterleave<double>(const piece_t &p0, const piece_t &p1, piece_t &re, piece_t &im)
{
    re = mk(p0.x, p0.y, p1.x, p1.y);            // (r0 i0) (r1 i1) -> (r0 r1), (i0 i1); a double is two dwords
    im = mk(p0.z, p0.w, p1.z, p1.w);
}
template <typename T>
__device__ __forceinline__ void interleave(const piece_t &re, const piece_t &im, piece_t &p0, piece_t &p1);
template <>
__device__ __forceinline__ void interleave<float>(const piece_t &re, const piece_t &im, piece_t &p0, piece_t &p1)
{
    p0 = mk(re.x, im.x, re.y, im.y);
    p1 = mk(re.z, im.z, re.w, im.w);
}
template <>
__device__ __forceinline__ void interleave<double>(const piece_t &re, const piece_t &im, piece_t &p0, piece_t &p1)
{
    p0 = mk(re.x, re.y, im.x, im.y);
    p1 = mk(re.z, re.w, im.z, im.w);
}

__device__ __forceinline__ piece_t shfl4(const piece_t &v, int src)
{
    return mk((unsigned)__shfl((int)v.x, src), (unsigned)__shfl((int)v.y, src), (unsigned)__shfl((int)v.z, src),
                      (unsigned)__shfl((int)v.w, src));
}
__device__ __forceinline__ piece_t pick(bool first, const piece_t &a, const piece_t &b) { return first ? a : b; }

// grid: x = workgroups striding over one unit, y = units of this launch.  vec: every unit and plane base is 16-byte aligned.
template <typename T>
__global__ void __launch_bounds__(CPLX_THREADS) k_cplx_split(T *__restrict__ planes, int64_t plane_stride, const T *__restrict__ z, int64_t n,
                                                            int64_t unit_stride, int vec)
{
    constexpr int E = 16 / (int)sizeof(T);
    const int64_t u = blockIdx.y;
    const T *zu = z + 2 * u * unit_stride;
    T *re = planes + 2 * u * plane_stride, *im = re + plane_stride;
    const int lane = threadIdx.x & 63;
    const int64_t q = vec ? n / E : 0;                   // plane pieces of the vector path; 2 q interleaved pieces
    const int64_t wave = (int64_t)blockIdx.x * (CPLX_THREADS / 64) + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * (CPLX_THREADS / 64);
    const piece_t *z4 = reinterpret_cast<const piece_t *>(zu);
    const piece_t zero = mk(0u, 0u, 0u, 0u);
    for (int64_t kb = wave * 64; kb < q; kb += nwaves * 64) {          // (wave-uniform bounds: every lane reaches the shuffles)
        const int64_t ia = 2 * kb + lane, ib = ia + 64;
        const piece_t a = ia < 2 * q ? z4[ia] : zero;
        const piece_t b = ib < 2 * q ? z4[ib] : zero;
        // lane k owns plane piece kb + k: interleaved pieces 2 kb + 2k and + 1, which instruction A (k < 32) or B loaded into
        // lanes (2k) mod 64 and (2k) mod 64 + 1
        const int s0 = (2 * lane) & 63;
        const bool low = lane < 32;
        const piece_t p0 = pick(low, shfl4(a, s0), shfl4(b, s0));
        const piece_t p1 = pick(low, shfl4(a, s0 + 1), shfl4(b, s0 + 1));
        piece_t r, i;
        deinterleave<T>(p0, p1, r, i);
        if (kb + lane < q) {
            reinterpret_cast<piece_t *>(re)[kb + lane] = r;
            reinterpret_cast<piece_t *>(im)[kb + lane] = i;
        }
    }
    const int64_t tid = (int64_t)blockIdx.x * CPLX_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * CPLX_THREADS;
    for (int64_t i = q * E + tid; i < n; i += nthreads) {
        re[i] = zu[2 * i];
        im[i] = zu[2 * i + 1];
    }
}

template <typename T>
__global__ void __launch_bounds__(CPLX_THREADS) k_cplx_merge(T *__restrict__ z, const T *__restrict__ planes, int64_t plane_stride, int64_t n,
                                                            int64_t unit_stride, int vec)
{
    constexpr int E = 16 / (int)sizeof(T);
    const int64_t u = blockIdx.y;
    T *zu = z + 2 * u * unit_stride;
    const T *re = planes + 2 * u * plane_stride, *im = re + plane_stride;
    const int lane = threadIdx.x & 63;
    const int64_t q = vec ? n / E : 0;
    const int64_t wave = (int64_t)blockIdx.x * (CPLX_THREADS / 64) + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * (CPLX_THREADS / 64);
    piece_t *z4 = reinterpret_cast<piece_t *>(zu);
    const piece_t zero = mk(0u, 0u, 0u, 0u);
    for (int64_t kb = wave * 64; kb < q; kb += nwaves * 64) {
        const bool have = kb + lane < q;
        const piece_t r = have ? reinterpret_cast<const piece_t *>(re)[kb + lane] : zero;
        const piece_t i = have ? reinterpret_cast<const piece_t *>(im)[kb + lane] : zero;
        piece_t p0, p1;
        interleave<T>(r, i, p0, p1);                      // interleaved pieces 2 (kb + lane) and + 1
        // instruction A stores piece 2 kb + l from lane l / 2, instruction B piece 2 kb + 64 + l from lane 32 + l / 2; an odd l
        // takes the second piece of its source lane
        const int sa = lane >> 1, sb = 32 + (lane >> 1);
        const bool even = (lane & 1) == 0;
        const piece_t a = pick(even, shfl4(p0, sa), shfl4(p1, sa));
        const piece_t b = pick(even, shfl4(p0, sb), shfl4(p1, sb));
        const int64_t ia = 2 * kb + lane, ib = ia + 64;
        if (ia < 2 * q) z4[ia] = a;
        if (ib < 2 * q) z4[ib] = b;
    }
    const int64_t tid = (int64_t)blockIdx.x * CPLX_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * CPLX_THREADS;
    for (int64_t i = q * E + tid; i < n; i += nthreads) {
        zu[2 * i] = re[i];
        zu[2 * i + 1] = im[i];
    }
}

// workgroups per unit: one per 256 lanes of work, no more than keeps about 16 workgroups per CU in flight over all units
inline unsigned cplx_blocks(int64_t n, int64_t per_lane, int64_t nu, int cu_count)
{
    int64_t want = (n / per_lane + CPLX_THREADS - 1) / CPLX_THREADS + 1;
    int64_t lim = ((int64_t)cu_count * 16 + nu - 1) / nu;
    if (lim < 1) lim = 1;
    if (want > lim) want = lim;
    return (unsigned)(want < 1 ? 1 : want);
}

}  // namespace

template <typename T>
hipError_t complex_split(hipStream_t st, int cu_count, T *planes, int64_t plane_stride, const T *z, int64_t n, int64_t nunits, int64_t unit_stride)
{
    constexpr int E = 16 / (int)sizeof(T);
    // every unit base: z + 2 u unit_stride reals; every plane base: planes + k plane_stride
    const bool vec = al16(z) && al16(planes) && (plane_stride % E) == 0 && (nunits == 1 || (2 * unit_stride) % E == 0);
    for (int64_t u0 = 0; u0 < nunits; u0 += 65535) {
        const int64_t nu = (nunits - u0 < 65535) ? (nunits - u0) : 65535;
        hipLaunchKernelGGL((k_cplx_split<T>), dim3(cplx_blocks(n, vec ? E : 1, nu, cu_count), (unsigned)nu), dim3(CPLX_THREADS), 0, st,
                           planes + 2 * u0 * plane_stride, plane_stride, z + 2 * u0 * unit_stride, n, unit_stride, vec ? 1 : 0);
    }
    return hipGetLastError();
}

template <typename T>
hipError_t complex_merge(hipStream_t st, int cu_count, T *z, const T *planes, int64_t plane_stride, int64_t n, int64_t nunits, int64_t unit_stride)
{
    constexpr int E = 16 / (int)sizeof(T);
    const bool vec = al16(z) && al16(planes) && (plane_stride % E) == 0 && (nunits == 1 || (2 * unit_stride) % E == 0);
    for (int64_t u0 = 0; u0 < nunits; u0 += 65535) {
        const int64_t nu = (nunits - u0 < 65535) ? (nunits - u0) : 65535;
        hipLaunchKernelGGL((k_cplx_merge<T>), dim3(cplx_blocks(n, vec ? E : 1, nu, cu_count), (unsigned)nu), dim3(CPLX_THREADS), 0, st,
                           z + 2 * u0 * unit_stride, planes + 2 * u0 * plane_stride, plane_stride, n, unit_stride, vec ? 1 : 0);
    }
    return hipGetLastError();
}

template hipError_t complex_split<float>(hipStream_t, int, float *, int64_t, const float *, int64_t, int64_t, int64_t);
template hipError_t complex_split<double>(hipStream_t, int, double *, int64_t, const double *, int64_t, int64_t, int64_t);
template hipError_t complex_merge<float>(hipStream_t, int, float *, const float *, int64_t, int64_t, int64_t, int64_t);
template hipError_t complex_merge<double>(hipStream_t, int, double *, const double *, int64_t, int64_t, int64_t, int64_t);

}  // namespace wl

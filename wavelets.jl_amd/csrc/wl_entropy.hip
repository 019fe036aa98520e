// wl_entropy.hip -- the best-basis search of wavelet packet trees: coefentropy with ShannonEntropy / LogEnergyEntropy and the
// decision of bestbasistree (src/Threshold/entropy.jl:15-133).  The packet content of every depth comes from the packet kernels
// (wpt_impl, wl_api.hip), bit for bit; this file reduces it to node entropies and turns those into the tree.
//
// Accuracy contract -- the one documented exception to "bit-identical to the reference" (DESIGN.md section 11).  The reference's
// log is Julia's own, its norm is BLAS nrm2 and its sums are sequential in T: no parallel reduction reproduces those bits.  Here
//   nrm    = T(sqrt(Float64 sum of x^2))                          (~1 ulp of T from the reference's)
//   s      = (x / nrm)^2 in T, IEEE division, separate roundings  (exactly as the reference)
//   term   = -s*log(s) (Shannon) / -log(s) (log energy), s and the log in Float64; s == 0 gives -0.0
//   sums   in Float64 in a fixed order (lane-strided partials, a fixed butterfly, pieces folded in index order): deterministic
//   nrm == 0 gives exactly 0 for every node (the reference's early return)
// giving |entropy - exact entropy of the same T coefficients| <= 1e-12 * sum|term| (Float64) / 4e-7 * sum|term| (Float32); the
// reference itself is off by ~n eps(T).  The decision runs in Float64 on these
// values with Julia's `min` (NaN propagates) and the reference's `entr_bf[i] <= best(i)` test.
//
// Batches (wl_bestbasistree_filter_batch): every kernel takes blockIdx.y as the unit and per-unit bases of its
// operands (EntUnits / BBUnits: element strides from one unit to the next).  What a segment's sum is made of -- the lane group,
// the piece size, the fold order -- depends on its length only, so a unit's values do not depend on the batch around it; the single
// search is the batch of one unit of the same instances.
#include "wl_ctx.h"

#include <cmath>

namespace wl {

namespace {

constexpr int ENT_THREADS = 256;
constexpr int64_t ENT_CHUNK = 4096;      // samples per piece of a long segment (16 per lane)
constexpr int BB_LEVELS = 9;             // depths of the decision per workgroup: 256 bottom nodes in LDS

// ET: 0 Shannon, 1 log energy, 2 square (the norm)
template <typename T, int ET>
__device__ __forceinline__ double ent_term(T v, T nrm)
{
    if (ET == 2) return (double)v * (double)v;
    const T q = v / nrm;
    const T s = q * q;
    if (s == T(0)) return -0.0;
    const double sd = (double)s;
    return ET == 0 ? -sd * log(sd) : -log(sd);
}

// strides from unit u to unit u + 1 (blockIdx.y): samples, norms (one double per unit), partials / outputs
struct EntUnits { int64_t x, nrm, out; };

// One group of G lanes (G divides 64, or G == 256) per piece; piece p of segment s is [p * chunk, min(nj, (p + 1) * chunk)) of
// x[s * nj ...].  Lanes sum a fixed lane-strided subset, the group folds them with a fixed butterfly: the same input always gives
// the same bits.  out[s * npieces + p] = the piece's sum.  nrmp == nullptr: the norm is nrm_val.
template <typename T, int ET, int G>
__global__ __launch_bounds__(ENT_THREADS) void k_entropy_seg(const T *__restrict__ x, int64_t nj, int64_t npieces, int64_t ngroups,
                                                             int64_t chunk, const double *__restrict__ nrmp, double nrm_val,
                                                             double *__restrict__ out, EntUnits us)
{
    const int64_t unit = blockIdx.y;
    x += unit * us.x;
    out += unit * us.out;
    if (nrmp) nrmp += unit * us.nrm;
    const int64_t grp = ((int64_t)blockIdx.x * ENT_THREADS + threadIdx.x) / G;
    const int lane = (int)(threadIdx.x % G);
    const T nrm = (T)(nrmp ? *nrmp : nrm_val);
    double acc = 0.0;
    if (grp < ngroups && (ET == 2 || nrm != T(0))) {
        const int64_t s = grp / npieces, p = grp - s * npieces;
        const int64_t lo = p * chunk, hi = (lo + chunk < nj) ? lo + chunk : nj;
        const T *seg = x + s * nj;
        for (int64_t i = lo + lane; i < hi; i += G) acc += ent_term<T, ET>(seg[i], nrm);
    }
    if (G == 256) {
        __shared__ double sh[ENT_THREADS];
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int o = ENT_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        acc = sh[0];
    } else {
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    }
    if (grp < ngroups && lane == 0) out[grp] = acc;
}

// out[s] = sum of the npieces partials of segment s, one wave per segment (lane-strided, then a fixed butterfly)
__global__ __launch_bounds__(ENT_THREADS) void k_entropy_fold(const double *__restrict__ part, int64_t npieces, int64_t nseg,
                                                              double *__restrict__ out, int64_t upart, int64_t uout)
{
    part += (int64_t)blockIdx.y * upart;
    out += (int64_t)blockIdx.y * uout;
    const int64_t s = ((int64_t)blockIdx.x * ENT_THREADS + threadIdx.x) / 64;
    const int lane = (int)(threadIdx.x % 64);
    double acc = 0.0;
    if (s < nseg)
        for (int64_t p = lane; p < npieces; p += 64) acc += part[s * npieces + p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (s < nseg && lane == 0) out[s] = acc;
}

// nrm[u] = T(sqrt(sum of squares of unit u)), kept as a double; unit u's sum is sumsq[u * usum]
template <typename T>
__global__ void k_entropy_nrm(const double *__restrict__ sumsq, double *__restrict__ nrm, int64_t usum, int64_t nunits)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nunits) nrm[u] = (double)(T)sqrt(sumsq[u * usum]);
}

// Julia's min(x, y) for floats: NaN propagates, -0.0 < +0.0
__device__ __forceinline__ double jl_min(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    return (b < a || (signbit(b) && !signbit(a))) ? b : a;
}

// Bottom-up decision over the depths dbot, dbot - 1, ..., dbot - nlev + 1 (0-based node k at depth d: k = 2^d - 1 + j).  A
// workgroup owns 2^(nlev - 1) consecutive nodes of depth dbot and the subtree above them, level by level in LDS.
//   cs(k)    = the children's best sum (depth Lmax - 1: entr_af of the node), left + right
//   split[k] = !(entr_bf[k] <= cs(k))        (== !(entr_bf[k] <= min(entr_bf[k], cs(k))), the reference's test)
//   best[k]  = min(entr_bf[k], cs(k))        stored for the band's top row only (the next band's children)
// blockIdx.y is the unit: uent / ubest / usplit elements from one unit's vector to the next.
__global__ __launch_bounds__(ENT_THREADS) void k_bb_up(const double *__restrict__ ent, int64_t ntree, int Lmax, int dbot, int nlev,
                                                       double *__restrict__ best, uint8_t *__restrict__ split, int64_t uent, int64_t ubest,
                                                       int64_t usplit)
{
    __shared__ double sh[ENT_THREADS];
    ent += (int64_t)blockIdx.y * uent;
    best += (int64_t)blockIdx.y * ubest;
    split += (int64_t)blockIdx.y * usplit;
    const int W = 1 << (nlev - 1);
    const int t = (int)threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * W;
    for (int lev = 0; lev < nlev; ++lev) {
        const int w = W >> lev;
        const int d = dbot - lev;
        double b = 0.0;
        if (t < w) {
            const int64_t k = ((int64_t)1 << d) - 1 + (j0 >> lev) + t;
            double cs;
            if (lev > 0) cs = sh[2 * t] + sh[2 * t + 1];
            else if (d == Lmax - 1) cs = ent[ntree + (k - (((int64_t)1 << d) - 1))];
            else cs = best[2 * k + 1] + best[2 * k + 2];
            const double bf = ent[k];
            split[k] = !(bf <= cs);
            b = jl_min(bf, cs);
            if (lev == nlev - 1) best[k] = b;
        }
        __syncthreads();
        if (t < w) sh[t] = b;
        __syncthreads();
    }
}

// Top-down: node k stays split iff the input tree has it and it and every ancestor split (a valid tree has every ancestor of a set
// node set, so tree[k] covers the input tree's ancestors).  tree == nullptr: the input tree is the full tree of depth Lfull, node k
// is in it iff k < 2^Lfull - 1.  blockIdx.y is the unit (utree == 0: one input tree for all).  With split == tree this is the
// closure of a tree nobody validated: a node counts iff it and every ancestor is set (tree_close).
__global__ __launch_bounds__(ENT_THREADS) void k_bb_down(const uint8_t *tree, int Lfull, const uint8_t *split, int64_t ntree, uint8_t *__restrict__ out,
                                                         int64_t utree, int64_t usplit, int64_t uout)
{
    const int64_t k = (int64_t)blockIdx.x * ENT_THREADS + threadIdx.x;
    if (k >= ntree) return;
    split += (int64_t)blockIdx.y * usplit;
    out += (int64_t)blockIdx.y * uout;
    const bool in_tree = tree ? tree[(int64_t)blockIdx.y * utree + k] != 0 : k < (((int64_t)1 << Lfull) - 1);
    bool v = in_tree && split[k] != 0;
    for (int64_t j = k; v && j > 0;) {
        j = (j - 1) >> 1;
        v = split[j] != 0;
    }
    out[k] = v ? 1 : 0;
}

inline unsigned nblocks(int64_t threads) { return (unsigned)((threads + ENT_THREADS - 1) / ENT_THREADS); }

// bu: the units of the launch (grid y) and the strides of x, the norms, the partials and the outputs between them
template <typename T, int ET>
hipError_t seg_launch(hipStream_t st, const T *x, int64_t nj, int64_t nseg, const double *nrmp, double nrm_val, double *part, double *out,
                      const EntBatch &bu)
{
    const unsigned nu = (unsigned)bu.nunits;
    if (nj > 2048) {
        const int64_t npieces = (nj + ENT_CHUNK - 1) / ENT_CHUNK, ng = nseg * npieces;
        double *dst = npieces == 1 ? out : part;
        const EntUnits us = {bu.x, 1, npieces == 1 ? bu.out : bu.part};
        hipLaunchKernelGGL((k_entropy_seg<T, ET, 256>), dim3(nblocks(ng * 256), nu), dim3(ENT_THREADS), 0, st, x, nj, npieces, ng, ENT_CHUNK,
                           nrmp, nrm_val, dst, us);
        if (npieces > 1)
            hipLaunchKernelGGL(k_entropy_fold, dim3(nblocks(nseg * 64), nu), dim3(ENT_THREADS), 0, st, (const double *)part, npieces, nseg, out,
                               bu.part, bu.out);
        return hipGetLastError();
    }
    // one group per segment, about 8 samples per lane
    const int64_t want = (nj + 7) / 8;
    const EntUnits us = {bu.x, 1, bu.out};
#define WL_ENT_SEG(G_)                                                                                                       \
    hipLaunchKernelGGL((k_entropy_seg<T, ET, G_>), dim3(nblocks(nseg * (G_)), nu), dim3(ENT_THREADS), 0, st, x, nj, (int64_t)1, nseg, \
                       nj, nrmp, nrm_val, out, us)
    if (want > 64) WL_ENT_SEG(256);
    else if (want > 32) WL_ENT_SEG(64);
    else if (want > 16) WL_ENT_SEG(32);
    else if (want > 8) WL_ENT_SEG(16);
    else if (want > 4) WL_ENT_SEG(8);
    else if (want > 2) WL_ENT_SEG(4);
    else if (want > 1) WL_ENT_SEG(2);
    else WL_ENT_SEG(1);
#undef WL_ENT_SEG
    return hipGetLastError();
}

}  // namespace

size_t entropy_partials(int64_t n) { return (size_t)(n / 1024 + 64); }

template <typename T>
hipError_t entropy_segments(hipStream_t st, int et, const T *x, int64_t nj, int64_t nseg, const double *nrmp, double nrm_val, double *part,
                            double *out, const EntBatch &bu)
{
    return et == WL_ENTROPY_SHANNON ? seg_launch<T, 0>(st, x, nj, nseg, nrmp, nrm_val, part, out, bu)
                                    : seg_launch<T, 1>(st, x, nj, nseg, nrmp, nrm_val, part, out, bu);
}

template <typename T>
hipError_t entropy_norm(hipStream_t st, const T *x, int64_t n, double *part, double *nrm_out, const EntBatch &bu)
{
    // the sum of squares of a unit lands in the last of its entropy_partials(n) partials, past every partial a one-segment reduction
    // writes (bu.out is not used: the sums stay with the partials)
    double *sumsq = part + entropy_partials(n) - 1;
    EntBatch b = bu;
    b.out = bu.part;
    hipError_t e = seg_launch<T, 2>(st, x, n, 1, nullptr, 0.0, part, sumsq, b);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_entropy_nrm<T>), dim3(nblocks(bu.nunits)), dim3(ENT_THREADS), 0, st, (const double *)sumsq, nrm_out, bu.part, bu.nunits);
    return hipGetLastError();
}

hipError_t bestbasis_decide(hipStream_t st, const double *ent, int64_t ntree, int Lmax, double *best, uint8_t *split, const uint8_t *tree,
                            int Lfull, uint8_t *tree_out, int64_t nunits, int64_t uent, int64_t uout)
{
    const unsigned nu = (unsigned)nunits;
    for (int d = Lmax - 1; d >= 0;) {
        const int nlev = d + 1 < BB_LEVELS ? d + 1 : BB_LEVELS;
        const int64_t nwg = (int64_t)1 << (d - nlev + 1);
        const int W = 1 << (nlev - 1);
        hipLaunchKernelGGL(k_bb_up, dim3((unsigned)nwg, nu), dim3(W < 64 ? 64 : W), 0, st, ent, ntree, Lmax, d, nlev, best, split, uent, ntree, ntree);
        d -= nlev;
    }
    hipLaunchKernelGGL(k_bb_down, dim3(nblocks(ntree), nu), dim3(ENT_THREADS), 0, st, tree, Lfull, (const uint8_t *)split, ntree, tree_out,
                       (int64_t)0, ntree, uout);
    return hipGetLastError();
}

hipError_t tree_close(hipStream_t st, const uint8_t *trees, int64_t utrees, int64_t nnodes, uint8_t *out, int64_t uout, int64_t nunits)
{
    hipLaunchKernelGGL(k_bb_down, dim3(nblocks(nnodes), (unsigned)nunits), dim3(ENT_THREADS), 0, st, trees, 0, trees, nnodes, out, utrees, utrees,
                       uout);
    return hipGetLastError();
}

template hipError_t entropy_segments<float>(hipStream_t, int, const float *, int64_t, int64_t, const double *, double, double *, double *,
                                            const EntBatch &);
template hipError_t entropy_segments<double>(hipStream_t, int, const double *, int64_t, int64_t, const double *, double, double *, double *,
                                             const EntBatch &);
template hipError_t entropy_norm<float>(hipStream_t, const float *, int64_t, double *, double *, const EntBatch &);
template hipError_t entropy_norm<double>(hipStream_t, const double *, int64_t, double *, double *, const EntBatch &);

}  // namespace wl

using namespace wl;

namespace {

// coefentropy(x, et, nrm): result = T(sum), returned as a double after one stream synchronisation
template <typename T>
int coefentropy_impl(wl_ctx *ctx, hipStream_t st, const T *x, int64_t n, int et, int have_nrm, double nrm, double *result)
{
    const size_t np = entropy_partials(n);
    int rc = wl_ensure_ws(ctx, (np + 8) * sizeof(double), st, true);
    if (rc) return rc;
    double *part = (double *)ctx->ws;
    double *nrmd = part + np, *res = nrmd + 1;
    const EntBatch one = {1, 0, 0, 0};
    if (!have_nrm) WL_HIP(ctx, entropy_norm<T>(st, x, n, part, nrmd, one));
    WL_HIP(ctx, entropy_segments<T>(st, et, x, n, 1, have_nrm ? nullptr : nrmd, (double)(T)nrm, part, res, one));
    double h = 0.0;
    WL_HIP(ctx, hipMemcpyAsync(&h, res, sizeof(double), hipMemcpyDeviceToHost, st));
    WL_HIP(ctx, hipStreamSynchronize(st));
    *result = (double)(T)h;
    ctx->last_kernel = "k_entropy_seg";
    return WL_OK;
}

}  // namespace

extern "C" {

int wl_coefentropy(wl_ctx *ctx, int dtype, const void *x, int64_t n, int et, int have_nrm, double nrm, double *result, void *stream)
{
    if (!ctx || !result || (!x && n > 0)) return WL_EINVAL_ARG;
    if (dtype != WL_F32 && dtype != WL_F64) return WL_EINVAL_DTYPE;
    if (et != WL_ENTROPY_SHANNON && et != WL_ENTROPY_LOGENERGY) return WL_EINVAL_ARG;
    if (n < 0) return WL_EDIMS;
    if (have_nrm && !(nrm >= 0)) return WL_EINVAL_ARG;         // @assert nrm >= 0 (entropy.jl:32); NaN fails it too
    if (n == 0) { *result = 0.0; return WL_OK; }
    WL_SCOPE(ctx);
    hipStream_t st = (hipStream_t)stream;
    return dtype == WL_F32 ? coefentropy_impl<float>(ctx, st, (const float *)x, n, et, have_nrm, nrm, result)
                           : coefentropy_impl<double>(ctx, st, (const double *)x, n, et, have_nrm, nrm, result);
}

}  // extern "C"

// wl_wpt2.hip -- wpt2 / iwpt2: the 2-D wavelet PACKET transform of an image over a quadtree.
//
// The node at depth d with block coordinates (bi, bj), 0 <= bi, bj < 2^d, is the sub-block of rows bi m0 .. (bi + 1) m0 - 1 and
// columns bj m1 .. (bj + 1) m1 - 1 of the n0 x n1 column-major image, m0 = n0 / 2^d, m1 = n1 / 2^d.  Splitting a node replaces the
// block by its one-level 2-D dwt, periodic WITHIN the block (forward: dimension 1 first, then dimension 0; the inverse in the
// reverse order), which leaves the quadrants [[ss, sd], [ds, dd]]; they are the four children.  The tree is a byte per node in
// breadth-first order: depth d starts at (4^d - 1) / 3, a node's place inside its depth is the Morton code of (bi, bj) with bi in
// the even bits -- so the bytes of one depth are that depth's split mask as they stand.
//
//   k_wpt2_level   one depth in one pass over HBM, for nodes too large for LDS.  A workgroup owns a tile of PA x PB coefficient
//                  pairs of ONE node (tiles are cut per node, so a tile never straddles two nodes; the tiles at a node's far edges
//                  are clipped): it stages the 2 PA x 2 PB samples behind them plus the filter halo, indices wrapped modulo the
//                  NODE's extents (no modulo for a tile whose window lies inside the node), runs both axis passes LDS -> LDS and
//                  stores the four quadrant pieces to their final places.  A node whose bit is clear is copied through.
//   k_wpt2_tail    every remaining depth in one launch, from the first depth whose nodes hold at most TAIL_MAX elements: a
//                  workgroup reads G whole nodes into LDS, runs every deeper split of their subtrees between two LDS buffers of
//                  the nodes' footprint (first axis A -> B, second axis B -> A: an unsplit node is never touched and stays put in
//                  A) and writes each node once.
//
// Forward: the level passes of depths 0 .. P - 1, then the tail; inverse: the tail, then the level passes upwards.  The passes
// ping-pong between y and one workspace plane, ordered so that the last one lands in y; x is only read.  Workgroups meet at launch
// boundaries only.
//
// Arithmetic: the closed forms of wl_internal.h in the reference's summation order with separate roundings, any filter length up
// to WL_MAX_FLEN (lines shorter than the filter wrap as often as it takes); the even lengths up to 8 get compile-time tap loops.
// Bit-identical to the oracle's one-level dwt of every split block (tests/test_gpu_wpt2.py).
#include "wl_entry.h"
#include "wl_dev.h"

#include <vector>

using namespace wl;

namespace {

constexpr int W2_THREADS = 256;
constexpr int64_t W2_TAIL_CAP = 4096;    // elements the tail's LDS buffers hold (two of them: 32 KiB Float32, 64 KiB Float64)
constexpr int64_t W2_TAIL_MAX = 256;     // elements of a node the tail takes by default (the sweep of profiles/wpt2.md)
constexpr int W2_TAIL_SLOTS = 16;        // nodes per workgroup of the tail, at most
constexpr int W2_PA = 32, W2_PB = 16;    // pairs per tile of the level kernel (64 x 32 samples), halved while LDS does not hold it

__host__ __device__ inline uint64_t w2_spread(uint32_t v)
{
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// a node's place inside its depth: bi in the even bits
__host__ __device__ inline uint64_t w2_morton(uint32_t bi, uint32_t bj) { return w2_spread(bi) | (w2_spread(bj) << 1); }
__host__ __device__ inline int64_t w2_depth_base(int d) { return (((int64_t)1 << (2 * d)) - 1) / 3; }

__device__ __forceinline__ int w2_pmod(int a, int n)
{
    const int r = a % n;
    return r < 0 ? r + n : r;
}

// g[m] = (-1)^m h[m] (mirror): the same value as Taps::g, taken from h so that a kernel holds one set of taps in scalar registers
template <typename T>
__device__ __forceinline__ T w2_g(const Taps<T> &tp, int m) { return (m & 1) ? -tp.h[m] : tp.h[m]; }

// ---- the four 1-D closed forms (wl_internal.h), on a pre-wrapped window and on a periodic line -------------------------------------
// (s, d) of a pair from its window w[e * st] = x[2k + 2 - F + e], e < 2F - 2 (F = 2: the pair itself)
template <typename T, int FC>
__device__ __forceinline__ void w2_fwd_window(const T *w, int st, int Frt, const Taps<T> &tp, T &s, T &d)
{
    const int F = FC ? FC : Frt;
    const T *ws = w + (F - 2) * st;
    T sv = tp.h[0] * ws[0];
#pragma unroll
    for (int m = 1; m < F; ++m) sv = sv + tp.h[m] * ws[m * st];
    T dv = w2_g(tp, F - 1) * w[0];
#pragma unroll
    for (int m = F - 2; m >= 0; --m) dv = dv + w2_g(tp, m) * w[(F - 1 - m) * st];
    s = sv;
    d = dv;
}
// (s, d) of pair k of the periodic line x[i * st], i < n: one modulo for the start of d, conditional wraps afterwards
template <typename T, int FC>
__device__ __forceinline__ void w2_fwd_line(const T *x, int st, int n, int k, int Frt, const Taps<T> &tp, T &s, T &d)
{
    const int F = FC ? FC : Frt;
    constexpr int UN = FC ? FC : 1;                          // (the run-time length keeps its tap loops rolled)
    int idx = 2 * k;
    T sv = tp.h[0] * x[idx * st];
#pragma unroll UN
    for (int m = 1; m < F; ++m) {
        if (++idx == n) idx = 0;
        sv = sv + tp.h[m] * x[idx * st];
    }
    idx = w2_pmod(2 * k + 2 - F, n);
    T dv = w2_g(tp, F - 1) * x[idx * st];
#pragma unroll UN
    for (int m = F - 2; m >= 0; --m) {
        if (++idx == n) idx = 0;
        dv = dv + w2_g(tp, m) * x[idx * st];
    }
    s = sv;
    d = dv;
}
// The inverse forms also carry the zeros the reference's shift register meets between the coefficients (filtup! upsamples by
// inserting zeros): a chain that enters the register on a zero starts as 0 + ..., one that leaves it on a zero ends with
// + tap * 0.  They change nothing but the sign of a zero result -- with them -0.0 comes out where the oracle has it.
// x[o] from the windows sw[e * st] = s[k0 - HI + e] and dw[e * st] = d[k0 + e], HI = (F - 1) / 2, o counted from sample 2 k0
template <typename T, int FC>
__device__ __forceinline__ T w2_inv_window(const T *sw, const T *dw, int st, int o, int Frt, const Taps<T> &tp)
{
    const int F = FC ? FC : Frt;
    const int HI = (F - 1) / 2;
    const int mt = (((F - 1 - o) & 1) == 0) ? F - 1 : F - 2;
    int e = (o - mt) / 2 + HI;                               // (o - mt is even)
    T S = tp.h[mt] * sw[e * st];
    if (mt == F - 2) S = T(0) + S;
    for (int m = mt - 2; m >= 0; m -= 2) {
        ++e;
        S = S + tp.h[m] * sw[e * st];
    }
    if (o & 1) S = S + tp.h[0] * T(0);
    const int mb = (o & 1) ? 0 : 1;
    e = (o + mb - 1) / 2;
    T D = w2_g(tp, mb) * dw[e * st];
    if (mb == 1) D = T(0) + D;
    for (int m = mb + 2; m < F; m += 2) {
        ++e;
        D = D + w2_g(tp, m) * dw[e * st];
    }
    if ((o + F) & 1) D = D + w2_g(tp, F - 1) * T(0);
    return S + D;
}
// x[o] of a periodic line of n = 2 h samples from its halves sp[k * st], dp[k * st], k < h
template <typename T, int FC>
__device__ __forceinline__ T w2_inv_line(const T *sp, const T *dp, int st, int h, int o, int Frt, const Taps<T> &tp)
{
    const int F = FC ? FC : Frt;
    const int mt = (((F - 1 - o) & 1) == 0) ? F - 1 : F - 2;
    int k = w2_pmod((o - mt) / 2, h);
    T S = tp.h[mt] * sp[k * st];
    if (mt == F - 2) S = T(0) + S;
    for (int m = mt - 2; m >= 0; m -= 2) {
        if (++k == h) k = 0;
        S = S + tp.h[m] * sp[k * st];
    }
    if (o & 1) S = S + tp.h[0] * T(0);
    const int mb = (o & 1) ? 0 : 1;
    k = (o + mb - 1) / 2;
    T D = w2_g(tp, mb) * dp[k * st];
    if (mb == 1) D = T(0) + D;
    for (int m = mb + 2; m < F; m += 2) {
        if (++k == h) k = 0;
        D = D + w2_g(tp, m) * dp[k * st];
    }
    if ((o + F) & 1) D = D + w2_g(tp, F - 1) * T(0);
    return S + D;
}

// Both samples of pair p, (x[2p], x[2p + 1]).  An even compile-time length reads the same coefficients for both -- s[p - HI .. p],
// d[p .. p + HI] -- with fixed taps (the closed form of window_inv, wl_dev.h, plus the zero terms above); the run-time lengths
// take the per-sample forms.
template <typename T, int FC>
__device__ __forceinline__ void w2_inv_pair_taps(const T (&sv)[FC / 2 + 1], const T (&dv)[FC / 2 + 1], const Taps<T> &tp, T &xe, T &xo)
{
    constexpr int HI = (FC - 1) / 2;
    T Se = T(0) + tp.h[FC - 2] * sv[0];
    T So = tp.h[FC - 1] * sv[0];
    T De = T(0) + w2_g(tp, 1) * dv[0];
    T Do = w2_g(tp, 0) * dv[0];
#pragma unroll
    for (int q = 1; q <= HI; ++q) {
        Se = Se + tp.h[FC - 2 - 2 * q] * sv[q];
        So = So + tp.h[FC - 1 - 2 * q] * sv[q];
        De = De + w2_g(tp, 1 + 2 * q) * dv[q];
        Do = Do + w2_g(tp, 2 * q) * dv[q];
    }
    So = So + tp.h[0] * T(0);
    Do = Do + w2_g(tp, FC - 1) * T(0);
    xe = Se + De;
    xo = So + Do;
}
template <typename T, int FC>
__device__ __forceinline__ void w2_inv_pair_window(const T *sw, const T *dw, int st, int p, int Frt, const Taps<T> &tp, T &xe, T &xo)
{
    if constexpr (FC == 0) {
        T x2[2];
#pragma unroll 1
        for (int r = 0; r < 2; ++r) x2[r] = w2_inv_window<T, 0>(sw, dw, st, 2 * p + r, Frt, tp);
        xe = x2[0];
        xo = x2[1];
    } else {
        T sv[FC / 2 + 1], dv[FC / 2 + 1];
#pragma unroll
        for (int q = 0; q <= (FC - 1) / 2; ++q) { sv[q] = sw[(p + q) * st]; dv[q] = dw[(p + q) * st]; }
        w2_inv_pair_taps<T, FC>(sv, dv, tp, xe, xo);
    }
}
template <typename T, int FC>
__device__ __forceinline__ void w2_inv_pair_line(const T *sp, const T *dp, int st, int h, int p, int Frt, const Taps<T> &tp, T &xe, T &xo)
{
    if constexpr (FC == 0) {
        T x2[2];
#pragma unroll 1
        for (int r = 0; r < 2; ++r) x2[r] = w2_inv_line<T, 0>(sp, dp, st, h, 2 * p + r, Frt, tp);
        xe = x2[0];
        xo = x2[1];
    } else {
        constexpr int HI = (FC - 1) / 2;
        T sv[FC / 2 + 1], dv[FC / 2 + 1];
        int ks = w2_pmod(p - HI, h), kd = p;
#pragma unroll
        for (int q = 0; q <= HI; ++q) {
            sv[q] = sp[ks * st];
            dv[q] = dp[kd * st];
            if (++ks == h) ks = 0;
            if (++kd == h) kd = 0;
        }
        w2_inv_pair_taps<T, FC>(sv, dv, tp, xe, xo);
    }
}

// ---- k_wpt2_level --------------------------------------------------------------------------------------------------------------
template <typename T>
struct W2LevelArgs {
    const T *src; T *dst;
    int64_t n0;                     // rows of the image (the stride of a column)
    int m0, m1;                     // extents of a node of this depth (even)
    int lgn;                        // the depth: 2^lgn nodes per dimension
    int PA, PB;                     // pairs per tile along dimension 0 / 1
    int ta, tb;                     // tiles per node along dimension 0 / 1
    const uint8_t *mask;            // the depth's node bits in Morton order (device), or nullptr: every node splits
    Taps<T> tp;
};

// where a workgroup of the level kernel stands: its node, its first pair (a0, b0) inside the node and the pairs it owns (pa x pb)
template <typename T>
struct W2Tile { const T *sn; T *dn; int a0, b0, pa, pb; bool split; };
template <typename T>
__device__ __forceinline__ W2Tile<T> w2_tile(const W2LevelArgs<T> &a)
{
    W2Tile<T> t;
    const int tpn = a.ta * a.tb;
    const int64_t node = (int64_t)blockIdx.x / tpn;
    const int tl = (int)((int64_t)blockIdx.x - node * tpn);
    const int tj = tl / a.ta, ti = tl - tj * a.ta;
    const uint32_t bi = (uint32_t)(node & (((int64_t)1 << a.lgn) - 1)), bj = (uint32_t)(node >> a.lgn);
    const int h0 = a.m0 >> 1, h1 = a.m1 >> 1;
    t.a0 = ti * a.PA; t.b0 = tj * a.PB;
    t.pa = (h0 - t.a0 < a.PA) ? h0 - t.a0 : a.PA;
    t.pb = (h1 - t.b0 < a.PB) ? h1 - t.b0 : a.PB;
    const int64_t off = (int64_t)bi * a.m0 + (int64_t)bj * a.m1 * a.n0;
    t.sn = a.src + off; t.dn = a.dst + off;
    t.split = !a.mask || a.mask[w2_morton(bi, bj)] != 0;
    return t;
}

template <typename T, int FC>
__global__ void __launch_bounds__(W2_THREADS) k_wpt2_level_fwd(W2LevelArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int F = FC ? FC : a.tp.F, H = F - 2;
    const int tid = threadIdx.x;
    const W2Tile<T> t = w2_tile(a);
    const int m0 = a.m0, m1 = a.m1, h0 = m0 >> 1, h1 = m1 >> 1;
    const int64_t n0 = a.n0;
    if (!t.split) {
        // the node is a leaf of the tree (or lies below one): the four quadrant pieces this tile owns pass through
        const int np = t.pa * t.pb;
        for (int it = tid; it < 4 * np; it += W2_THREADS) {
            const int q = it / np, r = it - q * np;
            const int j = r / t.pa, i = r - j * t.pa;
            const int64_t o = (int64_t)(t.a0 + i + (q & 1) * h0) + (int64_t)(t.b0 + j + (q >> 1) * h1) * n0;
            t.dn[o] = t.sn[o];
        }
        return;
    }
    const int R = 2 * t.pa + 2 * H, C = 2 * t.pb + 2 * H, LD = R | 1;
    T *In = reinterpret_cast<T *>(smem_raw);                              // In[i + j LD] = node[(2 a0 - H + i) mod m0, (2 b0 - H + j) mod m1]
    T *Mid = In + (size_t)LD * C;                                         // R rows x (pb s-columns | pb d-columns)
    {
        const int bi0 = 2 * t.a0 - H, bj0 = 2 * t.b0 - H;
        const bool wrap = bi0 < 0 || bi0 + R > m0 || bj0 < 0 || bj0 + C > m1;
        for (int it = tid; it < R * C; it += W2_THREADS) {
            const int j = it / R, i = it - j * R;
            int gi = bi0 + i, gj = bj0 + j;
            if (wrap) { gi = w2_pmod(gi, m0); gj = w2_pmod(gj, m1); }
            In[i + j * LD] = t.sn[gi + (int64_t)gj * n0];
        }
    }
    __syncthreads();
    // dimension 1 first
    for (int it = tid; it < R * t.pb; it += W2_THREADS) {
        const int b = it / R, i = it - b * R;
        T s, d;
        w2_fwd_window<T, FC>(In + i + 2 * b * LD, LD, F, a.tp, s, d);
        Mid[i + b * LD] = s;
        Mid[i + (t.pb + b) * LD] = d;
    }
    __syncthreads();
    for (int it = tid; it < t.pa * 2 * t.pb; it += W2_THREADS) {
        const int jj = it / t.pa, i = it - jj * t.pa;
        T s, d;
        w2_fwd_window<T, FC>(Mid + 2 * i + jj * LD, 1, F, a.tp, s, d);
        const int col = (jj < t.pb) ? t.b0 + jj : h1 + t.b0 + (jj - t.pb);
        T *o = t.dn + (t.a0 + i) + (int64_t)col * n0;
        o[0] = s;
        o[h0] = d;
    }
}

template <typename T, int FC>
__global__ void __launch_bounds__(W2_THREADS) k_wpt2_level_inv(W2LevelArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int F = FC ? FC : a.tp.F, HI = (F - 1) / 2;
    const int tid = threadIdx.x;
    const W2Tile<T> t = w2_tile(a);
    const int h0 = a.m0 >> 1, h1 = a.m1 >> 1;
    const int64_t n0 = a.n0;
    const int TA = 2 * t.pa, TB = 2 * t.pb;
    if (!t.split) {
        for (int it = tid; it < TA * TB; it += W2_THREADS) {
            const int j = it / TA, i = it - j * TA;
            const int64_t o = (int64_t)(2 * t.a0 + i) + (int64_t)(2 * t.b0 + j) * n0;
            t.dn[o] = t.sn[o];
        }
        return;
    }
    const int WA = t.pa + HI, WB = t.pb + HI, RA = 2 * WA, CB = 2 * WB, LD = RA | 1, LDM = TA | 1;
    // In: rows [s-window | d-window] of dimension 0 (WA each), columns the same of dimension 1 (WB each);
    // s-window e <-> half-index (a0 - HI + e) mod h0, d-window e <-> (a0 + e) mod h0
    T *In = reinterpret_cast<T *>(smem_raw);
    T *Mid = In + (size_t)LD * CB;                                        // TA rows x CB columns
    {
        const bool wrap = t.a0 - HI < 0 || t.a0 + WA > h0 || t.b0 - HI < 0 || t.b0 + WB > h1;
        for (int it = tid; it < RA * CB; it += W2_THREADS) {
            const int j = it / RA, i = it - j * RA;
            int gi = (i < WA) ? t.a0 - HI + i : t.a0 + (i - WA);
            int gj = (j < WB) ? t.b0 - HI + j : t.b0 + (j - WB);
            if (wrap) { gi = w2_pmod(gi, h0); gj = w2_pmod(gj, h1); }
            if (i >= WA) gi += h0;
            if (j >= WB) gj += h1;
            In[i + j * LD] = t.sn[gi + (int64_t)gj * n0];
        }
    }
    __syncthreads();
    // dimension 0 first: the reverse of the forward order
    for (int it = tid; it < t.pa * CB; it += W2_THREADS) {
        const int j = it / t.pa, p = it - j * t.pa;
        const T *col = In + j * LD;
        T xe, xo;
        w2_inv_pair_window<T, FC>(col, col + WA, 1, p, F, a.tp, xe, xo);
        Mid[2 * p + j * LDM] = xe;
        Mid[2 * p + 1 + j * LDM] = xo;
    }
    __syncthreads();
    for (int it = tid; it < TA * t.pb; it += W2_THREADS) {
        const int q = it / TA, i = it - q * TA;
        const T *row = Mid + i;
        T xe, xo;
        w2_inv_pair_window<T, FC>(row, row + WB * LDM, LDM, q, F, a.tp, xe, xo);
        T *o = t.dn + (2 * t.a0 + i) + (int64_t)(2 * t.b0 + 2 * q) * n0;
        o[0] = xe;
        o[n0] = xo;
    }
}

// ---- k_wpt2_tail ---------------------------------------------------------------------------------------------------------------
template <typename T>
struct W2TailArgs {
    const T *src; T *dst;
    int64_t n0;
    int m0, m1;                     // extents of a node of depth dt
    int dt, nd;                     // the first depth handled here and the number of depths
    int G;                          // nodes per workgroup
    int lgw;                        // 2^lgw lanes walk dimension 0 (the power of two that covers m0, at most 64), the rest the columns
    int64_t nnodes;                 // 4^dt
    const uint8_t *tree;            // the whole tree (device), or nullptr: every node above depth dt + nd splits
    Taps<T> tp;
};

// node g of the workgroup: its block coordinates at depth dt
template <typename T>
__device__ __forceinline__ void w2_tail_node(const W2TailArgs<T> &a, int g, uint32_t &bi, uint32_t &bj)
{
    const int64_t node = (int64_t)blockIdx.x * a.G + g;
    bi = (uint32_t)(node & (((int64_t)1 << a.dt) - 1));
    bj = (uint32_t)(node >> a.dt);
}
// does sub-node (u, v) at q depths below node g split?
template <typename T>
__device__ __forceinline__ bool w2_tail_split(const W2TailArgs<T> &a, int g, int q, int u, int v)
{
    if (!a.tree) return true;
    uint32_t bi, bj;
    w2_tail_node(a, g, bi, bj);
    return a.tree[w2_depth_base(a.dt + q) + (int64_t)w2_morton((bi << q) + (uint32_t)u, (bj << q) + (uint32_t)v)] != 0;
}
// The loops of the tail: lane tx of 2^lgw walks dimension 0 (contiguous in memory and in LDS), row ty of the rest walks the
// (node, column) pairs -- the divisions that find a column's node are paid once per column, not once per element.
#define W2_TAIL_LANES                                                                                   \
    const int W = 1 << a.lgw, tx = (int)threadIdx.x & (W - 1), ty = (int)threadIdx.x >> a.lgw, NY = W2_THREADS >> a.lgw
template <typename T, bool IN>
__device__ __forceinline__ void w2_tail_move(const W2TailArgs<T> &a, T *A, int cnt)
{
    W2_TAIL_LANES;
    const int m0 = a.m0, m1 = a.m1;
    for (int gj = ty; gj < cnt * m1; gj += NY) {
        const int g = gj / m1, j = gj - g * m1;
        uint32_t bi, bj;
        w2_tail_node(a, g, bi, bj);
        const int64_t o = (int64_t)bi * m0 + ((int64_t)bj * m1 + j) * a.n0;
        for (int i = tx; i < m0; i += W) {
            if (IN) A[gj * m0 + i] = a.src[o + i];
            else a.dst[o + i] = A[gj * m0 + i];
        }
    }
}

template <typename T, int FC>
__global__ void __launch_bounds__(W2_THREADS) k_wpt2_tail_fwd(W2TailArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int F = FC ? FC : a.tp.F;
    W2_TAIL_LANES;
    const int m0 = a.m0, m1 = a.m1, E = m0 * m1, hm0 = m0 >> 1, hm1 = m1 >> 1;
    const int64_t left = a.nnodes - (int64_t)blockIdx.x * a.G;
    const int cnt = left < a.G ? (int)left : a.G;
    T *A = reinterpret_cast<T *>(smem_raw);
    T *B = A + (size_t)a.G * E;
    w2_tail_move<T, true>(a, A, cnt);
    __syncthreads();
    for (int q = 0; q < a.nd; ++q) {
        const int s0 = m0 >> q, s1 = m1 >> q, h0 = s0 >> 1, h1 = s1 >> 1;
        // dimension 1, A -> B: pair b of sub-node column v, every row i
        for (int gp = ty; gp < cnt * hm1; gp += NY) {
            const int g = gp / hm1, pc = gp - g * hm1;
            const int v = pc / h1, b = pc - v * h1;
            for (int i = tx; i < m0; i += W) {
                if (!w2_tail_split(a, g, q, i / s0, v)) continue;
                const int o = g * E + i + v * s1 * m0;
                T s, d;
                w2_fwd_line<T, FC>(A + o, m0, s1, b, F, a.tp, s, d);
                B[o + b * m0] = s;
                B[o + (h1 + b) * m0] = d;
            }
        }
        __syncthreads();
        // dimension 0, B -> A: column j, every pair of rows
        for (int gj = ty; gj < cnt * m1; gj += NY) {
            const int g = gj / m1, j = gj - g * m1, v = j / s1;
            for (int pr = tx; pr < hm0; pr += W) {
                const int u = pr / h0, k = pr - u * h0;
                if (!w2_tail_split(a, g, q, u, v)) continue;
                const int o = g * E + u * s0 + j * m0;
                T s, d;
                w2_fwd_line<T, FC>(B + o, 1, s0, k, F, a.tp, s, d);
                A[o + k] = s;
                A[o + h0 + k] = d;
            }
        }
        __syncthreads();
    }
    w2_tail_move<T, false>(a, A, cnt);
}

template <typename T, int FC>
__global__ void __launch_bounds__(W2_THREADS) k_wpt2_tail_inv(W2TailArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int F = FC ? FC : a.tp.F;
    W2_TAIL_LANES;
    const int m0 = a.m0, m1 = a.m1, E = m0 * m1, hm0 = m0 >> 1, hm1 = m1 >> 1;
    const int64_t left = a.nnodes - (int64_t)blockIdx.x * a.G;
    const int cnt = left < a.G ? (int)left : a.G;
    T *A = reinterpret_cast<T *>(smem_raw);
    T *B = A + (size_t)a.G * E;
    w2_tail_move<T, true>(a, A, cnt);
    __syncthreads();
    for (int q = a.nd - 1; q >= 0; --q) {                                 // children before parents
        const int s0 = m0 >> q, s1 = m1 >> q, h0 = s0 >> 1, h1 = s1 >> 1;
        // dimension 0, A -> B: column j, every pair of rows
        for (int gj = ty; gj < cnt * m1; gj += NY) {
            const int g = gj / m1, j = gj - g * m1, v = j / s1;
            for (int pr = tx; pr < hm0; pr += W) {
                const int u = pr / h0, k = pr - u * h0;
                if (!w2_tail_split(a, g, q, u, v)) continue;
                const int o = g * E + u * s0 + j * m0;
                T xe, xo;
                w2_inv_pair_line<T, FC>(A + o, A + o + h0, 1, h0, k, F, a.tp, xe, xo);
                B[o + 2 * k] = xe;
                B[o + 2 * k + 1] = xo;
            }
        }
        __syncthreads();
        // dimension 1, B -> A: pair b of sub-node column v, every row i
        for (int gp = ty; gp < cnt * hm1; gp += NY) {
            const int g = gp / hm1, pc = gp - g * hm1;
            const int v = pc / h1, b = pc - v * h1;
            for (int i = tx; i < m0; i += W) {
                if (!w2_tail_split(a, g, q, i / s0, v)) continue;
                const int o = g * E + i + v * s1 * m0;
                T xe, xo;
                w2_inv_pair_line<T, FC>(B + o, B + o + h1 * m0, m0, h1, b, F, a.tp, xe, xo);
                A[o + 2 * b * m0] = xe;
                A[o + (2 * b + 1) * m0] = xo;
            }
        }
        __syncthreads();
    }
    w2_tail_move<T, false>(a, A, cnt);
}
#undef W2_TAIL_LANES

// ---- launch geometry -------------------------------------------------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is sticky per (function, device): once
inline hipError_t w2_allow_lds(const void *fn, size_t shmem)
{
    if (shmem <= 48 * 1024) return hipSuccess;
    static thread_local const void *done_fn[64];
    static thread_local int done_dev[64];
    static thread_local int ndone = 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    for (int i = 0; i < ndone; ++i)
        if (done_fn[i] == fn && done_dev[i] == dev) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    if (ndone < 64) { done_fn[ndone] = fn; done_dev[ndone] = dev; ++ndone; }
    return hipSuccess;
}

// LDS elements of a level tile of PA x PB pairs
inline size_t w2_level_elems(int F, int fw, int PA, int PB)
{
    if (fw) {
        const size_t R = (size_t)2 * PA + 2 * (F - 2), C = (size_t)2 * PB + 2 * (F - 2);
        return (R | 1) * C + (R | 1) * 2 * PB;
    }
    const size_t HI = (size_t)(F - 1) / 2, RA = 2 * (PA + HI), CB = 2 * (PB + HI);
    return (RA | 1) * CB + ((size_t)(2 * PA) | 1) * CB;
}
// the tile of a level pass: W2_PA x W2_PB pairs, halved (the larger side first) until the tile and its halo fit 64 KiB with at least
// 8 pairs per side; filters too long for that take the whole 160 KiB of a CU
template <typename T>
inline void w2_level_tile(int F, int fw, int &PA, int &PB)
{
    for (size_t budget : {(size_t)64 * 1024, (size_t)160 * 1024}) {
        const int least = budget == (size_t)64 * 1024 ? 8 : 1;
        PA = W2_PA; PB = W2_PB;
        while (w2_level_elems(F, fw, PA, PB) * sizeof(T) > budget && (PA > least || PB > least)) {
            if (PA >= PB && PA > least) PA >>= 1;
            else if (PB > least) PB >>= 1;
            else PA >>= 1;
        }
        if (w2_level_elems(F, fw, PA, PB) * sizeof(T) <= budget) return;
    }
}

template <typename T, int FC>
hipError_t w2_level_launch_f(hipStream_t st, const W2LevelArgs<T> &a, int fw, size_t shmem, int64_t blocks)
{
    const void *fn = fw ? reinterpret_cast<const void *>(&k_wpt2_level_fwd<T, FC>) : reinterpret_cast<const void *>(&k_wpt2_level_inv<T, FC>);
    const hipError_t e = w2_allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    if (fw) hipLaunchKernelGGL((k_wpt2_level_fwd<T, FC>), dim3((unsigned)blocks), dim3(W2_THREADS), shmem, st, a);
    else hipLaunchKernelGGL((k_wpt2_level_inv<T, FC>), dim3((unsigned)blocks), dim3(W2_THREADS), shmem, st, a);
    return hipGetLastError();
}
template <typename T, int FC>
hipError_t w2_tail_launch_f(hipStream_t st, const W2TailArgs<T> &a, int fw, size_t shmem, int64_t blocks)
{
    const void *fn = fw ? reinterpret_cast<const void *>(&k_wpt2_tail_fwd<T, FC>) : reinterpret_cast<const void *>(&k_wpt2_tail_inv<T, FC>);
    const hipError_t e = w2_allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    if (fw) hipLaunchKernelGGL((k_wpt2_tail_fwd<T, FC>), dim3((unsigned)blocks), dim3(W2_THREADS), shmem, st, a);
    else hipLaunchKernelGGL((k_wpt2_tail_inv<T, FC>), dim3((unsigned)blocks), dim3(W2_THREADS), shmem, st, a);
    return hipGetLastError();
}
// compile-time tap loops for the even lengths up to 8, the run-time length otherwise (with 10 Float64 taps held in scalar
// registers the forward tail spilled four of them: the longer filters keep their taps in memory)
#define W2_BY_F(CALL)                    \
    switch (F) {                         \
    case 2: return CALL(2);              \
    case 4: return CALL(4);              \
    case 6: return CALL(6);              \
    case 8: return CALL(8);              \
    default: return CALL(0);             \
    }

// one depth: nodes of m0 x m1 at depth d, mask = that depth's bits on the device (nullptr: all split)
template <typename T>
hipError_t w2_level(hipStream_t st, const Taps<T> &taps, int fw, const T *src, T *dst, int64_t n0, int64_t n1, int d, const uint8_t *mask)
{
    W2LevelArgs<T> a;
    a.src = src; a.dst = dst; a.n0 = n0;
    a.m0 = (int)(n0 >> d); a.m1 = (int)(n1 >> d); a.lgn = d;
    const int F = taps.F;
    w2_level_tile<T>(F, fw, a.PA, a.PB);
    const int h0 = a.m0 >> 1, h1 = a.m1 >> 1;
    a.ta = (h0 + a.PA - 1) / a.PA; a.tb = (h1 + a.PB - 1) / a.PB;
    a.mask = mask; a.tp = taps;
    const int64_t blocks = ((int64_t)1 << (2 * d)) * a.ta * a.tb;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidConfiguration;
    const size_t shmem = w2_level_elems(F, fw, a.PA, a.PB) * sizeof(T);
#define W2_CALL(FF_) w2_level_launch_f<T, FF_>(st, a, fw, shmem, blocks)
    W2_BY_F(W2_CALL)
#undef W2_CALL
}

// depths dt .. dt + nd - 1 of nodes of at most W2_TAIL_CAP elements; tree = the whole tree on the device (nullptr: all split)
template <typename T>
hipError_t w2_tail(hipStream_t st, const Taps<T> &taps, int fw, const T *src, T *dst, int64_t n0, int64_t n1, int dt, int nd, const uint8_t *tree)
{
    W2TailArgs<T> a;
    a.src = src; a.dst = dst; a.n0 = n0;
    a.m0 = (int)(n0 >> dt); a.m1 = (int)(n1 >> dt); a.dt = dt; a.nd = nd;
    a.nnodes = (int64_t)1 << (2 * dt);
    const int64_t E = (int64_t)a.m0 * a.m1;
    int64_t G = W2_TAIL_CAP / E;
    if (G > W2_TAIL_SLOTS) G = W2_TAIL_SLOTS;
    if (G > a.nnodes) G = a.nnodes;
    if (G < 1) G = 1;
    a.G = (int)G;
    a.lgw = 0;
    while (a.lgw < 6 && (1 << a.lgw) < a.m0) ++a.lgw;
    a.tree = tree; a.tp = taps;
    const int F = taps.F;
    const int64_t blocks = (a.nnodes + G - 1) / G;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidConfiguration;
    const size_t shmem = (size_t)(2 * G * E) * sizeof(T);
#define W2_CALL(FF_) w2_tail_launch_f<T, FF_>(st, a, fw, shmem, blocks)
    W2_BY_F(W2_CALL)
#undef W2_CALL
}

// the largest node the tail takes: option WL_WPT2_TAIL_MAX in elements, clamped to [1, W2_TAIL_CAP] (1: the tail is never used)
inline int64_t w2_tail_max()
{
    const int64_t v = (int64_t)opt("WL_WPT2_TAIL_MAX", (long long)W2_TAIL_MAX);
    return v < 1 ? 1 : (v > W2_TAIL_CAP ? W2_TAIL_CAP : v);
}

// tree: the HOST tree cut to depth L ((4^L - 1) / 3 nodes, valid, some node of depth L - 1 set), or nullptr: the full tree of depth L
template <typename T>
int wpt2_impl(wl_ctx *ctx, hipStream_t st, T *y, const T *x, int64_t n0, int64_t n1, const Taps<T> &taps, int L, const uint8_t *tree, int fw)
{
    const size_t plane = (size_t)(n0 * n1) * sizeof(T);
    if (L == 0) {
        WL_HIP(ctx, hipMemcpyAsync(y, x, plane, hipMemcpyDeviceToDevice, st));
        ctx->last_kernel = "copy";
        return WL_OK;
    }
    // the first depth whose nodes the tail takes; P level passes above it
    const int64_t tmax = w2_tail_max();
    int dt = 0;
    while (dt < L && (n0 >> dt) * (n1 >> dt) > tmax) ++dt;
    const int P = dt, K = P + (dt < L ? 1 : 0);
    const size_t pb = K >= 2 ? up256(plane) : 0, tb = tree ? (size_t)w2_depth_base(L) : 0;
    if (pb + tb) WL_TRY(wl_ensure_ws(ctx, pb + tb, st, true));
    T *ws = (T *)ctx->ws;
    const uint8_t *dtree = nullptr;
    if (tree) {
        dtree = (const uint8_t *)ctx->ws + pb;
        WL_TRY(wl_stage_to_device(ctx, (void *)dtree, tree, tb, st));
    }
    // pass i of K reads what pass i - 1 wrote (pass 0: x) and writes y when an even number of passes follow it
    const T *cur = x;
    for (int i = 0; i < K; ++i) {
        T *dst = ((K - 1 - i) % 2 == 0) ? y : ws;
        const bool tail = fw ? (i == P) : (dt < L && i == 0);
        if (tail) {
            WL_HIP(ctx, w2_tail<T>(st, taps, fw, cur, dst, n0, n1, dt, L - dt, dtree));
            ctx->last_kernel = "k_wpt2_tail";
        } else {
            const int d = fw ? i : K - 1 - i;
            WL_HIP(ctx, w2_level<T>(st, taps, fw, cur, dst, n0, n1, d, dtree ? dtree + w2_depth_base(d) : nullptr));
            ctx->last_kernel = "k_wpt2_level";
        }
        cur = dst;
    }
    return WL_OK;
}

// the checks both entry points share after their pointers: dtype, filter, extents
inline int wpt2_check(int dtype, const int64_t *dims, int flen)
{
    WL_TRY(check_dtype(dtype));
    WL_TRY(check_flen(flen));
    // (an extent of 2^31 or more: beyond the 32-bit node coordinates of the kernels)
    if (dims[0] < 1 || dims[1] < 1 || dims[0] >= ((int64_t)1 << 31) || dims[1] >= ((int64_t)1 << 31)) return WL_EDIMS;
    return WL_OK;
}
inline bool w2_divides(const int64_t *dims, int L) { return L < 31 && dims[0] % ((int64_t)1 << L) == 0 && dims[1] % ((int64_t)1 << L) == 0; }

}  // namespace

extern "C" {

int wl_wpt2_filter_full(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, const double *qmf, int flen, int L, int fw,
                        void *stream)
{
    if (!ctx || !y || !x || !dims || !qmf) return WL_EINVAL_ARG;
    WL_TRY(wpt2_check(dtype, dims, flen));
    if (L < 0) return WL_EINVAL_L;
    if (!w2_divides(dims, L)) return WL_EINVAL_SIZE;
    if (y == x) return WL_EALIAS;
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return wpt2_impl<T>(ctx, st, (T *)y, (const T *)x, dims[0], dims[1], taps_of<T>(qmf, flen), L, nullptr, fw);
    });
}

int wl_wpt2_filter(wl_ctx *ctx, int dtype, void *y, const void *x, const int64_t *dims, const double *qmf, int flen, const uint8_t *tree,
                   int64_t ntree, int fw, void *stream)
{
    if (!ctx || !y || !x || !dims || !qmf || (!tree && ntree > 0)) return WL_EINVAL_ARG;
    WL_TRY(wpt2_check(dtype, dims, flen));
    if (y == x) return WL_EALIAS;
    // ntree = (4^L - 1) / 3 for an L the extents allow; no set node below a clear one
    int L = 0;
    while (L < 31 && w2_depth_base(L) < ntree) ++L;
    if (ntree < 0 || w2_depth_base(L) != ntree || !w2_divides(dims, L)) return WL_EINVAL_TREE;
    int Leff = 0;                                            // 1 + the depth of the deepest set node
    for (int d = 0; d < L; ++d) {
        const int64_t b = w2_depth_base(d), e = w2_depth_base(d + 1);
        for (int64_t k = b; k < e; ++k)
            if (tree[k]) {
                if (k > 0 && !tree[(k - 1) / 4]) return WL_EINVAL_TREE;
                Leff = d + 1;
            }
    }
    return scoped_by_dtype(ctx, dtype, stream, [&](auto t, hipStream_t st) {
        using T = decltype(t);
        return wpt2_impl<T>(ctx, st, (T *)y, (const T *)x, dims[0], dims[1], taps_of<T>(qmf, flen), Leff, Leff ? tree : nullptr, fw);
    });
}

}  // extern "C"

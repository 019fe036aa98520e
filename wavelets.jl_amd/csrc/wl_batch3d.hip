// wl_batch3d.hip -- level loops of a BATCH of independent 3-D filter-bank transforms (wl_dwt_filter_batch3; the spins of a
// translation-invariant denoise of a cube): patches of a volume, video blocks -- boxes so small that a transform is a handful of
// launches whose time is launch latency.  Here every level that one of the one-launch 3-D tiers accepts is ONE launch over all volumes:
//
//   k_tail3       (wl_tail.hip)    <= 4096 elements, all remaining levels: one workgroup per volume (blockIdx.x)
//   k_level3_lds  (wl_level3.hip)  4096 < elements <= 2^18 (2^20): the volume on blockIdx.y
//   k_fwd3d_one / k_inv3d_one      the volume is the slowest-varying part of the workgroup index
//
// The choice per level is the single-volume one (tail3_ok, then fast3d_fwd_tier / fast3d_inv_tier of wl_axis.hip), judged on the
// pointers of volume 0: every volume base is 16-byte aligned (the loops below require xs, ys and the approximation slot to be
// multiples of 16 bytes), so all volumes answer alike.  Levels of the axis-pass, any-extent and generic families run volume after
// volume on the same stream, sharing one volume's T0 / T1.  Nothing in the arithmetic changes: the kernels are the single-volume
// ones with a base offset per volume.
#include "wl_fast.h"

namespace wl {

namespace {

// the single-volume loops, volume after volume
template <typename T>
bool loop_all(int path, int F, int64_t N, int64_t nvol, int64_t xs, int64_t ys, const T *x, const T *y)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    return opt("WL_BATCH3_LOOP", 0) != 0 || nvol == 1 || path != 0 || (F % 2) != 0 || F > 10 || (xs % VEC) != 0 || (ys % VEC) != 0 ||
           ((N >> 3) % VEC) != 0 || !al16(x) || !al16(y);
}

inline BoxSpec volume_box(const int64_t dims[3])
{
    BoxSpec b;
    b.nd = 3; b.nt = 3;
    for (int d = 0; d < 3; ++d) b.dims[d] = dims[d];
    b.full = dense_strides(b.dims);
    return b;
}

}  // namespace

#define WL_TRYB(expr)                                                  \
    do {                                                               \
        hipError_t e__ = (expr);                                       \
        if (e__ != hipSuccess) { if (hip_err) *hip_err = (int)e__; return WL_EHIP; } \
    } while (0)

template <typename T>
int filter_fwd_levels_vols(void *ws, bool ws_gen, int cu_count, int path, hipStream_t st, const int64_t dims[3], int64_t nvol, int64_t xs,
                           int64_t ys, T *y, const T *x, const Taps<T> &taps, int L, const char **kernel_name, int *hip_err)
{
    const int F = taps.F;
    const int64_t N = dims[0] * dims[1] * dims[2], as = N >> 3;
    const BoxSpec b = volume_box(dims);
    if (nvol < 1 || nvol > 65535) return WL_EINVAL_ARG;
    if (loop_all<T>(path, F, N, nvol, xs, ys, x, y)) {
        for (int64_t v = 0; v < nvol; ++v) {
            int rc = filter_fwd_levels<T>(ws, ws_gen, cu_count, path, st, b, y + v * ys, x + v * xs, taps, L, kernel_name, hip_err);
            if (rc) return rc;
        }
        return WL_OK;
    }
    // A, B: nvol slots of `as` elements each (the level-l approximation of volume v, dense, at slot v); T0, T1: one volume
    T *const A = (T *)ws, *const B = A + nvol * as + 64;
    T *const T0 = ws_gen ? B + nvol * as + 64 : nullptr, *const T1 = ws_gen ? T0 + N : nullptr;
    const char *dominant = nullptr;
    const T *cur = x;
    Strides3 cur_st = b.full;
    int64_t cur_vs = xs;
    int pp = 0;
    for (int l = 1; l <= L; ++l) {
        int64_t n[3];
        level_box(b, l, n);
        const bool last = (l == L);
        T *const llbuf = pp ? B : A;
        const int64_t hn[3] = {n[0] >> 1, n[1] >> 1, n[2] >> 1};
        const Strides3 ll_st = dense_strides(hn), box_st = dense_strides(n);
        // ---- <= 4096 elements: every remaining level, one workgroup per volume ----
        if (opt("WL_TAIL3", 1) != 0 && tail3_ok<T>(F, n[0], n[1], n[2], L - l + 1)) {
            WL_TRYB(launch_tail3<T>(st, taps, 1, cur, cur_st.s[1], cur_st.s[2], y, b.full.s[1], b.full.s[2], (int)n[0], (int)n[1], (int)n[2],
                                    L - l + 1, (int)nvol, cur_vs, ys));
            if (!dominant) dominant = "k_tail3_batch";
            break;
        }
        if (!ws_gen) return WL_RETRY_GEN;
        T *const ll = last ? (T *)nullptr : llbuf;
        const int tier = opt("WL_NO_FAST3D", 0) == 0 ? fast3d_fwd_tier<T>(F, cur, cur_st.s[1], cur_st.s[2], y, b.full.s[1], b.full.s[2], ll, n, T0, T1) : 0;
        const VolBatch vb = {nvol, cur_vs, ys, as};
        if (tier == 1) {
            WL_TRYB(fwd3d_one_launch<T>(st, taps, cur, cur_st.s[1], cur_st.s[2], y, b.full.s[1], b.full.s[2], ll, n, cu_count, vb));
            if (!dominant) dominant = "k_fwd3d_one_batch";
        } else if (tier == 2) {
            WL_TRYB(level3_lds_launch<T>(st, taps, 1, cur, cur_st.s[1], cur_st.s[2], y, b.full.s[1], b.full.s[2], (const T *)nullptr, ll, n, vb));
            if (!dominant) dominant = "k_level3_lds_batch";
        } else {
            // ---- volume after volume: the axis passes, else the any-extent / generic passes (as filter_fwd_levels) ----
            const Extent3 ext = {{n[0], n[1], n[2]}}, lo = {{hn[0], hn[1], hn[2]}};
            for (int64_t v = 0; v < nvol; ++v) {
                const T *const cv = cur + v * cur_vs;
                T *const yv = y + v * ys, *const lv = last ? (T *)nullptr : llbuf + v * as;
                bool done = false;
                if (tier == 3) {
                    hipError_t e3 = hipSuccess;
                    const char *k3 = nullptr;
                    done = fast3d_fwd_level<T>(st, taps, cv, cur_st.s[1], cur_st.s[2], yv, b.full.s[1], b.full.s[2], lv, n, T0, T1, cu_count, &e3, &k3);
                    WL_TRYB(e3);
                    if (done && !dominant) dominant = k3;
                }
                if (done) continue;
                const T *in = cv;
                Strides3 in_st = cur_st;
                int tog = 0;
                for (int a = 2; a >= 0; --a) {
                    const bool any = opt("WL_ANYAXIS", 1) != 0 && any_axis_ok(F, ext, a);
                    T *const out = (a != 0) ? (tog ? T1 : T0) : yv;
                    const Strides3 out_st = (a != 0) ? box_st : b.full;
                    T *const lla = (a != 0) ? (T *)nullptr : lv;
                    const Strides3 lla_st = (a != 0) ? box_st : ll_st;
                    if (any) WL_TRYB(any_axis_pass<T>(st, taps, 1, in, in_st, out, out_st, lla, lla_st, ext, a, lo));
                    else WL_TRYB(generic_fwd_filter_pass<T>(st, taps, in, in_st, out, out_st, lla, lla_st, ext, a, lo));
                    if (a == 0 && !dominant) dominant = any ? "k_fwd_any" : "k_generic_fwd_filter";
                    in = out; in_st = out_st; tog ^= 1;
                }
            }
        }
        cur = llbuf; cur_st = ll_st; cur_vs = as; pp ^= 1;
    }
    if (kernel_name) *kernel_name = dominant ? dominant : "none";
    return WL_OK;
}

template <typename T>
int filter_inv_levels_vols(void *ws, bool ws_gen, int cu_count, int path, hipStream_t st, const int64_t dims[3], int64_t nvol, int64_t xs,
                           int64_t ys, T *y, const T *x, const Taps<T> &taps, int L, const char **kernel_name, int *hip_err)
{
    const int F = taps.F;
    const int64_t N = dims[0] * dims[1] * dims[2], as = N >> 3;
    const BoxSpec b = volume_box(dims);
    if (nvol < 1 || nvol > 65535) return WL_EINVAL_ARG;
    // (here x is the coefficient array and y the reconstruction)
    if (loop_all<T>(path, F, N, nvol, xs, ys, x, y)) {
        for (int64_t v = 0; v < nvol; ++v) {
            int rc = filter_inv_levels<T>(ws, ws_gen, cu_count, path, st, b, y + v * ys, x + v * xs, taps, L, kernel_name, hip_err);
            if (rc) return rc;
        }
        return WL_OK;
    }
    T *const A = (T *)ws, *const B = A + nvol * as + 64;
    T *const T0 = ws_gen ? B + nvol * as + 64 : nullptr, *const T1 = ws_gen ? T0 + N : nullptr;
    const char *dominant = nullptr;
    const T *llsrc = nullptr;                    // the deeper reconstruction (slot v of A / B, dense), or nullptr: the approximation is in x
    int pp = 0;
    int l_start = L;
    // ---- the deepest levels whose output is a power-of-two box of <= 4096 elements: one workgroup per volume ----
    if (opt("WL_TAIL3", 1) != 0) {
        int l_lo = L + 1;
        for (int q = L; q >= 1; --q) {
            int64_t nq[3];
            level_box(b, q, nq);
            if (tail3_ok<T>(F, nq[0], nq[1], nq[2], L - q + 1)) l_lo = q; else break;
        }
        if (l_lo <= L) {
            int64_t nq[3];
            level_box(b, l_lo, nq);
            const bool to_y = (l_lo == 1);
            T *const res = to_y ? y : (pp ? B : A);
            const Strides3 res_st = to_y ? b.full : dense_strides(nq);
            WL_TRYB(launch_tail3<T>(st, taps, 0, x, b.full.s[1], b.full.s[2], res, res_st.s[1], res_st.s[2], (int)nq[0], (int)nq[1], (int)nq[2],
                                    L - l_lo + 1, (int)nvol, xs, to_y ? ys : as));
            dominant = "k_tail3_batch";
            llsrc = res; pp ^= 1;
            l_start = l_lo - 1;
        }
    }
    for (int l = l_start; l >= 1; --l) {
        int64_t n[3];
        level_box(b, l, n);
        if (!ws_gen) return WL_RETRY_GEN;
        const int64_t hn[3] = {n[0] >> 1, n[1] >> 1, n[2] >> 1};
        const Strides3 box_st = dense_strides(n), llsrc_st = dense_strides(hn);
        T *const res = (l == 1) ? y : (pp ? B : A);
        const Strides3 res_st = (l == 1) ? b.full : box_st;
        const int64_t res_vs = (l == 1) ? ys : as;
        const int tier = opt("WL_NO_FAST3D", 0) == 0 ? fast3d_inv_tier<T>(F, x, b.full.s[1], b.full.s[2], llsrc, res, res_st.s[1], res_st.s[2], n, T0, T1) : 0;
        const VolBatch vb = {nvol, xs, res_vs, as};
        if (tier == 1) {
            WL_TRYB(inv3d_one_launch<T>(st, taps, x, b.full.s[1], b.full.s[2], llsrc, res, res_st.s[1], res_st.s[2], n, cu_count, vb));
            dominant = "k_inv3d_one_batch";
        } else if (tier == 2) {
            WL_TRYB(level3_lds_launch<T>(st, taps, 0, x, b.full.s[1], b.full.s[2], res, res_st.s[1], res_st.s[2], llsrc, (T *)nullptr, n, vb));
            dominant = "k_level3_lds_batch";
        } else {
            const Extent3 ext = {{n[0], n[1], n[2]}}, lo = {{hn[0], hn[1], hn[2]}};
            for (int64_t v = 0; v < nvol; ++v) {
                const T *const xv = x + v * xs, *const lv = llsrc ? llsrc + v * as : (const T *)nullptr;
                T *const rv = res + v * res_vs;
                bool done = false;
                if (tier == 3) {
                    hipError_t e3 = hipSuccess;
                    const char *k3 = nullptr;
                    done = fast3d_inv_level<T>(st, taps, xv, b.full.s[1], b.full.s[2], lv, rv, res_st.s[1], res_st.s[2], n, T0, T1, cu_count, &e3, &k3);
                    WL_TRYB(e3);
                    if (done) dominant = k3;
                }
                if (done) continue;
                const T *in = xv;
                Strides3 in_st = b.full;
                int tog = 0;
                for (int a = 0; a < 3; ++a) {
                    const bool firstp = (a == 0), lastp = (a == 2);
                    T *out; Strides3 out_st;
                    if (lastp) { out = rv; out_st = res_st; }
                    else { out = tog ? T1 : T0; out_st = box_st; tog ^= 1; }
                    const bool any = opt("WL_ANYAXIS", 1) != 0 && any_axis_ok(F, ext, a);
                    if (any)
                        WL_TRYB(any_axis_pass<T>(st, taps, 0, in, in_st, out, out_st, firstp ? const_cast<T *>(lv) : (T *)nullptr, llsrc_st, ext, a, lo));
                    else
                        WL_TRYB(generic_inv_filter_pass<T>(st, taps, in, in_st, firstp ? lv : (const T *)nullptr, llsrc_st, out, out_st, ext, a, lo));
                    in = out; in_st = out_st;
                    if (lastp && !dominant) dominant = any ? "k_inv_any" : "k_generic_inv_filter";
                }
            }
        }
        llsrc = res; pp ^= 1;
    }
    if (kernel_name) *kernel_name = dominant ? dominant : "none";
    return WL_OK;
}
#undef WL_TRYB

#define WL_INST_VOLS(T)                                                                                                                   \
    template int filter_fwd_levels_vols<T>(void *, bool, int, int, hipStream_t, const int64_t[3], int64_t, int64_t, int64_t, T *, const T *, \
                                           const Taps<T> &, int, const char **, int *);                                                   \
    template int filter_inv_levels_vols<T>(void *, bool, int, int, hipStream_t, const int64_t[3], int64_t, int64_t, int64_t, T *, const T *, \
                                           const Taps<T> &, int, const char **, int *);
WL_INST_VOLS(float)
WL_INST_VOLS(double)

}  // namespace wl

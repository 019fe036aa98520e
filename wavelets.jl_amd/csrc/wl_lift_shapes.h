// wl_lift_shapes.h -- what the lifting fast paths (wl_lift.hip, wl_lift_tile.hip) share on the host side: the scheme shapes known
// at compile time, the coefficient block their kernels take, the dispatch from a run-time shape id to a kernel template, and the
// small launch helpers.
#pragma once
#include <type_traits>
#include <vector>
#include "wl_internal.h"

namespace wl {

// ---- scheme shapes known at compile time (coefficients stay run-time data) -----------------------
// direction-adjusted order (as produced by make_scheme): step i = {is_update, nc, shift}
struct StepShape { int upd, nc, sh; };
// the shape-specialised kernels never have more steps than this; their argument blocks carry only these coefficients
// (keeping kernel arguments small matters: launches with > 256 bytes of arguments were seen to stall the enqueue path)
constexpr int LIFT_FAST_STEPS = 4;
template <int ID> struct Shape;
// cdf9/7 forward and inverse have the same shape sequence read in opposite order
template <> struct Shape<0> { static constexpr int NS = 4; static constexpr StepShape S[4] = {{1, 2, 0}, {0, 2, 1}, {1, 2, 0}, {0, 2, 1}}; };   // cdf9/7 fw
template <> struct Shape<1> { static constexpr int NS = 4; static constexpr StepShape S[4] = {{0, 2, 1}, {1, 2, 0}, {0, 2, 1}, {1, 2, 0}}; };   // cdf9/7 inv
template <> struct Shape<2> { static constexpr int NS = 3; static constexpr StepShape S[3] = {{0, 1, 0}, {1, 2, 1}, {0, 1, -1}}; };             // db2 fw
template <> struct Shape<3> { static constexpr int NS = 3; static constexpr StepShape S[3] = {{0, 1, -1}, {1, 2, 1}, {0, 1, 0}}; };             // db2 inv
template <> struct Shape<4> { static constexpr int NS = 2; static constexpr StepShape S[2] = {{0, 1, 0}, {1, 1, 0}}; };                          // haar/db1 fw
template <> struct Shape<5> { static constexpr int NS = 2; static constexpr StepShape S[2] = {{1, 1, 0}, {0, 1, 0}}; };                          // haar/db1 inv

// dependency cone of a scheme in (s, d) pairs: how far a pair's final value reaches to the left / right
template <int ID>
struct LiftReach {
    static constexpr int left()
    {
        int v = 0;
        for (int k = 0; k < Shape<ID>::NS; ++k) { const int a = Shape<ID>::S[k].sh; if (a > 0) v += a; }
        return v;
    }
    static constexpr int right()
    {
        int v = 0;
        for (int k = 0; k < Shape<ID>::NS; ++k) { const int b = Shape<ID>::S[k].nc - 1 - Shape<ID>::S[k].sh; if (b > 0) v += b; }
        return v;
    }
    static constexpr int HP = left() > right() ? left() : right();
};

// ---- the coefficient block every shape-specialised kernel takes among its arguments -----------------------------------------
// (an aggregate, carried by the argument structs as one member `cf`; steps beyond the scheme's own are zero)
template <typename T>
struct LiftCoefs {
    T c[LIFT_FAST_STEPS][WL_MAX_NCOEF];
    T norm1, norm2;
};
template <typename T>
inline LiftCoefs<T> lift_coefs(const LiftScheme<T> &sc)
{
    LiftCoefs<T> k;
    for (int i = 0; i < LIFT_FAST_STEPS; ++i)
        for (int j = 0; j < WL_MAX_NCOEF; ++j) k.c[i][j] = (i < sc.nsteps) ? sc.step[i].c[j] : (T)0;
    k.norm1 = sc.norm1; k.norm2 = sc.norm2;
    return k;
}

// ---- from a run-time shape id to a kernel template --------------------------------------------------------------------------
// f(ShapeId<id>()): the one place where a shape id becomes a template argument (as by_dtype in wl_entry.h for the element type).
// Callers write
//     return by_shape(id, hipErrorInvalidValue, [&](auto sid) { constexpr int ID = decltype(sid)::value; ...k_foo<T, ID, FW>... });
// An id outside the set returns `none` without calling f: it never reaches another shape's kernel.
template <int ID> using ShapeId = std::integral_constant<int, ID>;
// the direction a shape belongs to: even ids are the forward step sequences, odd ids the same sequences read backwards
constexpr int shape_fw(int id) { return (id & 1) ? 0 : 1; }

// all six shapes: the kernel families that take either direction's shape in either direction (stream, axis, short lines)
template <typename R, typename F>
inline R by_shape(int id, R none, F f)
{
    switch (id) {
    case 0: return f(ShapeId<0>());
    case 1: return f(ShapeId<1>());
    case 2: return f(ShapeId<2>());
    case 3: return f(ShapeId<3>());
    case 4: return f(ShapeId<4>());
    case 5: return f(ShapeId<5>());
    default: return none;
    }
}
// the three shapes of one direction, FW ? {0, 2, 4} : {1, 3, 5}: every other family, instantiated for its own direction only
template <int FW, typename R, typename F>
inline R by_shape_dir(int id, R none, F f)
{
    if constexpr (FW != 0) {
        switch (id) {
        case 0: return f(ShapeId<0>());
        case 2: return f(ShapeId<2>());
        case 4: return f(ShapeId<4>());
        default: return none;
        }
    } else {
        switch (id) {
        case 1: return f(ShapeId<1>());
        case 3: return f(ShapeId<3>());
        case 5: return f(ShapeId<5>());
        default: return none;
        }
    }
}
// ... with the direction a run-time value (f takes its direction from the id: shape_fw(ID))
template <typename R, typename F>
inline R by_shape_dir(int fw, int id, R none, F f)
{
    return fw ? by_shape_dir<1>(id, none, f) : by_shape_dir<0>(id, none, f);
}
inline bool shape_in_dir(int id, int fw) { return id >= 0 && id <= 5 && shape_fw(id) == (fw ? 1 : 0); }

// the id of the known shape a direction-adjusted scheme has, or -1
template <typename T>
inline int match_shape(const LiftScheme<T> &sc)
{
    for (int id = 0; id <= 5; ++id) {
        const bool same = by_shape(id, false, [&](auto sid) {
            typedef Shape<decltype(sid)::value> SH;
            if (sc.nsteps != SH::NS) return false;
            for (int i = 0; i < SH::NS; ++i)
                if (sc.step[i].is_update != SH::S[i].upd || sc.step[i].nc != SH::S[i].nc || sc.step[i].shift != SH::S[i].sh) return false;
            return true;
        });
        if (same) return id;
    }
    return -1;
}

// ---- launch helpers ---------------------------------------------------------------------------------------------------------
inline int l_env(const char *name, int dflt) { return (int)opt(name, dflt); }   // per-context options

// a failed call / launch inside a *_fast function: its HIP error goes to the function's *hip_err and WL_EHIP comes back
#define WL_E(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { if (hip_err) *hip_err = (int)e__; return WL_EHIP; } } while (0)
#define WL_EL() WL_E(hipGetLastError())

// gridDim.y holds at most 65535 blocks: `nlines` lines go out in slabs of at most `slab` per launch, f(first line, lines)
template <typename F>
inline void for_line_slabs(int64_t nlines, int64_t slab, F f)
{
    for (int64_t l0 = 0; l0 < nlines; l0 += slab) f(l0, (nlines - l0 < slab) ? (nlines - l0) : slab);
}
// the slab size the line kernels that read the option use
inline int64_t slab_lines_opt() { return (l_env("WL_SLAB_LINES", 32768) > 0) ? l_env("WL_SLAB_LINES", 32768) : 32768; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is sticky per (function, device) and costs tens of microseconds: raise the
// limit to the LDS size once per kernel and device (and host thread) instead of on every call
template <auto KERNEL>
inline hipError_t lift_max_lds_once()
{
    static thread_local std::vector<char> done;         // by device
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0) return hipErrorInvalidDevice;
    if ((size_t)dev < done.size() && done[dev]) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    if ((size_t)dev >= done.size()) done.resize((size_t)dev + 1, 0);
    done[dev] = 1;
    return hipSuccess;
}

}  // namespace wl

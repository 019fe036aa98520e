// wl_lift_dev.h -- what the lifting kernels (wl_lift.hip, wl_lift_tile.hip) share on the device side: the cross-lane moves, the
// vector loads / stores of a lane's registers, and lift_update: how a lifting step updates an element whose operands are in
// registers.  Its callers are reg_line_steps (wl_lift.hip) and seg_line_steps_v (wl_lift_tile.hip); the other kernels of
// wl_lift.hip carry the same two sums written out.
#pragma once
#include "wl_internal.h"
#include "wl_lift_shapes.h"

namespace wl {

// ---- cross-lane moves ---------------------------------------------------------------------------------------------------------
// l_next / l_prev: the value of lane i+1 / i-1 (zero past the ends of the wave); l_rol / l_ror: the same with lane 63's neighbour
// lane 0 (a line held by the whole wave: the periodic boundary); l_partner: lane i ^ 1; l_gather: any lane (ds_bpermute)
__device__ __forceinline__ int l_dpp_next(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false); }
__device__ __forceinline__ int l_dpp_prev(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int l_dpp_partner(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ int l_dpp_rol(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x134, 0xf, 0xf, false); }   // lane i <- lane i+1 (mod 64)
__device__ __forceinline__ int l_dpp_ror(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x13C, 0xf, 0xf, false); }   // lane i <- lane i-1 (mod 64)
__device__ __forceinline__ float l_partner(float v) { return __int_as_float(l_dpp_partner(__float_as_int(v))); }
__device__ __forceinline__ double l_partner(double v) { return __hiloint2double(l_dpp_partner(__double2hiint(v)), l_dpp_partner(__double2loint(v))); }
__device__ __forceinline__ float l_next(float v) { return __int_as_float(l_dpp_next(__float_as_int(v))); }
__device__ __forceinline__ float l_prev(float v) { return __int_as_float(l_dpp_prev(__float_as_int(v))); }
__device__ __forceinline__ double l_next(double v) { return __hiloint2double(l_dpp_next(__double2hiint(v)), l_dpp_next(__double2loint(v))); }
__device__ __forceinline__ double l_prev(double v) { return __hiloint2double(l_dpp_prev(__double2hiint(v)), l_dpp_prev(__double2loint(v))); }
__device__ __forceinline__ float l_rol(float v) { return __int_as_float(l_dpp_rol(__float_as_int(v))); }
__device__ __forceinline__ float l_ror(float v) { return __int_as_float(l_dpp_ror(__float_as_int(v))); }
__device__ __forceinline__ double l_rol(double v) { return __hiloint2double(l_dpp_rol(__double2hiint(v)), l_dpp_rol(__double2loint(v))); }
__device__ __forceinline__ double l_ror(double v) { return __hiloint2double(l_dpp_ror(__double2hiint(v)), l_dpp_ror(__double2loint(v))); }
__device__ __forceinline__ float l_gather(float v, int srclane) { return __int_as_float(__builtin_amdgcn_ds_bpermute(srclane << 2, __float_as_int(v))); }
__device__ __forceinline__ double l_gather(double v, int srclane)
{
    return __hiloint2double(__builtin_amdgcn_ds_bpermute(srclane << 2, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(srclane << 2, __double2loint(v)));
}

// ---- N consecutive elements of a lane, moved in 16-byte pieces (or one piece of N elements when that is less) --------------------
template <typename T, int N>
__device__ __forceinline__ void ldv_l(const T *p, T (&v)[N])
{
    constexpr int C = ((int)(16 / sizeof(T)) < N) ? (int)(16 / sizeof(T)) : N;
    typedef T V __attribute__((ext_vector_type(C)));
#pragma unroll
    for (int c = 0; c < N / C; ++c) {
        V t = *reinterpret_cast<const V *>(p + c * C);
#pragma unroll
        for (int i = 0; i < C; ++i) v[c * C + i] = t[i];
    }
}
template <typename T, int N>
__device__ __forceinline__ void stv_l(T *p, const T (&v)[N])
{
    constexpr int C = ((int)(16 / sizeof(T)) < N) ? (int)(16 / sizeof(T)) : N;
    typedef T V __attribute__((ext_vector_type(C)));
#pragma unroll
    for (int c = 0; c < N / C; ++c) {
        V t;
#pragma unroll
        for (int i = 0; i < C; ++i) t[i] = v[c * C + i];
        *reinterpret_cast<V *>(p + c * C) = t;
    }
}

// ---- the arithmetic contract ----------------------------------------------------------------------------------------------------
// Rounding follows the reference exactly: an element none of whose nc operands wraps around the ends of the line is updated as
//     x + (c0*a + c1*b [+ c2*c])              lift_inbounds!, transforms_lifting.jl:455-483
// and a wrapped one as
//     ((x + c0*a) + c1*b) [+ c2*c]            lift_perboundary!, transforms_lifting.jl:437-451
// The two differ in the last bit for nc >= 2.  "In bounds" is 0 <= j - shift and j - shift + nc - 1 <= half - 1 for element j of a
// half of `half` elements (irlimits, :383-390).  The exact library is built without FMA contraction; the opt-in fused library
// compiles these same functions with contraction allowed.
//
// The operands o[0 .. nc-1] are already in registers; both sums are computed (they share their products) and one is selected, so
// a wave whose lanes differ in `inb` does not branch.  FAST: the caller has established that nothing wraps.  (The kernels
// that still spell the two sums out themselves, and why: profiles/lift_dev_refactor.md.)
template <typename T, bool FAST = false>
__device__ __forceinline__ T lift_update(const T x, const T (&c)[WL_MAX_NCOEF], const T (&o)[3], const int nc, const bool inb)
{
    const T m0 = c[0] * o[0];
    T acc = m0;
    T xb = x + m0;
    if (nc > 1) { const T m1 = c[1] * o[1]; acc = acc + m1; xb = xb + m1; }
    if (nc > 2) { const T m2 = c[2] * o[2]; acc = acc + m2; xb = xb + m2; }
    const T xin = x + acc;
    if constexpr (FAST) return xin;
    else return inb ? xin : xb;
}

}  // namespace wl

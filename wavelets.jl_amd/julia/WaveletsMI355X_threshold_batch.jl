# WaveletsMI355X_threshold_batch.jl -- threshold! of a batch of independent units on the device, included from WaveletsMI355X.jl:
#   threshold_batch!(x, TH, t)            HardTH / SoftTH / SemiSoftTH / SteinTH: t a number, or a device vector of one Float64 per unit
#   threshold_batch!(x, PosTH()|NegTH())  no threshold
#   threshold_batch!(x, BiggestTH(), m)   the best m-term approximation of every unit: m an integer, or a device vector of one Int64 per unit
# x is a device array whose last dimension is the batch; a unit is everything in front of it.  The reference has no batched form:
# every call equals the loop of `threshold!(x[.., i], TH, t_i)` over the units, bit for bit (ties of BiggestTH at the cut are cleared
# in index order, as the single call on the device does), in one launch for the element-wise kinds and without a host round trip for
# BiggestTH (wl_threshold_batch / wl_threshold_biggest_batch).  Host numbers are checked as the reference does (@assert t >= 0,
# m >= 0); the entries of a device vector are not -- that would synchronise -- and m is clamped to [0, length of a unit] there.
# tests/test_julia_glue_threshold_batch.py lints every ccall of this file against the ABI.

# (elements per unit, units)
function threshold_units(x::ROCArray{T,N}) where {T,N}
    nb = Int64(size(x, N))
    nb >= 1 && length(x) >= 1 || throw(ArgumentError("empty batch"))
    return Int64(length(x) ÷ nb), nb
end

# One method per threshold type, as the single threshold! (WaveletsMI355X.jl) has them
for TH in (:HardTH, :SoftTH, :SemiSoftTH, :SteinTH)
    @eval function threshold_batch!(x::ROCArray{T,N}, ::$TH, t::Real) where {T<:Union{Float32,Float64},N}
        t >= 0 || throw(AssertionError("t >= 0"))
        n, nb = threshold_units(x)
        GC.@preserve x check(ccall((:wl_threshold_batch, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cdouble, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                    ctx(), DT[T], pointer(x), n, nb, n, THCODE[$TH], Float64(t), C_NULL, t_is_f64(T, t), stream()))
        return x
    end
    @eval function threshold_batch!(x::ROCArray{T,N}, ::$TH, t::ROCVector{Float64}) where {T<:Union{Float32,Float64},N}
        n, nb = threshold_units(x)
        length(t) == nb || throw(DimensionMismatch("t must have one entry per unit"))
        GC.@preserve x t check(ccall((:wl_threshold_batch, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cdouble, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                    ctx(), DT[T], pointer(x), n, nb, n, THCODE[$TH], 0.0, pointer(t), t_is_f64(T, 0.0), stream()))
        return x
    end
end
for TH in (:PosTH, :NegTH)
    @eval function threshold_batch!(x::ROCArray{T,N}, ::$TH) where {T<:Union{Float32,Float64},N}
        n, nb = threshold_units(x)
        GC.@preserve x check(ccall((:wl_threshold_batch, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Cdouble, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                    ctx(), DT[T], pointer(x), n, nb, n, THCODE[$TH], 0.0, C_NULL, Cint(0), stream()))
        return x
    end
end
function threshold_batch!(x::ROCArray{T,N}, ::BiggestTH, m::Integer) where {T<:Union{Float32,Float64},N}
    m >= 0 || throw(AssertionError("m >= 0"))
    n, nb = threshold_units(x)
    GC.@preserve x check(ccall((:wl_threshold_biggest_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(x), n, nb, n, Int64(m), C_NULL, stream()))
    return x
end
function threshold_batch!(x::ROCArray{T,N}, ::BiggestTH, m::ROCVector{Int64}) where {T<:Union{Float32,Float64},N}
    n, nb = threshold_units(x)
    length(m) == nb || throw(DimensionMismatch("m must have one entry per unit"))
    GC.@preserve x m check(ccall((:wl_threshold_biggest_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(x), n, nb, n, Int64(0), pointer(m), stream()))
    return x
end

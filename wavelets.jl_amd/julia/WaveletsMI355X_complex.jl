# WaveletsMI355X_complex.jl -- complex-valued dwt / idwt / wpt on the device, included from WaveletsMI355X.jl.
# The reference's transforms take ValueType = Union{AbstractFloat, Complex} (transforms_main.jl:7); with these methods a
# ROCArray{ComplexF32} / ROCArray{ComplexF64} reaches the library instead of the reference's generic scalar loops:
#   _dwt!(y, x, filter::OrthoFilter, L, fw)   vectors, matrices, 3-D arrays     (wl_dwt_filter_complex)
#   _dwt!(y, scheme::GLS, L, fw)              vectors, square matrices, cubes   (wl_dwt_lifting_complex, in place)
#   _wpt!(y, x, filter, tree, fw) / _wpt!(y, scheme, tree, fw) and the wpt! / iwpt! / wpt / iwpt forms that take a depth
# Complex{T} is (re, im) interleaved and the taps are real: re(y) = transform(re(x)), im(y) = transform(im(x)), each bit for bit
# what the real methods return (DESIGN.md section 13).  dtype is the COMPONENT type, extents count complex elements.
# The pre-checks and exceptions are those of the real methods.  tests/test_julia_glue_complex.py lints every ccall of this file.
const CplxT = Union{Float32,Float64}

function dwt_filter_complex_device!(y, x, filter::OrthoFilter, L::Integer, fw::Bool, ::Type{T}, N::Int) where {T}
    size(x) == size(y) || throw(DimensionMismatch("in and out array size must match"))
    q = filter.qmf
    GC.@preserve y x check(ccall((:wl_dwt_filter_complex, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Int64, Ptr{Float64}, Cint, Cint, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), N, dims3(x), 1, length(x), q, length(q), L, fw, stream()))
    return y
end
function Transforms._dwt!(y::ROCVector{Complex{T}}, x::ROCVector{Complex{T}}, filter::OrthoFilter, L::Integer, fw::Bool) where {T<:CplxT}
    return dwt_filter_complex_device!(y, x, filter, L, fw, T, 1)
end
function Transforms._dwt!(y::ROCMatrix{Complex{T}}, x::ROCMatrix{Complex{T}}, filter::OrthoFilter, L::Integer, fw::Bool) where {T<:CplxT}
    return dwt_filter_complex_device!(y, x, filter, L, fw, T, 2)
end
function Transforms._dwt!(y::ROCArray{Complex{T},3}, x::ROCArray{Complex{T},3}, filter::OrthoFilter, L::Integer, fw::Bool) where {T<:CplxT}
    return dwt_filter_complex_device!(y, x, filter, L, fw, T, 3)
end

# dwt!(y, scheme, L): in place on y (y == x in the library's terms)
function dwt_lifting_complex_device!(y, scheme::GLS, L::Integer, fw::Bool, ::Type{T}, N::Int) where {T}
    isup, nc, sh, cf = flatten(scheme)
    GC.@preserve y check(ccall((:wl_dwt_lifting_complex, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                 Cdouble, Cdouble, Cint, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(y), N, dims3(y), 1, length(y), length(isup), isup, nc, sh, cf,
                scheme.norm1, scheme.norm2, L, fw, stream()))
    return y
end
function Transforms._dwt!(y::ROCVector{Complex{T}}, scheme::GLS, L::Integer, fw::Bool) where {T<:CplxT}
    return dwt_lifting_complex_device!(y, scheme, L, fw, T, 1)
end
function Transforms._dwt!(y::ROCMatrix{Complex{T}}, scheme::GLS, L::Integer, fw::Bool) where {T<:CplxT}
    return dwt_lifting_complex_device!(y, scheme, L, fw, T, 2)
end
function Transforms._dwt!(y::ROCArray{Complex{T},3}, scheme::GLS, L::Integer, fw::Bool) where {T<:CplxT}
    return dwt_lifting_complex_device!(y, scheme, L, fw, T, 3)
end

# dwt(x, scheme, L) / idwt: out of place straight from x (the reference's copyto!(y, x) is the split pass)
for (f, fw) in ((:dwt, true), (:idwt, false))
    @eval function Transforms.$f(x::ROCArray{Complex{T},N}, scheme::GLS, L::Integer=Util.maxtransformlevels(x)) where {T<:CplxT,N}
        y = similar(x)
        isup, nc, sh, cf = flatten(scheme)
        GC.@preserve y x check(ccall((:wl_dwt_lifting_complex, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                     Cdouble, Cdouble, Cint, Cint, Ptr{Cvoid}),
                    ctx(), DT[T], pointer(y), pointer(x), N, dims3(x), 1, length(x), length(isup), isup, nc, sh, cf,
                    scheme.norm1, scheme.norm2, L, $fw, stream()))
        return y
    end
end

# ---- wavelet packets: one complex signal -------------------------------------------------------------------------------------
function Transforms._wpt!(y::ROCVector{Complex{T}}, x::ROCVector{Complex{T}}, filter::OrthoFilter, tree::BitVector, fw::Bool) where {T<:CplxT}
    size(x) == size(y) || throw(DimensionMismatch("in and out array size must match"))
    t = UInt8.(tree)
    GC.@preserve y x check(ccall((:wl_wpt_filter_complex, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), length(x), filter.qmf, length(filter.qmf), t, length(t), 0, fw, stream()))
    return y
end
function Transforms._wpt!(y::ROCVector{Complex{T}}, scheme::GLS, tree::BitVector, fw::Bool) where {T<:CplxT}
    isup, nc, sh, cf = flatten(scheme)
    t = UInt8.(tree)
    GC.@preserve y check(ccall((:wl_wpt_lifting_complex, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                 Cdouble, Cdouble, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(y), length(y), length(isup), isup, nc, sh, cf, scheme.norm1, scheme.norm2,
                t, length(t), 0, fw, stream()))
    return y
end

# wpt!(y, x, filter, L::Integer) / wpt!(y, scheme, L::Integer) / wpt(x, wt, L): the full tree of depth L, no tree vector (tree = NULL)
for (f, fw) in ((:wpt!, true), (:iwpt!, false))
    @eval function Transforms.$f(y::ROCVector{Complex{T}}, x::ROCVector{Complex{T}}, filter::OrthoFilter,
                                 L::Integer=Util.maxtransformlevels(x)) where {T<:CplxT}
        size(x) == size(y) || throw(DimensionMismatch("in and out array size must match"))
        0 <= L <= Util.maxtransformlevels(x) || throw(AssertionError("0 <= L <= maxtransformlevels(n)"))   # maketree's @assert
        GC.@preserve y x check(ccall((:wl_wpt_filter_complex, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid}),
                    ctx(), DT[T], pointer(y), pointer(x), length(x), filter.qmf, length(filter.qmf), Ptr{UInt8}(C_NULL), 0, L, $fw, stream()))
        return y
    end
    @eval function Transforms.$f(y::ROCVector{Complex{T}}, scheme::GLS, L::Integer=Util.maxtransformlevels(y)) where {T<:CplxT}
        0 <= L <= Util.maxtransformlevels(y) || throw(AssertionError("0 <= L <= maxtransformlevels(n)"))
        isup, nc, sh, cf = flatten(scheme)
        GC.@preserve y check(ccall((:wl_wpt_lifting_complex, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                     Cdouble, Cdouble, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid}),
                    ctx(), DT[T], pointer(y), pointer(y), length(y), length(isup), isup, nc, sh, cf, scheme.norm1, scheme.norm2,
                    Ptr{UInt8}(C_NULL), 0, L, $fw, stream()))
        return y
    end
end
for (f, fb) in ((:wpt, :wpt!), (:iwpt, :iwpt!))
    @eval function Transforms.$f(x::ROCVector{Complex{T}}, filter::OrthoFilter, L::Integer=Util.maxtransformlevels(x)) where {T<:CplxT}
        return Transforms.$fb(similar(x), x, filter, L)
    end
    @eval function Transforms.$f(x::ROCVector{Complex{T}}, scheme::GLS, L::Integer=Util.maxtransformlevels(x)) where {T<:CplxT}
        return Transforms.$fb(copy(x), scheme, L)
    end
end

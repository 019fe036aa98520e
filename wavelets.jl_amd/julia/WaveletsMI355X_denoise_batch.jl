# WaveletsMI355X_denoise_batch.jl -- denoise of a batch of independent units on the device, included from WaveletsMI355X.jl:
#   denoise_batch(x, wt; L, dnt, sigma, return_sigma)   x: len x B signals, n x n x B square images or n x n x n x B cubes
#   noisest_batch(x, wt, L)                             the B noise estimates as a device vector of Float64
#   mad_batch!(y)                                       mad! of every column of a device matrix
# The reference has no batched form: denoise_batch(x, wt) equals the loop of `denoise(x[.., i], wt)` over the units, bit for bit,
# but every unit's sigma = noisest(x_i, wt) is estimated and applied on the device (wl_denoise_batch_filter /
# wl_denoise_batch_lifting: one forward transform, one MAD launch, one threshold launch and one inverse per group of units, no host
# round trip).  Not part of these calls: wt = nothing, BiggestTH / PosTH / NegTH and TI = true (denoise_ti_batch,
# WaveletsMI355X_denoise_ti_batch.jl).
# tests/test_julia_glue_denoise_batch.py lints every ccall of this file against the ABI.
using Wavelets.Threshold: DNFT, VisuShrink, HardTH, SoftTH, SemiSoftTH, SteinTH

const BATCH_TH = Union{HardTH,SoftTH,SemiSoftTH,SteinTH}

# (unit extents padded to three, units, elements per unit); the reference's error for a unit that is no square / cube
function batch_units(x::ROCArray{T,N}) where {T,N}
    2 <= N <= 4 || throw(ArgumentError("expected len x B signals, n x n x B images or n x n x n x B cubes"))
    unit = size(x)[1:N-1]
    all(==(unit[1]), unit) || throw(ArgumentError("array must be square/cube"))
    return Int64[unit..., ones(Int, 4 - N)...], Int64(size(x, N)), Int64(prod(unit))
end

"""mad!(y[:, i]) for every column of a device matrix in one launch; y is overwritten by the absolute deviations.  Returns a device
vector of Float64; nothing synchronises."""
function mad_batch!(y::ROCMatrix{T}) where {T<:Union{Float32,Float64}}
    r = ROCVector{Float64}(undef, size(y, 2))
    GC.@preserve y r check(ccall((:wl_mad_batch, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), size(y, 1), size(y, 2), size(y, 1), pointer(r), stream()))
    return r
end

"""noisest(x[.., i], wt, L) of every unit: batched transform, the detail range of every first column, one mad_batch!, / 0.6745"""
function noisest_batch(x::ROCArray{T,N}, wt::Union{OrthoFilter,GLS}=Threshold.DEFAULT_WAVELET, L::Integer=1) where {T<:Union{Float32,Float64},N}
    batch_units(x)
    y = N == 2 ? dwtc(x, wt, L) : dwt_batch(x, wt, L)
    dr = y[Util.detailrange(size(y, 1), L), ntuple(_ -> 1, N - 2)..., :]
    return mad_batch!(dr) ./ 0.6745
end

function denoise_batch(x::ROCArray{T,N}, wt::OrthoFilter=Threshold.DEFAULT_WAVELET;
                       L::Int=min(Util.maxtransformlevels(size(x, 1)), 6), dnt::VisuShrink{<:BATCH_TH}=VisuShrink(size(x, 1)),
                       sigma::Union{Nothing,AbstractVector{<:Real}}=nothing, return_sigma::Bool=false) where {T<:Union{Float32,Float64},N}
    dims, nb, nunit = batch_units(x)
    sg = batch_sigma(sigma, nb)
    sout = ROCVector{Float64}(undef, nb)
    sig_in = sg === nothing ? sout : sg
    y = similar(x)
    q = Vector{Float64}(wt.qmf)
    GC.@preserve y x sig_in sout check(ccall((:wl_denoise_batch_filter, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Int64, Ptr{Float64}, Cint, Cint, Cint, Cdouble,
                 Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), Cint(N - 1), dims, nb, nunit, q, length(q), L, THCODE[typeof(dnt.th)], Float64(dnt.t),
                sg === nothing ? Ptr{Float64}(C_NULL) : pointer(sig_in), pointer(sout), stream()))
    return return_sigma ? (y, sout) : y
end

function denoise_batch(x::ROCArray{T,N}, wt::GLS;
                       L::Int=min(Util.maxtransformlevels(size(x, 1)), 6), dnt::VisuShrink{<:BATCH_TH}=VisuShrink(size(x, 1)),
                       sigma::Union{Nothing,AbstractVector{<:Real}}=nothing, return_sigma::Bool=false) where {T<:Union{Float32,Float64},N}
    dims, nb, nunit = batch_units(x)
    sg = batch_sigma(sigma, nb)
    sout = ROCVector{Float64}(undef, nb)
    sig_in = sg === nothing ? sout : sg
    y = similar(x)
    isup, nc, sh, cf = flatten(wt)
    GC.@preserve y x sig_in sout check(ccall((:wl_denoise_batch_lifting, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                 Cdouble, Cdouble, Cint, Cint, Cdouble, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), Cint(N - 1), dims, nb, nunit, length(isup), isup, nc, sh, cf, Float64(wt.norm1),
                Float64(wt.norm2), L, THCODE[typeof(dnt.th)], Float64(dnt.t),
                sg === nothing ? Ptr{Float64}(C_NULL) : pointer(sig_in), pointer(sout), stream()))
    return return_sigma ? (y, sout) : y
end

# per-unit noise levels from the caller: a host vector is validated as threshold! would (@assert t >= 0) and uploaded, a device
# vector of Float64 is taken as it is
batch_sigma(::Nothing, nb) = nothing
function batch_sigma(s::ROCVector{Float64}, nb)
    length(s) == nb || throw(DimensionMismatch("sigma must have one entry per unit"))
    return s
end
function batch_sigma(s::AbstractVector{<:Real}, nb)
    length(s) == nb || throw(DimensionMismatch("sigma must have one entry per unit"))
    all(>=(0), s) || throw(AssertionError("t >= 0"))
    return ROCVector{Float64}(Vector{Float64}(s))
end

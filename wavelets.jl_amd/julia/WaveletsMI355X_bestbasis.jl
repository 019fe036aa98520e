# WaveletsMI355X_bestbasis.jl -- best-basis search of packet trees on the device: `Threshold.bestbasistree` (both forms) and
# `Threshold.coefentropy` for ROCArrays (src/Threshold/entropy.jl:15-111), included from WaveletsMI355X.jl.
#
# The reference's own methods do not reach the device: bestbasistree allocates a host Vector{T} as scratch, calls `dwt!` with a
# host view on one side and a device view on the other, and sums `coefentropy` one element at a time (entropy.jl:47-111) -- on a
# ROCVector that is a scalar-indexing error.  These methods call wl_bestbasistree_filter / wl_coefentropy instead: the packet
# content of every node is bit-identical to wpt's, the entropies follow the accuracy contract of DESIGN.md section 11 (Float64 log
# and sums, deterministic; the tree equals the reference's wherever a decision is not a near-tie).
# Kept apart from WaveletsMI355X.jl because tests/test_julia_glue.py lints that file against the transform and threshold seam
# (tests/golden/reference_seam_signatures.json); tests/test_julia_glue_bestbasis.py lints this one against entropy.jl
# (tests/golden/reference_bestbasis_signatures.json).
using Wavelets.Threshold: Entropy, ShannonEntropy, LogEnergyEntropy
using Wavelets.WT: DiscreteWavelet, OrthoFilter

# the entropies with a device form; any other Entropy subtype keeps the reference's generic method
entcode(::ShannonEntropy) = Cint(0)
entcode(::LogEnergyEntropy) = Cint(1)
entcode(::Entropy) = nothing

function Threshold.coefentropy(x::ROCArray{T}, et::Entropy, nrm::T) where {T<:Union{Float32,Float64}}
    code = entcode(et)
    code === nothing && return invoke(Threshold.coefentropy, Tuple{AbstractArray{T},Entropy,T}, x, et, nrm)
    @assert nrm >= 0
    r = Ref{Cdouble}(0)
    GC.@preserve x check(ccall((:wl_coefentropy, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(x), length(x), code, Cint(1), Float64(nrm), r, stream()))
    return T(r[])
end
# nrm = norm(x), computed on the device (Float64 sum of squares, rounded to T)
function Threshold.coefentropy(x::ROCArray{T}, et::Entropy) where {T<:Union{Float32,Float64}}
    code = entcode(et)
    code === nothing && return invoke(Threshold.coefentropy, Tuple{AbstractArray{T},Entropy}, x, et)
    r = Ref{Cdouble}(0)
    GC.@preserve x check(ccall((:wl_coefentropy, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(x), length(x), code, Cint(0), 0.0, r, stream()))
    return T(r[])
end

# The tree is a host BitVector in and out, one byte per node across the ABI.  One stream synchronisation (the returned tree).
function Threshold.bestbasistree(y::ROCVector{T}, wt::OrthoFilter, tree::BitVector,
                                 et::Entropy=ShannonEntropy()) where {T<:Union{Float32,Float64}}
    code = entcode(et)
    code === nothing && return invoke(Threshold.bestbasistree, Tuple{AbstractVector{T},DiscreteWavelet,BitVector,Entropy}, y, wt, tree, et)
    tb = Vector{UInt8}(tree)
    out = zeros(UInt8, length(tb))
    q = Vector{Float64}(wt.qmf)
    GC.@preserve y check(ccall((:wl_bestbasistree_filter, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Ptr{UInt8}, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), length(y), q, length(q), tb, length(tb), code, out, Ptr{Float64}(C_NULL), stream()))
    return BitVector(out .!= 0)
end
function Threshold.bestbasistree(y::ROCVector{T}, wt::OrthoFilter, L::Integer=Util.maxtransformlevels(y),
                                 et::Entropy=ShannonEntropy()) where {T<:Union{Float32,Float64}}
    return Threshold.bestbasistree(y, wt, Util.maketree(length(y), L, :full), et)
end

# WaveletsMI355X_modwt_batch.jl -- the maximal-overlap transform of a panel of vectors, included from WaveletsMI355X.jl:
#   modwt_batch(x, wt[, L])    x: len x B device matrix, unit i = x[:, i]  ->  len x (L+1) x B, [:, :, i] = modwt(x[:, i], wt, L)
#   imodwt_batch(xw, wt)       xw: len x ncols x B                          ->  len x B,        [:, i]    = imodwt(xw[:, :, i], wt)
# The reference has no batched form: both equal the loop of modwt / imodwt over the units, bit for bit, in one launch for units
# that fit in LDS and one launch per level otherwise (wl_modwt_batch / wl_imodwt_batch).  The reference's errors for a bad L.
# tests/test_julia_glue_modwt_batch.py lints every ccall of this file against the ABI.

function modwt_batch(x::ROCMatrix{T}, wt::OrthoFilter, L::Integer=Util.maxmodwttransformlevels(size(x, 1))) where {T<:Union{Float32,Float64}}
    n, nb = size(x)
    L <= Util.maxmodwttransformlevels(n) || throw(ArgumentError("Too many transform levels (length(x) < 2^L)"))
    L >= 1 || throw(ArgumentError("L must be >= 1"))
    out = similar(x, n, L + 1, nb)
    q = Vector{Float64}(wt.qmf)
    GC.@preserve out x check(ccall((:wl_modwt_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(out), n, n * (L + 1), pointer(x), n, nb, n, q, length(q), L, stream()))
    return out
end

function imodwt_batch(xw::ROCArray{T,3}, wt::OrthoFilter) where {T<:Union{Float32,Float64}}
    n, nc, nb = size(xw)
    x = similar(xw, n, nb)
    q = Vector{Float64}(wt.qmf)
    GC.@preserve x xw check(ccall((:wl_imodwt_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(x), n, pointer(xw), n, n * nc, n, nc, nb, q, length(q), stream()))
    return x
end

# WaveletsMI355X_modwt_mra.jl -- the MODWT multiresolution analysis, included from WaveletsMI355X.jl:
#   modwt_mra_batch(xw, wt)    xw: len x ncols x B (what modwt_batch returns)  ->  len x ncols x B
#   modwt_mra(xw, wt)          xw: len x ncols     (what modwt returns)        ->  len x ncols
# Column c of a unit of the result is imodwt of that unit with every column but c set to zero: the details D_1 .. D_L in columns
# 1 .. L and the smooth S_L in column L + 1 (L = ncols - 1), aligned with x and adding up to it.  The reference has no such function;
# the result equals (==) that loop of its imodwt for finite input, in one launch for units that fit in LDS and two launches per level
# otherwise (wl_modwt_mra_batch).  tests/test_julia_glue_modwt_mra.py lints every ccall of this file against the ABI.

function modwt_mra_batch(xw::ROCArray{T,3}, wt::OrthoFilter) where {T<:Union{Float32,Float64}}
    n, nc, nb = size(xw)
    out = similar(xw, n, nc, nb)
    q = Vector{Float64}(wt.qmf)
    GC.@preserve out xw check(ccall((:wl_modwt_mra_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(out), n, n * nc, pointer(xw), n, n * nc, n, nc, nb, q, length(q), stream()))
    return out
end

function modwt_mra(xw::ROCMatrix{T}, wt::OrthoFilter) where {T<:Union{Float32,Float64}}
    n, nc = size(xw)
    out = similar(xw, n, nc)
    q = Vector{Float64}(wt.qmf)
    GC.@preserve out xw check(ccall((:wl_modwt_mra_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(out), n, n * nc, pointer(xw), n, n * nc, n, nc, 1, q, length(q), stream()))
    return out
end

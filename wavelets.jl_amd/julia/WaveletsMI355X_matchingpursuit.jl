# WaveletsMI355X_matchingpursuit.jl -- Threshold.matchingpursuit on the device, included from WaveletsMI355X.jl:
#   matchingpursuit(x, wts, tol, nmax=-1; L)    wts: a vector of OrthoFilters, the dictionary is the union of their wavelet bases
#   matchingpursuit(x, f, ft, tol, nmax=-1)     the reference's generic form, f / ft on ROCVectors
#   findmaxabs(v)                               the reference's arg-max-abs (first index of the strictly greatest magnitude), 1-based
# Both forms OVERWRITE x with the residual, as the reference's `r = x` does (basis_functions.jl:11,38); copy x first to keep it.
# Everything but the norm that gates the loop is the reference bit for bit; the norm is T(sqrt(Float64 sum of squares)) in a fixed
# order, about 1 ulp of T from BLAS nrm2.  The reference's `oop` / `N` arguments are not mirrored.
# tests/test_julia_glue_matchingpursuit.py lints every ccall of this file against the ABI.

# idx[1] = findmaxabs(v) - 1 on the device; nothing synchronises
function findmaxabs!(idx::ROCVector{Int64}, v::ROCVector{T}) where {T<:Union{Float32,Float64}}
    GC.@preserve idx v check(ccall((:wl_findmaxabs, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(v), length(v), pointer(idx), stream()))
    return idx
end

function Threshold.findmaxabs(v::ROCVector{T}) where {T<:Union{Float32,Float64}}
    idx = AMDGPU.zeros(Int64, 1)
    findmaxabs!(idx, v)
    return Int(Array(idx)[1]) + 1
end

# nrm(r) after r .-= aphi (aphi === nothing: the norm alone); spat's spike at idx is cleared when spat is as long as r
function mp_residual!(r::ROCVector{T}, aphi::Union{Nothing,ROCVector{T}}, spat::Union{Nothing,ROCVector{T}},
                      idx::ROCVector{Int64}) where {T<:Union{Float32,Float64}}
    nrm = Ref{Float64}(0.0)
    n = length(r)
    if aphi === nothing
        GC.@preserve r check(ccall((:wl_mp_residual, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(r), C_NULL, n, C_NULL, 0, C_NULL, nrm, stream()))
    elseif spat === nothing
        GC.@preserve r aphi check(ccall((:wl_mp_residual, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(r), pointer(aphi), n, C_NULL, 0, C_NULL, nrm, stream()))
    else
        GC.@preserve r aphi spat idx check(ccall((:wl_mp_residual, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(r), pointer(aphi), n, pointer(spat), n, pointer(idx), nrm, stream()))
    end
    return nrm[]
end

function Threshold.matchingpursuit(x::ROCVector{T}, wts::AbstractVector{<:OrthoFilter}, tol::Real, nmax::Int=-1;
                         L=Util.maxtransformlevels(length(x))) where {T<:Union{Float32,Float64}}
    @assert nmax >= -1
    @assert tol > 0
    n, nb = length(x), length(wts)
    y = similar(x, n * nb)
    q = reduce(vcat, [Vector{Float64}(w.qmf) for w in wts]; init=Float64[])
    fl = Int32[length(w.qmf) for w in wts]
    Ls = L isa Integer ? fill(Int32(L), nb) : Vector{Int32}(L)
    length(Ls) == nb || throw(ArgumentError("L must be one integer or one per base"))
    niter, nrm = Ref{Int64}(0), Ref{Float64}(0.0)
    GC.@preserve y x check(ccall((:wl_matchingpursuit_filter, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Cdouble, Int64, Ptr{Int64},
                 Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), n, nb, q, fl, Ls, tol, nmax, niter, nrm, stream()))
    return y
end

function Threshold.matchingpursuit(x::ROCVector{T}, f::Function, ft::Function, tol::Real, nmax::Int=-1) where {T<:Union{Float32,Float64}}
    @assert nmax >= -1
    @assert tol > 0
    r = x
    ftr = ft(r)
    N = length(ftr)
    y = AMDGPU.zeros(T, N)
    spat = AMDGPU.zeros(T, N)
    idx = AMDGPU.zeros(Int64, 1)
    nmax == -1 && (nmax = N)
    nrm = mp_residual!(r, nothing, nothing, idx)
    it = 0
    while nrm > tol && it < nmax
        it > 0 && (ftr = ft(r))
        findmaxabs!(idx, ftr)
        GC.@preserve spat y ftr idx check(ccall((:wl_mp_select, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(spat), N, pointer(y), pointer(ftr), N, pointer(idx), stream()))
        aphi = f(spat)
        if N == length(r)
            nrm = mp_residual!(r, aphi, spat, idx)
        else
            nrm = mp_residual!(r, aphi, nothing, idx)
            fill!(spat, zero(T))
        end
        it += 1
    end
    return y
end

# WaveletsMI355X_wpt2.jl -- the 2-D wavelet packet transform of an image over a quadtree, included from WaveletsMI355X.jl:
#   wpt2(x, filter[, L | tree])   iwpt2(x, filter[, L | tree])          x::ROCMatrix{Float32|Float64}
#   wpt2!(y, x, filter[, L | tree])   iwpt2!(y, x, filter[, L | tree])   out of place: y is not x
#   maketree2(n0, n1, L, s=:full)   isvalidtree2(x, tree)
# The reference has no 2-D packet transform (WPTArray = AbstractVector), so these are plain functions of this module, not methods of
# Transforms.  The node at depth d with block coordinates (bi, bj) is the sub-block of rows bi n0 / 2^d ... and columns
# bj n1 / 2^d ...; splitting it replaces the block by its one-level 2-D dwt, periodic within the block; the quadrants
# [[ss, sd], [ds, dd]] are the children c = ci + 2 cj.  A tree is a Vector{UInt8} or BitVector in breadth-first order: node k
# (0-based) has the children 4k + 1 + c, (4^L - 1) / 3 nodes.  An integer is the full quadtree of that depth, never materialised.
# tests/test_julia_glue_wpt2.py lints every ccall of this file against the ABI.

quadtreesize(L::Integer) = (4^L - 1) ÷ 3

maxtransformlevels2(n0::Integer, n1::Integer) = min(Util.maxtransformlevels(n0), Util.maxtransformlevels(n1))

function maketree2(n0::Integer, n1::Integer, L::Integer=maxtransformlevels2(n0, n1), s::Symbol=:full)
    @assert 0 <= L <= maxtransformlevels2(n0, n1)
    b = zeros(UInt8, quadtreesize(L))
    if s == :full
        fill!(b, 0x01)
    elseif s == :dwt
        for d in 0:L-1
            b[quadtreesize(d) + 1] = 0x01        # child 0 of child 0 of ...: the Mallat pyramid of dwt(x, wt, L)
        end
    else
        throw(ArgumentError("uknown symbol"))
    end
    return b
end

function isvalidtree2(x::AbstractMatrix, tree::AbstractVector)
    n0, n1 = size(x)
    L = 0
    while quadtreesize(L) < length(tree)
        L += 1
    end
    (quadtreesize(L) == length(tree) && n0 % 2^L == 0 && n1 % 2^L == 0) || return false
    for k in 1:length(tree)-1                  # 0-based node k, its parent (k - 1) / 4
        (tree[k + 1] != 0 && tree[(k - 1) ÷ 4 + 1] == 0) && return false
    end
    return true
end

function wpt2_call!(y::ROCMatrix{T}, x::ROCMatrix{T}, filter::OrthoFilter, L::Integer, fw::Bool) where {T<:Union{Float32,Float64}}
    size(x) == size(y) || throw(DimensionMismatch("in and out array size must match"))
    dims = Int64[size(x, 1), size(x, 2)]
    GC.@preserve y x check(ccall((:wl_wpt2_filter_full, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Cint, Cint, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), dims, filter.qmf, length(filter.qmf), L, fw, stream()))
    return y
end

function wpt2_call!(y::ROCMatrix{T}, x::ROCMatrix{T}, filter::OrthoFilter, tree::Union{BitVector,AbstractVector{UInt8},AbstractVector{Bool}},
                    fw::Bool) where {T<:Union{Float32,Float64}}
    size(x) == size(y) || throw(DimensionMismatch("in and out array size must match"))
    isvalidtree2(x, tree) || throw(ArgumentError("invalid tree"))
    dims = Int64[size(x, 1), size(x, 2)]
    t = Vector{UInt8}(tree)
    GC.@preserve y x check(ccall((:wl_wpt2_filter, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), dims, filter.qmf, length(filter.qmf), t, length(t), fw, stream()))
    return y
end

wpt2!(y::ROCMatrix, x::ROCMatrix, filter::OrthoFilter, L_or_tree=maxtransformlevels2(size(x)...)) = wpt2_call!(y, x, filter, L_or_tree, true)
iwpt2!(y::ROCMatrix, x::ROCMatrix, filter::OrthoFilter, L_or_tree=maxtransformlevels2(size(x)...)) = wpt2_call!(y, x, filter, L_or_tree, false)
wpt2(x::ROCMatrix, filter::OrthoFilter, L_or_tree=maxtransformlevels2(size(x)...)) = wpt2_call!(similar(x), x, filter, L_or_tree, true)
iwpt2(x::ROCMatrix, filter::OrthoFilter, L_or_tree=maxtransformlevels2(size(x)...)) = wpt2_call!(similar(x), x, filter, L_or_tree, false)

# WaveletsMI355X_bestbasis_batch.jl -- the best-basis search of a batch of signals and the packet transforms that take one tree
# per signal, included from WaveletsMI355X.jl (after WaveletsMI355X_bestbasis.jl and WaveletsMI355X_wpt_batch.jl, whose entcode
# and wpt_batch_tree it uses):
#   bestbasistree_batch(x, wt[, L | tree][, et])                 x: len x B device matrix, unit i = x[:, i]
#       -> ROCMatrix{UInt8} of size (2^maxtransformlevels(len) - 1, B): column i is bestbasistree(x[:, i], wt, L | tree, et), one
#          byte per node, bit for bit, left in device memory.  One chain of launches over all columns (wl_bestbasistree_filter_batch);
#          nothing synchronises.  L::Integer is maketree(len, L, :full), tree::BitVector ONE input tree shared by all columns.
#   wpt_batch(x, filter, trees) / iwpt_batch(...)                trees::ROCMatrix{UInt8}: column i is the tree of x[:, i]
#   wpt_batch!(y, x, filter, trees) / iwpt_batch!(...)           out of place into y (y must not be x)
#       (wl_wpt_filter_batch_trees).  A device tree is not validated: it counts as its largest valid subtree.  L bounds the depth.
# The reference has none of these.  Lifting schemes have neither the search nor per-unit trees.
# tests/test_julia_glue_bestbasis_batch.py lints every ccall of this file against the ABI.

function bestbasistree_batch(x::ROCMatrix{T}, wt::OrthoFilter, tree::Union{Integer,BitVector}=Util.maxtransformlevels(size(x, 1)),
                             et::Entropy=ShannonEntropy()) where {T<:Union{Float32,Float64}}
    code = entcode(et)
    code === nothing && throw(ArgumentError("bestbasistree_batch takes ShannonEntropy() or LogEnergyEntropy()"))
    n = size(x, 1)
    t, nt, L = wpt_batch_tree(n, tree)
    ntree = 2^Util.maxtransformlevels(n) - 1
    trees = ROCMatrix{UInt8}(undef, ntree, size(x, 2))
    q = Vector{Float64}(wt.qmf)
    GC.@preserve x t trees check(ccall((:wl_bestbasistree_filter_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid}, Int64,
                 Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                ctx(), DT[T], pointer(x), n, size(x, 2), n, q, length(q), nt == 0 ? Ptr{UInt8}(C_NULL) : pointer(t), nt, L, code,
                pointer(trees), ntree, C_NULL, 0, stream()))
    return trees
end

for (f, fw) in ((:wpt_batch!, true), (:iwpt_batch!, false))
    @eval function $f(y::ROCMatrix{T}, x::ROCMatrix{T}, filter::OrthoFilter, trees::ROCMatrix{UInt8},
                      L::Integer=Util.maxtransformlevels(size(x, 1))) where {T<:Union{Float32,Float64}}
        size(x) == size(y) || throw(DimensionMismatch("in and out array size must match"))
        pointer(y) == pointer(x) && throw(ArgumentError("in array is out array"))
        n = size(x, 1)
        size(trees) == (2^Util.maxtransformlevels(n) - 1, size(x, 2)) || throw(DimensionMismatch("trees must be (2^maxtransformlevels(n) - 1) x B"))
        0 <= L <= Util.maxtransformlevels(n) || throw(AssertionError("0 <= L <= maxtransformlevels(n)"))
        q = Vector{Float64}(filter.qmf)
        GC.@preserve y x trees check(ccall((:wl_wpt_filter_batch_trees, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}),
                    ctx(), DT[T], pointer(y), pointer(x), n, size(x, 2), n, q, length(q), pointer(trees), size(trees, 1), Cint(L), $fw,
                    stream()))
        return y
    end
end

for (f, fb) in ((:wpt_batch, :wpt_batch!), (:iwpt_batch, :iwpt_batch!))
    @eval function $f(x::ROCMatrix{T}, filter::OrthoFilter, trees::ROCMatrix{UInt8},
                      L::Integer=Util.maxtransformlevels(size(x, 1))) where {T<:Union{Float32,Float64}}
        return $fb(similar(x), x, filter, trees, L)
    end
end

# WaveletsMI355X_wpt_batch.jl -- the packet transform of a batch of signals that share one tree, included from WaveletsMI355X.jl:
#   wpt_batch(x, wt[, L | tree]) / iwpt_batch(...)            x: len x B device matrix, unit i = x[:, i]
#   wpt_batch!(y, x, filter[, L | tree]) / iwpt_batch!(...)   out of place into y (y must not be x)
#   wpt_batch!(y, scheme[, L | tree]) / iwpt_batch!(...)      in place on every column of y
# The reference has no batched form: wpt_batch(x, wt, tree) equals the loop of `wpt(x[:, i], wt, tree)` over the columns, bit for
# bit, in one chain of launches over all columns (wl_wpt_filter_batch / wl_wpt_lifting_batch).  L::Integer is the full tree of
# that depth (never materialised), tree::BitVector the reference's node vector of 2^maxtransformlevels(len) - 1 bits.
# tests/test_julia_glue_wpt_batch.py lints every ccall of this file against the ABI.

# (tree pointer, node count, depth) as the C entry points take them; the reference's errors for a bad depth / a bad tree
function wpt_batch_tree(n::Integer, L::Integer)
    0 <= L <= Util.maxtransformlevels(n) || throw(AssertionError("0 <= L <= maxtransformlevels(n)"))   # maketree's @assert
    return UInt8[], Int64(0), Cint(L)
end
function wpt_batch_tree(n::Integer, tree::BitVector)
    Util.isvalidtree(zeros(n), tree) || throw(ArgumentError("invalid tree"))
    return UInt8.(tree), Int64(length(tree)), Cint(0)
end

for (f, fw) in ((:wpt_batch!, true), (:iwpt_batch!, false))
    @eval function $f(y::ROCMatrix{T}, x::ROCMatrix{T}, filter::OrthoFilter,
                      tree::Union{Integer,BitVector}=Util.maxtransformlevels(size(x, 1))) where {T<:Union{Float32,Float64}}
        size(x) == size(y) || throw(DimensionMismatch("in and out array size must match"))
        pointer(y) == pointer(x) && throw(ArgumentError("in array is out array"))
        t, nt, L = wpt_batch_tree(size(x, 1), tree)
        q = Vector{Float64}(filter.qmf)
        GC.@preserve y x t check(ccall((:wl_wpt_filter_batch, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid}),
                    ctx(), DT[T], pointer(y), pointer(x), size(x, 1), size(x, 2), size(x, 1), q, length(q),
                    nt == 0 ? Ptr{UInt8}(C_NULL) : pointer(t), nt, L, $fw, stream()))
        return y
    end
    @eval function $f(y::ROCMatrix{T}, scheme::GLS,
                      tree::Union{Integer,BitVector}=Util.maxtransformlevels(size(y, 1))) where {T<:Union{Float32,Float64}}
        return wpt_lifting_batch_device!(y, y, scheme, tree, $fw)
    end
end

# y === x: wpt!(y[:, i], scheme, tree) of every column in place; otherwise x stays untouched (the first pass reads it)
function wpt_lifting_batch_device!(y::ROCMatrix{T}, x::ROCMatrix{T}, scheme::GLS, tree::Union{Integer,BitVector}, fw::Bool) where {T<:Union{Float32,Float64}}
    size(x) == size(y) || throw(DimensionMismatch("in and out array size must match"))
    t, nt, L = wpt_batch_tree(size(x, 1), tree)
    isup, nc, sh, cf = flatten(scheme)
    GC.@preserve y x t check(ccall((:wl_wpt_lifting_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                 Cdouble, Cdouble, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), size(x, 1), size(x, 2), size(x, 1), length(isup), isup, nc, sh, cf,
                scheme.norm1, scheme.norm2, nt == 0 ? Ptr{UInt8}(C_NULL) : pointer(t), nt, L, fw, stream()))
    return y
end

for (f, fb, fw) in ((:wpt_batch, :wpt_batch!, true), (:iwpt_batch, :iwpt_batch!, false))
    @eval function $f(x::ROCMatrix{T}, filter::OrthoFilter,
                      tree::Union{Integer,BitVector}=Util.maxtransformlevels(size(x, 1))) where {T<:Union{Float32,Float64}}
        return $fb(similar(x), x, filter, tree)
    end
    @eval function $f(x::ROCMatrix{T}, scheme::GLS,
                      tree::Union{Integer,BitVector}=Util.maxtransformlevels(size(x, 1))) where {T<:Union{Float32,Float64}}
        return wpt_lifting_batch_device!(similar(x), x, scheme, tree, $fw)
    end
end

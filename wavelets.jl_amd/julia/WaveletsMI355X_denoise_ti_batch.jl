# WaveletsMI355X_denoise_ti_batch.jl -- translation-invariant denoise of a batch of independent units on the device, included from
# WaveletsMI355X.jl after WaveletsMI355X_denoise_batch.jl (batch_units, batch_sigma and BATCH_TH are defined there):
#   denoise_ti_batch(x, wt; L, dnt, nspin, sigma, return_sigma)   x: len x B signals, n x n x B square images or n x n x n x B cubes
# The reference has no batched form: denoise_ti_batch(x, wt; nspin) equals the loop of `denoise(x[.., i], wt; TI=true, nspin)` over
# the units, bit for bit, but every unit's sigma = noisest(x_i, wt) is estimated from the unshifted unit and applied on the device,
# and the shifted copies of all units run as batches (wl_denoise_ti_batch_filter / wl_denoise_ti_batch_lifting: per group of planes
# one shift, one forward batch, one threshold, one inverse batch and one un-shift / accumulate launch, no host round trip).
# nspin: 8 per unit dimension by default; signals take an Int or any tuple (its product is the number of spins), images and cubes
# one entry per unit dimension.  Not part of these calls: wt = nothing and BiggestTH / PosTH / NegTH.
# tests/test_julia_glue_denoise_ti_batch.py lints every ccall of this file against the ABI.

# the spins of a unit of N - 1 dimensions, padded to three entries
function batch_nspin(nspin::Union{Int,Tuple}, nd::Int)
    nspt = nspin isa Int ? (nspin,) : nspin
    nd == 1 && (nspt = (prod(nspt),))                       # vectors: prod(nspin) spins shifted by 0 .. pns-1 (denoising.jl:38-42)
    length(nspt) == nd || throw(ArgumentError("nspin must have one entry per unit dimension"))
    all(>=(1), nspt) || throw(ArgumentError("nspin must be positive"))
    return Int64[nspt..., ones(Int, 3 - nd)...]
end

function denoise_ti_batch(x::ROCArray{T,N}, wt::OrthoFilter=Threshold.DEFAULT_WAVELET;
                          L::Int=min(Util.maxtransformlevels(size(x, 1)), 6), dnt::VisuShrink{<:BATCH_TH}=VisuShrink(size(x, 1)),
                          nspin::Union{Int,Tuple}=ntuple(_ -> 8, N - 1),
                          sigma::Union{Nothing,AbstractVector{<:Real}}=nothing, return_sigma::Bool=false) where {T<:Union{Float32,Float64},N}
    dims, nb, nunit = batch_units(x)
    nsp = batch_nspin(nspin, N - 1)
    sg = batch_sigma(sigma, nb)
    sout = ROCVector{Float64}(undef, nb)
    sig_in = sg === nothing ? sout : sg
    y = similar(x)
    q = Vector{Float64}(wt.qmf)
    GC.@preserve y x sig_in sout check(ccall((:wl_denoise_ti_batch_filter, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Int64, Ptr{Float64}, Cint, Cint, Cint, Cdouble,
                 Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), Cint(N - 1), dims, nb, nunit, q, length(q), L, THCODE[typeof(dnt.th)], Float64(dnt.t),
                nsp, sg === nothing ? Ptr{Float64}(C_NULL) : pointer(sig_in), pointer(sout), stream()))
    return return_sigma ? (y, sout) : y
end

function denoise_ti_batch(x::ROCArray{T,N}, wt::GLS;
                          L::Int=min(Util.maxtransformlevels(size(x, 1)), 6), dnt::VisuShrink{<:BATCH_TH}=VisuShrink(size(x, 1)),
                          nspin::Union{Int,Tuple}=ntuple(_ -> 8, N - 1),
                          sigma::Union{Nothing,AbstractVector{<:Real}}=nothing, return_sigma::Bool=false) where {T<:Union{Float32,Float64},N}
    dims, nb, nunit = batch_units(x)
    nsp = batch_nspin(nspin, N - 1)
    sg = batch_sigma(sigma, nb)
    sout = ROCVector{Float64}(undef, nb)
    sig_in = sg === nothing ? sout : sg
    y = similar(x)
    isup, nc, sh, cf = flatten(wt)
    GC.@preserve y x sig_in sout check(ccall((:wl_denoise_ti_batch_lifting, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
                 Cdouble, Cdouble, Cint, Cint, Cdouble, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                ctx(), DT[T], pointer(y), pointer(x), Cint(N - 1), dims, nb, nunit, length(isup), isup, nc, sh, cf, Float64(wt.norm1),
                Float64(wt.norm2), L, THCODE[typeof(dnt.th)], Float64(dnt.t), nsp,
                sg === nothing ? Ptr{Float64}(C_NULL) : pointer(sig_in), pointer(sout), stream()))
    return return_sigma ? (y, sout) : y
end

# Batched block Jacobi and ensemble balanced truncation (included by DREHip.jl, inside module DREHip; dre_version >= 111).
# Members of one shape share every launch; a member's result is bit for bit the single call's, and a failed member is a DREError in its slot.

member_error(ctx::Context, b::Integer) =
    unsafe_string(ccall((:dre_batch_member_error, LIB), Cstring, (Ptr{Cvoid}, Cint), ctx.ptr, b))

# per member: f(b) for status 0, the member's DREError otherwise (b counts from 1)
batch_results(f, ctx::Context, status::Vector{Int32}) =
    Any[status[b] == 0 ? f(b) : DREError(status[b], member_error(ctx, b - 1)) for b in eachindex(status)]

"eigen-decompositions of symmetric matrices of one order in shared launches (dre_sym_eig_jacobi_batched): a vector of (w, V), w ascending, or the member's DREError; stats = true adds (sweeps, rounds)."
function sym_eigh_batch(As::AbstractVector{<:AbstractMatrix}; tol::Float64=0.0, stats::Bool=false, ctx::Context=default_context())
    nb = length(As)
    nb >= 1 || throw(ArgumentError("sym_eigh_batch: empty batch"))
    all(size(A) == size(As[1]) && size(A, 1) == size(A, 2) for A in As) || throw(ArgumentError("sym_eigh_batch: square matrices of one order expected"))
    d = [upload(ctx, Matrix{Float64}(A)) for A in As]
    h = Ptr{Cvoid}[x.ptr for x in d]
    w, V = fill(C_NULL, nb), fill(C_NULL, nb)
    ii, status = zeros(Int64, 2nb), zeros(Int32, nb)
    GC.@preserve d chk(ctx, ccall((:dre_sym_eig_jacobi_batched, LIB), Cint,
                                  (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Cdouble, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int32}),
                                  ctx.ptr, nb, h, tol, w, V, ii, status))
    batch_results(ctx, status) do b
        out = (vec(download(ctx, w[b])), download(ctx, V[b]))
        stats ? (out..., (sweeps = ii[2b - 1], rounds = ii[2b])) : out
    end
end

"svd(A_b) of matrices of one shape in shared launches (dre_svd_jacobi_batched): a vector of (U, s, V) or the member's DREError; stats = true adds (sweeps, rounds, rank)."
function svd_jacobi_batch(As::AbstractVector{<:AbstractMatrix}; tol::Float64=0.0, stats::Bool=false, ctx::Context=default_context())
    nb = length(As)
    nb >= 1 || throw(ArgumentError("svd_jacobi_batch: empty batch"))
    all(size(A) == size(As[1]) for A in As) || throw(ArgumentError("svd_jacobi_batch: matrices of one shape expected"))
    d = [upload(ctx, Matrix{Float64}(A)) for A in As]
    h = Ptr{Cvoid}[x.ptr for x in d]
    U, S, V = fill(C_NULL, nb), fill(C_NULL, nb), fill(C_NULL, nb)
    ii, status = zeros(Int64, 3nb), zeros(Int32, nb)
    GC.@preserve d chk(ctx, ccall((:dre_svd_jacobi_batched, LIB), Cint,
                                  (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Cdouble, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int32}),
                                  ctx.ptr, nb, h, tol, U, S, V, ii, status))
    batch_results(ctx, status) do b
        out = (download(ctx, U[b]), vec(download(ctx, S[b])), download(ctx, V[b]))
        stats ? (out..., (sweeps = ii[3b - 2], rounds = ii[3b - 1], rank = ii[3b])) : out
    end
end

"""Square-root balanced truncation of an ensemble from factored Gramians (dre_balance_lr_batched): `systems` is a vector of
(E, A, B, C, Lc, Dc, Lo, Do) with one (n, m, q); the Gramian factors' ranks may differ.  One batched SVD over the zero-padded stack of the
Z_o'E Z_c; a member's result depends on the other members only through the padded shape.  A vector of ReducedModel or the member's DREError."""
function balance_lr_batch(systems::AbstractVector; order::Int=0, tol::Float64=1e-8, ctx::Context=default_context())
    nb = length(systems)
    nb >= 1 || throw(ArgumentError("balance_lr_batch: empty batch"))
    all(length(s) == 8 for s in systems) || throw(ArgumentError("balance_lr_batch: every member is (E, A, B, C, Lc, Dc, Lo, Do)"))
    d = [[upload(ctx, Matrix{Float64}(reshape(M, size(M, 1), :))) for M in s] for s in systems]
    h = [Ptr{Cvoid}[d[b][j].ptr for b in 1:nb] for j in 1:8]
    o = [fill(C_NULL, nb) for _ in 1:6]
    ii, dd, status = zeros(Int64, 6nb), zeros(3nb), zeros(Int32, nb)
    GC.@preserve d chk(ctx, ccall((:dre_balance_lr_batched, LIB), Cint,
                                  (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
                                   Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Cdouble, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
                                   Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
                                  ctx.ptr, nb, h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], order, tol, o[1], o[2], o[3], o[4], o[5], o[6], ii, dd,
                                  status))
    batch_results(ctx, status) do b
        hsv, T, W, Ar, Br, Cr = (download(ctx, r[b]) for r in o)
        i, x = ii[6b - 5:6b], dd[3b - 2:3b]
        ReducedModel(Ar, Br, Cr, vec(hsv), T, W,
                     (order = i[1], rank = i[2], r_c = i[3], r_o = i[4], dropped = i[5], svd_sweeps = i[6], eye_err = x[1], bound = x[2], neg_max = x[3]))
    end
end

export sym_eigh_batch, svd_jacobi_batch, balance_lr_batch

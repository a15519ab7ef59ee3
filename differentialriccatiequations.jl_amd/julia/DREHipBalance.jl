# Device SVD and square-root balanced truncation (included by DREHip.jl, inside module DREHip; dre_version >= 110).

"svd(A) on the device by one-sided block Jacobi (dre_svd_jacobi): (U, s, V) with A ≈ U diag(s) V', s descending; norm-wise accuracy (errors of order eps s[1]).  tol = 0: sqrt(max(m, w)) eps; stats = true adds (sweeps, rounds, rank)."
function svd_jacobi(A::AbstractMatrix; tol::Float64=0.0, stats::Bool=false, ctx::Context=default_context())
    Ad = upload(ctx, Matrix{Float64}(A))
    U, S, V = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    ii = zeros(Int64, 3)
    chk(ctx, ccall((:dre_svd_jacobi, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ptr{Int64}),
                   ctx.ptr, Ad.ptr, tol, U, S, V, ii))
    out = (download(ctx, U[]), vec(download(ctx, S[])), download(ctx, V[]))
    stats ? (out..., (sweeps = ii[1], rounds = ii[2], rank = ii[3])) : out
end

"The balanced truncation of E ẋ = A x + B u, y = C x: ẋ_r = Ar x_r + Br u, y = Cr x_r (Er = I); hsv the Hankel singular values, W'E T = I"
struct ReducedModel
    Ar::Matrix{Float64}; Br::Matrix{Float64}; Cr::Matrix{Float64}
    hsv::Vector{Float64}; T::Matrix{Float64}; W::Matrix{Float64}
    info::NamedTuple
end

"""Square-root balanced truncation on the device (dre_balance_lr) from ONE sign factorisation of (A, E) and two factored replays: the
observability Gramian from C'C (primal) and the controllability Gramian from B B' (dual).  order = 0: the smallest r with
2 Σ_{i>r} σ_i <= tol σ_1; an order above the numerical rank of Z_o'E Z_c is DREError(-1)."""
function balanced_truncation(E, A, B::AbstractMatrix, C::AbstractMatrix; alg::FactoredSign=FactoredSign(), order::Int=0, tol::Float64=1e-8,
                             ctx::Context=default_context())
    n = size(E, 1)
    (size(E) == (n, n) && size(A) == (n, n) && size(B, 1) == n && size(C, 2) == n) ||
        throw(ArgumentError("balanced_truncation: E and A must be n x n, B n x m and C q x n"))
    order >= 0 || throw(ArgumentError("balanced_truncation: order must be positive (0: chosen by tol)"))
    Eh, Ah = dense_operator(E), dense_operator(A)
    s = SignFactorization(ctx, Eh, Ah; maxiters = alg.maxiters, tol = alg.tol)
    Lo, Do, ip = solve_lr(s, Matrix{Float64}(C'), Matrix{Float64}(I, size(C, 1), size(C, 1)); rtol = alg.rtol, max_width = alg.max_width, max_refine = alg.max_refine)
    Lc, Dc, id = solve_lr_t(s, Matrix{Float64}(B), Matrix{Float64}(I, size(B, 2), size(B, 2)); rtol = alg.rtol, max_width = alg.max_width, max_refine = alg.max_refine)
    finalize(s)
    d = [upload(ctx, Matrix{Float64}(M)) for M in (Eh, Ah, B, C, Lc, Dc, Lo, Do)]
    o = [Ref{Ptr{Cvoid}}(C_NULL) for _ in 1:6]
    ii, dd = zeros(Int64, 6), zeros(3)
    chk(ctx, ccall((:dre_balance_lr, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble,
                    Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, d[7].ptr, d[8].ptr, order, tol,
                   o[1], o[2], o[3], o[4], o[5], o[6], ii, dd))
    hsv, T, W, Ar, Br, Cr = (download(ctx, r[]) for r in o)
    ReducedModel(Ar, Br, Cr, vec(hsv), T, W,
                 (primal = ip, dual = id, factorizations = 1, order = ii[1], rank = ii[2], r_c = ii[3], r_o = ii[4], dropped = ii[5], svd_sweeps = ii[6],
                  eye_err = dd[1], bound = dd[2], neg_max = dd[3]))
end

export svd_jacobi, balanced_truncation, ReducedModel

# LQG balanced truncation from one Hamiltonian sign iteration (included by DREHip.jl, inside module DREHip; dre_version >= 113).
# Both Riccati solutions of LQG design come from dre_dense_gare_solve_pair; dre_lqg_balance balances them and adds the reduced-order controller.

"""Both Riccati equations of LQG design from ONE sign iteration of the Hamiltonian pencil (dre_dense_gare_solve_pair): (X, Y, info) with
A'XE + E'XA - E'XGXE + Q = 0 (regulator) and A Y E' + E Y A' - E Y Q Y E' + G = 0 (filter), G = B Rinv B', Q = C'S C (nothing: identity).
X is bit for bit the X of `solve(DenseGAREProblem(...), MatrixSign())`."""
function solve_gare_pair(E, A, B::AbstractMatrix, C::AbstractMatrix; alg::MatrixSign=MatrixSign(), Rinv=nothing, S=nothing, ctx::Context=default_context())
    n = size(E, 1)
    (size(E) == (n, n) && size(A) == (n, n) && size(B, 1) == n && size(C, 2) == n) ||
        throw(ArgumentError("solve_gare_pair: E and A must be n x n, B n x m and C q x n"))
    d = Any[upload(ctx, Matrix{Float64}(M)) for M in (dense_operator(E), dense_operator(A), B, C')]
    push!(d, Rinv === nothing ? nothing : upload(ctx, Matrix{Float64}(Rinv)), S === nothing ? nothing : upload(ctx, Matrix{Float64}(S)))
    p = o -> o === nothing ? C_NULL : o.ptr
    X, Y = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 4), zeros(4)
    GC.@preserve d chk(ctx, ccall((:dre_dense_gare_solve_pair, LIB), Cint,
                                  (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cint, Ref{Ptr{Cvoid}},
                                   Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                                  ctx.ptr, p(d[1]), p(d[2]), p(d[3]), p(d[5]), p(d[4]), p(d[6]), alg.maxiters, alg.tol, alg.max_refine, X, Y, ii, dd))
    (download(ctx, X[]), download(ctx, Y[]),
     (iters = ii[1], factorizations = 1, regulator = (refinements = ii[2], res0 = dd[1], res = dd[2]), filter = (refinements = ii[4], res0 = dd[3], res = dd[4])))
end

"""The LQG balanced truncation of E ẋ = A x + B u, y = C x: ẋ_r = Ar x_r + Br u, y = Cr x_r (Er = I); mu the LQG characteristic values,
W'E T = I; the reduced-order LQG controller ẋ_c = Ac x_c + Lr y, u = -Kr x_c; K = B'XE the full-order feedback"""
struct LQGReducedModel
    Ar::Matrix{Float64}; Br::Matrix{Float64}; Cr::Matrix{Float64}
    mu::Vector{Float64}; T::Matrix{Float64}; W::Matrix{Float64}
    Kr::Matrix{Float64}; Lr::Matrix{Float64}; Ac::Matrix{Float64}; K::Matrix{Float64}
    info::NamedTuple
end

"(Ac, Lr, Kr) of ẋ_c = Ac x_c + Lr y, u = -Kr x_c"
controller(rom::LQGReducedModel) = (rom.Ac, rom.Lr, rom.Kr)

"""LQG balanced truncation on the device (dre_dense_gare_solve_pair, dre_lqg_balance); the pencil (A, E) need not be c-stable.  order = 0: the
smallest r with 2 Σ_{i>r} ν_i <= tol, ν_i = μ_i / sqrt(1 + μ_i²); an order above the numerical rank is DREError(-1)."""
function lqg_balanced_truncation(E, A, B::AbstractMatrix, C::AbstractMatrix; alg::MatrixSign=MatrixSign(), order::Int=0, tol::Float64=1e-8,
                                 ctx::Context=default_context())
    order >= 0 || throw(ArgumentError("lqg_balanced_truncation: order must be positive (0: chosen by tol)"))
    Eh, Ah = dense_operator(E), dense_operator(A)
    X, Y, pair = solve_gare_pair(Eh, Ah, B, C; alg = alg, ctx = ctx)
    d = [upload(ctx, Matrix{Float64}(M)) for M in (Eh, Ah, B, C, X, Y)]
    o = [Ref{Ptr{Cvoid}}(C_NULL) for _ in 1:9]
    ii, dd = zeros(Int64, 6), zeros(3)
    GC.@preserve d chk(ctx, ccall((:dre_lqg_balance, LIB), Cint,
                                  (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble,
                                   Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}},
                                   Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                                  ctx.ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, order, tol,
                                  o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], ii, dd))
    mu, T, W, Ar, Br, Cr, Kr, Lr, Ac = (download(ctx, r[]) for r in o)
    LQGReducedModel(Ar, Br, Cr, vec(mu), T, W, Kr, Lr, Ac, Matrix{Float64}(B' * X * Eh),
                    (pair..., order = ii[1], rank = ii[2], r_c = ii[3], r_o = ii[4], dropped = ii[5], svd_sweeps = ii[6], eye_err = dd[1], bound = dd[2],
                     neg_max = dd[3]))
end

"the LQG characteristic values, descending"
lqg_characteristic_values(E, A, B, C; kw...) = lqg_balanced_truncation(E, A, B, C; order = 0, tol = 0.0, kw...).mu

"H_r(iω) of an LQGReducedModel (E_r = I)"
freq_response(rom::LQGReducedModel, omega::AbstractVector{<:Real}; kw...) =
    freq_response(Matrix{Float64}(I, size(rom.Ar)...), rom.Ar, rom.Br, rom.Cr, omega; kw...)

"""(err, bound): err = max_k ‖[N; M](iω_k) - [N_r; M_r](iω_k)‖₂ of the normalised right coprime factors, from two freq_response calls on
(E, A - B K, B, [C; -K]) and (I, Ar - Br Kr, Br, [Cr; -Kr]) with D = [0; I]; bound = 2 Σ_{i>r} μ_i / sqrt(1 + μ_i²)"""
function lqg_error(E, A, B, C, rom::LQGReducedModel, omega::AbstractVector{<:Real}; ctx::Context=default_context())
    m, q, r = size(B, 2), size(C, 1), size(rom.Ar, 1)
    D = [zeros(q, m); Matrix{Float64}(I, m, m)]
    H, _, _ = freq_response(dense_operator(E), dense_operator(A) - B * rom.K, B, [C; -rom.K], omega; D = D, ctx = ctx)
    Hr, _, _ = freq_response(Matrix{Float64}(I, r, r), rom.Ar - rom.Br * rom.Kr, rom.Br, [rom.Cr; -rom.Kr], omega; D = D, ctx = ctx)
    err = maximum(opnorm(H[:, :, k] - Hr[:, :, k]) for k in eachindex(omega))
    mu = rom.mu[r + 1:end]
    (err, 2 * sum(reverse(mu ./ sqrt.(1 .+ mu .^ 2))))
end

export solve_gare_pair, LQGReducedModel, controller, lqg_balanced_truncation, lqg_characteristic_values, lqg_error

# Dense generalized Sylvester solver by the coupled sign iteration, and the H2 tools on it (included by DREHip.jl, inside module DREHip;
# dre_version >= 119, csrc/dense_sylvester.hip, DESIGN.md 9.15).  These wrappers are UNRUN: no Julia was available where they were written.

"A X F + E X B = -C, all dense (A, E n x n; B, F m x m; C n x m); `E = nothing` or `F = nothing` is the identity.  Both pencils must be c-stable."
struct DenseGSYLEProblem; E; A; F; B; C; end

optional_ptr(ctx::Context, M) = M === nothing ? (nothing, C_NULL) : (d = upload(ctx, Matrix{Float64}(M)); (d, d.ptr))

"solve(DenseGSYLEProblem, MatrixSign()): (X, info); `transposed = true` solves A'X F' + E'X B' = -C.  DREError(-7) names the pencil that is not c-stable."
function CommonSolve.solve(prob::DenseGSYLEProblem, alg::MatrixSign; transposed::Bool=false, ctx::Context=default_context())
    (Ed, pE), (Fd, pF) = optional_ptr(ctx, prob.E), optional_ptr(ctx, prob.F)
    ops = [upload(ctx, Matrix{Float64}(M)) for M in (prob.A, prob.B, prob.C)]
    X = Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 2), zeros(3)
    GC.@preserve Ed Fd ops chk(ctx, ccall((:dre_dense_sylvester_solve, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cdouble, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, pE, ops[1].ptr, pF, ops[2].ptr, ops[3].ptr, transposed ? 1 : 0, alg.maxiters, alg.tol, alg.max_refine, X, ii, dd))
    download(ctx, X[]), (iters = ii[1], refinements = ii[2], res0 = dd[1], res = dd[2], step = dd[3])
end

"residual(::DenseGSYLEProblem, X): (C + A X F + E X B, its Frobenius norm, the scaled norm ||Res|| / (||C|| + ||AXF|| + ||EXB||))"
function residual(prob::DenseGSYLEProblem, X::AbstractMatrix; transposed::Bool=false, ctx::Context=default_context())
    (Ed, pE), (Fd, pF) = optional_ptr(ctx, prob.E), optional_ptr(ctx, prob.F)
    ops = [upload(ctx, Matrix{Float64}(M)) for M in (prob.A, prob.B, prob.C, X)]
    R, nrm, sc = Ref{Ptr{Cvoid}}(C_NULL), Ref{Cdouble}(0.0), Ref{Cdouble}(0.0)
    GC.@preserve Ed Fd ops chk(ctx, ccall((:dre_dense_sylvester_residual, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}, Ref{Cdouble}, Ref{Cdouble}),
                   ctx.ptr, pE, ops[1].ptr, pF, ops[2].ptr, ops[3].ptr, ops[4].ptr, transposed ? 1 : 0, R, nrm, sc))
    download(ctx, R[]), nrm[], sc[]
end

"A kept coupled sign iteration of the pencils (A, E) and (B, F) on the device (dre_sylvester_create): every right-hand side, in either direction, costs a replay only"
mutable struct SylvesterFactorization
    ctx::Context
    ptr::Ptr{Cvoid}
    n::Int
    m::Int
    iters::Int
end
function SylvesterFactorization(ctx::Context, E, A, F, B; maxiters::Int=50, tol::Float64=0.0)
    (Ed, pE), (Fd, pF) = optional_ptr(ctx, E), optional_ptr(ctx, F)
    Ad, Bd = upload(ctx, dense_operator(A)), upload(ctx, dense_operator(B))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Ed Fd chk(ctx, ccall((:dre_sylvester_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Ref{Ptr{Cvoid}}),
                                      ctx.ptr, pE, Ad.ptr, pF, Bd.ptr, maxiters, tol, h))
    it = Ref{Int64}(0)
    ccall((:dre_sylvester_iters, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), h[], it)
    s = SylvesterFactorization(ctx, h[], size(A, 1), size(B, 1), it[])
    finalizer(x -> ccall((:dre_sylvester_destroy, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.ptr, x.ptr), s)
end

"A X F + E X B = -C on a kept factorisation: (X, info); transposed = true: A'X F' + E'X B' = -C from the same factorisation"
function solve_dense(s::SylvesterFactorization, C::AbstractMatrix; max_refine::Int=2, transposed::Bool=false)
    ctx = s.ctx
    Cd = upload(ctx, Matrix{Float64}(C))
    X = Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 2), zeros(3)
    chk(ctx, ccall((:dre_sylvester_solve, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, s.ptr, Cd.ptr, transposed ? 1 : 0, max_refine, X, ii, dd))
    download(ctx, X[]), (iters = ii[1], refinements = ii[2], res0 = dd[1], res = dd[2], step = dd[3])
end

# The H2 formulas cancel, so each trace gets a first-order correction: the solution's residual is replayed once through the kept sequence and
# its trace added (the solver's own rule stops refining at a relative residual of 100 n eps).

"||H||_H2^2 = tr(C P C') with A P E' + E P A' = -B B': one sign factorisation on the Lyapunov path, the dual replay of B B' and of the residual"
function h2_norm2(E, A, B, C; alg::MatrixSign=MatrixSign(), ctx::Context=default_context())
    R = Matrix{Float64}(B) * Matrix{Float64}(B)'
    s = SignFactorization(ctx, E, A; maxiters = alg.maxiters, tol = alg.tol)
    P, _ = solve_dense(s, R; max_refine = alg.max_refine, transposed = true)
    Res, _, _ = residual(DenseGSYLEProblem(E, A, Matrix{Float64}(E'), Matrix{Float64}(A'), R), P; ctx = ctx)
    dP, _ = solve_dense(s, Res; max_refine = 0, transposed = true)
    finalize(s)
    tr(C * P * C') + tr(C * dP * C')
end
"||H||_H2 = sqrt(tr(C P C'))"
h2_norm(E, A, B, C; kw...) = sqrt(max(h2_norm2(E, A, B, C; kw...), 0.0))

"<H1, H2> = tr(C1 X C2') with A1 X E2' + E1 X A2' = -B1 B2' for two systems (E, A, B, C): one Sylvester factorisation with the right pencil (A2', E2')"
function h2_inner(sys1, sys2; alg::MatrixSign=MatrixSign(), ctx::Context=default_context())
    (E1, A1, B1, C1), (E2, A2, B2, C2) = sys1, sys2
    F, Bt, R = Matrix{Float64}(E2'), Matrix{Float64}(A2'), Matrix{Float64}(B1) * Matrix{Float64}(B2)'
    s = SylvesterFactorization(ctx, E1, A1, F, Bt; maxiters = alg.maxiters, tol = alg.tol)
    X, _ = solve_dense(s, R; max_refine = alg.max_refine)
    Res, _, _ = residual(DenseGSYLEProblem(E1, A1, F, Bt, R), X; ctx = ctx)
    dX, _ = solve_dense(s, Res; max_refine = 0)
    finalize(s)
    tr(C1 * X * C2') + tr(C1 * dX * C2')
end

"""||H - H_r||_H2 by err² = ||H||² - 2 <H, H_r> + ||H_r||²: (err, info) with info = (err2, norm2, norm2_r, inner, floor).  The formula cancels:
floor = eps (||H||² + ||H_r||²) is its accuracy level, err = sqrt(max(err2, 0)).  `rom`: a ReducedModel (Er = I) or a tuple (Er, Ar, Br, Cr)."""
function h2_error(E, A, B, C, rom; alg::MatrixSign=MatrixSign(), ctx::Context=default_context())
    rsys = rom isa Tuple ? rom : (Matrix{Float64}(I, size(rom.Ar, 1), size(rom.Ar, 1)), rom.Ar, rom.Br, rom.Cr)
    norm2, norm2_r = h2_norm2(E, A, B, C; alg = alg, ctx = ctx), h2_norm2(rsys...; alg = alg, ctx = ctx)
    inner = h2_inner((E, A, B, C), rsys; alg = alg, ctx = ctx)
    err2 = norm2 - 2 * inner + norm2_r
    sqrt(max(err2, 0.0)), (err2 = err2, norm2 = norm2, norm2_r = norm2_r, inner = inner, floor = eps() * (norm2 + norm2_r))
end

export DenseGSYLEProblem, SylvesterFactorization, h2_norm, h2_inner, h2_error

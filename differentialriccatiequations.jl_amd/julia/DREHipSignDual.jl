# Dual solves on a kept sign factorisation (included by DREHip.jl, inside module DREHip): F Y E' + E Y F' = -R from the SignFactorization of
# (F, E), without a second factorisation of (F', E').  Reached through solve_dense(s, R; transposed = true) and solve_lr(s, G, S; transposed = true).

"F Y E' + E Y F' = -R for a dense symmetric R on the kept factorisation of (F, E): (Y, info)"
function solve_dense_t(s::SignFactorization, R::AbstractMatrix; max_refine::Int=2)
    ctx = s.ctx
    Rd = upload(ctx, Matrix{Float64}(R))
    Y = Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 2), zeros(2)
    chk(ctx, ccall((:dre_sign_solve_dense_t, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, s.ptr, Rd.ptr, max_refine, Y, ii, dd))
    download(ctx, Y[]), (iters = ii[1], refinements = ii[2], res0 = dd[1], res = dd[2])
end

"F Y E' + E Y F' = -G S G' on the kept factorisation of (F, E): (L, D, info) with Y = L D L', D diagonal"
function solve_lr_t(s::SignFactorization, G::AbstractMatrix, S::AbstractMatrix; rtol::Float64=0.0, max_width::Int=256, max_refine::Int=1)
    ctx = s.ctx
    Gd, Sd = upload(ctx, Matrix{Float64}(G)), upload(ctx, Matrix{Float64}(S))
    L, D = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 4), zeros(2)
    chk(ctx, ccall((:dre_sign_solve_lr_t, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cint, Cint, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, s.ptr, Gd.ptr, Sd.ptr, rtol > 0 ? rtol : s.n * eps(), max_width, max_refine, L, D, ii, dd))
    download(ctx, L[]), download(ctx, D[]), (iters = s.iters, rank = ii[1], peak_width = ii[2], compressions = ii[3], refinements = ii[4], res0 = dd[1], res = dd[2])
end

# DREHip.jl — Julia shim binding libdre_hip.so with `ccall`.
#
# Keeps the CommonSolve surface of DifferentialRiccatiEquations.jl for the low-rank GDRE path
# (GDREProblem / GALEProblem, Ros1 / Ros2, ADI, Shifts, lowrank, compress!, residual, Callbacks) and forwards
# every arithmetic operation to the MI355X engine.  `julia` is not installed in the build image, so this file
# could only be syntax-reviewed there; the Python/ctypes mirror (`../api.py`, `../device.py`) exercises exactly
# the same C entry points in the test-suite.  See INTEGRATION.md for the binding table.
module DREHip

using LinearAlgebra, SparseArrays
import CommonSolve
import CommonSolve: solve, init, solve!, step!

const LIB = get(ENV, "DRE_HIP_LIB", joinpath(@__DIR__, "..", "libdre_hip.so"))

struct DREError <: Exception
    code::Int32
    msg::String
end

# Julia runs finalizers in no particular order, and a device object freed after its context would touch freed memory
# (the pool lives in the context).  Every handle therefore counts itself in (`retain!`) and out (`release!`); the native context is
# destroyed by whoever goes last — the Context's own finalizer or the last handle's.
mutable struct Context
    ptr::Ptr{Cvoid}
    live::Int          # device objects that still reference this context
    dead::Bool         # the Context object itself has been finalized
    function Context(device::Integer=0)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:dre_ctx_create, LIB), Cint, (Cint, Ref{Ptr{Cvoid}}), device, out)
        rc == 0 || throw(DREError(rc, unsafe_string(ccall((:dre_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL))))
        ctx = new(out[], 0, false)
        finalizer(ctx) do c
            c.dead = true
            c.live == 0 && c.ptr != C_NULL && (ccall((:dre_ctx_destroy, LIB), Cint, (Ptr{Cvoid},), c.ptr); c.ptr = C_NULL)
        end
    end
end
retain!(ctx::Context) = (ctx.live += 1; ctx)
function release!(ctx::Context)
    ctx.live -= 1
    if ctx.dead && ctx.live == 0 && ctx.ptr != C_NULL
        ccall((:dre_ctx_destroy, LIB), Cint, (Ptr{Cvoid},), ctx.ptr); ctx.ptr = C_NULL
    end
    nothing
end

function chk(ctx::Context, rc)
    rc == 0 && return nothing
    throw(DREError(rc, unsafe_string(ccall((:dre_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx.ptr))))
end

# engine tunables (include/dre_hip.h: dre_ctx_set_option), e.g. set_option!(ctx, "dense_inverse_max_n", 0) forces the multifrontal sweeps
set_option!(ctx::Context, name::AbstractString, value::Real) =
    chk(ctx, ccall((:dre_ctx_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Cdouble), ctx.ptr, name, Float64(value)))

const DEFAULT = Ref{Union{Nothing,Context}}(nothing)
default_context() = something(DEFAULT[], (DEFAULT[] = Context(0)))

# ---- handles -------------------------------------------------------------------------------------
mutable struct Dense
    ctx::Context
    ptr::Ptr{Cvoid}
end
function upload(ctx::Context, A::AbstractMatrix{<:Real})
    M = Matrix{Float64}(A)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    chk(ctx, ccall((:dre_dense_upload, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
                   ctx.ptr, size(M, 1), size(M, 2), M, max(size(M, 1), 1), out))
    d = Dense(retain!(ctx), out[])
    finalizer(x -> (ccall((:dre_dense_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.ptr, x.ptr); release!(x.ctx)), d)
end

# A Julia SparseMatrixCSC is handed over verbatim: CSC of M is CSR of M' (include/dre_hip.h conventions)
mutable struct Pencil
    ctx::Context
    ptr::Ptr{Cvoid}
    n::Int
end
function Pencil(ctx::Context, E::SparseMatrixCSC{Float64,Int64}, A::SparseMatrixCSC{Float64,Int64}; leaf_size=0)
    n = size(E, 1)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    chk(ctx, ccall((:dre_pencil_create, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Cint, Ref{Ptr{Cvoid}}),
                   ctx.ptr, n, E.colptr, E.rowval, E.nzval, A.colptr, A.rowval, A.nzval, 1, leaf_size, out))
    p = Pencil(retain!(ctx), out[], n)
    finalizer(x -> (ccall((:dre_pencil_free, LIB), Cint, (Ptr{Cvoid},), x.ptr); release!(x.ctx)), p)
end
Pencil(ctx, E, A; kw...) = Pencil(ctx, SparseMatrixCSC{Float64,Int64}(sparse(E)), SparseMatrixCSC{Float64,Int64}(sparse(A)); kw...)

# ---- LDLᵀ (src/LDLt.jl) --------------------------------------------------------------------------
"Host-side lazy `Σ αᵢ Lᵢ Dᵢ Lᵢᵀ`; `handle` is set for results that still live on the device."
mutable struct LDLᵀ
    alphas::Vector{Float64}
    Ls::Vector{Matrix{Float64}}
    Ds::Vector{Matrix{Float64}}
    handle::Ptr{Cvoid}
    ctx::Union{Nothing,Context}
end
lowrank(L, D=Matrix{Float64}(I, size(L, 2), size(L, 2))) = LDLᵀ([1.0], [Matrix{Float64}(L)], [Matrix{Float64}(D)], C_NULL, nothing)
LinearAlgebra.rank(X::LDLᵀ) = sum(L -> size(L, 2), X.Ls; init=0)
Base.size(X::LDLᵀ) = (n = size(first(X.Ls), 1); (n, n))
Base.:*(a::Real, X::LDLᵀ) = LDLᵀ(a .* X.alphas, X.Ls, X.Ds, C_NULL, nothing)
Base.:+(X::LDLᵀ, Y::LDLᵀ) = LDLᵀ(vcat(X.alphas, Y.alphas), vcat(X.Ls, Y.Ls), vcat(X.Ds, Y.Ds), C_NULL, nothing)

function to_device(ctx::Context, p::Union{Nothing,Pencil}, X::LDLᵀ)
    pp = p === nothing ? C_NULL : p.ptr
    h = C_NULL
    if isempty(X.Ls)                  # zero(X): no blocks (src/LDLt.jl:62-66) -> an explicit zero object, never a NULL handle
        p === nothing && throw(ArgumentError("a zero LDLᵀ (no blocks) takes its dimension from a pencil"))
        out = Ref{Ptr{Cvoid}}(C_NULL)
        chk(ctx, ccall((:dre_ldlt_zero, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), ctx.ptr, pp, p.n, out))
        return out[]
    end
    for (a, L, D) in zip(X.alphas, X.Ls, X.Ds)
        Ld, Dd = upload(ctx, L), upload(ctx, D)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        chk(ctx, ccall((:dre_ldlt_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}),
                       ctx.ptr, pp, Ld.ptr, Dd.ptr, a, out))
        if h == C_NULL
            h = out[]
        else
            s = Ref{Ptr{Cvoid}}(C_NULL)
            chk(ctx, ccall((:dre_ldlt_add, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), ctx.ptr, h, out[], s))
            h = s[]
        end
    end
    h
end

"alpha, L, D of a device object in the reference's canonical form (D = diagm(λ))"
function from_device(ctx::Context, h::Ptr{Cvoid})
    chk(ctx, ccall((:dre_ldlt_canonicalize, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, h))
    n, r, nb = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
    ccall((:dre_ldlt_info, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}), h, n, r, nb)
    L = zeros(n[], r[]); D = zeros(r[], r[]); alpha = Ref{Cdouble}(1.0)
    chk(ctx, ccall((:dre_ldlt_destructure, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cdouble}, Ptr{Float64}, Cint, Ptr{Float64}, Cint),
                   ctx.ptr, h, alpha, L, max(n[], 1), D, max(r[], 1)))
    LDLᵀ([alpha[]], [L], [D], C_NULL, nothing)
end

function compress!(X::LDLᵀ; ctx=default_context())     # src/LDLt.jl:204-225
    h = to_device(ctx, nothing, X)
    chk(ctx, ccall((:dre_ldlt_compress, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, h))
    Y = from_device(ctx, h)
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, h)
    X.alphas, X.Ls, X.Ds = Y.alphas, Y.Ls, Y.Ds
    X
end
function LinearAlgebra.norm(X::LDLᵀ; ctx=default_context())    # src/LDLt.jl:77-89
    h = to_device(ctx, nothing, X)
    out = Ref{Cdouble}(0.0)
    chk(ctx, ccall((:dre_ldlt_norm, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cdouble}), ctx.ptr, h, out))
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, h)
    out[]
end

# ---- Shifts, ADI, problems (src/Shifts.jl, src/lyapunov/types.jl, src/riccati/types.jl) ------------
module Shifts
abstract type Strategy end
struct Cyclic <: Strategy; inner; end
struct Heuristic <: Strategy           # src/shifts/heuristic.jl:22-37
    nshifts::Int
    k₊::Int
    k₋::Int
end
struct Projection <: Strategy
    n_history::Int
    Projection(u) = isodd(u) ? throw(ArgumentError("History must be even; got $u")) : new(u)
end
struct UserDefined <: Strategy          # plug-in strategy: `fn` is a @cfunction pointer of the signature dre_shift_fn (include/dre_hip.h)
    fn::Ptr{Cvoid}
    user::Ptr{Cvoid}
    n_history::Int
end
UserDefined(fn; user=C_NULL, n_history=2) = UserDefined(fn, user, n_history)
# Structural hash / equality: a `Cyclic` holds a Vector, whose default hash is its identity — two separately built `Cyclic([1.0])` must hash
# alike (test/hash.jl; the reference does the same in src/shifts/helpers.jl:23-27).  `Heuristic` and `Projection` are bits types.
Base.hash(c::Cyclic, h::UInt) = hash(c.inner, hash(:DREHipCyclic, h))
Base.:(==)(a::Cyclic, b::Cyclic) = a.inner == b.inner
end

Base.@kwdef struct ADI
    maxiters::Int = 100
    reltol::Union{Nothing,Real} = nothing
    abstol::Union{Nothing,Real} = nothing
    shifts::Shifts.Strategy = Shifts.Projection(2)
    ignore_initial_guess::Bool = false
    compression_interval::Int = 10
    compression::Bool = true
    warn_convergence::Bool = true
    compress_exact::Bool = false
    # `nothing` / Backslash(): the device multifrontal LU.  A `Ptr{Cvoid}` obtained with `@cfunction` for a function of the signature
    # `dre_block_solver_fn` (include/dre_hip.h) plugs a user solver of the sparse shifted system in — the ALG of
    # `ShermanMorrisonWoodbury(ALG, Backslash())` (src/blocklinear/types.jl:15-62, example test/cuda.jl:23-30,74)
    inner_alg::Union{Nothing,Ptr{Cvoid}} = nothing
end
inner_ptr(alg::ADI) = something(alg.inner_alg, C_NULL)
# options hash by their properties (src/lyapunov/types.jl:34-40; test/hash.jl builds `ADI(; shifts=...)` twice and compares)
function Base.hash(alg::ADI, h::UInt)
    acc = hash(:DREHipADI, h)
    for p in fieldnames(ADI)
        acc = hash(getfield(alg, p), hash(p, acc))
    end
    acc
end
Base.:(==)(a::ADI, b::ADI) = all(getfield(a, p) == getfield(b, p) for p in fieldnames(ADI))

# mirrors `dre_adi_options` of include/dre_hip.h field by field
struct AdiOptionsC
    maxiters::Int32
    reltol::Float64
    abstol::Float64
    ignore_initial_guess::Int32
    compression_interval::Int32
    compression::Int32
    shift_kind::Int32
    n_history::Int32
    nshifts::Int32
    shifts_re::Ptr{Float64}
    shifts_im::Ptr{Float64}
    compress_tolfac::Float64
    compress_exact::Int32
    heuristic_kplus::Int32
    heuristic_kminus::Int32
    inner_solve::Ptr{Cvoid}     # dre_block_solver_fn or C_NULL (inner_alg = Backslash() on the device LU)
    inner_user::Ptr{Cvoid}
    shift_fn::Ptr{Cvoid}        # dre_shift_fn (shift_kind 3) or C_NULL
    shift_user::Ptr{Cvoid}
end

function options(alg::ADI)
    if alg.shifts isa Shifts.UserDefined
        # a user-defined strategy (src/Shifts.jl:79-116): `fn` = @cfunction of the signature dre_shift_fn (include/dre_hip.h) — it is shown the
        # residual factor / the last n_history increments as a device block and fills a batch of shifts (take_many!, shifts/helpers.jl:60-89)
        o = AdiOptionsC(alg.maxiters, something(alg.reltol, -1.0), something(alg.abstol, -1.0), alg.ignore_initial_guess,
                        alg.compression_interval, alg.compression, 3, alg.shifts.n_history, 0, C_NULL, C_NULL, 4.0, alg.compress_exact, 0, 0, inner_ptr(alg), C_NULL,
                        alg.shifts.fn, alg.shifts.user)
        return o, nothing
    end
    if alg.shifts isa Shifts.Cyclic && alg.shifts.inner isa Shifts.Heuristic
        h = alg.shifts.inner          # Cyclic(Heuristic(nshifts, k₊, k₋)): recomputed on the device at the start of every Lyapunov solve
        o = AdiOptionsC(alg.maxiters, something(alg.reltol, -1.0), something(alg.abstol, -1.0), alg.ignore_initial_guess,
                        alg.compression_interval, alg.compression, 2, 2, h.nshifts, C_NULL, C_NULL, 4.0, alg.compress_exact, h.k₊, h.k₋, inner_ptr(alg), C_NULL, C_NULL, C_NULL)
        return o, nothing
    elseif alg.shifts isa Shifts.Cyclic
        vals = ComplexF64.(collect(alg.shifts.inner))
        re, im = real.(vals), imag.(vals)
        o = AdiOptionsC(alg.maxiters, something(alg.reltol, -1.0), something(alg.abstol, -1.0), alg.ignore_initial_guess,
                        alg.compression_interval, alg.compression, 0, 2, length(vals), pointer(re), pointer(im), 4.0, alg.compress_exact, 0, 0, inner_ptr(alg), C_NULL, C_NULL, C_NULL)
        return o, (re, im)
    end
    o = AdiOptionsC(alg.maxiters, something(alg.reltol, -1.0), something(alg.abstol, -1.0), alg.ignore_initial_guess,
                    alg.compression_interval, alg.compression, 1, alg.shifts.n_history, 0, C_NULL, C_NULL, 4.0, alg.compress_exact, 0, 0, inner_ptr(alg), C_NULL, C_NULL, C_NULL)
    o, nothing
end

# ---- Callbacks (src/Callbacks.jl:97-187): no-op generic functions taking the observer first --------------------------------------
module Callbacks
observe_gale_start!(::Any, args...) = nothing
observe_gale_step!(::Any, args...) = nothing
observe_gale_done!(::Any, args...) = nothing
observe_gale_failed!(::Any, args...) = nothing
observe_gale_metadata!(::Any, args...) = nothing
observe_gdre_start!(::Any, args...) = nothing
observe_gdre_step!(::Any, args...) = nothing
observe_gdre_done!(::Any, args...) = nothing
end
using .Callbacks

# ---- GALE: A'XE + E'XA = -C  (src/lyapunov/types.jl:10-16) ------------------------------------------------------------------------
"`A` is a sparse matrix or a `LowRankUpdate(A0, α, U, V)` = A0 + inv(α) U V (src/LowRankUpdate.jl:18-39)"
struct LowRankUpdate
    A; α::Float64; U::Matrix{Float64}; V::Matrix{Float64}
end
lr_update(A, α, U, V) = LowRankUpdate(A, Float64(α), Matrix{Float64}(U), Matrix{Float64}(V))
struct GALEProblem
    E; A; C            # LDLᵀ (ADI, GMRES) or a dense matrix (MatrixSign)
end
split_operator(A::LowRankUpdate) = (A.A, A.α, A.U, permutedims(A.V))
split_operator(A) = (A, 1.0, nothing, nothing)

function gale_operands(ctx, prob::GALEProblem, X0)
    A0, α, U, Vt = split_operator(prob.A)
    pencil = Pencil(ctx, prob.E, A0)
    Ud = U === nothing ? nothing : upload(ctx, U)
    Vd = Vt === nothing ? nothing : upload(ctx, Vt)
    Ch = to_device(ctx, pencil, prob.C)
    Xh = X0 === nothing ? C_NULL : to_device(ctx, pencil, X0)
    (; pencil, α, Ud, Vd, Ch, Xh)
end
"device LDLᵀ handles made by gale_operands belong to the call that made them (ADVICE round 2: they leaked n×k doubles per call)"
function free_operands(ctx, o)
    o.Ch == C_NULL || ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, o.Ch)
    o.Xh == C_NULL || ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, o.Xh)
    nothing
end
dptr(x) = x === nothing ? C_NULL : x.ptr

"iteration record of a finished ADI run (dre_adi_result_info / dre_adi_result_history)"
function adi_history(res::Ptr{Cvoid})
    ii = zeros(Int64, 5); dd = zeros(3)
    ccall((:dre_adi_result_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}), res, ii, dd)
    norms = zeros(ii[4]); its = zeros(Int32, ii[4]); sre = zeros(max(ii[1], 1)); sim = zeros(max(ii[1], 1))
    ccall((:dre_adi_result_history, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}), res, norms, its, sre, sim)
    (; iters=Int(ii[1]), converged=ii[2] != 0, warnings=Int(ii[3]), res_norm=dd[1], abstol=dd[2], norms, its, shifts=complex.(sre, sim)[1:ii[1]])
end
"replays observe_gale_start!/step!/metadata!/failed! in the order of src/lyapunov/adi.jl:37,65,103,119,125,192 (the loop ran on the device)"
function replay_gale(observer, prob, alg, h)
    observer === nothing && return
    Callbacks.observe_gale_start!(observer, prob, alg)
    pos = 0
    for (it, nrm) in zip(h.its, h.norms)
        while pos < it
            pos += 1
            Callbacks.observe_gale_metadata!(observer, "ADI shifts", h.shifts[pos])
        end
        Callbacks.observe_gale_step!(observer, Int(it), nothing, nothing, nrm)
    end
    h.converged || Callbacks.observe_gale_failed!(observer)
end

"solve(::GALEProblem, ::ADI; initial_guess, observer)  — src/lyapunov/adi.jl:29-89"
function CommonSolve.solve(prob::GALEProblem, alg::ADI; initial_guess=nothing, observer=nothing, ctx::Context=default_context())
    solver = CommonSolve.init(prob, alg; initial_guess, observer, ctx)
    CommonSolve.solve!(solver)
end

"The reference's ADICache protocol on the device (src/lyapunov/adi.jl:5-21,91-141): init / step! / isdone / solve! / iterate"
mutable struct ADISolver
    ctx::Context
    ptr::Ptr{Cvoid}
    prob::GALEProblem
    alg::ADI
    observer
    keep
end
function CommonSolve.init(prob::GALEProblem, alg::ADI; initial_guess=nothing, observer=nothing, ctx::Context=default_context())
    o = gale_operands(ctx, prob, initial_guess)
    opt, keep = options(alg)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve keep chk(ctx, ccall((:dre_adi_init, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{AdiOptionsC}, Ref{Ptr{Cvoid}}),
        ctx.ptr, o.pencil.ptr, 1.0, 0.0, o.α, dptr(o.Ud), dptr(o.Vd), o.Ch, o.Xh, Ref(opt), out))
    s = ADISolver(retain!(ctx), out[], prob, alg, observer, (o, keep))
    finalizer(x -> (ccall((:dre_adi_free, LIB), Cint, (Ptr{Cvoid},), x.ptr); free_operands(x.ctx, x.keep[1]); release!(x.ctx)), s)
end
isdone(s::ADISolver) = (d = Ref{Cint}(0); ccall((:dre_adi_isdone, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), s.ptr, d); d[] != 0)
"(X, residual) of the solver's current iteration — the payload of observe_gale_step! (src/lyapunov/adi.jl:119, src/Callbacks.jl:97-107); dre_adi_snapshot"
function snapshot(s::ADISolver)
    xh, rh = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    chk(s.ctx, ccall((:dre_adi_snapshot, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}), s.ctx.ptr, s.ptr, xh, rh))
    X, R = from_device(s.ctx, xh[]), from_device(s.ctx, rh[])
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), s.ctx.ptr, xh[])
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), s.ctx.ptr, rh[])
    X, R
end

# ---- multi-GPU: the communicator lives inside the library (RCCL over xGMI; include/dre_hip.h dre_comm_*) ---------------------------
"128-byte RCCL unique id (rank 0 creates it; hand it to the other ranks with MPI / Distributed)"
comm_unique_id(ctx::Context) = (id = zeros(UInt8, 128); chk(ctx, ccall((:dre_comm_unique_id, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}), ctx.ptr, id)); id)
"attach a communicator: from here on the solves entered through `ctx` run column-sharded over the ranks (same calls, same inputs on every rank)"
comm_init!(ctx::Context, nranks::Integer, rank::Integer, id::Vector{UInt8}) =
    chk(ctx, ccall((:dre_comm_init, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}), ctx.ptr, nranks, rank, id))
comm_free!(ctx::Context) = chk(ctx, ccall((:dre_comm_free, LIB), Cint, (Ptr{Cvoid},), ctx.ptr))
CommonSolve.step!(s::ADISolver) = (chk(s.ctx, ccall((:dre_adi_step, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), s.ctx.ptr, s.ptr)); s)
Base.iterate(s::ADISolver, _=nothing) = isdone(s) ? nothing : (CommonSolve.step!(s), nothing)
function CommonSolve.solve!(s::ADISolver)
    chk(s.ctx, ccall((:dre_adi_solve, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), s.ctx.ptr, s.ptr))
    res = Ref{Ptr{Cvoid}}(C_NULL)
    chk(s.ctx, ccall((:dre_adi_finish, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), s.ctx.ptr, s.ptr, res))
    h = adi_history(res[])
    xh = Ref{Ptr{Cvoid}}(C_NULL)
    ccall((:dre_adi_result_take_x, LIB), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), res[], xh)
    X = from_device(s.ctx, xh[])
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), s.ctx.ptr, xh[])
    ccall((:dre_adi_result_free, LIB), Cint, (Ptr{Cvoid},), res[])
    replay_gale(s.observer, s.prob, s.alg, h)
    s.observer === nothing || Callbacks.observe_gale_done!(s.observer, h.iters, X, nothing, h.res_norm)
    h.converged || !s.alg.warn_convergence || @warn "ADI did not converge" residual = h.res_norm abstol = h.abstol maxiters = s.alg.maxiters
    X
end

"residual(::GALEProblem, ::LDLᵀ)  — src/lyapunov/residual.jl:3-31"
function residual(prob::GALEProblem, X::LDLᵀ; ctx::Context=default_context())
    o = gale_operands(ctx, prob, X)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    chk(ctx, ccall((:dre_gale_residual, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                   ctx.ptr, o.pencil.ptr, 1.0, 0.0, o.α, dptr(o.Ud), dptr(o.Vd), o.Ch, o.Xh, out))
    R = from_device(ctx, out[])
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, out[])
    free_operands(ctx, o)
    R
end

"dot(X, Y) = tr(X'Y) for two LDLᵀ objects — src/LDLt.jl:91-108 (dre_ldlt_dot: block-wise trace form on the device)"
function LinearAlgebra.dot(X::LDLᵀ, Y::LDLᵀ; ctx::Context=default_context())
    hx = to_device(ctx, nothing, X); hy = to_device(ctx, nothing, Y)
    out = Ref{Cdouble}(0.0)
    chk(ctx, ccall((:dre_ldlt_dot, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cdouble}), ctx.ptr, hx, hy, out))
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, hx)
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, hy)
    out[]
end

"LyapunovOperator(E, A) * X = A'XE + E'XA as an LDLᵀ object — src/lyapunov/gmres.jl:108-120 (dre_gale_apply)"
function lyapunov_apply(prob::GALEProblem, X::LDLᵀ; ctx::Context=default_context())
    o = gale_operands(ctx, prob, X)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    chk(ctx, ccall((:dre_gale_apply, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                   ctx.ptr, o.pencil.ptr, 1.0, 0.0, o.α, dptr(o.Ud), dptr(o.Vd), o.Xh, out))
    R = from_device(ctx, out[])
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, out[])
    free_operands(ctx, o)
    R
end

"compress_fast!(X): the engine's own early-terminating compression (dre_ldlt_compress_fast); same X up to 4 eps ‖X‖, orthonormal factor, band D"
function compress_fast!(X::LDLᵀ; ctx=default_context())
    h = to_device(ctx, nothing, X)
    chk(ctx, ccall((:dre_ldlt_compress_fast, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, h))
    Y = from_device(ctx, h)
    ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, h)
    X.alphas, X.Ls, X.Ds = Y.alphas, Y.Ls, Y.Ds
    X
end

"concatenate!(X)  — src/LDLt.jl:174-191 (host side: hcat of the factors, block-diagonal of the scaled inner matrices)"
function concatenate!(X::LDLᵀ)
    length(X.Ls) <= 1 && return X
    L = reduce(hcat, X.Ls)
    r = size(L, 2); D = zeros(r, r); off = 0
    for (a, Di) in zip(X.alphas, X.Ds)
        k = size(Di, 1); D[off+1:off+k, off+1:off+k] .= a .* Di; off += k
    end
    X.alphas, X.Ls, X.Ds = [1.0], [L], [D]
    X
end

struct GDREProblem{XT}
    E; A; B; C
    X0::XT
    tspan
end
struct DRESolution
    X; K; t
end
Base.@kwdef struct Ros1; inner_alg = nothing; end
Base.@kwdef struct Ros2; inner_alg = nothing; end

"solve(::GDREProblem{LDLᵀ}, ::Ros1/Ros2; dt, save_state)  — src/riccati/lowrank_ros1.jl, lowrank_ros2.jl"
function CommonSolve.solve(prob::GDREProblem{LDLᵀ}, alg::Union{Ros1,Ros2}; dt::Real, save_state::Bool=false, observer=nothing,
                           ctx::Context=default_context())
    inner = something(alg.inner_alg, ADI())
    pencil = Pencil(ctx, prob.E, prob.A)
    X0 = to_device(ctx, pencil, prob.X0)
    B, C = upload(ctx, prob.B), upload(ctx, prob.C)
    opt, keep = options(inner)
    res = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve keep begin
        chk(ctx, ccall((:dre_gdre_solve, LIB), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cint, Cint, Ref{AdiOptionsC}, Ref{Ptr{Cvoid}}),
                       ctx.ptr, pencil.ptr, B.ptr, C.ptr, X0, prob.tspan[1], prob.tspan[2], dt, alg isa Ros1 ? 1 : 2, save_state, Ref(opt), res))
    end
    info = zeros(Int64, 7)
    ccall((:dre_gdre_result_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), res[], info)
    nt, nx, m, n = info[1], info[2], info[6], info[7]
    t = zeros(nt)
    ccall((:dre_gdre_result_times, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), res[], t)
    Ks = map(0:nt-1) do i
        K = zeros(m, n)
        chk(ctx, ccall((:dre_gdre_result_K, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Cint), ctx.ptr, res[], i, K, m))
        K
    end
    Xs = Any[prob.X0]                                  # first(sol.X) === prob.X0 (test/rail.jl:40)
    for i in 1:nx-1
        h = Ref{Ptr{Cvoid}}(C_NULL)
        ccall((:dre_gdre_result_X, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), res[], i, h)
        push!(Xs, from_device(ctx, h[]))
        ccall((:dre_ldlt_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, h[])
    end
    if observer !== nothing
        # hooks in the reference's order (lowrank_ros1.jl:10,32,59,63 around adi.jl:37-126); X of intermediate steps only with save_state
        ngale = Int(info[5]); per = nt > 1 ? ngale ÷ (nt - 1) : 0
        Callbacks.observe_gdre_start!(observer, prob, alg)
        Callbacks.observe_gdre_step!(observer, t[1], Xs[1], Ks[1])
        for i in 2:nt
            for j in (i-2)*per:(i-1)*per-1
                cnt = zeros(Int64, 2)
                ccall((:dre_gdre_result_gale_history, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                      res[], j, cnt, C_NULL, C_NULL, C_NULL, C_NULL)
                norms = zeros(cnt[1]); its = zeros(Int32, cnt[1]); sre = zeros(max(cnt[2], 1)); sim = zeros(max(cnt[2], 1))
                ccall((:dre_gdre_result_gale_history, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                      res[], j, cnt, norms, its, sre, sim)
                gi = zeros(Int64, 4); gd = zeros(2)
                ccall((:dre_gdre_result_gale, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Float64}), res[], j, gi, gd)
                h = (; iters=Int(gi[1]), converged=gi[2] != 0, res_norm=gd[1], abstol=gd[2], norms, its, shifts=complex.(sre, sim)[1:cnt[2]])
                replay_gale(observer, nothing, inner, h)
                Callbacks.observe_gale_done!(observer, h.iters, nothing, nothing, h.res_norm)
            end
            Xi = save_state ? Xs[i] : (i == nt ? Xs[end] : nothing)
            Callbacks.observe_gdre_step!(observer, t[i], Xi, Ks[i])
        end
        Callbacks.observe_gdre_done!(observer)
    end
    ccall((:dre_gdre_result_free, LIB), Cint, (Ptr{Cvoid},), res[])
    DRESolution(Xs, Ks, t)
end

# ---- dense path: solve(::GDREProblem{<:Matrix}, Ros1..Ros4(MatrixSign())), solve(::GALEProblem, MatrixSign()) ----------------------
"Dense GALE algorithm tag: the generalized matrix-sign-function iteration (needs a c-stable pencil; DREError(-7) otherwise).  tol = 0: 10 n eps.  Any n <= 46340 whose (maxiters + 26) n^2 doubles fit in device memory (register pivoting panel for n <= 4096, tournament panel above: option dense_gj_panel)."
Base.@kwdef struct MatrixSign; maxiters::Int = 50; tol::Float64 = 0.0; max_refine::Int = 2; end
Base.@kwdef struct Ros3; inner_alg = nothing; end
Base.@kwdef struct Ros4; inner_alg = nothing; end

function download(ctx::Context, d::Ptr{Cvoid})
    r, c = Ref{Cint}(0), Ref{Cint}(0)
    ccall((:dre_dense_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), d, r, c)
    M = zeros(r[], c[])
    chk(ctx, ccall((:dre_dense_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cint), ctx.ptr, d, M, max(r[], 1)))
    ccall((:dre_dense_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.ptr, d)
    M
end

"solve(GALEProblem(E, A, C), MatrixSign()): A'XE + E'XA = -C with dense X (bartels-stewart.jl:3-12, lyapc replaced); an LDLᵀ C is densified"
function CommonSolve.solve(prob::GALEProblem, alg::MatrixSign; ctx::Context=default_context())
    C = prob.C isa LDLᵀ ? sum(a * L * D * L' for (a, L, D) in zip(prob.C.alphas, prob.C.Ls, prob.C.Ds)) : prob.C
    E, A, R = upload(ctx, Matrix(prob.E)), upload(ctx, Matrix(prob.A)), upload(ctx, Matrix(C))
    X = Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 2), zeros(2)
    chk(ctx, ccall((:dre_dense_gale_solve, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, E.ptr, A.ptr, R.ptr, alg.maxiters, alg.tol, alg.max_refine, X, ii, dd))
    download(ctx, X[])
end

# ---- factored sign-function solver: solve(::GALEProblem{LDLᵀ}, FactoredSign()) -> LDLᵀ (in the place of lyapunov/adi.jl where no shifts are at hand) ----
"Low-rank GALE algorithm tag: the sign iteration on the densified pencil with its kept sequence applied to the factor of the right-hand side; LDLᵀ in, LDLᵀ out, no shifts (c-stable pencils only; DREError(-7) otherwise).  tol = 0: 10 n eps; rtol = 0: n eps (compress!, LDLt.jl:237-245)."
Base.@kwdef struct FactoredSign; maxiters::Int = 50; tol::Float64 = 0.0; rtol::Float64 = 0.0; max_width::Int = 256; max_refine::Int = 1; end

dense_operator(A::LowRankUpdate) = Matrix{Float64}(A.A) + inv(A.α) * (A.U * A.V)
dense_operator(A) = Matrix{Float64}(A)

"A kept sign factorisation of one pencil (F, E) on the device (dre_sign_create): further right-hand sides cost a replay only (the two stages of Ros2, lowrank_ros2.jl:41-69)"
mutable struct SignFactorization
    ctx::Context
    ptr::Ptr{Cvoid}
    n::Int
    iters::Int
end
function SignFactorization(ctx::Context, E, F; maxiters::Int=50, tol::Float64=0.0)
    Ed, Fd = upload(ctx, dense_operator(E)), upload(ctx, dense_operator(F))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    chk(ctx, ccall((:dre_sign_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Ref{Ptr{Cvoid}}), ctx.ptr, Ed.ptr, Fd.ptr, maxiters, tol, h))
    it = Ref{Int64}(0)
    ccall((:dre_sign_info, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), h[], it)
    s = SignFactorization(ctx, h[], size(E, 1), it[])
    finalizer(x -> ccall((:dre_sign_free, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.ptr, x.ptr), s)
end

"F'XE + E'XF = -G S G' on a kept factorisation: (L, D, info) with X = L D L', D diagonal; transposed = true: the dual equation F Y E' + E Y F' = -G S G' from the same factorisation"
function solve_lr(s::SignFactorization, G::AbstractMatrix, S::AbstractMatrix; rtol::Float64=0.0, max_width::Int=256, max_refine::Int=1, transposed::Bool=false)
    transposed && return solve_lr_t(s, G, S; rtol = rtol, max_width = max_width, max_refine = max_refine)
    ctx = s.ctx
    Gd, Sd = upload(ctx, Matrix{Float64}(G)), upload(ctx, Matrix{Float64}(S))
    L, D = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 4), zeros(2)
    chk(ctx, ccall((:dre_sign_solve_lr, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cint, Cint, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, s.ptr, Gd.ptr, Sd.ptr, rtol > 0 ? rtol : s.n * eps(), max_width, max_refine, L, D, ii, dd))
    download(ctx, L[]), download(ctx, D[]), (iters = s.iters, rank = ii[1], peak_width = ii[2], compressions = ii[3], refinements = ii[4], res0 = dd[1], res = dd[2])
end

"F'XE + E'XF = -R for a dense symmetric R on a kept factorisation (the MatrixSign replay): (X, info); transposed = true: the dual equation F Y E' + E Y F' = -R from the same factorisation"
function solve_dense(s::SignFactorization, R::AbstractMatrix; max_refine::Int=2, transposed::Bool=false)
    transposed && return solve_dense_t(s, R; max_refine = max_refine)
    ctx = s.ctx
    Rd = upload(ctx, Matrix{Float64}(R))
    X = Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 2), zeros(2)
    chk(ctx, ccall((:dre_sign_solve_dense, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, s.ptr, Rd.ptr, max_refine, X, ii, dd))
    download(ctx, X[]), (iters = ii[1], refinements = ii[2], res0 = dd[1], res = dd[2])
end

"solve(GALEProblem(E, A, C::LDLᵀ), FactoredSign()) -> LDLᵀ; A may be a matrix or a LowRankUpdate (densified); a multi-component C is concatenated"
function CommonSolve.solve(prob::GALEProblem, alg::FactoredSign; ctx::Context=default_context())
    prob.C isa LDLᵀ || throw(ArgumentError("FactoredSign() takes an LDLᵀ right-hand side; a dense C goes with MatrixSign()"))
    G = reduce(hcat, prob.C.Ls)
    S = zeros(size(G, 2), size(G, 2))
    o = 0
    for (a, L, D) in zip(prob.C.alphas, prob.C.Ls, prob.C.Ds)
        k = size(L, 2)
        S[o+1:o+k, o+1:o+k] = a * D
        o += k
    end
    s = SignFactorization(ctx, prob.E, prob.A; maxiters = alg.maxiters, tol = alg.tol)
    L, D, _ = solve_lr(s, G, S; rtol = alg.rtol, max_width = alg.max_width, max_refine = alg.max_refine)
    finalize(s)
    LDLᵀ([1.0], [L], [D], C_NULL, nothing)
end

include("DREHipSignDual.jl")          # solve_dense_t, solve_lr_t: the dual equation on a kept factorisation (dre_version >= 109)
include("DREHipBalance.jl")           # svd_jacobi, balanced_truncation: device SVD and balanced truncation (dre_version >= 110)
include("DREHipBatchJacobi.jl")       # sym_eigh_batch, svd_jacobi_batch, balance_lr_batch: ensembles in shared launches (dre_version >= 111)
include("DREHipFreq.jl")              # freq_response, sigma_response, bt_error: frequency response batched by frequency (dre_version >= 112)
include("DREHipLQG.jl")               # solve_gare_pair, lqg_balanced_truncation, lqg_error: LQG balanced truncation (dre_version >= 113)
include("DREHipSylvester.jl")         # DenseGSYLEProblem, SylvesterFactorization, h2_norm, h2_inner, h2_error: Sylvester solver and H2 tools (dre_version >= 119; unrun)

"""Dense GARE: Q + A'XE + E'XA - E'XGXE = 0 with G = β B R⁻¹ Bᵀ, Q = γ Cᵀ S C (riccati/types.jl:41-52), all dense.  `solve(prob, MatrixSign())`
returns the stabilizing X from the sign function of the Hamiltonian pencil plus Newton-Kleinman refinement (DREError(-7) when the
Hamiltonian has eigenvalues on or near the imaginary axis)."""
Base.@kwdef struct DenseGAREProblem; E; A; B; Rinv = nothing; Ct; S = nothing; beta::Float64 = 1.0; gamma::Float64 = 1.0; end

function gare_operands(ctx::Context, prob::DenseGAREProblem)
    m, q = size(prob.B, 2), size(prob.Ct, 2)
    Rinv = prob.Rinv === nothing && prob.beta == 1 ? nothing : prob.beta * (prob.Rinv === nothing ? Matrix(1.0I, m, m) : Matrix{Float64}(prob.Rinv))
    S = prob.S === nothing && prob.gamma == 1 ? nothing : prob.gamma * (prob.S === nothing ? Matrix(1.0I, q, q) : Matrix{Float64}(prob.S))
    ops = Any[upload(ctx, Matrix{Float64}(M)) for M in (prob.E, prob.A, prob.B, prob.Ct)]
    push!(ops, Rinv === nothing ? nothing : upload(ctx, Rinv), S === nothing ? nothing : upload(ctx, S))
    ops, (o -> o === nothing ? C_NULL : o.ptr)
end

"solve(GAREProblem, MatrixSign()): dense stabilizing X (X, info) — no reference counterpart (riccati/newton.jl solves the low-rank case)"
function CommonSolve.solve(prob::DenseGAREProblem, alg::MatrixSign; ctx::Context=default_context())
    ops, p = gare_operands(ctx, prob)
    X = Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 2), zeros(2)
    chk(ctx, ccall((:dre_dense_gare_solve, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, p(ops[1]), p(ops[2]), p(ops[3]), p(ops[5]), p(ops[4]), p(ops[6]), alg.maxiters, alg.tol, alg.max_refine, X, ii, dd))
    download(ctx, X[]), (iters = ii[1], refinements = ii[2], res0 = dd[1], res = dd[2])
end

"residual(::DenseGAREProblem, X::Matrix) — riccati/residual.jl:54-66: (Q + A'XE + E'XA - E'XGXE, its Frobenius norm)"
function residual(prob::DenseGAREProblem, X::AbstractMatrix; ctx::Context=default_context())
    ops, p = gare_operands(ctx, prob)
    Xd = upload(ctx, Matrix{Float64}(X))
    R, nrm = Ref{Ptr{Cvoid}}(C_NULL), Ref{Cdouble}(0.0)
    chk(ctx, ccall((:dre_dense_gare_residual, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Cdouble}),
                   ctx.ptr, p(ops[1]), p(ops[2]), p(ops[3]), p(ops[5]), p(ops[4]), p(ops[6]), Xd.ptr, R, nrm))
    download(ctx, R[]), nrm[]
end

"""Discrete-time algorithm tag (dre_version >= 118): the squared Smith iteration for a `DenseGDALEProblem`, the structure-preserving doubling
algorithm for a `DenseGDAREProblem`; tol = 0: 10 n eps on the relative step; max_refine Newton (Hewer) steps of the DARE."""
Base.@kwdef struct Doubling; maxiters::Int = 50; tol::Float64 = 0.0; max_refine::Int = 2; end

"Generalized Stein equation A'XA - E'XE = -C, all dense (`dual = true` in `solve`: A X A' - E X E' = -C)"
struct DenseGDALEProblem; E; A; C; end

"""Generalized DARE: Q + A'X(I + GX)⁻¹A - E'XE = 0 with G = β B R⁻¹ Bᵀ, Q = γ Cᵀ S C, all dense; the fields of `DenseGAREProblem`."""
Base.@kwdef struct DenseGDAREProblem; E; A; B; Rinv = nothing; Ct; S = nothing; beta::Float64 = 1.0; gamma::Float64 = 1.0; end

gare_operands(ctx::Context, prob::DenseGDAREProblem) =
    gare_operands(ctx, DenseGAREProblem(E = prob.E, A = prob.A, B = prob.B, Rinv = prob.Rinv, Ct = prob.Ct, S = prob.S, beta = prob.beta, gamma = prob.gamma))

"solve(DenseGDALEProblem, Doubling()): (X, info) by the squared Smith iteration on E⁻¹A (DREError(-7) unless its eigenvalues lie inside the unit circle)"
function CommonSolve.solve(prob::DenseGDALEProblem, alg::Doubling; dual::Bool=false, ctx::Context=default_context())
    ops = [upload(ctx, Matrix{Float64}(M)) for M in (prob.E, prob.A, prob.C)]
    X = Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 2), zeros(2)
    GC.@preserve ops chk(ctx, ccall((:dre_dense_stein_solve, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, dual ? 1 : 0, alg.maxiters, alg.tol, X, ii, dd))
    download(ctx, X[]), (iters = ii[1], step = dd[1])
end

"residual(::DenseGDALEProblem, X): (C + A'XA - E'XE, its Frobenius norm, the scaled norm)"
function residual(prob::DenseGDALEProblem, X::AbstractMatrix; dual::Bool=false, ctx::Context=default_context())
    ops = [upload(ctx, Matrix{Float64}(M)) for M in (prob.E, prob.A, prob.C, X)]
    R, nrm, sc = Ref{Ptr{Cvoid}}(C_NULL), Ref{Cdouble}(0.0), Ref{Cdouble}(0.0)
    GC.@preserve ops chk(ctx, ccall((:dre_dense_stein_residual, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}, Ref{Cdouble}, Ref{Cdouble}),
                   ctx.ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, ops[4].ptr, dual ? 1 : 0, R, nrm, sc))
    download(ctx, R[]), nrm[], sc[]
end

"solve(DenseGDAREProblem, Doubling()): the dense stabilizing X, (X, info)"
function CommonSolve.solve(prob::DenseGDAREProblem, alg::Doubling; ctx::Context=default_context())
    ops, p = gare_operands(ctx, prob)
    X = Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 2), zeros(2)
    GC.@preserve ops chk(ctx, ccall((:dre_dense_dare_solve, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, p(ops[1]), p(ops[2]), p(ops[3]), p(ops[5]), p(ops[4]), p(ops[6]), alg.maxiters, alg.tol, alg.max_refine, X, ii, dd))
    download(ctx, X[]), (iters = ii[1], refinements = ii[2], res0 = dd[1], res = dd[2])
end

"""Both solutions of discrete-time LQG design from ONE doubling (dre_dense_dare_solve_pair): (X, Y, info) with the regulator's
Q + A'X(I + GX)⁻¹A - E'XE = 0 and the filter's G + A Y (I + QY)⁻¹ A' - E Y E' = 0; X is bit for bit the X of `solve(prob, Doubling())`."""
function solve_gdare_pair(prob::DenseGDAREProblem; alg::Doubling=Doubling(), ctx::Context=default_context())
    ops, p = gare_operands(ctx, prob)
    X, Y = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    ii, dd = zeros(Int64, 4), zeros(4)
    GC.@preserve ops chk(ctx, ccall((:dre_dense_dare_solve_pair, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cint, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}},
                    Ptr{Int64}, Ptr{Float64}),
                   ctx.ptr, p(ops[1]), p(ops[2]), p(ops[3]), p(ops[5]), p(ops[4]), p(ops[6]), alg.maxiters, alg.tol, alg.max_refine, X, Y, ii, dd))
    download(ctx, X[]), download(ctx, Y[]), (iters = ii[1], regulator = (refinements = ii[2], res0 = dd[1], res = dd[2]),
                                             filter = (refinements = ii[4], res0 = dd[3], res = dd[4]))
end

"residual(::DenseGDAREProblem, X): (Q + A'X(I + GX)⁻¹A - E'XE, its Frobenius norm, the scaled norm)"
function residual(prob::DenseGDAREProblem, X::AbstractMatrix; ctx::Context=default_context())
    ops, p = gare_operands(ctx, prob)
    Xd = upload(ctx, Matrix{Float64}(X))
    R, nrm, sc = Ref{Ptr{Cvoid}}(C_NULL), Ref{Cdouble}(0.0), Ref{Cdouble}(0.0)
    GC.@preserve ops Xd chk(ctx, ccall((:dre_dense_dare_residual, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Cdouble}, Ref{Cdouble}),
                   ctx.ptr, p(ops[1]), p(ops[2]), p(ops[3]), p(ops[5]), p(ops[4]), p(ops[6]), Xd.ptr, R, nrm, sc))
    download(ctx, R[]), nrm[], sc[]
end

"""Step-size control of the dense Ros2 path, `solve(prob, Ros2(inner_alg = MatrixSign()); dt = dt0, adaptive = StepControl(...))`: a trial step is
judged by Ros2's embedded first-order solution (weighted RMS error with `rtol`, `atol`), accepted iff err ≤ 1, the next size is
τ·clamp(0.9·err^(−1/2), 0.2, 5) inside [dt_min, dt_max]; `tspan[2]` and the `tstops` are hit exactly.  DREError(-8) on a rejection at `dt_min`
or more than `max_steps` trial steps."""
Base.@kwdef struct StepControl
    rtol::Float64 = 1e-3
    atol::Float64 = 1e-6
    dt_min::Float64 = 0.0
    dt_max::Float64 = Inf
    max_steps::Int = 10_000
    tstops::Vector{Float64} = Float64[]
end

"""solve(::GDREProblem{<:Matrix}, Ros1..Ros4(MatrixSign()); dt, save_state, observer)  — src/riccati/dense_ros{1,2,3,4}.jl
`adaptive = StepControl(...)` (Ros2 only): `dt` is the first step and `sol.t` the non-uniform grid of the accepted steps; `stats = true`
returns `(sol, (accepted, rejected, err))`."""
function CommonSolve.solve(prob::GDREProblem{<:AbstractMatrix}, alg::Union{Ros1,Ros2,Ros3,Ros4}; dt::Real, save_state::Bool=false, observer=nothing,
                           ctx::Context=default_context(), adaptive::Union{Nothing,StepControl}=nothing, stats::Bool=false)
    alg.inner_alg isa MatrixSign || throw(ArgumentError("a dense X0 runs on the device only with the inner algorithm named: Ros1(inner_alg = MatrixSign())"))
    adaptive === nothing || alg isa Ros2 || throw(ArgumentError("adaptive = StepControl(...) exists for Ros2 only (its embedded first-order solution is the estimator)"))
    sa = alg.inner_alg
    order = alg isa Ros1 ? 1 : alg isa Ros2 ? 2 : alg isa Ros3 ? 3 : 4
    ops = [upload(ctx, Matrix(M)) for M in (prob.E, prob.A, prob.B, prob.C, prob.X0)]
    res = Ref{Ptr{Cvoid}}(C_NULL)
    if adaptive === nothing
        chk(ctx, ccall((:dre_dense_gdre_solve, LIB), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cint, Cint, Cint, Cdouble, Cint, Ref{Ptr{Cvoid}}),
                       ctx.ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, ops[4].ptr, ops[5].ptr, prob.tspan[1], prob.tspan[2], dt, order, save_state,
                       sa.maxiters, sa.tol, sa.max_refine, res))
    else
        sc = adaptive
        chk(ctx, ccall((:dre_dense_gdre_solve_adaptive, LIB), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cint, Cdouble, Cdouble, Cdouble, Cdouble,
                        Int64, Ptr{Float64}, Cint, Cint, Cint, Cdouble, Cint, Ref{Ptr{Cvoid}}),
                       ctx.ptr, ops[1].ptr, ops[2].ptr, ops[3].ptr, ops[4].ptr, ops[5].ptr, prob.tspan[1], prob.tspan[2], dt, order, sc.rtol, sc.atol,
                       sc.dt_min, sc.dt_max, sc.max_steps, sc.tstops, length(sc.tstops), save_state, sa.maxiters, sa.tol, sa.max_refine, res))
    end
    info = zeros(Int64, 7)
    ccall((:dre_gdre_result_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), res[], info)
    nt, nx, m, n = info[1], info[2], info[6], info[7]
    t = zeros(nt)
    ccall((:dre_gdre_result_times, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), res[], t)
    Kall = zeros(m, n, nt)
    chk(ctx, ccall((:dre_gdre_result_K_all, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, res[], Kall))
    Ks = [Kall[:, :, i] for i in 1:nt]
    Xs = Any[prob.X0]                                  # first(sol.X) === prob.X0 (test/rail.jl:40)
    for i in 1:nx-1
        h = Ref{Ptr{Cvoid}}(C_NULL)
        chk(ctx, ccall((:dre_gdre_result_X_dense, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), ctx.ptr, res[], i, h))
        push!(Xs, download(ctx, h[]))
    end
    counts, errs = zeros(Int64, 2), zeros(max(nt - 1, 1))
    adaptive === nothing || ccall((:dre_gdre_result_step_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}), res[], counts, errs)
    ccall((:dre_gdre_result_free, LIB), Cint, (Ptr{Cvoid},), res[])
    if observer !== nothing                            # dense_ros1.jl's order, replayed after the device run
        Callbacks.observe_gdre_start!(observer, prob, alg)
        for i in 1:nt
            Xi = (save_state || i == 1) ? Xs[i] : (i == nt ? Xs[end] : nothing)
            Callbacks.observe_gdre_step!(observer, t[i], Xi, Ks[i])
        end
        Callbacks.observe_gdre_done!(observer)
    end
    sol = DRESolution(Xs, Ks, t)
    stats && adaptive !== nothing ? (sol, (accepted = counts[1], rejected = counts[2], err = errs[1:nt-1])) : sol
end

"eigen(Symmetric(A)) on the device: (values ascending, vectors).  method = :jacobi: whole-device block Jacobi (dre_sym_eig_jacobi; converged when off(A) <= tol ||A||_F, tol = 0: n eps; stats = true adds (sweeps, rounds)); :ql: Householder + implicit QL (dre_sym_eig)."
function sym_eigh(A::AbstractMatrix; method::Symbol=:jacobi, tol::Float64=0.0, stats::Bool=false, ctx::Context=default_context())
    size(A, 1) == size(A, 2) || throw(ArgumentError("sym_eigh: a square matrix is expected"))
    method in (:jacobi, :ql) || throw(ArgumentError("sym_eigh: method must be :jacobi or :ql"))
    Ad = upload(ctx, Matrix{Float64}(A))
    w, V = Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(C_NULL)
    ii = zeros(Int64, 2)
    if method === :jacobi
        chk(ctx, ccall((:dre_sym_eig_jacobi, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ptr{Int64}), ctx.ptr, Ad.ptr, tol, w, V, ii))
    else
        chk(ctx, ccall((:dre_sym_eig, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}), ctx.ptr, Ad.ptr, 4.0, w, V))
    end
    vals, vecs = vec(download(ctx, w[])), download(ctx, V[])
    stats ? (vals, vecs, (sweeps = ii[1], rounds = ii[2])) : (vals, vecs)
end

export Context, Pencil, LDLᵀ, lowrank, compress!, compress_fast!, concatenate!, residual, lyapunov_apply, ADI, Shifts, Callbacks, GALEProblem, GDREProblem, DRESolution, Ros1, Ros2,
       Ros3, Ros4, MatrixSign, StepControl, FactoredSign, SignFactorization, solve_lr, solve_dense, DenseGAREProblem, Doubling, DenseGDALEProblem, DenseGDAREProblem, solve_gdare_pair, LowRankUpdate, lr_update, ADISolver, isdone, solve, sym_eigh

end # module

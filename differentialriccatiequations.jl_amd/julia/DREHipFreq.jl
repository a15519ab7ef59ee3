# Frequency response of dense descriptor systems, batched by frequency (included by DREHip.jl, inside module DREHip; dre_version >= 112; the complex
# points at the end: dre_version >= 115).
# H(iω) = C (iωE - A)⁻¹ B for K frequencies in shared launches; a frequency's result is bit for bit independent of the others and of the chunk.

"""H(iω_k) = C (iω_k E - A)⁻¹ B + D at every frequency of omega on the device (dre_freq_response): a complex array q x m x K.  Per frequency the
real form [[-A, -ωE], [ωE, -A]] is inverted with the register panel (2n <= 4096, 16 n³ flops); E may be singular.  A frequency on a pole fails
alone: its slice is NaN and `errors[k]` holds its DREError (`nothing` otherwise).  chunk = 0: as many frequencies per chunk as fit.
method = :complex evaluates `transfer_function` at s = iω instead (the complex Gauss-Jordan panel: n <= 4096, 8 n³ flops); the two agree to
rounding.  Returns (H, errors, (chunk, chunks))."""
function freq_response(E, A, B::AbstractMatrix, C::AbstractMatrix, omega::AbstractVector{<:Real}; D=nothing, chunk::Int=0, ctx::Context=default_context(),
                       method::Symbol=:embedding)
    method in (:embedding, :complex) || throw(ArgumentError("freq_response: method must be :embedding or :complex"))
    method == :complex && return transfer_function(E, A, B, C, complex.(0.0, Vector{Float64}(omega)); D = D, chunk = chunk, ctx = ctx)
    n = size(E, 1)
    (size(E) == (n, n) && size(A) == (n, n) && size(B, 1) == n && size(C, 2) == n) ||
        throw(ArgumentError("freq_response: E and A must be n x n, B n x m and C q x n"))
    K, m, q = length(omega), size(B, 2), size(C, 1)
    (K >= 1 && all(isfinite, omega)) || throw(ArgumentError("freq_response: at least one frequency, all finite"))
    d = [upload(ctx, Matrix{Float64}(M)) for M in (dense_operator(E), dense_operator(A), B, C)]
    w = Vector{Float64}(omega)
    re, im = zeros(q * m * K), zeros(q * m * K)
    status, info = zeros(Int32, K), zeros(Int64, 2)
    GC.@preserve d chk(ctx, ccall((:dre_freq_response, LIB), Cint,
                                  (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}),
                                  ctx.ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, K, w, chunk, re, im, status, info))
    H = reshape(complex.(re, im), q, m, K)
    D === nothing || (H = H .+ D)
    errs = Any[status[k] == 0 ? nothing : DREError(status[k], member_error(ctx, k - 1)) for k in 1:K]
    (H, errs, (chunk = info[1], chunks = info[2]))
end

"freq_response for systems (E, A, B, C) of one (n, m, q) in one call (dre_freq_response_batched): H of size q x m x K x nsys, errors K x nsys"
function freq_response_batch(systems::AbstractVector, omega::AbstractVector{<:Real}; chunk::Int=0, ctx::Context=default_context(), method::Symbol=:embedding)
    method in (:embedding, :complex) || throw(ArgumentError("freq_response_batch: method must be :embedding or :complex"))
    method == :complex && return transfer_function_batch(systems, complex.(0.0, Vector{Float64}(omega)); chunk = chunk, ctx = ctx)
    ns, K = length(systems), length(omega)
    (ns >= 1 && K >= 1 && all(isfinite, omega)) || throw(ArgumentError("freq_response_batch: at least one system and one frequency, all finite"))
    d = [[upload(ctx, Matrix{Float64}(M)) for M in (dense_operator(s[1]), dense_operator(s[2]), s[3], s[4])] for s in systems]
    h = [Ptr{Cvoid}[x[j].ptr for x in d] for j in 1:4]
    m, q = size(systems[1][3], 2), size(systems[1][4], 1)
    w = Vector{Float64}(omega)
    re, im = zeros(q * m * K * ns), zeros(q * m * K * ns)
    status, info = zeros(Int32, K * ns), zeros(Int64, 2)
    GC.@preserve d chk(ctx, ccall((:dre_freq_response_batched, LIB), Cint,
                                  (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Ptr{Float64}, Cint, Ptr{Float64},
                                   Ptr{Float64}, Ptr{Int32}, Ptr{Int64}),
                                  ctx.ptr, ns, h[1], h[2], h[3], h[4], K, w, chunk, re, im, status, info))
    errs = Any[status[g] == 0 ? nothing : DREError(status[g], member_error(ctx, g - 1)) for g in 1:K * ns]
    (reshape(complex.(re, im), q, m, K, ns), reshape(errs, K, ns), (chunk = info[1], chunks = info[2]))
end

"singular values of H(iω_k), descending: min(q, m) x K (the K small SVDs run on the host); NaN for a failed frequency"
function sigma_response(E, A, B, C, omega; kw...)
    H, errs, info = freq_response(E, A, B, C, omega; kw...)
    S = fill(NaN, min(size(H, 1), size(H, 2)), size(H, 3))
    for k in axes(H, 3)
        errs[k] === nothing && (S[:, k] = svdvals(H[:, :, k]))
    end
    (S, errs, info)
end

"H_r(iω) of a ReducedModel (E_r = I)"
freq_response(rom::ReducedModel, omega::AbstractVector{<:Real}; kw...) =
    freq_response(Matrix{Float64}(I, size(rom.Ar)...), rom.Ar, rom.Br, rom.Cr, omega; kw...)

"max_k ‖H(iω_k) - H_r(iω_k)‖₂ against the a-priori bound 2 Σ_{i>r} σ_i: (max_error, omega_at_max, bound, ratio)"
function bt_error(E, A, B, C, rom::ReducedModel, omega::AbstractVector{<:Real}; ctx::Context=default_context(), method::Symbol=:embedding)
    H, _, _ = freq_response(E, A, B, C, omega; ctx = ctx, method = method)
    Hr, _, _ = freq_response(rom, omega; ctx = ctx, method = method)
    err = [opnorm(H[:, :, k] - Hr[:, :, k]) for k in eachindex(omega)]
    k = argmax(err)
    bound = 2 * sum(reverse(rom.hsv[size(rom.Ar, 1) + 1:end]))
    (max_error = err[k], omega_at_max = omega[k], bound = bound, ratio = bound / err[k])
end

# ---- complex points (dre_version >= 115) ---------------- ----------------------------------------------------------------------
"""H(s_k) = C (s_k E - A)⁻¹ B + D at every complex point of s on the device (dre_transfer_eval): a complex array q x m x K.  Per point the planes
of s E - A are inverted with the complex Gauss-Jordan panel (n <= 4096, 8 n³ flops); E may be singular.  A point on a pole fails alone, as in
`freq_response`.  Returns (H, errors, (chunk, chunks))."""
function transfer_function(E, A, B::AbstractMatrix, C::AbstractMatrix, s::AbstractVector{<:Number}; D=nothing, chunk::Int=0, ctx::Context=default_context())
    n = size(E, 1)
    (size(E) == (n, n) && size(A) == (n, n) && size(B, 1) == n && size(C, 2) == n) ||
        throw(ArgumentError("transfer_function: E and A must be n x n, B n x m and C q x n"))
    K, m, q = length(s), size(B, 2), size(C, 1)
    (K >= 1 && all(isfinite, s)) || throw(ArgumentError("transfer_function: at least one point, all finite"))
    d = [upload(ctx, Matrix{Float64}(M)) for M in (dense_operator(E), dense_operator(A), B, C)]
    sr, si = Vector{Float64}(real.(s)), Vector{Float64}(imag.(s))
    re, im = zeros(q * m * K), zeros(q * m * K)
    status, info = zeros(Int32, K), zeros(Int64, 2)
    GC.@preserve d chk(ctx, ccall((:dre_transfer_eval, LIB), Cint,
                                  (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64},
                                   Ptr{Int32}, Ptr{Int64}),
                                  ctx.ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, K, sr, si, chunk, re, im, status, info))
    H = reshape(complex.(re, im), q, m, K)
    D === nothing || (H = H .+ D)
    errs = Any[status[k] == 0 ? nothing : DREError(status[k], member_error(ctx, k - 1)) for k in 1:K]
    (H, errs, (chunk = info[1], chunks = info[2]))
end

"transfer_function for systems (E, A, B, C) of one (n, m, q) in one call (dre_transfer_eval_batched): H of size q x m x K x nsys, errors K x nsys"
function transfer_function_batch(systems::AbstractVector, s::AbstractVector{<:Number}; chunk::Int=0, ctx::Context=default_context())
    ns, K = length(systems), length(s)
    (ns >= 1 && K >= 1 && all(isfinite, s)) || throw(ArgumentError("transfer_function_batch: at least one system and one point, all finite"))
    d = [[upload(ctx, Matrix{Float64}(M)) for M in (dense_operator(t[1]), dense_operator(t[2]), t[3], t[4])] for t in systems]
    h = [Ptr{Cvoid}[x[j].ptr for x in d] for j in 1:4]
    m, q = size(systems[1][3], 2), size(systems[1][4], 1)
    sr, si = Vector{Float64}(real.(s)), Vector{Float64}(imag.(s))
    re, im = zeros(q * m * K * ns), zeros(q * m * K * ns)
    status, info = zeros(Int32, K * ns), zeros(Int64, 2)
    GC.@preserve d chk(ctx, ccall((:dre_transfer_eval_batched, LIB), Cint,
                                  (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Ptr{Float64}, Ptr{Float64}, Cint,
                                   Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}),
                                  ctx.ptr, ns, h[1], h[2], h[3], h[4], K, sr, si, chunk, re, im, status, info))
    errs = Any[status[g] == 0 ? nothing : DREError(status[g], member_error(ctx, g - 1)) for g in 1:K * ns]
    (reshape(complex.(re, im), q, m, K, ns), reshape(errs, K, ns), (chunk = info[1], chunks = info[2]))
end

export freq_response, freq_response_batch, sigma_response, bt_error, transfer_function, transfer_function_batch

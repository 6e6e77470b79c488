# Julia @ccall binding of libyfm_hip.so (include/yfm.h). Not executable in this image (no julia).
# See INTEGRATION.md for the drop-in get_loss / predict / get_loss_array / estimate_steps! methods.
module YFMAMD
const LIB = get(ENV, "YFM_LIB", joinpath(@__DIR__, "..", "yfm_amd", "libyfm_hip.so"))

const YFM_MODEL_DNS, YFM_MODEL_TVL, YFM_MODEL_GNS5 = Cint(0), Cint(1), Cint(2)
# the static and score-driven λ models of src/models/filter.jl:52-110 (7 is not a kind)
const YFM_MODEL_NS, YFM_MODEL_SD_NS, YFM_MODEL_RWSD_NS, YFM_MODEL_SSD_NS, YFM_MODEL_SRWSD_NS =
    Cint(3), Cint(4), Cint(5), Cint(6), Cint(8)
# the neural Nelson–Siegel models (ABI 5): static, and score-driven = YFM_MODEL_SD_NNS | dynamics | flags with
# dynamics 0 "scalar", 1 "block_diag", 2 "diag"
const YFM_MODEL_NNS, YFM_MODEL_NNS_ANCHORED, YFM_MODEL_SD_NNS = Cint(16), Cint(17), Cint(32)
const YFM_NNS_RW, YFM_NNS_SCALED, YFM_NNS_ANCHORED = Cint(4), Cint(8), Cint(16)
const UNCONSTRAINED, CONSTRAINED = Cint(0), Cint(1)
const PREC_CERTIFIED, PREC_FP64 = Cint(0), Cint(1)     # TVλ arithmetic (yfm_set_precision)

struct YFMError <: Exception; code::Cint; msg::String; end
check(rc) = rc == 0 || throw(YFMError(rc, unsafe_string(@ccall LIB.yfm_last_error()::Cstring)))

mutable struct Context
    ptr::Ptr{Cvoid}
    # The panel last uploaded, held by reference: identity (===) then means "this very array",
    # and holding it keeps the GC from freeing it and handing its address to a later slice
    # (an objectid comparison could match a new array at a reused address).  A panel changed
    # IN PLACE still compares equal: call set_panel! explicitly after mutating it.
    panel::Union{Nothing,Matrix{Float64}}
    maturities::Vector{Float64}
    function Context(device::Integer = 0)
        p = @ccall LIB.yfm_create(Cint(device)::Cint)::Ptr{Cvoid}
        p == C_NULL && throw(YFMError(-2, unsafe_string(@ccall LIB.yfm_last_error()::Cstring)))
        ctx = new(p, nothing, Float64[])
        finalizer(c -> @ccall(LIB.yfm_destroy(c.ptr::Ptr{Cvoid})::Cvoid), ctx)
    end
end
const CTX = Ref{Context}()
ctx() = isassigned(CTX) ? CTX[] : (CTX[] = Context(0))

function set_panel!(c::Context, data::Matrix{Float64}, maturities::Vector{Float64})
    N, T = size(data)                       # N×T column-major, as load_data returns it
    GC.@preserve data maturities check(@ccall LIB.yfm_set_panel(c.ptr::Ptr{Cvoid}, data::Ptr{Cdouble},
        Cint(N)::Cint, Cint(T)::Cint, maturities::Ptr{Cdouble})::Cint)
    c.panel = data
    c.maturities = copy(maturities)
    c
end

function ensure_panel!(model, data::Matrix{Float64})
    c = ctx()
    m = Vector{Float64}(model.base.maturities)
    (c.panel === data && c.maturities == m) || set_panel!(c, data, m)
    c
end

"Select the TVλ arithmetic: PREC_CERTIFIED (default, double-double) or PREC_FP64."
set_precision!(mode::Integer; c::Context = ctx()) = check(@ccall LIB.yfm_set_precision(c.ptr::Ptr{Cvoid},
                                                                                      Cint(mode)::Cint)::Cint)

"A P×B matrix in page-locked host memory (yfm_alloc_host): θ batches built in it reach the GPU by DMA."
function pinned_matrix(P::Integer, B::Integer)
    p = @ccall LIB.yfm_alloc_host((P * B * sizeof(Float64))::Csize_t)::Ptr{Cvoid}
    p == C_NULL && throw(YFMError(-2, unsafe_string(@ccall LIB.yfm_last_error()::Cstring)))
    A = unsafe_wrap(Array, Ptr{Float64}(p), (P, B); own = false)
    finalizer(_ -> @ccall(LIB.yfm_free_host(p::Ptr{Cvoid})::Cint), A)
    A
end

kind(::YieldFactorModels.AbstractDNSModel) = YFM_MODEL_DNS
kind(::YieldFactorModels.AbstractTVλDNSModel) = YFM_MODEL_TVL
kind(::YieldFactorModels.AbstractStaticλModel) = YFM_MODEL_NS
# MSEDλModel: random walk ⇔ no B (mselambda.jl:20-27), scale_grad (msebasemodel.jl:45)
kind(m::YieldFactorModels.AbstractλMSEDrivenModel) =
    isempty(m.base.B) ? (m.base.scale_grad ? YFM_MODEL_SRWSD_NS : YFM_MODEL_RWSD_NS) :
                        (m.base.scale_grad ? YFM_MODEL_SSD_NS : YFM_MODEL_SD_NS)
kind(m::YieldFactorModels.AbstractStaticNeuralModel) = m.transform_bool ? YFM_MODEL_NNS : YFM_MODEL_NNS_ANCHORED
# MSEDNeuralModel: the duplicator's largest entry tells the dynamics (2 scalar, 6 block_diag, 18 diag; mseneural.jl:33-48)
kind(m::YieldFactorModels.AbstractNeuralMSEDrivenModel) =
    YFM_MODEL_SD_NNS | Cint(maximum(m.base.duplicator) == 2 ? 0 : maximum(m.base.duplicator) == 6 ? 1 : 2) |
    (isempty(m.base.B) ? YFM_NNS_RW : Cint(0)) | (m.base.scale_grad ? YFM_NNS_SCALED : Cint(0)) |
    (m.transform_bool ? Cint(0) : YFM_NNS_ANCHORED)
tuse_ptr(T_use) = T_use === nothing ? C_NULL : pointer(T_use)

"Batched loglik: Θ is P×B (one candidate per column).  space: UNCONSTRAINED (compute_loss input) or CONSTRAINED (set_params! input)."
function loglik_batch(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                      T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    out = Vector{Float64}(undef, B)
    GC.@preserve Θ out T_use check(@ccall LIB.yfm_loglik_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint, space::Cint,
        Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, out::Ptr{Cdouble})::Cint)
    out                                        # +loglik per column; -Inf / NaN as documented in yfm.h
end

"Batched loglik and its gradient (DNS, N ≤ 64): (ll[B], grad[P, B]), grad[:, b] = ∂(+loglik)/∂Θ[:, b] in `space` —
what estimate!'s TwiceDifferentiable(...; autodiff=:forward) evaluates (optimization.jl:367), with get_loss's sign.
NaN gradient columns where ll is -Inf / NaN or the candidate ran on the double-double path (yfm.h)."
function loglik_grad_batch(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                           T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    ll, grad = Vector{Float64}(undef, B), Matrix{Float64}(undef, P, B)
    GC.@preserve Θ ll grad T_use check(@ccall LIB.yfm_loglik_grad_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, ll::Ptr{Cdouble},
        grad::Ptr{Cdouble})::Cint)
    ll, grad
end

"Fixed-interval Kalman smoother of the fixed-loading models (DNS, GNS5; N ≤ 64) — an extension, predict returns the
forecasts a_{t+1|t} only: (β̂[M, T, B], V[M, M, T, B], C[M, M, T-1, B]) with β̂[:, t, b] = E[β_t | y_1..n],
V its covariance and C[:, :, t, b] = Cov(β_{t+1}, β_t | y_1..n), n = T_use[b] (nothing: every column).  NaN beyond a
window and for a candidate without states (ll -Inf / NaN, the double-double path, a non-finite output: yfm.h; counted
by yfm_last_batch_grad_unavailable).  lag_one = false skips C (returned as nothing)."
function smooth(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = CONSTRAINED,
                T_use::Union{Nothing,Vector{Cint}} = nothing, lag_one::Bool = true)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    M, T = Int(@ccall LIB.yfm_state_dim(kind(model)::Cint)::Cint), size(data, 2)
    βs, V = Array{Float64}(undef, M, T, B), Array{Float64}(undef, M, M, T, B)
    C = lag_one ? Array{Float64}(undef, M, M, max(T - 1, 0), B) : nothing
    GC.@preserve Θ βs V C T_use check(@ccall LIB.yfm_smooth_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint, space::Cint,
        Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, βs::Ptr{Cdouble}, V::Ptr{Cdouble},
        (lag_one ? pointer(C) : Ptr{Cdouble}(C_NULL))::Ptr{Cdouble})::Cint)
    βs, V, C
end

"Extended Kalman smoother of the TVλ model — an extension, linearised once at the forward pass's predicted states:
(β̂[4, T, B], V[4, 4, T, B], C[4, 4, T-1, B]) as `smooth` returns them, so λ̂[t, b] = 0.01 + exp(β̂[4, t, b]) is the decay
path given all the data.  NaN beyond a window and for an unavailable candidate (ll -Inf / NaN, a data column with
det(σ²I + P_tG_t) ≤ 0, a non-finite output: yfm.h; counted by yfm_last_batch_grad_unavailable).  lag_one = false skips C."
function tvl_smooth(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = CONSTRAINED,
                    T_use::Union{Nothing,Vector{Cint}} = nothing, lag_one::Bool = true)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    M, T = 4, size(data, 2)
    βs, V = Array{Float64}(undef, M, T, B), Array{Float64}(undef, M, M, T, B)
    C = lag_one ? Array{Float64}(undef, M, M, max(T - 1, 0), B) : nothing
    GC.@preserve Θ βs V C T_use check(@ccall LIB.yfm_tvl_smooth_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, βs::Ptr{Cdouble},
        V::Ptr{Cdouble}, (lag_one ? pointer(C) : Ptr{Cdouble}(C_NULL))::Ptr{Cdouble})::Cint)
    βs, V, C
end

"TVλ loglik and its score series — an extension, the reference's estimate! returns no covariance: (ll[B],
S[31, T-1, B]) with S[d, k, b] = ∂ℓ_k/∂Θ[d, b] in `space`, ℓ_k the term get_loss adds after column k (0-based slot k + 1
here): exact zeros outside a window's accumulated columns, sum(S, dims = 2) the gradient of tvl_loglik_grad_batch up to
the order of the sum.  NaN in all of a candidate without a gradient (yfm.h; counted by
yfm_last_batch_grad_unavailable).  TVλ only."
function tvl_loglik_scores(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                           T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    ll, S = Vector{Float64}(undef, B), Array{Float64}(undef, P, max(size(data, 2) - 1, 0), B)
    GC.@preserve Θ ll S T_use check(@ccall LIB.yfm_tvl_loglik_scores_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, ll::Ptr{Cdouble},
        S::Ptr{Cdouble})::Cint)
    ll, S
end

"TVλ information matrices — an extension: (ll[B], grad[31, B], H[31, 31, B], J[31, 31, B]) with ll and grad those of
tvl_loglik_grad_batch bit for bit, H = ∂²ll/∂Θ∂Θ' by fourth-order central differences of the exact gradient (step ≤ 0: the
library's default) and J = Γ₀ + Σ_ℓ (1 − ℓ/(lags+1))(Γ_ℓ + Γ_ℓ') of the score series.  hessian = false or opg = false skips
that half (returned as nothing; not both).  NaN matrices for a candidate without a gradient, a NaN H where one of its
124 perturbed points has none (yfm.h; yfm_last_batch_grad_unavailable counts the NaN H).  TVλ only."
function tvl_loglik_info(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                         T_use::Union{Nothing,Vector{Cint}} = nothing, lags::Integer = 0, step::Real = 0.0,
                         hessian::Bool = true, opg::Bool = true)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    ll, grad = Vector{Float64}(undef, B), Matrix{Float64}(undef, P, B)
    H = hessian ? Array{Float64}(undef, P, P, B) : nothing
    J = opg ? Array{Float64}(undef, P, P, B) : nothing
    GC.@preserve Θ ll grad H J T_use check(@ccall LIB.yfm_tvl_loglik_info_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, Cint(lags)::Cint,
        Float64(step)::Cdouble, ll::Ptr{Cdouble}, grad::Ptr{Cdouble},
        (hessian ? pointer(H) : Ptr{Cdouble}(C_NULL))::Ptr{Cdouble},
        (opg ? pointer(J) : Ptr{Cdouble}(C_NULL))::Ptr{Cdouble})::Cint)
    ll, grad, H, J
end

"TVλ loglik and its gradient: (ll[B], grad[31, B]), grad[:, b] = ∂(+loglik)/∂Θ[:, b] in `space` — estimate!'s
ForwardDiff gradient (optimization.jl:367, :10-23) of the EKF of filter.jl:12-80.  ll is bitwise loglik_batch's under the
context's precision; the gradient is the FP64 tangent recursion.  NaN gradient columns where ll is -Inf / NaN or the
recursion's own value or tangents are not usable (yfm.h; counted by yfm_last_batch_grad_unavailable).  TVλ only."
function tvl_loglik_grad_batch(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                               T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    ll, grad = Vector{Float64}(undef, B), Matrix{Float64}(undef, P, B)
    GC.@preserve Θ ll grad T_use check(@ccall LIB.yfm_tvl_loglik_grad_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, ll::Ptr{Cdouble},
        grad::Ptr{Cdouble})::Cint)
    ll, grad
end

"The λ models' loss and its gradient over parameter group \"2\" (optimization.jl:442-479): (loss[B], grad[12, B]),
loss bitwise loglik_batch's (get_loss, filter.jl:209-243), grad[:, b] = ∂(+get_loss)/∂(δ, vec Φ) of Θ[:, b] in `space`
— the rows are Θ's last 12.  NaN gradient columns where the loss is -Inf.  NS, SD-NS, RWSD-NS, SSD-NS, SRWSD-NS only."
function lambda_loss_grad_batch(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                                T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    loss, grad = Vector{Float64}(undef, B), Matrix{Float64}(undef, 12, B)
    GC.@preserve Θ loss grad T_use check(@ccall LIB.yfm_lambda_loss_grad_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, loss::Ptr{Cdouble},
        grad::Ptr{Cdouble})::Cint)
    loss, grad
end

"The λ models' loss and its gradient over every row of Θ — estimate!'s value and gradient (optimization.jl:329-410,
:367) for these kinds: (loss[B], grad[P, B]), loss bitwise loglik_batch's (get_loss, filter.jl:209-243), grad[:, b] =
∂(+get_loss)/∂Θ[:, b] in `space`.  The leading rows (A, B, ω; γ for NS) come from a forward tangent through the score
recursion — the derivative of the function get_loss computes, not the reference's dual-number path (filter.jl:175
strips β's tangent); the last 12 rows are lambda_loss_grad_batch's bit for bit.  NaN gradient columns where the loss is
-Inf or a tangent is not finite (yfm.h; the second counted by yfm_last_batch_grad_unavailable).  NS, SD-NS, RWSD-NS,
SSD-NS, SRWSD-NS only; binds yfm_lambda_loss_fullgrad_batch."
function lambda_loss_fullgrad_batch(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                                    T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    loss, grad = Vector{Float64}(undef, B), Matrix{Float64}(undef, P, B)
    GC.@preserve Θ loss grad T_use check(@ccall LIB.yfm_lambda_loss_fullgrad_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, loss::Ptr{Cdouble},
        grad::Ptr{Cdouble})::Cint)
    loss, grad
end

"The same for the neural models (NNS, NNS-Anchored and the score-driven NNS kinds): (loss[B], grad[12, B]) with
lambda_loss_grad_batch's layout, spaces and NaN columns; binds yfm_neural_loss_grad_batch."
function neural_loss_grad_batch(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                                T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    loss, grad = Vector{Float64}(undef, B), Matrix{Float64}(undef, 12, B)
    GC.@preserve Θ loss grad T_use check(@ccall LIB.yfm_neural_loss_grad_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, loss::Ptr{Cdouble},
        grad::Ptr{Cdouble})::Cint)
    loss, grad
end

"The neural models' loss and its gradient over every row of Θ: (loss[B], grad[P, B]) with lambda_loss_fullgrad_batch's
layout, spaces and NaN columns.  The leading rows (A, B, ω; γ for the static kinds) come from an adjoint sweep over the
score recursion — the derivative of the function get_loss computes; the last 12 rows are neural_loss_grad_batch's bit
for bit (yfm.h).  Binds yfm_neural_loss_fullgrad_batch."
function neural_loss_fullgrad_batch(model, data::Matrix{Float64}, Θ::Matrix{Float64}; space = UNCONSTRAINED,
                                    T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θ)
    loss, grad = Vector{Float64}(undef, B), Matrix{Float64}(undef, P, B)
    GC.@preserve Θ loss grad T_use check(@ccall LIB.yfm_neural_loss_fullgrad_batch(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        space::Cint, Θ::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, loss::Ptr{Cdouble},
        grad::Ptr{Cdouble})::Cint)
    loss, grad
end

"One Optim.NelderMead run (opt1, optimization.jl:442-451) per column of p (P×R, unconstrained) on the coordinates
`inds` (1-based, as findall(param_groups .== g) gives them, optimization.jl:229), the others held: what estimate_steps!
does for one NelderMead group of one group iteration (:218-247), all chains sharing one launch per round.  Returns
(p with the block at Optim's minimizer, f[R] = compute_loss there, n_evals)."
function nm_block(model, data::Matrix{Float64}, p::Matrix{Float64}, inds::Vector{Int}; T_use = nothing,
                  iterations = 500, g_tol = 1e-6)
    c = ensure_panel!(model, data)
    P, R = size(p)
    x, f, nev = copy(p), Vector{Float64}(undef, R), Ref{Clonglong}(0)
    idx = Cint.(inds .- 1)
    GC.@preserve x f idx T_use check(@ccall LIB.yfm_nm_block(c.ptr::Ptr{Cvoid}, kind(model)::Cint, x::Ptr{Cdouble},
        Cint(P)::Cint, Cint(R)::Cint, tuse_ptr(T_use)::Ptr{Cint}, idx::Ptr{Cint}, Cint(length(idx))::Cint,
        Cint(iterations)::Cint, Float64(g_tol)::Cdouble, f::Ptr{Cdouble}, nev::Ptr{Clonglong})::Cint)
    x, f, nev[]
end

"Batched predict (filter.jl:250-282) on hcat(data[:, 1:T_use[b]], NaN × (horizon−1)); arrays get a trailing batch axis."
function predict_batch(model, data::Matrix{Float64}, Θc::Matrix{Float64}; horizon::Integer = 1,
                       T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θc)
    N, T = size(data)
    M = @ccall LIB.yfm_state_dim(kind(model)::Cint)::Cint
    L = @ccall LIB.yfm_gamma_dim(kind(model)::Cint)::Cint
    ncol = T + horizon - 1
    preds, fl1, fl2 = (Array{Float64}(undef, N, ncol, B) for _ in 1:3)
    factors = Array{Float64}(undef, M, ncol, B)
    states = Array{Float64}(undef, L, ncol, B)
    GC.@preserve Θc T_use preds fl1 fl2 factors states check(@ccall LIB.yfm_predict(c.ptr::Ptr{Cvoid},
        kind(model)::Cint, CONSTRAINED::Cint, Θc::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint},
        Cint(horizon)::Cint, preds::Ptr{Cdouble}, factors::Ptr{Cdouble}, states::Ptr{Cdouble}, fl1::Ptr{Cdouble},
        fl2::Ptr{Cdouble})::Cint)
    (preds = preds, factors = factors, states = states, factor_loadings_1 = fl1, factor_loadings_2 = fl2)
end

"get_loss_array (filter.jl:211-247) per column of Θc: (T−1)×B, −Inf rows where the reference returns −Inf."
function loss_array_batch(model, data::Matrix{Float64}, Θc::Matrix{Float64}; K::Integer = 1,
                          T_use::Union{Nothing,Vector{Cint}} = nothing)
    c = ensure_panel!(model, data)
    P, B = size(Θc)
    out = Matrix{Float64}(undef, size(data, 2) - 1, B)
    GC.@preserve Θc T_use out check(@ccall LIB.yfm_loss_array(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        CONSTRAINED::Cint, Θc::Ptr{Cdouble}, Cint(P)::Cint, Cint(B)::Cint, tuse_ptr(T_use)::Ptr{Cint}, Cint(K)::Cint,
        out::Ptr{Cdouble})::Cint)
    out
end

"R estimate_steps! chains (optimization.jl:137-312) batched on the device; starts Θ0c (constrained) on windows T_use."
function estimate_batch(model, data::Matrix{Float64}, Θ0c::Matrix{Float64}; T_use = nothing, iterations = 500,
                        g_tol = 1e-6, max_group_iters = 10, tol = 1e-8)
    c = ensure_panel!(model, data)
    P, R = size(Θ0c)
    θc, p, init = Matrix{Float64}(undef, P, R), Matrix{Float64}(undef, P, R), Matrix{Float64}(undef, P, R)
    ll, status, nev = Vector{Float64}(undef, R), Vector{Cint}(undef, R), Ref{Clonglong}(0)
    GC.@preserve Θ0c T_use θc p init ll status check(@ccall LIB.yfm_estimate(c.ptr::Ptr{Cvoid}, kind(model)::Cint,
        CONSTRAINED::Cint, Θ0c::Ptr{Cdouble}, Cint(P)::Cint, Cint(R)::Cint, tuse_ptr(T_use)::Ptr{Cint},
        Cint(iterations)::Cint, Float64(g_tol)::Cdouble, Cint(max_group_iters)::Cint, Float64(tol)::Cdouble,
        θc::Ptr{Cdouble}, p::Ptr{Cdouble}, init::Ptr{Cdouble}, ll::Ptr{Cdouble}, status::Ptr{Cint},
        nev::Ptr{Clonglong})::Cint)
    (theta_c = θc, p = p, init_c = init, ll = ll, status = status, n_evals = nev[])
end
end # module

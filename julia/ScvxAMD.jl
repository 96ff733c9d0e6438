# ScvxAMD.jl — ccall binding of libscvx_hip.so behind the reference's own API.
#
# NOT EXECUTED IN THE BUILD CONTAINER (no Julia there, SURVEY.md F6): this is the binding a maintainer of
# BenChung/SuccessiveConvexification adds next to master.jl (`include("ScvxAMD.jl")` after master.jl:137-142).
# It keeps RocketlandDefns' types and replaces
#   Dynamics.IntegratorCache (dynamics.jl:258), Dynamics.linearize_dynamics (:321), Dynamics.predict_state (:315),
#   Rocketland.create_initial (rocketland.jl:34), solve_step (:226), solve_problem (:432)
#   FirstRound.solve_initial (initial_solve.jl:17-110): the 3-DoF initialiser, batched on the device
# with calls through include/scvx.h.  The exact ccall sequence, argument types and array layouts used below for the
# reference's recipe (rocketland.jl:26-32, the aero problem) are replayed from C by tests/abi_harness.c on the GPU
# and compared bit for bit with the Python host layer, which binds the identical C signatures.
module ScvxAMD
using ..RocketlandDefns
using LinearAlgebra

const LIB = get(ENV, "SCVX_HIP_LIB", joinpath(@__DIR__, "..", "successiveconvexification_amd", "libscvx_hip.so"))

# struct scvx_problem (include/scvx.h) — field order and types must match exactly (tests check sizeof/offsets with gcc)
struct CProblem
    g::Cdouble; mdry::Cdouble; mwet::Cdouble; Tmin::Cdouble; Tmax::Cdouble
    deltaMax::Cdouble; thetaMax::Cdouble; gammaGs::Cdouble; omMax::Cdouble; dpMax::Cdouble
    jB::NTuple{9,Cdouble}
    alpha::Cdouble; rho::Cdouble; sos::Cdouble
    rTB::NTuple{3,Cdouble}; rFB::NTuple{3,Cdouble}
    rIi::NTuple{3,Cdouble}; rIf::NTuple{3,Cdouble}; vIi::NTuple{3,Cdouble}; vIf::NTuple{3,Cdouble}
    qBIi::NTuple{4,Cdouble}; qBIf::NTuple{4,Cdouble}
    wBi::NTuple{3,Cdouble}; wBf::NTuple{3,Cdouble}
    wNu::Cdouble; wID::Cdouble; wDS::Cdouble; wCst::Cdouble; wTviol::Cdouble; nuTol::Cdouble; delTol::Cdouble; tf_guess::Cdouble
    ri::Cdouble; rh0::Cdouble; rh1::Cdouble; rh2::Cdouble; alph::Cdouble; bet::Cdouble
    force_scalar::Cdouble; length_scalar::Cdouble; finmxf::Cdouble
    K::Int32; imax::Int32; aero_kind::Int32; model_flags::Int32
end

const MODEL_DPMAX = 1   # SCVX_MODEL_DPMAX: enforce 1/2 rho |v|^2 <= dpMax (fields master.jl:27,30; a todo at rocketland.jl:211)
const MODEL_FINS = 2    # SCVX_MODEL_FINS: the fin extension, control_dim = 5 -- the model the reference sketches in comments
                        # (dynamics.jl:60-69, rocketland.jl:203-209) and include/scvx.h defines; LinPoint.control then has 5 entries
const MODEL_AERO_TORQUE = 4   # SCVX_MODEL_AERO_TORQUE: the aerodynamic body torque T(c, M) (v x bv) the reference comments out
                              # (dynamics.jl:69); AtmosphericData only, and the `trq` table of `tables` then reaches the dynamics

t3(v) = (Float64(v[1]), Float64(v[2]), Float64(v[3]))
t4(v) = (Float64(v[1]), Float64(v[2]), Float64(v[3]), Float64(v[4]))

function CProblem(p::DescentProblem; model_flags::Integer=0, finmxf::Real=0.01)   # model_flags: MODEL_DPMAX | MODEL_FINS | MODEL_AERO_TORQUE
    aero = p.aero isa AtmosphericData
    CProblem(p.g, p.mdry, p.mwet, p.Tmin, p.Tmax, p.deltaMax, p.thetaMax, p.gammaGs, p.omMax, p.dpMax,
             Tuple(Float64.(vec(p.jB))), p.alpha, p.rho, p.sos, t3(p.rTB), t3(p.rFB), t3(p.rIi), t3(p.rIf), t3(p.vIi), t3(p.vIf),
             t4(p.qBIi), t4(p.qBIf), t3(p.wBi), t3(p.wBf),
             p.wNu, p.wID, p.wDS, p.wCst, p.wTviol, p.nuTol, p.delTol, p.tf_guess, p.ri, p.rh0, p.rh1, p.rh2, p.alph, p.bet,
             aero ? p.aero.force_scalar : 1.0, aero ? p.aero.length_scalar : 1.0, Float64(finmxf),
             Int32(p.K), Int32(p.imax), Int32(aero ? 1 : 0), Int32(model_flags))
end

# the ABI guard of include/scvx.h (SCVX_ABI_VERSION; sizeof of scvx_problem / scvx_solver_opts / scvx_threedof_opts as the library sees them)
const ABI_VERSION = 4
function check_abi()
    v = Int(ccall((:scvx_abi_version, LIB), Cint, ()))
    sz = zeros(Int32, 3)
    ccall((:scvx_abi_struct_sizes, LIB), Cint, (Ptr{Int32},), sz)
    mine = Int32[sizeof(CProblem), sizeof(SolverOpts), sizeof(ThreedofOpts)]
    (v == ABI_VERSION && sz == mine) || error("libscvx_hip.so: ABI version $v / struct sizes $sz, this binding expects $ABI_VERSION / $mine")
    nothing
end

check(ctx, rc, what) = rc == 0 || error("$what failed ($rc): " * unsafe_string(ccall((:scvx_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))

# ---- IntegratorCache (dynamics.jl:258): owner of the device context -------------------------------------------------
mutable struct Cache
    ctx::Ptr{Cvoid}
    problem::DescentProblem
    nu::Int          # control_dim of the context's model (scvx_control_dim): 3, or 5 with MODEL_FINS
end
control_dim(c::Cache) = c.nu

# The raw table values behind AtmosphericData's interpolation objects (aerodynamics.jl:17-21): the three 181 x 61 grids
# `reshape(col, 181, 61)` of lift_drag.csv, cos(AoA) fastest.  Interpolations.jl keeps the prefiltered coefficients, so
# the shim reads the CSV columns the same way load_aerodata does and applies rescale_aerodata's force scalar through
# the problem struct (force_scalar / length_scalar), exactly as the reference's generated module does.
function upload_aero!(c::Cache, drag::Matrix{Float64}, lift::Matrix{Float64}, trq::Matrix{Float64};
                      aoa0=-1.0, daoa=1 / 90, mach0=0.0, dmach=0.025)
    n_aoa, n_mach = size(drag)
    check(c.ctx, ccall((:scvx_set_aero_table, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble),
        c.ctx, drag, lift, trq, n_aoa, n_mach, aoa0, daoa, mach0, dmach), "scvx_set_aero_table")
    return c
end

# IntegratorCache(prob, info, lin_mod) of the recipe: `info` and the generated module are not needed (the RHS and its
# Jacobians are compiled into the library); `tables` = (drag, lift, trq) raw grids for an AtmosphericData problem.
function Cache(prob::DescentProblem, info=nothing, lin_mod=nothing; device::Int=0, npts::Int=10, tables=nothing,
               model_flags::Integer=0, finmxf::Real=0.01)
    check_abi()   # before the first struct crosses the boundary
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    cp = Ref(CProblem(prob; model_flags=model_flags, finmxf=finmxf))
    rc = ccall((:scvx_ctx_create, LIB), Cint, (Ref{CProblem}, Cint, Ref{Ptr{Cvoid}}), cp, device, ref)
    rc == 0 || error("scvx_ctx_create failed ($rc)")
    c = Cache(ref[], prob, Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), ref[])))
    check(c.ctx, ccall((:scvx_set_nsub, LIB), Cint, (Ptr{Cvoid}, Cint), c.ctx, npts), "scvx_set_nsub")
    if prob.aero isa AtmosphericData
        tables === nothing && error("AtmosphericData problem: pass tables=(drag, lift, trq), the 181x61 grids of lift_drag.csv")
        upload_aero!(c, tables...)
    end
    return c     # release with close(cache) AFTER every Batch made from it (no finalizers: their order is arbitrary)
end
Base.close(c::Cache) = (c.ctx == C_NULL || ccall((:scvx_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.ctx); c.ctx = C_NULL; nothing)
make_dynamics_module(info) = nothing   # dynamics.jl:141: code generation is replaced by the compiled kernels

# Dynamics.linearize_dynamics(states, tf_guess, base_dt, cache) -> Array{LinRes,1}   (dynamics.jl:321-334)
function linearize_dynamics(states::Array{LinPoint,1}, tf_guess::Float64, base_dt::Float64, cache::Cache)
    K = length(states) - 1
    x = hcat((s.state for s in states)...)       # 14 x (K+1), column-major == [K+1][14]
    u = hcat((s.control for s in states)...)     # NU x (K+1)
    size(u, 1) == cache.nu || error("LinPoint.control has $(size(u, 1)) entries, the context's model has control_dim $(cache.nu)")
    endpoint = Matrix{Float64}(undef, 14, K)
    deriv = Array{Float64,3}(undef, 14, 14 + 2 * cache.nu + 1, K)   # column-major 14x21 (14x25) per segment == [K][21][14]
    check(cache.ctx, ccall((:scvx_linearize_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, 1, K, x, u, [tf_guess], base_dt, endpoint, deriv), "scvx_linearize_f64_host")
    return [LinRes(endpoint[:, k], deriv[:, :, k]) for k = 1:K]
end

# Dynamics.predict_state(initial_state, uk, up, sigma, dt, pinfo, cache)   (dynamics.jl:315-317)
function predict_state(initial_state, uk, up, sigma, dt, pinfo, cache::Cache)
    x = hcat(initial_state, zeros(14)); u = hcat(uk, up); out = Matrix{Float64}(undef, 14, 1)
    check(cache.ctx, ccall((:scvx_propagate_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
        cache.ctx, 1, 1, x, u, [Float64(sigma)], dt, out), "scvx_propagate_f64_host")
    return out[:, 1]
end

# ---- the batched iterate --------------------------------------------------------------------------------------------
mutable struct Batch
    h::Ptr{Cvoid}
    cache::Cache
    B::Int
end
Base.close(b::Batch) = (b.h == C_NULL || ccall((:scvx_batch_destroy, LIB), Cvoid, (Ptr{Cvoid},), b.h); b.h = C_NULL; nothing)

# ProblemIteration (master.jl:122-134) with the same field names; `model` holds the device batch instead of MOI handles.
struct Iteration
    problem::DescentProblem
    cache::Cache
    sigma::Float64
    about::Array{LinPoint,1}
    dynam::Array{LinRes,1}
    model::Batch
    iter::Int64
    rk::Float64
    cost::Float64
end

# mixed precision: derivative tiles kept in float (K1 integrates in double, the conic solve stays double)
linearization_f32!(b::Batch, on::Bool=true) =
    (check(b.cache.ctx, ccall((:scvx_batch_set_linearization_f32, LIB), Cint, (Ptr{Cvoid}, Cint), b.h, on ? 1 : 0), "scvx_batch_set_linearization_f32"); b)

# snapshot of trajectory t (1-based) of a batch as the reference's ProblemIteration
function iteration(b::Batch, t::Int=1)
    K = b.cache.problem.K; NU = b.cache.nu; nrec = (K + 1) * (14 + NU) + 1
    rec = Matrix{Float64}(undef, nrec, b.B)
    check(b.cache.ctx, ccall((:scvx_batch_get_trajectory, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), b.h, rec), "scvx_batch_get_trajectory")
    endpoint = Array{Float64,3}(undef, 14, K, b.B); deriv = Array{Float64,4}(undef, 14, 14 + 2NU + 1, K, b.B)
    check(b.cache.ctx, ccall((:scvx_batch_get_linearization, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), b.h, endpoint, deriv), "scvx_batch_get_linearization")
    rk = Vector{Float64}(undef, b.B); cost = Vector{Float64}(undef, b.B); it = Vector{Int32}(undef, b.B)
    check(b.cache.ctx, ccall((:scvx_batch_get_scalars, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}), b.h, rk, cost, it), "scvx_batch_get_scalars")
    x = reshape(rec[1:14(K+1), t], 14, K + 1); u = reshape(rec[14(K+1)+1:(14+NU)*(K+1), t], NU, K + 1)
    Iteration(b.cache.problem, b.cache, rec[end, t],
              [LinPoint(x[:, k], u[:, k]) for k = 1:K+1], [LinRes(endpoint[:, k, t], deriv[:, :, k, t]) for k = 1:K],
              b, it[t], rk[t], cost[t])
end

# create_initial(problem, cache) -> ProblemIteration            (rocketland.jl:34-39); ics: 6 x B = (rIi; vIi) per trajectory
function create_batch(problem::DescentProblem, cache::Cache; ics::Union{Nothing,Matrix{Float64}}=nothing)
    B = ics === nothing ? 1 : size(ics, 2)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(cache.ctx, ccall((:scvx_batch_create, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), cache.ctx, B, ref), "scvx_batch_create")
    b = Batch(ref[], cache, B)
    check(cache.ctx, ccall((:scvx_batch_init, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), b.h, ics === nothing ? C_NULL : ics), "scvx_batch_init")
    return b
end
create_initial(problem::DescentProblem, cache::Cache) = iteration(create_batch(problem, cache))

# What stands behind "the solver reports OPTIMAL" (rocketland.jl:271-276): struct scvx_solver_opts of include/scvx.h, field for field.
struct SolverOpts
    max_iter::Int32; refine::Int32; tol::Cdouble; accept_tol::Cdouble; reuse_inactive_tr::Int32; warm_start::Int32
    retries::Int32; reserved0::Int32
end
# set_solver!(batch; tol = 1e-10, retries = 0, warm_start = false, ...): the defaults of the library for what is not named
# (tol also moves accept_tol, whose default band is empty: OPTIMAL or error, as in the reference)
function set_solver!(batch::Batch; kw...)
    o = Ref(SolverOpts(0, 0, 0.0, 0.0, 0, 0, 0, 0))
    ccall((:scvx_solver_default_opts, LIB), Cint, (Ref{SolverOpts},), o)
    d = Dict(kw)
    tol = get(d, :tol, o[].tol)
    n = SolverOpts(get(d, :max_iter, o[].max_iter), get(d, :refine, o[].refine), tol, get(d, :accept_tol, tol),
                   get(d, :reuse_inactive_tr, false) ? 1 : 0, get(d, :warm_start, o[].warm_start != 0) ? 1 : 0,
                   get(d, :retries, o[].retries), 0)
    check(batch.cache.ctx, ccall((:scvx_batch_set_solver, LIB), Cint, (Ptr{Cvoid}, Ref{SolverOpts}), batch.h, Ref(n)), "scvx_batch_set_solver")
    return batch
end

# FirstRound.solve_initial (initial_solve.jl:17-110): the 3-DoF lossless-convexification landing SOCP, on the device.
struct ThreedofOpts
    max_iter::Int32; refine::Int32; tol::Cdouble; delta::Cdouble; attitude::Int32; reserved::Int32
end
function threedof_opts(; kw...)
    o = Ref(ThreedofOpts(0, 0, 0.0, 0.0, 0, 0))
    ccall((:scvx_threedof_default_opts, LIB), Cint, (Ref{ThreedofOpts},), o)
    d = Dict(kw)
    return ThreedofOpts(get(d, :max_iter, o[].max_iter), get(d, :refine, o[].refine), get(d, :tol, o[].tol), get(d, :delta, o[].delta),
                        get(d, :align_thrust, false) ? 1 : 0, 0)   # align_thrust: rotation_between(e1, +T) instead of the reference's -T
end
# ics: 6 x B = (rIi; vIi) per trajectory.  Returns (sol, status, info): sol is 15 x (K+1) x B in the variable order
# r(3) v(3) ma T(3) ga kaR ar(3) per node plus nkaR (length B); status 0 = optimal, 5 = infeasible; info 5 x B.
function solve_initial_batch(cache::Cache, ics::Matrix{Float64}; kw...)
    B = size(ics, 2); K = Int(cache.problem.K)
    n = ccall((:scvx_threedof_record_doubles, LIB), Int32, (Cint,), K)
    rec = Matrix{Float64}(undef, n, B); st = Vector{Int32}(undef, B); info = Matrix{Float64}(undef, 5, B)
    o = Ref(threedof_opts(; kw...))
    check(cache.ctx, ccall((:scvx_threedof_solve, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ref{ThreedofOpts}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}),
                           cache.ctx, B, ics, o, rec, st, info), "scvx_threedof_solve")
    return reshape(rec[1:end-1, :], 15, K + 1, B), rec[end, :], st, info
end
# create_initial from solve_initial instead of the straight line (initial_solve.jl:90-107): trajectories whose 3-DoF solve is
# not optimal keep the straight-line guess; returns (batch, 3-DoF statuses)
function create_batch_threedof(problem::DescentProblem, cache::Cache; ics::Union{Nothing,Matrix{Float64}}=nothing, kw...)
    B = ics === nothing ? 1 : size(ics, 2)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    check(cache.ctx, ccall((:scvx_batch_create, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), cache.ctx, B, ref), "scvx_batch_create")
    b = Batch(ref[], cache, B)
    st3 = Vector{Int32}(undef, B)
    o = Ref(threedof_opts(; kw...))
    check(cache.ctx, ccall((:scvx_batch_init_threedof, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{ThreedofOpts}, Ptr{Int32}),
                           b.h, ics === nothing ? C_NULL : ics, o, st3), "scvx_batch_init_threedof")
    return b, st3
end
# solve_initial(prob) -> (initial_points, linearisation), as the reference's commented-out function returns them
function solve_initial(problem::DescentProblem, cache::Cache; kw...)
    b, st3 = create_batch_threedof(problem, cache; kw...)
    st3[1] == 0 || error("3-DoF initial solve not optimal (status $(st3[1]))")
    it = iteration(b)
    return it.about, it.dynam
end

const STATUS_NAME = Dict(3 => "SLOW_PROGRESS", 4 => "NUMERICAL_ERROR", 5 => "INFEASIBLE")

# one solve_step of every trajectory of a batch: (status, ||nu||, dJ) vectors
function step!(b::Batch)
    st = Vector{Int32}(undef, b.B); nu = Vector{Float64}(undef, b.B); dj = Vector{Float64}(undef, b.B)
    check(b.cache.ctx, ccall((:scvx_solve_step, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}), b.h, st, nu, dj), "scvx_solve_step")
    return st, nu, dj
end

# solve_step(iteration, cache) -> (ProblemIteration, ||nu||, dJ)     (rocketland.jl:226-321)
function solve_step(iter::Iteration, cache::Cache=iter.cache)
    st, nu, dj = step!(iter.model)
    st[1] in (3, 4, 5) && error("Non-optimal result $(STATUS_NAME[st[1]]) exiting")   # rocketland.jl:273-276
    return iteration(iter.model), nu[1], dj[1]
end

# solve_problem(iprob, cache) -> (ProblemIteration, cnu, cdel)        (rocketland.jl:432-443)
function solve_problem(iprob::DescentProblem, cache::Cache)
    prob = create_initial(iprob, cache)
    cnu = Inf; cdel = Inf; iter = 1
    while (iprob.nuTol < cnu || iprob.delTol < cdel) && iter < iprob.imax
        prob, cnu, cdel = solve_step(prob, cache)
        iter = iter + 1
    end
    return prob, cnu, cdel
end

# batched solve_problem (new): every trajectory until converged, failed or imax; returns (batch, status, iters, nu, dJ)
function solve_batch(iprob::DescentProblem, cache::Cache, ics::Matrix{Float64})
    b = create_batch(iprob, cache; ics=ics)
    st = Vector{Int32}(undef, b.B); it = Vector{Int32}(undef, b.B); nu = Vector{Float64}(undef, b.B); dj = Vector{Float64}(undef, b.B)
    check(cache.ctx, ccall((:scvx_solve, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}), b.h, st, it, nu, dj), "scvx_solve")
    return b, st, it, nu, dj
end

# ---- flight check (new): open-loop rollout of a plan and audit of its path constraints between the nodes ---------------------
# include/scvx.h, "flight check".  The report is 16 x B (column-major == [B][16]); row FLIGHT_* + 1 holds that column.  g <= 0 means
# satisfied.  G_TMIN > 0 between nodes on the bound belongs to the reference's formulation (rocketland.jl:199-201), not to the solver.
const FLIGHT_SHOOT = 0   # SCVX_FLIGHT_SHOOT: single shooting from x[0]
const FLIGHT_PLAN = 1    # SCVX_FLIGHT_PLAN: restart at every planned node
const FLIGHT_NREP = 16   # SCVX_FLIGHT_NREP
const FLIGHT_GAP = 0; const FLIGHT_MISS_R = 1; const FLIGHT_MISS_V = 2; const FLIGHT_MISS_Q = 3; const FLIGHT_MISS_W = 4
const FLIGHT_MASS_END = 5; const FLIGHT_G_MASS = 6; const FLIGHT_G_GLIDE = 7; const FLIGHT_G_TILT = 8; const FLIGHT_G_RATE = 9
const FLIGHT_G_TMAX = 10; const FLIGHT_G_TMIN = 11; const FLIGHT_G_GIMBAL = 12; const FLIGHT_G_DP = 13; const FLIGHT_G_FIN = 14
const FLIGHT_QNORM = 15

# the current accepted iterate of a batch: (report 16 x B, xfly 14 x (K+1) x B or nothing); nsub = 0 takes the context's
function flight_check(b::Batch; nsub::Int=0, mode::Int=FLIGHT_SHOOT, dense::Bool=false)
    K = b.cache.problem.K
    report = Matrix{Float64}(undef, FLIGHT_NREP, b.B)
    xfly = dense ? Array{Float64,3}(undef, 14, K + 1, b.B) : nothing
    check(b.cache.ctx, ccall((:scvx_batch_flight_check, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, nsub, mode, report, dense ? pointer(xfly) : Ptr{Cdouble}(C_NULL)), "scvx_batch_flight_check")
    return report, xfly
end

# any plans: x 14 x (K+1) x B, u NU x (K+1) x B, sigma B (host arrays)
function flight_check(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}; nsub::Int=10,
                      mode::Int=FLIGHT_SHOOT, dense::Bool=false)
    K = size(x, 2) - 1; B = size(x, 3)
    report = Matrix{Float64}(undef, FLIGHT_NREP, B)
    xfly = dense ? Array{Float64,3}(undef, 14, K + 1, B) : nothing
    check(cache.ctx, ccall((:scvx_flight_check_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, sigma, nsub, mode, report, dense ? pointer(xfly) : Ptr{Cdouble}(C_NULL)), "scvx_flight_check_f64_host")
    return report, xfly
end

# the same on device pointers (e.g. AMDGPU.jl ROCArrays), asynchronous on the context's stream; xfly_dev may be C_NULL
flight_check_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble}, nsub::Int, mode::Int,
                  report_dev::Ptr{Cdouble}, xfly_dev::Ptr{Cdouble}) =
    check(cache.ctx, ccall((:scvx_flight_check_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, sigma_dev, nsub, mode, report_dev, xfly_dev), "scvx_flight_check_f64")

# ---- segment audit (new): the PLAN-mode flight check per segment, and back-offs from it ---------------------------------------
# include/scvx.h, "segment audit".  seg is SEG_N x K x B (column-major == [B][K][SEG_N]); the rows, 0-based as in the header:
const SEG_N = 11
const SEG_DEFECT = 0; const SEG_G_MASS = 1; const SEG_G_GLIDE = 2; const SEG_G_TILT = 3; const SEG_G_RATE = 4; const SEG_G_TMAX = 5
const SEG_G_TMIN = 6; const SEG_G_GIMBAL = 7; const SEG_G_DP = 8; const SEG_G_FIN = 9; const SEG_QNORM = 10

# any plans: (seg SEG_N x K x B, the PLAN-mode report 16 x B); nsub = 0 takes the context's
function segment_audit(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}; nsub::Int=0)
    K = size(x, 2) - 1; B = size(x, 3)
    seg = Array{Float64,3}(undef, SEG_N, K, B)
    report = Matrix{Float64}(undef, FLIGHT_NREP, B)
    check(cache.ctx, ccall((:scvx_segment_audit_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, sigma, nsub, seg, report), "scvx_segment_audit_f64_host")
    return seg, report
end

# the current accepted iterate of a batch
function segment_audit(b::Batch; nsub::Int=0)
    seg = Array{Float64,3}(undef, SEG_N, b.cache.problem.K, b.B)
    report = Matrix{Float64}(undef, FLIGHT_NREP, b.B)
    check(b.cache.ctx, ccall((:scvx_batch_segment_audit, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, nsub, seg, report), "scvx_batch_segment_audit")
    return seg, report
end

# the same on device pointers, asynchronous on the context's stream; report_dev may be C_NULL
segment_audit_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble}, nsub::Int,
                   seg_dev::Ptr{Cdouble}, report_dev::Ptr{Cdouble}) =
    check(cache.ctx, ccall((:scvx_segment_audit_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, sigma_dev, nsub, seg_dev, report_dev), "scvx_segment_audit_f64")

# back-offs from the audit of the batch's current accepted iterate, accumulated on what it carries: new = min(old + gain e_k, cap width_k);
# which: MARGIN_THRUST (lo alone) | MARGIN_GLIDE | MARGIN_TILT | MARGIN_RATE (the constants further down; the default is thrust + tilt).  Returns seg, or nothing with seg = false
function margins_from_audit!(b::Batch; which::Integer=0x09, gain::Float64=1.5, tol::Float64=1e-7,
                             cap::Float64=0.25, nsub::Int=0, seg::Bool=true)
    out = seg ? Array{Float64,3}(undef, SEG_N, b.cache.problem.K, b.B) : nothing
    check(b.cache.ctx, ccall((:scvx_batch_audit_margins, LIB), Cint, (Ptr{Cvoid}, Cint, Cuint, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}),
        b.h, nsub, which, gain, tol, cap, seg ? pointer(out) : Ptr{Cdouble}(C_NULL)), "scvx_batch_audit_margins")
    return out
end

# ---- plan tracking (new): time-varying LQR gains about a plan and the closed-loop flight under them ---------------------------
# include/scvx.h, "plan tracking".  gain is n x NU x K x B (column-major == [B][K][NU][n], n = 14 + NU): du_{k+1} = gain[:, :, k, b]' * [dx_k; du_k].
# q, r, qf: diagonal weights (scalars broadcast); 1, 1, 100 is a starting point, not tuning advice.
const TRACK_CLAMP = 1    # SCVX_TRACK_CLAMP: rescale the commanded thrust / fin norms into their bounds
_track_w(v, m::Int) = v isa Real ? fill(Float64(v), m) : (length(v) == m ? Vector{Float64}(v) : error("weight needs $m components"))

# the gains of a batch's current accepted iterate from its own derivative tiles: (gain, p0 n x n x B or nothing)
function track_gains(b::Batch; q=1.0, r=1.0, qf=100.0, cost::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx)); n = 14 + NU
    gain = Array{Float64,4}(undef, n, NU, K, b.B)
    p0 = cost ? Array{Float64,3}(undef, n, n, b.B) : nothing
    check(b.cache.ctx, ccall((:scvx_batch_track_gains, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), gain, cost ? pointer(p0) : Ptr{Cdouble}(C_NULL)), "scvx_batch_track_gains")
    return gain, p0
end

# closed-loop flight of a batch's current accepted iterate from x[0] + dx0 (14 x B or nothing): (report 16 x B, xfly, ufly);
# the report's rows are the flight check's (FLIGHT_* + 1); nsub = 0 takes the context's
function track(b::Batch; dx0::Union{Nothing,Matrix{Float64}}=nothing, q=1.0, r=1.0, qf=100.0, nsub::Int=0, clamp::Bool=false,
               dense::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx))
    dx0 === nothing || size(dx0) == (14, b.B) || error("dx0 must be 14 x B")
    report = Matrix{Float64}(undef, FLIGHT_NREP, b.B)
    xfly = dense ? Array{Float64,3}(undef, 14, K + 1, b.B) : nothing
    ufly = dense ? Array{Float64,3}(undef, NU, K + 1, b.B) : nothing
    check(b.cache.ctx, ccall((:scvx_batch_track_fly, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), dx0 === nothing ? Ptr{Cdouble}(C_NULL) : pointer(dx0), nsub,
        clamp ? TRACK_CLAMP : 0, report, dense ? pointer(xfly) : Ptr{Cdouble}(C_NULL), dense ? pointer(ufly) : Ptr{Cdouble}(C_NULL)),
        "scvx_batch_track_fly")
    return report, xfly, ufly
end

# any plans (host arrays): gains from derivative tiles 14 x (14 + 2 NU + 1) x K x B as linearisation returns them
function track_gains(cache::Cache, deriv::Array{Float64,4}; q=1.0, r=1.0, qf=100.0, cost::Bool=false)
    NU = (size(deriv, 2) - 15) ÷ 2; n = 14 + NU; K = size(deriv, 3); B = size(deriv, 4)
    gain = Array{Float64,4}(undef, n, NU, K, B)
    p0 = cost ? Array{Float64,3}(undef, n, n, B) : nothing
    check(cache.ctx, ccall((:scvx_track_gains_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, deriv, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), gain, cost ? pointer(p0) : Ptr{Cdouble}(C_NULL)),
        "scvx_track_gains_f64_host")
    return gain, p0
end

# x 14 x (K+1) x B, u NU x (K+1) x B, sigma B, gain n x NU x K x B, dx0 14 x B or nothing
function track(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, gain::Array{Float64,4};
               dx0::Union{Nothing,Matrix{Float64}}=nothing, nsub::Int=10, clamp::Bool=false, dense::Bool=false)
    K = size(x, 2) - 1; B = size(x, 3); NU = size(u, 1)
    report = Matrix{Float64}(undef, FLIGHT_NREP, B)
    xfly = dense ? Array{Float64,3}(undef, 14, K + 1, B) : nothing
    ufly = dense ? Array{Float64,3}(undef, NU, K + 1, B) : nothing
    check(cache.ctx, ccall((:scvx_track_fly_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, sigma, gain, dx0 === nothing ? Ptr{Cdouble}(C_NULL) : pointer(dx0), nsub, clamp ? TRACK_CLAMP : 0, report,
        dense ? pointer(xfly) : Ptr{Cdouble}(C_NULL), dense ? pointer(ufly) : Ptr{Cdouble}(C_NULL)), "scvx_track_fly_f64_host")
    return report, xfly, ufly
end

# the same two on device pointers (e.g. AMDGPU.jl ROCArrays), asynchronous on the context's stream; q, r, qf stay host vectors
track_gains_dev!(cache::Cache, B::Int, K::Int, deriv_dev::Ptr{Cdouble}, q::Vector{Float64}, r::Vector{Float64}, qf::Vector{Float64},
                 gain_dev::Ptr{Cdouble}, p0_dev::Ptr{Cdouble}) =
    check(cache.ctx, ccall((:scvx_track_gains_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, deriv_dev, q, r, qf, gain_dev, p0_dev), "scvx_track_gains_f64")
track_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble}, gain_dev::Ptr{Cdouble},
           dx0_dev::Ptr{Cdouble}, nsub::Int, flags::Int, report_dev::Ptr{Cdouble}, xfly_dev::Ptr{Cdouble}, ufly_dev::Ptr{Cdouble}) =
    check(cache.ctx, ccall((:scvx_track_fly_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, sigma_dev, gain_dev, dx0_dev, nsub, flags, report_dev, xfly_dev, ufly_dev), "scvx_track_fly_f64")

# ---- covariance analysis (new): the closed-loop dispersion of a tracked plan, to first order -----------------------------------
# include/scvx.h, "covariance analysis".  S0 is 14 x 14 x B (only its symmetric part is used), w a scalar, 14 values or nothing;
# the report is COV_NREP x B (rows COV_* + 1); dense outputs: sig n x (K+1) x B, covK n x n x B, cov n x n x (K+1) x B.
const COV_NREP = 16   # SCVX_COV_NREP
const COV_SIG_M = 0; const COV_SIG_R = 1; const COV_SIG_V = 2; const COV_SIG_Q = 3; const COV_SIG_W = 4
const COV_ELL_A = 5; const COV_ELL_B = 6; const COV_ELL_ANG = 7; const COV_SIG_PEAK = 8; const COV_S_THRUST = 9
const COV_N_MASS = 10; const COV_N_GLIDE = 11; const COV_N_TILT = 12; const COV_N_RATE = 13; const COV_N_TMAX = 14; const COV_N_TMIN = 15
_cov_opt(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)

# the current accepted iterate of a batch under its own LQR gains: (report, sig, covK, cov)
function covariance(b::Batch, S0::Array{Float64,3}; w=nothing, q=1.0, r=1.0, qf=100.0, dense::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx)); n = 14 + NU
    size(S0) == (14, 14, b.B) || error("S0 must be 14 x 14 x B")
    report = Matrix{Float64}(undef, COV_NREP, b.B)
    sig = dense ? Array{Float64,3}(undef, n, K + 1, b.B) : nothing
    covK = dense ? Array{Float64,3}(undef, n, n, b.B) : nothing
    cov = dense ? Array{Float64,4}(undef, n, n, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv check(b.cache.ctx, ccall((:scvx_batch_cov, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, _cov_opt(wv), report, _cov_opt(sig), _cov_opt(covK), _cov_opt(cov)),
        "scvx_batch_cov")
    return report, sig, covK, cov
end

# any plans (host arrays): x 14 x (K+1) x B, u NU x (K+1) x B, deriv 14 x (14 + 2 NU + 1) x K x B, gain n x NU x K x B, S0 14 x 14 x B
function covariance(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, deriv::Array{Float64,4}, gain::Array{Float64,4},
                    S0::Array{Float64,3}; w=nothing, dense::Bool=false)
    K = size(x, 2) - 1; B = size(x, 3); NU = size(u, 1); n = 14 + NU
    size(S0) == (14, 14, B) || error("S0 must be 14 x 14 x B")
    report = Matrix{Float64}(undef, COV_NREP, B)
    sig = dense ? Array{Float64,3}(undef, n, K + 1, B) : nothing
    covK = dense ? Array{Float64,3}(undef, n, n, B) : nothing
    cov = dense ? Array{Float64,4}(undef, n, n, K + 1, B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv check(cache.ctx, ccall((:scvx_cov_propagate_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, deriv, gain, S0, _cov_opt(wv), report, _cov_opt(sig), _cov_opt(covK), _cov_opt(cov)),
        "scvx_cov_propagate_f64_host")
    return report, sig, covK, cov
end

# the same on device pointers (e.g. AMDGPU.jl ROCArrays), asynchronous on the context's stream; w stays a host vector (or C_NULL)
cov_propagate_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, deriv_dev::Ptr{Cdouble}, gain_dev::Ptr{Cdouble},
                   S0_dev::Ptr{Cdouble}, w::Union{Nothing,Vector{Float64}}, report_dev::Ptr{Cdouble}, sig_dev::Ptr{Cdouble},
                   covK_dev::Ptr{Cdouble}, cov_dev::Ptr{Cdouble}) =
    GC.@preserve w check(cache.ctx, ccall((:scvx_cov_propagate_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, _cov_opt(w), report_dev, sig_dev, covK_dev, cov_dev), "scvx_cov_propagate_f64")

# ---- clamp-aware covariance analysis by statistical linearisation (new) ---------------------------------------------------------
# include/scvx.h, "CLAMP-AWARE covariance analysis": the thrust clamp of the closed-loop flight as a random-input describing function, a
# mean beside the covariance; an approximation.  band = (Tlo, Thi) or nothing (the problem's Tmin, Tmax).  satrep is SAT_NREP x B
# (rows SAT_* + 1); dense outputs: mean n x (K+1) x B, sig, covK, cov as covariance, satk 4 x K x B = (That, s, P_lo, P_hi).
const SAT_NREP = 16   # SCVX_SAT_NREP
const SAT_SIG_M = 0; const SAT_SIG_R = 1; const SAT_SIG_V = 2; const SAT_SIG_Q = 3; const SAT_SIG_W = 4
const SAT_BIAS_M = 5; const SAT_BIAS_R = 6; const SAT_BIAS_V = 7; const SAT_BIAS_Q = 8; const SAT_BIAS_W = 9
const SAT_RMS_R = 10; const SAT_RMS_V = 11; const SAT_P_LO = 12; const SAT_P_HI = 13; const SAT_GAIN_MIN = 14; const SAT_BIAS_PEAK = 15
_cov_band(band) = band === nothing ? nothing : Float64[band[1], band[2]]

# the current accepted iterate of a batch under its own LQR gains: (report, satrep, mean, sig, covK, cov, satk)
function cov_clamp(b::Batch, S0::Array{Float64,3}; w=nothing, band=nothing, q=1.0, r=1.0, qf=100.0, dense::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx)); n = 14 + NU
    size(S0) == (14, 14, b.B) || error("S0 must be 14 x 14 x B")
    report = Matrix{Float64}(undef, COV_NREP, b.B)
    satrep = Matrix{Float64}(undef, SAT_NREP, b.B)
    mean = dense ? Array{Float64,3}(undef, n, K + 1, b.B) : nothing
    sig = dense ? Array{Float64,3}(undef, n, K + 1, b.B) : nothing
    covK = dense ? Array{Float64,3}(undef, n, n, b.B) : nothing
    cov = dense ? Array{Float64,4}(undef, n, n, K + 1, b.B) : nothing
    satk = dense ? Array{Float64,3}(undef, 4, K, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    bd = _cov_band(band)
    GC.@preserve wv bd check(b.cache.ctx, ccall((:scvx_batch_cov_clamp, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, _cov_opt(wv), _cov_opt(bd), report, satrep, _cov_opt(mean),
        _cov_opt(sig), _cov_opt(covK), _cov_opt(cov), _cov_opt(satk)), "scvx_batch_cov_clamp")
    return report, satrep, mean, sig, covK, cov, satk
end

# any plans (host arrays), shapes as covariance(cache, ...)
function cov_clamp(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, deriv::Array{Float64,4}, gain::Array{Float64,4},
                   S0::Array{Float64,3}; w=nothing, band=nothing, dense::Bool=false)
    K = size(x, 2) - 1; B = size(x, 3); NU = size(u, 1); n = 14 + NU
    size(S0) == (14, 14, B) || error("S0 must be 14 x 14 x B")
    report = Matrix{Float64}(undef, COV_NREP, B)
    satrep = Matrix{Float64}(undef, SAT_NREP, B)
    mean = dense ? Array{Float64,3}(undef, n, K + 1, B) : nothing
    sig = dense ? Array{Float64,3}(undef, n, K + 1, B) : nothing
    covK = dense ? Array{Float64,3}(undef, n, n, B) : nothing
    cov = dense ? Array{Float64,4}(undef, n, n, K + 1, B) : nothing
    satk = dense ? Array{Float64,3}(undef, 4, K, B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    bd = _cov_band(band)
    GC.@preserve wv bd check(cache.ctx, ccall((:scvx_cov_clamp_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, deriv, gain, S0, _cov_opt(wv), _cov_opt(bd), report, satrep, _cov_opt(mean), _cov_opt(sig), _cov_opt(covK),
        _cov_opt(cov), _cov_opt(satk)), "scvx_cov_clamp_f64_host")
    return report, satrep, mean, sig, covK, cov, satk
end

# the same on device pointers, asynchronous on the context's stream; w and band stay host vectors (or nothing)
cov_clamp_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, deriv_dev::Ptr{Cdouble}, gain_dev::Ptr{Cdouble},
               S0_dev::Ptr{Cdouble}, w::Union{Nothing,Vector{Float64}}, band::Union{Nothing,Vector{Float64}}, report_dev::Ptr{Cdouble},
               satrep_dev::Ptr{Cdouble}, mean_dev::Ptr{Cdouble}, sig_dev::Ptr{Cdouble}, covK_dev::Ptr{Cdouble}, cov_dev::Ptr{Cdouble},
               satk_dev::Ptr{Cdouble}) =
    GC.@preserve w band check(cache.ctx, ccall((:scvx_cov_clamp_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, _cov_opt(w), _cov_opt(band), report_dev, satrep_dev, mean_dev,
        sig_dev, covK_dev, cov_dev, satk_dev), "scvx_cov_clamp_f64")

# ---- navigation-error (LQG) covariance analysis (new): the closed loop flown on an estimate, to first order --------------------
# include/scvx.h, "navigation-error (LQG) covariance analysis".  S0, N0 are 14 x 14 x B; H is 14 x m (column-major == [m][14]) or
# nothing (no measurement), rm a scalar or m variances; the reports are COV_NREP x B and NAV_NREP x B (rows NAV_* + 1); dense outputs:
# sig n x (K+1) x B, navsig 14 x (K+1) x B, kf m x 14 x K x B, joint N x N x (K+1) x B with N = n + 14.
const NAV_NREP = 8    # SCVX_NAV_NREP
const NAV_M = 0; const NAV_R = 1; const NAV_V = 2; const NAV_Q = 3; const NAV_W = 4; const NAV_PEAK = 5; const NAV_EST_R = 6; const NAV_EST_V = 7

function _nav_model(H, rm)
    H === nothing && return 0, nothing, nothing
    size(H, 1) == 14 || error("H must be 14 x m (one column per measurement)")
    m = size(H, 2)
    return m, Matrix{Float64}(H), _track_w(rm, m)
end

# the current accepted iterate of a batch under its own LQR gains: (report, navrep, sig, navsig, kf, joint)
function navigation(b::Batch, S0::Array{Float64,3}, N0::Array{Float64,3}, H, rm; w=nothing, q=1.0, r=1.0, qf=100.0, dense::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx)); n = 14 + NU; N = n + 14
    (size(S0) == (14, 14, b.B) && size(N0) == (14, 14, b.B)) || error("S0 and N0 must be 14 x 14 x B")
    m, Hm, rmv = _nav_model(H, rm)
    report = Matrix{Float64}(undef, COV_NREP, b.B)
    navrep = Matrix{Float64}(undef, NAV_NREP, b.B)
    sig = dense ? Array{Float64,3}(undef, n, K + 1, b.B) : nothing
    navsig = dense ? Array{Float64,3}(undef, 14, K + 1, b.B) : nothing
    kf = dense && m > 0 ? Array{Float64,4}(undef, m, 14, K, b.B) : nothing
    joint = dense ? Array{Float64,4}(undef, N, N, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv check(b.cache.ctx, ccall((:scvx_batch_nav_cov, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, N0, m, _cov_opt(Hm), _cov_opt(rmv), _cov_opt(wv), report, navrep,
        _cov_opt(sig), _cov_opt(navsig), _cov_opt(kf), _cov_opt(joint)), "scvx_batch_nav_cov")
    return report, navrep, sig, navsig, kf, joint
end

# any plans (host arrays), as covariance(cache, ...)
function navigation(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, deriv::Array{Float64,4}, gain::Array{Float64,4},
                    S0::Array{Float64,3}, N0::Array{Float64,3}, H, rm; w=nothing, dense::Bool=false)
    K = size(x, 2) - 1; B = size(x, 3); NU = size(u, 1); n = 14 + NU; N = n + 14
    (size(S0) == (14, 14, B) && size(N0) == (14, 14, B)) || error("S0 and N0 must be 14 x 14 x B")
    m, Hm, rmv = _nav_model(H, rm)
    report = Matrix{Float64}(undef, COV_NREP, B)
    navrep = Matrix{Float64}(undef, NAV_NREP, B)
    sig = dense ? Array{Float64,3}(undef, n, K + 1, B) : nothing
    navsig = dense ? Array{Float64,3}(undef, 14, K + 1, B) : nothing
    kf = dense && m > 0 ? Array{Float64,4}(undef, m, 14, K, B) : nothing
    joint = dense ? Array{Float64,4}(undef, N, N, K + 1, B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv check(cache.ctx, ccall((:scvx_nav_cov_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, deriv, gain, S0, N0, m, _cov_opt(Hm), _cov_opt(rmv), _cov_opt(wv), report, navrep, _cov_opt(sig),
        _cov_opt(navsig), _cov_opt(kf), _cov_opt(joint)), "scvx_nav_cov_f64_host")
    return report, navrep, sig, navsig, kf, joint
end

# the same on device pointers, asynchronous on the context's stream; H, rm and w stay host arrays (or nothing)
nav_cov_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, deriv_dev::Ptr{Cdouble}, gain_dev::Ptr{Cdouble},
             S0_dev::Ptr{Cdouble}, N0_dev::Ptr{Cdouble}, m::Int, H::Union{Nothing,Matrix{Float64}}, rm::Union{Nothing,Vector{Float64}},
             w::Union{Nothing,Vector{Float64}}, report_dev::Ptr{Cdouble}, navrep_dev::Ptr{Cdouble}, sig_dev::Ptr{Cdouble},
             navsig_dev::Ptr{Cdouble}, kf_dev::Ptr{Cdouble}, joint_dev::Ptr{Cdouble}) =
    GC.@preserve H rm w check(cache.ctx, ccall((:scvx_nav_cov_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, N0_dev, m, _cov_opt(H), _cov_opt(rm), _cov_opt(w), report_dev, navrep_dev,
        sig_dev, navsig_dev, kf_dev, joint_dev), "scvx_nav_cov_f64")

# closed-loop flight with the law fed an estimate: nav 14 x K x B, the estimate's error at node k (zeros: track bit for bit)
function track_nav(b::Batch, nav::Array{Float64,3}; dx0::Union{Nothing,Matrix{Float64}}=nothing, q=1.0, r=1.0, qf=100.0, nsub::Int=0,
                   clamp::Bool=false, dense::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx))
    size(nav) == (14, K, b.B) || error("nav must be 14 x K x B")
    dx0 === nothing || size(dx0) == (14, b.B) || error("dx0 must be 14 x B")
    report = Matrix{Float64}(undef, FLIGHT_NREP, b.B)
    xfly = dense ? Array{Float64,3}(undef, 14, K + 1, b.B) : nothing
    ufly = dense ? Array{Float64,3}(undef, NU, K + 1, b.B) : nothing
    check(b.cache.ctx, ccall((:scvx_batch_track_fly_nav, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), _cov_opt(dx0), nav, nsub, clamp ? TRACK_CLAMP : 0, report, _cov_opt(xfly),
        _cov_opt(ufly)), "scvx_batch_track_fly_nav")
    return report, xfly, ufly
end

function track_nav(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, gain::Array{Float64,4},
                   nav::Array{Float64,3}; dx0::Union{Nothing,Matrix{Float64}}=nothing, nsub::Int=10, clamp::Bool=false, dense::Bool=false)
    K = size(x, 2) - 1; B = size(x, 3); NU = size(u, 1)
    size(nav) == (14, K, B) || error("nav must be 14 x K x B")
    report = Matrix{Float64}(undef, FLIGHT_NREP, B)
    xfly = dense ? Array{Float64,3}(undef, 14, K + 1, B) : nothing
    ufly = dense ? Array{Float64,3}(undef, NU, K + 1, B) : nothing
    check(cache.ctx, ccall((:scvx_track_fly_nav_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, sigma, gain, _cov_opt(dx0), nav, nsub, clamp ? TRACK_CLAMP : 0, report, _cov_opt(xfly), _cov_opt(ufly)),
        "scvx_track_fly_nav_f64_host")
    return report, xfly, ufly
end

track_nav_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble}, gain_dev::Ptr{Cdouble},
               dx0_dev::Ptr{Cdouble}, nav_dev::Ptr{Cdouble}, nsub::Int, flags::Int, report_dev::Ptr{Cdouble}, xfly_dev::Ptr{Cdouble},
               ufly_dev::Ptr{Cdouble}) =
    check(cache.ctx, ccall((:scvx_track_fly_nav_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, sigma_dev, gain_dev, dx0_dev, nav_dev, nsub, flags, report_dev, xfly_dev, ufly_dev),
        "scvx_track_fly_nav_f64")

# ---- sampled closed-loop dispersion (new) --------------------------------------------------------------------------------------
# include/scvx.h, "sampled closed-loop dispersion": S flights per plan under the tracking law, reduced on the device to one row of
# MC_NREP statistics per plan.  C0 14 x 14 x B holds every plan's factor ROW-major as the library reads it (C0[j, i, b] = C[i, j]);
# xi0 14 x S and eta 14 x K x S (or nothing) are standard-normal draws shared by all plans; w the per-segment noise variance.
const MC_NREP = 48
const MC_MAX, MC_MEAN, MC_P_MASS, MC_P_ANY, MC_OUT_LO, MC_OUT_HI, MC_N_BAD, MC_S = 0, 16, 32, 41, 42, 43, 44, 45

function _mc_outputs(B::Int, S::Int, dense::Bool)
    return (Matrix{Float64}(undef, MC_NREP, B), Matrix{Float64}(undef, 14, B), Array{Float64,3}(undef, 14, 14, B),
            dense ? Array{Float64,3}(undef, FLIGHT_NREP, S, B) : nothing, dense ? Array{Float64,3}(undef, 14, S, B) : nothing,
            dense ? Array{Float64,3}(undef, 14, S, B) : nothing)
end

function track_mc(b::Batch, C0::Array{Float64,3}, xi0::Matrix{Float64}; eta::Union{Nothing,Array{Float64,3}}=nothing, w=nothing, q=1.0,
                  r=1.0, qf=100.0, nsub::Int=0, clamp::Bool=false, tol::Float64=0.0, dense::Bool=false)
    NU = control_dim(b.cache)
    S = size(xi0, 2)
    size(C0) == (14, 14, b.B) && size(xi0, 1) == 14 || throw(ArgumentError("C0 must be 14 x 14 x B, xi0 14 x S"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(b.B, S, dense)
    sw = w === nothing ? nothing : sqrt.(_track_w(w, 14))
    GC.@preserve sw check(b.cache.ctx, ccall((:scvx_batch_track_mc, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S, C0, xi0, _cov_opt(eta), _cov_opt(sw), C_NULL, nsub,
        clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0)), "scvx_batch_track_mc")
    return mcrep, xmean, xcov, flights, xland, dx0
end

function track_mc(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, gain::Array{Float64,4},
                  C0::Array{Float64,3}, xi0::Matrix{Float64}; eta::Union{Nothing,Array{Float64,3}}=nothing, w=nothing, nsub::Int=10,
                  clamp::Bool=false, tol::Float64=0.0, dense::Bool=false)
    B, K, S = size(x, 3), size(x, 2) - 1, size(xi0, 2)
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(B, S, dense)
    sw = w === nothing ? nothing : sqrt.(_track_w(w, 14))
    GC.@preserve sw check(cache.ctx, ccall((:scvx_track_mc_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x, u, sigma, gain, C0, xi0, _cov_opt(eta), _cov_opt(sw), C_NULL, nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep,
        xmean, xcov, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0)), "scvx_track_mc_f64_host")
    return mcrep, xmean, xcov, flights, xland, dx0
end

# the same on device pointers, asynchronous on the context's stream; sw = sqrt(w) stays a host array (or nothing)
track_mc_dev!(cache::Cache, B::Int, K::Int, S::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble},
              gain_dev::Ptr{Cdouble}, C0_dev::Ptr{Cdouble}, xi0_dev::Ptr{Cdouble}, eta_dev::Ptr{Cdouble}, sw::Union{Nothing,Vector{Float64}},
              nsub::Int, flags::Int, tol::Float64, mcrep_dev::Ptr{Cdouble}, xmean_dev::Ptr{Cdouble}, xcov_dev::Ptr{Cdouble},
              flights_dev::Ptr{Cdouble}, xland_dev::Ptr{Cdouble}, dx0_dev::Ptr{Cdouble}) =
    GC.@preserve sw check(cache.ctx, ccall((:scvx_track_mc_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, _cov_opt(sw), C_NULL, nsub, flags, tol, mcrep_dev,
        xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev), "scvx_track_mc_f64")

# ---- sampled closed-loop dispersion flown on a navigation estimate (new) ----------------------------------------------------
# include/scvx.h, "sampled closed-loop dispersion flown on a navigation ESTIMATE": track_mc with the law fed x_fly - eps+_k, the error
# eps generated per flight on the device.  Besides track_mc's arguments: N0 14 x 14 x B (batch form: the filter gains come from it), CN
# 14 x 14 x B its factors stored ROW-major like C0, xin 14 x S and nud m x K x S (or nothing with H === nothing) standard-normal draws,
# H 14 x m and rm as navigation(); kf m x 14 x K x B the gains navigation(...; dense=true) returns; w the VARIANCE (the library roots it).
# Returns mcrep, xmean, xcov, jmean 28 x B, jcov 28 x 28 x B, mcnav NAV_NREP x B (row MCNAV_MAX_FED + 1 where navrep has NAV_PEAK),
# and with dense flights, xland, dx0, navfed 14 x K x S x B, navK 14 x S x B.
const MCNAV_MAX_FED = 5   # SCVX_MCNAV_MAX_FED

function _mc_nav_outputs(B::Int, S::Int, K::Int, dense::Bool)
    return (Matrix{Float64}(undef, 28, B), Array{Float64,3}(undef, 28, 28, B), Matrix{Float64}(undef, NAV_NREP, B),
            dense ? Array{Float64,4}(undef, 14, K, S, B) : nothing, dense ? Array{Float64,3}(undef, 14, S, B) : nothing)
end

function track_mc_nav(b::Batch, C0::Array{Float64,3}, xi0::Matrix{Float64}, N0::Array{Float64,3}, CN::Array{Float64,3},
                      xin::Matrix{Float64}, H, rm; nud::Union{Nothing,Array{Float64,3}}=nothing, eta::Union{Nothing,Array{Float64,3}}=nothing,
                      w=nothing, q=1.0, r=1.0, qf=100.0, nsub::Int=0, clamp::Bool=false, tol::Float64=0.0, dense::Bool=false)
    NU = control_dim(b.cache)
    S = size(xi0, 2); K = b.cache.problem.K
    (size(C0) == (14, 14, b.B) && size(N0) == (14, 14, b.B) && size(CN) == (14, 14, b.B) && size(xi0, 1) == 14 && size(xin) == (14, S)) ||
        throw(ArgumentError("C0, N0, CN must be 14 x 14 x B, xi0 and xin 14 x S"))
    m, Hm, rmv = _nav_model(H, rm)
    (m == 0 || (nud !== nothing && size(nud) == (m, K, S))) || throw(ArgumentError("nud must be m x K x S"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(b.B, S, dense)
    jmean, jcov, mcnav, navfed, navK = _mc_nav_outputs(b.B, S, K, dense)
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv check(b.cache.ctx, ccall((:scvx_batch_track_mc_nav, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S, C0, xi0, _cov_opt(eta), _cov_opt(wv), N0, CN, xin,
        _cov_opt(m > 0 ? nud : nothing), m, _cov_opt(Hm), _cov_opt(rmv), nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, jmean,
        jcov, mcnav, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), _cov_opt(navfed), _cov_opt(navK)), "scvx_batch_track_mc_nav")
    return mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK
end

function track_mc_nav(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, deriv::Array{Float64,4},
                      gain::Array{Float64,4}, C0::Array{Float64,3}, xi0::Matrix{Float64}, CN::Array{Float64,3}, xin::Matrix{Float64}, H, rm;
                      kf::Union{Nothing,Array{Float64,4}}=nothing, nud::Union{Nothing,Array{Float64,3}}=nothing,
                      eta::Union{Nothing,Array{Float64,3}}=nothing, w=nothing, nsub::Int=10, clamp::Bool=false, tol::Float64=0.0,
                      dense::Bool=false)
    B, K, S = size(x, 3), size(x, 2) - 1, size(xi0, 2)
    m, Hm, rmv = _nav_model(H, rm)
    (m == 0 || (kf !== nothing && size(kf) == (m, 14, K, B) && nud !== nothing && size(nud) == (m, K, S))) ||
        throw(ArgumentError("with measurements: kf m x 14 x K x B (navigation(...; dense=true)) and nud m x K x S"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(B, S, dense)
    jmean, jcov, mcnav, navfed, navK = _mc_nav_outputs(B, S, K, dense)
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv check(cache.ctx, ccall((:scvx_track_mc_nav_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x, u, sigma, gain, C0, xi0, _cov_opt(eta), _cov_opt(wv), deriv, _cov_opt(m > 0 ? kf : nothing), CN, xin,
        _cov_opt(m > 0 ? nud : nothing), m, _cov_opt(Hm), _cov_opt(rmv), nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, jmean, jcov,
        mcnav, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), _cov_opt(navfed), _cov_opt(navK)), "scvx_track_mc_nav_f64_host")
    return mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK
end

# the same on device pointers, asynchronous on the context's stream; w (the variance), H (14 x m) and rm stay host arrays (or nothing)
track_mc_nav_dev!(cache::Cache, B::Int, K::Int, S::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble},
                  gain_dev::Ptr{Cdouble}, C0_dev::Ptr{Cdouble}, xi0_dev::Ptr{Cdouble}, eta_dev::Ptr{Cdouble}, w::Union{Nothing,Vector{Float64}},
                  deriv_dev::Ptr{Cdouble}, kf_dev::Ptr{Cdouble}, CN_dev::Ptr{Cdouble}, xin_dev::Ptr{Cdouble}, nud_dev::Ptr{Cdouble}, m::Int,
                  H::Union{Nothing,Matrix{Float64}}, rm::Union{Nothing,Vector{Float64}}, nsub::Int, flags::Int, tol::Float64,
                  mcrep_dev::Ptr{Cdouble}, xmean_dev::Ptr{Cdouble}, xcov_dev::Ptr{Cdouble}, jmean_dev::Ptr{Cdouble}, jcov_dev::Ptr{Cdouble},
                  mcnav_dev::Ptr{Cdouble}, flights_dev::Ptr{Cdouble}, xland_dev::Ptr{Cdouble}, dx0_dev::Ptr{Cdouble},
                  navfed_dev::Ptr{Cdouble}, navK_dev::Ptr{Cdouble}) =
    GC.@preserve w H rm check(cache.ctx, ccall((:scvx_track_mc_nav_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, _cov_opt(w), deriv_dev, kf_dev, CN_dev, xin_dev,
        nud_dev, m, _cov_opt(H), _cov_opt(rm), nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev, jcov_dev, mcnav_dev,
        flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev), "scvx_track_mc_nav_f64")

# ---- order statistics, and the sampled dispersions with them and the per-node samples (new) ----------------------------------
# include/scvx.h, "exact batched order statistics": v is S x R (one row of the library per COLUMN here), ranks are the library's 0-based
# ascending ranks (quantile_ranks maps probabilities to them: numpy's "inverted_cdf"); the result is nq x R, a selection of the inputs.
const Q_MAX = 16
quantile_ranks(p, S::Int) = Cint[min(S - 1, max(0, ceil(Int, x * S) - 1)) for x in p]

function order_stats(cache::Cache, v::Matrix{Float64}, ranks::Vector{Cint})
    S, R = size(v)
    out = Matrix{Float64}(undef, length(ranks), R)
    check(cache.ctx, ccall((:scvx_order_stats_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Csize_t, Csize_t, Cint, Ptr{Cint}, Ptr{Cdouble}),
        cache.ctx, R, S, v, S, 1, length(ranks), ranks, out), "scvx_order_stats_f64_host")
    return out
end

# on device pointers, asynchronous on the context's stream: row r is the S values v_dev[r * ld + s * inc]; ranks stay a host array
order_stats_dev!(cache::Cache, R::Int, S::Int, v_dev::Ptr{Cdouble}, ld::Int, inc::Int, ranks::Vector{Cint}, out_dev::Ptr{Cdouble}) =
    GC.@preserve ranks check(cache.ctx, ccall((:scvx_order_stats_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Csize_t, Csize_t, Cint, Ptr{Cint}, Ptr{Cdouble}),
        cache.ctx, R, S, v_dev, ld, inc, length(ranks), ranks, out_dev), "scvx_order_stats_f64")

# include/scvx.h, "sampled closed-loop dispersion with order statistics and per-node samples": track_mc / track_mc_nav followed by the
# ranks.  Besides their returns: flightq nq x 16 x B, and with per_node pathq nq x 5 x (K+1) x B (row PSIG_* + 1 holds that function),
# with pathv the samples themselves S x 5 x (K+1) x B.
function _mc_q_outputs(B::Int, S::Int, K::Int, nq::Int, per_node::Bool, pathv::Bool)
    return (Array{Float64,3}(undef, nq, FLIGHT_NREP, B), per_node ? Array{Float64,4}(undef, nq, 5, K + 1, B) : nothing,
            pathv ? Array{Float64,4}(undef, S, 5, K + 1, B) : nothing)
end

function track_mc_q(b::Batch, C0::Array{Float64,3}, xi0::Matrix{Float64}, ranks::Vector{Cint}; eta::Union{Nothing,Array{Float64,3}}=nothing,
                    w=nothing, q=1.0, r=1.0, qf=100.0, nsub::Int=0, clamp::Bool=false, tol::Float64=0.0, dense::Bool=false,
                    per_node::Bool=false, pathv::Bool=false)
    NU = control_dim(b.cache)
    S = size(xi0, 2); K = b.cache.problem.K
    size(C0) == (14, 14, b.B) && size(xi0, 1) == 14 || throw(ArgumentError("C0 must be 14 x 14 x B, xi0 14 x S"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(b.B, S, dense)
    flightq, pathq, pv = _mc_q_outputs(b.B, S, K, length(ranks), per_node, pathv)
    sw = w === nothing ? nothing : sqrt.(_track_w(w, 14))
    GC.@preserve sw ranks check(b.cache.ctx, ccall((:scvx_batch_track_mc_q, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S, C0, xi0, _cov_opt(eta), _cov_opt(sw), C_NULL, nsub,
        clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), length(ranks), ranks,
        flightq, _cov_opt(pathq), _cov_opt(pv)), "scvx_batch_track_mc_q")
    return mcrep, xmean, xcov, flights, xland, dx0, flightq, pathq, pv
end

function track_mc_q(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, gain::Array{Float64,4},
                    C0::Array{Float64,3}, xi0::Matrix{Float64}, ranks::Vector{Cint}; eta::Union{Nothing,Array{Float64,3}}=nothing,
                    w=nothing, nsub::Int=10, clamp::Bool=false, tol::Float64=0.0, dense::Bool=false, per_node::Bool=false,
                    pathv::Bool=false)
    B, K, S = size(x, 3), size(x, 2) - 1, size(xi0, 2)
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(B, S, dense)
    flightq, pathq, pv = _mc_q_outputs(B, S, K, length(ranks), per_node, pathv)
    sw = w === nothing ? nothing : sqrt.(_track_w(w, 14))
    GC.@preserve sw ranks check(cache.ctx, ccall((:scvx_track_mc_q_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x, u, sigma, gain, C0, xi0, _cov_opt(eta), _cov_opt(sw), C_NULL, nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep,
        xmean, xcov, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), length(ranks), ranks, flightq, _cov_opt(pathq), _cov_opt(pv)),
        "scvx_track_mc_q_f64_host")
    return mcrep, xmean, xcov, flights, xland, dx0, flightq, pathq, pv
end

# on device pointers, asynchronous on the context's stream; sw = sqrt(w) and ranks stay host arrays; C_NULL for an output not wanted
track_mc_q_dev!(cache::Cache, B::Int, K::Int, S::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble},
                gain_dev::Ptr{Cdouble}, C0_dev::Ptr{Cdouble}, xi0_dev::Ptr{Cdouble}, eta_dev::Ptr{Cdouble}, sw::Union{Nothing,Vector{Float64}},
                nsub::Int, flags::Int, tol::Float64, mcrep_dev::Ptr{Cdouble}, xmean_dev::Ptr{Cdouble}, xcov_dev::Ptr{Cdouble},
                flights_dev::Ptr{Cdouble}, xland_dev::Ptr{Cdouble}, dx0_dev::Ptr{Cdouble}, ranks::Vector{Cint}, flightq_dev::Ptr{Cdouble},
                pathq_dev::Ptr{Cdouble}, pathv_dev::Ptr{Cdouble}) =
    GC.@preserve sw ranks check(cache.ctx, ccall((:scvx_track_mc_q_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, _cov_opt(sw), C_NULL, nsub, flags, tol, mcrep_dev,
        xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, length(ranks), ranks, flightq_dev, pathq_dev, pathv_dev), "scvx_track_mc_q_f64")

function track_mc_nav_q(b::Batch, C0::Array{Float64,3}, xi0::Matrix{Float64}, N0::Array{Float64,3}, CN::Array{Float64,3},
                        xin::Matrix{Float64}, H, rm, ranks::Vector{Cint}; nud::Union{Nothing,Array{Float64,3}}=nothing,
                        eta::Union{Nothing,Array{Float64,3}}=nothing, w=nothing, q=1.0, r=1.0, qf=100.0, nsub::Int=0, clamp::Bool=false,
                        tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false)
    NU = control_dim(b.cache)
    S = size(xi0, 2); K = b.cache.problem.K
    (size(C0) == (14, 14, b.B) && size(N0) == (14, 14, b.B) && size(CN) == (14, 14, b.B) && size(xi0, 1) == 14 && size(xin) == (14, S)) ||
        throw(ArgumentError("C0, N0, CN must be 14 x 14 x B, xi0 and xin 14 x S"))
    m, Hm, rmv = _nav_model(H, rm)
    (m == 0 || (nud !== nothing && size(nud) == (m, K, S))) || throw(ArgumentError("nud must be m x K x S"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(b.B, S, dense)
    jmean, jcov, mcnav, navfed, navK = _mc_nav_outputs(b.B, S, K, dense)
    flightq, pathq, pv = _mc_q_outputs(b.B, S, K, length(ranks), per_node, pathv)
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv ranks check(b.cache.ctx, ccall((:scvx_batch_track_mc_nav_q, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S, C0, xi0, _cov_opt(eta), _cov_opt(wv), N0, CN, xin,
        _cov_opt(m > 0 ? nud : nothing), m, _cov_opt(Hm), _cov_opt(rmv), nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, jmean,
        jcov, mcnav, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), _cov_opt(navfed), _cov_opt(navK), length(ranks), ranks, flightq,
        _cov_opt(pathq), _cov_opt(pv)), "scvx_batch_track_mc_nav_q")
    return mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, flightq, pathq, pv
end

function track_mc_nav_q(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, deriv::Array{Float64,4},
                        gain::Array{Float64,4}, C0::Array{Float64,3}, xi0::Matrix{Float64}, CN::Array{Float64,3}, xin::Matrix{Float64}, H,
                        rm, ranks::Vector{Cint}; kf::Union{Nothing,Array{Float64,4}}=nothing,
                        nud::Union{Nothing,Array{Float64,3}}=nothing, eta::Union{Nothing,Array{Float64,3}}=nothing, w=nothing,
                        nsub::Int=10, clamp::Bool=false, tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false)
    B, K, S = size(x, 3), size(x, 2) - 1, size(xi0, 2)
    m, Hm, rmv = _nav_model(H, rm)
    (m == 0 || (kf !== nothing && size(kf) == (m, 14, K, B) && nud !== nothing && size(nud) == (m, K, S))) ||
        throw(ArgumentError("with measurements: kf m x 14 x K x B (navigation(...; dense=true)) and nud m x K x S"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(B, S, dense)
    jmean, jcov, mcnav, navfed, navK = _mc_nav_outputs(B, S, K, dense)
    flightq, pathq, pv = _mc_q_outputs(B, S, K, length(ranks), per_node, pathv)
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv ranks check(cache.ctx, ccall((:scvx_track_mc_nav_q_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x, u, sigma, gain, C0, xi0, _cov_opt(eta), _cov_opt(wv), deriv, _cov_opt(m > 0 ? kf : nothing), CN, xin,
        _cov_opt(m > 0 ? nud : nothing), m, _cov_opt(Hm), _cov_opt(rmv), nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, jmean, jcov,
        mcnav, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), _cov_opt(navfed), _cov_opt(navK), length(ranks), ranks, flightq,
        _cov_opt(pathq), _cov_opt(pv)), "scvx_track_mc_nav_q_f64_host")
    return mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, flightq, pathq, pv
end

track_mc_nav_q_dev!(cache::Cache, B::Int, K::Int, S::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble},
                    gain_dev::Ptr{Cdouble}, C0_dev::Ptr{Cdouble}, xi0_dev::Ptr{Cdouble}, eta_dev::Ptr{Cdouble},
                    w::Union{Nothing,Vector{Float64}}, deriv_dev::Ptr{Cdouble}, kf_dev::Ptr{Cdouble}, CN_dev::Ptr{Cdouble},
                    xin_dev::Ptr{Cdouble}, nud_dev::Ptr{Cdouble}, m::Int, H::Union{Nothing,Matrix{Float64}},
                    rm::Union{Nothing,Vector{Float64}}, nsub::Int, flags::Int, tol::Float64, mcrep_dev::Ptr{Cdouble},
                    xmean_dev::Ptr{Cdouble}, xcov_dev::Ptr{Cdouble}, jmean_dev::Ptr{Cdouble}, jcov_dev::Ptr{Cdouble},
                    mcnav_dev::Ptr{Cdouble}, flights_dev::Ptr{Cdouble}, xland_dev::Ptr{Cdouble}, dx0_dev::Ptr{Cdouble},
                    navfed_dev::Ptr{Cdouble}, navK_dev::Ptr{Cdouble}, ranks::Vector{Cint}, flightq_dev::Ptr{Cdouble},
                    pathq_dev::Ptr{Cdouble}, pathv_dev::Ptr{Cdouble}) =
    GC.@preserve w H rm ranks check(cache.ctx, ccall((:scvx_track_mc_nav_q_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, _cov_opt(w), deriv_dev, kf_dev, CN_dev, xin_dev,
        nud_dev, m, _cov_opt(H), _cov_opt(rm), nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev, jcov_dev, mcnav_dev,
        flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev, length(ranks), ranks, flightq_dev, pathq_dev, pathv_dev),
        "scvx_track_mc_nav_q_f64")

# include/scvx.h, "sampled closed-loop dispersion with the draws made on the device": the _q calls with (xi0, eta) replaced by
# (rng, noise) -- every lane makes its own draws from Philox4x64-10 (numpy's np.random.Philox; the stream is spelled out in the header),
# shared by all plans or, with independent = true, per plan -- and, in the navigation form, (xin, nud) dropped.  An empty ranks
# vector asks for no order statistics.  mc_draws returns the draws themselves, the bits the flying kernels consume.
struct McRng
    seed::UInt64
    s_lo::UInt64
    b_lo::UInt64
    independent::Int32
    reserved::Int32
end
McRng(seed::Integer; s_lo::Integer=0, b_lo::Integer=0, independent::Bool=false) =
    McRng(UInt64(seed), UInt64(s_lo), UInt64(b_lo), Int32(independent), Int32(0))

function mc_draws(cache::Cache, rng::McRng, S::Int; P::Int=1, K::Int=cache.problem.K)
    xi0 = Array{Float64,3}(undef, 14, S, P); xin = similar(xi0)
    eta = Array{Float64,4}(undef, 14, K, S, P); nud = similar(eta)
    check(cache.ctx, ccall((:scvx_mc_draws_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Ref{McRng}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, rng, P, S, K, xi0, eta, xin, nud), "scvx_mc_draws_f64_host")
    return xi0, eta, xin, nud
end

# on device pointers, asynchronous on the context's stream; C_NULL for an output not wanted
mc_draws_dev!(cache::Cache, rng::McRng, P::Int, S::Int, K::Int, xi0_dev::Ptr{Cdouble}, eta_dev::Ptr{Cdouble}, xin_dev::Ptr{Cdouble},
              nud_dev::Ptr{Cdouble}) =
    check(cache.ctx, ccall((:scvx_mc_draws_f64, LIB), Cint,
        (Ptr{Cvoid}, Ref{McRng}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, rng, P, S, K, xi0_dev, eta_dev, xin_dev, nud_dev), "scvx_mc_draws_f64")

function track_mc_rng(b::Batch, C0::Array{Float64,3}, rng::McRng, S::Int; ranks::Vector{Cint}=Cint[], w=nothing, q=1.0, r=1.0, qf=100.0,
                      nsub::Int=0, clamp::Bool=false, tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false)
    NU = control_dim(b.cache); K = b.cache.problem.K; nq = length(ranks)
    size(C0) == (14, 14, b.B) || throw(ArgumentError("C0 must be 14 x 14 x B"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(b.B, S, dense)
    flightq, pathq, pv = _mc_q_outputs(b.B, S, K, nq, per_node && nq > 0, pathv)
    sw = w === nothing ? nothing : sqrt.(_track_w(w, 14))
    GC.@preserve sw ranks check(b.cache.ctx, ccall((:scvx_batch_track_mc_rng, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ref{McRng}, Cint, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S, C0, rng, sw === nothing ? 0 : 1, _cov_opt(sw), C_NULL, nsub,
        clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), nq,
        nq > 0 ? ranks : C_NULL, nq > 0 ? flightq : C_NULL, _cov_opt(pathq), _cov_opt(pv)), "scvx_batch_track_mc_rng")
    return mcrep, xmean, xcov, flights, xland, dx0, (nq > 0 ? flightq : nothing), pathq, pv
end

function track_mc_rng(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, gain::Array{Float64,4},
                      C0::Array{Float64,3}, rng::McRng, S::Int; ranks::Vector{Cint}=Cint[], w=nothing, nsub::Int=10, clamp::Bool=false,
                      tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false)
    B, K, nq = size(x, 3), size(x, 2) - 1, length(ranks)
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(B, S, dense)
    flightq, pathq, pv = _mc_q_outputs(B, S, K, nq, per_node && nq > 0, pathv)
    sw = w === nothing ? nothing : sqrt.(_track_w(w, 14))
    GC.@preserve sw ranks check(cache.ctx, ccall((:scvx_track_mc_rng_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{McRng}, Cint, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x, u, sigma, gain, C0, rng, sw === nothing ? 0 : 1, _cov_opt(sw), C_NULL, nsub, clamp ? TRACK_CLAMP : 0, tol,
        mcrep, xmean, xcov, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), nq, nq > 0 ? ranks : C_NULL, nq > 0 ? flightq : C_NULL,
        _cov_opt(pathq), _cov_opt(pv)), "scvx_track_mc_rng_f64_host")
    return mcrep, xmean, xcov, flights, xland, dx0, (nq > 0 ? flightq : nothing), pathq, pv
end

# on device pointers, asynchronous on the context's stream; sw = sqrt(w) and ranks stay host arrays; C_NULL for an output not wanted
track_mc_rng_dev!(cache::Cache, B::Int, K::Int, S::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble},
                  gain_dev::Ptr{Cdouble}, C0_dev::Ptr{Cdouble}, rng::McRng, sw::Union{Nothing,Vector{Float64}}, nsub::Int, flags::Int,
                  tol::Float64, mcrep_dev::Ptr{Cdouble}, xmean_dev::Ptr{Cdouble}, xcov_dev::Ptr{Cdouble}, flights_dev::Ptr{Cdouble},
                  xland_dev::Ptr{Cdouble}, dx0_dev::Ptr{Cdouble}, ranks::Vector{Cint}, flightq_dev::Ptr{Cdouble},
                  pathq_dev::Ptr{Cdouble}, pathv_dev::Ptr{Cdouble}) =
    GC.@preserve sw ranks check(cache.ctx, ccall((:scvx_track_mc_rng_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{McRng}, Cint, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, rng, sw === nothing ? 0 : 1, _cov_opt(sw), C_NULL, nsub, flags, tol,
        mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, length(ranks), isempty(ranks) ? C_NULL : ranks, flightq_dev,
        pathq_dev, pathv_dev), "scvx_track_mc_rng_f64")

function track_mc_nav_rng(b::Batch, C0::Array{Float64,3}, N0::Array{Float64,3}, CN::Array{Float64,3}, H, rm, rng::McRng, S::Int;
                          ranks::Vector{Cint}=Cint[], w=nothing, q=1.0, r=1.0, qf=100.0, nsub::Int=0, clamp::Bool=false,
                          tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false)
    NU = control_dim(b.cache); K = b.cache.problem.K; nq = length(ranks)
    (size(C0) == (14, 14, b.B) && size(N0) == (14, 14, b.B) && size(CN) == (14, 14, b.B)) ||
        throw(ArgumentError("C0, N0, CN must be 14 x 14 x B"))
    m, Hm, rmv = _nav_model(H, rm)
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(b.B, S, dense)
    jmean, jcov, mcnav, navfed, navK = _mc_nav_outputs(b.B, S, K, dense)
    flightq, pathq, pv = _mc_q_outputs(b.B, S, K, nq, per_node && nq > 0, pathv)
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv ranks check(b.cache.ctx, ccall((:scvx_batch_track_mc_nav_rng, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ref{McRng}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S, C0, rng, wv === nothing ? 0 : 1, _cov_opt(wv), N0, CN, m,
        _cov_opt(Hm), _cov_opt(rmv), nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, jmean, jcov, mcnav, _cov_opt(flights),
        _cov_opt(xland), _cov_opt(dx0), _cov_opt(navfed), _cov_opt(navK), nq, nq > 0 ? ranks : C_NULL, nq > 0 ? flightq : C_NULL,
        _cov_opt(pathq), _cov_opt(pv)), "scvx_batch_track_mc_nav_rng")
    return mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, (nq > 0 ? flightq : nothing), pathq, pv
end

function track_mc_nav_rng(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, deriv::Array{Float64,4},
                          gain::Array{Float64,4}, C0::Array{Float64,3}, CN::Array{Float64,3}, H, rm, rng::McRng, S::Int;
                          kf::Union{Nothing,Array{Float64,4}}=nothing, ranks::Vector{Cint}=Cint[], w=nothing, nsub::Int=10,
                          clamp::Bool=false, tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false)
    B, K, nq = size(x, 3), size(x, 2) - 1, length(ranks)
    m, Hm, rmv = _nav_model(H, rm)
    (m == 0 || (kf !== nothing && size(kf) == (m, 14, K, B))) ||
        throw(ArgumentError("with measurements: kf m x 14 x K x B (navigation(...; dense=true))"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(B, S, dense)
    jmean, jcov, mcnav, navfed, navK = _mc_nav_outputs(B, S, K, dense)
    flightq, pathq, pv = _mc_q_outputs(B, S, K, nq, per_node && nq > 0, pathv)
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv ranks check(cache.ctx, ccall((:scvx_track_mc_nav_rng_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{McRng}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x, u, sigma, gain, C0, rng, wv === nothing ? 0 : 1, _cov_opt(wv), deriv, _cov_opt(m > 0 ? kf : nothing), CN, m,
        _cov_opt(Hm), _cov_opt(rmv), nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, jmean, jcov, mcnav, _cov_opt(flights),
        _cov_opt(xland), _cov_opt(dx0), _cov_opt(navfed), _cov_opt(navK), nq, nq > 0 ? ranks : C_NULL, nq > 0 ? flightq : C_NULL,
        _cov_opt(pathq), _cov_opt(pv)), "scvx_track_mc_nav_rng_f64_host")
    return mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, (nq > 0 ? flightq : nothing), pathq, pv
end

# on device pointers, asynchronous on the context's stream; w (the VARIANCE), H, rm and ranks stay host arrays; C_NULL for an output not wanted
track_mc_nav_rng_dev!(cache::Cache, B::Int, K::Int, S::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble},
                      gain_dev::Ptr{Cdouble}, C0_dev::Ptr{Cdouble}, rng::McRng, w::Union{Nothing,Vector{Float64}},
                      deriv_dev::Ptr{Cdouble}, kf_dev::Ptr{Cdouble}, CN_dev::Ptr{Cdouble}, m::Int, H::Union{Nothing,Matrix{Float64}},
                      rm::Union{Nothing,Vector{Float64}}, nsub::Int, flags::Int, tol::Float64, mcrep_dev::Ptr{Cdouble},
                      xmean_dev::Ptr{Cdouble}, xcov_dev::Ptr{Cdouble}, jmean_dev::Ptr{Cdouble}, jcov_dev::Ptr{Cdouble},
                      mcnav_dev::Ptr{Cdouble}, flights_dev::Ptr{Cdouble}, xland_dev::Ptr{Cdouble}, dx0_dev::Ptr{Cdouble},
                      navfed_dev::Ptr{Cdouble}, navK_dev::Ptr{Cdouble}, ranks::Vector{Cint}, flightq_dev::Ptr{Cdouble},
                      pathq_dev::Ptr{Cdouble}, pathv_dev::Ptr{Cdouble}) =
    GC.@preserve w H rm ranks check(cache.ctx, ccall((:scvx_track_mc_nav_rng_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{McRng}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, rng, w === nothing ? 0 : 1, _cov_opt(w), deriv_dev, kf_dev, CN_dev,
        m, _cov_opt(H), _cov_opt(rm), nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev, jcov_dev, mcnav_dev, flights_dev,
        xland_dev, dx0_dev, navfed_dev, navK_dev, length(ranks), isempty(ranks) ? C_NULL : ranks, flightq_dev, pathq_dev, pathv_dev),
        "scvx_track_mc_nav_rng_f64")

# include/scvx.h, "sampled closed-loop dispersion with per-flight VEHICLE ERRORS": the _q calls followed by (rng, noise, veh, zeta,
# theta) -- every flight flies a vehicle of its own, theta = mu + sp .* zeta constant over the flight, in the order THRUST, MIS_Y,
# MIS_Z, ISP, AERO, FIN (the model and its limits are in the header).  rng = nothing: the uploaded draws xi0 (14 x S), eta (14 x K x S
# or nothing), zeta (6 x S; needed as soon as any sp > 0), with nav also xin and nud; rng::McRng: the lanes make all of them (zeta from
# stream 8) and the uploaded ones must stay nothing.  theta = true returns the errors flown, 6 x S x B.
struct McVehicle
    mu::NTuple{6,Float64}
    sp::NTuple{6,Float64}
    reserved::NTuple{2,Int32}
end
McVehicle(mu::AbstractVector, sp::AbstractVector) = McVehicle(Tuple(Float64.(mu)), Tuple(Float64.(sp)), (Int32(0), Int32(0)))
McVehicle(; thrust=0.0, mis_y=0.0, mis_z=0.0, isp=0.0, aero=0.0, fin=0.0, mean=zeros(6)) =
    McVehicle(mean, [thrust, mis_y, mis_z, isp, aero, fin])
_mc_rng_ptr(rng) = rng === nothing ? C_NULL : Ref(rng)

function track_mc_veh(b::Batch, C0::Array{Float64,3}, veh::McVehicle, S::Int; rng::Union{Nothing,McRng}=nothing, xi0=nothing, eta=nothing,
                      zeta=nothing, ranks::Vector{Cint}=Cint[], w=nothing, q=1.0, r=1.0, qf=100.0, nsub::Int=0, clamp::Bool=false,
                      tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false, theta::Bool=false)
    NU = control_dim(b.cache); K = b.cache.problem.K; nq = length(ranks)
    size(C0) == (14, 14, b.B) || throw(ArgumentError("C0 must be 14 x 14 x B"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(b.B, S, dense)
    flightq, pathq, pv = _mc_q_outputs(b.B, S, K, nq, per_node && nq > 0, pathv)
    th = theta ? Array{Float64,3}(undef, 6, S, b.B) : nothing
    sw = w === nothing ? nothing : sqrt.(_track_w(w, 14))
    rp = _mc_rng_ptr(rng); vr = Ref(veh)
    GC.@preserve sw ranks rp vr check(b.cache.ctx, ccall((:scvx_batch_track_mc_veh, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{McRng}, Cint, Ptr{McVehicle}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S, C0, _cov_opt(xi0), _cov_opt(eta), _cov_opt(sw), C_NULL, nsub,
        clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), nq,
        nq > 0 ? ranks : C_NULL, nq > 0 ? flightq : C_NULL, _cov_opt(pathq), _cov_opt(pv), rp, (rng !== nothing && sw !== nothing) ? 1 : 0,
        vr, _cov_opt(zeta), _cov_opt(th)), "scvx_batch_track_mc_veh")
    return mcrep, xmean, xcov, flights, xland, dx0, (nq > 0 ? flightq : nothing), pathq, pv, th
end

function track_mc_veh(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, gain::Array{Float64,4},
                      C0::Array{Float64,3}, veh::McVehicle, S::Int; rng::Union{Nothing,McRng}=nothing, xi0=nothing, eta=nothing,
                      zeta=nothing, ranks::Vector{Cint}=Cint[], w=nothing, nsub::Int=10, clamp::Bool=false, tol::Float64=0.0,
                      dense::Bool=false, per_node::Bool=false, pathv::Bool=false, theta::Bool=false)
    B, K, nq = size(x, 3), size(x, 2) - 1, length(ranks)
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(B, S, dense)
    flightq, pathq, pv = _mc_q_outputs(B, S, K, nq, per_node && nq > 0, pathv)
    th = theta ? Array{Float64,3}(undef, 6, S, B) : nothing
    sw = w === nothing ? nothing : sqrt.(_track_w(w, 14))
    rp = _mc_rng_ptr(rng); vr = Ref(veh)
    GC.@preserve sw ranks rp vr check(cache.ctx, ccall((:scvx_track_mc_veh_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{McRng}, Cint, Ptr{McVehicle}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x, u, sigma, gain, C0, _cov_opt(xi0), _cov_opt(eta), _cov_opt(sw), C_NULL, nsub, clamp ? TRACK_CLAMP : 0, tol,
        mcrep, xmean, xcov, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), nq, nq > 0 ? ranks : C_NULL, nq > 0 ? flightq : C_NULL,
        _cov_opt(pathq), _cov_opt(pv), rp, (rng !== nothing && sw !== nothing) ? 1 : 0, vr, _cov_opt(zeta), _cov_opt(th)),
        "scvx_track_mc_veh_f64_host")
    return mcrep, xmean, xcov, flights, xland, dx0, (nq > 0 ? flightq : nothing), pathq, pv, th
end

# on device pointers, asynchronous on the context's stream; sw = sqrt(w) and ranks stay host arrays; C_NULL for an array not given
track_mc_veh_dev!(cache::Cache, B::Int, K::Int, S::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble},
                  gain_dev::Ptr{Cdouble}, C0_dev::Ptr{Cdouble}, xi0_dev::Ptr{Cdouble}, eta_dev::Ptr{Cdouble},
                  sw::Union{Nothing,Vector{Float64}}, nsub::Int, flags::Int, tol::Float64, mcrep_dev::Ptr{Cdouble},
                  xmean_dev::Ptr{Cdouble}, xcov_dev::Ptr{Cdouble}, flights_dev::Ptr{Cdouble}, xland_dev::Ptr{Cdouble},
                  dx0_dev::Ptr{Cdouble}, ranks::Vector{Cint}, flightq_dev::Ptr{Cdouble}, pathq_dev::Ptr{Cdouble},
                  pathv_dev::Ptr{Cdouble}, rng::Union{Nothing,McRng}, noise::Bool, veh::McVehicle, zeta_dev::Ptr{Cdouble},
                  theta_dev::Ptr{Cdouble}) = begin
    rp = _mc_rng_ptr(rng); vr = Ref(veh)
    GC.@preserve sw ranks rp vr check(cache.ctx, ccall((:scvx_track_mc_veh_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{McRng}, Cint, Ptr{McVehicle}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, _cov_opt(sw), C_NULL, nsub, flags, tol,
        mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, length(ranks), isempty(ranks) ? C_NULL : ranks, flightq_dev,
        pathq_dev, pathv_dev, rp, noise ? 1 : 0, vr, zeta_dev, theta_dev), "scvx_track_mc_veh_f64")
end

function track_mc_nav_veh(b::Batch, C0::Array{Float64,3}, N0::Array{Float64,3}, CN::Array{Float64,3}, H, rm, veh::McVehicle, S::Int;
                          rng::Union{Nothing,McRng}=nothing, xi0=nothing, eta=nothing, xin=nothing, nud=nothing, zeta=nothing,
                          ranks::Vector{Cint}=Cint[], w=nothing, q=1.0, r=1.0, qf=100.0, nsub::Int=0, clamp::Bool=false,
                          tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false, theta::Bool=false)
    NU = control_dim(b.cache); K = b.cache.problem.K; nq = length(ranks)
    (size(C0) == (14, 14, b.B) && size(N0) == (14, 14, b.B) && size(CN) == (14, 14, b.B)) ||
        throw(ArgumentError("C0, N0, CN must be 14 x 14 x B"))
    m, Hm, rmv = _nav_model(H, rm)
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(b.B, S, dense)
    jmean, jcov, mcnav, navfed, navK = _mc_nav_outputs(b.B, S, K, dense)
    flightq, pathq, pv = _mc_q_outputs(b.B, S, K, nq, per_node && nq > 0, pathv)
    th = theta ? Array{Float64,3}(undef, 6, S, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    rp = _mc_rng_ptr(rng); vr = Ref(veh)
    GC.@preserve wv Hm rmv ranks rp vr check(b.cache.ctx, ccall((:scvx_batch_track_mc_nav_veh, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{McRng}, Cint, Ptr{McVehicle}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S, C0, _cov_opt(xi0), _cov_opt(eta), _cov_opt(wv), N0, CN, _cov_opt(xin),
        _cov_opt(m > 0 ? nud : nothing), m, _cov_opt(Hm), _cov_opt(rmv), nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean, xcov, jmean, jcov,
        mcnav, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), _cov_opt(navfed), _cov_opt(navK), nq, nq > 0 ? ranks : C_NULL,
        nq > 0 ? flightq : C_NULL, _cov_opt(pathq), _cov_opt(pv), rp, (rng !== nothing && wv !== nothing) ? 1 : 0, vr, _cov_opt(zeta),
        _cov_opt(th)), "scvx_batch_track_mc_nav_veh")
    return mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, (nq > 0 ? flightq : nothing), pathq, pv, th
end

function track_mc_nav_veh(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64}, deriv::Array{Float64,4},
                          gain::Array{Float64,4}, C0::Array{Float64,3}, CN::Array{Float64,3}, H, rm, veh::McVehicle, S::Int;
                          rng::Union{Nothing,McRng}=nothing, xi0=nothing, eta=nothing, xin=nothing, nud=nothing, zeta=nothing,
                          kf::Union{Nothing,Array{Float64,4}}=nothing, ranks::Vector{Cint}=Cint[], w=nothing, nsub::Int=10,
                          clamp::Bool=false, tol::Float64=0.0, dense::Bool=false, per_node::Bool=false, pathv::Bool=false,
                          theta::Bool=false)
    B, K, nq = size(x, 3), size(x, 2) - 1, length(ranks)
    m, Hm, rmv = _nav_model(H, rm)
    (m == 0 || (kf !== nothing && size(kf) == (m, 14, K, B))) ||
        throw(ArgumentError("with measurements: kf m x 14 x K x B (navigation(...; dense=true))"))
    mcrep, xmean, xcov, flights, xland, dx0 = _mc_outputs(B, S, dense)
    jmean, jcov, mcnav, navfed, navK = _mc_nav_outputs(B, S, K, dense)
    flightq, pathq, pv = _mc_q_outputs(B, S, K, nq, per_node && nq > 0, pathv)
    th = theta ? Array{Float64,3}(undef, 6, S, B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    rp = _mc_rng_ptr(rng); vr = Ref(veh)
    GC.@preserve wv Hm rmv ranks rp vr check(cache.ctx, ccall((:scvx_track_mc_nav_veh_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{McRng}, Cint, Ptr{McVehicle}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x, u, sigma, gain, C0, _cov_opt(xi0), _cov_opt(eta), _cov_opt(wv), deriv, _cov_opt(m > 0 ? kf : nothing), CN,
        _cov_opt(xin), _cov_opt(m > 0 ? nud : nothing), m, _cov_opt(Hm), _cov_opt(rmv), nsub, clamp ? TRACK_CLAMP : 0, tol, mcrep, xmean,
        xcov, jmean, jcov, mcnav, _cov_opt(flights), _cov_opt(xland), _cov_opt(dx0), _cov_opt(navfed), _cov_opt(navK), nq,
        nq > 0 ? ranks : C_NULL, nq > 0 ? flightq : C_NULL, _cov_opt(pathq), _cov_opt(pv), rp,
        (rng !== nothing && wv !== nothing) ? 1 : 0, vr, _cov_opt(zeta), _cov_opt(th)), "scvx_track_mc_nav_veh_f64_host")
    return mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, (nq > 0 ? flightq : nothing), pathq, pv, th
end

# on device pointers, asynchronous on the context's stream; w (the VARIANCE), H, rm and ranks stay host arrays; C_NULL for an array not given
track_mc_nav_veh_dev!(cache::Cache, B::Int, K::Int, S::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble},
                      gain_dev::Ptr{Cdouble}, C0_dev::Ptr{Cdouble}, xi0_dev::Ptr{Cdouble}, eta_dev::Ptr{Cdouble},
                      w::Union{Nothing,Vector{Float64}}, deriv_dev::Ptr{Cdouble}, kf_dev::Ptr{Cdouble}, CN_dev::Ptr{Cdouble},
                      xin_dev::Ptr{Cdouble}, nud_dev::Ptr{Cdouble}, m::Int, H::Union{Nothing,Matrix{Float64}},
                      rm::Union{Nothing,Vector{Float64}}, nsub::Int, flags::Int, tol::Float64, mcrep_dev::Ptr{Cdouble},
                      xmean_dev::Ptr{Cdouble}, xcov_dev::Ptr{Cdouble}, jmean_dev::Ptr{Cdouble}, jcov_dev::Ptr{Cdouble},
                      mcnav_dev::Ptr{Cdouble}, flights_dev::Ptr{Cdouble}, xland_dev::Ptr{Cdouble}, dx0_dev::Ptr{Cdouble},
                      navfed_dev::Ptr{Cdouble}, navK_dev::Ptr{Cdouble}, ranks::Vector{Cint}, flightq_dev::Ptr{Cdouble},
                      pathq_dev::Ptr{Cdouble}, pathv_dev::Ptr{Cdouble}, rng::Union{Nothing,McRng}, noise::Bool, veh::McVehicle,
                      zeta_dev::Ptr{Cdouble}, theta_dev::Ptr{Cdouble}) = begin
    rp = _mc_rng_ptr(rng); vr = Ref(veh)
    GC.@preserve w H rm ranks rp vr check(cache.ctx, ccall((:scvx_track_mc_nav_veh_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{McRng}, Cint, Ptr{McVehicle}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, _cov_opt(w), deriv_dev, kf_dev, CN_dev, xin_dev,
        nud_dev, m, _cov_opt(H), _cov_opt(rm), nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev, jcov_dev, mcnav_dev,
        flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev, length(ranks), isempty(ranks) ? C_NULL : ranks, flightq_dev, pathq_dev,
        pathv_dev, rp, noise ? 1 : 0, vr, zeta_dev, theta_dev), "scvx_track_mc_nav_veh_f64")
end

# ---- thrust-band back-offs and covariance-driven replanning (new) ----------------------------------------------------------
# include/scvx.h, "thrust-band back-offs".  Tmin + lo[k, b] <= |u_k| <= Tmax - hi[k, b], read by the conic solve alone; the flight
# check and the tracking calls keep auditing against the true Tmin / Tmax.  psig is 5 x (K+1) x B (row PSIG_* + 1 holds that column).
const PSIG_N = 5
const PSIG_MASS = 0; const PSIG_GLIDE = 1; const PSIG_TILT = 2; const PSIG_RATE = 3; const PSIG_THRUST = 4

# lo, hi: (K+1) x B each; both `nothing` clears
function set_thrust_margins!(b::Batch, lo::Union{Nothing,Matrix{Float64}}, hi::Union{Nothing,Matrix{Float64}})
    K = b.cache.problem.K
    (lo === nothing) == (hi === nothing) || error("give lo and hi, or neither")
    lo === nothing || (size(lo) == (K + 1, b.B) && size(hi) == (K + 1, b.B)) || error("lo, hi must be (K+1) x B")
    check(b.cache.ctx, ccall((:scvx_batch_set_thrust_margins, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _cov_opt(lo), _cov_opt(hi)), "scvx_batch_set_thrust_margins")
    return b
end

function thrust_margins(b::Batch)
    K = b.cache.problem.K
    lo = Matrix{Float64}(undef, K + 1, b.B); hi = Matrix{Float64}(undef, K + 1, b.B)
    check(b.cache.ctx, ccall((:scvx_batch_get_thrust_margins, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), b.h, lo, hi),
        "scvx_batch_get_thrust_margins")
    return lo, hi
end

# back-offs lo = hi = min(nsigma s_T(k), cap (Tmax - Tmin)) from the covariance analysis of the current iterate, on the device;
# psig=true also returns the 5 x (K+1) x B standard deviations of the path functions
function thrust_margins_from_cov!(b::Batch, S0::Array{Float64,3}; nsigma::Real=3.0, cap::Real=0.25, w=nothing, q=1.0, r=1.0, qf=100.0,
                                  psig::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx))
    size(S0) == (14, 14, b.B) || error("S0 must be 14 x 14 x B")
    ps = psig ? Array{Float64,3}(undef, PSIG_N, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv check(b.cache.ctx, ccall((:scvx_batch_thrust_margins_from_cov, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, _cov_opt(wv), Float64(nsigma), Float64(cap), _cov_opt(ps)),
        "scvx_batch_thrust_margins_from_cov")
    return ps
end

# start the SCvx loop again from the current iterate (rk = 100, cost = Inf, iter = 0; failed trajectories stay frozen)
replan!(b::Batch) = (check(b.cache.ctx, ccall((:scvx_batch_replan, LIB), Cint, (Ptr{Cvoid},), b.h), "scvx_batch_replan"); b)

# per round: back-offs from the covariance, replan, solve; returns (status, iters, nu, dJ, lo, hi).  First order; one round reaches
# about 2.5 - 3 sigma of headroom for nsigma = 3; a replan may land in another local optimum than a solve from the guess
# which: the constraints that are tightened (MARGIN_*); with a path constraint among them path_margins(b) holds their back-offs
function robustify!(b::Batch, S0::Array{Float64,3}; nsigma::Real=3.0, rounds::Int=1, cap::Real=0.25, w=nothing, q=1.0, r=1.0, qf=100.0,
                    which::Integer=MARGIN_THRUST, nav=nothing)
    rounds >= 1 || error("rounds >= 1")
    st = Vector{Int32}(undef, b.B); it = Vector{Int32}(undef, b.B); nu = Vector{Float64}(undef, b.B); dj = Vector{Float64}(undef, b.B)
    for _ in 1:rounds
        if nav !== nothing   # (N0, H, rm): the s(k) of the loop flown on an estimate (margins_from_nav!)
            margins_from_nav!(b, S0, nav[1], nav[2], nav[3]; which=which, nsigma=nsigma, cap=cap, w=w, q=q, r=r, qf=qf)
        elseif which == MARGIN_THRUST
            thrust_margins_from_cov!(b, S0; nsigma=nsigma, cap=cap, w=w, q=q, r=r, qf=qf)
        else
            margins_from_cov!(b, S0; which=which, nsigma=nsigma, cap=cap, w=w, q=q, r=r, qf=qf)
        end
        replan!(b)
        check(b.cache.ctx, ccall((:scvx_solve, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}), b.h, st, it, nu, dj), "scvx_solve")
    end
    lo, hi = thrust_margins(b)
    return st, it, nu, dj, lo, hi
end

# ---- path-constraint back-offs: mass, glide slope, tilt, rate (new) -----------------------------------------------------------
# include/scvx.h, "path-constraint back-offs".  pm is 4 x (K+1) x B (row PMARG_* + 1 holds that column), read by the conic solve
# alone; `nothing` clears.  Out of scope: gimbal, dynamic-pressure and fin back-offs, and back-offs on the estimate's constraints.
const PMARG_N = 4
const PMARG_MASS = 0; const PMARG_GLIDE = 1; const PMARG_TILT = 2; const PMARG_RATE = 3
const MARGIN_THRUST = UInt32(1); const MARGIN_MASS = UInt32(2); const MARGIN_GLIDE = UInt32(4); const MARGIN_TILT = UInt32(8)
const MARGIN_RATE = UInt32(16); const MARGIN_ALL = UInt32(31)

function set_path_margins!(b::Batch, pm::Union{Nothing,Array{Float64,3}})
    K = b.cache.problem.K
    pm === nothing || size(pm) == (PMARG_N, K + 1, b.B) || error("pm must be 4 x (K+1) x B")
    check(b.cache.ctx, ccall((:scvx_batch_set_path_margins, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), b.h, _cov_opt(pm)),
        "scvx_batch_set_path_margins")
    return b
end

function path_margins(b::Batch)
    pm = Array{Float64,3}(undef, PMARG_N, b.cache.problem.K + 1, b.B)
    check(b.cache.ctx, ccall((:scvx_batch_get_path_margins, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), b.h, pm), "scvx_batch_get_path_margins")
    return pm
end

# min(nsigma s(k), cap width_k) for the constraints in the mask `which` (MARGIN_*), the others stay as they are
function margins_from_cov!(b::Batch, S0::Array{Float64,3}; which::Integer=MARGIN_ALL, nsigma::Real=3.0, cap::Real=0.25, w=nothing, q=1.0,
                           r=1.0, qf=100.0, psig::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx))
    size(S0) == (14, 14, b.B) || error("S0 must be 14 x 14 x B")
    ps = psig ? Array{Float64,3}(undef, PSIG_N, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv check(b.cache.ctx, ccall((:scvx_batch_margins_from_cov, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Cuint, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, _cov_opt(wv), Float64(nsigma), Float64(cap), UInt32(which), _cov_opt(ps)),
        "scvx_batch_margins_from_cov")
    return ps
end

# psig 5 x (K+1) x B of any plans (host arrays, as covariance(cache, ...)): (report, psig)
function path_sigma(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, deriv::Array{Float64,4}, gain::Array{Float64,4},
                    S0::Array{Float64,3}; w=nothing)
    K = size(x, 2) - 1; B = size(x, 3)
    size(S0) == (14, 14, B) || error("S0 must be 14 x 14 x B")
    report = Matrix{Float64}(undef, COV_NREP, B)
    ps = Array{Float64,3}(undef, PSIG_N, K + 1, B)
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv check(cache.ctx, ccall((:scvx_cov_path_sigma_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, deriv, gain, S0, _cov_opt(wv), report, ps), "scvx_cov_path_sigma_f64_host")
    return report, ps
end

path_sigma_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, deriv_dev::Ptr{Cdouble}, gain_dev::Ptr{Cdouble},
                S0_dev::Ptr{Cdouble}, w::Union{Nothing,Vector{Float64}}, report_dev::Ptr{Cdouble}, psig_dev::Ptr{Cdouble}) =
    GC.@preserve w check(cache.ctx, ccall((:scvx_cov_path_sigma_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, _cov_opt(w), report_dev, psig_dev), "scvx_cov_path_sigma_f64")

# ---- back-offs from the analysis of the loop flown on an estimate (new) --------------------------------------------------------
# include/scvx.h, scvx_batch_margins_from_nav: margins_from_cov! with the s(k) of the closed loop fed an estimate.  N0 14 x 14 x B,
# H and rm as navigation(b, ...) takes them.
function margins_from_nav!(b::Batch, S0::Array{Float64,3}, N0::Array{Float64,3}, H, rm;
                           which::Integer=MARGIN_ALL, nsigma::Real=3.0, cap::Real=0.25, w=nothing, q=1.0, r=1.0, qf=100.0, psig::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx))
    size(S0) == (14, 14, b.B) || error("S0 must be 14 x 14 x B")
    size(N0) == (14, 14, b.B) || error("N0 must be 14 x 14 x B")
    m, Hm, rmv = _nav_model(H, rm)
    ps = psig ? Array{Float64,3}(undef, PSIG_N, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv check(b.cache.ctx, ccall((:scvx_batch_margins_from_nav, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Cuint, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, N0, m, _cov_opt(Hm), _cov_opt(rmv), _cov_opt(wv), Float64(nsigma),
        Float64(cap), UInt32(which), _cov_opt(ps)), "scvx_batch_margins_from_nav")
    return ps
end
margins_from_nav(b::Batch, S0, N0, H, rm; kw...) = margins_from_nav!(b, S0, N0, H, rm; kw...)

# psig 5 x (K+1) x B of any plans flown on an estimate (host arrays): (report, navrep, psig)
function nav_path_sigma(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, deriv::Array{Float64,4}, gain::Array{Float64,4},
                        S0::Array{Float64,3}, N0::Array{Float64,3}, H, rm; w=nothing)
    K = size(x, 2) - 1; B = size(x, 3)
    size(S0) == (14, 14, B) || error("S0 must be 14 x 14 x B")
    size(N0) == (14, 14, B) || error("N0 must be 14 x 14 x B")
    m, Hm, rmv = _nav_model(H, rm)
    report = Matrix{Float64}(undef, COV_NREP, B)
    navrep = Matrix{Float64}(undef, NAV_NREP, B)
    ps = Array{Float64,3}(undef, PSIG_N, K + 1, B)
    wv = w === nothing ? nothing : _track_w(w, 14)
    GC.@preserve wv Hm rmv check(cache.ctx, ccall((:scvx_nav_path_sigma_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, deriv, gain, S0, N0, m, _cov_opt(Hm), _cov_opt(rmv), _cov_opt(wv), report, navrep, ps),
        "scvx_nav_path_sigma_f64_host")
    return report, navrep, ps
end

nav_path_sigma_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, deriv_dev::Ptr{Cdouble}, gain_dev::Ptr{Cdouble},
                    S0_dev::Ptr{Cdouble}, N0_dev::Ptr{Cdouble}, m::Int, H::Union{Nothing,Matrix{Float64}}, rm::Union{Nothing,Vector{Float64}},
                    w::Union{Nothing,Vector{Float64}}, report_dev::Ptr{Cdouble}, navrep_dev::Ptr{Cdouble}, psig_dev::Ptr{Cdouble}) =
    GC.@preserve H rm w check(cache.ctx, ccall((:scvx_nav_path_sigma_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, N0_dev, m, _cov_opt(H), _cov_opt(rm), _cov_opt(w), report_dev, navrep_dev,
        psig_dev), "scvx_nav_path_sigma_f64")

# multi-GPU (one Julia process per GPU): rank 0 draws the id, the host ships its 128 bytes (Distributed / MPI.jl / a file)
unique_id() = (id = Vector{UInt8}(undef, 128); ccall((:scvx_comm_unique_id, LIB), Cint, (Ptr{UInt8},), id) == 0 || error("RCCL unavailable"); id)
comm_create!(c::Cache, id::Vector{UInt8}, rank::Int, world::Int) =
    check(c.ctx, ccall((:scvx_comm_create, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), c.ctx, id, rank, world), "scvx_comm_create")
# out_dev: device pointer to world x B x ((K+1)*(14+NU)+1) doubles (e.g. an AMDGPU.jl ROCArray)
allgather_trajectories!(b::Batch, out_dev::Ptr{Cdouble}) =
    check(b.cache.ctx, ccall((:scvx_allgather_trajectories, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), b.h, out_dev), "scvx_allgather_trajectories")

# ---- drop-in by dispatch: the reference's OWN call sites run unedited -----------------------------------------------------
# install!() defines methods IN the reference's modules with the reference's exact argument lists (dynamics.jl:141, 258, 315,
# 321; rocketland.jl:34, 226, 432), so that the recipe of rocketland.jl:26-32
#     Dynamics.make_dynamics_module(RocketlandDefns.ProbInfo(prob))
#     cache = Dynamics.IntegratorCache(prob, RocketlandDefns.ProbInfo(prob), Linearizer)
#     pi = Rocketland.create_initial(prob, cache);  pi, nu, dJ = Rocketland.solve_step(pi, cache)
# reaches the HIP path.  The reference's IntegratorCache (master.jl:113-120) has untyped fields: the device Cache rides in
# `sim_prob`.  ProblemIteration.model is a ProblemModel of MOI handles (master.jl:96-111): a placeholder is built whose untyped
# `debug` field carries the device Batch.  An AtmosphericData problem needs its raw tables once: ScvxAMD.TABLES[] = (drag, lift, trq).
# The build's model extensions reach the installed methods through ScvxAMD.MODEL_FLAGS[] (default 0, the reference's model), e.g.
# MODEL_FLAGS[] = MODEL_AERO_TORQUE to add the aerodynamic body torque of an AtmosphericData problem.
const TABLES = Ref{Any}(nothing)
const MODEL_FLAGS = Ref{Int}(0)
const HOST = parentmodule(@__MODULE__)     # where master.jl included Dynamics / Rocketland / FirstRound
device_cache(c::IntegratorCache) = c.sim_prob::Cache
device_batch(it::ProblemIteration) = it.model.debug::Batch

function placeholder_model(b::Batch)
    MOI = HOST.RocketlandDefns.MOI
    vi = MOI.VariableIndex(0); va = Array{MOI.VariableIndex,2}(undef, 0, 0)
    ci = MOI.ConstraintIndex{MOI.VectorAffineFunction{Float64},MOI.Zeros}(0)
    ProblemModel(MOI.Utilities.Model{Float64}(), va, va, va, va, vi, va, vi, ci, ci, MOI.ConstraintIndex[], ci, ci, b)
end
reference_iteration(it::Iteration, cache::IntegratorCache) =
    ProblemIteration(it.problem, cache, it.sigma, it.about, it.dynam, placeholder_model(it.model), it.iter, it.rk, it.cost)

# ---- vehicle errors in the first-order analyses (new) ------------------------------------------------------------------------------
# include/scvx.h, "VEHICLE ERRORS in the first-order analyses": the six errors of the sampled calls as consider parameters, sp their
# standard deviations (there is no mu).  vtile 14 x 2 x K x B: d x_{k+1} / d theta_ISP and / d theta_AERO of every segment.
const VTILE_N = 2
const VEH_N = 6     # SCVX_VEH_N
_veh_sp(sp) = (length(sp) == VEH_N || error("sp must have $(VEH_N) components"); Vector{Float64}(sp))

function vehicle_tiles(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, sigma::Vector{Float64})
    K = size(x, 2) - 1; B = size(x, 3)
    vt = Array{Float64,4}(undef, 14, VTILE_N, K, B)
    check(cache.ctx, ccall((:scvx_vehicle_tiles_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, sigma, vt), "scvx_vehicle_tiles_f64_host")
    return vt
end

vehicle_tiles_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, sigma_dev::Ptr{Cdouble}, vtile_dev::Ptr{Cdouble}) =
    check(cache.ctx, ccall((:scvx_vehicle_tiles_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, sigma_dev, vtile_dev), "scvx_vehicle_tiles_f64")

# any plans (host arrays, as covariance(cache, ...)) with vehicle errors: (report, psig, sig, covK, cov, sens); sens 6 x n x (K+1) x B
function covariance_vehicle(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, deriv::Array{Float64,4}, gain::Array{Float64,4},
                            S0::Array{Float64,3}, sp; vtile=nothing, w=nothing, dense::Bool=false)
    K = size(x, 2) - 1; B = size(x, 3); n = 14 + size(u, 1)
    size(S0) == (14, 14, B) || error("S0 must be 14 x 14 x B")
    report = Matrix{Float64}(undef, COV_NREP, B)
    ps = Array{Float64,3}(undef, PSIG_N, K + 1, B)
    sig = dense ? Array{Float64,3}(undef, n, K + 1, B) : nothing
    covK = dense ? Array{Float64,3}(undef, n, n, B) : nothing
    cov = dense ? Array{Float64,4}(undef, n, n, K + 1, B) : nothing
    sens = dense ? Array{Float64,4}(undef, VEH_N, n, K + 1, B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    spv = _veh_sp(sp)
    GC.@preserve wv spv check(cache.ctx, ccall((:scvx_cov_vehicle_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, deriv, gain, S0, _cov_opt(wv), report, ps, _cov_opt(sig), _cov_opt(covK), _cov_opt(cov), _cov_opt(vtile),
        spv, _cov_opt(sens)), "scvx_cov_vehicle_f64_host")
    return report, ps, sig, covK, cov, sens
end

covariance_vehicle_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, deriv_dev::Ptr{Cdouble},
                        gain_dev::Ptr{Cdouble}, S0_dev::Ptr{Cdouble}, w::Union{Nothing,Vector{Float64}}, report_dev::Ptr{Cdouble},
                        psig_dev::Ptr{Cdouble}, sig_dev::Ptr{Cdouble}, covK_dev::Ptr{Cdouble}, cov_dev::Ptr{Cdouble},
                        vtile_dev::Ptr{Cdouble}, sp::Vector{Float64}, sens_dev::Ptr{Cdouble}) =
    GC.@preserve w sp check(cache.ctx, ccall((:scvx_cov_vehicle_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, _cov_opt(w), report_dev, psig_dev, sig_dev, covK_dev, cov_dev,
        vtile_dev, sp, sens_dev), "scvx_cov_vehicle_f64")

# the same flown on an estimate: (report, navrep, psig, sig, navsig, kf, joint, sens)
function navigation_vehicle(cache::Cache, x::Array{Float64,3}, u::Array{Float64,3}, deriv::Array{Float64,4}, gain::Array{Float64,4},
                            S0::Array{Float64,3}, N0::Array{Float64,3}, H, rm, sp; vtile=nothing, w=nothing, dense::Bool=false)
    K = size(x, 2) - 1; B = size(x, 3); n = 14 + size(u, 1); N = n + 14
    (size(S0) == (14, 14, B) && size(N0) == (14, 14, B)) || error("S0 and N0 must be 14 x 14 x B")
    m, Hm, rmv = _nav_model(H, rm)
    report = Matrix{Float64}(undef, COV_NREP, B)
    navrep = Matrix{Float64}(undef, NAV_NREP, B)
    ps = Array{Float64,3}(undef, PSIG_N, K + 1, B)
    sig = dense ? Array{Float64,3}(undef, n, K + 1, B) : nothing
    navsig = dense ? Array{Float64,3}(undef, 14, K + 1, B) : nothing
    kf = dense && m > 0 ? Array{Float64,4}(undef, m, 14, K, B) : nothing
    joint = dense ? Array{Float64,4}(undef, N, N, K + 1, B) : nothing
    sens = dense ? Array{Float64,4}(undef, VEH_N, n, K + 1, B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    spv = _veh_sp(sp)
    GC.@preserve wv Hm rmv spv check(cache.ctx, ccall((:scvx_nav_cov_vehicle_f64_host, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x, u, deriv, gain, S0, N0, m, _cov_opt(Hm), _cov_opt(rmv), _cov_opt(wv), report, navrep, ps, _cov_opt(sig),
        _cov_opt(navsig), _cov_opt(kf), _cov_opt(joint), _cov_opt(vtile), spv, _cov_opt(sens)), "scvx_nav_cov_vehicle_f64_host")
    return report, navrep, ps, sig, navsig, kf, joint, sens
end

navigation_vehicle_dev!(cache::Cache, B::Int, K::Int, x_dev::Ptr{Cdouble}, u_dev::Ptr{Cdouble}, deriv_dev::Ptr{Cdouble},
                        gain_dev::Ptr{Cdouble}, S0_dev::Ptr{Cdouble}, N0_dev::Ptr{Cdouble}, m::Int, H, rm,
                        w::Union{Nothing,Vector{Float64}}, report_dev::Ptr{Cdouble}, navrep_dev::Ptr{Cdouble}, psig_dev::Ptr{Cdouble},
                        sig_dev::Ptr{Cdouble}, navsig_dev::Ptr{Cdouble}, kf_dev::Ptr{Cdouble}, joint_dev::Ptr{Cdouble},
                        vtile_dev::Ptr{Cdouble}, sp::Vector{Float64}, sens_dev::Ptr{Cdouble}) =
    GC.@preserve w H rm sp check(cache.ctx, ccall((:scvx_nav_cov_vehicle_f64, LIB), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        cache.ctx, B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, N0_dev, m, _cov_opt(H), _cov_opt(rm), _cov_opt(w), report_dev,
        navrep_dev, psig_dev, sig_dev, navsig_dev, kf_dev, joint_dev, vtile_dev, sp, sens_dev), "scvx_nav_cov_vehicle_f64")

# the batch-level forms on the current accepted iterate: the vehicle tiles of the iterate, then the analysis
function covariance_vehicle(b::Batch, S0::Array{Float64,3}, sp; w=nothing, q=1.0, r=1.0, qf=100.0, dense::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx)); n = 14 + NU
    size(S0) == (14, 14, b.B) || error("S0 must be 14 x 14 x B")
    report = Matrix{Float64}(undef, COV_NREP, b.B)
    sig = dense ? Array{Float64,3}(undef, n, K + 1, b.B) : nothing
    covK = dense ? Array{Float64,3}(undef, n, n, b.B) : nothing
    cov = dense ? Array{Float64,4}(undef, n, n, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    spv = _veh_sp(sp)
    GC.@preserve wv spv check(b.cache.ctx, ccall((:scvx_batch_cov_veh, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, _cov_opt(wv), report, _cov_opt(sig), _cov_opt(covK), _cov_opt(cov), spv),
        "scvx_batch_cov_veh")
    return report, sig, covK, cov
end

function navigation_vehicle(b::Batch, S0::Array{Float64,3}, N0::Array{Float64,3}, H, rm, sp; w=nothing, q=1.0, r=1.0, qf=100.0,
                            dense::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx)); n = 14 + NU; N = n + 14
    (size(S0) == (14, 14, b.B) && size(N0) == (14, 14, b.B)) || error("S0 and N0 must be 14 x 14 x B")
    m, Hm, rmv = _nav_model(H, rm)
    report = Matrix{Float64}(undef, COV_NREP, b.B)
    navrep = Matrix{Float64}(undef, NAV_NREP, b.B)
    sig = dense ? Array{Float64,3}(undef, n, K + 1, b.B) : nothing
    navsig = dense ? Array{Float64,3}(undef, 14, K + 1, b.B) : nothing
    kf = dense && m > 0 ? Array{Float64,4}(undef, m, 14, K, b.B) : nothing
    joint = dense ? Array{Float64,4}(undef, N, N, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    spv = _veh_sp(sp)
    GC.@preserve wv Hm rmv spv check(b.cache.ctx, ccall((:scvx_batch_nav_cov_veh, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, N0, m, _cov_opt(Hm), _cov_opt(rmv), _cov_opt(wv), report, navrep,
        _cov_opt(sig), _cov_opt(navsig), _cov_opt(kf), _cov_opt(joint), spv), "scvx_batch_nav_cov_veh")
    return report, navrep, sig, navsig, kf, joint
end

function margins_from_cov_vehicle!(b::Batch, S0::Array{Float64,3}, sp; which::Integer=MARGIN_ALL, nsigma::Real=3.0, cap::Real=0.25,
                                   w=nothing, q=1.0, r=1.0, qf=100.0, psig::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx))
    size(S0) == (14, 14, b.B) || error("S0 must be 14 x 14 x B")
    ps = psig ? Array{Float64,3}(undef, PSIG_N, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    spv = _veh_sp(sp)
    GC.@preserve wv spv check(b.cache.ctx, ccall((:scvx_batch_margins_from_cov_veh, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Cuint, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, _cov_opt(wv), Float64(nsigma), Float64(cap), UInt32(which),
        _cov_opt(ps), spv), "scvx_batch_margins_from_cov_veh")
    return ps
end

function margins_from_nav_vehicle!(b::Batch, S0::Array{Float64,3}, N0::Array{Float64,3}, H, rm, sp; which::Integer=MARGIN_ALL,
                                   nsigma::Real=3.0, cap::Real=0.25, w=nothing, q=1.0, r=1.0, qf=100.0, psig::Bool=false)
    K = b.cache.problem.K
    NU = Int(ccall((:scvx_control_dim, LIB), Cint, (Ptr{Cvoid},), b.cache.ctx))
    (size(S0) == (14, 14, b.B) && size(N0) == (14, 14, b.B)) || error("S0 and N0 must be 14 x 14 x B")
    m, Hm, rmv = _nav_model(H, rm)
    ps = psig ? Array{Float64,3}(undef, PSIG_N, K + 1, b.B) : nothing
    wv = w === nothing ? nothing : _track_w(w, 14)
    spv = _veh_sp(sp)
    GC.@preserve wv Hm rmv spv check(b.cache.ctx, ccall((:scvx_batch_margins_from_nav_veh, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Cuint, Ptr{Cdouble}, Ptr{Cdouble}),
        b.h, _track_w(q, 14), _track_w(r, NU), _track_w(qf, 14), S0, N0, m, _cov_opt(Hm), _cov_opt(rmv), _cov_opt(wv), Float64(nsigma),
        Float64(cap), UInt32(which), _cov_opt(ps), spv), "scvx_batch_margins_from_nav_veh")
    return ps
end

function install!()
    @eval HOST.Dynamics begin
        function make_dynamics_module(info::ProbInfo)
            Core.eval(Main, :(Linearizer = nothing))     # the recipe passes `Linearizer` on: nothing is generated on this path
            return nothing
        end
        function (::Type{IntegratorCache})(prob::DescentProblem, info::ProbInfo, lin_mod)
            dc = $(@__MODULE__).Cache(prob; tables=$(@__MODULE__).TABLES[], model_flags=$(@__MODULE__).MODEL_FLAGS[])
            return IntegratorCache(dc, nothing, nothing, nothing, nothing, info)
        end
        function predict_state(initial_state, uk, up, sigma, dt, pinfo, cache)
            return $(@__MODULE__).predict_state(initial_state, uk, up, sigma, dt, pinfo, $(@__MODULE__).device_cache(cache))
        end
        function linearize_dynamics(states::Array{LinPoint,1}, tf_guess::Float64, base_dt::Float64, cache::IntegratorCache)
            return $(@__MODULE__).linearize_dynamics(states, tf_guess, base_dt, $(@__MODULE__).device_cache(cache))
        end
    end
    @eval HOST.Rocketland begin
        function create_initial(problem::DescentProblem, linear_cache::IntegratorCache)
            it = $(@__MODULE__).create_initial(problem, $(@__MODULE__).device_cache(linear_cache))
            return $(@__MODULE__).reference_iteration(it, linear_cache)
        end
        function solve_step(iteration::ProblemIteration, linear_cache::IntegratorCache)
            b = $(@__MODULE__).device_batch(iteration)
            st, nu, dj = $(@__MODULE__).step!(b)
            st[1] in (3, 4, 5) && error("Non-optimal result $($(@__MODULE__).STATUS_NAME[st[1]]) exiting")   # rocketland.jl:273-276
            return $(@__MODULE__).reference_iteration($(@__MODULE__).iteration(b), linear_cache), nu[1], dj[1]
        end
        # rocketland.jl:432 types `cache::LinearCache`, a name that exists nowhere at HEAD (SURVEY F4): the working type is used
        function solve_problem(iprob::DescentProblem, cache::IntegratorCache)
            prob = create_initial(iprob, cache)
            cnu = Inf; cdel = Inf; iter = 1
            while (iprob.nuTol < cnu || iprob.delTol < cdel) && iter < iprob.imax
                prob, cnu, cdel = solve_step(prob, cache)
                iter = iter + 1
            end
            return prob, cnu, cdel
        end
    end
    return nothing
end
end

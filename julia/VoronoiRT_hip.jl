# VoronoiRT_hip.jl -- reference-side binding of libvrt_hip.so (include/voronoirt.h).
#
# `include` this file AFTER VoronoiRT.jl.  It redefines, inside the reference's module,
#   * both methods of `J_λ_voronoi` (src/lambda_iteration.jl:60-113, the line case, and
#     src/lambda_continuum.jl:27-56, the continuum case) so that the angle x wavelength loop the
#     reference threads over λ becomes ONE batched device solve -- the line case through
#     vrt_plan_execute_line: seven per-site vectors + S go in, J comes out, the Voigt profiles and
#     α_tot (nλ, n, n_angles) are made on the device and never exist on the host,
#   * `Λ_voronoi` (src/lambda_iteration.jl:205-300) over vrt_lambda_create / _iterate / _get: the loop's
#     state lives on the device, per iteration only the criterion's scalar comes back (plus the
#     populations and S_new the reference checkpoints); with ENV["VRT_DEVICES"] = "0,1,...,7" the same loop
#     runs across those GPUs (vrt_multi_create + vrt_multi_lambda_*: wavelength blocks per device, one RCCL
#     all-reduce of the rate-integral shares per iteration), and
#   * `Delaunay_upII` / `Delaunay_downII` (src/irregular_ray_tracing.jl:15-82, :96-163) for the
#     direct call sites in compare_searchlight.jl (:113,129,434),
#   * `short_characteristics_up/down` (src/characteristics.jl:19-95, :110-180),
#   * and adds `Λ_regular` (src/lambda_iteration.jl:116-205) over vrt_regular_lambda_*: the regular half of the
#     comparison with the same device-resident loop,
#   * and the 4-argument `Λ_voronoi` / `Λ_regular` of src/lambda_continuum.jl:109-160, :58-107 (the continuum scattering
#     loop of compare_continuum.jl) over vrt_continuum_* / vrt_regular_continuum_*: `Λ_continuum`, `Λ_continuum_regular`.
# The physics that produces S, α and I_0 (γ, damping, Voigt profile, αline_λ, B_λ) stays in Julia
# exactly as the reference writes it; only the formal solves leave the process.
#
# Julia is not available in the build image: this file is shipped UNTESTED by execution.
# examples/c_caller.c plays exactly the callers written below -- same arrays, same call sequences:
# scenario 2 the batched J_λ_voronoi, scenario 3 the Λ_voronoi loop, scenario 4 that loop across several
# device handles -- and is checked against the
# oracle on the GPU (tests/test_gpu_parity.py).
#
# Unitful quantities are bit-identical to Float64 in memory, so `ustrip.(x)` gives the plain
# double* the C ABI takes.  Julia arrays are column-major and 1-based, exactly the conventions of
# the C ABI, so no transposition or index shift happens anywhere.
#
# `ccall` needs its (symbol, library) pair to be a constant expression, so every entry point gets
# its own literal-symbol wrapper below (no symbol is passed through a variable).

module VoronoiRTHip

using Unitful
using Libdl
import ..VoronoiRT
import ..VoronoiRT: VoronoiSites, HydrogenicLine, read_quadrature

const libvrt = get(ENV, "VRT_LIB", joinpath(@__DIR__, "..", "voronoirt_amd", "libvrt_hip.so"))

# entry points chosen at run time (one device or several: Λ below) are called through dlsym'd function pointers
const LIBVRT_HANDLE = Ref{Ptr{Cvoid}}(C_NULL)
# the companion library of include/voronoirt_multi_accel.h (it links libvrt_hip.so): vrt_multi_lambda_set_acceleration / _last_acceleration
const libvrt_multi_accel = joinpath(dirname(abspath(libvrt)), "libvrt_hip_multi_accel.so")   # beside the library it links
const LIBVRT_MULTI_ACCEL_HANDLE = Ref{Ptr{Cvoid}}(C_NULL)
function libvrt_multi_accel_handle()
    libvrt_handle()
    LIBVRT_MULTI_ACCEL_HANDLE[] == C_NULL && (LIBVRT_MULTI_ACCEL_HANDLE[] = dlopen(libvrt_multi_accel))
    return LIBVRT_MULTI_ACCEL_HANDLE[]
end
function libvrt_handle()
    LIBVRT_HANDLE[] == C_NULL && (LIBVRT_HANDLE[] = dlopen(libvrt))
    return LIBVRT_HANDLE[]
end

vrt_error() = unsafe_string(ccall((:vrt_last_error, libvrt), Cstring, ()))
check(rc::Cint) = rc == 0 ? nothing : error("libvrt_hip error $rc: $(vrt_error())")

const VRT_ALPHA_SITE = Cint(0)            # α[n]
const VRT_ALPHA_SITE_LAM = Cint(1)        # α[nλ, n]
const VRT_ALPHA_ANGLE_SITE_LAM = Cint(2)  # α[nλ, n, n_angles]
const VRT_ALPHA_ANGLE_NATIVE = Cint(3)    # per angle in the library's own layout (vrt_line_opacity_dev writes it)
const VRT_ALPHA_SITE_LAM_NATIVE = Cint(4) # α[nλ, n] in sweep order, both directions (vrt_plan_to_native_dev), with vrt_plan_execute_native_dev

# ---- one device-resident grid handle per VoronoiSites object -----------------------------------
const GRIDS = IdDict{Any,Ptr{Cvoid}}()

function grid_handle(sites::VoronoiSites; device::Integer=0)
    get!(GRIDS, sites) do
        pos = Matrix{Float64}(ustrip.(u"m", sites.positions))    # (3, n) z,x,y
        bounds = Float64[ustrip(u"m", b) for b in (sites.z_min, sites.z_max, sites.x_min,
                                                   sites.x_max, sites.y_min, sites.y_max)]
        nbr = Matrix{Int64}(sites.neighbours)                    # (n, D+1), column 1 = count
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve pos bounds nbr begin
            check(ccall((:vrt_grid_create, libvrt), Cint,
                        (Int64, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
                        sites.n, pos, nbr, size(nbr, 2), bounds, device, out))
        end
        out[]
    end
end

# ---- one plan (upwind tables + sweep schedule) per (grid, quadrature, n_sweeps) -----------------
const PLANS = Dict{Tuple{Ptr{Cvoid},String,Int},Ptr{Cvoid}}()

direction(θ, ϕ) = [cos(θ*π/180), cos(ϕ*π/180)*sin(θ*π/180), sin(ϕ*π/180)*sin(θ*π/180)]   # lambda_iteration.jl:87

function plan_handle(sites::VoronoiSites, quadrature::String, n_sweeps::Int)
    g = grid_handle(sites)
    get!(PLANS, (g, quadrature, n_sweeps)) do
        weights, θ, ϕ, n_angles = read_quadrature(quadrature)
        k = Matrix{Float64}(undef, 3, n_angles)
        for i in 1:n_angles
            k[:, i] = direction(θ[i], ϕ[i])
        end
        # the reference branches on θ in degrees (lambda_iteration.jl:98,104), not on sign(k_z)
        dirs = Cint[θ[i] > 90 ? 1 : (θ[i] < 90 ? -1 : 0) for i in 1:n_angles]
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve k dirs begin
            check(ccall((:vrt_plan_create_ex, libvrt), Cint,
                        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Cint}, Cint, Ref{Ptr{Cvoid}}),
                        g, n_angles, k, dirs, n_sweeps, out))
        end
        out[]
    end
end

# ---- several GPUs of the node from this one Julia process: ENV["VRT_DEVICES"] = "0,1,2,3,4,5,6,7" -------------
# (vrt_multi_*: a grid + plan per device and an in-process RCCL communicator; the Λ-iteration then runs as
# vrt_multi_lambda_*: wavelength blocks per device, ONE all-reduce of the rate-integral shares per iteration)
vrt_devices() = haskey(ENV, "VRT_DEVICES") && !isempty(ENV["VRT_DEVICES"]) ?
                Cint[parse(Cint, d) for d in split(ENV["VRT_DEVICES"], ",")] : Cint[]

const MULTIS = Dict{Tuple{UInt,String,Int},Ptr{Cvoid}}()

function multi_handle(sites::VoronoiSites, quadrature::String, n_sweeps::Int)
    get!(MULTIS, (objectid(sites), quadrature, n_sweeps)) do
        devices = vrt_devices()
        pos = Matrix{Float64}(ustrip.(u"m", sites.positions))
        bounds = Float64[ustrip(u"m", b) for b in (sites.z_min, sites.z_max, sites.x_min,
                                                   sites.x_max, sites.y_min, sites.y_max)]
        nbr = Matrix{Int64}(sites.neighbours)
        weights, θ, ϕ, n_angles = read_quadrature(quadrature)
        k = Matrix{Float64}(undef, 3, n_angles)
        for i in 1:n_angles
            k[:, i] = direction(θ[i], ϕ[i])
        end
        dirs = Cint[θ[i] > 90 ? 1 : (θ[i] < 90 ? -1 : 0) for i in 1:n_angles]
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve devices pos bounds nbr k dirs begin
            check(ccall((:vrt_multi_create, libvrt), Cint,
                        (Cint, Ptr{Cint}, Int64, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Int64, Ptr{Float64},
                         Ptr{Cint}, Cint, Ref{Ptr{Cvoid}}),
                        length(devices), devices, sites.n, pos, nbr, size(nbr, 2), bounds, n_angles, k, dirs, n_sweeps, out))
        end
        out[]
    end
end

"""
    execute(plan, S, α, mode, I0_up, weights) -> J

One call = every angle x every wavelength of the quadrature (vrt_plan_execute).  `S` is (nλ, n),
`α` is `[n]`, `(nλ, n)` or `(nλ, n, n_angles)` according to `mode`, `I0_up` is
(nλ, layers_up[2]-1) ordered like perm_up (lambda_iteration.jl:99-101); down rays start from zeros
(:105-106), which is what a NULL I0_down means.
"""
function execute(plan::Ptr{Cvoid}, S::Matrix{Float64}, α::Array{Float64}, mode::Cint,
                 I0_up::Matrix{Float64}, weights::Vector{Float64})
    nλ, n = size(S)
    J = similar(S)
    GC.@preserve S α I0_up weights J begin
        check(ccall((:vrt_plan_execute, libvrt), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    plan, nλ, nλ, S, α, mode, I0_up, C_NULL, weights, J, C_NULL))
    end
    return J
end

# ---- J_λ_voronoi, line case: src/lambda_iteration.jl:60-113 -------------------------------------
# What stays in Julia: γ_constant of the current populations (:72-75) and damping_λ (:77-80; the
# caller, Λ_voronoi, hands it on to calculate_R).  What leaves: compute_voigt_profile per angle (:89),
# αline_λ + α_cont (:93-96) and the n_angles x nλ formal solves (:98-108) -- one call,
# vrt_plan_execute_line, with the per-site ingredients of α_tot instead of α_tot itself.
const I_unit = u"kW*m^-2*nm^-1"

# αline_λ for a unit profile (1 m^-1): the λ-independent factor h c_0/(4π λ0) (n_i B_ij - n_j B_ji) of
# src/line.jl:219-225, evaluated by the reference's own function so that no unit is guessed here
line_strength(line::HydrogenicLine, n_j, n_i) =
    Vector{Float64}(ustrip.(u"m^-1", VoronoiRT.αline_λ(line, fill(1.0u"m^-1", length(n_i)), n_j, n_i)))

function site_velocity(sites::VoronoiSites)               # (3, n) rows z, x, y: line_of_sight_velocity, line.jl:198-208
    v = Matrix{Float64}(undef, 3, sites.n)
    v[1, :] = ustrip.(u"m/s", sites.velocity_z); v[2, :] = ustrip.(u"m/s", sites.velocity_x)
    v[3, :] = ustrip.(u"m/s", sites.velocity_y)
    return v
end

function bottom_planck(sites::VoronoiSites, line::HydrogenicLine)
    # I_0 for up rays: B_λ(λ_l, T) of the bottom layer in perm_up order (:99-101); rows = λ
    bottom_layer = sites.layers_up[2] - 1
    bottom_layer_idx = sites.perm_up[1:bottom_layer]
    I0_up = Matrix{Float64}(undef, length(line.λ), bottom_layer)
    for l in eachindex(line.λ)
        I0_up[l, :] = ustrip.(I_unit, VoronoiRT.B_λ.(line.λ[l], sites.temperature[bottom_layer_idx]))
    end
    return I0_up
end

function J_line(S_λ, α_cont, populations, sites::VoronoiSites, line::HydrogenicLine, quadrature::String)
    weights, θ_array, ϕ_array, n_angles = read_quadrature(quadrature)
    nλ, n = size(S_λ)

    γ = VoronoiRT.γ_constant(line, sites.temperature,
                             (populations[:, 1] .+ populations[:, 2]), sites.electron_density)
    damping_λ = Matrix{Float64}(undef, size(S_λ))
    Threads.@threads for l in eachindex(line.λ)
        damping_λ[l, :] = VoronoiRT.damping.(γ, line.λ[l], line.ΔD)
    end

    λ = Vector{Float64}(ustrip.(u"m", line.λ))
    vel = site_velocity(sites)
    ΔD = Vector{Float64}(ustrip.(u"m", line.ΔD))
    γv = Vector{Float64}(ustrip.(u"s^-1", γ))
    strength = line_strength(line, populations[:, 2], populations[:, 1])
    αc = Vector{Float64}(ustrip.(u"m^-1", α_cont))
    S = Matrix{Float64}(ustrip.(I_unit, S_λ))
    I0_up = bottom_planck(sites, line)
    w = Vector{Float64}(weights)
    J = similar(S)
    plan = plan_handle(sites, quadrature, 3)            # n_sweeps = 3, :82
    GC.@preserve λ vel ΔD γv strength αc S I0_up w J begin
        check(ccall((:vrt_plan_execute_line, libvrt), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    plan, nλ, nλ, λ, ustrip(u"m", line.λ0), ustrip(u"m/s", VoronoiRT.c_0), vel, ΔD, γv, strength, αc,
                    S, I0_up, C_NULL, w, J))
    end
    return J * I_unit, damping_λ
end

# ---- Λ_voronoi: src/lambda_iteration.jl:205-300 ----------------------------------------------------
# mirrors `struct vrt_line_case` of include/voronoirt.h field for field (all 8-byte members)
struct LineCase
    nlam::Int64
    lambda::Ptr{Float64}
    blocks::NTuple{6,Int64}
    lambda0::Float64
    c0::Float64
    velocity::Ptr{Float64}
    doppler_width::Ptr{Float64}
    gamma_static::Ptr{Float64}
    gamma_unsold::Ptr{Float64}
    alpha_cont::Ptr{Float64}
    eps::Ptr{Float64}
    temperature::Ptr{Float64}
    atom_density::Ptr{Float64}
    B0::Ptr{Float64}
    lte_populations::Ptr{Float64}
    C::Ptr{Float64}
    planck2::Ptr{Float64}
    sigma_bf1::Ptr{Float64}
    sigma_bf2::Ptr{Float64}
    strength_const::Float64
    Bij::Float64
    Bji::Float64
    sigma_bb_const::Float64
    hc_over_kB::Float64
    pref_ij::Float64
    pref_ji::Float64
end

# ---- the state a line session resumes from (vrt_*_lambda_set_state; src/recover_simulation.jl) -- unrun ----------------
# `a` (nothing, plain numbers or a Unitful array) as a dense Float64 array of the session's dims
function plain_array(a, unit, dims)
    a === nothing && return nothing
    out = Array{Float64}(eltype(a) <: Real ? a : ustrip.(unit, a))
    size(out) == dims || error("the saved state has dims $(size(out)), the case needs $dims")
    return out
end

# S (nλ, n) and populations (n, 3) into the session; `nothing` leaves that half as it is, both `nothing` is no call
function set_state(f::Symbol, ses::Ptr{Cvoid}, S, pops)
    S === nothing && pops === nothing && return
    GC.@preserve S pops check(ccall(dlsym(libvrt_handle(), f), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ses,
                                    S === nothing ? Ptr{Float64}(C_NULL) : pointer(S),
                                    pops === nothing ? Ptr{Float64}(C_NULL) : pointer(pops)))
end

"""
    Λ(ϵ, maxiter, sites, line, quadrature, DATA) -> (J_new, S_new, α_cont, populations)

The reference's Λ_voronoi with its loop body on the device.  Everything Λ_voronoi derives BEFORE the loop
(LTE populations, α_cont, B_0, ε, C: :217-246) is computed by the reference's own functions; the loop
(:253-283) is vrt_lambda_iterate; after every iteration populations and S_new are fetched and written to the
HDF5 file exactly as the reference checkpoints them (:280-281); `criterion` keeps writing the history (:346).
`ng = (start, period)`: second-order Ng acceleration inside the session (vrt_lambda_set_acceleration, or
vrt_multi_lambda_set_acceleration when several devices are listed), the first step after iterate `start`, then every `period`
iterates, both >= 4.  The keyword is unrun: Julia is not installed where the library is built.
`S0` (nλ, n), `populations0` (n, 3), with or without units: the loop starts from them instead of LTE with S = B_0
(vrt_lambda_set_state / vrt_multi_lambda_set_state; the state the reference checkpoints, :280-281) and continues bit for
bit as the run that wrote them; either alone replaces that half.  Unrun as well.
`storage = :f32`: the session holds S, J, B_0, I_0 and α_tot as Float32 (vrt_lambda_create_f32, or
vrt_multi_lambda_create_f32 when several devices are listed: every device then holds its wavelength block as Float32;
arithmetic stays Float64; the patch path only -- the library refuses anything else, there is no Float64 fallback).  J_new
and S_new come back as Float64 arrays of Float32 values; `ng` is an error with it (the Ng kernels work on Float64 planes).
Unrun as well.
`operator = :diagonal`: accelerated Λ-iteration with the diagonal operator Λ* formed on the device from every iterate's
α_tot (vrt_lambda_use_operator): the same fixed point in fewer iterates where ε is small -- what src/rates.jl:1-3 sets
BOOST for.  One device and Float64 storage only (an error with `storage = :f32` or several devices); composes with `ng`,
`S0` and `populations0`.  Unrun as well.
"""
function Λ(ϵ::AbstractFloat, maxiter::Integer, sites::VoronoiSites, line::HydrogenicLine, quadrature::String, DATA::String;
           ng::Union{Nothing,Tuple{Int,Int}}=nothing, S0=nothing, populations0=nothing, storage::Symbol=:f64,
           operator::Union{Nothing,Symbol}=nothing)
    storage in (:f64, :f32) || error("storage must be :f64 or :f32")
    storage == :f32 && ng !== nothing && error("Ng acceleration is not available with storage = :f32")
    operator in (nothing, :diagonal) || error("operator must be nothing or :diagonal")
    operator !== nothing && storage == :f32 && error("operator = :diagonal is not available with storage = :f32")
    operator !== nothing && length(vrt_devices()) > 1 && error("operator = :diagonal is not available on several devices")
    println("---Iterating---")
    LTE_pops = VoronoiRT.LTE_populations(line, sites)
    populations = copy(LTE_pops)
    α_cont = VoronoiRT.α_absorption.(line.λ0, sites.temperature, sites.electron_density * 1.0,
                                     LTE_pops[:, 1] .+ LTE_pops[:, 2], LTE_pops[:, 3]) .+
             VoronoiRT.α_scattering.(line.λ0, sites.electron_density, LTE_pops[:, 1])
    nλ, n = length(line.λ), sites.n
    B_0 = Matrix{Float64}(undef, nλ, n)
    for l in eachindex(line.λ)
        B_0[l, :] = ustrip.(I_unit, VoronoiRT.B_λ.(line.λ[l], sites.temperature))
    end
    ελ = VoronoiRT.destruction(LTE_pops, sites.electron_density, sites.temperature, line)
    println("Minimum $(minimum(ελ)) destruction probability")
    C = VoronoiRT.calculate_C(sites, LTE_pops)

    # γ_constant (src/broadening.jl:63-82) split into the part that follows the populations -- γ_unsold is linear in
    # the neutral-hydrogen density -- and the rest (natural width + the two Stark terms: n_e and T only)
    one_density = fill(1.0u"m^-3", n)
    γ_unsold_unit = VoronoiRT.γ_unsold.(VoronoiRT.const_unsold(line), sites.temperature, one_density)
    γ_static = VoronoiRT.γ_constant(line, sites.temperature, 0.0 .* one_density, sites.electron_density)

    λ = Vector{Float64}(ustrip.(u"m", line.λ))
    blocks = (Int64(line.λidx[1]), Int64(line.λidx[2]), Int64(line.λidx[2]), Int64(line.λidx[3]),
              Int64(line.λidx[3]), Int64(line.λidx[4]))                    # [lo, hi) 0-based: rates.jl:166-167,181-182
    hc = VoronoiRT.h * VoronoiRT.c_0
    # unit factors the reference gets from Unitful in Rij / Rji (rates.jl:226-364): J is a plain number in I_unit
    pref_ij = ustrip(u"s^-1", 2π / hc * 1u"m" * 1u"m^2" * 1I_unit * 1u"m") / 1000      # the explicit /1000 of :237,263
    pref_ji = ustrip(u"s^-1", 2π / hc * 1u"m" * 1u"m^2" * 1I_unit * 1u"m")
    planck2 = Vector{Float64}(ustrip.(I_unit, 2 * VoronoiRT.h * VoronoiRT.c_0^2 ./ line.λ .^ 5))
    σ1 = Vector{Float64}(ustrip.(u"m^2", VoronoiRT.σic(1, line, line.λ[line.λidx[2]+1:line.λidx[3]])))
    σ2 = Vector{Float64}(ustrip.(u"m^2", VoronoiRT.σic(2, line, line.λ[line.λidx[3]+1:line.λidx[4]])))
    vel = site_velocity(sites)
    ΔD = Vector{Float64}(ustrip.(u"m", line.ΔD))
    γs = Vector{Float64}(ustrip.(u"s^-1", γ_static)); γu = Vector{Float64}(ustrip.(u"s^-1", γ_unsold_unit))
    αc = Vector{Float64}(ustrip.(u"m^-1", α_cont)); εv = Vector{Float64}(ελ)
    T = Vector{Float64}(ustrip.(u"K", sites.temperature))
    atom = Vector{Float64}(ustrip.(u"m^-3", sites.hydrogen_populations))
    lte = Matrix{Float64}(ustrip.(u"m^-3", LTE_pops)); Cm = Array{Float64,3}(ustrip.(u"s^-1", C))
    weights, _, _, _ = read_quadrature(quadrature)
    w = Vector{Float64}(weights)
    # αline_λ = strength_const (n_1 B_ij - n_2 B_ji) φ: the two coefficients per unit density, from αline_λ itself
    a_i = line_strength(line, [0.0u"m^-3"], [1.0u"m^-3"])[1]
    a_j = -line_strength(line, [1.0u"m^-3"], [0.0u"m^-3"])[1]
    # one device: vrt_lambda_* on the plan; ENV["VRT_DEVICES"] lists several: vrt_multi_lambda_* (same arguments)
    multi = length(vrt_devices()) > 1
    plan = multi ? multi_handle(sites, quadrature, 3) : plan_handle(sites, quadrature, 3)
    f_create = multi ? (storage == :f32 ? :vrt_multi_lambda_create_f32 : :vrt_multi_lambda_create) :
               storage == :f32 ? :vrt_lambda_create_f32 : :vrt_lambda_create
    f_iterate = multi ? :vrt_multi_lambda_iterate : :vrt_lambda_iterate
    f_get = multi ? :vrt_multi_lambda_get : :vrt_lambda_get
    f_destroy = multi ? :vrt_multi_lambda_destroy : :vrt_lambda_destroy
    ses = Ref{Ptr{Cvoid}}(C_NULL)
    J = Matrix{Float64}(undef, nλ, n); S = Matrix{Float64}(undef, nλ, n); pops = Matrix{Float64}(undef, n, 3)
    GC.@preserve λ vel ΔD γs γu αc εv T atom B_0 lte Cm planck2 σ1 σ2 w begin
        lc = Ref(LineCase(nλ, pointer(λ), blocks, ustrip(u"m", line.λ0), ustrip(u"m/s", VoronoiRT.c_0), pointer(vel),
                          pointer(ΔD), pointer(γs), pointer(γu), pointer(αc), pointer(εv), pointer(T), pointer(atom),
                          pointer(B_0), pointer(lte), pointer(Cm), pointer(planck2), pointer(σ1), pointer(σ2),
                          1.0, a_i, a_j,
                          ustrip(u"m^3", hc / (4 * π * line.λ0) * line.Bij),     # σ_constant of σij, rates.jl:398: x profile [1/m] = m^2
                          ustrip(u"m*K", hc / VoronoiRT.k_B), pref_ij, pref_ji))
        check(ccall(dlsym(libvrt_handle(), f_create), Cint, (Ptr{Cvoid}, Ref{LineCase}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                    plan, lc, w, ses))
    end
    if ng !== nothing
        f_accel = multi ? :vrt_multi_lambda_set_acceleration : :vrt_lambda_set_acceleration
        check(ccall(dlsym(multi ? libvrt_multi_accel_handle() : libvrt_handle(), f_accel), Cint, (Ptr{Cvoid}, Cint, Cint, Cint),
                    ses[], 2, ng[1], ng[2]))
    end
    operator === :diagonal && check(ccall(dlsym(libvrt_handle(), :vrt_lambda_use_operator), Cint, (Ptr{Cvoid}, Cint), ses[], 1))
    set_state(multi ? :vrt_multi_lambda_set_state : :vrt_lambda_set_state, ses[], plain_array(S0, I_unit, (nλ, n)),
              plain_array(populations0, u"m^-3", (n, 3)))
    ng_applied = Ref{Cint}(0); ng_coeffs = zeros(2)
    i = 0
    diff = Ref{Float64}(1.0)                  # criterion(S_new = B_0, S_old = 0) = |1 - 0/B| = 1, :325-349
    VoronoiRT.write_to_file(diff[], i + 1, DATA)
    while diff[] > ϵ && i < maxiter
        @time check(ccall(dlsym(libvrt_handle(), f_iterate), Cint, (Ptr{Cvoid}, Ref{Float64}), ses[], diff))
        isnan(diff[]) && println("NaN DIFF!")
        println("   Rel. diff.: $(diff[])")
        if ng !== nothing
            f_last = multi ? :vrt_multi_lambda_last_acceleration : :vrt_lambda_last_acceleration
            check(ccall(dlsym(multi ? libvrt_multi_accel_handle() : libvrt_handle(), f_last), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Float64}, Ptr{Float64}),
                        ses[], ng_applied, C_NULL, ng_coeffs))
            ng_applied[] != 0 && println("   Ng step ", ng_applied[] == 1 ? "taken" : "rejected", ": a = $(ng_coeffs[1]), b = $(ng_coeffs[2])")
        end
        GC.@preserve S pops check(ccall(dlsym(libvrt_handle(), f_get), Cint,
                                        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                        ses[], C_NULL, S, pops, C_NULL, C_NULL))
        VoronoiRT.write_to_file(pops * 1u"m^-3", DATA)                    # the checkpoint, :280-281
        VoronoiRT.write_to_file(S * I_unit, DATA)
        i += 1
        VoronoiRT.write_to_file(diff[], i + 1, DATA)                      # convergence history, :346
    end
    GC.@preserve J S pops check(ccall(dlsym(libvrt_handle(), f_get), Cint,
                                      (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                      ses[], J, S, pops, C_NULL, C_NULL))
    ccall(dlsym(libvrt_handle(), f_destroy), Cvoid, (Ptr{Cvoid},), ses[])
    println(i == maxiter ? "Did not converge inside scope" : "Converged in $i iterations")
    return J * I_unit, S * I_unit, α_cont, pops * 1u"m^-3"
end

# ---- Λ_regular: src/lambda_iteration.jl:116-205 ---------------------------------------------------
"""
    Λ_regular(ϵ, maxiter, atmos, line, quadrature, DATA) -> (J_new, S_new, α_cont, populations)

The reference's Λ_regular with its loop body on the device (vrt_regular_lambda_*).  `atmos` is the periodic
atmosphere the reference iterates on (get_atmos(...; periodic=true)): every point, ghost border included, is a
point of the loop.  What Λ_regular derives before the loop (LTE populations, α_cont, ε, B_0, C: :124-157) comes from
the reference's own functions, as in `Λ` above; each iteration is vrt_regular_lambda_iterate, after which
populations and S_new are fetched and checkpointed without the ghost border like the reference (:188-189).
Arrays keep their Julia shapes: (nλ, nz, nx, ny), (nz, nx, ny, 3) and (3, 3, nz, nx, ny) are vrt_line_case's
(nλ, n), (n, 3) and (3, 3, n) with n = nz nx ny.  `ng = (start, period)` as for `Λ`
(vrt_regular_lambda_set_acceleration).  `S0` (nλ, nz, nx, ny), `populations0` (nz, nx, ny, 3), ghost border included,
as for `Λ` (vrt_regular_lambda_set_state).  `operator = :diagonal`: accelerated Λ-iteration with the raster's one-sweep
diagonal Λ* formed on the device from every iterate's per-angle α_tot (vrt_regular_lambda_use_operator), as for `Λ`; it
composes with `ng`, `S0` and `populations0`.  Unrun: Julia is not installed where the library is built.
"""
function Λ_regular(ϵ::AbstractFloat, maxiter::Integer, atmos, line::HydrogenicLine, quadrature::String, DATA::String;
                   ng::Union{Nothing,Tuple{Int,Int}}=nothing, S0=nothing, populations0=nothing,
                   operator::Union{Nothing,Symbol}=nothing)
    operator in (nothing, :diagonal) || error("operator must be nothing or :diagonal")
    LTE_pops = VoronoiRT.LTE_populations(line, atmos)
    α_cont = VoronoiRT.α_absorption.(line.λ0, atmos.temperature, atmos.electron_density * 1.0,
                                     LTE_pops[:, :, :, 1] .+ LTE_pops[:, :, :, 2], LTE_pops[:, :, :, 3]) .+
             VoronoiRT.α_scattering.(line.λ0, atmos.electron_density, LTE_pops[:, :, :, 1])
    ελ = VoronoiRT.destruction(LTE_pops, atmos.electron_density, atmos.temperature, line)
    println("Minimum $(minimum(ελ)) destruction probability")
    nz, nx, ny = size(atmos.temperature)
    nλ = length(line.λ)
    B_0 = Array{Float64,4}(undef, nλ, nz, nx, ny)
    for l in eachindex(line.λ)
        B_0[l, :, :, :] = ustrip.(I_unit, VoronoiRT.B_λ.(line.λ[l], atmos.temperature))
    end
    C = VoronoiRT.calculate_C(atmos, LTE_pops)

    one_density = fill(1.0u"m^-3", nz, nx, ny)                   # γ_constant split as in Λ above
    γ_unsold_unit = VoronoiRT.γ_unsold.(VoronoiRT.const_unsold(line), atmos.temperature, one_density)
    γ_static = VoronoiRT.γ_constant(line, atmos.temperature, 0.0 .* one_density, atmos.electron_density)
    λ = Vector{Float64}(ustrip.(u"m", line.λ))
    blocks = (Int64(line.λidx[1]), Int64(line.λidx[2]), Int64(line.λidx[2]), Int64(line.λidx[3]),
              Int64(line.λidx[3]), Int64(line.λidx[4]))
    hc = VoronoiRT.h * VoronoiRT.c_0
    pref_ij = ustrip(u"s^-1", 2π / hc * 1u"m" * 1u"m^2" * 1I_unit * 1u"m") / 1000
    pref_ji = ustrip(u"s^-1", 2π / hc * 1u"m" * 1u"m^2" * 1I_unit * 1u"m")
    planck2 = Vector{Float64}(ustrip.(I_unit, 2 * VoronoiRT.h * VoronoiRT.c_0^2 ./ line.λ .^ 5))
    σ1 = Vector{Float64}(ustrip.(u"m^2", VoronoiRT.σic(1, line, line.λ[line.λidx[2]+1:line.λidx[3]])))
    σ2 = Vector{Float64}(ustrip.(u"m^2", VoronoiRT.σic(2, line, line.λ[line.λidx[3]+1:line.λidx[4]])))
    vel = Array{Float64,4}(undef, 3, nz, nx, ny)                 # (3, n) rows z, x, y
    vel[1, :, :, :] = ustrip.(u"m/s", atmos.velocity_z); vel[2, :, :, :] = ustrip.(u"m/s", atmos.velocity_x)
    vel[3, :, :, :] = ustrip.(u"m/s", atmos.velocity_y)
    ΔD = Array{Float64,3}(ustrip.(u"m", line.ΔD))
    γs = Array{Float64,3}(ustrip.(u"s^-1", γ_static)); γu = Array{Float64,3}(ustrip.(u"s^-1", γ_unsold_unit))
    αc = Array{Float64,3}(ustrip.(u"m^-1", α_cont)); εv = Array{Float64,3}(ελ)
    T = Array{Float64,3}(ustrip.(u"K", atmos.temperature))
    atom = Array{Float64,3}(ustrip.(u"m^-3", atmos.hydrogen_populations))
    lte = Array{Float64,4}(ustrip.(u"m^-3", LTE_pops)); Cm = Array{Float64,5}(ustrip.(u"s^-1", C))
    a_i = line_strength(line, [0.0u"m^-3"], [1.0u"m^-3"])[1]
    a_j = -line_strength(line, [1.0u"m^-3"], [0.0u"m^-3"])[1]

    weights, θ_array, ϕ_array, n_angles = read_quadrature(quadrature)
    k = Matrix{Float64}(undef, 3, n_angles)
    for i in 1:n_angles
        k[:, i] = direction(θ_array[i], ϕ_array[i])              # :23-26
    end
    dirs = Cint[θ > 90 ? 1 : (θ < 90 ? -1 : 0) for θ in θ_array]  # θ = 90 adds nothing (:37-55)
    w = Vector{Float64}(weights)
    z = Vector{Float64}(ustrip.(u"m", atmos.z)); x = Vector{Float64}(ustrip.(u"m", atmos.x))
    y = Vector{Float64}(ustrip.(u"m", atmos.y))
    reg = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve z x y check(ccall((:vrt_regular_create, libvrt), Cint,
                                   (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
                                   nz, nx, ny, z, x, y, 0, reg))
    ses = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve λ vel ΔD γs γu αc εv T atom B_0 lte Cm planck2 σ1 σ2 k dirs w begin
        lc = Ref(LineCase(nλ, pointer(λ), blocks, ustrip(u"m", line.λ0), ustrip(u"m/s", VoronoiRT.c_0), pointer(vel),
                          pointer(ΔD), pointer(γs), pointer(γu), pointer(αc), pointer(εv), pointer(T), pointer(atom),
                          pointer(B_0), pointer(lte), pointer(Cm), pointer(planck2), pointer(σ1), pointer(σ2),
                          1.0, a_i, a_j, ustrip(u"m^3", hc / (4 * π * line.λ0) * line.Bij),
                          ustrip(u"m*K", hc / VoronoiRT.k_B), pref_ij, pref_ji))
        check(ccall((:vrt_regular_lambda_create, libvrt), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Ref{LineCase}, Cint, Ref{Ptr{Cvoid}}),
                    reg[], n_angles, k, dirs, w, lc, 3, ses))
    end
    J = Array{Float64,4}(undef, nλ, nz, nx, ny); S = Array{Float64,4}(undef, nλ, nz, nx, ny)
    pops = Array{Float64,4}(undef, nz, nx, ny, 3)
    fetch_state(Jp, Sp) = GC.@preserve J S pops check(ccall((:vrt_regular_lambda_get, libvrt), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ses[], Jp, Sp, pops, C_NULL, C_NULL))
    ng !== nothing && check(ccall((:vrt_regular_lambda_set_acceleration, libvrt), Cint, (Ptr{Cvoid}, Cint, Cint, Cint),
                                  ses[], 2, ng[1], ng[2]))
    operator === :diagonal && check(ccall((:vrt_regular_lambda_use_operator, libvrt), Cint, (Ptr{Cvoid}, Cint), ses[], 1))
    set_state(:vrt_regular_lambda_set_state, ses[], plain_array(S0, I_unit, (nλ, nz, nx, ny)),
              plain_array(populations0, u"m^-3", (nz, nx, ny, 3)))
    ng_applied = Ref{Cint}(0); ng_coeffs = zeros(2)
    i = 0
    diff = Ref{Float64}(1.0)                  # criterion(S_new = B_0, S_old = 0) = 1
    VoronoiRT.write_to_file(diff[], i + 1, DATA)
    while diff[] > ϵ && i < maxiter
        @time check(ccall((:vrt_regular_lambda_iterate, libvrt), Cint, (Ptr{Cvoid}, Ref{Float64}), ses[], diff))
        isnan(diff[]) && println("NaN DIFF!")
        println("   Rel. diff.: $(diff[])")
        if ng !== nothing
            check(ccall((:vrt_regular_lambda_last_acceleration, libvrt), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Float64}, Ptr{Float64}),
                        ses[], ng_applied, C_NULL, ng_coeffs))
            ng_applied[] != 0 && println("   Ng step ", ng_applied[] == 1 ? "taken" : "rejected", ": a = $(ng_coeffs[1]), b = $(ng_coeffs[2])")
        end
        fetch_state(C_NULL, pointer(S))
        VoronoiRT.write_to_file(pops[:, 2:end-1, 2:end-1, :] * 1u"m^-3", DATA)     # the checkpoint, :188-189
        VoronoiRT.write_to_file(S[:, :, 2:end-1, 2:end-1] * I_unit, DATA)
        i += 1
        VoronoiRT.write_to_file(diff[], i + 1, DATA)
    end
    fetch_state(pointer(J), pointer(S))
    ccall((:vrt_regular_lambda_destroy, libvrt), Cvoid, (Ptr{Cvoid},), ses[])
    ccall((:vrt_regular_destroy, libvrt), Cvoid, (Ptr{Cvoid},), reg[])
    println(i == maxiter ? "Did not converge inside scope" : "Converged in $i iterations")
    return J * I_unit, S * I_unit, α_cont, pops * 1u"m^-3"
end

# ---- recover_voronoi / recover_regular: src/recover_simulation.jl -- unrun -----------------------------------------------
"""
    recover_voronoi(ϵ, maxiter, quadrature, DATA; ng=nothing) -> (J_new, S_new, α_cont, populations)

The reference's recover_voronoi (src/recover_simulation.jl:103-206): `read_sites(DATA)` (:213-277) rebuilds the sites and
reads the datasets "source_function" (nλ, n) and "populations" (n, 3) the last pass wrote, and `Λ` carries on from them.
`line` is made as the reference makes it there (test_atom(nλ_bb, nλ_bf) on the sites' temperature).  Unrun.
"""
function recover_voronoi(ϵ::AbstractFloat, maxiter::Integer, quadrature::String, DATA::String; ng=nothing)
    println("---Recovering simulation---")
    sites, S_new, populations = VoronoiRT.read_sites(DATA)
    line = HydrogenicLine(VoronoiRT.test_atom(VoronoiRT.nλ_bb, VoronoiRT.nλ_bf)..., sites.temperature)
    return Λ(ϵ, maxiter, sites, line, quadrature, DATA; ng=ng, S0=S_new, populations0=populations)
end

"""
    recover_regular(ϵ, maxiter, quadrature, DATA; ng=nothing) -> (J_new, S_new, α_cont, populations)

The reference's recover_regular (src/recover_simulation.jl:4-101) on the periodic atmosphere of `read_quantities(DATA;
periodic=true)`, whose populations carry the ghost border.  The dataset "source_function" is stored without the border
(src/lambda_iteration.jl:188-189) and gets it back here the way the reference gives it to every field
(`periodic_borders`): the interior resumes exactly, the border points start from their periodic images.  Unrun.
"""
function recover_regular(ϵ::AbstractFloat, maxiter::Integer, quadrature::String, DATA::String; ng=nothing)
    println("---Recovering simulation---")
    atmos, populations, _ = VoronoiRT.read_quantities(DATA; periodic=true)
    S_new = VoronoiRT.h5open(DATA, "r") do file
        VoronoiRT.periodic_borders(read(file, "source_function")[:, :, :, :] * I_unit)
    end
    line = HydrogenicLine(VoronoiRT.test_atom(VoronoiRT.nλ_bb, VoronoiRT.nλ_bf)..., atmos.temperature)
    return Λ_regular(ϵ, maxiter, atmos, line, quadrature, DATA; ng=ng, S0=S_new, populations0=populations)
end

# ---- J_λ_voronoi, continuum case: src/lambda_continuum.jl:27-56 ---------------------------------
# one wavelength (500 nm), α independent of the angle; S_λ and α_cont are n-vectors there
function J_continuum(S_λ::AbstractVector, α_cont::AbstractVector, sites::VoronoiSites, quadrature::String)
    weights, θ_array, ϕ_array, n_points = read_quadrature(quadrature)
    bottom_layer = sites.layers_up[2] - 1
    bottom_layer_idx = sites.perm_up[1:bottom_layer]
    I0_up = reshape(Vector{Float64}(ustrip.(I_unit,
                VoronoiRT.blackbody_λ.(500u"nm", sites.temperature[bottom_layer_idx]))), 1, bottom_layer)
    plan = plan_handle(sites, quadrature, 3)
    S = reshape(Vector{Float64}(ustrip.(I_unit, S_λ)), 1, length(S_λ))
    α = Vector{Float64}(ustrip.(u"m^-1", α_cont))
    J = execute(plan, S, α, VRT_ALPHA_SITE, I0_up, Vector{Float64}(weights))
    return vec(J) * I_unit
end

# ---- Λ_voronoi / Λ_regular, continuum case: src/lambda_continuum.jl:109-160, :58-107 ------------------------
# vrt_continuum_case of include/voronoirt.h
struct ContinuumCase
    nlam::Int64
    alpha::Ptr{Float64}
    eps::Ptr{Float64}
    B0::Ptr{Float64}
    eps_thick::Float64
end

# the loop shared by both grids: `prefix` is :vrt_continuum_ or :vrt_regular_continuum_ spelled out (a ccall's symbol
# must be a literal), so the two callers pass closures
function continuum_loop(ϵ, maxiter, iterate, fetch, last_acc, ng)
    i = 0
    diff = Ref{Float64}(1.0)                  # criterion(S_new = B_0, S_old = 0) = 1 (:145, :92)
    ng_applied = Ref{Cint}(0); ng_coeffs = zeros(2)
    println("Iteration 1...")
    while diff[] > ϵ && i < maxiter           # criterion: diff > ϵ && i < maxiter (:178, :197)
        check(iterate(diff))
        isnan(diff[]) && println("NaN DIFF!")
        println("   Rel. diff.: $(diff[])")
        if ng !== nothing
            check(last_acc(ng_applied, ng_coeffs))
            ng_applied[] != 0 && println("   Ng step ", ng_applied[] == 1 ? "taken" : "rejected", ": a = $(ng_coeffs[1]), b = $(ng_coeffs[2])")
        end
        i += 1
        println("Iteration $(i+1)...")
    end
    check(fetch())
    println(i == maxiter ? "Did not converge inside scope" : "Converged in $i iterations")
end

"""
    Λ_continuum(ϵ, maxiter, sites, quadrature; ng=nothing, S0=nothing, operator=nothing) -> (J_new, S_new, α_cont)

The reference's continuum Λ_voronoi (src/lambda_continuum.jl:109-160) with its loop on the device (vrt_continuum_*).
What it derives before the loop -- LTE populations, α_s, α_a, ε_λ, B_0 at 500 nm (:116-137) -- comes from the reference's
own functions; every iteration is vrt_continuum_iterate, whose scalar is the maximum over thick = ε_λ .> 1e-4.
`ng = (start, period)`: vrt_continuum_set_acceleration; `S0`: a source function to resume from
(vrt_continuum_set_source, the recover_* use of src/recover_simulation.jl).  `operator = :diagonal`: accelerated
Λ-iteration with the local operator Λ* (vrt_continuum_set_operator), which composes with `ng`.  Unrun: Julia is not
installed where the library is built.
"""
function Λ_continuum(ϵ::AbstractFloat, maxiter::Integer, sites::VoronoiSites, quadrature::String;
                     ng::Union{Nothing,Tuple{Int,Int}}=nothing, S0=nothing, operator::Union{Nothing,Symbol}=nothing)
    operator === nothing || operator === :diagonal || throw(ArgumentError("operator must be nothing or :diagonal"))
    println("---Iterating---")
    λ = 500u"nm"
    LTE_pops = VoronoiRT.LTE_populations(sites)
    α_s = VoronoiRT.α_scattering.(λ, sites.electron_density * 1.0, LTE_pops[:, 1])
    α_a = VoronoiRT.α_absorption.(λ, sites.temperature, sites.electron_density * 1.0,
                                  LTE_pops[:, 1] .+ LTE_pops[:, 2], LTE_pops[:, 3])
    α_cont = α_s + α_a
    ε_λ = Vector{Float64}(α_a ./ α_cont)
    B_0 = Vector{Float64}(ustrip.(I_unit, VoronoiRT.blackbody_λ.(λ, sites.temperature)))
    αc = Vector{Float64}(ustrip.(u"m^-1", α_cont))
    weights, = read_quadrature(quadrature)
    w = Vector{Float64}(weights)
    plan = plan_handle(sites, quadrature, 3)
    n = length(B_0)
    ses = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve αc ε_λ B_0 w begin
        cc = Ref(ContinuumCase(1, pointer(αc), pointer(ε_λ), pointer(B_0), 1e-4))
        check(ccall((:vrt_continuum_create, libvrt), Cint, (Ptr{Cvoid}, Ref{ContinuumCase}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                    plan, cc, w, ses))
    end
    if S0 !== nothing
        S_in = Vector{Float64}(ustrip.(I_unit, S0))
        check(ccall((:vrt_continuum_set_source, libvrt), Cint, (Ptr{Cvoid}, Ptr{Float64}), ses[], S_in))
    end
    operator === :diagonal && check(ccall((:vrt_continuum_set_operator, libvrt), Cint, (Ptr{Cvoid}, Cint), ses[], 1))
    ng !== nothing && check(ccall((:vrt_continuum_set_acceleration, libvrt), Cint, (Ptr{Cvoid}, Cint, Cint, Cint),
                                  ses[], 2, ng[1], ng[2]))
    J = Vector{Float64}(undef, n); S = Vector{Float64}(undef, n)
    continuum_loop(ϵ, maxiter,
                   d -> ccall((:vrt_continuum_iterate, libvrt), Cint, (Ptr{Cvoid}, Ref{Float64}), ses[], d),
                   () -> ccall((:vrt_continuum_get, libvrt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ses[], J, S),
                   (a, c) -> ccall((:vrt_continuum_last_acceleration, libvrt), Cint,
                                   (Ptr{Cvoid}, Ref{Cint}, Ptr{Float64}, Ptr{Float64}), ses[], a, C_NULL, c), ng)
    ccall((:vrt_continuum_destroy, libvrt), Cvoid, (Ptr{Cvoid},), ses[])
    return J * I_unit, S * I_unit, α_cont
end

"""
    Λ_continuum_regular(ϵ, maxiter, atmos, quadrature; ng=nothing, S0=nothing, operator=nothing) -> (J_new, S_new, α_cont)

The reference's continuum Λ_regular (src/lambda_continuum.jl:58-107) on the device (vrt_regular_continuum_*); `atmos` is
the atmosphere the reference iterates on, every point of it a point of the loop.  (nz, nx, ny) arrays are
vrt_continuum_case's (1, n) with n = nz nx ny.  Keywords as `Λ_continuum`, `operator = :diagonal`
(vrt_regular_continuum_select_operator) included.  Unrun.
"""
function Λ_continuum_regular(ϵ::AbstractFloat, maxiter::Integer, atmos, quadrature::String;
                             ng::Union{Nothing,Tuple{Int,Int}}=nothing, S0=nothing, operator::Union{Nothing,Symbol}=nothing)
    operator === nothing || operator === :diagonal || throw(ArgumentError("operator must be nothing or :diagonal"))
    λ = 500u"nm"
    LTE_pops = VoronoiRT.LTE_populations(atmos)
    α_s = VoronoiRT.α_scattering.(λ, atmos.electron_density * 1.0, LTE_pops[:, :, :, 1])
    α_a = VoronoiRT.α_absorption.(λ, atmos.temperature, atmos.electron_density * 1.0,
                                  LTE_pops[:, :, :, 1] .+ LTE_pops[:, :, :, 2], LTE_pops[:, :, :, 3])
    α_cont = α_s + α_a
    ε_λ = Array{Float64,3}(α_a ./ α_cont)
    B_0 = Array{Float64,3}(ustrip.(I_unit, VoronoiRT.blackbody_λ.(λ, atmos.temperature)))
    αc = Array{Float64,3}(ustrip.(u"m^-1", α_cont))
    nz, nx, ny = size(B_0)
    weights, θ_array, ϕ_array, n_angles = read_quadrature(quadrature)
    k = Matrix{Float64}(undef, 3, n_angles)
    for i in 1:n_angles
        k[:, i] = direction(θ_array[i], ϕ_array[i])              # :14
    end
    dirs = Cint[θ > 90 ? 1 : (θ < 90 ? -1 : 0) for θ in θ_array]  # θ = 90 adds nothing (:15-21)
    w = Vector{Float64}(weights)
    z = Vector{Float64}(ustrip.(u"m", atmos.z)); x = Vector{Float64}(ustrip.(u"m", atmos.x))
    y = Vector{Float64}(ustrip.(u"m", atmos.y))
    reg = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve z x y check(ccall((:vrt_regular_create, libvrt), Cint,
                                   (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
                                   nz, nx, ny, z, x, y, 0, reg))
    ses = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve αc ε_λ B_0 k dirs w begin
        cc = Ref(ContinuumCase(1, pointer(αc), pointer(ε_λ), pointer(B_0), 1e-4))
        check(ccall((:vrt_regular_continuum_create, libvrt), Cint,
                    (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Ref{ContinuumCase}, Cint, Ref{Ptr{Cvoid}}),
                    reg[], n_angles, k, dirs, w, cc, 3, ses))
    end
    if S0 !== nothing
        S_in = Array{Float64,3}(ustrip.(I_unit, S0))
        check(ccall((:vrt_regular_continuum_set_source, libvrt), Cint, (Ptr{Cvoid}, Ptr{Float64}), ses[], S_in))
    end
    operator === :diagonal && check(ccall((:vrt_regular_continuum_select_operator, libvrt), Cint, (Ptr{Cvoid}, Cint), ses[], 1))
    ng !== nothing && check(ccall((:vrt_regular_continuum_set_acceleration, libvrt), Cint, (Ptr{Cvoid}, Cint, Cint, Cint),
                                  ses[], 2, ng[1], ng[2]))
    J = Array{Float64,3}(undef, nz, nx, ny); S = Array{Float64,3}(undef, nz, nx, ny)
    continuum_loop(ϵ, maxiter,
                   d -> ccall((:vrt_regular_continuum_iterate, libvrt), Cint, (Ptr{Cvoid}, Ref{Float64}), ses[], d),
                   () -> ccall((:vrt_regular_continuum_get, libvrt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ses[], J, S),
                   (a, c) -> ccall((:vrt_regular_continuum_last_acceleration, libvrt), Cint,
                                   (Ptr{Cvoid}, Ref{Cint}, Ptr{Float64}, Ptr{Float64}), ses[], a, C_NULL, c), ng)
    ccall((:vrt_regular_continuum_destroy, libvrt), Cvoid, (Ptr{Cvoid},), ses[])
    ccall((:vrt_regular_destroy, libvrt), Cvoid, (Ptr{Cvoid},), reg[])
    return J * I_unit, S * I_unit, α_cont
end

"""
    lambda_diagonal_regular(z, x, y, α, quadrature) -> Λ*

The diagonal approximate operator of accelerated Λ-iteration on a raster (vrt_regular_lambda_diagonal): per point the
coefficient of its own S in its intensity after one sweep of the raster solve, summed over the quadrature; 0 on the ghost
border.  z, x, y: the ghosted axes in metres; α (nz, nx, ny) in m^-1, finite and > 0.  Unrun.
"""
function lambda_diagonal_regular(z::Vector{Float64}, x::Vector{Float64}, y::Vector{Float64}, α::Array{Float64,3},
                                 quadrature::String)
    nz, nx, ny = size(α)
    (nz, nx, ny) == (length(z), length(x), length(y)) || throw(ArgumentError("α must be (nz, nx, ny) of the axes"))
    weights, θ_array, ϕ_array, n_angles = read_quadrature(quadrature)
    k = Matrix{Float64}(undef, 3, n_angles)
    for i in 1:n_angles
        k[:, i] = direction(θ_array[i], ϕ_array[i])
    end
    dirs = Cint[θ > 90 ? 1 : (θ < 90 ? -1 : 0) for θ in θ_array]
    w = Vector{Float64}(weights)
    reg = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:vrt_regular_create, libvrt), Cint,
                (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
                nz, nx, ny, z, x, y, 0, reg))
    diag = zeros(Float64, nz, nx, ny)
    rc = ccall((:vrt_regular_lambda_diagonal, libvrt), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
               reg[], n_angles, k, dirs, w, 1, 1, α, diag)
    ccall((:vrt_regular_destroy, libvrt), Cvoid, (Ptr{Cvoid},), reg[])
    check(rc)
    return diag
end

"""
    line_lambda_diagonal_regular(z, x, y, α, quadrature) -> Λ*

Λ* of the line Λ-iteration on a raster (vrt_regular_line_lambda_diagonal): `lambda_diagonal_regular` with an α of its own
per angle.  z, x, y: the ghosted axes in metres; α (nλ, nz, nx, ny, n_angles) in m^-1 for every angle of the quadrature in
order, finite and > 0 (the block of a θ = 90 angle is not read).  Returns (nλ, nz, nx, ny).  Unrun.
"""
function line_lambda_diagonal_regular(z::Vector{Float64}, x::Vector{Float64}, y::Vector{Float64}, α::Array{Float64,5},
                                      quadrature::String)
    nλ, nz, nx, ny, na = size(α)
    (nz, nx, ny) == (length(z), length(x), length(y)) || throw(ArgumentError("α must be (nλ, nz, nx, ny, n_angles) of the axes"))
    weights, θ_array, ϕ_array, n_angles = read_quadrature(quadrature)
    na == n_angles || throw(ArgumentError("α needs one block per angle of the quadrature"))
    k = Matrix{Float64}(undef, 3, n_angles)
    for i in 1:n_angles
        k[:, i] = direction(θ_array[i], ϕ_array[i])
    end
    dirs = Cint[θ > 90 ? 1 : (θ < 90 ? -1 : 0) for θ in θ_array]
    w = Vector{Float64}(weights)
    reg = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:vrt_regular_create, libvrt), Cint,
                (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
                nz, nx, ny, z, x, y, 0, reg))
    diag = zeros(Float64, nλ, nz, nx, ny)
    rc = ccall((:vrt_regular_line_lambda_diagonal, libvrt), Cint,
               (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
               reg[], n_angles, k, dirs, w, nλ, nλ, α, diag)
    ccall((:vrt_regular_destroy, libvrt), Cvoid, (Ptr{Cvoid},), reg[])
    check(rc)
    return diag
end

# ---- single solves: src/irregular_ray_tracing.jl:15-20, :96-101 ----------------------------------
# literal-symbol wrappers (the name/library tuple of a ccall must not reference a local variable)
c_delaunay_up(g, k, S, I0, α, n_sweeps, I) =
    ccall((:vrt_delaunay_up, libvrt), Cint,
          (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Cint, Ptr{Float64}),
          g, k, S, I0, length(I0), α, n_sweeps, I)
c_delaunay_down(g, k, S, I0, α, n_sweeps, I) =
    ccall((:vrt_delaunay_down, libvrt), Cint,
          (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Cint, Ptr{Float64}),
          g, k, S, I0, length(I0), α, n_sweeps, I)

function solve(up::Bool, k, S, I_0, α, sites::VoronoiSites, n_sweeps::Int)
    g = grid_handle(sites)
    kv = Vector{Float64}(k)
    Sv = Vector{Float64}(ustrip.(I_unit, S)); I0 = Vector{Float64}(ustrip.(I_unit, I_0))
    αv = Vector{Float64}(ustrip.(u"m^-1", α))
    I = similar(Sv)
    GC.@preserve kv Sv I0 αv I begin
        check(up ? c_delaunay_up(g, kv, Sv, I0, αv, n_sweeps, I) : c_delaunay_down(g, kv, Sv, I0, αv, n_sweeps, I))
    end
    return I * I_unit
end

# ---- voro (src/functions.jl:13-23): the voro++ fork/exec, in-process --------------------------------
# Reads the sites file the driver has just written (write_arrays, src/io.jl:16-20: "id\tx\ty\tz"),
# tessellates with vrt_tessellate and writes the "%i %n" neighbours file read_cell parses, so the
# driver's own `voro(...); read_cell(...)` sequence (compare_line.jl:100-103) runs unchanged.
# device = nothing: the host code (vrt_tessellate); device = ordinal: the same matrix from the device tessellation
# (vrt_tessellate_gpu; a site it cannot hold is recomputed by the host code) -- the keyword is unrun: Julia is not
# installed where the library is built.
function voro_inprocess(sites_file::String, neighbours_file::String,
                        x_min::Float64, x_max::Float64, y_min::Float64, y_max::Float64,
                        z_min::Float64, z_max::Float64; device::Union{Nothing,Integer}=nothing)
    rows = [split(l) for l in eachline(sites_file) if !isempty(strip(l))]
    n = length(rows)
    pos = Matrix{Float64}(undef, 3, n)                      # (3, n) rows z, x, y
    for r in rows
        i = parse(Int, r[1])
        pos[2, i] = parse(Float64, r[2]); pos[3, i] = parse(Float64, r[3]); pos[1, i] = parse(Float64, r[4])
    end
    bounds = Float64[z_min, z_max, x_min, x_max, y_min, y_max]
    D1 = 71                                                  # max_guess + 1, voronoi_utils.jl:42
    nbr = zeros(Int64, n, D1)
    mx = Ref{Int64}(0)
    GC.@preserve pos bounds nbr begin
        if device === nothing
            check(ccall((:vrt_tessellate, libvrt), Cint,
                        (Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ref{Int64}),
                        n, pos, bounds, D1, nbr, mx))
        else
            check(ccall((:vrt_tessellate_gpu, libvrt), Cint,
                        (Cint, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ref{Int64}, Ptr{Int64}),
                        device, n, pos, bounds, D1, nbr, mx, C_NULL))
        end
        check(ccall((:vrt_write_neighbours_file, libvrt), Cint, (Cstring, Int64, Ptr{Int64}, Int64),
                    neighbours_file, n, nbr, D1))
    end
    return nothing
end

# ---- regular-grid short characteristics (src/characteristics.jl:19-95, :110-180) ----------------
# S_0, α are (nz, nx, ny) Julia arrays, I_0 is (nx, ny); `atmos` contributes its three axes only
function regular_solve(up::Bool, k, S_0::AbstractArray{<:Any,3}, I_0::AbstractMatrix, α::AbstractArray{<:Any,3},
                       atmos; n_sweeps::Int=3, device::Integer=0)
    z = Vector{Float64}(ustrip.(u"m", atmos.z)); x = Vector{Float64}(ustrip.(u"m", atmos.x))
    y = Vector{Float64}(ustrip.(u"m", atmos.y))
    S = Array{Float64,3}(ustrip.(I_unit, S_0)); A = Array{Float64,3}(ustrip.(u"m^-1", α))
    I0 = Matrix{Float64}(ustrip.(I_unit, I_0))
    I = similar(S)
    kk = Vector{Float64}(k); upv = Cint[up ? 1 : 0]
    GC.@preserve z x y S A I0 I kk upv begin
        check(ccall((:vrt_short_characteristics, libvrt), Cint,
                    (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Cint},
                     Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Cint, Cint, Ptr{Float64}),
                    length(z), length(x), length(y), z, x, y, 1, kk, upv, S, 0, A, 0, I0, n_sweeps, device, I))
    end
    return I * I_unit
end

# ---- rejection_sampling (src/functions.jl:79-120) on the device ---------------------------------------------------------
# `quantity` is the (nz, nx, ny) array the sample_from_* functions form (src/sample_grids.jl); the sites are drawn by
# vrt_sample_sites from a counter-based stream keyed by `seed`, so (atmos, quantity, n_sites, seed) fixes the grid.  The
# reference's Julia RNG stream is not reproduced.  Returns (3, n_sites) positions [z; x; y] in metres, as the reference.
function rejection_sampling(n_sites::Integer, atmos, quantity::AbstractArray; seed::Integer=0, device::Integer=0,
                            max_proposals::Integer=0)
    z = Vector{Float64}(ustrip.(u"m", atmos.z)); x = Vector{Float64}(ustrip.(u"m", atmos.x))
    y = Vector{Float64}(ustrip.(u"m", atmos.y))
    q = Array{Float64,3}(ustrip.(quantity))
    size(q) == (length(z), length(x), length(y)) || error("quantity must be (nz, nx, ny)")
    p_vec = Matrix{Float64}(undef, 3, n_sites)
    used = Ref{Int64}(0)
    GC.@preserve z x y q p_vec begin
        check(ccall((:vrt_sample_sites, libvrt), Cint,
                    (Cint, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, UInt64,
                     Int64, Int64, Ptr{Float64}, Ref{Int64}),
                    device, length(z), length(x), length(y), z, x, y, q, n_sites, UInt64(seed), 0, max_proposals,
                    p_vec, used))
    end
    return p_vec * u"m"
end

# ---- the observable (write_top_intensity / write_tau_unity, src/plot_utils.jl:101-140, :434-576) -------------------------
# S_λ, α_tot (nλ, nz, nx + 2, ny + 2) as plotter makes them on the periodic atmos (ghost border included); `atmos` gives
# the axes WITH the border, as short_characteristics_up reads them.  Returns I_top (nλ, nx, ny) in S's unit per
# steradian, the top plane's interior of each wavelength's up solve with I_0 = the bottom plane of S (vrt_top_intensity).
function top_intensity(S_λ::AbstractArray{<:Any,4}, α_tot::AbstractArray{<:Any,4}, atmos, θ::Float64, ϕ::Float64;
                       n_sweeps::Int=3, device::Integer=0)
    k = [cos(θ*π/180), cos(ϕ*π/180)*sin(θ*π/180), sin(ϕ*π/180)*sin(θ*π/180)]
    z = Vector{Float64}(ustrip.(u"m", atmos.z)); x = Vector{Float64}(ustrip.(u"m", atmos.x))
    y = Vector{Float64}(ustrip.(u"m", atmos.y))
    I_unit = unit(S_λ[1])
    nl = size(S_λ, 1)
    S = permutedims(Array{Float64,4}(ustrip.(S_λ)), (2, 3, 4, 1))        # (nz, nx, ny, nλ): one Julia array per λ
    A = permutedims(Array{Float64,4}(ustrip.(u"m^-1", α_tot)), (2, 3, 4, 1))
    size(S) == (length(z), length(x), length(y), nl) || error("S_λ must be (nλ, nz, nx, ny) on atmos's axes")
    I = Array{Float64,3}(undef, length(x) - 2, length(y) - 2, nl)
    GC.@preserve z x y k S A I begin
        check(ccall((:vrt_top_intensity, libvrt), Cint,
                    (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
                     Ptr{Float64}, Cint, Cint, Ptr{Float64}),
                    length(z), length(x), length(y), z, x, y, k, nl, S, A, n_sweeps, device, I))
    end
    return permutedims(I, (3, 1, 2)) * I_unit
end

# Heights of τ = 1 (nλ, nx, ny) in metres for α_tot (nλ, nz, nx + 2, ny + 2) with the periodic ghost border; `atmos`
# gives the INTERIOR axes (periodic = false, as write_tau_unity reads them).  θ = 180° is write_tau_unity(DATA)
# exactly; an inclined direction follows the solver's characteristic (INTEGRATION.md: the reference's inclined
# method is not reproduced).
function tau_unity(α_tot::AbstractArray{<:Any,4}, atmos, θ::Float64, ϕ::Float64; device::Integer=0)
    k = [cos(θ*π/180), cos(ϕ*π/180)*sin(θ*π/180), sin(ϕ*π/180)*sin(θ*π/180)]
    θ == 180.0 && (k = [-1.0, 0.0, 0.0])
    z = Vector{Float64}(ustrip.(u"m", atmos.z)); x = Vector{Float64}(ustrip.(u"m", atmos.x))
    y = Vector{Float64}(ustrip.(u"m", atmos.y))
    nl = size(α_tot, 1)
    A = permutedims(Array{Float64,4}(ustrip.(u"m^-1", α_tot)), (2, 3, 4, 1))
    size(A) == (length(z), length(x) + 2, length(y) + 2, nl) || error("α_tot must be (nλ, nz, nx + 2, ny + 2)")
    H = Array{Float64,3}(undef, length(x), length(y), nl)
    GC.@preserve z x y k A H begin
        check(ccall((:vrt_tau_unity, libvrt), Cint,
                    (Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64},
                     Cint, Ptr{Float64}),
                    length(z), length(x), length(y), z, x, y, k, nl, A, device, H))
    end
    return permutedims(H, (3, 1, 2)) * u"m"
end

end # module

# ---- drop-in redefinitions (same signatures as the reference's methods) --------------------------
# the batched path: what compare_line.jl / Λ_voronoi (lambda_iteration.jl:259) and the continuum
# driver (lambda_continuum.jl) call
VoronoiRT.J_λ_voronoi(S_λ::Matrix{<:VoronoiRT.UnitsIntensity_λ}, α_cont::Vector{<:VoronoiRT.PerLength},
                      populations::Matrix{<:VoronoiRT.NumberDensity}, sites::VoronoiRT.VoronoiSites,
                      line::VoronoiRT.HydrogenicLine, quadrature::String) =
    VoronoiRTHip.J_line(S_λ, α_cont, populations, sites, line, quadrature)
VoronoiRT.J_λ_voronoi(S_λ::AbstractArray, α_cont::AbstractArray, sites::VoronoiRT.VoronoiSites,
                      quadrature::String) =
    VoronoiRTHip.J_continuum(S_λ, α_cont, sites, quadrature)
# the Λ-iteration driver of compare_line.jl:125 (src/lambda_iteration.jl:205-300): loop body on the device
VoronoiRT.Λ_voronoi(ϵ::AbstractFloat, maxiter::Integer, sites::VoronoiRT.VoronoiSites, line::VoronoiRT.HydrogenicLine,
                    quadrature::String, DATA::String) =
    VoronoiRTHip.Λ(ϵ, maxiter, sites, line, quadrature, DATA)
# the continuum drivers of compare_continuum.jl (src/lambda_continuum.jl:109-160, :58-107): the 4-argument methods
VoronoiRT.Λ_voronoi(ϵ::AbstractFloat, maxiter::Integer, sites::VoronoiRT.VoronoiSites, quadrature::String) =
    VoronoiRTHip.Λ_continuum(ϵ, maxiter, sites, quadrature)
VoronoiRT.Λ_regular(ϵ::AbstractFloat, maxiter::Integer, atmos::VoronoiRT.Atmosphere, quadrature::String) =
    VoronoiRTHip.Λ_continuum_regular(ϵ, maxiter, atmos, quadrature)
# preprocessing (compare_line.jl:100, compare_continuum.jl, compare_searchlight.jl): the executable's
# path is ignored, the tessellation runs inside the library
VoronoiRT.voro(voro_executable::String, sites_file::String, neighbours_file::String,
               x_min::Float64, x_max::Float64, y_min::Float64, y_max::Float64,
               z_min::Float64, z_max::Float64; device::Union{Nothing,Integer}=nothing) =
    VoronoiRTHip.voro_inprocess(sites_file, neighbours_file, x_min, x_max, y_min, y_max, z_min, z_max; device=device)
# (device = an ordinal: the tessellation on that device, vrt_tessellate_gpu; the keyword is unrun)
# single solves (compare_searchlight.jl:113,129,434)
VoronoiRT.Delaunay_upII(k::Vector{Float64}, S, I_0, α, sites::VoronoiRT.VoronoiSites, n_sweeps::Int) =
    VoronoiRTHip.solve(true, k, S, I_0, α, sites, n_sweeps)
VoronoiRT.Delaunay_downII(k::Vector{Float64}, S, I_0, α, sites::VoronoiRT.VoronoiSites, n_sweeps::Int) =
    VoronoiRTHip.solve(false, k, S, I_0, α, sites, n_sweeps)
VoronoiRT.short_characteristics_up(k::Vector{Float64}, S_0, I_0, α, atmos::VoronoiRT.Atmosphere;
                                   pt::Bool=false, n_sweeps::Int=3) =
    VoronoiRTHip.regular_solve(true, k, S_0, I_0, α, atmos; n_sweeps=n_sweeps)
VoronoiRT.short_characteristics_down(k::Vector{Float64}, S_0, I_0, α, atmos::VoronoiRT.Atmosphere;
                                     pt::Bool=false, n_sweeps::Int=3) =
    VoronoiRTHip.regular_solve(false, k, S_0, I_0, α, atmos; n_sweeps=n_sweeps)

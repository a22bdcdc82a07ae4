# CEGHip.jl -- reference-side binding of libceg_hip.so (include/ceg_hip.h).
#
# Drop-in for the two loop nests of CrystalEnergyGrids.jl that fill an energy grid:
#
#     create_grid_vdw      src/grids.jl:137-157   (loop nest :144-150)
#     create_grid_coulomb  src/grids.jl:159-185   (loop nest :171-177)
#
# Everything else -- ProbeSystem, GridCoordinatesSetup, initialize_ewald, the unit constants,
# `_create_grid_common` and the file layout -- is the reference's own code, called unchanged, so
# `retrieve_or_create_grid` (src/raspa.jl:420-439), `setup_RASPA`, `setup_montecarlo`,
# `CrystalEnergySetup` and `energy_point` keep working without modification.
#
# NOT EXECUTED IN THIS REPOSITORY'S CI: the build image has no Julia toolchain.  The Python
# package `ceg_hip` is the tested twin of this file (same argument marshalling, same C calls), and
# tests/test_boundary_static.py parses every `ccall` below and checks symbol, arity and C types
# against include/ceg_hip.h and ceg_hip/_abi.py.
#
# Usage (after `using CrystalEnergyGrids`):
#     include("CEGHip.jl"); CEGHip.install!()        # overrides the two methods
#     ENV["CEG_HIP_LIB"] = "/path/to/libceg_hip.so"   # optional, default next to this file
#     ENV["CEG_HIP_NGPUS"] = "8"                      # optional, default 1
module CEGHip

import CrystalEnergyGrids as CEG
using CrystalEnergyGrids: ProbeSystem, ForceField, InteractionRule, InteractionRuleSum, FF,
                          EwaldFramework, GridCoordinatesSetup, GRID_TO_KELVIN,
                          COULOMBIC_CONVERSION_FACTOR, TÅ
using Unitful, UnitfulAtomic
using AtomsBase: AbstractSystem, position
using LinearAlgebra: norm
using StaticArrays

const LIB = Ref(get(ENV, "CEG_HIP_LIB", joinpath(@__DIR__, "..", "csrc", "libceg_hip.so")))
ngpus() = parse(Int, get(ENV, "CEG_HIP_NGPUS", "1"))

# struct ceg_rule { int32 kind; int32 _pad; double p[3]; double shift; }   (include/ceg_hip.h)
struct CegRule
    kind::Int32
    _pad::Int32
    p1::Float64
    p2::Float64
    p3::Float64
    shift::Float64
end

_rules(r::InteractionRule) = (r,)
_rules(r::InteractionRuleSum) = r.rules

"Flatten `ff.interactions[:, probe]` (what `derivatives_nocutoff`, src/forcefields.jl:302-304, dispatches on)."
function rule_table(ff::ForceField, probe::Int)
    n = size(ff.interactions, 1)
    flat = CegRule[]
    offsets = Int32[0]
    for k in 1:n
        for r in _rules(ff.interactions[k, probe])
            p = r.params
            push!(flat, CegRule(Int32(Int(r.kind)), 0, get(p, 1, 0.0), get(p, 2, 0.0), get(p, 3, 0.0), r.shift))
        end
        push!(offsets, Int32(length(flat)))
    end
    flat, offsets
end

"Raise what `derivativesGrid` (src/interactions.jl:442-443,462-467) would raise for the kinds present."
function check_rules(ff::ForceField, probe::Int, kinds)
    for k in unique(kinds), r in _rules(ff.interactions[k, probe])
        r.kind === FF.UndefinedInteraction && throw(CEG.UndefinedInteractionError())
        r.kind === FF.Coulomb && error("Coulomb interactions should not be taken into account in VdW grids.")
        r.kind === FF.Monomial && error("VdW grid not implemented for Monomial")
        r.kind === FF.Exponential && error("VdW grid not implemented for Exponential")
    end
end

function _check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:ceg_last_error, LIB[]), Cstring, ()))
    error("libceg_hip error $rc: $msg")
end

function _geometry(cset::GridCoordinatesSetup)
    dims = Int32[cset.dims...]
    size = Float64[NoUnits(x/u"Å") for x in cset.size]
    shift = Float64[NoUnits(x/u"Å") for x in cset.shift]
    Δ = Float64[NoUnits(x/u"Å") for x in cset.Δ]
    dims, size, shift, Δ
end

function _flatpos(probe::ProbeSystem)
    pos = Vector{Float64}(undef, 3*length(probe.positions))
    for (i, p) in enumerate(probe.positions)
        pos[3i-2] = p[1]; pos[3i-1] = p[2]; pos[3i] = p[3]
    end
    pos
end

"GPU replacement of the loop nest src/grids.jl:144-150; fills and returns `grid`."
function fill_grid_vdw!(grid::Array{Cfloat,4}, probe::ProbeSystem, cset::GridCoordinatesSetup, λ, thr)
    ff = probe.forcefield
    check_rules(ff, probe.probe, probe.atomkinds)
    rules, offsets = rule_table(ff, probe.probe)
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(probe.mat)   # src/utils.jl:146-155
    cutoff2 = NoUnits(ff.cutoff^2/u"Å^2")                                          # src/probes.jl:75
    dims, size, shift, Δ = _geometry(cset)
    pos = _flatpos(probe)
    kinds = Int64.(probe.atomkinds)
    mat = Vector{Float64}(vec(probe.mat)); invmat = Vector{Float64}(vec(probe.invmat))   # column-major
    GC.@preserve grid pos kinds mat invmat rules offsets dims size shift Δ begin
        _check(ccall((:ceg_grid_vdw, LIB[]), Cint,
            (Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Float64,
             Ptr{CegRule}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Float64, Float64, Ptr{Cfloat}, Int32),
            pos, kinds, length(kinds), mat, invmat, ortho, safemin^2, cutoff2,
            rules, offsets, length(offsets)-1, dims, size, shift, Δ, λ, thr, grid, ngpus()))
    end
    grid
end

"GPU replacement of the loop nest src/grids.jl:171-177."
function fill_grid_coulomb!(grid::Array{Cfloat,4}, probe::ProbeSystem, ewald::EwaldFramework, cset::GridCoordinatesSetup, λ, thr)
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(probe.mat)
    cutoff2 = NoUnits(probe.forcefield.cutoff^2/u"Å^2")                            # src/probes.jl:98
    dims, size, shift, Δ = _geometry(cset)
    pos = _flatpos(probe)
    mat = Vector{Float64}(vec(probe.mat)); invmat = Vector{Float64}(vec(probe.invmat))
    α = NoUnits(ewald.α*u"Å")
    GC.@preserve grid pos mat invmat dims size shift Δ begin
        _check(ccall((:ceg_grid_coulomb, LIB[]), Cint,
            (Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Float64, Float64,
             Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Cfloat}, Int32),
            pos, probe.charges, length(probe.charges), mat, invmat, ortho, safemin^2, cutoff2, α,
            dims, size, shift, Δ, λ, thr, grid, ngpus()))
    end
    grid
end

# Result arrays.  By default (round 4) the grid array is page-locked memory of the library (ceg_host_grid_alloc) wrapped as an Array: the
# build then copies every chunk D2H straight to its place (256^3 VdW grid: 10.5 instead of 13.4 ms, the driver-run figures are in
# BENCH_r04.json `oneshot`).  The Array goes back to the library's cache when it is finalized, or at once through `release!(grid)` when the
# caller is done with it (the reference's own caller, retrieve_or_create_grid, src/raspa.jl:420-439, drops the returned array and parses
# the file it has just written).  The page-locked memory in Julia's hands is BOUNDED by the library (CEG_HIP_PINNED_LIMIT_MB, default
# 4096 MB): beyond it ceg_host_grid_alloc refuses and an ordinary Array is used, so a collector that has not run yet cannot pin host
# memory without limit.  ENV["CEG_HIP_PINNED_RESULT"] = "0" turns the page-locked arrays off.
pinned_results() = get(ENV, "CEG_HIP_PINNED_RESULT", "1") != "0"

_free_pinned(g) = (ccall((:ceg_host_grid_free, LIB[]), Cint, (Ptr{Cfloat},), pointer(g)); nothing)

function result_array(cset::GridCoordinatesSetup)
    dims = (cset.dims[3]+1, cset.dims[2]+1, cset.dims[1]+1, 8)
    pinned_results() || return Array{Cfloat,4}(undef, dims...)
    d = Int32[cset.dims...]
    ptr = GC.@preserve d ccall((:ceg_host_grid_alloc, LIB[]), Ptr{Cfloat}, (Ptr{Int32},), d)
    ptr == C_NULL && return Array{Cfloat,4}(undef, dims...)      # over the limit (or no page-locked memory): the ordinary route
    grid = unsafe_wrap(Array, ptr, dims; own=false)
    finalizer(_free_pinned, grid)
    grid
end

"""
    release!(grid)

Hand the page-locked memory behind a grid returned by `create_grid_vdw` / `create_grid_coulomb` back to the library NOW instead of at
the next garbage collection.  `grid` must not be used afterwards.  A no-op for ordinary arrays.
"""
release!(grid::Array{Cfloat,4}) = (finalize(grid); nothing)     # runs (and retires) the finalizer registered by result_array

# The two methods below are the reference's (src/grids.jl:137-185) with the `@threads` loop nest
# replaced by one call; every other line is unchanged.
function create_grid_vdw(file, framework::AbstractSystem{3}, forcefield::ForceField, spacing::TÅ, atom::Symbol)
    cset, num_unitcell = CEG._setup_grid_common(framework, spacing, forcefield.cutoff)
    grid = result_array(cset)            # reference: Array{Cfloat,4}(undef, cset.dims[3]+1, cset.dims[2]+1, cset.dims[1]+1, 8)
    probe_vdw = ProbeSystem(framework, forcefield, atom)
    λ⁻¹ = GRID_TO_KELVIN
    λ = inv(λ⁻¹)
    fill_grid_vdw!(grid, probe_vdw, cset, λ, λ⁻¹*1e7)
    open(file, "w") do f
        CEG._create_grid_common(f, cset, num_unitcell)
        write(f, grid)
        write(f, NoUnits.(cset.cell.mat./u"Å"))
    end
    grid
end

function create_grid_coulomb(file, framework::AbstractSystem{3}, forcefield::ForceField, spacing::TÅ, _ewald=nothing)
    cset, num_unitcell = CEG._setup_grid_common(framework, spacing, 12.0u"Å")
    ewald = _ewald isa EwaldFramework ? _ewald : CEG.initialize_ewald(framework, num_unitcell)
    grid = result_array(cset)
    probe_coulomb = ProbeSystem(framework, forcefield)
    λ = ustrip(u"K*Å/e_au^2", COULOMBIC_CONVERSION_FACTOR)/GRID_TO_KELVIN
    λ⁻¹e7 = inv(λ)*1e7
    fill_grid_coulomb!(grid, probe_coulomb, ewald, cset, λ, λ⁻¹e7)
    open(file, "w") do f
        CEG._create_grid_common(f, cset, num_unitcell)
        write(f, ewald.precision)
        write(f, grid)
        write(f, NoUnits.(cset.cell.mat./u"Å"))
    end
    grid
end

# ------------------------------------------------------------------ all the grids of a setup in one pass
# setup_RASPA (src/raspa.jl:497-520) calls retrieve_or_create_grid once for the Coulomb grid and once per distinct atom of the
# molecule; each call that has to CREATE its grid runs a full pass over the framework.  ceg_grids_multi (include/ceg_hip.h)
# builds the VdW grids of up to 4 probes OF ANY RULE CLASS (round 4: Na + the C and O of CO2) and the Coulomb grid from one
# lattice-image list: the Lennard-Jones-only probes share accumulating loops, a Buckingham cation is launched alone or fused with the
# Coulomb grid.  (These multi-probe paths -- create_grids_multi, prebuild_grids!, result_array, interp_handle_from_file -- have never been
# executed: no Julia in the build image; tests/test_boundary_static.py checks ccall names and arities only.)

"True when `atom` meets every kind present in `probe` with at most one Lennard-Jones rule (such probes share accumulating loops; informational)."
function lj_only(ff::ForceField, probe::Int, kinds)
    for k in unique(kinds)
        real = [r for r in _rules(ff.interactions[k, probe]) if r.kind !== FF.NoInteraction && r.kind !== FF.CoulombEwaldDirect]
        (length(real) > 1 || (length(real) == 1 && real[1].kind !== FF.LennardJones)) && return false
    end
    true
end

"GPU replacement of K + 1 loop nests (src/grids.jl:144-150 per probe, :171-177): fills `vgrids[k]` for `probes[k]` and, if given, `cgrid`."
function fill_grids_multi!(vgrids::Vector{Array{Cfloat,4}}, cgrid::Union{Nothing,Array{Cfloat,4}}, probes::Vector{<:ProbeSystem},
                           probe_coulomb::Union{Nothing,ProbeSystem}, ewald::Union{Nothing,EwaldFramework}, cset::GridCoordinatesSetup)
    ref = probes[1]
    ff = ref.forcefield
    tables = map(probes) do p
        check_rules(ff, p.probe, p.atomkinds)
        rule_table(ff, p.probe)
    end
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(ref.mat)
    cutoff2 = NoUnits(ff.cutoff^2/u"Å^2")
    dims, size, shift, Δ = _geometry(cset)
    pos = _flatpos(ref)
    kinds = Int64.(ref.atomkinds)
    mat = Vector{Float64}(vec(ref.mat)); invmat = Vector{Float64}(vec(ref.invmat))
    λv = inv(GRID_TO_KELVIN); thrv = GRID_TO_KELVIN*1e7                                    # src/grids.jl:141-143,148
    λc = ustrip(u"K*Å/e_au^2", COULOMBIC_CONVERSION_FACTOR)/GRID_TO_KELVIN; thrc = inv(λc)*1e7   # :169-170
    α = ewald isa Nothing ? 0.0 : NoUnits(ewald.α*u"Å")
    charges = probe_coulomb isa Nothing ? Float64[] : probe_coulomb.charges
    rules = [t[1] for t in tables]; offsets = [t[2] for t in tables]
    GC.@preserve vgrids cgrid pos kinds charges mat invmat rules offsets dims size shift Δ begin
        rules_pp = Ptr{Cvoid}[pointer(r) for r in rules]
        offs_pp = Ptr{Cvoid}[pointer(o) for o in offsets]
        out_pp = Ptr{Cvoid}[pointer(g) for g in vgrids]
        GC.@preserve rules_pp offs_pp out_pp _check(ccall((:ceg_grids_multi, LIB[]), Cint,
            (Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Float64,
             Int32, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Int32, Float64,
             Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Float64, Float64, Float64, Float64, Ptr{Ptr{Cvoid}}, Ptr{Cfloat}, Int32),
            pos, kinds, (probe_coulomb isa Nothing ? C_NULL : pointer(charges)), length(kinds), mat, invmat, ortho, safemin^2, cutoff2,
            length(probes), rules_pp, offs_pp, length(offsets[1])-1, α,
            dims, size, shift, Δ,
            λv, thrv, λc, thrc, out_pp, (cgrid isa Nothing ? C_NULL : pointer(cgrid)), ngpus()))
    end
    vgrids, cgrid
end

"""
    create_grids_multi(vdw_files, coulomb_file, framework, forcefield, spacing, atoms, _ewald=nothing)

`create_grid_vdw` (src/grids.jl:137-157) for every atom of `atoms` (1 to 4, of any rule class) and, unless
`coulomb_file === nothing`, `create_grid_coulomb` (:159-185) in one GPU pass; the files are written by the reference's own lines --
each to a temporary name in its directory, renamed onto the target only when ALL are complete (the cache of src/raspa.jl:426 looks no
further than `isfile`: a truncated file at a cache path would be "retrieved" ever after); on failure the temporaries are removed.
"""
function create_grids_multi(vdw_files, coulomb_file, framework::AbstractSystem{3}, forcefield::ForceField, spacing::TÅ, atoms::Vector{Symbol}, _ewald=nothing)
    cset, num_unitcell = CEG._setup_grid_common(framework, spacing, forcefield.cutoff)
    newgrid() = result_array(cset)
    probes = [ProbeSystem(framework, forcefield, atom) for atom in atoms]
    vgrids = [newgrid() for _ in atoms]
    tmps = String[]
    targets = String[]
    try
        if coulomb_file === nothing
            fill_grids_multi!(vgrids, nothing, probes, nothing, nothing, cset)
        else
            _, num_unitcell_c = CEG._setup_grid_common(framework, spacing, 12.0u"Å")       # src/grids.jl:160: 12 Å whatever the force field says
            ewald = _ewald isa EwaldFramework ? _ewald : CEG.initialize_ewald(framework, num_unitcell_c)
            cgrid = newgrid()
            push!(vgrids, cgrid)           # (released with the others below; only the first length(atoms) entries are VdW grids)
            fill_grids_multi!(vgrids[1:length(atoms)], cgrid, probes, ProbeSystem(framework, forcefield), ewald, cset)
            tmp = string(coulomb_file, ".tmp.", getpid(), ".c")
            push!(tmps, tmp); push!(targets, String(coulomb_file))
            open(tmp, "w") do f
                CEG._create_grid_common(f, cset, num_unitcell_c)
                write(f, ewald.precision)
                write(f, cgrid)
                write(f, NoUnits.(cset.cell.mat./u"Å"))
            end
        end
        for (n, (file, grid)) in enumerate(zip(vdw_files, vgrids[1:length(atoms)]))
            tmp = string(file, ".tmp.", getpid(), ".", n)
            push!(tmps, tmp); push!(targets, String(file))
            open(tmp, "w") do f
                CEG._create_grid_common(f, cset, num_unitcell)
                write(f, grid)
                write(f, NoUnits.(cset.cell.mat./u"Å"))
            end
        end
        foreach(((t, f),) -> mv(t, f; force=true), zip(tmps, targets))
    catch
        foreach(t -> rm(t; force=true), tmps)
        rethrow()
    finally
        foreach(release!, vgrids)          # nothing is returned: the page-locked arrays go back to the library at once
    end
    nothing
end

"""
    prebuild_grids!(framework, pff, syst_mol; gridstep=0.15u"Å", supercell=nothing, new=false, cutoff=12.0u"Å")

Call with the arguments of `setup_RASPA` (src/raspa.jl:472-531) right before it: every grid that `setup_RASPA` would have to
create -- same paths (`grid_locations`, :403-419), same conditions (`retrieve_or_create_grid`, :420-439) -- is created here by
`create_grids_multi`, four probes at a time whatever their rule classes; `setup_RASPA` then only retrieves.
"""
function prebuild_grids!(framework, pff, syst_mol; gridstep=0.15u"Å", supercell=nothing, new=false, cutoff=12.0u"Å")
    (framework isa AbstractMatrix || isinf(cutoff) || cutoff != 12.0u"Å") && return nothing
    syst_framework = CEG.load_framework_RASPA(framework, pff)
    supercell = supercell isa Nothing ? CEG.find_supercell(syst_framework, cutoff) : supercell
    forcefield = CEG._ff(pff; cutoff)
    atoms = unique(syst_mol[:,:atomic_symbol])
    coulomb_grid_path, vdws = CEG.grid_locations(framework, pff, forcefield, atoms, gridstep, supercell)
    needcoulomb = any(!iszero(syst_mol[i,:atomic_charge])::Bool for i in 1:length(syst_mol))
    todo = [i for (i, atom) in enumerate(atoms) if CEG.needsvdwgrid(forcefield, atom) && (new || !isfile(vdws[i]))]
    want_c = needcoulomb && (new || !isfile(coulomb_grid_path))
    groups = [todo[lo:min(lo+3, length(todo))] for lo in 1:4:length(todo)]
    for (n, part) in enumerate(groups)
        with_c = want_c && n == 1
        length(part) + with_c < 2 && continue
        foreach(p -> mkpath(dirname(p)), vdws[part]); with_c && mkpath(dirname(coulomb_grid_path))
        create_grids_multi(vdws[part], with_c ? coulomb_grid_path : nothing, syst_framework, forcefield, gridstep, atoms[part],
                           with_c ? CEG.initialize_ewald(syst_framework, supercell) : nothing)
    end
    nothing
end

"Override the package's two grid builders with the GPU versions (method overwrite)."
function install!()
    @eval CEG begin
        create_grid_vdw(file, framework::AbstractSystem{3}, forcefield::ForceField, spacing::TÅ, atom::Symbol) =
            $(create_grid_vdw)(file, framework, forcefield, spacing, atom)
        create_grid_coulomb(file, framework::AbstractSystem{3}, forcefield::ForceField, spacing::TÅ, _ewald=nothing) =
            $(create_grid_coulomb)(file, framework, forcefield, spacing, _ewald)
    end
    nothing
end

# ------------------------------------------------------------------ consumers of the grids (SURVEY 8f rows f1-f3)
# Batched versions of interpolate_grid (src/grids.jl:212-273), compute_ewald(ctx) for one rigid molecule
# (src/ewald.jl:555-577) and single_contribution_vdw (src/energy.jl:397-427).  Handles are opaque pointers.

_pts(positions) = Float64[NoUnits(x/u"Å") for p in positions for x in p]

"`ceg_interp_create` from a parsed `EnergyGrid` (the array is already in K, src/grids.jl:78)."
function interp_handle(g::CEG.EnergyGrid; device=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    dims, size, shift, _ = _geometry(g.csetup)
    mat = Vector{Float64}(vec(NoUnits.(g.csetup.cell.mat ./ u"Å")))
    invmat = Vector{Float64}(vec(NoUnits.(g.csetup.cell.invmat .* u"Å")))
    GC.@preserve g dims size shift mat invmat _check(ccall((:ceg_interp_create, LIB[]), Cint,
        (Ref{Ptr{Cvoid}}, Int32, Ptr{Cfloat}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32),
        h, device, g.grid, 0, dims, size, shift, mat, invmat, g.ewald_precision == Inf))
    h[]
end

# struct ceg_grid_header (include/ceg_hip.h): what parse_grid (src/grids.jl:61-94) reads besides the payload
struct CegGridHeader
    spacing::Float64
    dims::NTuple{3,Int32}
    has_mat::Int32
    size::NTuple{3,Float64}
    shift::NTuple{3,Float64}
    delta::NTuple{3,Float64}
    unitcell::NTuple{3,Float64}
    num_unitcell::NTuple{3,Int32}
    _pad::Int32
    ewald_precision::Float64
    mat::NTuple{9,Float64}
end

"""
    interp_handle_from_file(path, iscoulomb; mat=nothing, device=0) -> (handle, header)

The GPU interpolation handle of a CACHED grid straight from its file ("Retrieved ... grid", src/raspa.jl:426-438): what
`parse_grid(path, iscoulomb, mat)` + `interp_handle` do, without the host array -- the payload is streamed to the device and multiplied
by `GRID_TO_KELVIN` there (src/grids.jl:78).  `mat`: the unit-cell matrix as for `parse_grid` (Å, unitless); `nothing` uses the one
stored at the end of the file.
"""
function interp_handle_from_file(path::AbstractString, iscoulomb::Bool; mat=nothing, device=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    hdr = Ref{CegGridHeader}()
    m = mat isa Nothing ? Float64[] : Vector{Float64}(vec(Matrix{Float64}(mat)))
    im = mat isa Nothing ? Float64[] : Vector{Float64}(vec(inv(Matrix{Float64}(mat))))
    GC.@preserve m im _check(ccall((:ceg_interp_create_from_file, LIB[]), Cint,
        (Ref{Ptr{Cvoid}}, Int32, Cstring, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
        h, device, path, iscoulomb, GRID_TO_KELVIN, (mat isa Nothing ? C_NULL : pointer(m)), (mat isa Nothing ? C_NULL : pointer(im)), hdr))
    h[], hdr[]
end

"interpolate_grid(g, p) for every p of `positions` -> Vector{Float64} (K)"
function interp_points(h::Ptr{Cvoid}, positions)
    pts = _pts(positions); out = Vector{Float64}(undef, length(positions))
    GC.@preserve pts out _check(ccall((:ceg_interp_points, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}),
                                      h, pts, length(out), out))
    out
end

"`ceg_recip_create` from an `EwaldFramework` (k-vectors in the order of kspace.kindices, src/ewald.jl:213-236)."
function recip_handle(ef::EwaldFramework; device=0)
    ijk = Int32[]
    for (jy, jz, jxrange, _) in ef.kspace.kindices, jx in jxrange
        push!(ijk, jx, jy, jz)
    end
    sf = ef.StoreRigidChargeFramework
    re, im_ = Vector{Float64}(real.(sf)), Vector{Float64}(imag.(sf))
    ks = Int32[ef.kspace.ks...]; invmat = Vector{Float64}(vec(NoUnits.(ef.invmat .* u"Å")))    # invmat carries Å^-1 (ewald.jl:44)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ijk re im_ ks invmat _check(ccall((:ceg_recip_create, LIB[]), Cint,
        (Ref{Ptr{Cvoid}}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int32}, Ptr{Float64}),
        h, device, ijk, ef.kfactors, re, im_, length(ef.kfactors), ks, invmat))
    h[]
end

"compute_ewald for `placements` (each a vector of atom positions) of a molecule with `charges`; `enc`, `static` = ctx.energy_net_charges, ctx.static_contribution[] in K"
function recip_energy(h::Ptr{Cvoid}, placements, charges::Vector{Float64}, enc::Float64, static::Float64)
    pts = Float64[NoUnits(x/u"Å") for mol in placements for p in mol for x in p]
    out = Vector{Float64}(undef, length(placements))
    GC.@preserve pts charges out _check(ccall((:ceg_recip_energy, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int64, Float64, Float64, Ptr{Float64}),
        h, pts, charges, length(charges), length(out), enc, static, out))
    out
end

"single_contribution_vdw of a molecule with ff indices `idx2` at every trial placement; `h` from ceg_pairs_create / ceg_pairs_set_atoms"
function pairs_energy(h::Ptr{Cvoid}, placements, idx2::Vector{Int}, exclude_molecule::Int)
    pts = Float64[NoUnits(x/u"Å") for mol in placements for p in mol for x in p]
    kinds = Int32.(idx2 .- 1); out = Vector{Float64}(undef, length(placements))
    GC.@preserve pts kinds out _check(ccall((:ceg_pairs_energy, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Int32, Int64, Int32, Ptr{Float64}),
        h, pts, kinds, length(kinds), length(out), exclude_molecule, out))
    out
end

# ------------------------------------------------------------------ Monte-Carlo inner loop (BASELINE config 5)
# Device-resident twin of the energy state of a MonteCarloSetup: movement_energy (src/montecarlo.jl:563-579) in one launch,
# update_mc! (src/montecarlo.jl:615-628) on the device.  The driver (src/simulation.jl:727-781) keeps proposing and accepting.

"`ceg_mc_create` + `ceg_mc_set_guests` from a `MonteCarloSetup` after `baseline_energy(mc)`; `vdw`/`coulomb` from `interp_handle`"
function mc_handle(mc::CEG.MonteCarloSetup, vdw::Vector{Ptr{Cvoid}}, coulomb::Ptr{Cvoid}; device=0)
    step = mc.step; ff = step.ff
    nkinds = size(ff.interactions, 1)
    charge = Float64[k <= length(step.charges) ? NoUnits(step.charges[k]/u"e_au") : 0.0 for k in 1:nkinds]
    charge[isnan.(charge)] .= 0.0
    flat = CegRule[]; offsets = Int32[0]
    for a in 1:nkinds, b in 1:nkinds
        for r in _rules(ff.interactions[a, b])
            p = r.params
            push!(flat, CegRule(Int32(Int(r.kind)), 0, get(p, 1, 0.0), get(p, 2, 0.0), get(p, 3, 0.0), r.shift))
        end
        push!(offsets, Int32(length(flat)))
    end
    mat = Vector{Float64}(vec(NoUnits.(step.mat ./ u"Å"))); invmat = Vector{Float64}(vec(inv(NoUnits.(step.mat ./ u"Å"))))
    ef = mc.ewald.ctx.eframework
    ijk = Int32[]
    for (jy, jz, jxrange, _) in ef.kspace.kindices, jx in jxrange
        push!(ijk, jx, jy, jz)
    end
    sf = ef.StoreRigidChargeFramework
    re, im_ = Vector{Float64}(real.(sf)), Vector{Float64}(imag.(sf))
    ks = Int32[ef.kspace.ks...]; einv = Vector{Float64}(vec(NoUnits.(ef.invmat .* u"Å")))
    cutoff2 = NoUnits(ff.cutoff^2/u"Å^2")
    coulombic = ustrip(u"K*Å/e_au^2", COULOMBIC_CONVERSION_FACTOR)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve vdw charge mat invmat flat offsets ijk re im_ ks einv _check(ccall((:ceg_mc_create, LIB[]), Cint,
        (Ref{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Float64,
         Ptr{CegRule}, Ptr{Int32}, Float64, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int32}, Ptr{Float64}),
        h, device, vdw, coulomb, charge, nkinds, mat, invmat, cutoff2, flat, offsets, coulombic,
        ijk, ef.kfactors, re, im_, length(ef.kfactors), ks, einv))
    # guests in the order of the Ewald indices ij (mc.revflatidx)
    pos = Float64[]; kinds = Int32[]; first = Int32[0]
    for (i, j) in mc.revflatidx
        for (k, l) in enumerate(step.posidx[i][j])
            append!(pos, NoUnits.(step.positions[l] ./ u"Å")); push!(kinds, Int32(step.ffidx[i][k] - 1))
        end
        push!(first, Int32(length(kinds)))
    end
    GC.@preserve pos kinds first _check(ccall((:ceg_mc_set_guests, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Int32), h[], pos, kinds, first, length(first)-1))
    h[]
end

"movement_energy of species `ij` (Ewald index, 1-based) where it is (column 1) and at `newpos` (column 2); rows: framework vdw, framework direct, inter, reciprocal (K)"
function mc_trial(h::Ptr{Cvoid}, ij::Int, newpos)
    pts = _pts(newpos); out = Matrix{Float64}(undef, 4, 2)
    GC.@preserve pts out _check(ccall((:ceg_mc_trial, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Float64}),
                                      h, ij - 1, pts, 1, out))
    out
end

"""
`n` trial placements of species `ij` that already lie in DEVICE memory (`d_trial`: 3 x m x n Float64, e.g. `pointer(::ROCArray)`),
rows into device memory `d_out` (4 x (n + 1) Float64, column 1 = where it is), enqueued on `stream` (a `hipStream_t`, `C_NULL` = null stream):
no copy, no synchronisation.
"""
function mc_trial_device(h::Ptr{Cvoid}, ij::Int, d_trial::Ptr{Float64}, n::Integer, d_out::Ptr{Float64}, stream::Ptr{Cvoid}=C_NULL)
    _check(ccall((:ceg_mc_trial_device, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Cvoid}),
                 h, ij - 1, d_trial, n, d_out, stream))
    nothing
end

"the same for a NEW species with ff indices `idx` (rows 4 x n)"
function mc_trial_insert_device(h::Ptr{Cvoid}, idx::Vector{Int}, d_trial::Ptr{Float64}, n::Integer, d_out::Ptr{Float64}, stream::Ptr{Cvoid}=C_NULL)
    kinds = Int32.(idx .- 1)
    GC.@preserve kinds _check(ccall((:ceg_mc_trial_insert_device, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Cvoid}), h, kinds, length(kinds), d_trial, n, d_out, stream))
    nothing
end

"update_mc!(mc, idx, newpos) for a displacement, on the device (asynchronous)"
function mc_accept(h::Ptr{Cvoid}, ij::Int, newpos)
    pts = _pts(newpos)
    GC.@preserve pts _check(ccall((:ceg_mc_accept, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), h, ij - 1, pts))
    nothing
end

"movement_energy of a NEW species with ff indices `idx` at `newpos` (ij < 0 in src/ewald.jl:704-728) -> 4 energies"
function mc_trial_insert(h::Ptr{Cvoid}, idx::Vector{Int}, newpos)
    pts = _pts(newpos); kinds = Int32.(idx .- 1); out = Vector{Float64}(undef, 4)
    GC.@preserve pts kinds out _check(ccall((:ceg_mc_trial_insert, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Float64}, Int64, Ptr{Float64}), h, kinds, length(kinds), pts, 1, out))
    out
end

"add_one_system! on the device; returns the new Ewald index ij (1-based)"
function mc_insert(h::Ptr{Cvoid}, idx::Vector{Int}, newpos)
    pts = _pts(newpos); kinds = Int32.(idx .- 1); ij = Ref{Int32}(-1)
    GC.@preserve pts kinds _check(ccall((:ceg_mc_insert, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Float64}, Ref{Int32}), h, kinds, length(kinds), pts, ij))
    Int(ij[]) + 1
end

"remove_one_system! on the device; returns oldij like src/ewald.jl:404-413 (the species that now answers to `ij`)"
function mc_remove(h::Ptr{Cvoid}, ij::Int)
    moved = Ref{Int32}(-1)
    _check(ccall((:ceg_mc_remove, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}), h, ij - 1, moved))
    Int(moved[]) + 1
end

# ---- chain groups (ceg_mc_group_*): the chains of make_isotherm (src/parameterinputs.jl:316-329), one per pressure, stepped in
# lockstep -- one launch for every chain's trial, one for every accepted move.  Like the rest of this file these four are not
# executed here (no Julia in the build image); tests/test_gpu_mc_chains.py runs the same calls through ceg_hip.energy.

"`ceg_mc_group_create` over the handles of K chains (`mc_handle`, one per `run_gcmc`); drive the group and its chains from one task"
function mc_group(handles::Vector{Ptr{Cvoid}})
    g = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handles _check(ccall((:ceg_mc_group_create, LIB[]), Cint, (Ref{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Int32),
                                      g, handles, length(handles)))
    g[]
end

"""
One trial per chain: `moves[c]` is `(ij, placements)` (displacement of species `ij`, Ewald index, 1-based; 4 x (n + 1) energies,
column 1 where it is; `placements` empty for the deletion energy), `(:insert, placements)` (a new species with ff indices
`insert_idx`, 4 x n) or `nothing` (idle).  Each placement is a vector of positions.  Returns the energies per chain.
"""
function mc_group_trial!(g::Ptr{Cvoid}, moves::Vector, insert_idx::Vector{Int}=Int[])
    k = length(moves)
    mol = fill(Int32(-2), k); n = zeros(Int32, k); nrows = zeros(Int, k); pts = Float64[]
    for (c, mv) in enumerate(moves)
        mv === nothing && continue
        what, placements = mv
        for p in placements
            append!(pts, _pts(p))
        end
        n[c] = length(placements)
        mol[c] = what === :insert ? Int32(-1) : Int32(what - 1)
        nrows[c] = length(placements) + (what === :insert ? 0 : 1)
    end
    kinds = Int32.(insert_idx .- 1); out = Matrix{Float64}(undef, 4, sum(nrows))
    GC.@preserve mol n kinds pts out _check(ccall((:ceg_mc_group_trial, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Float64}, Ptr{Float64}), g, mol, n, kinds, length(kinds), pts, out))
    first = cumsum([0; nrows])
    [moves[c] === nothing ? nothing : out[:, first[c]+1:first[c+1]] for c in 1:k]
end

"update_mc! on every chain whose entry of `accepted` is `(ij, newpos)` (`nothing`: no change); asynchronous"
function mc_group_accept!(g::Ptr{Cvoid}, accepted::Vector)
    mol = Int32[a === nothing ? -1 : a[1] - 1 for a in accepted]
    pts = Float64[]
    for a in accepted
        a === nothing || append!(pts, _pts(a[2]))
    end
    GC.@preserve mol pts _check(ccall((:ceg_mc_group_accept, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}), g, mol, pts))
    nothing
end

# `ceg_mc_sweep_params_t`, `ceg_mc_sweep_stats_t`, `ceg_mc_sweep_record_t` of include/ceg_hip.h
struct McSweepParams
    seed::UInt64
    first_step::UInt64
    stream_id::Ptr{UInt32}
    temperature::Ptr{Float64}
    dmax::Ptr{Float64}
    thetamax::Ptr{Float64}
    p_rotation::Ptr{Float64}
    bead::Ptr{Int32}
end
struct McSweepStats
    translation_trials::Int64
    translation_accepted::Int64
    rotation_trials::Int64
    rotation_accepted::Int64
    blocked::Int64
    delta::Float64
end
struct McSweepRecord
    molecule::Int32        # 0-based Ewald index, -1 for an idle chain
    kind::Int32            # 0 translation, 1 rotation, -1 idle
    accepted::Int32
    _pad::Int32
    u::Float64
    rows::NTuple{8,Float64}          # before (4), after (4)
    positions::NTuple{48,Float64}    # x, y, z of up to 16 atoms
end

"""
`ceg_mc_group_sweep`: `nsteps` steps of the inner loop of `run_montecarlo!` (src/simulation.jl:727-781; translations and rotations)
for every chain of the group, proposals and Metropolis rule on the device, one synchronisation at the end.  `temperature` (K),
`dmax` (Å), `thetamax` (unitful angle or radians) and `p_rotation` per chain; `bead[c]` the 1-based reference atom of every species
of chain `c` in Ewald order (`mc.bead[i]` of its kind); step `s` of the call is step `first_step + s` of the counter-based stream.
Returns the statistics per chain and, with `log=true`, the `nsteps x K` records (stored chain-fastest).
"""
function mc_group_sweep!(g::Ptr{Cvoid}, nsteps::Integer, seed::Integer, first_step::Integer, temperature::Vector, dmax::Vector,
                         thetamax::Vector, p_rotation::Vector{Float64}, bead::Vector{Vector{Int}};
                         stream_id::Vector{UInt32}=UInt32.(0:length(temperature)-1), log::Bool=false)
    k = length(temperature)
    T = Float64[ustrip(u"K", t) for t in temperature]
    dm = Float64[d isa Real ? d : ustrip(u"Å", d) for d in dmax]
    th = Float64[t isa Real ? t : ustrip(u"rad", t) for t in thetamax]
    beads = Int32[b - 1 for chain in bead for b in chain]
    stats = Vector{McSweepStats}(undef, k)
    records = Matrix{McSweepRecord}(undef, k, log ? nsteps : 0)
    GC.@preserve stream_id T dm th p_rotation beads stats records begin
        params = Ref(McSweepParams(UInt64(seed), UInt64(first_step), pointer(stream_id), pointer(T), pointer(dm), pointer(th),
                                   pointer(p_rotation), pointer(beads)))
        _check(ccall((:ceg_mc_group_sweep, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                     g, params, nsteps, stats, log && nsteps > 0 ? pointer(records) : C_NULL))
    end
    log ? (stats, records) : stats
end

# `ceg_mc_gcmc_species_t`, `ceg_mc_gcmc_params_t`, `ceg_mc_gcmc_stats_t`, `ceg_mc_gcmc_record_t` of include/ceg_hip.h
# (584, 88, 192 and 488 bytes; CEG_MC_GCMC_MAX_SPECIES = 8)
struct McGcmcSpecies
    m::Int32
    bead::Int32                      # 0-based
    kinds::NTuple{16,Int32}          # 0-based force-field indices
    model::NTuple{48,Float64}        # x, y, z of up to 16 atoms (mc.models[i])
    cumulative::NTuple{5,Float64}    # MCMoves.cumulatives
    phiPV_div_k::Float64
    self_reciprocal::Float64         # ctx.energies[i]
    tail_framework::Float64
    tail_cross::NTuple{8,Float64}
end
struct McGcmcParams
    seed::UInt64
    first_step::UInt64
    stream_id::Ptr{UInt32}
    temperature::Ptr{Float64}
    dmax::Ptr{Float64}
    thetamax::Ptr{Float64}
    nspecies::Int32
    _pad::Int32
    species::Ptr{McGcmcSpecies}
    molecule_species::Ptr{Int32}
    max_molecules::Ptr{Int32}
    molecule_species_out::Ptr{Int32}
end
struct McGcmcStats
    trials::NTuple{7,Int64}          # translation, rotation, random_translation, random_rotation, random_reinsertion, swap_insertion, swap_deletion
    accepted::NTuple{7,Int64}
    blocked::Int64
    capacity::Int64
    spent::Int64
    delta_moves::Float64
    delta_swaps::Float64
    count::NTuple{8,Int32}
    nmol::Int32
    _pad::Int32
end
struct McGcmcRecord
    species::Int32
    molecule::Int32
    kind::Int32
    accepted::Int32
    n_species::Int32
    flags::Int32                     # 1 spent, 2 blocked, 4 capacity
    u::Float64
    tc::Float64
    rows::NTuple{8,Float64}
    positions::NTuple{48,Float64}
end

"""
`ceg_mc_group_sweep_gcmc`: `nsteps` steps of the inner loop of `run_montecarlo!` (src/simulation.jl:730-781) with all six move kinds of
`MCMoves`, swaps included, on the device; the molecule table changes there and `molecule_species` (0-based species of every molecule
of every chain, in Ewald order) is the table the sweep starts from; it is left as it is, and the final table is returned.  `species` is built by the caller from `mc.mcmoves[i].cumulatives`,
`mc.models[i]`, `mc.bead[i] - 1`, `φPV_div_k[i]`, `mc.ewald.ctx.energies[i]` and the rows of `mc.tailcorrection`.  Returns the statistics
per chain (and the records with `log=true`) and the final species of every chain's molecules.  Never executed here (no Julia in the image).
"""
function mc_group_sweep_gcmc!(g::Ptr{Cvoid}, nsteps::Integer, seed::Integer, first_step::Integer, temperature::Vector, dmax::Vector,
                              thetamax::Vector, species::Vector{McGcmcSpecies}, molecule_species::Vector{Vector{Int32}},
                              max_molecules::Vector{Int32}; stream_id::Vector{UInt32}=UInt32.(0:length(temperature)-1), log::Bool=false)
    k = length(temperature)
    T = Float64[ustrip(u"K", t) for t in temperature]
    dm = Float64[d isa Real ? d : ustrip(u"Å", d) for d in dmax]
    th = Float64[t isa Real ? t : ustrip(u"rad", t) for t in thetamax]
    given = Int32[s for chain in molecule_species for s in chain]
    push!(given, Int32(0))
    out = fill(Int32(-1), max(sum(max_molecules), 1))
    stats = Vector{McGcmcStats}(undef, k)
    records = Matrix{McGcmcRecord}(undef, k, log ? nsteps : 0)
    GC.@preserve stream_id T dm th species given max_molecules out stats records begin
        params = Ref(McGcmcParams(UInt64(seed), UInt64(first_step), pointer(stream_id), pointer(T), pointer(dm), pointer(th),
                                  Int32(length(species)), Int32(0), pointer(species), pointer(given), pointer(max_molecules), pointer(out)))
        _check(ccall((:ceg_mc_group_sweep_gcmc, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                     g, params, nsteps, stats, log && nsteps > 0 ? pointer(records) : C_NULL))
    end
    offsets = cumsum(vcat(0, max_molecules))
    final = [out[offsets[c]+1:offsets[c]+stats[c].nmol] for c in 1:k]
    log ? (stats, final, records) : (stats, final)
end

# `ceg_mc_cycles_t` and `ceg_mc_cycle_record_t` of include/ceg_hip.h (48 and 96 bytes)
const MC_ADAPT_DMAX = Int32(1)
const MC_ADAPT_THETAMAX = Int32(2)
struct McCycles
    ncycles::Int64
    steps_per_cycle::Int64
    cycle0::Int64                    # counter_cycle of the first cycle of this call (>= 1)
    adapt::Int32                     # MC_ADAPT_* bits
    _pad::Int32
    temperatures::Ptr{Float64}       # K x ncycles (chain-fastest), or C_NULL: the temperature of the parameters throughout
    prior::Ptr{Int64}                # 4 x K: translation trials, accepted, rotation trials, accepted before this call; C_NULL: zeros
end
struct McCycleRecord
    temperature::Float64             # in force during the cycle
    dmax::Float64
    thetamax::Float64                # rad
    dmax_next::Float64               # after the adaptation at the end of the cycle
    thetamax_next::Float64
    delta_moves::Float64             # the call's sums as they stand at the end of the cycle
    delta_swaps::Float64
    translation_trials::Int64        # prior + this call, at the end of the cycle
    translation_accepted::Int64
    rotation_trials::Int64
    rotation_accepted::Int64
    nmol::Int32
    _pad::Int32
end

# the `ceg_mc_cycles_t` of a call and the arrays it points to (keep them alive across the ccall)
function _mc_cycles(k::Integer, ncycles::Integer, steps_per_cycle::Integer, temperatures, adapt::Integer, cycle0::Integer, prior)
    table = temperatures isa AbstractMatrix ? Float64[ustrip(u"K", temperatures[j, c]) for c in 1:k, j in 1:ncycles] : nothing
    pr = prior === nothing ? nothing : Int64[prior[c][q] for q in 1:4, c in 1:k]
    cyc = McCycles(Int64(ncycles), Int64(steps_per_cycle), Int64(cycle0), Int32(adapt), Int32(0),
                   table === nothing ? Ptr{Float64}(C_NULL) : pointer(table), pr === nothing ? Ptr{Int64}(C_NULL) : pointer(pr))
    cyc, table, pr
end

"""
`ceg_mc_group_sweep_cycles`: `ncycles` whole cycles of `steps_per_cycle` steps of `mc_group_sweep!` with the end-of-cycle block of
`run_montecarlo!` (src/simulation.jl:727-728, 818-827) on the device: `temperatures` is a vector (one per chain, in force throughout) or
an `ncycles x K` matrix whose row `j` is in force during cycle `j` (`simu.temperatures`), and `statistics.dmax` / `θmax` are adapted
from the cumulative acceptance ratios after every cycle (`adapt`: `MC_ADAPT_*` bits).  `cycle0` is the `counter_cycle` of the first
cycle of this call, `prior[c]` the (translation trials, accepted, rotation trials, accepted) of chain `c` before it.  Returns the
statistics, the `ncycles x K` cycle records (stored chain-fastest) and, with `log=true`, the step records.  thetamax is held in
radians: the adaptation is a restatement of the reference's degree arithmetic, equal to rounding.  Never executed here (no Julia in
the image).
"""
function mc_group_sweep_cycles!(g::Ptr{Cvoid}, ncycles::Integer, steps_per_cycle::Integer, seed::Integer, first_step::Integer, temperatures,
                                dmax::Vector, thetamax::Vector, p_rotation::Vector{Float64}, bead::Vector{Vector{Int}};
                                adapt::Integer=MC_ADAPT_DMAX | MC_ADAPT_THETAMAX, cycle0::Integer=1, prior=nothing,
                                stream_id::Vector{UInt32}=UInt32.(0:length(dmax)-1), log::Bool=false)
    k = length(dmax)
    cyc, table, pr = _mc_cycles(k, ncycles, steps_per_cycle, temperatures, adapt, cycle0, prior)
    T = table === nothing ? Float64[ustrip(u"K", t) for t in temperatures] : Float64[]
    dm = Float64[d isa Real ? d : ustrip(u"Å", d) for d in dmax]
    th = Float64[t isa Real ? t : ustrip(u"rad", t) for t in thetamax]
    beads = Int32[b - 1 for chain in bead for b in chain]
    nsteps = ncycles * steps_per_cycle
    stats = Vector{McSweepStats}(undef, k)
    cycles = Matrix{McCycleRecord}(undef, k, ncycles)
    records = Matrix{McSweepRecord}(undef, k, log ? nsteps : 0)
    GC.@preserve stream_id T dm th p_rotation beads stats cycles records table pr begin
        params = Ref(McSweepParams(UInt64(seed), UInt64(first_step), pointer(stream_id), table === nothing ? pointer(T) : Ptr{Float64}(C_NULL),
                                   pointer(dm), pointer(th), pointer(p_rotation), pointer(beads)))
        _check(ccall((:ceg_mc_group_sweep_cycles, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     g, params, Ref(cyc), stats, ncycles > 0 ? pointer(cycles) : C_NULL, log && nsteps > 0 ? pointer(records) : C_NULL))
    end
    log ? (stats, cycles, records) : (stats, cycles)
end

"""
`ceg_mc_group_sweep_gcmc_cycles`: the same for `mc_group_sweep_gcmc!` -- a whole GCMC production run of K chains in one call.  Where a
species has a swap probability > 0 every chain's temperature must be constant over the cycles (src/simulation.jl:688).  Returns the
statistics, the final species of every chain's molecules, the cycle records and, with `log=true`, the step records.  Never executed
here (no Julia in the image).
"""
function mc_group_sweep_gcmc_cycles!(g::Ptr{Cvoid}, ncycles::Integer, steps_per_cycle::Integer, seed::Integer, first_step::Integer, temperatures,
                                     dmax::Vector, thetamax::Vector, species::Vector{McGcmcSpecies}, molecule_species::Vector{Vector{Int32}},
                                     max_molecules::Vector{Int32}; adapt::Integer=MC_ADAPT_DMAX | MC_ADAPT_THETAMAX, cycle0::Integer=1,
                                     prior=nothing, stream_id::Vector{UInt32}=UInt32.(0:length(dmax)-1), log::Bool=false)
    k = length(dmax)
    cyc, table, pr = _mc_cycles(k, ncycles, steps_per_cycle, temperatures, adapt, cycle0, prior)
    T = table === nothing ? Float64[ustrip(u"K", t) for t in temperatures] : Float64[]
    dm = Float64[d isa Real ? d : ustrip(u"Å", d) for d in dmax]
    th = Float64[t isa Real ? t : ustrip(u"rad", t) for t in thetamax]
    given = Int32[s for chain in molecule_species for s in chain]
    push!(given, Int32(0))
    out = fill(Int32(-1), max(sum(max_molecules), 1))
    nsteps = ncycles * steps_per_cycle
    stats = Vector{McGcmcStats}(undef, k)
    cycles = Matrix{McCycleRecord}(undef, k, ncycles)
    records = Matrix{McGcmcRecord}(undef, k, log ? nsteps : 0)
    GC.@preserve stream_id T dm th species given max_molecules out stats cycles records table pr begin
        params = Ref(McGcmcParams(UInt64(seed), UInt64(first_step), pointer(stream_id), table === nothing ? pointer(T) : Ptr{Float64}(C_NULL),
                                  pointer(dm), pointer(th), Int32(length(species)), Int32(0), pointer(species), pointer(given),
                                  pointer(max_molecules), pointer(out)))
        _check(ccall((:ceg_mc_group_sweep_gcmc_cycles, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     g, params, Ref(cyc), stats, ncycles > 0 ? pointer(cycles) : C_NULL, log && nsteps > 0 ? pointer(records) : C_NULL))
    end
    offsets = cumsum(vcat(0, max_molecules))
    final = [out[offsets[c]+1:offsets[c]+stats[c].nmol] for c in 1:k]
    log ? (stats, final, cycles, records) : (stats, final, cycles)
end

# `ceg_mc_block_t` of include/ceg_hip.h (240 bytes)
struct McBlock
    mask::Ptr{UInt8}                 # host memory, [x][y][z] with z fastest; C_NULL: an empty block
    dims::NTuple{3,Int32}
    _pad::Int32
    size::NTuple{3,Float64}
    shift::NTuple{3,Float64}
    offset::NTuple{3,Float64}
    mat::NTuple{9,Float64}           # column-major
    invmat::NTuple{9,Float64}
end

_block_mask(b::CEG.BlockFile) = b.empty ? UInt8[] : vec(UInt8.(permutedims(b.block, (3, 2, 1))))
function _mc_block(b::CEG.BlockFile, mask::Vector{UInt8}, half::Bool)
    cs = b.csetup
    size = Float64[NoUnits(x/u"Å") for x in cs.size]
    offset = half ? (size ./ cs.dims) ./ 2 : zeros(3)
    McBlock(isempty(mask) ? Ptr{UInt8}(C_NULL) : pointer(mask), Tuple(Int32.(cs.dims)), Int32(0), Tuple(size),
            Tuple(Float64[NoUnits(x/u"Å") for x in cs.shift]), Tuple(offset), Tuple(Float64[NoUnits(x/u"Å") for x in vec(cs.cell.mat)]),
            Tuple(Float64[NoUnits(x*u"Å") for x in vec(cs.cell.invmat)]))
end

"""
`ceg_mc_group_set_blocks`: the block pockets `ceg_mc_group_sweep_gcmc` tests like `choose_step!` (src/simulation.jl:271-326):
`speciesblocks` = `mc.speciesblocks`, `atomblocks` = `mc.atomblocks` (looked up at `pos + Δ/2`, src/montecarlo.jl:636; empty: none).
The masks are copied to the device; two empty vectors clear them.  Never executed here (no Julia in the image).
"""
function mc_group_set_blocks!(g::Ptr{Cvoid}, speciesblocks::Vector{CEG.BlockFile}, atomblocks::Vector{CEG.BlockFile}=CEG.BlockFile[])
    smasks = [_block_mask(b) for b in speciesblocks]
    amasks = [_block_mask(b) for b in atomblocks]
    GC.@preserve smasks amasks begin
        sb = McBlock[_mc_block(b, m, false) for (b, m) in zip(speciesblocks, smasks)]
        ab = McBlock[_mc_block(b, m, true) for (b, m) in zip(atomblocks, amasks)]
        GC.@preserve sb ab _check(ccall((:ceg_mc_group_set_blocks, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32),
                                        g, isempty(sb) ? C_NULL : pointer(sb), length(sb), isempty(ab) ? C_NULL : pointer(ab), length(ab)))
    end
    nothing
end

"`ceg_mc_group_block_counts`: per chain, the pocket-blocked steps of the last GCMC sweep and the sum of the attempt indices it used"
function mc_group_block_counts(g::Ptr{Cvoid}, k::Integer)
    pocket = zeros(Int64, k)
    attempts = zeros(Int64, k)
    _check(ccall((:ceg_mc_group_block_counts, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), g, pocket, attempts))
    pocket, attempts
end

# `ceg_mc_chain_plan_t` of include/ceg_hip.h (24 bytes)
struct McChainPlan
    nspecies::Int32
    _pad::Int32
    phiPV_div_k::Ptr{Float64}        # [K][nspecies] in K, species fastest; C_NULL: the species table's value for every chain
    stop_step::Ptr{Int64}            # [K] absolute steps; C_NULL: no chain ever stops
end

"""
`ceg_mc_group_set_chain_plan`: what differs between the chains of `make_isotherm` (src/parameterinputs.jl:305-334).  `phiPV_div_k` is an
`nspecies x K` matrix (`φPV_div_k[i]` of src/simulation.jl:714-715 for the pressure of chain `c` in column `c`; unitful or in K) that
replaces the species table's value in the swap rules of `mc_group_sweep_gcmc!` / `mc_group_sweep_gcmc_cycles!`; chain `c` takes no part
in the absolute steps `s ≥ stop_step[c]` of any sweep (its `ncycles` of :319 times `steps_per_cycle`, counted from step 0 of the run).
Either may be `nothing`; both `nothing` removes the plan.  Never executed here (no Julia in the image).
"""
function mc_group_set_chain_plan!(g::Ptr{Cvoid}; phiPV_div_k::Union{Nothing,AbstractMatrix}=nothing, stop_step::Union{Nothing,AbstractVector{<:Integer}}=nothing)
    if phiPV_div_k === nothing && stop_step === nothing
        _check(ccall((:ceg_mc_group_set_chain_plan, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, C_NULL))
        return nothing
    end
    phi = phiPV_div_k === nothing ? Float64[] : Float64[x isa Real ? x : ustrip(u"K", x) for x in vec(phiPV_div_k)]
    stop = stop_step === nothing ? Int64[] : Vector{Int64}(stop_step)
    GC.@preserve phi stop begin
        plan = Ref(McChainPlan(phiPV_div_k === nothing ? Int32(0) : Int32(size(phiPV_div_k, 1)), Int32(0),
                               phiPV_div_k === nothing ? Ptr{Float64}(C_NULL) : pointer(phi), stop_step === nothing ? Ptr{Int64}(C_NULL) : pointer(stop)))
        _check(ccall((:ceg_mc_group_set_chain_plan, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, plan))
    end
    nothing
end

"""
`ceg_mc_group_set_device_cells`: with `on`, the four sweep entry points (`mc_group_sweep!`, `mc_group_sweep_gcmc!` and their `_cycles!`
forms) take the chains that keep their guests in neighbour cells (their cell lists are kept on the device during a sweep);
`capacity > 0` gives such chains at least that many entries per cell.  Never executed here (no Julia in the image).
"""
function mc_group_set_device_cells!(g::Ptr{Cvoid}, on::Bool=true; capacity::Integer=0)
    _check(ccall((:ceg_mc_group_set_device_cells, LIB[]), Cint, (Ptr{Cvoid}, Int32, Int32), g, on ? 1 : 0, capacity))
    nothing
end

"`ceg_mc_group_halted`: per chain the absolute step at which the last sweep call halted it on a full cell (continue from it with a larger capacity), -1 if it did not"
function mc_group_halted(g::Ptr{Cvoid}, k::Integer)
    halted = fill(Int64(-1), k)
    _check(ccall((:ceg_mc_group_halted, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}), g, halted))
    halted
end

# `ceg_mc_tempering_t` (32 bytes) and `ceg_mc_exchange_record_t` (48 bytes) of include/ceg_hip.h
struct McTempering
    every::Int64
    record_capacity::Int64
    rung::Ptr{Int32}                 # [K] 0-based, a permutation; C_NULL: chain c on rung c
    energy::Ptr{Float64}             # [K] in K
end

struct McExchangeRecord
    rung::Int32                      # 0-based, during the ended cycle
    rung_next::Int32
    partner::Int32                   # 0-based chain, -1: none
    accepted::Int32                  # 1, 0, or -1: no attempt
    energy::Float64
    temperature_next::Float64
    u::Float64
    threshold::Float64
end

"""
`ceg_mc_group_set_tempering`: replica exchange between the chains on neighbouring rungs of the temperature ladder at the end of every
cycle `cc` with `cc % every == 0` of `mc_group_sweep_cycles!` / `mc_group_sweep_gcmc_cycles!` (`run_parallel_tempering`,
src/simulation.jl:461-622; the rule of :533).  Temperatures are exchanged, not configurations: the temperatures of those calls are then
indexed by rung.  `energy`: the total energy of every chain now (unitful or in K); `rung`: 0-based, `nothing` for the identity;
`energy === nothing` removes the state.  UNVERIFIED: never executed.
"""
function mc_group_set_tempering!(g::Ptr{Cvoid}, energy::Union{Nothing,AbstractVector}; every::Integer=1, capacity::Integer=1024,
                                 rung::Union{Nothing,AbstractVector{<:Integer}}=nothing)
    if energy === nothing
        _check(ccall((:ceg_mc_group_set_tempering, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, C_NULL))
        return nothing
    end
    e = Float64[x isa Real ? x : ustrip(u"K", x) for x in energy]
    r = rung === nothing ? Int32[] : Vector{Int32}(rung)
    GC.@preserve e r begin
        spec = Ref(McTempering(Int64(every), Int64(capacity), rung === nothing ? Ptr{Int32}(C_NULL) : pointer(r), pointer(e)))
        _check(ccall((:ceg_mc_group_set_tempering, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, spec))
    end
    nothing
end

"""
`ceg_mc_group_tempering_read` for a group of `k` chains -> (rungs (0-based), energies (K), pair counts `2 x k`: attempted and accepted of
the rung pair (r, r + 1) in column r, records `k x cycles`).  UNVERIFIED: never executed.
"""
function mc_group_tempering_read(g::Ptr{Cvoid}, k::Integer)
    n = Ref{Int64}(0)
    _check(ccall((:ceg_mc_group_tempering_read, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}),
                 g, C_NULL, C_NULL, C_NULL, C_NULL, n))
    rung = zeros(Int32, k)
    energy = zeros(Float64, k)
    pairs = zeros(Int64, 2, k)
    records = Matrix{McExchangeRecord}(undef, k, n[])
    _check(ccall((:ceg_mc_group_tempering_read, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}),
                 g, rung, energy, pairs, records, n))
    rung, energy, pairs, records
end

# `ceg_mc_recorder_t` (48 bytes) and `ceg_mc_snapshot_record_t` (40 bytes) of include/ceg_hip.h
struct McRecorder
    every::Int64                     # 0: no periodic frames
    origin::Int64
    frame_capacity::Int64
    max_atoms::Int32
    max_molecules::Int32
    track_min::Int32
    _pad::Int32
    energy::Ptr{Float64}             # [K] in K
end

struct McSnapshotRecord
    cycle::Int64                     # -1: mc_group_snapshot!, or the state at installation
    step::Int64
    energy::Float64
    nmol::Int32
    natoms::Int32
    flags::Int32                     # 1: does not fit, no body; 2: stopped or halted
    _pad::Int32
end

"""
`ceg_mc_group_set_recorder`: from now on `mc_group_sweep_cycles!` / `mc_group_sweep_gcmc_cycles!` take a frame of every chain's
positions at the end of cycle `cc` iff `every > 0 && cc >= origin && (cc - origin) % every == 0` (the trajectory of `run_montecarlo!`,
src/simulation.jl:784-799) and, with `track_min`, keep the lowest-energy configuration per chain (`RMinimumEnergy`,
src/parameterinputs.jl:86-108), on the device.  `energy`: the total energy of every chain now (unitful or in K);
`energy === nothing` removes the recorder.  UNVERIFIED: never executed.
"""
function mc_group_set_recorder!(g::Ptr{Cvoid}, energy::Union{Nothing,AbstractVector}; every::Integer=1, origin::Integer=0,
                                capacity::Integer=1024, max_atoms::Integer=1, max_molecules::Integer=1, track_min::Bool=false)
    if energy === nothing
        _check(ccall((:ceg_mc_group_set_recorder, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, C_NULL))
        return nothing
    end
    e = Float64[x isa Real ? x : ustrip(u"K", x) for x in energy]
    GC.@preserve e begin
        spec = Ref(McRecorder(Int64(every), Int64(origin), Int64(capacity), Int32(max_atoms), Int32(max_molecules), Int32(track_min), Int32(0),
                              pointer(e)))
        _check(ccall((:ceg_mc_group_set_recorder, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, spec))
    end
    nothing
end

"""
`ceg_mc_group_snapshot`: one frame of the resident state now, asynchronous on the group's stream.  UNVERIFIED: never executed.
"""
function mc_group_snapshot!(g::Ptr{Cvoid})
    _check(ccall((:ceg_mc_group_snapshot, LIB[]), Cint, (Ptr{Cvoid},), g))
    nothing
end

"""
`ceg_mc_group_recorder_read` for a group of `k` chains whose recorder was installed with `max_atoms` / `max_molecules` -> (records
`k x frames`, xyz `3 x max_atoms x k x frames` in Å, kinds (0-based) `max_atoms x k x frames`, mol_first (0-based)
`(max_molecules + 1) x k x frames`, species (0-based, -1: unknown) `max_molecules x k x frames`).  UNVERIFIED: never executed.
"""
function mc_group_recorder_read(g::Ptr{Cvoid}, k::Integer, max_atoms::Integer, max_molecules::Integer)
    n = Ref{Int64}(0)
    _check(ccall((:ceg_mc_group_recorder_read, LIB[]), Cint,
                 (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                 g, Int64(0), Int64(0), C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, n))
    records = Matrix{McSnapshotRecord}(undef, k, n[])
    xyz = zeros(Float64, 3, max_atoms, k, n[])
    kinds = zeros(Int32, max_atoms, k, n[])
    first = zeros(Int32, max_molecules + 1, k, n[])
    species = zeros(Int32, max_molecules, k, n[])
    _check(ccall((:ceg_mc_group_recorder_read, LIB[]), Cint,
                 (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                 g, Int64(0), n[], records, xyz, kinds, first, species, n))
    records, xyz, kinds, first, species
end

"""
`ceg_mc_group_recorder_min` -> (mink, mine (K), records `k`, xyz, kinds, mol_first, species as `mc_group_recorder_read` lays them out,
without the frame axis).  UNVERIFIED: never executed.
"""
function mc_group_recorder_min(g::Ptr{Cvoid}, k::Integer, max_atoms::Integer, max_molecules::Integer)
    mink = zeros(Int64, k)
    mine = zeros(Float64, k)
    records = Vector{McSnapshotRecord}(undef, k)
    xyz = zeros(Float64, 3, max_atoms, k)
    kinds = zeros(Int32, max_atoms, k)
    first = zeros(Int32, max_molecules + 1, k)
    species = zeros(Int32, max_molecules, k)
    _check(ccall((:ceg_mc_group_recorder_min, LIB[]), Cint,
                 (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                 g, mink, mine, records, xyz, kinds, first, species))
    mink, mine, records, xyz, kinds, first, species
end

# `ceg_mc_sampler_t` (152 bytes) and `ceg_mc_sample_record_t` (64 bytes) of include/ceg_hip.h
struct McSampler
    every::Int64
    from_step::Int64
    series_capacity::Int64
    dims::NTuple{3,Int32}            # na, nb, nc; all zero: the series only
    nmaps::Int32
    nchannels::Int32
    nkinds::Int32
    nsym::Int32
    _pad::Int32
    unit_invmat::NTuple{9,Float64}   # column-major
    chain_map::Ptr{Int32}
    kind_channel::Ptr{Int32}
    sym::Ptr{Float64}
end
struct McSampleRecord
    step::Int64                      # the step the frame follows; -1 from mc_group_sample!
    nmol::Int32
    natoms::Int32
    count::NTuple{8,Int32}           # molecules per species (GCMC sweeps)
    delta_moves::Float64
    delta_swaps::Float64
end

# what mc_group_sampler_read needs to shape its result: (na, nb, nc, nchannels, nmaps), K, the factor of `total` per frame and map
const SAMPLERS = Dict{Ptr{Cvoid},Tuple{NTuple{5,Int},Int,Vector{Int}}}()

"""
`ceg_mc_group_set_sampler`: from now on `mc_group_sweep!` and `mc_group_sweep_gcmc!` take a frame after every absolute step `s` with
`s ≥ from_step` and `(s + 1) % every == 0`: every atom binned as `bin_trajectory` bins it (src/averageclusters.jl:154-202) and one
record per chain (the `Ns` of `GCMCRecorder`, src/parameterinputs.jl:232-249, and the running energy change) appended to the series.
`mat` is the MC cell (`mc.ewald.mat` without units, Å); the map lives on `mat ./ supercell'`, with `dims` bins or
`floor.(Int, cell_lengths ./ step)` (:169); neither: the series only.  `kind_channel[k]` is the 0-based channel of force-field index
`k` (-1: not binned), `chain_map[c]` the 0-based map of chain `c` (-1: not binned), `symmetries` the `eq(y) = R*y + t` of
`bin_trajectory` as `(R, t)` pairs.  Never executed here (no Julia in the image).
"""
function mc_group_set_sampler!(g::Ptr{Cvoid}, k::Integer, mat::AbstractMatrix{Float64}, every::Integer; from_step::Integer=0, step=nothing,
                               dims=nothing, supercell=(1, 1, 1), kind_channel::Vector{Int32}=Int32[], chain_map::Vector{Int32}=zeros(Int32, k),
                               symmetries=[], series_capacity::Integer=0)
    unit = mat ./ collect(Float64, supercell)'
    if dims === nothing && step !== nothing
        dims = Tuple(floor.(Int, [norm(unit[:, j]) for j in 1:3] ./ (step isa Real ? step : ustrip(u"Å", step))))
    end
    withmap = dims !== nothing
    d = withmap ? NTuple{3,Int32}(Int32.(dims)) : (Int32(0), Int32(0), Int32(0))
    nmaps = withmap ? Int(maximum(chain_map)) + 1 : 0
    nchannels = withmap ? Int(maximum(kind_channel; init=Int32(-1))) + 1 : 0
    sym = Float64[]
    for (R, t) in symmetries, r in 1:3
        append!(sym, (R[r, 1], R[r, 2], R[r, 3], t[r]))
    end
    GC.@preserve chain_map kind_channel sym begin
        spec = Ref(McSampler(every, from_step, series_capacity, d, nmaps, nchannels, length(kind_channel), length(symmetries), 0,
                             Tuple(vec(inv(unit))), pointer(chain_map), pointer(kind_channel), isempty(sym) ? Ptr{Float64}(C_NULL) : pointer(sym)))
        _check(ccall((:ceg_mc_group_set_sampler, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, spec))
    end
    per_frame = [(1 + length(symmetries))*prod(supercell)*count(==(m - 1), chain_map) for m in 1:nmaps]
    SAMPLERS[g] = ((Int(d[1]), Int(d[2]), Int(d[3]), nchannels, nmaps), Int(k), per_frame)
    nothing
end

"`ceg_mc_group_sample`: one frame of the resident state, now (asynchronous), for runs driven through `mc_group_trial!` / `mc_group_accept!`"
function mc_group_sample!(g::Ptr{Cvoid})
    _check(ccall((:ceg_mc_group_sample, LIB[]), Cint, (Ptr{Cvoid},), g))
    nothing
end

"""
`ceg_mc_group_sampler_read` -> `(bins, totals, series)`: `bins::Array{Int,5}` of size `(na, nb, nc, nchannels, nmaps)` --
`bins[:, :, :, ch, m]` is the `Array{Int,3}` of `bin_trajectory` for channel `ch` of map `m` --, `totals[m]` the `total` of
`bin_trajectories` summed over the chains of map `m` (src/averageclusters.jl:196,233-234), and `series`, a `K x frames` matrix of
`McSampleRecord` (chain-fastest): `[r.nmol for r in series[c, :]]` is the `Ns` of chain `c`'s `GCMCRecorder`.
"""
function mc_group_sampler_read(g::Ptr{Cvoid})
    shape, k, per_frame = SAMPLERS[g]
    frames = Ref{Int64}(0)
    _check(ccall((:ceg_mc_group_sampler_read, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}), g, C_NULL, C_NULL, frames))
    bins = zeros(Int64, shape)
    series = Matrix{McSampleRecord}(undef, k, frames[])
    GC.@preserve bins series _check(ccall((:ceg_mc_group_sampler_read, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}),
                                          g, isempty(bins) ? C_NULL : pointer(bins), frames[] > 0 ? pointer(series) : C_NULL, C_NULL))
    bins, frames[] .* per_frame, series
end

"`ceg_mc_group_sampler_reset`: bins, series and the frame count back to zero"
function mc_group_sampler_reset!(g::Ptr{Cvoid})
    _check(ccall((:ceg_mc_group_sampler_reset, LIB[]), Cint, (Ptr{Cvoid},), g))
    nothing
end

# `ceg_mc_baseline_t` of include/ceg_hip.h (48 bytes)
struct McBaseline
    framework_vdw::Float64
    framework_direct::Float64
    inter::Float64
    recip_framework::Float64
    recip_guests::Float64
    nmol::Int32
    natoms::Int32
end
const MC_BASELINE_REFRESH = Int32(1)

"`ceg_mc_baseline`: the sums of `baseline_energy` (src/montecarlo.jl:530-542) over the device state of one chain, in K; `refresh` recomputes every structure factor from the positions first, as `compute_ewald(::IncrementalEwaldContext)` does"
function mc_baseline(h::Ptr{Cvoid}; refresh::Bool=false)
    out = Vector{McBaseline}(undef, 1)
    GC.@preserve out _check(ccall((:ceg_mc_baseline, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}),
                                  h, refresh ? MC_BASELINE_REFRESH : Int32(0), pointer(out)))
    out[1]
end

"`ceg_mc_group_baseline`: the same for the `k` chains of a group in one pass; entry `c` holds what `mc_baseline` gives for chain `c`"
function mc_group_baseline(g::Ptr{Cvoid}, k::Integer; refresh::Bool=false)
    out = Vector{McBaseline}(undef, k)
    GC.@preserve out _check(ccall((:ceg_mc_group_baseline, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}),
                                  g, refresh ? MC_BASELINE_REFRESH : Int32(0), pointer(out)))
    out
end

# ------------------------------------------------------------------ site hopping (src/sitehopping.jl) on the device
# `ceg_site_*` of include/ceg_hip.h: the two tables from a guest-free handle, and whole runs of K chains on them.
# Sites are 0-based on the device: the wrappers below take and return the reference's 1-based `UInt16` sites.
struct SiteParams                    # ceg_site_params_t (24 bytes)
    seed::UInt64
    first_step::UInt64
    stream_id::Ptr{UInt32}           # [K] or C_NULL
end

struct SiteCycles                    # ceg_site_cycles_t (32 bytes)
    ncycles::Int64
    steps_per_cycle::Int64
    cycle0::Int64
    temperature::Ptr{Float64}        # [ncycles][K]
end

struct SiteStats                     # ceg_site_stats_t (32 bytes)
    attempted::Int64
    accepted::Int64
    delta::Float64
    energy::Float64
end

struct SiteCycleRecord               # ceg_site_cycle_record_t (56 bytes)
    cycle::Int64
    temperature::Float64
    energy::Float64
    delta::Float64
    attempted::Int64
    accepted::Int64
    flags::Int32                     # 1: frame taken, 2: frame dropped (store full), 4: new minimum, 8: grouped cycle accepted, 16: restarted
    _pad::Int32
end

struct SiteRecord                    # ceg_site_record_t (40 bytes)
    molecule::Int32
    old_site::Int32
    new_site::Int32
    accepted::Int32
    before::Float64
    after::Float64
    u::Float64
end

struct SiteGroupedRecord             # ceg_site_grouped_record_t (48 bytes)
    before::Float64                  # E0, the energy at the start of the cycle
    restart_energy::Float64          # Er, the baseline of the restart's population (E0 without a restart)
    after::Float64                   # E1, the energy after the hops
    u::Float64
    accepted::Int32
    restarted::Int32
    hops_accepted::Int64
end

struct SiteRecorder                  # ceg_site_recorder_t (32 bytes)
    every::Int64
    origin::Int64
    frame_capacity::Int64
    track_min::Int32
    _pad::Int32
end

struct SiteFrameRecord               # ceg_site_frame_record_t (16 bytes)
    cycle::Int64
    energy::Float64
end

"""
`ceg_site_tables`: `(frameworkenergies, ewaldenergies, interactions)` in K of the constructor of `SiteHopping`
(src/sitehopping.jl:41-82) for `sites` (`3 x m_atoms x n`, Å) of a molecule with the 0-based `kinds`, from the guest-free handle `h`.
`offset_one` = c(1) and `offset_pair` = c(2) - 2c(1) with c(N) = 2 `energy_net_charges` + `static_contribution` of an `EwaldContext`
of N such molecules, in K.  UNVERIFIED: never executed.
"""
function site_tables(h::Ptr{Cvoid}, kinds::Vector{Int32}, sites::Array{Float64,3}, offset_one::Float64, offset_pair::Float64)
    n = size(sites, 3)
    fw = zeros(Float64, n); rec = zeros(Float64, n); inter = zeros(Float64, n, n)
    GC.@preserve kinds sites fw rec inter begin
        _check(ccall((:ceg_site_tables, LIB[]), Cint,
                     (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Float64}, Int32, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     h, kinds, Int32(length(kinds)), sites, Int32(n), offset_one, offset_pair, fw, rec, inter))
    end
    fw, rec, inter
end

"`ceg_site_tables_device`: the same into device memory of the handle's device (three `Ptr{Cvoid}`).  UNVERIFIED: never executed."
function site_tables_device!(d_fw::Ptr{Cvoid}, d_rec::Ptr{Cvoid}, d_inter::Ptr{Cvoid}, h::Ptr{Cvoid}, kinds::Vector{Int32}, sites::Array{Float64,3},
                             offset_one::Float64, offset_pair::Float64)
    GC.@preserve kinds sites begin
        _check(ccall((:ceg_site_tables_device, LIB[]), Cint,
                     (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Float64}, Int32, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     h, kinds, Int32(length(kinds)), sites, Int32(size(sites, 3)), offset_one, offset_pair, d_fw, d_rec, d_inter))
    end
    nothing
end

"""
`ceg_site_group_create`: K chains on one copy of the tables (K); `populations` is `m x K`, 1-based as `sh.population`.
UNVERIFIED: never executed.
"""
function site_group_create(frameworkenergies::Vector{Float64}, interactions::Matrix{Float64}, populations::Matrix{UInt16}, tailcorrection::Float64;
                           device::Integer=0)
    pops = UInt16.(populations .- 0x0001)
    g = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve frameworkenergies interactions pops begin
        _check(ccall((:ceg_site_group_create, LIB[]), Cint,
                     (Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Cvoid}, Float64, Ref{Ptr{Cvoid}}),
                     Int32(device), Int32(length(frameworkenergies)), Int32(size(pops, 1)), Int32(size(pops, 2)), frameworkenergies, interactions,
                     Int32(0), pointer(pops), tailcorrection, g))
    end
    g[]
end

"`ceg_site_group_destroy`.  UNVERIFIED: never executed."
function site_group_destroy!(g::Ptr{Cvoid})
    _check(ccall((:ceg_site_group_destroy, LIB[]), Cint, (Ptr{Cvoid},), g))
    nothing
end

"""
`ceg_site_group_sweep_cycles`: the main loop of `run_montecarlo!(::SiteHopping, simu)` (src/simulation.jl:922-966, `groupcycles = nothing`)
for the `k` chains of `g`: `temperatures` is `K x ncycles` in K.  -> (stats `k`, cycle records `k x ncycles`, log `k x steps` or nothing).
UNVERIFIED: never executed.
"""
function site_group_sweep_cycles!(g::Ptr{Cvoid}, k::Integer, temperatures::Matrix{Float64}, steps_per_cycle::Integer; seed::UInt64=UInt64(0),
                                  first_step::UInt64=UInt64(0), cycle0::Integer=0, log::Bool=false)
    ncycles = size(temperatures, 2)
    stats = Vector{SiteStats}(undef, k)
    records = Matrix{SiteCycleRecord}(undef, k, ncycles)
    steps = log ? Matrix{SiteRecord}(undef, k, ncycles * steps_per_cycle) : nothing
    GC.@preserve temperatures stats records steps begin
        params = Ref(SiteParams(seed, first_step, C_NULL))
        cycles = Ref(SiteCycles(Int64(ncycles), Int64(steps_per_cycle), Int64(cycle0), pointer(temperatures)))
        _check(ccall((:ceg_site_group_sweep_cycles, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     g, params, cycles, pointer(stats), pointer(records), log ? pointer(steps) : C_NULL))
    end
    stats, records, steps
end

"""
`ceg_site_group_sweep_grouped`: the main loop of `run_montecarlo!(::SiteHopping, simu; groupcycles, restartgroupcycle)`
(src/simulation.jl:917-982) for the `k` chains of `g`: every cycle of `steps_per_cycle` (`groupcycles * m`) hops is accepted or rejected
as one move, after a restart from a fresh random population if `restart`.  `temperatures` is `K x ncycles` in K.
-> (stats `k`, cycle records `k x ncycles`, log `k x steps` or nothing, grouped records `k x ncycles`).  UNVERIFIED: never executed.
"""
function site_group_sweep_grouped!(g::Ptr{Cvoid}, k::Integer, temperatures::Matrix{Float64}, steps_per_cycle::Integer; restart::Bool=false,
                                   seed::UInt64=UInt64(0), first_step::UInt64=UInt64(0), cycle0::Integer=0, log::Bool=false)
    ncycles = size(temperatures, 2)
    stats = Vector{SiteStats}(undef, k)
    records = Matrix{SiteCycleRecord}(undef, k, ncycles)
    grouped = Matrix{SiteGroupedRecord}(undef, k, ncycles)
    steps = log ? Matrix{SiteRecord}(undef, k, ncycles * steps_per_cycle) : nothing
    GC.@preserve temperatures stats records steps grouped begin
        params = Ref(SiteParams(seed, first_step, C_NULL))
        cycles = Ref(SiteCycles(Int64(ncycles), Int64(steps_per_cycle), Int64(cycle0), pointer(temperatures)))
        _check(ccall((:ceg_site_group_sweep_grouped, LIB[]), Cint,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     g, params, cycles, Int32(restart), pointer(stats), pointer(records), log ? pointer(steps) : C_NULL, pointer(grouped)))
    end
    stats, records, steps, grouped
end

"`ceg_site_group_baseline`: `baseline_energy(sh)` (src/sitehopping.jl:105-112) of every chain, in K.  UNVERIFIED: never executed."
function site_group_baseline(g::Ptr{Cvoid}, k::Integer)
    out = zeros(Float64, k)
    _check(ccall((:ceg_site_group_baseline, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), g, out))
    out
end

"`ceg_site_group_rebase`: every running energy becomes the baseline (the `idx_cycle == 0` step).  UNVERIFIED: never executed."
function site_group_rebase!(g::Ptr{Cvoid})
    _check(ccall((:ceg_site_group_rebase, LIB[]), Cint, (Ptr{Cvoid},), g))
    nothing
end

"`ceg_site_group_get_populations` -> `m x k`, 1-based.  UNVERIFIED: never executed."
function site_group_populations(g::Ptr{Cvoid}, m::Integer, k::Integer)
    pops = zeros(UInt16, m, k)
    GC.@preserve pops _check(ccall((:ceg_site_group_get_populations, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, pointer(pops)))
    pops .+ 0x0001
end

"`ceg_site_group_set_populations` (`m x k`, 1-based); rebases.  UNVERIFIED: never executed."
function site_group_set_populations!(g::Ptr{Cvoid}, populations::Matrix{UInt16})
    pops = UInt16.(populations .- 0x0001)
    GC.@preserve pops _check(ccall((:ceg_site_group_set_populations, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, pointer(pops)))
    nothing
end

"`ceg_site_group_set_recorder`; `every === nothing` removes it.  UNVERIFIED: never executed."
function site_group_set_recorder!(g::Ptr{Cvoid}, every::Union{Nothing,Integer}; origin::Integer=0, capacity::Integer=1024, track_min::Bool=false)
    if every === nothing
        _check(ccall((:ceg_site_group_set_recorder, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, C_NULL))
        return nothing
    end
    spec = Ref(SiteRecorder(Int64(every), Int64(origin), Int64(capacity), Int32(track_min), Int32(0)))
    _check(ccall((:ceg_site_group_set_recorder, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, spec))
    nothing
end

"`ceg_site_group_recorder_read` -> (records `k x frames`, populations `m x k x frames`, 1-based).  UNVERIFIED: never executed."
function site_group_recorder_read(g::Ptr{Cvoid}, m::Integer, k::Integer)
    n = Ref{Int64}(0)
    _check(ccall((:ceg_site_group_recorder_read, LIB[]), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}),
                 g, Int64(0), Int64(0), C_NULL, C_NULL, n))
    records = Matrix{SiteFrameRecord}(undef, k, n[])
    pops = zeros(UInt16, m, k, n[])
    GC.@preserve records pops begin
        _check(ccall((:ceg_site_group_recorder_read, LIB[]), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}),
                     g, Int64(0), n[], pointer(records), pointer(pops), n))
    end
    records, pops .+ 0x0001
end

"`ceg_site_group_recorder_min` -> (mink, mine (K), populations `m x k`, 1-based): `RMinimumEnergy` per chain.  UNVERIFIED: never executed."
function site_group_recorder_min(g::Ptr{Cvoid}, m::Integer, k::Integer)
    mink = zeros(Int64, k); mine = zeros(Float64, k); pops = zeros(UInt16, m, k)
    GC.@preserve pops begin
        _check(ccall((:ceg_site_group_recorder_min, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Cvoid}), g, mink, mine, pointer(pops)))
    end
    mink, mine, pops .+ 0x0001
end

struct SiteTempering                 # ceg_site_tempering_t (32 bytes)
    rungs::Int32
    _pad::Int32
    pair_cdf::Ptr{Float64}
    ladder_stream::Ptr{UInt32}
    _reserved::Int64
end

"""
`ceg_site_group_set_tempering`: the K chains become `K ÷ rungs` ladders whose neighbouring rungs exchange configurations per step
inside the sweep kernel, as `run_parallel_tempering` (src/simulation.jl:461-634) does; the rule is stated in include/ceg_hip.h.
`pair_cdf` defaults to the reference's schedule, the first element of `randsubseq(1:(Npt-1), p)`: `1 - q` with `q` multiplied by
`1 - p` once per pair.  The temperatures of later sweeps must rise strictly with the rung.  `rungs === nothing` removes it.
UNVERIFIED: never executed.
"""
function site_group_set_tempering!(g::Ptr{Cvoid}, rungs::Union{Nothing,Integer}; p::Float64=0.1, pair_cdf::Union{Nothing,Vector{Float64}}=nothing,
                                   ladder_stream::Union{Nothing,Vector{UInt32}}=nothing)
    if rungs === nothing
        _check(ccall((:ceg_site_group_set_tempering, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, C_NULL))
        return nothing
    end
    cdf = pair_cdf
    if cdf === nothing
        cdf = Vector{Float64}(undef, max(rungs - 1, 0))
        q = 1.0
        for j in 1:length(cdf)
            q = q * (1.0 - p)
            cdf[j] = 1.0 - q
        end
    end
    GC.@preserve cdf ladder_stream begin
        spec = Ref(SiteTempering(Int32(rungs), Int32(0), pointer(cdf), ladder_stream === nothing ? Ptr{UInt32}(C_NULL) : pointer(ladder_stream), Int64(0)))
        _check(ccall((:ceg_site_group_set_tempering, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g, spec))
    end
    nothing
end

"""
`ceg_site_group_tempering_read` -> (attempted `(rungs-1) x ladders`, accepted `(rungs-1) x ladders`, replica `k`: per rung, the
1-based rung on which the configuration now there sat when tempering was installed).  UNVERIFIED: never executed.
"""
function site_group_tempering_read(g::Ptr{Cvoid}, rungs::Integer, k::Integer)
    attempted = zeros(Int64, rungs - 1, k ÷ rungs); accepted = zeros(Int64, rungs - 1, k ÷ rungs); replica = zeros(Int32, k)
    _check(ccall((:ceg_site_group_tempering_read, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}), g, attempted, accepted, replica))
    attempted, accepted, replica .+ Int32(1)
end

"""
`baseline_energy(mc)` (src/montecarlo.jl:530-542) from the device state behind `h` (`mc_handle(mc, ...)`): the sums come from
`ceg_mc_baseline`, the two constants of the Ewald context (`energy_net_charges`, `static_contribution`, src/ewald.jl:555-577) and
the tail correction from `mc`, whose species counts must be those of the device state.
"""
function baseline_energy(h::Ptr{Cvoid}, mc::CEG.MonteCarloSetup; refresh::Bool=false)
    b = mc_baseline(h; refresh)
    ctx = mc.ewald.ctx
    reciprocal = CEG.isdefined_ewald(ctx) ? 2*(b.recip_framework*u"K" + ctx.energy_net_charges) + b.recip_guests*u"K" + ctx.static_contribution[] : 0.0u"K"
    CEG.BaselineEnergyReport(b.framework_vdw*u"K", b.framework_direct*u"K", b.inter*u"K", reciprocal, mc.tailcorrection[])
end

"`ceg_mc_group_destroy`: the chains get their own streams back and stay valid"
function mc_group_close(g::Ptr{Cvoid})
    delete!(SAMPLERS, g)                 # (the sampler dies with the group: a later group at this address starts without one)
    _check(ccall((:ceg_mc_group_destroy, LIB[]), Cint, (Ptr{Cvoid},), g))
    nothing
end

"(bins per axis, capacity) of the guest neighbour cells (the CellListMap branch of src/energy.jl:399-404), or `nothing` when the MC cell is small enough for the exhaustive loop"
function mc_neighbour_cells(h::Ptr{Cvoid})
    nb = zeros(Int32, 3)
    cap = Ref{Int32}(0)
    rc = ccall((:ceg_mc_neighbour_cells, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ref{Int32}), h, nb, cap)
    rc < 0 && _check(rc)
    rc == 1 ? (Tuple(Int.(nb)), Int(cap[])) : nothing
end


# ------------------------------------------------------------------ blocking masks (SURVEY 8f row f4)
_to_bitarray(mask::Vector{UInt8}, a, b, c) = BitArray(permutedims(reshape(mask, c, b, a), (3, 2, 1)) .!= 0)

"BlockFile(g::EnergyGrid) (src/grids.jl:188-204) with the cell scan on the GPU"
function blockfile(g::CEG.EnergyGrid; device=0)
    a, b, c = g.csetup.dims .+ 1
    value = Array{Cfloat}(@view g.grid[:, :, :, 1])                 # [z, y, x] column-major = C order [x][y][z]
    mask = Vector{UInt8}(undef, a*b*c)
    dims = Int32[g.csetup.dims...]
    GC.@preserve value mask dims _check(ccall((:ceg_block_from_grid, LIB[]), Cint,
        (Int32, Ptr{Cfloat}, Int32, Ptr{Int32}, Float64, Ptr{UInt8}), device, value, 0, dims, 5e6, mask))
    CEG.BlockFile(g.csetup, _to_bitarray(mask, a, b, c))
end

"The scan of parse_blockfile (src/coordinates.jl:139-152): `protoblocks` as built at :123-133"
function block_spheres(csetup::GridCoordinatesSetup, centers::Vector{SVector{3,Float64}}, radius2::Vector{Float64}; device=0)
    a, b, c = csetup.dims .+ 1
    mat = NoUnits.(csetup.cell.mat ./ u"Å"); invmat = NoUnits.(csetup.cell.invmat .* u"Å")
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(mat)
    dims, _, shift, Δ = _geometry(csetup)
    cs = Float64[x for p in centers for x in p]
    m = Vector{Float64}(vec(mat)); im = Vector{Float64}(vec(invmat))
    mask = Vector{UInt8}(undef, a*b*c)
    GC.@preserve dims Δ shift m im cs radius2 mask _check(ccall((:ceg_block_spheres, LIB[]), Cint,
        (Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{UInt8}),
        device, dims, Δ, shift, m, im, ortho, safemin^2, cs, radius2, length(radius2), mask))
    CEG.BlockFile(csetup, _to_bitarray(mask, a, b, c))
end

# ------------------------------------------------------------------ energy_grid for polyatomic guests (ceg_energy_grid, ceg_energy_grid_reduced)
"""
    energy_grid_rotations(setup, vdw, coulomb, recip, rots, numABC, stepABC) -> Array{Float64,4}

`allvals[k, iA, iB, iC]` of energy_grid (src/grids.jl:391-419) from ONE device pass: `vdw` = interpolation handle of each grid of
`setup.grids` (C_NULL for a zero grid), `coulomb` / `recip` = handles of the Coulomb grid and of `setup.ewald` (both C_NULL when the
framework carries no charges), `rots` the rotation matrices (any source: `get_rotation_matrices`), `stepABC` the three step vectors (Å).
The array is the buffer the library filled: its element order is Julia's.
"""
function energy_grid_rotations(setup::CEG.CrystalEnergySetup, vdw::Vector{Ptr{Cvoid}}, coulomb::Ptr{Cvoid}, recip::Ptr{Cvoid},
                               rots, numABC::NTuple{3,Int}, stepABC)
    a = _egrid_inputs(setup, vdw, coulomb, rots, numABC, stepABC)
    out = Array{Float64,4}(undef, length(rots), numABC[1], numABC[2], numABC[3])             # grids.jl:391
    GC.@preserve a out _check(ccall((:ceg_energy_grid, LIB[]), Cint,
        (Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Int32},
         Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Int32, Ptr{Cvoid}),
        a.handles, coulomb, recip, a.base, a.charges, a.natoms, a.rotv, length(rots), a.steps, a.num,
        a.pmask, a.bdims, a.bsize, a.bshift, a.bmat, a.binv, a.enc, a.static, out, 0, C_NULL))
    out
end

# what ceg_energy_grid and ceg_energy_grid_reduced share: every argument up to static_contribution, as flat arrays
function _egrid_inputs(setup::CEG.CrystalEnergySetup, vdw::Vector{Ptr{Cvoid}}, coulomb::Ptr{Cvoid}, rots, numABC::NTuple{3,Int}, stepABC)
    molecule = setup.molecule
    base = Float64[NoUnits(x/u"Å") for p in position(molecule) for x in p]                   # grids.jl:356
    natoms = length(setup.atomsidx)
    handles = Ptr{Cvoid}[vdw[setup.atomsidx[i]] for i in 1:natoms]                             # grids.jl:316
    rotv = Float64[x for r in rots for x in r]                                               # SMatrix iterates column-major
    steps = Float64[x for s in stepABC for x in s]
    num = Int32[numABC...]
    enc = 0.0; static = 0.0
    if coulomb != C_NULL
        ctx = CEG.EwaldContext(setup.ewald, ((molecule,),))                                  # grids.jl:365
        enc = NoUnits(ctx.energy_net_charges/u"K"); static = NoUnits(ctx.static_contribution[]/u"K")
    end
    blk = setup.block
    cs = blk.csetup
    mask = blk.empty ? UInt8[] : vec(UInt8.(permutedims(blk.block, (3, 2, 1))))              # [x][y][z], z fastest
    bdims, bsize, bshift, _ = _geometry(cs)
    bmat = Vector{Float64}(vec(NoUnits.(cs.cell.mat ./ u"Å"))); binv = Vector{Float64}(vec(NoUnits.(cs.cell.invmat .* u"Å")))
    pmask = blk.empty ? Ptr{UInt8}(C_NULL) : pointer(mask)                                   # `mask` stays referenced by the tuple
    (; handles, base, charges=setup.charges, natoms, rotv, steps, num, mask, pmask, bdims, bsize, bshift, bmat, binv, enc, static)
end

"""
    energy_grid_reduced(setup, vdw, coulomb, recip, rots, numABC, stepABC, temperatures; weights=nothing, want_argmin=false)

The rotation axis of `energy_grid_rotations` collapsed on the device (`ceg_energy_grid_reduced`): `(mean, min, argmin)` with
`mean[iA, iB, iC, t]` = `meanBoltzmann(allvals, temperatures[t], weights)[iA, iB, iC]` (src/utils.jl:415-443), `min` the minimum over
the orientations and `argmin` (1-based, `nothing` unless asked for) the first orientation that attains it.
"""
function energy_grid_reduced(setup::CEG.CrystalEnergySetup, vdw::Vector{Ptr{Cvoid}}, coulomb::Ptr{Cvoid}, recip::Ptr{Cvoid},
                             rots, numABC::NTuple{3,Int}, stepABC, temperatures; weights=nothing, want_argmin::Bool=false)
    a = _egrid_inputs(setup, vdw, coulomb, rots, numABC, stepABC)
    temps = Float64[T isa Unitful.Quantity ? ustrip(u"K", T) : T for T in temperatures]        # meanBoltzmann takes plain kelvins
    w = weights isa Nothing ? Float64[] : Vector{Float64}(weights)
    weights isa Nothing || length(w) == length(rots) || error("one weight per rotation")
    mean = Array{Float64,4}(undef, numABC[1], numABC[2], numABC[3], length(temps))
    mn = Array{Float64,3}(undef, numABC...)
    amin = Array{Int32,3}(undef, (want_argmin ? numABC : (0, 0, 0))...)
    GC.@preserve a temps w mean mn amin _check(ccall((:ceg_energy_grid_reduced, LIB[]), Cint,
        (Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Int32},
         Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64,
         Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Cvoid}),
        a.handles, coulomb, recip, a.base, a.charges, a.natoms, a.rotv, length(rots), a.steps, a.num,
        a.pmask, a.bdims, a.bsize, a.bshift, a.bmat, a.binv, a.enc, a.static,
        (isempty(temps) ? Ptr{Float64}(C_NULL) : pointer(temps)), length(temps), (weights isa Nothing ? Ptr{Float64}(C_NULL) : pointer(w)),
        (isempty(temps) ? Ptr{Float64}(C_NULL) : pointer(mean)), mn, (want_argmin ? pointer(amin) : Ptr{Int32}(C_NULL)), 0, C_NULL))
    (mean, mn, want_argmin ? amin .+ Int32(1) : nothing)
end

# lattice (grids.jl:378-384), rotations with their Lebedev weights (:385-390) and device handles of a setup; f(vdw, coulomb, recip, rots,
# weights, numABC, stepABC) runs with the handles alive
function _with_egrid_setup(f, setup::CEG.CrystalEnergySetup, step, num_rotate)
    molecule = setup.molecule
    axeA, axeB, axeC = CEG.bounding_box(setup.framework)
    numA = floor(Int, norm(axeA) / step) + 1
    numB = floor(Int, norm(axeB) / step) + 1
    numC = floor(Int, norm(axeC) / step) + 1
    stepABC = (NoUnits.(axeA ./ numA ./ u"Å"), NoUnits.(axeB ./ numB ./ u"Å"), NoUnits.(axeC ./ numC ./ u"Å"))
    rots, weights = if num_rotate == 0 || length(molecule) == 1
        [one(SMatrix{3,3,Float64,9})], [1.0]
    else
        CEG.get_rotation_matrices(molecule, num_rotate)
    end
    vdw = Ptr{Cvoid}[g.ewald_precision == Inf ? interp_handle(g) : C_NULL for g in setup.grids]
    withcoulomb = setup.coulomb.ewald_precision != -Inf
    coulomb = withcoulomb ? interp_handle(setup.coulomb) : C_NULL
    recip = withcoulomb ? recip_handle(setup.ewald) : C_NULL
    try
        return f(vdw, coulomb, recip, rots, weights, (numA, numB, numC), stepABC)
    finally
        for h in vdw
            h == C_NULL || ccall((:ceg_interp_destroy, LIB[]), Cint, (Ptr{Cvoid},), h)
        end
        withcoulomb && ccall((:ceg_interp_destroy, LIB[]), Cint, (Ptr{Cvoid},), coulomb)
        withcoulomb && ccall((:ceg_recip_destroy, LIB[]), Cint, (Ptr{Cvoid},), recip)
    end
end

"""
    energy_grid(setup::CrystalEnergySetup, step, num_rotate=40)

The reference's energy_grid (src/grids.jl:346-424) with the loop nest :394-419 on the GPU; lattice (:378-384) and rotations (:385-390,
`get_rotation_matrices`) are the reference's own.  Not covered: `num_rotate < 0` (random offsets, :404-406), the scratchspace cache
(:349-354) and a `MonteCarloSetup` -- for those call `CrystalEnergyGrids.energy_grid`.
"""
function energy_grid(setup::CEG.CrystalEnergySetup, step, num_rotate=40)
    num_rotate < 0 && return CEG.energy_grid(setup, step, num_rotate)
    _with_egrid_setup(setup, step, num_rotate) do vdw, coulomb, recip, rots, _weights, numABC, stepABC
        energy_grid_rotations(setup, vdw, coulomb, recip, rots, numABC, stepABC)
    end
end

"""
    energy_grid_reduced(setup::CrystalEnergySetup, step, temperatures; num_rotate=40, weights=nothing, want_argmin=false)

`(mean, min, argmin)` of `energy_grid(setup, step, num_rotate)` over its rotation axis without the 4-D array ever reaching the host:
`mean[:, :, :, t] == meanBoltzmann(energy_grid(setup, step, num_rotate), temperatures[t], weights)` to rounding.  `weights`: `nothing`
(what `output_cube` and `compute_levels` use), `:lebedev` (the weights `get_rotation_matrices` returns next to the matrices) or one
number per rotation.  Lattice and rotations are the reference's own, as for `energy_grid`; `num_rotate < 0` is not covered.
"""
function energy_grid_reduced(setup::CEG.CrystalEnergySetup, step, temperatures; num_rotate=40, weights=nothing, want_argmin::Bool=false)
    num_rotate < 0 && error("num_rotate < 0 (random offsets) is not covered: reduce CrystalEnergyGrids.energy_grid with meanBoltzmann")
    _with_egrid_setup(setup, step, num_rotate) do vdw, coulomb, recip, rots, lebedev, numABC, stepABC
        w = weights === :lebedev ? lebedev : weights
        energy_grid_reduced(setup, vdw, coulomb, recip, rots, numABC, stepABC, temperatures; weights=w, want_argmin=want_argmin)
    end
end

"""
    mean_boltzmann_grid(setup, step, T; num_rotate=40) -> Array{Float64,3}

What `meanBoltzmann(energy_grid(setup, step, num_rotate), T)` returns (the grid `output_cube` writes), reduced on the device.
"""
function mean_boltzmann_grid(setup::CEG.CrystalEnergySetup, step, T; num_rotate=40)
    mean, _, _ = energy_grid_reduced(setup, step, (T,); num_rotate=num_rotate)
    mean[:, :, :, 1]
end

# ------------------------------------------------------------------ build + file in one call (row f4)
"create_grid_vdw with the .grid file written by the library while the grid is built (ceg_grid_vdw_file)"
function create_grid_vdw_streamed(file, framework::AbstractSystem{3}, forcefield::ForceField, spacing::TÅ, atom::Symbol)
    cset, num_unitcell = CEG._setup_grid_common(framework, spacing, forcefield.cutoff)
    grid = Array{Cfloat,4}(undef, cset.dims[3]+1, cset.dims[2]+1, cset.dims[1]+1, 8)
    probe = ProbeSystem(framework, forcefield, atom)
    ff = probe.forcefield
    check_rules(ff, probe.probe, probe.atomkinds)
    rules, offsets = rule_table(ff, probe.probe)
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(probe.mat)
    λ = inv(GRID_TO_KELVIN); thr = GRID_TO_KELVIN*1e7                       # grids.jl:141-143,148 (GRID_TO_KELVIN is a plain Float64, constants.jl:20)
    io = IOBuffer(); CEG._create_grid_common(io, cset, num_unitcell); header = take!(io)   # grids.jl:108-116
    trailer = reinterpret(UInt8, Vector{Float64}(vec(NoUnits.(cset.cell.mat ./ u"Å")))) |> collect   # :154
    dims, size, shift, Δ = _geometry(cset)
    pos = _flatpos(probe); kinds = Int64.(probe.atomkinds)
    mat = Vector{Float64}(vec(probe.mat)); invmat = Vector{Float64}(vec(probe.invmat))
    GC.@preserve grid pos kinds mat invmat rules offsets dims size shift Δ header trailer begin
        _check(ccall((:ceg_grid_vdw_file, LIB[]), Cint,
            (Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Float64,
             Ptr{CegRule}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Float64, Float64, Ptr{Cfloat}, Int32, Cstring, Ptr{UInt8}, Int64, Ptr{UInt8}, Int64),
            pos, kinds, length(kinds), mat, invmat, ortho, safemin^2, NoUnits(ff.cutoff^2/u"Å^2"),
            rules, offsets, length(offsets)-1, dims, size, shift, Δ, λ, thr, grid, ngpus(),
            String(file), header, length(header), trailer, length(trailer)))
    end
    grid
end

# ------------------------------------------------------------------ grid analysis (src/basins.jl)
# 1-based at this boundary; the library is 0-based.  A grid is an Array{T,3} (host) or a `Ptr{Cvoid}` to device memory in the same
# memory order together with its `dims`.  UNVERIFIED: never executed.
_dims32(dims) = Int32[dims...]

"""
    local_minima(grid::Array{Float64,3}, tolerance=1e-2; lt=(<), device=0) -> Vector{CartesianIndex{3}}

`CrystalEnergyGrids.local_minima` (src/basins.jl:40-99) with the scan on the device (`ceg_grid_local_minima`), sorted.  `lt` is `<`
or `>`.  The reference's `@assert min_energy < 0` arrives as an error of the library; a grid without any local extremum gives an
empty list where the reference throws.
"""
function local_minima(grid::Array{Float64,3}, tolerance=1e-2; lt=(<), device=0)
    lt === (<) || lt === (>) || error("lt must be < or >")
    _local_minima(grid, 0, size(grid), tolerance, lt === (>), device)
end
"the same for a grid in device memory (e.g. a `min` lattice of `ceg_energy_grid_reduced`)"
local_minima(d_grid::Ptr{Cvoid}, dims::NTuple{3,Int}, tolerance=1e-2; lt=(<), device=0) =
    _local_minima(d_grid, 1, dims, tolerance, lt === (>), device)

function _local_minima(grid, on_device::Int, dims, tolerance, maxima::Bool, device)
    d = _dims32(dims)
    count = Int64[0]; ext = Float64[0.0]
    cap = 4096
    while true
        ijk = Matrix{Int32}(undef, 3, max(cap, 1))
        GC.@preserve grid d ijk count ext _check(ccall((:ceg_grid_local_minima, LIB[]), Cint,
            (Int32, Ptr{Cvoid}, Int32, Ptr{Int32}, Int32, Float64, Ptr{Int32}, Int32, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Cvoid}),
            device, grid, on_device, d, maxima ? 1 : 0, Float64(tolerance), ijk, 0, cap, count, ext, C_NULL))
        count[1] <= cap && return [CartesianIndex(Int(ijk[1, n]) + 1, Int(ijk[2, n]) + 1, Int(ijk[3, n]) + 1) for n in 1:count[1]]
        cap = Int(count[1])
    end
end

"""
    grid_components(grid::Array{T,3}; band=nothing, device=0) -> (labels, seeds, sizes, sums)

The periodic 6-connected components of the non-zero points of `grid` (`T` = Int64 or Float64: `local_components`, src/basins.jl:279-313)
or, with `band = (mine, maxe)`, of the points with `mine < value < maxe` of a Float64 lattice (`compute_levels`, :842-869; strict on
both sides).  `labels[i,j,k]` is 0 for an inactive point, else the 1-based rank of its component in the order in which the reference's
scan finds them; `seeds` are `CartesianIndex`es (the first point of each component in that scan), `sums` the exact Int64 sums (empty
for Float64).  The unwrapped coordinates of the reference's lists, Float64 sums and the atol / rtol / ntol cut are not covered.
"""
function grid_components(grid::Array{T,3}; band=nothing, device=0) where {T<:Union{Int64,Float64}}
    a, b, c = size(grid)
    d = _dims32(size(grid))
    isint = T === Int64
    mode = band === nothing ? 0 : 1
    lo, hi = band === nothing ? (0.0, 0.0) : Float64.(band)
    labels = Array{Int32,3}(undef, a, b, c)
    count = Int64[0]
    cap = 4096
    while true
        seed = zeros(Int32, max(cap, 1)); sz = zeros(Int32, max(cap, 1)); sm = zeros(Int64, max(cap, 1))
        GC.@preserve grid d labels seed sz sm count _check(ccall((:ceg_grid_components, LIB[]), Cint,
            (Int32, Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Int32, Float64, Float64, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64},
             Int32, Int64, Ptr{Int64}, Ptr{Cvoid}),
            device, grid, isint ? 1 : 0, 0, d, mode, lo, hi, labels, 0, seed, sz, isint ? pointer(sm) : Ptr{Int64}(C_NULL), 0, cap, count, C_NULL))
        if count[1] <= cap
            n = Int(count[1])
            seeds = [CartesianIndex(Int(s % a) + 1, Int((s ÷ a) % b) + 1, Int(s ÷ (a*b)) + 1) for s in seed[1:n]]
            return labels .+ Int32(1), seeds, Int.(sz[1:n]), isint ? sm[1:n] : Int64[]
        end
        cap = Int(count[1])
    end
end

"""
    site_proximity_map(sites, dims, mat, maxdist=2.0; device=0) -> (map, deleted)

`site_proximity_map!` (src/basins.jl:466-578): `map[i,j,k] == (s, ofs)` as the reference returns it.  `sites` (fractional) is NOT
mutated: the indices the reference would delete (sites that snap to the voxel of an earlier one, :471-484) are returned, and `s`
indexes the kept ones.  `mat` in Å, unitless.  Refused when a ball of `maxdist` plus the skin would meet its own periodic image.
"""
function site_proximity_map(sites::AbstractVector, dims::NTuple{3,Int}, mat::AbstractMatrix, maxdist=2.0; device=0)
    a, b, c = dims
    known = Set{NTuple{3,Int}}(); deleted = Int[]
    for (idx, (i, j, k)) in enumerate(sites)
        ijk = (1 + round(Int, a*i), 1 + round(Int, b*j), 1 + round(Int, c*k))
        ijk in known ? push!(deleted, idx) : push!(known, ijk)
    end
    kept = [Float64(x) for (idx, s) in enumerate(sites) if !(idx in deleted) for x in s]
    m = Vector{Float64}(vec(Matrix{Float64}(mat)))
    d = _dims32(dims)
    site = Array{Int32,3}(undef, a, b, c)
    ofs = Array{Int8,4}(undef, 3, a, b, c)
    GC.@preserve d m kept site ofs _check(ccall((:ceg_grid_site_proximity, LIB[]), Cint,
        (Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Ptr{Int32}, Ptr{Cvoid}, Int32, Ptr{Cvoid}),
        device, d, m, kept, length(kept) ÷ 3, Float64(maxdist), site, ofs, 0, C_NULL))
    [(site[i, j, k], SVector{3,Int8}(ofs[1, i, j, k], ofs[2, i, j, k], ofs[3, i, j, k])) for i in 1:a, j in 1:b, k in 1:c], deleted
end

"""
    site_density(bins::Array{Int64,3}, proximity, numsites; device=0) -> Vector{Tuple{Float64,SVector{3,Float64}}}

`closest_from_proximity(bins, proximity, numsites)` (src/basins.jl:580-597) for the Int64 bins of a density map: the sums are exact
integers on the device, `pos` is one division of them.  `first.(site_density(...))` is `proximal_map`.
"""
function site_density(bins::Array{Int64,3}, proximity::Array{<:Tuple,3}, numsites::Int; device=0)
    a, b, c = size(bins)
    size(proximity) == (a, b, c) || error("the proximity map and the bins differ in size")
    site = Int32[p[1] for p in proximity]
    ofs = Array{Int8,4}(undef, 3, a, b, c)
    for k in 1:c, j in 1:b, i in 1:a, q in 1:3
        ofs[q, i, j, k] = proximity[i, j, k][2][q]
    end
    d = _dims32((a, b, c))
    rho = zeros(Int64, numsites + 1); mom = zeros(Int64, 3, numsites + 1)
    GC.@preserve bins site ofs d rho mom _check(ccall((:ceg_grid_site_density, LIB[]), Cint,
        (Int32, Ptr{Int64}, Int32, Ptr{Int32}, Ptr{Cvoid}, Int32, Ptr{Int32}, Int32, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Cvoid}),
        device, bins, 0, site, ofs, 0, d, numsites, rho, mom, 0, C_NULL))
    [(Float64(rho[s]), SVector{3,Float64}(mom[1, s] / (a*rho[s]), mom[2, s] / (b*rho[s]), mom[3, s] / (c*rho[s]))) for s in 1:numsites+1]
end

# circular_distance (src/basins.jl:108-113) as written: the wrapped distance only when min < a ÷ 2 < max
function _circular_distance(a::Int, m::Int, n::Int)
    b = a ÷ 2
    i, j = minmax(m, n)
    i < b < j && return min(j - i, i - j + a)
    j - i
end

"""
    local_basins(grid::Array{Float64,3}, minima::Vector{CartesianIndex{3}}; lt=(<), cluster=0, skip_above=Inf, maxdist=0, device=0)
    local_basins(grid::Array{Float64,3}, tolerance::Float64=-Inf; kwargs...)

`CrystalEnergyGrids.local_basins` (src/basins.jl:195-264) with one levelled pass for all minima on the device (`ceg_grid_basins`).
Returns `Vector{Set{NTuple{3,Int}}}`, 1-based.  Differences from the reference: `skip` is `v -> v > skip_above`; the sets hold WRAPPED
coordinates, where the reference's hold whichever periodic image its queue met first; and the result follows the definition of the
reference's docstring, where the reference as written skips the last level of a basin when that level holds exactly one point
(:153).  `cluster` is `clean_cluster!` (:116-138) over the kept minima.  More than 16 basins at one point is an error of the library.
"""
function local_basins(grid::Array{Float64,3}, minima::Vector{CartesianIndex{3}}; lt=(<), cluster=0, skip_above=Inf, maxdist=0, device=0)
    lt === (<) || lt === (>) || error("lt must be < or >")
    a, b, c = size(grid)
    n = length(minima)
    d = _dims32(size(grid))
    starts = Matrix{Int32}(undef, 3, max(n, 1))
    for (s, m) in enumerate(minima), q in 1:3
        starts[q, s] = m[q] - 1
    end
    owner = Array{Int32,3}(undef, a, b, c); nown = Array{UInt8,3}(undef, a, b, c)
    sz = zeros(Int32, max(n, 1)); count = Int64[0]
    cap = a*b*c ÷ 2 + 4096
    shared = Matrix{Int32}(undef, 2, cap)
    while true
        GC.@preserve grid d starts owner nown shared count sz _check(ccall((:ceg_grid_basins, LIB[]), Cint,
            (Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Int32, Int64, Int32, Float64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}, Int32,
             Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}, Int32, Ptr{Cvoid}),
            device, grid, 0, d, starts, 0, n, lt === (>) ? 1 : 0, Float64(skip_above), Int64(maxdist), Ptr{Int32}(C_NULL), owner, nown, 0,
            shared, cap, count, sz, 0, C_NULL))
        count[1] <= cap && break
        cap = Int(count[1])
        shared = Matrix{Int32}(undef, 2, cap)
    end
    sets = [Set{NTuple{3,Int}}() for _ in 1:n]
    for k in 1:c, j in 1:b, i in 1:a
        nown[i, j, k] == 1 && push!(sets[owner[i, j, k] + 1], (i, j, k))
    end
    for p in 1:Int(count[1])
        lin = Int(shared[1, p])
        push!(sets[shared[2, p] + 1], (lin % a + 1, (lin ÷ a) % b + 1, lin ÷ (a*b) + 1))
    end
    kept = [s for s in 1:n if sz[s] > 0]
    sets = sets[kept]
    if cluster > 0
        km = minima[kept]
        unions = collect(1:length(km))
        for i1 in 1:length(km), i2 in (i1+1):length(km)
            if _circular_distance(a, km[i1][1], km[i2][1]) + _circular_distance(b, km[i1][2], km[i2][2]) +
               _circular_distance(c, km[i1][3], km[i2][3]) ≤ cluster
                unions[i2] = unions[i1]
            end
        end
        todelete = Int[]
        for i in 1:length(km)
            j = unions[i]
            i == j && continue
            union!(sets[j], sets[i])
            push!(todelete, i)
        end
        deleteat!(sets, todelete)
    end
    sets
end
local_basins(grid::Array{Float64,3}, tolerance::Float64=-Inf; lt=(<), device=0, kwargs...) =
    local_basins(grid, local_minima(grid, tolerance; lt, device); lt, device, kwargs...)

"""
    decompose_basins(grid::Array{Float64,3}, basinsets::Vector{Set{NTuple{3,Int}}}) -> (points, nodes)
    decompose_basins(grid::Array{Float64,3}, tolerance::Float64=-Inf; kwargs...)

`CrystalEnergyGrids.decompose_basins` (src/basins.jl:765-797) on the sets of `local_basins` above: `points` sorted as :790 sorts them,
`nodes[i,j,k]` the ascending list of the basins the point belongs to.  Host work: the device pass is the one behind `local_basins`.
"""
function decompose_basins(grid::Array{Float64,3}, basinsets::Vector{Set{NTuple{3,Int}}})
    a, b, c = size(grid)
    nodes = [Int[] for _ in 1:a, _ in 1:b, _ in 1:c]
    pointsset = Set{NTuple{3,Int}}()
    for (iset, set) in enumerate(basinsets)
        union!(pointsset, set)
        for (i, j, k) in set
            push!(nodes[mod1(i, a), mod1(j, b), mod1(k, c)], iset)
        end
    end
    points = collect(pointsset)
    sort!(points; by = p -> (p[3], p[2], p[1]))
    points, nodes
end
decompose_basins(grid::Array{Float64,3}, tolerance::Float64=-Inf; kwargs...) = decompose_basins(grid, local_basins(grid, tolerance; kwargs...))

# ---- from a density map to the sites: ceg_grid_smooth / ceg_grid_ranked / ceg_grid_site_nearest / ceg_coalesce_ranked ----------
"""
    gaussian_taps(sigma) -> Vector{Float64}

The taps of one axis as `ceg_hip.basins.gaussian_taps` defines them: `[1.0]` for `sigma == 0`, else `w = 2ceil(sigma)`,
`exp(-x^2/(2sigma^2))` for `x = -w:w`, divided by their sum.  The definition is this package's.
"""
function gaussian_taps(sigma::Real)
    sigma == 0 && return [1.0]
    w = 2 * ceil(Int, sigma)
    g = [exp(-(x * x) / (2.0 * sigma * sigma)) for x in -w:w]
    g ./ sum(g)
end

"""
    smooth_grid(grid::Array{<:Union{Float64,Int64},3}, taps::NTuple{3,Vector{Float64}}; scale=1.0, device=0) -> Array{Float64,3}

`imfilter(grid, kernel, "circular")` (src/basins.jl:668) with the separable kernel given as three tap vectors of odd length (at most
129), on the device: `y[p] = sum_t taps[t+w] * x[mod(p+t, n)]`, `t` ascending, one fma per tap, along axis 1, 2, then 3.  Int64 bins are
multiplied by `scale` first (`1/counter`).
"""
function smooth_grid(grid::Array{T,3}, taps::NTuple{3,Vector{Float64}}; scale::Float64=1.0, device=0) where {T<:Union{Int64,Float64}}
    d = _dims32(size(grid))
    out = Array{Float64,3}(undef, size(grid))
    t1, t2, t3 = taps
    GC.@preserve grid d t1 t2 t3 out _check(ccall((:ceg_grid_smooth, LIB[]), Cint,
        (Int32, Ptr{Cvoid}, Int32, Int32, Float64, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Cvoid}),
        device, grid, T === Int64 ? 1 : 0, 0, scale, d, t1, length(t1), t2, length(t2), t3, length(t3), out, 0, C_NULL))
    out
end

"""
    ranked_above(grid::Array{Float64,3}, crop; device=0) -> (idx::Vector{Int}, values::Vector{Float64})

`sortperm(vec(grid), rev=true)` cut where the value is `<= crop` (src/basins.jl:670, 679): 1-based linear indices by decreasing value,
equal values by increasing index.  A NaN is dropped; `crop >= 0`.
"""
function ranked_above(grid::Array{Float64,3}, crop::Real; device=0)
    d = _dims32(size(grid))
    cap = length(grid)
    idx = Vector{Int32}(undef, max(cap, 1)); val = Vector{Float64}(undef, max(cap, 1))
    count = Int64[0]
    GC.@preserve grid d idx val count _check(ccall((:ceg_grid_ranked, LIB[]), Cint,
        (Int32, Ptr{Float64}, Int32, Ptr{Int32}, Float64, Ptr{Int32}, Ptr{Float64}, Int32, Int64, Ptr{Int64}, Ptr{Cvoid}),
        device, grid, 0, d, Float64(crop), idx, val, 0, cap, count, C_NULL))
    n = Int(count[1])
    Int.(idx[1:n]) .+ 1, val[1:n]
end

"""
    site_nearest(sites, dims, mat; bins=nothing, origin=1, device=0) -> (points, site, ofs, dist)

Phase 2 of `closest_to_sites` (src/basins.jl:400-422) for every voxel with a non-zero bin (every voxel without `bins`): the site at
the smallest `periodic_distance_with_ofs!` of `site .- (ijk .- 1 .+ origin) ./ dims`, the lowest index among equals, and its cell
offset.  `origin = 1` is the reference as written, `origin = 0` the convention of `site_proximity_map!`.  `points`: 1-based linear
indices in increasing order; `site`: 1-based.
"""
function site_nearest(sites::AbstractVector, dims::NTuple{3,Int}, mat::AbstractMatrix; bins::Union{Nothing,Array{Int64,3}}=nothing,
                      origin::Integer=1, device=0)
    m = Vector{Float64}(vec(Matrix{Float64}(mat)))
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(mat)
    flat = [Float64(x) for s in sites for x in s]
    d = _dims32(dims)
    cap = prod(dims)
    lin = Vector{Int32}(undef, cap); site = Vector{Int32}(undef, cap); ofs = Matrix{Int8}(undef, 3, cap); dist = Vector{Float64}(undef, cap)
    count = Int64[0]
    bptr = bins === nothing ? Ptr{Int64}(C_NULL) : pointer(bins)
    GC.@preserve bins d m flat lin site ofs dist count _check(ccall((:ceg_grid_site_nearest, LIB[]), Cint,
        (Int32, Ptr{Int32}, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Int32, Int32, Ptr{Int64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Cvoid},
         Ptr{Float64}, Int32, Int64, Ptr{Int64}, Ptr{Cvoid}),
        device, d, m, ortho ? 1 : 0, Float64(ustrip(safemin)), flat, length(flat) ÷ 3, origin, bptr, 0, lin, site, ofs, dist, 0, cap, count, C_NULL))
    n = Int(count[1])
    Int.(lin[1:n]) .+ 1, Int.(site[1:n]) .+ 1, [SVector{3,Int}(ofs[1, q], ofs[2, q], ofs[3, q]) for q in 1:n], dist[1:n]
end

"""
    coalesce_ranked(idx, smoothed, values, dims, mat, maxdist; atol=0.1, maxbasins=Inf) -> Vector{Tuple{Float64,SVector{3,Float64}}}

The greedy pass of `coalescing_basins` (src/basins.jl:677-719) in the library's host code: `idx` the 1-based ranking of `ranked_above`,
`smoothed` and `values` the smoothed and the unsmoothed grid at those indices.  The same IEEE operations in the same order as the
reference's loop.
"""
function coalesce_ranked(idx::Vector{Int}, smoothed::Vector{Float64}, values::Vector{Float64}, dims::NTuple{3,Int}, mat::AbstractMatrix,
                         maxdist::Real; atol::Real=0.1, maxbasins::Real=Inf)
    m = Vector{Float64}(vec(Matrix{Float64}(mat)))
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(mat)
    lin = Int32.(idx .- 1)
    d = _dims32(dims)
    cap = max(length(lin), 1)
    val = Vector{Float64}(undef, cap); cen = Matrix{Float64}(undef, 3, cap)
    count = Int64[0]
    GC.@preserve lin smoothed values d m val cen count _check(ccall((:ceg_coalesce_ranked, LIB[]), Cint,
        (Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int32}, Ptr{Float64}, Int32, Float64, Float64, Float64, Float64, Ptr{Float64},
         Ptr{Float64}, Int64, Ptr{Int64}),
        lin, smoothed, values, length(lin), d, m, ortho ? 1 : 0, Float64(ustrip(safemin)), Float64(maxdist), Float64(atol), Float64(maxbasins),
        val, cen, cap, count))
    [(val[q], SVector{3,Float64}(cen[1, q], cen[2, q], cen[3, q])) for q in 1:Int(count[1])]
end

"""
    grid_coalesce(idx, smoothed, grid, mat, maxdist; scale=1.0, atol=0.1, maxbasins=Inf, voxels_per_launch=0, device=0)
        -> Vector{Tuple{Float64,SVector{3,Float64}}}

The greedy pass of `coalescing_basins` (src/basins.jl:677-719) on the device, the bytes of `coalesce_ranked`: `idx` and `smoothed` the
1-based ranking of `ranked_above`, `grid` the unsmoothed map (`Float64`, or `Int64` bins times `scale`), whose values the kernel gathers
itself.  The loop runs in launches of at most `voxels_per_launch` voxels (0: the default); the result does not depend on the cut.
"""
function grid_coalesce(idx::Vector{Int}, smoothed::Vector{Float64}, grid::Array{T,3}, mat::AbstractMatrix, maxdist::Real;
                       scale::Float64=1.0, atol::Real=0.1, maxbasins::Real=Inf, voxels_per_launch::Integer=0,
                       device=0) where {T<:Union{Int64,Float64}}
    m = Vector{Float64}(vec(Matrix{Float64}(mat)))
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(mat)
    lin = Int32.(idx .- 1)
    d = _dims32(size(grid))
    cap = max(length(lin), 1)
    val = Vector{Float64}(undef, cap); cen = Matrix{Float64}(undef, 3, cap)
    count = Int64[0]
    GC.@preserve lin smoothed grid d m val cen count _check(ccall((:ceg_grid_coalesce, LIB[]), Cint,
        (Int32, Ptr{Int32}, Ptr{Float64}, Int32, Int64, Ptr{Cvoid}, Int32, Int32, Float64, Ptr{Int32}, Ptr{Float64}, Int32, Float64, Float64,
         Float64, Float64, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Int64, Ptr{Int64}, Ptr{Cvoid}),
        device, lin, smoothed, 0, length(lin), grid, T === Int64 ? 1 : 0, 0, scale, d, m, ortho ? 1 : 0, Float64(ustrip(safemin)),
        Float64(maxdist), Float64(atol), Float64(maxbasins), voxels_per_launch, val, cen, 0, cap, count, C_NULL))
    [(val[q], SVector{3,Float64}(cen[1, q], cen[2, q], cen[3, q])) for q in 1:Int(count[1])]
end

"""
    site_partition(grid, sites, mat; scale=1.0, origin=0, device=0) -> (sums, centres, cap_bound, nactive)

Stages 2 and 3 of `closest_to_sites` (src/basins.jl:400-434) and the centres of `updated_sites_with_closest` (:454) in one device call,
for any number of sites: every non-zero voxel of `grid` (`Float64`, or `Int64` bins times `scale`) goes to its nearest site, and each
site adds its voxels up in linear-index order, skipping a voxel that would take its sum above 1 (`cap_bound`).  `centres[s]` is NaN for
a site without a voxel.
"""
function site_partition(grid::Array{T,3}, sites::AbstractVector, mat::AbstractMatrix; scale::Float64=1.0, origin::Integer=0,
                        device=0) where {T<:Union{Int64,Float64}}
    m = Vector{Float64}(vec(Matrix{Float64}(mat)))
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(mat)
    flat = [Float64(x) for s in sites for x in s]
    ns = length(flat) ÷ 3
    d = _dims32(size(grid))
    sums = Vector{Float64}(undef, ns); cen = Matrix{Float64}(undef, 3, ns)
    cap = Int32[0]; count = Int64[0]
    GC.@preserve grid d m flat sums cen cap count _check(ccall((:ceg_grid_site_partition, LIB[]), Cint,
        (Int32, Ptr{Cvoid}, Int32, Int32, Float64, Ptr{Int32}, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Int32, Int32, Ptr{Float64},
         Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Cvoid}),
        device, grid, T === Int64 ? 1 : 0, 0, scale, d, m, ortho ? 1 : 0, Float64(ustrip(safemin)), flat, ns, origin, sums, cen, 0, cap, count,
        C_NULL))
    sums, [SVector{3,Float64}(cen[1, q], cen[2, q], cen[3, q]) for q in 1:ns], cap[1] != 0, Int(count[1])
end

"""
    cluster_closer_than(ret, mat, maxdist) -> Vector{Tuple{Float64,SVector{3,Float64}}}

`cluster_closer_than!` (src/basins.jl:613-642) in the library's host code, line by line; returns the new list.
"""
function cluster_closer_than(ret::Vector{Tuple{Float64,SVector{3,Float64}}}, mat::AbstractMatrix, maxdist::Real)
    m = Vector{Float64}(vec(Matrix{Float64}(mat)))
    _, ortho, safemin = CEG.prepare_periodic_distance_computations(mat)
    n = length(ret)
    rho = Float64[r for (r, _) in ret]
    pos = Matrix{Float64}(undef, 3, max(n, 1))
    for (q, (_, p)) in enumerate(ret)
        pos[:, q] .= p
    end
    count = Int64[0]
    GC.@preserve rho pos m count _check(ccall((:ceg_cluster_closer_than, LIB[]), Cint,
        (Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Int32, Float64, Float64, Ptr{Int64}),
        rho, pos, n, m, ortho ? 1 : 0, Float64(ustrip(safemin)), Float64(maxdist), count))
    [(rho[q], SVector{3,Float64}(pos[1, q], pos[2, q], pos[3, q])) for q in 1:Int(count[1])]
end

end # module

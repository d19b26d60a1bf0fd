"""GPU: the grid operations of include/open/manta_hip_gridops.h on the device against the reference's recorded outputs
(tests/golden/gridops.npz) and the numpy model (tests/gridops_model.py), bit for bit; the three fp64 sums within the bound that
gridops_model's docstring derives (equal wherever no fp32 rounding boundary lies within it).  Outputs that a kernel overwrites, and the
pool scratch it takes, are filled with NaN beforehand."""
import numpy as np
import pytest

import gridops_model as M

pytestmark = pytest.mark.gpu

GOLDEN = np.load(M.GOLDEN)
f32, i32 = np.float32, np.int32
NAN_WORD = np.array([np.nan], f32).view(i32)[0]


def solver(m, dims):
    return m.Solver(name="s", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


def grid_from(s, cls, a):
    g = s.create(cls)
    g.from_numpy(a)
    return g


def cls_of(m, kind):
    return {"real": m.RealGrid, "int": m.IntGrid, "vec": m.VecGrid}[kind]


def nan_like(dims, kind):
    shp = M.shape_of(dims, 3 if kind == "vec" else 1)
    return np.full(shp, NAN_WORD, i32) if kind == "int" else np.full(shp, np.nan, f32)


def poison_pool(m, s, kind):
    """the next scratch grid of that kind the pool hands out is full of NaN"""
    g = grid_from(s, cls_of(m, kind), nan_like(s.mGridSize, kind))
    del g


def same(tag, got, want):
    assert M.same(got, want), "%s: %d of %d elements differ" % (tag, M.differing(np.asarray(got), np.asarray(want)), np.asarray(want).size)


# ---- permutation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("dims", M.PERMUTE_INPLACE, ids=M.name_of)
def test_permute_axes_in_place(hip_backend, dims, kind):
    import manta as m
    s = solver(m, dims)
    a = M.distinct(dims, kind)
    for ax in M.PERMUTATIONS:
        g = grid_from(s, cls_of(m, kind), a)
        poison_pool(m, s, kind)
        g.permuteAxes(*ax)
        want = M.permute(a, ax)
        same("permuteAxes%s" % (ax,), g.to_numpy(), want)
        key = "perm/in/%s/%d%d%d/%s" % ((M.name_of(dims),) + ax + (kind,))
        if key in GOLDEN.files:
            same(key, g.to_numpy(), GOLDEN[key])
        poison_pool(m, s, kind)
        g.permuteAxes(*M.inverse(ax))
        same("the inverse of %s restores the input" % (ax,), g.to_numpy(), a)
        live = s._live
        g.permuteAxes(0, 1, 1)                     # a repeated axis and an axis out of range: silently nothing
        g.permuteAxes(0, 1, 3)
        same("invalid axes", g.to_numpy(), a)
        assert s._live == live                     # the scratch went back to the pool


@pytest.mark.parametrize("case", list(M.permute_cases()), ids=lambda c: c[0])
def test_permute_fixture_cases(hip_backend, case):
    import manta as m
    key, dims, odims, ax, kind = case
    s = solver(m, dims)
    g = grid_from(s, cls_of(m, kind), M.distinct(dims, kind))
    if odims is None:
        g.permuteAxes(*ax)
        same(key, g.to_numpy(), GOLDEN[key])
        return
    t = solver(m, odims)
    out = grid_from(t, cls_of(m, kind), nan_like(odims, kind))
    g.permuteAxesCopyToGrid(ax[0], ax[1], ax[2], out)
    same(key, out.to_numpy(), GOLDEN[key])
    same(key + " (model)", out.to_numpy(), M.permute(M.distinct(dims, kind), ax))
    same("the source", g.to_numpy(), M.distinct(dims, kind))
    back = grid_from(s, cls_of(m, kind), nan_like(dims, kind))
    out.permuteAxesCopyToGrid(*M.inverse(ax), out=back)
    same("the inverse restores the input", back.to_numpy(), M.distinct(dims, kind))


def test_permute_copy_all_permutations_non_cubic(hip_backend):
    """every permutation that the contract allows on a non-cubic grid, and the refusals: `out` stays as it was"""
    import manta as m
    dims = (37, 6, 3)
    s = solver(m, dims)
    for kind in M.KINDS:
        a = M.distinct(dims, kind)
        g = grid_from(s, cls_of(m, kind), a)
        for ax in M.PERMUTATIONS:
            # the dims the reference's assert accepts: sizeTarget[ax[n]] == size[n]
            odims = [0, 0, 0]
            for n in range(3):
                odims[ax[n]] = dims[n]
            odims = tuple(odims)
            t = solver(m, odims)
            fill = M.out_fill(odims, kind)
            out = grid_from(t, cls_of(m, kind), fill)
            if M.permute_refusal(dims, odims, ax) == "outside":
                assert ax in ((1, 2, 0), (2, 0, 1))
                with pytest.raises(RuntimeError, match="permuteAxesCopyToGrid: a cyclic permutation"):
                    g.permuteAxesCopyToGrid(ax[0], ax[1], ax[2], out)
                same("out after the refusal", out.to_numpy(), fill)
            else:
                g.permuteAxesCopyToGrid(ax[0], ax[1], ax[2], out)
                same("copy %s" % (ax,), out.to_numpy(), M.permute(a, ax))
    # a 2-D grid: a permutation that moves axis 2 is refused, with the sizes the reference's assert accepts
    s2, t2 = solver(m, (6, 6, 1)), solver(m, (6, 6, 1))
    g = grid_from(s2, m.RealGrid, M.distinct((6, 6, 1), "real"))
    fill = M.out_fill((6, 6, 1), "real")
    out = grid_from(t2, m.RealGrid, fill)
    with pytest.raises(RuntimeError, match="Permuted grids must have the same dimensions!"):
        g.permuteAxesCopyToGrid(0, 2, 1, out)
    thin = grid_from(m.Solver(name="t", gridSize=m.vec3(6, 1, 6), dim=3), m.RealGrid, M.out_fill((6, 1, 6), "real"))
    with pytest.raises(RuntimeError, match="permuteAxesCopyToGrid: .* moves axis 2 of a 2-D grid"):
        g.permuteAxesCopyToGrid(0, 2, 1, thin)                # the sizes pass the reference's assert
    same("the thin grid", thin.to_numpy(), M.out_fill((6, 1, 6), "real"))
    with pytest.raises(RuntimeError, match="Grids must have same data type!"):
        g.permuteAxesCopyToGrid(1, 0, 2, grid_from(t2, m.IntGrid, M.out_fill((6, 6, 1), "int")))
    with pytest.raises(RuntimeError, match="Grid must be cubic!"):
        grid_from(solver(m, (6, 5, 1)), m.RealGrid, M.distinct((6, 5, 1), "real")).permuteAxes(1, 0, 2)
    with pytest.raises(RuntimeError, match="moves axis 2 of a 2-D grid"):
        g.permuteAxes(2, 1, 0)
    same("out", out.to_numpy(), fill)


# ---- norms ---------------------------------------------------------------------------------------------------------------------------
def check_norm(tag, got, a, bnd, l2, exact):
    want = M.norm(a, bnd, l2)
    lo, hi = M.norm_bounds(a, bnd, l2)
    print(tag, "got", repr(got), "serial", repr(want), "bounds", repr(lo), repr(hi))
    if exact:
        assert f32(got) == want, tag
    assert lo <= f32(got) <= hi, tag


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("dims", M.NORM_DIMS, ids=M.name_of)
def test_norms(hip_backend, dims, kind):
    import manta as m
    s = solver(m, dims)
    table = GOLDEN["norm/%s/%s" % (M.name_of(dims), kind)]
    for fi, fill in enumerate(M.NORM_FILLS):
        a = M.norm_input(dims, kind, fill)
        g = grid_from(s, cls_of(m, kind), a)
        for bi, bnd in enumerate(M.NORM_BNDS):
            for l2, fn in ((0, g.getL1), (1, g.getL2)):
                got = fn(bnd)
                tag = "%s %s bnd %d L%d" % (kind, fill, bnd, l2 + 1)
                check_norm(tag, got, a, bnd, l2, M.exactly_summable(kind, fill, l2))
                if M.exactly_summable(kind, fill, l2):
                    assert f32(got) == table[fi, bi, l2], tag               # the reference's own figure
        assert g.getL1() == g.getL1(0) and g.getL2() == g.getL2(bnd=0)
        assert g.getL1(max(dims)) == 0.0 and g.getL2(dims[1] // 2 + 1) == 0.0      # bnd larger than half a side
        same("the grid", g.to_numpy(), a)


@pytest.mark.parametrize("kind", M.KINDS)
def test_norms_many_blocks(hip_backend, kind):
    import manta as m
    s = solver(m, M.NORM_BIG)
    a = M.norm_input(M.NORM_BIG, kind, "random")
    g = grid_from(s, cls_of(m, kind), a)
    check_norm(kind + " L1", g.getL1(), a, 0, 0, False)
    check_norm(kind + " L2", g.getL2(), a, 0, 1, False)
    q = M.norm_input(M.NORM_BIG, kind, "quarters")
    g.from_numpy(q)
    check_norm(kind + " L2 exact", g.getL2(), q, 0, 1, True)
    check_norm(kind + " L2 exact bnd 1", g.getL2(1), q, 1, 1, True)


# ---- join ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(M.join_cases()), ids=lambda c: c[0])
def test_join(hip_backend, case):
    import manta as m
    key, dims, kind, keep = case
    s = solver(m, dims)
    a, b = M.join_inputs(dims, kind)
    ga, gb = grid_from(s, cls_of(m, kind), a), grid_from(s, cls_of(m, kind), b)
    if keep:
        ga.join(gb)
    else:
        ga.join(gb, keepMax=False)
    same(key, ga.to_numpy(), GOLDEN[key])
    same("b", gb.to_numpy(), b)


# ---- force fields --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", M.FORCE_DIMS, ids=M.name_of)
def test_force_fields_and_initial_velocity(hip_backend, dims):
    import manta as m
    s = solver(m, dims)
    f, v, fo, r = M.force_inputs(dims)
    flags, force, region = grid_from(s, m.FlagGrid, f), grid_from(s, m.VecGrid, fo), grid_from(s, m.RealGrid, r)
    for key, _, reg, mac, add in M.force_cases():
        if _ != dims:
            continue
        vel = grid_from(s, m.MACGrid, v)
        kw = {}
        if reg:
            kw["region"] = region
        if mac:
            kw["isMAC"] = True
        (m.addForceField if add else m.setForceField)(flags, vel, force, **kw)
        same(key, vel.to_numpy(), GOLDEN[key])
    vel = grid_from(s, m.MACGrid, v)
    m.setInitialVelocity(flags, vel, force)
    same("setInitialVelocity", vel.to_numpy(), GOLDEN["initvel/" + M.name_of(dims)])
    for g, a in ((flags, f), (force, fo), (region, r)):
        same("an input", g.to_numpy(), a)
    # both arms of the clamp are in the input
    half = f32(0.5) * (M.lower(fo[..., 0], 0) + fo[..., 0])
    assert (half > 0).any() and (half < 0).any()


# ---- extrapolateVec3Simple -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", M.EXTRAP_DIMS, ids=M.name_of)
def test_extrapolate_vec3_simple(hip_backend, dims):
    import manta as m
    s = solver(m, dims)
    for key, d, which, dist, inside in M.extrap_cases():
        if d != dims:
            continue
        v, p = M.extrap_phi(dims, which, inside)
        vel, phi = grid_from(s, m.VecGrid, v), grid_from(s, m.RealGrid, p)
        poison = grid_from(s, m.IntGrid, nan_like(dims, "int"))
        del poison
        live = s._live
        m.extrapolateVec3Simple(vel, phi, distance=dist, inside=bool(inside))
        same(key, vel.to_numpy(), GOLDEN[key])
        same("phi", phi.to_numpy(), p)
        assert s._live == live
    v, p = M.extrap_phi(dims, "blob", 0)
    vel, phi = grid_from(s, m.VecGrid, v), grid_from(s, m.RealGrid, p)
    m.extrapolateVec3Simple(vel, phi)                                       # the defaults: distance 4, outwards
    same("defaults", vel.to_numpy(), M.extrapolate_vec3_simple(v, p, 4, False))


# ---- emission, reset, converters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", M.SMALL_DIMS, ids=M.name_of)
def test_emission_and_reset(hip_backend, dims):
    import manta as m
    s, g = solver(m, dims), M.name_of(dims)
    f, t, so, te = M.emission_inputs(dims)
    flags, source, tex = grid_from(s, m.FlagGrid, f), grid_from(s, m.RealGrid, so), grid_from(s, m.RealGrid, te)
    for q, (with_tex, absolute, type_) in enumerate(M.EMISSION_CASES):
        target = grid_from(s, m.RealGrid, t)
        m.applyEmission(flags, target, source, tex if with_tex else None, absolute, type_)
        same("emission %d" % q, target.to_numpy(), GOLDEN["emission/%s/%d" % (g, q)])
    target = grid_from(s, m.RealGrid, t)
    m.applyEmission(flags, target, source)
    same("emission, defaults", target.to_numpy(), so)

    f, v, grids = M.reset_inputs(dims)
    flags = grid_from(s, m.FlagGrid, f)
    for q, names in enumerate(M.RESET_CASES):
        vel = grid_from(s, m.MACGrid, v)
        given = {k: grid_from(s, m.RealGrid, grids[k]) for k in names}
        m.resetInObstacle(flags, vel, given.get("density"), resetValue=float(M.RESET_VALUE), **{k: x for k, x in given.items() if k != "density"})
        same("reset %d vel" % q, vel.to_numpy(), GOLDEN["reset/%s/%d/vel" % (g, q)])
        for k in names:
            same("reset %d %s" % (q, k), given[k].to_numpy(), GOLDEN["reset/%s/%d/%s" % (g, q, k)])
    vel = grid_from(s, m.MACGrid, v)
    m.resetInObstacle(flags, vel, None)                                     # the default value: 0
    same("reset, defaults", vel.to_numpy(), M.reset_in_obstacle(f, v, {}, f32(0))[0])


@pytest.mark.parametrize("dims", M.SMALL_DIMS, ids=M.name_of)
def test_converters(hip_backend, dims):
    import manta as m
    s, g = solver(m, dims), M.name_of(dims)
    f, src, tgt = M.random_flags(dims, "macdata"), M.vec(dims, "macsrc"), M.vec(dims, "mactgt")
    flags, source = grid_from(s, m.FlagGrid, f), grid_from(s, m.MACGrid, src)
    for bnd in M.MAC_BNDS:
        target = grid_from(s, m.MACGrid, tgt)
        m.copyMACData(source, target, flags, M.MAC_FLAG, bnd)
        same("copyMACData %d" % bnd, target.to_numpy(), GOLDEN["macdata/%s/b%d" % (g, bnd)])
    target = grid_from(s, m.MACGrid, tgt)
    m.copyMACData(source, target, flags, M.MAC_FLAG, max(dims))              # an empty range
    same("copyMACData, empty", target.to_numpy(), tgt)

    x, y, z, v = M.real(dims, "x"), M.real(dims, "y"), M.real(dims, "z"), M.vec(dims, "v")
    gx, gy, gz = (grid_from(s, m.RealGrid, a) for a in (x, y, z))
    out = grid_from(s, m.VecGrid, nan_like(dims, "vec"))
    m.copyRealToVec3(gx, gy, gz, out)
    same("copyRealToVec3", out.to_numpy(), GOLDEN["r2v/" + g])
    gv = grid_from(s, m.VecGrid, v)
    ox, oy, oz = (grid_from(s, m.RealGrid, nan_like(dims, "real")) for _ in range(3))
    m.copyVec3ToReal(gv, ox, oy, oz)
    for k, o in (("x", ox), ("y", oy), ("z", oz)):
        same("copyVec3ToReal " + k, o.to_numpy(), GOLDEN["v2r/%s/%s" % (g, k)])

    target = grid_from(s, m.VecGrid, tgt)
    m.resampleMacToVec3(source, target)
    same("resampleMacToVec3", target.to_numpy(), GOLDEN["resample/" + g])

    for c in M.SWAPS:
        gv = grid_from(s, m.VecGrid, v)
        m.swapComponents(gv, *c)
        same("swapComponents%s" % (c,), gv.to_numpy(), GOLDEN["swap/%s/%d%d%d" % ((g,) + c)])
    gv = grid_from(s, m.VecGrid, v)
    m.swapComponents(gv)
    same("swapComponents()", gv.to_numpy(), v)

    for which in M.AVG_FLAGS:
        fl = M.avg_flags(dims, which)
        got = m.getGridAvg(gx, None if fl is None else grid_from(s, m.FlagGrid, fl))
        lo, hi = M.grid_avg_bounds(x, fl)
        print("getGridAvg", which, repr(got), "reference", repr(GOLDEN["avg/%s/%s" % (g, which)][0]), "bounds", repr(lo), repr(hi))
        assert lo <= f32(got) <= hi, which
    assert m.getGridAvg(gx, grid_from(s, m.FlagGrid, M.avg_flags(dims, "nofluid"))) == -1.0
    quarters = (M.rng("avgq", dims).randint(-32, 33, M.shape_of(dims)) / 4.0).astype(f32)           # exactly summable
    assert f32(m.getGridAvg(grid_from(s, m.RealGrid, quarters))) == M.grid_avg(quarters, None)

    src = M.int_input(dims)
    dest = grid_from(s, m.RealGrid, nan_like(dims, "real"))
    m.debugIntToReal(grid_from(s, m.IntGrid, src), dest, float(M.INT_FACTOR))
    same("debugIntToReal", dest.to_numpy(), GOLDEN["i2r/" + g])
    m.debugIntToReal(grid_from(s, m.IntGrid, src), dest)
    same("debugIntToReal, factor 1", dest.to_numpy(), src.astype(f32))


# ---- the legacy single-potential whitewater plugins -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(M.legacy_cases()), ids=lambda c: c[0])
def test_legacy_potentials(hip_backend, case):
    import manta as m
    key, dims, radius, t = case
    s = solver(m, dims)
    f, v, nr, ph = M.legacy_inputs(dims, radius)
    itype, jtype = M.LEGACY_TYPES[t]
    assert M.legacy_preconditions(f, radius, itype, jtype)
    flags, vel, normal = grid_from(s, m.FlagGrid, f), grid_from(s, m.MACGrid, v), grid_from(s, m.VecGrid, nr)
    scale = float(M.LEGACY_SCALE)
    types = {} if t == 0 else dict(itype=itype, jtype=jtype)                    # the defaults are TypeFluid, TypeFluid
    pot = grid_from(s, m.RealGrid, nan_like(dims, "real"))
    tmin, tmax = (float(x) for x in M.LEGACY_TAU["ta"][t])
    m.flipComputePotentialTrappedAir(pot, flags, vel, radius, tmin, tmax, scale, **types)
    same(key + "/ta", pot.to_numpy(), GOLDEN[key + "/ta"])
    pot.from_numpy(nan_like(dims, "real"))
    tmin, tmax = (float(x) for x in M.LEGACY_TAU["wc"][t])
    m.flipComputePotentialWaveCrest(pot, flags, vel, radius, normal, tmin, tmax, scale, **types)
    same(key + "/wc", pot.to_numpy(), GOLDEN[key + "/wc"])
    pot.from_numpy(nan_like(dims, "real"))
    tmin, tmax = (float(x) for x in M.LEGACY_TAU["ke"][t])
    m.flipComputePotentialKineticEnergy(pot, flags, vel, tmin, tmax, scale, **({} if t == 0 else dict(itype=itype)))
    same(key + "/ke", pot.to_numpy(), GOLDEN[key + "/ke"])
    itype, jtype = M.LEGACY_RATIO_TYPES[t]
    pot.from_numpy(nan_like(dims, "real"))
    m.flipUpdateNeighborRatio(flags, pot, radius, **({} if t == 0 else dict(itype=itype, jtype=jtype)))      # defaults: fluid, obstacle
    same(key + "/ratio", pot.to_numpy(), GOLDEN[key + "/ratio"])                # NaN in the same place
    if t == 0:
        m.flipComputeSurfaceNormals(normal, grid_from(s, m.RealGrid, ph))
        same(key + "/normals", normal.to_numpy(), GOLDEN[key + "/normals"])
    for g, a in ((flags, f), (vel, v)):
        same("an input", g.to_numpy(), a)


# ---- host-only samplers on device grids -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(M.interp_cases()), ids=lambda c: c[0])
def test_get_interpolated_reads_back_the_device_grid(hip_backend, case):
    import manta as m
    key, dims, kind = case
    s = solver(m, dims)
    g = grid_from(s, {"real": m.RealGrid, "vec": m.VecGrid, "mac": m.MACGrid}[kind], M.interp_input(dims, kind))
    want = GOLDEN[key]
    for q, p in list(enumerate(M.interp_positions(dims)))[::4]:
        got = g.getInterpolated(m.vec3(float(p[0]), float(p[1]), float(p[2])))
        got = np.array([got], f32)[0] if kind == "real" else np.array(list(got), f32)
        assert M.same(got, want[q]), (q, p, got, want[q])


# ---- simple noise --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", M.NOISE_DIMS, ids=M.name_of)
def test_simple_noise(hip_backend, dims):
    import manta as m
    s = solver(m, dims)
    for key, d, is_vec, w, nset in M.noise_cases():
        if d != dims:
            continue
        f, t, wt = M.noise_inputs(dims, is_vec)
        flags, weight = grid_from(s, m.FlagGrid, f), grid_from(s, m.RealGrid, wt)
        target = grid_from(s, m.VecGrid if is_vec else m.RealGrid, t)
        noise = M.noise_field(m, s, nset)
        fn = m.applySimpleNoiseVec3 if is_vec else m.applySimpleNoiseReal
        if w:
            fn(flags, target, noise, float(M.NOISE_SCALE), weight)
        else:
            fn(flags, target, noise, scale=float(M.NOISE_SCALE))
        same(key, target.to_numpy(), GOLDEN[key])
        same("flags", flags.to_numpy(), f)
        same("weight", weight.to_numpy(), wt)
    assert isinstance(M.noise_field(m, s, 0), m.WaveletNoiseField)

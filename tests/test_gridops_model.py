"""CPU: the numpy model of the grid operations (tests/gridops_model.py) against the reference's recorded outputs
(tests/golden/gridops.npz): bit for bit in every case.  The reference sums its three fp64 sums serially and so does the model, so these
agree exactly as well; the bound a device result is held to is checked here for what it must allow (the serial figure) and for what it
must exclude."""
import numpy as np
import pytest

import gridops_model as M

GOLDEN = np.load(M.GOLDEN)
f32, f64 = np.float32, np.float64


def same(tag, got, want):
    assert M.same(got, want), "%s: %d of %d elements differ" % (tag, M.differing(np.asarray(got), np.asarray(want)), np.asarray(want).size)


def test_every_key_of_the_fixture_is_a_case():
    keys = {c[0] for fn in (M.permute_cases, M.norm_cases, M.join_cases, M.force_cases, M.extrap_cases, M.noise_cases) for c in fn()}
    keys |= {"norm/big/" + k for k in M.KINDS} | {"initvel/" + M.name_of(d) for d in M.FORCE_DIMS}
    keys |= {c[0] for c in M.interp_cases()} | {"npzsize/file"}
    for key, _, _, t in M.legacy_cases():
        keys |= {key + "/" + k for k in ("ta", "wc", "ke", "ratio") + (("normals",) if t == 0 else ())}
    for dims in M.SMALL_DIMS:
        g = M.name_of(dims)
        keys |= {"emission/%s/%d" % (g, q) for q in range(len(M.EMISSION_CASES))}
        for q, names in enumerate(M.RESET_CASES):
            keys |= {"reset/%s/%d/%s" % (g, q, k) for k in ("vel",) + names}
        keys |= {"macdata/%s/b%d" % (g, b) for b in M.MAC_BNDS} | {"r2v/" + g, "resample/" + g, "i2r/" + g}
        keys |= {"v2r/%s/%s" % (g, k) for k in "xyz"} | {"swap/%s/%d%d%d" % ((g,) + c) for c in M.SWAPS}
        keys |= {"avg/%s/%s" % (g, w) for w in M.AVG_FLAGS}
    assert keys == set(GOLDEN.files)


@pytest.mark.parametrize("case", list(M.permute_cases()), ids=lambda c: c[0])
def test_permutation(case):
    key, dims, odims, ax, kind = case
    want = GOLDEN[key]
    same(key, M.permute_model(dims, odims, ax, kind), want)
    if odims is not None:
        assert want.shape[:3] == M.shape_of(odims) and M.permute_refusal(dims, odims, ax) is None
        assert not M.same(want, M.out_fill(odims, kind))
    if sorted(ax) == [0, 1, 2]:
        same("the inverse", M.permute(want, M.inverse(ax)), M.distinct(dims, kind))
        # the rule itself, cell by cell: target(s[ax0], s[ax1], s[ax2]) = self(s0, s1, s2)
        a = M.distinct(dims, kind)
        for s in ((0, 0, 0), (1, 2, 0), (dims[0] - 1, 0, dims[2] - 1), (2, dims[1] - 1, dims[2] // 2)):
            t = (s[ax[0]], s[ax[1]], s[ax[2]])
            assert np.array_equal(want[t[2], t[1], t[0]], a[s[2], s[1], s[0]]), (s, t)


def test_permutation_refusals_of_the_contract():
    # the two 3-cycles on a non-cubic grid pass the reference's assert and would write outside; the swaps and a cube do not
    for ax in M.PERMUTATIONS:
        dims = (7, 5, 3)
        odims = [0, 0, 0]
        for n in range(3):
            odims[ax[n]] = dims[n]
        assert M.permute_refusal(dims, tuple(odims), ax) == ("outside" if ax in ((1, 2, 0), (2, 0, 1)) else None), ax
        assert M.permute_refusal((4, 4, 4), (4, 4, 4), ax) is None
        assert M.permute_refusal((4, 4, 1), (4, 4, 1), ax) == (None if ax[2] == 2 else "assert")
    assert M.permute_refusal((6, 6, 1), (6, 1, 6), (0, 2, 1)) == "outside"
    assert M.permute_refusal((7, 5, 3), (7, 5, 3), (1, 0, 2)) == "assert"


@pytest.mark.parametrize("case", list(M.norm_cases()), ids=lambda c: c[0])
def test_norms(case):
    key, dims, kind = case
    want = GOLDEN[key]
    same(key, M.norm_table(dims, kind, M.norm), want)
    for fi, fill in enumerate(M.NORM_FILLS):
        a = M.norm_input(dims, kind, fill)
        for bi, bnd in enumerate(M.NORM_BNDS):
            for l2 in (0, 1):
                lo, hi = M.norm_bounds(a, bnd, l2)
                assert lo <= want[fi, bi, l2] <= hi
                t = M.norm_terms(a, bnd, l2)
                if M.exactly_summable(kind, fill, l2):
                    # exactly summable: any order gives the same fp64 sum
                    assert M.serial_sum(t) == M.serial_sum(t[::-1]) == f64(np.sort(t.astype(f64)).sum())
                    if kind != "vec" or fill == "zero":
                        assert lo == hi == want[fi, bi, l2]
                # the bound excludes the neighbouring floats unless a rounding boundary is within delta
                assert np.nextafter(lo, f32(-np.inf)) < lo and hi - lo <= np.spacing(hi)
    assert (want[2] == 0).all()                                       # the all-zero grid


def test_norm_of_the_large_grid():
    for kind in M.KINDS:
        a = M.norm_input(M.NORM_BIG, kind, "random")
        want = GOLDEN["norm/big/" + kind]
        for l2 in (0, 1):
            assert M.norm(a, 0, l2) == want[l2]
            lo, hi = M.norm_bounds(a, 0, l2)
            assert lo <= want[l2] <= hi and hi - lo <= np.spacing(hi)
    assert a.size // 3 == 129 * 127 * 64 > 256 * 8 * 256 and (129 * 127 * 64) % 256 != 0      # many blocks, a ragged tail


def test_norm_ranges():
    assert M.in_range((12, 9, 1), 3).sum() == 6 * 3 and M.in_range((12, 9, 1), 5).sum() == 0        # z is not cut in 2-D
    assert M.in_range((33, 7, 5), 3).sum() == 0 and M.in_range((33, 7, 5), 2).sum() == 29 * 3 * 1
    assert M.norm(np.ones(M.shape_of((33, 7, 5)), f32), 3, 1) == 0


@pytest.mark.parametrize("case", list(M.join_cases()), ids=lambda c: c[0])
def test_join(case):
    key, dims, kind, keep = case
    a, b = M.join_inputs(dims, kind)
    same(key, M.join(a, b, keep), GOLDEN[key])
    if kind == "vec":
        w = GOLDEN[key]
        assert (w[..., 0] == w[..., 1]).all() and (w[..., 0] == w[..., 2]).all() and (w >= 0).all()
    else:
        assert (a == b).any() and (a < b).any() and (a > b).any()


@pytest.mark.parametrize("case", list(M.force_cases()), ids=lambda c: c[0])
def test_force_fields(case):
    key, dims, reg, mac, add = case
    same(key, M.force_model(dims, reg, mac, add), GOLDEN[key])
    flags, vel, force, region = M.force_inputs(dims)
    want = GOLDEN[key]
    assert not M.same(want, vel)
    changed = (want != vel).any(axis=3)
    assert not (changed & ~M.in_range(dims, 1)).any()                       # bnd = 1
    assert not (changed & ((flags & (M.FLUID | M.EMPTY)) == 0)).any()
    if reg:
        assert not (changed & (region > 0)).any() and (changed & (region == 0)).any() and (changed & (region < 0)).any()
    if dims[2] == 1:
        same("z in 2-D", want[..., 2], vel[..., 2])


@pytest.mark.parametrize("dims", M.FORCE_DIMS, ids=M.name_of)
def test_set_initial_velocity(dims):
    flags, vel, force, _ = M.force_inputs(dims)
    want = GOLDEN["initvel/" + M.name_of(dims)]
    same("setInitialVelocity", M.add_force_if_lower(flags, vel, force), want)
    # the clamp: never past max(vel, f) for f > 0, never below min(vel, f) otherwise
    for c in range(3 if dims[2] > 1 else 2):
        fv = (f32(0.5) * (M.lower(force[..., c], c) + force[..., c])).astype(f32)
        ch = want[..., c] != vel[..., c]
        assert (ch & (fv > 0)).any() and (ch & (fv < 0)).any()
        assert (want[..., c][ch & (fv > 0)] <= np.maximum(vel[..., c], fv)[ch & (fv > 0)]).all()
        assert (want[..., c][ch & (fv <= 0)] >= np.minimum(vel[..., c], fv)[ch & (fv <= 0)]).all()


@pytest.mark.parametrize("case", list(M.extrap_cases()), ids=lambda c: c[0])
def test_extrapolate_vec3_simple(case):
    key, dims, which, dist, inside = case
    vel, phi = M.extrap_phi(dims, which, inside)
    want = GOLDEN[key]
    same(key, M.extrapolate_vec3_simple(vel, phi, dist, bool(inside)), want)
    interior = M.in_range(dims, 1)
    same("the border", want[~interior], vel[~interior])
    marked = interior & ((phi > 0) if inside else (phi < 0))
    same("the marked cells", want[marked], vel[marked])
    if which == "none":
        assert not marked.any() and (want[interior] == 0).all()
    if which == "all":
        assert marked[interior].all() and M.same(want, vel)
    if which == "blob":
        assert marked.any() and (interior & ~marked).any()


def test_extrapolation_first_layer_keeps_its_values_and_distance_matters():
    dims = M.EXTRAP_DIMS[0]
    g = M.name_of(dims)
    vel, phi = M.extrap_phi(dims, "blob", 0)
    d1, d2, d5 = (GOLDEN["extrap/%s/blob/d%d/i0" % (g, d)] for d in (1, 2, 5))
    assert not M.same(d1, d2) and not M.same(d2, d5)          # distance 1 runs no pass, distance 2 one (d = 2), distance 5 four
    interior, marked = M.in_range(dims, 1), M.in_range(dims, 1) & (phi < 0)
    near = np.zeros(marked.shape, bool)
    for c in range(3):
        near |= M.lower(marked, c) | M.upper(marked, c)
    first = interior & ~marked & near
    assert first.any()
    same("the first layer", d5[first], vel[first])
    assert (d1[interior & ~marked & ~first] == 0).all()


@pytest.mark.parametrize("dims", M.SMALL_DIMS, ids=M.name_of)
def test_small_plugins(dims):
    g = M.name_of(dims)
    flags, target, source, tex = M.emission_inputs(dims)
    for q, (with_tex, absolute, type_) in enumerate(M.EMISSION_CASES):
        want = GOLDEN["emission/%s/%d" % (g, q)]
        same("emission %d" % q, M.apply_emission(flags, target, source, tex if with_tex else None, absolute, type_), want)
        kept = want == target
        if not (with_tex and type_):
            assert M.same(want, source if absolute else (target + source))             # the && : one condition alone never skips
        else:
            assert kept.any() and not kept.all()
            assert (tex[kept] == 0).all()
    flags, vel, grids = M.reset_inputs(dims)
    for q, names in enumerate(M.RESET_CASES):
        wv, wg = M.reset_in_obstacle(flags, vel, {k: grids[k] for k in names}, M.RESET_VALUE)
        same("reset %d vel" % q, wv, GOLDEN["reset/%s/%d/vel" % (g, q)])
        for k in names:
            same("reset %d %s" % (q, k), wg[k], GOLDEN["reset/%s/%d/%s" % (g, q, k)])
            assert (wg[k][(flags & M.OBSTACLE) != 0] == M.RESET_VALUE).all()
    f, src, tgt = M.random_flags(dims, "macdata"), M.vec(dims, "macsrc"), M.vec(dims, "mactgt")
    for bnd in M.MAC_BNDS:
        same("copyMACData %d" % bnd, M.copy_mac_data(src, tgt, f, M.MAC_FLAG, bnd), GOLDEN["macdata/%s/b%d" % (g, bnd)])
    assert not M.same(GOLDEN["macdata/%s/b0" % g], GOLDEN["macdata/%s/b2" % g])
    x, y, z, v = M.real(dims, "x"), M.real(dims, "y"), M.real(dims, "z"), M.vec(dims, "v")
    same("copyRealToVec3", np.stack([x, y, z], axis=3), GOLDEN["r2v/" + g])
    for c, k in enumerate("xyz"):
        same("copyVec3ToReal " + k, np.ascontiguousarray(v[..., c]), GOLDEN["v2r/%s/%s" % (g, k)])
    want = GOLDEN["resample/" + g]
    same("resampleMacToVec3", M.resample_mac_to_vec3(src, tgt), want)
    same("its border", want[~M.in_range(dims, 1)], tgt[~M.in_range(dims, 1)])
    if dims[2] == 1:
        assert (want[..., 2][M.in_range(dims, 1)] == 0).all()
    for c in M.SWAPS:
        same("swapComponents%s" % (c,), M.swap_components(v, *c), GOLDEN["swap/%s/%d%d%d" % ((g,) + c)])
    for which in M.AVG_FLAGS:
        fl = M.avg_flags(dims, which)
        want = GOLDEN["avg/%s/%s" % (g, which)][0]
        assert M.grid_avg(x, fl) == want
        lo, hi = M.grid_avg_bounds(x, fl)
        assert lo <= want <= hi
    assert GOLDEN["avg/%s/nofluid" % g][0] == -1
    same("debugIntToReal", M.int_to_real(M.int_input(dims), M.INT_FACTOR), GOLDEN["i2r/" + g])


@pytest.mark.parametrize("case", list(M.legacy_cases()), ids=lambda c: c[0])
def test_legacy_potentials(case):
    key, dims, radius, t = case
    flags, vel, nrm, phi = M.legacy_inputs(dims, radius)
    itype, jtype = M.LEGACY_TYPES[t]
    assert M.legacy_preconditions(flags, radius, itype, jtype)                  # the inputs' side of the contract
    cell = M.in_range(dims, 1) & ((flags & itype) != 0)
    for which, name, normal in ((0, "ta", None), (1, "wc", nrm)):
        tmin, tmax = M.LEGACY_TAU[name][t]
        pot, _ = M.legacy_gather(which, flags, vel, normal, radius, tmin, tmax, M.LEGACY_SCALE, itype, jtype)
        same(key + "/" + name, pot, GOLDEN[key + "/" + name])
        assert (pot[~cell] == 0).all() and cell.any()                           # pot.clear() and bnd = 1
    tmin, tmax = M.LEGACY_TAU["ke"][t]
    same(key + "/ke", M.legacy_kinetic(flags, vel, tmin, tmax, M.LEGACY_SCALE, itype), GOLDEN[key + "/ke"])
    itype, jtype = M.LEGACY_RATIO_TYPES[t]
    assert M.legacy_preconditions(flags, radius, itype, jtype, with_centres=False)
    ratio = GOLDEN[key + "/ratio"]
    same(key + "/ratio", M.legacy_ratio(flags, radius, itype, jtype), ratio)
    walled = ratio[dims[2] // 2 if dims[2] > 1 else 0, dims[1] // 2, dims[0] // 2]
    # no countable neighbour: 0 / 0 in 3-D; in 2-D the cell meets itself on the aliased planes z != k, and those count
    assert np.isnan(walled) if dims[2] > 1 else walled == 1
    if t == 0:
        want = GOLDEN[key + "/normals"]
        same(key + "/normals", M.surface_normals(nrm, phi), want)
        l = np.sqrt((want.astype(f64) ** 2).sum(axis=3))
        assert (np.abs(l[M.in_range(dims, 1)] - 1) < 1e-6).all()


def test_legacy_thresholds_lie_on_both_sides_of_the_sums():
    for which, name in ((0, "ta"), (1, "wc")):
        below = between = above = False
        for key, dims, radius, t in M.legacy_cases():
            flags, vel, nrm, _ = M.legacy_inputs(dims, radius)
            itype, jtype = M.LEGACY_TYPES[t]
            tmin, tmax = M.LEGACY_TAU[name][t]
            _, acc = M.legacy_gather(which, flags, vel, nrm if which else None, radius, tmin, tmax, M.LEGACY_SCALE, itype, jtype)
            a = acc[M.in_range(dims, 1) & ((flags & itype) != 0)]
            below, between, above = below or (a < tmin).any(), between or ((a > tmin) & (a < tmax)).any(), above or (a > tmax).any()
        assert below and between and above, name
    # the 2-D aliasing: with radius 1 a 2-D cell has 3 * 3 * 3 - 1 = 26 visits; its 8 neighbours are met three times, itself twice.
    # One fluid cell among empty ones therefore has the ratio 2 / 26, where a 3-D reading of the loop would give 0 / 8.
    dims = M.LEGACY_DIMS[1]
    f = np.full(M.shape_of(dims), M.EMPTY, np.int32)
    f[0, 5, 5] = M.FLUID
    assert M.legacy_ratio(f, 1, M.FLUID, M.OBSTACLE)[0, 5, 5] == np.float32(2) / np.float32(26)


@pytest.mark.parametrize("case", list(M.noise_cases()), ids=lambda c: c[0])
def test_simple_noise(oracle_backend, case):
    key, dims, is_vec, w, nset = case
    flags, target, weight = M.noise_inputs(dims, is_vec)
    tile, params = M.noise_tile_and_params(dims, nset)
    want = GOLDEN[key]
    same(key, M.apply_simple_noise(flags, target, tile, params, M.NOISE_SCALE, weight if w else None), want)
    changed = (want != target) if not is_vec else (want != target).any(axis=3)
    assert changed.any() and not (changed & ((flags & M.FLUID) == 0)).any()
    if w:
        assert not (changed & (weight == 0)).any()
    if nset == 1 and not is_vec and not w:
        # the clamp is on: the added value lies in [clampNeg, clampPos] * scale
        add = (want - target)[changed]
        assert add.min() >= -0.2 * M.NOISE_SCALE - 1e-5 and add.max() <= 0.3 * M.NOISE_SCALE + 1e-5

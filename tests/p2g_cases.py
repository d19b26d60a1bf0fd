"""Seeded inputs of the atomic particle->grid tests (tests/test_p2g_model.py on the CPU, tests/test_gpu_p2g_atomic.py on the GPU) and
the numpy predicates that assert what each input was built to force.  Every input is built once per process, with its model
(p2g_model) and the oracle's outputs, and handed out read-only.

Two families:
  dyadic   positions cell + {0, 1/4, 1/2, 3/4} per axis, values integer multiples of 1/2 in [-4, 4]: every weight is a multiple of
           2^-6, every term one of 2^-7, so while sum |term| < 2^17 on every entry all partial sums of any order are exact in fp32
  random   jittered positions (util.make_particles), normal values
"""
import functools

import numpy as np

import p2g_model as M
import util

EXCLUDE = 4
QUARTERS = np.array([0.0, 0.25, 0.5, 0.75], np.float32)
BLOCK, SLOTS = 256, 2048          # k_p2g_mac_lds: particles per block, slots of its LDS table


class Input:
    def __init__(self, name, dims, pos, pflag, pvel, ptype):
        self.name, self.dims = name, tuple(dims)
        self.pos, self.pflag = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(pflag, np.int32)
        self.pvel, self.ptype = np.ascontiguousarray(pvel, np.float32), np.ascontiguousarray(ptype, np.int32)
        self.np = self.pos.shape[1]
        sx, sy, sz = self.dims
        assert np.isfinite(self.pos).all() and self.pos.min() >= 0 and (self.pos.max(axis=1) < np.array([sx, sy, sz])).all()
        for a in (self.pos, self.pflag, self.pvel, self.ptype):
            a.setflags(write=False)

    def prefix(self, m):
        """the first m particles (contiguous copies)"""
        return Input("%s[:%d]" % (self.name, m), self.dims, self.pos[:, :m], self.pflag[:m], self.pvel[:, :m], self.ptype[:m])

    def permuted(self, name, perm):
        return Input(name, self.dims, self.pos[:, perm], self.pflag[perm], self.pvel[:, perm], self.ptype[perm])

    # models: built on first use, shared by every test of the process
    @functools.cached_property
    def mac(self):
        return M.mac_accum(self.dims, self.pos, self.pflag, self.pvel, self.ptype, EXCLUDE)

    @functools.lru_cache(maxsize=None)
    def cell(self, ncomp):
        return M.cell_accum(self.dims, ncomp, self.pos, self.pflag, self.pvel if ncomp == 3 else self.pvel[0])


def _flags_types(rng, n, deleted_frac=0.02):
    pflag = np.zeros(n, np.int32)
    pflag[rng.random(n) < deleted_frac] = M.PDELETE
    pflag[rng.random(n) < 0.05] |= 1      # PNEW: must not matter
    return pflag, rng.choice(np.array([1, 4, 1], np.int32), n).astype(np.int32)


def _dyadic_at(rng, cells):
    return cells.astype(np.float32) + QUARTERS[rng.integers(0, 4, cells.shape)]


def _dyadic_values(rng, n):
    return (rng.integers(-8, 9, (3, n)) / 2.0).astype(np.float32)


def _edge_cells(rng, dims, m):
    """m cells anywhere on the grid, a third of them in the first and a third in the last column (x < 0.5 and x >= sx - 1:
    the face stencil is clamped, and the +1 corner of the last row's cells is the first entry of the next row)"""
    sx, sy, sz = dims
    c = np.stack([rng.integers(0, sx, m), rng.integers(0, sy, m), rng.integers(0, sz, m)], 0)
    c[0, : m // 3] = 0
    c[0, m // 3: 2 * (m // 3)] = sx - 1
    return c


def _dyadic(name, dims, seed, per_cell, crowds, nborder, all_cells):
    rng = np.random.default_rng(seed)
    flags = util.make_flags(*dims, seed, empty_top=True)
    kk, jj, ii = np.nonzero(np.ones_like(flags) if all_cells else (flags & util.FLUID))     # memory order: cell-ordered particles
    cells = [np.repeat(np.stack([ii, jj, kk], 0), per_cell, axis=1)]
    cells += [np.repeat(np.array(c)[:, None], m, axis=1) for c, m in crowds]
    if nborder:
        cells.append(_edge_cells(rng, dims, nborder))
    pos = _dyadic_at(rng, np.concatenate(cells, axis=1))
    n = pos.shape[1]
    pflag, ptype = _flags_types(rng, n)
    return Input(name, dims, pos, pflag, _dyadic_values(rng, n), ptype)


def _shuffled(inp, seed):
    return inp.permuted(inp.name + "-shuffled", np.random.default_rng(seed).permutation(inp.np))


# ---- the run shapes of k_p2g_mac_atomic: aligned groups of 8 lanes -------------------------------------------------------------------
PATTERNS = ("eight_equal", "AABBCCDD", "ABABABAB", "straddle", "split")


def run_patterns(keys):
    """keys: [np] base address per particle, -1 = inactive.  -> {pattern: set of group parities (0 / 1) it occurs at}.  A DPP row is
    16 lanes = two groups, and the row's edges are where bound_ctrl and the old operand matter, so both parities are wanted."""
    m = -(-keys.size // 8) * 8
    g = np.full(m, -1, np.int64)
    g[:keys.size] = keys
    g = g.reshape(-1, 8)
    ok = (g >= 0).all(1)
    ne = g[:, 1:] != g[:, :-1]
    found = {
        "eight_equal": ok & ~ne.any(1),
        "AABBCCDD": ok & ~ne[:, 0::2].any(1) & ne[:, 1::2].all(1),
        "ABABABAB": ok & ne.all(1) & (g[:, 2:] == g[:, :-2]).all(1),
        "straddle": np.append((g[:-1, 7] >= 0) & (g[:-1, 7] == g[1:, 0]) & (g[:-1, 6] == g[:-1, 7]) & (g[1:, 1] == g[1:, 0]), False),
        "split": ((g[:, 1:-1] < 0) & (g[:, :-2] >= 0) & (g[:, :-2] == g[:, 2:])).any(1),
    }
    return {k: set((np.nonzero(v)[0] & 1).tolist()) for k, v in found.items()}


def _pattern_input():
    """12x10x9, 392 particles: seven groups of 8 -- eight equal / AABBCCDD / ABABABAB / two groups sharing a straddling run / a run
    with a deleted particle inside / a run with an excluded one -- repeated seven times.  Seven is odd, so each shape falls on both
    group parities.  In repetitions 0 and 1 every particle sits in the upper half of its cell on all axes, where build_index and
    build_index_shift return the same cell and the keys of all three components follow the cells; later repetitions use all four
    quarter offsets, so the three components see different runs (a particle's b.yi differs from s.yi below the half-cell line)."""
    dims = (12, 10, 9)
    rng = np.random.default_rng(81)
    cells, upper, dele, excl = [], [], [], []
    for rep in range(7):
        c = [np.array([1 + (rep + 2 * i) % 9, 1 + (rep + i) % 7, 1 + (3 * rep + i) % 6]) for i in range(6)]
        groups = [[0] * 8, [0, 0, 1, 1, 2, 2, 3, 3], [4, 5] * 4, [1, 1, 1, 3, 3, 2, 2, 2], [2, 2, 2, 4, 4, 4, 5, 5], [3] * 8, [5] * 8]
        for gi, g in enumerate(groups):
            for lane, ci in enumerate(g):
                cells.append(c[ci])
                upper.append(rep < 2)
                dele.append(gi == 5 and lane == 3)
                excl.append(gi == 6 and lane == 5)
    cells, upper = np.stack(cells, 1), np.array(upper)
    n = cells.shape[1]
    q = rng.integers(0, 4, (3, n))
    q[:, upper] = rng.integers(2, 4, (3, int(upper.sum())))
    pos = cells.astype(np.float32) + QUARTERS[q]
    pflag = np.where(np.array(dele), M.PDELETE, 0).astype(np.int32)
    ptype = np.where(np.array(excl), EXCLUDE, 1).astype(np.int32)
    pvel = _dyadic_values(rng, n)
    pvel[:, 0] = 4.0        # inactive lanes read particle 0: make what they must not add as large as the family allows
    return Input("patterns", dims, pos, pflag, pvel, ptype)


def _random(name, dims, seed, per_cell, crowds=()):
    rng = np.random.default_rng(seed)
    sx, sy, sz = dims
    flags = util.make_flags(*dims, seed, empty_top=not crowds)
    pos, pflag, pvel = util.make_particles(flags, per_cell, seed + 1)        # shuffled, border particles, 2 % deleted
    m = 200
    z = (lambda k: rng.uniform(0.0, sz - 1e-3, k)) if sz > 1 else (lambda k: np.full(k, 0.5))
    edge = [np.stack([rng.uniform(0.0, 0.5, m), rng.uniform(0.0, sy - 1e-3, m), z(m)], 0),
            np.stack([rng.uniform(sx - 1.0, sx - 1e-3, m), rng.uniform(0.0, sy - 1e-3, m), z(m)], 0)]
    crowd = [np.array(c, np.float64)[:, None] + rng.uniform(0.0, 1.0, (3, k)) for c, k in crowds]
    extra = np.concatenate(edge + crowd, axis=1).astype(np.float32)
    ev = rng.normal(0, 0.5, extra.shape).astype(np.float32)
    if sz == 1:
        ev[2] = 0
    pos, pvel = np.concatenate([pos, extra], axis=1), np.concatenate([pvel, ev], axis=1)
    pflag = np.concatenate([pflag, np.zeros(extra.shape[1], np.int32)])
    n = pos.shape[1]
    perm = rng.permutation(n)
    ptype = rng.choice(np.array([1, 4, 1], np.int32), n).astype(np.int32)
    return Input(name, dims, pos[:, perm], pflag[perm], pvel[:, perm], ptype)


def _cell_sorted(inp):
    sx, sy, _ = inp.dims
    c = inp.pos.astype(np.int64)
    return inp.permuted(inp.name + "-sorted", np.argsort((c[2] * sy + c[1]) * sx + c[0], kind="stable"))


CROWDS_BIG = (((7, 6, 5), 6000), ((8, 6, 5), 700))
CROWDS_RANDOM = (((7, 6, 5), 6000), ((8, 6, 5), 700), ((7, 7, 5), 300), ((12, 3, 9), 40), ((1, 1, 1), 5000))   # test_ordered_p2g_crowded_cells

DYADIC = ("d3", "d3-shuffled", "d2", "d2-shuffled", "hits", "patterns")
RANDOM = ("r3", "r3-sorted", "r2", "crowded")


@functools.lru_cache(maxsize=None)
def get(name):
    if name == "d3":          # bulk cell-ordered, then a 6000- and a 700-particle cell, then 500 particles all over the grid
        return _dyadic(name, (40, 33, 27), 91, 8, (((20, 8, 13), 6000), ((21, 8, 13), 700)), 500, False)
    if name == "d3-shuffled":
        return _shuffled(get("d3"), 92)
    if name == "d2":
        return _dyadic(name, (96, 80, 1), 93, 8, (((40, 20, 0), 6000), ((41, 20, 0), 700)), 500, False)
    if name == "d2-shuffled":
        return _shuffled(get("d2"), 94)
    if name == "hits":        # every cell of the grid, border cells included, 16 each, in memory order; crowded cells at the end
        return _dyadic(name, (20, 16, 12), 95, 16, CROWDS_BIG, 0, True)
    if name == "patterns":
        return _pattern_input()
    if name == "r3":
        return _random(name, (40, 33, 27), 101, 4)
    if name == "r3-sorted":
        return _cell_sorted(get("r3"))
    if name == "r2":
        return _random(name, (96, 80, 1), 103, 4)
    if name == "crowded":
        return _random(name, (20, 16, 12), 105, 3, CROWDS_RANDOM)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def distinct_per_block(name):
    """number of distinct face addresses that each block of 256 consecutive particles of input `name` touches (k_p2g_mac_lds's
    table load)"""
    inp = get(name)
    a = inp.mac["addr"]
    return np.array([np.unique(a[i:i + BLOCK][a[i:i + BLOCK] >= 0]).size for i in range(0, inp.np, BLOCK)])


# ---- running an implementation of the ABI (util.Impl: the oracle on the host, the HIP library on the GPU) ------------------------------
def _garbage(impl, n, seed):
    return impl.dev(util.rand_real((n,), seed, 3.0))     # outputs start dirty: clearing them is the entry point's job


def _pargs(impl, inp, m):
    m = inp.np if m is None else m
    return (m, inp.np) + tuple(impl.dev(a.copy()) for a in (inp.pos, inp.pflag, inp.pvel, inp.ptype))     # the inputs stay read-only


def run_mac_accum(impl, inp, m=None):
    """mf_map_parts_to_mac_accum on the first m particles (stride = all of them), atomic mode -> raw (vel, weight)"""
    sx, sy, sz = inp.dims
    n3 = 3 * sx * sy * sz
    m, ps, pos, pflag, pvel, ptype = _pargs(impl, inp, m)
    vel, w = _garbage(impl, n3, 1), _garbage(impl, n3, 2)
    impl.call("mf_map_parts_to_mac_accum", sx, sy, sz, vel, w, m, ps, pos, pflag, pvel, ptype, EXCLUDE, 0, None)
    impl.sync()
    return impl.host(vel), impl.host(w)


def run_mac(impl, inp, m=None, deterministic=0):
    """mf_map_parts_to_mac, atomic mode (or the ordered one: deterministic=1) -> finished (vel, velOld, weight)"""
    sx, sy, sz = inp.dims
    n3 = 3 * sx * sy * sz
    m, ps, pos, pflag, pvel, ptype = _pargs(impl, inp, m)
    vel, vo, w = _garbage(impl, n3, 1), _garbage(impl, n3, 3), _garbage(impl, n3, 2)
    impl.call("mf_map_parts_to_mac", sx, sy, sz, vel, vo, w, m, ps, pos, pflag, pvel, ptype, EXCLUDE, deterministic, None)
    impl.sync()
    return impl.host(vel), impl.host(vo), impl.host(w)


def run_cell(impl, inp, ncomp, m=None, deterministic=0):
    """mf_map_parts_to_grid, atomic mode (or the ordered one: deterministic=1) -> (divided target, raw weight sums)"""
    sx, sy, sz = inp.dims
    n = sx * sy * sz
    m, ps, pos, pflag, pvel, _ = _pargs(impl, inp, m)
    tgt, w = _garbage(impl, ncomp * n, 4), _garbage(impl, n, 5)
    impl.call("mf_map_parts_to_grid", sx, sy, sz, ncomp, tgt, w, m, ps, pos, pflag, pvel, deterministic, None)      # ncomp 1 reads pvel's x row
    impl.sync()
    return impl.host(tgt), impl.host(w)


@functools.lru_cache(maxsize=None)
def oracle_outputs(name, m=None):
    """the oracle's serial scatter on input `name` (first m particles): computed once, shared, read-only"""
    impl, inp = util.Impl("oracle"), get(name)
    out = {}
    out["acc_vel"], out["acc_weight"] = run_mac_accum(impl, inp, m)
    out["vel"], out["velOld"], out["weight"] = run_mac(impl, inp, m)
    for nc in (1, 3):
        out["target%d" % nc], out["wtmp%d" % nc] = run_cell(impl, inp, nc, m)
    for a in out.values():
        a.setflags(write=False)
    return out


P2G_KEYS = ("p2g_vel", "p2g_velOld", "p2g_weight", "p2g_real", "p2g_vec3")


def run_plugins(inp, deterministic):
    """mapPartsToMAC / mapPartsToGrid / mapPartsToGridVec3 through the package (cases.run_flip_pkg) on the active backend"""
    import cases
    flags, vel = util.make_flags(*inp.dims, 7), util.rand_vel(*inp.dims, 8)
    r = cases.run_flip_pkg(inp.dims, flags, vel, vel, inp.pos.copy(), inp.pflag.copy(), inp.pvel.copy(), ptype=inp.ptype.copy(),
                           exclude=EXCLUDE, deterministic=deterministic)
    return {k: r[k] for k in P2G_KEYS}


def check_plugins_equal_abi(r, o):
    """the plugins' grids against the serial scatter through the ABI (oracle_outputs)"""
    for k, ref in (("p2g_vel", "vel"), ("p2g_velOld", "velOld"), ("p2g_weight", "weight"), ("p2g_real", "target1"), ("p2g_vec3", "target3")):
        util.assert_bitexact(r[k].ravel(), o[ref], k + " vs the serial scatter")


# ---- the checks both test files share -------------------------------------------------------------------------------------------
def check_sums(got, sums, what):
    """raw sums of any fp32 summation order against the model: the bound per entry, 0 where nothing was added, the one term where
    one was.  Returns the largest used share of the bound (for printing)."""
    got64 = np.asarray(got, np.float64)
    err, bound = np.abs(got64 - sums.S), sums.bound
    bad = np.nonzero(err > bound)[0]
    assert bad.size == 0, "%s: %d entries outside gamma(k-1)*A + u|S|; first %d: got %r, S %r, k %d, error %g > bound %g" % (
        what, bad.size, bad[0], got[bad[0]], sums.S[bad[0]], sums.k[bad[0]], err[bad[0]], bound[bad[0]])
    assert (got64[sums.k == 0] == 0).all(), "%s: an entry that no particle touches is not 0" % what
    one = sums.k == 1
    util.assert_bitexact(np.asarray(got, np.float32)[one], sums.S[one].astype(np.float32), what + " (k = 1)")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))


def check_quotients(got, num, den, stomped_value, what):
    """a divided output against the model: the propagated bound where the weight is >= 1e-3, exactly the stomped value (0, or the
    undivided sum within its own bound when stomped_value is None) where the weight is below the threshold in any order"""
    q, qb, divided, stomped, _ = M.quotient_classes(num, den)
    got64 = np.asarray(got, np.float64)
    err = np.abs(got64 - q)
    bad = np.nonzero(divided & (err > qb))[0]
    assert bad.size == 0, "%s: %d quotients outside the propagated bound; first %d: got %r, q %r, error %g > %g" % (
        what, bad.size, bad[0], got[bad[0]], q[bad[0]], err[bad[0]], qb[bad[0]])
    if stomped_value is None:
        assert (np.abs(got64 - num.S)[stomped] <= num.bound[stomped]).all(), what + ": a stomped entry is not its undivided sum"
    else:
        assert (got64[stomped] == stomped_value).all(), what + ": a stomped entry is not %r" % stomped_value


def left_out_share(num, den):
    *_, left = M.quotient_classes(num, den)
    return float(left[num.k > 0].mean())

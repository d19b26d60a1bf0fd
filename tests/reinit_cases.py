"""Inputs of the reinitMarching sweep (tests/test_reinit_cases.py on the CPU, tests/test_gpu_reinit_sweep.py on the GPU,
tools/reinit_host_check.py --sweep on the host bodies) and the predicates that assert what each input reaches.

  * SWEEP: reinit_model.random_case(q) for q < 240 -- the model's own generator, up to 10x9x8 cells, from smooth to sigma 1.0, both outward
    seedings, with and without transport and walls.
  * DESIGNED: families of fields built to hit one structure of csrc/reinit.hip each.  `plane`: whole planes of exactly equal keys, which
    only the index tie-break of `precedes` orders (offset 0: values +-0.5, +-1.5, ...; offset 0.5: integers and one plane of exact 0.0).
    `box`: flat faces, edges and corners of equal keys.  `zeros`: +0.0 and -0.0 scattered over the interface.  `far1000`: a far field of
    +-1000.  `halfint`: a sphere rounded to halves.  `eighths`: an off-centre sphere rounded to multiples of 1/8, so that keys sit exactly
    on a window's end (T + DELTA), with maxTime below one cell (0.5), the default (4) and beyond the grid (1000).
    Every family runs on 9x8x7 and 12x9x1 in three variants: `default` (correctOuterLayer, no walls), `inner` (correctOuterLayer=False) and
    `walls` (ignoreWalls with an obstacle box).  The planes also run on the one-cell-wide 65x3x3 (across x) and 3x3x70 (across z).  `box`,
    `zeros` and `eighths` at maxTime 1000 also run on 20x18x16, where the list holds more than four blocks of entries, and `eighths` at
    maxTime 0.5 as the short march on that grid.

`run(case, mode)` is reinit_model.call with the popped cells and their keys recorded per march; results are computed once per process."""
import functools

import numpy as np

import reinit_model as M

f32 = np.float32
SWEEP = range(240)
D3, D2, BIG = (9, 8, 7), (12, 9, 1), (20, 18, 16)
LONG_X, LONG_Z = (65, 3, 3), (3, 3, 70)
VARIANTS = ("default", "inner", "walls")
BLOCK = 256                     # csrc/common.h


# ---- fields ---------------------------------------------------------------------------------------------------------------------------
def plane(dims, axis, offset):
    """cell-centre coordinate along `axis` minus (dims[axis] // 2 + offset)"""
    return (M.centres(dims)[axis] - (dims[axis] // 2 + offset)).astype(f32).reshape(-1)


def box(dims):
    sx, sy, sz = dims
    return M.box(dims, (2, 2, 2 if sz > 1 else 0), (sx - 2, sy - 2, sz - 2 if sz > 1 else 1))


def ball(dims):
    return M.make_phi("centred", dims, 0)


def zeros(dims):
    phi, r = ball(dims).copy(), np.random.default_rng(3).random(int(np.prod(dims)))
    near = np.abs(phi) < 0.6
    phi[near & (r < 0.3)] = 0.0
    phi[near & (r > 0.7)] = -0.0
    return phi


def far1000(dims):
    phi = ball(dims).copy()
    far = ball(dims)
    phi[far > 1.5] = 1000.
    phi[far < -1.5] = -1000.
    return phi


def halfint(dims):
    return (np.round(2. * ball(dims).astype(np.float64)) / 2.).astype(f32)


def eighths(dims):
    return (np.round(8. * M.make_phi("off", dims, 0).astype(np.float64)) / 8.).astype(f32)


# family -> (field, maxTime, what the reach predicate looks for)
FAMILIES = {
    "plane_x0": (lambda d: plane(d, 0, 0.), 4.0, ("plane", 0)), "plane_x5": (lambda d: plane(d, 0, 0.5), 4.0, ("plane", 0)),
    "plane_y0": (lambda d: plane(d, 1, 0.), 4.0, ("plane", 1)), "plane_y5": (lambda d: plane(d, 1, 0.5), 4.0, ("plane", 1)),
    "plane_z0": (lambda d: plane(d, 2, 0.), 4.0, ("plane", 2)), "plane_z5": (lambda d: plane(d, 2, 0.5), 4.0, ("plane", 2)),
    "box": (box, 4.0, None), "zeros": (zeros, 4.0, ("zeros",)), "far1000": (far1000, 6.0, None), "halfint": (halfint, 4.0, None),
    "eighths_t05": (eighths, 0.5, ("eighths",)), "eighths_t4": (eighths, 4.0, ("eighths",)), "eighths_t1000": (eighths, 1000.0, ("eighths",)),
}
EVERYWHERE = ("plane_x0", "plane_x5", "plane_y0", "plane_y5", "box", "zeros", "far1000", "halfint", "eighths_t05", "eighths_t4", "eighths_t1000")


def _designed():
    out = {}

    def add(family, dims, variant="default"):
        out["%s-%dx%dx%d-%s" % ((family,) + tuple(dims) + (variant,))] = (family, dims, variant)
    for variant in VARIANTS:
        for dims in (D3, D2):
            for family in EVERYWHERE:
                add(family, dims, variant)
    for family in ("plane_z0", "plane_z5"):
        add(family, D3)
        add(family, LONG_Z)
    for family in ("plane_x0", "plane_x5"):
        add(family, LONG_X)
    for family in ("box", "zeros", "eighths_t1000", "eighths_t05"):     # the last: a short list on the grid of the long ones
        add(family, BIG)
    return out


DESIGNED = _designed()


@functools.lru_cache(maxsize=None)
def designed(name):
    """the inputs of a designed case, with the keys of reinit_model.case"""
    family, dims, variant = DESIGNED[name]
    field, maxTime, reach = FAMILIES[family]
    n = int(np.prod(dims))
    phi = np.ascontiguousarray(field(dims), f32)
    flags = M.domain_flags(dims, phi)
    if variant == "walls":
        flags = M.obstacle_box(dims, flags, M.OBSTACLE)
    return dict(name=name, family=family, dims=dims, variant=variant, reach=reach, n=n, phi=phi, flags=flags,
                velocity=np.random.default_rng(7).standard_normal(3 * n).astype(f32), maxTime=maxTime, ignoreWalls=variant == "walls",
                correctOuterLayer=variant != "inner", obstacleType=M.OBSTACLE)


@functools.lru_cache(maxsize=None)
def sweep(q):
    c = M.random_case(q)
    c.update(name="sweep%d" % q, n=int(np.prod(c["dims"])))
    return c


def get(name):
    return sweep(name) if isinstance(name, int) else designed(name)


# ---- the model, with the pops recorded ------------------------------------------------------------------------------------------------
class Recording(M.March):
    """reinit_model.March that notes (cell, key) of every pop of the statement that stands in the end"""

    def pop(self, c, push):
        self.popped.append((c, self.key[c]))
        M.March.pop(self, c, push)

    def serial(self, outer):
        self.popped = []                 # the pops of a flagged march in rounds are undone
        return M.March.serial(self, outer)


@functools.lru_cache(maxsize=None)
def run(name, mode):
    """reinit_model.call on a case (the same passes in the same order), plus "popped": per direction the (cell, key) of every pop"""
    c = get(name)
    p = [float(x) for x in c["phi"]]
    fl = [int(x) for x in c["flags"]]
    v = None if c["velocity"] is None else [float(x) for x in c["velocity"]]
    fm, key, cnt, stats, popped = [-1] * c["n"], [float("nan")] * c["n"], M.new_counters(), {}, []
    maxTime = M.F(c["maxTime"])
    for d in (-1, 1):
        m = Recording(c["dims"], p, fm, key, fl, v, maxTime, d, c["ignoreWalls"], c["obstacleType"], cnt)
        m.popped = []
        m.init_fm()
        outer = d > 0 and bool(c["correctOuterLayer"])
        st = m.serial(outer) if mode == "serial" else m.rounds(outer)
        for k, x in st.items():
            stats.setdefault(k, []).append(x)
        popped.append(m.popped)
        m.set_uninitialized(M.F(-maxTime - 1.) if d < 0 else M.F(maxTime + 1.))
    return {"phi": np.array(p, f32), "vel": None if v is None else np.array(v, f32), "fm": np.array(fm, np.int32), "key": np.array(key, f32),
            "stats": {k: tuple(x) for k, x in stats.items()}, "popped": popped}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def first_difference(want, got):
    """None when the arrays agree bit for bit, else (flat index, wanted, got) of the first cell that differs"""
    bad = np.flatnonzero(bits(np.asarray(want)) != bits(np.asarray(got, np.asarray(want).dtype)))
    return None if bad.size == 0 else (int(bad[0]), np.asarray(want)[bad[0]].item(), np.asarray(got)[bad[0]].item())


def verdict(name):
    """which marches the model redoes serially: (inward, outward)"""
    return run(name, "rounds")["stats"]["serial"]


# ---- reach predicates -----------------------------------------------------------------------------------------------------------------
def plane_cells(dims, axis):
    """interior cells of one plane across `axis`"""
    ext = [s - 2 if s > 1 else 1 for s in dims]
    return int(np.prod(ext)) // ext[axis]


def most_equal_keys(name):
    """the largest number of popped cells of one march that share one key"""
    best = 0
    for march in run(name, "serial")["popped"]:
        if march:
            best = max(best, int(np.unique(bits(np.array([t for _, t in march], f32)), return_counts=True)[1].max()))
    return best


def pairs_one_window_apart(name):
    """adjacent pairs of popped cells of one march whose keys differ by exactly DELTA"""
    c, pairs = get(name), 0
    sx, sy, sz = c["dims"]
    for march in run(name, "serial")["popped"]:
        key = np.full(c["n"], np.nan)
        for cell, t in march:
            key[cell] = t
        key = key.reshape(sz, sy, sx)
        for axis in range(3):
            a, b = np.moveaxis(key, axis, 0)[1:], np.moveaxis(key, axis, 0)[:-1]
            with np.errstate(invalid="ignore"):
                pairs += int((np.abs(a - b) == M.DELTA).sum())
    return pairs


def signed_zeros(name):
    """interior input cells that are (+0.0 inside, +0.0 outside, -0.0 inside, -0.0 outside) the sphere the field was cut from"""
    c = get(name)
    sx, sy, sz = c["dims"]
    side = ball(c["dims"])
    inner = np.zeros((sz, sy, sx), bool)
    inner[(slice(1, -1) if sz > 1 else slice(None)), 1:-1, 1:-1] = True
    inner, zero, minus = inner.reshape(-1), c["phi"] == 0., np.signbit(c["phi"])
    return tuple(int((inner & zero & (minus == m) & ((side < 0) == s)).sum()) for m in (False, True) for s in (True, False))


def reaches(name):
    """the reach predicate of a designed case: (holds, what was counted)"""
    c = designed(name)
    pops = run(name, "serial")["stats"]["pops"]
    if c["reach"] is None:
        return sum(pops) > 0, "pops %s" % (pops,)
    if c["reach"][0] == "plane":
        # a whole plane of equal keys; an obstacle box takes cells out of some planes, so there sx - 2 cells of one key have to do
        got, want = most_equal_keys(name), plane_cells(c["dims"], c["reach"][1])
        if c["variant"] == "walls":
            want = min(want, c["dims"][0] - 2)
        return got >= want and sum(pops) > 0, "%d popped cells share a key, %d asked; pops %s" % (got, want, pops)
    if c["reach"][0] == "eighths":
        got = pairs_one_window_apart(name)
        return got > 0, "%d adjacent popped pairs whose keys differ by DELTA" % got
    got = signed_zeros(name)
    return min(got) > 0, "(+0 inside, +0 outside, -0 inside, -0 outside) = %s" % (got,)


def longest_list(name):
    """a lower bound of the device list's length: every popped cell was an entry"""
    return max(run(name, "serial")["stats"]["pops"])

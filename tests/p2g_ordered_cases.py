"""Seeded inputs of the ordered particle->grid tests (tests/test_p2g_ordered_model.py on the CPU, tests/test_gpu_p2g_ordered.py on the
GPU), one set per structure of csrc/p2g_ordered.hip, and the predicates (p2g_ordered_model) that assert what each input reaches.

Every structure is planted in its own box of the grid (a Region: label + box of nodes), so that the nodes of a bit difference name
the structure.  Two families, as in p2g_cases: `dyadic` (quarter-cell offsets, values multiples of 1/2: a lost, doubled or misrouted
contribution shows in any order) and `random` (jittered positions, normal values: the order of summation shows).

Planted particles are active at every entry point, so the planted counts hold for the MAC entries (ptype & 4 excluded) and the
cell-centred ones (no exclusion) alike.  On top come 2 % deleted particles inside the planted cells and excluded particles in
`background` cells away from the structures (a third of the bulk inputs; fewer where the planted counts already use up the size that
keeps the serial oracle to a second)."""
import collections
import functools

import numpy as np

import p2g_cases as C
import p2g_model as M
import p2g_ordered_model as O
import util

EXCLUDE = C.EXCLUDE
FAMILIES = ("dyadic", "random")
Region = collections.namedtuple("Region", "label lo hi order_shows")       # nodes lo..hi (inclusive) per axis


class Input(C.Input):
    def __init__(self, name, dims, pos, pflag, pvel, ptype, family, regions, cp=None, planted=None):
        C.Input.__init__(self, name, dims, pos, pflag, pvel, ptype)
        self.family, self.regions, self.planted = family, tuple(regions), planted or {}
        self.cp = None if cp is None else np.ascontiguousarray(cp, np.float32)         # [3][3][np]: APIC affine rows cpx, cpy, cpz
        self.n = int(np.prod(self.dims))

    def reversed(self):
        r = slice(None, None, -1)
        return Input(self.name + "-reversed", self.dims, self.pos[:, r], self.pflag[r], self.pvel[:, r], self.ptype[r], self.family,
                     self.regions, None if self.cp is None else self.cp[:, :, r], self.planted)

    @functools.cached_property
    def keys_mac(self):
        return O.cell_keys(self.dims, self.pos, self.pflag, self.ptype, EXCLUDE)

    @functools.cached_property
    def keys_cell(self):
        return O.cell_keys(self.dims, self.pos, self.pflag)

    @functools.cached_property
    def counts_mac(self):
        return O.bin_order_fast(self.keys_mac, self.n)[0]

    @functools.cached_property
    def counts_cell(self):
        return O.bin_order_fast(self.keys_cell, self.n)[0]

    def count_at(self, cell, counts=None):
        return int((self.counts_mac if counts is None else counts)[O.flat(self.dims, *cell)])

    def labels_at(self, node_index):
        """labels of the regions that hold the nodes (flat indices inside one plane) -> Counter"""
        sx, sy, _ = self.dims
        i, j, k = node_index % sx, (node_index // sx) % sy, node_index // (sx * sy)
        out = collections.Counter()
        hit = np.zeros(node_index.shape, bool)
        for r in self.regions:
            m = (i >= r.lo[0]) & (i <= r.hi[0]) & (j >= r.lo[1]) & (j <= r.hi[1]) & (k >= r.lo[2]) & (k <= r.hi[2])
            if m.any():
                out[r.label] = int(m.sum())
            hit |= m
        if not hit.all():
            out["outside every planted region"] = int((~hit).sum())
        return out

    def region_mask(self, r, planes):
        """boolean mask over `planes` grids of n nodes each: the nodes of region r"""
        sx, sy, sz = self.dims
        m = np.zeros((sz, sy, sx), bool)
        m[max(r.lo[2], 0):r.hi[2] + 1, max(r.lo[1], 0):r.hi[1] + 1, max(r.lo[0], 0):r.hi[0] + 1] = True
        return np.tile(m.ravel(), planes)


def assert_same(inp, got, ref, what):
    """bit for bit (+0 == -0, as util.assert_bitexact); the message names the structures the differing nodes belong to"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = (util.bits(got) == util.bits(ref)) | ((got == 0) & (ref == 0))
    if same.all():
        return
    bad = np.nonzero(~same)[0]
    first = int(bad[0])
    sx, sy, _ = inp.dims
    node = first % inp.n
    raise AssertionError("%s on %s: %d of %d values differ; first in plane %d at node (%d, %d, %d): %r vs %r; structures of the differing "
                         "nodes: %s" % (what, inp.name, bad.size, got.size, first // inp.n, node % sx, (node // sx) % sy, node // (sx * sy),
                                        got[first], ref[first], dict(inp.labels_at(bad % inp.n))))


# ---- building ----------------------------------------------------------------------------------------------------------------------
class Builder:
    """particles are appended in index order; finish() shuffles them unless the structure needs the order it was given"""

    def __init__(self, dims, family, seed):
        assert family in FAMILIES
        self.dims, self.family, self.rng = tuple(dims), family, np.random.default_rng(seed)
        self.pos, self.dele, self.excl, self.regions, self.groups, self.n = [], [], [], [], [], 0
        self.planted = {}

    def add(self, cells, e=None, deleted=False, excluded=False, upper=False):
        """particles whose BUILD_INDEX base cell is cells[:, q] and whose shifted base is that + e (random e by default); upper: in the
        upper half of the cell that holds them (e = 0).  -> their indices"""
        cells = np.asarray(cells, np.int64).reshape(3, -1)
        m = cells.shape[1]
        e = self.rng.integers(0, 2, (3, m)) if e is None else np.broadcast_to(np.asarray(e, np.int64).reshape(3, -1), (3, m))
        if upper:
            e = np.zeros((3, m), np.int64)
        frac = self.rng.integers(0, 2, (3, m)) * 0.25 if self.family == "dyadic" else self.rng.uniform(0.01, 0.49, (3, m))
        pos = cells + 0.5 + 0.5 * e + frac
        if self.dims[2] == 1:
            pos[2] = 0.5
        self.pos.append(pos.astype(np.float32))
        self.dele.append(np.full(m, bool(deleted)))
        self.excl.append(np.full(m, bool(excluded)))
        idx = np.arange(self.n, self.n + m)
        self.n += m
        return idx

    def crowd(self, cell, count, **kw):
        return self.add(np.repeat(np.array(cell)[:, None], count, axis=1), **kw)

    def region(self, label, lo_cell, hi_cell, order_shows=True):
        """the nodes that particles based in cells lo..hi feed: up to + 2 along a MAC component's own axis"""
        self.regions.append(Region(label, tuple(int(v) for v in lo_cell), tuple(int(v) + 2 for v in hi_cell), order_shows))

    def deleted_extras(self, frac=0.02):
        """deleted particles inside the cells planted so far: they are skipped, and the planted counts stay"""
        allpos = np.concatenate(self.pos, axis=1)
        k = max(2, int(frac * self.n))
        pick = self.rng.integers(0, self.n, k)
        self.pos.append(allpos[:, pick].copy())
        self.dele.append(np.ones(k, bool))
        self.excl.append(np.zeros(k, bool))
        self.n += k

    def background(self, lo, hi, per, label="background", order_shows=True):
        """excluded particles (ptype & 4), `per` in every cell of lo..hi: skipped by the MAC entries, binned by the cell-centred ones"""
        g = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij"), 0).reshape(3, -1)
        self.add(np.repeat(g, per, axis=1), excluded=True)
        self.region(label, lo, hi, order_shows)

    def finish(self, name, order="shuffle", cp=False):
        pos, dele, excl = np.concatenate(self.pos, axis=1), np.concatenate(self.dele), np.concatenate(self.excl)
        n, rng = self.n, self.rng
        pvel = C._dyadic_values(rng, n) if self.family == "dyadic" else rng.normal(0, 0.5, (3, n)).astype(np.float32)
        cpv = None
        if cp:
            cpv = (rng.integers(-2, 3, (3, 3, n)) / 2.0 if self.family == "dyadic" else rng.normal(0, 0.3, (3, 3, n))).astype(np.float32)
        pflag = np.where(dele, M.PDELETE, 0).astype(np.int32)
        pflag[rng.random(n) < 0.05] |= 1          # PNEW: must not matter
        ptype = np.where(excl, EXCLUDE, 1).astype(np.int32)
        if order == "shuffle":
            dest = rng.permutation(n)             # particle i goes to index dest[i]; the groups keep the order they were planted in
            for g in self.groups:
                dest[g] = np.sort(dest[g])
            perm = np.argsort(dest)
            pos, pflag, pvel, ptype = pos[:, perm], pflag[perm], pvel[:, perm], ptype[perm]
            cpv = None if cpv is None else cpv[:, :, perm]
        else:
            assert order == "keep"
        return Input(name, self.dims, pos, pflag, pvel, ptype, self.family, self.regions, cpv, self.planted)


def _wrap(inp, family, regions, cp_seed=None):
    cp = None
    if cp_seed is not None:
        rng = np.random.default_rng(cp_seed)
        cp = (rng.integers(-2, 3, (3, 3, inp.np)) / 2.0 if family == "dyadic" else rng.normal(0, 0.3, (3, 3, inp.np))).astype(np.float32)
    return Input(inp.name, inp.dims, inp.pos, inp.pflag, inp.pvel, inp.ptype, family, regions, cp)


# ---- S1 runs64: key sequences over 64-lane waves, in a chosen index order ---------------------------------------------------------------
RUNS_DIMS = (12, 10, 9)
RUNS_PREFIXES = (1, 63, 64, 65, 255, 256, 257)


def _runs64(family):
    b = Builder(RUNS_DIMS, family, 201)
    cells = np.stack(np.meshgrid(np.arange(1, 10), np.arange(1, 8), np.arange(1, 7), indexing="ij"), 0).reshape(3, -1)
    cells = cells[:, b.rng.permutation(cells.shape[1])]
    cursor = [0]

    def fresh():
        cursor[0] += 1
        return cursor[0] % cells.shape[1]

    seq = []            # (cell, deleted, excluded) per particle, in index order

    def run(c, k, deleted=False, excluded=False):
        seq.extend([(c, deleted, excluded)] * k)

    def fill(k, excluded_middle=False):
        while k > 0:
            c, m = fresh(), min(3, k)
            if excluded_middle and m == 3:
                run(c, 1), run(c, 1, excluded=True), run(c, 1)
            else:
                run(c, m)
            k -= m

    for rep in range(2):
        assert len(seq) == rep * 640
        run(fresh(), 64)                                                  # wave 0: one run of 64
        for _ in range(64):                                               # wave 1: runs of 1
            run(fresh(), 1)
        fill(54), run(fresh(), 10)                                        # wave 2: a run ending at lane 63
        d = fresh()
        fill(60), run(d, 4)                                               # wave 3 | 4: a run crossing the wave (rep 0: the block of 256)
        run(d, 6), fill(58)
        g = fresh()
        fill(61), run(g, 3)                                               # wave 5 | 6: a run crossing the wave (rep 1: the block of 256)
        run(g, 2), fill(60), run(fresh(), 1), run(fresh(), 1)             # wave 6 ends with a run that starts at lane 63
        f, h, x = fresh(), fresh(), fresh()                               # wave 7: skipped particles inside runs
        run(f, 3), run(f, 1, deleted=True), run(f, 2)
        run(h, 3), run(h, 4, deleted=True), run(h, 3)
        run(x, 2), run(x, 3, excluded=True), run(x, 2)
        fill(41)
        fill(54), run(fresh(), 10)                                        # wave 8: a run ending at lane 63
        fill(63, excluded_middle=True), run(fresh(), 1)                   # wave 9: excluded lanes; a run that starts at lane 63
    run(fresh(), 23)                                                      # a last wave partly past np
    for c, dele, excl in seq:
        b.add(cells[:, c:c + 1], deleted=dele, excluded=excl, upper=True)
    b.region("runs64", (0, 0, 0), RUNS_DIMS)
    return b.finish("runs64-" + family, order="keep")


def reach_runs64(inp):
    for keys in (inp.keys_mac, inp.keys_cell):
        found = O.run_shapes(keys, inp.n)
        for s in O.SHAPES:
            assert found[s] >= (1 if s == "partial_wave" else 2), (inp.name, s, found)
    assert 1250 <= inp.np <= 1350 and inp.np > max(RUNS_PREFIXES)
    e = O.e_bits(inp.dims, inp.pos)
    assert (e == 0).all(), "upper-half positions: every component shares the key pattern"
    for m in RUNS_PREFIXES:     # what the prefixes are for: one lane, a wave less / plus one lane, a block less / plus one lane
        assert m in (1, O.WAVE - 1, O.WAVE, O.WAVE + 1, O.BLOCK - 1, O.BLOCK, O.BLOCK + 1)


# ---- S2 scan: n + 1 at the edges of a scan block, and the second round of k_scan_top ------------------------------------------------------
SCAN_DIMS = ((65, 63, 1), (64, 64, 1), (16, 16, 16), (1040, 1010, 1))


def _reachable(dims, f):
    sx, sy, sz = dims
    x, y, z = f % sx, (f // sx) % sy, f // (sx * sy)
    return x <= sx - 2 and y <= sy - 2 and z <= max(sz - 2, 0) and f >= 0


def _scan(dims, family):
    sx, sy, sz = dims
    n = sx * sy * sz
    b = Builder(dims, family, 211 + sx)
    last = O.flat(dims, sx - 2, sy - 2, max(sz - 2, 0))                  # the highest base cell a position can have
    targets = {"first scan block": [0, 1, sx + 2], "highest base cell": [last - 1, last]}
    for k in sorted(set(k for k in (1, 2, 128, 255, 256) if k < O.scan_blocks(n))):
        t = [f for f in (k * O.SCAN_BLOCK - 2, k * O.SCAN_BLOCK - 1, k * O.SCAN_BLOCK, k * O.SCAN_BLOCK + 1) if _reachable(dims, f) and f < last - 1]
        if t:
            targets["scan blocks %d | %d" % (k - 1, k)] = t
    planted = {}
    for label, fl in targets.items():
        fl = np.array(fl)
        c = np.stack([fl % sx, (fl // sx) % sy, fl // (sx * sy)], 0)
        for q in range(c.shape[1]):
            b.crowd(c[:, q], 3 + q)
        b.region(label, c.min(1), c.max(1))
        planted[label] = fl
    b.planted = planted
    b.deleted_extras()
    y0 = sy // 2
    b.background((10, y0, 0), (12, y0, 0), max(2, b.n // 6))
    return b.finish("scan-%dx%dx%d-%s" % (sx, sy, sz, family))


def reach_scan(inp):
    n = inp.n
    want = {(65, 63, 1): (4096, 1), (64, 64, 1): (4097, 2), (16, 16, 16): (4097, 2), (1040, 1010, 1): (1050401, 257)}[inp.dims]
    assert (n + 1, O.scan_blocks(n)) == want
    if want[1] == 2:
        assert (n + 1) - O.SCAN_BLOCK == 1, "the second scan block holds start[n] alone"
    for counts in (inp.counts_mac, inp.counts_cell):
        blocks = set((np.nonzero(counts)[0] // O.SCAN_BLOCK).tolist())
        assert 0 in blocks
        for label, fl in inp.planted.items():
            assert (counts[fl] >= 3).all(), (inp.name, label)
        if want[1] == 257:
            assert {254, 255, 256} <= blocks, blocks
            assert O.scan_blocks(n) > O.BLOCK, "k_scan_top takes a second round"
            for k in (1, 2, 128, 255, 256):      # the last entry of a scan block and the first of the next both hold particles
                assert counts[k * O.SCAN_BLOCK - 1] > 0 and counts[k * O.SCAN_BLOCK] > 0, k
            sx, sy, _ = inp.dims
            assert counts[O.flat(inp.dims, sx - 2, sy - 2, 0)] > 0, "highest base cell"


# ---- S3 sorts: every size boundary of the two sort kernels, and more crowded cells than workgroups --------------------------------------
SORT_DIMS = (20, 16, 12)
SORT_SIZES = ((2, (12, 2, 2)), (32, (15, 2, 2)), (33, (18, 2, 2)), (64, (12, 6, 2)), (65, (15, 6, 2)), (4096, (18, 6, 2)),
              (4097, (12, 10, 2)), (6000, (15, 10, 2)), (4097, (18, 10, 2)), (4097, (12, 13, 7)), (4097, (15, 13, 7)), (4097, (18, 13, 7)),
              (4097, (12, 6, 7)))
SORT_BULK = ((0, 0, 0), (8, 8, 6))           # 9 x 9 x 7 = 567 cells with 33..40 particles


def _sorts(family):
    b = Builder(SORT_DIMS, family, 221)
    for count, cell in SORT_SIZES:
        b.crowd(cell, count)
        b.region("cell of %d at %r" % (count, cell), cell, cell, order_shows=count > 2)     # a sum of two terms has one order
    g = np.stack(np.meshgrid(*[np.arange(a, c + 1) for a, c in zip(*SORT_BULK)], indexing="ij"), 0).reshape(3, -1)
    per = b.rng.integers(SORT_SIZES[2][0], 41, g.shape[1])
    b.add(np.repeat(g, per, axis=1))
    b.region("bulk of 33..40 per cell", *SORT_BULK)
    b.deleted_extras()
    b.background((0, 12, 9), (9, 14, 10), 8)
    return b.finish("sorts-" + family)


def reach_sorts(inp):
    for counts in (inp.counts_mac, inp.counts_cell):
        for count, cell in SORT_SIZES:
            assert inp.count_at(cell, counts) == count, (cell, count)
        big = counts[counts > O.SMALL_RUN]
        assert sorted(set(big.tolist()) - set(range(33, 41))) == [64, 65, 4096, 4097, 6000]
        assert ((big >= 33) & (big <= 40)).sum() >= 2 * O.BIG_BLOCKS + 1, "every workgroup of k_bin_sort_big loops"
        assert big.size > 2 * O.BIG_BLOCKS and (big == 4097).sum() >= 5
        routes = collections.Counter(O.sort_route(int(c)) for c in counts[counts > 0])
        assert routes["insertion"] >= 2 and routes["bitonic"] >= 516 and routes["rank"] >= 6, routes
    assert O.sort_route(32) == "insertion" and O.sort_route(33) == "bitonic" and O.sort_route(4096) == "bitonic" and O.sort_route(4097) == "rank"
    assert O.bitonic_size(64) == 64 and O.bitonic_size(65) == 128 and O.bitonic_size(4096) == 4096      # unpadded, padded, full
    assert 4097 - O.BIG_LDS == 1, "the last tile of the rank counting holds one entry"
    assert inp.np <= 60000


# ---- S4 wcap: the LDS / fallback choice of k_gather_wave and rows longer than the wave ----------------------------------------------------
# One input per structure (exactly WCAP, WCAP + 1, long rows), each planted in an interior tile, the low-corner tile (x0, y0, z0 < 0:
# the rows start xin cells in) and the high-corner tile: 6 x 5 x 4 tiles leave two positions per axis that are 8 cells apart, so the
# nine tiles cannot share one grid.  The edges of this grid are multiples of the tile, so the high corner's neighbourhood ends with
# the grid (its last cell, s - 1, can hold no base cell); neighbourhoods that stick out are S6's (17, 11, 9) and (5, 4, 3).
WCAP_DIMS = (24, 20, 16)
WCAP_TILES = (("interior", (3, 1, 1)), ("low corner", (0, 0, 0)), ("high corner", (5, 4, 3)))
WCAP_KINDS = ("1536", "1537", "rows")
WCAP_ROWS = (64, 65, 129)


def _common_cells(dims, tile):
    """per axis the cells that every mode's neighbourhood of the tile holds and a position can be based in"""
    return [np.arange(max(4 * t - 1, 0), min(4 * t + 3, s - 2) + 1) for t, s in zip(tile, dims)]


def _spread(total, m):
    return np.full(m, total // m) + (np.arange(m) < total % m)


def _wcap(kind, family):
    b = Builder(WCAP_DIMS, family, 231 + WCAP_KINDS.index(kind))
    for where, tile in WCAP_TILES:
        X, Y, Z = _common_cells(WCAP_DIMS, tile)
        if kind == "rows":
            for length, (y, z) in zip(WCAP_ROWS, ((Y[0], Z[0]), (Y[2], Z[1]), (Y[-1], Z[-1]))):
                for x, k in zip(X, _spread(length, X.size)):
                    b.crowd((x, y, z), int(k))
        else:
            g = np.stack(np.meshgrid(X, Y, Z, indexing="ij"), 0).reshape(3, -1)
            per = _spread(int(kind), g.shape[1])
            assert per.max() <= 32
            b.add(np.repeat(g, per, axis=1))
        b.region("%s tile %r (%s)" % (where, tile, kind), (X[0], Y[0], Z[0]), (X[-1], Y[-1], Z[-1]))
    b.deleted_extras()
    b.background((0, 15, 0), (3, 17, 2), 12)
    return b.finish("wcap-%s-%s" % (kind, family))


def reach_wcap(inp, kind):
    sx, sy, sz = inp.dims
    for mode in O.MODES:
        counts = inp.counts_cell if mode == 3 else inp.counts_mac
        c3 = counts.reshape(sz, sy, sx)
        for where, tile in WCAP_TILES:
            total, longest, path = O.tile_info(c3, mode, tile)
            rows = O.row_lengths(c3, mode, tile)
            if kind == "rows":
                assert path == "lds" and total == sum(WCAP_ROWS) <= O.WCAP, (mode, where, total, path)
                assert sorted(rows[rows > 0].tolist()) == list(WCAP_ROWS), (mode, where, rows)
                assert WCAP_ROWS[0] == O.GBLOCK and WCAP_ROWS[1] == O.GBLOCK + 1 and WCAP_ROWS[2] == 2 * O.GBLOCK + 1
            else:
                assert total == int(kind) and path == ("lds" if kind == "1536" else "fallback"), (mode, where, total, path)
                assert int(kind) - O.WCAP == (0 if kind == "1536" else 1)
                assert counts.max() <= O.SMALL_RUN or mode == 3
        assert 4 * WCAP_TILES[1][1][0] - O.reach(mode)[0] < 0, "low corner: x0 < 0, the rows start xin cells in"
    # the tiles are at least 8 cells apart
    boxes = [_common_cells(inp.dims, t) for _, t in WCAP_TILES]
    for a in range(3):
        for c in range(a + 1, 3):
            assert max(max(boxes[c][q][0] - boxes[a][q][-1], boxes[a][q][0] - boxes[c][q][-1]) for q in range(3)) >= 8


# ---- S5 links: the dist field of the link words, from the LDS copy, from global memory in the fallback, and in k_gather --------------------
LINK_DIMS_3D, LINK_DIMS_2D = (40, 20, 12), (96, 80, 1)


def link_patterns():
    """e bits of a cell's particles in increasing index: a, b x k, a for k = 0..8 | a, b x 20 | all equal -- for a = 0 and a = 1"""
    out = []
    for a in (0, 1):
        out += [[a] + [1 - a] * k + [a] for k in range(9)] + [[a] + [1 - a] * 20, [a] * 10]
    return out


def _links_plant(b, source, x_off, axes):
    """the patterns of every axis on a lattice of every second cell"""
    slots = [(1 + 2 * i + x_off, 1 + 2 * j, 2 + 2 * k) for k in range(2 if b.dims[2] > 1 else 1) for j in range(9 if b.dims[2] == 1 else 7) for i in range(5)]
    if b.dims[2] == 1:
        slots = [(x, y, 0) for x, y, _ in slots]
    cells = []
    for q, (axis, pat) in enumerate((axis, pat) for axis in axes for pat in link_patterns()):
        cell = slots[q]
        e = b.rng.integers(0, 2, (3, len(pat)))
        e[axis] = pat
        b.groups.append(b.crowd(cell, len(pat), e=e))
        b.planted.setdefault((source, axis), []).append(O.flat(b.dims, *cell))
        cells.append(cell)
    cells = np.array(cells).T
    b.region("link patterns, %s" % source, cells.min(1), cells.max(1))
    return cells


def _links(dims, family):
    b = Builder(dims, family, 241 + dims[0])
    if dims[2] == 1:
        _links_plant(b, "2d", 0, (0, 1))
        b.deleted_extras()
        b.background((40, 40, 0), (50, 44, 0), 4)
        return b.finish("links2d-" + family)
    _links_plant(b, "lds", 0, (0, 1, 2))
    cells = _links_plant(b, "fallback", 20, (0, 1, 2))
    # the tiles that hold a node fed by a fallback pattern; a 1600-particle cell at (4a + 3, 4b + 3, 4c + 3) lies in the neighbourhood
    # of the eight tiles around it in every mode
    tiles = set()
    for c in cells.T:
        tiles |= {tuple(t) for t in np.stack(np.meshgrid(*[np.unique(np.arange(v, v + 3) // 4) for v in c], indexing="ij"), 0).reshape(3, -1).T}
    crowds = {tuple(4 * (v - v % 2) + 3 for v in t) for t in tiles}
    for c in sorted(crowds):
        assert O.flat(dims, *c) not in b.planted[("fallback", 0)] + b.planted[("fallback", 1)] + b.planted[("fallback", 2)]
        b.crowd(c, 1600)
        b.region("1600-particle cell at %r beside the fallback link patterns" % (c,), c, c)
    b.planted["fallback tiles"], b.planted["crowds"] = sorted(tiles), sorted(crowds)
    b.deleted_extras()
    b.background((0, 16, 9), (9, 18, 10), 6)
    return b.finish("links3d-" + family)


def reach_links(inp):
    sx, sy, sz = inp.dims
    e = O.e_bits(inp.dims, inp.pos)
    order, dist, true, after = O.link_dists(inp.keys_mac, e, inp.n)
    cell_of_slot = inp.keys_mac[order]
    sources = ("2d",) if sz == 1 else ("lds", "fallback")
    for source in sources:
        for axis in ((0, 1) if sz == 1 else (0, 1, 2)):
            mine = np.isin(cell_of_slot, inp.planted[(source, axis)])
            for a in (0, 1):        # entries with e = a: each distance 0..7 is written, and the walk has its three outcomes
                sel = mine & (e[axis][order] == a)
                assert set(dist[axis][sel].tolist()) == set(range(8)), (source, axis, a, set(dist[axis][sel].tolist()))
                walks = O.walk_outcomes(dist[axis][sel], true[axis][sel], after[sel])
                for w in O.WALKS:
                    assert walks[w].any(), (source, axis, a, w)
    if sz > 1:
        c3 = inp.counts_mac.reshape(sz, sy, sx)
        for mode in (0, 1, 2):
            table = O.tile_table(inp.dims, inp.counts_mac, mode)
            for t in inp.planted["fallback tiles"]:
                assert table[t][2] == "fallback", (mode, t, table[t])
            lds_cells = np.concatenate([inp.planted[("lds", a)] for a in range(3)])
            for f in lds_cells:
                x, y, z = f % sx, (f // sx) % sy, f // (sx * sy)
                for t in {(i // 4, j // 4, k // 4) for i in (x, x + 2) for j in (y, y + 2) for k in (z, z + 2)}:
                    assert table[t][2] == "lds", (mode, t, table[t])
        assert all(c3[c[2], c[1], c[0]] == 1600 for c in inp.planted["crowds"])


# ---- S6 shapes: the bulk on grids whose edges are, and are not, multiples of the tile ------------------------------------------------------
SHAPE_DIMS = ((12, 10, 9), (17, 11, 9), (5, 4, 3), (6, 5, 2), (16, 16, 16), (20, 16, 12), (24, 18, 1), (33, 7, 1))


def _shapes(dims, family, cp_seed=None):
    name = "shapes-%dx%dx%d-%s" % (dims + (family,))
    seed = 251 + 7 * SHAPE_DIMS.index(dims)
    if family == "dyadic":
        inp = C._shuffled(C._dyadic(name, dims, seed, 8, (), 120, False), seed + 1)
    else:
        inp = C._random(name, dims, seed, 8)
    inp.name = name
    return _wrap(inp, family, [Region("bulk and border particles", (0, 0, 0), dims, True)], cp_seed)


def reach_shapes(inp):
    import cases
    assert cases.SIZE_2D in SHAPE_DIMS
    sx, sy, sz = inp.dims
    act = M.active(inp.pflag, inp.ptype, EXCLUDE)
    assert (act & (inp.pos[0] < 0.5)).sum() >= 5 and (act & (inp.pos[0] >= sx - 1)).sum() >= 5, "border particles in the first and last column"
    assert 0.2 < ((inp.ptype & EXCLUDE) != 0).mean() < 0.45
    assert ((inp.pflag & M.PDELETE) != 0).any() or inp.np < 1000      # 2 % of the bulk; the smallest grids have next to no bulk
    assert O.swizzled((16, 16, 16)) and not O.swizzled((20, 16, 12))
    assert O.tiles_of((33, 7, 1)) == (3, 2, 1) and 33 % (O.GX * O.GZ) != 0 and 7 % O.GY != 0
    if sz > 1 and min(inp.dims) > 6:
        paths = collections.Counter(v[2] for v in O.tile_table(inp.dims, inp.counts_mac, 0).values())
        assert paths["lds"] > 0 and paths["empty"] == 0, paths


# ---- S7 apic: crowded faces ------------------------------------------------------------------------------------------------------------
APIC_CROWDS = ((20, (4, 10, 4)), (33, (4, 4, 4)), (300, (10, 4, 4)), (4097, (16, 4, 4)))
APIC_SPLIT = (4097, (10, 11, 6))


def _apic_crowds(family):
    b = Builder(SORT_DIMS, family, 261)
    for count, cell in APIC_CROWDS:       # upper half of one cell on every axis: the three face keys are the cell
        b.crowd(cell, count, upper=True)
        b.region("face of %d at %r" % (count, cell), cell, cell)
    b.crowd(APIC_SPLIT[1], APIC_SPLIT[0])    # any e: every component splits it over two faces
    b.region("cell of %d at %r over two faces per component" % APIC_SPLIT, APIC_SPLIT[1], APIC_SPLIT[1])
    b.deleted_extras()
    b.background((0, 12, 9), (9, 14, 10), 8, order_shows=False)      # excluded: the APIC entry adds nothing there
    return b.finish("apic-crowds-" + family, cp=True)


def reach_apic(inp):
    if not inp.name.startswith("apic-crowds"):
        keys = [O.apic_keys(inp.dims, inp.pos, inp.pflag, inp.ptype, EXCLUDE, c) for c in range(3)]
        assert any((keys[a] != keys[b]).any() for a, b in ((0, 1), (1, 2), (0, 2))), "the face keys differ per component"
        act = M.active(inp.pflag, inp.ptype, EXCLUDE)
        assert (act & (inp.pos[0] < 0.5)).sum() >= 5 and (act & (inp.pos[0] >= inp.dims[0] - 1)).sum() >= 5, "border particles"
        return
    for comp in range(3):
        keys = O.apic_keys(inp.dims, inp.pos, inp.pflag, inp.ptype, EXCLUDE, comp)
        counts = O.bin_order_fast(keys, inp.n)[0]
        for count, cell in APIC_CROWDS:
            assert counts[O.flat(inp.dims, *cell)] == count, (comp, cell)
        routes = collections.Counter(O.sort_route(int(c)) for c in counts[counts > 0])
        assert routes["bitonic"] >= 4 and routes["rank"] >= 1 and routes["insertion"] >= 1, (comp, routes)
        f = O.flat(inp.dims, *APIC_SPLIT[1])
        off = (1, inp.dims[0], inp.dims[0] * inp.dims[1])[comp]
        assert counts[f] + counts[f + off] == APIC_SPLIT[0] and min(counts[f], counts[f + off]) > 1000


# ---- the table of inputs ----------------------------------------------------------------------------------------------------------------
def _dimname(d):
    return "%dx%dx%d" % d


STRUCTURES = collections.OrderedDict()      # structure -> input names without the family
STRUCTURES["runs64"] = ("runs64",)
STRUCTURES["scan"] = tuple("scan-" + _dimname(d) for d in SCAN_DIMS)
STRUCTURES["sorts"] = ("sorts",)
STRUCTURES["wcap"] = tuple("wcap-" + k for k in WCAP_KINDS)
STRUCTURES["links"] = ("links3d", "links2d")
STRUCTURES["shapes"] = tuple("shapes-" + _dimname(d) for d in SHAPE_DIMS)
STRUCTURES["apic"] = ("apic-crowds", "apic-shapes-17x11x9")
MAC_CELL_NAMES = tuple("%s-%s" % (b, f) for s, bases in STRUCTURES.items() if s != "apic" for b in bases for f in FAMILIES)
APIC_NAMES = tuple("%s-%s" % (b, f) for b in STRUCTURES["apic"] for f in FAMILIES)
ALL_NAMES = MAC_CELL_NAMES + APIC_NAMES


def _dims_of(text):
    return tuple(int(v) for v in text.split("x"))


@functools.lru_cache(maxsize=None)
def get(name):
    base, family = name.rsplit("-", 1)
    if base == "runs64":
        return _runs64(family)
    if base.startswith("scan-"):
        return _scan(_dims_of(base[5:]), family)
    if base == "sorts":
        return _sorts(family)
    if base.startswith("wcap-"):
        return _wcap(base[5:], family)
    if base == "links3d":
        return _links(LINK_DIMS_3D, family)
    if base == "links2d":
        return _links(LINK_DIMS_2D, family)
    if base.startswith("shapes-"):
        return _shapes(_dims_of(base[7:]), family)
    if base == "apic-crowds":
        return _apic_crowds(family)
    if base.startswith("apic-shapes-"):
        inp = _shapes(_dims_of(base[12:]), family, cp_seed=271)
        inp.name = name
        return inp
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reach(name):
    """assert what input `name` was planted for (once per process)"""
    inp, base = get(name), name.rsplit("-", 1)[0]
    assert inp.np <= 61000 and inp.n <= 1.06e6
    if base == "runs64":
        reach_runs64(inp)
    elif base.startswith("scan-"):
        reach_scan(inp)
    elif base == "sorts":
        reach_sorts(inp)
    elif base.startswith("wcap-"):
        reach_wcap(inp, base[5:])
    elif base.startswith("links"):
        reach_links(inp)
    elif base.startswith("shapes-"):
        reach_shapes(inp)
    else:
        reach_apic(inp)
    return True


# ---- running the ABI with deterministic = 1 ---------------------------------------------------------------------------------------------
ENTRIES = ("mac_accum", "mac", "grid1", "grid3")


def run_apic(impl, inp, m=None):
    """mf_apic_map_parts_to_mac -> finished (vel, mass)"""
    sx, sy, sz = inp.dims
    n3 = 3 * sx * sy * sz
    m, ps, pos, pflag, pvel, ptype = C._pargs(impl, inp, m)
    cp = [impl.dev(inp.cp[q].copy()) for q in range(3)]
    vel, mass = C._garbage(impl, n3, 6), C._garbage(impl, n3, 7)
    impl.call("mf_apic_map_parts_to_mac", sx, sy, sz, vel, mass, m, ps, pos, pflag, pvel, cp[0], cp[1], cp[2], ptype, EXCLUDE, None)
    impl.sync()
    return impl.host(vel), impl.host(mass)


def run_mac_accum(impl, inp, m=None):
    sx, sy, sz = inp.dims
    n3 = 3 * sx * sy * sz
    m, ps, pos, pflag, pvel, ptype = C._pargs(impl, inp, m)
    vel, w = C._garbage(impl, n3, 1), C._garbage(impl, n3, 2)
    impl.call("mf_map_parts_to_mac_accum", sx, sy, sz, vel, w, m, ps, pos, pflag, pvel, ptype, EXCLUDE, 1, None)
    impl.sync()
    return impl.host(vel), impl.host(w)


def run_entry(impl, inp, entry, m=None):
    """-> {output name: array} of one entry point, outputs starting dirty"""
    if entry == "mac_accum":
        return dict(zip(("acc_vel", "acc_weight"), run_mac_accum(impl, inp, m)))
    if entry == "mac":
        return dict(zip(("vel", "velOld", "weight"), C.run_mac(impl, inp, m, deterministic=1)))
    if entry in ("grid1", "grid3"):
        nc = int(entry[4])
        return dict(zip(("target%d" % nc, "wtmp%d" % nc), C.run_cell(impl, inp, nc, m, deterministic=1)))
    if entry == "apic":
        return dict(zip(("apic_vel", "apic_mass"), run_apic(impl, inp, m)))
    raise KeyError(entry)


def _oracle_on(inp, entries, m=None):
    impl, out = util.Impl("oracle"), {}
    for entry in entries:
        out.update(run_entry(impl, inp, entry, m))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_outputs(name, m=None, apic=False, backwards=False):
    """the oracle's serial scatter on input `name` (its first m particles; in reversed particle order): computed once, read-only"""
    inp = get(name)
    return _oracle_on(inp.reversed() if backwards else inp, ("apic",) if apic else ENTRIES, m)

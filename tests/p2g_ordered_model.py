"""numpy model of the GEOMETRY of the ordered particle->grid path (csrc/p2g_ordered.hip): which key a particle is binned under, where
the scan puts every cell's run, which link distances k_bin_links writes, which path every gather tile takes and which run shapes a key
sequence shows to run_of.  It models no sums -- those are tests/p2g_model.py's.  tests/p2g_ordered_cases.py uses it to ASSERT that an
input reaches the branch it was planted for; tests/test_p2g_ordered_model.py checks the model itself and that the constants below
are the kernel's.
"""
import re

import numpy as np

import p2g_model as M

# the kernel constants the predicates mirror (test_constants_are_the_kernels reads them back from the sources)
BLOCK = 256                       # common.h
PBITS = 28
SMALL_RUN = 32                    # longest run of k_bin_sort_cells' insertion sort
BIG_LDS = 4096                    # longest run of k_bin_sort_big's bitonic sort; longer runs are rank-counted
SCAN_ITEMS = 16
BIG_BLOCKS = 256                  # workgroups of the k_bin_sort_big launch
GBLOCK, GX, GY, GZ = 64, 4, 4, 4
WCAP = 1536
SCAN_BLOCK = BLOCK * SCAN_ITEMS   # entries of start[] per scan block
WAVE = 64
KERNEL_CONSTANTS = {"p2g_ordered.hip": ("PBITS", "SMALL_RUN", "BIG_LDS", "SCAN_ITEMS", "BIG_BLOCKS", "GBLOCK", "GX", "GY", "GZ", "WCAP"),
                    "common.h": ("BLOCK",)}
# the comparisons the predicates below restate, as they stand in p2g_ordered.hip
KERNEL_PREDICATES = ("if (e - a > SMALL_RUN) {", "if (cnt <= BIG_LDS) {", "if (total > WCAP) {", "dim3(BIG_BLOCKS), dim3(BLOCK)",
                     "a - slot < 7 ? (unsigned)(a - slot) : 7u")


def constants_in(text):
    """every `constexpr int NAME = value` of a source text (also the comma-separated form) -> {NAME: value}"""
    out = {}
    for decl in re.findall(r"constexpr\s+int\s+([^;]+);", text):
        for name, value in re.findall(r"(\w+)\s*=\s*(\d+)\b", decl):
            out[name] = int(value)
    return out


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
def flat(dims, x, y, z):
    return x + dims[0] * (y + dims[1] * z)


def base_cells(dims, pos):
    (bx, by, bz), *_ = M.build_index(dims, np.ascontiguousarray(pos, np.float32), False)
    return bx, by, bz


def cell_keys(dims, pos, pflag, ptype=None, exclude=0):
    """key_of<3>: the flat BUILD_INDEX base cell, n for a particle that is skipped (deleted / excluded)"""
    n = int(np.prod(dims))
    bx, by, bz = base_cells(dims, pos)
    return np.where(M.active(pflag, ptype, exclude), flat(dims, bx, by, bz), n).astype(np.int64)


def apic_face_index(dims, pos, comp):
    """apic_face<comp>().gidx: (IndexInt)pos along the face's own axis, (IndexInt)(pos - 0.5) with the subtraction in double elsewhere,
    flat, unchecked; Z = 0 in 2-D"""
    sx, sy, sz = dims
    b = [np.trunc(pos[q].astype(np.float64) - (0.0 if q == comp else 0.5)).astype(np.int64) for q in range(3)]
    return b[0] + sx * b[1] + (sx * sy if sz > 1 else 0) * b[2]


def apic_keys(dims, pos, pflag, ptype, exclude, comp):
    n = int(np.prod(dims))
    g = apic_face_index(dims, pos, comp)
    ok = M.active(pflag, ptype, exclude) & (g >= 0) & (g < n)
    return np.where(ok, g, n).astype(np.int64)


def e_bits(dims, pos):
    """[3][np]: shifted base (BUILD_INDEX_SHIFT) minus base (BUILD_INDEX) per axis; always 0 or 1"""
    p = np.ascontiguousarray(pos, np.float32)
    b, *_ = M.build_index(dims, p, False)
    s, *_ = M.build_index(dims, p, True)
    e = np.stack([s[q] - b[q] for q in range(3)], 0)
    assert ((e == 0) | (e == 1)).all()
    return e


# ---- counts, start, order -----------------------------------------------------------------------------------------------------------
def bin_order(keys, n):
    """-> counts[n], start[n + 1] (exclusive scan), order[start[n]]: the binned particles, every key's run in increasing particle
    index (counting sort, written out)"""
    keys = np.asarray(keys, np.int64)
    counts = np.zeros(n, np.int64)
    for k in keys[keys < n]:
        counts[k] += 1
    start = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=start[1:])
    cursor, order = start[:-1].copy(), np.empty(start[n], np.int64)
    for p, k in enumerate(keys):
        if k < n:
            order[cursor[k]] = p
            cursor[k] += 1
    return counts, start, order


def bin_order_fast(keys, n):
    """the same, vectorised (test_model_bin_order checks it against bin_order and against np.argsort)"""
    keys = np.asarray(keys, np.int64)
    binned = np.nonzero(keys < n)[0]
    counts = np.bincount(keys[binned], minlength=n).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return counts, start, binned[np.argsort(keys[binned], kind="stable")]


def scan_blocks(n):
    """blocks of the three-launch scan over start[0..n]"""
    return -(-(n + 1) // SCAN_BLOCK)


def sort_route(count):
    """which kernel puts a run of `count` particles in order"""
    if count < 2:
        return "none"
    if count <= SMALL_RUN:
        return "insertion"
    return "bitonic" if count <= BIG_LDS else "rank"


def bitonic_size(count):
    m = 64
    while m < count:
        m <<= 1
    return m


# ---- link words ---------------------------------------------------------------------------------------------------------------------
def link_dists(keys, e, n):
    """k_bin_links on the sorted arrays.  -> order, dist[3][slots] (0: no later entry of the cell with this entry's e bit, 1..6, 7: seven
    or more), true[3][slots] (the distance itself, 0 for none), after[slots] (entries of the cell behind this one)"""
    _, start, order = bin_order_fast(keys, n)
    m = order.size
    k = np.asarray(keys)[order]
    slot = np.arange(m)
    after = start[k + 1] - 1 - slot
    true = np.zeros((3, m), np.int64)
    for c in range(3):
        ec = e[c][order]
        g = np.lexsort((slot, ec, k))                # the entries of every (cell, e bit) side by side, in slot order
        same = (k[g[1:]] == k[g[:-1]]) & (ec[g[1:]] == ec[g[:-1]])
        true[c, g[:-1][same]] = (g[1:] - g[:-1])[same]
    return order, np.minimum(true, 7), true, after


WALKS = ("at7", "later", "none")


def walk_outcomes(dist, true, after):
    """of the entries that have seven or more entries of their cell behind them: the one with the same e bit is the seventh (at7), a
    later one (later), or there is none (none) -> three boolean arrays"""
    return {"at7": true == 7, "later": true > 7, "none": (true == 0) & (after >= 7)}


# ---- gather tiles -------------------------------------------------------------------------------------------------------------------
MODES = (0, 1, 2, 3)              # MAC component X / Y / Z, cell-centred
PATHS = ("early", "empty", "lds", "fallback")


def reach(mode):
    """cells below a tile's origin that its nodes reach: 2 along a MAC component's own axis, 1 elsewhere"""
    return tuple(2 if mode == q else 1 for q in range(3))


def tiles_of(dims):
    sx, sy, sz = dims
    if sz == 1:
        return (-(-sx // (GX * GZ)), -(-sy // GY), 1)
    return (-(-sx // GX), -(-sy // GY), -(-sz // GZ))


def swizzled(dims):
    """xcd_swizzle permutes the tiles only when their number is a multiple of 8"""
    return int(np.prod(tiles_of(dims))) % 8 == 0


def tile_info(counts3, mode, tile):
    """counts3: [sz][sy][sx] run length of every cell.  One 4x4x4 tile of a 3-D grid -> (neighbourhood total, longest row, path).
    `empty` is the kernel's `total == 0` after the cell table; the row counts of the early-out cover the same cells, so it never
    follows (test_tile_table_hand_counted asserts that the model never returns it)."""
    sz, sy, sx = counts3.shape
    L = reach(mode)
    lo = [t * g - l for t, g, l in zip(tile, (GX, GY, GZ), L)]
    hi = [t * g + g for t, g in zip(tile, (GX, GY, GZ))]
    box = counts3[max(lo[2], 0):min(hi[2], sz), max(lo[1], 0):min(hi[1], sy), max(lo[0], 0):min(hi[0], sx)]
    rows = box.sum(axis=2)
    total = int(box.sum())
    early = not (rows != 0).any()
    path = "early" if early else ("fallback" if total > WCAP else ("empty" if total == 0 else "lds"))
    return total, int(rows.max()) if rows.size else 0, path


def tile_table(dims, counts, mode):
    """{tile: (total, longest row, path)} of every tile of a 3-D grid"""
    sx, sy, sz = dims
    assert sz > 1
    c3 = np.asarray(counts).reshape(sz, sy, sx)
    ntx, nty, ntz = tiles_of(dims)
    return {(tx, ty, tz): tile_info(c3, mode, (tx, ty, tz)) for tz in range(ntz) for ty in range(nty) for tx in range(ntx)}


def row_lengths(counts3, mode, tile):
    sz, sy, sx = counts3.shape
    L = reach(mode)
    lo = [t * g - l for t, g, l in zip(tile, (GX, GY, GZ), L)]
    hi = [t * g + g for t, g in zip(tile, (GX, GY, GZ))]
    return counts3[max(lo[2], 0):min(hi[2], sz), max(lo[1], 0):min(hi[1], sy), max(lo[0], 0):min(hi[0], sx)].sum(axis=2).ravel()


# ---- run shapes of a key sequence over 64-lane waves (run_of, k_bin_keys, k_bin_place) -------------------------------------------------
SHAPES = ("run64", "runs1", "end63", "start63", "cross_wave", "cross_block", "deleted_inside", "skipped_run", "partial_wave")


def run_shapes(keys, n):
    """keys: [np] with n for skipped particles.  -> {shape: number of occurrences}
      run64           a wave that is one run of a cell
      runs1           a wave of 64 binned lanes in which every lane is a run of its own
      end63           a run of two or more lanes, not the whole wave, that ends at lane 63 (lane 0 of the next wave holds another key)
      start63         a run that starts at lane 63 and ends there
      cross_wave      lane 63 and lane 0 of the next wave hold the same cell, inside one block of 256
      cross_block     the same across a block boundary (lanes 255 | 256)
      deleted_inside  cell, skipped, cell inside one wave
      skipped_run     cell, two or more skipped, the same cell, inside one wave
      partial_wave    the last wave is partly past np"""
    keys = np.asarray(keys, np.int64)
    m = -(-keys.size // WAVE) * WAVE
    g = np.full(m, n + 1, np.int64)
    g[:keys.size] = keys
    w = g.reshape(-1, WAVE)
    nxt0 = np.append(w[1:, 0], n + 1)
    cell63 = w[:, 63] < n
    found = dict.fromkeys(SHAPES, 0)
    whole = (w == w[:, :1]).all(1)
    found["run64"] = int((whole & (w[:, 0] < n)).sum())
    found["runs1"] = int(((w[:, 1:] != w[:, :-1]).all(1) & (w < n).all(1)).sum())
    found["end63"] = int((cell63 & ~whole & (w[:, 62] == w[:, 63]) & (nxt0 != w[:, 63])).sum())
    found["start63"] = int((cell63 & (w[:, 62] != w[:, 63]) & (nxt0 != w[:, 63])).sum())
    cross = cell63 & (nxt0 == w[:, 63])
    last_of_block = (np.arange(w.shape[0]) % (BLOCK // WAVE)) == BLOCK // WAVE - 1
    found["cross_wave"], found["cross_block"] = int((cross & ~last_of_block).sum()), int((cross & last_of_block).sum())
    for row in w:
        i = 0
        while i < WAVE:
            if row[i] == n and i > 0 and row[i - 1] < n:
                j = i
                while j < WAVE and row[j] == n:
                    j += 1
                if j < WAVE and row[j] == row[i - 1]:
                    found["deleted_inside" if j - i == 1 else "skipped_run"] += 1
                i = j
            else:
                i += 1
    found["partial_wave"] = int(keys.size % WAVE != 0)
    return found

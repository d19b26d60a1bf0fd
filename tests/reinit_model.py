"""Model of LevelsetGrid.reinitMarching (levelset.cpp:32-85, 122-228, fastmarch.cpp:23-221, fastmarch.h), in plain Python on lists of
floats that hold fp32 values; every fp32 operation is a double operation rounded once (exact for +, -, *, / and sqrt).  Three statements
of a march, over one set of per-cell bodies:

  * `serial`: the literal one -- the seeding loop of doReinitMarch in its order, performMarching with a binary heap ordered as the
    reference's comparator, the SetLevelsetBoundaries sweep;
  * the order-free seeding (`seed_free`): one evaluation per cell from the flags as the Init pass left them;
  * `rounds`: the order-free seeding, then windows of keys [T, T + DELTA) popped in sub-rounds of entries that no earlier window entry
    within L1 distance 2 holds back; a cell that goes on the heap inside the window joins it; the flag rule (a cell goes on the heap
    although a cell within L1 distance 2 with a later key has popped in this window) and the restart through the serial statement when
    a march flags.  Counters: windows, sub-rounds, pops, serial -- what lastReinitStats() reports.

`call` runs the whole method.  `CASES` / `case` are the fixture cases of tests/golden/reinit.npz (inputs are regenerated from seeded
generators, never stored); tools/record_reinit.py records the reference's results for them.
"""
import hashlib
import math
import os

import numpy as np

f32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLD, "reinit.npz")
FULL_LIMIT = 4096            # larger arrays are kept as SHA-256 digests
DELTA = 0.125
INITED, ONHEAP = 1, 2
EMPTY, FLUID, OBSTACLE, RESERVED = 4, 1, 2, 256


def F(x):
    """round to fp32"""
    with np.errstate(all="ignore"):
        return float(f32(x))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def new_counters():
    return {"invcnt0": 0, "invcnt1": 0, "invcnt2": 0, "plus": 0, "minus": 0, "plus_over_minus": 0, "maxtime_cut": 0, "equal_overwrite": 0,
            "worse_kept": 0, "transport": 0, "clamped_sqrt": 0}


class March(object):
    """one direction on shared lists (phi, fm, key, vel are modified in place)"""

    def __init__(self, dims, phi, fm, key, flags, vel, maxTime, direction, ignoreWalls, obsType, cnt):
        self.sx, self.sy, self.sz = dims
        self.is3d = dims[2] > 1
        self.Y, self.Z = dims[0], dims[0] * dims[1] if self.is3d else 0
        self.n = dims[0] * dims[1] * dims[2]
        self.phi, self.fm, self.key, self.flags = phi, fm, key, flags
        self.vel = vel if direction > 0 else None           # the reference transports on the outward march only
        self.dir, self.maxT = direction, F(F(maxTime) * direction)
        self.iw, self.obs, self.cnt = bool(ignoreWalls), int(obsType), cnt
        self.fm0 = fm
        self.nb = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)] + ([(0, 0, -1), (0, 0, 1)] if self.is3d else [])

    # --- helpers ---
    def ijk(self, idx):
        return idx % self.sx, (idx // self.sx) % self.sy, idx // (self.sx * self.sy)

    def index(self, i, j, k):
        return i + self.Y * j + self.Z * k

    def interior(self, i, j, k):
        return 1 <= i < self.sx - 1 and 1 <= j < self.sy - 1 and ((1 <= k < self.sz - 1) if self.is3d else k == 0)

    def in_grid(self, i, j, k):
        return 0 <= i < self.sx and 0 <= j < self.sy and 0 <= k < self.sz

    def wall(self, idx):
        return self.iw and (self.flags[idx] & self.obs) != 0

    def beyond(self, x, y):
        return x > y if self.dir > 0 else x < y

    def precedes(self, ta, a, tb, b):
        if abs(ta - tb) > 0.:
            return ta < tb if self.dir > 0 else ta > tb
        return a < b if self.dir > 0 else a > b

    def in_window(self, t, te):
        return t < te if self.dir > 0 else t > te

    # --- calculateDistance with its fp32 / fp64 map ---
    def calc(self, idx, inited):
        w, v, ax, inv, cnt = [0.] * 6, [], [0.] * 3, 0, self.cnt
        for c, st in enumerate((1, self.Y, self.Z)):
            if c == 2 and not self.is3d:
                inv += 1
                continue
            if inited(idx + st):
                ax[c] = self.phi[idx + st]
                v.append(ax[c])
                w[2 * c] = 1.
                cnt["plus"] += 1
                if inited(idx - st):
                    cnt["plus_over_minus"] += 1
            elif inited(idx - st):
                ax[c] = self.phi[idx - st]
                v.append(ax[c])
                w[2 * c + 1] = 1.
                cnt["minus"] += 1
            else:
                inv += 1
        d = float(self.dir)
        if inv == 0:
            ca, cb, cc = v
            e = F(F(F(F(F(ca * ca) + F(cb * cb)) - F(cb * cc)) + F(cc * cc)) - F(ca * F(cb + cc)))
            q = -2. * e + 3
            cs = F(q if 0. < q else 0.)
            cnt["clamped_sqrt"] += not 0. < q
            ret = F(0.333333 * F(F(F(ca + cb) + cc) + F(d * F(math.sqrt(cs)))))
        elif inv == 1:
            df = F(v[1] - v[0])
            q = 2. - F(df * df)
            cs = F(q if 0. < q else 0.)
            cnt["clamped_sqrt"] += not 0. < q
            ret = F(0.5 * F(F(v[0] + v[1]) + F(d * F(math.sqrt(cs)))))
        elif inv == 2:
            cnt["invcnt2"] += 1
            return F(v[0] + d), w
        else:
            raise AssertionError("calculateDistance: three invalid axes at a touched cell")
        cnt["invcnt%d" % inv] += 1
        for c in range(3):
            f = abs(F(ret - ax[c]))
            w[2 * c], w[2 * c + 1] = F(w[2 * c] * f), F(w[2 * c + 1] * f)
        norm = 0.
        for a in range(6):
            norm = F(norm + w[a])
        norm = F(1.0 / norm) if norm != 0. else math.copysign(math.inf, norm)
        return ret, [F(x * norm) for x in w]

    def transp(self, idx, w):
        if not self.flags[idx] & EMPTY:
            return
        self.cnt["transport"] += 1
        n, vel = self.n, self.vel
        val = [0., 0., 0.]
        for a, o in enumerate((1, -1, self.Y, -self.Y, self.Z, -self.Z)[:6 if self.is3d else 4]):
            if w[a] > 0.:
                for c in range(3):
                    val[c] = F(val[c] + F(vel[c * n + idx + o] * w[a]))
        if self.flags[idx - 1] & EMPTY:
            vel[idx] = val[0]
        if self.flags[idx - self.Y] & EMPTY:
            vel[n + idx] = val[1]
        if self.is3d and self.flags[idx - self.Z] & EMPTY:
            vel[2 * n + idx] = val[2]

    # --- addToList for an interior cell; True when it goes on the heap ---
    def touch(self, p, src):
        fm, phi = self.fm, self.phi
        if fm[p] == INITED:
            return False
        if self.beyond(phi[src], self.maxT):
            self.cnt["maxtime_cut"] += 1
            return False
        t, w = self.calc(p, lambda q: fm[q] == INITED)
        found = fm[p] == ONHEAP
        if found:
            if self.beyond(t, phi[p]):
                self.cnt["worse_kept"] += 1
                return False
            self.cnt["equal_overwrite"] += t == phi[p]
        fm[p], phi[p] = ONHEAP, t
        if self.vel is not None:
            self.transp(p, w)
        if found:
            return False
        self.key[p] = t
        return True

    def pop(self, c, push):
        i, j, k = self.ijk(c)
        self.fm[c] = INITED
        for di, dj, dk in self.nb:
            if self.interior(i + di, j + dj, k + dk):
                q = self.index(i + di, j + dj, k + dk)
                if self.touch(q, c):
                    push(q)

    # --- set-up passes ---
    def init_fm(self):
        for idx in range(self.n):
            self.key[idx] = 0.
            if not self.interior(*self.ijk(idx)):
                self.fm[idx] = 0
                continue
            v, wall = self.phi[idx], self.wall(idx)
            if self.dir < 0:
                self.fm[idx] = INITED if v >= 0 and not wall else 0
            else:
                self.fm[idx] = INITED if v < 0 and not wall else 0
                if wall:
                    self.phi[idx] = 0.

    def set_uninitialized(self, val):
        for idx in range(self.n):
            if self.interior(*self.ijk(idx)) and self.fm[idx] != INITED and not self.wall(idx):
                self.phi[idx] = val

    def boundaries_serial(self):
        """the KERNEL(single) sweep as written"""
        phi, ix = self.phi, self.index
        for k in range(self.sz):
            for j in range(self.sy):
                for i in range(self.sx):
                    c = ix(i, j, k)
                    if i == 0: phi[c] = phi[ix(1, j, k)]
                    if i == self.sx - 1: phi[c] = phi[ix(i - 1, j, k)]
                    if j == 0: phi[c] = phi[ix(i, 1, k)]
                    if j == self.sy - 1: phi[c] = phi[ix(i, j - 1, k)]
                    if self.is3d:
                        if k == 0: phi[c] = phi[ix(i, j, 1)]
                        if k == self.sz - 1: phi[c] = phi[ix(i, j, k - 1)]

    def boundary_value(self, old, i, j, k):
        """the same per cell, from the field before the sweep"""
        ix = self.index
        while True:
            if self.is3d and k == self.sz - 1 and k > 0:
                k -= 1
            elif self.is3d and k == 0:
                return old[ix(i, j, 1)]
            elif j == self.sy - 1:
                j -= 1
            elif j == 0:
                return old[ix(i, 1, k)]
            elif i == self.sx - 1:
                i -= 1
            elif i == 0:
                return old[ix(1, j, k)]
            else:
                return old[ix(i, j, k)]

    def boundaries_free(self):
        old = list(self.phi)
        for idx in range(self.n):
            i, j, k = self.ijk(idx)
            if not self.interior(i, j, k):
                self.phi[idx] = self.boundary_value(old, i, j, k)

    # --- seeding ---
    def at_interface(self, fm, i, j, k):
        for di, dj, dk in self.nb:
            if not self.in_grid(i + di, j + dj, k + dk):
                continue
            q = self.index(i + di, j + dj, k + dk)
            if fm[q] != INITED:
                continue
            if (self.phi[q] >= 0) if self.dir < 0 else (self.phi[q] < 0):
                return True
        return False

    def cells(self):
        for k in range(1, self.sz - 1) if self.is3d else (0,):
            for j in range(1, self.sy - 1):
                for i in range(1, self.sx - 1):
                    yield i, j, k

    def seed_serial(self, outer, push):
        """the loops of doReinitMarch, levelset.cpp:134-154 / 168-215, as written"""
        fm, phi = self.fm, self.phi

        def add(i, j, k, src):
            if self.interior(i, j, k):
                p = self.index(i, j, k)
                if self.touch(p, src):
                    push(p)
        for i, j, k in self.cells():
            p = self.index(i, j, k)
            if outer:
                if self.wall(p):
                    continue
                for di, dj, dk in self.nb:
                    q = self.index(i + di, j + dj, k + dk)
                    if fm[q] != INITED or self.wall(q):
                        continue
                    if phi[q] < 0 and phi[q] >= -2:
                        add(i, j, k, q)
                continue
            if self.dir < 0 and fm[p] == INITED:
                continue
            if self.wall(p):
                continue
            if self.dir > 0 and phi[p] < 0:
                continue
            if not self.at_interface(fm, i, j, k):
                continue
            fm[p] = INITED
            for di, dj, dk in self.nb:
                x, y, z = i + di, j + dj, k + dk
                q = self.index(x, y, z)
                if self.wall(q):
                    continue
                if ((phi[q] < 0) if self.dir < 0 else (phi[q] > 0)) and not self.at_interface(fm, x, y, z):
                    add(x, y, z, p)

    def is_marked(self, i, j, k):
        if not self.interior(i, j, k):
            return False
        idx = self.index(i, j, k)
        if self.fm0[idx] == INITED or self.wall(idx) or not self.at_interface(self.fm0, i, j, k):
            return False
        return not (self.dir > 0 and self.phi[idx] < 0)

    def seed_free(self, outer, push):
        """one evaluation per cell; reads the flags of the Init pass (fm0), writes fm"""
        self.fm0 = list(self.fm)
        fm0, phi = self.fm0, self.phi
        for i, j, k in self.cells():
            idx = self.index(i, j, k)
            if outer:
                if self.wall(idx) or fm0[idx] == INITED:
                    continue
                hit = False
                for di, dj, dk in self.nb:
                    q = self.index(i + di, j + dj, k + dk)
                    if fm0[q] == INITED and not self.wall(q) and phi[q] < 0 and phi[q] >= -2 and not self.beyond(phi[q], self.maxT):
                        hit = True
                if not hit:
                    continue
                t, w = self.calc(idx, lambda q: fm0[q] == INITED)
                self.fm[idx], phi[idx], self.key[idx] = ONHEAP, t, t
                if self.vel is not None:
                    self.transp(idx, w)
                push(idx)
                continue
            if self.is_marked(i, j, k):
                self.fm[idx] = INITED
                continue
            if self.wall(idx) or fm0[idx] == INITED or self.at_interface(fm0, i, j, k):
                continue
            order = [(0, 0, -1), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]            # ascending index: the loop's order
            nbs = [(self.index(i + a, j + b, k + c), self.is_marked(i + a, j + b, k + c)) for a, b, c in order if self.is3d or c == 0]
            inited = {q: fm0[q] == INITED for q, _ in nbs}
            cur, key, onheap = phi[idx], 0., False
            for q, marked in nbs:
                if not marked:
                    continue
                inited[q] = True
                if not ((cur < 0) if self.dir < 0 else (cur > 0)):
                    continue
                if self.beyond(phi[q], self.maxT):
                    continue
                t, w = self.calc(idx, lambda r: inited.get(r, False))
                if onheap and self.beyond(t, cur):
                    continue
                cur = t
                if self.vel is not None:
                    self.transp(idx, w)
                if not onheap:
                    key = t
                onheap = True
            if onheap:
                phi[idx], self.fm[idx], self.key[idx] = cur, ONHEAP, key
                push(idx)

    # --- the literal march ---
    def serial(self, outer):
        heap = []                       # binary heap of (key, cell), ordered by precedes

        def before(a, b):
            return self.precedes(heap[a][0], heap[a][1], heap[b][0], heap[b][1])

        def push(q):
            heap.append((self.key[q], q))
            a = len(heap) - 1
            while a > 0 and before(a, (a - 1) // 2):
                heap[a], heap[(a - 1) // 2] = heap[(a - 1) // 2], heap[a]
                a = (a - 1) // 2

        def pop():
            top = heap[0][1]
            last = heap.pop()
            if heap:
                heap[0] = last
                a = 0
                while True:
                    b = a
                    for c in (2 * a + 1, 2 * a + 2):
                        if c < len(heap) and before(c, b):
                            b = c
                    if b == a:
                        break
                    heap[a], heap[b] = heap[b], heap[a]
                    a = b
            return top
        self.seed_serial(outer, push)
        pops = 0
        while heap:
            self.pop(pop(), push)
            pops += 1
        self.boundaries_serial()
        return {"windows": 0, "subrounds": 0, "pops": pops, "serial": 1}

    # --- the march in rounds ---
    def selectable(self, c, te):
        i, j, k = self.ijk(c)
        t = self.key[c]
        rk = 2 if self.is3d else 0
        for dk in range(-rk, rk + 1):
            for dj in range(-2, 3):
                for di in range(-2, 3):
                    if not 1 <= abs(di) + abs(dj) + abs(dk) <= 2 or not self.in_grid(i + di, j + dj, k + dk):
                        continue
                    q = self.index(i + di, j + dj, k + dk)
                    if self.fm[q] == ONHEAP and self.in_window(self.key[q], te) and self.precedes(self.key[q], q, t, c):
                        return False
        return True

    def late_conflict(self, c, epoch, w):
        i, j, k = self.ijk(c)
        rk = 2 if self.is3d else 0
        for dk in range(-rk, rk + 1):
            for dj in range(-2, 3):
                for di in range(-2, 3):
                    if not 1 <= abs(di) + abs(dj) + abs(dk) <= 2 or not self.in_grid(i + di, j + dj, k + dk):
                        continue
                    q = self.index(i + di, j + dj, k + dk)
                    if epoch[q] == w and self.precedes(self.key[c], c, self.key[q], q):
                        return True
        return False

    def rounds(self, outer, delta=DELTA, rule="refined"):
        snap = (list(self.phi), list(self.fm), None if self.vel is None else list(self.vel))
        cnt0 = dict(self.cnt)
        lst = []
        self.seed_free(outer, lst.append)
        st = {"windows": 0, "subrounds": 0, "pops": 0, "serial": 0}
        flag, joined, epoch = [False], [0], [0] * self.n
        while not flag[0]:
            live = [self.key[c] for c in lst if self.fm[c] == ONHEAP]
            if not live:
                break
            T = min(live) if self.dir > 0 else max(live)
            te = F(T + delta) if self.dir > 0 else F(T - delta)
            st["windows"] += 1

            def push(q):
                lst.append(q)
                if self.in_window(self.key[q], te):
                    joined[0] += 1
                    if rule == "simple":
                        flag[0] = True
                if self.late_conflict(q, epoch, st["windows"]):
                    flag[0] = True
            while True:
                W = [c for c in lst if self.fm[c] == ONHEAP and self.in_window(self.key[c], te)]
                sel = [c for c in W if self.selectable(c, te)]
                if not W or not sel:
                    flag[0] = True
                    break
                st["subrounds"] += 1
                st["pops"] += len(sel)
                joined[0] = 0
                for c in sel:
                    epoch[c] = st["windows"]
                for c in sel:
                    self.pop(c, push)
                if flag[0] or (len(sel) == len(W) and not joined[0]):
                    break
        if flag[0]:
            self.phi[:], self.fm[:] = snap[0], snap[1]
            if self.vel is not None:
                self.vel[:] = snap[2]
            self.key[:] = [0.] * self.n
            self.cnt.clear()
            self.cnt.update(cnt0)
            return self.serial(outer)
        self.boundaries_free()
        return st


def call(dims, phi, flags, vel=None, maxTime=4.0, ignoreWalls=False, correctOuterLayer=True, obstacleType=OBSTACLE, mode="rounds", delta=DELTA, rule="refined"):
    """the whole method; arrays in, a dict of arrays out: phi, vel, fm and key as the outward march leaves them, stats[name] = (inward,
    outward), counters"""
    n = int(np.prod(dims))
    p = [float(x) for x in np.asarray(phi, f32).reshape(-1)]
    fl = [int(x) for x in np.asarray(flags).reshape(-1)]
    v = None if vel is None else [float(x) for x in np.asarray(vel, f32).reshape(-1)]
    fm, key, cnt = [-1] * n, [math.nan] * n, new_counters()
    stats = {}
    maxTime = F(maxTime)
    for d in (-1, 1):
        m = March(dims, p, fm, key, fl, v, maxTime, d, ignoreWalls, obstacleType, cnt)
        m.init_fm()
        outer = d > 0 and bool(correctOuterLayer)
        st = m.serial(outer) if mode == "serial" else m.rounds(outer, delta, rule)
        for name, x in st.items():
            stats.setdefault(name, []).append(x)
        m.set_uninitialized(F(-maxTime - 1.) if d < 0 else F(maxTime + 1.))
    return {"phi": np.array(p, f32), "vel": None if v is None else np.array(v, f32), "fm": np.array(fm, np.int32), "key": np.array(key, f32),
            "stats": {k: tuple(x) for k, x in stats.items()}, "counters": cnt}


def seeded(dims, phi, flags, vel, maxTime, ignoreWalls, correctOuterLayer, obstacleType, direction, free):
    """the state after the Init pass and the seeding of one direction alone: (phi, fm, key, vel, heap entries sorted)"""
    n = int(np.prod(dims))
    p = [float(x) for x in np.asarray(phi, f32).reshape(-1)]
    fl = [int(x) for x in np.asarray(flags).reshape(-1)]
    v = None if vel is None else [float(x) for x in np.asarray(vel, f32).reshape(-1)]
    fm, key = [-1] * n, [math.nan] * n
    m = March(dims, p, fm, key, fl, v, F(maxTime), direction, ignoreWalls, obstacleType, new_counters())
    m.init_fm()
    lst = []
    (m.seed_free if free else m.seed_serial)(direction > 0 and bool(correctOuterLayer), lst.append)
    return np.array(p, f32), np.array(fm, np.int32), np.array(key, f32), None if v is None else np.array(v, f32), sorted(lst)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def centres(dims):
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) + 0.5 for s in dims[::-1]], indexing="ij")
    return x, y, z


def sphere(dims, centre, radius):
    x, y, z = centres(dims)
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(f32).reshape(-1)


def box(dims, p0, p1):
    x, y, z = centres(dims)
    d = np.maximum.reduce([p0[0] - x, x - p1[0], p0[1] - y, y - p1[1]] + ([p0[2] - z, z - p1[2]] if dims[2] > 1 else []))
    return d.astype(f32).reshape(-1)


def domain_flags(dims, phi):
    """initDomain's obstacle border, then fluid where phi < 0 and empty elsewhere (updateFromLevelset's result on a clean field)"""
    fl = np.where(np.asarray(phi) < 0, FLUID, EMPTY).astype(np.int32).reshape(dims[::-1])
    fl[:, :, 0] = fl[:, :, -1] = fl[:, 0, :] = fl[:, -1, :] = OBSTACLE
    if dims[2] > 1:
        fl[0] = fl[-1] = OBSTACLE
    return fl.reshape(-1)


def obstacle_box(dims, flags, bit):
    """a box of `bit` cells in the lower middle of the domain"""
    fl = flags.reshape(dims[::-1]).copy()
    zs = slice(dims[2] // 3, max(dims[2] // 3 + 1, 2 * dims[2] // 3)) if dims[2] > 1 else slice(0, 1)
    sel = fl[zs, dims[1] // 3:max(dims[1] // 3 + 1, dims[1] // 2), dims[0] // 3:max(dims[0] // 3 + 1, 2 * dims[0] // 3)]
    sel[...] = (sel & ~(FLUID | EMPTY)) | bit if bit == OBSTACLE else sel | bit
    return fl.reshape(-1)


def middle(dims):
    """a cell centre near the middle"""
    return [s // 2 + 0.5 for s in dims]


def make_phi(kind, dims, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    r = max(1.2, min(dims[0], dims[1], dims[2] if dims[2] > 1 else dims[0]) * 0.3)
    if kind == "centred":
        return sphere(dims, middle(dims), r)
    if kind == "off":
        return sphere(dims, [c + o for c, o in zip(middle(dims), (0.31, -0.17, 0.23 if dims[2] > 1 else 0.))], r)
    if kind == "basin":            # the basin of test_2050_freesurface.py joined with its drop
        gs = dims
        b = box(dims, (0, 0, 0), (gs[0], gs[1] * 0.2, gs[2]))
        return np.minimum(b, sphere(dims, [gs[0] * 0.5, gs[1] * 0.5, gs[2] * 0.5], max(dims) * 0.15))
    if kind == "flags":            # initFromFlags of the basin's flags
        return np.where(make_phi("basin", dims, seed) < 0, -0.5, 0.5).astype(f32)
    if kind == "positive":
        return (1.0 + rng.random(n)).astype(f32)
    if kind == "negative":
        return (-1.0 - rng.random(n)).astype(f32)
    if kind.startswith("noise"):
        sigma = {"noise02": 0.2, "noise10": 1.0}[kind]
        return (sphere(dims, middle(dims), r).astype(np.float64) + sigma * rng.standard_normal(n)).astype(f32)
    raise KeyError(kind)


SIZES = [(7, 5, 4), (6, 6, 6), (33, 31, 29), (65, 3, 3), (3, 3, 70), (12, 9, 1), (3, 3, 1)]
SMALL = [(7, 5, 4), (6, 6, 6), (12, 9, 1)]


def _name(kind, dims):
    return "%s_%dx%dx%d" % ((kind,) + tuple(dims))


def _cases():
    out = {}

    def add(name, dims, kind, maxTime=4.0, iw=False, outer=True, obs=OBSTACLE, vel=False, wallbit=0, seed=None):
        out[name] = dict(dims=dims, kind=kind, maxTime=maxTime, ignoreWalls=iw, correctOuterLayer=outer, obstacleType=obs, vel=vel,
                         wallbit=wallbit, seed=len(out) + 11 if seed is None else seed)
    for dims in SIZES:
        add(_name("centred", dims), dims, "centred", 4.0, vel=True)
        add(_name("off", dims), dims, "off", 2.0)
    for dims in SMALL + [(33, 31, 29)]:
        add(_name("basin", dims), dims, "basin", 6.0, vel=True)
    for dims in [(6, 6, 6), (12, 9, 1), (65, 3, 3)]:
        add(_name("flags", dims), dims, "flags", 4.0, vel=True)
    for dims in [(7, 5, 4), (12, 9, 1), (3, 3, 1)]:
        add(_name("positive", dims), dims, "positive", 4.0)
        add(_name("negative", dims), dims, "negative", 4.0, vel=True)
    for dims in SMALL + [(33, 31, 29), (3, 3, 70)]:
        add(_name("noise02", dims), dims, "noise02", 4.0, vel=True)
    # sigma 1.0 has to flag.  On the small grids a field does so by chance (about one in four does not), so their seed is fixed at the
    # first one whose field does; 64 interior cells (6x6x6) are left to noise02
    for dims in [(7, 5, 4), (12, 9, 1), (33, 31, 29)]:
        add(_name("noise10", dims), dims, "noise10", 2.0 if dims == (33, 31, 29) else 6.0, vel=True, seed=None if dims == (33, 31, 29) else 1)
    for dims in [(12, 9, 1), (7, 5, 4), (33, 31, 29)]:
        add(_name("wallbox", dims), dims, "basin", 4.0, iw=True, wallbit=OBSTACLE, vel=True)
        add(_name("wallres", dims), dims, "off", 6.0, iw=True, obs=RESERVED, wallbit=RESERVED, vel=True)
    for dims in [(12, 9, 1), (6, 6, 6), (7, 5, 4)]:     # obstacleLevelset's call, initplugins.cpp:93-107, on -+0.5 from obstacle flags
        add(_name("obsls", dims), dims, "obsls", 6.0, iw=True, outer=False, obs=RESERVED, wallbit=OBSTACLE)
        add(_name("inner", dims), dims, "off", 4.0, outer=False, vel=True)
    return out


CASES = _cases()
# the recorded loops: name -> (dims, steps, scene); scene 0 = tools/tests/test_2050_freesurface.py, 1 = test_2045_fallingDrop.py (a liquid
# box of 4 cells a side at res 20: the smallest at which the drop still has an interior)
LOOPS = {"fs3d": ((24, 24, 24), 8, 0), "fs2d": ((32, 32, 1), 12, 0), "drop": ((20, 20, 20), 6, 1)}
SMOOTH = ("centred", "off", "basin")          # kinds whose correctOuterLayer cases must not flag


def case(name):
    """the inputs of a fixture case: dims, phi, flags, vel (or None) and the call's arguments"""
    c = dict(CASES[name])
    dims, seed = c["dims"], c["seed"]
    n = int(np.prod(dims))
    rng = np.random.default_rng(1000 + seed)
    if c["kind"] == "obsls":
        flags = obstacle_box(dims, domain_flags(dims, np.ones(n, f32)), OBSTACLE)
        phi = np.where((flags & OBSTACLE) != 0, -0.5, 0.5).astype(f32)
    else:
        phi = make_phi(c["kind"], dims, seed)
        flags = domain_flags(dims, phi)
        if c["wallbit"]:
            flags = obstacle_box(dims, flags, c["wallbit"])
    vel = rng.standard_normal(3 * n).astype(f32) if c["vel"] else None
    c.update(phi=phi, flags=flags, velocity=vel, n=n)
    return c


_memo = {}


def model(name, mode="rounds"):
    if (name, mode) not in _memo:
        c = case(name)
        _memo[name, mode] = call(c["dims"], c["phi"], c["flags"], c["velocity"], c["maxTime"], c["ignoreWalls"], c["correctOuterLayer"],
                                 c["obstacleType"], mode)
    return _memo[name, mode]


def random_case(q):
    """case q of the equivalence sweep: up to 10x9x8, from smooth to sigma 1.0, both seedings, with and without transport and walls"""
    rng = np.random.default_rng(50000 + q)
    if q % 3 == 0:
        dims = (int(rng.integers(3, 11)), int(rng.integers(3, 10)), 1)
    else:
        dims = (int(rng.integers(3, 11)), int(rng.integers(3, 10)), int(rng.integers(3, 9)))
    n = int(np.prod(dims))
    sigma = (0., 0., 0.02, 0.05, 0.1, 0.2, 0.5, 1.0)[q % 8]
    r = float(rng.uniform(1.0, 3.5))
    centre = [float(rng.uniform(1.0, s - 1.0)) if s > 1 else 0.5 for s in dims]
    phi = (sphere(dims, centre, r).astype(np.float64) + sigma * rng.standard_normal(n)).astype(f32)
    if q % 11 == 0:
        phi = np.where(phi < 0, -0.5, 0.5).astype(f32)
    flags = domain_flags(dims, phi)
    iw, obs = bool(q % 5 == 0), OBSTACLE if q % 10 else RESERVED
    if iw:
        flags = obstacle_box(dims, flags, obs)
    vel = rng.standard_normal(3 * n).astype(f32) if q % 4 else None
    return dict(dims=dims, phi=phi, flags=flags, velocity=vel, maxTime=(2.0, 4.0, 6.0)[q % 3], ignoreWalls=iw, correctOuterLayer=bool(q % 7),
                obstacleType=obs, sigma=sigma)

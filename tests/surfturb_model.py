"""Shared by the surface-turbulence tests and tools/surfturb_host_check.py: access to tests/golden/surfturb.npz (the reference's
recorded calls and stages, tools/record_surfturb.py), the case files of the stand-alone host program, the comparisons with their
bounds, and the numpy model: the index work (the cell list, the serial greedy delete pass and its order-free statement in rounds,
ParticleSystem::compress) and every stage's per-point arithmetic (class Model), run from recorded inputs, with the edge cases that
the GPU tests and the host program share.

Bounds.  expf and logf are the only values that may differ between two correct implementations, by at most
1 ulp (2^-23 relative) each.  Every sum runs in the same order, so with at most NEIGHBOURS = 128 terms a sum of such values moves by at
most (NEIGHBOURS + 1) * 2^-23 = 1.6e-5 relative to sum |term|.  The level is a sum of positive terms: with A >= 2.2 / outer^2 and
sqrt(-log lvl / A) >= 0.4 outer inside the kept band, its error is below 2e-5.  The normalised gradient has sum |term| / |sum| <= 3 on
points outside the coarse particles, so its direction moves by at most 5e-5.  constrainSurface moves a point by at most 0.6 (outer -
inner) along it: 2e-5 outer.  The add pass places a point one meanFineDistance along the normalised sum of at most NEIGHBOURS tangent
parts, each moved by twice the gradient's error, with a cancellation of at most 4 in the fixture: POS_BOUND = 1e-4 (outer = 1).  The
fitted normal divides by a 3 x 3 determinant of sums of the frame's coordinates; the frame moves with the gradient, the fit's
condition in the fixture is below 20: NRM_BOUND = 1e-3.
"""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "surfturb.npz")
f32, i32, i64 = np.float32, np.int32, np.int64
PNEW, PDELETE = 1, 1 << 10
RES = 12
POS_BOUND, NRM_BOUND = 1e-4, 1e-3
# the stages with nothing downstream of expf / logf: bit for bit against the reference
EXACT_STAGES = ("accel", "regularize", "waves", "advect")
KEYS = ("pos", "flag", "normals", "real")


def golden():
    return np.load(GOLDEN)


def state(G, pre):
    return {k: G[pre + "/" + k] for k in KEYS + ("sizes",)}


def chain_names(G):
    return [n.decode() for n in G["chain/names"]]


def call_case(G, f):
    """the inputs of whole call f: parameters, frameCount, flags, coarse particles with their previous positions, the surface before"""
    st = state(G, "call%d/before" % f)
    return dict(args=G["set0/args"], frame=f, nb=int(G["set0/args"][2]), R=G["set0/res"], flags=G["flags"], cpos=G["call%d/coarse_pos" % f],
                cflag=G["call%d/coarse_flag" % f], prev=G["call%d/coarse_prev" % f], **st)


def chain_case(G, i):
    """the inputs of stage i of the chain: the state after stage i - 1; the coarse particles of the last call (advect: moved once more)"""
    names = chain_names(G)
    st = state(G, "chain/%d" % (i - 1) if i else "chain/start")
    cpos = G["chain/coarse2_pos"] if names[i] == "advect" else G["call2/coarse_pos"]
    return dict(args=G["set0/args"], frame=3, nb=int(G["set0/args"][2]), R=G["set0/res"], flags=G["flags"], cpos=cpos, cflag=G["call2/coarse_flag"],
                prev=G["chain/coarse_prev"], **st)


def init_case(G, k):
    """a first call with nb = 0 under parameter set k: initFines alone"""
    c = call_case(G, 0)
    c.update(args=G["set%d/args" % k], nb=0, R=G["set%d/res" % k])
    return c


# ---- the stand-alone host program
def _soa(a):
    return np.ascontiguousarray(np.asarray(a, f32).T).tobytes()


def host_run(exe, mode, c):
    n, nc = len(c["flag"]), len(c["cflag"])
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(a, "wb") as f:
            f.write(np.array([RES, c["frame"], c["nb"], c["R"][0], c["R"][1], nc, n, c["sizes"][1], c["sizes"][2]], i64).tobytes())
            f.write(np.asarray(c["args"], f32).tobytes() + np.ascontiguousarray(c["flags"], i32).tobytes())
            f.write(_soa(c["cpos"]) + np.asarray(c["cflag"], i32).tobytes() + _soa(c["prev"]))
            f.write(_soa(c["pos"]) + np.asarray(c["flag"], i32).tobytes() + _soa(c["normals"]) + np.ascontiguousarray(c["real"], f32).tobytes())
        r = subprocess.run([exe, mode, a, b], capture_output=True, text=True)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
        raw = open(b, "rb").read()
    if mode == "params":
        par = np.frombuffer(raw, f32, 32)
        R = np.frombuffer(raw, i32, 2, 128)
        return par, R, np.frombuffer(raw, f32, offset=136).reshape(-1, 3)
    o = np.frombuffer(raw, i64, 6)
    m, nd, it = int(o[0]), int(o[3]), int(o[4])
    at = [48]

    def take(dtype, *shape):
        x = np.frombuffer(raw, dtype, int(np.prod(shape)), at[0]).reshape(shape)
        at[0] += x.nbytes
        return x
    got = dict(sizes=o, pos=take(f32, 3, m).T, flag=take(i32, m), normals=take(f32, 3, m).T, real=take(f32, 5, m), displaced=take(f32, 3, nd).T,
               stats=take(i64, it, 6))
    assert at[0] == len(raw)
    return got


def host_params(exe, G, k):
    return host_run(exe, "params", init_case(G, k))


def compare(got, want, exact, displaced=None):
    """asserts the discrete results exactly and the arrays bit for bit (exact) or within the bounds; -> a summary"""
    assert [int(x) for x in got["sizes"][:3]] == [int(x) for x in want["sizes"][:3]], (got["sizes"], want["sizes"])
    assert np.array_equal(got["flag"], want["flag"])
    live = (want["flag"] & PDELETE) == 0
    out = []
    for k, bound in (("pos", POS_BOUND), ("normals", NRM_BOUND), ("real", NRM_BOUND)):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if exact:
            assert g.tobytes() == w.tobytes(), k
            continue
        sel = live if k != "real" else np.broadcast_to(live, w.shape)
        gl, wl = g[sel], w[sel]
        both_nan = np.isnan(gl) & np.isnan(wl)
        d = np.where(both_nan, 0, np.abs(gl.astype(np.float64) - wl))
        worst = float(d.max()) if d.size else 0.0
        differ = int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).sum())
        out.append("%s: %d values differ, max %.3g = %.3g of the bound" % (k, differ, worst, worst / bound))
        assert worst <= bound, (k, worst, bound)
    if displaced is not None:
        assert len(got["displaced"]) == len(displaced)
    return "equal bit for bit" if exact else "; ".join(out)


# ---- numpy statements of the index work
def cell_of(pos, res, R):
    """clamp(int(floor(p / res * R)), 0, R - 1) per axis in fp32 with the x86 conversion: NaN and out-of-range give INT_MIN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.floor(np.asarray(pos, f32) / f32(res) * f32(R))
        ok = (v >= f32(-2147483648.0)) & (v < f32(2147483648.0))
        c = np.where(ok, np.where(ok, v, 0).astype(np.int64), -2 ** 31)
    c = np.clip(c, 0, R - 1)
    return (c[:, 0] * R + c[:, 1]) * R + c[:, 2]


def cell_list(pos, res, R):
    """-> (start[R^3 + 1], ids[n]): the slots of a cell ascending (a stable sort by cell)"""
    cell = cell_of(pos, res, R)
    ids = np.argsort(cell, kind="stable").astype(i32)
    start = np.searchsorted(cell[ids], np.arange(R ** 3 + 1)).astype(i32)
    return start, ids


def _norm(d):
    """norm() of vectorbase.h:384-389 on fp32 vectors"""
    d = np.asarray(d, f32)
    l = f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])
    eps2 = f32(1e-6) * f32(1e-6)
    if l <= eps2:
        return f32(0)
    return f32(1) if abs(float(l) - 1.0) < float(eps2) else np.sqrt(f32(l))


def _in_range(pos, i, j, radius):
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(_norm(pos[j] - pos[i]) <= radius)


def greedy_serial(pos, flag, listed, radius, lo, hi):
    """delete pass 1 as the reference runs it (:611-618): slots in order, a kill is seen by the later slots.  Brute force over the
    listed slots (the first `listed`), which is what the cell query finds.  -> kill calls per slot (bool)"""
    flag = flag.copy()
    killed = np.zeros(len(pos), bool)
    for i in range(len(pos)):
        p = pos[i]
        inside = bool(np.all((p >= lo) & (p <= hi)))
        hit = not inside
        if not hit:
            for j in range(listed):
                if j != i and not (flag[j] & PDELETE) and _in_range(pos, i, j, radius):
                    hit = True
                    break
        if hit:
            flag[i] |= PDELETE
            killed[i] = True
    return killed


def greedy_rounds(pos, flag, listed, radius, lo, hi):
    """the order-free statement: a slot outside the domain is killed at once; any other is decided once its lower listed neighbours
    within range (active before the pass) are -- killed if one of them is kept or a higher listed active neighbour is in range.
    Every round reads the states of the round before.  -> (kill calls per slot, rounds)"""
    n = len(pos)
    nb = [[j for j in range(listed) if j != i and not (flag[j] & PDELETE) and _in_range(pos, i, j, radius)] for i in range(n)]
    inside = [bool(np.all((pos[i] >= lo) & (pos[i] <= hi))) for i in range(n)]
    state = np.zeros(n, i32)
    rounds = 0
    while (state == 0).any():
        new = state.copy()
        for i in np.nonzero(state == 0)[0]:
            if not inside[i]:
                new[i] = 2
            elif any(j < i and state[j] == 0 for j in nb[i]):
                continue
            else:
                new[i] = 2 if any(j > i or state[j] == 1 for j in nb[i]) else 1
        state = new
        rounds += 1
        assert rounds <= n + 1
    return state == 2, rounds


def compress(flag):
    """ParticleSystem::compress, particle.h:614-633 -> src[new slot] = the old slot it holds"""
    n = len(flag)
    flag = flag.copy()
    src = np.arange(n)
    nxt = n
    for i in range(n):
        while flag[i] & PDELETE:
            nxt -= 1
            src[i], flag[i] = src[nxt], flag[nxt]
            flag[nxt] = 1 << 30
    return src[:nxt]


# ---- the per-point arithmetic, stage by stage: fp32 in the evaluation order of the contract.  Every function
# works on all points at once; a point's neighbours are walked in the contract's order (cells i outer, j, k inner, slots ascending,
# per neighbour the ghost chain x-, x+, y-, y+, z-, z+, then the neighbour itself) by stepping through the padded lists rank by rank
# and adding under a mask, so every sum has the order of the serial loop.
PAR_NAMES = ("res", "outer", "inner", "mfd", "A", "nrad", "trad", "bndm", "bndp", "dt", "wspeed", "wdamp", "wfreq", "wamp", "wmaxf", "wseedamp",
             "ccenter", "cradius", "sstep", "costheta", "addr", "delr", "dtheta")


class Par(object):
    def __init__(self, values):
        for k, v in zip(PAR_NAMES, np.asarray(values, f32)):
            setattr(self, k, f32(v))


def par_of(G, k, frame):
    """the parameter block from the recorded host values of parameter set k and the plugin's arguments"""
    p, a = G["set%d/par" % k], np.asarray(G["set%d/args" % k], f32)
    mfd = p[3]
    theta = f32(f32(f32(a[3] * f32(frame)) * a[4]) * a[6])
    cos = f32(np.cos(np.float64(theta)))        # the fp64 function rounded once; the recorded cosf(theta) of the frame where the fixture has it
    for name in ("st%d/costheta" % frame, "chain/costheta"):
        if k == 0 and name in G and (name != "chain/costheta" or frame == 3):
            assert cos == G[name][0], (name, cos, G[name][0])
            cos = G[name][0]
    rest = [a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], cos,
            f32(np.float64(mfd) - 1e-6), f32(0.67 * np.float64(mfd)), f32(f32(2) * mfd) / f32(p[1] + p[2])]
    return Par(list(p) + rest)


def _coord(v, res, R):
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.floor(np.asarray(v, f32) / f32(res) * f32(R))
        ok = (v >= f32(-2147483648.0)) & (v < f32(2147483648.0))
        c = np.where(ok, np.where(ok, v, 0).astype(np.int64), -2 ** 31)
    return np.clip(c, 0, R - 1)


def walk(P, R, cells, active, centers, radius):
    """-> (idx[n][L], valid[n][L]): the active slots a query around every centre visits, in its order, padded"""
    start, ids = cells
    centers = np.asarray(centers, f32).reshape(-1, 3)
    radius = f32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = _coord(centers - radius, P.res, R), _coord(centers + radius, P.res, R)
    rows = []
    for a, b in zip(lo, hi):
        row = []
        for ci in range(a[0], b[0] + 1):
            for cj in range(a[1], b[1] + 1):
                c0 = (ci * R + cj) * R
                row.append(ids[start[c0 + a[2]]:start[c0 + b[2] + 1]])       # the cells of one k run are adjacent in the list
        row = np.concatenate(row) if row else np.zeros(0, i32)
        rows.append(row[active[row]])
    L = max([len(r) for r in rows] + [1])
    idx, valid = np.zeros((len(rows), L), np.int64), np.zeros((len(rows), L), bool)
    for i, r in enumerate(rows):
        idx[i, :len(r)], valid[i, :len(r)] = r, True
    return idx, valid


def dot(a, b):
    return f32(a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(t, v):
    return np.stack([t[..., 1] * v[..., 2] - t[..., 2] * v[..., 1], t[..., 2] * v[..., 0] - t[..., 0] * v[..., 2],
                     t[..., 0] * v[..., 1] - t[..., 1] * v[..., 0]], -1)


_EPS2 = f32(1e-6) * f32(1e-6)


def norm(v):
    l = dot(v, v)
    one = np.abs(l.astype(np.float64) - 1.0) < np.float64(_EPS2)
    return np.where(l <= _EPS2, f32(0), np.where(one, f32(1), np.sqrt(l))).astype(f32)


def normalized(v):
    l = dot(v, v)
    one = np.abs(l.astype(np.float64) - 1.0) < np.float64(_EPS2)
    fac = (1.0 / np.sqrt(l.astype(np.float64))).astype(f32)
    return np.where(one[..., None], v, np.where((l > _EPS2)[..., None], v * fac[..., None], f32(0))).astype(f32)


def weight(dist, radius):
    return np.where(dist > radius, f32(0), f32(1) - dist / radius).astype(f32)


def clampf(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(f32)


def st_exp(x):
    return np.exp(x.astype(np.float64)).astype(f32)


def st_log(x):
    return np.log(x.astype(np.float64)).astype(f32)


def in_domain(P, p):
    return ((p >= P.bndm) & (p <= P.bndp)).all(-1)


def ghosts(P, q, radius):
    """the chain of neighbour positions q[n][3]: seven (mask[n], image[n][3], the axis whose normal component flips or -1)"""
    out = []
    for a in range(3):
        for plane, near in ((P.bndm, q[:, a] - P.bndm <= radius), (P.bndp, P.bndp - q[:, a] <= radius)):
            g = q.copy()
            g[:, a] = f32(2) * plane - q[:, a]
            out.append((near, g, a))
    out.append((np.ones(len(q), bool), q, -1))
    return out


def _flip(v, a):
    if a < 0:
        return v
    v = v.copy()
    v[:, a] = -v[:, a]
    return v


def _acc(mask, acc, term):
    return np.where(mask if acc.ndim == 1 else mask[:, None], acc + term, acc).astype(f32)


class Model(object):
    """the state of one call between its stages: the surface (pos, flag, normals, real = H, DtH, source, seed, seedAmp rows, the
    delete bookkeeping) and the coarse particles with both cell lists"""

    def __init__(self, P, R, c, listed=None):
        self.P, self.Rc, self.Rs = P, int(R[0]), int(R[1])
        self.margins = {}       # decision -> (smallest distance from its threshold over the live points, the bound it is held to)
        self.pos, self.flag, self.normals, self.real = (np.array(c[k]) for k in KEYS)
        self.mDeletes, self.mDeleteChunk = int(c["sizes"][1]), int(c["sizes"][2])
        self.cpos, self.cflag, self.prev = np.asarray(c["cpos"], f32), np.asarray(c["cflag"], i32), np.asarray(c["prev"], f32)
        self.stats = {}
        self.coarse_list()
        self.surface_list(empty=listed == 0)

    def state(self):
        return dict(pos=self.pos, flag=self.flag, normals=self.normals, real=self.real, sizes=[len(self.flag), self.mDeletes, self.mDeleteChunk])

    def coarse_list(self, of_prev=False):
        self.cc = cell_list(self.prev if of_prev else self.cpos, self.P.res, self.Rc)

    def surface_list(self, empty=False):
        self.listed = 0 if empty else len(self.pos)
        self.cs = cell_list(self.pos[:self.listed], self.P.res, self.Rs)

    def _coarse(self, centers, radius):
        return walk(self.P, self.Rc, self.cc, (self.cflag & PDELETE) == 0, centers, radius)

    def _surf(self, centers, radius):
        return walk(self.P, self.Rs, self.cs, (self.flag & PDELETE) == 0, centers, radius)

    # computeConstraintLevel / computeConstraintGradient
    def level(self, pos):
        P = self.P
        idx, valid = self._coarse(pos, f32(1.5) * P.outer)
        lvl = np.zeros(len(pos), f32)
        for l in range(idx.shape[1]):
            d = self.cpos[idx[:, l]] - pos
            lvl = _acc(valid[:, l], lvl, st_exp(-P.A * dot(d, d)))
        lvl = np.where(lvl > 1, f32(1), lvl)
        return ((np.sqrt(-st_log(lvl) / P.A) - P.inner) / (P.outer - P.inner)).astype(f32)

    def gradient(self, pos):
        P = self.P
        idx, valid = self._coarse(pos, f32(1.5) * P.outer)
        g = np.zeros((len(pos), 3), f32)
        for l in range(idx.shape[1]):
            cp = self.cpos[idx[:, l]]
            d = cp - pos
            s = f32(f32(2) * P.A) * st_exp(-P.A * dot(d, d))
            g = _acc(valid[:, l], g, (pos - cp) * s[:, None])
        return normalized(g)

    def has_neighbour(self, lists, src, pos, radius):
        idx, valid = lists(pos, radius)
        hit = np.zeros(len(pos), bool)
        for l in range(idx.shape[1]):
            hit |= valid[:, l] & (norm(src[idx[:, l]] - pos) <= radius)
        return hit

    # advectSurfacePoints: the list is over the previous positions, every slot active; only active surface slots move
    def advect(self):
        P = self.P
        r = f32(2) * P.outer
        p = self.pos
        idx, valid = walk(P, self.Rc, self.cc, np.ones(len(self.cflag), bool), p, r)
        avg, total = np.zeros((len(p), 3), f32), np.zeros(len(p), f32)
        for l in range(idx.shape[1]):
            j = idx[:, l]
            ok = valid[:, l] & ((self.cflag[j] & (PNEW | PDELETE)) == 0)
            pp = self.prev[j]
            w = weight(norm(pp - p), r)
            avg = _acc(ok, avg, (self.cpos[j] - pp) * w[:, None])
            total = _acc(ok, total, w)
        avg = np.where((total != 0)[:, None], avg / total[:, None], avg)
        live = (self.flag & PDELETE) == 0
        self.pos = np.where(live[:, None], p + avg, p).astype(f32)

    # addDeleteSurfacePoints
    def add(self):
        """the add pass, the first doCompress (which must not compress) and insertBufferedParticles; -> points added"""
        P = self.P
        n = len(self.pos)
        assert self.mDeletes <= self.mDeleteChunk            # the invariant that keeps the first doCompress from compressing
        if n == 0:
            return 0
        pos = self.pos
        grad = self.gradient(pos)
        idx, valid = self._surf(pos, P.trad)
        td = np.zeros((n, 3), f32)
        for l in range(idx.shape[1]):
            j = idx[:, l]
            d = pos - pos[j]
            length = norm(d)
            d = normalized(d)
            dt = d - dot(d, grad)[:, None] * grad
            td = _acc(valid[:, l] & (j != np.arange(n)), td, weight(length, P.trad)[:, None] * dt)
        td = np.where((norm(td) != 0)[:, None], normalized(td), td)
        out = (pos + P.mfd * td).astype(f32)
        keep = in_domain(P, out) & ~self.has_neighbour(self._surf, pos, out, P.addr)
        live = (self.flag & PDELETE) == 0
        if live.any() and self.listed:
            plane = np.minimum(np.abs(out - P.bndm), np.abs(out - P.bndp)).min(axis=1)[live]
            i2, v2 = self._surf(out, P.addr + f32(2 * POS_BOUND))
            # the added point is p + d * t with t a unit vector that moves by eps = POS_BOUND / d with the gradient; its distance
            # D to a neighbour q then moves by at most d * eps * |p - q| / D: nothing for the point's own source and its exact
            # duplicates (that distance is d |t|, 1e-6 beyond the add radius by construction), next to nothing for a near-duplicate
            ratio = [1e30]
            for l in range(i2.shape[1]):
                q = pos[i2[:, l]]
                D, pq = norm(q - out).astype(np.float64), norm(q - pos).astype(np.float64)
                m = v2[:, l] & live & (pq > 0)
                if m.any():
                    ratio.append(float((np.abs(D - np.float64(P.addr)) / (POS_BOUND * pq / np.maximum(D, 1e-30)))[m].min()))
            self.margins["an added point against the domain planes"] = (float(plane.min()), POS_BOUND)
            self.margins["an added point against the add radius, in units of what the gradient can move it"] = (min(ratio), 1.0)
        new = out[keep]                                      # survivors in ascending source order
        m = len(new)
        self.flag = np.concatenate([self.flag & ~PNEW, np.full(m, PNEW, i32)]).astype(i32)
        self.pos = np.concatenate([pos, new])
        self.normals = np.concatenate([self.normals, np.zeros((m, 3), f32)])      # new points get zero entries in every channel
        self.real = np.concatenate([self.real, np.zeros((5, m), f32)], 1)
        return m

    def delete(self):
        """-> kill calls of the three passes; every call counts, also on a slot that is deleted already"""
        P = self.P
        n = len(self.pos)
        if n == 0:
            return (0, 0, 0)
        pos = self.pos
        # pass 1: serial, greedy; the list holds the first `listed` slots, the appended points are tested but never seen
        k1 = np.zeros(n, bool)
        flag = self.flag.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            near = [norm(pos[:self.listed] - pos[i]) <= P.delr for i in range(n)]
            inside = in_domain(P, pos)
        for i in range(n):
            hit = not inside[i]
            if not hit:
                c = near[i] & ((flag[:self.listed] & PDELETE) == 0)
                if i < self.listed:
                    c[i] = False
                hit = bool(c.any())
            if hit:
                flag[i] |= PDELETE
                k1[i] = True
        # passes 2 and 3, order-free, over every slot
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            k2 = ~self.has_neighbour(self._coarse, self.cpos, pos, f32(2) * P.outer)
            lvl = self.level(pos).astype(np.float64)
        k3 = (lvl < -0.2) | (lvl > 1.2)
        self.flag = (flag | np.where(k2 | k3, PDELETE, 0)).astype(i32)
        kills = (int(k1.sum()), int(k2.sum()), int(k3.sum()))
        self.mDeletes += sum(kills)
        self.last_level = lvl
        return kills

    def compress_and_insert(self):
        did = self.mDeletes > self.mDeleteChunk
        if did:
            src = compress(self.flag)
            self.pos, self.flag, self.normals, self.real = self.pos[src], self.flag[src], self.normals[src], self.real[:, src]
            self.mDeletes, self.mDeleteChunk = 0, len(self.flag) // 20          # compress(), particle.h:614-633
        self.flag = (self.flag & ~PNEW).astype(i32)          # the second insertBufferedParticles clears PNEW everywhere
        return did

    def adddelete(self):
        added = self.add()
        kills = self.delete()
        did = self.compress_and_insert()
        self.stats = dict(added=added, kills=kills, compressed=did)

    # computeSurfaceNormals, computeAveragedNormals
    @staticmethod
    def _frame(nv):
        pick = np.abs(nv[:, 0]) < np.abs(nv[:, 1])
        vx, vy = np.array([1, 0, 0], f32), np.array([0, 1, 0], f32)
        t1 = normalized(np.where(pick[:, None], cross(nv, vx[None]), cross(nv, vy[None])).astype(f32))
        return t1, normalized(cross(nv, t1))

    @staticmethod
    def _fit_abc(F):
        sw, swx, swy, swxy, swx2, swy2, swxz, swyz, swz = F
        det = -sw * swxy * swxy + f32(2) * swx * swxy * swy - swx2 * swy * swy - swx * swx * swy2 + sw * swx2 * swy2
        v = np.stack([swxz * (-swy * swy + sw * swy2) + swyz * (-sw * swxy + swx * swy) + swz * (swxy * swy - swx * swy2),
                      swxz * (-sw * swxy + swx * swy) + swyz * (-swx * swx + sw * swx2) + swz * (swx * swxy - swx2 * swy),
                      swxz * (swxy * swy - swx * swy2) + swyz * (swx * swxy - swx2 * swy) + swz * (-swxy * swxy + swx2 * swy2)], -1)
        return det, (v * (f32(1) / det)[:, None]).astype(f32)

    def _fit(self, pos, t1, t2, radius, z_of):
        idx, valid = self._surf(pos, radius)
        F = [np.zeros(len(pos), f32) for _ in range(9)]
        for l in range(idx.shape[1]):
            j = idx[:, l]
            for near, g, _ in ghosts(self.P, self.pos[j], radius):
                m = valid[:, l] & near
                x, y, z = dot(g - pos, t1), dot(g - pos, t2), z_of(g, j)
                w = weight(norm(pos - g), radius)
                terms = (w, w * x, w * y, w * x * y, w * x * x, w * y * y, w * x * z, w * y * z, w * z)
                F = [_acc(m, f, t) for f, t in zip(F, terms)]
        return self._fit_abc(F)

    def normals_stage(self):
        P, pos = self.P, self.pos
        if len(pos) == 0:
            return
        grad = self.gradient(pos)
        nv = normalized(grad)
        t1, t2 = self._frame(nv)
        det, abc = self._fit(pos, t1, t2, P.nrad, lambda g, j: dot(g - pos, nv))
        normal = -normalized(t1 * abc[:, :1] + t2 * abc[:, 1:2] - nv)
        ok = ((self.flag & PDELETE) == 0) & (det != 0)
        if ok.any():
            self.margins["dot(gradient, normal)"] = (float(np.abs(dot(grad, normal))[ok].min()), NRM_BOUND + 5e-5)
        normal = np.where((dot(grad, normal) < 0)[:, None], -normal, normal)
        normal = np.where((det == 0)[:, None], f32(0), normal).astype(f32)
        idx, valid = self._surf(pos, P.nrad)
        nn = np.zeros((len(pos), 3), f32)
        for l in range(idx.shape[1]):
            j = idx[:, l]
            nn = _acc(valid[:, l], nn, weight(norm(pos - pos[j]), P.nrad)[:, None] * normal[j])
        self.normals = normalized(nn)

    # computeSurfaceDensities, computeSurfaceDisplacements
    def densities(self):
        P, pos = self.P, self.pos
        idx, valid = self._surf(pos, P.nrad)
        den = np.zeros(len(pos), f32)
        for l in range(idx.shape[1]):
            for near, g, _ in ghosts(P, pos[idx[:, l]], P.nrad):
                den = _acc(valid[:, l] & near, den, weight(norm(pos - g), P.nrad))
        return den

    def regularize(self):
        P, pos, N = self.P, self.pos, self.normals
        if len(pos) == 0:
            return
        den = self.densities()
        self.last_density = den
        idx, valid = self._surf(pos, P.nrad)
        dN, dT, wT = np.zeros((len(pos), 3), f32), np.zeros((len(pos), 3), f32), np.zeros(len(pos), f32)
        for l in range(idx.shape[1]):
            j = idx[:, l]
            for near, g, axis in ghosts(P, pos[j], P.nrad):
                gn = _flip(N[j], axis)
                d = pos - g
                length = norm(d)
                dt = d - dot(d, N)[:, None] * N
                w = weight(length, P.nrad) / den[j]
                cv = normalized(cross(N, -d))
                pr = normalized(gn - dot(cv, gn)[:, None] * cv)
                npj = dot(N, N + pr)
                skip = (den[j] == 0) | (dot(pr, N) < 0) | (np.abs(npj).astype(np.float64) < 1e-6)
                dn = (-dot(N + pr, d) / npj)[:, None] * N
                m = valid[:, l] & near & ~skip
                dN, dT, wT = _acc(m, dN, w[:, None] * dn), _acc(m, dT, w[:, None] * normalized(dt)), _acc(m, wT, w)
        nz = (wT != 0)[:, None]
        dN, dT = np.where(nz, dN / wT[:, None], dN), np.where(nz, dT / wT[:, None], dT)
        self.pos = (pos + (dN * f32(.75) + dT * f32(f32(.25) * P.mfd))).astype(f32)

    def constrain(self):
        P, pos = self.P, self.pos
        if len(pos) == 0:
            return
        lvl, grad = self.level(pos), self.gradient(pos)
        span = P.outer - P.inner
        hi, lo = pos - (span * (lvl - f32(1)))[:, None] * grad, pos - (span * lvl)[:, None] * grad
        self.last_level = lvl.astype(np.float64)
        self.pos = np.where((lvl > 1)[:, None], hi, np.where((lvl < 0)[:, None], lo, pos)).astype(f32)

    # the wave passes of a later frame: H += seed, wave normal, laplacian, evolveWave, curvature, smoothCurvature, seedWaves
    def waves(self):
        P, pos, N = self.P, self.pos, self.normals
        n = len(pos)
        if n == 0:
            return
        H, DtH, source, seed, amp = (r.copy() for r in self.real)
        H = H + seed
        nv = normalized(N)
        t1, t2 = self._frame(nv)
        det, abc = self._fit(pos, t1, t2, P.trad, lambda g, j: H[j])
        wn = -normalized(np.stack([abc[:, 0], abc[:, 1], -np.ones(n, f32)], -1).astype(f32))
        wn = np.where((det == 0)[:, None], f32(0), wn).astype(f32)
        t1, t2 = self._frame(N)
        idx, valid = self._surf(pos, P.trad)
        lap, wT = np.zeros(n, f32), np.zeros(n, f32)
        for l in range(idx.shape[1]):
            j = idx[:, l]
            for near, g, _ in ghosts(P, pos[j], P.trad):
                d = g - pos
                ld = norm(d)
                td = ld[:, None] * normalized(d - dot(d, N)[:, None] * N)
                dz = H[j] - H - (-wn[:, 0] / wn[:, 2]) * dot(td, t1) - (-wn[:, 1] / wn[:, 2]) * dot(td, t2)
                w = weight(norm(pos - g), P.trad)
                m = valid[:, l] & near & ~(ld.astype(np.float64) < 1e-5)
                wT = _acc(m, wT, w)
                lap = _acc(m, lap, clampf(w * f32(4) * dz / (ld * ld), f32(-100), f32(100)))
        lap = np.where(wn[:, 2] == 0, f32(0), np.where(wT != 0, lap / wT, f32(0))).astype(f32)
        damp = f32(1) + P.dt * P.wdamp
        DtH = (DtH + P.wspeed * P.wspeed * P.dt * lap) / damp
        H = (H + P.dt * DtH) / damp - seed
        DtH = clampf(DtH, -P.wmaxf * P.wamp, P.wmaxf * P.wamp)
        H = clampf(H, -P.wamp, P.wamp)
        idx, valid = self._surf(pos, P.nrad)
        curv, wT = np.zeros(n, f32), np.zeros(n, f32)
        for l in range(idx.shape[1]):
            j = idx[:, l]
            for near, g, axis in ghosts(P, pos[j], P.nrad):
                d = pos - g
                dist = norm(d)
                m = valid[:, l] & near & ~(dot(N, _flip(N[j], axis)) < 0) & ~(dist < P.nrad / f32(100))
                w = weight(dist, P.nrad)
                curv, wT = _acc(m, curv, w * dot(d, N)), _acc(m, wT, w)
        curv = np.abs(np.where(wT != 0, curv / wT, curv)).astype(f32)
        sm, wT = np.zeros(n, f32), np.zeros(n, f32)
        for l in range(idx.shape[1]):
            j = idx[:, l]
            w = weight(norm(pos - pos[j]), P.nrad)
            sm, wT = _acc(valid[:, l], sm, w * curv[j]), _acc(valid[:, l], wT, w)
        source = np.where(wT != 0, sm / wT, sm).astype(f32)
        el, er = P.ccenter - P.cradius, P.ccenter + P.cradius
        x = clampf((source - el) / (er - el), f32(0), f32(1))
        s = x * x * (f32(3) - f32(2) * x) * f32(2) - f32(1)
        top = P.wseedamp * P.wamp
        amp = clampf(amp + s * P.sstep * top, f32(0), top)
        seed = amp * P.costheta
        source = np.where(s >= 0, f32(1), f32(0))
        self.real = np.stack([H, DtH, source, seed, amp]).astype(f32)

    def run(self, name):
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if name == "advect":
                self.coarse_list(of_prev=True)
            {"accel": lambda: None, "adddelete": self.adddelete, "normals": self.normals_stage, "regularize": self.regularize,
             "constrain": self.constrain, "waves": self.waves, "advect": self.advect}[name]()
        return self.state()


def direction_table(P):
    """the directions of initFines, i then phi: fp32 sin / cos (the fp64 function rounded once) and the fp32 running phi"""
    def sinf(x):
        return f32(np.sin(np.float64(f32(x))))

    def cosf(x):
        return f32(np.cos(np.float64(f32(x))))
    disc = int(f32(f32(3) * f32(P.outer + P.inner)) / P.mfd)
    out = []
    for i in range(disc // 2 + 1):
        theta = f32(f32(i) * P.dtheta)
        d2 = f32(np.floor(2 * np.pi * np.float64(sinf(theta)) / np.float64(P.dtheta)) + 1)
        phi = f32(0)
        with np.errstate(divide="ignore"):
            step = f32(2 * np.pi / np.float64(d2))
        while np.float64(phi) < 2 * np.pi:
            out.append([sinf(theta) * cosf(phi), cosf(theta), sinf(theta) * sinf(phi)])
            phi = f32(phi + step)
    return np.array(out, f32)


def init_fines(P, Rc, gridflags, cpos, cflag, dirs=None):
    """initFines over (coarse particle, direction), compacted in the order particle, then i, then phi -> positions.  dirs: the
    library's host table where a test has it, else the model's own"""
    dirs = direction_table(P) if dirs is None else np.asarray(dirs, f32).reshape(-1, 3)
    live = (cflag & PDELETE) == 0
    sz, sy, sx = gridflags.shape
    cell = cpos.astype(np.int64)
    assert (cell[live] >= 1).all() and (cell[live] <= np.array([sx, sy, sz]) - 2).all()        # the precondition of the contract
    near = np.zeros(len(cpos), bool)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                x, y, z = (np.clip(cell[:, a] + d, 0, m - 1) for a, d, m in ((0, i, sx), (1, j, sy), (2, k, sz)))
                near |= (gridflags[z, y, x] & 1) == 0
    cc = cell_list(cpos, P.res, Rc)
    out = []
    r, r2 = f32(2) * P.outer, P.outer * P.outer
    for p in np.nonzero(live & near)[0]:
        cand = (cpos[p] + P.outer * dirs).astype(f32)
        idx, valid = walk(P, Rc, cc, live, cand, r)
        ok = np.ones(len(cand), bool)
        for l in range(idx.shape[1]):
            d = cand - cpos[idx[:, l]]
            ok &= ~(valid[:, l] & (idx[:, l] != p) & (dot(d, d) < r2))
        out.append(cand[ok])
    return np.concatenate(out) if out else np.zeros((0, 3), f32)


def model_call_case(P, R, c, f, nb, trace=None, dirs=None):
    """a whole call in the model from the inputs c (call_case): frame f, nb maintenance iterations -> (the model, stats per iteration,
    displaced points).  trace(iteration, stage, model, before) is called around every stage with before = True / False"""
    mdl = Model(P, R, c)
    its = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if f == 0:
            pos = init_fines(P, int(R[0]), c["flags"], mdl.cpos, mdl.cflag, dirs)
            n = len(pos)
            mdl.pos, mdl.flag, mdl.normals, mdl.real = pos, np.zeros(n, i32), np.zeros((n, 3), f32), np.zeros((5, n), f32)
            mdl.mDeletes, mdl.mDeleteChunk = 0, n // 20
            mdl.init = n
            mdl.surface_list(empty=True)                     # nothing fills the surface list after initFines
            count = 6 * nb
        else:
            mdl.run("advect")
            mdl.surface_list()
            mdl.coarse_list()
            count = nb
        for it in range(count):
            for name in ("adddelete", "accel", "normals", "regularize", "accel", "constrain", "accel"):
                if trace is not None:
                    trace(it, name, mdl, True)
                if name == "accel":
                    mdl.surface_list()
                else:
                    mdl.run(name)
                if trace is not None:
                    trace(it, name, mdl, False)
            its.append(dict(mdl.stats, size=len(mdl.pos)))
        if f == 0:
            mdl.real[[0, 1, 3, 4]] = 0
        else:
            mdl.run("waves")
    live = (mdl.flag & PDELETE) == 0
    displaced = (mdl.pos[live] + mdl.normals[live] * mdl.real[0][live][:, None]).astype(f32)
    return mdl, its, displaced


_CALLS = {}


def model_call(G, f):
    """whole call f of the recorded run in the model, once per process: -> (state after, stats per iteration, displaced points, the
    states before and after every stage of the iterations 0, 1 and the last, keyed (iteration, position in the iteration))"""
    if f not in _CALLS:
        c = call_case(G, f)
        nb = int(G["set0/args"][2])
        last = (6 * nb if f == 0 else nb) - 1
        stages, at = {}, [0]

        def trace(it, name, mdl, before):
            if before:
                at[0] = at[0] + 1 if it == trace.it else 0
                trace.it = it
            if it in (0, 1, last):
                rec = stages.setdefault((it, at[0]), dict(name=name))
                rec["before" if before else "after"] = dict({k: np.array(v) for k, v in mdl.state().items()}, listed=mdl.listed, stats=dict(mdl.stats))
        trace.it = -1
        mdl, its, disp = model_call_case(par_of(G, 0, f), G["set0/res"], c, f, nb, trace)
        _CALLS[f] = (mdl.state(), its, disp, stages)
    return _CALLS[f]


ITERATION = ("adddelete", "accel", "normals", "regularize", "accel", "constrain", "accel")


def stage_cases(G):
    """the recorded stages inside the calls (st<f>/..., tools/record_surfturb.py) -> [(what, stage name, the case before the stage,
    the reference's state after it)]: the first two and the last maintenance iteration of frame 0, everything of frames 1 and 2"""
    out = []
    nb = int(G["set0/args"][2])
    for f in range(3):
        base = call_case(G, f)
        key = "st%d/" % f
        last = None
        if f:
            after = dict(state(G, "call%d/before" % f), pos=G[key + "advect/pos"])
            out.append(("frame %d" % f, "advect", dict(base), after))
        count = 6 * nb if f == 0 else nb
        for it in sorted(set((0, 1, count - 1))):
            cur = state(G, key + "%d/start" % it)
            for j, name in enumerate(ITERATION):
                if name == "accel":
                    continue
                c = dict(base, **cur)
                if f == 0 and it == 0 and j == 0:
                    c["listed"] = 0             # nothing fills the surface list after initFines
                nxt = dict(cur, sizes=G[key + "%d/%d/sizes" % (it, j)])
                for k in KEYS:
                    if key + "%d/%d/%s" % (it, j, k) in G:
                        nxt[k] = G[key + "%d/%d/%s" % (it, j, k)]
                out.append(("frame %d iteration %d" % (f, it), name, c, nxt))
                cur = last = nxt
        if f:
            c = dict(base, **last)
            out.append(("frame %d" % f, "waves", c, dict(last, real=G[key + "waves/real"])))
    return out


def model_stage(G, i):
    """stage i of the recorded chain from its recorded inputs -> (the model, its state after the stage)"""
    c = chain_case(G, i)
    mdl = Model(par_of(G, 0, c["frame"]), c["R"], c)
    return mdl, mdl.run(chain_names(G)[i])


# ---- HIP (or the host program) against the model
def compare_model(got, want, what=""):
    """the rule of the contract for an implementation against the model: sizes, delete bookkeeping and flags equal; every value equal bit
    for bit (two NaNs count as equal) except at no more than ONE point, where the fp64 exp / log of the two sides may differ in the last
    place -- and that point stays within the bounds.  -> the number of differing points (printed by the callers)"""
    assert [int(x) for x in got["sizes"][:3]] == [int(x) for x in want["sizes"][:3]], (what, got["sizes"], want["sizes"])
    assert np.array_equal(got["flag"], want["flag"]), what
    n = len(want["flag"])
    bad = np.zeros(n, bool)
    for k, bound in (("pos", POS_BOUND), ("normals", NRM_BOUND), ("real", NRM_BOUND)):
        g, w = np.ascontiguousarray(got[k], f32), np.ascontiguousarray(want[k], f32)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        differ = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
        if differ.any():
            with np.errstate(invalid="ignore"):
                worst = float(np.abs(g.astype(np.float64) - w)[differ].max())
            assert worst <= bound, (what, k, worst, bound)
        bad |= differ.any(axis=0) if k == "real" else differ.any(axis=1)
    count = int(bad.sum())
    assert count <= 1, (what, "points that differ from the model:", np.nonzero(bad)[0][:10].tolist())
    return count


EDGE_STAGES = ("adddelete", "normals", "regularize", "constrain", "waves", "advect")
EDGE_CASES = ("n0", "n1", "n63", "n64", "n65", "n257", "one_cell", "planes", "compress", "no_compress", "line_up", "line_down")


def edge_case(G, name):
    """a small state at an edge of the code: coarse particles on a jittered lattice through the whole domain, so that points at the
    ghost planes and in the corners have a level and a gradient; surface points per case.  From 63 points on: exact duplicates, points
    outside the domain, deleted slots holding inf / NaN / 1e30"""
    rng = np.random.RandomState(EDGE_CASES.index(name) + 3)
    axis = np.arange(2.5, 10.0, 1.0)
    cpos = (np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.2, 0.2, (512, 3))).astype(f32)
    cflag = np.zeros(512, i32)
    cflag[[5, 77]], cflag[[9, 300]] = PDELETE, PNEW
    prev = (cpos + rng.uniform(-0.05, 0.05, cpos.shape)).astype(f32)
    mdel, chunk = 0, 3
    if name == "one_cell":
        pos = f32(5.01) + rng.uniform(0, 0.2, (90, 3))
    elif name == "planes":
        # twelve points at each of the six planes (one exactly on it), in two corners (three ghosts each) and inside
        centres = [[2.2, 6, 6], [9.8, 6, 6], [6, 2.2, 6], [6, 9.8, 6], [6, 6, 2.2], [6, 6, 9.8], [2.3, 2.3, 2.3], [9.7, 9.7, 2.2], [6, 6, 6]]
        pos = np.concatenate([np.array(c) + rng.uniform(-0.3, 0.3, (12, 3)) for c in centres])
        pos[5], pos[17] = [2, 6, 6], [10, 6.1, 5.9]
    elif name in ("line_up", "line_down"):
        # nine points half a meanFineDistance apart, in ascending and in descending slot order: the greedy pass needs nine rounds
        x = f32(4) + G["set0/par"][3] * f32(0.5) * np.arange(9, dtype=f32)[::1 if name == "line_up" else -1]
        pos = np.stack([x, np.full(9, 5, f32), np.full(9, 5, f32)], 1)
    elif name in ("compress", "no_compress"):
        pos = rng.uniform(4, 6, (120, 3))
        pos[rng.choice(120, 12, replace=False)] += 100            # twelve kills outside the domain
        mdel, chunk = (2, 6) if name == "compress" else (0, 100000)         # every kill call counts: far more than twelve
    else:
        n = int(name[1:])
        pos = rng.uniform(3, 3 + 0.6 * max(n, 1) ** (1 / 3.0), (n, 3))
    pos = pos.astype(f32)
    n = len(pos)
    flag = np.zeros(n, i32)
    if n >= 63:
        pos[3] = pos[40]
        pos[7], pos[11] = [1.5, 5, 5], [5, 10.5, 5]
        pos[20], pos[21], pos[22] = [np.nan, 5, 5], [np.inf, -np.inf, 5], [1e30, 5, 5]
        flag[[20, 21, 22, 30]] = PDELETE
        mdel += 0 if name in ("compress", "no_compress") else 2
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)).astype(f32)
    if name == "planes":
        nrm[:12] = [-1, 0, 0]               # facing the plane x-: the images' flipped normals fail the projected-normal test
    real = rng.uniform(-0.2, 0.2, (5, n)).astype(f32)
    real[4] = np.abs(real[4])
    return dict(args=G["set0/args"], frame=3, nb=2, R=G["set0/res"], flags=G["flags"], cpos=cpos, cflag=cflag, prev=prev, pos=pos, flag=flag,
                normals=nrm, real=real, sizes=np.array([n, mdel, chunk, 0, 3, 512], i64))


def edge_model(G, name, stage):
    c = edge_case(G, name)
    mdl = Model(par_of(G, 0, c["frame"]), c["R"], c)
    return c, mdl, mdl.run(stage)

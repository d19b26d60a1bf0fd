"""numpy statement of the particle->grid transfers, for the fp32-atomic mode (setDeterministicP2G(False)).

What the model is.  A transfer is a scatter of per-particle terms: each active particle adds 8 weights and 8 weighted values per
component to 8 grid entries.  The terms themselves do not depend on the order of summation, only the sums do.  The model therefore
forms every term exactly as the kernels do --

  * index and fractions as build_index / build_index_shift of csrc/common.h: fp32 subtraction for the fraction,
    s0 = float(1.0 - double(s1)), the lower clamps, the upper clamp on px (build_index: the fork) or on the integer index
    (build_index_shift), no upper z clamp and Z = 0 in 2-D;
  * the eight weights as single fp32 products in the kernels' association order, sa*fa, then ta*(...), and the weighted value as one
    more fp32 product w*val (the library is built with -ffp-contract=off, so numpy float32 products are the same bits)

-- and returns per grid entry the exact sum S of the terms (fp64 accumulation; the fp64 rounding of at most a few thousand fp32
terms is 2^-29 of the fp32 bound below and is not accounted for), the number of terms k and A = sum |term|.

What follows from it.  ANY order or tree of fp32 additions of the same k terms -- LDS atomics, global atomics, DPP merges, a serial
loop -- returns got with

        |got - S| <= gamma(k - 1) * A + u * |S|,      u = 2^-24, gamma(m) = m u / (1 - m u)

(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; the last term is the rounding of S itself).  Where all terms
are multiples of one power of two and A stays below 2^24 times it, every partial sum is exact and got == S bit for bit.
"""
import numpy as np

PDELETE = 1 << 10
U = 2.0 ** -24
STOMP = np.float32(1e-6)          # weight.stomp(1e-6) of k_p2g_mac_finish / the w < 1e-6 test of k_safe_div_real
DIVIDED_ABOVE = 1e-3              # quotients are checked where the model's weight sum is at least this
f32, f64 = np.float32, np.float64


def gamma(m):
    m = np.asarray(m, f64)
    return m * U / (1.0 - m * U)


def _axis(p, n, shifted, clamp_hi):
    """one axis of BUILD_INDEX (p = pos - 0.5; upper clamp on p) or of the shifted half of BUILD_INDEX_SHIFT (p = pos; upper clamp on
    the integer index) -> index, w0, w1"""
    assert p.dtype == f32
    i = p.astype(np.int32)                     # (int)p: truncation toward zero
    w1 = p - i.astype(f32)
    w0 = (1.0 - w1.astype(f64)).astype(f32)
    lo = p < f32(0)
    i[lo], w0[lo], w1[lo] = 0, 1, 0
    if clamp_hi:
        hi = (i >= n - 1) if shifted else (p >= f32(n - 1))
        i[hi], w0[hi], w1[hi] = n - 2, 0, 1
    return i, w0, w1


def build_index(dims, pos, shifted=False):
    """-> (xi, yi, zi), (s0, s1), (t0, t1), (f0, f1) of all particles; pos is [3][np] float32"""
    sx, sy, sz = dims
    h = f32(0.0 if shifted else 0.5)
    xi, s0, s1 = _axis(pos[0] - h, sx, shifted, True)
    yi, t0, t1 = _axis(pos[1] - h, sy, shifted, True)
    zi, f0, f1 = _axis(pos[2] - h, sz, shifted, sz > 1)
    return (xi.astype(np.int64), yi.astype(np.int64), zi.astype(np.int64)), (s0, s1), (t0, t1), (f0, f1)


def _corners(dims, s, t, f):
    """the eight weights (single fp32 products, t*(s*f)) and address offsets in the kernels' corner order"""
    sx, sy, sz = dims
    Y, Z = sx, (sx * sy if sz > 1 else 0)
    sf = [s[0] * f[0], s[1] * f[0], s[0] * f[1], s[1] * f[1]]              # s0f0 s1f0 s0f1 s1f1
    w = [t[0] * sf[0], t[0] * sf[1], t[1] * sf[0], t[1] * sf[1], t[0] * sf[2], t[0] * sf[3], t[1] * sf[2], t[1] * sf[3]]
    assert all(x.dtype == f32 for x in w)
    return np.stack(w, 1), np.array([0, 1, Y, 1 + Y, Z, 1 + Z, Y + Z, 1 + Y + Z], np.int64)


class Sums:
    """per grid entry: exact sum S (fp64), number of terms k, A = sum |term| (fp64); and the bound every fp32 summation meets"""

    def __init__(self, size, addr, term):
        assert term.dtype == f32 and addr.shape == term.shape
        addr, term = addr.ravel(), term.ravel().astype(f64)
        assert addr.size == 0 or (addr.min() >= 0 and addr.max() < size), "a term outside the grid"
        self.S, self.A = np.zeros(size, f64), np.zeros(size, f64)
        np.add.at(self.S, addr, term)
        np.add.at(self.A, addr, np.abs(term))
        self.k = np.bincount(addr, minlength=size).astype(np.int64)
        nz = np.abs(term[term != 0])
        self.min_term = float(nz.min()) if nz.size else np.inf

    @property
    def bound(self):
        return gamma(np.maximum(self.k - 1, 0)) * self.A + U * np.abs(self.S)

    def tiled(self, reps):
        o = object.__new__(Sums)
        o.S, o.A, o.k, o.min_term = np.tile(self.S, reps), np.tile(self.A, reps), np.tile(self.k, reps), self.min_term
        return o


def active(pflag, ptype=None, exclude=0):
    a = (pflag & PDELETE) == 0
    if ptype is not None:
        a &= (ptype & exclude) == 0
    return a


def mac_accum(dims, pos, pflag, pvel, ptype=None, exclude=0):
    """mf_map_parts_to_mac_accum: the raw sums.  -> dict(weight=Sums, vel=Sums over the 3n face entries,
    keys=[3][np] base address of each component inside its plane (-1: inactive particle),
    addr=[np][24] flat addresses into the 3n entries (-1: inactive))"""
    sx, sy, sz = dims
    n = sx * sy * sz
    npart = pos.shape[1]
    act = active(pflag, ptype, exclude)
    P = np.ascontiguousarray(pos[:, act])
    V = pvel[:, act]
    (bx, by, bz), bs, bt, bf = build_index(dims, P, False)
    (hx, hy, hz), hs, ht, hf = build_index(dims, P, True)
    comps = [((bz * sy + by) * sx + hx, hs, bt, bf),       # x faces: shifted along x
             ((bz * sy + hy) * sx + bx, bs, ht, bf),       # y faces
             ((hz * sy + by) * sx + bx, bs, bt, hf)]       # z faces
    keys = np.full((3, npart), -1, np.int64)
    addr = np.full((npart, 24), -1, np.int64)
    A, W, T = [], [], []
    for c, (base, s, t, f) in enumerate(comps):
        w, off = _corners(dims, s, t, f)
        a = base[:, None] + off[None, :]
        assert a.size == 0 or (a.min() >= 0 and a.max() < n), "a face stencil outside its plane"
        keys[c, act] = base
        addr[act, 8 * c:8 * c + 8] = c * n + a
        A.append(c * n + a); W.append(w); T.append(w * V[c][:, None])
    A, W, T = np.concatenate(A, 1), np.concatenate(W, 1), np.concatenate(T, 1)
    assert T.dtype == f32
    return dict(weight=Sums(3 * n, A, W), vel=Sums(3 * n, A, T), keys=keys, addr=addr)


def cell_accum(dims, ncomp, pos, pflag, psrc):
    """mf_map_parts_to_grid before the division: -> dict(weight=Sums over n cells, val=Sums over ncomp*n); psrc is [np] or [3][np]"""
    sx, sy, sz = dims
    n = sx * sy * sz
    act = active(pflag)
    P = np.ascontiguousarray(pos[:, act])
    src = np.asarray(psrc, f32).reshape(ncomp, -1)[:, act]
    (bx, by, bz), bs, bt, bf = build_index(dims, P, False)
    w, off = _corners(dims, bs, bt, bf)
    Z = sx * sy if sz > 1 else 0
    a = (bx + sx * by + Z * bz)[:, None] + off[None, :]
    wsum = Sums(n, a, w)
    A = np.concatenate([c * n + a for c in range(ncomp)], 1)
    T = np.concatenate([w * src[c][:, None] for c in range(ncomp)], 1)
    return dict(weight=wsum, val=Sums(ncomp * n, A, T))


def mac_finish(vel, weight):
    """k_p2g_mac_finish on fp32 sums: weight.stomp(1e-6), vel.safeDivide(weight) -> (vel, weight); velOld is a copy of vel"""
    vel, weight = np.asarray(vel, f32), np.asarray(weight, f32)
    w = np.where(weight < STOMP, f32(0), weight)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(w != 0, vel / w, vel)
    return v.astype(f32), w


def safe_div(target, wsum, ncomp):
    """k_safe_div_real on fp32 sums: 0 where the weight is below 1e-6, the quotient elsewhere"""
    target, w = np.asarray(target, f32).reshape(ncomp, -1), np.asarray(wsum, f32).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(w[None] < STOMP, f32(0), target / w[None])
    return q.astype(f32).ravel()


def quotient_classes(num, den):
    """entries of a divided output by what can be said about them from the model alone.
    num / den: Sums of the numerator and (tiled to the same length) the weight.  ->
      q, qbound   the model's quotient and |got - q| <= (dv + |q| dw) / (w - dw) + u |q|, valid where `divided`
      divided     w >= 1e-3
      stomped     w + dw < 1e-6: the fp32 weight sum is below the threshold in any order, so the stomped value is returned
      left_out    the rest: the order of summation may decide on which side of the threshold the entry falls"""
    w, dw, dv = den.S, den.bound, num.bound
    divided = w >= DIVIDED_ABOVE
    stomped = w < float(STOMP) - dw
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(divided, num.S / w, 0.0)
        qb = np.where(divided, (dv + np.abs(q) * dw) / (w - dw) + U * np.abs(q), np.inf)
    return q, qb, divided, stomped, ~(divided | stomped)

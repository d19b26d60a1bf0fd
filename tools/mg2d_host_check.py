"""Driver of tools/mg2d_host_check.hip (its header has the build line): runs the stand-alone host program on every stage system of
tests/mg2d_cases.py and compares each output with the numpy model tests/mg2d_model.py bit for bit -- the types, the operators, b and
x of every level after one V-cycle, the coarsest CG's iteration count, the two "found" flags -- with the tail taking every level, no
level but the coarsest, and the default hand-over; and the program's sorted level-1 paths with the reference's recorded ones
(tests/golden/mg2d.npz, `paths`): the order that std::sort leaves inside one (sc, U) group is part of the contract.  The program is
a separate process; nothing is loaded into this one.

    python tools/mg2d_host_check.py <path to mg2d_host_check>
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mg2d_cases as C  # noqa: E402
import mg2d_model as M  # noqa: E402

f32, i32 = np.float32, np.int32


def run(exe, dims, A, rhs, accuracy, tail_verts):
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(a, "wb") as f:
            f.write(np.array(dims[:2], i32).tobytes() + np.array([accuracy], f32).tobytes())
            for arr in list(A) + [rhs]:
                f.write(np.ascontiguousarray(arr, f32).tobytes())
        r = subprocess.run([exe, a, b, str(tail_verts)], capture_output=True, text=True)
        assert r.returncode == 0, (dims, r.returncode, r.stderr[-3000:])
        return open(b, "rb").read()


class Take(object):
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def __call__(self, dtype, *shape):
        a = np.frombuffer(self.raw, dtype, int(np.prod(shape)), self.at).reshape(shape)
        self.at += a.nbytes
        return a

    def done(self):
        assert self.at == len(self.raw), (self.at, len(self.raw))


def check(exe, g, tag, tail_verts):
    dims, A, rhs = C.stage_system(tag)
    H = C.model_hierarchy(g, tag, dims, A)
    cyc = M.vcycle(H, rhs)
    take = Take(run(exe, dims, A, rhs, 1e-8, tail_verts))
    nl, tail_first, cg, nonzero, trivial, npaths = (int(v) for v in take(i32, 6))
    paths = take(i32, npaths, 12)
    what = "%s with the hand-over at %d vertices" % (tag, tail_verts)
    assert paths.tobytes() == np.ascontiguousarray(g["paths"]).tobytes(), what + ": the sorted paths are not the reference's"
    assert nl == H.nl and tail_first == C.expected_tail_first(H.sizes, tail_verts), what
    assert cg == cyc["cg_iters"] and bool(nonzero) == H.nonzero_sum_found and bool(trivial) == H.trivial_found, what
    for l in range(nl):
        sx, sy, active = (int(v) for v in take(i32, 3))
        n = sx * sy
        assert (sx, sy, 1) == H.sizes[l] and active == H.active[l], (what, l)
        t, a, b, x = take(np.uint8, n), take(f32, 3 if l == 0 else 5, n).copy(), take(f32, n), take(f32, n)
        act = H.t[l] != 0
        assert t.tobytes() == H.t[l].tobytes(), "%s: vertex types of level %d" % (what, l)
        assert a[:, act].tobytes() == H.A2[l][:, act].tobytes(), "%s: operator of level %d" % (what, l)
        # the model starts every vector at 0, the program at NaN: compare what a pass writes (b and x of active vertices; x of every
        # vertex above level 0, where the restriction sets it to 0)
        assert b[act].tobytes() == cyc["b"][l][act].tobytes(), "%s: b of level %d" % (what, l)
        where = act if l == 0 else np.ones(n, bool)
        assert x[where].tobytes() == cyc["x"][l][where].tobytes(), "%s: x of level %d" % (what, l)
    take.done()


def main(exe):
    g = np.load(C.GOLDEN)
    tags = C.stage_tags()
    for tag in tags:
        for tail_verts in (0, C.TAIL_VERTS, 10 ** 9):
            check(exe, g, tag, tail_verts)
    print("mg2d host check: %d stage systems x 3 hand-overs equal the model; the sorted paths equal the reference's" % len(tags))


if __name__ == "__main__":
    main(sys.argv[1])

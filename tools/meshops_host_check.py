"""Driver of tools/meshops_host_check.hip (its header has the build line): runs the stand-alone host program on every case of
tests/meshops_model.py and compares each output with the numpy model bit for bit.  The program is a separate process; nothing is
loaded into this one.

    python tools/meshops_host_check.py <path to meshops_host_check>
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meshops_model as M  # noqa: E402

f32, f64, i32 = np.float32, np.float64, np.int32


def run(exe, mode, m, *args):
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(a, "wb") as f:
            f.write(np.array([m["pos"].shape[0], m["tris"].shape[0]], np.int64).tobytes())
            for k in ("pos", "normal"):
                f.write(np.ascontiguousarray(m[k].T).tobytes())
            f.write(m["flags"].tobytes() + np.ascontiguousarray(m["tris"].T).tobytes() + m["tflags"].tobytes())
        r = subprocess.run([exe, mode, a, b] + [repr(float(x)) if isinstance(x, (float, f32)) else str(x) for x in args], capture_output=True, text=True)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-2000:])
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


def check_conn(exe, name, m, refused=None):
    n, t = m["pos"].shape[0], m["tris"].shape[0]
    take = Take(run(exe, "conn", m))
    counts = take(i32, 4)
    if refused == "repeated":
        assert counts[2] == 4 and counts[3] == -1, counts
        return take.done()
    opp, singles, multi = M.corners(m["tris"])
    assert counts.tolist() == [singles, multi, -1, -1], (name, counts)
    r = M.ring(m["tris"], n)
    assert np.array_equal(take(i32, 3 * t), opp), name
    assert np.array_equal(take(i32, n + 1), r[0]), name
    ln = int(take(i32, 1)[0])
    assert ln == r[1].size and np.array_equal(take(i32, ln), r[1]), name
    assert np.array_equal(take(i32, n + 1), r[2]) and np.array_equal(take(i32, 3 * t), r[3]), name
    take.done()


def main(exe):
    for name, make in M.CONNECTIVITY_CASES.items():
        check_conn(exe, name, make())
    for name, (make, _) in M.REFUSED_CASES.items():
        check_conn(exe, name, make(), refused=name)
    for name, (make, _) in M.KILL_REFUSED.items():
        check_conn(exe, name, make()[0])
    print("connectivity: %d cases equal the model" % (len(M.CONNECTIVITY_CASES) + len(M.REFUSED_CASES) + len(M.KILL_REFUSED)))
    for name, make in M.SMOOTH_CASES.items():
        m, dt, strength, steps, minLength = make()
        n, t = m["pos"].shape[0], m["tris"].shape[0]
        str_ = min(f32(f32(dt) * f32(strength)), f32(1))
        take = Take(run(exe, "smooth", m, str_, f32(minLength), steps))
        pos, terms = take(f32, 3, n).T, take(f64, 4, t).T
        take.done()
        c = M.connectivity("check", m)
        want, free = m["pos"].copy(), (m["flags"] & 1) == 0
        for _ in range(steps):
            want[free] = M.smooth_step(want, c["nodeOff"], c["nodes"], c["triOff"], str_, f32(minLength))[free]
        assert pos.tobytes() == want.tobytes(), name
        assert np.ascontiguousarray(terms).tobytes() == M.volume_terms(want, m["tris"]).tobytes(), name
    print("smoothMesh: %d cases equal the model (positions after the steps, volume terms)" % len(M.SMOOTH_CASES))
    for name, make in M.KILL_CASES.items():
        m, elements = make()
        take = Take(run(exe, "kill", m, elements))
        nn, nt = take(np.int64, 2)
        got = {"pos": take(f32, 3, nn).T, "normal": take(f32, 3, nn).T, "flags": take(i32, nn), "tris": take(i32, 3, nt).T, "tflags": take(i32, nt)}
        take.done()
        want, _ = M.kill_small_components(m, elements)
        for k in M.MESH_KEYS:
            assert np.ascontiguousarray(got[k]).tobytes() == want[k].tobytes(), (name, k)
    print("killSmallComponents: %d cases equal the model" % len(M.KILL_CASES))


if __name__ == "__main__":
    main(sys.argv[1])

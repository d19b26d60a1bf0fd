"""Driver of tools/reinit_host_check.hip (its header has the build line): the bodies of mantaflow_amd/csrc/reinit_cells.h on the host,
serially, under the host sanitizers, on every fixture case of tests/reinit_model.py.  Both the literal serial call and the call in rounds
must equal the recorded reference bit for bit in phi and vel, the model's flags and keys, and the model's counters; the program must
end clean.  Usage: python tools/reinit_host_check.py <program> [--counts] [--sweep]
With --sweep every input of tests/reinit_cases.py follows (240 random cases and the designed families in their variants: whole planes of
equal keys, keys on a window's end, signed zeros, a far field of +-1000, maxTime below a cell and beyond the grid, with and without
correctOuterLayer and walls): both calls must equal the model's serial statement bit for bit, and the four counters of the call in
rounds the model's statement in rounds, case by case; every case that differs is named before the run fails.
With --counts nothing is compared with the fixture's counters: the windows, sub-rounds, pops and serial marches of every case are
printed (the program may have been built with another -DMF_REINIT_DELTA=...), and phi / vel must still be the reference's."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reinit_model as M  # noqa: E402

f32 = np.float32


def run(prog, tmp, c):
    n, vel = c["n"], c["velocity"]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        np.array(list(c["dims"]) + [0 if vel is None else 1, int(c["ignoreWalls"]), int(c["correctOuterLayer"]), c["obstacleType"]], np.int32).tofile(f)
        np.array([c["maxTime"]], f32).tofile(f)
        c["phi"].astype(f32).tofile(f)
        c["flags"].astype(np.int32).tofile(f)
        if vel is not None:
            vel.astype(f32).tofile(f)
    r = subprocess.run([prog, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(fout, "rb").read()
    per = n * (3 + (3 if vel is not None else 0))
    w = np.frombuffer(raw, np.uint32, 2 * per)
    st = np.frombuffer(raw, np.int64, offset=8 * per)
    assert st.size == 10
    out = []
    for q in range(2):
        b, o = w[q * per:(q + 1) * per], n
        d = {"phi": b[:n].view(f32), "vel": None}
        if vel is not None:
            d["vel"] = b[o:o + 3 * n].view(f32)
            o += 3 * n
        d["fm"], d["key"] = b[o:o + n].view(np.int32), b[o + n:o + 2 * n].view(f32)
        out.append(d)
    return out[0], out[1], st[:2], st[2:].reshape(4, 2)


def sweep(prog, tmp):
    """every input of tests/reinit_cases.py against the live model; returns the totals and the names of the cases that differ"""
    import reinit_cases as C
    total, bad, flagged = np.zeros((4, 2), np.int64), [], 0
    names = list(C.SWEEP) + list(C.DESIGNED)
    for name in names:
        c, want, stats = C.get(name), C.run(name, "serial"), C.run(name, "rounds")["stats"]
        serial, rounds, spops, st = run(prog, tmp, c)
        diff = []
        for tag, r in (("serial", serial), ("rounds", rounds)):
            for k in ("phi", "vel", "fm", "key"):
                d = None if want[k] is None else C.first_difference(want[k], r[k])
                if d is not None:
                    diff.append("%s %s: cell %d, model %r, program %r" % ((tag, k) + d))
        if tuple(spops) != want["stats"]["pops"]:
            diff.append("serial pops %s, model %s" % (tuple(spops), want["stats"]["pops"]))
        wst = [list(stats[k]) for k in ("windows", "subrounds", "pops", "serial")]
        if st.tolist() != wst:
            diff.append("windows, sub-rounds, pops, serial %s, model %s" % (st.tolist(), wst))
        if diff:
            bad.append(c["name"])
            print("DIFFERS %s (%s): %s" % (c["name"], "x".join(str(s) for s in c["dims"]), "; ".join(diff[:4])))
        flagged += max(stats["serial"])
        total += st
    print("reinit_host_check --sweep: %d cases (%d random, %d designed; the model flags %d), %d differ from the model; windows %s sub-rounds %s "
          "pops %s serial %s" % ((len(names), len(C.SWEEP), len(C.DESIGNED), flagged, len(bad)) + tuple(str(tuple(x)) for x in total.tolist())))
    return bad


def main(prog, counts=False, with_sweep=False):
    G = np.load(M.GOLDEN)
    total = np.zeros((4, 2), np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        for name in M.CASES:
            c = M.case(name)
            serial, rounds, spops, st = run(prog, tmp, c)
            for tag, r in (("serial", serial), ("rounds", rounds)):
                for k in ("phi", "vel", "fm", "key"):
                    if r[k] is None:
                        continue
                    a = r[k].astype(np.int8) if k == "fm" else r[k]
                    if name + "/" + k in G.files:
                        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(G[name + "/" + k]).view(np.uint8)), (name, tag, k)
                    else:
                        assert M.sha(a) == str(G[name + "/" + k + "_sha"]), (name, tag, k)
            want = G[name + "/stats"]
            assert np.array_equal(spops, np.where(want[3] == 1, want[2], spops)), (name, spops, want)
            if counts:
                print("%-22s windows %-10s sub-rounds %-10s pops %-14s serial %s" % ((name,) + tuple(str(tuple(x)) for x in st.tolist())))
            else:
                assert np.array_equal(st, want), (name, st.tolist(), want.tolist())
            total += st
    print("reinit_host_check: %d cases equal the reference and the model, no sanitizer report; windows %s sub-rounds %s pops %s serial %s"
          % ((len(M.CASES),) + tuple(str(tuple(x)) for x in total.tolist())))
    if with_sweep:
        with tempfile.TemporaryDirectory() as tmp:
            bad = sweep(prog, tmp)
        assert not bad, "%d sweep cases differ from the model: %s" % (len(bad), bad)


if __name__ == "__main__":
    main(sys.argv[1], "--counts" in sys.argv[2:], "--sweep" in sys.argv[2:])

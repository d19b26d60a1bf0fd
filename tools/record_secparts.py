"""Recorder of tests/golden/secparts.npz: the reference's outputs for the fixture cases of tests/secparts_model.py (inputs are
regenerated from its seeded generators, never stored) and for the recorded dam-break loop.  No test runs this; it needs the reference
checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays in a scratch directory outside the tree.
Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/secondaryparticles.cpp $B/plugin/secondaryparticles.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libsecparts_rec.so $B/plugin/secondaryparticles.cpp tools/secparts_record.cpp \\
        -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_secparts.py $B/libsecparts_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

All cases run in this one process in a fixed order, because the random streams of the two sampling kernels are process-wide: per
mode the sampling cases in SAMPLE_ORDER, then (mode "single") the loop.  The file holds: <potentials case>/{potTA, potWC, potKE,
ratio, normal}; sample/<mode>/<case>/{pos, flag, ch0..ch3, sizes, start}: the system after the calls, its size after each call and
the stream offset at which the case began; update/<case>/... and delete/<case>/...: the system after the call (its length tells
whether doCompress compressed); set/<case>/{flags, vel}; loop/{counts, pots, start}.  Stream offsets are kept by counting the reals
of each call from the reference's particle counts (single: 3 per emitting or negative cell + 4 per particle; multiple: 4 per
particle).  The conditions each case exists for are asserted here.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secparts_model as M  # noqa: E402

f32 = np.float32


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def soa(g):
    """[z][y][x][3] -> [3][n]"""
    return np.ascontiguousarray(np.asarray(g, f32).reshape(-1, 3).T)


def aos(a, shape):
    return np.ascontiguousarray(a.reshape(3, -1).T.reshape(shape + (3,)))


def fc(x):
    return ctypes.c_float(float(x))


def sys_arrays(parts, cap):
    """SoA arrays of capacity cap for the shim's Sec"""
    n = parts.size()
    pos, pv, pf = np.zeros((3, cap), f32), np.zeros((3, cap), f32), np.zeros((3, cap), f32)
    flag, pl, px = np.zeros(cap, np.int32), np.zeros(cap, f32), np.zeros(cap, np.int32)
    pos[:, :n], pv[:, :n], pf[:, :n] = parts.pos.T, parts.channels[0].data.T, parts.channels[2].data.T
    flag[:n], pl[:n], px[:n] = parts.flag, parts.channels[1].data, parts.channels[3].data
    return [pos, flag, pv, pl, pf, px]


def sys_result(arrs, n):
    pos, flag, pv, pl, pf, px = arrs
    return {"pos": np.ascontiguousarray(pos[:, :n].T), "flag": flag[:n].copy(), "ch0": np.ascontiguousarray(pv[:, :n].T), "ch1": pl[:n].copy(),
            "ch2": np.ascontiguousarray(pf[:, :n].T), "ch3": px[:n].copy()}


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p
    i64 = ctypes.c_int64

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    # ---- potentials
    seen = dict(nan=0, zero_v=0, unit_n=0, inside=0, lo=0, hi=0)
    for name in M.POT_CASES:
        I = M.pot_inputs(name)
        sx, sy, sz = I["dims"]
        sh = (sz, sy, sx)
        normal = soa(I["normal"])
        res = [np.full(sh, 123.0, f32) for _ in range(4)]
        taus = np.array(I["taus"], f32)
        call("rec_potentials", sx, sy, sz, P(I["flags"]), P(soa(I["vel"])), P(normal), P(I["phi"]), I["radius"], P(taus), fc(I["scale"]),
             I["itype"], I["jtype"], *[P(r) for r in res])
        for k, r in zip(("potTA", "potWC", "potKE", "ratio"), res):
            out["%s/%s" % (name, k)] = r
        out[name + "/normal"] = aos(normal, sh)
        raw = {}
        M.potentials(I["flags"], I["vel"], I["normal"], I["phi"], I["radius"], *I["taus"], I["scale"], I["itype"], I["jtype"], raw=raw)
        seen["nan"] += int(np.isnan(res[3]).sum())
        if raw:
            m = raw["cells"]
            seen["zero_v"] += int((m & (M._l2(raw["vi"]) == 0)).sum())
            seen["unit_n"] += int((m & (M._l2(raw["ni"]) == 1)).sum())
        for r in res[:3]:
            seen["inside"] += int(((r > 0) & (r < 1)).sum())
            seen["lo"] += int((r == 0).sum())
            seen["hi"] += int((r == 1).sum())
        print(name, {k: (float(np.nanmin(r)), float(np.nanmax(r))) for k, r in zip("twkr", res)})
    print("potentials:", seen)
    assert all(v > 0 for v in seen.values()), seen
    out["p3d_r3/interior"] = np.array([int((M.pot_inputs("p3d_r3")["flags"][3:4, 3:5, 3:6] >= 0).sum())])
    assert out["p3d_r3/interior"][0] == 6

    # ---- sampling: per mode one stream, the cases in order
    cursor = {m: 0 for m in M.MODES}
    for mode in M.MODES:
        big = neg = 0
        for name in M.SAMPLE_ORDER:
            I = M.sample_inputs(name)
            sx, sy, sz = I["dims"]
            parts = I["parts"]
            cap = 1 << 16
            arrs = sys_arrays(parts, cap)
            sizes = (i64 * I["calls"])()
            call("rec_sample", mode.encode(), I["calls"], sx, sy, sz, fc(I["solver_dt"]), P(I["flags"]), P(soa(I["vel"])), P(I["potTA"]),
                 P(I["potWC"]), P(I["potKE"]), P(I["ratio"]), fc(I["lMin"]), fc(I["lMax"]), fc(I["c_s"]), fc(I["c_b"]), fc(I["k_ta"]),
                 fc(I["k_wc"]), fc(I["dt"]), M.TypeFluid, i64(parts.size()), i64(cap), sizes, *[P(a) for a in arrs])
            sizes = np.array(list(sizes), np.int64)
            key = "sample/%s/%s/" % (mode, name)
            for k, v in sys_result(arrs, int(sizes[-1])).items():
                out[key + k] = v
            out[key + "sizes"] = sizes
            out[key + "start"] = np.array([cursor[mode]], np.int64)
            # the reals this case drew: from the counts (which the reference's sizes confirm)
            dt = I["dt"] if I["dt"] > 0 else I["solver_dt"]
            E = M.sample_entries(mode, I["flags"], I["potTA"], I["potWC"], I["potKE"], I["k_ta"], I["k_wc"], dt)
            per_call = int(np.maximum(E["n"], 0).sum())
            assert list(np.diff(np.concatenate([[parts.size()], sizes]))) == [per_call] * I["calls"], (name, sizes, per_call)
            used = 4 * per_call + (3 * int((E["n"] != 0).sum()) if mode == "single" else 0)
            cursor[mode] += used * I["calls"]
            big = max(big, int(E["n"].max()))
            neg += int((E["n"] < 0).sum())
            hist = np.bincount(np.clip(E["n"], 0, 3))
            print(key, "sizes", sizes, "reals", used, "max n", int(E["n"].max()), "negative", int((E["n"] < 0).sum()), "n=0,1,2,3+", hist)
            if name == "s3d_none":
                assert per_call == 0
            elif name != "s3d_twice":
                assert hist[0] > 0.8 * hist.sum() and hist[1] > 0
            if name == "s3d":
                fl = out[key + "flag"][parts.size():]
                assert all((fl == t).any() for t in (M.PSPRAY, M.PBUBBLE, M.PFOAM))
                assert (out[key + "ch3"][parts.size():] == 0).all() and np.array_equal(out[key + "ch3"][:parts.size()], parts.channels[3].data)
        assert big > 300 and neg > 0, (mode, big, neg)

    # ---- update / delete
    ct_seen, compressed = set(), set()
    for name, c in M.UPDATE_CASES.items():
        if not c.get("fixture", True):
            continue
        I = M.update_inputs(name)
        sx, sy, sz = I["dims"]
        parts = I["parts"]
        cap = max(parts.size(), 1)
        arrs = sys_arrays(parts, cap)
        n_out = i64(0)
        g = np.array(I["gravity"], f32)
        call("rec_update", I["mode"].encode(), sx, sy, sz, fc(I["solver_dt"]), P(I["flags"]), P(soa(I["vel"])), P(I["ratio"]), I["radius"], P(g),
             fc(I["k_b"]), fc(I["k_d"]), fc(I["c_s"]), fc(I["c_b"]), fc(I["dt"]), int(I["scale"]), I["exclude"], I["at"], I["itype"],
             i64(parts.size()), i64(cap), ctypes.byref(n_out), *[P(a) for a in arrs])
        for k, v in sys_result(arrs, n_out.value).items():
            out["update/%s/%s" % (name, k)] = v
        compressed.add((I["mode"], n_out.value < parts.size()))
        info = {}
        M.run_update_case(name, info)
        ct_seen |= set(int(v) for v in info["tunnel_ct"])
        if I["mode"] == "cubic":
            assert (info["cubic_neighbours"] != 0).all(), name      # the precondition of the cubic mode
        assert not ((I["flags"] & I["itype"]) != 0)[~M._interior(I["dims"])].any()
        print("update", name, parts.size(), "->", n_out.value)
    assert {1, 3} <= ct_seen, ct_seen
    assert compressed == {("linear", True), ("linear", False), ("cubic", True), ("cubic", False)}, compressed
    compressed = set()
    for name in M.DELETE_CASES:
        I = M.update_inputs(name, M.DELETE_CASES)
        sx, sy, sz = I["dims"]
        parts = I["parts"]
        arrs = sys_arrays(parts, parts.size())
        n_out = i64(0)
        call("rec_delete", sx, sy, sz, P(I["flags"]), i64(parts.size()), i64(parts.size()), ctypes.byref(n_out), *[P(a) for a in arrs])
        for k, v in sys_result(arrs, n_out.value).items():
            out["delete/%s/%s" % (name, k)] = v
        compressed.add(n_out.value < parts.size())
        print("delete", name, parts.size(), "->", n_out.value)
    assert compressed == {True, False}

    # ---- setFlagsFromLevelset / setMACFromLevelset
    for name in M.SET_CASES:
        I = M.set_inputs(name)
        sx, sy, sz = I["dims"]
        flags = I["flags"].copy()
        call("rec_set_flags", sx, sy, sz, P(flags), P(I["phi"]), I["exclude"], I["itype"])
        vel = soa(I["vel"])
        call("rec_set_mac", sx, sy, sz, P(vel), P(I["phi"]), P(np.array(I["c"], f32)))
        out["set/%s/flags" % name] = flags
        out["set/%s/vel" % name] = aos(vel, (sz, sy, sx))
        assert (flags != I["flags"]).any() and (out["set/%s/vel" % name] != I["vel"]).any()

    # ---- the loop (sampling mode "single": it continues that stream)
    C = M.LOOP
    res, steps = C["res"], C["steps"]
    par = np.array(list(C["taus"]) + [C["scale"], C["lMin"], C["lMax"], C["c_s"], C["c_b"], C["k_ta"], C["k_wc"], C["k_b"], C["k_d"],
                                      C["gravity"][1]], f32)
    counts = np.zeros((steps, 6), np.int64)
    pots = np.zeros((4, res, res, res), f32)
    call("rec_loop", res, steps, fc(C["dt"]), P(par), P(counts), P(pots))
    print("loop counts (live, spawned, slots, spray, bubble, foam):\n", counts)
    spawned = int(counts[:, 1].sum())
    assert 10 ** 3 <= spawned <= 10 ** 5, spawned
    assert (counts[:, 3:].max(axis=0) > 0).all(), "not every type occurs"
    out["loop/counts"], out["loop/pots"], out["loop/start"] = counts, pots, np.array([cursor["single"]], np.int64)

    path = os.path.join(ROOT, "tests", "golden", "secparts.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])

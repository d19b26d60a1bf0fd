"""CPU: the public face of level-set reinitialisation without a GPU -- the method's signature and lastReinitStats, the row of the open
extension table with its header, entry names disjoint from every other extension, the product library's exports with its host entry
(the literal serial march) held against the recorded reference, and both refusals, by name, with the grids left as they were."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

import reinit_model as M
import util


def test_names_and_signatures():
    import manta as m
    assert str(inspect.signature(m.LevelsetGrid.reinitMarching)) == (
        "(self, flags, maxTime=4.0, velTransport=None, ignoreWalls=False, correctOuterLayer=True, obstacleType=2)")
    assert m.FlagObstacle == 2
    assert set(m.lastReinitStats()) == {"windows", "subrounds", "pops", "serial"}
    assert all(len(v) == 2 for v in m.lastReinitStats().values())
    assert not hasattr(m, "reinitMarching")               # a method only


def test_row_of_the_open_table_and_header():
    from mantaflow_amd import _lib
    e = _lib.extension("reinit")
    assert e in _lib.OPEN_EXTENSIONS and (e.what, e.verb) == ("level-set reinitialisation by fast marching", "does")
    inc = os.path.dirname(_lib.HEADER)
    assert e.header == os.path.join(inc, "open", "manta_hip_reinit.h") == _lib.REINIT_HEADER and os.path.exists(e.header)
    assert {x.header for x in _lib.OPEN_EXTENSIONS} == set(glob.glob(os.path.join(inc, "open", "manta_hip_*.h")))
    assert (e.version_fn, e.version_macro) == ("mf_reinit_abi_version", "MF_REINIT_ABI_VERSION")
    assert re.search(r"^#define\s+MF_REINIT_ABI_VERSION\s+\d+\s*$", open(e.header).read(), flags=re.M)
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []
    assert "reinit.hip" in open(os.path.join(os.path.dirname(_lib.DEFAULT_LIB), "Makefile")).read()


def test_entry_names_are_disjoint_from_every_other_header():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.all_extensions():
        if e.name != "reinit":
            for n in _lib.parse_header(e.header):
                seen[n] = os.path.basename(e.header)
    mine = _lib.parse_header(_lib.REINIT_HEADER)
    assert set(mine) == {"mf_reinit_abi_version", "mf_reinit_march", "mf_reinit_set_uninitialized", "mf_reinit_march_serial"}
    for n in mine:
        assert n not in seen, "%s is declared by %s as well" % (n, seen.get(n))


def _serial_entry(L, c, direction, phi, fm, vel):
    """one march through mf_reinit_march_serial on host arrays that the Init pass has been applied to"""
    key = np.zeros(c["n"], np.float32)
    pops = ctypes.c_int64(0)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = L.mf_reinit_march_serial(*c["dims"], P(phi), P(fm), P(key), P(c["flags"]), P(vel), ctypes.c_float(c["maxTime"]), direction,
                                  int(c["ignoreWalls"]), int(c["correctOuterLayer"]), c["obstacleType"], ctypes.byref(pops))
    assert rc == 0
    return key, pops.value


@pytest.mark.skipif(not os.path.exists(util.HIP_LIB), reason="libmanta_hip.so not built")
def test_product_library_exports_the_extension_and_its_serial_march_is_the_reference():
    from mantaflow_amd import _lib
    L = ctypes.CDLL(util.HIP_LIB)          # loads without a GPU; only host entries are called
    protos = _lib.parse_header(_lib.REINIT_HEADER)
    for n in protos:
        assert hasattr(L, n), n
    want = int(re.search(r"#define\s+MF_REINIT_ABI_VERSION\s+(\d+)", open(_lib.REINIT_HEADER).read()).group(1))
    assert L.mf_reinit_abi_version() == want
    L.mf_reinit_march_serial.argtypes = protos["mf_reinit_march_serial"][1]
    G = np.load(M.GOLDEN)
    names = [n for n in M.CASES if M.CASES[n]["dims"] != (33, 31, 29)]
    for name in names:
        c = M.case(name)
        n = c["n"]
        phi = [float(x) for x in c["phi"]]
        fl = [int(x) for x in c["flags"]]
        vel = None if c["velocity"] is None else c["velocity"].copy()
        fm, key = [0] * n, [0.] * n
        pops = []
        for d in (-1, 1):
            # the element-wise passes are the model's; the march is the library's
            mm = M.March(c["dims"], phi, fm, key, fl, None, c["maxTime"], d, c["ignoreWalls"], c["obstacleType"], M.new_counters())
            mm.init_fm()
            a, f = np.array(phi, np.float32), np.array(fm, np.int32)
            k, p = _serial_entry(L, c, d, a, f, vel)
            pops.append(p)
            phi[:], fm[:] = [float(x) for x in a], [int(x) for x in f]
            mm.set_uninitialized(M.F(-M.F(c["maxTime"]) - 1.) if d < 0 else M.F(M.F(c["maxTime"]) + 1.))
        got = np.array(phi, np.float32)
        assert np.array_equal(got.view(np.uint32), G[name + "/phi"].view(np.uint32)), name
        if vel is not None:
            assert np.array_equal(vel.view(np.uint32), G[name + "/vel"].view(np.uint32)), name
        assert np.array_equal(np.array(fm, np.int8), G[name + "/fm"]) and np.array_equal(k.view(np.uint32), G[name + "/key"].view(np.uint32)), name
        assert tuple(pops) == tuple(G[name + "/stats"][2]), name           # the serial loop pops what the rounds pop
    bad = ctypes.c_int64(0)
    a = np.zeros(8, np.float32)
    assert L.mf_reinit_march_serial(2, 2, 2, a.ctypes.data_as(ctypes.c_void_p), None, None, None, None, ctypes.c_float(4.), 1, 0, 1, 2,
                                    ctypes.byref(bad)) != 0


def _scene(m, dims=(10, 9, 8)):
    s = m.Solver(name="o", gridSize=m.vec3(*dims), dim=3)
    g = {"phi": s.create(m.LevelsetGrid), "flags": s.create(m.FlagGrid), "vel": s.create(m.MACGrid)}
    g["flags"].initDomain()
    g["flags"].fillGrid()
    g["phi"].setConst(-3.0)
    g["vel"].setConst(m.vec3(1, 2, 3))
    return s, g


def _state(g):
    return [x.data.cpu().numpy().tobytes() for x in g.values()]


def test_refusals_leave_the_grids_as_they_were(oracle_backend):
    import manta as m
    from mantaflow_amd import _lib
    assert _lib.get().reinit is False
    s, g = _scene(m)
    before = _state(g)
    stats = m.lastReinitStats()
    with pytest.raises(RuntimeError) as e:
        g["phi"].reinitMarching(flags=g["flags"], velTransport=g["vel"])
    assert str(e.value) == ("LevelsetGrid::reinitMarching: the 'oracle' backend does not implement level-set reinitialisation by fast "
                            "marching (manta_hip_reinit.h)")
    with pytest.raises(RuntimeError, match="^LevelsetGrid::reinitMarching: the 'oracle' backend does not implement "):
        g["phi"].reinitMarching(flags=None)                                 # before any argument check
    s._slab_window = (2, 8)
    try:
        with pytest.raises(RuntimeError) as e:
            g["phi"].reinitMarching(flags=g["flags"], velTransport=g["vel"])
        assert str(e.value) == "LevelsetGrid::reinitMarching: level-set reinitialisation by fast marching does not run on a z-slab solver"
    finally:
        s._slab_window = (0, 0)
    assert _state(g) == before and m.lastReinitStats() == stats
    # the names that other test files pin stay as they are
    for name in ("obstacleLevelset", "obstacleGradient", "reinitMarching", "particleSurfaceTurbulence"):
        assert not hasattr(m, name), name


def test_fixture_is_small_and_covers_the_cases():
    G = np.load(M.GOLDEN)
    assert os.path.getsize(M.GOLDEN) < 1 << 19
    for name in M.CASES:
        assert name + "/stats" in G.files and (name + "/phi" in G.files or name + "/phi_sha" in G.files), name
    assert {c["dims"] for c in M.CASES.values()} == set(M.SIZES)
    assert {c["maxTime"] for c in M.CASES.values()} == {2.0, 4.0, 6.0}

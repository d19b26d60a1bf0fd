"""GPU: LevelsetGrid.reinitMarching through the package on the HIP backend against the model (tests/reinit_model.py) on the inputs of
tests/reinit_cases.py, which tests/test_reinit_cases.py checks on the CPU: 240 random cases and the designed families (whole planes of
equal keys, keys on a window's end, signed zeros at the interface, a far field of +-1000, maxTime below a cell and beyond the grid, lists
of more than four blocks of entries) in their variants.  Every comparison is bit for bit, per case:

  * phi, vel and the outward march's FastMarch flags and keys (read through LevelsetGrid._reinit_keep) are the model's serial statement;
  * lastReinitStats() -- windows, sub-rounds, pops, serial, per direction -- is the model's statement in rounds.  A flagged march is redone
    serially and cannot differ, so the equal counters per case are what keeps a case from passing by falling back: the device flags
    exactly where the model does (29 of the 240 random cases), and pops in the same sub-rounds elsewhere.

Pool scratch and the counters are poisoned before each call.  A designed case runs three times on one solver (the order of the device
list differs from run to run; the bits must not), and once more under MF_REINIT_SERIAL=1."""
import pytest

import reinit_cases as C
from test_gpu_reinit import _call, _load, _poison

pytestmark = pytest.mark.gpu
CHUNK = 60
STATS = ("windows", "subrounds", "pops", "serial")


def _grids(m, dims, cache=None):
    if cache is not None and dims in cache:
        return cache[dims]
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=2 if dims[2] == 1 else 3)
    g = {"solver": s, "phi": s.create(m.LevelsetGrid), "flags": s.create(m.FlagGrid), "vel": s.create(m.MACGrid)}
    if cache is not None:
        cache[dims] = g
    return g


def _differences(m, g, name, serial_only=False, poison=True):
    """one device call on the case: the list of what differs from the model, each entry naming the array and the first cell, and whether
    the device redid a march serially"""
    c, want, stats = C.get(name), C.run(name, "serial"), C.run(name, "rounds")["stats"]
    if serial_only:
        stats = {"windows": (0, 0), "subrounds": (0, 0), "pops": stats["pops"], "serial": (1, 1)}
    _load(g["flags"].data, c["flags"])
    if poison:
        _poison(g["solver"], c["velocity"] is not None)
    phi, vel, fm, key, st = _call(m, g, c, c["phi"], c["velocity"])
    out = []
    for k, got in (("phi", phi), ("vel", vel), ("fm", fm), ("key", key)):
        d = None if want[k] is None else C.first_difference(want[k], got)
        if d is not None:
            i = d[0] % c["n"]
            out.append("%s %s: first at cell %d = (%d, %d, %d)%s, model %r, device %r" % (
                c["name"], k, d[0], i % c["dims"][0], i // c["dims"][0] % c["dims"][1], i // (c["dims"][0] * c["dims"][1]),
                " component %d" % (d[0] // c["n"]) if k == "vel" else "", d[1], d[2]))
    if {k: tuple(st[k]) for k in STATS} != {k: tuple(stats[k]) for k in STATS}:
        out.append("%s stats: device %s, model %s" % (c["name"], {k: tuple(st[k]) for k in STATS}, {k: tuple(stats[k]) for k in STATS}))
    return out, max(st["serial"])


@pytest.mark.parametrize("chunk", range(len(C.SWEEP) // CHUNK))
def test_sweep_chunk(hip_backend, monkeypatch, chunk):
    import manta as m
    monkeypatch.delenv("MF_REINIT_SERIAL", raising=False)
    solvers, bad, flagged = {}, [], 0
    for q in C.SWEEP[chunk * CHUNK:(chunk + 1) * CHUNK]:
        diff, serial = _differences(m, _grids(m, C.get(q)["dims"], solvers), q)
        bad += diff
        flagged += serial
    want = sum(max(C.verdict(q)) for q in C.SWEEP[chunk * CHUNK:(chunk + 1) * CHUNK])
    print("chunk %d: the device flagged %d of %d cases, the model %d; %d solvers; %d differences" % (chunk, flagged, CHUNK, want, len(solvers), len(bad)))
    assert not bad, "\n".join(bad)
    assert flagged == want


@pytest.mark.parametrize("name", list(C.DESIGNED))
def test_designed(hip_backend, monkeypatch, name):
    import manta as m
    monkeypatch.delenv("MF_REINIT_SERIAL", raising=False)
    ok, what = C.reaches(name)
    assert ok, (name, what)
    g = _grids(m, C.designed(name)["dims"])
    for run in range(3):
        bad, _ = _differences(m, g, name)
        assert not bad, "run %d\n%s" % (run, "\n".join(bad))
    monkeypatch.setenv("MF_REINIT_SERIAL", "1")
    bad, _ = _differences(m, g, name, serial_only=True)
    assert not bad, "under MF_REINIT_SERIAL=1\n" + "\n".join(bad)
    print(name, what, C.run(name, "rounds")["stats"])


def test_small_after_large(hip_backend, monkeypatch):
    """a short march after the longest list: on a small solver that shares only the library with the large one, and on the large solver
    itself, whose scratch grids and counters still hold what the large call left (no poison in between)"""
    import manta as m
    monkeypatch.delenv("MF_REINIT_SERIAL", raising=False)
    large, small, short = "box-20x18x16-default", "eighths_t4-9x8x7-default", "eighths_t05-20x18x16-default"
    assert C.longest_list(large) > 4 * C.BLOCK and C.longest_list(short) < C.longest_list(large) // 3 and C.longest_list(small) < C.BLOCK
    big, little = _grids(m, C.BIG), _grids(m, C.D3)
    bad = _differences(m, big, large)[0]
    bad += _differences(m, little, small)[0]
    bad += _differences(m, big, short, poison=False)[0]
    bad += _differences(m, big, large, poison=False)[0]
    bad += _differences(m, little, small, poison=False)[0]
    assert not bad, "\n".join(bad)

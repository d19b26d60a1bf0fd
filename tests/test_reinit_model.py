"""CPU: the model of LevelsetGrid.reinitMarching (tests/reinit_model.py) against the recorded reference (tests/golden/reinit.npz; how it
was produced: tools/record_reinit.py) and against itself.  Every comparison is bit for bit.

  * the literal serial statement and the statement in rounds give the reference's phi and vel in every fixture case, the same FastMarch
    flags and keys as each other, and the recorded counters;
  * the order-free seeding equals the serial seeding loop on 1000 random small grids, both directions, both outward variants;
  * the statement in rounds equals the serial one on 2000 random cases of up to 10x9x8, smooth to sigma 1.0, both outward seedings, with
    and without transport and walls -- and no more than half of them may have flagged (a flagged march is redone serially, so it cannot
    differ; the bound keeps the test from passing that way);
  * the sigma 1.0 fixture cases flag, the smooth ones do not;
  * every branch was entered: each invcnt case, + over -, the maxTime cut, an equal time overwriting, a worse time kept, transport.
"""
import numpy as np
import pytest

import reinit_model as M

G = np.load(M.GOLDEN)
BIG = (33, 31, 29)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_as_fixture(name, key, a):
    if name + "/" + key in G.files:
        return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(G[name + "/" + key]).view(np.uint8))
    return M.sha(a) == str(G[name + "/" + key + "_sha"])


@pytest.mark.parametrize("name", list(M.CASES))
def test_model_equals_the_reference(name):
    modes = ("rounds",) if M.CASES[name]["dims"] == BIG and not name.startswith("off") else ("serial", "rounds")
    for mode in modes:
        R = M.model(name, mode)
        assert _same_as_fixture(name, "phi", R["phi"]), (name, mode)
        if R["vel"] is not None:
            assert _same_as_fixture(name, "vel", R["vel"]), (name, mode)
        assert _same_as_fixture(name, "fm", R["fm"].astype(np.int8)) and _same_as_fixture(name, "key", R["key"]), (name, mode)
    R = M.model(name, "rounds")
    assert np.array_equal(np.array([R["stats"][k] for k in ("windows", "subrounds", "pops", "serial")]), G[name + "/stats"]), name
    if "serial" in modes:
        assert M.model(name, "serial")["stats"]["pops"] == R["stats"]["pops"]


def test_sigma_one_cases_flag_and_smooth_cases_do_not():
    for name, c in M.CASES.items():
        serial = tuple(G[name + "/stats"][3])
        if c["kind"] == "noise10":
            assert max(serial) == 1, name
        if c["kind"] in M.SMOOTH and c["correctOuterLayer"] and not c["ignoreWalls"]:
            assert serial == (0, 0), name
    big = G["centred_33x31x29/stats"]
    assert big[0].min() > 10 and (big[1] > big[0]).all() and big[2].min() > 1000       # windows, sub-rounds, pops: it ran in rounds


def test_every_branch_was_entered():
    total = M.new_counters()
    for name in M.CASES:
        if M.CASES[name]["dims"] != BIG:
            for k, v in M.model(name, "serial")["counters"].items():
                total[k] += int(v)
    for k in ("invcnt0", "invcnt1", "invcnt2", "plus", "minus", "plus_over_minus", "maxtime_cut", "equal_overwrite", "worse_kept", "transport"):
        assert total[k] > 0, (k, total)
    assert M.model("noise10_12x9x1", "serial")["counters"]["clamped_sqrt"] + M.model("noise10_7x5x4", "serial")["counters"]["clamped_sqrt"] > 0


def test_order_free_seeding_equals_the_serial_loop_on_random_grids():
    pushed = 0
    for q in range(1000):
        c = M.random_case(q)
        for d in (-1, 1):
            a = M.seeded(c["dims"], c["phi"], c["flags"], c["velocity"], c["maxTime"], c["ignoreWalls"], c["correctOuterLayer"], c["obstacleType"], d, False)
            b = M.seeded(c["dims"], c["phi"], c["flags"], c["velocity"], c["maxTime"], c["ignoreWalls"], c["correctOuterLayer"], c["obstacleType"], d, True)
            for x, y in zip(a[:4], b[:4]):
                assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), (q, d)
            assert a[4] == b[4], (q, d)
            pushed += len(a[4])
    assert pushed > 10000                   # five cells and more go on the heap per march on average


def test_rounds_equal_the_serial_loop_on_random_cases():
    flagged = marches = 0
    by_sigma = {}
    for q in range(2000):
        c = M.random_case(q)
        args = (c["dims"], c["phi"], c["flags"], c["velocity"], c["maxTime"], c["ignoreWalls"], c["correctOuterLayer"], c["obstacleType"])
        S, R = M.call(*args, mode="serial"), M.call(*args, mode="rounds")
        for k in ("phi", "vel", "fm", "key"):
            assert (S[k] is None and R[k] is None) or np.array_equal(_bits(S[k]), _bits(R[k])), (q, k)
        assert S["stats"]["pops"] == R["stats"]["pops"], q
        f = max(R["stats"]["serial"])
        flagged += f
        marches += sum(1 for w in R["stats"]["windows"] if w > 0)
        n = by_sigma.setdefault(c["sigma"], [0, 0])
        n[0] += 1
        n[1] += f
    print("flagged %d of 2000 cases; per sigma (cases, flagged): %s; marches in rounds with a window: %d" % (flagged, sorted(by_sigma.items()), marches))
    assert flagged <= 1000 and marches >= 1000
    assert by_sigma[0.][1] * 4 <= by_sigma[0.][0] and by_sigma[1.0][1] > 0

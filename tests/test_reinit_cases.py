"""CPU: the inputs of the reinitMarching sweep (tests/reinit_cases.py) on the model alone.  For every input -- 240 random cases and the
designed families in their variants -- the model's statement in rounds equals its serial statement bit for bit in phi, vel, the outward
march's FastMarch flags and keys, with equal pops; the reach predicate of every designed case holds; and the caps that keep the device
test (tests/test_gpu_reinit_sweep.py) from passing by falling back hold:

  * at most a quarter of the random cases flag (29 of 240), and each of the four (inward, outward) verdicts occurs with and without
    velocity transport;
  * every designed case in its default variant runs in rounds, both marches;
  * of the `inner` (correctOuterLayer=False) and `walls` (ignoreWalls with an obstacle box) variants at least half run in rounds.  What
    flags there is recorded below: the outward march of `zeros` without correctOuterLayer, and with the obstacle box every family but
    `eighths` at maxTime 0.5 -- the march enters the obstacle cells the seeding skipped with a key that precedes its pusher's, which the
    flag rule is there to catch ("conservative in one direction").
"""
import numpy as np
import pytest

import reinit_cases as C
import reinit_model as M

ARRAYS = ("phi", "vel", "fm", "key")
# the designed cases that the model redoes serially, (inward, outward); every other one runs in rounds
FLAGGED = {"zeros-9x8x7-inner": (0, 1), "zeros-12x9x1-inner": (0, 1), "box-12x9x1-walls": (1, 0)}
FLAGGED.update({"%s-%s-walls" % (f, d): (1, 1) for d in ("9x8x7", "12x9x1") for f in C.EVERYWHERE if f not in ("eighths_t05", "box")})
FLAGGED["box-9x8x7-walls"] = (1, 1)


def _rounds_equal_serial(name):
    S, R = C.run(name, "serial"), C.run(name, "rounds")
    for k in ARRAYS:
        assert (S[k] is None and R[k] is None) or C.first_difference(S[k], R[k]) is None, (name, k, C.first_difference(S[k], R[k]))
    assert S["stats"]["pops"] == R["stats"]["pops"], name
    assert S["stats"]["serial"] == (1, 1) and S["stats"]["windows"] == (0, 0)
    return R["stats"]


def test_run_is_the_models_call():
    """reinit_cases.run only adds the record of the pops"""
    for name in list(C.SWEEP)[::12] + ["zeros-12x9x1-inner", "eighths_t4-9x8x7-walls", "plane_x5-12x9x1-default"]:
        c = C.get(name)
        for mode in ("serial", "rounds"):
            want = M.call(c["dims"], c["phi"], c["flags"], c["velocity"], c["maxTime"], c["ignoreWalls"], c["correctOuterLayer"], c["obstacleType"], mode)
            got = C.run(name, mode)
            for k in ARRAYS:
                assert (want[k] is None and got[k] is None) or C.first_difference(want[k], got[k]) is None, (name, mode, k)
            assert want["stats"] == got["stats"], (name, mode)
            assert [len(p) for p in got["popped"]] == list(got["stats"]["pops"]), (name, mode)


def test_sweep_rounds_equal_serial_and_few_flag():
    verdicts, total = {}, np.zeros(3, np.int64)
    for q in C.SWEEP:
        st = _rounds_equal_serial(q)
        verdicts.setdefault(st["serial"], []).append(C.get(q)["velocity"] is not None)
        total += [sum(st[k]) for k in ("windows", "subrounds", "pops")]
    flagged = sum(len(v) for k, v in verdicts.items() if k != (0, 0))
    print("flagged %d of %d; (inward, outward) -> cases: %s; windows, sub-rounds, pops in rounds or serial: %s"
          % (flagged, len(C.SWEEP), {k: len(v) for k, v in sorted(verdicts.items())}, total.tolist()))
    assert 4 * flagged <= len(C.SWEEP)
    for v in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert True in verdicts.get(v, []) and False in verdicts.get(v, []), (v, verdicts.get(v))
    assert total[0] > 2000 and total[1] > 4000           # the sweep runs in rounds: 2713 windows, 5176 sub-rounds


@pytest.mark.parametrize("name", list(C.DESIGNED))
def test_designed_rounds_equal_serial_and_reach(name):
    st = _rounds_equal_serial(name)
    ok, what = C.reaches(name)
    print(name, st, what)
    assert ok, (name, what)
    assert st["serial"] == FLAGGED.get(name, (0, 0)), (name, st)
    if C.designed(name)["variant"] == "default":
        assert st["serial"] == (0, 0) and min(st["windows"]) > 0, (name, st)


def test_caps_of_the_designed_cases():
    assert not [n for n in FLAGGED if n not in C.DESIGNED or C.DESIGNED[n][2] == "default"]
    variants = [n for n, (_, _, v) in C.DESIGNED.items() if v != "default"]
    in_rounds = [n for n in variants if n not in FLAGGED]
    print("variants in rounds: %d of %d" % (len(in_rounds), len(variants)))
    assert 2 * len(in_rounds) >= len(variants)
    # every family in every variant on a 3-D and a 2-D grid
    assert {(f, d, v) for f in C.EVERYWHERE for d in (C.D3, C.D2) for v in C.VARIANTS} <= set(C.DESIGNED.values())


def test_some_list_exceeds_four_blocks_of_entries():
    for name in ("box-20x18x16-default", "zeros-20x18x16-default", "eighths_t1000-20x18x16-default"):
        assert C.longest_list(name) > 4 * C.BLOCK, (name, C.longest_list(name))
    # and a whole block of entries with one key: a face of the box
    assert C.most_equal_keys("box-20x18x16-default") > C.BLOCK

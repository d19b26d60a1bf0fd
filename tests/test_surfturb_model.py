"""CPU: the numpy model of surface turbulence (tests/surfturb_model.py) against the recorded reference run of
tests/golden/surfturb.npz -- every recorded stage from its recorded inputs and three whole calls from the recorded coarse states:
sizes, delete bookkeeping and flags equal, everything not downstream of expf / logf within the stage bit for bit, the rest within the
bounds derived in DESIGN.md section 27 (the largest observed fraction is printed) -- the quirks the contract keeps, each asserted on
the model and, where the fixture holds them, on the reference's states; and the index work: the serial greedy delete pass against its
order-free statement in rounds on random small cases, the cell list's conversion and order, ParticleSystem::compress."""
import numpy as np
import pytest

import surfturb_model as M

f32, i32 = np.float32, np.int32


def test_greedy_rounds_equal_the_serial_loop_on_random_cases():
    rng = np.random.RandomState(11)
    lo, hi = f32(2), f32(10)
    seen_rounds = set()
    for case in range(1000):
        n = int(rng.randint(0, 13))
        listed = int(rng.randint(0, n + 1))
        pos = rng.uniform(4, 5.2, (n, 3)).astype(f32)
        if n and case % 5 == 0:
            pos[rng.randint(n)] = rng.choice([1.5, 10.5, np.nan, np.inf])          # outside the domain
        if n > 1 and case % 7 == 0:
            pos[rng.randint(n)] = pos[rng.randint(n)]                              # an exact duplicate (or itself)
        flag = np.where(rng.uniform(size=n) < 0.15, M.PDELETE, 0).astype(i32)
        radius = f32(rng.choice([0.3, 0.5, 0.8]))
        want = M.greedy_serial(pos, flag, listed, radius, lo, hi)
        got, rounds = M.greedy_rounds(pos, flag, listed, radius, lo, hi)
        assert np.array_equal(got, want), case
        assert rounds <= max(n, 1)
        seen_rounds.add(rounds)
    assert {1, 2, 3} <= seen_rounds


def test_greedy_rounds_of_a_line_equal_its_length():
    d = f32(0.4)
    for n in (1, 2, 7):
        for order in (1, -1):
            pos = np.stack([f32(4) + d * f32(0.5) * np.arange(n, dtype=f32)[::order], np.full(n, 5, f32), np.full(n, 5, f32)], 1)
            flag = np.zeros(n, i32)
            got, rounds = M.greedy_rounds(pos, flag, n, f32(0.67) * d, f32(2), f32(10))
            assert rounds == n
            assert np.array_equal(got, M.greedy_serial(pos, flag, n, f32(0.67) * d, f32(2), f32(10)))
            assert got.tolist() == [True] * (n - 1) + [False]          # every slot but the last has a higher active neighbour


def test_cell_of_converts_like_x86_and_lists_are_stable():
    pos = np.array([[0, 0, 0], [11.99, 5, 5], [np.nan, 5, 5], [np.inf, 5, 5], [-np.inf, 5, 5], [1e30, 5, 5], [-3, 5, 5], [12, 5, 5], [5, 5, 5], [5, 5, 5]], f32)
    R = 23
    c = M.cell_of(pos, 12, R)
    x = c // (R * R)
    assert x.tolist() == [0, 22, 0, 0, 0, 0, 0, 22, 9, 9]          # NaN, +-inf and 1e30 land in cell 0: INT_MIN after the conversion
    start, ids = M.cell_list(pos, 12, R)
    assert start[0] == 0 and start[-1] == len(pos) and (np.diff(start) >= 0).all()
    for cell in np.unique(c):
        assert ids[start[cell]:start[cell + 1]].tolist() == np.nonzero(c == cell)[0].tolist()


def test_compress_fills_holes_from_the_tail():
    D = M.PDELETE
    assert M.compress(np.array([0, D, 0, 0, D], i32)).tolist() == [0, 3, 2]
    assert M.compress(np.array([D, D, D], i32)).tolist() == []
    assert M.compress(np.array([0, 0], i32)).tolist() == [0, 1]
    assert M.compress(np.array([D, 0, D, 0, 0, D, D], i32)).tolist() == [4, 1, 3]


# what a stage computes downstream of expf / logf (the level and the gradient): only these may differ from the reference, within the bounds
LOOSE = {"adddelete": ("pos",), "normals": ("normals",), "constrain": ("pos",)}


def _against_reference(got, want, loose, what):
    assert [int(x) for x in got["sizes"][:3]] == [int(x) for x in want["sizes"][:3]], what
    assert np.array_equal(got["flag"], want["flag"]), what
    out = []
    for k, bound in (("pos", M.POS_BOUND), ("normals", M.NRM_BOUND), ("real", M.NRM_BOUND)):
        g, w = np.ascontiguousarray(got[k], f32), np.ascontiguousarray(want[k], f32)
        differ = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
        if k not in loose:
            assert not differ.any(), (what, k, int(differ.sum()))
            continue
        worst = float(np.abs(g.astype(np.float64) - w)[differ].max()) if differ.any() else 0.0
        out.append("%s: %d values differ, largest %.3g = %.3g of the bound" % (k, int(differ.sum()), worst, worst / bound))
        assert worst <= bound, (what, k, worst, bound)
    return "; ".join(out) or "equal bit for bit"


@pytest.mark.parametrize("i", range(16))
def test_model_reproduces_every_recorded_stage(i):
    G = M.golden()
    name = M.chain_names(G)[i]
    mdl, got = M.model_stage(G, i)
    print("chain %d %s:" % (i, name), _against_reference(got, M.state(G, "chain/%d" % i), LOOSE.get(name, ()), name))


@pytest.mark.parametrize("i", range(32))
def test_model_reproduces_every_recorded_stage_inside_the_calls(i):
    """the first two and the last maintenance iteration of frame 0 and everything of frames 1 and 2, each stage from the reference's
    state before it"""
    G = M.golden()
    cases = M.stage_cases(G)
    assert len(cases) == 32
    what, name, c, want = cases[i]
    mdl = M.Model(M.par_of(G, 0, c["frame"]), c["R"], c, listed=c.get("listed"))
    print(what, name + ":", _against_reference(mdl.run(name), want, LOOSE.get(name, ()), (what, name)))


def test_reference_states_inside_the_first_frame_show_the_quirks():
    G = M.golden()
    cases = {(w, n): (c, want) for w, n, c, want in M.stage_cases(G)}
    P = M.par_of(G, 0, 0)
    # the surface list is empty during the first add / delete: every point inside the domain buffers a copy of itself, no point is
    # killed by the greedy pass or for want of a coarse neighbour; the level test of pass 3 kills, the system compresses
    c, want = cases[("frame 0 iteration 0", "adddelete")]
    n = len(c["flag"])
    inside = M.in_domain(P, c["pos"])
    assert n > 0 and not c["flag"].any() and c["sizes"][1] == 0
    mdl = M.Model(P, c["R"], c, listed=0)
    mdl.run("adddelete")
    assert mdl.stats["added"] == int(inside.sum()) and mdl.stats["kills"][:2] == (0, 0) and mdl.stats["kills"][2] > 0
    assert len(want["flag"]) == n + mdl.stats["added"] - mdl.stats["kills"][2] and want["sizes"][1] == 0        # compressed: the killed are gone
    live = np.unique(want["pos"], axis=0)
    assert len(want["pos"]) - len(live) > 100                    # the reference's state holds the copies: exact duplicates
    # ... the second iteration's greedy pass kills every such pair's lower slot
    c, want = cases[("frame 0 iteration 1", "adddelete")]

    def duplicates(st):
        p = st["pos"][(st["flag"] & M.PDELETE) == 0]
        return len(p) - len(np.unique(p, axis=0))
    assert duplicates(c) > 100 and duplicates(want) < duplicates(c)
    # new points get zero entries in every channel, PNEW is cleared everywhere, in every recorded add / delete of the reference
    for (w, name), (c, want) in cases.items():
        if name == "adddelete":
            assert not (want["flag"] & M.PNEW).any() and c["sizes"][1] <= c["sizes"][2]
            if want["sizes"][1]:                                  # not compressed: the appended slots are the last ones
                n0 = len(c["flag"])
                assert not want["normals"][n0:].any() and not want["real"][:, n0:].any()


@pytest.mark.parametrize("f", [0, 1, 2])
def test_model_reproduces_the_whole_recorded_calls(f):
    """from the recorded coarse states: the point counts, the delete bookkeeping and the flags equal the reference's"""
    G = M.golden()
    got, its, displaced, _ = M.model_call(G, f)
    want = M.state(G, "call%d/after" % f)
    print("call %d:" % f, _against_reference(got, want, ("pos", "normals", "real"), f), [(i["added"], i["kills"], i["compressed"], i["size"]) for i in its])
    wd = G["call%d/displaced" % f]
    assert displaced.shape == wd.shape and np.abs(displaced.astype(np.float64) - wd).max() <= M.POS_BOUND
    assert len(its) == (12 if f == 0 else 2)


def test_init_fines_and_direction_table_against_the_reference():
    G = M.golden()
    for k in (1, 2):
        P = M.par_of(G, k, 0)
        pos = M.init_fines(P, int(G["set%d/res" % k][0]), G["flags"], G["call0/coarse_pos"], G["call0/coarse_flag"])
        want = G["set%d/init_pos" % k]
        # the table's sin / cos are the library's host code (held to the fixture bit for bit on the GPU and by the host program); the
        # model rounds the fp64 functions once, which may differ from sinf / cosf in the last place of a direction's component
        assert pos.shape == want.shape and np.abs(pos.astype(np.float64) - want).max() <= 2.0 ** -23 * float(P.outer) * 2
        print("set %d: %d of %d values differ from the reference" % (k, int((pos.view(np.uint32) != want.view(np.uint32)).sum()), pos.size))


def test_quirks_of_the_first_frame():
    G = M.golden()
    _, its, _, stages = M.model_call(G, 0)
    P = M.par_of(G, 0, 0)
    first = stages[(0, 0)]
    b, a = first["before"], first["after"]
    n = len(b["flag"])
    # the surface list is empty during the first add / delete: no point has a neighbour, so every point inside the domain buffers a copy
    # of itself (the tangential direction is zero), the greedy pass kills nothing, and only the level test of pass 3 kills
    inside = M.in_domain(P, b["pos"])
    assert first["name"] == "adddelete" and b["listed"] == 0 and n > 0
    assert a["stats"]["added"] == int(inside.sum()) and a["stats"]["kills"][:2] == (0, 0) and a["stats"]["kills"][2] > 0
    # ... the copies are exact duplicates of live points; the second iteration's greedy pass kills every such pair's lower slot (two
    # duplicates buffer the same new point twice, and buffered points do not see each other, so duplicates can remain among the new)
    second = stages[(1, 0)]

    def duplicates(st):
        live = st["pos"][(st["flag"] & M.PDELETE) == 0]
        return len(live) - len(np.unique(live, axis=0))
    assert duplicates(second["before"]) > 100 and duplicates(second["after"]) < duplicates(second["before"])
    assert second["after"]["stats"]["kills"][0] >= duplicates(second["before"])
    # the first doCompress of addDeleteSurfacePoints never compresses: before every add / delete mDeletes <= mDeleteChunk
    for f in range(3):
        for (it, at), rec in M.model_call(G, f)[3].items():
            if rec["name"] == "adddelete":
                assert rec["before"]["sizes"][1] <= rec["before"]["sizes"][2]
                # the second insertBufferedParticles clears PNEW everywhere
                assert not (rec["after"]["flag"] & M.PNEW).any()
    # a compress happens exactly when the kills take mDeletes beyond the chunk
    for f in range(3):
        for (it, at), rec in M.model_call(G, f)[3].items():
            if rec["name"] == "adddelete":
                st = rec["after"]["stats"]
                assert st["compressed"] == (rec["before"]["sizes"][1] + sum(st["kills"]) > rec["before"]["sizes"][2])
    assert any(i["compressed"] for i in its) and not all(i["compressed"] for i in its)


def test_quirks_of_add_and_delete():
    G = M.golden()
    # new points get zero entries in every channel, on the reference's recorded states: before the second add / delete of frame 0 every
    # live point has a normal; after it (it compresses, so the new points sit in holes) as many slots as points survived it have none
    cases = {(w, n): (c, want) for w, n, c, want in M.stage_cases(G)}
    c, want = cases[("frame 0 iteration 1", "adddelete")]
    had = c["normals"].any(axis=1) | ((c["flag"] & M.PDELETE) != 0)
    new = ~want["normals"].any(axis=1)
    assert had.all() and new.sum() > 0 and not want["real"][:, new].any() and not (want["flag"][new] & (M.PNEW | M.PDELETE)).any()
    assert not (want["flag"] & M.PNEW).any()                            # PNEW is cleared everywhere: no new point is ever found
    # every kill call counts, also on a slot that is deleted already: the three passes run over every slot with its stored position
    c = M.edge_case(G, "n63")
    mdl = M.Model(M.par_of(G, 0, 3), c["R"], c)
    dead = np.nonzero(c["flag"] & M.PDELETE)[0]
    assert len(dead) == 4 and mdl.mDeletes == 2
    with np.errstate(all="ignore"):
        kills = mdl.delete()
    assert mdl.mDeletes == 2 + sum(kills)
    # slots 20, 21, 22 are deleted and hold NaN / inf / 1e30: outside the domain (pass 1), no coarse neighbour (pass 2), level not in
    # [-0.2, 1.2] for inf and 1e30 (pass 3; a NaN level compares false) -- at least eight calls on deleted slots alone
    live = (c["flag"] & M.PDELETE) == 0
    c2 = dict(c, pos=c["pos"][live], flag=c["flag"][live], normals=c["normals"][live], real=c["real"][:, live])
    alive = M.Model(M.par_of(G, 0, 3), c["R"], c2)
    with np.errstate(all="ignore"):
        kills_alive = alive.delete()
    assert sum(kills) >= sum(kills_alive) + 8


def test_a_continue_continues_the_ghost_chain():
    """points at the plane x = 2 with normals facing it: every image's flipped normal fails the projected-normal test of
    computeSurfaceDisplacements and is skipped, the neighbour itself, last in the chain, still counts"""
    G = M.golden()
    c = M.edge_case(G, "planes")
    P = M.par_of(G, 0, 3)
    with np.errstate(all="ignore"):
        mdl = M.Model(P, c["R"], c)
        mdl.run("regularize")
        far = M.par_of(G, 0, 3)
        far.bndm, far.bndp = f32(-100), f32(100)
        plain = M.Model(far, c["R"], c)
        plain.run("regularize")
    rows = [0, 1, 2, 4, 5, 6, 8, 9, 10]          # the points at the plane that the case does not move elsewhere (3, 7 and 11)
    # the images count in the densities (they are not skipped there) ...
    assert (mdl.last_density[rows] > plain.last_density[rows]).all()
    # ... and the points still move: the chain went on to the neighbour itself after the skipped images
    assert (np.abs(mdl.pos[rows] - c["pos"][rows]).sum(axis=1) > 0).all()


def test_recorded_reference_run_shows_the_quirks():
    G = M.golden()
    a0, b1 = M.state(G, "call0/after"), M.state(G, "call1/before")
    # the first frame leaves zero wave channels and no PNEW; a call's result is the next call's input
    assert not a0["real"][[0, 1, 3, 4]].any() and not (a0["flag"] & M.PNEW).any()
    assert a0["pos"].tobytes() == b1["pos"].tobytes()
    # previous positions are saved on the coarse particles without PNEW / PDELETE only
    cf, prev, cp = G["call0/coarse_flag"], G["call1/coarse_prev"], G["call0/coarse_pos"]
    keep = (cf & (M.PNEW | M.PDELETE)) == 0
    assert (~keep).sum() >= 10 and prev[keep].tobytes() == cp[keep].tobytes() and not prev[~keep].any()
    # a call that compresses and calls that do not (mDeletes stays counted): the first add / delete of the fixture's first frame, and
    # the calls of the harness loop
    assert G["st0/0/0/sizes"][1] == 0 and all(G["loop/%d/after/sizes" % t][1] > 0 for t in range(3))
    # the displaced points are the live slots
    for f in range(3):
        st = M.state(G, "call%d/after" % f)
        assert len(G["call%d/displaced" % f]) == int(((st["flag"] & M.PDELETE) == 0).sum()) == st["sizes"][3]
    # the list resolutions are int(2.f * res / outerRadius) and int(1.f * res / (2.f * meanFineDistance))
    for k in range(3):
        par, R = G["set%d/par" % k], G["set%d/res" % k]
        assert R.tolist() == [int(f32(2) * f32(12) / par[1]), int(f32(12) / (f32(2) * par[3]))]

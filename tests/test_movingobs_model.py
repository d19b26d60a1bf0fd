"""CPU: the numpy statement of moving obstacles and obstacle coupling (tests/movingobs_model.py) against the reference's recorded outputs
(tests/golden/movingobs.npz), bit for bit, entry by entry, and the conditions the cases are there to reach.

MovingObstacle::moveLinear is recorded only as far as the reference library can run it (see movingobs_model's docstring): the shapes'
new centres and the reset flags where the obstacle has a shape, everything where it has none or alpha is outside [0, 1].  The keys
move/<case>/model_* are the model's own output; they are compared here only to show that the model is stable, not as a reference."""
import numpy as np
import pytest

import movingobs_model as M

GOLDEN = np.load(M.GOLDEN)
f32 = np.float32
GRIDS = sorted(M.DIMS)


def same(tag, got, want):
    assert M.same(got, want), "%s: %d of %d elements differ" % (tag, M.differing(np.asarray(got), np.asarray(want)), np.asarray(want).size)


def test_every_key_of_the_file_is_checked_by_this_module():
    keys = set(GOLDEN.files)
    want = set()
    for g in GRIDS:
        want |= {"wall2/" + g, "reset/" + g, "extrap/%s/o0" % g, "extrap/%s/o1" % g, "extrap/%s/plain" % g, "clear/%s/b0" % g, "clear/%s/b1" % g}
        want |= {"bound/%s/r%d/w%d" % (g, r, w) for r in range(3) for w in M.BOUND_WIDTHS}
        want |= {"surf/%s/%s" % (g, k) for k in M.SURF_KINDS}
        want |= {"cnorm/%s/%s/v%d" % (g, k, q) for k in ("real", "vec", "mac") for q in range(len(M.CNORM_VALS))}
    want |= {"setters/%d/%s" % (q, k) for q in range(len(M.SETTER_CASES)) for k in ("state", "centre")}
    want |= {"ids/ids", "ids/threw", "ids/after", "ids/message"}
    want |= {"proj/%d" % q for q in range(len(M.PROJECT_SEQUENCE))}
    moves = {k for k in keys if k.startswith("move/")}
    assert keys - moves == want
    for case, c in M.move_cases().items():
        mine = {k for k in moves if k.startswith("move/%s/" % case)}
        whole = not c["shapes"] or M.ease(c["t"], c["t0"], c["t1"], c["p0"], c["p1"], M.MOVE_DT, bool(c["smooth"])) is None
        names = {"states", "flags", "vel"} if whole else {"states", "reset_flags", "model_flags", "model_vel"}
        assert mine == {"move/%s/%s" % (case, n) for n in names}, case


@pytest.mark.parametrize("g", GRIDS)
def test_set_wall_bcs2(g):
    f, v, o = M.wall2_inputs(g)
    same(g, M.set_wall_bcs2(f, v, o), GOLDEN["wall2/" + g])
    # each face test true on the lower cell only, on the upper cell only, on neither, and faces at index 0
    fl, ob = (f & M.FLUID) != 0, (f & M.OBSTACLE) != 0
    for ax in ((2, 1, 0) if M.DIMS[g][2] > 1 else (2, 1)):
        cur = tuple(slice(1, None) if a == ax else slice(None) for a in range(3))
        low = tuple(slice(0, -1) if a == ax else slice(None) for a in range(3))
        for a, b in ((fl, ob), (ob, fl)):
            assert (a[low] & b[cur] & ~a[cur] & ~b[low]).any() and (a[cur] & b[low] & ~a[low] & ~b[cur]).any()
        assert (~(fl[cur] | fl[low])).any() and (~(ob[cur] | ob[low])).any()
    if M.DIMS[g][2] == 1:
        assert (GOLDEN["wall2/" + g][..., 2] == 0).all() and (v[..., 2] != 0).all()      # vel.z = 0 in every cell of a 2-D grid


@pytest.mark.parametrize("g", GRIDS)
def test_mac_boundary_bands(g):
    v = M.bound_input(g)
    seen = set()
    for rule in range(3):
        for w in M.BOUND_WIDTHS:
            want = GOLDEN["bound/%s/r%d/w%d" % (g, rule, w)]
            same("rule %d width %d" % (rule, w), M.set_bound_mac(v, M.BOUND_VALUE, w, rule), want)
            seen.add(want.tobytes())
    if g == "b":
        assert len(seen) == 3 * len(M.BOUND_WIDTHS)           # every rule and width is a different band (the small grids saturate)
    assert any(2 * w + 3 > min(d for d in M.DIMS[g] if d > 1) for w in M.BOUND_WIDTHS)      # opposite bands overlap


@pytest.mark.parametrize("g", GRIDS)
def test_mark_surface_and_clear_obstacle(g):
    for kind in M.SURF_KINDS:
        f = M.surf_input(g, kind)
        want = GOLDEN["surf/%s/%s" % (g, kind)]
        same(kind, M.mark_surface(f), want)
        assert ((want ^ f) & ~M.SURFACE == 0).all()          # only the surface bit changes
        assert ((want & M.SURFACE != 0) <= (want & M.FLUID != 0)).all()
    f, want = M.surf_input(g, "rand"), GOLDEN["surf/%s/rand" % g]
    bnd = M.on_boundary(M.DIMS[g])
    fluid, marked = (f & M.FLUID) != 0, (want & M.SURFACE) != 0
    assert marked[bnd & fluid].all() and (bnd & fluid).any()                                   # fluid in a boundary cell: always marked
    assert ((f & M.SURFACE != 0) & ~fluid).any() and not (marked & ~fluid).any()                # stale bits on non-fluid cells are cleared
    assert ((f & M.OBSTACLE != 0) & ~bnd).any()
    f, want = M.surf_input(g, "diag"), GOLDEN["surf/%s/diag" % g]
    sx, sy, sz = M.DIMS[g]
    hole = (sz // 2, sy // 2, sx // 2)
    marked = (want & M.SURFACE) != 0
    diag = (hole[0] - (1 if sz > 1 else 0), hole[1] - 1, hole[2] - 1)
    if not M.on_boundary(M.DIMS[g])[diag]:
        assert marked[diag]                                   # its only non-fluid neighbour is diagonal
    if sx >= 8 and sz != 1:
        assert not marked[hole[0], hole[1], hole[2] + 2]      # one cell further in: fluid all round
    for b in (0, 1):
        f = M.clear_input(g)
        want = GOLDEN["clear/%s/b%d" % (g, b)]
        same("clear %d" % b, M.clear_obstacle(f, bool(b)), want)
        assert ((f & M.OBSTACLE != 0) & ~bnd).any() and ((f & M.OBSTACLE != 0) & bnd).any()
    assert not M.same(GOLDEN["clear/%s/b0" % g], GOLDEN["clear/%s/b1" % g])


@pytest.mark.parametrize("g", GRIDS)
def test_clamp_norm_and_reset_phi(g):
    for kind in ("real", "vec", "mac"):
        a = M.cnorm_input(g, "real" if kind == "real" else "vec")
        n = np.abs(a) if kind == "real" else np.sqrt((a.astype(np.float64) ** 2).sum(-1))
        for q, val in enumerate(M.CNORM_VALS):
            same("%s %g" % (kind, val), M.clamp_norm(a, val), GOLDEN["cnorm/%s/%s/v%d" % (g, kind, q)])
        assert (n == 0).any() and (n == 0.5).any() and (n < 0.5).any() and (n > 1.25).any() and n.max() < 100.0
        same("val above every norm", GOLDEN["cnorm/%s/%s/v3" % (g, kind)], a)
        assert (GOLDEN["cnorm/%s/%s/v0" % (g, kind)] == 0).all()
    f, phi = M.reset_inputs(g)
    same("reset", M.reset_phi_in_obs(f, phi), GOLDEN["reset/" + g])


@pytest.mark.parametrize("g", GRIDS)
def test_extrapolate_with_phi_obs(g):
    for into in (0, 1):
        f, v, phi, planted = M.extrap_inputs(g)
        br = {}
        same("intoObs %d" % into, M.extrapolate_mac_simple(f, v, M.EXTRAP_DISTANCE, phi, bool(into), br), GOLDEN["extrap/%s/o%d" % (g, into)])
        need = {"outside", "deep", "away", "scaled"} | ({"unit", "zero"} if planted else set())
        assert need <= set(br), br
    f, v, phi, _ = M.extrap_inputs(g)
    same("phiObs None", M.extrapolate_mac_simple(f, v, M.EXTRAP_DISTANCE, None, False), GOLDEN["extrap/%s/plain" % g])
    assert not M.same(GOLDEN["extrap/%s/o0" % g], GOLDEN["extrap/%s/o1" % g])
    assert any(M.extrap_inputs(q)[3] for q in GRIDS if M.DIMS[q][2] == 1) and any(M.extrap_inputs(q)[3] for q in GRIDS if M.DIMS[q][2] > 1)


def test_get_normal_clamps_its_centre():
    """knUnprojectNormalComp runs on the interior, where the clamp of getNormal never binds; the function itself is stated with it"""
    phi = M.rand_real("b", "normal")
    sx, sy, sz = M.DIMS["b"]
    same("low corner", M.get_normal(phi, 0, 0, 0), M.get_normal(phi, 1, 1, 1))
    same("high corner", M.get_normal(phi, sx - 1, sy - 1, sz - 1), M.get_normal(phi, sx - 2, sy - 2, sz - 2))
    phi2 = M.rand_real("c", "normal")
    assert M.get_normal(phi2, 3, 3, 0)[2] == 0


def test_shape_setters():
    for q, case in enumerate(M.SETTER_CASES):
        state, centre = M.setters_model(*case)
        same("state %d" % q, state, GOLDEN["setters/%d/state" % q])
        same("centre %d" % q, centre, GOLDEN["setters/%d/centre" % q])


def test_ids():
    assert list(GOLDEN["ids/ids"]) == [1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14, 0, 0]
    assert int(GOLDEN["ids/threw"][0]) == 5 and int(GOLDEN["ids/after"][0]) == 17       # the counter moves before the sixth raises
    assert bytes(GOLDEN["ids/message"]).decode() == "currently only 5 separate moving obstacles supported (are you generating them in a loop?)"


@pytest.mark.parametrize("case", sorted(M.move_cases()))
def test_move_linear(case):
    c = M.move_cases()[case]
    f0, v0 = M.move_inputs(case)
    fl, vel, states = M.move_model(case)
    same("states", states, GOLDEN["move/%s/states" % case])
    mine, other = M.move_id(c["which"]), M.move_id((c["which"] + 1) % 5)
    eased = M.ease(c["t"], c["t0"], c["t1"], c["p0"], c["p1"], M.MOVE_DT, bool(c["smooth"]))
    if "move/%s/flags" % case in GOLDEN.files:           # recorded whole
        same("flags", fl, GOLDEN["move/%s/flags" % case])
        same("vel", vel, GOLDEN["move/%s/vel" % case])
        if eased is None:
            same("nothing happens", fl, f0)
            same("nothing happens", vel, v0)
    else:                                                 # recorded up to the reference's "Not yet supported..."
        reset = GOLDEN["move/%s/reset_flags" % case]
        same("reset flags", M.move_reset(f0, mine, c["emptyType"]), reset)
        assert ((f0 & mine) != 0).any() and (reset & mine == 0).all() and (reset[(f0 & mine) != 0] == c["emptyType"]).all()
        same("the other obstacle's cells survive", reset & other, f0 & other)
        # model only from here
        same("model flags", fl, GOLDEN["move/%s/model_flags" % case])
        same("model vel", vel, GOLDEN["move/%s/model_vel" % case])
        assert (fl == (M.OBSTACLE | mine)).any() and not M.same(vel, v0)


def test_move_cases_cover_their_conditions():
    C = M.move_cases()
    alphas = {}
    for case, c in C.items():
        e = M.ease(c["t"], c["t0"], c["t1"], c["p0"], c["p1"], M.MOVE_DT, False)
        alphas[case] = None if e is None else float(e[0])
    assert alphas["b/below/s0"] is None and alphas["b/above/s1"] is None and alphas["b/at0/s0"] == 0.0 and alphas["b/at1/s1"] == 1.0
    assert 0 < alphas["b/inside/s0"] < 1
    assert {c["smooth"] for c in C.values()} == {0, 1} and {c["emptyType"] for c in C.values()} == {M.EMPTY, M.MOVE_EMPTY}
    assert any(len(c["shapes"]) == 2 for c in C.values()) and {k for c in C.values() for k, _ in c["shapes"]} == {0, 1, 2}
    # the two shapes of the b cases overlap at the eased position
    c = C["b/inside/s1"]
    shapes = [M.ShapeModel(k, a) for k, a in c["shapes"]]
    for sh in shapes:
        sh.setCenter(M.ease(c["t"], c["t0"], c["t1"], c["p0"], c["p1"], M.MOVE_DT, True)[2])
    K, J, I = M.ijk(M.DIMS["b"])
    x, y, z = (a.astype(f32) + f32(0.5) for a in (I, J, K))
    assert (shapes[0].inside(x, y, z) & shapes[1].inside(x, y, z)).any()
    # 2-D: vel.z is written wherever the cell carries the ID
    fl, vel, _ = M.move_model("c/inside")
    f0, v0 = M.move_inputs("c/inside")
    has = ((fl & M.move_id(3)) != 0) & M.interior(M.DIMS["c"])
    assert has.any() and (vel[..., 2][has] == vel[..., 2][has][0]).all() and M.same(vel[..., 2][~has], v0[..., 2][~has])


def test_projections_in_sequence():
    stream = M.Stream()
    drawn = []
    for q, (what, g, n) in enumerate(M.PROJECT_SEQUENCE):
        same("step %d" % q, M.project_step(q, stream), GOLDEN["proj/%d" % q])
        drawn.append(stream.drawn)
        pos, flag = M.particles(g, n, what)
        if n >= 65:
            inside = np.array([M.pos_in_grid(M.DIMS[g], p) for p in pos])
            dead = (flag & M.PDELETE) != 0
            assert dead.any() and (inside & ~dead).any() and (~inside & ~dead).any()
            same("deleted particles stay", GOLDEN["proj/%d" % q][dead], pos[dead])
            assert drawn[-1] - drawn[-2] == 4 * int((inside & ~dead).sum()) + 3 * int((~inside & ~dead).sum())
    assert drawn[0] == 0 and [n for _, _, n in M.PROJECT_SEQUENCE[:4]] == [0, 1, 65, 300]
    assert M.PROJECT_SEQUENCE[3] == M.PROJECT_SEQUENCE[4] and not M.same(GOLDEN["proj/3"], GOLDEN["proj/4"])     # the stream continues
    same("a fresh stream repeats the first steps", M.project_step(1, M.Stream()), GOLDEN["proj/1"])


def test_loop_model_runs_and_moves_the_box():
    r = M.loop_model()
    f0, v0, phi0, pos0, _ = M.loop_inputs()
    mid = M.move_id(M.LOOP["which"])
    assert ((r["flags"] & mid) != 0).any() and ((r["flags"] & M.SURFACE) != 0).any()
    assert not M.same(r["vel"], v0) and not M.same(r["pos"], pos0) and np.isfinite(r["vel"]).all() and np.isfinite(r["pos"]).all()
    n = np.sqrt((r["vel"].astype(np.float64) ** 2).sum(-1))
    assert n.max() <= 1.5 * (1 + 1e-6)

"""GPU: surface turbulence (mantaflow_amd/surfturb.py on include/open/manta_hip_surfturb.h) against the numpy model of
tests/surfturb_model.py and the recorded reference run of tests/golden/surfturb.npz.  The rule against the model
(surfturb_model.compare_model): sizes, delete bookkeeping and flags equal, every value equal bit for bit except at no more than one
point per case, which stays within the derived bounds; the count is printed and asserted.  Held to it: every stage of the recorded
chain, three whole calls with their statistics per iteration, every recorded stage inside the calls (the first two and the last maintenance
iteration of the first frame -- the empty surface list, the copies killed in the second iteration -- and all of frames 1 and 2), every
stage on every edge case
(surfturb_model.EDGE_CASES: 0, 1, 63, 64, 65, 257 points, one cell, the six ghost planes and two corners, points outside the domain,
deleted slots holding inf / NaN, duplicates, a compressing and a non-compressing add / delete), and the calls of the harness script's
loop, whose sizes, delete bookkeeping and flags are also held to the reference's recorded run on the same coarse particles.
Against the reference: the library's parameters and direction table bit for bit, sizes and flags exactly, everything that is not
downstream of expf / logf within the stage bit for bit, the rest within the bounds.  The index work (cell list, greedy rounds) is also
tested through its entries.  Scratch and outputs are pre-filled with NaN."""
import ctypes

import numpy as np
import pytest

import surfturb_model as M

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
NAN_BITS = 0x7FC00000


def _scene(m, c, prefill=True):
    """solver, systems and channels holding the state of case c (surfturb_model.call_case / chain_case)"""
    import torch
    from mantaflow_amd import surfturb
    surfturb.resetSurfaceTurbulenceState()
    s = m.Solver(name="g", gridSize=m.vec3(M.RES, M.RES, M.RES), dim=3)
    if prefill:         # what the pool hands out as scratch holds NaN
        for kind in ("int", "vec", "real"):
            t = s._alloc(kind, zero=False)
            t.view(torch.int32).fill_(NAN_BITS)
            s._release(kind, t)
    flags = s.create(m.FlagGrid).from_numpy(c["flags"])
    pp, sp, spd = (s.create(m.BasicParticleSystem) for _ in range(3))
    prev = pp.create(m.PdataVec3)
    nrm = sp.create(m.PdataVec3)
    H, DtH, src, amp, seed = (sp.create(m.PdataReal) for _ in range(5))
    pp.set_positions(c["cpos"], c["cflag"])
    prev.from_numpy(c["prev"])
    sp.set_positions(c["pos"], c["flag"])
    sp.mDeletes, sp.mDeleteChunk = int(c["sizes"][1]), int(c["sizes"][2])
    nrm.from_numpy(c["normals"])
    for pd, row in zip((H, DtH, src, seed, amp), c["real"]):
        pd.from_numpy(row)
    spd.set_positions(np.full((3, 3), np.nan, f32))
    chan = dict(normals=nrm, H=H, DtH=DtH, source=src, seed=seed, seedAmp=amp)
    return s, dict(flags=flags, coarse=pp, prev=prev, surf=sp, displaced=spd, chan=chan)


def _state(S):
    sp, ch = S["surf"], S["chan"]
    real = np.stack([ch[k].to_numpy() for k in ("H", "DtH", "source", "seed", "seedAmp")]) if sp.np else np.zeros((5, 0), f32)
    return dict(pos=sp.get_positions(), flag=sp.get_flags(), normals=ch["normals"].to_numpy().reshape(-1, 3), real=real,
                sizes=[sp.np, sp.mDeletes, sp.mDeleteChunk])


def _plugin_args(S, a):
    ch = S["chan"]
    return dict(flags=S["flags"], coarseParts=S["coarse"], coarsePartsPrevPos=S["prev"], surfPoints=S["surf"], surfaceNormals=ch["normals"],
                surfaceWaveH=ch["H"], surfaceWaveDtH=ch["DtH"], surfacePointsDisplaced=S["displaced"], surfaceWaveSource=ch["source"],
                surfaceWaveSeed=ch["seed"], surfaceWaveSeedAmplitude=ch["seedAmp"], res=M.RES, outerRadius=float(a[0]), surfaceDensity=int(a[1]),
                nbSurfaceMaintenanceIterations=int(a[2]), dt=float(a[3]), waveSpeed=float(a[4]), waveDamping=float(a[5]), waveSeedFrequency=float(a[6]),
                waveMaxAmplitude=float(a[7]), waveMaxFrequency=float(a[8]), waveMaxSeedingAmplitude=float(a[9]),
                waveSeedingCurvatureThresholdRegionCenter=float(a[10]), waveSeedingCurvatureThresholdRegionRadius=float(a[11]),
                waveSeedStepSizeRatioOfMax=float(a[12]))


def _run(S, c):
    """a surfturb._Run on the scene with the parameters, frame count and list resolutions of case c"""
    from mantaflow_amd import surfturb
    s = S["flags"].parent
    a = c["args"]
    par, _ = surfturb._params(s.lib, c["frame"], M.RES, a[0], a[1], *a[3:])
    return surfturb._Run(s.lib, s, S["flags"], S["coarse"], S["prev"], S["surf"], S["chan"], par, int(c["R"][0]), int(c["R"][1]))


def test_parameters_and_direction_table_equal_the_reference(hip_backend):
    import manta as m
    from mantaflow_amd import surfturb
    G = M.golden()
    for k in range(3):
        c = M.init_case(G, k)
        s, S = _scene(m, c)
        a = c["args"]
        par, R = surfturb._params(s.lib, 0, M.RES, a[0], a[1], *a[3:])
        assert np.array(list(par)[:9], f32).tobytes() == G["set%d/par" % k].tobytes() and list(R) == G["set%d/res" % k].tolist()
        for frame in (0, 3):        # the model's block (tests/surfturb_model.par_of) is the library's, cosf(theta) included
            lib_par, _ = surfturb._params(s.lib, frame, M.RES, a[0], a[1], *a[3:])
            assert np.array(list(lib_par)[:23], f32).tobytes() == np.array([getattr(M.par_of(G, k, frame), n) for n in M.PAR_NAMES], f32).tobytes()
        if k:       # initFines alone: the direction table around every coarse particle near the surface, compacted in order
            surfturb.particleSurfaceTurbulence(**dict(_plugin_args(S, a), nbSurfaceMaintenanceIterations=0))
            assert S["surf"].get_positions().tobytes() == G["set%d/init_pos" % k].tobytes()
            assert not S["surf"].get_flags().any() and S["surf"].mDeleteChunk == S["surf"].np // 20
            assert surfturb.lastSurfaceTurbulenceStats()["init"] == S["surf"].np == S["displaced"].np


@pytest.mark.parametrize("f", [0, 1, 2])
def test_whole_calls_from_the_recorded_states(hip_backend, f):
    import manta as m
    from mantaflow_amd import surfturb
    G = M.golden()
    c = M.call_case(G, f)
    s, S = _scene(m, c)
    surfturb._state.frameCount, surfturb._state.Rc, surfturb._state.Rs = f, int(c["R"][0]), int(c["R"][1])
    surfturb.particleSurfaceTurbulence(**_plugin_args(S, c["args"]))
    want = M.state(G, "call%d/after" % f)
    print("call %d against the reference:" % f, M.compare(_state(S), want, exact=False))
    st = surfturb.lastSurfaceTurbulenceStats()
    print(st)
    model, its, model_displaced, _ = M.model_call(G, f)
    print("call %d: points that differ from the model: %d" % (f, M.compare_model(_state(S), model, "call %d" % f)))
    assert [(i["added"], tuple(i["kills"]), i["compressed"], i["size"]) for i in st["iterations"]] == \
        [(i["added"], i["kills"], i["compressed"], i["size"]) for i in its]
    gd = S["displaced"].get_positions()
    assert gd.shape == model_displaced.shape and int((gd.view(np.uint32) != model_displaced.view(np.uint32)).any(axis=1).sum()) <= 1
    assert surfturb._state.frameCount == f + 1 and st["frame"] == f and len(st["iterations"]) == (12 if f == 0 else 2)
    d, wd = S["displaced"].get_positions(), G["call%d/displaced" % f]
    assert d.shape == wd.shape and np.abs(d.astype(np.float64) - wd).max() <= M.POS_BOUND and not S["displaced"].get_flags().any()
    keep = (c["cflag"] & (M.PNEW | M.PDELETE)) == 0
    prev = S["prev"].to_numpy().reshape(-1, 3)
    assert prev[keep].tobytes() == c["cpos"][keep].tobytes() and prev[~keep].tobytes() == c["prev"][~keep].tobytes()
    if f == 0:
        # the surface list is empty during the first add / delete: every point inside the domain buffers a copy of itself, the greedy
        # pass sees no neighbour (one round, kills only outside the domain); the copies go in the second iteration
        it = st["iterations"]
        assert it[0]["added"] > 0.5 * st["init"] and it[0]["rounds"] == 1 and it[0]["kills"][0] == 0
        assert st["compressions"] >= 1 and not all(i["compressed"] for i in it)


@pytest.mark.parametrize("i", range(16))
def test_every_stage_of_the_recorded_chain(hip_backend, i):
    import manta as m
    G = M.golden()
    name = M.chain_names(G)[i]
    c = M.chain_case(G, i)
    s, S = _scene(m, c)
    run = _run(S, c)
    try:
        run.coarse_list(of_prev=name == "advect")
        run.surface_list()
        if name == "adddelete":
            added = run.add()
            rounds, kills = run.delete()
            did = run.compress_and_insert()
            print("added", added, "rounds", rounds, "kills", kills, "compressed", did)
            assert did == (c["sizes"][1] + sum(kills) > c["sizes"][2])
        elif name != "accel":
            getattr(run, name)()
        s.sync()
    finally:
        run.close()
    print("chain %d %s against the reference:" % (i, name), M.compare(_state(S), M.state(G, "chain/%d" % i), exact=name in M.EXACT_STAGES))
    mdl, want = M.model_stage(G, i)
    print("chain %d %s: points that differ from the model: %d" % (i, name, M.compare_model(_state(S), want, name)))
    if name == "adddelete":
        assert (added, kills, did) == (mdl.stats["added"], mdl.stats["kills"], mdl.stats["compressed"])


def _run_stage(S, c, name, empty=False):
    """one stage on the scene S of case c, with the lists the call has at that point"""
    run = _run(S, c)
    try:
        run.coarse_list(of_prev=name == "advect")
        run.surface_list(empty=empty)
        if name == "adddelete":
            out = (run.add(), run.delete()[1], run.compress_and_insert())
        else:
            out = getattr(run, name)() if name != "accel" else None
        S["flags"].parent.sync()
    finally:
        run.close()
    return out


@pytest.mark.parametrize("group", ["frame 0 iteration 0", "frame 0 iteration 1", "frame 0 iteration 11", "frame 1", "frame 2"])
def test_recorded_stages_inside_the_calls(hip_backend, group):
    """every stage of the first two and the last maintenance iteration of frame 0 and of the whole frames 1 and 2, each from the
    reference's recorded state before it: against the model by the rule, against the reference's state after it in sizes and flags
    exactly and in the values as far as they are not downstream of expf / logf.  The surface list is empty in the first add / delete
    (every point inside the domain buffers a copy of itself); the copies go in the second"""
    import manta as m
    G = M.golden()
    counts = []
    for what, name, c, want in M.stage_cases(G):
        if what != group and not what.startswith(group + " "):
            continue
        first = c.get("listed") == 0
        s, S = _scene(m, c)
        out = _run_stage(S, c, name, empty=first)
        got = _state(S)
        mdl = M.Model(M.par_of(G, 0, c["frame"]), c["R"], c, listed=c.get("listed"))
        counts.append(M.compare_model(got, mdl.run(name), (what, name)))
        print(what, name, "against the reference:", M.compare(got, want, exact=name in M.EXACT_STAGES))
        if name == "adddelete":
            assert out == (mdl.stats["added"], mdl.stats["kills"], mdl.stats["compressed"])
            if first:
                assert out[0] == int(M.in_domain(mdl.P, c["pos"]).sum()) > 0 and out[1][:2] == (0, 0) and out[1][2] > 0
    assert len(counts) == (4 if group.startswith("frame 0") else 10)
    print("%s: points that differ from the model per stage %s" % (group, counts))


@pytest.mark.parametrize("case", M.EDGE_CASES)
def test_every_stage_at_the_edges_against_the_model(hip_backend, case):
    import manta as m
    G = M.golden()
    counts = []
    for stage in M.EDGE_STAGES:
        c, mdl, want = M.edge_model(G, case, stage)
        s, S = _scene(m, c)
        out = _run_stage(S, c, stage)
        counts.append(M.compare_model(_state(S), want, (case, stage)))
        if stage == "adddelete":
            assert out == (mdl.stats["added"], mdl.stats["kills"], mdl.stats["compressed"])
            if case in ("compress", "no_compress"):
                assert out[2] == (case == "compress") and out[1][0] >= 12
    print("edge %s: points that differ from the model per stage %s" % (case, counts))


# ---- the index work at its edges, through the entries on tensors of exact size
def _lib_and_par(m, k=0):
    from mantaflow_amd import surfturb
    G = M.golden()
    s = m.Solver(name="e", gridSize=m.vec3(M.RES, M.RES, M.RES), dim=3)
    a = G["set%d/args" % k]
    par, R = surfturb._params(s.lib, 0, M.RES, a[0], a[1], *a[3:])
    return s, par, R, np.array(list(par), f32)


def _dev(s, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(s.device)


def _nan(s, n, dtype):
    import torch
    t = torch.empty(max(n, 1), dtype=torch.int32, device=s.device).fill_(NAN_BITS)
    return t.view(torch.float32) if dtype == "f" else t


def _cells(s, par, R, pos):
    """the library's cell list of pos[n][3] -> (start, ids) tensors"""
    from mantaflow_amd.core import _ptr
    n = len(pos)
    need = ctypes.c_int64(0)
    s.lib.call("mf_surfturb_tmp_bytes", n, R ** 3, max(n, 1), ctypes.byref(need))
    tmp = _nan(s, need.value // 4 + 1, "i")
    start, ids = _nan(s, R ** 3 + 1, "i"), _nan(s, n, "i")
    p = _dev(s, np.asarray(pos, f32).T.reshape(-1) if n else np.zeros(1, f32))
    s.lib.call("mf_surfturb_cells", par, R, n, n, _ptr(p), _ptr(start), _ptr(ids), _ptr(tmp), need.value, s.stream)
    return start, ids, p


def _edge_points(name, n, rng):
    if name == "random":
        pos = rng.uniform(4, 4 + 0.25 * max(n, 1) ** (1 / 3.0), (n, 3)).astype(f32)
    elif name == "one_cell":
        pos = (f32(5.01) + rng.uniform(0, 0.2, (n, 3))).astype(f32)
    pos = pos.copy()
    flag = np.zeros(n, i32)
    if n >= 63 and name == "random":
        pos[3] = pos[40]                                    # exact duplicates
        pos[7] = [1.5, 5, 5]                                # outside the domain
        pos[11] = [5, 10.5, 5]
        pos[20] = [np.nan, 5, 5]                            # deleted slots holding inf / NaN
        pos[21] = [np.inf, -np.inf, 5]
        pos[22] = [1e30, 5, 5]
        flag[[20, 21, 22, 30]] = M.PDELETE
    return pos, flag


@pytest.mark.parametrize("name,n", [("random", 0), ("random", 1), ("random", 63), ("random", 64), ("random", 65), ("random", 257), ("one_cell", 90)])
def test_cell_list_and_greedy_pass_at_the_edges(hip_backend, name, n):
    import manta as m
    from mantaflow_amd.core import _ptr
    s, par, R, p = _lib_and_par(m)
    Rs = int(R[1])
    rng = np.random.RandomState(n + 1)
    pos, flag = _edge_points(name, n, rng)
    listed = n - n // 5                                     # the last fifth are appended points: tested, never seen
    start, ids, _ = _cells(s, par, Rs, pos[:listed])
    ws, wi = M.cell_list(pos[:listed], M.RES, Rs)
    assert np.array_equal(start.cpu().numpy(), ws) and np.array_equal(ids.cpu().numpy()[:listed], wi[:listed])
    if name == "one_cell":
        assert np.diff(ws).max() == listed >= 70           # every listed point in one cell
    radius, lo, hi = p[21], p[7], p[8]
    dp, df = _dev(s, pos.T.reshape(-1) if n else np.zeros(1, f32)), _dev(s, flag if n else np.zeros(1, i32))
    a, b, head = _nan(s, n, "i"), _nan(s, n, "i"), _nan(s, 64, "i")
    und, rounds = ctypes.c_int32(1), 0
    while und.value and rounds <= n:
        s.lib.call("mf_surfturb_greedy_round", par, Rs, _ptr(start), _ptr(ids), n, n, _ptr(dp), _ptr(df), int(rounds == 0), _ptr(a), _ptr(b), _ptr(head),
                   ctypes.byref(und), s.stream)
        a, b = b, a
        rounds += 1
    want = M.greedy_serial(pos, flag, listed, radius, lo, hi)
    want2, want_rounds = M.greedy_rounds(pos, flag, listed, radius, lo, hi)
    assert np.array_equal(want, want2)
    if n:
        got = a.cpu().numpy()[:n]
        assert set(got.tolist()) <= {1, 2} and np.array_equal(got == 2, want)
        assert rounds == want_rounds
        print(name, n, "rounds", rounds, "killed", int(want.sum()))
    else:
        assert rounds == 1 and und.value == 0


@pytest.mark.parametrize("order", [1, -1])
def test_greedy_rounds_of_a_line_equal_its_length(hip_backend, order):
    import manta as m
    from mantaflow_amd.core import _ptr
    s, par, R, p = _lib_and_par(m)
    Rs, n, d = int(R[1]), 9, p[3]
    pos = np.stack([f32(4) + d * f32(0.5) * np.arange(n, dtype=f32)[::order], np.full(n, 5, f32), np.full(n, 5, f32)], 1)
    flag = np.zeros(n, i32)
    start, ids, dp = _cells(s, par, Rs, pos)
    df, a, b, head = _dev(s, flag), _nan(s, n, "i"), _nan(s, n, "i"), _nan(s, 64, "i")
    und, rounds = ctypes.c_int32(1), 0
    while und.value and rounds <= n:
        s.lib.call("mf_surfturb_greedy_round", par, Rs, _ptr(start), _ptr(ids), n, n, _ptr(dp), _ptr(df), int(rounds == 0), _ptr(a), _ptr(b), _ptr(head),
                   ctypes.byref(und), s.stream)
        a, b = b, a
        rounds += 1
    assert rounds == n and (a.cpu().numpy() == 2).tolist() == [True] * (n - 1) + [False]
    assert np.array_equal(a.cpu().numpy() == 2, M.greedy_serial(pos, flag, n, p[21], p[7], p[8]))


def _density_model(pos, flag, p, Rs):
    """computeSurfaceDensities in numpy: cells i outer, j, k inner, slots ascending, inactive ones skipped; per neighbour the ghost chain
    x-, x+, y-, y+, z-, z+ and the neighbour itself; fp32 in order"""
    res, radius, bm, bp = p[0], p[5], p[7], p[8]
    start, ids = M.cell_list(pos, res, Rs)
    out = np.zeros(len(pos), f32)

    def coord(v):
        return int(np.clip(np.floor(f32(v) / res * f32(Rs)), 0, Rs - 1))
    for i, c in enumerate(pos):
        lo, hi = [coord(c[a] - radius) for a in range(3)], [coord(c[a] + radius) for a in range(3)]
        acc = f32(0)
        for ci in range(lo[0], hi[0] + 1):
            for cj in range(lo[1], hi[1] + 1):
                for ck in range(lo[2], hi[2] + 1):
                    cell = (ci * Rs + cj) * Rs + ck
                    for j in ids[start[cell]:start[cell + 1]]:
                        if flag[j] & M.PDELETE:
                            continue
                        q = pos[j]
                        images = []
                        for a in range(3):
                            if q[a] - bm <= radius:
                                g = q.copy(); g[a] = f32(2) * bm - q[a]; images.append(g)
                            if bp - q[a] <= radius:
                                g = q.copy(); g[a] = f32(2) * bp - q[a]; images.append(g)
                        images.append(q)
                        for g in images:
                            dist = M._norm(c - g)
                            acc = f32(acc + (f32(0) if dist > radius else f32(1) - f32(dist / radius)))
        out[i] = acc
    return out


def test_densities_with_ghosts_at_the_six_planes_and_in_a_corner(hip_backend):
    import manta as m
    from mantaflow_amd.core import _ptr
    s, par, R, p = _lib_and_par(m)
    Rs = int(R[1])
    rng = np.random.RandomState(5)
    centres = [[2.2, 6, 6], [9.8, 6, 6], [6, 2.2, 6], [6, 9.8, 6], [6, 6, 2.2], [6, 6, 9.8], [2.3, 2.3, 2.3], [9.7, 9.7, 2.2], [6, 6, 6]]
    pos = np.concatenate([np.array(c, f32) + rng.uniform(-0.3, 0.3, (12, 3)).astype(f32) for c in centres]).astype(f32)
    pos[5] = [2, 6, 6]                                      # on a plane
    flag = np.zeros(len(pos), i32)
    flag[[1, 14, 80]] = M.PDELETE
    n = len(pos)
    start, ids, dp = _cells(s, par, Rs, pos)
    before = dp.clone()
    df, nrm = _dev(s, flag), _dev(s, np.zeros(3 * n, f32))
    tempf, tempv = _nan(s, n, "f"), _nan(s, 3 * n, "f")
    s.lib.call("mf_surfturb_regularize", par, Rs, _ptr(start), _ptr(ids), n, n, _ptr(dp), _ptr(df), _ptr(nrm), _ptr(tempf), _ptr(tempv), s.stream)
    want = _density_model(pos, flag, p, Rs)
    got = tempf.cpu().numpy()[:n]
    assert got.tobytes() == want.tobytes()
    far = p.copy()
    far[7], far[8] = -100, 100                              # the same model without images: they matter at every plane and corner, not inside
    plain = _density_model(pos, flag, far, Rs)
    assert (want[:96] != plain[:96]).reshape(8, 12).any(axis=1).all() and want[96:].tobytes() == plain[96:].tobytes()
    # zero normals: no displacement passes the projected-normal test, the positions stay as they were
    assert np.array_equal(dp.cpu().numpy(), before.cpu().numpy()) and not np.isnan(tempv.cpu().numpy()[:3 * n]).any()


def test_second_dimension_refusal_and_debug_check_parts(hip_backend):
    import manta as m
    from mantaflow_amd import surfturb
    from test_surfturb_api import _scene as api_scene, _snapshot
    surfturb.resetSurfaceTurbulenceState()
    s, args = api_scene(m, dim=2)
    before = _snapshot(args)
    with pytest.raises(RuntimeError) as e:
        surfturb.particleSurfaceTurbulence(**args)
    assert str(e.value) == "particleSurfaceTurbulence: surface turbulence does not run on a 2-D solver"
    assert _snapshot(args) == before
    s, args = api_scene(m)
    pp = args["coarseParts"]
    surfturb.debugCheckParts(pp, args["flags"])
    surfturb.debugCheckParts(args["surfacePointsDisplaced"], args["flags"])        # empty
    pos = np.tile(np.array([[5, 5, 5]], f32), (300, 1))
    pos[[77, 290]] = [[5, 12.5, 5], [-1, 5, 5]]
    pp.set_positions(pos)
    with pytest.raises(RuntimeError, match=r"^bad position\?\?\? 77 \[\+5.00,\+12.50,\+5.00\]$"):
        surfturb.debugCheckParts(pp, args["flags"])


LOOP_ARGS = [1.0, 15, 2, 0.005, float(M.RES), 0.1, 4.0, 0.5, 128.0, 0.5, 0.025, 0.01, 0.05]


def harness_loop(frames=3, first_nb=None):
    """the loop of the reference's harness script test_2100_surfTurb.py (a basin and a drop; FLIP with unionParticleLevelset, the
    ghost-fluid solve and adjustNumber; the plugin with the script's arguments) at res 12 with two maintenance iterations, the plugin
    imported the way a scene does.  Yields per frame (t, the plugin's inputs as a case, the scene, the solver) after the call.
    first_nb: the maintenance iterations of the first call only (0: initFines alone)"""
    g = {}
    exec("from mantaflow_amd.surfturb import *\nfrom manta import *", g)
    g["resetSurfaceTurbulenceState"]()
    res = M.RES
    gs = g["vec3"](res, res, res)
    s = g["Solver"](name="main", gridSize=gs, dim=3)
    s.timestep = 0.8
    flags, phi, vel, velOld, pressure, tmpVec3 = (s.create(g[k]) for k in ("FlagGrid", "LevelsetGrid", "MACGrid", "MACGrid", "RealGrid", "VecGrid"))
    spd, pp, sp = (s.create(g["BasicParticleSystem"]) for _ in range(3))
    pVel, pPrev = pp.create(g["PdataVec3"]), pp.create(g["PdataVec3"])
    nrm = sp.create(g["PdataVec3"])
    H, DtH, src, amp, seed = (sp.create(g["PdataReal"]) for _ in range(5))
    pindex, gpi = s.create(g["ParticleIndexSystem"]), s.create(g["IntGrid"])
    flags.initDomain(boundaryWidth=1)
    phi = s.create(g["Box"], p0=gs * g["vec3"](0, 0, 0), p1=gs * g["vec3"](1.0, 0.2, 1.0)).computeLevelset()
    phi.join(s.create(g["Sphere"], center=gs * g["vec3"](0.5, 0.4, 0.5), radius=res * 0.1).computeLevelset())
    flags.updateFromLevelset(phi)
    g["sampleLevelsetWithParticles"](phi=phi, flags=flags, parts=pp, discretization=2, randomness=0.35)
    chan = dict(normals=nrm, H=H, DtH=DtH, source=src, seed=seed, seedAmp=amp)
    S = dict(flags=flags, coarse=pp, prev=pPrev, surf=sp, displaced=spd, chan=chan)
    for t in range(frames):
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=g["IntRK4"], deleteInObstacle=False)
        g["mapPartsToMAC"](vel=vel, flags=flags, velOld=velOld, parts=pp, partVel=pVel, weight=tmpVec3)
        g["extrapolateMACFromWeight"](vel=vel, distance=2, weight=tmpVec3)
        g["markFluidCells"](parts=pp, flags=flags)
        g["gridParticleIndex"](parts=pp, flags=flags, indexSys=pindex, index=gpi)
        g["unionParticleLevelset"](pp, pindex, flags, gpi, phi, radiusFactor=1.)
        g["resetOutflow"](flags=flags, parts=pp, index=gpi, indexSys=pindex)
        g["extrapolateLsSimple"](phi=phi, distance=4, inside=True)
        g["addGravity"](flags=flags, vel=vel, gravity=(0, -0.001, 0))
        g["setWallBcs"](flags=flags, vel=vel)
        g["solvePressure"](flags=flags, vel=vel, pressure=pressure, phi=phi)
        g["setWallBcs"](flags=flags, vel=vel)
        pVel.setSource(vel, isMAC=True)
        g["adjustNumber"](parts=pp, vel=vel, flags=flags, minParticles=8, maxParticles=16, phi=phi, radiusFactor=1.)
        g["extrapolateMACSimple"](flags=flags, vel=vel)
        g["flipVelocityUpdate"](vel=vel, velOld=velOld, flags=flags, parts=pp, partVel=pVel, flipRatio=0.97)
        c = dict(_state(S), flags=flags.to_numpy(), cpos=pp.get_positions(), cflag=pp.get_flags(), prev=pPrev.to_numpy().reshape(-1, 3))
        a = list(LOOP_ARGS)
        if t == 0 and first_nb is not None:
            a[2] = first_nb
        g["particleSurfaceTurbulence"](**_plugin_args(S, a))
        g["debugCheckParts"](spd, flags)
        yield t, c, S, s
        s.step()


def test_harness_loop_call_by_call_against_the_model_and_the_reference(hip_backend):
    """three frames of harness_loop.  The fixture holds the coarse particles the loop hands to the plugin (loop/<t>/coarse_*, taken
    from this loop) and what the reference's plugin made of them (tools/record_surfturb.py --loop): the loop must hand over the same
    particles bit for bit, and the sizes, the delete bookkeeping and the flags after every call must equal the reference's.  Every
    call is also run again in the model from the same inputs.  The direction table of the loop's parameters is the library's host
    code; loop/init_pos pins it to the reference (test_harness_loop_first_points_equal_the_reference)."""
    import ctypes
    from mantaflow_amd import surfturb
    G = M.golden()
    a, sizes = LOOP_ARGS, []
    for t, c, S, s in harness_loop():
        sp, spd = S["surf"], S["displaced"]
        st = surfturb.lastSurfaceTurbulenceStats()
        got = _state(S)
        live = int(((got["flag"] & M.PDELETE) == 0).sum())
        assert st["frame"] == t and st["displaced"] == spd.np == live and live > 200 and len(st["iterations"]) == (12 if t == 0 else 2)
        for k, v in (("coarse_pos", c["cpos"]), ("coarse_flag", c["cflag"]), ("coarse_prev", c["prev"])):
            w = G["loop/%d/%s" % (t, k)]
            assert v.shape == w.shape and v.tobytes() == w.tobytes(), "frame %d: the loop hands the plugin other coarse particles (%s) than were recorded" % (t, k)
        want = G["loop/%d/after/sizes" % t]
        print("frame %d: sizes %s, the reference's %s" % (t, got["sizes"], want[:3].tolist()))
        assert [int(x) for x in got["sizes"]] == want[:3].tolist() and live == int(want[3])
        assert np.array_equal(got["flag"], G["loop/%d/after/flag" % t])
        par, _ = surfturb._params(s.lib, t, M.RES, a[0], a[1], *a[3:])
        count = ctypes.c_int64(0)
        s.lib.call("mf_surfturb_directions", par, 0, None, ctypes.byref(count))
        host = (ctypes.c_float * (3 * count.value))()
        s.lib.call("mf_surfturb_directions", par, count.value, host, ctypes.byref(count))
        mdl, its, disp = M.model_call_case(M.Par(np.array(list(par), f32)), (st["Rc"], st["Rs"]), c, t, 2, dirs=np.array(list(host), f32))
        print("frame %d: points that differ from the model: %d" % (t, M.compare_model(got, mdl.state(), "frame %d" % t)))
        assert [(i["added"], tuple(i["kills"]), i["compressed"], i["size"]) for i in st["iterations"]] == \
            [(i["added"], i["kills"], i["compressed"], i["size"]) for i in its]
        assert int((spd.get_positions().view(np.uint32) != disp.view(np.uint32)).any(axis=1).sum()) <= 1
        sizes.append(sp.np)
    print("surface points per frame:", sizes)


def test_harness_loop_first_points_equal_the_reference(hip_backend):
    """initFines alone under the loop's parameters (surfaceDensity 15, outerRadius 1): the library's direction table around the loop's
    coarse particles, against the reference's points bit for bit"""
    G = M.golden()
    for t, c, S, s in harness_loop(frames=1, first_nb=0):
        assert c["cpos"].tobytes() == G["loop/0/coarse_pos"].tobytes()
        assert S["surf"].get_positions().tobytes() == G["loop/init_pos"].tobytes() and not S["surf"].get_flags().any()

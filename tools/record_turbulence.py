"""Recorder of tests/golden/turbulence.npz: the reference's outputs for the fixture cases of tests/turbulence_model.py (inputs are
regenerated from its seeded generators, never stored) and for the recorded k-epsilon loop.  No test runs this; it needs the reference
checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays in a scratch directory outside the tree.
Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/kepsilon.cpp $B/plugin/kepsilon.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libturbulence_rec.so $B/plugin/kepsilon.cpp tools/turbulence_record.cpp \\
        -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_turbulence.py $B/libturbulence_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction; turbulencepart.cpp and waveletturbulence.cpp are
part of oracle/ref.mk's library)

Arrays of more than turbulence_model.FULL_LIMIT elements are kept as the SHA-256 of their bytes under <key>#sha: the cases at
33 x 31 x 29 and the loop alone would be 3 MB of incompressible floats.  Before anything is written the recorder asserts that the
numpy model reproduces every recorded array bit for bit, so a digest in the file is the digest of an array the model can regenerate.

All particle cases run in this one process in the fixed order PARTICLE_ORDER and the loop after them, because seed()'s random stream
and synthesize()'s clock and inflow offset are statics of the reference.  The file holds <plugin>/<case>/<array>; for the particle
cases parts/<case>/{pos, color, tex0, tex1, flag, sizes, cursors, start}: the system after the last call, its size and the stream
position after every call, and the state (stream position, clock bits, inflow bits) at which the case began; loop/...  The conditions
each case exists for are asserted here and again, from the model's counters, in tests/test_turbulence_model.py.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import turbulence_model as M  # noqa: E402

f32 = np.float32


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def soa(g):
    """[z][y][x][3] -> [3][n]"""
    return np.ascontiguousarray(np.asarray(g, f32).reshape(-1, 3).T)


def aos(a, shape):
    return np.ascontiguousarray(a.reshape(3, -1).T.reshape(shape + (3,)))


def fc(x):
    return ctypes.c_float(float(x))


def same(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape)
    u = "u%d" % got.dtype.itemsize
    d = got.view(u) != want.view(u)
    assert not d.any(), "%s: the model differs from the reference in %d of %d words, first at %s (%r vs %r)" % (
        tag, int(d.sum()), d.size, np.argwhere(d)[0], got[tuple(np.argwhere(d)[0])], want[tuple(np.argwhere(d)[0])])


def record_grids(call, out):
    cnt = {}
    for name in M.PRODUCTION_CASES:
        I = M.ke_inputs(name, nan=True)
        sx, sy, sz = I["dims"]
        sh = M.shape_of(I["dims"])
        res = {}
        for with_strain in (True, False):
            k, eps = I["k"].copy(), I["eps"].copy()
            prod, nuT = M.prefill(name, "prod"), M.prefill(name, "nuT")
            strain = M.prefill(name, "strain") if with_strain else None
            call("rec_production", sx, sy, sz, P(soa(I["vel"])), P(k), P(eps), P(prod), P(nuT), P(strain), fc(M.PSCALE))
            r = dict(k=k, eps=eps, prod=prod, nuT=nuT)
            if with_strain:
                r["strain"] = strain
            model = M.run_production(name, with_strain, cnt)
            for key in r:
                same("production/%s/%s" % (name, key), model[key], r[key])
            res[with_strain] = r
        for key in ("k", "eps", "prod", "nuT"):      # strain = None changes nothing else: kept once
            same("production/%s/%s without strain" % (name, key), res[False][key], res[True][key])
        for key, a in res[True].items():
            M.put(out, "production/%s/%s" % (name, key), a)
        b = ~M.interior_mask(sh)
        assert np.array_equal(res[True]["prod"][b], M.prefill(name, "prod")[b]) and np.array_equal(res[True]["strain"][b], M.prefill(name, "strain")[b])
    for name in M.SOURCES_CASES:
        I = M.ke_inputs(name)
        sx, sy, sz = I["dims"]
        k, eps = I["k"].copy(), I["eps"].copy()
        call("rec_sources", sx, sy, sz, fc(M.DT), P(k), P(eps), P(I["prod"]))
        model = M.run_sources(name, cnt)
        for key, a in (("k", k), ("eps", eps)):
            same("sources/%s/%s" % (name, key), model[key], a)
            M.put(out, "sources/%s/%s" % (name, key), a)
        for fill in (False, True):
            k, eps = I["k"].copy(), I["eps"].copy()
            call("rec_bcs", sx, sy, sz, P(I["flags"]), P(k), P(eps), fc(M.BCS["intensity"]), fc(M.BCS["nu"]), int(fill))
            model = M.run_bcs(name, fill)
            for key, a in (("k", k), ("eps", eps)):
                same("bcs/%s/%d/%s" % (name, fill, key), model[key], a)
                M.put(out, "bcs/%s/%d/%s" % (name, fill, key), a)
            assert fill or ((k != I["k"]).any() and (k == I["k"]).any())
    print("branch counts:", cnt)
    for key in ("k_low", "k_high", "nu_high", "nu_low", "eps_nonpositive", "eps_nan", "eps_positive", "ke_nonpositive", "newEps_nonpositive", "strain_none",
                "strain_given"):
        assert cnt.get(key, 0) > 0, key
    for name in M.GRADDIFF_CASES:
        I = M.graddiff_inputs(name)
        sx, sy, sz = I["dims"]
        sh = M.shape_of(I["dims"])
        for with_vel in (False, True):
            k, eps = I["k"].copy(), I["eps"].copy()
            vel = soa(I["vel"]) if with_vel else None
            call("rec_graddiff", sx, sy, sz, fc(M.DT), 2, P(k), P(eps), P(I["nuT"]), fc(M.SIGMA_U), P(vel))
            r = dict(k=k, eps=eps)
            if with_vel:
                r["vel"] = aos(vel, sh)
            model = M.run_graddiff(name, with_vel)
            for key, a in r.items():
                assert np.isfinite(a).all(), (name, key)
                same("graddiff/%s/%d/%s" % (name, with_vel, key), model[key], a)
                M.put(out, "graddiff/%s/%d/%s" % (name, with_vel, key), a)
        assert np.signbit(r["k"][~M.interior_mask(sh)]).sum() == 0
    for name in M.DIAG_CASES:
        sx, sy, sz = M.DIMS[name]
        sh = M.shape_of(M.DIMS[name])
        vel = M.rand_vel(name, 2.0)
        mag, vort, nrm, curl = M.prefill(name, "mag"), soa(M.diag_prefill_vec(name)), np.full(sh, 77, f32), np.zeros((3,) + sh, f32)
        call("rec_diagnostics", sx, sy, sz, P(soa(vel)), P(mag), P(vort), P(nrm), P(curl))
        r = dict(mag=mag, vort=aos(vort, sh), norm=nrm, curl0=curl[0], curl1=curl[1], curl2=curl[2])
        model = M.run_diagnostics(name)
        for key, a in r.items():
            same("diag/%s/%s" % (name, key), model[key], a)
            M.put(out, "diag/%s/%s" % (name, key), a)


def record_particles(L, call, out):
    """the particle cases in PARTICLE_ORDER on one stage, then the loop; the model runs beside the reference and must agree"""
    i64 = ctypes.c_int64
    tile, params = M.noise_tile_and_params(M.PDIMS)
    flags, vel, k = M.particle_grids()
    sx, sy, sz = M.PDIMS
    call("rec_stage_open", sx, sy, sz, fc(M.PDT), P(flags), P(soa(vel)), P(k))
    st, cnt = M.State(), {}
    for name in M.PARTICLE_ORDER:
        start = st.snapshot()
        call("rec_stage_clear")
        sizes = []
        for op in M.PARTICLE_CASES[name]:
            if op[0] == "seed":
                a = np.array(op[2][0], f32)
                b = np.array(op[2][1] if op[1] == "box" else [op[2][1]] * 3, f32)
                call("rec_stage_seed", 0 if op[1] == "box" else 1, P(a), P(b), op[3])
            elif op[0] == "advect":
                call("rec_stage_advect")
            elif op[0] == "synth":
                call("rec_stage_synthesize", op[1], fc(op[2]), fc(op[3]), fc(op[4]), P(np.array(op[5], f32)))
            elif op[0] == "delete":
                call("rec_stage_delete")
            elif op[0] == "move":
                call("rec_stage_move", i64(op[1]), P(np.array(op[2], f32)))
            sizes.append(int(L.rec_stage_size()))
        n = sizes[-1]
        cap = max(n, 1)
        arrs = [np.zeros((3, cap), f32) for _ in range(4)] + [np.zeros(cap, np.int32)]
        call("rec_stage_read", i64(cap), *[P(a) for a in arrs])
        ref = {c: (np.ascontiguousarray(a[:, :n].T) if a.ndim == 2 else a[:n].copy()) for c, a in zip(M.CHANNELS, arrs)}
        state, msizes, cursors = M.run_particle_case(name, st, tile, params, cnt)
        assert list(msizes) == sizes, (name, list(msizes), sizes)
        for c in M.CHANNELS:
            same("parts/%s/%s" % (name, c), state[c], ref[c])
            M.put(out, "parts/%s/%s" % (name, c), ref[c])
        out["parts/%s/sizes" % name] = np.array(sizes, np.int64)
        out["parts/%s/cursors" % name] = cursors
        out["parts/%s/start" % name] = start
        print("parts", name, "sizes", sizes, "cursor", int(cursors[-1]))
    call("rec_stage_close")
    print("particle branch counts:", cnt)
    for key in M.PARTICLE_CONDITIONS:
        assert cnt.get(key, 0) > 0, key

    # ---- the loop (it continues the statics)
    C = M.LOOP
    res, steps = C["res"], C["steps"]
    n = res * (res // 2) * (res // 2)
    sh = (res // 2, res // 2, res)
    per_step = np.zeros((steps, 2), np.int64)
    grids = np.zeros((9, n), f32)
    cap = 500 * steps
    arrs = [np.zeros((3, cap), f32) for _ in range(4)] + [np.zeros(cap, np.int32)]
    np_out, obs = i64(0), i64(0)
    call("rec_loop", res, steps, fc(C["dt"]), P(per_step), P(grids), i64(cap), ctypes.byref(np_out), *[P(a) for a in arrs], ctypes.byref(obs))
    print("loop: obstacle cells", obs.value, "per step (particles, CG iterations):\n", per_step)
    assert obs.value >= 16, "the spheres mark no obstacle cells at this resolution"
    assert per_step[0, 0] > 0 and (per_step[:, 1] > 0).all()
    out["loop/start"] = st.snapshot()
    out["loop/per_step"] = per_step
    out["loop/obstacle_cells"] = np.array([obs.value], np.int64)
    for q, key in enumerate(("k", "eps", "prod", "nuT", "strain", "pressure")):
        M.put(out, "loop/" + key, grids[q].reshape(sh))
    M.put(out, "loop/vel", aos(grids[6:9], sh))
    out["loop/k"] = grids[0].reshape(sh).copy()          # two grids in full beside the digests, for a diagnosis
    out["loop/strain"] = grids[4].reshape(sh).copy()
    for key in ("loop/k#sha", "loop/strain#sha"):
        out.pop(key, None)
    m = np_out.value
    for c, a in zip(M.CHANNELS, arrs):
        M.put(out, "loop/parts/" + c, np.ascontiguousarray(a[:, :m].T) if a.ndim == 2 else a[:m].copy())


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p
    L.rec_stage_size.restype = ctypes.c_int64

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    record_grids(call, out)
    record_particles(L, call, out)
    path = os.path.join(ROOT, "tests", "golden", "turbulence.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])

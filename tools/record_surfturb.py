"""Recorder of tests/golden/surfturb.npz: the reference's particleSurfaceTurbulence on a small seeded scene.  No test runs this; it
needs the reference checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays under oracle/_ref/.
Run on the CPU machine (REF: the reference checkout):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    OMP_NUM_THREADS=1 python tools/record_surfturb.py REF [LOOP.npz]

It expands plugin/surfaceturbulence.cpp with `prep` into oracle/_ref/build/surfturb/, compiles tools/surfturb_record.cpp (which
includes the expanded source) with the flags of oracle/ref.mk (-O3, no -march, so no contraction; fp32 Real) against libmanta_ref.so,
and runs it with one thread.  The reference keeps its state in process-wide globals, so each parameter set runs in a process of its
own (this script starts itself again with --set K).

The file holds arrays only.  Per parameter set K in 0..2: set<K>/par (the nine derived parameters), set<K>/res (the two list
resolutions), set<K>/args, set<K>/init_pos (the surface points of a first call with nb = 0: the direction table times outerRadius
around the coarse particles).  For set 0 the scene: flags, and per frame f in 0..2 call<f>/coarse_{pos,flag,prev} and the surface
state before and after the whole call (call<f>/before/*, call<f>/after/*, .../sizes = size, mDeletes, mDeleteChunk, displaced size,
frameCount, coarse size), call<f>/displaced; then a chain of single stages run on the state the last call left, chain/names and
chain/<i>/* the state after stage i (chain/start/* before the first), for two maintenance iterations, the wave passes and, after
the coarse particles moved once more (chain/coarse2_pos), the advection; chain/costheta is cosf(theta) of those wave passes.

The stages INSIDE the calls, st<f>/...: frame f is driven stage by stage in a process of its own (after f whole calls; frame 0 after
a first call with nb = 0, which runs initFines and leaves the surface list empty as the whole call has it), and the state it ends in
must equal call<f>/after bit for bit, or nothing is written.  Recorded are the first two and the last maintenance iteration of frame
0 and everything of frames 1 and 2: st<f>/<it>/start/* the full state before iteration it, st<f>/<it>/<j>/<key> what stage j of
the iteration (adddelete, accel, normals, regularize, accel, constrain, accel) changed, with its sizes; for f > 0 also
st<f>/advect/pos, st<f>/waves/real and st<f>/costheta.  tests/surfturb_model.stage_cases puts the states together again.

The harness loop, loop/...: tests/test_gpu_surfturb.harness_loop is the loop of the reference's test_2100_surfTurb.py at res 12.
LOOP.npz holds what that loop, run by the package on the GPU, hands to the plugin in each of three frames (loop/flags of the first,
loop/<t>/coarse_{pos,flag,prev}); without the argument these arrays are taken from the fixture as it is.  The reference's plugin is
run on them with the script's arguments (LOOP_ARGS): loop/<t>/after/{flag,sizes}, and loop/init_pos, its points after a first call
with nb = 0.

The recorder refuses to write when a decision downstream of expf / logf is undecided within the bounds of DESIGN.md section 27 at
a recorded stage: a constraint level within MARGIN of a threshold (-0.2, 0, 1, 1.2), and -- found by running the numpy model of
tests/surfturb_model.py on every recorded stage -- dot(gradient, normal) of the fitted normal, an added point's distance to the
domain planes, and its distance to a neighbour against the add radius.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDIR = os.path.join(ROOT, "oracle", "_ref")
B = os.path.join(REFDIR, "build", "surfturb")
f32 = np.float32
LEVEL_BOUND = 2e-5      # the level's error bound of DESIGN.md section 27 (tests/surfturb_model.py)
MARGIN = LEVEL_BOUND

RES = 12
SEED = int(os.environ.get("SURFTURB_SEED", "40"))      # the scene seed; another one is tried through the environment
# (outerRadius, surfaceDensity, nb, dt, waveSpeed, waveDamping, waveSeedFrequency, waveMaxAmplitude, waveMaxFrequency,
#  waveMaxSeedingAmplitude, centre, radius, step)
SETS = [
    (1.0, 12, 2, 0.005, 12.0, 0.1, 4.0, 0.5, 128.0, 0.5, 0.025, 0.01, 0.05),      # the harness script's, at res 12
    (1.0, 20, 2, 0.005, 16.0, 0.0, 4.0, 0.25, 800.0, 0.5, 0.025, 0.01, 0.05),     # the defaults
    (0.8, 15, 2, 0.005, 32.0, 0.05, 4.0, 0.5, 128.0, 0.5, 0.025, 0.01, 0.05),
]
LOOP_ARGS = (1.0, 15, 2, 0.005, float(RES), 0.1, 4.0, 0.5, 128.0, 0.5, 0.025, 0.01, 0.05)
ITER = ["adddelete", "accel", "normals", "regularize", "accel", "constrain", "accel"]
CHAIN = ITER * 2 + ["waves"]
CHANGED = {"adddelete": ("pos", "flag", "normals", "real"), "normals": ("normals",), "regularize": ("pos",), "constrain": ("pos",)}


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def scene(seed=SEED):
    """coarse particles of a jittered block, their flags (a few PNEW / PDELETE), the flag grid, and a displacement per frame"""
    rng = np.random.RandomState(seed)
    ax = np.arange(3.4, 5.81, 0.4)
    ay = np.arange(3.4, 5.01, 0.4)
    pos = np.stack(np.meshgrid(ax, ay, ax, indexing="ij"), -1).reshape(-1, 3)
    pos = (pos + rng.uniform(-0.12, 0.12, pos.shape)).astype(f32)
    flag = np.zeros(len(pos), np.int32)
    flag[rng.choice(len(pos), 6, replace=False)] = 1        # PNEW
    flag[rng.choice(len(pos), 6, replace=False)] |= 1 << 10 # PDELETE
    grid = np.full((RES, RES, RES), 4, np.int32)            # TypeEmpty, [z][y][x]
    grid[[0, -1]] = grid[:, [0, -1]] = grid[:, :, [0, -1]] = 2
    c = pos.astype(np.int32)
    grid[c[:, 2], c[:, 1], c[:, 0]] = 1                     # TypeFluid
    assert c.min() >= 1 and c.max() <= RES - 2              # the precondition of initFines
    moves = [(rng.uniform(-0.05, 0.05, pos.shape) + np.array([0.06, -0.04, 0.03])).astype(f32) for _ in range(4)]
    return pos, flag, grid, moves


def build(ref):
    os.makedirs(os.path.join(B, "plugin"), exist_ok=True)
    prep = os.path.join(REFDIR, "build", "prep")
    subprocess.check_call([prep, "generate", "0", "OPENMP", ref + "/source/", "plugin/surfaceturbulence.cpp",
                           os.path.join(B, "plugin", "surfaceturbulence.cpp")], stdout=subprocess.DEVNULL)
    pp = os.path.join(REFDIR, "build", "pp", "source")
    out = os.path.join(B, "libsurfturb_rec.so")
    inc = [B, pp, pp + "/util", pp + "/fileio", ref + "/source/nopython", ref + "/source/util", ref + "/source/fileio", ref + "/dependencies/cnpy"]
    subprocess.check_call(["g++", "-O3", "-DNDEBUG", "-DNOPYTHON=1", "-DMANTA_MT=1", "-DOPENMP=1", "-fopenmp", "-fPIC", "-std=c++14", "-w"]
                          + ["-I" + i for i in inc] + ["-shared", "-o", out, os.path.join(ROOT, "tools", "surfturb_record.cpp"),
                                                       "-L" + REFDIR, "-lmanta_ref", "-Wl,-rpath," + REFDIR])
    return out


class Rec(object):
    def __init__(self, libpath):
        self.L = ctypes.CDLL(libpath)
        self.L.rec_last_error.restype = ctypes.c_char_p

    def call(self, name, *args):
        if getattr(self.L, name)(*args):
            raise RuntimeError(self.L.rec_last_error().decode())

    def plugin(self, a):
        fc = lambda x: ctypes.c_float(float(x))
        self.call("rec_call", RES, fc(a[0]), int(a[1]), int(a[2]), *[fc(x) for x in a[3:]])

    def sizes(self):
        s = (ctypes.c_int64 * 6)()
        self.call("rec_sizes", s)
        return np.array(list(s), np.int64)

    def surface(self):
        sz = self.sizes()
        n = int(sz[0])
        pos, flag, nrm, real = np.zeros((n, 3), f32), np.zeros(n, np.int32), np.zeros((n, 3), f32), np.zeros((5, n), f32)
        self.call("rec_get_surface", P(pos), P(flag), P(nrm), P(real))
        lev = np.zeros(n, f32)
        self.call("rec_levels", P(lev))
        return dict(pos=pos, flag=flag, normals=nrm, real=real, sizes=sz), lev

    def coarse(self):
        n = int(self.sizes()[5])
        pos, flag, prev = np.zeros((n, 3), f32), np.zeros(n, np.int32), np.zeros((n, 3), f32)
        self.call("rec_get_coarse", P(pos), P(flag), P(prev))
        return pos, flag, prev

    def params(self):
        par, res = np.zeros(9, f32), np.zeros(2, np.int32)
        self.call("rec_get_params", P(par), P(res))
        return par, res


def check_levels(what, lev, flag):
    lev = lev[(flag & 1024) == 0].astype(np.float64)
    lev = lev[np.isfinite(lev)]
    for t in (-0.2, 0.0, 1.0, 1.2):
        d = np.abs(lev - t).min() if lev.size else 1.0
        if d < MARGIN:
            raise SystemExit("refused: %s has a level within %g of the threshold %g -- pick another scene seed" % (what, d, t))


def run_staged(libpath, f, path):
    """frame f stage by stage -> st<f>/... and final/* (compared with call<f>/after by main, not written)"""
    R = Rec(libpath)
    pos, flag, grid, moves = scene()
    out = {}
    R.call("rec_open", RES, P(np.ascontiguousarray(grid)))
    put = lambda pre, st: out.update({pre + "/" + n: v for n, v in st.items()})
    for g in range(f):
        R.call("rec_set_coarse", ctypes.c_int64(len(pos)), P(pos), P(flag))
        R.plugin(SETS[0])
        pos = pos + moves[g]
    R.call("rec_set_coarse", ctypes.c_int64(len(pos)), P(pos), P(flag))
    key = "st%d/" % f
    nb = int(SETS[0][2])
    if f == 0:
        a = list(SETS[0])
        a[2] = 0                                     # initFines alone; nothing fills the surface list
        R.plugin(a)
        count = 6 * nb
    else:
        R.call("rec_stage", b"advect")
        out[key + "advect/pos"] = R.surface()[0]["pos"]
        R.call("rec_stage", b"accel")
        R.call("rec_stage", b"accel_coarse")
        count = nb
    for it in range(count):
        keep = it in (0, 1, count - 1)
        st, lev = R.surface()
        if keep:
            put(key + "%d/start" % it, st)
        for j, name in enumerate(ITER):
            R.call("rec_stage", name.encode())
            if not keep or name == "accel":
                continue
            st, lev = R.surface()
            for k in CHANGED[name]:
                out[key + "%d/%d/%s" % (it, j, k)] = st[k]
            out[key + "%d/%d/sizes" % (it, j)] = st["sizes"]
            if name in ("regularize", "adddelete"):
                check_levels("frame %d iteration %d %s" % (f, it, name), lev, st["flag"])
    if f:
        c = np.zeros(1, f32)
        R.call("rec_costheta", P(c))
        out[key + "costheta"] = c
        R.call("rec_stage", b"waves")
        out[key + "waves/real"] = R.surface()[0]["real"]
    put("final", R.surface()[0])
    np.savez_compressed(path, **out)


def run_loop(libpath, inputs, path, init):
    I = np.load(inputs)
    R = Rec(libpath)
    out = {}
    R.call("rec_open", RES, P(np.ascontiguousarray(I["loop/flags"].reshape(RES, RES, RES).astype(np.int32))))
    for t in range(1 if init else 3):
        pos, flag, prev = (np.ascontiguousarray(I["loop/%d/coarse_%s" % (t, k)]) for k in ("pos", "flag", "prev"))
        R.call("rec_set_coarse", ctypes.c_int64(len(pos)), P(pos), P(flag))
        R.call("rec_set_prev", P(prev))
        a = list(LOOP_ARGS)
        if init:
            a[2] = 0
        R.plugin(a)
        st, lev = R.surface()
        if init:
            out["loop/init_pos"] = st["pos"]
            break
        check_levels("loop frame %d" % t, lev, st["flag"])
        out["loop/%d/after/flag" % t], out["loop/%d/after/sizes" % t] = st["flag"], st["sizes"]
        print("loop", t, st["sizes"])
    np.savez_compressed(path, **out)


def run_set(libpath, k, path):
    R = Rec(libpath)
    pos, flag, grid, moves = scene()
    out = {}
    R.call("rec_open", RES, P(np.ascontiguousarray(grid)))
    key = "set%d/" % k
    out[key + "args"] = np.array(SETS[k], np.float64)
    if k > 0:
        a = list(SETS[k])
        a[2] = 0                                     # nb = 0: initFines alone
        R.call("rec_set_coarse", ctypes.c_int64(len(pos)), P(pos), P(flag))
        R.plugin(a)
        out[key + "par"], out[key + "res"] = R.params()
        out[key + "init_pos"] = R.surface()[0]["pos"]
        np.savez_compressed(path, **out)
        return
    out["flags"] = grid
    out["seed"] = np.array([SEED])
    put = lambda pre, st: out.update({pre + "/" + n: v for n, v in st.items()})
    for f in range(3):
        R.call("rec_set_coarse", ctypes.c_int64(len(pos)), P(pos), P(flag))
        cp, cf, prev = R.coarse()
        out["call%d/coarse_pos" % f], out["call%d/coarse_flag" % f], out["call%d/coarse_prev" % f] = cp, cf, prev
        st, _ = R.surface()
        put("call%d/before" % f, st)
        R.plugin(SETS[0])
        st, lev = R.surface()
        put("call%d/after" % f, st)
        check_levels("call %d" % f, lev, st["flag"])
        d = np.zeros((int(st["sizes"][3]), 3), f32)
        R.call("rec_get_displaced", P(d))
        out["call%d/displaced" % f] = d
        if f == 0:
            out[key + "par"], out[key + "res"] = R.params()
        print("call", f, "sizes", st["sizes"], "deleted", int(((st["flag"] & 1024) != 0).sum()))
        pos = pos + moves[f]
    # single stages on the state the last call left; the coarse particles stay where the call saw them
    _, _, prev = R.coarse()
    out["chain/coarse_prev"] = prev
    st, lev = R.surface()
    put("chain/start", st)
    check_levels("chain start", lev, st["flag"])
    names = list(CHAIN)
    for i, name in enumerate(names):
        R.call("rec_stage", name.encode())
        st, lev = R.surface()
        put("chain/%d" % i, st)
        if name in ("regularize", "adddelete"):
            check_levels("chain %d" % i, lev, st["flag"])
        print("chain", i, name, st["sizes"][:3])
    c = np.zeros(1, f32)
    R.call("rec_costheta", P(c))
    out["chain/costheta"] = c
    R.call("rec_set_coarse", ctypes.c_int64(len(pos)), P(pos), P(flag))
    out["chain/coarse2_pos"] = pos
    R.call("rec_stage", b"advect")
    st, _ = R.surface()
    put("chain/%d" % len(names), st)
    names.append("advect")
    out["chain/names"] = np.array([n.encode() for n in names])
    np.savez_compressed(path, **out)


def check_signs(out):
    """the numpy model on every recorded stage: refuses where a decision downstream of expf / logf within the stage is undecided"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import surfturb_model as M
    worst = {}
    for what, name, c, _ in M.stage_cases(out) + [("chain %d" % i, n, M.chain_case(out, i), None) for i, n in enumerate(M.chain_names(out))]:
        if name == "accel":
            continue
        mdl = M.Model(M.par_of(out, 0, c["frame"]), c["R"], c, listed=c.get("listed"))
        mdl.run(name)
        for k, (v, bound) in mdl.margins.items():
            if v < bound:
                raise SystemExit("refused: %s %s: %s is %g, undecided within %g -- pick another scene seed" % (what, name, k, v, bound))
            worst[k] = min(worst.get(k, (np.inf, 0)), (v / bound, v))
    print("smallest margins of the sign tests (multiple of the bound, value):", worst)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--set":
        return run_set(sys.argv[3], int(sys.argv[2]), sys.argv[4])
    if len(sys.argv) > 2 and sys.argv[1] in ("--loop", "--loop-init"):
        return run_loop(sys.argv[3], sys.argv[2], sys.argv[4], sys.argv[1] == "--loop-init")
    if len(sys.argv) > 2 and sys.argv[1] == "--staged":
        return run_staged(sys.argv[3], int(sys.argv[2]), sys.argv[4])
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    ref = sys.argv[1]
    libpath = build(ref)
    out = {}
    for k in range(len(SETS)):
        part = os.path.join(B, "set%d.npz" % k)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--set", str(k), libpath, part])
        out.update(np.load(part))
    for f in range(3):
        part = os.path.join(B, "staged%d.npz" % f)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--staged", str(f), libpath, part])
        st = dict(np.load(part))
        for k in ("pos", "flag", "normals", "real"):     # the staged run is the whole call
            a, b = st.pop("final/" + k), out["call%d/after/%s" % (f, k)]
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), ("the staged frame %d does not end where the whole call does" % f, k)
        assert st.pop("final/sizes")[:3].tolist() == out["call%d/after/sizes" % f][:3].tolist()
        out.update(st)
    check_signs(out)
    path = os.path.join(ROOT, "tests", "golden", "surfturb.npz")
    inputs = sys.argv[2] if len(sys.argv) > 2 else path
    I = np.load(inputs)
    out.update({k: I[k] for k in I.files if k == "loop/flags" or (k.startswith("loop/") and "/coarse_" in k)})
    for mode in ("--loop", "--loop-init"):
        part = os.path.join(B, "loop%s.npz" % mode[6:])
        subprocess.check_call([sys.executable, os.path.abspath(__file__), mode, inputs, libpath, part])
        out.update(np.load(part))
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), size))
    assert size < 1 << 20


if __name__ == "__main__":
    main()

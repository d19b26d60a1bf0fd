"""Driver of tools/fields_host_check.hip (its header has the build line): every kernel body of mantaflow_amd/csrc/fields_cells.h on
the host, serially, under the host sanitizers, on the inputs of tests/fields_model.py; every output must equal the model bit for bit
and the program must end clean.  Usage: python tools/fields_host_check.py <program>."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fields_model as M  # noqa: E402

f32 = np.float32


def soa(g):
    return np.ascontiguousarray(np.asarray(g).reshape(-1, 3).T)


def aos(a, shape):
    return np.ascontiguousarray(a.reshape(3, -1).T.reshape(shape + (3,)))


def run(prog, tmp, op, dims, arrays, *numbers):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([prog, op] + [str(v) for v in dims] + [fin, fout] + [repr(float(v)) if isinstance(v, (float, np.floating)) else str(int(v)) for v in numbers],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (op, dims, r.returncode, r.stderr[-2000:])
    return np.fromfile(fout, np.uint32)


def same(tag, got_words, want):
    w = np.ascontiguousarray(want).view(np.uint32).ravel()
    assert got_words.size == w.size and (got_words == w).all(), tag


def main(prog):
    n = 0
    with tempfile.TemporaryDirectory() as tmp:
        for case, (name, absent, par) in M.FIRE_CASES.items():
            dims = M.DIMS[name]
            g = M.fire_inputs(name)
            given = [k for k in M.OPTIONAL if k not in absent]
            present = sum(1 << q for q, k in enumerate(M.OPTIONAL) if k not in absent)
            keys = ["fuel", "density", "react"] + given
            out = run(prog, tmp, "burn", dims, [g[k] for k in keys], present, f32(par["burningRate"]), f32(par["flameSmoke"]), f32(par["ignitionTemp"]),
                      f32(par["maxTemp"]), f32(M.FIRE_DT), *[f32(c) for c in par["color"]])
            model, mflame = M.run_fire(case)
            same("burn " + case, out, np.concatenate([model[k].ravel() for k in keys]))
            same("flame " + case, run(prog, tmp, "flame", dims, [model["react"], M.prefill(name, "flame")]), mflame)
            n += 2
        for name in M.ALL:
            dims = M.DIMS[name]
            v = M.secderiv_input(name)
            same("secderiv " + name, run(prog, tmp, "secderiv", dims, [v, M.prefill(name, "curv")]), M.sec_deriv_2d(v, M.prefill(name, "curv")))
            for cn in (0, 1):
                I = M.wave_inputs(name)
                A = M.make_laplace_matrix(I["flags"])
                model = M.run_wave_system(name, bool(cn))
                out = run(prog, tmp, "wave", dims, list(A) + [I["ut"], I["utm1"]], M.wave_s(M.WAVE_DT, M.WAVE_CSQR), cn)
                same("wave %s %d" % (name, cn), out, np.concatenate([model[k].ravel() for k in ("A0", "Ai", "Aj", "Ak", "rhs")]))
                n += 1
            n += 1
        for case, (name, kind, vtype, dist, ff, ft) in M.EXTRAP_CASES.items():
            flags, val, dist, ff, ft = M.extrap_inputs(case)
            model = M.run_extrap(case)
            vec = vtype == "vec"
            out = run(prog, tmp, "extrap", M.DIMS[name], [flags, soa(val) if vec else val], 3 if vec else 1, int(vtype in ("int", "flag")), dist, ff, ft)
            same("extrap " + case, out, soa(model) if vec else model)
            n += 1
    print("fields_host_check: %d runs equal the model bit for bit, no sanitizer report" % n)


if __name__ == "__main__":
    main(sys.argv[1])

"""Driver of tools/meshsdf_host_check.hip (its header has the build line): the bodies of mantaflow_amd/csrc/meshsdf_cells.h on the host,
serially, under the host sanitizers, on every case of tests/meshsdf_model.py and on its synthetic flood-fill fields.  Sources, binning and
the flooded field must equal the model bit for bit; the pre-flood field may differ from the model in at most one written cell per case,
within the model's bound (the C library's fp64 exp against numpy's); the tile rounds must be the model's.  The program must end clean.
Usage: python tools/meshsdf_host_check.py <program>."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meshsdf_model as M  # noqa: E402

f32 = np.float32


def run(prog, tmp, dims, pos, tris, mult, sigma, cutoff, phi=None):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        np.array(list(dims) + [pos.shape[0], tris.shape[0], 0 if phi is None else 1], np.int32).tofile(f)
        np.array(list(mult) + [sigma, cutoff], f32).tofile(f)
        np.ascontiguousarray(pos.T).astype(f32).tofile(f)
        np.ascontiguousarray(tris.T).astype(np.int32).tofile(f)
        if phi is not None:
            phi.astype(f32).tofile(f)
    r = subprocess.run([prog, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(fout, "rb").read()
    return np.frombuffer(raw, np.int64, 3), np.frombuffer(raw, np.uint32, offset=24)


def same(tag, a, b):
    a, b = np.ascontiguousarray(a).view(np.uint32).reshape(-1), np.ascontiguousarray(b).view(np.uint32).reshape(-1)
    assert a.shape == b.shape and (a == b).all(), "%s: %d words differ" % (tag, int((a != b).sum()) if a.shape == b.shape else -1)


def main(prog):
    ndiff = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in M.CASES:
            c, R = M.case(name), M.model(name)
            n = int(np.prod(c["dims"]))
            mult = np.array(c["dims"], f32) / np.array(c["mesh_gs"], f32)
            counts, w = run(prog, tmp, c["dims"], c["pos"], c["tris"], mult, c["sigma"], c["cutoff"])
            ns, B = int(counts[0]), R["bin"]
            assert (ns, int(counts[1])) == (R["spos"].shape[0], B["binned"]), (name, counts)
            assert w.size == 12 * ns + 4 * n, name
            same(name + "/spos", w[:3 * ns].reshape(3, ns).T, R["spos"])
            same(name + "/snrm", w[3 * ns:6 * ns].reshape(3, ns).T, R["snrm"])
            o = 6 * ns
            same(name + "/len", w[o:o + n], B["len"])
            same(name + "/start", w[o + n:o + 2 * n], B["start"])
            o += 2 * n
            nb = B["binned"]
            same(name + "/bpos", w[o:o + 3 * ns].reshape(3, ns)[:, :nb].T, B["bpos"])
            same(name + "/bnrm", w[o + 3 * ns:o + 6 * ns].reshape(3, ns)[:, :nb].T, B["bnrm"])
            o += 6 * ns
            pre, phi = w[o:o + n].view(f32), w[o + n:o + 2 * n].view(f32)
            d = np.nonzero(pre.view(np.uint32) != R["pre"].view(np.uint32))[0]
            assert d.size <= 1 and (np.abs(pre[d].astype(np.float64) - R["pre"][d]) <= M.bound(R["C"], R["pre"])[d]).all(), (name, d)
            ndiff += d.size
            if d.size == 0:
                same(name + "/phi", phi, R["phi"])
            assert int(counts[2]) == M.tile_rounds(R["pre"], c["dims"], R["P"]["cutoff"])[1] or d.size, (name, counts)
        fields = ["snake", "corner"] + ["rand%d" % q for q in range(200)]
        for name in fields:
            dims, v, cutoff = M.flood_field(name)
            counts, w = run(prog, tmp, dims, np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), (1, 1, 1), 1.0, cutoff, v)
            same("flood/" + name, w.view(f32), M.flood_closure(v, dims, cutoff)[0])
            assert int(counts[2]) == M.tile_rounds(v, dims, cutoff)[1], (name, counts)
    print("meshsdf_host_check: %d cases and %d flood fields equal the model (%d pre-flood cells differ within the bound), no sanitizer report"
          % (len(M.CASES), len(fields), ndiff))


if __name__ == "__main__":
    main(sys.argv[1])

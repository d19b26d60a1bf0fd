"""Driver of tools/vsheet_host_check.hip (its header has the build line): runs the stand-alone host program on the cases of
tests/vsheet_model.py and compares each output with the numpy model, and where the fixture has the stage with the recorded reference,
bit for bit.  The program is a separate process; nothing is loaded into this one.

    python tools/vsheet_host_check.py <path to vsheet_host_check>
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_model as MM  # noqa: E402
import meshops_model as MO  # noqa: E402
import vsheet_model as M  # noqa: E402

f32, i32 = np.float32, np.int32


def planes(a):
    return np.ascontiguousarray(np.asarray(a, f32).T).tobytes()


def run(exe, mode, m, extra, *args):
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(a, "wb") as f:
            f.write(np.array([m["pos"].shape[0], m["tris"].shape[0]], np.int64).tobytes())
            f.write(planes(m["pos"]) + m["flags"].astype(i32).tobytes() + np.ascontiguousarray(m["tris"].T.astype(i32)).tobytes())
            f.write(b"".join(extra))
        r = subprocess.run([exe, mode, a, b] + [repr(float(x)) if isinstance(x, (float, f32)) else str(x) for x in args], capture_output=True, text=True)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-2000:])
        return np.frombuffer(open(b, "rb").read(), np.uint8)


def same(tag, raw, want):
    want = np.ascontiguousarray(want)
    assert raw.tobytes() == want.tobytes(), tag


def main(exe):
    G = M.golden()
    for name in list(M.MESHES) + list(M.OPEN_MESHES):
        is_open = name in M.OPEN_MESHES
        m = (M.OPEN_MESHES[name]() if is_open else M.with_fixed(M.MESHES[name](), name))
        t = m["tris"].shape[0]
        st = M.sheet_state(name, t)
        raw = run(exe, "geometry", m, [])
        want = planes(M.face_center(m)) + M.face_area(m).tobytes() + planes(M.face_normal(m)) + M.tri_fixed(m).astype(i32).tobytes()
        assert raw.tobytes() == want, name
        raw = run(exe, "calc", m, [planes(st["circulation"])])
        same(name, raw, M.calc_vorticity(m, st["circulation"])[0].T)
        if not is_open:
            same(name, raw, G["calc/%s/vorticity" % name].T)
        vel, old = M.mac_grid("src-" + name), M.mac_grid("src-old-" + name)
        for vname, (with_vel, maxAmount, mult, scale) in M.SOURCE_VARIANTS.items():
            a = np.zeros((t, 3), f32)
            if with_vel:
                a = MM.interpol_mac(M.DIMS, M.acceleration(vel, old, M.DT), np.ascontiguousarray(M.face_center(m).T)).T
            raw = run(exe, "source", m, [planes(st["vorticity"]), planes(a)], int(with_vel), *[f32(x) for x in M.GRAVITY + (scale, maxAmount, mult, M.DT,
                                                                                                                        1.0 / max(M.DIMS))])
            w, v = M.vorticity_source(m, st["vorticity"], M.GRAVITY, M.DIMS, M.DT, vel if with_vel else None, old if with_vel else None, scale, maxAmount,
                                      mult)
            assert raw.tobytes() == planes(w) + v.tobytes(), (name, vname)
            if not is_open:
                same((name, vname), raw[:12 * t], G["source/%s/%s" % (name, vname)].T)
        m0 = (M.OPEN_MESHES if is_open else M.MESHES)[name]()
        opp = MO.corners(m0["tris"])[0]
        st0 = M.sheet_state(name, t)
        for sigma in M.SMOOTH_SIGMAS:
            key = "smooth/%s/%g" % (name, sigma)
            raw = run(exe, "weights", m0, [opp.astype(i32).tobytes()], M.smooth_mult(sigma))
            w, idx = np.frombuffer(raw[:12 * t].tobytes(), f32), np.frombuffer(raw[12 * t:].tobytes(), i32)
            assert np.array_equal(idx, G[key + "/index"]), key
            assert M.ulps_apart(w, G[key + "/weights"]).max(initial=0) <= M.WEIGHT_ULPS, key
            wm = M.smooth_weights(m0, opp, sigma)[0]
            assert (M.ulps_apart(w, wm) != 0).sum() <= 1, key
            for it in M.SMOOTH_ITERS:
                raw = run(exe, "passes", m0, [G[key + "/weights"].tobytes(), G[key + "/index"].tobytes(), planes(st0["vorticity"])], it, f32(M.ALPHA))
                same((key, it), raw, G["%s/out%d" % (key, it)].T)
        print("%s: %d triangles equal the model and the reference" % (name, t))
    for name, (dims, sigma, T, rev) in M.vic_cases().items():
        if dims[0] > 20 and sigma != 1.5:
            continue
        m, vorticity = M.vic_soup(dims, T, 1, rev)
        flags = M.vic_flags(dims)
        raw = run(exe, "spread", m, [planes(vorticity), flags.tobytes()], dims[0], dims[1], dims[2], f32(sigma))
        want, wnorm = M.spread(m, vorticity, flags, dims, sigma)
        assert raw.tobytes() == wnorm.tobytes() + planes(want), name
        print("%s: the spreading equals the model" % name)


if __name__ == "__main__":
    main(sys.argv[1])

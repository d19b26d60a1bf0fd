"""scenes/flip03_gen.py -- particles in, `fluidsurface_final_%04d.bobj.gz` out -- run through `from manta import *` with `out` pointed
at a temporary directory, fed a particle file and a reference `.uni` grid written by the package, its `.vdb` line taken out and its
frame range cut to one frame (edits applied to the text read from the reference checkout at test time; nothing is copied).

On the CPU checker backend the level set is the union one (method 0: the smooth particle level sets are not part of that backend),
createMesh is accepted and ignored, and the scene writes a valid empty mesh file.  (The device path of the same calls -- createMesh, then
save -- is held against the reference's bytes in tests/test_gpu_mesh.py.)"""
import gzip
import os
import struct

import numpy as np
import pytest

from test_scenes_run import SCENES, run_scene

pytestmark = pytest.mark.skipif(not os.path.isdir(SCENES), reason="reference scenes not present on this machine")
RES = 12


def _inputs(m, out):
    """what flip02_surface.py (saveParts) leaves behind: a grid file for the resolution and the particles of frame 1"""
    s = m.Solver(name="src", gridSize=m.vec3(RES, RES, RES), dim=3)
    s.create(m.RealGrid).save(os.path.join(out, "ref_parts_0000.uni"))
    pp = s.create(m.BasicParticleSystem)
    r = np.random.RandomState(5)
    pos = np.stack([r.uniform(1.5, 0.45 * RES, 4000), r.uniform(1.5, 0.6 * RES, 4000), r.uniform(1.5, RES - 1.5, 4000)], 1).astype(np.float32)
    pp.set_positions(pos)
    pp.save(os.path.join(out, "parts_0001.uni"))
    assert m.getUniFileSize(os.path.join(out, "ref_parts_0000.uni")) == m.vec3(RES, RES, RES)
    assert m.getUniFileSize(os.path.join(out, "absent.uni")) == m.vec3(0, 0, 0)
    return pos


def _run(out, method):
    subst = [("out = r'c:/prj-external-libs/mantaflow/out/'", "out = %r" % (out + os.sep)), ("endFrame   = 1000", "endFrame   = 2"),
             ("            save( name=out + 'fluid_data_%04d.vdb' % outCnt, objects=objects )", "            pass")]
    if method != 2:
        subst.append(("method = 2", "method = %d" % method))
    return run_scene("flip03_gen.py", None, subst)


def _bobj(path):
    raw = gzip.open(path).read()
    n = struct.unpack_from("<i", raw, 0)[0]
    n2 = struct.unpack_from("<i", raw, 4 + 12 * n)[0]
    t = struct.unpack_from("<i", raw, 8 + 24 * n)[0]
    assert n2 == n and len(raw) == 12 + 24 * n + 12 * t
    return n, t, raw


def test_flip03_gen_on_the_cpu_backend_writes_a_valid_empty_mesh(oracle_backend, tmp_path):
    import manta as m
    out = str(tmp_path)
    pos = _inputs(m, out)
    g = _run(out, 0)
    assert g["s"].getGridSize() == m.vec3(2 * RES, 2 * RES, 2 * RES) and g["outCnt"] == 1
    assert g["pp"].pySize() == pos.shape[0]
    assert np.array_equal(g["pp"].get_positions(), pos * np.float32(2))          # transformPositions: upres 2
    phi = g["phi"].to_numpy()
    assert (phi < 0).sum() > 1000                                               # the level set was built; createMesh was reached
    assert _bobj(os.path.join(out, "fluidsurface_final_0000.bobj.gz"))[:2] == (0, 0)
    assert g["mesh"].numNodes() == 0

"""CPU: the public face of the mesh operations without a GPU -- smoothMesh, killSmallComponents, Mesh.corners_numpy / ring_numpy and
lastMeshOpsStats with the reference's signatures, the row of the open extension table with its header and version macro, entry names
disjoint from every other extension, the host entry of the built library against the model, and the refusals by name (the CPU checker
backend, a z-slab solver, a wrong argument) with the mesh and its topology generation left as they were.  The kernels run in
tests/test_gpu_meshops.py."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

import meshops_model as M
import util

GOLDEN = np.load(M.GOLDEN)
f32 = np.float32


def _mesh(m, model):
    s = m.Solver(name="o", gridSize=m.vec3(8, 8, 8), dim=3)
    mesh = s.create(m.Mesh)
    mesh.set_numpy(model["pos"], model["normal"], model["flags"], model["tris"], model["tflags"])
    return s, mesh


def _state(mesh):
    return [a.tobytes() for a in mesh.nodes_numpy() + mesh.tris_numpy()] + [mesh._topo_gen, mesh._conn]


def test_names_and_signatures():
    import manta as m
    assert str(inspect.signature(m.smoothMesh)) == "(mesh, strength, steps=1, minLength=1e-05)"
    assert str(inspect.signature(m.killSmallComponents)) == "(mesh, elements=10)"
    assert str(inspect.signature(m.Mesh.corners_numpy)) == "(self)" and str(inspect.signature(m.Mesh.ring_numpy)) == "(self)"
    assert str(inspect.signature(m.lastMeshOpsStats)) == "()" and isinstance(m.lastMeshOpsStats(), dict)


def test_row_of_the_open_table_and_header():
    from mantaflow_amd import _lib
    e = _lib.extension("meshops")
    assert e in _lib.OPEN_EXTENSIONS and (e.what, e.verb) == ("mesh connectivity, smoothing and component removal", "do")
    inc = os.path.dirname(_lib.HEADER)
    assert e.header == os.path.join(inc, "open", "manta_hip_meshops.h") == _lib.MESHOPS_HEADER and os.path.exists(e.header)
    assert {x.header for x in _lib.OPEN_EXTENSIONS} == set(glob.glob(os.path.join(inc, "open", "manta_hip_*.h")))
    assert (e.version_fn, e.version_macro) == ("mf_meshops_abi_version", "MF_MESHOPS_ABI_VERSION")
    assert re.search(r"^#define\s+MF_MESHOPS_ABI_VERSION\s+\d+\s*$", open(e.header).read(), flags=re.M)
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []
    assert e in _lib.all_extensions()


def test_entry_names_are_disjoint_from_every_other_header():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.all_extensions():
        if e.name != "meshops":
            for n in _lib.parse_header(e.header):
                seen[n] = os.path.basename(e.header)
    mine = _lib.parse_header(_lib.MESHOPS_HEADER)
    assert len(mine) == 10 and all(n.startswith("mf_meshops_") for n in mine)
    for n in mine:
        assert n not in seen, "%s is declared by %s as well" % (n, seen.get(n))
    # the mesh header and its revision stay as they were
    assert len(_lib.parse_header(_lib.MESH_HEADER)) == 9 and re.search(r"#define\s+MF_MESH_ABI_VERSION\s+1\s", open(_lib.MESH_HEADER).read())


@pytest.mark.skipif(not os.path.exists(util.HIP_LIB), reason="libmanta_hip.so not built")
def test_product_library_exports_the_extension_and_its_host_entries_answer():
    from mantaflow_amd import _lib
    L = ctypes.CDLL(util.HIP_LIB)          # loads without a GPU; only the host entries are called
    for n in _lib.parse_header(_lib.MESHOPS_HEADER):
        assert hasattr(L, n), n
    want = int(re.search(r"#define\s+MF_MESHOPS_ABI_VERSION\s+(\d+)", open(_lib.MESHOPS_HEADER).read()).group(1))
    assert L.mf_meshops_abi_version() == want
    L.mf_meshops_rescale_scalars.argtypes = [ctypes.c_void_p] * 3
    cases = [GOLDEN["smooth/%s/sums" % name] for name in sorted(M.SMOOTH_CASES)]
    cases += [np.array([[1.5, 1, 2, 3], [0.0, 4, 5, 6]]), np.array([[0.0, 1, 2, 3], [0.0, 4, 5, 6]]), np.array([[-2.0, 1, 2, 3], [3.0, 4, 5, 6]])]
    for sums in cases:
        out = np.full(7, 9, f32)
        assert L.mf_meshops_rescale_scalars(sums[0].ctypes.data_as(ctypes.c_void_p), sums[1].ctypes.data_as(ctypes.c_void_p),
                                            out.ctypes.data_as(ctypes.c_void_p)) == 0
        o, n, beta = M.rescale_scalars(sums[0], sums[1])
        assert out.tobytes() == np.concatenate([o, n, [beta]]).astype(f32).tobytes(), sums       # inf and nan included, by bits
    need = ctypes.c_int64(0)
    L.mf_meshops_tmp_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    assert L.mf_meshops_tmp_bytes(1000, 502, ctypes.byref(need)) == 0 and need.value >= 4 * 4 * 6000
    assert L.mf_meshops_tmp_bytes(-1, 5, ctypes.byref(need)) != 0


def test_refusals_on_the_checker_backend_leave_the_mesh_as_it_was(oracle_backend):
    import manta as m
    s, mesh = _mesh(m, M.KILL_CASES["plus1"]()[0])
    before = _state(mesh)
    tail = ": the 'oracle' backend does not implement mesh connectivity, smoothing and component removal (manta_hip_meshops.h)"
    for who, call in (("smoothMesh", lambda: m.smoothMesh(mesh, 0.5)), ("killSmallComponents", lambda: m.killSmallComponents(mesh, 5)),
                      ("Mesh::corners_numpy", mesh.corners_numpy), ("Mesh::ring_numpy", mesh.ring_numpy)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == who + tail
    s._slab_window = (2, 8)
    try:
        for who, call in (("smoothMesh", lambda: m.smoothMesh(mesh, 0.5)), ("killSmallComponents", lambda: m.killSmallComponents(mesh))):
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value) == who + ": mesh connectivity, smoothing and component removal do not run on a z-slab solver"
    finally:
        s._slab_window = (0, 0)
    for call in (lambda: m.smoothMesh(s.create(m.FlagGrid), 0.5), lambda: m.killSmallComponents(3), lambda: m.smoothMesh(None, 1.0)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "can't convert argument to Mesh*"
    with pytest.raises(RuntimeError, match="argument is not an int"):
        m.killSmallComponents(mesh, 2.5)
    with pytest.raises(RuntimeError, match="argument is not an int"):
        m.smoothMesh(mesh, 0.5, steps="3")
    assert _state(mesh) == before


def test_topology_generation_moves_with_the_triangle_list_only(oracle_backend, tmp_path):
    import manta as m
    model = M.bipyramid(5)
    s, mesh = _mesh(m, model)
    g = mesh._topo_gen
    mesh.scale(m.vec3(2, 2, 2)); mesh.offset(m.vec3(1, 0, 0)); mesh.rotate(m.vec3(0.1, 0, 0)); mesh.save_pos(); mesh.load_pos()
    mesh.save(str(tmp_path / "a.bobj.gz"))
    assert mesh._topo_gen == g
    mesh.load(str(tmp_path / "a.bobj.gz"))
    assert mesh._topo_gen > g
    g = mesh._topo_gen
    mesh.set_numpy(model["pos"], tris=model["tris"])
    assert mesh._topo_gen > g
    g = mesh._topo_gen
    mesh.clear()
    assert mesh._topo_gen > g

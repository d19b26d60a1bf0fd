"""CPU: the numpy model of the surface-mesh extension (tests/mesh_model.py) against the recorded reference (tests/golden/mesh.npz; how
each array was produced: tools/record_mesh.py).  createMesh is held twice: the order-free owner / rank statement the kernels implement,
bit for bit against the reference on every fixture case -- all 256 sign configurations of a cell, which pins every entry of the
triangle table -- and against the literal serial sweep of levelset.cpp:343-408 on the small cases and on 1000 random small grids.  The
conditions each case exists for are asserted from the model's counters."""
import os
import re

import numpy as np
import pytest

import mesh_model as M

GOLDEN = np.load(M.GOLDEN)
f32 = np.float32


def _same_mesh(tag, a, b):
    for k in ("pos", "normal", "tris"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)


def test_all_256_sign_configurations_equal_the_reference():
    """cell (0, 0, 0) of a 3x3x3 grid takes every sign pattern; its seven neighbours share its edges.  A wrong table entry shows up
    here with its configuration number."""
    for c in range(256):
        name = "cfg%03d" % c
        mesh = M.model_mesh(name)[0]
        ref_tris = GOLDEN["create/%s/tris" % name]
        assert mesh["tris"].shape == ref_tris.shape and np.array_equal(mesh["tris"], ref_tris), \
            "configuration %d (table entry %r): triangles %s, the reference's %s" % (c, M.TRI_WORDS.split()[c], mesh["tris"].tolist(), ref_tris.tolist())
        msg = M.mesh_same_as_fixture(GOLDEN, "create/" + name, mesh)
        assert msg is None, msg


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_create_mesh_equals_the_reference(name):
    mesh, _ = M.model_mesh(name)
    msg = M.mesh_same_as_fixture(GOLDEN, "create/" + name, mesh)
    assert msg is None, msg


@pytest.mark.parametrize("name", M.SERIAL_CASES + ("sphere",))
def test_serial_sweep_equals_the_order_free_statement(name):
    _same_mesh(name, M.create_mesh_serial(M.case_phi(name)), M.model_mesh(name)[0])


def test_serial_sweep_equals_the_order_free_statement_on_1000_random_grids():
    r = np.random.RandomState(20240607)
    active = passed = 0
    for q in range(1000):
        sx, sy, sz = r.randint(3, 6, 3)
        phi = r.uniform(-1, 1, (sz, sy, sx)).astype(f32)
        if q % 3 == 0:                                   # invalid-time corners: ownership passes to later cells
            phi[r.uniform(size=phi.shape) < 0.1] = M.INVALID
        if q % 5 == 0:
            phi[r.uniform(size=phi.shape) < 0.1] = -M.ISO
        cnt = {}
        a, b = M.create_mesh_serial(phi), M.create_mesh(phi, cnt)
        _same_mesh("grid %d %s" % (q, (sx, sy, sz)), a, b)
        active += b["tris"].shape[0]
        passed += cnt["owner_passed"]
    assert active > 10000 and passed > 100


def test_case_conditions_from_the_counters():
    cnt = {name: M.model_mesh(name)[1] for name in M.CASES}
    # cells with phi <= -1000 that would have owned an edge: a later cell owns it, with its own orientation and mu
    assert cnt["invalid"]["owner_passed"] > 0 and cnt["rand33"]["owner_passed"] > 0
    phi = M.case_phi("invalid")
    whole = phi.copy()
    whole[phi <= M.INVALID] = 0.5
    w = M.create_mesh(whole)
    assert w["pos"].shape[0] > M.model_mesh("invalid")[0]["pos"].shape[0]
    assert cnt["iso"]["iso_exact"] > 0                                   # phi == -1e-4f exactly at a corner
    assert cnt["altx"] == {"owner_passed": 0, "norm_zero": 60}            # every gradient is zero
    assert (M.model_mesh("altx")[0]["normal"] == 0).all()
    assert cnt["planex"].get("norm_one", 0) > 0 and cnt["noise"].get("norm_scaled", 0) > 0
    for name in ("pos", "neg"):
        m = M.model_mesh(name)[0]
        assert m["pos"].shape == (0, 3) and m["tris"].shape == (0, 3)
    assert M.model_mesh("sphere")[0]["tris"].shape[0] > 2000


def test_invalid_cell_changes_owner_orientation_and_mu():
    """one edge, two sharing cells: with the first cell invalid the second owns the edge and runs it the other way round"""
    phi = np.full((3, 3, 3), 0.5, f32)
    phi[1, 1, 1] = -0.5
    full = M.create_mesh(phi)
    assert full["pos"].shape[0] == 6 and full["tris"].shape[0] == 8
    phi2 = phi.copy()
    phi2[0, 0, 0] = M.INVALID                     # cell (0, 0, 0) drops out; its three edges at (1, 1, 1) pass to later cells
    cnt = {}
    part = M.create_mesh(phi2, cnt)
    assert cnt["owner_passed"] == 3 and part["pos"].shape[0] == 6 and part["tris"].shape[0] == 7
    _same_mesh("serial", M.create_mesh_serial(phi2), part)
    # the same six points (mu and 1 - mu of the reversed edge round differently at most in the last bit), in another order
    a = full["pos"][np.lexsort(np.round(full["pos"], 3).T)]
    b = part["pos"][np.lexsort(np.round(part["pos"], 3).T)]
    assert np.abs(a - b).max() < 1e-6 and not np.array_equal(full["pos"], part["pos"])


def test_2d_grid_raises_and_thin_grids_are_refused():
    with pytest.raises(RuntimeError, match="Only 3D grids supported so far"):
        M.create_mesh(np.zeros((1, 4, 4), f32))
    with pytest.raises(RuntimeError, match="Only 3D grids supported so far"):
        M.create_mesh_serial(np.zeros((1, 4, 4), f32))
    with pytest.raises(AssertionError):
        M.create_mesh(np.zeros((2, 4, 4), f32))


def test_table_in_the_kernel_header_is_the_models_table():
    """mesh_cells.h packs the same table as 64-bit words: nibble q is corner q, 0xf ends the list"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mantaflow_amd", "csrc", "mesh_cells.h")
    text = open(path).read()
    body = text[text.index("TRI_WORDS[256] = {"):]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", body[:body.index("};")])]
    assert len(words) == 256
    for c, w in enumerate(words):
        row = []
        for q in range(16):
            e = (w >> (4 * q)) & 15
            if e == 15:
                break
            row.append(e)
        assert tuple(row) == M.TRI_TABLE[c], c
        assert (w >> (4 * len(row))) == (1 << (64 - 4 * len(row))) - 1, c      # every nibble after the list is 0xf


def test_geometry_tables():
    for e in range(12):
        sh = M.SHARERS[e]
        assert len(sh) == 4 and sum(off == (0, 0, 0) for off, _ in sh) == 1
        assert [(off[2], off[1], off[0]) for off, _ in sh] == sorted((off[2], off[1], off[0]) for off, _ in sh)      # sweep order
        assert dict(sh)[(0, 0, 0)] == e
        before = [off for off, _ in sh[:[o for o, _ in sh].index((0, 0, 0))]]
        assert len(before) <= 3                              # at most three earlier cells decide an owner


@pytest.mark.parametrize("name", M.VNORM_CASES)
def test_vertex_normals(name):
    pos, tris = M.vnorm_inputs(name)
    n = M.vertex_normals(pos, tris)
    msg = M.same_as_fixture(GOLDEN, "vnorm/" + name, n)
    assert msg is None, msg
    if name == "degenerate":
        # what the reference yields: in triangle (1, 1, 3) node 1 gets 0 * (1 / 0) = NaN twice, which normalize() sends to 0, and
        # node 3 gets 0 * a finite weight; (7, 7, 7) gives NaN -> 0 as well; node 6 is only in the collinear triangle: a zero sum
        assert (n[[1, 6, 7]] == 0).all() and not np.isnan(n).any()
        assert (np.abs(np.linalg.norm(n[[0, 2, 3, 4, 5]].astype(np.float64), axis=1) - 1) < 1e-6).all()
    if name == "fan":
        assert abs(np.linalg.norm(n[0].astype(np.float64)) - 1) < 1e-6


@pytest.mark.parametrize("n", M.ADV_SIZES)
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_advect_model_equals_the_reference(n, mode):
    vel, pos, nflags = M.advect_inputs(n)
    got = M.advect_nodes(M.ADV_DIMS, vel, pos, nflags, M.ADV_DT, mode)
    msg = M.same_as_fixture(GOLDEN, "adv/%d/%d" % (n, mode), np.ascontiguousarray(got.T))
    assert msg is None, msg
    fixed = (nflags & M.NF_FIXED) != 0
    assert np.array_equal(got[:, fixed], pos[:, fixed])


def test_transform_models_equal_the_reference():
    pos = M.xf_inputs()
    for key, want in (("scale", pos * np.array(M.XF_SCALE, f32)), ("offset", pos + np.array(M.XF_OFFSET, f32)), ("savepos", pos)):
        msg = M.same_as_fixture(GOLDEN, "xf/" + key, want)
        assert msg is None, msg
    for q, th in enumerate(M.ROT_THETAS):
        sc = GOLDEN["xf/rotate/%d/scalars" % q]
        got = np.ascontiguousarray(M.rotate(np.ascontiguousarray(pos.T), th, sc).T)
        msg = M.same_as_fixture(GOLDEN, "xf/rotate/%d" % q, got)
        assert msg is None, msg
    assert np.array_equal(GOLDEN["xf/rotate/3"], pos)                     # three zero angles: nothing is touched

"""Inputs shared by the z-slab multigrid tests (test_mgslab_model.py, test_gpu_mgslab.py, test_gpu_mgslab_worlds.py): the two
kinds of system, regenerated from tests/mg_cases.py, never stored."""
import functools

import numpy as np

import mg_cases

KINDS = ["lap", "trivial_gf"]
PcMIC, PcMGDynamic, PcMGStatic = 1, 2, 3


@functools.lru_cache(maxsize=None)
def system(kind, dims):
    """-> A (four flat fp32 planes), rhs.  "lap": MakeLaplaceMatrix of the ghost-fluid case's flags (obstacles, an empty top).
    "trivial_gf": the coefficient system of that case (ghost-fluid diagonals: non-integer entries) with a dozen rows made trivial
    the way mf_fix_pressure does it (1 * x = b, no couplings), spread over the planes so that every cut has one nearby."""
    sx, sy, sz = dims
    systems = dict((tag, (A, rhs)) for tag, flags, A, rhs in mg_cases.edge_stage_systems("gf", dims))
    A, rhs = systems["lap" if kind == "lap" else "coef"]
    A = [np.array(a, np.float32).reshape(-1).copy() for a in A]
    rhs = np.array(rhs, np.float32).reshape(-1).copy()
    if kind == "lap":
        return A, rhs
    assert kind == "trivial_gf"
    active = np.nonzero(A[0] != 0)[0]
    assert active.size > 40
    made = 0
    for v in active[::max(active.size // 12, 1)]:
        X, Y, Z = v % sx, (v // sx) % sy, v // (sx * sy)
        A[0][v] = 1
        A[1][v] = A[2][v] = A[3][v] = 0
        if X > 0:
            A[1][v - 1] = 0
        if Y > 0:
            A[2][v - sx] = 0
        if Z > 0:
            A[3][v - sx * sy] = 0
        made += 1
    assert made >= 8
    return A, rhs


def ranges_of(NZ, cuts):
    """cuts: the interior boundaries, increasing -> [(z0, z1)] per rank"""
    edges = [0] + list(cuts) + [NZ]
    assert all(a < b for a, b in zip(edges, edges[1:])), "every rank owns at least one plane"
    return list(zip(edges, edges[1:]))

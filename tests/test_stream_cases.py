"""Without a GPU: the case table of tests/stream_cases.py names every csrc/*.hip file that holds kernels, and its `solve` and
`device_syncs` flags point at lines that still say what they are cited for."""
import glob
import os
import re

import stream_cases as S
import util

CSRC = os.path.join(util.ROOT, "mantaflow_amd", "csrc")
REQUIRED = ["advect", "flip", "p2g_ordered", "surface", "glue", "runtime", "noise", "turbulence", "pressure", "mic", "multigrid", "mg2d", "mgslab",
            "reinit", "resample", "obstacles", "idp", "partls", "guiding", "secparts", "turbulence_model", "fields", "mesh", "meshops", "meshsdf",
            "grid4d", "gridops", "movingobs", "mlflip", "datagen", "vortex", "vsheet", "surfturb"]


def _has_kernels(path):
    """a __global__ in the file itself, or in a *_cells.h / mg_driver.h it includes"""
    text = open(path).read()
    if "__global__" in text:
        return True
    for inc in re.findall(r'#include "(\w+_cells\.h|mg_driver\.h)"', text):
        if "__global__" in open(os.path.join(CSRC, inc)).read():
            return True
    return False


def test_every_file_with_kernels_is_named_by_a_case():
    named = {f for c in S.CASES for f in c.files}
    for f in named | set(S.EXEMPT):
        assert os.path.exists(os.path.join(CSRC, f + ".hip")), "%s.hip does not exist" % f
    with_kernels = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CSRC, "*.hip")) if _has_kernels(p)}
    assert len(with_kernels) > 30
    missing = sorted(with_kernels - named - set(S.EXEMPT))
    assert not missing, "no case of tests/stream_cases.py runs the kernels of: %s" % ", ".join(f + ".hip" for f in missing)
    assert len(S.EXEMPT) <= 2 and all(isinstance(r, str) and r for r in S.EXEMPT.values())
    assert not set(S.EXEMPT) & named
    assert not [f for f in REQUIRED if f not in named]


def test_flags_cite_lines_that_still_hold_the_call():
    seen = 0
    for c in S.CASES:
        for flag in (c.solve, c.device_syncs):
            if flag is None:
                continue
            assert isinstance(flag, S.Flag), c.id
            path = os.path.join(util.ROOT, flag.file)
            assert os.path.exists(path), (c.id, flag)
            lines = open(path).read().split("\n")
            assert 1 <= flag.line <= len(lines) and flag.call in lines[flag.line - 1], (c.id, flag, lines[flag.line - 1] if flag.line <= len(lines) else None)
            seen += 1
    assert seen


def test_at_most_a_quarter_of_the_late_cases_synchronise_the_device():
    late = [c for c in S.CASES if not c.solve]
    assert 4 * len([c for c in late if c.device_syncs]) <= len(late)
    assert any(c.solve for c in S.CASES) and len(late) > 30


def test_ids_are_unique_and_the_span_covers_the_slowest_case():
    assert len(set(S.IDS)) == len(S.CASES)
    assert S.SPAN >= 3 * S.SLOWEST_CASE_SECONDS and S.busy_ops(S.SPAN) * S.BUSY_OP_SECONDS >= S.SPAN

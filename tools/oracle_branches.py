#!/usr/bin/env python3
"""tools/oracle_branches.py -- which branches of the oracle do a set of test inputs leave untaken?

The HIP kernels of the base files restate the oracle's per-cell logic, so a branch the oracle never takes under a set of inputs is
a branch the kernels never take under them either.  This CPU tool builds oracle/manta_oracle.c with `--coverage -O0` (without
OpenMP: the loop bodies then stay in their own functions) into a temporary directory, runs a named set of case builders of
tests/cases.py through the package on that library (in a child process, so that the counters are written when it exits), calls
`gcov -b` and prints, for every oracle function that was called, the source lines that still hold a branch taken zero times.

  python tools/oracle_branches.py                 # both sets
  python tools/oracle_branches.py --set edges

  parity   the inputs of test_gpu_parity.py's test_advect, test_advect_cubic, test_flip_transfers, test_advect_in_grid, test_glue,
           test_flip_glue, test_reset_outflow, test_surface_pieces, test_wavelet_turbulence_pieces
  edges    the inputs of test_gpu_base_edges.py (the edge section of tests/cases.py)

profiles/base_edges_branches.txt is the output of the first command.  It touches neither HIP code nor its assembly."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oracle", "manta_oracle.c")


def run_parity():
    import numpy as np
    import cases
    import util
    big = [(14, 12, 10), cases.SIZE_2D, (33, 17, 9), (16, 12, 10), (40, 17, 12)]
    for dims in big:
        sx, sy, sz = dims
        for kind in (0, 1, 2):
            flags, vel = cases.advect_inputs(dims, 9, vmax=2.5, outflow=(kind == 2))
            field = util.rand_real((sz, sy, sx), 10) if kind == 0 else util.rand_vel(sx, sy, sz, 10)
            for order, cm in ((1, 2), (2, 1), (2, 2)):
                for ot in (1, 2):
                    cases.run_advect_pkg(dims, 0.9, flags, vel, field, kind, order=order, clampMode=cm, orderTrace=ot,
                                         strength=0.8 if order == 2 else 1.0)
            if dims in ((14, 12, 10), cases.SIZE_2D, (40, 17, 12)):
                for order, ot in ((1, 1), (2, 1), (2, 2)):
                    cases.run_advect_pkg(dims, 0.9, flags, vel, field, kind, order=order, clampMode=2, orderTrace=ot, orderSpace=2,
                                         strength=0.8 if order == 2 else 1.0)
    for dims in ((12, 10, 9), cases.SIZE_2D):
        sx, sy, sz = dims
        flags = util.make_flags(sx, sy, sz, 14, empty_top=True)
        vel, velOld = util.rand_vel(sx, sy, sz, 15), util.rand_vel(sx, sy, sz, 16)
        pos, pflag, pvel = util.make_particles(flags, 3, 17)
        ptype = (np.random.default_rng(18).integers(0, 4, pos.shape[1]) * 2).astype(np.int32)
        cases.run_flip_pkg(dims, flags, vel, velOld, pos, pflag, pvel, None, 0)
        cases.run_flip_pkg(dims, flags, vel, velOld, pos, pflag, pvel, ptype, 4)
        flags = util.make_flags(sx, sy, sz, 19, empty_top=True)
        vel = util.smooth_vel(sx, sy, sz, 20, 2.0)
        pos, pflag, _ = util.make_particles(flags, 2, 21)
        for mode in (0, 1, 2):
            for dele, stop in ((False, True), (True, True), (False, False), (True, False)):
                cases.run_advect_parts_pkg(dims, 0.8, flags, vel, pos, pflag, mode, dele, stop)
        flags = util.make_flags(sx, sy, sz, 26, empty_top=True)
        flags[flags.shape[0] // 2, 3, 3] |= util.STICK
        cases.run_glue_pkg(dims, 0.7, flags, util.rand_vel(sx, sy, sz, 27), util.rand_real((sz, sy, sx), 28))
    for dims in ((14, 12, 10), cases.SIZE_2D, (33, 18, 9)):
        fl0, pos, pflag, pvel, vel = cases.flipglue_inputs(dims, 31)
        for ph in (None, util.rand_real((dims[2], dims[1], dims[0]), 35)):
            cases.run_flipglue_pkg(dims, fl0, pos, pflag, pvel, vel, ph)
    for dims in ((14, 12, 10), cases.SIZE_2D):
        cases.run_outflow_pkg(dims, *cases.outflow_inputs(dims, 71))
    for dims in ((14, 12, 10), cases.SIZE_2D, (33, 18, 9), (64, 48, 40)):
        cases.run_surface_pkg(dims, cases.surface_inputs(dims, 51))
    for dims, small in (((20, 14, 12), (10, 7, 6)), ((24, 30, 1), (12, 15, 1)), ((17, 11, 9), (9, 6, 5)), ((64, 48, 40), (32, 24, 20))):
        cases.run_turb_pkg(dims, *cases.turb_inputs(dims, small, 91), small)


def run_edges():
    import cases
    import util
    for dims in cases.EDGE_DIMS:
        I = cases.advect_parts_edge_inputs(dims, 19)
        for mode, dele, stop, skip in cases.ADVECT_PARTS_MODES:
            cases.run_advect_parts_edge(dims, I, mode, dele, stop, skip)
        I = cases.flip_edge_inputs(dims, 14)
        cases.run_flip_pkg(dims, I["flags"], I["vel"], I["velOld"], I["pos"], I["pflag"], I["pvel"], I["ptype"], 4)
        I = cases.surface_edge_inputs(dims, 51)
        cases.run_surface_pkg(dims, I)
        cases.run_project_pkg(dims, I)
        cases.run_markfluid_pkg(dims, cases.markfluid_edge_inputs(dims, 31))
    for dims, small in (((20, 14, 12), (10, 7, 6)), (cases.SIZE_2D, (12, 9, 1)), ((17, 11, 9), (9, 6, 5))):
        I = cases.turb_edge_inputs(dims, small, 91)
        cases.run_turb_edge_pkg(dims, I)
        cases.run_turb_edge_pkg(dims, I, clamp=None)
    for dims in ((14, 12, 10), cases.SIZE_2D):
        sx, sy, sz = dims
        for kind, order, cm, ot, os_ in cases.ADVECT_POISON_CASES:
            flags, vel = cases.advect_inputs(dims, 9, vmax=2.5, outflow=(kind == 2))
            field = util.rand_real((sz, sy, sx), 10) if kind == 0 else util.rand_vel(sx, sy, sz, 10)
            cases.run_advect_poisoned(dims, 0.9, flags, vel, field, kind, order=order, clampMode=cm, orderTrace=ot, orderSpace=os_,
                                      strength=0.8 if order == 2 else 1.0)
        flags, vel, field = cases.outflow_edge_inputs(dims, 9)
        for dt in cases.OUTFLOW_DTS:
            for order in (1, 2):
                cases.run_advect_pkg(dims, dt, flags, vel, field, 2, order=order, strength=0.8 if order == 2 else 1.0)
    for dims in cases.ZMARCH_DIMS:
        sx, sy, sz = dims
        flags, vel = cases.advect_inputs(dims, 9, vmax=2.5)
        for kind in (0, 1):
            field = util.rand_real((sz, sy, sx), 10) if kind == 0 else util.rand_vel(sx, sy, sz, 10)
            for order in (1, 2):
                cases.run_advect_poisoned(dims, 0.9, flags, vel, field, kind, order=order)


SETS = {"parity": run_parity, "edges": run_edges}


def child(name, lib):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mantaflow_amd import _lib
    _lib.use_library(lib, "cpu")
    SETS[name]()
    _lib.reset()


def measure(name):
    """-> {function: [(line number, source text, untaken, branches)]} for the functions called under the set"""
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "libmanta_oracle_cov.so")
        subprocess.check_call(["gcc", "--coverage", "-O0", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                               "-shared", "-o", lib, SRC, "-lm"], cwd=tmp)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", name, "--lib", lib], cwd=tmp)
        gcno = [f for f in os.listdir(tmp) if f.endswith(".gcno")][0]
        subprocess.check_call(["gcov", "-b", "-c", gcno], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(os.path.join(tmp, "manta_oracle.c.gcov"), errors="replace").read().splitlines()
    out, fn, called, cur = {}, None, False, None
    for ln in text:
        m = re.match(r"function (\S+) called (\d+)", ln)
        if m:
            fn, called = m.group(1), int(m.group(2)) > 0
            continue
        m = re.match(r"\s*([\d#=\-]+)\*?:\s*(\d+):(.*)", ln)
        if m:
            cur = [int(m.group(2)), m.group(3).strip(), 0, 0]
            continue
        m = re.match(r"branch\s+\d+ (taken (\d+)|never executed)", ln)
        if m and fn and called and cur:
            cur[3] += 1
            if m.group(2) is None or int(m.group(2)) == 0:
                cur[2] += 1
                rows = out.setdefault(fn, [])
                if not rows or rows[-1] is not cur:
                    rows.append(cur)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--set", choices=sorted(SETS), action="append")
    ap.add_argument("--child")
    ap.add_argument("--lib")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.lib)
    for name in a.set or ["parity", "edges"]:
        res = measure(name)
        print("== set %s: oracle functions called, source lines with a branch that was never taken ==" % name)
        for fn in sorted(res, key=lambda f: res[f][0][0]):
            print("%s" % fn)
            for line, src, untaken, total in res[fn]:
                print("  %5d  [%d of %d untaken]  %s" % (line, untaken, total, src[:150]))
        print()


if __name__ == "__main__":
    main()

"""-m gpu: slab.solvePressure with the multigrid preconditioners through the HIP library, 1, 2 and 3 ranks sharing the one GPU of
the box over gloo (tests/mgslab_worker.py, driven as tests/test_gpu_slab.py drives tests/slab_worker.py), on 20 x 16 x 36 and
24 x 20 x 18, a smoke step and a liquid (phi) step, PcMGDynamic and PcMGStatic.

World 1: pressure and iteration count equal the plugin solvePressure with the same preconditioner, bit for bit; a Static solve
after a flag change reproduces the plugin's count for the stale hierarchy, and releaseMG restores the fresh count.
Worlds 2 and 3: a probe V-cycle equals the world-1 one bit for bit on the owned planes; the solve meets check_against_single of
test_slab_gloo; the iteration count is at most the world-1 count plus one (the preconditioner is bit-identical; only the
rank-order fp64 sums of the dots differ, which can move the stopping test by one step).

Observed iteration counts (world 1 / 2 / 3) are printed by the tests and recorded in DESIGN.md section 30."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import util
from test_slab_gloo import check_against_single

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mgslab_worker.py")
DIMS = ["20x16x36", "24x20x18"]
SCENES = ["smoke", "liquid"]
PCS = ["dynamic", "static"]
STEP_SECONDS = 240          # the limit of one worker run (a run takes a few seconds; the limit only ends a hung one)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_runs = {}


def run_world(tmp_path_factory, world, dims):
    """one worker run per (world, dims), shared by the tests that look at it -> the ranks' files"""
    key = (world, dims)
    if key not in _runs:
        out = str(tmp_path_factory.mktemp("mgslab") / ("w%d" % world))
        env = dict(os.environ, OMP_NUM_THREADS="2")
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable]
        if world > 1:
            cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                    "--master-port", str(_free_port())]
        subprocess.run(cmd + [WORKER, out, dims], check=True, env=env, timeout=STEP_SECONDS + 30)
        _runs[key] = [dict(np.load(out + ".%d.npz" % r)) for r in range(world)]
    return _runs[key]


def as_single(parts, name):
    """the worker's files in the shape check_against_single reads"""
    cat = lambda k, ax: np.concatenate([p[k] for p in parts], axis=ax)
    return dict(dens=cat("dens", 0), vel_adv=cat("vel_adv", 1), vel=cat(name + "__vel", 1), pres=cat(name + "__pres", 0),
                div=cat(name + "__div", 0), iters=[int(p[name + "__iters"]) for p in parts], res=[float(p[name + "__res"]) for p in parts],
                plain_dens=[p["plain_dens"] for p in parts])


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("dims", DIMS)
def test_world_1_equals_the_plugin(tmp_path_factory, dims, scene, pc):
    one = run_world(tmp_path_factory, 1, dims)[0]
    name = "%s_%s" % (scene, pc)
    print("%s %s: slab %d iterations, plugin %d" % (dims, name, int(one[name + "__iters"]), int(one["plugin_" + name + "__iters"])))
    assert int(one[name + "__levels"]) >= 2
    assert str(one[name + "__form"]) == "cut"          # both shapes have more than 8192 vertices: level 0 is above the tail
    assert 0 < int(one[name + "__iters"]) < 100
    assert int(one[name + "__iters"]) == int(one["plugin_" + name + "__iters"])
    util.assert_bitexact(one[name + "__pres"], one["plugin_" + name + "__pres"], "pressure, slab world 1 vs plugin")


@pytest.mark.parametrize("dims", DIMS)
def test_static_keeps_a_stale_hierarchy_until_release(tmp_path_factory, dims):
    one = run_world(tmp_path_factory, 1, dims)[0]
    counts = [int(one[k + "__iters"]) for k in ("seq0", "seq1_stale", "seq2_fresh")]
    plugin = [int(one["plugin_" + k + "__iters"]) for k in ("seq0", "seq1_stale", "seq2_fresh")]
    print("%s Static sequence (fresh, stale, fresh after releaseMG): slab %r, plugin %r" % (dims, counts, plugin))
    assert counts == plugin
    for k in ("seq0", "seq1_stale", "seq2_fresh"):
        util.assert_bitexact(one[k + "__pres"], one["plugin_" + k + "__pres"], k + ": pressure, slab world 1 vs plugin")
    # the stale hierarchy is a different preconditioner from the fresh one of the same system
    assert not np.array_equal(one["seq1_stale__pres"], one["seq2_fresh__pres"])


REPLICATED_DIMS = "16x12x20"      # 3840 vertices: level 0 runs inside the single-workgroup tail, so the V-cycle is not cut


def test_replicated_form_world_1_equals_the_plugin(tmp_path_factory):
    one = run_world(tmp_path_factory, 1, REPLICATED_DIMS)[0]
    for scene in SCENES:
        for pc in PCS:
            name = "%s_%s" % (scene, pc)
            assert str(one[name + "__form"]) == "replicated" and int(one[name + "__levels"]) == 2
            assert 0 < int(one[name + "__iters"]) == int(one["plugin_" + name + "__iters"]) < 100
            util.assert_bitexact(one[name + "__pres"], one["plugin_" + name + "__pres"], "pressure, slab world 1 vs plugin")


@pytest.mark.parametrize("dims,world", [(d, w) for d in DIMS for w in (2, 3)] + [(REPLICATED_DIMS, 2)])
def test_worlds_against_world_1(tmp_path_factory, dims, world):
    one = run_world(tmp_path_factory, 1, dims)
    multi = run_world(tmp_path_factory, world, dims)
    assert [int(p["z0"]) for p in multi][0] == 0 and int(multi[-1]["z1"]) == int(dims.split("x")[2])
    for scene in SCENES:
        # the probe V-cycle: the preconditioner itself, bit for bit on the owned planes
        name = scene + "_static"
        util.assert_bitexact(np.concatenate([p[name + "__probe"] for p in multi], axis=0), one[0][name + "__probe"],
                             "probe V-cycle, %s, world %d vs world 1" % (scene, world))
        assert np.isfinite(one[0][name + "__probe"]).all() and not (one[0][name + "__probe"] == -7.0).any()
        for pc in PCS:
            name = "%s_%s" % (scene, pc)
            single, many = as_single(one, name), as_single(multi, name)
            print("%s %s: world 1 %d iterations, world %d %d" % (dims, name, single["iters"][0], world, many["iters"][0]))
            check_against_single(single, many)
            assert many["iters"][0] <= single["iters"][0] + 1
            assert {str(p[name + "__form"]) for p in multi} == {str(one[0][name + "__form"])}

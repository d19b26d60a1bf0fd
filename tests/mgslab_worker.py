"""Worker for the z-slab multigrid tests (tests/test_gpu_mgslab_worlds.py): run alone (world 1) or under torch.distributed.run
(gloo, every rank on cuda:0 through the HIP library), as tests/slab_worker.py is.  One run does, on the scene of slab_worker's
smoke case (its flags, velocity and density seeds; MacCormack advection, setWallBcs):
  * per scene ("smoke": solvePressure as it stands; "liquid": the same with a level set phi, the ghost-fluid solve) and per
    preconditioner (PcMGDynamic, PcMGStatic) one slab.solvePressure from the same advected velocity,
  * after each Static solve a probe V-cycle (slab.applyMG) on a seeded vector with the hierarchy that solve left,
  * at world 1 the plugin solvePressure on a plain solver with the same preconditioner and exactly the options the slab path
    takes (no zero-pressure fixing, none of the other optional terms), and the Static sequence: a solve, a solve after the flags
    changed (the stale hierarchy), releaseMG and the same solve again (a fresh one) -- on both routes.
Writes the owned planes of its results."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import util  # noqa: E402
from mantaflow_amd import _lib  # noqa: E402

ACCURACY = 1e-4
PCS = {"dynamic": 2, "static": 3}


def level_set(dims):
    """the free surface of the liquid scene: the plane y = 2/3 sy (mg_cases.inputs' ghost-fluid case)"""
    sx, sy, sz = dims
    zz, yy, xx = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return (yy - (2 * sy) // 3 + 0.3).astype(np.float32)


def blob_flags(flags_g, dims):
    """the flags with an obstacle blob added: the system a stale Static hierarchy was not built from"""
    sx, sy, sz = dims
    zz, yy, xx = np.ogrid[:sz, :sy, :sx]
    blob = (xx - sx // 2) ** 2 + (yy - sy // 3) ** 2 + (zz - sz // 2) ** 2 <= 9
    out = flags_g.copy()
    out[blob & (out == util.FLUID)] = util.OBS
    assert (out != flags_g).sum() > 20
    return out


def main():
    out = sys.argv[1]
    dims = tuple(int(v) for v in sys.argv[2].split("x"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    _lib.get()
    import cases
    from mantaflow_amd import core, plugins, slab
    NX, NY, NZ = dims
    dom = slab.SlabDomain(dims, slab.required_ghost(2.0))
    s = dom.solver
    s.timestep = 0.9
    flags_g = util.make_flags(NX, NY, NZ, 51, obstacles=True, empty_top=True)
    vel_g = util.smooth_vel(NX, NY, NZ, 52, 2.0)
    vel_g[2] *= 0.95
    dens_g = util.rand_real((NZ, NY, NX), 53)
    phi_g = level_set(dims)
    probe_g = util.rand_real((NZ, NY, NX), 54)
    flags, vel, dens, pres, phi, probe, pout = (core.FlagGrid(s), core.MACGrid(s), core.Grid(s), core.Grid(s), core.LevelsetGrid(s),
                                                core.Grid(s), core.Grid(s))
    dom.scatter_global(flags, flags_g); dom.scatter_global(vel, vel_g); dom.scatter_global(dens, dens_g)
    dom.scatter_global(phi, phi_g); dom.scatter_global(probe, probe_g)
    slab.advectSemiLagrange(dom, flags, vel, dens, order=2)
    slab.advectSemiLagrange(dom, flags, vel, vel, order=2)
    dom.exchange(vel, 1)
    slab.setWallBcs(dom, flags, vel)
    dom.exchange(vel, 1)
    vel_adv = core.MACGrid(s)
    vel_adv.copyFrom(vel)
    rec = dict(z0=dom.z0, z1=dom.z1, dens=dom.gather_owned(dens), vel_adv=dom.gather_owned(vel_adv).copy())
    rhs = core.Grid(s)

    def slab_solve(name, use_phi, pc, fl=flags, v0=vel_adv):
        vel.copyFrom(v0)
        st = {}
        slab.solvePressure(dom, vel, pres, fl, cgAccuracy=ACCURACY, stats=st, phi=phi if use_phi else None, preconditioner=pc)
        rec[name + "__pres"], rec[name + "__vel"] = dom.gather_owned(pres).copy(), dom.gather_owned(vel).copy()
        rec[name + "__iters"], rec[name + "__res"] = st["iterations"], st["residual"]
        rec[name + "__levels"], rec[name + "__form"] = st["mg_levels"], st["mg_form"]
        dom.exchange(vel, 1)
        s.lib.call("mf_make_rhs", NX, NY, dom.LZ, fl.ptr, rhs.ptr, vel.ptr, None, None, None, None, None, 0.0, 1e-4, None, None, s.stream)
        rec[name + "__div"] = dom.gather_owned(rhs).copy()

    for scene, use_phi in (("smoke", False), ("liquid", True)):
        for pcname, pc in PCS.items():
            name = scene + "_" + pcname
            slab_solve(name, use_phi, pc)
            if pc == slab.PcMGStatic:
                assert dom._mg is not None and dom._mg.is_set
                pout.setConst(-7.0)
                slab.applyMG(dom, pout, probe)
                rec[name + "__probe"] = dom.gather_owned(pout).copy()
                slab.releaseMG(dom)
            assert getattr(dom, "_mg", None) is None
    # a plain whole-domain solver beside the slab solver, as in slab_worker: its advection is the single-device result on every rank
    sg = core.Solver(gridSize=core.vec3(NX, NY, NZ), dim=3)
    sg.timestep = 0.9
    fg, vg, dg, pg, phg = core.FlagGrid(sg), core.MACGrid(sg), core.Grid(sg), core.Grid(sg), core.LevelsetGrid(sg)
    cases.soa_to_grid(fg, flags_g); cases.soa_to_grid(vg, vel_g); cases.soa_to_grid(dg, dens_g); cases.soa_to_grid(phg, phi_g)
    plugins.advectSemiLagrange(fg, vg, dg, order=2)
    rec["plain_dens"] = cases.grid_to_soa(dg)
    if world == 1:
        adv = rec["vel_adv"]

        def plugin_solve(name, use_phi, pc, fl=fg):
            cases.soa_to_grid(vg, adv)
            plugins.solvePressure(vg, pg, fl, cgAccuracy=ACCURACY, phi=phg if use_phi else None, preconditioner=pc)
            sg.sync()
            rec[name + "__pres"], rec[name + "__iters"] = cases.grid_to_soa(pg), plugins.lastCgStats()["iterations"]

        for scene, use_phi in (("smoke", False), ("liquid", True)):
            for pcname, pc in PCS.items():
                plugin_solve("plugin_%s_%s" % (scene, pcname), use_phi, pc)
                plugins.releaseMG(sg)
        # the Static sequence on both routes: fresh, stale (the flags changed under the kept hierarchy), fresh again after releaseMG
        flags2_g = blob_flags(flags_g, dims)
        flags2, fg2 = core.FlagGrid(s), core.FlagGrid(sg)
        dom.scatter_global(flags2, flags2_g); cases.soa_to_grid(fg2, flags2_g)
        slab_solve("seq0", False, slab.PcMGStatic)
        slab_solve("seq1_stale", False, slab.PcMGStatic, fl=flags2)
        slab.releaseMG(dom)
        slab_solve("seq2_fresh", False, slab.PcMGStatic, fl=flags2)
        slab.releaseMG(dom)
        plugin_solve("plugin_seq0", False, slab.PcMGStatic)
        plugin_solve("plugin_seq1_stale", False, slab.PcMGStatic, fl=fg2)
        plugins.releaseMG(sg)
        plugin_solve("plugin_seq2_fresh", False, slab.PcMGStatic, fl=fg2)
        plugins.releaseMG(sg)
    np.savez(out + ".%d.npz" % dom.comm.rank, **rec)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

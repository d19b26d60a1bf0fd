"""The opt-in switch of the multigrid preconditioner on 2-D solvers (include/open/manta_hip_mg2d.h, csrc/mg2d.hip).

The reference's GridMg has a complete 2-D mode (source/multigrid.cpp:231-236, 723-726) and it is the reference's only real
preconditioner for 2-D systems: on a grid that is not 3-D its PcMIC degrades to plain CG (conjugategrad.cpp:315-321).  This package
refuses PcMGStatic / PcMGDynamic on a 2-D solver by default, word for word as it always did; a scene that wants them puts two
lines in front and is otherwise unchanged:

    from mantaflow_amd.multigrid2d import setMultigrid2D
    setMultigrid2D()

With the switch on, a 2-D whole-domain solver on the HIP backend accepts both preconditioners in solvePressure,
solvePressureSystem and PD_fluid_guiding, with every optional term they take; maxIter is 100 (pressure.cpp:421), and the life
cycle is the 3-D one (one hierarchy per solver; Dynamic releases before and after the solve, Static keeps the hierarchy with its
matrix until releaseMG).  The CPU checker backend and z-slab solvers are refused by name before any grid is touched.

mantaflow_amd.api does not import this module and `manta` does not export it.  Importing it does not flip the switch; the switch
itself lives in plugins.py next to _multigrid_lib, the one place that decides."""
from . import core  # noqa: F401  (first: the package's modules import in the order core, plugins, scene)
from . import plugins

__all__ = ["setMultigrid2D", "multigrid2DEnabled"]


def setMultigrid2D(on=True):
    """turn the 2-D multigrid preconditioners on (or off) for the whole process; returns the previous setting"""
    prev = plugins._multigrid_2d
    plugins._multigrid_2d = bool(on)
    return prev


def multigrid2DEnabled():
    return plugins._multigrid_2d

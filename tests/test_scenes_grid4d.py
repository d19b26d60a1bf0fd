"""CPU: the reference's own harness scripts that need the 4-D grids, the particle-data arithmetic and the symmetry checks, through `from manta import *` on the CPU checker backend.  The
script text is read from the reference checkout at test time (nothing is copied; where the checkout is absent the tests skip), runs
its set-up and every call that goes through the core header, and stops at its first call into the extension, which the checker backend
refuses by name.  On the device the scripts' sequences run to their end in tests/test_gpu_grid4d.py."""
import os
import sys
import types

import pytest

REF = "/root/reference"
WHAT = "the 4-D grid and particle-data kernels"

# script -> (text substitutions, the first call the checker backend refuses, names the script must have created before it)
SCRIPTS = {
    # the Real grids' whole sequence (setConst, addConst, multConst, copyFrom, add, addScaled) runs; the Vec3 broadcast form is a kernel
    "tools/tests/test_0032_grid4dop.py": ((), "Grid4d::setConst", ("rlg3", "vcg1", "int3", "fdg3")),
    "tools/tests/test_0042_interpol4d.py": ((("res = 40", "res = 8"),), "setRegion4d", ("sm_density", "xl_v3", "sm_velDisp2", "rend")),
    # reading its particle file (written here by the script's own generate branch, see below), the Real and Vec3 sequences run
    "tools/tests/test_0500_pdataop.py": ((), "ParticleDataImpl::addConst", ("rlg3", "vcg3", "int3")),
    # the pressure solve runs; the first symmetry check is a kernel
    "tools/tests/test_2005_symmAdv.py": ((("res = 34", "res = 12"),), "checkSymmetry", ("errV2", "drop", "fluidVel", "velDir")),
    # generate branch: sampling, mapPartsToGrid, buoyancy, the solve and the wall conditions run; the noise channel is a kernel
    "tools/tests/test_2065_partIo.py": ((("res = 50", "res = 16"),), "setNoisePdata", ("pDens", "noise", "fluidbox2")),
}
GENERATES = ("tools/tests/test_2065_partIo.py",)
USES = {
    "tools/tests/test_0032_grid4dop.py": ("Grid4Real", "Grid4Vec3", "Grid4Int", "Grid4Vec4"),
    "tools/tests/test_0042_interpol4d.py": ("setRegion4d", "setRegion4dVec4", "interpolateGrid4d", "interpolateGrid4dVec", "getSliceFrom4d", "getSliceFrom4dVec"),
    "tools/tests/test_0500_pdataop.py": ("addTestParts", "PdataReal", "PdataVec3", "PdataInt"),
    "tools/tests/test_2005_symmAdv.py": ("checkSymmetry", "checkSymmetryVec3"),
    "tools/tests/test_2065_partIo.py": ("setNoisePdata", "mapPartsToGrid"),
}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "tools", "tests")), reason="reference scripts not present on this machine")
@pytest.mark.parametrize("script", sorted(SCRIPTS))
def test_script_runs_to_its_first_refused_call(oracle_backend, monkeypatch, tmp_path, script):
    import manta as m
    subs, first, left = SCRIPTS[script]
    src = open(os.path.join(REF, script)).read()
    for a, b in subs:
        assert a in src, (script, a)
        src = src.replace(a, b)
    for name in USES[script]:
        assert name in src and callable(getattr(m, name)), (script, name)
    # the harness tests import the reference's helperInclude for their final comparison, which is never reached here
    helper = types.ModuleType("helperInclude")
    helper.doTestGrid = lambda *a, **k: None
    helper.getGenRefFileSetting = lambda: int(script in GENERATES)
    helper.getVisualSetting = lambda: 0
    helper.referenceFilename = lambda sc, name: str(tmp_path / (name + ".uni"))
    if script.endswith("test_0500_pdataop.py"):      # what its generate branch writes first: ten test particles (host code, every backend)
        gen = m.Solver(name="gen", gridSize=m.vec3(12, 19, 31), dim=3).create(m.BasicParticleSystem)
        m.addTestParts(gen, 10)
        gen.save(helper.referenceFilename(script, "parts"))
    monkeypatch.setitem(sys.modules, "helperInclude", helper)
    g = {"__name__": "__main__", "__file__": os.path.basename(script)}
    with pytest.raises(RuntimeError) as err:
        exec(compile(src, os.path.basename(script), "exec"), g)
    assert str(err.value) == "%s: the 'oracle' backend does not implement %s (manta_hip_grid4d.h)" % (first, WHAT)
    for name in left:
        assert name in g, (script, name)
    if script.endswith("test_0500_pdataop.py"):
        assert g["pp"].pySize() == 10 and g["rlg3"].size() == 10
    elif "rlg3" in g:               # what ran before the refusal is the script's own arithmetic: 1.1 + 1.2 + 0.5 * 1.2
        import numpy as np
        f32 = np.float32
        want = (f32(1.0) + f32(0.1)) + f32(2.4) * f32(0.5)
        want = want + f32(0.5) * (f32(2.4) * f32(0.5))
        assert (g["rlg3"].to_numpy() == want).all() and g["rlg3"].to_numpy().shape == (12, 30, 20, 10)

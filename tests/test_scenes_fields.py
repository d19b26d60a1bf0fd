"""CPU: the reference's own scripts that need the fire, wave-equation and uv-grid plugins, through `from manta import *` on the CPU
checker backend.  The script text is read from the reference checkout at test time (nothing is copied; where the checkout is absent
the tests skip) with its resolution reduced, and runs up to its first call into the extension, which the checker backend refuses by
name: every name the script uses before that point exists, and the set-up in front of it runs.  On the device the scripts run to their
end; their loops are tests/test_gpu_fields.py's."""
import os
import sys
import types

import pytest

REF = "/root/reference"
WHAT = "the fire, wave-equation and uv-grid plugins"

# script -> (text substitutions, the first call the checker backend refuses, names the set-up must have left behind)
SCRIPTS = {
    "scenes/fire.py": ((("res = 52", "res = 16"),), "processBurn", ("sourceBox", "noise", "flame")),
    "scenes/waveEquation.py": ((("res = 100", "res = 24"),), "totalSum", ("source", "hprev")),
    "scenes/waveletTurbulenceObs.py": ((("res = 80", "res = 12"), ("upres = 4", "upres = 2")), "resetUvGrid", ("xl_noise", "obs")),
    "tools/tests/test_1020_uvs.py": ((("res = 50", "res = 16"),), "resetUvGrid", ("source", "sourceVel")),
    "tools/tests/test_1030_waveeq.py": ((("vec3( 113,127, 1)", "vec3( 23,19, 1)"),), "totalSum", ("source", "hprev")),
    "tools/tests/test_1040_secOrderBnd.py": ((), "initVortexVelocity", ("phiObs", "sphere")),
}
# names of the extension each script calls: all of them exist
USES = {
    "scenes/fire.py": ("processBurn", "updateFlame"),
    "scenes/waveEquation.py": ("totalSum", "cgSolveWE", "calcSecDeriv2d", "normalizeSumTo"),
    "scenes/waveletTurbulenceObs.py": ("resetUvGrid", "updateUvWeight", "extrapolateSimpleFlags", "getUvWeight"),
    "tools/tests/test_1020_uvs.py": ("resetUvGrid", "updateUvWeight"),
    "tools/tests/test_1030_waveeq.py": ("totalSum", "cgSolveWE", "calcSecDeriv2d", "normalizeSumTo"),
    "tools/tests/test_1040_secOrderBnd.py": ("initVortexVelocity",),
}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "scenes")), reason="reference scripts not present on this machine")
@pytest.mark.parametrize("script", sorted(SCRIPTS))
def test_script_runs_to_its_first_refused_call(oracle_backend, monkeypatch, script):
    import manta as m
    subs, first, left = SCRIPTS[script]
    src = open(os.path.join(REF, script)).read()
    for a, b in subs:
        assert a in src, (script, a)
        src = src.replace(a, b)
    for name in USES[script]:
        assert name + "(" in src.replace(" (", "(") and callable(getattr(m, name)), (script, name)
    # the harness tests import the reference's helperInclude for their final comparison, which is never reached here
    helper = types.ModuleType("helperInclude")
    helper.doTestGrid = lambda *a, **k: None
    monkeypatch.setitem(sys.modules, "helperInclude", helper)
    g = {"__name__": "__main__", "__file__": os.path.basename(script)}
    with pytest.raises(RuntimeError) as err:
        exec(compile(src, os.path.basename(script), "exec"), g)
    assert str(err.value) == "%s: the 'oracle' backend does not implement %s (manta_hip_fields.h)" % (first, WHAT)
    for name in left:
        assert name in g, (script, name)

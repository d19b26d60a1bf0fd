"""The reference's guiding scripts through `from manta import *`, as far as a machine without a GPU can take them (the script text is
read from the reference checkout at test time -- nothing is copied; the checkout exists only beside the CPU checker backend, which
refuses PD_fluid_guiding by design, so the guided loops themselves are tests/test_gpu_guiding.py's cases (a) and (b)):

  * scenes/guiding_3d01_low.py runs a few frames at a reduced res and writes its plume3DLowRes_%04d.uni files;
  * scenes/guiding_3d02_high.py, unchanged but for res1 and the frame count, loads them, interpolates them to the fine grid and
    reaches its first PD_fluid_guiding call with every argument in place;
  * scenes/guiding_2d.py (its one PcMGStatic switched to PcMIC: multigrid stays out of 2-D solvers) does the same through
    getSpiralVelocity and setGradientYWeight with the script's float row numbers."""
import os

import numpy as np
import pytest

from test_scenes_run import SCENES, run_scene

pytestmark = pytest.mark.skipif(not os.path.isdir(SCENES), reason="reference scenes not present on this machine")
REFUSAL = r"PD_fluid_guiding: the 'oracle' backend does not implement fluid guiding"


@pytest.fixture
def reached(monkeypatch):
    """records the arguments of the first PD_fluid_guiding call, then lets the call go on (to its refusal on this backend)"""
    import manta
    from mantaflow_amd import api
    seen = {}
    real = api.PD_fluid_guiding

    def spy(*a, **kw):
        seen.setdefault("kw", dict(kw))
        seen.setdefault("velT", kw["velT"].to_numpy().copy())
        seen.setdefault("W", kw["weight"].to_numpy().copy())
        return real(*a, **kw)

    for mod in (manta, api):
        monkeypatch.setattr(mod, "PD_fluid_guiding", spy)
    manta.releaseBlurPrecomp()
    yield seen
    manta.releaseBlurPrecomp()


def test_guiding_3d_low_feeds_high(oracle_backend, reached, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    g = run_scene("guiding_3d01_low.py", None, [("res0 = 40", "res0 = 8"), ("numFrames = 200", "numFrames = 3")])
    for t in range(3):
        assert os.path.exists("plume3DLowRes_%04d.uni" % t)
    low = g["vel"].to_numpy()
    assert np.isfinite(low).all() and np.abs(low).max() > 0
    with pytest.raises(RuntimeError, match=REFUSAL):
        run_scene("guiding_3d02_high.py", None, [("res1 = 40", "res1 = 8"), ("numFrames = 200", "numFrames = 3")])
    kw = reached["kw"]
    assert kw["blurRadius"] == 5 and kw["preconditioner"] == 3 and kw["zeroPressureFixing"] is True
    assert abs(kw["tau"] - 0.29) < 1e-12 and abs(kw["sigma"] - 2.44 / 0.29) < 1e-12 and kw["theta"] == 0.3
    assert reached["velT"].shape == (16, 32, 16, 3) and (reached["W"] == 2).all()
    assert np.isfinite(reached["velT"]).all()          # frame 0 of the low-res run (at rest before its first solve's effect is saved)


def test_guiding_2d_reaches_the_solve(oracle_backend, reached):
    with pytest.raises(RuntimeError, match=REFUSAL):
        run_scene("guiding_2d.py", None, [("res0 = 64", "res0 = 16"), ("preconditioner = PcMGStatic", "preconditioner = PcMIC")])
    kw = reached["kw"]
    assert kw["blurRadius"] == 2 and kw["preconditioner"] == 1 and kw["sigma"] == 0.99 and kw["tau"] == 1.0
    W, velT = reached["W"], reached["velT"]
    assert W.shape == (1, 32, 32) and (W[:, :16] == 1).all() and (W[:, 16:] == 5).all()
    speed = np.sqrt(velT[..., 0] ** 2 + velT[..., 1] ** 2)
    assert np.allclose(speed, 1.0, atol=1e-6) and not velT[..., 2].any()          # strength 0.5 * scale = 1

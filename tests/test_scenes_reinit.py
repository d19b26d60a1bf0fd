"""scenes/freesurface.py with its fast-marching switch on, run through `from manta import *` at a reduced size on the CPU checker backend
(edits applied to the text read from the reference checkout at test time; nothing is copied): the set-up -- Box and Sphere level sets,
join, updateFromLevelset -- runs, and the first call the backend does not have is LevelsetGrid.reinitMarching, refused by name.  (The
device path of the same loop is held against recorded reference runs in tests/test_gpu_reinit.py.)"""
import os

import pytest

from test_scenes_run import SCENES, run_scene

pytestmark = pytest.mark.skipif(not os.path.isdir(SCENES), reason="reference scenes not present on this machine")


def test_freesurface_with_marching_reaches_reinit_marching_on_the_cpu_backend(oracle_backend):
    with pytest.raises(RuntimeError) as e:
        run_scene("freesurface.py", 2, [("res = 64", "res = 16"), ("useMarching = False", "useMarching = True")])
    assert str(e.value) == ("LevelsetGrid::reinitMarching: the 'oracle' backend does not implement level-set reinitialisation by fast "
                            "marching (manta_hip_reinit.h)")

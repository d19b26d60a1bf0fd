"""-m gpu: the z-slab window code of the HIP library, entry point by entry point (tests/window_cases.py).  Every case on the planes
[lo, hi) under mf_set_slab_window(lo, gsz):
  - against the undivided oracle, bit for bit on the planes (particles) left after trimming the case's reach at every cut;
  - against the oracle under the same window, bit for bit on the whole local result, ghost planes and particles outside the window
    included: the window code itself must not diverge.
tests/test_oracle_window_kernels.py checks the oracle's side, and that no case is empty, on the CPU."""
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("win", list(wc.WINDOWS))
@pytest.mark.parametrize("name,shape", wc.PARAMS, ids=["%s-%s" % p for p in wc.PARAMS])
def test_window(hip, oracle, name, shape, win):
    wc.check_hip(hip, oracle, name, shape, win)

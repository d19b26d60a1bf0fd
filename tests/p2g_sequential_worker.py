"""Worker of test_gpu_p2g_ordered.py::test_sequential_kernels: started as a fresh process with MF_P2G_SEQUENTIAL set (the library reads
the variable once per process), runs the one-thread cross-check kernels k_p2g_mac_sequential and k_p2g_cell_sequential<1|3> through
the ABI with deterministic = 1 on the `patterns` input and writes the results to the .npz file named on the command line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import p2g_cases as C  # noqa: E402
import util  # noqa: E402


def main():
    assert os.environ.get("MF_P2G_SEQUENTIAL"), "the parent starts this worker with MF_P2G_SEQUENTIAL set"
    hip, inp = util.Impl("hip"), C.get("patterns")
    out = dict(zip(("vel", "velOld", "weight"), C.run_mac(hip, inp, deterministic=1)))
    for nc in (1, 3):
        out["target%d" % nc], out["wtmp%d" % nc] = C.run_cell(hip, inp, nc, deterministic=1)
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()

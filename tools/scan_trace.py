"""One small FLIP script over the users of csrc/scan.hip, for a kernel trace or an A/B of two builds of the library: a 32^3
narrow-band dam break (gridParticleIndex and adjustNumber every step), then createMesh on its level set and Mesh.computeLevelset on
that mesh.  Prints a SHA-256 over everything it computed.
  [MF_LIB=path/to/libmanta_hip.so] rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/scan_trace.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: both then share the HIP runtime that torch loads)
from mantaflow_amd import _lib  # noqa: E402

if os.environ.get("MF_LIB"):
    _lib.use_library(os.path.abspath(os.environ["MF_LIB"]), "cuda")
import manta as m  # noqa: E402
import nbflip_model  # noqa: E402

out = nbflip_model.nb_loop(m, res=32, dim=3, steps=3)
s = out["solver"]
phi = s.create(m.LevelsetGrid)
phi.from_numpy(out["phi"])
mesh = s.create(m.Mesh)
phi.createMesh(mesh)
sdf = s.create(m.LevelsetGrid)
mesh.computeLevelset(sdf, 2.)
h = hashlib.sha256()
for k in ("counts", "iters", "phi", "vel", "phiParts", "velParts", "pos", "flag", "pvel"):
    h.update(np.ascontiguousarray(out[k]).tobytes())
h.update(sdf.to_numpy().tobytes())
print("particles per step %s, sha256 %s" % (out["counts"].tolist(), h.hexdigest()))

"""Driver of tools/surfturb_host_check.hip (its header has the build line): runs the stand-alone host program on the recorded calls and
stages of tests/golden/surfturb.npz and compares with the reference's states and with the numpy model of tests/surfturb_model.py, the latter also on every stage of every
edge case (surfturb_model.EDGE_CASES) -- against the reference bit for bit where nothing is downstream of expf / logf
within the stage, within the bounds of tests/surfturb_model.py elsewhere; the discrete results (sizes, flags, delete bookkeeping)
always exactly.  The program is a separate process; nothing is loaded into this one.

    python tools/surfturb_host_check.py <path to surfturb_host_check>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import surfturb_model as M  # noqa: E402


def main(exe):
    G = M.golden()
    for k in range(3):
        par, R, dirs = M.host_params(exe, G, k)
        assert par[:9].tobytes() == G["set%d/par" % k].tobytes(), (k, par[:9], G["set%d/par" % k])
        assert R.tolist() == G["set%d/res" % k].tolist(), (k, R)
        if k:
            got = M.host_run(exe, "call", M.init_case(G, k))
            assert got["pos"].tobytes() == G["set%d/init_pos" % k].tobytes(), k
        print("set %d: parameters, list resolutions%s equal the reference bit for bit (%d directions)"
              % (k, " and initFines" if k else "", len(dirs)))
    for f in range(3):
        got = M.host_run(exe, "call", M.call_case(G, f))
        print("call %d:" % f, M.compare(got, M.state(G, "call%d/after" % f), exact=False, displaced=G["call%d/displaced" % f]),
              "iterations (added, rounds, kills x 3, compressed):", got["stats"].tolist())
    names = M.chain_names(G)
    for i, name in enumerate(names):
        got = M.host_run(exe, name, M.chain_case(G, i))
        print("chain %d %s:" % (i, name), M.compare(got, M.state(G, "chain/%d" % i), exact=name in M.EXACT_STAGES),
              "| points that differ from the model:", M.compare_model(got, M.model_stage(G, i)[1], name))
    # the same text against the numpy model at the edges: every stage on every edge case
    for case in M.EDGE_CASES:
        counts = []
        for stage in M.EDGE_STAGES:
            c, mdl, want = M.edge_model(G, case, stage)
            counts.append(M.compare_model(M.host_run(exe, stage, c), want, (case, stage)))
        print("edge %s: points that differ from the model per stage %s" % (case, counts))


if __name__ == "__main__":
    main(sys.argv[1])

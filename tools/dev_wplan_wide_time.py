"""dev tool: zk_wplan_solve time of the tape plan beside the wide plan (lanes = 8, 16, 32, 64) at k = 1, 32, 256, 1 024 witnesses per call, for the
depth-29 Poseidon membership circuit, the Poseidon preimage circuit and the depth-29 MiMC Merkle circuit -- one process, every figure after a
warm-up call, the median of three calls.  Every solve starts from the supplied variables alone and its first and last rows are compared with
the front end's witness."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
from ethsnarks_amd import prover as P, fields as F, gadgets as G
P.load_library(os.environ.get("ZK_LIB") or None)
print("library:", P._lib.zk_version().decode())
KS = (1, 32, 256, 1024)
LANES = (8, 16, 32, 64)
CIRCUITS = [("poseidon_membership_circuit(29)", lambda: G.poseidon_membership_circuit(29), 1 + 1 + 29 + 29 + 1),
            ("poseidon_preimage_circuit(2)", lambda: G.poseidon_preimage_circuit(2), 1 + 1 + 2),
            ("merkle_membership_circuit(29)", lambda: G.merkle_membership_circuit(29), 1 + 1 + 29 + 29 + 1 + 29)]
for name, make, n_sup in CIRCUITS:
    r, w, _ = make()
    supplied = list(range(n_sup))
    full = F.fr_to_mont(w)
    plans = [("tape", P.WitnessPlan(r, supplied))]
    for lanes in LANES:
        try:
            plans.append(("wide %2d" % lanes, P.WitnessPlan(r, supplied, lanes=lanes)))
        except P.ZkError as e:
            print("%s, lanes = %d: %s" % (name, lanes, e))
    nnz = sum(int(m.row_ptr[-1]) for m in (r.A, r.B, r.C))
    print("%s: %d constraints, %d variables, %.1f non-zeros per constraint" % (name, r.nC, r.V, nnz / r.nC))
    for label, plan in plans:
        print("  %s: %s" % (label, plan.info()))
    row = 32 * (r.V + 1)
    for k in KS:
        start = np.zeros((k, r.V + 1, 4), dtype=np.uint64)
        start[:, supplied] = full[supplied]
        buf = P.DeviceBuffer(row * k)
        line = []
        for label, plan in plans:
            buf.upload(start)
            plan.solve(buf.ptr, k)                                   # warm-up
            ts = []
            for _ in range(3):
                buf.upload(start)
                t0 = time.perf_counter(); bad = plan.solve(buf.ptr, k); ts.append(1e3 * (time.perf_counter() - t0))
            ok = bad == 0 and all(np.array_equal(buf.download((r.V + 1, 4), offset=row * p), full) for p in (0, k - 1))
            line.append("%s %8.2f ms%s" % (label, statistics.median(ts), "" if ok else " WRONG"))
        print("  k = %4d: %s" % (k, " | ".join(line)), flush=True)
        buf.free()
    for _, plan in plans:
        plan.close()

#!/usr/bin/env python3
"""dev tool: the measurements of profiles/poseidon.txt -- the Poseidon hash kernel in both MIX forms (Fr::ldot6 against six lmul per row), builds
and single appends of the Poseidon tree at widths 2 and 4 beside the MiMC tree in the same run, and membership proofs per second of the Poseidon
circuit beside the MiMC circuit, through the planner (fill_witnesses -> WitnessPlan.solve) and straight from the tree (fill_full_witnesses).
usage: python tools/poseidon_bench.py [--log-hashes 20] [--reps 5] [--no-proofs]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethsnarks_amd import prover as P, merkle as M, gadgets as G, fields as F  # noqa: E402


def random_limbs(n, seed):
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)                        # < 2^252 < r: valid as canonical and as Montgomery values
    return a


def kernel_ms(fn, reps):
    """median / min / max of the kernel time of fn() (HIP events around every launch, zk_profile_*): copies and allocations stay out"""
    fn()
    ts = []
    for _ in range(reps):
        P.profile_begin()
        fn()
        ts.append(P.profile_end()[0])
    return statistics.median(ts), min(ts), max(ts)


def wall_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-hashes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-proofs", action="store_true")
    ap.add_argument("--lanes", type=int, default=None, help="the chain leg's WitnessPlan: lanes per witness of the wide plan (default: the tape plan)")
    ap.add_argument("--chain-only", action="store_true", help="only the membership-proof chain legs")
    a = ap.parse_args()
    P.load_library()
    lib = P._lib
    print("library:", lib.zk_version().decode(), "| device:", P.device_info(0))
    # ---- independent hashes, both MIX forms (kernel time; the entry point's copies are not the kernel's)
    n = 1 << a.log_hashes
    for n_in in () if a.chain_only else (2, 4):
        rows = random_limbs(n * n_in, 10 + n_in)
        out = np.zeros((n, 4), dtype=np.uint64)
        call = lambda: P._check(lib.zk_poseidon_hash(P._p64(rows), C.c_uint32(n_in), C.c_uint32(n), 0, P._p64(out)))
        ref = None
        for mix, products in (("dot6", 1700), ("lmul", 2655)):
            os.environ["ZK_POSEIDON_MIX"] = mix
            med, lo, hi = kernel_ms(call, a.reps)
            os.environ.pop("ZK_POSEIDON_MIX")
            assert ref is None or np.array_equal(ref, out)          # the two forms agree
            ref = out.copy()
            print("poseidon_hash n = 2^%d, n_in = %d, MIX %s: kernel median %.3f ms (min %.3f, max %.3f, %d reps) = %.2f M hashes/s (%.1f G product-equivalents/s at %d per permutation)"
                  % (a.log_hashes, n_in, mix, med, lo, hi, a.reps, n / med / 1e3, n * products / med / 1e6, products))
    # ---- tree builds from a device buffer (Montgomery leaves), MiMC beside Poseidon in the same run
    trees = [("mimc", 2, 29), ("poseidon", 2, 29), ("poseidon", 4, 14)]
    for lg in () if a.chain_only else (16, 20):
        n = 1 << lg
        buf = P.DeviceBuffer(32 * n)
        buf.upload(random_limbs(n, lg))
        for hasher, w, depth in trees:
            launches = []

            def build():
                t = M.MerkleTree(w ** depth, reserve=n, width=w, hasher=hasher)
                c0 = P.launch_count()
                t0 = time.perf_counter()
                t.extend(buf, canonical=False)
                dt = 1e3 * (time.perf_counter() - t0)
                launches.append(P.launch_count() - c0)
                t.close()
                return dt
            build()
            ts = [build() for _ in range(a.reps)]
            nodes = sum(-(-n // w ** d) for d in range(1, depth + 1))
            print("build 2^%d leaves, %s width %d depth %d: median %.3f ms (min %.3f, max %.3f, %d reps), %d launches, %d nodes"
                  % (lg, hasher, w, depth, statistics.median(ts), min(ts), max(ts), a.reps, launches[-1], nodes))
        buf.free()
    # ---- one append at full depth: the latency floor, one dependent hash chain per level
    for hasher, w, depth in () if a.chain_only else trees:
        t = M.MerkleTree(w ** depth, reserve=1 << 12, width=w, hasher=hasher)
        t.extend(random_limbs(1000, 5))
        leaf = random_limbs(1, 6)
        med, lo, hi = wall_ms(lambda: t.extend(leaf), 50, warm=5)
        print("single append, %s width %d depth %d: median %.1f us (min %.1f, max %.1f, 50 reps)" % (hasher, w, depth, 1e3 * med, 1e3 * lo, 1e3 * hi))
        t.close()
    if a.no_proofs:
        return
    # ---- membership proofs per second at k = 32: resident chain tree -> fill_witnesses -> solve -> submit_batch -> collect
    k = 32
    for hasher in ("mimc", "poseidon"):
        r = (G.merkle_membership_circuit if hasher == "mimc" else G.poseidon_membership_circuit)(29)[0]
        n_sup = 1 + 1 + 29 + 29 + 1 + (29 if hasher == "mimc" else 0)
        pk, _ = P.keygen(r, seed=5)
        ctx = P.ProverContext(pk, r, max_batch=k)
        plan = P.WitnessPlan(r, list(range(n_sup)), lanes=a.lanes)
        print("  witness plan, %s: %s" % (hasher, plan.info()))
        t = M.MerkleTree(1 << 29, hasher=hasher)
        t.extend(random_limbs(4096, 7))
        idx = [(i * 127) % 4096 for i in range(k)]
        buf = P.DeviceBuffer(32 * (r.V + 1) * k)
        buf.upload(np.zeros((k, r.V + 1, 4), dtype=np.uint64))

        def chain():
            t.fill_witnesses(idx, buf, r)
            assert plan.solve(buf.ptr, k) == 0
            ctx.submit_batch(None, device_ptr=buf.ptr, k=k)
            ctx.collect_batch(k)
        med, lo, hi = wall_ms(chain, a.reps * 2, warm=2)
        # the parts, each on its own (every call is complete when it returns)
        parts = [("fill_witnesses", lambda: t.fill_witnesses(idx, buf, r)), ("WitnessPlan.solve", lambda: plan.solve(buf.ptr, k)),
                 ("submit_batch + collect_batch", lambda: (ctx.submit_batch(None, device_ptr=buf.ptr, k=k), ctx.collect_batch(k)))]
        print("  parts, %s: " % hasher + "; ".join("%s median %.2f ms (min %.2f, max %.2f)" % ((name,) + wall_ms(fn, a.reps * 2, warm=1)) for name, fn in parts))
        nnz = sum(int(m.row_ptr[-1]) if hasattr(m, "row_ptr") else 0 for m in (r.A, r.B, r.C))
        print("  non-zeros of A + B + C: %d (%.1f per constraint)" % (nnz, nnz / r.nC))
        print("membership proofs, %s depth 29 (%d constraints, domain 2^%d), k = %d: median %.2f ms (min %.2f, max %.2f, %d reps) = %.0f proofs/s"
              % (hasher, r.nC, r.domain_size.bit_length() - 1, k, med, lo, hi, a.reps * 2, 1e3 * k / med))
        # ---- the same proofs with the complete witness straight from the tree: fill_full_witnesses -> submit_batch -> collect
        solved = buf.download((k, r.V + 1, 4))

        def full_chain():
            t.fill_full_witnesses(idx, buf, r)
            ctx.submit_batch(None, device_ptr=buf.ptr, k=k)
            ctx.collect_batch(k)
        buf.upload(np.zeros((k, r.V + 1, 4), dtype=np.uint64))
        t.fill_full_witnesses(idx, buf, r)
        assert np.array_equal(buf.download((k, r.V + 1, 4)), solved)   # the rows the planner left, byte for byte
        fmed, flo, fhi = wall_ms(full_chain, a.reps * 2, warm=2)
        parts = [("fill_full_witnesses", lambda: t.fill_full_witnesses(idx, buf, r)),
                 ("submit_batch + collect_batch", lambda: (ctx.submit_batch(None, device_ptr=buf.ptr, k=k), ctx.collect_batch(k)))]
        print("  parts, %s, full witness: " % hasher + "; ".join("%s median %.2f ms (min %.2f, max %.2f)" % ((name,) + wall_ms(fn, a.reps * 2, warm=1)) for name, fn in parts))
        print("membership proofs from full witnesses, %s depth 29 (%d constraints), k = %d: median %.2f ms (min %.2f, max %.2f, %d reps) = %.0f proofs/s (%.2f x the chain above)"
              % (hasher, r.nC, k, fmed, flo, fhi, a.reps * 2, 1e3 * k / fmed, med / fmed))
        # ... and the call alone at k = 4096 (every leaf of the tree once): a throughput figure
        kk = 4096
        big = P.DeviceBuffer(32 * (r.V + 1) * kk)
        all_idx = list(range(kk))
        bmed, blo, bhi = wall_ms(lambda: t.fill_full_witnesses(all_idx, big, r), a.reps, warm=1)
        print("fill_full_witnesses, %s depth 29, k = %d: median %.2f ms (min %.2f, max %.2f, %d reps) = %.0f witnesses/s, %.1f GB/s written"
              % (hasher, kk, bmed, blo, bhi, a.reps, 1e3 * kk / bmed, 32e-6 * (r.V + 1) * kk / bmed))
        big.free()
        ctx.close(); plan.close(); t.close(); buf.free()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""dev tool: the measurements of profiles/merkle_tree.txt -- bulk builds, the latency floor of one append / update with and without the
one-workgroup tail kernel, update_many, proofs and fill_witnesses of the device MiMC Merkle tree (ethsnarks_amd/merkle.py) at depth 29.
usage: python tools/dev_merkle_tree.py [--max-log 24] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethsnarks_amd import prover as P, merkle as M, gadgets as G  # noqa: E402

PRODUCTS_PER_NODE = 728


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def random_limbs(n, seed):
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)                        # < 2^252 < r: valid as canonical and as Montgomery values
    return a


def nodes_of(n, depth=29):
    return sum((n + (1 << d) - 1) >> d for d in range(1, depth + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-log", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    P.load_library()
    print("library:", P._lib.zk_version().decode(), "| device:", P.device_info(0))
    # ---- bulk builds from a device buffer (Montgomery leaves): D2D copy + range check + hashing
    for lg in (16, 20, 24):
        if lg > a.max_log:
            continue
        n = 1 << lg
        buf = P.DeviceBuffer(32 * n)
        buf.upload(random_limbs(n, lg))
        launches = []

        def build():
            t = M.MerkleTree(1 << 29, reserve=n)
            c0 = P.launch_count()
            t0 = time.perf_counter()
            t.extend(buf, canonical=False)
            dt = time.perf_counter() - t0
            launches.append(P.launch_count() - c0)
            t.close()
            return dt
        build()
        ts = [build() for _ in range(a.reps)]
        med = statistics.median(ts)
        print("build 2^%d leaves, depth 29: median %.3f ms (min %.3f, max %.3f, %d reps), %d launches, %d nodes, %.2f G Fr products/s"
              % (lg, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts), a.reps, launches[-1], nodes_of(n), nodes_of(n) * PRODUCTS_PER_NODE / med / 1e9))
        buf.free()
    # ---- the latency floor: one append, one update (29 dependent hashes), with and without the tail kernel
    for no_tail in ("0", "1"):
        os.environ["ZK_MTREE_NO_TAIL"] = no_tail
        t = M.MerkleTree(1 << 29, reserve=1 << 12)
        os.environ.pop("ZK_MTREE_NO_TAIL")
        t.extend(random_limbs(1000, 5))
        leaf = random_limbs(1, 6)
        state = {"i": 0}

        def upd():
            state["i"] = (state["i"] + 37) % 1000
            t.update_many([state["i"]], leaf)
        c0 = P.launch_count()
        t.extend(leaf)
        la = P.launch_count() - c0
        ma = timed(lambda: t.extend(leaf), 50, warm=5)
        c0 = P.launch_count()
        upd()
        lu = P.launch_count() - c0
        mu = timed(upd, 50, warm=5)
        print("%s: single append median %.1f us (min %.1f) in %d launches; single update median %.1f us (min %.1f) in %d launches"
              % ("every level its own launch" if no_tail == "1" else "one-workgroup tail", 1e6 * ma[0], 1e6 * ma[1], la, 1e6 * mu[0], 1e6 * mu[1], lu))
        t.close()
    # ---- batched updates, paths and witness rows on a 2^20-leaf tree
    n = 1 << min(20, a.max_log)
    t = M.MerkleTree(1 << 29, reserve=n)
    t.extend(random_limbs(n, 9))
    r = G.merkle_membership_circuit(29)[0]
    rng = np.random.default_rng(1)
    for k in (1, 64, 4096):
        idx = rng.choice(n, size=k, replace=False).astype(np.uint64)
        vals = random_limbs(k, 10 + k)
        c0 = P.launch_count()
        t.update_many(idx, vals)
        lu = P.launch_count() - c0
        m = timed(lambda: t.update_many(idx, vals), a.reps * 2)
        print("update_many k = %d: median %.3f ms (min %.3f), %d launches, %.0f leaves/s" % (k, 1e3 * m[0], 1e3 * m[1], lu, k / m[0]))
    for k in (64, 4096):
        idx = rng.choice(n, size=k, replace=False).astype(np.uint64)
        m = timed(lambda: t.proofs(idx), a.reps * 2)
        ip = np.ascontiguousarray(idx)
        leaves = np.zeros((k, 4), dtype=np.uint64); paths = np.zeros((k * 29, 4), dtype=np.uint64)
        import ctypes as C
        raw = timed(lambda: P._check(P._lib.zk_mtree_paths(t._h, P._p64(ip), C.c_uint32(k), P._p64(leaves), P._p64(paths))), a.reps * 2)
        buf = P.DeviceBuffer(32 * (r.V + 1) * k)
        f = timed(lambda: t.fill_witnesses(idx, buf, r), a.reps * 2)
        print("k = %d: zk_mtree_paths median %.3f ms (%.0f paths/s; MerkleTree.proofs with Python ints %.3f ms); fill_witnesses median %.3f ms (%.0f rows/s)"
              % (k, 1e3 * raw[0], k / raw[0], 1e3 * m[0], 1e3 * f[0], k / f[0]))
        buf.free()
    t.close()
    # ---- the only other baseline: gadgets.mimc_hash in pure Python
    t0 = time.perf_counter()
    for i in range(200):
        G.mimc_hash([i, i + 1], 7)
    print("gadgets.mimc_hash (pure Python): %.3f ms per node" % (1e3 * (time.perf_counter() - t0) / 200))


if __name__ == "__main__":
    main()

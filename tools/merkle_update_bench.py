#!/usr/bin/env python3
"""dev tool: the measurements of profiles/merkle_update_seq.txt -- MerkleTree.update_seq (ordered leaf updates with root-to-root transition
witnesses) on a 2^20-leaf tree of depth 29, both hashers, against the two things it can be compared with in the same session:
  * the only equivalent without it: k single update() calls with a fill_full_witnesses pair around each (measured at k = 32, EXTRAPOLATED
    linearly to the larger k);
  * update_many + one fill_full_witnesses over the de-duplicated indices: DIFFERENT semantics (no intermediate states), shown as the floor that
    one dependent chain plus one trace pass costs.
usage: python tools/merkle_update_bench.py [--log-leaves 20] [--reps 7] [--out profiles/merkle_update_seq.txt]"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethsnarks_amd import prover as P, merkle as M  # noqa: E402

DEPTH = 29


def random_limbs(n, seed):
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)                        # < 2^252 < r
    return a


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def fmt(ts):
    return "median %.3f ms (min %.3f, max %.3f, %d reps)" % (statistics.median(ts), min(ts), max(ts), len(ts))


def predecessor_ms(fn, reps):
    """the host predecessor pass of `reps` further calls, in ms: ZK_MTREE_USEQ_TIMING=1 makes zk_mtree_update_seq report it on stderr, which is
    pointed at a file meanwhile (calls of their own, so the timed calls above read no clock and print nothing)"""
    sys.stderr.flush()
    saved = os.dup(2)
    os.environ["ZK_MTREE_USEQ_TIMING"] = "1"
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            for _ in range(reps):
                fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("ZK_MTREE_USEQ_TIMING", None)
        f.seek(0)
        return [float(v) for v in re.findall(r"host predecessor pass ([0-9.]+) ms", f.read().decode())]


def indices_with_repeats(n, k, rng):
    """k indices of which about a tenth repeat an earlier one"""
    idx = rng.choice(n, size=k, replace=False).astype(np.uint64)
    for j in range(1, k):
        if rng.random() < 0.1:
            idx[j] = idx[rng.integers(0, j)]
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-leaves", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_update_seq.txt"))
    a = ap.parse_args()
    P.load_library()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("MerkleTree.update_seq: tools/merkle_update_bench.py --log-leaves %d --reps %d" % (a.log_leaves, a.reps))
    say("library: %s | device: %s" % (P._lib.zk_version().decode(), P.device_info(0)))
    say("depth %d, 2^%d leaves, about 10 %% of the indices repeat an earlier one.  Every figure is HOST WALL-CLOCK time (perf_counter) around a call that" % (DEPTH, a.log_leaves))
    say("synchronises before it returns -- uploads, launches, kernels, root download -- not device time.  2 warm-up calls, then the median of %d with the spread.  Rows: %d (MiMC) / %d (Poseidon) elements of 32 bytes." % (a.reps, M.update_layout(DEPTH, "mimc")[3], M.update_layout(DEPTH, "poseidon")[3]))
    n = 1 << a.log_leaves
    for hasher in ("mimc", "poseidon"):
        say()
        say("---- %s" % hasher)
        t = M.MerkleTree(1 << DEPTH, reserve=n, hasher=hasher)
        buf0 = P.DeviceBuffer(32 * n)
        buf0.upload(random_limbs(n, 3))
        t.extend(buf0, canonical=False)
        buf0.free()
        _, _, _, row = M.update_layout(DEPTH, hasher)
        _, _, _, mrow = M.membership_full_layout(DEPTH, hasher)
        rng = np.random.default_rng(7)
        one = timed(lambda: t.update_many([12345], random_limbs(1, 4)), 20, warm=3)
        say("one update() = update_many of one index (the %d-hash dependent chain): %s" % (DEPTH, fmt(one)))
        per_update_old = None
        for k in (32, 1024, 4096):
            idx = indices_with_repeats(n, k, rng)
            vals = random_limbs(k, 100 + k)
            distinct = len(set(idx.tolist()))
            buf = P.DeviceBuffer(32 * row * k)

            def with_rows():
                t.update_seq(idx, vals, buf, row_elems=row)
            c0 = P.launch_count()
            with_rows()
            launches = P.launch_count() - c0
            w = timed(with_rows, a.reps)
            pred_med = statistics.median(predecessor_ms(with_rows, a.reps))
            bare = timed(lambda: t.update_seq(idx, vals), a.reps)
            say("k = %d (%d distinct): update_seq with rows %s, %d launches, %.1f us per update" % (k, distinct, fmt(w), launches, 1e3 * statistics.median(w) / k))
            say("    of which the host's predecessor pass: median %.3f ms (%.1f %% of the call)" % (pred_med, 100 * pred_med / statistics.median(w)))
            say("    update_seq without a buffer: %s" % fmt(bare))
            buf.free()
            # the floor (other semantics): one batched update, one trace pass over the distinct indices
            uniq = np.unique(idx)
            mbuf = P.DeviceBuffer(32 * mrow * len(uniq))
            uvals = random_limbs(len(uniq), 5)

            def floor():
                t.update_many(uniq, uvals)
                t.fill_full_witnesses(uniq, mbuf, row_elems=mrow)
            say("    floor, different semantics: update_many + fill_full_witnesses of the %d distinct indices: %s" % (len(uniq), fmt(timed(floor, a.reps))))
            mbuf.free()
            if k == 32:
                pair = P.DeviceBuffer(32 * mrow * 2)

                def single_updates():
                    for j in range(k):
                        t.fill_full_witnesses(idx[j:j + 1], pair, row_elems=mrow)
                        t.update_many(idx[j:j + 1], vals[j:j + 1])
                        t.fill_full_witnesses(idx[j:j + 1], pair.ptr + 32 * mrow, row_elems=mrow)
                old = timed(single_updates, a.reps)
                per_update_old = statistics.median(old) / k
                say("    without update_seq: 32 x (fill_full_witnesses, update, fill_full_witnesses): %s = %.3f ms per update" % (fmt(old), per_update_old))
                pair.free()
            else:
                say("    without update_seq, EXTRAPOLATED linearly from k = 32 (not measured): %.1f ms" % (per_update_old * k))
        t.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

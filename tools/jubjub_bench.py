"""Baby JubJub on the device at n = 2^16: kernel time (the library's event pairs) and call time (staging and copies included) of every kernel,
the field products per item from the formulas of csrc/jubjub.hpp, and the fraction of a product-chain rate (tools/mulbench, "mul chain 8
waves/SIMD", passed as --chain in G/s) that the kernel reaches.  Writes the table profiles/jubjub.txt records.

    python tools/jubjub_bench.py --chain 142.4
"""
import argparse
import ctypes as C
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ethsnarks_amd import fields as F, jubjub as J, prover as P   # noqa: E402
import jubjub_cases as JC                                         # noqa: E402

INV = 254 + bin(F.FR - 2).count("1")                               # jj_inv: a squaring per bit, a product per set bit
TABLE = 2 + 14 * 9 + 15                                            # T = x y, d T, 14 mixed additions, 15 products by d
AFFINE = INV + 4                                                   # X / Z, Y / Z, two conversions
CURVE = 5
CORE = 4 + 2 * CURVE + TABLE + 64 * (3 * 8 + 9 + 9 + 10) + 2       # Straus: 3 short doublings, 1 full, a mixed and a full addition per window
PRODUCTS = {
    "k_jj_scalar_mul": 2 + CURVE + TABLE + 64 * (3 * 8 + 9 + 10) + AFFINE,
    "k_jj_point_op": 4 + 2 * CURVE + 3 + 10 + AFFINE,
    "k_jj_pedersen": 9 * 254 + AFFINE,
    "mimc": CORE + 7 * 91 * 4 + 3 + 1,
    "pure": CORE + 9 * ((508 + 24 + 2) // 3) + AFFINE,
    "hash": CORE + 9 * 8 + AFFINE + 9 * 254 + AFFINE,
}


def tile(points, n):
    a = F.ints_to_limbs([c for p in points for c in p]).reshape(-1, 8)
    return np.ascontiguousarray(np.tile(a, (n // len(points), 1)))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run(label, key, n, chain, fn):
    fn()                                                           # warm-up: code object, scratch, allocations
    P.profile_begin()
    t0 = time.perf_counter()
    fn()
    wall = 1e3 * (time.perf_counter() - t0)
    ms, launches, _ = P.profile_end()
    prod = PRODUCTS[key]
    rate = n * prod / (ms * 1e-3) / 1e9
    print("%-28s kernel %8.3f ms (%d launch), call %8.3f ms, %10.0f items/s (kernel), %5d products/item, %6.1f G products/s = %.2f of the chain rate"
          % (label, ms, launches, wall, n / (ms * 1e-3), prod, rate, rate / chain))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain", type=float, required=True, help="product-chain rate of the same session in G products/s")
    ap.add_argument("--log-n", type=int, default=16)
    a = ap.parse_args()
    n = 1 << a.log_n
    L = J._lib()
    print("n = 2^%d, %s, chain rate %.2f G products/s" % (a.log_n, L.zk_version().decode(), a.chain))
    rng = np.random.default_rng(5)
    p = tile(JC.random_points(64, 43), n)
    k = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    out = np.zeros((n, 8), dtype=np.uint64)
    run("scalar multiplication", "k_jj_scalar_mul", n, a.chain, lambda: P._check(L.zk_jj_scalar_mul(P._p64(p), P._p64(k), C.c_uint32(n), 0, P._p64(out))))
    run("point addition", "k_jj_point_op", n, a.chain, lambda: P._check(L.zk_jj_point_op(0, P._p64(p), P._p64(p), C.c_uint32(n), 0, P._p64(out))))
    with J.PedersenHasher(b"test", 3 * 254) as h:
        win = rng.integers(0, 8, size=(n, 254), dtype=np.uint8)
        run("Pedersen hash, 254 windows", "k_jj_pedersen", n, a.chain, lambda: P._check(L.zk_pedersen_hash(h._h, ptr(win), None, 254, n, ptr(out))))
    for scheme in ("mimc", "pure", "hash"):
        prng = random.Random(8)
        t0 = time.perf_counter()
        signed = [JC.sign(scheme, JC.make_msg(scheme, 3, prng), prng.randrange(1, JC.L)) for _ in range(64)]
        t_sign = (time.perf_counter() - t0) / 64
        t0 = time.perf_counter()
        assert all(JC.verify(scheme, x, sig, m) for x, sig, m in signed[:8])
        t_ver = (time.perf_counter() - t0) / 8
        A = tile([x for x, _, _ in signed], n)
        R = tile([sig[0] for _, sig, _ in signed], n)
        s = np.ascontiguousarray(np.tile(F.ints_to_limbs([sig[1] for _, sig, _ in signed]), (n // 64, 1)))
        if scheme == "mimc":
            m = np.ascontiguousarray(np.tile(F.ints_to_limbs([x for _, _, msg in signed for x in msg]).reshape(64, -1), (n // 64, 1)))
        else:
            m = np.ascontiguousarray(np.tile(np.frombuffer(b"".join(msg for _, _, msg in signed), dtype=np.uint8).reshape(64, 3), (n // 64, 1)))
        verdicts = np.zeros(n, dtype=np.uint8)
        with J.EdDSAVerifier(scheme, msg_len=3) as v:
            run("EdDSA verify, %s" % scheme, scheme, n, a.chain, lambda: P._check(L.zk_eddsa_verify_batch(v._h, ptr(A), ptr(R), ptr(s), ptr(m), n, ptr(verdicts))))
        assert verdicts.all()
        print("    the Python restatement on the CPU: %.2f ms per signature made, %.2f ms per verification" % (1e3 * t_sign, 1e3 * t_ver))


if __name__ == "__main__":
    main()

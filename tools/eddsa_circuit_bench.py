"""The witness fill of the MiMC-EdDSA circuit (zk_eddsa_fill_witnesses, csrc/jubjub.hpp k_eddsa_fill) on the device: kernel time by the library's
event pairs after a warm-up call at n = 1, 32, 1 024 and 2^14, the field products per witness from the formulas, the fraction of a product-chain
rate (tools/mulbench, "mul chain 8 waves/SIMD", passed as --chain in G/s) that the kernel reaches, the time of submit_batch + collect for the
same k on the same circuit, and the front end's generate_r1cs_witness per signature on the CPU.  Prints the table and, with --out, also writes it to that file: profiles/eddsa_circuit.txt is such a run.
--scheme pure measures the PureEdDSA circuit instead (zk_eddsa_fill_pure_witnesses, k_eddsa_fill_pure; msg_len in bytes); profiles/eddsa_pure_circuit.txt
holds both schemes from one session.  --scheme hash measures the EdDSA circuit that hashes the message first (zk_eddsa_fill_hash_witnesses,
k_eddsa_fill_hash); profiles/eddsa_hash_circuit.txt holds it beside the pure scheme, one session.
--lanes 2 or 4 (scheme mimc) measures zk_eddsa_fill_witnesses_wide (k_eddsa_fill_wide: that many lanes per signature) and prints, from the same
formulas, the products per role and phase and the critical path of its partition; profiles/eddsa_circuit_wide.txt holds lanes 1, 2 and 4 from
one session (--repeat 7: the median of seven timed calls per size with the smallest and the largest; --append: several runs into one --out file).

    python tools/eddsa_circuit_bench.py --chain 142.4 --out profiles/eddsa_circuit.txt
    python tools/eddsa_circuit_bench.py --scheme pure --chain 142.4
    python tools/eddsa_circuit_bench.py --scheme hash --chain 142.4
    python tools/eddsa_circuit_bench.py --lanes 4 --chain 142.4
"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ethsnarks_amd import fields as F, jubjub as J, prover as P   # noqa: E402
import jubjub_cases as JC                                         # noqa: E402

INV = 254 + bin(F.FR - 2).count("1")                               # jj_inv: a squaring per bit, a product per set bit
DBL, DBL_T, ADD, MIXED, CURVE = 8, 9, 10, 9, 5


def products(msg_len):
    """field products of one lane of k_eddsa_fill, part by part"""
    steps, fixed, parked = 253, 126, 3 + 126 + 2 * 253 + 1
    return {
        "inputs: conversions, two curve equations": 4 + 2 * CURVE + msg_len,
        "MiMC, (4 + m) x 91 x 4, and t": (4 + msg_len) * 91 * 4 + 1,
        "validator: three doublings, x of 8 R": 1 + 3 * (DBL + 1) + 1,
        "fixed base: 126 mixed additions": 1 + fixed * (MIXED + 1),
        "variable base: 253 x (doubling, d T, addition), R + t A": 2 + steps * (DBL_T + 1 + 1 + ADD + 1) + 2 + MIXED + 1,
        "the inversion": INV,
        "the way back: 4 per parked point, 3 for 1 / x": 4 * parked + 3,
        "gadget products: 5 per doubler, 5 per adder, xx, yy": 5 * (3 + steps) + 5 * (fixed + steps + 1) + 2,
    }


def wide_cut(lanes):
    """WideCut<lanes> of csrc/jubjub.hpp: (the last step of each variable-base segment, the role that owns segment 0 (validator, x of 8 R, fixed
    base), 1, 2, ..)"""
    return ((84, 169, 253), (1, 0, 2, 3)) if lanes == 4 else ((94, 253), (1, 1, 0))


def products_wide(msg_len, lanes):
    """field products of k_eddsa_fill_wide<lanes>, per phase and role, from the parts of products(): {phase: [products of role 0, 1, ..]}.  The
    critical path is the sum over the phases of the busiest role: the phases are separated by barriers"""
    p = products(msg_len)
    steps, fixed = 253, 126
    ends, owner = wide_cut(lanes)
    nseg = len(owner)
    valid = 4 + 2 * CURVE                                           # every role converts A and R and checks both curve equations itself
    forward = [valid] * lanes
    forward[0] += msg_len + p["MiMC, (4 + m) x 91 x 4, and t"] + p["variable base: 253 x (doubling, d T, addition), R + t A"]
    forward[1] += p["validator: three doublings, x of 8 R"] + p["fixed base: 126 mixed additions"]
    first = (1,) + tuple(e + 1 for e in ends[:-1])
    seg = [4 * (3 + fixed) + 3] + [4 * 2 * (e - f + 1) for f, e in zip(first, ends)]     # the way back of each segment
    seg[-1] += 4                                                    # the closing adder
    assert sum(seg) == p["the way back: 4 per parked point, 3 for 1 / x"]
    back = [(nseg - 1) + INV for _ in range(lanes)]                 # the product of the totals, the inversion: on every role
    for sg, role in enumerate(owner):
        back[role] += (nseg - 1) + seg[sg]                          # 1 / (its total) = 1 / (all) x the other totals, then unparking
    gadgets = []
    for role in range(lanes):
        f = fixed * (role + 1) // lanes - fixed * role // lanes
        st = steps * (role + 1) // lanes - steps * role // lanes
        gadgets.append(5 * f + 10 * st + (5 * 3 + 2 if role == lanes - 1 else 0) + (5 if role == 0 else 0))
    assert sum(gadgets) == p["gadget products: 5 per doubler, 5 per adder, xx, yy"]
    return {"forward: role 0 MiMC and the variable base, role 1 validator and fixed base": forward,
            "way back: totals, the inversion on every role, own segments": back,
            "gadget products: adders and steps split evenly": gadgets}


def products_pure(msg_len):
    """field products of one lane of k_eddsa_fill_pure, part by part.  A segment of m windows: forward 1 (x y) + 9 (m - 1) mixed additions + m
    (the running product) + 3 (m - 2) + 2 (the denominators E); back 2 m + 1 (lambda of the first adder) + 10 (m - 2) + 9 (the last, with the
    converter)"""
    steps, fixed = 253, 126
    W = (508 + 8 * msg_len + 2) // 3
    lone = 1 if W % 62 == 1 else 0
    seg = [min(62, W - lone - j) for j in range(0, W - lone, 62)]
    n_ed = len(seg) + lone - 1
    return {
        "inputs: conversions, two curve equations": 4 + 2 * CURVE,
        "validator: three doublings, x of 8 R": 1 + 3 * (DBL + 1) + 1,
        "fixed base: 126 mixed additions": 1 + fixed * (MIXED + 1),
        "hash, forward: %d windows in %d segments, 13 m - 12 each; %d Edwards additions" % (W, len(seg), n_ed): sum(13 * m - 12 for m in seg) + lone + n_ed * (1 + ADD + 1),
        "the first inversion": INV,
        "hash, back: 12 m - 10 a segment, 4 an Edwards addition": sum(12 * m - 10 for m in seg) + 4 * n_ed,
        "the way back of validator and fixed base": 4 * (3 + fixed) + 3,
        "Edwards adders of the hash (5 each), t": 5 * n_ed + 1,
        "variable base: 253 x (doubling, d T, addition), R + t A": 2 + steps * (DBL_T + 1 + 1 + ADD + 1) + 2 + MIXED + 1,
        "the second inversion": INV,
        "its way back: 4 per parked point": 4 * (2 * steps + 1),
        "gadget products: 5 per doubler, 5 per adder, xx, yy": 5 * (3 + steps) + 5 * (fixed + steps + 1) + 2,
    }


def hash_walk(W):
    """one in-circuit Pedersen hash of W windows as products_pure counts it: (segments, Edwards additions, forward, back, closing products)"""
    lone = 1 if W % 62 == 1 else 0
    seg = [min(62, W - lone - j) for j in range(0, W - lone, 62)]
    n_ed = len(seg) + lone - 1
    return seg, n_ed, sum(13 * m - 12 for m in seg) + lone + n_ed * (1 + ADD + 1), sum(12 * m - 10 for m in seg) + 4 * n_ed, 5 * n_ed + 1


def products_hash(msg_len):
    """field products of one lane of k_eddsa_fill_hash, part by part: k_eddsa_fill_pure with the message hash in front of the first inversion and
    the RAM hash, 254 windows whatever msg_len, behind an inversion of its own"""
    steps, fixed = 253, 126
    Wm = (8 * msg_len + 2) // 3
    mseg, m_ed, m_fwd, m_back, m_close = hash_walk(Wm)
    rseg, r_ed, r_fwd, r_back, r_close = hash_walk(254)
    return {
        "inputs: conversions, two curve equations": 4 + 2 * CURVE,
        "validator: three doublings, x of 8 R": 1 + 3 * (DBL + 1) + 1,
        "fixed base: 126 mixed additions": 1 + fixed * (MIXED + 1),
        "message hash, forward: %d windows in %d segments, 13 m - 12 each; %d Edwards additions" % (Wm, len(mseg), m_ed): m_fwd,
        "the first inversion": INV,
        "message hash, back: 12 m - 10 a segment, 4 an Edwards addition": m_back,
        "the way back of validator and fixed base": 4 * (3 + fixed) + 3,
        "Edwards adders of the message hash (5 each), M.x": m_close,
        "RAM hash, forward: 254 windows in %d segments; %d Edwards additions" % (len(rseg), r_ed): r_fwd,
        "the second inversion": INV,
        "RAM hash, back": r_back,
        "Edwards adders of the RAM hash (5 each), t": r_close,
        "variable base: 253 x (doubling, d T, addition), R + t A": 2 + steps * (DBL_T + 1 + 1 + ADD + 1) + 2 + MIXED + 1,
        "the third inversion": INV,
        "its way back: 4 per parked point": 4 * (2 * steps + 1),
        "gadget products: 5 per doubler, 5 per adder, xx, yy": 5 * (3 + steps) + 5 * (fixed + steps + 1) + 2,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain", type=float, required=True, help="product-chain rate of the same session in G products/s")
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 32, 1024, 1 << 14])
    ap.add_argument("--prove-up-to", type=int, default=32, help="largest k that is also proven (submit_batch + collect)")
    ap.add_argument("--msg-len", type=int, default=1)
    ap.add_argument("--scheme", choices=["mimc", "pure", "hash"], default="mimc")
    ap.add_argument("--lanes", type=int, choices=[1, 2, 4], default=1, help="lanes per signature (scheme mimc): 1 = k_eddsa_fill, 2 / 4 = k_eddsa_fill_wide")
    ap.add_argument("--repeat", type=int, default=1, help="timed calls per size: the median is reported, with the smallest and the largest")
    ap.add_argument("--out", help="also write every printed line to this file")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    a = ap.parse_args()
    if a.lanes != 1 and a.scheme != "mimc":
        ap.error("--lanes: only the mimc scheme has a fill with several lanes per signature")
    out = open(a.out, "a" if a.append else "w") if a.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    L = J._lib()
    parts = {"mimc": products, "pure": products_pure, "hash": products_hash}[a.scheme](a.msg_len)
    n_inv = {"mimc": 1, "pure": 2, "hash": 3}[a.scheme]
    total = sum(parts.values())
    emit("%s, scheme %s, lanes %d, chain rate %.2f G products/s, msg_len %d" % (L.zk_version().decode(), a.scheme, a.lanes, a.chain, a.msg_len))
    for label, v in parts.items():
        emit("    %6d  %s" % (v, label))
    emit("    %6d  products per witness on one lane, %d inversion%s" % (total, n_inv, "s" if n_inv > 1 else ""))
    if a.lanes > 1:
        wide = products_wide(a.msg_len, a.lanes)
        for label, roles in wide.items():
            emit("    %6d  %s: %s" % (max(roles), label, " | ".join("%d" % r for r in roles)))
        emit("    %6d  critical path of %d lanes (the busiest role of each phase; 2 barriers), %.3f of one lane's" % (
            sum(max(r) for r in wide.values()), a.lanes, sum(max(r) for r in wide.values()) / total))
        total = sum(sum(r) for r in wide.values())
        emit("    %6d  products per witness over all lanes (every role checks the inputs and inverts for itself)" % total)
    prng = random.Random(8)
    signed = [JC.sign(a.scheme, JC.make_msg(a.scheme, a.msg_len, prng), prng.randrange(1, JC.L)) for _ in range(32)]
    signed = [(A, (R, s % (1 << 254)), m) for A, (R, s), m in signed]
    with J.EdDSAVerifier(a.scheme, msg_len=a.msg_len) as v:
        r, lay = {"mimc": v.circuit, "pure": v.pedersen_circuit, "hash": v.hash_circuit}[a.scheme]()
        c = {"mimc": v._circuit, "pure": v._pedersen_circuit, "hash": v._hash_circuit}[a.scheme]
        fill = {"mimc": (lambda *x: v.fill_witnesses(*x, lanes=a.lanes)) if a.lanes > 1 else v.fill_witnesses, "pure": v.fill_pedersen_witnesses, "hash": v.fill_hash_witnesses}[a.scheme]
        want = [JC.verify(a.scheme, x[0], x[1], x[2]) for x in signed]
        t0 = time.perf_counter()
        for A, (R, s), m in signed[:8]:
            c.assign(A, R, s, m)
        t_front = (time.perf_counter() - t0) / 8
        emit("circuit: %d variables, %d constraints, domain 2^%d, a row of %.1f KB; the front end's generate_r1cs_witness: %.1f ms per signature on the CPU"
              % (r.V, r.nC, r.domain_size.bit_length() - 1, 32 * (r.V + 1) / 1024, 1e3 * t_front))
        pk, _ = P.keygen(r, seed=41)
        for n in a.sizes:
            items = [signed[i % 32] for i in range(n)]
            A, sigs, msgs = [x[0] for x in items], [x[1] for x in items], [x[2] for x in items]
            buf = P.DeviceBuffer(32 * (r.V + 1) * n)
            verdicts, _ = fill(A, sigs, msgs, buf)                       # warm-up: code object, scratch
            runs = []
            for _ in range(max(a.repeat, 1)):
                P.profile_begin()
                t0 = time.perf_counter()
                verdicts, _ = fill(A, sigs, msgs, buf)
                wall = 1e3 * (time.perf_counter() - t0)
                ms, launches, _ = P.profile_end()
                runs.append((ms, wall))
            runs.sort()
            ms, wall = runs[len(runs) // 2]
            rate = n * total / (ms * 1e-3) / 1e9
            line = "fill n = %6d: kernel %9.3f ms (%d launch), call %9.3f ms, %9.0f witnesses/s, %6.2f G products/s = %.3f of the chain rate" % (
                n, ms, launches, wall, n / (ms * 1e-3), rate, rate / a.chain)
            if len(runs) > 1:
                line += " (median of %d: %.3f .. %.3f ms)" % (len(runs), runs[0][0], runs[-1][0])
            assert sum(verdicts) == sum(want) * (n // 32) + sum(want[:n % 32])
            if n <= a.prove_up_to:
                ctx = P.ProverContext(pk, r, max_batch=n)
                ctx.submit_batch(None, device_ptr=buf.ptr, k=n)
                ctx.collect_batch(n)                                     # warm-up
                t0 = time.perf_counter()
                ctx.submit_batch(None, device_ptr=buf.ptr, k=n)
                ctx.collect_batch(n)
                line += "; submit_batch + collect %9.3f ms" % (1e3 * (time.perf_counter() - t0))
                ctx.close()
            emit(line)
            buf.free()
    if out:
        out.close()


if __name__ == "__main__":
    main()

"""The C++ Poseidon layer (FifthPower_gadget, Poseidon128, poseidon() of include/ethsnarks_hip/gadgets.hpp; MerkleTreeHIP with width and hasher of
include/ethsnarks_hip/merkle.hpp) compiled against the CPU emulation build: tests/cpp/poseidon_test.cpp.  The gadget and the depth-3 membership
circuit must be the same R1CS and witness as the Python front end's, two independent restatements of src/gadgets/poseidon.hpp.
test_poseidon_gpu.py runs the tree part of the same program against libzkhip.so."""
import os
import subprocess
import pytest
from ethsnarks_amd import gadgets as G, r1cs as R, fields as F
import merkle_cases as MC
import poseidon_cases as PC
from test_poseidon_emul import emul_merkle  # noqa: F401  (fixture)

TREES = [(2, 3, 5), (3, 2, 4), (4, 2, 16)]                         # width, depth, leaves: placeholders at widths 2 and 3, a full tree at width 4


def compile_cpp(tmp, libdir, libs, rpaths):
    from conftest import ROOT
    exe = os.path.join(str(tmp), "poseidon_test")
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "poseidon_test.cpp"), "-o", exe, "-L" + libdir, "-L" + os.path.join(ROOT, "tests", "emul")] +
                       ["-l" + l for l in libs] + ["-Wl,-rpath," + r for r in rpaths], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def tree_args(width, depth, n):
    leaves = MC.random_leaves(n, 980 + width)
    return ["tree", str(width), str(depth), str(PC.PyTree(depth, width, leaves).root)] + [str(v) for v in leaves]


def run_trees(exe):
    for shape in TREES:
        p = subprocess.run([exe] + tree_args(*shape), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.strip() == "PTREE OK", (shape, p.stdout + p.stderr)


@pytest.fixture(scope="module")
def exe(emul_merkle, tmp_path_factory):  # noqa: F811
    from conftest import ROOT
    d, e = os.path.dirname(emul_merkle), os.path.join(ROOT, "tests", "emul")
    return compile_cpp(tmp_path_factory.mktemp("poseidon_cpp"), d, ["zkhip_emul_merkle", "zkhip_emul"], [d, e])


def _rows(csr):
    out = []
    for row in csr.to_rows():
        d = {}
        for i, c in row:
            d[i] = (d.get(i, 0) + c) % F.FR
        out.append({i: c for i, c in d.items() if c})
    return out


def same_circuit(rj, wj, r_py, w_py):
    r_cpp = R.r1cs_from_json(open(rj).read())
    w_cpp = R.witness_from_json(open(wj).read())
    assert (r_cpp.nC, r_cpp.nIn, r_cpp.V) == (r_py.nC, r_py.nIn, r_py.V)
    assert w_cpp == [int(v) for v in w_py]
    for a, b in ((r_cpp.A, r_py.A), (r_cpp.B, r_py.B), (r_cpp.C, r_py.C)):
        assert _rows(a) == _rows(b)


def test_pinned_values_and_gadget_shapes_in_cpp(exe):
    p = subprocess.run([exe, "kat"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "OK", p.stdout + p.stderr


def test_cpp_and_python_build_the_same_gadget(exe, tmp_path):
    rj, wj = str(tmp_path / "r1cs.json"), str(tmp_path / "witness.json")
    p = subprocess.run([exe, "dump_gadget", rj, wj], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    pb = G.Protoboard()
    g = G.PoseidonGadget(pb, pb.allocate_array(2, [1, 2]))
    g.generate_r1cs_witness(); g.generate_r1cs_constraints()
    r_py, w_py = pb.to_r1cs()
    assert r_py.nC == 316 and w_py[-1] == PC.HASH_1_2
    same_circuit(rj, wj, r_py, w_py)


def test_cpp_and_python_build_the_same_membership_circuit(exe, tmp_path):
    leaves = MC.random_leaves(6, 71)
    ref = PC.PyTree(3, 2, leaves)
    for i in (0, 5):                                               # 5: a placeholder on its path
        rj, wj = str(tmp_path / ("r1cs%d.json" % i)), str(tmp_path / ("witness%d.json" % i))
        p = subprocess.run([exe, "dump_circuit", rj, wj, str(i), str(leaves[i])] + [str(v) for v in ref.path(i)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        r_py, w_py, root = G.poseidon_membership_circuit(3, leaf=leaves[i], address=i, path=ref.path(i))
        assert r_py.nC == 322 * 3 + 1 and root == ref.root
        same_circuit(rj, wj, r_py, w_py)


def test_cpp_wrapper_with_the_poseidon_hasher_on_the_emulation(exe):
    run_trees(exe)

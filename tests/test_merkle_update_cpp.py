"""The C++ front end's MerkleTreeHIP::update_seq (include/ethsnarks_hip/merkle.hpp) compiled against the CPU emulation build:
tests/cpp/merkle_update_test.cpp applies the depth-3 update sequence of merkle_update_cases.shapes_case through the wrapper, checks rows, buffer and
refusals by itself, and prints the roots, which must be the PyTree chain's and those of MerkleTree.update_seq.  test_merkle_update_gpu.py runs the
same program against libzkhip.so."""
import os
import subprocess
import pytest
import merkle_update_cases as UC
import merkle_update_checks as chk
from test_full_witness_emul import emul_merkle, zk, M  # noqa: F401  (fixtures)


def compile_cpp(tmp, libdir, libs, rpaths):
    from conftest import ROOT
    exe = os.path.join(str(tmp), "merkle_update_test")
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "merkle_update_test.cpp"), "-o", exe, "-L" + libdir, "-L" + os.path.join(ROOT, "tests", "emul")] +
                       ["-l" + l for l in libs] + ["-Wl,-rpath," + r for r in rpaths], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def run_hasher(exe, M, hasher):
    """the roots the program prints are the PyTree chain's and the Python binding's"""
    case = UC.shapes_case()
    ref = UC.reference(hasher, case)
    args = [hasher, str(case.depth), str(len(case.leaves)), str(len(case.indices))] + [str(v) for v in case.leaves]
    for a, y in zip(case.indices, case.values):
        args += [str(a), str(y)]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    lines = p.stdout.split()
    assert p.returncode == 0 and lines[-1:] == ["OK"] and lines[-2:-1] == ["UPDATE"], (hasher, p.stdout + p.stderr)
    roots = [int(v) for v in lines[:-2]]
    assert roots == ref.roots
    t = chk.new_tree(M, hasher, case)
    assert t.update_seq(case.indices, case.values) == roots
    t.close()


@pytest.fixture(scope="module")
def exe(emul_merkle, tmp_path_factory):  # noqa: F811
    from conftest import ROOT
    d, e = os.path.dirname(emul_merkle), os.path.join(ROOT, "tests", "emul")
    return compile_cpp(tmp_path_factory.mktemp("merkle_update_cpp"), d, ["zkhip_emul_merkle", "zkhip_emul"], [d, e])


@pytest.mark.parametrize("hasher", UC.HASHERS)
def test_cpp_update_seq_gives_the_python_roots(exe, M, hasher):  # noqa: F811
    run_hasher(exe, M, hasher)

"""The C++ front end's MerkleTreeHIP::fill_full_witnesses (include/ethsnarks_hip/merkle.hpp) compiled against the CPU emulation build:
tests/cpp/full_witness_test.cpp compares the rows the device wrote with the witness of the C++ gadgets of gadgets.hpp, byte for byte, for both
hashers at depth 3.  test_full_witness_gpu.py runs the same program against libzkhip.so."""
import os
import subprocess
import pytest
import merkle_cases as MC
from test_full_witness_emul import emul_merkle  # noqa: F401  (fixture)

DEPTH, LEAVES = 3, 7                                               # 7 of 8 leaves: a placeholder on the path of the last one


def compile_cpp(tmp, libdir, libs, rpaths):
    from conftest import ROOT
    exe = os.path.join(str(tmp), "full_witness_test")
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "full_witness_test.cpp"), "-o", exe, "-L" + libdir, "-L" + os.path.join(ROOT, "tests", "emul")] +
                       ["-l" + l for l in libs] + ["-Wl,-rpath," + r for r in rpaths], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def run_hasher(exe, hasher):
    leaves = MC.random_leaves(LEAVES, 990)
    p = subprocess.run([exe, hasher, str(DEPTH)] + [str(v) for v in leaves], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "FULL OK", (hasher, p.stdout + p.stderr)


@pytest.fixture(scope="module")
def exe(emul_merkle, tmp_path_factory):  # noqa: F811
    from conftest import ROOT
    d, e = os.path.dirname(emul_merkle), os.path.join(ROOT, "tests", "emul")
    return compile_cpp(tmp_path_factory.mktemp("full_witness_cpp"), d, ["zkhip_emul_merkle", "zkhip_emul"], [d, e])


@pytest.mark.parametrize("hasher", ["mimc", "poseidon"])
def test_cpp_fill_full_witnesses_equals_the_cpp_gadgets(exe, hasher):
    run_hasher(exe, hasher)

"""The C++ adapter of the device Merkle tree (include/ethsnarks_hip/merkle.hpp) compiled against the CPU emulation build: tests/cpp/merkle_tree_test.cpp
on the reference's depth-29 known answers.  test_merkle_gpu.py runs the same program against libzkhip.so."""
import os
import subprocess
import merkle_cases as MC
from test_merkle_emul import emul_merkle  # noqa: F401  (fixture)


def cpp_args():
    return ["%064x" % v for v in (MC.ITEM_A, MC.ITEM_B, MC.KNOWN29_ROOT_ONE, MC.KNOWN29_ROOT_TWO, MC.KNOWN29_NODES[(13, 1)])]


def compile_cpp(tmp_path, libdir, libs, rpaths):
    from conftest import ROOT
    exe = str(tmp_path / "merkle_tree_test")
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "merkle_tree_test.cpp"), "-o", exe, "-L" + libdir, "-L" + os.path.join(ROOT, "tests", "emul")] + ["-l" + l for l in libs] +
                       ["-Wl,-rpath," + r for r in rpaths], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_cpp_wrapper_on_the_emulation(emul_merkle, tmp_path):  # noqa: F811
    from conftest import ROOT
    d, e = os.path.dirname(emul_merkle), os.path.join(ROOT, "tests", "emul")
    exe = compile_cpp(tmp_path, d, ["zkhip_emul_merkle", "zkhip_emul"], [d, e])
    p = subprocess.run([exe] + cpp_args(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "MTREE OK", p.stdout + p.stderr

"""The SEAL-free adapter (include/pasta_seal_gfx950.hpp) on levels, driven from C++ (tests/cpp/mod_switch_main.cpp):
get_cipher_size(ct), (ct, true, 0) and (ct, true, 1) shrink the saved object by the ratio of the limb counts, `decrypting` works on
the switched ciphertexts, an out-of-range levels_from_last throws.  The words the driver wrote equal the definition of
tests/mod_switch_common.py.  On the CPU against the tests-only emulator library and, marked gpu, against libhhe_gfx950.so."""
import os
import subprocess

import numpy as np
import pytest

import mod_switch_common as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LOGN, BITS = 65537, 10, [50] * 5
HEADER = 16 + 32 + 1 + 40 + 16 + 8


def drive(orc, tmp_path, libdir, libname):
    n = 1 << LOGN
    q = orc.coeff_modulus_create(n, BITS)
    K, L = len(q), len(q) - 1
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        np.array([LOGN, K, T], dtype=np.uint64).tofile(f)
        np.array(q, dtype=np.uint64).tofile(f)
    exe = tmp_path / "mod_switch"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mod_switch_main.cpp"), "-L" + libdir, "-l" + libname,
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    sizes = [HEADER + 2 * l * n * 8 for l in (L, 2, 1)]
    assert "sizes: %d %d %d\n" % tuple(sizes) in r.stdout
    assert (sizes[0] - HEADER) == L * (sizes[2] - HEADER) and (sizes[1] - HEADER) == 2 * (sizes[2] - HEADER)
    w = np.fromfile(out, dtype=np.uint64)
    top = w[K * n:][:2 * L * n].reshape(2, L, n)
    second = w[(K + 2 * L) * n:][:4 * n].reshape(2, 2, n)
    last = w[(K + 2 * L + 4) * n:].reshape(2, 1, n)
    truth = ms.chain(top, q)
    assert (second == truth[2]).all() and (last == truth[1]).all()
    return r.stdout


def test_cpp_mod_switch_on_emulator(orc, emu_lib, tmp_path):
    assert "emulator" in drive(orc, tmp_path, os.path.join(ROOT, "tests", "emu"), "hhe_emu")


@pytest.mark.gpu
def test_cpp_mod_switch_on_gfx950(orc, tmp_path):
    assert "hip-gfx950" in drive(orc, tmp_path, os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950")

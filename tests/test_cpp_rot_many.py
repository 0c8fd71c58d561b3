"""Hoisted rotations and the packed encrypted FC with a hoisted chain through the SEAL-free adapter (include/pasta_seal_gfx950.hpp),
driven from C++ (tests/cpp/rot_many_main.cpp): keygen on the device including a key for each of 1 .. r-1, rotate_rows_many (member and
sealhelper:: free function), fc_packed_hoisted, decrypting, the same on SEALZpCipher::level(3), the refusals.  The driver checks every
rotation and the ten slots against plain integers itself; its results are decrypted again here through the Python binding of the same
library and compared with Python integers.  The SEAL-typed form of the same calls is type-checked against the reference's headers.
On the CPU against the tests-only emulator library and, marked gpu, against libhhe_gfx950.so."""
import os
import subprocess

import numpy as np
import pytest

import parity_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LOGN, BITS, LEVELS_FROM_LAST = 65537, 10, [50] * 9, 3
ROWS, COLS = 10, 256


def drive(orc, api, lib, mem, tmp_path, libdir, libname):
    n = 1 << LOGN
    q = orc.coeff_modulus_create(n, BITS)
    K, l = len(q), LEVELS_FROM_LAST + 1
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        np.array([LOGN, K, T, LEVELS_FROM_LAST], dtype=np.uint64).tofile(f)
        np.array(q, dtype=np.uint64).tofile(f)
    exe, out = tmp_path / "rot_many_main", tmp_path / "out.bin"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "rot_many_main.cpp"),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", str(exe)])
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    w = np.fromfile(out, dtype=np.uint64)
    L = K - 1
    ctw = 2 * L * n
    sk = w[:K * n].reshape(K, n)
    top = w[K * n:K * n + ctw].reshape(1, 2, L, n)
    low = w[K * n + ctw:K * n + ctw + 2 * l * n].reshape(1, 2, l, n)
    rot17 = w[K * n + ctw + 2 * l * n:].reshape(1, 2, L, n)
    # the driver's weights and record, restated
    pt = [(7 * i + 3) % 256 for i in range(COLS)]
    M = [[((31 * r + 17 * c + 1) % 17 - 8) % T for c in range(COLS)] for r in range(ROWS)]
    want = [sum(M[r][c] * pt[c] for c in range(COLS)) % T for r in range(ROWS)]
    X = api.Context(LOGN, q, T, lib=lib)
    vals = mem.empty((1, n))
    X.decrypt(sk, mem.to_dev(top), 1, vals)
    assert [int(v) for v in mem.to_host(vals)[0, :ROWS]] == want
    assert int(X.noise_budget(sk, mem.to_dev(top), 1)[0]) > 0
    X.decrypt_level(sk, mem.to_dev(low), l, 1, vals)
    assert [int(v) for v in mem.to_host(vals)[0, :ROWS]] == want
    budget = int(X.noise_budget(sk, mem.to_dev(low), 1, limbs=l)[0])
    assert budget > 0 and ("noise budget: %d" % budget) in r.stdout.splitlines()
    X.decrypt(sk, mem.to_dev(rot17), 1, vals)   # rotate_rows(x, 17): slot i <- slot i + 17
    assert [int(v) for v in mem.to_host(vals)[0, :COLS]] == pt[17:] + [0] * 17
    X.close()
    return r.stdout.splitlines()[-1]


def test_cpp_rot_many_on_emulator(orc, api, emu_lib, tmp_path):
    assert "emulator" in drive(orc, api, emu_lib, pc.HostMem(), tmp_path, os.path.join(ROOT, "tests", "emu"), "hhe_emu")


REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "libs/seal/include/SEAL-4.0")), reason="reference headers not present")
def test_seal_typed_rot_many_type_checks_against_the_reference_headers():
    """SEALZpCipher::rotate_rows_many, sealhelper::rotate_rows_many / fc_packed_hoisted and SEALZpLevel::rotate_rows_many /
    fc_packed_hoisted in include/pasta_seal_gfx950_seal.hpp: type-checked only, as the rest of that header"""
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable",
           "-I" + os.path.join(REF, "libs/seal/include/SEAL-4.0"), "-I" + os.path.join(REF, "src/pasta"),
           "-I" + os.path.join(REF, "libs/keccak"), "-I" + os.path.join(REF, "libs/keccak/opt64"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/cpp/seal_rot_many_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.gpu
def test_cpp_rot_many_on_gfx950(orc, api, tmp_path):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    assert "hip-gfx950" in drive(orc, api, lib, pc.TorchMem("cuda:0"), tmp_path,
                                 os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950")

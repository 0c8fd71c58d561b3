"""The chainable packed FC and the FC-square-FC network through the SEAL-free adapter (include/pasta_seal_gfx950.hpp), driven from C++
(tests/cpp/mlp_main.cpp): keygen on the device, a two-layer model (6 x 256, 3 x 6) of encrypted open diagonals, one decomposition of a
two-block record, flatten, sealhelper::mlp and the members, fc_open + packed_square + fc_open by hand, the refusals.  The driver checks
the three slots itself; its results are decrypted again here through the Python binding of the same library and compared with Python
integers.  The SEAL-typed form of the same calls is type-checked against the reference's headers.  On the CPU against the tests-only
emulator library and, marked gpu, against libhhe_gfx950.so."""
import os
import subprocess

import numpy as np
import pytest

import parity_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LOGN, BITS = 65537, 10, [50] * 9


def _weights(rows, cols, salt):
    return [[((31 * r + 17 * c + salt) % 17 - 8) % T for c in range(cols)] for r in range(rows)]


def drive(orc, api, lib, mem, tmp_path, libdir, libname):
    n = 1 << LOGN
    q = orc.coeff_modulus_create(n, BITS)
    K = len(q)
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        np.array([LOGN, K, T], dtype=np.uint64).tofile(f)
        np.array(q, dtype=np.uint64).tofile(f)
    exe, out = tmp_path / "mlp_main", tmp_path / "out.bin"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mlp_main.cpp"),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", str(exe)])
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    w = np.fromfile(out, dtype=np.uint64)
    L = K - 1
    ctw = 2 * L * n
    sk = w[:K * n].reshape(K, n)
    cts = w[K * n:].reshape(2, 2, L, n)   # the network's result, the first layer's
    # the driver's model and record, restated
    pt = [(7 * i + 3) % 4 for i in range(256)]
    M1, M2 = _weights(6, 256, 1), _weights(3, 6, 5)
    y1 = [sum(M1[i][j] * pt[j] for j in range(256)) % T for i in range(6)]
    want = [sum(M2[i][j] * (y1[j] * y1[j] % T) for j in range(6)) % T for i in range(3)]
    X = api.Context(LOGN, q, T, lib=lib)
    vals = mem.empty((2, n))
    X.decrypt(sk, mem.to_dev(cts), 2, vals)
    got = mem.to_host(vals)
    assert [int(v) for v in got[0, :3]] == want
    assert [int(v) for v in got[1, :6]] == y1
    budgets = [int(v) for v in X.noise_budget(sk, mem.to_dev(cts), 2)]
    assert min(budgets) > 0 and ("noise budget: %d" % budgets[0]) in r.stdout.splitlines()
    X.close()
    assert w.size == K * n + 2 * ctw
    return r.stdout.splitlines()[-1]


def test_cpp_mlp_on_emulator(orc, api, emu_lib, tmp_path):
    assert "emulator" in drive(orc, api, emu_lib, pc.HostMem(), tmp_path, os.path.join(ROOT, "tests", "emu"), "hhe_emu")


REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "libs/seal/include/SEAL-4.0")), reason="reference headers not present")
def test_seal_typed_mlp_type_checks_against_the_reference_headers():
    """EncMatrix's open kind, SEALZpCipher::enc_matrix_open / fc_open / mlp, the level object's and sealhelper::fc_open / mlp in
    include/pasta_seal_gfx950_seal.hpp: type-checked only, as the rest of that header"""
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable",
           "-I" + os.path.join(REF, "libs/seal/include/SEAL-4.0"), "-I" + os.path.join(REF, "src/pasta"),
           "-I" + os.path.join(REF, "libs/keccak"), "-I" + os.path.join(REF, "libs/keccak/opt64"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/cpp/seal_mlp_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.gpu
def test_cpp_mlp_on_gfx950(orc, api, tmp_path):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    assert "hip-gfx950" in drive(orc, api, lib, pc.TorchMem("cuda:0"), tmp_path,
                                 os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950")

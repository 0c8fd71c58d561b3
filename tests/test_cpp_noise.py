"""The SEAL-free adapter (include/pasta_seal_gfx950.hpp) on the noise budget, driven from C++ (tests/cpp/noise_main.cpp): the three
forms of SEALZpCipher::print_noise and sealhelper::invariant_noise_budget on the encrypted PASTA key, a decomposition result, a result
switched to the last level, a size-3 product and a vector of mixed levels.  The driver's stdout is compared line by line with the
budgets hhe_noise_budget gives, through the Python binding of the same library, for the words the driver wrote; the empty vector and
the missing key throw inside the driver.  On the CPU against the tests-only emulator library and, marked gpu, against
libhhe_gfx950.so."""
import os
import subprocess

import numpy as np
import pytest

import parity_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LOGN, BITS = 65537, 10, [50] * 9


def drive(orc, api, lib, mem, tmp_path, libdir, libname):
    n = 1 << LOGN
    q = orc.coeff_modulus_create(n, BITS)
    K, L = len(q), len(q) - 1
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        np.array([LOGN, K, T], dtype=np.uint64).tofile(f)
        np.array(q, dtype=np.uint64).tofile(f)
    exe = tmp_path / "noise"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "noise_main.cpp"), "-L" + libdir, "-l" + libname,
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    w = np.fromfile(out, dtype=np.uint64)
    pos = 0

    def take(shape):
        nonlocal pos
        cnt = int(np.prod(shape))
        v = w[pos:pos + cnt].reshape(shape)
        pos += cnt
        return v
    sk, key, b0, b1, last, prod = take((K, n)), take((2, L, n)), take((2, L, n)), take((2, L, n)), take((2, 1, n)), take((3, L, n))
    assert pos == len(w)
    X = api.Context(LOGN, q, T, lib=lib)
    abi = lambda words, size, limbs: [int(v) for v in X.noise_budget(sk, mem.to_dev(words), words.shape[0], size, limbs)]
    (k,), (x0, x1), (xl,), (xp,) = abi(key[None], 2, L), abi(np.stack([b0, b1]), 2, L), abi(last[None], 2, 1), abi(prod[None], 3, L)
    assert k > max(x0, x1) and min(x0, x1) > xl > 0 and k > xp > 0, (k, x0, x1, xl, xp)   # the budgets tell the cases apart
    mixed = [x1, xl, xp, x0]
    want = ["min noise budget: %d" % k, "max noise budget: %d" % k, "returned: %d" % k,
            "min noise budget: %d" % min(x0, x1), "max noise budget: %d" % max(x0, x1), "returned: %d" % min(x0, x1),
            "noise budget: %d" % x0, "returned: %d" % x0, "noise budget: %d" % x1, "returned: %d" % x1,
            "noise budget: %d" % xl, "returned: %d" % xl,
            "noise budget: %d" % xp, "returned: %d" % xp,
            "min noise budget: %d" % min(mixed), "max noise budget: %d" % max(mixed), "returned: %d" % min(mixed),
            "free: %d" % xl]
    lines = r.stdout.splitlines()
    assert lines[:-1] == want, (lines, want)
    return lines[-1]


def test_cpp_noise_on_emulator(orc, api, emu_lib, tmp_path):
    assert "emulator" in drive(orc, api, emu_lib, pc.HostMem(), tmp_path, os.path.join(ROOT, "tests", "emu"), "hhe_emu")


@pytest.mark.gpu
def test_cpp_noise_on_gfx950(orc, api, tmp_path):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    assert "hip-gfx950" in drive(orc, api, lib, pc.TorchMem("cuda:0"), tmp_path,
                                 os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950")

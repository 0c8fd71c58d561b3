"""The SEAL-free adapter (include/pasta_seal_gfx950.hpp) evaluating at a level, driven from C++ (tests/cpp/level_main.cpp): keygen,
encrypt_key_2, one decomposition, get_cipher_size(ct, true, k), then mask, flatten, packed_affine, packed_square, print_noise and
decrypting on SEALZpCipher::level(k).  The driver checks the slots against plain integers and the refusals itself; its printed budgets
are compared line by line with hhe_noise_budget through the Python binding of the same library, on the level's context with
level_rows(sk) and on the chain's context at `limbs`.  tests/cpp/level_lifecycle_main.cpp (the C ABI at the levels with 2 and 1 data
primes) runs as well, linked against the library instead of the emulator sources its header names for the sanitizer build.  On the CPU
against the tests-only emulator library and, marked gpu, against libhhe_gfx950.so."""
import os
import subprocess

import numpy as np
import pytest

import parity_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LOGN, BITS, LEVELS_FROM_LAST = 65537, 10, [50] * 9, 3


def build(tmp_path, source, libdir, libname):
    exe = tmp_path / os.path.splitext(source)[0]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", source),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", str(exe)])
    return str(exe)


def drive(orc, api, lib, mem, tmp_path, libdir, libname):
    n = 1 << LOGN
    q = orc.coeff_modulus_create(n, BITS)
    K, l = len(q), LEVELS_FROM_LAST + 1
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        np.array([LOGN, K, T, LEVELS_FROM_LAST], dtype=np.uint64).tofile(f)
        np.array(q, dtype=np.uint64).tofile(f)
    out = tmp_path / "out.bin"
    r = subprocess.run([build(tmp_path, "level_main.cpp", libdir, libname), str(blob), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    w = np.fromfile(out, dtype=np.uint64)
    sk, cts = w[:K * n].reshape(K, n), w[K * n:].reshape(5, 2, l, n)   # the switched block, masked, flattened, affine layer, its square
    X = api.Context(LOGN, q, T, lib=lib)
    Xl = X.at_level(l)
    d = mem.to_dev(cts)
    at_level = [int(v) for v in Xl.noise_budget(api.level_rows(sk, l), d, 5)]
    on_chain = [int(v) for v in X.noise_budget(sk, d, 5, limbs=l)]
    assert at_level == on_chain and min(at_level) > 0, (at_level, on_chain)
    assert at_level[0] > at_level[1] > at_level[3] > at_level[4], at_level   # every op costs budget: the figures tell the cases apart
    want = [s % b for b in at_level for s in ("noise budget: %d", "returned: %d")]
    lines = r.stdout.splitlines()
    assert lines[:-1] == want, (lines, want)
    return lines[-1]


def lifecycle(tmp_path, libdir, libname):
    r = subprocess.run([build(tmp_path, "level_lifecycle_main.cpp", libdir, libname)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["logn 10 ok", "logn 12 ok"]


def test_cpp_level_on_emulator(orc, api, emu_lib, tmp_path):
    assert "emulator" in drive(orc, api, emu_lib, pc.HostMem(), tmp_path, os.path.join(ROOT, "tests", "emu"), "hhe_emu")


def test_cpp_level_lifecycle_on_emulator(emu_lib, tmp_path):
    lifecycle(tmp_path, os.path.join(ROOT, "tests", "emu"), "hhe_emu")


REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "libs/seal/include/SEAL-4.0")), reason="reference headers not present")
def test_seal_typed_level_object_type_checks_against_the_reference_headers():
    """pasta::SEALZpCipher::level over parms_id in include/pasta_seal_gfx950_seal.hpp: type-checked only, as the rest of that header"""
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable",
           "-I" + os.path.join(REF, "libs/seal/include/SEAL-4.0"), "-I" + os.path.join(REF, "src/pasta"),
           "-I" + os.path.join(REF, "libs/keccak"), "-I" + os.path.join(REF, "libs/keccak/opt64"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/cpp/seal_level_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.gpu
def test_cpp_level_on_gfx950(orc, api, tmp_path):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    assert "hip-gfx950" in drive(orc, api, lib, pc.TorchMem("cuda:0"), tmp_path,
                                 os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950")


@pytest.mark.gpu
def test_cpp_level_lifecycle_on_gfx950(api, tmp_path):
    api.load_library()
    lifecycle(tmp_path, os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950")

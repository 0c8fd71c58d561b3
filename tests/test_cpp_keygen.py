"""The SEAL-free adapter (include/pasta_seal_gfx950.hpp) with no key from anywhere else, driven from C++ (tests/cpp/keygen_main.cpp):
keygen, create_relin_keys, create_gk, encrypt_key_2, one decomposition, decrypting.  The keys equal the restatement of the sampler
(tests/keygen_common.py), the transciphered block equals the oracle's given the words the driver wrote, and it decrypts to the
plaintext.  On the CPU against the tests-only emulator library and, marked gpu, against libhhe_gfx950.so."""
import os
import subprocess
import types

import numpy as np
import pytest

import keygen_common as kg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LOGN, BITS, NPT = 65537, 10, [50] * 9, 100

_RUNS = {}


def _run(orc, tmp_path_factory, libdir, libname):
    if libname not in _RUNS:
        try:
            _RUNS[libname] = _drive(orc, tmp_path_factory.mktemp("keygen_" + libname), libdir, libname)
        except BaseException as e:
            _RUNS[libname] = e
    if isinstance(_RUNS[libname], BaseException):
        raise _RUNS[libname]
    return _RUNS[libname]


def _drive(orc, tmp_path, libdir, libname):
    n = 1 << LOGN
    q = orc.coeff_modulus_create(n, BITS)
    O = orc.Oracle(LOGN, q, T)
    ssk = np.array([(i * 2654435761 + 12345) % T for i in range(256)], dtype=np.uint64)
    pt = np.array([(7 * i + 3) % 256 for i in range(NPT)], dtype=np.uint64)
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        np.array([LOGN, O.K, T, NPT], dtype=np.uint64).tofile(f)
        np.array(q, dtype=np.uint64).tofile(f)
        ssk.tofile(f)
        pt.tofile(f)
    exe = tmp_path / "keygen"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "keygen_main.cpp"), "-L" + libdir, "-l" + libname,
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    w = np.fromfile(out, dtype=np.uint64)
    elts = sorted({O.galois_elt(s) for s in (0, -1, 128)})
    R = types.SimpleNamespace(stdout=r.stdout, O=O, ssk=ssk, pt=pt, elts=elts)
    pos = 0

    def take(shape):
        nonlocal pos
        cnt = int(np.prod(shape))
        v = w[pos:pos + cnt].reshape(shape)
        pos += cnt
        return v
    R.sk, R.pk, R.rk = take((O.K, n)), take((2, O.K, n)), take(O.ksk_shape)
    R.gk = {}
    for e in elts:
        assert int(take((1,))[0]) == e
        R.gk[e] = take(O.ksk_shape)
    R.enc_key, R.sym, R.block, R.vals = take(O.ct_shape), take((NPT,)), take(O.ct_shape), take((NPT,))
    assert pos == len(w)
    return R


def check(R, orc):
    O = R.O
    assert "galois keys: " + " ".join(str(e) for e in R.elts) + "\n" in R.stdout
    _, sk = kg.expected_secret(O, kg.SEED)
    assert (R.sk == sk).all()
    assert (R.pk == kg.expected_enc_zero(O, sk, kg.SEED, kg.PUBLIC, 0, 1)[0][0]).all()
    assert (R.rk == kg.expected_enc_zero(O, sk, kg.SEED2, kg.RELIN, 0, O.L, kg.new_key_relin(O, sk))[0]).all()
    e = R.elts[0]
    assert (R.gk[e] == kg.expected_enc_zero(O, sk, kg.SEED2, kg.GALOIS, e, O.L, kg.new_key_galois(O, sk, e))[0]).all()
    assert (R.enc_key == kg.expected_encrypt(O, R.pk, O.pasta_pack_key(R.ssk), kg.SEED2, 0)).all()
    assert (R.sym == orc.pasta_encrypt(T, R.ssk, R.pt)).all()
    gk = orc.GaloisKeys(R.elts, np.stack([R.gk[e] for e in R.elts]))
    assert (R.block == O.transcipher_block(R.enc_key, R.rk, gk, R.sym, 0)).all()
    assert (R.vals == R.pt).all()
    assert (O.decode(O.decrypt(R.sk, R.block))[:NPT] == R.pt).all()


def test_cpp_keygen_on_emulator(orc, emu_lib, tmp_path_factory):
    R = _run(orc, tmp_path_factory, os.path.join(ROOT, "tests", "emu"), "hhe_emu")
    assert "emulator" in R.stdout
    check(R, orc)


@pytest.mark.gpu
def test_cpp_keygen_on_gfx950(orc, tmp_path_factory):
    R = _run(orc, tmp_path_factory, os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950")
    assert "hip-gfx950" in R.stdout
    check(R, orc)

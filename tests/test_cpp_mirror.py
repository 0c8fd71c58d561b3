"""The C++ host-side mirror of pasta::PASTA_SEAL (include/pasta_seal_gfx950.hpp) driven like CSP.cpp:238-278:
decomposition of a multi-block record + flatten, compared with the oracle; then SEALZpCipher::mask, the FC row as the three
calls CSP.cpp:296-316 makes, and a key-set cache smaller than the number of live key objects.  Every call body the driver reaches
is include/hhe_adapter_core.hpp, the code the SEAL-typed adapter calls too.  Runs on the CPU against the tests-only emulator
library and, marked gpu, against libhhe_gfx950.so: the driver runs once per library, the tests below read its outputs."""
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import Setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_RUNS = {}


def _run(orc, tmp_path_factory, libdir, libname):
    """One run of the driver per library (a failed run is not repeated): its outputs, with the checks of the mirror itself."""
    if libname not in _RUNS:
        try:
            _RUNS[libname] = _drive(orc, tmp_path_factory.mktemp("mirror_" + libname), libdir, libname)
        except BaseException as e:
            _RUNS[libname] = e
    if isinstance(_RUNS[libname], BaseException):
        raise _RUNS[libname]
    return _RUNS[libname]


def _drive(orc, tmp_path, libdir, libname):
    S = Setup(orc, 10, [50] * 9, extra_steps=(-128, -256))
    O = S.O
    # the CSP's own key objects under the same secret key, different randomness (Analyst.cpp:70-94); -2 serves the 3-input FC row
    csp_gk = O.keygen_galois(S.sk, [int(O.galois_elt(s)) for s in (0, -1, 128, -128, -256, -2)], 808)
    csp_rk = O.keygen_relin(S.sk, 909)
    w_vals = np.array([3, 5, 7], dtype=np.uint64)
    w_row = O.encrypt(S.pk, O.encode(w_vals), 77)
    # two more analysts: RelinKeys / GaloisKeys objects of other randomness (the eviction sequence)
    more = [(O.keygen_relin(S.sk, 1000 + a), O.keygen_galois(S.sk, [int(e) for e in S.gk.elts], 2000 + a)) for a in range(2)]
    pt = np.array([(7 * i + 3) % 256 for i in range(300)], dtype=np.uint64)
    record = orc.pasta_encrypt(S.t, S.key, pt)
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        np.array([S.logn, O.K, S.t, len(S.gk.elts), len(record), 1], dtype=np.uint64).tofile(f)
        np.array(S.q, dtype=np.uint64).tofile(f)
        S.rk.tofile(f)
        for e, k in zip(S.gk.elts, S.gk.keys):
            np.array([int(e)], dtype=np.uint64).tofile(f)
            k.tofile(f)
        S.enc_key.tofile(f)
        record.tofile(f)
        np.ascontiguousarray(S.sk, dtype=np.uint64).tofile(f)
        S.key.tofile(f)
        np.asarray(pt, dtype=np.uint64).tofile(f)
        np.array([len(csp_gk.elts)], dtype=np.uint64).tofile(f)
        for e, k in zip(csp_gk.elts, csp_gk.keys):
            np.array([int(e)], dtype=np.uint64).tofile(f)
            k.tofile(f)
        csp_rk.tofile(f)
        w_row.tofile(f)
        for m_rk, m_gk in more:
            m_rk.tofile(f)
            for e, k in zip(m_gk.elts, m_gk.keys):
                np.array([int(e)], dtype=np.uint64).tofile(f)
                k.tofile(f)
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mirror_main.cpp"), "-L" + libdir, "-l" + libname,
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "throws: Galois key not present" in r.stdout
    words = np.fromfile(out, dtype=np.uint64)
    nb = int(words[0])
    assert nb == 3
    ctw = int(np.prod(O.ct_shape))
    base = 1 + (nb + 1) * ctw
    cts = words[1:base].reshape(nb + 1, *O.ct_shape)
    sq = words[base:base + ctw].reshape(O.ct_shape)
    prod = words[base + ctw:base + ctw + ctw // 2 * 3].reshape(3, O.L, O.n)
    o2 = base + ctw + ctw // 2 * 3
    ssum = words[o2:o2 + ctw].reshape(O.ct_shape)
    sym_ct, sym_back = words[o2 + ctw:o2 + ctw + len(pt)], words[o2 + ctw + len(pt):o2 + ctw + 2 * len(pt)]
    o3 = o2 + ctw + 2 * len(pt)
    dec_i64 = words[o3:o3 + 256].view(np.int64)
    # flatten with csp_gk, batched decompose x 2, FC row | masked block, three-call FC | capacity 2: square, nb blocks, flatten
    extra = words[o3 + 256:].reshape(4 + 2 + 2 + nb, *O.ct_shape)
    assert (sym_ct == record).all() and (sym_back == np.asarray(pt, dtype=np.uint64)).all()   # pasta::PASTA encrypt / decrypt
    assert "throws: Invalid Key length" in r.stdout
    assert len(dec_i64) == 256 and (dec_i64 == np.asarray(pt[:256], dtype=np.int64)).all()    # sealhelper::decrypting
    cw, ncw = S.sym_blocks(orc, pt)
    refs = [O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b) for b in range(nb)]
    for b in range(nb):
        assert (cts[b] == refs[b]).all()
    assert (sq == O.relinearize(O.multiply(refs[0], refs[0]), S.rk)).all()      # packed_square
    assert (prod == O.multiply(refs[0], refs[1])).all()                          # packed_enc_mul
    assert (ssum == O.add(refs[0], refs[1])).all()                               # packed_enc_add
    flat = O.flatten(np.stack(refs), S.gk)
    assert (cts[nb] == flat).all()
    # mask-free flatten decrypts to the record (SEAL_Cipher.cpp:170-181 semantics): first 300 slots
    dec = O.decode(O.decrypt(S.sk, cts[nb]))
    assert (dec[:256] == pt[:256]).all()
    # key objects named per call: flatten with the CSP's GaloisKeys differs from flatten with the cipher object's own, and both equal
    # the oracle called with that object; the batched decompose masks the ragged block (44 words) before flattening
    assert (extra[0] == O.flatten(np.stack(refs), csp_gk)).all() and not (extra[0] == flat).all()
    masked = list(refs)
    masked[2] = O.mask(refs[2], np.ones(44, np.uint64))
    ref_dec = O.flatten(np.stack(masked), csp_gk)
    assert (extra[1] == ref_dec).all() and (extra[2] == ref_dec).all()
    ref_fc, _ = O.fc_row(ref_dec, w_row, csp_rk, csp_gk, 3)
    assert (extra[3] == ref_fc).all()
    assert int(O.decode(O.decrypt(S.sk, extra[3]))[2]) == int(np.dot(pt[:3], w_vals)) % S.t
    # three requests built three cipher objects from the same key objects by value: 4 objects went to the device once (rk, gk, csp gk,
    # csp rk), the encrypted PASTA key once
    assert "key objects uploaded: 4, resident sets: 4, encrypted-key uploads: 1" in r.stdout, r.stdout
    return types.SimpleNamespace(stdout=r.stdout, O=O, nb=nb, refs=refs, flat=flat, sq=sq, ref_dec=ref_dec, ref_fc=ref_fc, fc_row=extra[3],
                                 masked=extra[4], fc3=extra[5], small_sq=extra[6], small_blocks=extra[7:7 + nb], small_flat=extra[7 + nb])


def _emu(orc, tmp_path_factory):
    return _run(orc, tmp_path_factory, os.path.join(ROOT, "tests", "emu"), "hhe_emu")


def _gpu(orc, tmp_path_factory):
    return _run(orc, tmp_path_factory, os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950")


def check_mask(R):
    """SEALZpCipher::mask on the ragged block: 44 ones, against the oracle's mask."""
    assert (R.masked == R.O.mask(R.refs[2], np.ones(44, np.uint64))).all()
    assert not (R.masked == R.refs[2]).all()


def check_three_call_fc(R):
    """packed_enc_multiply, relinearize_inplace(csp_rk), encrypted_vec_sum(csp_gk, 3): the oracle's FC row, and word for word what the
    one-call sealhelper::fc_row gave."""
    assert (R.fc3 == R.ref_fc).all()
    assert (R.fc3 == R.fc_row).all()


def check_eviction(R):
    """Cache capacity 2, three live cipher objects of three different RelinKeys / GaloisKeys pairs: the first object still computes
    with the first pair (the oracle called with it) although its sets left the cache; nothing was uploaded twice."""
    for b in range(R.nb):
        assert (R.small_blocks[b] == R.refs[b]).all()
    assert (R.small_sq == R.sq).all() and (R.small_flat == R.flat).all()   # R.sq, R.flat: checked against the oracle with the first pair
    assert "capacity 2: key objects uploaded: 6, resident sets: 2\n" in R.stdout, R.stdout


def test_cpp_mirror_on_emulator(orc, emu_lib, tmp_path_factory):
    assert "emulator" in _emu(orc, tmp_path_factory).stdout


def test_mask_is_executed_on_emulator(orc, emu_lib, tmp_path_factory):
    check_mask(_emu(orc, tmp_path_factory))


def test_three_call_fc_on_emulator(orc, emu_lib, tmp_path_factory):
    check_three_call_fc(_emu(orc, tmp_path_factory))


def test_eviction_keeps_sets_in_use_on_emulator(orc, emu_lib, tmp_path_factory):
    check_eviction(_emu(orc, tmp_path_factory))


@pytest.mark.gpu
def test_cpp_mirror_on_gfx950(orc, tmp_path_factory):
    assert "hip-gfx950" in _gpu(orc, tmp_path_factory).stdout


@pytest.mark.gpu
def test_mask_is_executed_on_gfx950(orc, tmp_path_factory):
    check_mask(_gpu(orc, tmp_path_factory))


@pytest.mark.gpu
def test_three_call_fc_on_gfx950(orc, tmp_path_factory):
    check_three_call_fc(_gpu(orc, tmp_path_factory))


@pytest.mark.gpu
def test_eviction_keeps_sets_in_use_on_gfx950(orc, tmp_path_factory):
    check_eviction(_gpu(orc, tmp_path_factory))

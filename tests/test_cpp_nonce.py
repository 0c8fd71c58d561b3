"""The SEAL-free adapter (include/pasta_seal_gfx950.hpp) under caller's nonces, driven by tests/cpp/nonce_main.cpp: the client's
encrypt of two records under two nonces, `decomposition` with the nonce, `decompose` with one nonce per record.  Its words are
compared with the oracle's keystreams and with what the C ABI gives for the same call on the same library.  Runs against the
tests-only emulator library and, marked gpu, against libhhe_gfx950.so.  The header of the driver carries the command of its
stand-alone sanitizer build."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nonce_common as nc
import parity_common as pc
from conftest import Setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NWORDS = 128 + 37


def drive(orc, api, lib, mem, tmp_path, libdir, libname, backend):
    S = Setup(orc, 10, [50] * 3, extra_steps=(-128,))
    O = S.O
    pt = np.random.default_rng(31).integers(0, S.t, size=(2, NWORDS), dtype=np.uint64)
    nonces = [nc.NA, nc.NB]
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        np.array([S.logn, O.K, S.t, len(S.gk.elts), NWORDS] + nonces, dtype=np.uint64).tofile(f)
        np.array(S.q, dtype=np.uint64).tofile(f)
        S.rk.tofile(f)
        for e, k in zip(S.gk.elts, S.gk.keys):
            np.array([int(e)], dtype=np.uint64).tofile(f)
            k.tofile(f)
        S.enc_key.tofile(f)
        S.key.tofile(f)
        pt.tofile(f)
    if os.environ.get("NONCE_KEEP_BLOB"):
        shutil.copy(blob, os.environ["NONCE_KEEP_BLOB"])
    exe = tmp_path / "nonce"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "nonce_main.cpp"),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nonce driver OK on " + backend in r.stdout, r.stdout + r.stderr
    words = np.fromfile(out, dtype=np.uint64)
    nb = int(words[0])
    assert nb == 2
    sym = words[1:1 + 2 * NWORDS].reshape(2, NWORDS)
    cts = words[1 + 2 * NWORDS:].reshape(nb + 2, *O.ct_shape)
    tt = np.uint64(S.t)
    for s in range(2):  # the client's words: the oracle's keystream under the record's nonce
        ks = np.concatenate([orc.pasta_keystream(S.t, S.key, b, nonces[s]) for b in range(2)])[:NWORDS]
        assert (sym[s] == (pt[s] + ks) % tt).all()
    # the server's words: the C ABI on the same library, and the restatement
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    cw = np.zeros((2, 128), np.uint64)
    cw[0], cw[1, :37] = sym[0, :128], sym[0, 128:]
    blocks = nc.run(X, S, mem, cw, [128, 37], [(nc.NA, 0), (nc.NA, 1)])
    assert (cts[:2] == blocks).all()
    assert (cts[1] == nc.item_truth(orc, S, cw[1], 37, nc.NA, 1)).all()
    out_d = mem.empty((2,) + O.ct_shape)
    X.decompose(mem.to_dev(S.enc_key), sym, out_d, nonces=nonces)
    assert (cts[2:] == mem.to_host(out_d)).all()
    dec = O.decode(O.decrypt(S.sk, cts[0]))  # too little budget at 3 primes for a meaning check: words only
    assert dec.shape == (S.n,)
    X.close()


def test_cpp_nonce_driver_on_emulator(orc, api, emu_lib, tmp_path):
    drive(orc, api, emu_lib, pc.HostMem(), tmp_path, os.path.join(ROOT, "tests", "emu"), "hhe_emu", "cpu-emulator")


@pytest.mark.gpu
def test_cpp_nonce_driver_on_gfx950(orc, api, tmp_path):
    lib = api.load_library()
    drive(orc, api, lib, pc.TorchMem("cuda:0"), tmp_path, os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "hhe_gfx950", "hip-gfx950")

"""Packed plain-matrix affine layers (hhe_matrix_create / hhe_packed_affine_ks / hhe_affine_galois_steps) on the tests-only emulator
(built with -DHHE_RANGE_CHECK): the host driver's schedules and the index arithmetic of the kernel bodies, word for word against
the Python restatement of SEALZpCipher::packed_matMul / packed_affine in affine_common.py."""
import threading

import numpy as np
import pytest

import affine_common as ac
import parity_common as pc

T = 65537


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def _params(orc, api, lib, name):
    """(logn, primes, expected row_kernel)"""
    if name == "n2048":      # ragged tiles: no row kernel at this degree
        return 11, orc.coeff_modulus_create(2048, [50] * 3), 0
    if name == "n4096pm":    # pseudo-Mersenne primes at full tiles: the fused row kernel
        return 12, orc.coeff_modulus_create(4096, [50] * 3), 1
    if name == "default4096":  # BFVDefault(4096), 36 + 36 + 37 bits: the separate-kernel path at full tiles
        return 12, api.bfv_default_coeff_modulus(4096, lib), 0
    raise KeyError(name)


def _ctx(orc, api, lib, name, steps, all_galois=False):
    logn, q, rowk = _params(orc, api, lib, name)
    S = ac.make_setup(orc, logn, q, T, steps, all_galois=all_galois)
    X = api.Context(logn, q, T, lib=lib)
    assert X.query("row_kernel") == rowk
    S.load_keys(X)
    return X, S


@pytest.mark.parametrize("n,dim,n1,n2", [
    (1024, 512, 0, 0),     # full-packed, diagonal: +1 alone
    (1024, 512, 32, 16),   # full-packed, BSGS
    (4096, 16, 0, 0),      # non-full-packed: -dim first
    (4096, 32, 8, 4),
    (4096, 12, 4, 3),      # not a power of two
    (4096, 16, 1, 16),     # n1 == 1: the diagonal method's list
    (4096, 16, 16, 1),
    (2048, 512, 0, 0),     # dim * 4 == N still fits
])
def test_step_lists(api, emu_lib, n, dim, n1, n2):
    want = ([] if 2 * dim == n else [-dim]) + [1] + ([k * n1 for k in range(1, n2)] if n1 > 1 and n2 > 1 else [])
    assert ac.hand_steps(n, dim, n1, n2) == want
    assert api.affine_galois_steps(n, dim, n1, n2, lib=emu_lib) == want


def test_step_list_errors(api, emu_lib):
    with pytest.raises(api.HheError) as e:
        api.affine_galois_steps(1024, 300, lib=emu_lib)   # 600 != 1024 and 1200 > 1024
    assert e.value.code == api.ERR_TOO_FEW_SLOTS and "too little slots" in str(e.value)
    with pytest.raises(api.HheError) as e:
        api.affine_galois_steps(4096, 16, 4, 3, lib=emu_lib)
    assert e.value.code == api.ERR_INVALID


CASES = [  # (dim, bsgs, bias, in place)
    (16, None, True, True),
    (16, (4, 4), False, False),
    (32, (8, 4), True, True),
    (12, None, False, False),
    (12, (4, 3), True, False),
]


@pytest.mark.parametrize("name", ["n2048", "n4096pm", "default4096"])
def test_word_parity(orc, api, emu_lib, mem, name):
    steps = sorted({s for dim, bsgs, _, _ in CASES for s in ac.hand_steps(1 << _params(orc, api, emu_lib, name)[0], dim, *(bsgs or (0, 0)))})
    X, S = _ctx(orc, api, emu_lib, name, steps)
    for i, (dim, bsgs, with_bias, in_place) in enumerate(CASES):
        M, b = ac.seeded_matrix(T, dim, 7 + i)
        ac.check_affine(X, S, mem, M, b if with_bias else None, bsgs, B=3, seed=i, in_place=in_place)
    X.close()


def test_diagonal_dim32_and_row_kernel_launch_count(orc, api, emu_lib, mem):
    """dim - 1 launches of ks_row_kernel per chunk, each over the chunk's items: the loop of the PASTA layers, not the generic rotation"""
    dim = 32
    X, S = _ctx(orc, api, emu_lib, "n4096pm", ac.hand_steps(4096, dim))
    M, b = ac.seeded_matrix(T, dim, 21)
    X.profile(True)
    ac.check_affine(X, S, mem, M, b, None, B=3, seed=9)
    _, launches, _, items = X.profile_read()
    assert launches == dim - 1 and items == 3 * (dim - 1)
    X.close()


def test_row_kernel_launches_per_chunk(orc, api, emu_lib, mem, monkeypatch):
    monkeypatch.setenv("HHE_CHUNK", "2")
    dim = 16
    X, S = _ctx(orc, api, emu_lib, "n4096pm", ac.hand_steps(4096, dim))
    M, _ = ac.seeded_matrix(T, dim, 22)
    X.profile(True)
    ac.check_affine(X, S, mem, M, None, None, B=3, seed=10)
    _, launches, _, items = X.profile_read()
    assert launches == 2 * (dim - 1) and items == 3 * (dim - 1)   # chunks of 2 + 1 items
    X.close()


@pytest.mark.parametrize("bsgs", [(32, 16), None])
def test_full_packed(orc, api, emu_lib, mem, bsgs):
    """dim = N / 2 at N = 1024: no preparation rotation, the diagonals fill the row.  BSGS 32 x 16, and the diagonal method's 511 steps."""
    n, dim = 1024, 512
    q = orc.coeff_modulus_create(n, [50] * 3)
    S = ac.make_setup(orc, 10, q, T, ac.hand_steps(n, dim, *(bsgs or (0, 0))))
    X = api.Context(10, q, T, lib=emu_lib)
    S.load_keys(X)
    M, b = ac.seeded_matrix(T, dim, 31)
    ac.check_affine(X, S, mem, M, b, bsgs, B=1, seed=3)
    X.close()


def test_degenerate_bsgs_is_the_diagonal_method(orc, api, emu_lib, mem):
    dim = 16
    X, S = _ctx(orc, api, emu_lib, "n2048", ac.hand_steps(2048, dim))
    M, b = ac.seeded_matrix(T, dim, 41)
    got, refs = ac.check_affine(X, S, mem, M, b, None, B=1, seed=4)
    for bsgs in ((1, 16), (16, 1)):
        g2, _ = ac.check_affine(X, S, mem, M, b, bsgs, B=1, seed=4, refs=refs)
        assert (g2 == got).all()
    X.close()


def test_missing_keys(orc, api, emu_lib, mem):
    """Steps without a key of their own go through their NAF terms over the set the call names, as SEAL's rotate_rows does (-12, 12 and
    20 here); step +1 has a one-term NAF, so without its key -- or without a usable decomposition of another step -- the call fails
    with HHE_ERR_NO_GALOIS_KEY before it writes anything."""
    logn, q, _ = _params(orc, api, emu_lib, "n2048")
    S = ac.make_setup(orc, logn, q, T, (), all_galois=True)   # +-2^k and the column swap: no key for -12, 12, 20, -24
    O = S.O
    X = api.Context(logn, q, T, lib=emu_lib)
    S.load_keys(X)
    for dim, bsgs in ((12, None), (24, (4, 6))):
        steps = ac.hand_steps(S.n, dim, *(bsgs or (0, 0)))
        assert any(int(O.galois_elt(s)) not in [int(e) for e in S.gk.elts] for s in steps)
        M, b = ac.seeded_matrix(T, dim, 51)
        ac.check_affine(X, S, mem, M, b, bsgs, B=2, seed=5)
    # a named set without +1 / with +1 but nothing that reaches -dim
    cts, _ = ac.inputs(S, 12, 1, 6)
    M, b = ac.seeded_matrix(T, 12, 52)
    mat = X.matrix(M, bias=b)
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}
    for have in ((-4, -8, -16), (1,)):
        ks = X.keyset()
        for s in have:
            ks.set_galois(int(O.galois_elt(s)), elt[int(O.galois_elt(s))])
        out = mem.to_dev(np.full((1,) + O.ct_shape, 12345, np.uint64))
        with pytest.raises(api.HheError) as e:
            X.packed_affine(mem.to_dev(cts), mat, out, 1, gk=ks)
        assert e.value.code == api.ERR_NO_GALOIS_KEY and "Galois key not present" in str(e.value)
        assert (mem.to_host(out) == 12345).all()
        ks.close()
    mat.close()
    X.close()


def test_matrix_identity(orc, api, emu_lib, mem):
    """Two matrices on one context used alternately; two threads, each with a matrix of its own; a handle of another context."""
    dim = 16
    X, S = _ctx(orc, api, emu_lib, "n2048", ac.hand_steps(2048, dim, 4, 4))
    O = S.O
    cts, _ = ac.inputs(S, dim, 2, 7)
    mats, refs = [], []
    for i, bsgs in enumerate((None, (4, 4))):
        M, b = ac.seeded_matrix(T, dim, 61 + i)
        mats.append(X.matrix(M, bias=b, bsgs=bsgs))
        refs.append(np.stack([ac.packed_affine_ref(O, S.gk, M, cts[k], b, bsgs) for k in range(2)]))
    assert mats[0].nbytes == (2 * dim * O.L + 1) * O.n * 8 and mats[1].nbytes == (dim * O.L + 1) * O.n * 8
    d_in = mem.to_dev(cts)
    for i in (0, 1, 0, 1):
        out = mem.empty((2,) + O.ct_shape)
        X.packed_affine(d_in, mats[i], out, 2)
        assert (mem.to_host(out) == refs[i]).all(), i
    errors = []

    def work(i):
        try:
            for _ in range(2):
                o = mem.empty((2,) + O.ct_shape)
                X.packed_affine(mem.to_dev(cts), mats[i], o, 2)
                assert (mem.to_host(o) == refs[i]).all(), i
        except BaseException as e:  # noqa: BLE001 -- reported by the asserting thread below
            errors.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    Y = api.Context(S.logn, S.q, T, lib=emu_lib)
    S.load_keys(Y)
    with pytest.raises(api.HheError) as e:
        Y.packed_affine(d_in, mats[0], mem.empty((2,) + O.ct_shape), 2)
    assert e.value.code == api.ERR_INVALID and "another context" in str(e.value)
    Y.close()
    for m in mats:
        m.close()
    X.close()


def test_create_rejects_bad_input(orc, api, emu_lib):
    logn, q, _ = _params(orc, api, emu_lib, "n2048")
    X = api.Context(logn, q, T, lib=emu_lib)
    M, b = ac.seeded_matrix(T, 16, 71)
    bad = M.copy()
    bad[3, 5] = T
    for args, code in (((bad,), api.ERR_INVALID), ((M, np.full(16, T, np.uint64)), api.ERR_INVALID), ((M, b, (4, 3)), api.ERR_INVALID)):
        with pytest.raises(api.HheError) as e:
            X.matrix(*args)
        assert e.value.code == code
    big, _ = ac.seeded_matrix(T, 600, 72)   # 1200 != 2048 and 2400 > 2048
    with pytest.raises(api.HheError) as e:
        X.matrix(big)
    assert e.value.code == api.ERR_TOO_FEW_SLOTS
    X.close()


def test_knob_neutrality(orc, api, emu_lib, mem, monkeypatch):
    """HHE_STREAMS x HHE_CHUNK only decide where the items run"""
    dim = 16
    logn, q, _ = _params(orc, api, emu_lib, "n2048")
    S = ac.make_setup(orc, logn, q, T, ac.hand_steps(2048, dim, 4, 4))
    M, b = ac.seeded_matrix(T, dim, 81)
    cts, _ = ac.inputs(S, dim, 3, 8)
    refs = {bsgs: np.stack([ac.packed_affine_ref(S.O, S.gk, M, cts[k], b, bsgs) for k in range(3)]) for bsgs in (None, (4, 4))}
    for streams in (1, 2):
        for chunk in (1, 128):
            monkeypatch.setenv("HHE_STREAMS", str(streams))
            monkeypatch.setenv("HHE_CHUNK", str(chunk))
            X = api.Context(logn, q, T, lib=emu_lib)
            S.load_keys(X)
            for bsgs in (None, (4, 4)):
                ac.check_affine(X, S, mem, M, b, bsgs, B=3, cts=cts, refs=refs[bsgs])
            X.close()


@pytest.mark.parametrize("n1,n2", [(16, 8), (40, 10)])
def test_inner_sum_kernel_at_its_bounds(orc, emu_lib, tmp_path, n1, n2):
    """60-bit primes, every operand word and every multiplier word at q_j - 1: n1 products of almost 2^120 in one 128-bit lazy sum
    (16 x 8: one group of 8 giant steps; 40 x 10: a fold after 32 products and a second group of 2).  The range check of the
    emulator build must not fire and every sum equals the exact integer reduced mod q_j."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    emu = os.path.join(root, "tests", "emu")
    q = orc.coeff_modulus_create(1024, [60] * 3)
    assert all(int(v).bit_length() == 60 for v in q)
    exe, out = tmp_path / "bsgs_inner", tmp_path / "out.bin"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(root, "privacy-preserving-ml-through-hhe_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "bsgs_inner_main.cpp"), "-L" + emu, "-lhhe_emu", "-Wl,-rpath," + emu, "-o", str(exe)])
    B, logn = 2, 10
    r = subprocess.run([str(exe), str(n1), str(n2), str(logn), str(B), str(out)] + [str(int(v)) for v in q], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = np.fromfile(out, dtype=np.uint64).reshape(n2, B, 2, len(q), 1 << logn)
    for j, qj in enumerate(q):
        want = (n1 * (int(qj) - 1) ** 2) % int(qj)
        assert (words[:, :, :, j, :] == np.uint64(want)).all(), (j, want)

"""hhe_fc_row / hhe_fc_row_ks where it is used: 784 inputs at the benchmarked and at the deployed parameters, real zero
coefficients under the shared digits, and a per-element sum of c1 that must be closed in mid-walk (8192 inputs).  Every comparison
is exact equality of ciphertext words with the CPU oracle: live where the oracle needs seconds, through the per-limb SHA-256 of
tests/golden/fc*.json (tests/golden/make_fc784.py) where it needs minutes per row.  The counters fc_fallbacks and fc_csum_closes
accumulate per context: every run here reads them on a fresh context.  Unmarked tests run on the tests-only emulator; the `gpu`
ones on an MI355X (python -m pytest tests -m gpu)."""
import json
import os

import numpy as np
import pytest

import parity_common as pc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hostmem():
    return pc.HostMem()


@pytest.fixture(scope="module")
def gpumem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.TorchMem("cuda:0")


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()  # fails loudly if the HIP library is missing
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


def golden(name):
    return json.load(open(os.path.join(HERE, "golden", name + ".json")))


def ctx_factory(api, lib, row_kernel):
    """contexts that assert the path they run (row_kernel as given, digit_reduce as the case says) before anything is computed"""
    def make_ctx(logn, q, t, digit_reduce):
        X = api.Context(logn, q, t, lib=lib)
        pc.assert_dispatch(X, q, row_kernel, digit_reduce)
        return X
    return make_ctx


# ---- the trie model ----

def test_trie_model_pins(orc):
    """the model of the rotation trie (parity_common.FcTrie) against values observed on the library: key switches, leaves, leaves
    per Galois element of the last term, closed c1 sums per chunk"""
    for n in (1024, 16384, 32768):
        O = orc.Oracle(n.bit_length() - 1, orc.coeff_modulus_create(n, [40, 40]), pc.T16)
        assert sorted(set(O.galois_elts_all())) == sorted(pc.default_galois_elts_py(n))
        for s in (0, 1, -1, 128, -128, -256, -(n // 2 - 4), n // 4, -(n // 4)):
            assert pc.galois_elt_py(n, s) == O.galois_elt(s), (n, s)

    def model(n, n_in, whole_set, keys=None):
        return pc.FcTrie(orc, n, n_in, pc.default_galois_elts_py(n) if keys is None else keys, whole_set)
    m = model(32768, 784, True)
    assert (m.nodes, m.leaves, m.closes) == (1054, 613, 3)
    assert m.leaves_per_step((-256, -512, -1024)) == {-256: 171, -512: 341, -1024: 101}
    # at N = 2^15 no step below 784 but the powers of two has a default element: both policies build the same trie, and keys of
    # steps that are no powers of two (flatten: -384, -640, -768) are invisible to default_galois_only = 1
    extra = [pc.galois_elt_py(32768, s) for s in (-384, -640, -768)]
    m1 = model(32768, 784, False, pc.default_galois_elts_py(32768) + extra)
    assert (m1.term, m1.parent, m1.mult) == (m.term, m.parent, m.mult)
    assert -384 in model(32768, 784, True, pc.default_galois_elts_py(32768) + extra).term and -384 not in m1.term
    m = model(1024, 400, False)   # NAF only
    assert m.nodes == 484 and m.leaves_per_step((-128, -256, 128)) == {-128: 85, -256: 171, 128: 58}
    for n, n_in in ((1024, 400), (1024, 37), (4096, 100), (16384, 784)):
        assert model(n, n_in, True).closes == 3, (n, n_in)
    # 8192 inputs at N = 2^14, the whole default set visible: the element of step -4096 collects 2731 leaves and is closed at 2000
    # and again with 731; -2048 and +2048 hold 1365 each; the eleven steps -(8192 - 2^k), k = 0..10, have the element of +2^k,
    # take the one-term shortcut and are sums of one term each.  15 closes.
    m = model(16384, 8192, True)
    e = lambda s: pc.galois_elt_py(16384, s)
    assert m.closes == 15
    assert sorted(c for el, c in m.closed_sums if el == e(-4096)) == [731, 2000]
    assert [c for el, c in m.closed_sums if el in (e(-2048), e(2048))] == [1365, 1365]
    assert sorted((el, c) for el, c in m.closed_sums if c == 1) == sorted((e(1 << k), 1) for k in range(11))
    assert e(-(8192 - 4)) == e(4)
    # default_galois_only = 1: those eleven go through NAF ([2^k, -8192] without the +-N/2 term: the same element, deeper in the trie)
    m = model(16384, 8192, False)
    assert m.closes == 4 and sorted(c for _, c in m.closed_sums) == [731, 1365, 1365, 2000]


# ---- A. 784 inputs ----

def keysets_of(X, S):
    """the FC's key objects as bench.py's MnistFlow names them: a RelinKeys set and the analyst's default GaloisKeys set"""
    rk, gk = X.keyset(), X.keyset()
    rk.set_relin(S.rk)
    for e, k in zip(S.gk.elts, S.gk.keys):
        gk.set_galois(int(e), k)
    return rk, gk


def run_bench_shape(orc, api, lib, mem, monkeypatch, forms, items):
    name = "fc784_n32768"
    p, fx = pc.FC_SHAPES[name], golden(name)
    assert fx["key_switches"] == [2875] * p["B"]   # the oracle ran the literal loop of 783 rotate_rows, not a trie
    S = pc.fc_shape_setup(orc, name)
    O = S.O
    _, _, vi, wc = pc.fc_shape_inputs(S, name, items=items)
    B = len(items)
    assert list(items) == list(range(B))
    closes = pc.FcTrie(orc, S.n, p["n_in"], S.gk.elts, whole_set=True).closes
    for form in forms:
        if form == "chunk2":
            monkeypatch.setenv("HHE_FC_CHUNK", "2")
        X = api.Context(S.logn, S.q, S.t, lib=lib)
        monkeypatch.delenv("HHE_FC_CHUNK", raising=False)
        pc.assert_dispatch(X, S.q, 1, 0)
        out = mem.empty((B,) + O.ct_shape)
        if form == "default_set":
            # the context's default set holds the FC's keys PLUS the flatten steps' keys (the PASTA steps -1, 0, 128 are default
            # elements already); default_galois_only = 1 must not see -384, -640, -768
            S.load_keys(X)
            steps = (-384, -640, -768)
            gx = O.keygen_galois(S.sk, [O.galois_elt(s) for s in steps], 9)
            for e, k in zip(gx.elts, gx.keys):
                assert not X.has_galois_key(int(e))
                X.set_galois_key(int(e), k)
            X.fc_row(mem.to_dev(vi[:B]), mem.to_dev(wc), p["W"], p["n_in"], out, B, relin_slot=0, default_galois_only=True)
        else:
            rk, gk = keysets_of(X, S)
            X.fc_row(mem.to_dev(vi[:B]), mem.to_dev(wc), p["W"], p["n_in"], out, B, rk=rk, gk=gk)
        got = mem.to_host(out)
        for b in range(B):
            pc.assert_limb_hashes(got[b], fx["items"][b], (form, "item", b))
        chunks = (B + 1) // 2 if form == "chunk2" else 1
        assert X.query("fc_fallbacks") == 0
        assert X.query("fc_csum_closes") == closes * chunks, (form, X.query("fc_csum_closes"), closes, chunks)
        X.close()


def test_fc784_bench_shape_two_items_emulator(orc, api, emu_lib, hostmem, monkeypatch):
    """N = 2^15, 4 x 60-bit primes, 784 inputs, hhe_fc_row_ks with the key sets of the bench: items 0 and 1 (weight rows 0 and 1)
    of the fixture's five, word for word through the per-limb hashes"""
    run_bench_shape(orc, api, emu_lib, hostmem, monkeypatch, ["keysets"], [0, 1])


@pytest.mark.gpu
def test_fc784_bench_shape(orc, api, lib, gpumem, monkeypatch):
    """the benchmarked FC row word for word: 1054 key switches in the trie, 613 leaves in three per-element sums (341 terms in the
    largest: the 64-bit word wraps ten to twenty times).  Five items over two weight rows against one set of hashes: the library's
    defaults (one chunk); HHE_FC_CHUNK=2 (chunks of 2, 2, 1 round-robin over the internal streams); hhe_fc_row with
    default_galois_only = 1 on a default set that also holds the flatten steps' keys"""
    run_bench_shape(orc, api, lib, gpumem, monkeypatch, ["keysets", "chunk2", "default_set"], range(5))


@pytest.mark.gpu
def test_fc784_deployed_shape(orc, api, lib, gpumem):
    """N = 2^14, BFVDefault(16384) (L = 8: no leaf groups, no c1 sums), 784 inputs, two items: every word against the oracle's
    hashes, and -- the one parameter set of these that decrypts -- slot 783 is the plain dot product"""
    name = "fc784_n16384"
    p, fx = pc.FC_SHAPES[name], golden(name)
    assert fx["key_switches"] == [2875] * p["B"]
    assert api.bfv_default_coeff_modulus(16384, lib) == pc.BFV_DEFAULT_16384
    S = pc.fc_shape_setup(orc, name)
    O = S.O
    v, w, vi, wc = pc.fc_shape_inputs(S, name)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    assert X.L == 8
    rk, gk = keysets_of(X, S)
    out = gpumem.empty((p["B"],) + O.ct_shape)
    X.fc_row(gpumem.to_dev(vi), gpumem.to_dev(wc), 1, p["n_in"], out, p["B"], rk=rk, gk=gk)
    got = gpumem.to_host(out)
    for b in range(p["B"]):
        pc.assert_limb_hashes(got[b], fx["items"][b], ("item", b))
        assert O.noise_budget(S.sk, got[b], 8) > 0
        assert int(O.decode(O.decrypt(S.sk, got[b]))[p["n_in"] - 1]) == int(np.dot(v[b], w[0])) % S.t
    assert X.query("fc_fallbacks") == 0 and X.query("fc_csum_closes") == 0
    X.close()


# ---- B. real zero coefficients ----

@pytest.mark.parametrize("name", list(pc.ZERO_CASES))
def test_real_zeros_fall_back_exactly_where_predicted_emulator(orc, api, emu_lib, hostmem, monkeypatch, name):
    """coefficient primes of 17 to 20 bits, where c1 has zero coefficients as a matter of course: fc_fallbacks equals the number of
    items (or chunks) the oracle-side walk of the trie predicts, and every word is the oracle's (parity_common.check_fc_real_zeros)"""
    pc.check_fc_real_zeros(ctx_factory(api, emu_lib, 0), orc, hostmem, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pc.ZERO_CASES))
def test_real_zeros_fall_back_exactly_where_predicted(orc, api, lib, gpumem, monkeypatch, name):
    """the same cases through the HIP kernels: the digit load of k_ntt raises the flag from the lanes that meet the zero"""
    pc.check_fc_real_zeros(ctx_factory(api, lib, 0), orc, gpumem, monkeypatch, name)


def test_transparent_item_falls_back_on_the_row_kernel_path_emulator(orc, api, emu_lib, hostmem, monkeypatch):
    """detection on the fused row kernels' path, by an item whose c1 is 0 throughout (parity_common.check_fc_transparent_row_kernel)"""
    pc.check_fc_transparent_row_kernel(ctx_factory(api, emu_lib, 1), orc, hostmem, monkeypatch)


@pytest.mark.gpu
def test_transparent_item_falls_back_on_the_row_kernel_path(orc, api, lib, gpumem, monkeypatch):
    pc.check_fc_transparent_row_kernel(ctx_factory(api, lib, 1), orc, gpumem, monkeypatch)


# ---- C. the long sum ----

def run_long_sum(orc, api, lib, mem, monkeypatch, policies):
    """N = 2^14, 3 x 60-bit primes (row kernel, L = 2), 8192 inputs -- the widest row the ABI admits: the element of step -4096
    collects 2731 leaves, so its sum is closed at CSUM_MAX = 2000 in mid-walk (a second inner product into the same accumulator,
    sums and wrap bytes reset, slots of parents still pending) and again at the end.  policies: (default_galois_only, HHE_FC_CSUM)"""
    name = "fc8192_n16384"
    p, fx = pc.FC_SHAPES[name], golden(name)
    assert fx["key_switches"] == [36409]
    S = pc.fc_shape_setup(orc, name)
    O = S.O
    _, _, vi, wc = pc.fc_shape_inputs(S, name)
    for dgo, csum in policies:
        monkeypatch.setenv("HHE_FC_CSUM", str(csum))
        X = api.Context(S.logn, S.q, S.t, lib=lib)
        monkeypatch.delenv("HHE_FC_CSUM")
        pc.assert_dispatch(X, S.q, 1, 0)
        S.load_keys(X)
        out = mem.empty((1,) + O.ct_shape)
        X.fc_row(mem.to_dev(vi), mem.to_dev(wc), 1, p["n_in"], out, 1, relin_slot=0, default_galois_only=bool(dgo))
        pc.assert_limb_hashes(mem.to_host(out)[0], fx["items"][0], (dgo, csum))
        closes = pc.FcTrie(orc, S.n, p["n_in"], S.gk.elts, whole_set=not dgo).closes if csum else 0
        assert closes == {(0, 1): 15, (1, 1): 4}.get((dgo, csum), 0)
        assert X.query("fc_fallbacks") == 0
        assert X.query("fc_csum_closes") == closes, (dgo, csum, X.query("fc_csum_closes"), closes)
        X.close()


def test_fc8192_long_sum_closes_in_mid_walk_emulator(orc, api, emu_lib, hostmem, monkeypatch):
    run_long_sum(orc, api, emu_lib, hostmem, monkeypatch, [(0, 1), (0, 0)])


@pytest.mark.gpu
def test_fc8192_long_sum_closes_in_mid_walk(orc, api, lib, gpumem, monkeypatch):
    run_long_sum(orc, api, lib, gpumem, monkeypatch, [(0, 1), (0, 0), (1, 1)])

"""One keystream per key on the gfx950 kernels (see kscache_common and test_ks_cache): on one context of the smallest shape that takes
the fused key-switch row kernel, and one case at the benchmark's parameters."""
import pytest

from conftest import Setup
import dedup_common as dc
import kscache_common as kc
import parity_common as pc


@pytest.fixture(scope="module")
def mem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.TorchMem("cuda:0")


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


@pytest.fixture(scope="module")
def row_setup(orc):
    return Setup(orc, 12, [50, 50, 50])


def make(api, lib, S, monkeypatch, **env):
    X, X0 = kc.ctx_on(api, lib, S, monkeypatch, **env), kc.ctx_off(api, lib, S, monkeypatch, **env)
    assert X.query("row_kernel") == 1 and X0.query("row_kernel") == 1
    return X, X0


@pytest.mark.gpu
def test_gpu_repeat_and_new_words(orc, api, lib, mem, row_setup, monkeypatch):
    S, ids = row_setup, [0, 0, 6, 0]
    X, X0 = make(api, lib, S, monkeypatch)
    cw, ncw = kc.words(S, 4, 31), [128, 128, 16, 5]
    r1 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (2, 0)
    r2 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (0, 2) and X.query("transcipher_unique") == 2
    r0 = kc.run(X0, S, mem, cw, ncw, ids)
    assert kc.counts(X0) == (2, 0)
    assert (r1 == r0).all() and (r2 == r0).all()
    assert (r2[3] == dc.oracle_block(S, cw, ncw, ids, 3)).all()
    cw, ncw = kc.words(S, 4, 32), [7, 128, 128, 90]  # other words and lengths against the kept keystreams
    r3 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (0, 2)
    assert (r3 == kc.run(X0, S, mem, cw, ncw, ids)).all()
    assert (r3[2] == dc.oracle_block(S, cw, ncw, ids, 2)).all()
    X.close(), X0.close()


@pytest.mark.gpu
def test_gpu_partial_hits_across_two_streams(orc, api, lib, mem, row_setup, monkeypatch):
    S = row_setup
    X, X0 = make(api, lib, S, monkeypatch, HHE_STREAMS=2, HHE_CHUNK=2)
    kc.run(X, S, mem, kc.words(S, 2, 33), [128, 128], [0, 1])
    assert kc.counts(X) == (2, 0)
    cw, ncw, ids = kc.words(S, 7, 34), [128, 30, 128, 128, 1, 128, 64], [1, 2, 0, 2, 3, 4, 1]  # 3 evaluations in 2 chunks, 7 items in 4
    r = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (3, 2) and X.query("transcipher_unique") == 5
    assert (r == kc.run(X0, S, mem, cw, ncw, ids)).all()
    for b in (4, 6):  # an evaluated counter and a kept one
        assert (r[b] == dc.oracle_block(S, cw, ncw, ids, b)).all(), b
    X.close(), X0.close()


@pytest.mark.gpu
def test_gpu_enc_key_overwritten_in_place(orc, api, lib, mem, row_setup, monkeypatch):
    """the device buffer is refilled on the stream the context runs on, with no host wait before the call: the comparison is ordered
    behind the copy that fills it"""
    S, ids, ncw = row_setup, [0, 0], [128, 40]
    cw = kc.words(S, 2, 35)
    enc2 = kc.other_enc_key(S, 0)
    X, X0 = make(api, lib, S, monkeypatch)
    buf, d1, d2 = mem.to_dev(S.enc_key), mem.to_dev(S.enc_key), mem.to_dev(enc2)
    ra = kc.run(X, S, mem, cw, ncw, ids, key=buf)
    buf.copy_(d2, non_blocking=True)
    rb = kc.run(X, S, mem, cw, ncw, ids, key=buf)
    assert kc.counts(X) == (1, 0)
    assert (rb == kc.run(X0, S, mem, cw, ncw, ids, key=d2)).all() and not (rb == ra).all()
    assert (rb[1] == dc.oracle_block(S, cw, ncw, ids, 1, enc_key=enc2)).all()
    buf.copy_(d1, non_blocking=True)
    assert (kc.run(X, S, mem, cw, ncw, ids, key=buf) == ra).all() and kc.counts(X) == (0, 1)
    buf.copy_(d2, non_blocking=True)
    assert (kc.run(X, S, mem, cw, ncw, ids, key=buf) == rb).all() and kc.counts(X) == (0, 1)
    assert (ra == kc.run(X0, S, mem, cw, ncw, ids, key=d1)).all()
    X.close(), X0.close()


@pytest.mark.gpu
def test_gpu_key_replaced(orc, api, lib, mem, row_setup, monkeypatch):
    S, O, ids, ncw = row_setup, row_setup.O, [2, 2], [128, 50]
    cw = kc.words(S, 2, 36)
    rk2, gk2 = kc.other_keys(S, 61)
    e1 = int(O.galois_elt(-1))
    g1 = gk2.keys[[int(e) for e in S.gk.elts].index(e1)]
    X, X0 = make(api, lib, S, monkeypatch)
    ra = kc.run(X, S, mem, cw, ncw, ids)
    X.set_galois_key(e1, g1)
    X0.set_galois_key(e1, g1)
    rb = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 1
    assert (rb == kc.run(X0, S, mem, cw, ncw, ids)).all() and not (rb == ra).all()
    X.set_relin_key(rk2)
    X0.set_relin_key(rk2)
    rc = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0)
    assert (rc == kc.run(X0, S, mem, cw, ncw, ids)).all() and not (rc == rb).all()
    assert (kc.run(X, S, mem, cw, ncw, ids) == rc).all() and kc.counts(X) == (0, 1)
    X.close(), X0.close()


@pytest.mark.gpu
def test_gpu_profiled_call_runs_the_chain(orc, api, lib, mem, row_setup, monkeypatch):
    S, ids, ncw = row_setup, [3, 3], [128, 40]
    cw = kc.words(S, 2, 37)
    X, X0 = make(api, lib, S, monkeypatch)
    r1 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 1
    X.profile(True)
    r2 = kc.run(X, S, mem, cw, ncw, ids)
    _, launches, _, items = X.profile_read()
    assert kc.counts(X) == (1, 0) and launches > 0 and items == launches, (launches, items)
    X.profile(False)
    r3 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (0, 1)
    r0 = kc.run(X0, S, mem, cw, ncw, ids)
    assert (r1 == r0).all() and (r2 == r0).all() and (r3 == r0).all()
    X.close(), X0.close()


@pytest.mark.gpu
def test_gpu_bench_parameters(orc, api, lib, mem, monkeypatch):
    """N = 2^15, 4 x 60 bits, counters [0, 0, 6, 0]: two calls with different words, the second against a context that keeps nothing"""
    S, ids = Setup(orc, 15, [60] * 4), [0, 0, 6, 0]
    X, X0 = make(api, lib, S, monkeypatch)
    kc.run(X, S, mem, kc.words(S, 4, 38), [128, 128, 16, 5], ids)
    assert kc.counts(X) == (2, 0) and X.query("ks_cache_bytes") == 2 * kc.ct_bytes(S)
    cw, ncw = kc.words(S, 4, 39), [128, 3, 16, 128]
    r = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (0, 2)
    assert (r == kc.run(X0, S, mem, cw, ncw, ids)).all()
    X.close(), X0.close()

"""hhe_ctx_set_stream on an MI355X: a context handed a PyTorch stream gives, word for word, what a context on the default stream
gives; it reads its inputs in the order of that stream (an input whose upload is still in flight behind a delay, the key ciphertext
overwritten in place by an asynchronous copy); a synchronous entry point's result is there when it returns; and two contexts on two
caller streams run concurrently from two threads.  One process, one context per stream, at most two caller streams, no graph capture.
Every comparison is exact equality of ciphertext words; named items also equal the oracle.

The generic ops (add, multiply, relinearize, rotations, add_plain) are asynchronous on the context's stream -- the tests wait with
Context.sync() before they read; the batched calls (transcipher, fc_row, packed_affine, decompose, mod_switch) return after their work.

The delay in front of a late input is torch.cuda._sleep where the build has it (else a chain of matrix products), sized to ten times
the measured time from the first enqueue to the entry of the call and at most 100 ms; an event recorded behind the upload must still
be pending when the call is entered, or the test fails: a drained delay proves nothing."""
import threading
import time

import numpy as np
import pytest

import affine_common as ac
import dedup_common as dc
import kscache_common as kc
from conftest import Setup

pytestmark = pytest.mark.gpu
N_IN, DIM, BSGS = 9, 16, (4, 4)
IDS, NCW = [0, 1, 0, 2, 1], [128, 30, 128, 1, 64]   # five items over three counters


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


@pytest.fixture(scope="module")
def S10(orc):
    """the `small` shape (N = 1024, 9 x 50 bits) with every default Galois key, the affine layer's and the flatten steps"""
    return Setup(orc, 10, [50] * 9, all_galois=True, extra_steps=[-128, -256] + ac.hand_steps(1024, DIM, *BSGS))


@pytest.fixture(scope="module")
def S12(orc):
    return Setup(orc, 12, [50] * 3)


class Mem:
    """uploads and read-backs under one torch stream (None: the default stream)"""

    def __init__(self, torch, stream=None):
        self.torch, self.stream = torch, stream

    def _on(self):
        return self.torch.cuda.stream(self.stream)

    def to_dev(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        with self._on():
            return self.torch.from_numpy(a.view(np.int64)).to("cuda:0")

    def empty(self, shape):
        with self._on():
            return self.torch.zeros(shape, dtype=self.torch.int64, device="cuda:0")

    def to_host(self, b):
        with self._on():
            return b.cpu().numpy().view(np.uint64)  # a copy on the stream the context works on, behind its work


def ctx(api, lib, S, monkeypatch, stream=None, **env):
    X = dc.make_ctx(api, lib, S, monkeypatch, **env)
    if stream is not None:
        X.set_stream(stream.cuda_stream)
    return X


def small_ops(X, S, orc, mem):
    """every call family at N = 1024 on one context; {name: words}"""
    O, r = S.O, {}
    rng = np.random.default_rng(5)
    cts = np.stack([O.encrypt(S.pk, O.encode(rng.integers(0, S.t, S.n).astype(np.uint64)), 40 + b) for b in range(2)])
    a, b = mem.to_dev(cts[:1]), mem.to_dev(cts[1:])
    out, out3 = mem.empty((1,) + O.ct_shape), mem.empty((1, 3) + O.ct_shape[1:])
    X.add(a, b, out, 1)
    X.sync()
    r["add"] = mem.to_host(out)
    out = mem.empty((1,) + O.ct_shape)
    X.multiply(a, b, out3, 1)
    X.relinearize(out3, out, 1)
    X.sync()
    r["multiply_relinearize"] = mem.to_host(out)
    out = mem.empty((1,) + O.ct_shape)
    X.rotate_rows(a, -1, out, 1)
    X.sync()
    r["rotate_rows"] = mem.to_host(out)
    out = mem.empty((1,) + O.ct_shape)
    X.rotate_columns(a, out, 1)
    X.sync()
    r["rotate_columns"] = mem.to_host(out)
    cw = kc.words(S, 5, 91)
    r["transcipher_cold"] = kc.run(X, S, mem, cw, NCW, IDS)
    assert kc.counts(X) == (3, 0)
    r["transcipher_kept"] = kc.run(X, S, mem, cw, NCW, IDS)
    assert kc.counts(X) == (0, 3)
    v, w = rng.integers(0, 4, (2, N_IN)), rng.integers(-8, 9, N_IN)
    vi = np.stack([O.encrypt(S.pk, O.encode(v[i]), 141 + i) for i in range(2)])
    wc = O.encrypt(S.pk, O.encode(w % S.t), 143)
    ks = X.keyset()
    ks.set_relin(S.rk)
    for e, k in zip(S.gk.elts, S.gk.keys):
        ks.set_galois(int(e), k)
    out = mem.empty((2,) + O.ct_shape)
    X.fc_row(mem.to_dev(vi), mem.to_dev(wc[None]), 1, N_IN, out, 2, rk=ks, gk=ks)
    r["fc_row"] = mem.to_host(out)
    M, bias = ac.seeded_matrix(S.t, DIM, 77)
    acts, _ = ac.inputs(S, DIM, 2, 7)
    mat = X.matrix(M, bias=bias, bsgs=BSGS)
    out = mem.empty((2,) + O.ct_shape)
    X.packed_affine(mem.to_dev(acts), mat, out, 2)
    r["packed_affine"] = mem.to_host(out)
    mat.close(), ks.close()
    pts = [np.array([(7 * i + 3 + s) % 256 for i in range(300)], dtype=np.uint64) for s in range(2)]
    recs = np.stack([orc.pasta_encrypt(S.t, S.key, p) for p in pts])
    out = mem.empty((2,) + O.ct_shape)
    X.decompose(mem.to_dev(S.enc_key), recs, out, mask_last=True)
    r["decompose"] = mem.to_host(out)
    L = O.L
    low, vals = mem.empty((1, 2, L - 1, S.n)), mem.empty((1, S.n))
    X.mod_switch(a, 2, 1, L, L - 1, low)
    X.decrypt_level(S.sk, low, L - 1, 1, vals)
    X.sync()
    r["mod_switch"], r["decrypt_level"] = mem.to_host(low), mem.to_host(vals)
    refs = dict(cw=cw, vi=vi, wc=wc, M=M, bias=bias, acts=acts)
    return r, refs


def same_words(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)


def test_same_words_on_a_callers_stream(orc, api, lib, torch, S10, S12, monkeypatch):
    S, O = S10, S10.O
    env = dict(HHE_STREAMS=2, HHE_CHUNK=2)
    s = torch.cuda.Stream()
    X0 = ctx(api, lib, S, monkeypatch, **env)
    want, refs = small_ops(X0, S, orc, Mem(torch))
    # the named items against the oracle
    assert (want["transcipher_cold"][3] == dc.oracle_block(S, refs["cw"], NCW, IDS, 3)).all()
    assert (want["fc_row"][0] == O.fc_row(refs["vi"][0], refs["wc"], S.rk, S.gk, N_IN)[0]).all()
    assert (want["packed_affine"][1] == ac.packed_affine_ref(O, S.gk, refs["M"], refs["acts"][1], refs["bias"], BSGS)).all()
    X1 = ctx(api, lib, S, monkeypatch, stream=s, **env)
    got, _ = small_ops(X1, S, orc, Mem(torch, s))
    same_words(got, want, "caller's stream")
    X1.set_stream(None)
    X1.clear_keystream_cache()  # the cold call evaluates again
    got, _ = small_ops(X1, S, orc, Mem(torch))
    same_words(got, want, "back on the default stream")
    # the finishing pass as one workgroup per item
    Xi0, Xi1 = ctx(api, lib, S, monkeypatch, HHE_FIN_ITEM=1, **env), ctx(api, lib, S, monkeypatch, stream=s, HHE_FIN_ITEM=1, **env)
    for _ in range(2):  # cold, then against the kept keystreams
        r0 = kc.run(Xi0, S, Mem(torch), refs["cw"], NCW, IDS)
        r1 = kc.run(Xi1, S, Mem(torch, s), refs["cw"], NCW, IDS)
        assert (r0 == want["transcipher_cold"]).all() and (r1 == r0).all()
    assert kc.counts(Xi1) == (0, 3) and Xi1.query("fin_item_launches") > 0
    for X in (X0, X1, Xi0, Xi1):
        X.close()
    # N = 4096: the row kernel
    S, O = S12, S12.O
    cw, ncw, ids = kc.words(S, 3, 92), [128, 17, 0], [0, 0, 5]
    ct = O.encrypt(S.pk, O.encode(np.arange(S.n, dtype=np.uint64) % S.t), 44)[None]
    res = []
    for stream in (None, s):
        X, mem = ctx(api, lib, S, monkeypatch, stream=stream, **env), Mem(torch, stream)
        assert X.query("row_kernel") == 1
        out = mem.empty((1,) + O.ct_shape)
        X.rotate_rows(mem.to_dev(ct), -1, out, 1)
        X.sync()
        res.append((kc.run(X, S, mem, cw, ncw, ids), mem.to_host(out)))
        X.close()
    assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
    assert (res[1][0][1] == dc.oracle_block(S, cw, ncw, ids, 1)).all()


class Delay:
    """a kernel that keeps a stream busy for `ms`; calibrated once"""

    def __init__(self, torch):
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.m = torch.ones((1024, 1024), device="cuda:0")
        self.unit_ms = self._time(self._unit)  # one unit of work
        self.unit_ms = self._time(self._unit)

    def _unit(self):
        if self.sleep:
            self.sleep(1_000_000)
        else:
            for _ in range(8):
                self.m = (self.m @ self.m).clamp_(0, 1)

    def _time(self, fn):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        t.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        t.cuda.synchronize()
        return max(e0.elapsed_time(e1), 1e-3)

    def enqueue(self, ms):
        if self.sleep:
            self.sleep(int(1_000_000 * ms / self.unit_ms))
        else:
            for _ in range(max(1, int(round(ms / self.unit_ms)))):
                self._unit()


def late(torch, delay, s, dst, pinned, call, measured):
    """under s: clear dst, a delay, the real words from page-locked memory without blocking; then `call` at once.  The delay is ten times
    what a rehearsal of the same enqueues took on the host (at most 100 ms); the upload must still be pending when the call is entered"""
    def enqueues(ms):
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            dst.zero_()
            delay.enqueue(ms)
            dst.copy_(pinned, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(s)
        return ev, (time.perf_counter() - t0) * 1e3

    _, host_ms = enqueues(0.01)  # rehearsal: what the enqueues cost before the call is entered
    torch.cuda.synchronize()
    ms = min(100.0, 10.0 * host_ms)
    ev, host_ms2 = enqueues(ms)
    pending = not ev.query()
    call()
    measured.append(dict(enqueue_to_entry_ms=round(host_ms2, 3), delay_ms=round(ms, 3), pending=pending))
    print("late input:", measured[-1])
    assert pending, "the delay had drained before the call was entered: this run proves nothing"


def pinned_of(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).pin_memory()


def test_input_produced_late_on_the_callers_stream(orc, api, lib, torch, S10, monkeypatch):
    S, O = S10, S10.O
    s, delay, measured = torch.cuda.Stream(), Delay(torch), []
    mem = Mem(torch, s)
    X = ctx(api, lib, S, monkeypatch, stream=s)
    ct = O.encrypt(S.pk, O.encode(np.arange(S.n, dtype=np.uint64) % S.t), 45)[None]
    plain = np.random.default_rng(6).integers(0, S.t, (1, S.n)).astype(np.uint64)
    cw, ncw, ids = kc.words(S, 2, 93), [128, 50], [0, 1]
    # expected: the same calls after a full synchronisation
    d_ct, d_plain, d_key = mem.to_dev(ct), mem.to_dev(plain), mem.to_dev(S.enc_key)
    o_rot, o_add = mem.empty((1,) + O.ct_shape), mem.empty((1,) + O.ct_shape)
    torch.cuda.synchronize()
    X.rotate_rows(d_ct, -1, o_rot, 1)
    X.add_plain(d_ct, d_plain, o_add, 1)
    X.sync()
    want_rot, want_add = mem.to_host(o_rot), mem.to_host(o_add)
    want_tr = kc.run(X, S, mem, cw, ncw, ids, key=d_key)
    X.clear_keystream_cache()
    torch.cuda.synchronize()
    # rotate_rows: the ciphertext arrives late
    o = mem.empty((1,) + O.ct_shape)
    late(torch, delay, s, d_ct, pinned_of(torch, ct), lambda: X.rotate_rows(d_ct, -1, o, 1), measured)
    X.sync()
    assert (mem.to_host(o) == want_rot).all()
    # add_plain: the plaintext arrives late
    o = mem.empty((1,) + O.ct_shape)
    late(torch, delay, s, d_plain, pinned_of(torch, plain), lambda: X.add_plain(d_ct, d_plain, o, 1), measured)
    X.sync()
    assert (mem.to_host(o) == want_add).all()
    # transcipher: the key ciphertext arrives late
    o = mem.empty((2,) + O.ct_shape)
    late(torch, delay, s, d_key, pinned_of(torch, S.enc_key), lambda: X.transcipher(d_key, cw, ncw, ids, o), measured)
    assert (mem.to_host(o) == want_tr).all() and kc.counts(X) == (2, 0)
    X.close()


def test_key_comparison_follows_the_stream(orc, api, lib, torch, S10, monkeypatch):
    S = S10
    s, delay, measured = torch.cuda.Stream(), Delay(torch), []
    mem = Mem(torch, s)
    cw, ncw, ids = kc.words(S, 3, 94), [128, 9, 128], [0, 2, 0]
    enc_b = kc.other_enc_key(S, 0)
    X = ctx(api, lib, S, monkeypatch, stream=s)
    buf = mem.to_dev(S.enc_key)
    ra = kc.run(X, S, mem, cw, ncw, ids, key=buf)
    assert kc.counts(X) == (2, 0)
    Xb = ctx(api, lib, S, monkeypatch)
    want_b = kc.run(Xb, S, Mem(torch), cw, ncw, ids, key=Mem(torch).to_dev(enc_b))
    Xb.close()
    torch.cuda.synchronize()
    o = mem.empty((3,) + S.O.ct_shape)
    late(torch, delay, s, buf, pinned_of(torch, enc_b), lambda: X.transcipher(buf, cw, ncw, ids, o), measured)
    assert (mem.to_host(o) == want_b).all() and not (want_b == ra).all()
    assert X.query("ks_cache_hits") == 0 and X.query("transcipher_evaluated") == 2  # the number of counters
    o = mem.empty((3,) + S.O.ct_shape)
    late(torch, delay, s, buf, pinned_of(torch, S.enc_key), lambda: X.transcipher(buf, cw, ncw, ids, o), measured)
    assert (mem.to_host(o) == ra).all() and kc.counts(X) == (0, 2)
    X.close()


def test_result_is_there_on_return(orc, api, lib, torch, S10, monkeypatch):
    """after a synchronous entry point returns, a synchronous copy on the DEFAULT stream reads the final words: torch's streams are
    non-blocking, so nothing but the call's own final wait orders that copy behind the work"""
    S, O = S10, S10.O
    s = torch.cuda.Stream()
    mem = Mem(torch, s)
    cw = kc.words(S, 5, 95)
    X0 = ctx(api, lib, S, monkeypatch, HHE_STREAMS=2, HHE_CHUNK=2)
    want = kc.run(X0, S, Mem(torch), cw, NCW, IDS)
    X0.close()
    X = ctx(api, lib, S, monkeypatch, stream=s, HHE_STREAMS=2, HHE_CHUNK=2)
    key, out = mem.to_dev(S.enc_key), mem.empty((5,) + O.ct_shape)
    low = mem.empty((5, 2, O.L - 1, S.n))
    torch.cuda.synchronize()
    X.transcipher(key, cw, NCW, IDS, out)
    got = out.cpu().numpy().view(np.uint64)  # default stream, no synchronisation in between
    X.mod_switch(out, 2, 5, O.L, O.L - 1, low)
    got_low = low.cpu().numpy().view(np.uint64)
    assert (got == want).all()
    torch.cuda.synchronize()
    assert (got_low == low.cpu().numpy().view(np.uint64)).all() and got_low.any()
    X.close()


def test_two_contexts_two_streams_two_threads(orc, api, lib, torch, S10, monkeypatch):
    S, O = S10, S10.O
    rng = np.random.default_rng(8)
    v, w = rng.integers(0, 4, (2, N_IN)), rng.integers(-8, 9, N_IN)
    vi = np.stack([O.encrypt(S.pk, O.encode(v[i]), 151 + i) for i in range(2)])
    wc = O.encrypt(S.pk, O.encode(w % S.t), 153)
    cws = [kc.words(S, 5, 96 + k) for k in range(2)]

    def work(X, mem, k, res):
        try:
            ks = X.keyset()
            ks.set_relin(S.rk)
            for e, key in zip(S.gk.elts, S.gk.keys):
                ks.set_galois(int(e), key)
            out = mem.empty((2,) + O.ct_shape)
            tr = kc.run(X, S, mem, cws[k], NCW, IDS)
            X.fc_row(mem.to_dev(vi), mem.to_dev(wc[None]), 1, N_IN, out, 2, rk=ks, gk=ks)
            res[k] = (tr, mem.to_host(out))
            ks.close()
        except BaseException as e:  # noqa: a failure in a thread must fail the test
            res[k] = e

    env = dict(HHE_STREAMS=2, HHE_CHUNK=2)
    seq, par = {}, {}
    for k in range(2):
        X = ctx(api, lib, S, monkeypatch, **env)
        work(X, Mem(torch), k, seq)
        X.close()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    Xs = [ctx(api, lib, S, monkeypatch, stream=st, **env) for st in streams]
    threads = [threading.Thread(target=work, args=(Xs[k], Mem(torch, streams[k]), k, par)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k in range(2):
        assert not isinstance(seq[k], BaseException), seq[k]
        assert not isinstance(par[k], BaseException), par[k]
        assert (par[k][0] == seq[k][0]).all() and (par[k][1] == seq[k][1]).all(), k
    assert (seq[0][1][0] == O.fc_row(vi[0], wc, S.rk, S.gk, N_IN)[0]).all()
    for X in Xs:
        X.close()

#!/usr/bin/env python3
"""The 10 x 784 open FC layer under PLAIN weights in one call against the same layer made from public calls, and against the layer under
encrypted weights, measured on one machine: CoeffModulus::BFVDefault(16384) (L = 8, K = 9), keys generated on the device, `items`
ciphertexts.
  plain          hhe_fc_open_plain_ks: one launch of the key-switch row kernel over the 16 children, one mod-down, the tail, the bias
  composed       hhe_rotate_rows_many_ks (0, -1 .. -15) + hhe_multiply_plain per diagonal + hhe_add_many + the tail + hhe_add_plain
  encrypted      hhe_fc_open_ks on the encryptions of the same diagonals (no bias)
  sum_B / composed_sum_B   the primitive hhe_rotate_plain_sum_ks at n = 16 against rotate_rows_many + multiply_plain + add_many, B = 8, 32
The inputs hold a random value in every slot outside [0, 784).  All three layers are checked against (M x + b) mod t in Python integers
before anything is timed.  Recorded beside the times: the device's hhe_noise_budget of the three outputs, the handle's bytes and its
creation time.  A call time is a host clock around a synchronous call (the composed forms end in hhe_ctx_sync).  All measures run in one
process, warmed up once, then alternated `reps` times.  Sets no threshold.  Writes profiles/fc_plain_time.json (or --out) and prints it.
tools/fc_plain_time.py [--reps 5] [--items 32] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

api = importlib.import_module("privacy-preserving-ml-through-hhe_amd.api")


def timed(fn):
    t0 = time.perf_counter()
    fn()  # synchronous
    return time.perf_counter() - t0


def galois_elt(n, step):
    return pow(3, step if step > 0 else n // 2 + step, 2 * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--logn", type=int, default=14)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_plain_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = api.load_library()
    logn, n, B, t = a.logn, 1 << a.logn, a.items, 65537
    rows, cols = 10, 784
    dev = "cuda:0"
    empty = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
    to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).to(dev)
    q = api.bfv_default_coeff_modulus(n, lib)
    X = api.Context(logn, q, t, lib=lib)
    L, K = X.L, X.K
    d_sk, d_pk = empty(K, n), empty(2, K, n)
    X.keygen_secret(os.urandom(32), d_sk)
    X.keygen_public(d_sk, os.urandom(32), d_pk)
    sk = d_sk.cpu().numpy().view(np.uint64)
    ks = X.keyset()
    ks.generate_relin(d_sk, os.urandom(32))
    steps = api.fc_open_galois_steps(n, rows, cols, lib)
    ks.generate_galois(d_sk, os.urandom(32), elts=sorted(set(galois_elt(n, s) for s in steps)))
    r, c = api.fc_open_shape(n, rows, cols, lib)
    rng = np.random.default_rng(1)
    M = (rng.integers(-8, 9, (rows, cols)) % t).astype(np.uint64)
    bias = rng.integers(0, t, rows).astype(np.uint64)
    x = rng.integers(0, 4, (B, cols))
    want = (x @ M.astype(np.int64).T) % t
    want_b = (want + bias.astype(np.int64)) % t
    diag = api.fc_open_diagonals(t, M, lib)   # [r][c]

    def encode(slot_rows):
        plain = empty(len(slot_rows), n)
        X.encode(to_dev(slot_rows), len(slot_rows), slot_rows.shape[1], plain)
        return plain

    def encrypt(slot_rows, fill=False):
        k = len(slot_rows)
        vals = rng.integers(0, t, (k, n)).astype(np.uint64) if fill else np.zeros((k, n), np.uint64)
        vals[:, :slot_rows.shape[1]] = slot_rows
        ct = empty(k, 2, L, n)
        X.encrypt(d_pk, encode(vals), os.urandom(32), k, ct)
        return ct
    vi = encrypt(x.astype(np.uint64), fill=True)
    t0 = time.perf_counter()
    mat = X.plain_fc_open(M, bias)
    create_s = time.perf_counter() - t0
    enc = X.enc_matrix_open(encrypt(diag), rows, cols)
    d_diag = encode(diag)          # [r][N] plaintexts of the diagonals
    d_bias = encode(bias[None])
    rot_steps = [-e for e in range(r)]
    ct = lambda b=B: empty(b, 2, L, n)
    o_plain, o_comp, o_enc, tmp = ct(), ct(), ct(), ct()
    rot = empty(r, B, 2, L, n)

    def rot_mul_sum(src, dst, buf, b):
        X.rotate_rows_many(src, rot_steps, buf, b, gk=ks)
        for e in range(r):
            X.multiply_plain(buf[e], d_diag[e:e + 1], buf[e], b, bcast=True)
        X.add_many(buf, r, dst, b)

    def plain():
        mat.apply(vi, B, gk=ks, out=o_plain)

    def composed():
        rot_mul_sum(vi, o_comp, rot, B)
        s = r
        while s < c:
            X.rotate_rows(o_comp, s, tmp, B, gk=ks)
            X.add(o_comp, tmp, o_comp, B)
            s *= 2
        X.add_plain(o_comp, d_bias, o_comp, B, bcast=True)
        X.sync()

    def encrypted():
        enc.apply_open(vi, B, rk=ks, gk=ks, out=o_enc)
    prim = {}
    rows16 = X.plain_rows(diag)
    for b in (8, 32):
        prim[b] = (encrypt(rng.integers(0, t, (b, 8)).astype(np.uint64), fill=True), ct(b), ct(b), empty(r, b, 2, L, n))

    def sum_at(b):
        return lambda: X.rotate_plain_sum(prim[b][0], rows16, rot_steps, prim[b][1], b, gk=ks)

    def composed_sum_at(b):
        def run():
            rot_mul_sum(prim[b][0], prim[b][2], prim[b][3], b)
            X.sync()
        return run
    measures = {"plain": plain, "composed": composed, "encrypted": encrypted}
    for b in (8, 32):
        measures["sum_%d" % b] = sum_at(b)
        measures["composed_sum_%d" % b] = composed_sum_at(b)
    queries = {}
    for name, fn in measures.items():  # warm-up: workspaces, the lazy tables of the keys
        fn()
        if name == "plain":
            queries = {w: int(X.query(w)) for w in ("plain_sum_launches", "plain_sum_mod_downs", "plain_sum_fallbacks", "plain_sum_fold")}
    torch.cuda.synchronize()
    d_vals = empty(B, n)

    def slots(o, b=B):
        X.decrypt(sk, o, b, d_vals[:b])
        return d_vals[:b].cpu().numpy().view(np.uint64)
    assert (slots(o_plain)[:, :rows].astype(np.int64) == want_b).all(), "plain: the layer does not return (M x + b) mod t"
    assert (slots(o_comp)[:, :rows].astype(np.int64) == want_b).all(), "composed: the layer does not return (M x + b) mod t"
    assert (slots(o_enc)[:, :rows].astype(np.int64) == want).all(), "encrypted: the layer does not return (M x) mod t"
    for b in (8, 32):
        assert (slots(prim[b][1], b) == slots(prim[b][2], b)).all(), "the primitive and its composition decrypt differently"

    def bud(o, b=B):
        v = X.noise_budget(sk, o, b)
        return dict(min_bits=int(v.min()), max_bits=int(v.max()))
    budgets = dict(input=bud(vi), plain=bud(o_plain), composed=bud(o_comp), encrypted=bud(o_enc),
                   sum_32=bud(prim[32][1], 32), composed_sum_32=bud(prim[32][2], 32))
    times = {k: [] for k in measures}
    for _ in range(a.reps):  # alternated
        for k, fn in measures.items():
            times[k].append(timed(fn))
    res = dict(backend=lib.hhe_backend().decode(), device=torch.cuda.get_device_name(0), items=B, logn=logn, L=L, K=K, shape=[rows, cols],
               r=r, c=c, reps=a.reps, queries=queries, noise_budget=budgets, handle_bytes=mat.bytes, handle_create_s=create_s,
               enc_handle_bytes=enc.bytes, measures={})
    for k, ts in times.items():
        res["measures"][k] = dict(call_s=ts, call_median_s=statistics.median(ts), call_min_s=min(ts), call_max_s=max(ts))
    med = {k: v["call_median_s"] for k, v in res["measures"].items()}
    res["per_sample_ms"] = {k: 1e3 * med[k] / B for k in ("plain", "composed", "encrypted")}
    res["composed_over_plain"] = med["composed"] / med["plain"]
    res["encrypted_over_plain"] = med["encrypted"] / med["plain"]
    for b in (8, 32):
        res["composed_sum_over_sum_%d" % b] = med["composed_sum_%d" % b] / med["sum_%d" % b]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The packed encrypted FC layer with one BEHZ floor per item against its per-product forms, measured on one machine:
CoeffModulus::BFVDefault(16384) (L = 8, K = 9), keys generated on the device, the 10 x 784 layer on `items` ciphertexts, ONE handle.
  chain / hoisted          hhe_fc_packed_ks / hhe_fc_packed_hoisted_ks: r floors per item
  sum_chain / sum_hoisted  hhe_fc_packed_sum_ks with hoisted 0 / 1: one floor per item
  multiply_sum / multiply_add_many   hhe_multiply_sum at K = 16, B = 8 against 16 hhe_multiply calls and one hhe_add_many
All four layers are checked against (M x) mod t in Python integers before anything is timed.  Recorded beside the times: the device's
hhe_noise_budget of every form's results and the counters.  A call time is a host clock around a synchronous call (the primitives end
in hhe_ctx_sync).  All measures run in one process, warmed up once, then alternated `reps` times.  Sets no threshold.  Writes
profiles/fc_sum_time.json (or --out) and prints it.
tools/fc_sum_time.py [--reps 5] [--items 32] [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_sum_time.json"))
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
    r, c = api.fc_packed_shape(n, rows, cols, lib)
    d_sk, d_pk = empty(K, n), empty(2, K, n)
    X.keygen_secret(os.urandom(32), d_sk)
    X.keygen_public(d_sk, os.urandom(32), d_pk)
    sk = d_sk.cpu().numpy().view(np.uint64)
    ks = X.keyset()
    ks.generate_relin(d_sk, os.urandom(32))
    ks.generate_galois(d_sk, os.urandom(32))   # the default set: -c, 1 and the tail
    extra = [galois_elt(n, s) for s in range(1, r) if not ks.has_galois(galois_elt(n, s))]
    ks.generate_galois(d_sk, os.urandom(32), elts=extra)
    rng = np.random.default_rng(1)
    M = rng.integers(-8, 9, (rows, cols)) % t
    x = rng.integers(0, 4, (B, cols))
    want = (x @ M.T) % t

    def encrypt(slot_rows):
        k = len(slot_rows)
        vals = np.zeros((k, n), np.uint64)
        vals[:, :slot_rows.shape[1]] = slot_rows
        plain, ct = empty(k, n), empty(k, 2, L, n)
        X.encode(to_dev(vals), k, n, plain)
        X.encrypt(d_pk, plain, os.urandom(32), k, ct)
        return ct
    vi = encrypt(x.astype(np.uint64))
    mat = X.enc_matrix(encrypt(api.fc_packed_diagonals(t, M.astype(np.uint64), lib)), rows, cols)
    outs = {k: empty(B, 2, L, n) for k in ("chain", "hoisted", "sum_chain", "sum_hoisted")}
    d_vals = empty(B, n)
    KS, BS = 16, 8   # the primitive: 16 addends of 8 items
    pa = encrypt(rng.integers(0, t, (KS * BS, 8)).astype(np.uint64)).reshape(KS, BS, 2, L, n)
    pb = encrypt(rng.integers(0, t, (KS * BS, 8)).astype(np.uint64)).reshape(KS, BS, 2, L, n)
    p_sum, p_prod, p_add = empty(BS, 3, L, n), empty(KS, BS, 3, L, n), empty(BS, 3, L, n)

    def multiply_sum():
        X.multiply_sum(pa, pb, KS, p_sum, BS)
        X.sync()

    def multiply_add_many():
        for k in range(KS):
            X.multiply(pa[k], pb[k], p_prod[k], BS)
        X.add_many(p_prod, KS, p_add, BS, size=3)
        X.sync()
    measures = {
        "chain": lambda: mat.apply(vi, B, rk=ks, gk=ks, out=outs["chain"]),
        "hoisted": lambda: mat.apply_hoisted(vi, B, rk=ks, gk=ks, out=outs["hoisted"]),
        "sum_chain": lambda: mat.apply_sum(vi, B, rk=ks, gk=ks, out=outs["sum_chain"], hoisted=False),
        "sum_hoisted": lambda: mat.apply_sum(vi, B, rk=ks, gk=ks, out=outs["sum_hoisted"], hoisted=True),
        "multiply_sum": multiply_sum,
        "multiply_add_many": multiply_add_many,
    }
    queries = {}
    for name, fn in measures.items():  # warm-up: workspaces, the lazy tables of the keys
        before = int(X.query("multiply_sum_launches")), int(X.query("add_many_launches"))
        fn()
        queries[name] = dict(multiply_sum_launches=int(X.query("multiply_sum_launches")) - before[0],
                             add_many_launches=int(X.query("add_many_launches")) - before[1])
        if name in outs:
            queries[name].update(fc_packed_floors=int(X.query("fc_packed_floors")), fc_packed_key_switches=int(X.query("fc_packed_key_switches")))
    torch.cuda.synchronize()
    budgets = {}
    for name, o in outs.items():
        X.decrypt(sk, o, B, d_vals)
        got = d_vals.cpu().numpy().view(np.uint64)[:, :rows].astype(np.int64)
        assert (got == want).all(), name + ": the layer does not return (M x) mod t"
        bud = X.noise_budget(sk, o, B)
        budgets[name] = dict(min_bits=int(bud.min()), max_bits=int(bud.max()))
    times = {k: [] for k in measures}
    for _ in range(a.reps):  # alternated
        for k, fn in measures.items():
            times[k].append(timed(fn))
    res = dict(backend=lib.hhe_backend().decode(), device=torch.cuda.get_device_name(0), items=B, logn=logn, L=L, K=K, rows=rows, cols=cols, r=r, c=c,
               reps=a.reps, behz_sum_cap=int(X.query("behz_sum_cap")), multiply_sum_fold_q=int(X.query("multiply_sum_fold_q")),
               multiply_sum_fold_bsk=int(X.query("multiply_sum_fold_bsk")), primitive=dict(K=KS, B=BS), queries=queries, noise_budget=budgets,
               measures={})
    for k, ts in times.items():
        res["measures"][k] = dict(call_s=ts, call_median_s=statistics.median(ts), call_min_s=min(ts), call_max_s=max(ts))
    med = {k: v["call_median_s"] for k, v in res["measures"].items()}
    res["per_sample_ms"] = {k: 1e3 * med[k] / B for k in outs}
    res["chain_over_sum_chain"] = med["chain"] / med["sum_chain"]
    res["hoisted_over_sum_hoisted"] = med["hoisted"] / med["sum_hoisted"]
    res["multiply_add_many_over_multiply_sum"] = med["multiply_add_many"] / med["multiply_sum"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

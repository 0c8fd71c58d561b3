#!/usr/bin/env python3
"""Modulus switching of finished results, measured on one machine: 160 result ciphertexts (16 samples x 10 neurons) at
CoeffModulus::BFVDefault(16384), L = 8, and the same batch under the 29-prime chain of N = 65536 used at N = 16384 (L = 28).
  switch   hhe_mod_switch 8 -> 1 and 8 -> 4 (28 -> 1 and 28 -> 14): call time = host clock around `inner` synchronous calls (launch and
           synchronise included: a call time, not a kernel time), and the bytes the algorithm needs,
           (limbs_in + limbs_out) * size * B * N * 8, over that call time, against 8 TB/s
  decrypt  hhe_decrypt at L against hhe_decrypt_level at 1 on the switched batch (L = 8 only)
  bytes    Ciphertext::save size per result at every level (uncompressed)
All measures run in one process, warmed up once each, then alternated `reps` times; a sample repeats its call until it lasts about
`--window` seconds (at least `--inner` calls).  Sets no threshold.  Writes profiles/mod_switch_time.json and prints it.
tools/mod_switch_time.py [--reps 7] [--inner 20] [--window 0.05] [--items 160]"""
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
PEAK = 8e12  # HBM bytes/s of the MI355X


def timed(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()  # every call ends in a device synchronise
    return (time.perf_counter() - t0) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--window", type=float, default=0.05, help="seconds one timed sample lasts")
    ap.add_argument("--items", type=int, default=160)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = api.load_library()
    logn, n, B, t = 14, 1 << 14, a.items, 65537
    dev = "cuda:0"
    empty = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)

    # L = 8: real results (device keys, device encryptions), so the decryptions mean something
    q8 = api.bfv_default_coeff_modulus(n, lib)
    X8 = api.Context(logn, q8, t, lib=lib)
    L8 = X8.L
    d_sk, d_pk = empty(X8.K, n), empty(2, X8.K, n)
    X8.keygen_secret(os.urandom(32), d_sk)
    X8.keygen_public(d_sk, os.urandom(32), d_pk)
    sk = d_sk.cpu().numpy().view(np.uint64)
    vals = np.random.default_rng(1).integers(0, t, (B, n), dtype=np.uint64)
    d_plain, ct8 = empty(B, n), empty(B, 2, L8, n)
    X8.encode(torch.from_numpy(vals.view(np.int64)).to(dev), B, n, d_plain)
    X8.encrypt(d_pk, d_plain, os.urandom(32), B, ct8)
    low1, low4, d_vals = empty(B, 2, 1, n), empty(B, 2, 4, n), empty(B, n)

    # L = 28: words below their primes (the switch does the same work on any words)
    q28 = api.bfv_default_coeff_modulus(65536, lib)
    X28 = api.Context(logn, q28, t, lib=lib)
    L28 = X28.L
    rng = np.random.default_rng(2)
    poly = np.stack([rng.integers(0, q28[j], n, dtype=np.uint64) for j in range(L28)])
    ct28 = torch.from_numpy(poly.view(np.int64)).to(dev).repeat(B * 2, 1, 1).reshape(B, 2, L28, n).contiguous()
    l28_1, l28_14 = empty(B, 2, 1, n), empty(B, 2, 14, n)

    measures = {
        "switch_8_to_1": (lambda: X8.mod_switch(ct8, 2, B, L8, 1, low1), (L8 + 1) * 2 * B * n * 8),
        "switch_8_to_4": (lambda: X8.mod_switch(ct8, 2, B, L8, 4, low4), (L8 + 4) * 2 * B * n * 8),
        "switch_28_to_1": (lambda: X28.mod_switch(ct28, 2, B, L28, 1, l28_1), (L28 + 1) * 2 * B * n * 8),
        "switch_28_to_14": (lambda: X28.mod_switch(ct28, 2, B, L28, 14, l28_14), (L28 + 14) * 2 * B * n * 8),
        "decrypt_at_8": (lambda: X8.decrypt(sk, ct8, B, d_vals), None),
        "decrypt_level_1": (lambda: X8.decrypt_level(sk, low1, 1, B, d_vals), None),
    }
    for fn, _ in measures.values():  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    assert (d_vals.cpu().numpy().view(np.uint64) == vals).all(), "level-1 decryption of the switched results"
    X8.decrypt(sk, ct8, B, d_vals)
    assert (d_vals.cpu().numpy().view(np.uint64) == vals).all()
    inner = {k: max(a.inner, int(a.window / timed(fn, 5)) + 1) for k, (fn, _) in measures.items()}  # calls per sample, from a first estimate
    times = {k: [] for k in measures}
    for _ in range(a.reps):  # alternated
        for k, (fn, _) in measures.items():
            times[k].append(timed(fn, inner[k]))
    res = dict(backend=lib.hhe_backend().decode(), device=torch.cuda.get_device_name(0), items=B, logn=logn, reps=a.reps, window_s=a.window, calls_per_sample=inner,
               peak_bytes_per_s=PEAK, measures={}, saved_bytes_per_result={})
    for k, (_, nbytes) in measures.items():
        med = statistics.median(times[k])
        m = dict(call_s=times[k], call_median_s=med, call_min_s=min(times[k]), call_max_s=max(times[k]))
        if nbytes:
            m.update(bytes=nbytes, bytes_per_call_s=nbytes / med, bytes_per_call_s_over_peak=nbytes / med / PEAK)  # over CALL time
        res["measures"][k] = m
    for l in range(1, L8 + 1):
        lo = empty(1, 2, l, n)
        X8.mod_switch(ct8, 2, 1, L8, l, lo)
        res["saved_bytes_per_result"][str(l)] = len(X8.seal_save_ciphertext_level(lo, 2, l, bytes(32)))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mod_switch_time.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

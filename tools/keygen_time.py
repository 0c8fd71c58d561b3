#!/usr/bin/env python3
"""Key generation, device against CPU oracle, on one machine: all default Galois keys of create_galois_keys() plus the relinearization
key, at N = 2^15 with 4 x 60-bit primes (the benchmarked parameters) and at CoeffModulus::BFVDefault(16384).
  device  hhe_keyset_generate_galois (default elements) + hhe_keyset_generate_relin into a key set, ending in a device synchronise
          (the keys stay in HBM, where the evaluator wants them)
  oracle  oracle.keygen_galois / keygen_relin for the same element list on the host CPUs (its keys would still have to cross PCIe)
One warm-up of each, then the two alternated.  Sets no threshold.  Writes profiles/keygen_time.json and prints it.
tools/keygen_time.py [--reps 3] [--params config2,default16384]"""
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
import oracle as orc

api = importlib.import_module("privacy-preserving-ml-through-hhe_amd.api")


def one(lib, name, reps):
    logn = 15 if name == "config2" else 14
    n = 1 << logn
    q = orc.coeff_modulus_create(n, [60] * 4) if name == "config2" else api.bfv_default_coeff_modulus(n, lib)
    O, X = orc.Oracle(logn, q, 65537), api.Context(logn, q, 65537, lib=lib)
    elts = list(dict.fromkeys(int(e) for e in O.galois_elts_all()))
    d_sk = torch.zeros((O.K, n), dtype=torch.int64, device="cuda:0")
    X.keygen_secret(os.urandom(32), d_sk)
    sk = d_sk.cpu().numpy().view(np.uint64)

    def device():
        ks = X.keyset()
        t0 = time.perf_counter()
        ks.generate_galois(d_sk, os.urandom(32))
        ks.generate_relin(d_sk, os.urandom(32))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert all(ks.has_galois(e) for e in elts) and ks.has_relin()
        ks.close()
        return dt

    def oracle():
        t0 = time.perf_counter()
        O.keygen_galois(sk, elts, 7)
        O.keygen_relin(sk, 3)
        return time.perf_counter() - t0

    device(), oracle()  # warm-up
    dev, cpu = [], []
    for _ in range(reps):
        dev.append(device())
        cpu.append(oracle())
    words = (len(elts) + 1) * O.L * 2 * O.K * n
    return dict(params=name, logn=logn, primes=len(q), keys=len(elts) + 1, key_bytes=words * 8, device_s=dev, oracle_s=cpu,
                device_median_s=statistics.median(dev), oracle_median_s=statistics.median(cpu))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--params", default="config2,default16384")
    a = ap.parse_args()
    lib = api.load_library()
    res = dict(backend=lib.hhe_backend().decode(), device=torch.cuda.get_device_name(0), runs=[one(lib, p, a.reps) for p in a.params.split(",") if p])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "keygen_time.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

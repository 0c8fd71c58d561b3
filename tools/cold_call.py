#!/usr/bin/env python3
"""Calls that have to evaluate the keystream, bench.py's config 2 (N=2^15, batch 256, counter 0), as one JSON line: the first call of
a fresh context (block tables + chain), then calls on that context under key ciphertexts it has not seen (tables resident: the chain,
plus whatever the library does to keep the keystream), then one repeat.  tools/cold_call.py [new keys]; HHE_LIB selects the library."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
api = importlib.import_module("privacy-preserving-ml-through-hhe_amd.api")
R = int(sys.argv[1]) if len(sys.argv) > 1 else 5
logn, q, t, B = 15, bench.Q_CONFIG2, 65537, 256
n, L = 1 << logn, len(bench.Q_CONFIG2) - 1
X = api.Context(logn, q, t)
rng = np.random.default_rng(1234)
X.set_relin_key(bench.synthetic_keys(rng, q, n))
for step in (-1, 128, 0):
    X.set_galois_key(X.query("galois_elt", step), bench.synthetic_keys(rng, q, n))
keys = [torch.from_numpy(bench.synthetic_ct(rng, q, n).view(np.int64)).cuda() for _ in range(R + 1)]
cw = rng.integers(0, t, size=(B, 128), dtype=np.uint64)
ncw, bidx = np.full(B, 128, np.uint32), np.zeros(B, np.uint64)
out = torch.zeros((B, 2, L, n), dtype=torch.int64, device="cuda")
X.reserve(B)


def call(k):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    X.transcipher(keys[k], cw, ncw, bidx, out)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


first = call(0)
new_key = [call(k) for k in range(1, R + 1)]
print(json.dumps({"workload": "config 2, batch 256, counter 0", "first_call_of_a_fresh_context_ms": first, "calls_under_a_new_key_ciphertext_ms": new_key,
                  "new_key_median_ms": float(np.median(new_key)), "repeat_ms": call(R), "evaluated_last": X.query("transcipher_evaluated"),
                  "transcipher_unique_last": X.query("transcipher_unique")}))

#!/usr/bin/env python3
"""tests/golden/fc784_n32768.json, fc784_n16384.json, fc8192_n16384.json: SHA-256 per (item, polynomial, limb) of the oracle's
FC rows at the shapes of parity_common.FC_SHAPES -- 784 inputs at the benchmarked parameters (N = 2^15, CoeffModulus::Create(32768,
{60 x 4})) and at the deployed ones (N = 2^14, BFVDefault(16384)), and 8192 inputs at N = 2^14 / {60 x 3}, where one Galois
element of the library's rotation trie collects more leaves than one integer sum may hold.  Computed once on the CPU oracle
(oracle/hhe_oracle.c: the literal loop of n_in - 1 rotate_rows calls, its key-switch count is recorded per row); one process per
row, minutes each.  Compared by tests/test_fc_shapes.py.  Keys and inputs: parity_common.fc_shape_setup / fc_shape_inputs
(Setup seeds sk 1, pk 2, rk 3, gk 7; default_rng(seed); encrypt seeds 100 + b, 200 + r).
usage: make_fc784.py [name ...]   (default: all three)"""
import json, os, sys
from concurrent.futures import ProcessPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def row(job):
    name, b = job
    import oracle as orc
    import parity_common as pc
    p = pc.FC_SHAPES[name]
    S = pc.fc_shape_setup(orc, name)
    _, _, vi, wc = pc.fc_shape_inputs(S, name, items=[b])
    ref, ks = S.O.fc_row(vi[b], wc[b % p["W"]], S.rk, S.gk, p["n_in"])
    print(name, b, ks, flush=True)
    return name, b, ks, pc.limb_hashes(ref)


if __name__ == "__main__":
    import oracle as orc
    import parity_common as pc
    orc.build()
    names = sys.argv[1:] or list(pc.FC_SHAPES)
    jobs = sorted(((n, b) for n in names for b in range(pc.FC_SHAPES[n]["B"])), key=lambda j: -pc.FC_SHAPES[j[0]]["n_in"])
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1, len(jobs))) as ex:
        res = list(ex.map(row, jobs))
    for n in names:
        p = pc.FC_SHAPES[n]
        mine = sorted(r for r in res if r[0] == n)
        q = p["primes"] if "primes" in p else orc.coeff_modulus_create(1 << p["logn"], p["bits"])
        params = (f"N={1 << p['logn']}, q={'BFVDefault' if 'primes' in p else 'CoeffModulus::Create'}({q}), t=65537, n_in={p['n_in']}, "
                  f"B={p['B']} items, W={p['W']} weight rows (item i uses row i % W), Setup seeds (sk 1, pk 2, rk 3, gk 7), Galois keys = "
                  f"create_galois_keys() without arguments, v in [0,4) and w in [-8,9) from default_rng({p['seed']}), encrypt seeds 100+b / 200+r; "
                  f"oracle key switches per row (relinearize not counted): {[r[2] for r in mine]}")
        json.dump({"params": params, "key_switches": [r[2] for r in mine], "items": [r[3] for r in mine]},
                  open(os.path.join(ROOT, "tests", "golden", n + ".json"), "w"), indent=1)

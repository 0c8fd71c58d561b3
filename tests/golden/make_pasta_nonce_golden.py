"""Generate tests/golden/pasta_plain_nonce.json from the REFERENCE's own plain PASTA-3 code, at nonces other than the one its
homomorphic side fixes.

Runs only where the reference sources are (`make -C oracle ref` compiles src/pasta/pasta_3_plain.cpp + libs/keccak into
oracle/_ref/libpasta_ref.so; oracle/ref_shim.cpp is the extern "C" driver, and it already takes the nonce).  The fixture is data
only.  Nonces of distinct bytes catch a byte order, a counter past 32 bits catches a truncation, 2^64 - 1 both ends of the range.

Per case: the SHA-256 of the eight matrices, of the round constants and of the keystream block (the comparison is exact either
way; 48 cases in full would be most of a megabyte).
"""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.DEVNULL)
ref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libpasta_ref.so"))
u64p = C.POINTER(C.c_uint64)


def p(a):
    return a.ctypes.data_as(u64p)


NONCES = (0, 1, 0x0102030405060708, 2**64 - 1)
COUNTERS = (0, 1, 2**32 + 5, 2**64 - 1)
cases = []
for t in (65537, 8088322049, 1096486890805657601):  # configs/config.cpp:19-26
    key = np.array([(i * 2654435761 + 12345) % t for i in range(256)], dtype=np.uint64)
    for nonce in NONCES:
        for block in COUNTERS:
            mats = np.zeros((4, 2, 128, 128), np.uint64)
            rcs = np.zeros((4, 2, 128), np.uint64)
            ref.ref_pasta_block_randomness(C.c_uint64(t), C.c_uint64(nonce), C.c_uint64(block), p(mats), p(rcs))
            ks = np.zeros(128, np.uint64)
            ref.ref_pasta_keystream(C.c_uint64(t), p(key), C.c_uint64(nonce), C.c_uint64(block), p(ks))
            cases.append({
                "t": t, "nonce": nonce, "block": block,
                "mats_sha256": hashlib.sha256(mats.tobytes()).hexdigest(),
                "rcs_sha256": hashlib.sha256(rcs.tobytes()).hexdigest(),
                "keystream_sha256": hashlib.sha256(ks.tobytes()).hexdigest(),
            })
out = {"generator": "tests/golden/make_pasta_nonce_golden.py (reference pasta_3_plain.cpp built from source)",
       "key_rule": "key[i]=(i*2654435761+12345) mod t, i<256", "randomness": cases}
path = os.path.join(ROOT, "tests", "golden", "pasta_plain_nonce.json")
json.dump(out, open(path, "w"), indent=None, separators=(",", ":"))
print("wrote", path, os.path.getsize(path), "bytes")

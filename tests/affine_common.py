"""Checker of the packed plain-matrix affine layers: SEALZpCipher::packed_matMul / packed_affine (src/pasta/SEAL_Cipher.cpp:522-543)
over `diagonal` (:271-313) and `babystep_giantstep` (:185-267), restated in Python and composed from the oracle's encode, rotate_rows,
multiply_plain, add and add_plain alone.  Shared by the emulator suite (numpy memory) and the GPU suite (torch memory): every comparison
is exact equality of ciphertext words."""
import numpy as np

import parity_common as pc


def hand_steps(n, dim, n1=0, n2=0):
    """add_bsgs_indices / add_diagonal_indices (:337-355) by hand: -dim unless the row is full, +1, then k n1 for 0 < k < n2"""
    steps = ([] if 2 * dim == n else [-dim]) + [1]
    if n1 > 1 and n2 > 1:
        steps += [k * n1 for k in range(1, n2)]
    return steps


def check_slots(n, dim):
    if dim * 2 != n and dim * 4 > n:
        raise RuntimeError("too little slots for matmul implementation!")


def diagonals(M, n):
    """the slot vectors `diagonal` encodes: diag_i[j] = M[j][(i + j) % dim]"""
    dim = len(M)
    return [[int(M[j][(i + j) % dim]) for j in range(dim)] for i in range(dim)]


def bsgs_diagonals(M, n, n1):
    """... and `babystep_giantstep`: diag_i turned right by k n1 (k = i // n1); when the row is not full its first k n1 entries move
    behind the end and leave zeros"""
    dim = len(M)
    out = []
    for i, d in enumerate(diagonals(M, n)):
        r = i // n1 * n1
        if r:
            d = d[len(d) - r:] + d[:len(d) - r]
        if n != 2 * dim:
            d = [0] * r + d[r:] + d[:r]
        out.append(d)
    return out


def packed_affine_ref(O, gk, M, ct, bias=None, bsgs=None):
    """one ciphertext through packed_matMul (+ the bias of packed_affine)"""
    dim, n = len(M), O.n
    check_slots(n, dim)
    use_bsgs = bsgs is not None and bsgs[0] != 1 and bsgs[1] != 1
    state = np.array(ct, dtype=np.uint64, copy=True)
    if n != 2 * dim:
        state = O.add(state, O.rotate_rows(state, -dim, gk)[0])
    if not use_bsgs:
        plains = [O.encode(d) for d in diagonals(M, n)]
        acc = O.multiply_plain(state, plains[0])
        for i in range(1, dim):
            state = O.rotate_rows(state, 1, gk)[0]
            acc = O.add(acc, O.multiply_plain(state, plains[i]))
    else:
        n1, n2 = bsgs
        assert n1 * n2 == dim
        plains = [O.encode(d) for d in bsgs_diagonals(M, n, n1)]
        rot = [state]
        for j in range(1, n1):
            rot.append(O.rotate_rows(rot[j - 1], 1, gk)[0])
        acc = None
        for k in range(n2):
            inner = O.multiply_plain(rot[0], plains[k * n1])
            for j in range(1, n1):
                inner = O.add(inner, O.multiply_plain(rot[j], plains[k * n1 + j]))
            acc = inner if k == 0 else O.add(acc, O.rotate_rows(inner, k * n1, gk)[0])
    if bias is not None:
        acc = O.add_plain(acc, O.encode([int(v) for v in bias]))
    return acc


def seeded_matrix(t, dim, seed):
    """all entries in [1, t) from a fixed seed; the bias too"""
    rng = np.random.default_rng(seed)
    return rng.integers(1, t, size=(dim, dim), dtype=np.uint64), rng.integers(1, t, size=dim, dtype=np.uint64)


def inputs(S, dim, B, seed=0, vals=None):
    """B oracle encryptions with zero slots beyond dim, and their slot values"""
    rng = np.random.default_rng(1000 + seed)
    xs = [np.asarray(vals[b], dtype=np.uint64) if vals is not None else rng.integers(0, S.t, size=dim, dtype=np.uint64) for b in range(B)]
    cts = np.stack([S.O.encrypt(S.pk, S.O.encode(x), 50 + seed * 16 + b) for b, x in enumerate(xs)])
    return cts, xs


def make_setup(orc, logn, q, t, steps, all_galois=False):
    """keys for exactly the steps a layer needs (plus the PASTA base the fixtures always make)"""
    return pc.setup_from_primes(orc, logn, q, t, all_galois=all_galois, extra_steps=steps)


def check_affine(X, S, mem, M, bias, bsgs, B=3, seed=0, in_place=False, gk=None, gk_ref=None, cts=None, refs=None):
    """hhe_packed_affine against the checker, word for word; returns (device words, reference words)"""
    O = S.O
    if cts is None:
        cts, _ = inputs(S, len(M), B, seed)
    mat = X.matrix(M, bias=bias, bsgs=bsgs)
    try:
        d_in = mem.to_dev(cts)
        d_out = d_in if in_place else mem.empty((B,) + O.ct_shape)
        X.packed_affine(d_in, mat, d_out, B, gk=gk)
        got = mem.to_host(d_out)
    finally:
        mat.close()
    if refs is None:
        refs = np.stack([packed_affine_ref(O, gk_ref or S.gk, M, cts[b], bias, bsgs) for b in range(B)])
    for b in range(B):
        assert (got[b] == refs[b]).all(), ("packed_affine differs from the checker", b, bsgs, bias is not None)
    return got, refs


def plain_affine(M, x, bias, t):
    """(M x + b) mod t in Python integers"""
    dim = len(M)
    return [(sum(int(M[i][j]) * int(x[j]) for j in range(dim)) + (int(bias[i]) if bias is not None else 0)) % t for i in range(dim)]

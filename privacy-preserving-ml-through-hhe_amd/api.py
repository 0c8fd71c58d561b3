"""ctypes binding of libhhe_gfx950.so (include/hhe_gfx950.h).

The library is the product: hand-written gfx950 kernels behind a C ABI.  This module
only marshals pointers; device memory comes from PyTorch-ROCm tensors (plumbing).
There is no CPU path: if the HIP library is missing, loading fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libhhe_gfx950.so")
PASTA_T = 128

u64p = C.POINTER(C.c_uint64)


class HheError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hhe error {code}: {msg}")
        self.code = code


# error codes of include/hhe_gfx950.h
ERR_INVALID, ERR_NO_GALOIS_KEY, ERR_TOO_FEW_SLOTS, ERR_DEVICE, ERR_NO_RELIN_KEY = 1, 2, 3, 4, 5
ERR_CAPACITY = 6

_SYMBOLS = [
    "hhe_last_error", "hhe_backend", "hhe_ctx_create", "hhe_bfv_default_coeff_modulus", "hhe_ctx_destroy", "hhe_ctx_set_stream",
    "hhe_ctx_reserve", "hhe_ctx_sync", "hhe_ctx_query", "hhe_set_relin_key", "hhe_set_relin_key_slot", "hhe_set_galois_key",
    "hhe_has_galois_key", "hhe_malloc", "hhe_free", "hhe_copy_h2d", "hhe_copy_d2h", "hhe_ntt",
    "hhe_encode", "hhe_add", "hhe_negate", "hhe_add_plain", "hhe_multiply_plain", "hhe_apply_galois",
    "hhe_rotate_rows", "hhe_rotate_columns", "hhe_multiply", "hhe_relinearize",
    "hhe_pasta3_transcipher", "hhe_pasta3_clear_block_cache", "hhe_mask", "hhe_flatten", "hhe_fc_row", "hhe_decompose",
    "hhe_pasta3_block_randomness", "hhe_pasta3_plain_keystream", "hhe_pasta3_plain_crypt", "hhe_decrypt",
    "hhe_ctx_profile", "hhe_ctx_profile_read", "hhe_relinearize_slot",
    "hhe_seal_load_ciphertext", "hhe_seal_save_ciphertext", "hhe_seal_load_relin_keys", "hhe_seal_load_galois_keys",
    "hhe_pasta3_set_block_cache_limit", "hhe_keyset_create", "hhe_keyset_destroy", "hhe_keyset_set_relin", "hhe_keyset_set_galois", "hhe_keyset_has_galois", "hhe_keyset_has_relin",
    "hhe_apply_galois_ks", "hhe_rotate_rows_ks", "hhe_rotate_columns_ks", "hhe_relinearize_ks", "hhe_pasta3_transcipher_ks",
    "hhe_flatten_ks", "hhe_decompose_ks", "hhe_fc_row_ks", "hhe_seal_load_relin_keys_ks", "hhe_seal_load_galois_keys_ks",
    "hhe_matrix_create", "hhe_matrix_destroy", "hhe_matrix_bytes", "hhe_packed_affine_ks", "hhe_affine_galois_steps",
    "hhe_pasta3_clear_keystream_cache",
    "hhe_sample_poly", "hhe_keygen_secret", "hhe_keygen_public", "hhe_keyset_generate_relin", "hhe_keyset_generate_galois",
    "hhe_keyset_get_relin", "hhe_keyset_get_galois", "hhe_encrypt",
    "hhe_mod_switch", "hhe_decrypt_level", "hhe_seal_save_ciphertext_level", "hhe_seal_load_ciphertext_level",
    "hhe_noise_budget", "hhe_ctx_create_level", "hhe_keyset_derive_level",
    "hhe_pasta3_block_randomness_nonce", "hhe_pasta3_plain_keystream_nonce", "hhe_pasta3_plain_crypt_nonce",
    "hhe_pasta3_transcipher_nonce_ks", "hhe_decompose_nonce_ks", "hhe_pasta3_block_randomness_dev", "hhe_pasta3_prepare_tables",
    "hhe_fc_packed_shape", "hhe_fc_packed_diagonals", "hhe_fc_packed_galois_steps", "hhe_enc_matrix_create", "hhe_enc_matrix_destroy",
    "hhe_enc_matrix_bytes", "hhe_fc_packed_ks", "hhe_add_many",
    "hhe_rotate_rows_many_ks", "hhe_fc_packed_hoisted_ks", "hhe_fc_packed_hoisted_galois_steps",
    "hhe_multiply_sum", "hhe_fc_packed_sum_ks",
    "hhe_fc_open_shape", "hhe_fc_open_diagonals", "hhe_fc_open_galois_steps", "hhe_enc_matrix_create_open", "hhe_fc_open_ks",
    "hhe_square", "hhe_mlp_ks",
    "hhe_plain_rows_create", "hhe_plain_rows_destroy", "hhe_plain_rows_bytes", "hhe_rotate_plain_sum_ks",
    "hhe_plain_fc_create_open", "hhe_plain_fc_destroy", "hhe_plain_fc_bytes", "hhe_fc_open_plain_ks",
]

_FC_PACKED_SYMBOLS = {"hhe_fc_packed_shape", "hhe_fc_packed_diagonals", "hhe_fc_packed_galois_steps", "hhe_enc_matrix_create",
                      "hhe_enc_matrix_destroy", "hhe_enc_matrix_bytes", "hhe_fc_packed_ks", "hhe_add_many"}
_ROT_MANY_SYMBOLS = {"hhe_rotate_rows_many_ks", "hhe_fc_packed_hoisted_ks", "hhe_fc_packed_hoisted_galois_steps"}
_MULT_SUM_SYMBOLS = {"hhe_multiply_sum", "hhe_fc_packed_sum_ks"}
_MLP_SYMBOLS = {"hhe_fc_open_shape", "hhe_fc_open_diagonals", "hhe_fc_open_galois_steps", "hhe_enc_matrix_create_open", "hhe_fc_open_ks",
                "hhe_square", "hhe_mlp_ks"}
_PLAIN_SUM_SYMBOLS = {"hhe_plain_rows_create", "hhe_plain_rows_destroy", "hhe_plain_rows_bytes", "hhe_rotate_plain_sum_ks",
                      "hhe_plain_fc_create_open", "hhe_plain_fc_destroy", "hhe_plain_fc_bytes", "hhe_fc_open_plain_ks"}
_NONCE_SYMBOLS = {"hhe_pasta3_block_randomness_nonce", "hhe_pasta3_plain_keystream_nonce", "hhe_pasta3_plain_crypt_nonce",
                  "hhe_pasta3_transcipher_nonce_ks", "hhe_decompose_nonce_ks", "hhe_pasta3_block_randomness_dev",
                  "hhe_pasta3_prepare_tables"}


# exports a library built from an earlier commit may lack (HHE_LIB selects such a build for A/B runs): bound when present, and the method
# that needs one raises when it is not
_OPTIONAL = {"hhe_pasta3_clear_keystream_cache", "hhe_sample_poly", "hhe_keygen_secret", "hhe_keygen_public", "hhe_keyset_generate_relin",
             "hhe_keyset_generate_galois", "hhe_keyset_get_relin", "hhe_keyset_get_galois", "hhe_encrypt",
             "hhe_mod_switch", "hhe_decrypt_level", "hhe_seal_save_ciphertext_level", "hhe_seal_load_ciphertext_level",
             "hhe_noise_budget", "hhe_ctx_create_level", "hhe_keyset_derive_level"} | _NONCE_SYMBOLS | _FC_PACKED_SYMBOLS | _ROT_MANY_SYMBOLS | _MULT_SUM_SYMBOLS | _MLP_SYMBOLS | _PLAIN_SUM_SYMBOLS


def exported_symbols():
    return list(_SYMBOLS)


def load_library(path=None):
    """Load the C-ABI library.  Default: the in-tree gfx950 build; anything else must be passed explicitly."""
    path = path or os.environ.get("HHE_LIB") or LIB_PATH  # HHE_LIB: another gfx950 build of the same sources (A/B runs)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the gfx950 HIP library is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    if os.path.abspath(path) == os.path.abspath(LIB_PATH) or path == os.environ.get("HHE_LIB"):
        # Device memory and streams are shared with PyTorch-ROCm, so both must sit on ONE HIP runtime:
        # import torch first so libamdhip64.so.7 resolves to the copy torch already loaded (two HSA
        # runtimes in one process cannot both open the GPU).
        import torch  # noqa: F401
    lib = C.CDLL(path)
    for s in _SYMBOLS:
        if s not in _OPTIONAL or hasattr(lib, s):
            getattr(lib, s)  # AttributeError if the ABI is incomplete
    lib.hhe_last_error.restype = C.c_char_p
    lib.hhe_backend.restype = C.c_char_p
    lib.hhe_ctx_query.restype = C.c_uint64
    lib.hhe_ctx_query.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.hhe_malloc.restype = C.c_void_p
    lib.hhe_malloc.argtypes = [C.c_size_t]
    lib.hhe_free.argtypes = [C.c_void_p]
    lib.hhe_ctx_destroy.argtypes = [C.c_void_p]
    lib.hhe_pasta3_clear_block_cache.argtypes = [C.c_void_p]
    if hasattr(lib, "hhe_pasta3_clear_keystream_cache"):
        lib.hhe_pasta3_clear_keystream_cache.argtypes = [C.c_void_p]
        lib.hhe_pasta3_clear_keystream_cache.restype = None
    lib.hhe_keyset_destroy.argtypes = [C.c_void_p]
    lib.hhe_keyset_destroy.restype = None
    lib.hhe_matrix_destroy.argtypes = [C.c_void_p]
    lib.hhe_matrix_destroy.restype = None
    lib.hhe_matrix_bytes.argtypes = [C.c_void_p]
    lib.hhe_matrix_bytes.restype = C.c_size_t
    if hasattr(lib, "hhe_enc_matrix_create"):
        lib.hhe_enc_matrix_destroy.argtypes = [C.c_void_p]
        lib.hhe_enc_matrix_destroy.restype = None
        lib.hhe_enc_matrix_bytes.argtypes = [C.c_void_p]
        lib.hhe_enc_matrix_bytes.restype = C.c_size_t
    if hasattr(lib, "hhe_plain_rows_create"):
        for kind in ("rows", "fc"):
            destroy, nbytes = getattr(lib, "hhe_plain_%s_destroy" % kind), getattr(lib, "hhe_plain_%s_bytes" % kind)
            destroy.argtypes = [C.c_void_p]
            destroy.restype = None
            nbytes.argtypes = [C.c_void_p]
            nbytes.restype = C.c_size_t
    return lib


def _ptr(x):
    """address of a torch tensor / numpy array / raw int"""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, int):
        return C.c_void_p(x)
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return C.c_void_p(x.ctypes.data)
    assert x.is_contiguous()
    return C.c_void_p(x.data_ptr())


def _seed(seed):
    """the 32 seed bytes of a key-generation call or an encryption batch (the only entropy: fresh per call)"""
    seed = bytes(seed)
    assert len(seed) == 32
    return (C.c_uint8 * 32).from_buffer_copy(seed)


def _ks(keyset):
    """handle of a KeySet, or NULL = the context's default set"""
    return keyset.h if keyset is not None else C.c_void_p(0)


class KeySet:
    """One seal::RelinKeys / seal::GaloisKeys object on the device (hhe_keyset): keys with identity."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._chk(ctx.lib.hhe_keyset_create(ctx.h, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.hhe_keyset_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_relin(self, ksk):
        ksk = np.ascontiguousarray(ksk, dtype=np.uint64)
        assert ksk.shape == (self.ctx.L, 2, self.ctx.K, self.ctx.n)
        self.ctx._chk(self.ctx.lib.hhe_keyset_set_relin(self.h, _ptr(ksk)))
        return self

    def set_galois(self, elt, ksk):
        ksk = np.ascontiguousarray(ksk, dtype=np.uint64)
        assert ksk.shape == (self.ctx.L, 2, self.ctx.K, self.ctx.n)
        self.ctx._chk(self.ctx.lib.hhe_keyset_set_galois(self.h, C.c_uint32(elt), _ptr(ksk)))
        return self

    def has_galois(self, elt):
        return bool(self.ctx.lib.hhe_keyset_has_galois(self.h, C.c_uint32(elt)))

    def has_relin(self):
        return bool(self.ctx.lib.hhe_keyset_has_relin(self.h))

    def generate_relin(self, sk, seed):
        """sk: device uint64 [K][N] (Context.keygen_secret); seed: 32 fresh bytes"""
        self.ctx._chk(self.ctx.lib.hhe_keyset_generate_relin(self.h, _ptr(sk), _seed(seed)))
        return self

    def generate_galois(self, sk, seed, elts=None):
        """elts: Galois elements, or None for the default set of create_galois_keys(); all-or-nothing"""
        if elts is None:
            self.ctx._chk(self.ctx.lib.hhe_keyset_generate_galois(self.h, _ptr(sk), C.c_void_p(0), C.c_size_t(0), _seed(seed)))
        else:
            e = np.ascontiguousarray(elts, dtype=np.uint32)
            self.ctx._chk(self.ctx.lib.hhe_keyset_generate_galois(self.h, _ptr(sk), _ptr(e), C.c_size_t(len(e)), _seed(seed)))
        return self

    def get_relin(self):
        ksk = np.zeros((self.ctx.L, 2, self.ctx.K, self.ctx.n), np.uint64)
        self.ctx._chk(self.ctx.lib.hhe_keyset_get_relin(self.h, _ptr(ksk)))
        return ksk

    def get_galois(self, elt):
        ksk = np.zeros((self.ctx.L, 2, self.ctx.K, self.ctx.n), np.uint64)
        self.ctx._chk(self.ctx.lib.hhe_keyset_get_galois(self.h, C.c_uint32(elt), _ptr(ksk)))
        return ksk

    def derive_from(self, src):
        """this set (of a level context, Context.at_level) becomes the projection of `src`, a set higher up the same chain: every key
        src holds, digits I < l and limbs {0..l-1, special}, made on the device; what this set held before is gone"""
        if not hasattr(self.ctx.lib, "hhe_keyset_derive_level"):
            raise RuntimeError("this library build does not export hhe_keyset_derive_level")
        self.ctx._chk(self.ctx.lib.hhe_keyset_derive_level(self.h, src.h))
        return self

    def seal_load_relin_keys(self, blob):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
        used = C.c_size_t(0)
        self.ctx._chk(self.ctx.lib.hhe_seal_load_relin_keys_ks(self.h, buf, C.c_size_t(len(blob)), C.byref(used)))
        return int(used.value)

    def seal_load_galois_keys(self, blob):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
        used, cnt = C.c_size_t(0), C.c_uint32(0)
        self.ctx._chk(self.ctx.lib.hhe_seal_load_galois_keys_ks(self.h, buf, C.c_size_t(len(blob)), C.byref(used), C.byref(cnt)))
        return int(used.value), int(cnt.value)


class Matrix:
    """One public matrix of a packed affine layer on the device (hhe_matrix), with its optional bias."""

    def __init__(self, ctx, M, bias=None, bsgs=None):
        M = np.ascontiguousarray(M, dtype=np.uint64)
        assert M.ndim == 2 and M.shape[0] == M.shape[1]
        self.ctx, self.dim = ctx, M.shape[0]
        self.n1, self.n2 = (int(bsgs[0]), int(bsgs[1])) if bsgs else (0, 0)
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.uint64)
        assert b is None or b.shape == (self.dim,)
        h = C.c_void_p()
        ctx._chk(ctx.lib.hhe_matrix_create(ctx.h, _ptr(M), C.c_size_t(self.dim), _ptr(b), C.c_size_t(self.n1), C.c_size_t(self.n2), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.hhe_matrix_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def nbytes(self):
        return int(self.ctx.lib.hhe_matrix_bytes(self.h))


class EncMatrix:
    """The encrypted weight matrix of a packed encrypted FC layer on the device (hhe_enc_matrix): its r generalized diagonals,
    extended and transformed once.  diag_cts: device uint64 [r][2][L][N], the encryptions of fc_packed_diagonals' slot vectors.
    open: the diagonals that do not wrap (fc_open_diagonals, hhe_enc_matrix_create_open); such a handle takes apply_open and
    Context.mlp, a cyclic one the other three forms."""

    def __init__(self, ctx, diag_cts, rows, cols, open=False):
        self.ctx, self.rows, self.cols, self.open = ctx, int(rows), int(cols), bool(open)
        h = C.c_void_p()
        create = ctx._need("hhe_enc_matrix_create_open" if open else "hhe_enc_matrix_create")
        ctx._chk(create(ctx.h, _ptr(diag_cts), C.c_size_t(rows), C.c_size_t(cols), C.byref(h)))
        self.h = h

    def apply_open(self, ct, B, rk=None, gk=None, out=None):
        """out[b] = the open layer on ct[b] (hhe_fc_open_ks): whatever ct[b] holds outside slots [0, cols) meets an encrypted zero, so
        the output of a previous layer or of a square is a legal input.  out None: in place.  Returns out."""
        out = ct if out is None else out
        self.ctx._chk(self.ctx._need("hhe_fc_open_ks")(self.ctx.h, _ks(rk), _ks(gk), self.h, _ptr(ct), _ptr(out), C.c_size_t(B)))
        return out

    def apply(self, ct, B, rk=None, gk=None, out=None):
        """out[b] = the layer on ct[b] (device [B][2][L][N]; out None: in place); slots [0, rows) of the decryption are (M x) mod t.
        rk / gk: the KeySet the call names (None = the context's default set).  Returns out."""
        out = ct if out is None else out
        self.ctx._chk(self.ctx.lib.hhe_fc_packed_ks(self.ctx.h, _ks(rk), _ks(gk), self.h, _ptr(ct), _ptr(out), C.c_size_t(B)))
        return out

    def apply_hoisted(self, ct, B, rk=None, gk=None, out=None):
        """the layer with its rotation chain hoisted (hhe_fc_packed_hoisted_ks): every rot_i = rotate_rows(x, i, gk); same slots, other words"""
        out = ct if out is None else out
        self.ctx._chk(self.ctx._need("hhe_fc_packed_hoisted_ks")(self.ctx.h, _ks(rk), _ks(gk), self.h, _ptr(ct), _ptr(out), C.c_size_t(B)))
        return out

    def apply_sum(self, ct, B, rk=None, gk=None, out=None, hoisted=False):
        """the layer with one BEHZ floor per item (hhe_fc_packed_sum_ks): the r products are summed before the floor (multiply_sum);
        hoisted: the rotations of apply_hoisted instead of apply's chain.  Same slots, other words."""
        out = ct if out is None else out
        self.ctx._chk(self.ctx._need("hhe_fc_packed_sum_ks")(self.ctx.h, _ks(rk), _ks(gk), self.h, _ptr(ct), _ptr(out), C.c_size_t(B),
                                                             C.c_int(1 if hoisted else 0)))
        return out

    def destroy(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.hhe_enc_matrix_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def bytes(self):
        return int(self.ctx.lib.hhe_enc_matrix_bytes(self.h))


class PlainRows:
    """Plaintexts as the right operands of Context.rotate_plain_sum, resident on the device (hhe_plain_rows): vals [n][count] slot
    values < t, each row encoded, lifted to every prime of the context and transformed once."""

    def __init__(self, ctx, vals):
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        assert vals.ndim == 2
        self.ctx, self.count = ctx, vals.shape[0]
        h = C.c_void_p()
        ctx._chk(ctx._need("hhe_plain_rows_create")(ctx.h, _ptr(vals), C.c_size_t(vals.shape[0]), C.c_size_t(vals.shape[1]), C.byref(h)))
        self.h = h

    def destroy(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.hhe_plain_rows_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def bytes(self):
        return int(self.ctx.lib.hhe_plain_rows_bytes(self.h))


class PlainFc:
    """A rows x cols FC layer under PLAIN weights in the open layout, resident on the device (hhe_plain_fc): M row-major with entries
    < t, bias `rows` words or None."""

    def __init__(self, ctx, M, bias=None):
        M = np.ascontiguousarray(M, dtype=np.uint64)
        assert M.ndim == 2
        self.ctx, (self.rows, self.cols) = ctx, M.shape
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.uint64)
        assert b is None or b.shape == (self.rows,)
        h = C.c_void_p()
        ctx._chk(ctx._need("hhe_plain_fc_create_open")(ctx.h, _ptr(M), C.c_size_t(self.rows), C.c_size_t(self.cols), _ptr(b), C.byref(h)))
        self.h = h

    def apply(self, ct, B, gk=None, out=None):
        """out[b] = the layer on ct[b] (hhe_fc_open_plain_ks; device [B][2][L][N]; out None: in place): slots [0, rows) of the decryption
        are (M x + bias) mod t.  Returns out."""
        out = ct if out is None else out
        self.ctx._chk(self.ctx._need("hhe_fc_open_plain_ks")(self.ctx.h, _ks(gk), self.h, _ptr(ct), _ptr(out), C.c_size_t(B)))
        return out

    def destroy(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.hhe_plain_fc_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    @property
    def bytes(self):
        return int(self.ctx.lib.hhe_plain_fc_bytes(self.h))


class Context:
    """One BFV context on one GPU (hhe_ctx)."""

    def __init__(self, logn, q, t, device=0, lib=None):
        self.lib = lib or load_library()
        self.logn, self.n, self.q, self.t = logn, 1 << logn, [int(v) for v in q], int(t)
        self.K, self.L = len(q), len(q) - 1
        qa = np.asarray(self.q, dtype=np.uint64)
        h = C.c_void_p()
        self._chk(self.lib.hhe_ctx_create(C.c_int(logn), C.c_int(self.K), _ptr(qa), C.c_uint64(t), C.c_int(device), C.byref(h)))
        self.h = h
        self.device = device
        self.ct_shape = (2, self.L, self.n)

    def at_level(self, limbs):
        """the context of the level with `limbs` data primes of this chain (hhe_ctx_create_level): q_0..q_{limbs-1} and the special
        prime.  Independent of this one; what hhe_mod_switch writes at `limbs` are its data-level ciphertexts."""
        if not hasattr(self.lib, "hhe_ctx_create_level"):
            raise RuntimeError("this library build does not export hhe_ctx_create_level")
        h = C.c_void_p()
        self._chk(self.lib.hhe_ctx_create_level(self.h, C.c_int(limbs), C.byref(h)))
        X = Context.__new__(Context)
        X.lib, X.logn, X.n, X.t, X.device = self.lib, self.logn, self.n, self.t, self.device
        X.q = self.q[:limbs] + [self.q[-1]]
        X.K, X.L = limbs + 1, limbs
        X.h = h
        X.ct_shape = (2, X.L, X.n)
        return X

    def _chk(self, rc):
        if rc != 0:
            raise HheError(rc, self.lib.hhe_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.hhe_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def backend(self):
        return self.lib.hhe_backend().decode()

    def query(self, what, i=0):
        return int(self.lib.hhe_ctx_query(self.h, what.encode(), C.c_int(i)))

    def set_stream(self, stream_ptr):
        self._chk(self.lib.hhe_ctx_set_stream(self.h, C.c_void_p(stream_ptr)))

    def reserve(self, B):
        self._chk(self.lib.hhe_ctx_reserve(self.h, C.c_size_t(B)))

    def sync(self):
        self._chk(self.lib.hhe_ctx_sync(self.h))

    def profile(self, enable=True):
        """bracket every launch of the fused key-switch row kernel with timed HIP events on its stream"""
        self._chk(self.lib.hhe_ctx_profile(self.h, C.c_int(1 if enable else 0)))

    def profile_read(self):
        """(kernel name as rocprofv3 prints it, launches, total ms, ciphertexts covered) since the last read"""
        name = C.create_string_buffer(128)
        n, items, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        self._chk(self.lib.hhe_ctx_profile_read(self.h, name, C.c_size_t(128), C.byref(n), C.byref(ms), C.byref(items)))
        return name.value.decode(), int(n.value), float(ms.value), int(items.value)

    def set_relin_key(self, ksk):
        ksk = np.ascontiguousarray(ksk, dtype=np.uint64)
        assert ksk.shape == (self.L, 2, self.K, self.n)
        self._chk(self.lib.hhe_set_relin_key(self.h, _ptr(ksk)))

    def set_galois_key(self, elt, ksk):
        ksk = np.ascontiguousarray(ksk, dtype=np.uint64)
        assert ksk.shape == (self.L, 2, self.K, self.n)
        self._chk(self.lib.hhe_set_galois_key(self.h, C.c_uint32(elt), _ptr(ksk)))

    def has_galois_key(self, elt):
        return bool(self.lib.hhe_has_galois_key(self.h, C.c_uint32(elt)))

    # ---- primitives on device batches (arguments: torch cuda tensors / raw addresses) ----
    def ntt(self, polys, count, mod_base, mod_cycle, inverse=False):
        self._chk(self.lib.hhe_ntt(self.h, _ptr(polys), C.c_size_t(count), C.c_int(mod_base), C.c_int(mod_cycle), C.c_int(int(inverse))))

    def encode(self, vals, B, count, plain):
        self._chk(self.lib.hhe_encode(self.h, _ptr(vals), C.c_size_t(B), C.c_size_t(count), _ptr(plain)))

    def add(self, a, b, out, B, size=2):
        self._chk(self.lib.hhe_add(self.h, _ptr(a), _ptr(b), _ptr(out), C.c_size_t(B), C.c_int(size)))

    def negate(self, a, out, B, size=2):
        self._chk(self.lib.hhe_negate(self.h, _ptr(a), _ptr(out), C.c_size_t(B), C.c_int(size)))

    def add_plain(self, ct, plain, out, B, bcast=False, subtract=False):
        self._chk(self.lib.hhe_add_plain(self.h, _ptr(ct), _ptr(plain), C.c_int(int(bcast)), C.c_int(int(subtract)), _ptr(out), C.c_size_t(B)))

    def multiply_plain(self, ct, plain, out, B, bcast=False):
        self._chk(self.lib.hhe_multiply_plain(self.h, _ptr(ct), _ptr(plain), C.c_int(int(bcast)), _ptr(out), C.c_size_t(B)))

    def keyset(self):
        return KeySet(self)

    # gk / rk: the KeySet the call names (None = the context's default set)
    def apply_galois(self, ct, elt, out, B, gk=None):
        self._chk(self.lib.hhe_apply_galois_ks(self.h, _ks(gk), _ptr(ct), C.c_uint32(elt), _ptr(out), C.c_size_t(B)))

    def rotate_rows(self, ct, step, out, B, gk=None):
        self._chk(self.lib.hhe_rotate_rows_ks(self.h, _ks(gk), _ptr(ct), C.c_int(step), _ptr(out), C.c_size_t(B)))

    def rotate_rows_many(self, ct, steps, out, B, gk=None):
        """out [len(steps)][B][2][L][N], step-major: out[k][b] = rotate_rows(ct[b], steps[k], gk), the rotations hoisted (one set of
        digit transforms per trie node).  Synchronous."""
        arr = (C.c_int * max(len(steps), 1))(*[int(v) for v in steps])
        self._chk(self._need("hhe_rotate_rows_many_ks")(self.h, _ks(gk), _ptr(ct), arr, C.c_size_t(len(steps)), _ptr(out), C.c_size_t(B)))

    def fc_packed_hoisted(self, ct, mat, out, B, rk=None, gk=None):
        """out[b] = the packed encrypted FC layer `mat` (an EncMatrix) on ct[b] with the rotation chain hoisted; out may be ct"""
        return mat.apply_hoisted(ct, B, rk=rk, gk=gk, out=out)

    def fc_packed_sum(self, ct, mat, out, B, rk=None, gk=None, hoisted=False):
        """out[b] = the packed encrypted FC layer `mat` on ct[b] with one floor over the sum of its r products; out may be ct"""
        return mat.apply_sum(ct, B, rk=rk, gk=gk, out=out, hoisted=hoisted)

    def rotate_columns(self, ct, out, B, gk=None):
        self._chk(self.lib.hhe_rotate_columns_ks(self.h, _ks(gk), _ptr(ct), _ptr(out), C.c_size_t(B)))

    def matrix(self, M, bias=None, bsgs=None):
        """resident plain matrix (+ bias) of a packed affine layer; bsgs = (n1, n2) or None for the diagonal method"""
        return Matrix(self, M, bias, bsgs)

    def packed_affine(self, ct, mat, out, B, gk=None):
        """out[b] = M * ct[b] (+ bias) on packed ciphertexts (SEALZpCipher::packed_matMul / packed_affine)"""
        self._chk(self.lib.hhe_packed_affine_ks(self.h, _ks(gk), mat.h, _ptr(ct), _ptr(out), C.c_size_t(B)))

    def enc_matrix(self, diag_cts, rows, cols):
        """resident encrypted matrix of a packed encrypted FC layer from its r diagonal ciphertexts (device [r][2][L][N])"""
        return EncMatrix(self, diag_cts, rows, cols)

    def enc_matrix_open(self, diag_cts, rows, cols):
        """resident encrypted matrix of an open layer from the encryptions of fc_open_diagonals' slot vectors (device [r][2][L][N])"""
        return EncMatrix(self, diag_cts, rows, cols, open=True)

    def plain_rows(self, vals):
        """resident plaintexts of rotate_plain_sum from their slot vectors vals [n][count]"""
        return PlainRows(self, vals)

    def rotate_plain_sum(self, ct, rows, steps, out, B, gk=None):
        """out[b] = sum_k rotate_rows(ct[b], steps[k], gk) * plaintext k of `rows` (a PlainRows), with one mod-down over the sum
        (hhe_rotate_plain_sum_ks); every non-zero step needs a key of its own; out may be ct.  Synchronous."""
        arr = (C.c_int * max(len(steps), 1))(*[int(v) for v in steps])
        self._chk(self._need("hhe_rotate_plain_sum_ks")(self.h, _ks(gk), None if rows is None else rows.h, arr, C.c_size_t(len(steps)),
                                                        _ptr(ct), _ptr(out), C.c_size_t(B)))
        return out

    def plain_fc_open(self, M, bias=None):
        """resident plain-weights open FC layer from its matrix (and bias)"""
        return PlainFc(self, M, bias)

    def square(self, a, out3, B):
        """out3 [B][3][L][N] = Evaluator::square(a) at size 2: the words of multiply(a, a, ..), one operand extension"""
        self._chk(self._need("hhe_square")(self.h, _ptr(a), _ptr(out3), C.c_size_t(B)))

    def mlp(self, handles, ct, out, B, rk=None, gk=None):
        """out[b] = the network on ct[b] (hhe_mlp_ks): handles[0] open, square + relinearize, handles[1] open, ...; every layer of a
        chunk on its lane with no host wait in between.  handles: open EncMatrix objects, rows of one == cols of the next; out may be ct"""
        arr = (C.c_void_p * max(len(handles), 1))(*[None if m is None else m.h for m in handles])
        self._chk(self._need("hhe_mlp_ks")(self.h, _ks(rk), _ks(gk), arr, C.c_size_t(len(handles)), _ptr(ct), _ptr(out), C.c_size_t(B)))
        return out

    def add_many(self, stacked, K, out, B, size=2):
        """out [B][size][L][N] = the sum of the K batches stacked [K][B][size][L][N] (Evaluator::add_many), one launch"""
        self._chk(self._need("hhe_add_many")(self.h, _ptr(stacked), C.c_size_t(K), _ptr(out), C.c_size_t(B), C.c_int(size)))

    def multiply(self, a, b, out3, B):
        self._chk(self.lib.hhe_multiply(self.h, _ptr(a), _ptr(b), _ptr(out3), C.c_size_t(B)))

    def multiply_sum(self, a, b, K, out3, B, b_bcast=False):
        """out3 [B][3][L][N] = the BEHZ floor of the sum of the K tensor products of a [K][B][2][L][N] and b [K][B][2][L][N]
        (b_bcast: [K][1][2][L][N]); K above query("behz_sum_cap") is refused"""
        self._chk(self._need("hhe_multiply_sum")(self.h, _ptr(a), _ptr(b), C.c_size_t(K), C.c_int(1 if b_bcast else 0), _ptr(out3),
                                                 C.c_size_t(B)))

    def relinearize(self, a3, out, B, slot=None, rk=None):
        if rk is not None:
            self._chk(self.lib.hhe_relinearize_ks(self.h, _ks(rk), _ptr(a3), _ptr(out), C.c_size_t(B)))
        elif slot is None:
            self._chk(self.lib.hhe_relinearize(self.h, _ptr(a3), _ptr(out), C.c_size_t(B)))
        else:
            self._chk(self.lib.hhe_relinearize_slot(self.h, C.c_int(slot), _ptr(a3), _ptr(out), C.c_size_t(B)))

    # ---- hot path ----
    def _need(self, name):
        if not hasattr(self.lib, name):
            raise RuntimeError(f"this library has no {name} (built from an earlier commit)")
        return getattr(self.lib, name)

    def transcipher(self, enc_key, cw, ncw, block_index, out, use_bsgs=False, rk=None, gk=None, nonces=None):
        """cw: host uint64 [B][128]; ncw [B]; block_index [B]; enc_key/out device.  nonces [B]: item i runs under the pair
        (nonces[i], block_index[i]) -- a pair encrypts one block, ever; None: the reference's fixed nonce"""
        cw = np.ascontiguousarray(cw, dtype=np.uint64)
        B = cw.shape[0]
        assert cw.shape == (B, PASTA_T)
        ncw = np.ascontiguousarray(ncw, dtype=np.uint32)
        bi = np.ascontiguousarray(block_index, dtype=np.uint64)
        assert ncw.shape == (B,) and bi.shape == (B,)
        if nonces is not None:
            nn = np.ascontiguousarray(nonces, dtype=np.uint64)
            assert nn.shape == (B,)
            self._chk(self._need("hhe_pasta3_transcipher_nonce_ks")(self.h, _ks(rk), _ks(gk), _ptr(enc_key), _ptr(cw), _ptr(ncw), _ptr(nn),
                                                                    _ptr(bi), C.c_size_t(B), C.c_int(int(use_bsgs)), _ptr(out)))
            return
        self._chk(self.lib.hhe_pasta3_transcipher_ks(self.h, _ks(rk), _ks(gk), _ptr(enc_key), _ptr(cw), _ptr(ncw), _ptr(bi), C.c_size_t(B),
                                                     C.c_int(int(use_bsgs)), _ptr(out)))

    def clear_block_cache(self):
        self.lib.hhe_pasta3_clear_block_cache(self.h)

    def clear_keystream_cache(self):
        """drop the keystream ciphertexts kept across transciphering calls (the block tables stay)"""
        if not hasattr(self.lib, "hhe_pasta3_clear_keystream_cache"):
            raise RuntimeError("this library keeps no keystreams across calls (no hhe_pasta3_clear_keystream_cache)")
        self.lib.hhe_pasta3_clear_keystream_cache(self.h)

    def set_block_cache_limit(self, nbytes):
        self._chk(self.lib.hhe_pasta3_set_block_cache_limit(self.h, C.c_size_t(nbytes)))

    def mask(self, ct, mask_vals, out, B):
        mv = np.ascontiguousarray(mask_vals, dtype=np.uint64)
        self._chk(self.lib.hhe_mask(self.h, _ptr(ct), _ptr(mv), C.c_size_t(len(mv)), _ptr(out), C.c_size_t(B)))

    def flatten(self, blocks, nblocks, out, S, gk=None):
        self._chk(self.lib.hhe_flatten_ks(self.h, _ks(gk), _ptr(blocks), C.c_size_t(nblocks), _ptr(out), C.c_size_t(S)))

    def block_randomness_dev(self, nonces, blocks, mats_out, rcs_out):
        """the public randomness of len(nonces) pairs drawn on the device: mats_out device [count][4][2][128][128], rcs_out [count][4][2][128]"""
        nn = np.ascontiguousarray(nonces, dtype=np.uint64)
        bb = np.ascontiguousarray(blocks, dtype=np.uint64)
        assert nn.shape == bb.shape and nn.ndim == 1
        self._chk(self._need("hhe_pasta3_block_randomness_dev")(self.h, _ptr(nn), _ptr(bb), C.c_size_t(len(nn)), _ptr(mats_out), _ptr(rcs_out)))

    def prepare_tables(self, nonces, blocks, use_bsgs=False):
        """build the public tables the cache lacks for these pairs; returns how many pairs anything was built for"""
        nn = np.ascontiguousarray(nonces, dtype=np.uint64)
        bb = np.ascontiguousarray(blocks, dtype=np.uint64)
        assert nn.shape == bb.shape and nn.ndim == 1
        built = C.c_size_t(0)
        self._chk(self._need("hhe_pasta3_prepare_tables")(self.h, _ptr(nn), _ptr(bb), C.c_size_t(len(nn)), C.c_int(int(use_bsgs)), C.byref(built)))
        return int(built.value)

    def decompose(self, enc_key, records, out, mask_last=True, rk=None, gk=None, flatten_gk=None, nonces=None):
        """records: host uint64 [S][nwords]; out device [S][2][L][N]; rk / gk: the PASTA_SEAL's keys, flatten_gk: the GaloisKeys of flatten;
        nonces [S]: one per record (None: the reference's fixed nonce)"""
        rec = np.ascontiguousarray(records, dtype=np.uint64)
        S, nwords = rec.shape
        if nonces is not None:
            nn = np.ascontiguousarray(nonces, dtype=np.uint64)
            assert nn.shape == (S,)
            self._chk(self._need("hhe_decompose_nonce_ks")(self.h, _ks(rk), _ks(gk), _ks(flatten_gk), _ptr(enc_key), _ptr(rec), _ptr(nn),
                                                           C.c_size_t(S), C.c_size_t(nwords), C.c_int(int(mask_last)), _ptr(out)))
            return
        self._chk(self.lib.hhe_decompose_ks(self.h, _ks(rk), _ks(gk), _ks(flatten_gk), _ptr(enc_key), _ptr(rec), C.c_size_t(S), C.c_size_t(nwords),
                                            C.c_int(int(mask_last)), _ptr(out)))

    def set_relin_key_slot(self, slot, ksk):
        ksk = np.ascontiguousarray(ksk, dtype=np.uint64)
        self._chk(self.lib.hhe_set_relin_key_slot(self.h, C.c_int(slot), _ptr(ksk)))

    def fc_row(self, vi, w, W, n_inputs, out, B, relin_slot=0, default_galois_only=True, rk=None, gk=None):
        if rk is not None or gk is not None:  # the key objects the CSP names (CSP.cpp:306, 312-316)
            self._chk(self.lib.hhe_fc_row_ks(self.h, _ks(rk), _ks(gk), _ptr(vi), _ptr(w), C.c_size_t(W), C.c_size_t(n_inputs), _ptr(out), C.c_size_t(B)))
            return
        self._chk(self.lib.hhe_fc_row(self.h, _ptr(vi), _ptr(w), C.c_size_t(W), C.c_size_t(n_inputs), C.c_int(relin_slot),
                                      C.c_int(int(default_galois_only)), _ptr(out), C.c_size_t(B)))


    # ---- SEAL 4.0 wire format (parity unpinned, see include/hhe_gfx950.h) ----
    def seal_load_ciphertext(self, blob, out, offset=0):
        """blob: bytes-like; out: device uint64 buffer.  Returns (ct_size, parms_id bytes, consumed)."""
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
        size, used = C.c_size_t(0), C.c_size_t(0)
        pid = (C.c_uint8 * 32)()
        self._chk(self.lib.hhe_seal_load_ciphertext(self.h, C.byref(buf, offset), C.c_size_t(len(blob) - offset), _ptr(out),
                                                    C.c_size_t(out.numel() if hasattr(out, "numel") else out.size),
                                                    C.byref(size), pid, C.byref(used)))
        return int(size.value), bytes(pid), int(used.value)

    def seal_save_ciphertext(self, ct, ct_size, parms_id):
        need = C.c_size_t(0)
        pid = (C.c_uint8 * 32).from_buffer_copy(parms_id)
        words = ct_size * self.L * self.n
        cap = 16 + 32 + 1 + 40 + 16 + 8 + words * 8
        out = (C.c_uint8 * cap)()
        self._chk(self.lib.hhe_seal_save_ciphertext(self.h, _ptr(ct), C.c_size_t(ct_size), pid, out, C.c_size_t(cap), C.byref(need)))
        return bytes(out[:need.value])

    def seal_load_relin_keys(self, blob, slot=0):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
        used = C.c_size_t(0)
        self._chk(self.lib.hhe_seal_load_relin_keys(self.h, C.c_int(slot), buf, C.c_size_t(len(blob)), C.byref(used)))
        return int(used.value)

    def seal_load_galois_keys(self, blob):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
        used, cnt = C.c_size_t(0), C.c_uint32(0)
        self._chk(self.lib.hhe_seal_load_galois_keys(self.h, buf, C.c_size_t(len(blob)), C.byref(used), C.byref(cnt)))
        return int(used.value), int(cnt.value)

    # ---- client / analyst ends ----
    def plain_keystream(self, key, first_block, nblocks, ks_out, nonce=None):
        """key: host uint64 [256]; ks_out device [nblocks][128]; nonce: None = the reference's fixed one"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        assert key.shape == (2 * PASTA_T,)
        if nonce is not None:
            self._chk(self._need("hhe_pasta3_plain_keystream_nonce")(self.h, _ptr(key), C.c_uint64(nonce), C.c_uint64(first_block),
                                                                     C.c_size_t(nblocks), _ptr(ks_out)))
            return
        self._chk(self.lib.hhe_pasta3_plain_keystream(self.h, _ptr(key), C.c_uint64(first_block), C.c_size_t(nblocks), _ptr(ks_out)))

    def plain_crypt(self, key, records, S, nwords, out, decrypt=False, nonces=None):
        """records/out: device uint64 [S][nwords]; nonces [S]: one per record, counters from 0 (None: the reference's fixed nonce)"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        assert key.shape == (2 * PASTA_T,)
        if nonces is not None:
            nn = np.ascontiguousarray(nonces, dtype=np.uint64)
            assert nn.shape == (S,)
            self._chk(self._need("hhe_pasta3_plain_crypt_nonce")(self.h, _ptr(key), _ptr(nn), _ptr(records), C.c_size_t(S), C.c_size_t(nwords),
                                                                 C.c_int(int(decrypt)), _ptr(out)))
            return
        self._chk(self.lib.hhe_pasta3_plain_crypt(self.h, _ptr(key), _ptr(records), C.c_size_t(S), C.c_size_t(nwords),
                                                  C.c_int(int(decrypt)), _ptr(out)))

    def decrypt(self, sk, ct, B, vals_out):
        """sk: host uint64 [K][N] (NTT form, key level); ct device [B][2][L][N]; vals_out device [B][N]"""
        sk = np.ascontiguousarray(sk, dtype=np.uint64)
        assert sk.size >= self.L * self.n
        self._chk(self.lib.hhe_decrypt(self.h, _ptr(sk), _ptr(ct), C.c_size_t(B), _ptr(vals_out)))

    # ---- levels: modulus switching of finished results, and the level-aware ends ----
    def mod_switch(self, ct, size, B, limbs_in, limbs_out, out):
        """ct device [B][size][limbs_in][N] -> out device [B][size][limbs_out][N] (Evaluator::mod_switch_to_inplace)"""
        self._chk(self.lib.hhe_mod_switch(self.h, _ptr(ct), C.c_int(size), C.c_size_t(B), C.c_int(limbs_in), C.c_int(limbs_out), _ptr(out)))

    def decrypt_level(self, sk, ct, limbs, B, vals_out):
        """sk: host uint64 [K][N]; ct device [B][2][limbs][N]; vals_out device [B][N]"""
        sk = np.ascontiguousarray(sk, dtype=np.uint64)
        assert sk.size >= limbs * self.n
        self._chk(self.lib.hhe_decrypt_level(self.h, _ptr(sk), _ptr(ct), C.c_int(limbs), C.c_size_t(B), _ptr(vals_out)))

    def noise_budget(self, sk, ct, B, size=2, limbs=None, with_bits=False):
        """Decryptor::invariant_noise_budget of B ciphertexts.  sk: host uint64 [K][N]; ct device [B][size][limbs][N] (limbs: L when
        None).  Returns the budgets as an int32 array [B], or (budget, norm_bits) with the bit counts of the largest centred noise
        coefficients (uint32 [B]) when with_bits is set"""
        limbs = self.L if limbs is None else limbs
        sk = np.ascontiguousarray(sk, dtype=np.uint64)
        assert sk.size >= max(limbs, 0) * self.n
        budget, bits = np.zeros(B, np.int32), np.zeros(B, np.uint32)
        self._chk(self.lib.hhe_noise_budget(self.h, _ptr(sk), _ptr(ct), C.c_int(size), C.c_int(limbs), C.c_size_t(B), _ptr(budget),
                                            _ptr(bits) if with_bits else _ptr(None)))
        return (budget, bits) if with_bits else budget

    def seal_save_ciphertext_level(self, ct, ct_size, limbs, parms_id):
        need = C.c_size_t(0)
        pid = (C.c_uint8 * 32).from_buffer_copy(parms_id)
        cap = 16 + 32 + 1 + 40 + 16 + 8 + ct_size * max(limbs, 0) * self.n * 8
        out = (C.c_uint8 * cap)()
        self._chk(self.lib.hhe_seal_save_ciphertext_level(self.h, _ptr(ct), C.c_size_t(ct_size), C.c_int(limbs), pid, out, C.c_size_t(cap),
                                                          C.byref(need)))
        return bytes(out[:need.value])

    def seal_load_ciphertext_level(self, blob, out, offset=0):
        """Returns (ct_size, limbs, parms_id bytes, consumed)."""
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
        size, used, limbs = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        pid = (C.c_uint8 * 32)()
        self._chk(self.lib.hhe_seal_load_ciphertext_level(self.h, C.byref(buf, offset), C.c_size_t(len(blob) - offset), _ptr(out),
                                                          C.c_size_t(out.numel() if hasattr(out, "numel") else out.size),
                                                          C.byref(size), C.byref(limbs), pid, C.byref(used)))
        return int(size.value), int(limbs.value), bytes(pid), int(used.value)

    # ---- keys and ciphertexts from a seed (32 fresh bytes per call: the only entropy) ----
    def sample_poly(self, seed, purpose, elt, index, kind, mod_base, mod_count, out):
        """the sampler alone: out device [mod_count][N]; kind 1 ternary, 2 noise, 3 uniform"""
        self._chk(self.lib.hhe_sample_poly(self.h, _seed(seed), C.c_uint32(purpose), C.c_uint32(elt), C.c_uint32(index), C.c_int(kind),
                                           C.c_int(mod_base), C.c_int(mod_count), _ptr(out)))

    def keygen_secret(self, seed, sk_out):
        """sk_out: device [K][N] (NTT form, key level)"""
        self._chk(self.lib.hhe_keygen_secret(self.h, _seed(seed), _ptr(sk_out)))

    def keygen_public(self, sk, seed, pk_out):
        """sk device [K][N]; pk_out device [2][K][N]"""
        self._chk(self.lib.hhe_keygen_public(self.h, _ptr(sk), _seed(seed), _ptr(pk_out)))

    def encrypt(self, pk, plain, seed, B, out, bcast=False):
        """pk device [2][K][N]; plain device [B][N] ([1][N] if bcast); out device [B][2][L][N]"""
        self._chk(self.lib.hhe_encrypt(self.h, _ptr(pk), _ptr(plain), C.c_int(int(bcast)), _seed(seed), C.c_size_t(B), _ptr(out)))


def level_rows(words, limbs):
    """rows {0..limbs-1, K-1} of the limb axis of a key-level object [..][K][N] (sk [K][N], pk [2][K][N], a digit of a key-switch
    key): the object of the level with `limbs` data primes (Context.at_level)"""
    K = words.shape[-2]
    assert 1 <= limbs < K
    if isinstance(words, np.ndarray):
        return np.ascontiguousarray(words[..., list(range(limbs)) + [K - 1], :])
    return words[..., list(range(limbs)) + [K - 1], :].contiguous()


def bfv_default_coeff_modulus(n, lib=None):
    lib = lib or load_library()
    out = np.zeros(64, np.uint64)
    cnt = C.c_size_t(64)
    rc = lib.hhe_bfv_default_coeff_modulus(C.c_size_t(n), _ptr(out), C.byref(cnt))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return [int(v) for v in out[:cnt.value]]


def affine_galois_steps(n, dim, n1=0, n2=0, lib=None):
    """the rotate_rows steps a packed affine layer needs Galois keys for (add_diagonal_indices / add_bsgs_indices)"""
    lib = lib or load_library()
    out = (C.c_int * 64)()
    cnt = C.c_size_t(64)
    rc = lib.hhe_affine_galois_steps(C.c_size_t(n), C.c_size_t(dim), C.c_size_t(n1), C.c_size_t(n2), out, C.byref(cnt))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return [int(v) for v in out[:cnt.value]]


def _lib_fn(lib, name):
    if not hasattr(lib, name):
        raise RuntimeError(f"this library has no {name} (built from an earlier commit)")
    return getattr(lib, name)


def fc_packed_shape(n, rows, cols, lib=None):
    """(r, c) of a rows x cols packed encrypted FC layer at degree n: powers of two, c >= r; HheError when the slots do not suffice"""
    lib = lib or load_library()
    r, c = C.c_size_t(0), C.c_size_t(0)
    rc = _lib_fn(lib, "hhe_fc_packed_shape")(C.c_size_t(n), C.c_size_t(rows), C.c_size_t(cols), C.byref(r), C.byref(c))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return int(r.value), int(c.value)


def fc_packed_diagonals(t, M, lib=None):
    """the generalized diagonals of M (rows x cols, entries < t) as slot vectors [r][c]: d_i[j] = M[j mod r][(j + i) mod c], zero padded"""
    lib = lib or load_library()
    M = np.ascontiguousarray(M, dtype=np.uint64)
    assert M.ndim == 2
    rows, cols = M.shape
    r = 1 << max(rows - 1, 0).bit_length()
    c = max(1 << max(cols - 1, 0).bit_length(), r)
    vals = np.zeros((r, c), np.uint64)
    rc = _lib_fn(lib, "hhe_fc_packed_diagonals")(C.c_uint64(t), _ptr(M), C.c_size_t(rows), C.c_size_t(cols), _ptr(vals))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return vals


def fc_packed_galois_steps(n, rows, cols, lib=None):
    """the rotate_rows steps a packed encrypted FC layer needs Galois keys for, in the order it takes them"""
    lib = lib or load_library()
    out = (C.c_int * 64)()
    cnt = C.c_size_t(64)
    rc = _lib_fn(lib, "hhe_fc_packed_galois_steps")(C.c_size_t(n), C.c_size_t(rows), C.c_size_t(cols), out, C.byref(cnt))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return [int(v) for v in out[:cnt.value]]


def fc_packed_hoisted_galois_steps(n, rows, cols, lib=None):
    """the Galois keys of the one-pass schedule of the hoisted layer: -c (when 2c != n), 1 .. r-1, then r, 2r, .. below c"""
    lib = lib or load_library()
    out = (C.c_int * max(int(n), 64))()
    cnt = C.c_size_t(len(out))
    rc = _lib_fn(lib, "hhe_fc_packed_hoisted_galois_steps")(C.c_size_t(n), C.c_size_t(rows), C.c_size_t(cols), out, C.byref(cnt))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return [int(v) for v in out[:cnt.value]]


def fc_open_shape(n, rows, cols, lib=None):
    """(r, c) of the open layout at degree n: r = pow2 >= rows, c = pow2 >= cols + r - 1; HheError when c > n / 2"""
    lib = lib or load_library()
    r, c = C.c_size_t(0), C.c_size_t(0)
    rc = _lib_fn(lib, "hhe_fc_open_shape")(C.c_size_t(n), C.c_size_t(rows), C.c_size_t(cols), C.byref(r), C.byref(c))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return int(r.value), int(c.value)


def fc_open_diagonals(t, M, lib=None):
    """the diagonals that do not wrap, as slot vectors [r][c]: D_e[j] = M[j mod r][j - e] where that entry exists, else 0"""
    lib = lib or load_library()
    M = np.ascontiguousarray(M, dtype=np.uint64)
    assert M.ndim == 2
    rows, cols = M.shape
    r = 1 << max(rows - 1, 0).bit_length()
    c = 1 << max(cols + r - 2, 0).bit_length()
    vals = np.zeros((r, c), np.uint64)
    rc = _lib_fn(lib, "hhe_fc_open_diagonals")(C.c_uint64(t), _ptr(M), C.c_size_t(rows), C.c_size_t(cols), _ptr(vals))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return vals


def fc_open_galois_steps(n, rows, cols, lib=None):
    """the Galois keys of the one-pass schedule of an open layer: -1 .. -(r-1), then r, 2r, .. below c"""
    lib = lib or load_library()
    out = (C.c_int * max(int(n), 64))()
    cnt = C.c_size_t(len(out))
    rc = _lib_fn(lib, "hhe_fc_open_galois_steps")(C.c_size_t(n), C.c_size_t(rows), C.c_size_t(cols), out, C.byref(cnt))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return [int(v) for v in out[:cnt.value]]


def block_randomness(t, block_index, lib=None, nonce=None):
    lib = lib or load_library()
    mats = np.zeros((4, 2, PASTA_T, PASTA_T), np.uint64)
    rcs = np.zeros((4, 2, PASTA_T), np.uint64)
    if nonce is None:
        rc = lib.hhe_pasta3_block_randomness(C.c_uint64(t), C.c_uint64(block_index), _ptr(mats), _ptr(rcs))
    else:
        rc = lib.hhe_pasta3_block_randomness_nonce(C.c_uint64(t), C.c_uint64(nonce), C.c_uint64(block_index), _ptr(mats), _ptr(rcs))
    if rc:
        raise HheError(rc, lib.hhe_last_error().decode())
    return mats, rcs

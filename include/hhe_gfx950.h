/*
 * hhe_gfx950.h -- C ABI of libhhe_gfx950.so: the MI355X (gfx950) implementation of the
 * CSP-side hot path of harpocrates-project/Privacy-Preserving-ML-through-HHE:
 * PASTA-3 -> BFV transciphering followed by the packed BFV linear layer.
 *
 * Plain C types only.  Every entry point returns 0 on success, non-zero on failure
 * (hhe_last_error() gives the message; INTEGRATION.md maps codes to the C++ exceptions
 * the reference throws).  "dptr" arguments are DEVICE pointers (HBM, uint64 words);
 * "hptr" arguments are host pointers.  Ciphertexts use SEAL's in-memory layout
 * [poly][limb][coeff] (seal/ciphertext.h:701-715) at the data level (L = K-1 limbs), in
 * coefficient (non-NTT) form, batches are contiguous: [B][2][L][N].
 * Key-switch keys use KSwitchKeys::data()[index][digit].data() layout, i.e.
 * [L digits][2][K][N] in NTT form (seal/kswitchkeys.h:90-130).
 *
 * Reference interface each entry replaces is cited as (file:line) relative to the
 * reference repository root.
 */
#ifndef HHE_GFX950_H
#define HHE_GFX950_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hhe_ctx hhe_ctx;
/* One seal::RelinKeys / seal::GaloisKeys OBJECT on the device (keys with identity).  The reference's CSP holds several, made by
 * the same key generator with different randomness, and names one at every call: PASTA_SEAL(context, pk, sk, analyst rk, analyst gk)
 * (src/examples/CSP/CSP.cpp:238-242), flatten(record, tmp, csp_he_gk) (:271-278), relinearize_inplace(record, csp rk) (:306),
 * encrypted_vec_sum(.., analyst_he_gk, ..) (:312-316); the objects are created at src/examples/Analyst/Analyst.cpp:62-94.
 * Which keys a rotation finds decides its NAF decomposition (seal/evaluator.h:955-1060) and the ciphertext words. */
typedef struct hhe_keyset hhe_keyset;

enum {
    HHE_OK = 0,
    HHE_ERR_INVALID = 1,        /* std::invalid_argument in SEAL / the reference        */
    HHE_ERR_NO_GALOIS_KEY = 2,  /* SEAL: "Galois key not present" (evaluator.h:955-1060) */
    HHE_ERR_TOO_FEW_SLOTS = 3,  /* "too little slots for matmul implementation!" (src/pasta/pasta_3_seal.cpp:376-377) */
    HHE_ERR_DEVICE = 4,         /* HIP runtime failure                                    */
    HHE_ERR_NO_RELIN_KEY = 5,
    HHE_ERR_CAPACITY = 6
};

const char *hhe_last_error(void);
/* "hip-gfx950" for the product library */
const char *hhe_backend(void);

/* ---- context: replaces SEALZpCipher::create_context / sealhelper::get_seal_context
 *      (src/pasta/SEAL_Cipher.cpp:38-68, src/util/sealhelper.cpp:8-41) with an explicit
 *      prime list: q[K] = coeff_modulus (last = special key-switch prime), t = plain_modulus.
 *      Derives NTT tables, BatchEncoder map, BEHZ base exactly as SEAL 4.0.0 does.
 *      t may be any batching prime below 2^61, on either side of the coefficient primes: the reference's 65537,
 *      8088322049 and 1096486890805657601 (configs/config.cpp:19-26), the last one above every prime of
 *      BFVDefault(32768).  What that means for plaintexts is stated at hhe_multiply_plain. ---- */
int hhe_ctx_create(int logn, int K, const uint64_t *q_hptr, uint64_t t, int device, hhe_ctx **out);
/* the prime chain SEALZpCipher::create_context picks: CoeffModulus::BFVDefault(N) for N <= 32768 and the hard-coded
 * 29-prime chain for N = 65536 (src/pasta/SEAL_Cipher.cpp:47-65).  *count: in = capacity, out = number of primes. */
int hhe_bfv_default_coeff_modulus(size_t poly_modulus_degree, uint64_t *out_hptr, size_t *count);
void hhe_ctx_destroy(hhe_ctx *c);
/* Run the work of this context on an existing HIP stream (hipStream_t, e.g. a torch.cuda.Stream's handle); NULL = the default
 * stream.  The stream contract (tests/test_gpu_streams.py, and tests/test_stream_order_emu.py for the schedule behind it):
 *  - Inputs are read in the order of the context's stream: every entry point enqueues its first read of a device input (ct, enc_key,
 *    plain ...) on that stream, so it is ordered behind whatever the caller enqueued there before the call -- an upload still in
 *    flight, a kernel that produces the input -- with no host synchronisation.  The key comparison of hhe_pasta3_transcipher runs
 *    there too: enc_key is taken as what the buffer holds in stream order.  Work the caller has on OTHER streams is not waited for.
 *    Host inputs (cw, ncw, block_index, records, keys, matrices, mask values) are read before the call returns.
 *  - The batched calls return after their work has finished (hhe_pasta3_transcipher[_ks], hhe_decompose[_ks], hhe_fc_row[_ks],
 *    hhe_packed_affine[_ks], hhe_fc_packed_ks, hhe_rotate_rows_many_ks, hhe_fc_packed_hoisted_ks, hhe_rotate_plain_sum_ks, hhe_fc_open_plain_ks, hhe_mod_switch, every upload, read-back, key generation and matrix creation): they fork onto the
 *    context's internal non-blocking streams (HHE_STREAMS), join the context's stream again and wait for it, so `out` may be read
 *    from any stream when they return.  The generic evaluator ops (hhe_ntt, hhe_encode, hhe_add, hhe_add_many, hhe_negate, hhe_add_plain,
 *    hhe_multiply_plain, hhe_multiply, hhe_relinearize, hhe_apply_galois, hhe_rotate_*, hhe_mask, hhe_flatten) only ENQUEUE on the
 *    context's stream: their result is ordered for later work on that stream, and for the host after hhe_ctx_sync (or a wait for
 *    the stream).  A non-blocking stream is not ordered with the default stream.
 *  - hhe_ctx_create uploads its tables on the default stream and waits.  Key uploads, key generation, hhe_matrix_create, hhe_enc_matrix_create, hhe_plain_rows_create and hhe_plain_fc_create_open use the
 *    stream the context has at that call and wait: what they leave resident is complete, whichever stream later calls run on.
 *  - Changing the stream waits for nothing.  Resident objects (keys, block tables, kept keystreams, matrices) stay valid, as they
 *    were finished under a host wait.  Generic ops still in flight on the old stream are NOT ordered with calls on the new one,
 *    and they share the context's workspaces: call hhe_ctx_sync before hhe_ctx_set_stream unless the last call was a batched one. */
int hhe_ctx_set_stream(hhe_ctx *c, void *hip_stream);
/* size per-batch workspaces for up to max_batch ciphertexts (allocated once, reused) */
int hhe_ctx_reserve(hhe_ctx *c, size_t max_batch);
int hhe_ctx_sync(hhe_ctx *c);
/* Thread safety: every entry point that takes a context serialises on a lock inside it (the reference's gRPC handlers call
 * the cipher concurrently, src/examples/CSP/CSPRPC.cpp:201-203); different contexts are independent.  hhe_ctx_destroy must
 * not race with other calls on the same context. */
/* Timing instrumentation of the dominant kernel (no reference counterpart; the reference brackets phases with std::chrono,
 * src/examples/hhe_pktnn_examples.cpp:73-76): while enabled, every launch of the fused key-switch row kernel is bracketed
 * by timed HIP events on the stream it is launched on.  hhe_ctx_profile_read waits for the work, returns the number of
 * launches, the sum of their durations and the ciphertexts they covered, and resets the counters.  Results of the ops are
 * unaffected.  kernel_name (optional, name_cap bytes) receives the kernel's name as rocprofv3 prints it. */
int hhe_ctx_profile(hhe_ctx *c, int enable);
int hhe_ctx_profile_read(hhe_ctx *c, char *kernel_name, size_t name_cap, uint64_t *launches, double *total_ms, uint64_t *items);
/* derived parameters, for cross-checking against SEAL's context: what in
 * {"root" i<K, "bsk" i<=L (B_0.., m_sk), "gamma", "galois_elt" i=step, "fc_fallbacks", "fc_csum_closes", "fc_packed_key_switches",
 * "add_many_launches", "rot_hoist", "rot_many_fallbacks", "rot_many_key_switches", "rot_many_launches", "rot_many_group",
 * "plain_sum_fold", "plain_sum_fallbacks", "plain_sum_launches", "plain_sum_mod_downs",
 * "mlp_layers", "mlp_key_switches", "tensor_launches", "square_launches"};
 * which kernels the context dispatches to (read-only diagnostics): "row_kernel" (1 = the fused key-switch row kernels run,
 * 0 = the separate-kernel path), "pm_ok" i<K (coefficient prime i has the pseudo-Mersenne form the lazy kernels need),
 * "digit_reduce" (key-switch digits are reduced before their transforms: some q_I >= 4 q_J) */
uint64_t hhe_ctx_query(const hhe_ctx *c, const char *what, int i);

/* ---- keys.  Key words must be reduced modulo their coefficient primes (what SEAL's safe load checks, is_data_valid_for):
 *      the kernels multiply them through Shoup quotients; an upload with a word >= its prime fails with HHE_ERR_INVALID.
 *      The DEFAULT set of a context = the by-value seal::RelinKeys / seal::GaloisKeys members of SEALZpCipher
 *      (src/pasta/SEAL_Cipher.h:28-31; ctor SEAL_Cipher.cpp:9-36): every entry point without a key-set argument uses it. ---- */
int hhe_set_relin_key(hhe_ctx *c, const uint64_t *ksk_hptr); /* slot 0: the key PASTA_SEAL was constructed with */
/* further RelinKeys objects (e.g. the CSP's own csp_rk used at CSP.cpp:306); slot < 4 */
int hhe_set_relin_key_slot(hhe_ctx *c, int slot, const uint64_t *ksk_hptr);
int hhe_set_galois_key(hhe_ctx *c, uint32_t galois_elt, const uint64_t *ksk_hptr);
int hhe_has_galois_key(const hhe_ctx *c, uint32_t galois_elt);
/* Key sets: one per RelinKeys / GaloisKeys object of the caller (a set may hold both kinds).  Uploaded once, resident in HBM
 * with everything derived from its keys (Shoup quotient tables, FC correction tables) until destroyed; using a set never
 * touches another set.  A set belongs to the context it was created on and must be destroyed before that context
 * (hhe_ctx_destroy releases forgotten ones).  In the *_ks entry points below a NULL set means the context's default set. */
int hhe_keyset_create(hhe_ctx *c, hhe_keyset **out);
void hhe_keyset_destroy(hhe_keyset *ks);
int hhe_keyset_set_relin(hhe_keyset *ks, const uint64_t *ksk_hptr);                        /* RelinKeys::key(2) */
int hhe_keyset_set_galois(hhe_keyset *ks, uint32_t galois_elt, const uint64_t *ksk_hptr);  /* GaloisKeys::key(galois_elt) */
int hhe_keyset_has_galois(const hhe_keyset *ks, uint32_t galois_elt);                      /* GaloisKeys::has_key */
int hhe_keyset_has_relin(const hhe_keyset *ks);

/* ---- device memory helpers for callers without their own HIP allocator ---- */
void *hhe_malloc(size_t bytes);
void hhe_free(void *dptr);
int hhe_copy_h2d(hhe_ctx *c, void *dptr, const void *hptr, size_t bytes);
int hhe_copy_d2h(hhe_ctx *c, void *hptr, const void *dptr, size_t bytes);

/* ---- BFV primitives on device batches (seal::Evaluator / BatchEncoder as used by the path) ---- */
/* util::ntt_negacyclic_harvey / inverse (seal/util/ntt.h:231,303): polys [count][N], modulus of
 * poly p = mod_base + p % mod_cycle (0..K-1 coeff primes, K..K+L Bsk, K+L+1 = t), in place */
int hhe_ntt(hhe_ctx *c, uint64_t *polys_dptr, size_t count, int mod_base, int mod_cycle, int inverse);
/* BatchEncoder::encode (seal/batchencoder.h:80): vals [B][count] -> plain [B][N] */
int hhe_encode(hhe_ctx *c, const uint64_t *vals_dptr, size_t B, size_t count, uint64_t *plain_dptr);
/* Evaluator::add_inplace / negate_inplace (seal/evaluator.h:92-132); size = polys per ct */
int hhe_add(hhe_ctx *c, const uint64_t *a_dptr, const uint64_t *b_dptr, uint64_t *out_dptr, size_t B, int size);
int hhe_negate(hhe_ctx *c, const uint64_t *a_dptr, uint64_t *out_dptr, size_t B, int size);
/* Evaluator::add_plain / sub_plain (seal/evaluator.h:665-680); plain [B][N] or [1][N] if bcast */
int hhe_add_plain(hhe_ctx *c, const uint64_t *ct_dptr, const uint64_t *plain_dptr, int plain_bcast,
                  int subtract, uint64_t *out_dptr, size_t B);
/* Evaluator::multiply_plain (seal/evaluator.h:729-747).  Plaintext lift, per limb j and for any t < 2^61 and any q_j: a
 * coefficient x in [0, t) becomes x mod q_j below (t + 1) / 2 and (x - t) mod q_j from there on, the residue of its centred
 * representative.  Where t < q_j that is SEAL's fast branch x + (q_j - t), no reduction; where t > q_j it is the per-prime
 * decomposition of x + (Q - t) (seal/context.h:359-372).  The same lift feeds hhe_mask, hhe_matrix_create and the public
 * tables of the transciphering. */
int hhe_multiply_plain(hhe_ctx *c, const uint64_t *ct_dptr, const uint64_t *plain_dptr, int plain_bcast,
                       uint64_t *out_dptr, size_t B);
/* Evaluator::apply_galois (seal/evaluator.h:889) */
int hhe_apply_galois(hhe_ctx *c, const uint64_t *ct_dptr, uint32_t galois_elt, uint64_t *out_dptr, size_t B);
/* Evaluator::rotate_rows / rotate_columns incl. NAF fallback (seal/evaluator.h:955-1060) */
int hhe_rotate_rows(hhe_ctx *c, const uint64_t *ct_dptr, int step, uint64_t *out_dptr, size_t B);
int hhe_rotate_columns(hhe_ctx *c, const uint64_t *ct_dptr, uint64_t *out_dptr, size_t B);
/* the same with the GaloisKeys object the call names, as Evaluator::rotate_rows(ct, step, galois_keys, out) does: a step whose
 * element is not in THIS set is NAF-decomposed over the keys of this set, whatever other sets hold */
int hhe_apply_galois_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *ct_dptr, uint32_t galois_elt, uint64_t *out_dptr, size_t B);
int hhe_rotate_rows_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *ct_dptr, int step, uint64_t *out_dptr, size_t B);
int hhe_rotate_columns_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *ct_dptr, uint64_t *out_dptr, size_t B);
/* Evaluator::multiply (seal/evaluator.h:214-277; BEHZ) -> size-3 ct [B][3][L][N] */
int hhe_multiply(hhe_ctx *c, const uint64_t *a_dptr, const uint64_t *b_dptr, uint64_t *out3_dptr, size_t B);
/* The BEHZ floor of a SUM of K products: a [K][B][2][L][N], b [K][B][2][L][N] or, with b_bcast set, [K][1][2][L][N] (addend k of every
 * item multiplies b[k]); out3 [B][3][L][N].  The steps of Evaluator::bfv_multiply with the tensor step replaced by a sum:
 *   1. every operand is extended to q u B_sk as a product's operands are (fastbconv_m_tilde + sm_mrq);
 *   2. under every modulus of q u B_sk the three tensor polynomials (a0 b0, a0 b1 + a1 b0, a1 b1) of the K pairs of an item are summed,
 *      in the NTT domain;
 *   3. the sum is multiplied by t, floored ONCE (fast_floor) and converted back ONCE (fastbconv_sk).
 * K == 1 gives the words of hhe_multiply.  The result does not depend on the order of the K pairs.  It lies within L + 1 of
 * floor((2 t D + Q) / (2 Q)) per coefficient, D the sum of the K integer tensor products of the operands' centred lifts, whatever K is:
 * the summed value passes through one fast conversion (at most L - 1 multiples of Q too much), one floor against round, and one unit for
 * the representative sm_mrq leaves -- the bound of a single product (DESIGN.md section 4 has the argument).
 * The cap on K.  fastbconv_sk recovers the floored value from its residues exactly while it stays below B (floor(m_sk / 2) - L) in
 * magnitude, B the product of the first L primes of B_sk.  An operand leaves sm_mrq within (Q / 2)(1 + rho), rho = (2L + 1) / 2^32, so
 * the floored value is at most K N t Q (1 + rho)^2 / 2 + L.  A call is admitted when
 *     K N t Q (1 + rho)^2 / 2 + L  <  B (floor(m_sk / 2) - L),
 * and hhe_ctx_query("behz_sum_cap") is the largest such K of the context (from its own primes, saturating at 2^63 - 1; 0 when there is
 * none).  K >= 2 above it: HHE_ERR_INVALID, out3 untouched.  K == 1 is always served, as hhe_multiply serves it.
 * "behz_sum_cap" == 0 (a 60-bit t over 60-bit primes at N = 1024, for one) means that even ONE product of arbitrary words is outside
 * the proved bound: on operands whose coefficients sit at +-Q / 2, hhe_multiply is then far more than L + 1 from the rounded integer
 * product -- word for word what Evaluator::multiply gives, the limit of BEHZ at such parameters and not of this library.  The calls
 * that floor one product at a time (hhe_multiply, hhe_square, hhe_fc_packed_ks, hhe_fc_packed_hoisted_ks) are still served, as SEAL
 * serves them, and decrypt correctly on real encryptions where the parameters leave noise budget (the words of an encryption are
 * uniform, far from that worst case); the sum forms with two addends or more (hhe_multiply_sum, hhe_fc_packed_sum_ks, hhe_fc_open_ks,
 * hhe_mlp_ks with r >= 2) refuse.
 * Also HHE_ERR_INVALID: a null pointer, K == 0, B == 0, out3 overlapping an operand, K * B operands whose extended polynomials pass
 * 2^31 coefficients.  The workspaces grow to K * B operands the way
 * hhe_multiply's grow to B.  One launch of the summed tensor kernel per modulus set ("multiply_sum_launches" counts them); its 128-bit
 * sums are reduced every "multiply_sum_fold_q" / "multiply_sum_fold_bsk" addends (2^(127 - 2 bits) for the widest modulus of the set, at
 * most 128).  Enqueues on the context's stream like hhe_multiply. */
int hhe_multiply_sum(hhe_ctx *c, const uint64_t *a_dptr, const uint64_t *b_dptr, size_t K, int b_bcast, uint64_t *out3_dptr, size_t B);
/* Evaluator::relinearize_inplace (seal/evaluator.h:301-304) size 3 -> 2 */
int hhe_relinearize(hhe_ctx *c, const uint64_t *a3_dptr, uint64_t *out_dptr, size_t B);
/* the same with the RelinKeys object of `slot` (hhe_set_relin_key_slot): Evaluator::relinearize_inplace(record, csp_rk) at
 * src/examples/CSP/CSP.cpp:306 uses the CSP's keys, not the ones PASTA_SEAL was built with */
int hhe_relinearize_slot(hhe_ctx *c, int slot, const uint64_t *a3_dptr, uint64_t *out_dptr, size_t B);
/* ... or with the RelinKeys object as a key set */
int hhe_relinearize_ks(hhe_ctx *c, const hhe_keyset *rk, const uint64_t *a3_dptr, uint64_t *out_dptr, size_t B);

/* ---- the hot path ---- */
/* PASTA_SEAL::decomposition / HE_decrypt (src/pasta/pasta_3_seal.cpp:106-172 / :42-104), batched over
 * independent blocks: item i transciphers the <=128 symmetric-ciphertext words cw[i][0..ncw[i]) that
 * were PASTA-encrypted with block counter block_index[i] (nonce 123456789) under the key whose BFV
 * encryption is enc_key (ONE ciphertext [2][L][N], shared by the batch: enc_ssk[0]).
 * cw_hptr [B][128] uint64 host, ncw_hptr [B], block_index_hptr [B]; out [B][2][L][N] device.
 * Needs relin key + Galois keys for steps {-1, +128 (if N/2 != 128), columns} (add_gk_indices :190-201);
 * use_bsgs!=0 selects PASTA_SEAL::babystep_giantstep (:267-366) and additionally steps -16k, k=1..7. */
int hhe_pasta3_transcipher(hhe_ctx *c, const uint64_t *enc_key_dptr, const uint64_t *cw_hptr,
                           const uint32_t *ncw_hptr, const uint64_t *block_index_hptr, size_t B,
                           int use_bsgs, uint64_t *out_dptr);
/* the same for a PASTA_SEAL constructed with the RelinKeys `rk` and the GaloisKeys `gk` (CSP.cpp:238-242: the analyst's) */
int hhe_pasta3_transcipher_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const uint64_t *enc_key_dptr, const uint64_t *cw_hptr,
                              const uint32_t *ncw_hptr, const uint64_t *block_index_hptr, size_t B, int use_bsgs, uint64_t *out_dptr);
/* The per-block public tables (matrices depend only on (nonce, block index)) are built on first use and cached per block counter:
 * (4 x 128 x L) x N words of multipliers, twice that with their Shoup quotients in the fused pipeline -- 768 MiB per counter at
 * N = 2^15, L = 3; 1.07 / 2.1 GiB at the reference defaults N = 2^14, L = 8 -- and the babystep-giantstep variant adds (4 x 128 x L) x N.
 * The cache is bounded: beyond `bytes` (default 32 GiB; HHE_BLOCK_CACHE_MB) the least recently used counters are dropped, never
 * one the running call uses (a single call that needs more than the limit is served).  hhe_ctx_query("block_cache_bytes" /
 * "block_cache_entries") report its state; hhe_pasta3_clear_block_cache drops everything.
 * One keystream per counter (HHE_DEDUP, default 1): everything a transciphering does before it adds the item's own words -- the
 * homomorphic keystream, res[b] = Enc(c_b) - state (pasta_3_seal.cpp:161-169) -- depends on enc_key, the key objects and the block
 * counter only.  A call in which counters repeat (every record starts at counter 0: a batch of S records of nb blocks has nb
 * distinct counters) evaluates each distinct counter once and finishes every item with one encode + add_plain against its counter's
 * keystream; the output words are those of the per-item evaluation.  A call whose counters are all distinct runs as before, and
 * HHE_DEDUP=0 makes every item evaluate its own keystream.  hhe_ctx_query("dedup") reports the knob, "transcipher_unique" the
 * distinct counters of the last call (its item count when it ran per item).
 * One keystream per key (HHE_KS_CACHE, default 1): the keystream ciphertext of a counter is also the same from call to call while
 * the words of enc_key, the key objects the call names and use_bsgs stay what they were -- a service under one analyst key evaluates
 * counter i once, not once per record.  The context keeps the keystream ciphertexts it has evaluated (ciphertexts under the analyst's
 * key, 2 L N words each; nothing else) with its counter's public tables and drops them with those tables (the limit below,
 * hhe_pasta3_clear_block_cache, hhe_ctx_destroy), beyond HHE_KS_CACHE_MB (default 256) of them, least recently used first, and on
 * hhe_pasta3_clear_keystream_cache.  What makes a kept keystream valid for a call: enc_key equals, word for word, a device copy taken
 * when the keystream was evaluated (compared on the device on the context's stream at every call, so the buffer may be overwritten in
 * place between calls; copies of up to 4 different key ciphertexts are kept); the key sets are the ones it was evaluated under and no key
 * of them has been uploaded, replaced or cleared since; same use_bsgs; same counter.  A call evaluates only the counters it finds no
 * keystream for; the output words are those of a call that evaluates everything.  The cache stands aside (no lookup, nothing kept)
 * under HHE_KS_CACHE=0 or HHE_DEDUP=0, and while hhe_ctx_profile is enabled.  hhe_ctx_query: "ks_cache" (the knob),
 * "transcipher_evaluated" / "ks_cache_hits" (keystreams the last call evaluated / found), "ks_cache_entries", "ks_cache_bytes". */
int hhe_pasta3_set_block_cache_limit(hhe_ctx *c, size_t bytes);
void hhe_pasta3_clear_block_cache(hhe_ctx *c);
void hhe_pasta3_clear_keystream_cache(hhe_ctx *c);
/* SEALZpCipher::mask (src/pasta/SEAL_Cipher.cpp:161-166): mask_vals_hptr[count], shared by the batch */
int hhe_mask(hhe_ctx *c, const uint64_t *ct_dptr, const uint64_t *mask_vals_hptr, size_t count,
             uint64_t *out_dptr, size_t B);
/* SEALZpCipher::flatten (src/pasta/SEAL_Cipher.cpp:170-181): blocks [S][nblocks][2][L][N] -> out [S][2][L][N] */
int hhe_flatten(hhe_ctx *c, const uint64_t *blocks_dptr, size_t nblocks, uint64_t *out_dptr, size_t S);
/* flatten(in, out, galois_keys) with the GaloisKeys object it is given (CSP.cpp:271-278 passes csp_he_gk, steps -128*i) */
int hhe_flatten_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *blocks_dptr, size_t nblocks, uint64_t *out_dptr, size_t S);
/* BaseCSP::decompose (src/examples/CSP/CSP.cpp:235-283): S records of nwords symmetric-ciphertext words (host, [S][nwords])
 * -> decomposition of every block + mask of the ragged last block (mask_last != 0: as hhe_pktnn_examples.cpp:620-626;
 * the CSP's own loop at CSP.cpp:264-269 masks a copy, i.e. has no effect: pass 0 to reproduce that) + flatten.
 * out [S][2][L][N] device.  Needs the PASTA keys plus Galois keys reaching steps -128*i (directly or through NAF). */
int hhe_decompose(hhe_ctx *c, const uint64_t *enc_key_dptr, const uint64_t *records_hptr, size_t S, size_t nwords,
                  int mask_last, uint64_t *out_dptr);
/* the same with the three key objects BaseCSP::decompose names: `rk` / `gk` construct the PASTA_SEAL (CSP.cpp:238-242), `flatten_gk`
 * is the GaloisKeys passed to flatten (CSP.cpp:271-278) */
int hhe_decompose_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_keyset *flatten_gk, const uint64_t *enc_key_dptr,
                     const uint64_t *records_hptr, size_t S, size_t nwords, int mask_last, uint64_t *out_dptr);
/* FC row: sealhelper::packed_enc_multiply + Evaluator::relinearize_inplace + sealhelper::encrypted_vec_sum
 * (src/util/sealhelper.cpp:268-274, src/examples/CSP/CSP.cpp:306, sealhelper.cpp:379-392).
 * vi [B][2][L][N]; w: weight-row ciphertexts [W][2][L][N]; item i uses w[i % W]. out [B][2][L][N];
 * the neuron's value is slot n_inputs-1 of the decryption.  relin_slot selects the RelinKeys object;
 * default_galois_only != 0 makes rotate_rows see only the power-of-two Galois elements, i.e. behave as if called
 * with a GaloisKeys made by create_galois_keys() without arguments (what the CSP passes, CSP.cpp:312-316), even when
 * the context also holds flatten / PASTA keys.  The n-1 NAF rotation chains share prefixes and are evaluated as a
 * trie (identical ciphertext words, ~2.7x fewer key switches for n = 784); the children of a trie node share the digit
 * transforms of its c1 (exact unless a c1 coefficient is 0, in which case the chunk is recomputed with per-child transforms;
 * hhe_ctx_query("fc_fallbacks") counts those).  Synchronous: returns when the results are in out. */
int hhe_fc_row(hhe_ctx *c, const uint64_t *vi_dptr, const uint64_t *w_dptr, size_t W, size_t n_inputs, int relin_slot,
               int default_galois_only, uint64_t *out_dptr, size_t B);
/* the same with the key objects the CSP names: relinearize_inplace(prod, rk) (CSP.cpp:306) and encrypted_vec_sum(prod, sum, evaluator,
 * gk, n) (CSP.cpp:312-316): a rotation step is one key switch exactly when `gk` holds its element, else its NAF terms over `gk` */
int hhe_fc_row_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const uint64_t *vi_dptr, const uint64_t *w_dptr, size_t W,
                  size_t n_inputs, uint64_t *out_dptr, size_t B);

/* ---- packed plain-matrix affine layers: SEALZpCipher::packed_matMul / packed_affine (src/pasta/SEAL_Cipher.cpp:522-543), a PUBLIC
 *      dim x dim matrix times an encrypted packed vector plus a plain bias, by the diagonal method (:271-313) or babystep-giantstep
 *      (:185-267).  The matrix is a resident handle, created once per matrix like a key set: it names its context, everything derived
 *      from it lives with it, and it is destroyed explicitly (hhe_ctx_destroy releases forgotten ones).  M_hptr: row-major dim x dim,
 *      entries < t; bias_hptr: dim words or NULL (packed_matMul).  n1 = n2 = 0: diagonal method; otherwise babystep-giantstep with
 *      n1 * n2 == dim (else HHE_ERR_INVALID; the reference only warns and computes garbage); n1 == 1 or n2 == 1 takes the diagonal
 *      method, as packed_matMul does.  dim need not be a power of two.  dim * 2 != N && dim * 4 > N: HHE_ERR_TOO_FEW_SLOTS (:192-193).
 *      Device footprint (hhe_matrix_bytes): 2 * dim * L * N words for the diagonal method (multipliers in the rotated NTT frame and
 *      their Shoup quotients), dim * L * N for babystep-giantstep, plus N words of bias: 201 MB / 101 MB at dim = 128, N = 2^15,
 *      L = 3.  Handles are not part of the block-table cache and are never evicted.
 *      One difference from SEAL: a diagonal that is all zero is multiplied like any other, where Evaluator::multiply_plain throws on
 *      the transparent product. ---- */
typedef struct hhe_matrix hhe_matrix;
int hhe_matrix_create(hhe_ctx *c, const uint64_t *M_hptr, size_t dim, const uint64_t *bias_hptr, size_t n1, size_t n2, hhe_matrix **out);
void hhe_matrix_destroy(hhe_matrix *m);
size_t hhe_matrix_bytes(const hhe_matrix *m);
/* out[b] = M * ct[b] (+ bias) for B ciphertexts [B][2][L][N] sharing the matrix; out_dptr == ct_dptr is allowed.  Includes the
 * non-full-packed preparation ct += rotate_rows(ct, -dim) when N != 2 dim and add_plain(encode(bias)).  gk: the GaloisKeys object
 * (NULL = the context's default set); it needs the steps of hhe_affine_galois_steps -- step +1 as a key of its own, the others directly
 * or through their NAF terms -- else HHE_ERR_NO_GALOIS_KEY with out untouched.  The batch is chunked over the internal streams like
 * hhe_pasta3_transcipher (HHE_CHUNK, HHE_STREAMS); babystep-giantstep keeps n1 + n2 ciphertexts per item of a chunk as workspace on top of
 * the lane's.  Synchronous. */
int hhe_packed_affine_ks(hhe_ctx *c, const hhe_keyset *gk, const hhe_matrix *mat, const uint64_t *ct_dptr, uint64_t *out_dptr, size_t B);
/* add_diagonal_indices / add_bsgs_indices (:337-355), host only: the rotate_rows steps a layer needs keys for, in the reference's
 * order.  *count: in = capacity of steps_out, out = number of steps (HHE_ERR_CAPACITY when too small). */
int hhe_affine_galois_steps(size_t N, size_t dim, size_t n1, size_t n2, int *steps_out, size_t *count);

/* ---- packed encrypted FC: a rows x cols matrix of ENCRYPTED weights times an encrypted packed vector, all outputs in one ciphertext,
 *      by the Halevi-Shoup hybrid diagonal method.  It replaces `rows` calls of the FC row above (src/examples/CSP/CSP.cpp:296-316):
 *      the analyst encrypts r generalized diagonals instead of `rows` weight rows and decrypts one ciphertext.
 *      Shape: r = the smallest power of two >= rows; c = the smallest power of two >= cols, raised to r if smaller.  Admitted when
 *      2c == N or 4c <= N, else HHE_ERR_TOO_FEW_SLOTS (the rule of src/pasta/SEAL_Cipher.cpp:192-193 with c for the dimension).
 *      Diagonals (host): with M zero-padded to r x c, d_i[j] = M[j mod r][(j + i) mod c], j in [0, c), i in [0, r); the analyst encodes
 *      d_i into slots [0, c) of row 0 and encrypts it: W_0 .. W_{r-1}.
 *      The layer on an input ciphertext x, in SEAL's operations:
 *        1. if 2c != N:  x = add(x, rotate_rows(x, -c, gk))
 *        2. rot_0 = x;  rot_i = rotate_rows(rot_{i-1}, 1, gk), i = 1 .. r-1
 *        3. acc = multiply(rot_0, W_0);  acc = add(acc, multiply(rot_i, W_i)), i = 1 .. r-1, at size 3
 *        4. y = relinearize(acc, rk)
 *        5. for s = r, 2r, .., c/2:  y = add(y, rotate_rows(y, s, gk))
 *      The words of `out` are the words of that composition.  Slots [0, rows) of the decryption are (M x) mod t; the other slots hold
 *      partial sums (hhe_mask removes them if they must not be returned).
 *      PRECONDITION, which cannot be checked: slots [c, N/2) of the input's row 0 are zero.  Slots [cols, c) may hold anything (the
 *      padded columns of the diagonals are zero).  Row 1 of the batching is carried along independently: a caller who also encodes the
 *      diagonals into row 1 gets a second input vector served per ciphertext.
 *      Galois keys: every step is +- a power of two -- -c (when 2c != N), +1 (when r > 1), r 2^k below c -- whose NAF has one term, so
 *      each needs a key of its own in `gk` (create_galois_keys() without arguments makes all of them).
 *      Key switches per item: (2c != N) + (r - 1) + log2(c / r) rotations and one relinearization, against `rows` relinearizations and
 *      the rotation tries of `rows` FC rows. ---- */
/* host only: r and c of a rows x cols layer at degree N; rows or cols == 0 or N not a power of two: HHE_ERR_INVALID */
int hhe_fc_packed_shape(size_t N, size_t rows, size_t cols, size_t *r_out, size_t *c_out);
/* host only: the generalized diagonals of M_hptr (row-major rows x cols, entries < t, else HHE_ERR_INVALID) as slot vectors
 * vals_hptr [r][c], r and c as above (no degree enters) */
int hhe_fc_packed_diagonals(uint64_t t, const uint64_t *M_hptr, size_t rows, size_t cols, uint64_t *vals_hptr);
/* host only: the rotate_rows steps of the layer in the order it takes them.  *count: in = capacity, out = number of steps
 * (HHE_ERR_CAPACITY when too small), as hhe_affine_galois_steps */
int hhe_fc_packed_galois_steps(size_t N, size_t rows, size_t cols, int *steps_out, size_t *count);
/* The encrypted matrix as a resident handle, created once per model like hhe_matrix: it names its context and is destroyed explicitly
 * (hhe_ctx_destroy releases forgotten ones).  wdiag_dptr: the r diagonal ciphertexts [r][2][L][N] at the data level of c, coefficient
 * form.  The handle holds what a BEHZ product needs from its second operand -- every diagonal extended to q u B_sk and in NTT form,
 * 2 (2L + 1) N words per diagonal (hhe_enc_matrix_bytes) -- computed once, here; the extension is deterministic, so the products of
 * the layer are the words of multiply(rot_i, W_i).  wdiag is not needed after the call.  Runs on the stream c has and waits. */
typedef struct hhe_enc_matrix hhe_enc_matrix;
int hhe_enc_matrix_create(hhe_ctx *c, const uint64_t *wdiag_dptr, size_t rows, size_t cols, hhe_enc_matrix **out);
void hhe_enc_matrix_destroy(hhe_enc_matrix *m);
size_t hhe_enc_matrix_bytes(const hhe_enc_matrix *m);
/* The layer: vi and out [B][2][L][N], out_dptr == vi_dptr is allowed; rk / gk NULL: the context's default set.  Refused before anything
 * is written: a null argument or B == 0 or a handle or key set of another context (HHE_ERR_INVALID), no relinearization key
 * (HHE_ERR_NO_RELIN_KEY), a step without its key (HHE_ERR_NO_GALOIS_KEY).  The batch is chunked over the internal streams
 * (HHE_STREAMS); a chunk keeps its r rotations and r size-3 products per item, 5 r L N words, reserved per lane, and runs the BEHZ
 * passes of all its r x items products at once, so a chunk holds max(1, HHE_CHUNK / r) items: r x items never exceeds what the other
 * batched calls reserve a lane for.  hhe_ctx_query("fc_packed_key_switches"): Galois key switches per item of the last call.
 * Synchronous. */
int hhe_fc_packed_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *mat, const uint64_t *vi_dptr,
                     uint64_t *out_dptr, size_t B);
/* ---- Hoisted rotations: many rotate_rows of the same ciphertexts.  ct [B][2][L][N]; out [n_steps][B][2][L][N], step-major: out[k][b] holds
 *      the words of Evaluator::rotate_rows(ct[b], steps[k], gk), exactly what hhe_rotate_rows_ks writes for that step under that set -- one key
 *      switch when gk holds the step's element, else the step's NAF terms over gk (terms equal to +-N/2 skipped).  Step 0 copies; repeated
 *      steps give equal words.  gk NULL: the context's default set.
 *      Refused before anything is written: a null pointer, B == 0, n_steps == 0, a step with |step| >= N/2, a key set of another context, out
 *      overlapping ct (HHE_ERR_INVALID); a step rotate_rows could not serve from gk (HHE_ERR_NO_GALOIS_KEY).
 *      Schedule: the steps' term sequences form a trie.  A node's ciphertext is computed once, and the children of a node share the digit
 *      transforms of its c1: K L forward transforms per node with children instead of per key switch.  Where the row kernels run
 *      ("row_kernel" == 1) up to "rot_many_group" children of a node are served by ONE launch of the key-switch row kernel and one mod-down.
 *      The shared transforms are exact unless a residue of some c1 is zero; a chunk that meets one is recomputed step by step after the wait
 *      (hhe_ctx_query("rot_many_fallbacks") counts those chunks).  HHE_ROT_HOIST (read at hhe_ctx_create, "rot_hoist"): 1 as described,
 *      0 every step through the path of hhe_rotate_rows_ks, 2 as 1 with every chunk also recomputed (tests).
 *      Synchronous and batched like hhe_fc_row_ks: chunked over the internal streams; a chunk keeps the sums of up to "rot_many_group"
 *      children of its items at once, so it holds max(1, HHE_CHUNK / min(group, most children of a node)) items.  About the last call:
 *      "rot_many_key_switches" (the trie's nodes = key switches per item), "rot_many_launches" (multi-child launches per chunk). ---- */
int hhe_rotate_rows_many_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *ct_dptr, const int *steps_hptr, size_t n_steps,
                            uint64_t *out_dptr, size_t B);
/* hhe_fc_packed_ks with step 2 hoisted: rot_0 = x; rot_i = rotate_rows(x, i, gk), i = 1 .. r-1 -- every rotation comes from the x of step 1,
 * served as hhe_rotate_rows_many_ks serves steps 1 .. r-1 (one node with r-1 children when gk holds a key for each; the NAF trie over the
 * power-of-two keys otherwise).  Handle, diagonals, precondition, steps 1, 3, 4, 5 and the refusals are those of hhe_fc_packed_ks; -c and
 * the tail r 2^k still need their own keys.  The words of `out` are the words of that composition (they differ from hhe_fc_packed_ks's:
 * rot_i carries the noise of one key switch instead of i); slots [0, rows) decrypt to the same (M x) mod t.  out == vi is allowed.
 * "fc_packed_key_switches" after the call: (2c != N) + the trie's nodes + log2(c / r).
 * hhe_fc_packed_hoisted_galois_steps lists the keys of the one-pass schedule: -c (when 2c != N), 1 .. r-1, then r, 2r, .. below c. */
int hhe_fc_packed_hoisted_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *mat, const uint64_t *vi_dptr,
                             uint64_t *out_dptr, size_t B);
int hhe_fc_packed_hoisted_galois_steps(size_t N, size_t rows, size_t cols, int *steps_out, size_t *count);
/* The layer with ONE floor per item: hhe_fc_packed_ks (hoisted == 0) or hhe_fc_packed_hoisted_ks (hoisted != 0) with steps 3 and 4
 * replaced by y = relinearize(multiply_sum(rot_0 .. rot_{r-1}, W_0 .. W_{r-1}), rk) -- hhe_multiply_sum with K = r against the handle's
 * resident diagonals.  Steps 1, 2 and 5, the handle, the keys, the refusals, the in-place call, the chunking, the exactness fallback of
 * the hoisted rotation and the levels are those of the form it follows; r >= 2 above "behz_sum_cap" is refused too (HHE_ERR_INVALID).
 * The words differ from the per-product forms' (one floor instead of r); slots [0, rows) decrypt to the same (M x) mod t.  A chunk keeps
 * its r rotations and one size-3 product per item, (2r + 3) L N words; it still holds max(1, HHE_CHUNK / r) items, since the operands of
 * its r x items products are extended at once.  "fc_packed_floors" after a packed FC call: the polynomials floored per item, 3 here and
 * 3 r for the two other forms; the sum kernel of hhe_add_many is not launched.  Synchronous. */
int hhe_fc_packed_sum_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *mat, const uint64_t *vi_dptr,
                         uint64_t *out_dptr, size_t B, int hoisted);
/* ---- Chainable packed FC: diagonals that do not wrap ("open"), the square, and the FC-square-FC network in one call.
 *      The output of a cyclic layer above is not a legal input of the next: partial sums outside [0, rows), and a precondition on slots
 *      [c, N/2).  The open layout needs neither a precondition nor a mask between layers.
 *      Shape: r = the smallest power of two >= rows; c = the smallest power of two >= cols + r - 1; c <= N/2, else HHE_ERR_TOO_FEW_SLOTS.
 *      Diagonals (host): D_e[j] = M[j mod r][j - e] if j mod r < rows and 0 <= j - e < cols, else 0, e in [0, r), j in [0, c); the analyst
 *      encodes D_e into slots [0, c) of row 0 and encrypts it: W_0 .. W_{r-1}.
 *      The layer on an input ciphertext x, in SEAL's operations:
 *        1. rot_0 = x;  rot_e = rotate_rows(x, -e, gk), e = 1 .. r-1   (every rotation from x, served as hhe_rotate_rows_many_ks serves them)
 *        2. y = relinearize(multiply_sum(rot_0 .. rot_{r-1}, W_0 .. W_{r-1}), rk)   (hhe_multiply_sum, K = r, the resident diagonals)
 *        3. for s = r, 2r, .., c/2:  y = add(y, rotate_rows(y, s, gk))
 *      Slot m < rows of y is sum_k sum_e x[m + kr - e] M[m][m + kr - e]; kr - e takes every value in [-(r-1), c - r] once, so every column
 *      in [0, cols) is met once, and every other slot of x meets a zero of a diagonal before any sum: THERE IS NO PRECONDITION on the
 *      input.  Row 1 of the batching is carried along independently.  The other slots of y hold partial sums, which the next open layer
 *      (or the square before it) may be handed as they are. ---- */
/* host only: r and c of the open layout; refusals as hhe_fc_packed_shape, HHE_ERR_TOO_FEW_SLOTS when c > N/2 */
int hhe_fc_open_shape(size_t N, size_t rows, size_t cols, size_t *r_out, size_t *c_out);
/* host only: the open diagonals of M_hptr (row-major rows x cols, entries < t, else HHE_ERR_INVALID) as slot vectors vals_hptr [r][c] */
int hhe_fc_open_diagonals(uint64_t t, const uint64_t *M_hptr, size_t rows, size_t cols, uint64_t *vals_hptr);
/* host only: the keys of the one-pass schedule: -1 .. -(r-1), then r, 2r, .. below c.  *count as hhe_fc_packed_galois_steps */
int hhe_fc_open_galois_steps(size_t N, size_t rows, size_t cols, int *steps_out, size_t *count);
/* hhe_enc_matrix_create for the open layout: the same handle type and resident form, marked open, r and c of the open shape.  The
 * hhe_fc_packed calls refuse an open handle and the calls below a cyclic one (HHE_ERR_INVALID, `out` untouched). */
int hhe_enc_matrix_create_open(hhe_ctx *c, const uint64_t *wdiag_dptr, size_t rows, size_t cols, hhe_enc_matrix **out);
/* One open layer.  Keys, in-place call, chunking (max(1, HHE_CHUNK / r) items per chunk), levels, refusals and the exactness fallback of
 * the hoisted rotation (HHE_ROT_HOIST) are those of hhe_fc_packed_sum_ks with hoisted != 0; r >= 2 above "behz_sum_cap" is refused.  The
 * tail steps need keys of their own; the steps -e are served from gk directly or through their NAF terms.  After the call
 * "fc_packed_key_switches" is the trie's nodes + log2(c / r) and "fc_packed_floors" is 3.  Synchronous. */
int hhe_fc_open_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *mat, const uint64_t *vi_dptr,
                   uint64_t *out_dptr, size_t B);
/* Evaluator::square at size 2: a [B][2][L][N] -> out3 [B][3][L][N], the words of hhe_multiply(a, a), with hhe_multiply's refusals.  One
 * operand extension instead of a second operand, and a tensor kernel of its own that reads the operand's two polynomials once and
 * writes a0^2, 2 a0 a1, a1^2 ("square_launches" counts its launches, two per call; hhe_multiply keeps the one-product kernel, counted by
 * "tensor_launches").  Enqueues on the context's stream like hhe_multiply. */
int hhe_square(hhe_ctx *c, const uint64_t *a_dptr, uint64_t *out3_dptr, size_t B);
/* The network: mats_hptr is a host array of n_layers open handles;
 *   x_0 = vi;  y_k = fc_open(mats[k], x_k);  x_{k+1} = relinearize(square(y_k), rk);  out = y_{n_layers - 1}.
 * The words of `out` are the words of that composition made from hhe_fc_open_ks, hhe_square and hhe_relinearize_ks; n_layers == 1 gives
 * hhe_fc_open_ks.  A chunk of max(1, HHE_CHUNK / max_k r_k) items runs all its layers on its lane with no host wait in between; the
 * plans and tables of all layers are made before the first chunk.  One flag per chunk covers the hoisted rotations of every layer: a
 * flagged chunk is recomputed whole, from vi, step by step, after the wait.  out == vi is allowed.
 * Refused before anything is written: n_layers == 0, a null or cyclic handle, a handle of another context, rows of layer k != cols of
 * layer k + 1, a layer above "behz_sum_cap" (HHE_ERR_INVALID); a missing relinearization or Galois key of any layer (their codes).
 * "mlp_layers" and "mlp_key_switches" (Galois key switches per item, summed over the layers; relinearizations are not counted)
 * describe the last call.  Synchronous.  Not built: a bias (hhe_add_plain between calls), a change of level between layers. */
int hhe_mlp_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *const *mats_hptr, size_t n_layers,
               const uint64_t *vi_dptr, uint64_t *out_dptr, size_t B);
/* ---- Plain-weights sum of rotations: out = sum_k rotate_rows(ct, steps[k]) * plain_k, with ONE mod-down over the sum.
 *      The handle holds `n` plaintexts, each given as count <= N slot values < t (vals_hptr [n][count]) and encoded as hhe_encode encodes
 *      them.  Each is lifted by the rule stated at hhe_multiply_plain (x below (t + 1) / 2 stays, x - t from there on, t on either side of a
 *      prime) to ALL K primes of the context, the special one included, in NTT form with Shoup quotients: 2 K N words per plaintext
 *      (hhe_plain_rows_bytes; 38 MB for 16 plaintexts at BFVDefault(16384)).  Resident and explicit like hhe_matrix: it names its context,
 *      hhe_ctx_destroy releases forgotten ones.  Runs on the stream c has and waits.
 *      DEFINITION (no composition of SEAL's operations).  q_0 .. q_{L-1} the data primes, Q their product, p = q_{K-1} the special prime;
 *      * the product in Z[X]/(X^N + 1); sigma_k the Galois map of rotate_rows(., steps[k]); m~_k plaintext k as the integer
 *      polynomial with centred coefficients (the lift above); key_k the Galois key of that element in gk; [.]_{q_I} the residue in
 *      [0, q_I) taken as an integer polynomial (the digit of SURVEY A.4).  For an input (c0, c1) and i in {0, 1} let X_i in [0, Q p) be the
 *      integer polynomial congruent, modulo every prime of q u {p}, to
 *          sum_{k: steps[k] != 0}  m~_k * sum_{I < L} [sigma_k(c1)]_{q_I} * key_k[I][i].
 *      Then
 *          out_0[j] = sum_k m~_k * sigma_k(c0)              + floor((X_0 + floor(p/2)) / p)   mod q_j
 *          out_1[j] = sum_{k: steps[k] == 0} m~_k * c1      + floor((X_1 + floor(p/2)) / p)   mod q_j.
 *      (The library carries c0, and c1 for step 0, through the extended basis as multiples of p, which divide out exactly.)  The order of
 *      the pairs does not matter; repeated steps are allowed.  With n = 1 and the plaintext whose slots are all 1 the words are those of
 *      hhe_rotate_rows_ks(ct, step) under a key of that step.  Slot s of the decryption is sum_k plain_k[s] x[rot_k(s)] mod t.  The
 *      rounding of the mod-down is taken once over the sum: the noise of n rotations' roundings is replaced by one.
 *      KEYS.  Every non-zero step needs a key OF ITS OWN in gk (a NAF chain would need a mod-down between its terms): a step without one
 *      gives HHE_ERR_NO_GALOIS_KEY.  Refused before anything is written, with HHE_ERR_INVALID: a null pointer, B == 0, n == 0 or n above
 *      the handle's count, |step| >= N/2, a handle or key set of another context.  out == ct is allowed.  hhe_plain_rows_create refuses
 *      (HHE_ERR_INVALID) a null pointer, n == 0 or n > 2^20 (polynomial counts of its launches are ints: 2 n K stays below 2^31 for every
 *      K the library admits), count == 0 or count > N, a slot value >= t.
 *      SCHEDULE.  Synchronous and batched like hhe_rotate_rows_many_ks (HHE_CHUNK, HHE_STREAMS).  The children share the digit transforms
 *      of c1; where the row kernels run ("row_kernel" == 1) ONE launch of the key-switch row kernel serves all n children of a chunk: a
 *      workgroup owns (item, key limb, row tile), forms each child's key-switch sums in registers, multiplies them by the child's
 *      plaintext and adds them up, and one inverse transform and ONE mod-down per item follow.  Elsewhere the same words come from one
 *      inner-product launch and the element-wise products per child.  A lane keeps the sums of one child and the sums over the children
 *      (2 x 2 K N words per item), the NTT forms of c0 and one rotated c1 (2 L N): it is reserved for 2 * per items, so a chunk holds
 *      per = max(1, HHE_CHUNK / 2) items.  The shared digits are exact unless a residue of c1 is 0; such a chunk is recomputed from the
 *      digits of each sigma_k(c1) itself ("plain_sum_fallbacks" counts those chunks); HHE_ROT_HOIST 0 / 1 / 2 as for
 *      hhe_rotate_rows_many_ks.  About the last call: "plain_sum_launches" (fused launches per chunk: 1 where the row kernel runs, else
 *      0), "plain_sum_mod_downs" (finish launches of the primitive per chunk: 1).  "plain_sum_fold": children between two folds of the
 *      kernel's outer lazy sums -- a fold leaves less than 2q, a product adds less than 4q, and 2q + 3 * 4q fits the 16q <= 2^64 of the
 *      primes the kernel runs on: 3. ---- */
typedef struct hhe_plain_rows hhe_plain_rows;
int hhe_plain_rows_create(hhe_ctx *c, const uint64_t *vals_hptr, size_t n, size_t count, hhe_plain_rows **out);
void hhe_plain_rows_destroy(hhe_plain_rows *p);
size_t hhe_plain_rows_bytes(const hhe_plain_rows *p);
int hhe_rotate_plain_sum_ks(hhe_ctx *c, const hhe_keyset *gk, const hhe_plain_rows *rows, const int *steps_hptr, size_t n,
                            const uint64_t *ct_dptr, uint64_t *out_dptr, size_t B);
/* The open layer (hhe_fc_open_shape / hhe_fc_open_diagonals) under PLAIN weights.  M_hptr row-major rows x cols, entries < t; bias_hptr
 * `rows` words or NULL.  The handle is the plain-rows form of the r open diagonals D_e plus the encoded bias.  The layer:
 *   y = rotate_plain_sum(x; steps -e, D_e, e < r);   y = add(y, rotate_rows(y, s, gk)) for s = r, 2r, .., c/2;
 *   with a bias  y = add_plain(y, encode(bias into slots [0, rows))), the words of hhe_add_plain.
 * Slots [0, rows) decrypt to (M x + b) mod t; no precondition on the other slots of the input ("Open diagonals" above).  Every step
 * -1 .. -(r-1) and every tail step needs a key of its own: hhe_fc_open_galois_steps lists exactly these.  Chunks, in-place call, levels
 * and the refusals are those of the primitive, plus an empty dimension (HHE_ERR_INVALID) and HHE_ERR_TOO_FEW_SLOTS at creation. */
typedef struct hhe_plain_fc hhe_plain_fc;
int hhe_plain_fc_create_open(hhe_ctx *c, const uint64_t *M_hptr, size_t rows, size_t cols, const uint64_t *bias_hptr, hhe_plain_fc **out);
void hhe_plain_fc_destroy(hhe_plain_fc *m);
size_t hhe_plain_fc_bytes(const hhe_plain_fc *m);
int hhe_fc_open_plain_ks(hhe_ctx *c, const hhe_keyset *gk, const hhe_plain_fc *mat, const uint64_t *vi_dptr, uint64_t *out_dptr, size_t B);
/* Evaluator::add_many (seal/evaluator.h:150) for K stacked batches in_dptr [K][B][size][L][N], size 2 or 3: out [B][size][L][N] = their
 * sum, in ONE kernel launch whatever K is (hhe_ctx_query("add_many_launches") counts them); the sum of a coefficient is kept in two
 * words and reduced once.  out may be one of the K operands.  K == 0, B == 0, a null pointer or another size: HHE_ERR_INVALID.
 * Enqueues on the context's stream like hhe_add. */
int hhe_add_many(hhe_ctx *c, const uint64_t *in_dptr, size_t K, uint64_t *out_dptr, size_t B, int size);

/* PASTA-3 public randomness for one block as the kernels consume it (host; src/pasta/pasta_3_plain.cpp:56-119,286-295):
 * mats [4][2][128][128], rcs [4][2][128] */
int hhe_pasta3_block_randomness(uint64_t t, uint64_t block_index, uint64_t *mats_hptr, uint64_t *rcs_hptr);

/* ---- client / analyst ends ---- */
/* pasta::Pasta::keystream (src/pasta/pasta_3_plain.cpp:156-178) for block counters first_block .. first_block+nblocks-1
 * (nonce 123456789) under the 256-word secret key key_hptr (words < t): ks_dptr [nblocks][128] device. */
int hhe_pasta3_plain_keystream(hhe_ctx *c, const uint64_t *key_hptr, uint64_t first_block, size_t nblocks, uint64_t *ks_dptr);
/* pasta::PASTA::encrypt / decrypt (src/pasta/pasta_3_plain.cpp:9-46) over S records of nwords words each (device,
 * [S][nwords]); every record starts at block counter 0, as each PASTA::encrypt call does.  in == out is allowed. */
int hhe_pasta3_plain_crypt(hhe_ctx *c, const uint64_t *key_hptr, const uint64_t *in_dptr, size_t S, size_t nwords,
                           int decrypt, uint64_t *out_dptr);

/* ---- PASTA under a caller's nonce ----
 * THE CONTRACT.  PASTA's definition draws a block's keystream from a nonce and a block counter (Pasta::init_shake(nonce,
 * block_counter), src/pasta/pasta_3_plain.cpp:56).  Under one PASTA key a (nonce, counter) pair encrypts one block, ever: two blocks
 * under one pair are a two-time pad, and whoever sees both symmetric ciphertexts learns the difference of the plaintexts mod t.  The
 * library does not and cannot check this -- it never sees the secret key on the server's end, and keeps no record of pairs on the
 * client's.  Choosing pairs that never repeat (a fresh nonce per record with counters from 0, or one nonce with a running counter)
 * is the caller's duty.  The entry points above that take no nonce repeat the reference, which fixes the nonce at 123456789 and
 * restarts at counter 0 for every record (pasta_3_seal.cpp:47,115; PASTA::encrypt, pasta_3_plain.cpp:9-27): they exist for parity
 * with it.  They name the same objects: a pair with nonce 123456789 reached through an entry below is the cache entry (public tables,
 * kept keystream) of that counter reached through an entry above. */
/* hhe_pasta3_block_randomness with the nonce of Pasta::init_shake (pasta_3_plain.cpp:56) as an argument (host) */
int hhe_pasta3_block_randomness_nonce(uint64_t t, uint64_t nonce, uint64_t block_index, uint64_t *mats_hptr, uint64_t *rcs_hptr);
/* hhe_pasta3_plain_keystream under `nonce` (Pasta::keystream(nonce, block_counter), pasta_3_plain.cpp:156-178) */
int hhe_pasta3_plain_keystream_nonce(hhe_ctx *c, const uint64_t *key_hptr, uint64_t nonce, uint64_t first_block, size_t nblocks,
                                     uint64_t *ks_dptr);
/* hhe_pasta3_plain_crypt with one nonce per record (PASTA::encrypt, pasta_3_plain.cpp:9-27, with its `nonce` a parameter): record s
 * runs under nonces_hptr[s], block counters from 0.  The other parameters are those of hhe_pasta3_plain_crypt. */
int hhe_pasta3_plain_crypt_nonce(hhe_ctx *c, const uint64_t *key_hptr, const uint64_t *nonces_hptr, const uint64_t *in_dptr, size_t S,
                                 size_t nwords, int decrypt, uint64_t *out_dptr);
/* hhe_pasta3_transcipher_ks with item i under the pair (nonce_hptr[i], block_index_hptr[i]) (PASTA_SEAL::decomposition,
 * pasta_3_seal.cpp:106-172, with the nonce of :115 a parameter).  rk / gk NULL: the context's default set.
 * A call through this entry runs its items in contiguous groups whose distinct pairs fit the block-cache limit (at least one pair per
 * group; 42 pairs at N = 2^15, L = 3 and the 32 GiB default), one group after the other, so that the tables of an earlier group can
 * make room for a later one: a stream of fresh pairs never needs all its tables at once.  The output words are those of one call.
 * hhe_ctx_query("transcipher_groups") reports the groups of the last call; "transcipher_unique" / "transcipher_evaluated" /
 * "ks_cache_hits" count pairs, summed over the groups. */
int hhe_pasta3_transcipher_nonce_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const uint64_t *enc_key_dptr,
                                    const uint64_t *cw_hptr, const uint32_t *ncw_hptr, const uint64_t *nonce_hptr,
                                    const uint64_t *block_index_hptr, size_t B, int use_bsgs, uint64_t *out_dptr);
/* hhe_decompose_ks with one nonce per record (BaseCSP::decompose, CSP.cpp:235-283): the blocks of record s run under
 * (nonces_hptr[s], 0), (nonces_hptr[s], 1), ...; grouped like hhe_pasta3_transcipher_nonce_ks */
int hhe_decompose_nonce_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_keyset *flatten_gk, const uint64_t *enc_key_dptr,
                           const uint64_t *records_hptr, const uint64_t *nonces_hptr, size_t S, size_t nwords, int mask_last,
                           uint64_t *out_dptr);
/* The public randomness of `count` pairs drawn on the device (Pasta::init_shake, get_random_matrix, get_rc_vec;
 * pasta_3_plain.cpp:56-119): one XOF launch with a pair per lane, one expansion launch with a workgroup per pair and affine layer.
 * mats_dptr [count][4][2][128][128], rcs_dptr [count][4][2][128] device: pair after pair what hhe_pasta3_block_randomness writes.
 * These are the launches a transciphering call uses for the pairs it has no tables for when the randomness is drawn on the device:
 * HHE_PUBLIC_DEVICE, read at context creation (0: on the host, pair by pair; 1: on the device, all missing pairs of a call at once;
 * unset: on the device when a call misses 8 pairs or more, where it measured faster, else on the host).  hhe_ctx_query("public_device")
 * reports the knob ((uint64_t)-1 when unset), "public_device_built" the pairs whose randomness the last call drew on the device. */
int hhe_pasta3_block_randomness_dev(hhe_ctx *c, const uint64_t *nonces_hptr, const uint64_t *blocks_hptr, size_t count,
                                    uint64_t *mats_dptr, uint64_t *rcs_dptr);
/* Builds the public tables the cache lacks for these pairs, exactly as a call of hhe_pasta3_transcipher_nonce_ks on them would
 * (groups included), without evaluating anything: a service warms a counter range with it.  *built_out (optional): the pairs
 * anything was built for. */
int hhe_pasta3_prepare_tables(hhe_ctx *c, const uint64_t *nonces_hptr, const uint64_t *blocks_hptr, size_t count, int use_bsgs,
                              size_t *built_out);
/* Decryptor::decrypt + BatchEncoder::decode (seal/decryptor.h:70, seal/batchencoder.h:282) as used by
 * sealhelper::decrypting / Analyst::decrypt_result (src/util/sealhelper.cpp:252-266): B size-2 data-level
 * ciphertexts [B][2][L][N] -> slot values [B][N] (unsigned, < t; the signed view of decode_int64 is v > t/2 ? v - t : v).
 * sk_hptr: the secret key polynomial at the key level, NTT form [K][N] (SecretKey::data().data()).
 * On a level context (hhe_ctx_create_level, l data primes) the key is [l+1][N]: rows {0..l-1, K-1} of the parent's
 * (api.py: level_rows(sk, l)). */
int hhe_decrypt(hhe_ctx *c, const uint64_t *sk_hptr, const uint64_t *ct_dptr, size_t B, uint64_t *vals_dptr);
/* hhe_decrypt for ciphertexts [B][2][limbs][N]; sk_hptr stays [K][N], its first `limbs` rows are used
 * (Decryptor::decrypt on a ciphertext whose parms_id names a lower level of the modulus switching chain, seal/decryptor.h:70;
 * 1 <= limbs <= L, hhe_decrypt is limbs = L).  The values are right exactly while the ciphertext's noise budget at that level
 * (Decryptor::invariant_noise_budget, seal/decryptor.h:103) is positive: a switch that drops too many primes leaves noise above
 * Q_level / 2t and the slots come back wrong, without an error, as in SEAL. */
int hhe_decrypt_level(hhe_ctx *c, const uint64_t *sk_hptr, const uint64_t *ct_dptr, int limbs, size_t B, uint64_t *vals_dptr);
/* Decryptor::invariant_noise_budget (seal/decryptor.h:103) of B ciphertexts ct [B][size][limbs][N] (coefficient form, size 2 or 3,
 * 1 <= limbs <= L; sk_hptr [K][N] as above).  With Q = q_0 ... q_{limbs-1} and m the largest centred magnitude over the coefficients
 * of t * (c0 + c1 s [+ c2 s^2]) mod Q:  norm_bits = bit_length(m) (0 for a zero noise polynomial),
 * budget = max(0, bit_length(Q) - norm_bits - 1).  budget_hptr [B] and norm_bits_hptr [B] (may be NULL) are host arrays; norm_bits is
 * there because the clamp at 0 hides the magnitude exactly where decryption fails.  One launch after the phase: exact mixed-radix
 * conversion of every coefficient's residue column and a multi-word comparison with (Q+1)/2, one lane per coefficient
 * (hhe_ctx_query("noise_form"): the limb count of the register form the last call took, 0 = the LDS form of more than 8 limbs).
 * A null pointer other than norm_bits_hptr, B == 0, a size other than 2 or 3 or limbs outside 1..L return HHE_ERR_INVALID with both
 * outputs untouched.  Synchronous. */
int hhe_noise_budget(hhe_ctx *c, const uint64_t *sk_hptr, const uint64_t *ct_dptr, int size, int limbs, size_t B, int32_t *budget_hptr,
                     uint32_t *norm_bits_hptr);

/* ---- levels: modulus switching.  On ONE context evaluation (add, multiply, rotate, key switch, transciphering, affine layers, FC
 *      rows) is at its data level; a lower-level ciphertext can be switched further, saved, loaded and decrypted there, and is
 *      evaluated on the context of its level (hhe_ctx_create_level below). ---- */
/* Evaluator::mod_switch_to_inplace (seal/evaluator.h:426) on B coefficient-form ciphertexts:
 * ct [B][size][limbs_in][N] under q_0..q_{limbs_in-1} -> out [B][size][limbs_out][N], dense.
 * Every dropped prime q_m rounds on its own, floor((x + floor(q_m/2)) / q_m), as the chain of mod_switch_to_next does.  size is 2 or
 * 3, 1 <= limbs_out <= limbs_in <= L (limbs_out == limbs_in copies), out must not overlap ct: a violation returns HHE_ERR_INVALID
 * with out untouched (SEAL throws std::invalid_argument on a switch to a higher level).  One kernel launch per chunk of 2^30
 * coefficients, i.e. one per call for any batch a service sends (hhe_ctx_query("mod_switch_launches") counts them).  Synchronous. */
int hhe_mod_switch(hhe_ctx *c, const uint64_t *ct_dptr, int size, size_t B, int limbs_in, int limbs_out, uint64_t *out_dptr);

/* ---- evaluation below the data level.  SEAL's level with l data primes is a BFV context over {q_0 .. q_{l-1}, q_sp}: a level is
 *      a context, and every entry point of this header works at it, unchanged, on [.][l][N]. ---- */
/* the context of the level with `limbs` data primes of c's chain: q_0..q_{limbs-1} and c's special prime, same N, t, device;
 * 1 <= limbs <= L (limbs == L: a second context of the same chain).  An independent context: own lock, workspaces, stream
 * (the default stream until hhe_ctx_set_stream), caches, knobs read from the environment as hhe_ctx_create reads them.
 * Ciphertexts [B][size][limbs][N] written by hhe_mod_switch on c are its data-level ciphertexts, word for word.  Its BEHZ base is a
 * prefix of c's with the same m_sk and gamma.  Destroyed on its own with hhe_ctx_destroy, before or after c. */
int hhe_ctx_create_level(const hhe_ctx *c, int limbs, hhe_ctx **out);
/* dst (a set of a level context) becomes the image of src (a set of a context higher up the same chain): every key src holds,
 * RelinKeys::key(2) and each Galois element, projected to digits I < l and limbs {0..l-1, special}; keys dst held before are gone.
 * Allowed when dst's and src's contexts have the same logn, t and device, equal special primes, and dst's data primes are a prefix of
 * src's (l_dst <= l_src: a level derives from a higher level, equal chains copy); otherwise, and for dst == src, HHE_ERR_INVALID with
 * dst exactly as it was.  All-or-nothing: the new buffers are complete before anything in dst is replaced.  A derived key enters the
 * set as an uploaded one does (a new serial, tables derived from replaced keys dropped, keystreams kept under the old content gone);
 * Shoup quotients and FC correction tables of the level's keys are built on first use.  One kernel launch per key
 * (hhe_ctx_query(dst's context, "key_proj_launches") counts them); runs on the stream dst's context has at the call and waits; src's
 * keys are complete by the contract of hhe_ctx_set_stream.  Locks BOTH contexts, the one with more data limbs first (equal: the lower
 * address first): concurrent derivations in any direction do not deadlock.  hhe_keyset_get_relin / _get_galois on dst return the
 * projected words [l][2][l+1][N]. */
int hhe_keyset_derive_level(hhe_keyset *dst, const hhe_keyset *src);

/* ---- key generation and encryption on the device, from a seed.
 *      THE SEED IS THE ONLY ENTROPY.  seed_hptr is 32 bytes on the host; every random word is SHAKE128 of the seed and a position
 *      (purpose, Galois element, digit or batch item, kind, limb, chunk of 64 coefficients; the definition is in
 *      csrc/hhe_keygen_bodies.h and DESIGN.md section 4), so the same seed for the same purpose repeats the randomness: the caller
 *      supplies 32 FRESH bytes from its own generator per key-generation call and per encryption batch, and keeps them as secret as
 *      the key they make.  Purposes and Galois elements are separate domains, so one seed may serve one call of each kind.
 *      Neither SEAL's nor any other library's random stream is reproduced: keys and ciphertexts are valid BFV objects of the context,
 *      not the words a seal::KeyGenerator would have drawn. ---- */
/* The sampler alone (the test seam of its definition, as hhe_ntt is for the transforms): one polynomial at position
 * (purpose < 256, elt, index) of kind 1 ternary / 2 noise / 3 uniform, out_dptr [mod_count][N] under the moduli
 * mod_base .. mod_base + mod_count - 1 of the table hhe_ntt indexes.  Ternary and noise: residues of one small polynomial;
 * uniform: an independent polynomial per limb (limb = the modulus index).  Shape of util::sample_poly_ternary / sample_poly_cbd /
 * sample_poly_uniform (seal/util/rlwe.h:31-66). */
int hhe_sample_poly(hhe_ctx *c, const uint8_t *seed_hptr, uint32_t purpose, uint32_t elt, uint32_t index, int kind, int mod_base,
                    int mod_count, uint64_t *out_dptr);
/* KeyGenerator::KeyGenerator / secret_key (src/examples/Analyst/Analyst.cpp:38-40, src/examples/hhe_pktnn_examples.cpp:435-437):
 * sk_dptr [K][N], the ternary secret in NTT form under every key-level prime (SecretKey::data() layout, what hhe_decrypt takes
 * once copied to the host) */
int hhe_keygen_secret(hhe_ctx *c, const uint8_t *seed_hptr, uint64_t *sk_dptr);
/* KeyGenerator::create_public_key (Analyst.cpp:41-42, hhe_pktnn_examples.cpp:438-439): pk_dptr [2][K][N] = (-(a s + e), a) at the
 * key level in NTT form (PublicKey::data() layout) */
int hhe_keygen_public(hhe_ctx *c, const uint64_t *sk_dptr, const uint8_t *seed_hptr, uint64_t *pk_dptr);
/* KeyGenerator::create_relin_keys (Analyst.cpp:62-66, hhe_pktnn_examples.cpp:440-441) into a key set.  A generated key enters the set
 * as an uploaded one does: what was derived from a replaced key is dropped and keystreams kept under the set's old content go. */
int hhe_keyset_generate_relin(hhe_keyset *ks, const uint64_t *sk_dptr, const uint8_t *seed_hptr);
/* KeyGenerator::create_galois_keys (Analyst.cpp:68-93, hhe_pktnn_examples.cpp:442-443, 615-617) for the `count` Galois elements
 * elts_hptr (from steps: hhe_ctx_query "galois_elt", as for hhe_keyset_set_galois); count == 0 with elts_hptr == NULL: the default
 * set create_galois_keys(gk) makes without indices (GaloisTool::get_elts_all, seal/util/galois.h:131, one key per element).
 * All-or-nothing: an even element or one >= 2N returns HHE_ERR_INVALID with the set exactly as it was. */
int hhe_keyset_generate_galois(hhe_keyset *ks, const uint64_t *sk_dptr, const uint32_t *elts_hptr, size_t count, const uint8_t *seed_hptr);
/* reading a set back (the analyst ships its RelinKeys / GaloisKeys to the CSP, Analyst.cpp:96-130): ksk_hptr [L][2][K][N];
 * HHE_ERR_NO_RELIN_KEY / HHE_ERR_NO_GALOIS_KEY when the set does not hold the key */
int hhe_keyset_get_relin(const hhe_keyset *ks, uint64_t *ksk_hptr);
int hhe_keyset_get_galois(const hhe_keyset *ks, uint32_t galois_elt, uint64_t *ksk_hptr);
/* Encryptor::encrypt with the public key (the client's PASTA key, src/util/pastahelper.cpp:355-377; the analyst's weight rows,
 * src/util/sealhelper.cpp:123-142) for B plaintexts plain_dptr [B][N] (or [1][N] if plain_bcast; coefficients mod t, from hhe_encode):
 * item b draws u (ternary), e_0, e_1 (noise) at index b; c_k = INTT(NTT(u) pk_k) + e_k on the data-level primes, then the scaled
 * plaintext is added as hhe_add_plain adds it.  out_dptr [B][2][L][N].  (SEAL encrypts at the key level and drops the special
 * prime; the noise is the same to a fraction of a bit.)  On a level context (hhe_ctx_create_level, l data primes) pk is
 * [2][l+1][N]: rows {0..l-1, K-1} of both polynomials of the parent's (api.py: level_rows(pk, l)). */
int hhe_encrypt(hhe_ctx *c, const uint64_t *pk_dptr, const uint64_t *plain_dptr, int plain_bcast, const uint8_t *seed_hptr, size_t B,
                uint64_t *out_dptr);

/* ---- SEAL 4.0 binary serialization at the boundary: the blobs the reference moves over gRPC and spills to
 *      disk (src/examples/CSP/CSP.cpp:328-490 `*.load(*context, bytes, size)`, :495-547 spill file = size_t count followed by
 *      Ciphertext::save streams, :552-605 concatenated stream, protos/hhe.proto:21-24) decoded straight into HBM.
 *      Layout sources: SEALHeader (seal/serialization.h:60-93), DynArray::save_members (seal/dynarray.h:652-680),
 *      KSwitchKeys members (seal/kswitchkeys.h:161-178), PublicKey = Ciphertext (seal/publickey.h:89-93); Ciphertext's member
 *      order is SEAL 4.0.0's as published.  PARITY UNPINNED: the reference holds no serialized SEAL object and libseal is never
 *      run here, so these are checked by round trips and size arithmetic only.  compr_mode none / zlib / zstd are accepted (the
 *      latter two through the system's libz.so.1 / libzstd.so.1, looked up at run time); seeded (symmetric-key) objects are
 *      rejected.  `consumed` returns the size field of the object's header, i.e. where the next object of a stream starts. ---- */
/* Ciphertext::load: data-level, coefficient-form BFV ciphertext -> out_dptr [size][L][N]; *ct_size = 2 or 3;
 * parms_id_out (32 bytes, optional) receives the object's parms_id for later saves */
int hhe_seal_load_ciphertext(hhe_ctx *c, const uint8_t *bytes_hptr, size_t nbytes, uint64_t *out_dptr, size_t out_cap_words,
                             size_t *ct_size, uint8_t *parms_id_out, size_t *consumed);
/* Ciphertext::save(stream, compr_mode_type::none) of a device ciphertext; *written = bytes needed (returned also when out_cap is
 * too small).  parms_id: 32 bytes taken from a loaded object of the same context (SEAL hashes the parameters into it) */
int hhe_seal_save_ciphertext(hhe_ctx *c, const uint64_t *ct_dptr, size_t ct_size, const uint8_t *parms_id, uint8_t *out_hptr,
                             size_t out_cap, size_t *written);
/* Ciphertext::save / Ciphertext::load of a ciphertext at any level of the chain: coeff_modulus_size = limbs, 1 <= limbs <= L, data
 * [size][limbs][N] with every word checked against its prime q_j, j < limbs; the bounds and the all-or-nothing rule of the two entries
 * above.  parms_id is carried, not computed: the caller passes the id of the target level (ContextData::parms_id of the level reached
 * by walking last_context_data() -> prev_context_data()); the loader returns the stream's id and its limb count in *limbs. */
int hhe_seal_save_ciphertext_level(hhe_ctx *c, const uint64_t *ct_dptr, size_t ct_size, int limbs, const uint8_t *parms_id,
                                   uint8_t *out_hptr, size_t out_cap, size_t *written);
int hhe_seal_load_ciphertext_level(hhe_ctx *c, const uint8_t *bytes_hptr, size_t nbytes, uint64_t *out_dptr, size_t out_cap_words,
                                   size_t *ct_size, int *limbs, uint8_t *parms_id_out, size_t *consumed);
/* RelinKeys::load / GaloisKeys::load: every key of the object is uploaded (relin key(2) into `slot`; Galois keys by element
 * 2*index+1, seal/galoiskeys.h:48-74) */
int hhe_seal_load_relin_keys(hhe_ctx *c, int slot, const uint8_t *bytes_hptr, size_t nbytes, size_t *consumed);
int hhe_seal_load_galois_keys(hhe_ctx *c, const uint8_t *bytes_hptr, size_t nbytes, size_t *consumed, uint32_t *n_keys);
/* the same into a key set (one set per loaded object).  All loads are all-or-nothing, as SEAL's load(context, ...) is: the whole
 * object is decoded and validated on the host first; a malformed, truncated or over-long object leaves the target untouched.
 * Inflated sizes are bounded by the largest legitimate object of the context (a few KB of zlib / zstd cannot expand into GBs). */
int hhe_seal_load_relin_keys_ks(hhe_keyset *ks, const uint8_t *bytes_hptr, size_t nbytes, size_t *consumed);
int hhe_seal_load_galois_keys_ks(hhe_keyset *ks, const uint8_t *bytes_hptr, size_t nbytes, size_t *consumed, uint32_t *n_keys);

#ifdef __cplusplus
}
#endif
#endif

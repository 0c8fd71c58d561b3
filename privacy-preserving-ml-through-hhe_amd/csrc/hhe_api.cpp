// hhe_api.cpp -- C ABI of libhhe_gfx950.so: batched BFV evaluator ops on device buffers
// and the PASTA-3 transciphering / FC schedules built from them.  Host code only decides
// the op order (the reference's schedule, src/pasta/pasta_3_seal.cpp); all arithmetic runs
// in the gfx950 kernels of hhe_kernels.hip.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include "hhe_args.h"

namespace {

int need(hhe_ctx *c, size_t B)
{
    if (!c || B == 0) return fail(HHE_ERR_INVALID, "null context or empty batch");
    c->w = &c->lanes[0];
    return lane_reserve(c, c->lanes[0], B);
}

// host staging of a lane: wait for the previous staged copy before the buffers are overwritten; mark the new one
void stage_begin(Lane &ln)
{
    if (ln.stage_pending && ln.ev_stage) rt_event_sync(ln.ev_stage);
    ln.stage_pending = false;
}
void stage_end(Lane &ln)
{
    if (!ln.ev_stage) ln.ev_stage = rt_event_create();
    if (ln.ev_stage && !rt_event_record(ln.ev_stage, ln.stream)) ln.stage_pending = true;
    else rt_sync(ln.stream);
}

void op_ntt(hhe_ctx *c, u64 *polys, size_t count, int mod_base, int mod_cycle, bool inverse, int store_op = STORE_PLAIN)
{
    NttArgs a = ntt_args(c, polys, polys, count, mod_base, mod_cycle);
    a.store_op = store_op;
    k_ntt(a, inverse, c->w->stream);
}
void op_elt(hhe_ctx *c, int op, const u64 *x, const u64 *y, u64 *out, size_t count, int mod_base, int mod_cycle, int b_cycle = 0)
{
    k_elt(elt_args(c, x, y, out, count, mod_base, mod_cycle, b_cycle), op, c->w->stream);
}
// ct (+) ct over [B][size][L][N]
void op_add(hhe_ctx *c, const u64 *x, const u64 *y, u64 *out, size_t B, int size) { op_elt(c, ELT_ADD, x, y, out, B * size * c->L, 0, c->L); }

void op_add_plain(hhe_ctx *c, const u64 *ct, const u64 *plain, const u64 *const *plain_ptrs, size_t shift, bool bcast,
                  bool subtract, bool negate, u64 *out, size_t B, const u32 *ct_map = nullptr)
{
    AddPlainArgs a = c->apl;
    a.ct = ct; a.ct_map = ct_map; a.plain = plain; a.plain_ptrs = plain_ptrs; a.plain_shift = shift; a.out = out; a.B = (int)B;
    a.plain_bcast = bcast; a.subtract = subtract; a.negate_ct = negate;
    k_add_plain(a, c->w->stream);
}

// BatchEncoder::encode: vals [B][stride] (first `count` used) -> plain [B][N]
void op_encode(hhe_ctx *c, const u64 *vals, size_t B, int stride, int count, int second_off, u64 *plain)
{
    rt_memset(plain, 0, B * c->n * 8, c->w->stream);
    EncodeArgs e = zeroed<EncodeArgs>();
    e.vals = vals; e.out = plain; e.slot_map = c->d_slot_map; e.logn = c->logn; e.B = (int)B;
    e.stride = stride; e.count = count; e.second_off = second_off; e.t = c->t;
    k_encode_scatter(e, c->w->stream);
    op_ntt(c, plain, B, c->mod_t, 1, true);
}

// res = Enc(c_b) - KS of a transciphering call (pasta_3_seal.cpp:161-169) for B items, in two halves on the current lane:
//   front: vals [B][128] (zero padded) -> tmp [B][N]; it does not depend on the keystreams
//   back:  out [B][2][L][N] from tmp and the items' keystream ciphertexts
// Fused (fin_fused_on): the first inverse pass mod t gathers its tile from the words (LOAD_ENCODE) and the last one ends in the
// add_plain epilogue (STORE_ADD_PLAIN), which reads item b's keystream at ks_ptrs[b], or at ks + b * 2LN without a table; the
// plaintexts are never written.  Else launch for launch: clear, scatter, transform; add_plain on ks through ks_map (or item for item).
void op_finish_front(hhe_ctx *c, const u64 *vals, u64 *tmp, size_t B)
{
    if (!fin_fused_on(c)) { op_encode(c, vals, B, PASTA_T, PASTA_T, -1, tmp); return; }
    NttArgs a = ntt_args(c, vals, tmp, B, c->mod_t, 1);
    a.load_op = LOAD_ENCODE; a.src_item_polys = 1; a.src_item_stride = PASTA_T; a.fin = c->d_fin;
    k_ntt_pass(a, true, false, c->w->stream);
}
void op_finish_back(hhe_ctx *c, u64 *tmp, const u64 *ks, const u64 *const *ks_ptrs, const u32 *ks_map, u64 *out, size_t B)
{
    if (!fin_fused_on(c)) { op_add_plain(c, ks, tmp, nullptr, 0, false, false, true, out, B, ks_map); return; }
    NttArgs a = ntt_args(c, tmp, tmp, B, c->mod_t, 1);
    a.store_op = STORE_ADD_PLAIN; a.mul = ks; a.mul_ptrs = ks_ptrs; a.aux_out = out; a.fin = c->d_fin;
    k_ntt_pass(a, true, true, c->w->stream);
}

// Both halves for B items in one launch with one workgroup per item (fin_item_for; fin_item_kernel, hhe_fin_bodies.h): the plaintext
// stays in LDS.  The launch is k_ntt's with both ops set; the kernel does not touch `tmp`, the two-pass form of the same launch
// (the tests-only emulator) goes through it.
void op_finish_item(hhe_ctx *c, const u64 *vals, u64 *tmp, const u64 *ks, const u64 *const *ks_ptrs, u64 *out, size_t B)
{
    NttArgs a = ntt_args(c, vals, tmp, B, c->mod_t, 1);
    a.load_op = LOAD_ENCODE; a.src_item_polys = 1; a.src_item_stride = PASTA_T;
    a.store_op = STORE_ADD_PLAIN; a.mul = ks; a.mul_ptrs = ks_ptrs; a.aux_out = out; a.fin = c->d_fin;
    a.base_mask = c->fin_scale32;  // which instantiation the launch takes
    k_ntt(a, true, c->w->stream);
    ++c->fin_item_launches;
}

// plain [P][N] (coefficients mod t) -> lifted NTT form [P][L][N]   
void op_lift_ntt(hhe_ctx *c, const u64 *plain, size_t P, u64 *out)
{
    NttArgs a = ntt_args(c, plain, out, P * c->L, 0, c->L);
    a.src_div = c->L; a.load_op = LOAD_LIFT;
    k_ntt(a, false, c->w->stream);
}

// out = INTT(NTT(ct) * D) with D an NTT-form lifted plaintext: shared [L][N] (ptrs null) or per item
void op_multiply_plain_ntt(hhe_ctx *c, const u64 *ct, const u64 *D, const u64 *const *D_ptrs, size_t shift, u64 *out, size_t B)
{
    NttArgs a = ntt_args(c, ct, out, B * 2 * c->L, 0, c->L);
    a.store_op = STORE_MUL; a.mul = D; a.mul_ptrs = D_ptrs; a.mul_shift = shift; a.mul_cycle = c->L; a.mul_item_polys = 2 * c->L;
    k_ntt(a, false, c->w->stream);
    op_ntt(c, out, B * 2 * c->L, 0, c->L, true);
}

// Shoup quotients floor(key * 2^64 / q_J) of a key-switch key ([L][2][K][N], as the key), built on first use by the
// fused row kernel and cached per key (by its device address; dropped when the key is replaced)
int ensure_key_shoup(hhe_ctx *c, const u64 *key, const u64 **out)
{
    auto it = c->d_key_shoup.find(key);
    if (it != c->d_key_shoup.end()) { *out = it->second; return HHE_OK; }
    DevBuf t(c->ksk_words() * 8);
    if (!t.p) return dev_fail("key Shoup table alloc");
    op_elt(c, ELT_SHOUP, key, nullptr, t.w(), (size_t)c->L * 2 * c->K, 0, c->K);
    if (rt_sync(c->w->stream)) return dev_fail("key Shoup table");
    *out = c->d_key_shoup[key] = t.release();
    return HHE_OK;
}

// [L][N] with q_sp mod q_j in every slot, once per context: the multiplier that turns the transform of a node's c0 into KsRowArgs::c0hat
int ensure_qsp_poly(hhe_ctx *c)
{
    if (c->d_qsp_poly) return 0;
    std::vector<u64> h((size_t)c->L * c->n);
    for (int j = 0; j < c->L; j++) std::fill(h.begin() + (size_t)j * c->n, h.begin() + (size_t)(j + 1) * c->n, c->ksc.qsp_mod[j]);
    if (!(c->d_qsp_poly = (u64 *)rt_malloc(h.size() * 8))) return -1;
    return rt_h2d(c->d_qsp_poly, h.data(), h.size() * 8, c->w->stream) || rt_sync(c->w->stream) ? -1 : 0;
}
// q_sp * NTT(c0) of B items (item b's c0 at ct + b * ct_words) into c0hat [B][L][N]
void op_c0hat(hhe_ctx *c, const u64 *ct, u64 *c0hat, size_t B)
{
    NttArgs t = ntt_args(c, ct, c0hat, B * c->L, 0, c->L);
    t.src_item_polys = c->L; t.src_item_stride = c->ct_words();
    t.store_op = STORE_MUL; t.mul = c->d_qsp_poly; t.mul_cycle = c->L;   // times q_sp: the sum it joins is divided by q_sp in the mod-down
    k_ntt(t, false, c->w->stream);
}

// The two inverse launches that finish a key switch whose sums sit in a split ws_S: the special limbs (STORE_RSP), then the data limbs
// with the mod-down in their store (`ksf`, from ks_ksf_args).  one_grid: the row passes of both share a grid (k_ntt2_inv); else each
// is the second pass of a transform whose row pass a row kernel has already run
void ks_finish_split(hhe_ctx *c, const KsSplit &sp, const NttArgs &ksf, size_t B, bool one_grid)
{
    const NttArgs rsp = ks_rsp_args(c, sp.Usp, sp.Usp, B * 2);
    if (one_grid) { k_ntt2_inv(rsp, ksf, c->w->stream); return; }
    k_ntt_pass(rsp, true, true, c->w->stream);
    k_ntt_pass(ksf, true, true, c->w->stream);
}

// Evaluator::switch_key_inplace core.  d: item b at d + b*d_stride, [L][N] coefficient form.
// out[b] = (base ? base polys selected by mask : 0) + key-switched pair.
// galois_einv > 0 (N >= 4096 only): d and base are the UN-rotated polynomials of a rotation; the digit loads and the base
// fetch of the fused mod-down read them through the Galois map, so no galois_kernel launch and no rotated copy is needed
int op_switch_key(hhe_ctx *c, const u64 *d, size_t d_stride, const u64 *key, const u64 *base, size_t base_stride,
                  int base_mask, u64 *out, size_t B, u32 galois_einv = 0)
{
    const NttArgs a = ks_digit_args(c, d, d_stride, c->w->ws_T, B, galois_einv);
    const u64 *key_s = nullptr;
    const bool rowk = use_row_kernel(c) && ensure_key_shoup(c, key, &key_s) == HHE_OK;
    if (galois_einv && !rowk) return fail(HHE_ERR_DEVICE, "switch_key: Shoup table of the key could not be built");
    if (rowk) {
        // N >= 4096: strided pass of the digit transforms, then ONE kernel for their row pass, the key inner product and
        // the inverse row pass of all 2K sums (ks_row_kernel, as in the matmul loop), then the strided inverse passes with
        // the mod-down fused into the store of the data limbs -- T and S never make a round trip
        const KsSplit sp = ks_split(c, c->w->ws_S, B);
        k_ntt_pass(a, false, false, c->w->stream);
        if (k_ks_row(a, ks_row_args(c, key, key_s, B, &sp), nullptr, c->w->stream)) return dev_fail("switch_key");
        ks_finish_split(c, sp, ks_ksf_args(c, sp, B, base, base_stride, base_mask, galois_einv, out), B, false);
        return HHE_OK;
    }
    k_ntt(a, false, c->w->stream);
    k_ks_mac(ks_mac_args(c, c->w->ws_T, key, c->w->ws_S, B), c->w->stream);
    op_ntt(c, c->w->ws_S, B * 2 * c->K, 0, c->K, true);
    KsFinishArgs f = c->ksf;
    f.S = c->w->ws_S; f.base = base; f.base_item_stride = base_stride; f.base_mask = base ? base_mask : 0; f.out = out; f.B = (int)B;
    k_ks_finish(f, c->w->stream);
    return HHE_OK;
}

int op_apply_galois(hhe_ctx *c, const u64 *ct, u32 elt, u64 *out, size_t B)
{
    const u64 *key = galois_key(c, elt);
    if (!key) return HHE_ERR_NO_GALOIS_KEY;
    const size_t ln = (size_t)c->L * c->n;
    const u32 einv = galois_einv(c, elt);
    const u64 *src = ct;
    if (ct == out) {  // gathers cannot run in place
        rt_d2d(c->w->ws_ct[3], ct, B * c->ct_words() * 8, c->w->stream);
        src = c->w->ws_ct[3];
    }
    if (use_row_kernel(c)) {
        // N >= 4096: no rotated copies -- the digit loads read c1 and the fused mod-down reads c0 through the Galois map
        const u64 *key_s = nullptr;
        int rc = ensure_key_shoup(c, key, &key_s);
        if (rc) return rc;
        return op_switch_key(c, src + ln, 2 * ln, key, src, 2 * ln, 1, out, B, einv);
    }
    // c0' = galois(c0) -> out poly 0 ; d = galois(c1) -> ws_d
    k_galois(galois_args(c, B, einv, src, 2 * ln, out, 2 * ln), c->w->stream);
    k_galois(galois_args(c, B, einv, src + ln, 2 * ln, c->w->ws_d, ln), c->w->stream);
    return op_switch_key(c, c->w->ws_d, ln, key, out, 2 * ln, 1, out, B);
}

// Evaluator::rotate_internal (seal/evaluator.h:1234)
int op_rotate_rows(hhe_ctx *c, const u64 *ct, int step, u64 *out, size_t B)
{
    if (step == 0) {
        if (ct != out) rt_d2d(out, ct, B * c->ct_words() * 8, c->w->stream);
        return HHE_OK;
    }
    const u32 elt = galois_elt_from_step(c, step);
    if (!elt) return fail(HHE_ERR_INVALID, "step count too large");
    if (c->gks->gk.count(elt)) return op_apply_galois(c, ct, elt, out, B);
    const std::vector<int> terms = nt_naf(step);
    if (terms.size() == 1) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
    const u64 *cur = ct;
    for (int term : terms) {
        if ((size_t)std::abs(term) == c->n / 2) continue;
        int rc = op_rotate_rows(c, cur, term, out, B);
        if (rc) return rc;
        cur = out;
    }
    if (cur == ct && ct != out) rt_d2d(out, ct, B * c->ct_words() * 8, c->w->stream);
    return HHE_OK;
}

// non-full-packed preparation of the matmul schedules (pasta_3_seal.cpp:330-336, :379-385; SEAL_Cipher.cpp:231, :279): state += rotate_rows(state, step)
int op_prep_rows(hhe_ctx *c, u64 *state, int step, u64 *scratch, size_t B)
{
    int rc = op_rotate_rows(c, state, step, scratch, B);
    if (!rc) op_add(c, state, scratch, state, B, 2);
    return rc;
}

// One operand of a BEHZ product: in [B][2][L][N] coefficient form -> oq [B][2][L][N] NTT form under the data primes, ob [B][2][L+1][N]
// NTT form of its extension to B_sk (fastbconv_m_tilde + sm_mrq).  Deterministic in the words of `in`.
void op_behz_operand(hhe_ctx *c, const u64 *in, u64 *oq, u64 *ob, size_t B)
{
    const int L = c->L, K = c->K;
    BehzExtendArgs e = zeroed<BehzExtendArgs>();
    e.x = in; e.xb = ob; e.mods = c->d_mods; e.bz = c->d_behz; e.logn = c->logn; e.P = (int)(B * 2); e.L = L; e.K = K;
    k_behz_extend(e, c->w->stream);
    op_ntt(c, ob, B * 2 * (L + 1), K, L + 1, false);
    k_ntt(ntt_args(c, in, oq, B * 2 * L, 0, L), false, c->w->stream);
}
// The passes of a BEHZ product behind its operands: the first operand of B items in the lane's bz_aq / bz_ab, the second at bq / bb in
// the same form; b_div > 0: item b multiplies ciphertext b / b_div of the second operand (TensorArgs::b_div).
// sum > 0: the operands are [sum][B] (the second [sum][1] when b_div is set) and the B results are the floors of the sums of their
// `sum` tensor products (hhe_multiply_sum): one summed tensor launch per modulus set, then the same passes over B * 3 polynomials
// square: the second operand is the first (hhe_square): bq / bb are not read and the squaring kernel runs
void behz_product(hhe_ctx *c, const u64 *bq, const u64 *bb, size_t b_div, u64 *out3, size_t B, size_t sum = 0, bool square = false)
{
    const int L = c->L, K = c->K;
    TensorArgs t = zeroed<TensorArgs>();
    t.mods = c->d_mods; t.logn = c->logn; t.B = (int)B; t.b_div = (int)b_div; t.sum = (int)sum; t.square = square;
    t.a = c->w->bz_aq; t.b = bq; t.d = c->w->bz_dq; t.limbs = L; t.mod_base = 0; t.fold = c->sum_fold_q;
    k_tensor(t, c->w->stream);
    t.a = c->w->bz_ab; t.b = bb; t.d = c->w->bz_db; t.limbs = L + 1; t.mod_base = K; t.fold = c->sum_fold_bsk;
    k_tensor(t, c->w->stream);
    if (sum) c->multiply_sum_launches += 2;
    else if (square) c->square_launches += 2;
    else c->tensor_launches += 2;
    op_ntt(c, c->w->bz_dq, B * 3 * L, 0, L, true, STORE_SCALE_T);
    op_ntt(c, c->w->bz_db, B * 3 * (L + 1), K, L + 1, true, STORE_SCALE_T);
    BehzFloorArgs f = zeroed<BehzFloorArgs>();
    f.dq = c->w->bz_dq; f.db = c->w->bz_db; f.out = out3; f.mods = c->d_mods; f.bz = c->d_behz; f.logn = c->logn;
    f.P = (int)(B * 3); f.L = L; f.K = K;
    k_behz_floor(f, c->w->stream);
}
// Evaluator::bfv_multiply (BEHZ): a, b [B][2][L][N] -> out3 [B][3][L][N]
void op_multiply(hhe_ctx *c, const u64 *x, const u64 *y, u64 *out3, size_t B)
{
    op_behz_operand(c, x, c->w->bz_aq, c->w->bz_ab, B);
    const u64 *bq = c->w->bz_aq, *bb = c->w->bz_ab;
    if (y != x) { op_behz_operand(c, y, c->w->bz_bq, c->w->bz_bb, B); bq = c->w->bz_bq; bb = c->w->bz_bb; }
    behz_product(c, bq, bb, 0, out3, B);
}
// Evaluator::square at size 2: one operand extension and the squaring kernel; the words of op_multiply(c, x, x, ..)
void op_square(hhe_ctx *c, const u64 *x, u64 *out3, size_t B)
{
    op_behz_operand(c, x, c->w->bz_aq, c->w->bz_ab, B);
    behz_product(c, nullptr, nullptr, 0, out3, B, 0, true);
}
// ... against a resident encrypted matrix: x [r][per][2][L][N], the r rotations of `per` items, rotation-major; product (i, b) is
// multiply(x[i][b], W_i) with W_i in the form the handle keeps -> out3 [r][per][3][L][N].  One extension, one transform and one floor
// over all r * per products; the lane is reserved for that many items.
void op_multiply_enc(hhe_ctx *c, const u64 *x, const hhe_enc_matrix *m, u64 *out3, size_t per)
{
    op_behz_operand(c, x, c->w->bz_aq, c->w->bz_ab, m->r * per);
    behz_product(c, m->wq, m->wb, per, out3, m->r * per);
}
// ... with the r products of an item summed before the floor (hhe_multiply_sum over x and the resident diagonals): out3 [per][3][L][N]
void op_multiply_sum_enc(hhe_ctx *c, const u64 *x, const hhe_enc_matrix *m, u64 *out3, size_t per)
{
    op_behz_operand(c, x, c->w->bz_aq, c->w->bz_ab, m->r * per);
    behz_product(c, m->wq, m->wb, 1, out3, per, m->r);
}

int op_relinearize(hhe_ctx *c, const u64 *a3, u64 *out, size_t B)
{
    if (!c->rks->rk) return fail(HHE_ERR_NO_RELIN_KEY, "relinearization key not set");
    const size_t ln = (size_t)c->L * c->n;
    return op_switch_key(c, a3 + 2 * ln, 3 * ln, c->rks->rk, a3, 3 * ln, 3, out, B);
}

// ------------------------------------------------------------------ PASTA public tables
int ensure_feistel_mask(hhe_ctx *c)
{
    if (c->d_feistel_mask) return HHE_OK;
    const size_t n = c->n, half = n / 2;
    // mask_vec: ones on [1,128) and [N/2+1, N/2+128) (pasta_3_seal.cpp:230-235)
    std::vector<u64> vals(2 * PASTA_T, 1);
    vals[0] = 0; vals[PASTA_T] = 0;
    DevBuf dv(vals.size() * 8), pl(n * 8), mask((size_t)c->L * n * 8);
    if (!dv.p || !pl.p || !mask.p) return dev_fail("feistel mask alloc");
    rt_h2d(dv.p, vals.data(), vals.size() * 8, c->w->stream);
    op_encode(c, dv.w(), 1, 2 * PASTA_T, PASTA_T, (int)half, pl.w());
    op_lift_ntt(c, pl.w(), 1, mask.w());
    if (rt_sync(c->w->stream)) return dev_fail("feistel mask");
    c->d_feistel_mask = mask.release();
    return HHE_OK;
}

void free_block(BlockTables &bt) { rt_free(bt.diag); rt_free(bt.pdiag); rt_free(bt.rc); rt_free(bt.bsgs); }
// make room for `need` more bytes of block tables: the least recently used counters that the running call (c->block_call) does not
// use are dropped while the cache would pass its limit.  A single call that needs more than the limit is served anyway.
void evict_blocks(hhe_ctx *c, size_t need)
{
    while (c->block_bytes + need > c->block_cache_limit) {
        auto victim = c->blocks.end();
        for (auto it = c->blocks.begin(); it != c->blocks.end(); ++it)
            if (it->second.last_call != c->block_call && (victim == c->blocks.end() || it->second.last_call < victim->second.last_call)) victim = it;
        if (victim == c->blocks.end()) return;
        sync_ctx(c);  // earlier batched calls have completed (they wait for their work), but generic ops enqueued on the caller's stream may lag
        c->block_bytes -= victim->second.bytes;
        free_block(victim->second);
        c->ks_cache.drop_counter(c, victim->first);  // a kept keystream goes with its counter's tables
        c->blocks.erase(victim);
    }
}
// Public tables of one (nonce, counter) pair, built on the device on first use.  Footprint per pair: (4 x 128 x L) x N words of
// multipliers -- twice that for `pdiag` with its Shoup quotients (fused pipeline; 768 MiB at N = 2^15, L = 3), once for `diag`
// (op-by-op schedule, HHE_MATMUL=0) -- plus 4 N words of round constants; the babystep-giantstep variant adds (4 x 128 x L) x N on
// its first use.  The cache is bounded (hhe_pasta3_set_block_cache_limit); hhe_pasta3_clear_block_cache() releases everything.
constexpr size_t PASTA_MATS_WORDS = (size_t)(PASTA_R + 1) * 2 * PASTA_T * PASTA_T, PASTA_RCS_WORDS = (size_t)(PASTA_R + 1) * 2 * PASTA_T;
size_t block_entry_bytes(const hhe_ctx *c)
{
    const size_t ndiag = (size_t)(PASTA_R + 1) * PASTA_T;
    return (c->matmul_mode == 1 ? 2 : 1) * ndiag * c->L * c->n * 8 + (size_t)(PASTA_R + 1) * c->n * 8;
}
size_t block_bsgs_bytes(const hhe_ctx *c) { return (size_t)(PASTA_R + 1) * PASTA_T * c->L * c->n * 8; }
// the randomness of a pair as the table pipeline takes it: on the host (uploaded here, behind the eviction) or already on the device
struct PairRandomness {
    const u64 *h_mats = nullptr, *h_rcs = nullptr;
    const u64 *d_mats = nullptr, *d_rcs = nullptr;
};
int build_block(hhe_ctx *c, const PastaPair &id, const PairRandomness &r, BlockTables **out)
{
    const size_t n = c->n, half = n / 2;
    const int L = c->L;
    const size_t ndiag = (size_t)(PASTA_R + 1) * PASTA_T;
    const bool fused = c->matmul_mode == 1;
    const size_t entry_bytes = block_entry_bytes(c);
    evict_blocks(c, entry_bytes);
    DevBuf d_mats(r.d_mats ? 8 : PASTA_MATS_WORDS * 8), d_rcs(r.d_rcs ? 8 : PASTA_RCS_WORDS * 8), slots(ndiag * n * 8), diag(ndiag * L * n * 8),
        rc((size_t)(PASTA_R + 1) * n * 8), pdiag(fused ? 2 * ndiag * L * n * 8 : 8);  // pdiag | its Shoup quotients
    if (!d_mats.p || !d_rcs.p || !slots.p || !diag.p || !rc.p || !pdiag.p) return dev_fail("block table alloc");
    if (!r.d_mats) {
        rt_h2d(d_mats.p, r.h_mats, PASTA_MATS_WORDS * 8, c->w->stream);
        rt_h2d(d_rcs.p, r.h_rcs, PASTA_RCS_WORDS * 8, c->w->stream);
    }
    // 128 diagonals per affine layer -> slot image -> INTT mod t (= batch encode) -> lift + NTT per limb
    rt_memset(slots.p, 0, ndiag * n * 8, c->w->stream);
    DiagArgs d = zeroed<DiagArgs>();
    d.mats = r.d_mats ? r.d_mats : d_mats.w(); d.out = slots.w(); d.slot_map = c->d_slot_map; d.logn = c->logn;
    k_diag(d, c->w->stream);
    op_ntt(c, slots.w(), ndiag, c->mod_t, 1, true);
    op_lift_ntt(c, slots.w(), ndiag, diag.w());
    // round constants: rc1 -> slots [0,128), rc2 -> slots [N/2, N/2+128) (pasta_3_plain.cpp:286-295)
    op_encode(c, r.d_rcs ? r.d_rcs : d_rcs.w(), PASTA_R + 1, 2 * PASTA_T, PASTA_T, (int)half, rc.w());
    if (fused) {
        // pdiag = diag o pi_g for g = elt(rotate_rows -1): multiplier tables in the rotated NTT frame
        PermArgs p = perm_args(c, ndiag * L, diag.w(), pdiag.w(), (size_t)L * n);
        p.elt = galois_elt_from_step(c, -1);
        k_perm(p, c->w->stream);
        op_elt(c, ELT_SHOUP, pdiag.w(), nullptr, pdiag.w() + ndiag * L * n, ndiag * L, 0, L);
    }
    if (rt_sync(c->w->stream)) return dev_fail("block tables");
    BlockTables bt;
    bt.rc = rc.release();
    if (fused) bt.pdiag = pdiag.release();  // the fused pipeline reads only pdiag: diag is dropped with this scope
    else bt.diag = diag.release();
    bt.bytes = entry_bytes;
    bt.last_call = c->block_call;
    c->block_bytes += entry_bytes;
    auto ins = c->blocks.emplace(id, bt);
    *out = &ins.first->second;
    return HHE_OK;
}

// babystep-giantstep multiplier tables of one pair (lazy): same pipeline as `diag` with the rearranged diagonals
int build_bsgs(hhe_ctx *c, BlockTables *bt, const PairRandomness &r)
{
    const size_t n = c->n;
    const int L = c->L;
    const size_t ndiag = (size_t)(PASTA_R + 1) * PASTA_T;
    evict_blocks(c, ndiag * L * n * 8);
    DevBuf d_mats(r.d_mats ? 8 : PASTA_MATS_WORDS * 8), slots(ndiag * n * 8), bsgs(ndiag * L * n * 8);
    if (!d_mats.p || !slots.p || !bsgs.p) return dev_fail("bsgs table alloc");
    if (!r.d_mats) rt_h2d(d_mats.p, r.h_mats, PASTA_MATS_WORDS * 8, c->w->stream);
    rt_memset(slots.p, 0, ndiag * n * 8, c->w->stream);
    BsgsDiagArgs d = zeroed<BsgsDiagArgs>();
    d.mats = r.d_mats ? r.d_mats : d_mats.w(); d.out = slots.w(); d.slot_map = c->d_slot_map; d.logn = c->logn; d.n1 = 16;
    k_bsgs_diag(d, c->w->stream);
    op_ntt(c, slots.w(), ndiag, c->mod_t, 1, true);
    op_lift_ntt(c, slots.w(), ndiag, bsgs.w());
    if (rt_sync(c->w->stream)) return dev_fail("bsgs tables");
    bt->bsgs = bsgs.release();
    bt->bytes += ndiag * L * n * 8;
    c->block_bytes += ndiag * L * n * 8;
    return HHE_OK;
}

// Pasta::init_shake + get_random_matrix + get_rc_vec (pasta_3_plain.cpp:56-119) for `count` pairs on the device: one XOF launch with a
// pair per lane, one expansion launch (a workgroup per pair and layer), nothing in between -- the stream orders them.  d_pairs
// [count], d_rand [count][2048], mats [count][4][2][128][128], rcs [count][4][2][128] are the caller's; enqueued on st
void public_randomness_enqueue(hhe_ctx *c, const PastaPair *pairs, size_t count, PastaPair *d_pairs, u64 *d_rand, u64 *mats, u64 *rcs, rt_stream st)
{
    rt_h2d(d_pairs, pairs, count * sizeof(PastaPair), st);
    PastaXofArgs x = zeroed<PastaXofArgs>();
    x.mode = XOF_PASTA;
    x.t = c->t; x.nblocks = (int)count; x.rand = d_rand; x.pairs = d_pairs;
    int bits = 0;
    for (u64 v = c->t; v; v >>= 1) ++bits;
    x.mask = bits >= 64 ? ~(u64)0 : (((u64)1 << bits) - 1);  // Pasta::Pasta(): max_prime_size (pasta_3_plain.cpp:150-153)
    k_pasta_xof(x, st);
    PastaPlainArgs p = zeroed<PastaPlainArgs>();
    p.mode = PP_MODE_EXPAND;
    p.t = c->t;
    p.r_hi = (u64)(((unsigned __int128)1 << 64) / c->t);
    p.r_lo = (u64)(((((unsigned __int128)1 << 64) % c->t) << 64) / c->t);
    p.rand = d_rand; p.nblocks = (int)count; p.mats = mats; p.rcs = rcs;
    k_pasta_plain(p, st);
}

// From this many missing pairs on, a call with HHE_PUBLIC_DEVICE unset draws their randomness on the device: a single lane's sponge
// is slower than a host core, many lanes at once are not.  profiles/block_tables_time.json (tools/block_tables_time.py, one MI355X):
// the host draws a pair in 0.53 ms, the two device launches take 3.0 ms for 1 to 40 pairs alike; builds of 1 and 4 missing pairs
// measured faster with the host's randomness (2.1 / 4.7 ms, 8.4 / 9.4 ms), builds of 16 and 40 with the device's.
constexpr size_t PUBLIC_DEVICE_MIN = 8;
constexpr size_t PUBLIC_DEVICE_BATCH = 256;  // pairs per XOF / expansion launch (1 MiB of matrices each); a call with more misses runs in rounds

// The public tables of the U pairs of a call (pinned for its duration; duplicates allowed): tabs[u], with the babystep-giantstep
// variant where use_bsgs.  The pairs the cache lacks get their randomness first -- on the host, pair by pair, or on the device for
// all of them at once (public_randomness_enqueue) -- and then go through the per-pair table pipeline.  *built: pairs anything was built for
int ensure_blocks(hhe_ctx *c, const PastaPair *pairs, size_t U, int use_bsgs, BlockTables **tabs, size_t *built = nullptr)
{
    std::vector<PastaPair> miss;  // distinct, in order of first appearance
    {
        std::map<PastaPair, bool> seen;
        for (size_t u = 0; u < U; ++u) {
            auto it = c->blocks.find(pairs[u]);
            if (it != c->blocks.end()) it->second.last_call = c->block_call;
            if ((it == c->blocks.end() || (use_bsgs && !it->second.bsgs)) && seen.emplace(pairs[u], true).second) miss.push_back(pairs[u]);
        }
    }
    if (built) *built = miss.size();
    if (miss.empty()) {  // the steady state of a service: nothing below is allocated
        for (size_t u = 0; u < U; ++u) tabs[u] = &c->blocks.find(pairs[u])->second;
        return HHE_OK;
    }
    const bool on_device = c->public_device >= 0 ? c->public_device != 0 : miss.size() >= PUBLIC_DEVICE_MIN;
    int rc = HHE_OK;
    auto build = [&](const PastaPair &id, const PairRandomness &r) {
        BlockTables *bt = nullptr;
        auto it = c->blocks.find(id);
        if (it != c->blocks.end()) bt = &it->second;
        else if (int e = build_block(c, id, r, &bt)) return e;
        return use_bsgs && !bt->bsgs ? build_bsgs(c, bt, r) : (int)HHE_OK;
    };
    if (on_device) {
        for (size_t m0 = 0; m0 < miss.size() && !rc; m0 += PUBLIC_DEVICE_BATCH) {
            const size_t cnt = std::min(PUBLIC_DEVICE_BATCH, miss.size() - m0);
            DevBuf d_pairs(cnt * sizeof(PastaPair)), d_rand(cnt * PASTA_RAND_PER_BLOCK * 8), d_mats(cnt * PASTA_MATS_WORDS * 8), d_rcs(cnt * PASTA_RCS_WORDS * 8);
            if (!d_pairs.p || !d_rand.p || !d_mats.p || !d_rcs.p) return dev_fail("public randomness alloc");
            public_randomness_enqueue(c, miss.data() + m0, cnt, (PastaPair *)d_pairs.p, d_rand.w(), d_mats.w(), d_rcs.w(), c->w->stream);
            c->last_public_built += cnt;
            for (size_t m = 0; m < cnt && !rc; ++m) {
                PairRandomness r;
                r.d_mats = d_mats.w() + m * PASTA_MATS_WORDS; r.d_rcs = d_rcs.w() + m * PASTA_RCS_WORDS;
                rc = build(miss[m0 + m], r);
            }
            if (rc) rt_sync(c->w->stream);  // the buffers above go with this scope
        }
    } else {
        std::vector<u64> mats(PASTA_MATS_WORDS), rcs(PASTA_RCS_WORDS);
        for (size_t m = 0; m < miss.size() && !rc; ++m) {
            pasta3_block_randomness(c->t, miss[m].nonce, miss[m].counter, mats.data(), rcs.data());
            PairRandomness r;
            r.h_mats = mats.data(); r.h_rcs = rcs.data();
            rc = build(miss[m], r);
        }
    }
    if (rc) return rc;
    for (size_t u = 0; u < U; ++u) tabs[u] = &c->blocks.find(pairs[u])->second;
    return HHE_OK;
}

// PASTA_SEAL::babystep_giantstep (pasta_3_seal.cpp:267-366), N1 = 16, N2 = 8 (pasta_3_seal.h:35-36): 15 baby
// rotations by -1, 8 inner sums of 16 plain products (accumulated in the NTT domain), 7 giant
// rotations by -16k.  State in ws_ct[0]; the lane's ws_rot holds ROT_SLOTS ciphertexts per item (reserved by the caller).
constexpr int ROT_SLOTS = 16;  // Lane::ws_rot per item: the N1 baby steps here, the trie depths of the FC row
int matmul_bsgs(hhe_ctx *c, int layer, const u64 *const *d_bsgs_ptrs, size_t B)
{
    constexpr int N1 = ROT_SLOTS, N2 = 8;
    const int L = c->L;
    const size_t n = c->n, ctw = c->ct_words();
    Lane &w = *c->w;
    u64 *state = w.ws_ct[0], *inner = w.ws_ct[1], *scratch = w.ws_ct[2], *outer = w.ws_ct3;  // ct3 holds [B][3].. >= [B][2]
    u64 *rot = w.ws_rot.p;  // rot[j] laid out [j][B][2][L][N]
    int rc;
    if (n / 2 != PASTA_T && (rc = op_prep_rows(c, state, PASTA_T, scratch, B))) return rc;
    rt_d2d(rot, state, B * ctw * 8, w.stream);
    for (int j = 1; j < N1; ++j)
        if ((rc = op_rotate_rows(c, rot + (size_t)(j - 1) * B * ctw, -1, rot + (size_t)j * B * ctw, B))) return rc;
    for (int k = 0; k < N2; ++k) {
        rt_memset(inner, 0, B * ctw * 8, w.stream);
        for (int j = 0; j < N1; ++j) {
            NttArgs a = ntt_args(c, rot + (size_t)j * B * ctw, scratch, B * 2 * L, 0, L);
            a.store_op = STORE_MAC; a.mul_ptrs = d_bsgs_ptrs; a.mul_shift = ((size_t)layer * PASTA_T + k * N1 + j) * L * n;
            a.mul_cycle = L; a.mul_item_polys = 2 * L; a.acc = inner;
            k_ntt(a, false, w.stream);
        }
        op_ntt(c, inner, B * 2 * L, 0, L, true);
        if (k == 0) rt_d2d(outer, inner, B * ctw * 8, w.stream);
        else {
            if ((rc = op_rotate_rows(c, inner, -k * N1, inner, B))) return rc;
            op_add(c, outer, inner, outer, B, 2);
        }
    }
    rt_d2d(state, outer, B * ctw * 8, w.stream);
    return HHE_OK;
}

// PASTA_SEAL::diagonal (pasta_3_seal.cpp:370-413) for affine layer `layer`, state in ws_ct[0].
// The 128 products are accumulated in the NTT domain and inverse-transformed once, which
// yields the same words as SEAL's multiply_plain + add_inplace chain.
int matmul_diagonal(hhe_ctx *c, int layer, const u64 *const *d_diag_ptrs, size_t B)
{
    const int L = c->L;
    const size_t n = c->n;
    u64 *state = c->w->ws_ct[0], *acc = c->w->ws_ct[1], *scratch = c->w->ws_ct[2];
    int rc;
    if (n / 2 != PASTA_T && (rc = op_prep_rows(c, state, PASTA_T, scratch, B))) return rc;
    rt_memset(acc, 0, B * c->ct_words() * 8, c->w->stream);
    for (int i = 0; i < PASTA_T; ++i) {
        if (i && (rc = op_rotate_rows(c, state, -1, state, B))) return rc;
        NttArgs a = ntt_args(c, state, scratch, B * 2 * L, 0, L);
        a.store_op = STORE_MAC; a.mul_ptrs = d_diag_ptrs; a.mul_shift = ((size_t)layer * PASTA_T + i) * L * n;
        a.mul_cycle = L; a.mul_item_polys = 2 * L; a.acc = acc;
        k_ntt(a, false, c->w->stream);
    }
    op_ntt(c, acc, B * 2 * L, 0, L, true);
    rt_d2d(state, acc, B * c->ct_words() * 8, c->w->stream);
    return HHE_OK;
}

// hhe_ctx_profile: one timed event pair around a launch on the lane's stream (the stream the kernel runs on)
struct ProfScope {
    Lane *ln = nullptr;
    void *e1 = nullptr;
    ProfScope(hhe_ctx *c, Lane &lane, size_t items)
    {
        if (!c->profile) return;
        if (lane.prof_used == lane.prof_ev.size()) {
            void *a = rt_event_create_timed(), *b = rt_event_create_timed();
            if (!a || !b) { rt_event_destroy(a); rt_event_destroy(b); return; }
            lane.prof_ev.emplace_back(a, b);
        }
        auto &pr = lane.prof_ev[lane.prof_used++];
        ln = &lane; e1 = pr.second;
        c->prof_items += items;
        rt_event_record(pr.first, lane.stream);
    }
    ~ProfScope() { if (ln) rt_event_record(e1, ln->stream); }
};

// PASTA_SEAL::diagonal (pasta_3_seal.cpp:370-413) as a fused pipeline: same ciphertext words as the
// op-by-op schedule, 20 transforms per rotation step instead of 35 (DESIGN.md "fused matmul").
//  - c0 stays in NTT form across the 127 rotate_rows(-1); c1 is kept in coefficient form because the
//    key-switch digits need its canonical residues;
//  - the 128 plain products are accumulated in the NTT domain, in the frame rotated by the Galois map
//    (pdiag tables), so the NTT of galois(c1) computed for the key switch is reused for the product;
//  - mod-down of c0 is finished in the NTT domain: NTT_j(r_0 mod q_j - half) replaces INTT+NTT.
// Shared first layer (`cap`, B = 1, state = the key ciphertext every item starts from): the chain's own plain products are not
// needed (they go to a scratch accumulator).  Instead the chain leaves state i where it is: c0 (NTT form) in slot i % S of cap->c0
// and the Galois-mapped c1 (the digit source d) in slot i % S of cap->d -- the step writes its successor's straight into the next
// slots, so the chain has no launch more than a plain one.  Once S states are there, l0_flush turns them into the two operands
// the plain products of those steps consume, in the frame in which pdiag multiplies them -- R0_i = c0 read through the NTT-domain
// map of g (one gather launch for all slots), R1_i = NTT_j(d_j) (one transform launch pair, in place) -- and adds the items'
// diagonal sums of the S steps into `out`.
struct L0Capture {
    u64 *c0, *r0, *d;  // [S][L][N] each: c0 of the states | R0 | d of the states, then R1
    int S;             // >= 2: a step reads slot i and writes slot i + 1
    u64 *out;          // [B][2][L][N]: accp0 | accp1 of item b (NTT form, rotated frame)
    size_t B;
};
void l0_flush(hhe_ctx *c, const L0Capture &cap, int first, int steps)
{
    const size_t ln = (size_t)c->L * c->n;
    PermArgs p = perm_args(c, (size_t)steps * c->L, cap.c0, cap.r0, ln);
    p.elt = galois_elt_from_step(c, -1);
    k_perm(p, c->w->stream);
    op_ntt(c, cap.d, (size_t)steps * c->L, 0, c->L, false);
    p = perm_args(c, cap.B * c->L, cap.r0, cap.out, 2 * ln);
    p.steps = steps; p.carry = first > 0; p.in2 = cap.d; p.in_step_stride = ln; p.out2 = cap.out + ln;
    p.mul_ptrs = c->l0_ptrs.p; p.mul_shift = (size_t)first * ln; p.mul_step_stride = ln;
    k_perm(p, c->w->stream);
}
// What the loop is run for: PASTA's affine layer `layer` (128 steps of rotate_rows(-1), the tables of build_block) or a plain-matrix
// handle (hhe_matrix: dim steps of rotate_rows(+1), one table for every item)
struct DiagSched {
    int steps;      // diagonals = states of the chain
    int rot_step;   // the chain's rotate_rows step; the tables are composed with the NTT-domain map of its Galois element
    int pre_step;   // non-full-packed preparation: state += rotate_rows(state, pre_step); 0: none
    size_t base;    // words from an item's table pointer to diagonal 0 ([steps][L][N] follow)
    size_t s_off;   // words from a multiplier to its Shoup quotient
};
DiagSched pasta_sched(const hhe_ctx *c, int layer)
{
    const size_t ln = (size_t)c->L * c->n;
    return DiagSched{PASTA_T, -1, c->n / 2 != (size_t)PASTA_T ? PASTA_T : 0, (size_t)layer * PASTA_T * ln, (size_t)(PASTA_R + 1) * PASTA_T * ln};
}
int matmul_diagonal_fused(hhe_ctx *c, const DiagSched &sch, const u64 *const *d_pdiag_ptrs, size_t B, const L0Capture *cap = nullptr)
{
    const int L = c->L, K = c->K;
    const size_t n = c->n, ln = (size_t)L * n, bln = B * ln;
    const int nsteps = sch.steps;
    u64 *state = c->w->ws_ct[0];
    if (sch.pre_step) {
        int rc = op_prep_rows(c, state, sch.pre_step, c->w->ws_ct[2], B);
        if (rc) return rc;
    }
    const u32 g = galois_elt_from_step(c, sch.rot_step);
    const u64 *key = galois_key(c, g);
    if (!key) return HHE_ERR_NO_GALOIS_KEY;
    const u32 ginv = galois_einv(c, g);
    u64 *accp0 = c->w->ws_ct[1], *accp1 = c->w->ws_ct[1] + bln;
    u64 *c0n[2] = {c->w->ws_ct[2], c->w->ws_ct[2] + bln};
    u64 *scr = c->w->ws_ct[3], *r = c->w->ws_ct[3] + bln, *scr2 = c->w->ws_ct3;
    rt_memset(c->w->ws_ct[1], 0, 2 * bln * 8, c->w->stream);
    // state i of the chain: its c0 in NTT form and its digit source
    auto c0_of = [&](int i) { return cap ? cap->c0 + (size_t)(i % cap->S) * ln : c0n[i & 1]; };
    auto d_of = [&](int i) { return cap ? cap->d + (size_t)(i % cap->S) * ln : c->w->ws_d; };
    u64 *d_src = d_of(0), *d_dst = d_of(1);  // the current step's
    {   // c0 -> NTT form ; d = galois(c1)
        NttArgs a = ntt_args(c, state, c0_of(0), B * L, 0, L);
        a.src_item_polys = L; a.src_item_stride = 2 * ln;
        k_ntt(a, false, c->w->stream);
        k_galois(galois_args(c, B, ginv, state + ln, 2 * ln, d_src, ln), c->w->stream);
    }
    // The c0 branch of step i only feeds the c0 branch of step i+1, and like the digit transforms of step i+1 it depends on
    // nothing later than the inverse transforms of step i: it is held back (k5) and launched in the grids of step i+1.
    // the shared chain takes the separate-kernel step for every N: one ciphertext is latency-bound either way, and the row kernel's
    // profile counters (hhe_ctx_profile) keep counting batch launches only
    const bool rowk = use_row_kernel(c) && !cap;
    const size_t pdiag_words = sch.s_off;  // the Shoup quotients of pdiag follow the table (build_block, hhe_matrix_create)
    const u64 *key_s = nullptr;
    if (rowk) {
        int rc = ensure_key_shoup(c, key, &key_s);
        if (rc) return rc;
    }
    NttArgs k5;
    bool k5_pending = false;
    // digit transforms of the current d: T[I][J] = NTT_J(d[I] mod q_J)
    auto digit_args = [&]() { return ks_digit_args(c, d_src, ln, c->w->ws_T, B); };
    // N >= 4096 -- four launches per step: strided pass of the digit transforms (+ the held-back c0 branch's strided pass in
    // the same grid); ks_row_kernel = row pass + key inner product + inverse row pass (+ the c0 branch's row pass as extra
    // tiles; S_0 alternates between the two halves of ws_S, so that branch reads the previous step's while this step's is
    // written); strided inverse pass of the special limbs (r_k = INTT(S_k[special]) + floor(q_sp/2)); strided inverse pass
    // of the c1 limbs with the mod-down epilogue and the Galois map (the next digits' source)
    int krc = 0;
    auto step_row_kernel = [&](int i, size_t shift) {
        const NttArgs a = digit_args();
        if (k5_pending) k_ntt2_fwd_first(k5, a, c->w->stream);
        else k_ntt_pass(a, false, false, c->w->stream);
        KsRowArgs x = ks_row_args(c, key, key_s, B);
        x.S = c->w->ws_S + (size_t)(i & 1) * K * n; x.U1 = scr; x.u_stride = ln; x.Usp = r;
        x.acc = accp1; x.mul_ptrs = d_pdiag_ptrs; x.mul_shift = shift; x.mul_s_off = pdiag_words;
        {
            ProfScope prof(c, *c->w, B);
            krc |= k_ks_row(a, x, k5_pending ? &k5 : nullptr, c->w->stream);
        }
        k5_pending = false;
        k_ntt_pass(ks_rsp_args(c, r, r, B * 2), true, true, c->w->stream);
        NttArgs a1 = ntt_args(c, scr, scr, B * L, 0, L);
        a1.store_op = STORE_KS1; a1.aux_r = r; a1.aux_out = d_dst; a1.gal_elt = g;
        k_ntt_pass(a1, true, true, c->w->stream);
    };
    // every context without the row kernel (use_row_kernel: N < 4096 with its ragged tiles, or ANY N when a coefficient prime lacks
    // the pseudo-Mersenne form, e.g. BFVDefault(4096)) -- the same step with the inner product as its own kernel: T and S are materialised
    auto step_separate = [&](size_t shift) {
        const NttArgs a = digit_args();
        KsMacArgs m = ks_mac_args(c, c->w->ws_T, key, c->w->ws_S, B);
        if (!cap) { m.acc = accp1; m.mul_ptrs = d_pdiag_ptrs; m.mul_shift = shift; }  // the I = J digit also feeds the plain product
        if (k5_pending) { k_ntt2_fwd(k5, a, c->w->stream); k5_pending = false; }
        else k_ntt(a, false, c->w->stream);
        k_ks_mac(m, c->w->stream);
        const NttArgs as = ks_rsp_args(c, c->w->ws_S, r, B * 2, true);
        NttArgs a1 = ntt_args(c, c->w->ws_S + (size_t)K * n, scr, B * L, 0, L);
        a1.src_item_polys = L; a1.src_item_stride = (size_t)2 * K * n; a1.store_op = STORE_KS1;
        a1.aux_r = r; a1.aux_out = d_dst; a1.gal_elt = g;
        k_ntt2_inv(as, a1, c->w->stream);
    };
    for (int i = 0; i < nsteps - 1; ++i) {
        const size_t shift = sch.base + (size_t)i * ln;
        d_src = d_of(i); d_dst = d_of(i + 1);
        if (cap && (i + 1) % cap->S == 0) {
            // the table is full (state i sits in its last slot) and this step writes state i + 1 into slot 0: finish state i's c0,
            // keep its d for this step (the flush transforms the slots in place), hand the S states to the items
            if (k5_pending) { k_ntt(k5, false, c->w->stream); k5_pending = false; }
            rt_d2d(c->w->ws_d, d_src, ln * 8, c->w->stream);
            d_src = c->w->ws_d;
            l0_flush(c, *cap, i + 1 - cap->S, cap->S);
        }
        if (rowk) step_row_kernel(i, shift);
        else step_separate(shift);
        {   // c0 of the next state in NTT form + permuted-frame product of the current c0
            NttArgs a = ntt_args(c, r, scr2, B * L, 0, L);
            a.src_item_polys = L; a.src_item_stride = 2 * n; a.src_div = L; a.load_op = LOAD_RNEG;
            a.store_op = STORE_KS0; a.aux_in = c0_of(i); a.aux_out = c0_of(i + 1); a.acc = accp0;
            a.aux_r = c->w->ws_S + (rowk ? (size_t)(i & 1) * K * n : 0);
            a.mul_ptrs = d_pdiag_ptrs; a.mul_shift = shift; a.gal_elt = g; a.mul_s_off = pdiag_words;
            k5 = a; k5_pending = true;  // launched in the grid of the next step's digit transforms
        }
    }
    if (krc) return dev_fail("matmul: key-switch row kernel");
    if (k5_pending) k_ntt(k5, false, c->w->stream);
    if (cap) {   // the last block of states; the items' tails (shared_l0_tail) follow on their own lanes
        const int first = (nsteps - 1) / cap->S * cap->S;
        l0_flush(c, *cap, first, nsteps - first);
        return HHE_OK;
    }
    const size_t shift = sch.base + (size_t)(nsteps - 1) * ln;
    {   // last state: products only (a "virtual" rotation keeps the frame uniform)
        NttArgs a = ntt_args(c, d_of(nsteps - 1), scr, B * L, 0, L);
        a.store_op = STORE_MAC; a.mul_ptrs = d_pdiag_ptrs; a.mul_shift = shift; a.mul_cycle = L; a.mul_item_polys = L; a.acc = accp1;
        k_ntt(a, false, c->w->stream);
        PermArgs p = perm_args(c, B * L, c0_of(nsteps - 1), accp0, ln);
        p.elt = g; p.mac = 1; p.mul_ptrs = d_pdiag_ptrs; p.mul_shift = shift;
        k_perm(p, c->w->stream);
        // back to the unrotated frame, then to coefficient form
        p.mac = 0; p.mul_ptrs = nullptr; p.elt = ginv; p.out_item_stride = 2 * ln;
        p.in = accp0; p.out = state;
        k_perm(p, c->w->stream);
        p.in = accp1; p.out = state + ln;
        k_perm(p, c->w->stream);
    }
    op_ntt(c, state, B * 2 * L, 0, L, true);
    return HHE_OK;
}

// Shared first layer, once per transciphering call on lane 0 before the chunks fork: the rotation chain of layer 0 on the ONE key
// ciphertext and, per block of S steps, the diagonal sums of all B items into `out` (which nothing else touches before a chunk's
// last kernel: the call's output, or its keystream table when items share counters).  The operand table is a workspace of the context: S = 128 states when 128 * 3 * L * N words fit the budget.
int shared_l0_chain(hhe_ctx *c, const u64 *enc_key, const u64 *const *h_pdiag_ptrs, size_t B, u64 *out)
{
    Lane &main = c->lanes[0];
    c->w = &main;
    int rc = lane_reserve(c, main, 1);
    if (rc) return rc;
    const size_t ln = (size_t)c->L * c->n;
    const size_t S = std::max<size_t>(2, std::min<size_t>(PASTA_T, c->l0_budget / (3 * ln * 8)));
    if (c->l0_tab.cap > S * 3 * ln) { sync_ctx(c); c->l0_tab.release(); }  // the table holds exactly S steps (hhe_ctx::l0_steps)
    if ((rc = c->l0_tab.reserve(c, S * 3 * ln, "shared first layer: operand table"))) return rc;
    if ((rc = c->l0_ptrs.reserve(c, B, "shared first layer: pointer table"))) return rc;
    rt_h2d(c->l0_ptrs.p, h_pdiag_ptrs, B * sizeof(u64 *), main.stream);  // the caller's array outlives the call's final sync
    rt_d2d(main.ws_ct[0], enc_key, c->ct_words() * 8, main.stream);
    L0Capture cap;
    cap.c0 = c->l0_tab.p; cap.r0 = cap.c0 + S * ln; cap.d = cap.r0 + S * ln; cap.S = (int)S; cap.out = out; cap.B = B;
    return matmul_diagonal_fused(c, pasta_sched(c, 0), c->l0_ptrs.p, 1, &cap);
}
// ... and per chunk: the sums go back to the unrotated frame and to coefficient form, as at the end of matmul_diagonal_fused
void shared_l0_tail(hhe_ctx *c, const u64 *sums, size_t B)
{
    const int L = c->L;
    const size_t ln = (size_t)L * c->n;
    u64 *state = c->w->ws_ct[0];
    PermArgs p = perm_args(c, B * L, sums, state, 2 * ln);
    p.in_item_stride = 2 * ln; p.elt = galois_einv(c, galois_elt_from_step(c, -1));
    k_perm(p, c->w->stream);
    p.in = sums + ln; p.out = state + ln;
    k_perm(p, c->w->stream);
    op_ntt(c, state, B * 2 * L, 0, L, true);
}

// ------------------------------------------------------------------ chunk scheduler of the batched calls
// Every batched call -- hhe_pasta3_transcipher, hhe_packed_affine, and through run_chunks_checked hhe_fc_row, hhe_rotate_rows_many_ks,
// the packed encrypted layers and hhe_mlp_ks -- cuts its batch into independent chunks of `per` items (the last one may be
// shorter): a chunk's working set stays cache resident, and chunks on concurrent streams de-phase the load / butterfly / store phases
// of the transforms.  Chunk idx runs on internal lane 1 + idx % ns; with ns = 0 every chunk runs on the main lane, in order.
struct ChunkPlan {
    size_t B = 0, per = 0, nch = 0;
    int ns = 0;  // internal lanes that receive a chunk
    ChunkPlan(size_t B_, size_t per_, int streams) : B(B_), per(per_), nch((B_ + per_ - 1) / per_), ns((int)std::min<size_t>(streams, nch)) {}
    int first_lane() const { return ns ? 1 : 0; }  // the lanes to reserve for `per` items before anything is enqueued:
    int last_lane() const { return ns; }           // [first_lane(), last_lane()]
    size_t count(size_t idx) const { return std::min(per, B - idx * per); }
};
// transciphering and the affine layer: as many chunks as HHE_CHUNK demands, rounded up to a multiple of the stream count, balanced
ChunkPlan plan_balanced(const hhe_ctx *c, size_t B)
{
    const int ns = c->nstreams;
    if (ns == 0) return ChunkPlan(B, B, 0);
    size_t nch = (B + c->chunk - 1) / c->chunk;
    if (nch > 1) nch = (nch + ns - 1) / ns * ns;
    return ChunkPlan(B, (B + nch - 1) / nch, ns);
}
// chunk(lane, idx, b0, count) enqueues items [b0, b0 + count) on `lane` (= *c->w while it runs).  The internal lanes fork from the
// main stream and join it again, whatever the chunks returned; no chunk is issued after the first error.  The caller syncs.
int run_chunks(hhe_ctx *c, const ChunkPlan &pl, const std::function<int(Lane &, size_t, size_t, size_t)> &chunk)
{
    Lane &main = c->lanes[0];
    if (pl.ns) rt_event_record(c->ev_fork, main.stream);
    for (int s = 1; s <= pl.ns; ++s) rt_stream_wait_event(c->lanes[s].stream, c->ev_fork);
    int rc = HHE_OK;
    for (size_t idx = 0; idx < pl.nch && !rc; ++idx) {
        c->w = &c->lanes[pl.ns ? 1 + idx % pl.ns : 0];
        rc = chunk(*c->w, idx, idx * pl.per, pl.count(idx));
    }
    for (int s = 1; s <= pl.ns; ++s) {
        rt_event_record(c->lanes[s].ev_done, c->lanes[s].stream);
        rt_stream_wait_event(main.stream, c->lanes[s].ev_done);
    }
    c->w = &main;
    return rc;
}
// A call whose result may alias its input (`in == out`, `item_words` words per item): a recomputed chunk would read its own result, so
// run_chunks_checked parks the results in c->d_blocks (reserved under `what`) and copies them out after the recomputations.  The
// chunks write to `res`, which the runner sets
struct Parked {
    const u64 *in; u64 *out; size_t item_words; const char *what;
    u64 *res;
};
// The whole of a call that has an optimistic form, exact unless a digit load meets a zero residue, and an exact one (DESIGN.md
// section 1, "Checked chunks").  reserve(lane, fast) reserves a lane for a chunk of pl.per items; chunk(lane, idx, b0, count, fast)
// enqueues one, as for run_chunks.  fast: every chunk runs in the optimistic form with lane.zero_flag on a flag of its own; the flags
// are read back after the join, and every chunk whose flag is up (every chunk with force_exact) counts in `fallbacks` and is
// recomputed in the exact form on the main lane -- which is reserved for that form only then: everything has completed.
// !fast: the chunks run in the exact form, no flag is made or read.  Ends with the call's final wait; `who` names the call in a
// device failure, `flags_what` its flags in an allocation failure.
int run_chunks_checked(hhe_ctx *c, const ChunkPlan &pl, const char *who, const char *flags_what, bool fast, bool force_exact, u64 &fallbacks,
                       const std::function<int(Lane &, bool)> &reserve,
                       const std::function<int(Lane &, size_t, size_t, size_t, bool)> &chunk, Parked *park = nullptr)
{
    Lane &main = c->lanes[0];
    int rc;
    for (int s = pl.first_lane(); s <= pl.last_lane(); ++s)
        if ((rc = reserve(c->lanes[s], fast))) return rc;
    const bool parked = fast && park && park->in == park->out;
    if (park) park->res = park->out;
    if (parked) {
        if ((rc = c->d_blocks.reserve(c, pl.B * park->item_words, park->what))) return rc;
        park->res = c->d_blocks.p;
    }
    u32 *flags = nullptr;
    if (fast) {
        if ((rc = c->d_flags.reserve(c, pl.nch, flags_what))) return rc;  // one flag per chunk
        flags = c->d_flags.p;
        rt_memset(flags, 0, pl.nch * 4, main.stream);
    }
    rc = run_chunks(c, pl, [&](Lane &ln, size_t idx, size_t b0, size_t bc) {
        ln.zero_flag = fast ? flags + idx : nullptr;
        return chunk(ln, idx, b0, bc, fast);
    });
    if (fast && !rc) {
        std::vector<u32> h(pl.nch, 0);
        if (rt_d2h(h.data(), flags, pl.nch * 4, main.stream) || rt_sync(main.stream)) rc = dev_fail(who);
        for (size_t idx = 0; idx < pl.nch && !rc; ++idx)
            if (h[idx] || force_exact) {
                fallbacks++;
                main.zero_flag = nullptr;
                if (!(rc = reserve(main, false))) rc = chunk(main, idx, idx * pl.per, pl.count(idx), false);
            }
        if (!rc && parked) rt_d2d(park->out, park->res, pl.B * park->item_words * 8, main.stream);
    }
    if (rt_sync(main.stream) && !rc) rc = dev_fail(who);
    return rc;
}
// the tail of the *_galois_steps entry points: the count always, the steps when they fit
int steps_out_copy(const char *who, const std::vector<int> &steps, int *steps_out, size_t *count)
{
    const size_t cap = *count;
    *count = steps.size();
    if (!steps_out || cap < steps.size()) return fail(HHE_ERR_CAPACITY, std::string(who) + ": output too small");
    std::copy(steps.begin(), steps.end(), steps_out);
    return HHE_OK;
}

}  // namespace

// ====================================================================== C ABI
extern "C" int hhe_ntt(hhe_ctx *c, uint64_t *polys, size_t count, int mod_base, int mod_cycle, int inverse)
{
    HHE_LOCK(c);
    if (!c || !polys || mod_cycle < 1 || mod_base < 0 || mod_base + mod_cycle > c->nmod) return fail(HHE_ERR_INVALID, "hhe_ntt: bad arguments");
    op_ntt(c, polys, count, mod_base, mod_cycle, inverse != 0);
    return HHE_OK;
}
extern "C" int hhe_encode(hhe_ctx *c, const uint64_t *vals, size_t B, size_t count, uint64_t *plain)
{
    HHE_LOCK(c);
    if (!c || !vals || !plain || count > c->n) return fail(HHE_ERR_INVALID, "hhe_encode: bad arguments");
    op_encode(c, vals, B, (int)count, (int)count, -1, plain);
    return HHE_OK;
}
extern "C" int hhe_add(hhe_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t B, int size)
{
    HHE_LOCK(c);
    if (!c || !a || !b || !out) return fail(HHE_ERR_INVALID, "hhe_add: bad arguments");
    op_add(c, a, b, out, B, size);
    return HHE_OK;
}
extern "C" int hhe_negate(hhe_ctx *c, const uint64_t *a, uint64_t *out, size_t B, int size)
{
    HHE_LOCK(c);
    if (!c || !a || !out) return fail(HHE_ERR_INVALID, "hhe_negate: bad arguments");
    op_elt(c, ELT_NEG, a, nullptr, out, B * size * c->L, 0, c->L);
    return HHE_OK;
}
// Evaluator::mod_switch_to_inplace on coefficient-form ciphertexts: one launch per chunk of items, every word read and written once
extern "C" int hhe_mod_switch(hhe_ctx *c, const uint64_t *ct, int size, size_t B, int limbs_in, int limbs_out, uint64_t *out)
{
    HHE_LOCK(c);
    if (!c || !ct || !out || B == 0) return fail(HHE_ERR_INVALID, "hhe_mod_switch: bad arguments");
    if (size < 2 || size > 3) return fail(HHE_ERR_INVALID, "hhe_mod_switch: ciphertext size must be 2 or 3");
    if (limbs_out < 1 || limbs_out > limbs_in || limbs_in > c->L)
        return fail(HHE_ERR_INVALID, "hhe_mod_switch: need 1 <= limbs_out <= limbs_in <= L (a ciphertext cannot be switched to a higher level)");
    const size_t n = c->n, in_item = (size_t)size * limbs_in * n, out_item = (size_t)size * limbs_out * n;
    if (B > ((size_t)1 << 40) / in_item) return fail(HHE_ERR_INVALID, "hhe_mod_switch: batch too large");
    if ((uintptr_t)ct < (uintptr_t)(out + B * out_item) && (uintptr_t)out < (uintptr_t)(ct + B * in_item))
        return fail(HHE_ERR_INVALID, "hhe_mod_switch: out overlaps ct");
    c->w = &c->lanes[0];
    // a chunk: as many items as one grid of 2^30 lanes covers (N = 16384, size 2: 32768 items)
    const size_t per = std::max<size_t>(1, (((size_t)1 << 30) >> c->logn) / size);
    for (size_t b0 = 0; b0 < B; b0 += per) {
        const size_t bc = std::min(per, B - b0);
        k_elt(elt_args(c, ct + b0 * in_item, c->d_moddown, out + b0 * out_item, bc * size, 0, limbs_in, limbs_out), ELT_MODDOWN, c->w->stream);
        ++c->mod_switch_launches;
    }
    if (rt_sync(c->w->stream)) return dev_fail("hhe_mod_switch");
    return HHE_OK;
}
// The key sets of a level (hhe_ctx_create_level) from resident sets higher up the chain: the key-switch key of the level with l data
// primes is digits I < l and limbs {0 .. l-1, special} of the parent's -- digit I carries q_sp s' in limb I only, whatever L is -- so
// one gather launch per key makes it, on the device.  Every new buffer is complete before anything of dst is replaced.
extern "C" int hhe_keyset_derive_level(hhe_keyset *dst, const hhe_keyset *src)
{
    if (!dst || !src) return fail(HHE_ERR_INVALID, "hhe_keyset_derive_level: null argument");
    hhe_ctx *cd = dst->ctx, *cs = src->ctx;
    // both contexts, the one with more data limbs first (equal: by address); L never changes after creation
    hhe_ctx *first = cs, *second = cd;
    if (cd->L > cs->L || (cd->L == cs->L && std::less<hhe_ctx *>()(cd, cs))) std::swap(first, second);
    CtxLock lock1(first), lock2(second == first ? nullptr : second);
    const int l = cd->L;
    bool ok = dst != src && cd->logn == cs->logn && cd->t == cs->t && cd->device == cs->device && l <= cs->L && cd->q[l] == cs->q[cs->L];
    for (int j = 0; ok && j < l; ++j) ok = cd->q[j] == cs->q[j];
    if (!ok)
        return fail(HHE_ERR_INVALID, "hhe_keyset_derive_level: dst is not a level of src's chain (same N, t, device and special prime, data primes a prefix)");
    rt_stream st = cd->lanes[0].stream;
    u64 *rk = nullptr;
    std::vector<std::pair<u32, u64 *>> gk;
    auto drop = [&]() { rt_free(rk); for (auto &kv : gk) rt_free(kv.second); };
    auto project = [&](const u64 *key) -> u64 * {
        u64 *out = (u64 *)rt_malloc(cd->ksk_words() * 8);
        if (!out) return nullptr;
        k_elt(elt_args(cd, key, nullptr, out, (size_t)l * 2 * cd->K, 0, cd->K, cs->K), ELT_KEYPROJ, st);
        ++cd->key_proj_launches;
        return out;
    };
    if (src->rk && !(rk = project(src->rk))) { rt_sync(st); drop(); return dev_fail("hhe_keyset_derive_level"); }
    for (auto &kv : src->gk) {
        u64 *key = project(kv.second);
        if (!key) { rt_sync(st); drop(); return dev_fail("hhe_keyset_derive_level"); }
        gk.emplace_back(kv.first, key);
    }
    if (rt_sync(st)) { drop(); return dev_fail("hhe_keyset_derive_level"); }
    sync_ctx(cd);  // a key of dst may still be read by work in flight on any lane
    keyset_clear(dst);  // a new serial; the tables derived from the replaced keys go with them
    dst->rk = rk;
    for (auto &kv : gk) dst->gk[kv.first] = kv.second;
    return HHE_OK;
}
extern "C" int hhe_add_plain(hhe_ctx *c, const uint64_t *ct, const uint64_t *plain, int bcast, int subtract, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || !ct || !plain || !out) return fail(HHE_ERR_INVALID, "hhe_add_plain: bad arguments");
    op_add_plain(c, ct, plain, nullptr, 0, bcast != 0, subtract != 0, false, out, B);
    return HHE_OK;
}
extern "C" int hhe_multiply_plain(hhe_ctx *c, const uint64_t *ct, const uint64_t *plain, int bcast, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || !ct || !plain || !out) return fail(HHE_ERR_INVALID, "hhe_multiply_plain: bad arguments");
    int rc = need(c, B);
    if (rc) return rc;
    const size_t P = bcast ? 1 : B;
    u64 *D = c->w->ws_ct3;  // [P][L][N] fits in [B][3][L][N]
    op_lift_ntt(c, plain, P, D);
    if (bcast) op_multiply_plain_ntt(c, ct, D, nullptr, 0, out, B);
    else {
        // per-item multiplier: items laid [B][L][N]; the pointer form of the fused store reads the lane's pointer table
        Lane &ln = *c->w;
        stage_begin(ln);
        ln.h_ptrs.assign(B, nullptr);
        for (size_t b = 0; b < B; ++b) ln.h_ptrs[b] = D + b * c->L * c->n;
        rt_h2d(ln.d_ptrs, ln.h_ptrs.data(), B * sizeof(u64 *), ln.stream);
        stage_end(ln);
        NttArgs a = ntt_args(c, ct, out, B * 2 * c->L, 0, c->L);
        a.store_op = STORE_MUL; a.mul_ptrs = ln.d_ptrs; a.mul_cycle = c->L; a.mul_item_polys = 2 * c->L;
        k_ntt(a, false, ln.stream);
        op_ntt(c, out, B * 2 * c->L, 0, c->L, true);
    }
    return HHE_OK;
}
// a key set handed to an entry point must belong to the context it is used with
static int check_sets(const hhe_ctx *c, const hhe_keyset *a, const hhe_keyset *b = nullptr, const hhe_keyset *d = nullptr)
{
    for (const hhe_keyset *ks : {a, b, d})
        if (ks && ks->ctx != c) return fail(HHE_ERR_INVALID, "key set belongs to another context");
    return HHE_OK;
}
// the prologue the _ks entry points of the key-switching ops share -- lock, workspace, ownership of the named set, null check, key
// scope -- then the op
template <class Op> static int ks_entry(hhe_ctx *c, size_t B, const hhe_keyset *gk, const hhe_keyset *rk, bool args_ok, const char *null_msg, Op op)
{
    HHE_LOCK(c);
    int rc = need(c, B);
    if (rc || (rc = check_sets(c, gk, rk))) return rc;
    if (!args_ok) return fail(HHE_ERR_INVALID, null_msg);
    KeyScope keys(c, gk, rk);
    return op();
}
extern "C" int hhe_apply_galois_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *ct, uint32_t elt, uint64_t *out, size_t B)
{
    return ks_entry(c, B, gk, nullptr, ct && out, "hhe_apply_galois: null argument", [&] { return op_apply_galois(c, ct, elt, out, B); });
}
extern "C" int hhe_apply_galois(hhe_ctx *c, const uint64_t *ct, uint32_t elt, uint64_t *out, size_t B) { return hhe_apply_galois_ks(c, nullptr, ct, elt, out, B); }
extern "C" int hhe_rotate_rows_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *ct, int step, uint64_t *out, size_t B)
{
    return ks_entry(c, B, gk, nullptr, ct && out, "hhe_rotate_rows: null argument", [&] { return op_rotate_rows(c, ct, step, out, B); });
}
extern "C" int hhe_rotate_rows(hhe_ctx *c, const uint64_t *ct, int step, uint64_t *out, size_t B) { return hhe_rotate_rows_ks(c, nullptr, ct, step, out, B); }
extern "C" int hhe_rotate_columns_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *ct, uint64_t *out, size_t B)
{
    return ks_entry(c, B, gk, nullptr, ct && out, "hhe_rotate_columns: null argument", [&] { return op_apply_galois(c, ct, (u32)(2 * c->n - 1), out, B); });
}
extern "C" int hhe_rotate_columns(hhe_ctx *c, const uint64_t *ct, uint64_t *out, size_t B) { return hhe_rotate_columns_ks(c, nullptr, ct, out, B); }
extern "C" int hhe_multiply(hhe_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out3, size_t B)
{
    HHE_LOCK(c);
    int rc = need(c, B);
    if (rc) return rc;
    op_multiply(c, a, b, out3, B);
    return HHE_OK;
}
extern "C" int hhe_square(hhe_ctx *c, const uint64_t *a, uint64_t *out3, size_t B)
{
    HHE_LOCK(c);
    int rc = need(c, B);
    if (rc) return rc;
    op_square(c, a, out3, B);
    return HHE_OK;
}
// the definition and the cap are in include/hhe_gfx950.h; DESIGN.md section 4 "One floor over a sum of products"
extern "C" int hhe_multiply_sum(hhe_ctx *c, const uint64_t *a, const uint64_t *b, size_t K, int b_bcast, uint64_t *out3, size_t B)
{
    HHE_LOCK(c);
    if (!c || !a || !b || !out3 || K == 0 || B == 0) return fail(HHE_ERR_INVALID, "hhe_multiply_sum: null argument, no addend or empty batch");
    if (K >= 2 && K > c->behz_sum_cap) return fail(HHE_ERR_INVALID, "hhe_multiply_sum: more addends than one floor takes (behz_sum_cap)");
    if (K > 0x7fffffff / B || K * B > ((size_t)0x7fffffff >> c->logn) / (2 * (c->L + 1))) return fail(HHE_ERR_INVALID, "hhe_multiply_sum: batch too large");
    const size_t ctw = c->ct_words(), nb = b_bcast ? K : K * B;
    auto overlaps = [&](const u64 *p, size_t words) { return out3 < p + words && p < out3 + B * 3 * c->L * c->n; };
    if (overlaps(a, K * B * ctw) || overlaps(b, nb * ctw)) return fail(HHE_ERR_INVALID, "hhe_multiply_sum: out3 overlaps an operand");
    int rc = need(c, K * B);
    if (rc) return rc;
    op_behz_operand(c, a, c->w->bz_aq, c->w->bz_ab, K * B);
    op_behz_operand(c, b, c->w->bz_bq, c->w->bz_bb, nb);
    behz_product(c, c->w->bz_bq, c->w->bz_bb, b_bcast ? 1 : 0, out3, B, K);
    return HHE_OK;
}
extern "C" int hhe_relinearize_ks(hhe_ctx *c, const hhe_keyset *rk, const uint64_t *a3, uint64_t *out, size_t B)
{
    return ks_entry(c, B, nullptr, rk, a3 && out, "hhe_relinearize: null argument", [&] { return op_relinearize(c, a3, out, B); });
}
extern "C" int hhe_relinearize(hhe_ctx *c, const uint64_t *a3, uint64_t *out, size_t B) { return hhe_relinearize_ks(c, nullptr, a3, out, B); }
extern "C" int hhe_relinearize_slot(hhe_ctx *c, int slot, const uint64_t *a3, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || slot < 0 || slot >= HHE_RELIN_SLOTS) return fail(HHE_ERR_INVALID, "hhe_relinearize_slot: bad arguments");
    KeyScope keys(c, nullptr, c->relin_set(slot));
    if (!c->rks->rk) return fail(HHE_ERR_NO_RELIN_KEY, "relinearization key not set");
    int rc = need(c, B);
    if (rc) return rc;
    return op_relinearize(c, a3, out, B);
}

// one chunk of the batch on the current lane (c->w): the schedule of PASTA_SEAL::decomposition (pasta_3_seal.cpp:123-170)
// shared_l0: `out` holds the items' first-layer sums (shared_l0_chain)
// cw_padded_host null: the keystream only -- the chunk stops before res = Enc(c_b) - KS and its last addition leaves the state in `out`
// (else the items' words, zero padded, in the context's host staging)
static int transcipher_chunk(hhe_ctx *c, const u64 *enc_key, const u64 *const *d_diag, const u64 *const *d_rc,
                             const u64 *cw_padded_host, u64 *out, size_t B, bool bsgs, bool shared_l0)
{
    const size_t n = c->n;
    const int L = c->L;
    const bool fused = c->matmul_mode == 1;
    int rc = HHE_OK;
    if (cw_padded_host) rt_h2d(c->w->ws_vals, cw_padded_host, B * PASTA_T * 8, c->w->stream);
    u64 *state = c->w->ws_ct[0], *tmp = c->w->ws_ct[1], *t3 = c->w->ws_ct3;
    // state <- enc_ssk[0] for every item (pasta_3_seal.cpp:126)
    if (!shared_l0) op_elt(c, ELT_BCAST, nullptr, enc_key, state, B * 2 * L, 0, L, 2 * L);
    for (int r = 0; r <= PASTA_R && !rc; ++r) {
        if (r == 0 && shared_l0) shared_l0_tail(c, out, B);
        else if ((rc = bsgs ? matmul_bsgs(c, r, d_diag, B) : fused ? matmul_diagonal_fused(c, pasta_sched(c, r), d_diag, B) : matmul_diagonal(c, r, d_diag, B))) break;
        // add_rc (:205-211)
        op_add_plain(c, state, nullptr, d_rc, (size_t)r * n, false, false, false, state, B);
        // mix (:417-423)
        if ((rc = op_apply_galois(c, state, (u32)(2 * n - 1), tmp, B))) break;
        op_add(c, tmp, state, tmp, B, 2);
        op_add(c, state, tmp, r == PASTA_R && !cw_padded_host ? out : state, B, 2);
        if (r == PASTA_R) break;
        if (r == PASTA_R - 1) {
            // sbox_cube (:215-218): exponentiate_inplace(x,3) == relin(mul(relin(mul(x,x)), x))
            op_multiply(c, state, state, t3, B);
            if ((rc = op_relinearize(c, t3, tmp, B))) break;
            op_multiply(c, tmp, state, t3, B);
            if ((rc = op_relinearize(c, t3, state, B))) break;
        } else {
            // sbox_feistel (:222-247)
            if ((rc = op_rotate_rows(c, state, -1, tmp, B))) break;
            op_multiply_plain_ntt(c, tmp, c->d_feistel_mask, nullptr, 0, tmp, B);
            op_multiply(c, tmp, tmp, t3, B);
            if ((rc = op_relinearize(c, t3, tmp, B))) break;
            op_add(c, state, tmp, state, B, 2);
        }
    }
    if (!rc && cw_padded_host) {
        // res = Enc(c_b) - KS : encode, negate, add_plain (:161-169)
        op_finish_front(c, c->w->ws_vals, c->w->ws_plain, B);
        op_finish_back(c, c->w->ws_plain, state, nullptr, nullptr, out, B);
    }
    return rc;
}

// Keystream cache, lookup side: which resident snapshot holds the words of enc_key.  The comparison runs on the main lane's stream --
// the caller's, so it is ordered behind whatever produced enc_key -- word for word against every snapshot: a launch raises its flag
// where a word differs.  ks_match_enqueue enqueues the clear, the launches, the read-back into the context's page-locked staging and
// an event; the caller goes on preparing and enqueueing what does not depend on the answer, and ks_match_resolve waits for the event
// (*snap = the snapshot's number, 0: none).
static int ks_match_enqueue(hhe_ctx *c, const u64 *enc_key)
{
    KsCache &kc = c->ks_cache;
    const size_t ns = kc.snaps.size();
    if (!ns) return HHE_OK;
    int rc = c->ks_flags.reserve(c, KsCache::MAX_SNAPSHOTS, "transciphering: key comparison");
    if (rc) return rc;
    c->w = &c->lanes[0];  // op_elt launches on the current lane: the main one, like the clear and the read around it
    rt_stream st = c->w->stream;
    u64 *flags = c->ks_flags.p;
    rt_memset(flags, 0, ns * 8, st);
    for (size_t i = 0; i < ns; ++i) op_elt(c, ELT_DIFF, enc_key, kc.snaps[i].words, flags + i, (size_t)2 * c->L, 0, c->L);
    if (rt_d2h(c->fin_host.p, flags, ns * 8, st) || rt_event_record(c->ev_cmp, st)) return dev_fail("hhe_pasta3_transcipher: key comparison");
    return HHE_OK;
}
static int ks_match_resolve(hhe_ctx *c, u64 *snap)
{
    KsCache &kc = c->ks_cache;
    *snap = 0;
    const size_t ns = kc.snaps.size();
    if (!ns) return HHE_OK;
    if (rt_event_sync(c->ev_cmp)) return dev_fail("hhe_pasta3_transcipher: key comparison");
    const u64 *h = c->fin_host.p;
    for (size_t i = 0; i < ns && !*snap; ++i)
        if (!h[i]) { *snap = kc.snaps[i].id; kc.snaps[i].last_use = c->block_call; }
    return HHE_OK;
}
// ... insertion side: the device copies a call has made for the cache and not handed over yet.  They are handed over after the call's
// final wait has succeeded (commit); on every other path they are freed when the call returns, which is after that wait as well
struct KsPending {
    u64 *snap = nullptr;                       // copy of enc_key (no resident snapshot equals it)
    std::vector<std::pair<PastaPair, u64 *>> cts;    // (pair, copy of its new keystream)
    ~KsPending()
    {
        rt_free(snap);
        for (auto &p : cts) rt_free(p.second);
    }
    void commit(hhe_ctx *c, KsCache::Entry key)
    {
        KsCache &kc = c->ks_cache;
        if (cts.empty()) return;
        if (snap) { key.snap = kc.add_snapshot(c, snap, c->block_call); snap = nullptr; }
        for (auto &p : cts)
            if (c->blocks.count(p.first)) { key.ct = p.second; kc.insert(c, p.first, key); }  // insert takes the copy either way
            else rt_free(p.second);
        cts.clear();
    }
};
// Every upload into the table part of fin_dev (the pointer tables of the fused finishing pass, the u32 map of the unfused one), on
// the main stream.  The context keeps the bytes of the last one (fin_tab_shadow); a table of the same length and bytes is what the
// device holds -- or will hold when anything enqueued after this call runs -- and is not sent again.  A table equal to the
// device's is right whatever lives at its addresses: the kernels would read the same pointers either way.
static int fin_tab_upload(hhe_ctx *c, const u64 *h_tab, size_t bytes)
{
    std::vector<unsigned char> &sh = c->fin_tab_shadow;
    if (sh.size() == bytes && !memcmp(sh.data(), h_tab, bytes)) return HHE_OK;
    sh.clear();
    if (rt_h2d(c->fin_dev.p, h_tab, bytes, c->lanes[0].stream)) return dev_fail("hhe_pasta3_transcipher: table upload");
    sh.assign((const unsigned char *)h_tab, (const unsigned char *)h_tab + bytes);
    ++c->fin_tab_uploads;
    return HHE_OK;
}

// hhe_pasta3_transcipher with the key objects already named (c->rks / c->gks)
// Everything before res = Enc(c_b) - KS is a function of the key ciphertext, the named key sets and the item's block counter only, so
// items of one call with the same counter share one keystream ciphertext, word for word (HHE_DEDUP, DESIGN.md "one keystream per
// counter").  Such a call runs in two phases: the chunk schedule over its distinct counters, which leaves the keystreams in ks_tab,
// then a finishing pass over all B items (op_finish_front / op_finish_back).
// The keystreams are kept from call to call (KsCache, DESIGN.md "one keystream per key"): every call then takes the two-phase shape and
// phase 1 runs over the counters no kept keystream was found for.  The fused finishing pass reads every item's keystream where it is,
// through a table of B pointers: a kept one in the cache (entries only go in commit, after the final wait, under the context's lock),
// an evaluated one in ks_tab.  The unfused one reads ks_tab through a map: the M evaluated counters first, in order of first
// appearance, then copies of the kept ones.
// Order of a call: the key comparison is enqueued first and the host does not wait for it until it has prepared the call and
// enqueued the half of the finishing pass that does not depend on the keystreams (upload of the words, first pass).  A call that
// may take the item kernel on a prediction (2b) prepares first and enqueues that kernel IN FRONT of the comparison: the kernel
// reads no word of enc_key, so it starts while the runtime calls of the comparison are still being issued, and the comparison,
// its event and ks_match_resolve mean what they mean elsewhere.  Such a call learns that it was refuted one kernel later.
// What a steady call sends to the device: the item kernel reads the words where they are staged (page-locked staging), and a
// table the device already holds is not uploaded again (fin_tab_upload) -- nothing, when the same counters come back.
// Without the cache (HHE_KS_CACHE=0, or a profiled call) a call of distinct counters (U == B) runs as one phase, with no table and no map.
// transcipher_enqueue returns after enqueueing; whatever it returns, its caller waits for the main stream before anything it staged goes.
static int transcipher_enqueue(hhe_ctx *c, const uint64_t *enc_key, const uint64_t *cw, const uint32_t *ncw,
                               const PastaPair *block_index, size_t B, int use_bsgs, uint64_t *out, KsPending &pend, KsCache::Entry &kkey)
{
    const size_t n = c->n, ctw = c->ct_words();
    Lane &main = c->lanes[0];
    int rc;
    if ((rc = fin_reserve(c, B))) return rc;  // before anything reads the staging: growth replaces it
    if (c->fin_tab_items != B) {  // the words and the intermediate of this call lie where the table of another item count was
        c->fin_tab_shadow.clear();
        c->fin_tab_items = B;
    }
    const bool cache = c->dedup && c->ks_cache.enabled && !c->profile;
    const bool item = c->dedup && fin_item_for(c, B);  // the finishing pass of a two-phase call is one launch, one workgroup per item
    // 1. the key comparison.  Where the item kernel may be enqueued on a prediction (2b) the comparison goes right behind it.  Not
    // where `out` overlaps the key ciphertext: every other path has read the key before it writes a result
    const bool apart = (uintptr_t)(enc_key + ctw) <= (uintptr_t)out || (uintptr_t)(out + B * ctw) <= (uintptr_t)enc_key;
    const bool may_predict = cache && item && apart && !c->ks_cache.snaps.empty();
    if (cache && !may_predict && (rc = ks_match_enqueue(c, enc_key))) return rc;
    // 2. host preparation.  The distinct counters in order of first appearance; umap[b]: where item b's counter stands among them
    std::vector<PastaPair> uniq;
    std::vector<u32> umap;
    if (c->dedup) {
        std::map<PastaPair, u32> seen;
        umap.resize(B);
        for (size_t b = 0; b < B; ++b) {
            if (b && block_index[b] == block_index[b - 1]) { umap[b] = umap[b - 1]; continue; }  // a run of one pair: no lookup
            auto ins = seen.emplace(block_index[b], (u32)uniq.size());
            if (ins.second) uniq.push_back(block_index[b]);
            umap[b] = ins.first->second;
        }
    }
    const bool dedup = c->dedup && (cache || uniq.size() < B);
    const size_t U = dedup ? uniq.size() : B;  // keystreams the call needs
    const PastaPair *counters = dedup ? uniq.data() : block_index;
    c->last_unique = c->last_evaluated = U;
    // staging: [MAX_SNAPSHOTS] flags | [B] pointers or map | [B][128] words.  Every word of the last part is written: nothing of an earlier call stays
    u64 *const h_tab = c->fin_host.p + KsCache::MAX_SNAPSHOTS, *const h_words = h_tab + fin_tab_words(B);
    u64 *const d_tab = c->fin_dev.p, *const d_words = d_tab + fin_tab_words(B), *const d_tmp = d_words + B * PASTA_T;
    // The item kernel reads an item's 128 words once (fin_item_encode): out of page-locked staging it reads them where they are, and
    // they are not uploaded.  The staging is not rewritten before the final wait of the call, which every path ends in.  The table is
    // reloaded in every phase of the kernel and stays in device memory
    const bool words_in_place = item && c->fin_host.pinned;
    const u64 *const item_words = words_in_place ? h_words : d_words;
    auto upload_words = [&] {
        rt_h2d(d_words, h_words, B * PASTA_T * 8, main.stream);
        ++c->fin_word_uploads;
    };
    for (size_t b = 0; b < B; ++b) {
        memcpy(h_words + b * PASTA_T, cw + b * PASTA_T, ncw[b] * 8);
        memset(h_words + b * PASTA_T + ncw[b], 0, (PASTA_T - ncw[b]) * 8);
    }
    // public tables of every counter of the call (pinned for its duration), kept keystreams or not
    std::vector<BlockTables *> tabs(U);
    if ((rc = ensure_blocks(c, counters, U, use_bsgs, tabs.data()))) return rc;
    // 2b. The item kernel has no half that runs ahead of the keystreams, so nothing would hide the wait for the comparison: predict
    // its answer -- the snapshot used last -- and, if every counter of the call has a kept keystream under it, enqueue the whole
    // finishing pass, then the comparison behind it, before waiting.  The probe touches no stamp.  A call the flags do not confirm
    // goes on as it would have without the prediction and finishes over `out` again, behind the stale launch on the same stream; what
    // that launch read are cache entries, which go only behind a wait for the context's streams.
    u64 predicted = 0;
    if (may_predict) {
        const KsCache &kc = c->ks_cache;
        size_t best = 0;
        for (size_t i = 1; i < kc.snaps.size(); ++i)
            if (kc.snaps[i].last_use > kc.snaps[best].last_use) best = i;
        KsCache::Entry probe = kkey;
        probe.snap = kc.snaps[best].id;
        std::vector<const u64 *> kept(U);
        bool all = true;
        for (size_t u = 0; u < U && all; ++u) all = (kept[u] = kc.peek(counters[u], probe)) != nullptr;
        if (all) {
            for (size_t b = 0; b < B; ++b) h_tab[b] = (u64)kept[umap[b]];
            if ((rc = fin_tab_upload(c, h_tab, B * sizeof(u64)))) return rc;
            if (!words_in_place) upload_words();
            c->w = &main;
            op_finish_item(c, item_words, d_tmp, nullptr, (const u64 *const *)d_tab, out, B);
            predicted = probe.snap;
        }
        if ((rc = ks_match_enqueue(c, enc_key))) return rc;
    }
    // 3. the half of the finishing pass that does not depend on the keystreams
    const ChunkPlan fin = item ? ChunkPlan(B, B, 0) : plan_balanced(c, B);  // the item kernel takes the batch whole
    if (dedup && !predicted) {
        if (!words_in_place) upload_words();
        if (!item) rc = run_chunks(c, fin, [&](Lane &, size_t, size_t b0, size_t bc) {
            op_finish_front(c, d_words + b0 * PASTA_T, d_tmp + b0 * n, bc);
            return (int)HHE_OK;
        });
        if (rc) return rc;
    }
    // 4. kept keystreams: found[u], or null = counter u is evaluated
    std::vector<const u64 *> found(U, nullptr);
    if (cache) {
        if ((rc = ks_match_resolve(c, &kkey.snap))) return rc;
        if (kkey.snap)
            for (size_t u = 0; u < U; ++u)
                if ((found[u] = c->ks_cache.find(counters[u], kkey, c->block_call))) ++c->last_hits;
    }
    const size_t M = U - c->last_hits;  // keystream evaluations
    c->last_evaluated = M;
    const bool by_ptr = dedup && fin_fused_on(c);  // the finishing pass reads kept keystreams in place
    std::vector<size_t> eval, slot(U);  // eval[m]: the counter (index u) evaluation m is for; slot[u]: its place in ks_tab
    for (size_t u = 0, h = M; u < U; ++u) {
        if (found[u]) slot[u] = h++;
        else { slot[u] = eval.size(); eval.push_back(u); }
    }
    // per-evaluation public tables
    std::vector<const u64 *> ptrs(2 * M);
    for (size_t m = 0; m < M; ++m) {
        const BlockTables *bt = tabs[eval[m]];
        ptrs[m] = use_bsgs ? bt->bsgs : c->matmul_mode == 1 ? bt->pdiag : bt->diag;
        ptrs[M + m] = bt->rc;
    }
    // fused diagonal method: layer 0 acts on the same ciphertext for every item -- its chain runs once, here (HHE_SHARED_L0)
    const bool shared = c->matmul_mode == 1 && !use_bsgs && c->shared_l0 > 0 && M >= (size_t)c->shared_l0;
    const ChunkPlan plan = plan_balanced(c, std::max<size_t>(M, 1));
    if (M)
        for (int s = plan.first_lane(); s <= plan.last_lane(); ++s) {
            if ((rc = lane_reserve(c, c->lanes[s], plan.per))) return rc;
            if (use_bsgs && (rc = c->lanes[s].ws_rot.reserve(c, plan.per * ROT_SLOTS * ctw, "bsgs workspace"))) return rc;
        }
    if (dedup && (rc = c->ks_tab.reserve(c, (by_ptr ? M : U) * ctw, "transciphering: keystream table"))) return rc;
    u64 *ks = dedup ? c->ks_tab.p : out;  // where an evaluation leaves its result
    // 5. the chain over the counters that are evaluated
    if (cache) {
        if (!by_ptr)
            for (size_t u = 0; u < U; ++u)
                if (found[u]) rt_d2d(ks + slot[u] * ctw, found[u], ctw * 8, main.stream);
        // a copy that cannot be allocated is a keystream that is not kept, nothing more
        if (M && !kkey.snap && (pend.snap = (u64 *)rt_malloc(ctw * 8))) rt_d2d(pend.snap, enc_key, ctw * 8, main.stream);
    }
    if (M && shared) rc = shared_l0_chain(c, enc_key, ptrs.data(), M, ks);
    std::vector<std::vector<const u64 *>> keep(plan.nch);  // per chunk: its pointer table
    if (M && !rc) rc = run_chunks(c, plan, [&](Lane &ln, size_t idx, size_t b0, size_t bc) {
        std::vector<const u64 *> &lp = keep[idx];
        lp.assign(2 * ln.ptr_cap, nullptr);
        for (size_t b = 0; b < bc; ++b) { lp[b] = ptrs[b0 + b]; lp[ln.ptr_cap + b] = ptrs[M + b0 + b]; }
        rt_h2d(ln.d_ptrs, lp.data(), lp.size() * sizeof(u64 *), ln.stream);
        return transcipher_chunk(c, enc_key, ln.d_ptrs, ln.d_ptrs + ln.ptr_cap, dedup ? nullptr : h_words + b0 * PASTA_T, ks + b0 * ctw, bc, use_bsgs != 0, shared);
    });
    if (rc) {  // the pointer tables in `keep` are read by copies in flight
        rt_sync(main.stream);
        return rc;
    }
    if (cache && (kkey.snap || pend.snap))  // the new keystreams, after the join of their chunks on the main stream
        for (size_t m = 0; m < M; ++m)
            if (u64 *copy = (u64 *)rt_malloc(ctw * 8)) {
                rt_d2d(copy, ks + m * ctw, ctw * 8, main.stream);
                pend.cts.emplace_back(counters[eval[m]], copy);
            }
    // 6. res = Enc(c_b) - KS for every item (:161-169), after the join of the keystream chunks on the main stream
    if (predicted && predicted == kkey.snap && !M) {}  // confirmed: the finishing pass is enqueued already
    else if (dedup) {
        if (by_ptr)
            for (size_t b = 0; b < B; ++b) {
                const size_t u = umap[b];
                h_tab[b] = (u64)(found[u] ? found[u] : ks + slot[u] * ctw);
            }
        else
            for (size_t b = 0; b < B; ++b) ((u32 *)h_tab)[b] = (u32)slot[umap[b]];
        if ((rc = fin_tab_upload(c, h_tab, B * (by_ptr ? sizeof(u64) : sizeof(u32))))) {
            rt_sync(main.stream);  // as above
            return rc;
        }
        c->w = &main;
        if (item) op_finish_item(c, item_words, d_tmp, ks, (const u64 *const *)d_tab, out, B);
        else rc = run_chunks(c, fin, [&](Lane &, size_t, size_t b0, size_t bc) {
            op_finish_back(c, d_tmp + b0 * n, ks, by_ptr ? (const u64 *const *)d_tab + b0 : nullptr, by_ptr ? nullptr : (const u32 *)d_tab + b0, out + b0 * ctw, bc);
            return (int)HHE_OK;
        });
    }
    if (rt_sync(main.stream) && !rc) rc = dev_fail("hhe_pasta3_transcipher");  // `keep` and the host vectors above go with this frame
    return rc;
}
// Groups of a call through an entry point that takes nonces: contiguous runs of items whose distinct pairs fit block_cache_limit (at
// least one pair per group), so that an earlier group's tables are evictable when a later one needs room -- an honest stream has a
// fresh pair per block, and the tables of all of them need not fit at once.  ends[g] = one past the last item of group g
static std::vector<size_t> pair_groups(const hhe_ctx *c, const PastaPair *ids, size_t B, int use_bsgs)
{
    const size_t per = block_entry_bytes(c) + (use_bsgs ? block_bsgs_bytes(c) : 0), cap = std::max<size_t>(1, c->block_cache_limit / per);
    std::vector<size_t> ends;
    std::map<PastaPair, bool> in;
    for (size_t b = 0; b < B; ++b) {
        if (!in.count(ids[b]) && in.size() == cap) { ends.push_back(b); in.clear(); }
        in.emplace(ids[b], true);
    }
    ends.push_back(B);
    return ends;
}
// grouped: the call came through an entry point with nonces (pair_groups); else it is one group whatever it needs
static int transcipher_impl(hhe_ctx *c, const uint64_t *enc_key, const uint64_t *cw, const uint32_t *ncw,
                            const PastaPair *ids, size_t B, int use_bsgs, uint64_t *out, bool grouped)
{
    if (!c || !enc_key || !cw || !ncw || !ids || !out || B == 0) return fail(HHE_ERR_INVALID, "hhe_pasta3_transcipher: null argument or empty batch");
    const size_t n = c->n, half = n / 2;
    // pasta_3_seal.cpp:376-377
    if ((size_t)PASTA_T * 2 != n && (size_t)PASTA_T * 4 > n) return fail(HHE_ERR_TOO_FEW_SLOTS, "too little slots for matmul implementation!");
    if (!c->rks->rk) return fail(HHE_ERR_NO_RELIN_KEY, "relinearization key not set");
    for (int step : {-1, half != PASTA_T ? PASTA_T : -1, 0})
        if (!c->gks->gk.count(galois_elt_from_step(c, step))) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
    if (use_bsgs)  // add_gk_indices (:196-200): -k*BSGS_N1, k = 1..7
        for (int k = 1; k < 8; ++k)
            if (!c->gks->gk.count(galois_elt_from_step(c, -16 * k))) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
    for (size_t b = 0; b < B; ++b)
        if (ncw[b] > PASTA_T) return fail(HHE_ERR_INVALID, "hhe_pasta3_transcipher: more than 128 words in a block");
    Lane &main = c->lanes[0];
    c->w = &main;
    int rc;
    if ((rc = ensure_feistel_mask(c))) return rc;
    const std::vector<size_t> ends = grouped ? pair_groups(c, ids, B, use_bsgs) : std::vector<size_t>{B};
    size_t unique = 0, evaluated = 0, hits = 0;
    c->last_public_built = 0;
    for (size_t g = 0, b0 = 0; g < ends.size() && !rc; b0 = ends[g++]) {
        const size_t bc = ends[g] - b0;
        ++c->block_call;
        c->last_hits = 0;
        // from here on work is enqueued that reads host staging and the pending copies: every path ends in the final wait
        KsPending pend;
        KsCache::Entry kkey{nullptr, 0, c->gks->serial, c->rks->serial, use_bsgs != 0, c->block_call};
        rc = transcipher_enqueue(c, enc_key, cw + b0 * PASTA_T, ncw + b0, ids + b0, bc, use_bsgs, out + b0 * c->ct_words(), pend, kkey);
        if (rt_sync(main.stream) && !rc) rc = dev_fail("hhe_pasta3_transcipher");
        if (!rc) pend.commit(c, kkey);  // a failed call leaves nothing behind
        unique += c->last_unique; evaluated += c->last_evaluated; hits += c->last_hits;
    }
    c->last_unique = unique; c->last_evaluated = evaluated; c->last_hits = hits;
    c->last_groups = ends.size();
    return rc;
}
// the items' pairs: (nonce[b], block_index[b]), or the counters under the reference's fixed nonce
static std::vector<PastaPair> pairs_of(const uint64_t *nonce, const uint64_t *block_index, size_t B)
{
    std::vector<PastaPair> ids(block_index ? B : 0);
    for (size_t b = 0; b < ids.size(); ++b) ids[b] = nonce ? PastaPair(nonce[b], block_index[b]) : PastaPair(block_index[b]);
    return ids;
}
extern "C" int hhe_pasta3_transcipher_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const uint64_t *enc_key, const uint64_t *cw,
                                         const uint32_t *ncw, const uint64_t *block_index, size_t B, int use_bsgs, uint64_t *out)
{
    HHE_LOCK(c);
    if (!c) return fail(HHE_ERR_INVALID, "hhe_pasta3_transcipher: null context");
    int rc = check_sets(c, rk, gk);
    if (rc) return rc;
    KeyScope keys(c, gk, rk);
    const std::vector<PastaPair> ids = pairs_of(nullptr, block_index, B);
    return transcipher_impl(c, enc_key, cw, ncw, block_index ? ids.data() : nullptr, B, use_bsgs, out, false);
}
extern "C" int hhe_pasta3_transcipher(hhe_ctx *c, const uint64_t *enc_key, const uint64_t *cw, const uint32_t *ncw,
                                      const uint64_t *block_index, size_t B, int use_bsgs, uint64_t *out)
{
    return hhe_pasta3_transcipher_ks(c, nullptr, nullptr, enc_key, cw, ncw, block_index, B, use_bsgs, out);
}
extern "C" int hhe_pasta3_transcipher_nonce_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const uint64_t *enc_key, const uint64_t *cw,
                                               const uint32_t *ncw, const uint64_t *nonce, const uint64_t *block_index, size_t B, int use_bsgs,
                                               uint64_t *out)
{
    HHE_LOCK(c);
    if (!c) return fail(HHE_ERR_INVALID, "hhe_pasta3_transcipher: null context");
    int rc = check_sets(c, rk, gk);
    if (rc) return rc;
    KeyScope keys(c, gk, rk);
    const bool have = nonce && block_index;
    const std::vector<PastaPair> ids = pairs_of(nonce, have ? block_index : nullptr, B);
    return transcipher_impl(c, enc_key, cw, ncw, have ? ids.data() : nullptr, B, use_bsgs, out, true);
}

// Pasta::init_shake + get_random_matrix + get_rc_vec (pasta_3_plain.cpp:56-119) on the device, for callers that want the matrices there
// (and for the tests of the kernels behind ensure_blocks)
extern "C" int hhe_pasta3_block_randomness_dev(hhe_ctx *c, const uint64_t *nonces, const uint64_t *blocks, size_t count, uint64_t *mats, uint64_t *rcs)
{
    HHE_LOCK(c);
    if (!c || !nonces || !blocks || !mats || !rcs || count == 0 || count > ((size_t)1 << 16))
        return fail(HHE_ERR_INVALID, "hhe_pasta3_block_randomness_dev: bad arguments");
    const std::vector<PastaPair> ids = pairs_of(nonces, blocks, count);
    rt_stream st = c->lanes[0].stream;
    DevBuf d_pairs(count * sizeof(PastaPair)), d_rand(count * PASTA_RAND_PER_BLOCK * 8);
    if (!d_pairs.p || !d_rand.p) return dev_fail("hhe_pasta3_block_randomness_dev");
    public_randomness_enqueue(c, ids.data(), count, (PastaPair *)d_pairs.p, d_rand.w(), mats, rcs, st);
    if (rt_sync(st)) return dev_fail("hhe_pasta3_block_randomness_dev");  // temporaries are released on return
    return HHE_OK;
}

// The table half of a transciphering call through hhe_pasta3_transcipher_nonce_ks on these pairs, in its groups: a service warms a
// counter range with it
extern "C" int hhe_pasta3_prepare_tables(hhe_ctx *c, const uint64_t *nonces, const uint64_t *blocks, size_t count, int use_bsgs, size_t *built_out)
{
    HHE_LOCK(c);
    if (!c || !nonces || !blocks || count == 0) return fail(HHE_ERR_INVALID, "hhe_pasta3_prepare_tables: bad arguments");
    const std::vector<PastaPair> ids = pairs_of(nonces, blocks, count);
    const std::vector<size_t> ends = pair_groups(c, ids.data(), count, use_bsgs);
    c->w = &c->lanes[0];
    c->last_public_built = 0;
    size_t total = 0;
    int rc = HHE_OK;
    for (size_t g = 0, b0 = 0; g < ends.size() && !rc; b0 = ends[g++]) {
        ++c->block_call;
        std::vector<BlockTables *> tabs(ends[g] - b0);
        size_t built = 0;
        rc = ensure_blocks(c, ids.data() + b0, tabs.size(), use_bsgs, tabs.data(), &built);
        if (!rc) total += built;
    }
    if (built_out) *built_out = total;
    return rc;
}

extern "C" int hhe_pasta3_set_block_cache_limit(hhe_ctx *c, size_t bytes)
{
    HHE_LOCK(c);
    if (!c) return fail(HHE_ERR_INVALID, "hhe_pasta3_set_block_cache_limit: null context");
    c->block_cache_limit = bytes;
    ++c->block_call;   // no transciphering call is running (the context is locked): nothing is pinned
    evict_blocks(c, 0);
    return HHE_OK;
}
extern "C" int hhe_mask(hhe_ctx *c, const uint64_t *ct, const uint64_t *mask_vals, size_t count, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || !ct || !mask_vals || !out || count > c->n) return fail(HHE_ERR_INVALID, "hhe_mask: bad arguments");
    int rc = need(c, B);
    if (rc) return rc;
    // D = lifted NTT form of the mask plaintext in ws_ct3 [0, L*N); the mask values are staged behind it
    Lane &ln = *c->w;
    u64 *D = ln.ws_ct3, *dv = ln.ws_ct3 + (size_t)c->L * c->n;
    stage_begin(ln);
    ln.h_stage.assign(mask_vals, mask_vals + count);
    rt_h2d(dv, ln.h_stage.data(), count * 8, ln.stream);
    stage_end(ln);
    op_encode(c, dv, 1, (int)count, (int)count, -1, ln.ws_plain);
    op_lift_ntt(c, ln.ws_plain, 1, D);
    op_multiply_plain_ntt(c, ct, D, nullptr, 0, out, B);
    return HHE_OK;
}

static int flatten_impl(hhe_ctx *c, const uint64_t *blocks, size_t nblocks, uint64_t *out, size_t S)
{
    if (!c || !blocks || !out || nblocks == 0) return fail(HHE_ERR_INVALID, "hhe_flatten: bad arguments");
    int rc = need(c, S);
    if (rc) return rc;
    const size_t ctw = c->ct_words();
    // gather block i of every sample into a contiguous batch (one strided copy kernel), rotate by -128*i, accumulate
    CopyItemsArgs g = zeroed<CopyItemsArgs>();
    g.src = blocks; g.words = ctw; g.count = S; g.src_stride = nblocks; g.dst_stride = 1;
    g.dst = out;
    k_copy_items(g, c->w->stream);
    for (size_t i = 1; i < nblocks; ++i) {
        g.dst = c->w->ws_ct[0]; g.src_off = i;
        k_copy_items(g, c->w->stream);
        if ((rc = op_rotate_rows(c, c->w->ws_ct[0], -(int)(i * PASTA_T), c->w->ws_ct[1], S))) return rc;
        op_add(c, out, c->w->ws_ct[1], out, S, 2);
    }
    return HHE_OK;
}
extern "C" int hhe_flatten_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *blocks, size_t nblocks, uint64_t *out, size_t S)
{
    HHE_LOCK(c);
    if (!c) return fail(HHE_ERR_INVALID, "hhe_flatten: null context");
    int rc = check_sets(c, gk);
    if (rc) return rc;
    KeyScope keys(c, gk, nullptr);
    return flatten_impl(c, blocks, nblocks, out, S);
}
extern "C" int hhe_flatten(hhe_ctx *c, const uint64_t *blocks, size_t nblocks, uint64_t *out, size_t S) { return hhe_flatten_ks(c, nullptr, blocks, nblocks, out, S); }

// BaseCSP::decompose (src/examples/CSP/CSP.cpp:235-283) / hhe_pktnn_1fc_inference (hhe_pktnn_examples.cpp:578-630) on device:
// per record: decomposition of every 128-word block, mask of the ragged last block, flatten -- without leaving HBM.
// nonces: one per record (its blocks run under (nonces[s], 0), (nonces[s], 1), ...), or null = the reference's fixed nonce
static int decompose_impl(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_keyset *flatten_gk, const uint64_t *enc_key,
                          const uint64_t *records, const uint64_t *nonces, size_t S, size_t nwords, int mask_last, uint64_t *out)
{
    HHE_LOCK(c);
    if (c) { int rcs = check_sets(c, rk, gk, flatten_gk); if (rcs) return rcs; }
    if (!c || !enc_key || !records || !out || S == 0 || nwords == 0) return fail(HHE_ERR_INVALID, "hhe_decompose: bad arguments");
    const size_t nb = (nwords + PASTA_T - 1) / PASTA_T, rem = nwords % PASTA_T, ctw = c->ct_words();
    if (nb * PASTA_T > c->n / 2) return fail(HHE_ERR_INVALID, "hhe_decompose: record does not fit one batching row");
    std::vector<u64> cw(S * nb * PASTA_T, 0);
    std::vector<PastaPair> bidx(S * nb);
    std::vector<uint32_t> ncw(S * nb);
    for (size_t s = 0; s < S; ++s)
        for (size_t b = 0; b < nb; ++b) {
            const size_t lo = b * PASTA_T, hi = std::min(lo + PASTA_T, nwords);
            memcpy(&cw[(s * nb + b) * PASTA_T], records + s * nwords + lo, (hi - lo) * 8);
            ncw[s * nb + b] = (uint32_t)(hi - lo);
            bidx[s * nb + b] = nonces ? PastaPair(nonces[s], b) : PastaPair(b);
        }
    int rc = c->d_blocks.reserve(c, S * nb * ctw, "hhe_decompose");  // the decompositions of all blocks
    if (rc) return rc;
    u64 *blocks = c->d_blocks.p;
    {   // PASTA_SEAL HHE(context, pk, sk, analyst rk, analyst gk).decomposition(...) (CSP.cpp:238-252)
        KeyScope keys(c, gk, rk);
        rc = transcipher_impl(c, enc_key, cw.data(), ncw.data(), bidx.data(), S * nb, 0, blocks, nonces != nullptr);
    }
    if (!rc && mask_last && rem) {
        // hhe_pktnn_examples.cpp:620-625: ones on the first `rem` slots (CSP.cpp:264-269 intends the same)
        if (!(rc = need(c, S))) {
            u64 *last = c->lanes[0].ws_ct[2];
            rt_stream st = c->lanes[0].stream;
            CopyItemsArgs g = zeroed<CopyItemsArgs>();
            g.src = blocks; g.dst = last; g.words = ctw; g.count = S; g.src_stride = nb; g.src_off = nb - 1; g.dst_stride = 1;
            k_copy_items(g, st);
            std::vector<u64> ones(rem, 1);
            rc = hhe_mask(c, last, ones.data(), rem, last, S);
            g.src = last; g.dst = blocks; g.src_stride = 1; g.src_off = 0; g.dst_stride = nb; g.dst_off = nb - 1;
            if (!rc) k_copy_items(g, st);
        }
    }
    if (!rc) {  // HHE.flatten(record, tmp, csp_gk) (CSP.cpp:271-278): the Galois keys the call names
        KeyScope keys(c, flatten_gk, nullptr);
        rc = flatten_impl(c, blocks, nb, out, S);
    }
    if (!rc && rt_sync(c->lanes[0].stream)) rc = dev_fail("hhe_decompose");
    return rc;
}
extern "C" int hhe_decompose_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_keyset *flatten_gk, const uint64_t *enc_key,
                                const uint64_t *records, size_t S, size_t nwords, int mask_last, uint64_t *out)
{
    return decompose_impl(c, rk, gk, flatten_gk, enc_key, records, nullptr, S, nwords, mask_last, out);
}
extern "C" int hhe_decompose_nonce_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_keyset *flatten_gk, const uint64_t *enc_key,
                                      const uint64_t *records, const uint64_t *nonces, size_t S, size_t nwords, int mask_last, uint64_t *out)
{
    if (!nonces) return fail(HHE_ERR_INVALID, "hhe_decompose: bad arguments");
    return decompose_impl(c, rk, gk, flatten_gk, enc_key, records, nonces, S, nwords, mask_last, out);
}
extern "C" int hhe_decompose(hhe_ctx *c, const uint64_t *enc_key, const uint64_t *records, size_t S, size_t nwords,
                             int mask_last, uint64_t *out)
{
    return hhe_decompose_ks(c, nullptr, nullptr, nullptr, enc_key, records, S, nwords, mask_last, out);
}

// sealhelper::encrypted_vec_sum (sealhelper.cpp:379-392) adds rotate_rows(prod, -i) for i = 1..n-1, each rotation
// going through SEAL's NAF decomposition (evaluator.h:955-1060).  The NAF term sequences of different i
// share prefixes, and every key switch is a deterministic function of its input, so the rotations form a trie whose
// nodes are computed once: 2875 key switches become 1054 for n = 784 with bit-identical ciphertexts
// (modular addition is commutative, so the order of the final additions is free).
namespace {
struct NafNode {
    int term = 0;
    int mult = 0;                 // how many i end exactly here
    std::vector<int> kids;
};
struct FcLeafAcc {  // sums over the leaves of the trie (DESIGN.md "FC rotation trie"): accS in the NTT domain, accH in the
    u64 *accS, *accH, *rscr;  // coefficient domain (rounding terms + q_sp * galois(c0), added by leaf_round_kernel)
};
// rounding terms of m leaf key switches: inverse transform of their special-limb sums (S: [B][2][m][N] when dense, else the special slot
// of ws_S [B][2][K][N] for one leaf) into acc.rscr [B][2][m][N] (r = INTT(S_k[special]) + half), then the element-wise sums
// half_j - (r mod q_j) (+ q_sp * galois_l(c0 of leaf l's parent) for k = 0) into acc.accH
static void fc_leaf_round(hhe_ctx *c, const u64 *S, bool dense, const u64 *const *parents, const u32 *einv, int m, const FcLeafAcc &acc, size_t B)
{
    k_ntt(ks_rsp_args(c, S, acc.rscr, B * 2 * m, !dense), true, c->w->stream);
    LeafRoundArgs lr = zeroed<LeafRoundArgs>();
    lr.r = acc.rscr; lr.accH = acc.accH; lr.base_stride = c->ct_words(); lr.mods = c->d_mods; lr.logn = c->logn;
    lr.B = (int)B; lr.L = c->L; lr.m = m; lr.ks = c->ksc;
    for (int l = 0; l < m; l++) { lr.base[l] = parents[l]; lr.gal_einv[l] = einv[l]; }
    k_leaf_round(lr, c->w->stream);
}
// A leaf's ciphertext is only ever added into the result.  Key switching is linear up to the rounding term, so for
// leaves the inverse transforms of S_k[j] are postponed: sum S_k[j] over all leaves in the NTT domain, sum the rounding
// terms half_j - (r_k mod q_j) and galois(c0) in the coefficient domain, inverse-transform once (14 instead of 20
// transforms per leaf; identical words because every step is exact modular arithmetic).
int fc_leaf(hhe_ctx *c, const u64 *parent, u32 elt, const FcLeafAcc &acc, size_t B)
{
    const u64 *key = galois_key(c, elt);
    if (!key) return HHE_ERR_NO_GALOIS_KEY;
    const size_t ln = (size_t)c->L * c->n;
    const u32 einv = galois_einv(c, elt);
    // d = galois(c1); galois(c0) joins the sums inside leaf_round_kernel below
    k_galois(galois_args(c, B, einv, parent + ln, 2 * ln, c->w->ws_d, ln), c->w->stream);
    k_ntt(ks_digit_args(c, c->w->ws_d, ln, c->w->ws_T, B), false, c->w->stream);
    KsMacArgs m = ks_mac_args(c, c->w->ws_T, key, c->w->ws_S, B);
    m.s_acc = acc.accS;
    k_ks_mac(m, c->w->stream);
    fc_leaf_round(c, c->w->ws_S, false, &parent, &einv, 1, acc, B);
    return HHE_OK;
}
// ---- shared digits (DESIGN.md "FC rotation trie", step 3) ----
// All children of a trie node rotate the SAME ciphertext.  The digit transforms NTT_J(c1_I) are computed once per node;
// for a child with Galois element g the transforms of the digits of galois_g(c1) are the NTT-domain index map of those
// (read through the map inside ks_mac_kernel) plus q_I * NTT_J(s_g) for I != J, where s_g marks the coefficients whose
// sign galois_g flips -- exact as long as no coefficient of c1 is 0 (a flipped 0 stays 0 instead of becoming q_I); the
// digit loads raise zero_flag in that case and the caller recomputes with per-child transforms.  The key-dependent part
// of the correction, NTT_J(s_g) * sum_{I != J} (q_I mod q_J) key_g[I][k][J], is tabulated once per Galois key.
int fc_corr(hhe_ctx *c, u32 elt, const u64 *key, const u64 **out)
{
    auto it = c->gks->gk_corr.find(elt);
    if (it != c->gks->gk_corr.end()) { *out = it->second; return HHE_OK; }
    const int L = c->L, K = c->K;
    const size_t n = c->n;
    std::vector<u64> s((size_t)K * n, 0), qmod((size_t)L * K);
    for (size_t i = 0; i < n; ++i) {  // GaloisTool::apply_galois (util/galois.h:32): i -> i*g mod 2N, negated when it wraps
        const u64 raw = (u64)i * elt;
        if ((raw >> c->logn) & 1) s[raw & (n - 1)] = 1;
    }
    for (int J = 1; J < K; ++J) memcpy(&s[(size_t)J * n], &s[0], n * 8);
    for (int I = 0; I < L; ++I)
        for (int J = 0; J < K; ++J) qmod[(size_t)I * K + J] = c->q[I] % c->q[J];
    u64 *shat = (u64 *)rt_malloc((size_t)K * n * 8), *dq = (u64 *)rt_malloc(qmod.size() * 8), *corr = (u64 *)rt_malloc((size_t)2 * K * n * 8);
    if (!shat || !dq || !corr) { rt_free(shat); rt_free(dq); rt_free(corr); return dev_fail("fc_corr"); }
    rt_stream st = c->w->stream;
    rt_h2d(shat, s.data(), s.size() * 8, st);
    rt_h2d(dq, qmod.data(), qmod.size() * 8, st);
    NttArgs a = ntt_args(c, shat, shat, K, 0, K);
    k_ntt(a, false, st);
    KsCorrArgs k;
    k.key = key; k.shat = shat; k.qmod = dq; k.corr = corr; k.mods = c->d_mods; k.logn = c->logn; k.L = L; k.K = K;
    k_ks_corr(k, st);
    const int bad = rt_sync(st);  // host staging buffers and the temporaries go out of scope
    rt_free(shat); rt_free(dq);
    if (bad) { rt_free(corr); return dev_fail("fc_corr"); }
    c->gks->gk_corr[elt] = corr;
    *out = corr;
    return HHE_OK;
}
// digit transforms of the un-rotated c1 of `parent` into tp ([B][L][K][N], lazy range)
// sp_only: the transforms modulo the special prime alone, tp [B][L][N] (a node whose children are all leaves of the c1-sum scheme)
void fc_parent_digits(hhe_ctx *c, const u64 *parent, u64 *tp, size_t B, bool sp_only = false)
{
    const size_t ln = (size_t)c->L * c->n;
    k_ntt(ks_digit_args(c, parent + ln, 2 * ln, tp, B, 0, c->w->zero_flag, sp_only), false, c->w->stream);
}
// one child of a node from the node's shared digit transforms: leaf (sums only) or full ciphertext into `cur`
int fc_child_shared(hhe_ctx *c, const u64 *parent, const u64 *tp, u32 elt, const FcLeafAcc *leaf, u64 *cur, size_t B, u64 *add_to = nullptr,
                    const u64 *c0hat = nullptr)
{
    const u64 *key = galois_key(c, elt);
    if (!key) return HHE_ERR_NO_GALOIS_KEY;
    const u64 *corr = nullptr;
    int rc = fc_corr(c, elt, key, &corr);
    if (rc) return rc;
    const u32 einv = galois_einv(c, elt);  // galois(c0) is gathered on the fly (leaf_round_kernel for leaves, the KSF epilogue otherwise)
    const KsSplit sp = ks_split(c, c->w->ws_S, B);  // the output of non-leaf children
    // ... whose mod-down also adds a child that is itself a term of the sum (add_to).  c0_inside: galois(c0) is already in S_0 (KsRowArgs::c0hat)
    auto ksf = [&](bool c0_inside) {
        NttArgs a = ks_ksf_args(c, sp, B, c0_inside ? nullptr : parent, c->ct_words(), 1, einv, cur);
        a.acc = add_to;
        return a;
    };
    const u64 *key_s = nullptr;
    if (!leaf && c->fc_row_fused && use_row_kernel(c) && ensure_key_shoup(c, key, &key_s) == HHE_OK) {
        // N >= 4096: inner product over the shared digits and the inverse row pass of all 2K sums in one kernel (the sums never make a
        // round trip), then the strided inverse passes with the mod-down, the Galois-gathered c0 and the running sum in the data limbs' store
        KsRowArgs x = ks_row_args(c, key, key_s, B, &sp);
        x.T = tp; x.corr = corr; x.perm_elt = elt; x.c0hat = c0hat;
        if (k_ks_perm_row(ntt_args(c, nullptr, nullptr, 0, 0, c->K), x, c->w->stream)) return dev_fail("fc: key-switch row kernel");
        ks_finish_split(c, sp, ksf(c0hat != nullptr), B, false);
        return HHE_OK;
    }
    KsMacArgs m = ks_mac_args(c, tp, key, c->w->ws_S, B);
    m.perm_elt = elt; m.corr = corr;
    if (leaf) m.s_acc = leaf->accS;
    else m.S_sp = sp.Usp;
    k_ks_mac(m, c->w->stream);
    if (leaf) {
        fc_leaf_round(c, c->w->ws_S, false, &parent, &einv, 1, *leaf, B);
        return HHE_OK;
    }
    // all 2K sums are inverse-transformed (the row passes of the special and the data limbs in one grid); the mod-down rides in the
    // store of the data limbs' last pass (STORE_KSF)
    ks_finish_split(c, sp, ksf(false), B, true);
    return HHE_OK;
}
// The walk over the trie with shared digits.  A node's digit transforms and ciphertext live in a slot of the lane's pool (Lane::FcSlot)
// for as long as something still reads them: the walk below the node, and its LEAF children, whose key switches are queued and run in
// groups of up to HHE_LEAF_GROUP -- leaves of different nodes together -- with one inner-product launch (the data-limb sums of all of them
// meet accS in one read-modify-write), one inverse transform of their 2 x m special-limb sums and one rounding kernel (accH read and
// written once).  The order of the additions into the sums is immaterial: exact modular arithmetic.
struct FcWalk {
    hhe_ctx *c;
    const std::vector<NafNode> &trie;
    u64 *out;
    const FcLeafAcc *acc;
    size_t B;
    int group, max_slots;
    bool csum;   // data limbs of the leaves through per-element sums of their parents' c1 (CsumArgs); the leaf queue then carries the special limb only
    struct Leaf { int slot; const u64 *parent; u32 elt; } q[HHE_LEAF_GROUP];
    int m = 0;
    struct ElemSum {   // one per Galois element among the leaves
        u32 elt;
        u64 *sums;      // [B][L][N] integer sums of c1 limbs
        u64 *sums0;     // [B][L][N] sums of c0 limbs mod q_j
        unsigned char *carry;  // [B][L][N] wraps of `sums`
        int count = 0;  // leaves summed into `sums`
        int npend = 0;  // parents queued for the next csum_add launch
        int pend_slot[HHE_CSUM_GROUP];
        const u64 *pend_c1[HHE_CSUM_GROUP];
    };
    std::vector<ElemSum> esums;
    static constexpr int CSUM_MAX = 2000;   // terms below 2^61: fewer than 255 wraps of the 64-bit word (CsumArgs::carry is a byte)

    CsumArgs csum_args(const ElemSum &e) const
    {
        CsumArgs a = zeroed<CsumArgs>();
        a.sums = e.sums; a.carry = e.carry; a.mods = c->d_mods; a.logn = c->logn; a.B = (int)B; a.L = c->L; a.K = c->K;
        return a;
    }
    int csum_add_pending(ElemSum &e)
    {
        if (!e.npend) return HHE_OK;
        Lane &ln = *c->w;
        CsumArgs a = csum_args(e);
        a.sums0 = e.sums0; a.src_stride = c->ct_words(); a.m = e.npend;
        for (int l = 0; l < e.npend; l++) a.src[l] = e.pend_c1[l];
        k_csum_add(a, ln.stream);
        for (int l = 0; l < e.npend; l++) ln.fc_slots[e.pend_slot[l]].refs--;
        e.count += e.npend;
        e.npend = 0;
        return HHE_OK;
    }
    // closes a sum: digits of galois(sum) mod every key-level prime, their transforms, ONE inner product into accS
    int csum_close(ElemSum &e)
    {
        int rc = csum_add_pending(e);
        if (rc || !e.count) return rc;
        Lane &ln = *c->w;
        const u64 *key = galois_key(c, e.elt);
        if (!key) return HHE_ERR_NO_GALOIS_KEY;
        const int L = c->L, K = c->K;
        CsumArgs a = csum_args(e);
        a.out = ln.ws_T; a.einv = galois_einv(c, e.elt); a.count = (u32)e.count;
        k_csum_digits(a, ln.stream);
        a.sums0 = e.sums0; a.accH = acc->accH;
        for (int j = 0; j < L; j++) { a.qsp_mod[j] = c->ksc.qsp_mod[j]; a.qsp_mod_s[j] = c->ksc.qsp_mod_s[j]; }
        k_csum_c0(a, ln.stream);
        NttArgs t = ntt_args(c, ln.ws_T, ln.ws_T, B * L * K, 0, K);
        t.store_op = STORE_LAZY;
        k_ntt(t, false, ln.stream);
        KsMacArgs mm = ks_mac_args(c, ln.ws_T, key, ln.ws_S, B);
        mm.s_acc = acc->accS; mm.perm_elt = 1; mm.corr = c->d_zero_corr;  // the digits are those of the ROTATED sum: identity map, no correction
        k_ks_mac(mm, ln.stream);
        rt_memset(e.sums, 0, B * (size_t)L * c->n * 17, ln.stream);   // sums | sums0 | carry
        e.count = 0;
        c->fc_csum_closes++;
        return HHE_OK;
    }
    int csum_leaf(int slot, const u64 *parent, u32 elt)
    {
        Lane &ln = *c->w;
        ElemSum *e = nullptr;
        for (auto &x : esums) if (x.elt == elt) e = &x;
        if (!e) {
            if (ln.csum_bufs.size() <= esums.size()) {
                u64 *p = (u64 *)rt_malloc(ln.fc_slot_cap * (size_t)c->L * c->n * 17);   // sums | sums0 | carry bytes
                if (!p) return dev_fail("hhe_fc_row workspace");
                ln.csum_bufs.push_back(p);
            }
            ElemSum x;
            x.elt = elt; x.sums = ln.csum_bufs[esums.size()]; x.sums0 = x.sums + B * (size_t)c->L * c->n;
            x.carry = (unsigned char *)(x.sums0 + B * (size_t)c->L * c->n);
            rt_memset(x.sums, 0, B * (size_t)c->L * c->n * 17, ln.stream);
            esums.push_back(x);
            e = &esums.back();
        }
        int rc;
        if (e->count + e->npend >= CSUM_MAX && (rc = csum_close(*e))) return rc;
        e->pend_slot[e->npend] = slot; e->pend_c1[e->npend] = parent;
        ++e->npend;
        ln.fc_slots[slot].refs++;
        if (e->npend == c->fc_csum_group) return csum_add_pending(*e);
        return HHE_OK;
    }

    int flush()
    {
        Lane &ln = *c->w;
        int rc = HHE_OK;
        if (m > 0 && !csum && (group == 1 || m == 1)) {
            for (int l = 0; l < m && !rc; l++) rc = fc_child_shared(c, q[l].parent, ln.fc_slots[q[l].slot].tp, q[l].elt, acc, nullptr, B);
        } else if (m > 0) {
            KsMacLeavesArgs a = zeroed<KsMacLeavesArgs>();
            u32 einv[HHE_LEAF_GROUP];
            const u64 *parents[HHE_LEAF_GROUP];
            for (int l = 0; l < m; l++) {
                if (!(a.key[l] = galois_key(c, q[l].elt))) return HHE_ERR_NO_GALOIS_KEY;
                if ((rc = fc_corr(c, q[l].elt, a.key[l], &a.corr[l]))) return rc;
                a.T[l] = ln.fc_slots[q[l].slot].tp; a.t_polys[l] = ln.fc_slots[q[l].slot].tp_polys; a.perm_elt[l] = q[l].elt;
                einv[l] = galois_einv(c, q[l].elt);
                parents[l] = csum ? nullptr : q[l].parent;   // the c0 terms of the leaves come from the per-element sums
            }
            a.S_sp = ln.ws_leaf.p; a.s_acc = acc->accS; a.mods = c->d_mods; a.logn = c->logn; a.B = (int)B; a.L = c->L; a.K = c->K; a.m = m;
            a.sp_only = csum ? 1 : 0;
            if (k_ks_mac_leaves(a, ln.stream)) return fail(HHE_ERR_INVALID, "fc: leaf group");
            fc_leaf_round(c, ln.ws_leaf.p, true, parents, einv, m, *acc, B);
        }
        for (int l = 0; l < m; l++) ln.fc_slots[q[l].slot].refs--;
        m = 0;
        return rc;
    }
    // a free slot (grow-only pool; everything runs in stream order on the lane's stream, so a slot whose readers have been ENQUEUED is free)
    int acquire(int *slot)
    {
        Lane &ln = *c->w;
        for (int pass = 0; pass < 2; pass++) {
            for (size_t i = 0; i < ln.fc_slots.size(); i++)
                if (ln.fc_slots[i].refs == 0) { ln.fc_slots[i].refs = 1; *slot = (int)i; return HHE_OK; }
            if ((int)ln.fc_slots.size() < max_slots) {
                Lane::FcSlot sl;
                sl.tp = (u64 *)rt_malloc(ln.fc_slot_cap * (size_t)c->L * c->K * c->n * 8);   // sized for the pool's capacity, not this call's batch
                sl.ct = (u64 *)rt_malloc(ln.fc_slot_cap * c->ct_words() * 8);
                sl.c0hat = (u64 *)rt_malloc(ln.fc_slot_cap * (size_t)c->L * c->n * 8);
                if (!sl.tp || !sl.ct || !sl.c0hat) { rt_free(sl.tp); rt_free(sl.ct); rt_free(sl.c0hat); return dev_fail("hhe_fc_row workspace"); }
                sl.refs = 1;
                ln.fc_slots.push_back(sl);
                *slot = (int)ln.fc_slots.size() - 1;
                return HHE_OK;
            }
            int rc = flush();  // the queued leaves hold the remaining slots
            for (auto &e : esums) if (!rc) rc = csum_add_pending(e);
            if (rc) return rc;
        }
        return fail(HHE_ERR_INVALID, "hhe_fc_row: slot pool");
    }
    // node's ciphertext is `parent`; `slot` receives the digit transforms of its c1
    int walk(int node, const u64 *parent, int slot)
    {
        if (trie[node].kids.empty()) return HHE_OK;
        Lane &ln = *c->w;
        auto is_leaf = [&](int kid) { return acc && trie[kid].kids.empty() && trie[kid].mult == 1; };
        bool only_leaves = csum;
        for (int kid : trie[node].kids) only_leaves = only_leaves && is_leaf(kid);
        // a node whose children are all leaves needs its digit transforms modulo the special prime only (their data limbs come from the c1 sums)
        fc_parent_digits(c, parent, ln.fc_slots[slot].tp, B, only_leaves);
        ln.fc_slots[slot].tp_polys = only_leaves ? 1 : c->K;
        bool has_nonleaf = false;
        for (int kid : trie[node].kids) has_nonleaf = has_nonleaf || !is_leaf(kid);
        const u64 *c0hat = nullptr;
        if (has_nonleaf && c->fc_c0hat && c->fc_row_fused && use_row_kernel(c)) {
            // NTT form of the node's c0: its non-leaf children take galois(c0) through the NTT-domain map inside ks_perm_row_kernel
            op_c0hat(c, parent, ln.fc_slots[slot].c0hat, B);
            c0hat = ln.fc_slots[slot].c0hat;
        }
        int rc;
        for (int kid : trie[node].kids) {
            if (!is_leaf(kid)) continue;
            const u32 elt = galois_elt_from_step(c, trie[kid].term);
            if (csum && (rc = csum_leaf(slot, parent, elt))) return rc;
            q[m].slot = slot; q[m].parent = parent; q[m].elt = elt;
            ++m;
            ln.fc_slots[slot].refs++;
            if (m >= group && (rc = flush())) return rc;
        }
        for (int kid : trie[node].kids) {
            if (acc && trie[kid].kids.empty() && trie[kid].mult == 1) continue;
            const u32 elt = galois_elt_from_step(c, trie[kid].term);
            int k = -1;
            if ((rc = acquire(&k))) return rc;
            u64 *cur = ln.fc_slots[k].ct;
            // a child that is itself a term of the sum (distinct steps have distinct term sequences: mult is 0 or 1) is added in its own epilogue
            if ((rc = fc_child_shared(c, parent, ln.fc_slots[slot].tp, elt, nullptr, cur, B, trie[kid].mult ? out : nullptr, c0hat))) return rc;
            for (int mm = 1; mm < trie[kid].mult; ++mm) op_add(c, out, cur, out, B, 2);
            if ((rc = walk(kid, cur, k))) return rc;
            ln.fc_slots[k].refs--;
        }
        return HHE_OK;
    }
};
int fc_dfs_shared(hhe_ctx *c, const std::vector<NafNode> &trie, int max_depth, const u64 *prod, u64 *out, const FcLeafAcc *acc, size_t B)
{
    Lane &ln = *c->w;
    if (ln.fc_slot_cap < B) {  // slots of a smaller batch: start over
        rt_sync(ln.stream);
        for (auto &sl : ln.fc_slots) { rt_free(sl.tp); rt_free(sl.ct); rt_free(sl.c0hat); }
        ln.fc_slots.clear();
        for (u64 *p : ln.csum_bufs) rt_free(p);
        ln.csum_bufs.clear();
        ln.fc_slot_cap = B;
    }
    for (auto &sl : ln.fc_slots) sl.refs = 0;
    const int group = c->L <= 4 ? std::min(HHE_LEAF_GROUP, c->fc_leaf_group) : 1;  // k_ks_mac_leaves is instantiated for L <= 4
    if (c->fc_c0hat && ensure_qsp_poly(c)) return dev_fail("hhe_fc_row workspace");
    // the c1-sum scheme serves leaf sums (acc) with a group kernel (L <= 4); its zero table stands in for the correction of the closing product
    bool csum = acc && c->fc_csum && c->L <= 4;
    if (csum && !c->d_zero_corr) {
        const size_t bytes = (size_t)2 * c->K * c->n * 8;
        if (!(c->d_zero_corr = (u64 *)rt_malloc(bytes))) return dev_fail("hhe_fc_row workspace");
        rt_memset(c->d_zero_corr, 0, bytes, ln.stream);
        if (rt_sync(ln.stream)) return dev_fail("hhe_fc_row workspace");   // once per context: chunks on other streams read the table too
    }
    FcWalk w{c, trie, out, acc, B, group, max_depth + 1 + group + 3 * HHE_CSUM_GROUP, csum};
    w.esums.reserve(64);
    int root = -1, rc = w.acquire(&root);
    if (!rc) rc = w.walk(0, prod, root);
    if (!rc) rc = w.flush();
    for (auto &e : w.esums) if (!rc) rc = w.csum_close(e);
    return rc;
}
int fc_dfs(hhe_ctx *c, const std::vector<NafNode> &trie, int node, int depth, const u64 *parent, u64 *bufs, u64 *out,
           const FcLeafAcc *acc, size_t B)
{
    const size_t ctw = c->ct_words();
    for (int kid : trie[node].kids) {
        const u32 elt = galois_elt_from_step(c, trie[kid].term);
        if (acc && trie[kid].kids.empty() && trie[kid].mult == 1) {
            int rc = fc_leaf(c, parent, elt, *acc, B);
            if (rc) return rc;
            continue;
        }
        u64 *cur = bufs + (size_t)depth * B * ctw;
        int rc = op_apply_galois(c, parent, elt, cur, B);
        if (rc) return rc;
        for (int m = 0; m < trie[kid].mult; ++m) op_add(c, out, cur, out, B, 2);
        if ((rc = fc_dfs(c, trie, kid, depth + 1, cur, bufs, out, acc, B))) return rc;
    }
    return HHE_OK;
}
}  // namespace

// trie of the NAF term sequences of steps -1 .. -(n_inputs - 1) over the named Galois keys (terms equal to +-N/2 are skipped,
// evaluator.h rotate_internal); depends on n_inputs, the key set and default_galois_only alone: built once per call
static int fc_build_trie(const hhe_ctx *c, size_t n_inputs, int default_galois_only, std::vector<NafNode> &trie, int &max_depth)
{
    trie.assign(1, NafNode());
    max_depth = 0;
    for (size_t i = 1; i < n_inputs; ++i) {
        const int step = -(int)i;
        std::vector<int> terms;
        const u32 direct = galois_elt_from_step(c, step);
        const bool pow2 = (i & (i - 1)) == 0;
        if (c->gks->gk.count(direct) && (pow2 || !default_galois_only)) terms.push_back(step);  // has_key(elt): one key switch
        else
            for (int t : nt_naf(step))
                if ((size_t)std::abs(t) != c->n / 2) terms.push_back(t);
        if (terms.size() == 1 && !c->gks->gk.count(galois_elt_from_step(c, terms[0]))) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
        int node = 0;
        for (int t : terms) {
            if (!c->gks->gk.count(galois_elt_from_step(c, t))) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
            int next = -1;
            for (int kid : trie[node].kids)
                if (trie[kid].term == t) { next = kid; break; }
            if (next < 0) {
                next = (int)trie.size();
                trie.push_back(NafNode());
                trie[next].term = t;
                trie[node].kids.push_back(next);
            }
            node = next;
        }
        trie[node].mult++;
        max_depth = std::max(max_depth, (int)terms.size());
    }
    if (max_depth + 1 > ROT_SLOTS) return fail(HHE_ERR_INVALID, "hhe_fc_row: NAF depth");  // the unshared walk keeps one ciphertext per depth in ws_rot
    return HHE_OK;
}

// one chunk on the current lane (c->w, workspaces reserved by the caller), enqueued asynchronously; shared = the shared-digit
// evaluation (raises the lane's zero_flag when it is not exact)
static int fc_row_chunk(hhe_ctx *c, bool shared, const std::vector<NafNode> &trie, int max_depth, const uint64_t *vi, const uint64_t *w,
                        size_t W, uint64_t *out, size_t B)
{
    Lane &ln = *c->w;
    const int L = c->L;
    const size_t ctw = c->ct_words();
    u64 *wb = ln.ws_ct[0], *prod = ln.ws_rot.p;  // depth-0 buffer holds the product
    op_elt(c, ELT_BCAST, nullptr, w, wb, B * 2 * L, 0, L, (int)(W * 2 * L));
    op_multiply(c, vi, wb, ln.ws_ct3, B);                                  // packed_enc_multiply
    int rc = op_relinearize(c, ln.ws_ct3, prod, B);                        // CSP.cpp:306 (the RelinKeys object the call names: c->rks)
    if (rc) return rc;
    const size_t bln = B * (size_t)L * c->n;
    // one evaluation of the rotation trie; shared = children of a node reuse the digit transforms of its c1
    if (max_depth == 0) shared = false;
    rt_d2d(out, prod, B * ctw * 8, ln.stream);
    auto dfs = [&](const FcLeafAcc *acc) {
        return shared ? fc_dfs_shared(c, trie, max_depth, prod, out, acc, B) : fc_dfs(c, trie, 0, 1, prod, ln.ws_rot.p, out, acc, B);
    };
    if (!c->fc_leaf_sums) return dfs(nullptr);
    FcLeafAcc acc;
    acc.accS = ln.ws_ct[0]; acc.accH = ln.ws_ct[1]; acc.rscr = ln.ws_leaf.p + B * 2 * (size_t)HHE_LEAF_GROUP * c->n;
    rt_memset(acc.accS, 0, 2 * bln * 8, ln.stream);
    rt_memset(acc.accH, 0, 2 * bln * 8, ln.stream);
    if ((rc = dfs(&acc))) return rc;
    op_ntt(c, acc.accS, B * 2 * L, 0, L, true);
    LeafSumArgs ls = zeroed<LeafSumArgs>();
    ls.accS = acc.accS; ls.accH = acc.accH; ls.out = out; ls.mods = c->d_mods; ls.logn = c->logn;
    ls.B = (int)B; ls.L = L; ls.ks = c->ksc;
    k_leaf_sum(ls, ln.stream);
    return HHE_OK;
}

// hhe_fc_row with the key objects already named: c->rks relinearizes the product, c->gks serves the rotation sum
static int fc_row_impl(hhe_ctx *c, const uint64_t *vi, const uint64_t *w, size_t W, size_t n_inputs, int default_galois_only, uint64_t *out, size_t B)
{
    if (!c || !vi || !w || !out || W == 0 || B == 0 || n_inputs == 0 || n_inputs > c->n / 2)
        return fail(HHE_ERR_INVALID, "hhe_fc_row: bad arguments");
    if (!c->rks->rk) return fail(HHE_ERR_NO_RELIN_KEY, "relinearization key not set");
    std::vector<NafNode> trie;
    int max_depth = 0, rc = fc_build_trie(c, n_inputs, default_galois_only, trie, max_depth);
    if (rc) return rc;
    // chunks bound the key-switch working set (digit transforms per trie level); a chunk is a multiple of W so that item i
    // of a chunk still uses weight row i % W.  A single chunk runs on the main lane, without a fork.
    size_t per = c->fc_chunk ? c->fc_chunk : B;
    if (per < B) per = std::max<size_t>(W, per / W * W);
    ChunkPlan plan(B, std::min(per, B), c->nstreams);
    if (plan.nch == 1) plan.ns = 0;
    const size_t ctw = c->ct_words();
    // a zero coefficient in some c1 (probability ~ N/q per ciphertext): that chunk is recomputed with per-child transforms
    return run_chunks_checked(c, plan, "hhe_fc_row", "hhe_fc_row", c->fc_shared != 0, c->fc_shared == 2, c->fc_fallbacks,
        [&](Lane &ln, bool) {
            int r = lane_reserve(c, ln, plan.per);
            if (!r) r = ln.ws_rot.reserve(c, plan.per * ROT_SLOTS * ctw, "hhe_fc_row workspace");
            if (!r && c->fc_leaf_sums) r = ln.ws_leaf.reserve(c, plan.per * 4 * (size_t)HHE_LEAF_GROUP * c->n, "hhe_fc_row workspace");
            return r;
        },
        [&](Lane &, size_t, size_t b0, size_t bc, bool shared) {
            return fc_row_chunk(c, shared, trie, max_depth, vi + b0 * ctw, w, W, out + b0 * ctw, bc);
        });
}
extern "C" int hhe_fc_row_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const uint64_t *vi, const uint64_t *w, size_t W, size_t n_inputs,
                             uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c) return fail(HHE_ERR_INVALID, "hhe_fc_row: null context");
    int rc = check_sets(c, rk, gk);
    if (rc) return rc;
    KeyScope keys(c, gk, rk);
    return fc_row_impl(c, vi, w, W, n_inputs, 0, out, B);  // the set IS the GaloisKeys object: every key it holds is visible to rotate_rows
}
extern "C" int hhe_fc_row(hhe_ctx *c, const uint64_t *vi, const uint64_t *w, size_t W, size_t n_inputs, int relin_slot,
                          int default_galois_only, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || relin_slot < 0 || relin_slot >= HHE_RELIN_SLOTS) return fail(HHE_ERR_INVALID, "hhe_fc_row: bad arguments");
    KeyScope keys(c, nullptr, c->relin_set(relin_slot));
    return fc_row_impl(c, vi, w, W, n_inputs, default_galois_only, out, B);
}

// ====================================================================== packed plain-matrix affine layers
// SEALZpCipher::packed_matMul / packed_affine (src/pasta/SEAL_Cipher.cpp:522-543) over diagonal (:271-313) and babystep_giantstep
// (:185-267) with a resident matrix handle.
namespace {
// add_bsgs_indices / add_diagonal_indices (:337-355): the rotate_rows steps of one layer, in the reference's order
int affine_steps(size_t N, size_t dim, size_t n1, size_t n2, std::vector<int> &steps)
{
    if (N == 0 || dim == 0 || (n1 == 0) != (n2 == 0)) return fail(HHE_ERR_INVALID, "affine layer: bad dimensions");
    if (n1 && n1 * n2 != dim) return fail(HHE_ERR_INVALID, "affine layer: n1 * n2 != dim");
    if (dim * 2 != N && dim * 4 > N) return fail(HHE_ERR_TOO_FEW_SLOTS, "too little slots for matmul implementation!");
    steps.clear();
    if (dim * 2 != N) steps.push_back(-(int)dim);
    steps.push_back(1);
    if (n1 > 1 && n2 > 1)
        for (size_t k = 1; k < n2; ++k) steps.push_back((int)(k * n1));
    return HHE_OK;
}
// can Evaluator::rotate_rows serve `step` from the named set: its key, or every term of its NAF (recursively, as op_rotate_rows goes)
bool rot_reachable(const hhe_ctx *c, int step)
{
    if (step == 0) return true;
    const u32 elt = galois_elt_from_step(c, step);
    if (!elt) return false;
    if (c->gks->gk.count(elt)) return true;
    const std::vector<int> terms = nt_naf(step);
    if (terms.size() == 1) return false;
    for (int term : terms) {
        if ((size_t)std::abs(term) == c->n / 2) continue;
        if (!rot_reachable(c, term)) return false;
    }
    return true;
}

// one chunk on the current lane: in / out [B][2][L][N] (may be the same buffer)
int affine_chunk(hhe_ctx *c, const hhe_matrix *m, const u64 *in, u64 *out, size_t B)
{
    const int L = c->L;
    const size_t ln = (size_t)L * c->n, ctw = 2 * ln;
    Lane &w = *c->w;
    const int pre = m->dim * 2 != c->n ? -(int)m->dim : 0;
    const u64 *res = nullptr;
    int rc;
    if (!m->n1) {
        // diagonal (:271-313): the fused loop of the PASTA layers with dim steps of rotate_rows(+1) and the one table for every item
        rt_d2d(w.ws_ct[0], in, B * ctw * 8, w.stream);
        const DiagSched sch{(int)m->dim, 1, pre, 0, m->dim * ln};
        if ((rc = matmul_diagonal_fused(c, sch, m->self.p, B))) return rc;
        res = w.ws_ct[0];
    } else {
        // babystep_giantstep (:185-267).  The baby steps are a sequential chain (each key switch's rounding feeds the next); then ONE
        // forward transform over all of them, all n2 inner sums in one kernel, ONE inverse transform, and the giant rotations
        const size_t n1 = (size_t)m->n1, n2 = (size_t)m->n2;
        u64 *rot = w.ws_aff.p, *inner = rot + n1 * B * ctw;  // [n1][B][2][L][N] | [n2][B][2][L][N]
        rt_d2d(rot, in, B * ctw * 8, w.stream);
        if (pre && (rc = op_prep_rows(c, rot, pre, w.ws_ct[2], B))) return rc;
        for (size_t j = 1; j < n1; ++j)
            if ((rc = op_rotate_rows(c, rot + (j - 1) * B * ctw, 1, rot + j * B * ctw, B))) return rc;
        op_ntt(c, rot, n1 * B * 2 * L, 0, L, false);
        PermArgs p = perm_args(c, B * 2 * L, rot, inner, ctw);
        p.bsgs_n1 = (int)n1; p.bsgs_n2 = (int)n2;
        p.in_step_stride = B * ctw; p.in_item_stride = ctw; p.out_step_stride = B * ctw;
        p.mul_ptrs = m->self.p; p.mul_step_stride = ln;
        k_perm(p, w.stream);
        op_ntt(c, inner, n2 * B * 2 * L, 0, L, true);
        // the generic key switch adds its base polynomials of the ROTATED ciphertext only (STORE_KSF), so the outer sum is an op_add
        for (size_t k = 1; k < n2; ++k) {
            u64 *ik = inner + k * B * ctw;
            if ((rc = op_rotate_rows(c, ik, (int)(k * n1), ik, B))) return rc;
            op_add(c, inner, ik, inner, B, 2);
        }
        res = inner;
    }
    if (m->bias) op_add_plain(c, res, m->bias, nullptr, 0, true, false, false, out, B);
    else rt_d2d(out, res, B * ctw * 8, w.stream);
    return HHE_OK;
}
// the handle's pointer array for chunks of `per` items: every entry names the one table
int matrix_reserve_self(hhe_ctx *c, hhe_matrix *m, size_t per)
{
    bool grew = false;
    int rc = m->self.reserve(c, per, "hhe_packed_affine: pointer table", &grew);
    if (rc || !grew) return rc;
    rt_stream st = c->lanes[0].stream;
    std::vector<const u64 *> h(m->self.cap, m->tab);
    if (rt_h2d((void *)m->self.p, h.data(), h.size() * sizeof(u64 *), st) || rt_sync(st)) {
        rc = dev_fail("hhe_packed_affine: pointer table");
        m->self.release();  // never leave an unfilled array behind
        return rc;
    }
    return HHE_OK;
}
}  // namespace

void matrix_free(hhe_matrix *m)
{
    if (!m) return;
    rt_free(m->tab); rt_free(m->bias); m->self.release();
    delete m;
}

extern "C" int hhe_affine_galois_steps(size_t N, size_t dim, size_t n1, size_t n2, int *steps_out, size_t *count)
{
    if (!count) return fail(HHE_ERR_INVALID, "hhe_affine_galois_steps: null argument");
    std::vector<int> steps;
    int rc = affine_steps(N, dim, n1, n2, steps);
    return rc ? rc : steps_out_copy("hhe_affine_galois_steps", steps, steps_out, count);
}

extern "C" int hhe_matrix_create(hhe_ctx *c, const uint64_t *M, size_t dim, const uint64_t *bias, size_t n1, size_t n2, hhe_matrix **out)
{
    HHE_LOCK(c);
    if (!c || !M || !out) return fail(HHE_ERR_INVALID, "hhe_matrix_create: null argument");
    std::vector<int> steps;
    int rc = affine_steps(c->n, dim, n1, n2, steps);
    if (rc) return rc;
    if (n1 == 1 || n2 == 1) n1 = n2 = 0;  // packed_matMul (:526): degenerate parameters take the diagonal method
    for (size_t i = 0; i < dim * dim; ++i)
        if (M[i] >= c->t) return fail(HHE_ERR_INVALID, "hhe_matrix_create: matrix entry not below the plain modulus");
    for (size_t i = 0; bias && i < dim; ++i)
        if (bias[i] >= c->t) return fail(HHE_ERR_INVALID, "hhe_matrix_create: bias entry not below the plain modulus");
    const size_t n = c->n, ln = (size_t)c->L * n;
    const bool full = dim * 2 == n;
    // the slot vectors BatchEncoder::encode receives, zero padded to one length: diag_i[j] = M[j][(i + j) % dim] (:290-301); BSGS
    // rotates diag_i right by k n1, k = i / n1, and in the non-full-packed case moves its first k n1 entries behind the end (:201-224)
    const size_t stride = n1 && !full ? dim + (n2 - 1) * n1 : dim;
    std::vector<u64> vals(dim * stride, 0), d(dim);
    for (size_t i = 0; i < dim; ++i) {
        for (size_t j = 0; j < dim; ++j) d[j] = M[j * dim + (i + j) % dim];
        u64 *v = &vals[i * stride];
        const size_t r = n1 ? i / n1 * n1 : 0;
        for (size_t j = 0; j < dim; ++j) v[(j + r) % dim] = d[j];
        if (!full)
            for (size_t j = 0; j < r; ++j) { v[dim + j] = v[j]; v[j] = 0; }
    }
    c->w = &c->lanes[0];
    hhe_matrix *m = new hhe_matrix();
    m->ctx = c; m->dim = dim; m->n1 = (int)n1; m->n2 = (int)n2;
    DevBuf dv(vals.size() * 8), plain(dim * n * 8), diag(dim * ln * 8), bv(dim * 8);
    bool ok = dv.p && plain.p && diag.p && bv.p;
    if (ok && !n1) ok = !!(m->tab = (u64 *)rt_malloc(2 * dim * ln * 8));
    if (ok && bias) ok = !!(m->bias = (u64 *)rt_malloc(n * 8));
    if (!ok) { matrix_free(m); return dev_fail("hhe_matrix_create: table alloc"); }
    rt_stream st = c->w->stream;
    rt_h2d(dv.p, vals.data(), vals.size() * 8, st);
    op_encode(c, dv.w(), dim, (int)stride, (int)stride, -1, plain.w());
    op_lift_ntt(c, plain.w(), dim, diag.w());
    if (!n1) {
        // multipliers in the frame of rotate_rows(+1) and their Shoup quotients: the `pdiag` form of build_block
        PermArgs p = perm_args(c, dim * c->L, diag.w(), m->tab, ln);
        p.elt = galois_elt_from_step(c, 1);
        k_perm(p, st);
        op_elt(c, ELT_SHOUP, m->tab, nullptr, m->tab + dim * ln, dim * c->L, 0, c->L);
    }
    if (bias) {
        rt_h2d(bv.p, bias, dim * 8, st);
        op_encode(c, bv.w(), 1, (int)dim, (int)dim, -1, m->bias);
    }
    if (rt_sync(st)) { matrix_free(m); return dev_fail("hhe_matrix_create"); }
    if (n1) m->tab = diag.release();
    m->bytes = (n1 ? 1 : 2) * dim * ln * 8 + (bias ? n * 8 : 0);
    c->mats.push_back(m);
    *out = m;
    return HHE_OK;
}
extern "C" void hhe_matrix_destroy(hhe_matrix *m)
{
    if (!m) return;
    hhe_ctx *c = m->ctx;
    HHE_LOCK(c);
    sync_ctx(c);
    c->mats.erase(std::remove(c->mats.begin(), c->mats.end(), m), c->mats.end());
    matrix_free(m);
}
extern "C" size_t hhe_matrix_bytes(const hhe_matrix *m) { return m ? m->bytes : 0; }

extern "C" int hhe_packed_affine_ks(hhe_ctx *c, const hhe_keyset *gk, const hhe_matrix *mat, const uint64_t *ct, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || !mat || !ct || !out || B == 0) return fail(HHE_ERR_INVALID, "hhe_packed_affine: null argument or empty batch");
    if (mat->ctx != c) return fail(HHE_ERR_INVALID, "matrix belongs to another context");
    int rc = check_sets(c, gk);
    if (rc) return rc;
    KeyScope keys(c, gk, nullptr);
    hhe_matrix *m = const_cast<hhe_matrix *>(mat);
    // every rotation must be servable before anything is written.  Step +1 needs its own key: its NAF is the one term, so SEAL
    // throws without it; the other steps may go through their NAF terms (op_rotate_rows)
    std::vector<int> steps;
    if ((rc = affine_steps(c->n, m->dim, (size_t)m->n1, (size_t)m->n2, steps))) return rc;
    for (int s : steps)
        if (s == 1 ? (m->dim > 1 && !c->gks->gk.count(galois_elt_from_step(c, 1))) : !rot_reachable(c, s)) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
    Lane &main = c->lanes[0];
    c->w = &main;
    const ChunkPlan plan = plan_balanced(c, B);
    const size_t ctw = c->ct_words();
    for (int s = plan.first_lane(); s <= plan.last_lane(); ++s) {
        if ((rc = lane_reserve(c, c->lanes[s], plan.per))) return rc;
        if (m->n1 && (rc = c->lanes[s].ws_aff.reserve(c, (size_t)(m->n1 + m->n2) * plan.per * ctw, "hhe_packed_affine: babystep-giantstep workspace"))) return rc;
    }
    if ((rc = matrix_reserve_self(c, m, plan.per))) return rc;
    rc = run_chunks(c, plan, [&](Lane &, size_t, size_t b0, size_t bc) { return affine_chunk(c, m, ct + b0 * ctw, out + b0 * ctw, bc); });
    if (rt_sync(main.stream) && !rc) rc = dev_fail("hhe_packed_affine");
    return rc;
}

// ====================================================================== hoisted rotations
// hhe_rotate_rows_many_ks and step 2 of hhe_fc_packed_hoisted_ks: many rotate_rows of ONE ciphertext.  The definition is in
// include/hhe_gfx950.h; DESIGN.md section 4 "Hoisted rotations" has the schedule and the workspace.
namespace {
struct RotNode {
    u32 elt = 0;             // Galois element of the key switch that makes the node from its parent
    std::vector<int> kids;   // nodes
    std::vector<int> outs;   // the steps (indices into the call's list) that end here
    size_t kid_ofs = 0;      // first row of the node's children in the call's table (RotPlan::kids)
};
struct RotPlan {
    std::vector<int> steps;
    std::vector<RotNode> trie;   // node 0 is the input itself (step 0 ends there)
    std::vector<KsKid> kids;     // host copy of the per-child table, node after node
    const KsKid *d_kids = nullptr;
    bool rowk = false;           // the row kernels run: children of a node in multi-child launches of ks_perm_row_kernel
    size_t max_kids = 0;
    u64 launches = 0;            // such launches per chunk
    size_t group() const { return std::min<size_t>(std::max<size_t>(max_kids, 1), HHE_ROT_GROUP); }
};
// The term sequences of the steps as Evaluator::rotate_rows takes them from the named set (a step's own key, else its NAF terms with
// +-N/2 skipped) form a trie, as in fc_build_trie; here every node that ends a step is an output.  Host only: nothing is enqueued.
int rot_plan_build(const hhe_ctx *c, const int *steps, size_t n_steps, RotPlan &p)
{
    p.steps.assign(steps, steps + n_steps);
    p.trie.assign(1, RotNode());
    for (size_t k = 0; k < n_steps; ++k)
        if ((size_t)std::abs((long long)steps[k]) >= c->n / 2) return fail(HHE_ERR_INVALID, "step count too large");
    for (size_t k = 0; k < n_steps; ++k) {
        const int step = steps[k];
        std::vector<int> terms;
        if (step != 0) {
            if (c->gks->gk.count(galois_elt_from_step(c, step))) terms.push_back(step);
            else
                for (int t : nt_naf(step))
                    if ((size_t)std::abs(t) != c->n / 2) terms.push_back(t);
        }
        int node = 0;
        for (int t : terms) {
            // children are told apart by their element: two terms that name one element (-1 and N/2 - 1) are the same key switch
            const u32 elt = galois_elt_from_step(c, t);
            if (!c->gks->gk.count(elt)) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
            int next = -1;
            for (int kid : p.trie[node].kids)
                if (p.trie[kid].elt == elt) { next = kid; break; }
            if (next < 0) {
                next = (int)p.trie.size();
                p.trie.push_back(RotNode());
                p.trie[next].elt = elt;
                p.trie[node].kids.push_back(next);
            }
            node = next;
        }
        p.trie[node].outs.push_back((int)k);
    }
    p.rowk = use_row_kernel(c);
    for (const RotNode &nd : p.trie) {
        p.max_kids = std::max(p.max_kids, nd.kids.size());
        if (p.rowk) p.launches += (nd.kids.size() + HHE_ROT_GROUP - 1) / HHE_ROT_GROUP;
    }
    return HHE_OK;
}
// Everything the chunks read that is made once per call, on the main lane before they fork: the correction table of every key of the
// trie (and its Shoup quotients where the row kernels run), and the per-child table on the device
// ofs / total: the plan's rows start at row `ofs` of a table of `total` rows (the layers of hhe_mlp_ks share one table; the caller
// lays the plans out one behind the other, a plan having one row per node below its root); total == 0: the table is this plan's alone
int rot_plan_tables(hhe_ctx *c, RotPlan &p, size_t ofs = 0, size_t total = 0)
{
    int rc;
    p.kids.clear();
    for (RotNode &nd : p.trie) {
        nd.kid_ofs = p.kids.size();
        for (int kid : nd.kids) {
            KsKid kd;
            memset(&kd, 0, sizeof(kd));
            kd.elt = p.trie[kid].elt;
            if (!(kd.key = galois_key(c, kd.elt))) return HHE_ERR_NO_GALOIS_KEY;
            if ((rc = fc_corr(c, kd.elt, kd.key, &kd.corr))) return rc;
            if (p.rowk && (rc = ensure_key_shoup(c, kd.key, &kd.key_s))) return rc;
            p.kids.push_back(kd);
        }
    }
    if (!p.rowk || p.kids.empty()) return HHE_OK;
    if (ensure_qsp_poly(c)) return dev_fail("hoisted rotations: workspace");
    if ((rc = c->d_rot_kids.reserve(c, std::max(total, ofs + p.kids.size()), "hoisted rotations: child table"))) return rc;
    // the earlier call's chunks have completed (the calls are synchronous); the host copy must outlive the upload
    if (rt_h2d(c->d_rot_kids.p + ofs, p.kids.data(), p.kids.size() * sizeof(KsKid), c->w->stream) || rt_sync(c->w->stream)) return dev_fail("hoisted rotations: child table");
    p.d_kids = c->d_rot_kids.p + ofs;
    return HHE_OK;
}
// The children of `node` may be written straight into the output when they land there as one block: the chunk covers the whole stride
// (item b of step k at out + (k * ostride + b) * ct_words with ostride == per) and child i's first step is the first child's first step + i
bool rot_direct(const RotPlan &p, int node, bool whole)
{
    const RotNode &nd = p.trie[node];
    if (!whole || nd.kids.empty()) return false;
    for (size_t i = 0; i < nd.kids.size(); ++i) {
        const RotNode &kd = p.trie[nd.kids[i]];
        if (kd.outs.empty() || (i && kd.outs[0] != p.trie[nd.kids[0]].outs[0] + (int)i)) return false;
    }
    return true;
}
// words of the lane's node arena (Lane::ws_rotm) that the walk below `node` needs for chunks of `per` items
size_t rot_arena_words(const hhe_ctx *c, const RotPlan &p, int node, bool whole, size_t per)
{
    const RotNode &nd = p.trie[node];
    size_t below = 0;
    for (int kid : nd.kids) below = std::max(below, rot_arena_words(c, p, kid, whole, per));
    return (rot_direct(p, node, whole) ? 0 : nd.kids.size() * per * c->ct_words()) + below;
}
// All children of `node` from ONE set of digit transforms of its ciphertext `parent` ([per][2][L][N]), then the walk below them.  Item b of
// step k goes to out + (k * ostride + b) * ct_words.  ws_T holds the node's transforms, ws_d its c0hat, ws_S the sums of one launch's
// children x items: the lane is reserved for group() * per items.
int rot_many_node(hhe_ctx *c, const RotPlan &p, int node, const u64 *parent, u64 *out, size_t ostride, size_t per, u64 *arena)
{
    const RotNode &nd = p.trie[node];
    const size_t m = nd.kids.size(), ctw = c->ct_words(), blk = per * ctw;
    if (!m) return HHE_OK;
    Lane &w = *c->w;
    u64 *dst = arena;
    if (rot_direct(p, node, ostride == per)) dst = out + (size_t)p.trie[nd.kids[0]].outs[0] * ostride * ctw;
    else arena += m * blk;
    fc_parent_digits(c, parent, w.ws_T, per);
    int rc;
    if (p.rowk) {
        op_c0hat(c, parent, w.ws_d, per);
        for (size_t g0 = 0; g0 < m; g0 += HHE_ROT_GROUP) {
            const size_t vb = std::min<size_t>(HHE_ROT_GROUP, m - g0) * per;   // virtual items of this launch: child-major
            const KsSplit sp = ks_split(c, w.ws_S, vb);
            KsRowArgs x = ks_row_args(c, nullptr, nullptr, vb, &sp);
            x.T = w.ws_T; x.c0hat = w.ws_d; x.kids = p.d_kids + nd.kid_ofs + g0; x.kid_B = (int)per;
            if (k_ks_perm_row(ntt_args(c, nullptr, nullptr, 0, 0, c->K), x, w.stream)) return dev_fail("hoisted rotations: key-switch row kernel");
            // galois(c0) is inside S_0 already: one mod-down over all child x item pairs writes the finished ciphertexts
            ks_finish_split(c, sp, ks_ksf_args(c, sp, vb, nullptr, ctw, 1, 0, dst + g0 * blk), vb, false);
        }
    } else {
        for (size_t i = 0; i < m; ++i)
            if ((rc = fc_child_shared(c, parent, w.ws_T, p.kids[nd.kid_ofs + i].elt, nullptr, dst + i * blk, per))) return rc;
    }
    for (size_t i = 0; i < m; ++i)
        for (int k : p.trie[nd.kids[i]].outs) {
            u64 *o = out + (size_t)k * ostride * ctw;
            if (o != dst + i * blk) rt_d2d(o, dst + i * blk, blk * 8, w.stream);
        }
    for (size_t i = 0; i < m; ++i)
        if ((rc = rot_many_node(c, p, nd.kids[i], dst + i * blk, out, ostride, per, arena))) return rc;
    return HHE_OK;
}
// one chunk on the current lane: every step of `per` items of `in`; hoisted, or step by step through op_rotate_rows (HHE_ROT_HOIST=0 and
// the exactness fallback)
int rot_many_chunk(hhe_ctx *c, const RotPlan &p, bool hoisted, const u64 *in, u64 *out, size_t ostride, size_t per)
{
    const size_t ctw = c->ct_words();
    int rc;
    if (!hoisted) {
        for (size_t k = 0; k < p.steps.size(); ++k)
            if ((rc = op_rotate_rows(c, in, p.steps[k], out + k * ostride * ctw, per))) return rc;
        return HHE_OK;
    }
    for (int k : p.trie[0].outs) rt_d2d(out + (size_t)k * ostride * ctw, in, per * ctw * 8, c->w->stream);
    return rot_many_node(c, p, 0, in, out, ostride, per, c->w->ws_rotm.p);
}
// lane workspaces of a chunk of `per` items; hoisted chunks keep the sums of group() children at once
int rot_many_reserve(hhe_ctx *c, Lane &ln, const RotPlan &p, bool hoisted, bool whole, size_t per, size_t lane_items = 0)
{
    int rc = lane_reserve(c, ln, std::max(lane_items, hoisted ? p.group() * per : per));
    if (!rc && hoisted) rc = ln.ws_rotm.reserve(c, rot_arena_words(c, p, 0, whole, per), "hoisted rotations: node ciphertexts");
    return rc;
}
}  // namespace

extern "C" int hhe_rotate_rows_many_ks(hhe_ctx *c, const hhe_keyset *gk, const uint64_t *ct, const int *steps, size_t n_steps, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || !ct || !steps || !out || B == 0 || n_steps == 0) return fail(HHE_ERR_INVALID, "hhe_rotate_rows_many: null argument, empty batch or no step");
    int rc = check_sets(c, gk);
    if (rc) return rc;
    KeyScope keys(c, gk, nullptr);
    const size_t ctw = c->ct_words();
    if (ct < out + n_steps * B * ctw && out < ct + B * ctw) return fail(HHE_ERR_INVALID, "hhe_rotate_rows_many: out overlaps ct");
    RotPlan plan;
    if ((rc = rot_plan_build(c, steps, n_steps, plan))) return rc;
    Lane &main = c->lanes[0];
    c->w = &main;
    const bool hoisted = c->rot_hoist != 0 && plan.trie.size() > 1;
    if (hoisted && (rc = rot_plan_tables(c, plan))) return rc;
    // a chunk keeps the sums of group() children of its items at once: group() * per stays within the HHE_CHUNK items a lane is reserved for elsewhere
    const size_t per = std::min(B, std::max<size_t>(1, c->chunk / plan.group()));
    const ChunkPlan cp(B, per, c->nstreams);
    const bool whole = cp.nch == 1;   // ostride == per
    // a zero residue in some c1: that chunk is recomputed step by step.  out does not overlap ct, so nothing is parked
    rc = run_chunks_checked(c, cp, "hhe_rotate_rows_many", "hhe_rotate_rows_many", hoisted, c->rot_hoist == 2, c->rot_many_fallbacks,
        [&](Lane &ln, bool h) { return rot_many_reserve(c, ln, plan, h, h && whole, per); },
        [&](Lane &, size_t, size_t b0, size_t bc, bool h) {
            // a shorter last chunk of several does not cover the stride: its children go through the arena, which is sized for that
            return rot_many_chunk(c, plan, h, ct + b0 * ctw, out + b0 * ctw, B, bc);
        });
    if (!rc) { c->rot_many_key_switches = plan.trie.size() - 1; c->rot_many_launches = hoisted ? plan.launches : 0; }
    return rc;
}

// ====================================================================== packed encrypted FC (hybrid diagonal method)
// The definition is in include/hhe_gfx950.h; DESIGN.md section 4 "Packed encrypted FC" has the schedule and the workspace.
namespace {
size_t pow2_ceil(size_t v)
{
    size_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
// r and c of a rows x cols layer; n = 0: no degree, no slot rule (the diagonals' layout does not depend on it).  Cyclic: c covers cols,
// and fills the row or leaves room for the copy at -c.  Open (hhe_fc_open_shape): the diagonals do not wrap, so c covers cols + r - 1
// slots; c <= N/2 is the only slot rule
int fc_dims(bool open, size_t n, size_t rows, size_t cols, size_t &r, size_t &cc)
{
    const std::string w = open ? "open FC" : "packed FC";
    if (rows == 0 || cols == 0 || rows > ((size_t)1 << 30) || cols > ((size_t)1 << 30)) return fail(HHE_ERR_INVALID, w + ": rows and cols must be positive (and at most 2^30)");
    if (n && (n < 4 || (n & (n - 1)))) return fail(HHE_ERR_INVALID, w + ": the degree must be a power of two");
    r = pow2_ceil(rows);
    cc = open ? pow2_ceil(cols + r - 1) : std::max(pow2_ceil(cols), r);
    if (n && (open ? cc * 2 > n : cc * 2 != n && cc * 4 > n)) return fail(HHE_ERR_TOO_FEW_SLOTS, "too little slots for matmul implementation!");
    return HHE_OK;
}
// The rotate_rows steps of a layer in the order it takes them (what the *_galois_steps entry points list): -c unless the row is full
// (cyclic only), the steps of the r - 1 rotations, the tail r 2^k < c.  The rotations are all[rot0, rot0 + nrot): 1 .. r-1 of a cyclic
// layer, -1 .. -(r-1) of an open one -- they go into the layer's RotPlan, which serves them as hhe_rotate_rows_many_ks does -- or,
// chained, the one step 1 that is taken r - 1 times.  Every other step needs its own key: its NAF has one term, so
// Evaluator::rotate_rows throws without it
struct FcSteps {
    std::vector<int> all;
    size_t rot0 = 0, nrot = 0;
    size_t own() const { return all.size() - nrot; }
};
FcSteps fc_layer_steps(bool open, bool chained, size_t n, size_t r, size_t cc)
{
    FcSteps s;
    if (!open && cc * 2 != n) s.all.push_back(-(int)cc);
    s.rot0 = s.all.size();
    for (size_t i = 1; i < (chained ? std::min<size_t>(r, 2) : r); ++i) s.all.push_back(open ? -(int)i : (int)i);
    s.nrot = s.all.size() - s.rot0;
    for (size_t t = r; t < cc; t <<= 1) s.all.push_back((int)t);
    return s;
}
// the shape and the step list entry points of both layouts
int fc_shape(const char *who, bool open, size_t N, size_t rows, size_t cols, size_t *r_out, size_t *c_out)
{
    if (!r_out || !c_out || N == 0) return fail(HHE_ERR_INVALID, std::string(who) + ": null argument or no degree");
    size_t r, cc;
    int rc = fc_dims(open, N, rows, cols, r, cc);
    if (rc) return rc;
    *r_out = r; *c_out = cc;
    return HHE_OK;
}
int fc_galois_steps(const char *who, bool open, bool chained, size_t N, size_t rows, size_t cols, int *steps_out, size_t *count)
{
    if (!count || N == 0) return fail(HHE_ERR_INVALID, std::string(who) + ": null argument or no degree");
    size_t r, cc;
    int rc = fc_dims(open, N, rows, cols, r, cc);
    return rc ? rc : steps_out_copy(who, fc_layer_steps(open, chained, N, r, cc).all, steps_out, count);
}
// one chunk on the current lane: in / out [per][2][L][N] (may be the same buffer); the lane is reserved for r * per items
// an open handle (hhe_fc_open_ks): no step 1, and the hoisted plan holds the steps -1 .. -(r-1)
// hoist: step 2 as rotations of the x of step 1 (hhe_fc_packed_hoisted_ks) -- one hoisted rotation of the chunk's items into rot + per * ctw,
// or with `stepwise` each through op_rotate_rows (HHE_ROT_HOIST=0 and the exactness fallback); null: the chain of hhe_fc_packed_ks
// sum: steps 3 and 4 as one multiply_sum (hhe_fc_packed_sum_ks) -- prod is [per][3][L][N] and the sum kernel is not launched
int fc_packed_chunk(hhe_ctx *c, const hhe_enc_matrix *m, const u64 *in, u64 *out, size_t per, const RotPlan *hoist = nullptr, bool stepwise = false,
                    bool sum = false)
{
    const size_t ctw = c->ct_words(), r = m->r;
    Lane &w = *c->w;
    u64 *rot = w.ws_fcp.p, *prod = rot + r * per * ctw;  // [r][per][2][L][N] | [r][per][3][L][N]
    int rc;
    rt_d2d(rot, in, per * ctw * 8, w.stream);
    if (!m->open && m->c * 2 != c->n && (rc = op_prep_rows(c, rot, -(int)m->c, w.ws_ct[2], per))) return rc;
    if (hoist) {
        if (r > 1 && (rc = rot_many_chunk(c, *hoist, !stepwise, rot, rot + per * ctw, per, per))) return rc;
    } else
        for (size_t i = 1; i < r; ++i)
            if ((rc = op_rotate_rows(c, rot + (i - 1) * per * ctw, 1, rot + i * per * ctw, per))) return rc;
    if (sum) op_multiply_sum_enc(c, rot, m, prod, per);
    else op_multiply_enc(c, rot, m, prod, per);
    if (r > 1 && !sum) {  // acc = the sum of the r products of every item, into the first one
        k_elt(elt_args(c, prod, nullptr, prod, per * 3 * c->L, 0, c->L, (int)r), ELT_ADDMANY, w.stream);
        ++c->add_many_launches;
    }
    u64 *y = w.ws_ct[0];
    if ((rc = op_relinearize(c, prod, y, per))) return rc;
    for (size_t s = r; s < m->c; s <<= 1)
        if ((rc = op_prep_rows(c, y, (int)s, w.ws_ct[2], per))) return rc;
    rt_d2d(out, y, per * ctw * 8, w.stream);
    return HHE_OK;
}
}  // namespace

void enc_matrix_free(hhe_enc_matrix *m)
{
    if (!m) return;
    rt_free(m->wq); rt_free(m->wb);
    delete m;
}

extern "C" int hhe_fc_packed_shape(size_t N, size_t rows, size_t cols, size_t *r_out, size_t *c_out)
{
    return fc_shape("hhe_fc_packed_shape", false, N, rows, cols, r_out, c_out);
}
extern "C" int hhe_fc_packed_diagonals(uint64_t t, const uint64_t *M, size_t rows, size_t cols, uint64_t *vals)
{
    if (!M || !vals) return fail(HHE_ERR_INVALID, "hhe_fc_packed_diagonals: null argument");
    size_t r, cc;
    int rc = fc_dims(false, 0, rows, cols, r, cc);
    if (rc) return rc;
    for (size_t i = 0; i < rows * cols; ++i)
        if (M[i] >= t) return fail(HHE_ERR_INVALID, "hhe_fc_packed_diagonals: matrix entry not below the plain modulus");
    // d_i[j] = M[j mod r][(j + i) mod c] of the zero-padded matrix
    for (size_t i = 0; i < r; ++i)
        for (size_t j = 0; j < cc; ++j) {
            const size_t row = j % r, col = (j + i) % cc;
            vals[i * cc + j] = row < rows && col < cols ? M[row * cols + col] : 0;
        }
    return HHE_OK;
}
extern "C" int hhe_fc_packed_galois_steps(size_t N, size_t rows, size_t cols, int *steps_out, size_t *count)
{
    return fc_galois_steps("hhe_fc_packed_galois_steps", false, true, N, rows, cols, steps_out, count);
}

// open: the shape and the mark of hhe_enc_matrix_create_open; the resident form is the same
static int enc_matrix_create(hhe_ctx *c, const uint64_t *wdiag, size_t rows, size_t cols, bool open, hhe_enc_matrix **out)
{
    HHE_LOCK(c);
    if (!c || !wdiag || !out) return fail(HHE_ERR_INVALID, "hhe_enc_matrix_create: null argument");
    size_t r, cc;
    int rc = fc_dims(open, c->n, rows, cols, r, cc);
    if (rc) return rc;
    const size_t n = c->n, L = c->L;
    hhe_enc_matrix *m = new hhe_enc_matrix();
    m->ctx = c; m->rows = rows; m->cols = cols; m->r = r; m->c = cc; m->open = open;
    m->wq = (u64 *)rt_malloc(r * 2 * L * n * 8);
    m->wb = (u64 *)rt_malloc(r * 2 * (L + 1) * n * 8);
    if (!m->wq || !m->wb) { enc_matrix_free(m); return dev_fail("hhe_enc_matrix_create: table alloc"); }
    c->w = &c->lanes[0];
    op_behz_operand(c, wdiag, m->wq, m->wb, r);
    if (rt_sync(c->w->stream)) { enc_matrix_free(m); return dev_fail("hhe_enc_matrix_create"); }
    m->bytes = r * 2 * (2 * L + 1) * n * 8;
    c->enc_mats.push_back(m);
    *out = m;
    return HHE_OK;
}
extern "C" int hhe_enc_matrix_create(hhe_ctx *c, const uint64_t *wdiag, size_t rows, size_t cols, hhe_enc_matrix **out)
{
    return enc_matrix_create(c, wdiag, rows, cols, false, out);
}
extern "C" int hhe_enc_matrix_create_open(hhe_ctx *c, const uint64_t *wdiag, size_t rows, size_t cols, hhe_enc_matrix **out)
{
    return enc_matrix_create(c, wdiag, rows, cols, true, out);
}
extern "C" void hhe_enc_matrix_destroy(hhe_enc_matrix *m)
{
    if (!m) return;
    hhe_ctx *c = m->ctx;
    HHE_LOCK(c);
    sync_ctx(c);
    c->enc_mats.erase(std::remove(c->enc_mats.begin(), c->enc_mats.end(), m), c->enc_mats.end());
    enc_matrix_free(m);
}
extern "C" size_t hhe_enc_matrix_bytes(const hhe_enc_matrix *m) { return m ? m->bytes : 0; }

// what a chunk keeps on its lane: the r rotations of its items and their r size-3 products, or with `sum` the one summed product
static size_t fc_packed_words(const hhe_ctx *c, const hhe_enc_matrix *m, size_t per, bool sum)
{
    return (m->r * 2 + (sum ? 1 : m->r) * 3) * per * (size_t)c->L * c->n;
}
// one chunk of a call on the current lane: every layer of `per` items, a square and a relinearization between two layers, with no host
// wait in between.  x_k lives in the lane's ws_ct[1] and the size-3 square in ws_ct3, which no step of a layer touches; the lane's
// ws_fcp is reserved for the largest layer.  plans: one RotPlan per layer, or null for the chain of hhe_fc_packed_ks
static int mlp_chunk(hhe_ctx *c, const hhe_enc_matrix *const *mats, size_t n_layers, const RotPlan *plans, const u64 *in, u64 *out, size_t per,
                     bool stepwise, bool sum)
{
    Lane &w = *c->w;
    u64 *x = w.ws_ct[1];
    int rc;
    for (size_t k = 0; k < n_layers; ++k) {
        const bool last = k + 1 == n_layers;
        if ((rc = fc_packed_chunk(c, mats[k], k ? x : in, last ? out : x, per, plans ? &plans[k] : nullptr, stepwise, sum))) return rc;
        if (last) break;
        op_square(c, x, w.ws_ct3, per);
        if ((rc = op_relinearize(c, w.ws_ct3, x, per))) return rc;
    }
    return HHE_OK;
}
// What tells the packed encrypted layer calls apart.  `who` names the entry point in messages; the calls on cyclic handles keep the
// texts they had as separate drivers
struct FcForm {
    bool open;     // open handles (hhe_enc_matrix_create_open), any number of layers, always summed; else ONE cyclic handle
    bool chained;  // step 2 as the chain of r - 1 rotations by 1: no RotPlan, nothing optimistic; else the hoisted rotations of the plan
    bool sum;      // steps 3 and 4 as one multiply_sum
    const char *who;
};
// hhe_fc_packed_ks, hhe_fc_packed_hoisted_ks, hhe_fc_packed_sum_ks, hhe_fc_open_ks and hhe_mlp_ks: the first four are one-layer cases
static int fc_layers_run(hhe_ctx *c, const FcForm &f, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *const *mats, size_t n_layers,
                         const uint64_t *vi, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    const std::string w(f.who);
    if (!c || !mats || !vi || !out || B == 0 || n_layers == 0 || (!f.open && !mats[0]))
        return fail(HHE_ERR_INVALID, w + (f.open ? ": null argument, empty batch or no layer" : ": null argument or empty batch"));
    size_t max_r = 1;
    for (size_t k = 0; k < n_layers; ++k) {
        const hhe_enc_matrix *m = mats[k];
        if (!m) return fail(HHE_ERR_INVALID, w + ": null handle");
        if (m->ctx != c) return fail(HHE_ERR_INVALID, "encrypted matrix belongs to another context");
        if (f.open && !m->open) return fail(HHE_ERR_INVALID, w + ": a cyclic handle (hhe_enc_matrix_create) takes the hhe_fc_packed calls");
        if (!f.open && m->open) return fail(HHE_ERR_INVALID, "hhe_fc_packed: an open handle (hhe_enc_matrix_create_open) takes hhe_fc_open_ks or hhe_mlp_ks");
        if (k && mats[k - 1]->rows != m->cols) return fail(HHE_ERR_INVALID, w + ": rows of a layer differ from cols of the next");
        if (f.sum && m->r >= 2 && m->r > c->behz_sum_cap)
            return fail(HHE_ERR_INVALID, (f.open ? w : "hhe_fc_packed_sum") + ": more diagonals than one floor takes (behz_sum_cap)");
        max_r = std::max(max_r, m->r);
    }
    int rc = check_sets(c, rk, gk);
    if (rc) return rc;
    KeyScope keys(c, gk, rk);
    // everything the layers need, before anything is written: the relinearization key, every step's own key, and the plans of all
    // layers, which refuse a rotation that the named set cannot serve (rot_plan_build is host only)
    if (!c->rks->rk) return fail(HHE_ERR_NO_RELIN_KEY, "relinearization key not set");
    std::vector<RotPlan> plans(n_layers);
    auto hoisted = [&](size_t k) { return !f.chained && c->rot_hoist != 0 && mats[k]->r > 1; };
    size_t kid_rows = 0, key_switches = 0, rot_ks = 0, layer_ks = 0;   // rot_ks, layer_ks: of the last layer
    bool any_hoisted = false;
    for (size_t k = 0; k < n_layers; ++k) {
        const FcSteps s = fc_layer_steps(f.open, f.chained, c->n, mats[k]->r, mats[k]->c);
        for (size_t i = 0; i < s.all.size(); ++i)
            if ((f.chained || i < s.rot0 || i >= s.rot0 + s.nrot) && !c->gks->gk.count(galois_elt_from_step(c, s.all[i])))
                return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
        rot_ks = f.chained ? mats[k]->r - 1 : 0;
        if (!f.chained && s.nrot) {
            if ((rc = rot_plan_build(c, s.all.data() + s.rot0, s.nrot, plans[k]))) return rc;
            kid_rows += rot_ks = plans[k].trie.size() - 1;
        }
        key_switches += layer_ks = s.own() + rot_ks;
        any_hoisted |= hoisted(k);
    }
    Lane &main = c->lanes[0];
    c->w = &main;
    // the layers share one child table: the plans lie one behind the other, a plan having one row per node below its root
    for (size_t k = 0, ofs = 0; k < n_layers; ++k)
        if (hoisted(k)) {
            if ((rc = rot_plan_tables(c, plans[k], ofs, kid_rows))) return rc;
            ofs += plans[k].trie.size() - 1;
        }
    // a chunk runs the BEHZ passes of its r * per products at once: r * per stays within the HHE_CHUNK items a lane is reserved for elsewhere
    const size_t per = std::min(B, std::max<size_t>(1, c->chunk / max_r));
    const ChunkPlan cp(B, per, c->nstreams);
    const size_t ctw = c->ct_words();
    Parked park{vi, out, ctw, f.open ? "hhe_mlp: results in place" : "hhe_fc_packed_hoisted: results in place", out};
    // one flag per chunk, for the hoisted rotations of every layer; a flagged chunk is recomputed whole, from vi, step by step
    rc = run_chunks_checked(c, cp, f.who, f.open ? "hhe_mlp" : "hhe_fc_packed_hoisted", any_hoisted, c->rot_hoist == 2, c->rot_many_fallbacks,
        [&](Lane &ln, bool h) {
            int r = HHE_OK;
            size_t words = 0;
            for (size_t k = 0; k < n_layers && !r; ++k) {
                r = rot_many_reserve(c, ln, plans[k], h && hoisted(k), true, per, max_r * per);
                words = std::max(words, fc_packed_words(c, mats[k], per, f.sum));
            }
            if (!r) r = ln.ws_fcp.reserve(c, words, f.open ? "hhe_mlp: rotations and products of the largest layer" : "hhe_fc_packed: rotations and products");
            return r;
        },
        [&](Lane &, size_t, size_t b0, size_t bc, bool h) {
            return mlp_chunk(c, mats, n_layers, f.chained ? nullptr : plans.data(), vi + b0 * ctw, park.res + b0 * ctw, bc, !h, f.sum);
        }, &park);
    if (rc) return rc;
    const size_t last = n_layers - 1;
    if (!f.chained) {
        c->rot_many_key_switches = rot_ks;
        c->rot_many_launches = hoisted(last) ? plans[last].launches : 0;
    }
    c->fc_packed_key_switches = layer_ks;
    c->fc_packed_floors = f.sum ? 3 : 3 * mats[last]->r;
    if (f.open) { c->mlp_layers = n_layers; c->mlp_key_switches = key_switches; }
    return HHE_OK;
}
extern "C" int hhe_fc_packed_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *m, const uint64_t *vi,
                                uint64_t *out, size_t B)
{
    return fc_layers_run(c, {false, true, false, "hhe_fc_packed"}, rk, gk, &m, 1, vi, out, B);
}
extern "C" int hhe_fc_packed_hoisted_galois_steps(size_t N, size_t rows, size_t cols, int *steps_out, size_t *count)
{
    return fc_galois_steps("hhe_fc_packed_hoisted_galois_steps", false, false, N, rows, cols, steps_out, count);
}
extern "C" int hhe_fc_packed_hoisted_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *m, const uint64_t *vi,
                                        uint64_t *out, size_t B)
{
    return fc_layers_run(c, {false, false, false, "hhe_fc_packed_hoisted"}, rk, gk, &m, 1, vi, out, B);
}
extern "C" int hhe_fc_packed_sum_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *m, const uint64_t *vi,
                                    uint64_t *out, size_t B, int hoisted)
{
    return fc_layers_run(c, {false, !hoisted, true, hoisted ? "hhe_fc_packed_hoisted" : "hhe_fc_packed"}, rk, gk, &m, 1, vi, out, B);
}

// ====================================================================== open packed FC and the FC-square-FC network
// The definition is in include/hhe_gfx950.h; DESIGN.md section 4 "Open diagonals and the network call" has the layout and the chunk.
extern "C" int hhe_fc_open_shape(size_t N, size_t rows, size_t cols, size_t *r_out, size_t *c_out)
{
    return fc_shape("hhe_fc_open_shape", true, N, rows, cols, r_out, c_out);
}
extern "C" int hhe_fc_open_diagonals(uint64_t t, const uint64_t *M, size_t rows, size_t cols, uint64_t *vals)
{
    if (!M || !vals) return fail(HHE_ERR_INVALID, "hhe_fc_open_diagonals: null argument");
    size_t r, cc;
    int rc = fc_dims(true, 0, rows, cols, r, cc);
    if (rc) return rc;
    for (size_t i = 0; i < rows * cols; ++i)
        if (M[i] >= t) return fail(HHE_ERR_INVALID, "hhe_fc_open_diagonals: matrix entry not below the plain modulus");
    // D_e[j] = M[j mod r][j - e] where that entry exists, else 0: no index wraps
    for (size_t e = 0; e < r; ++e)
        for (size_t j = 0; j < cc; ++j) {
            const size_t row = j % r;
            vals[e * cc + j] = row < rows && j >= e && j - e < cols ? M[row * cols + (j - e)] : 0;
        }
    return HHE_OK;
}
extern "C" int hhe_fc_open_galois_steps(size_t N, size_t rows, size_t cols, int *steps_out, size_t *count)
{
    return fc_galois_steps("hhe_fc_open_galois_steps", true, false, N, rows, cols, steps_out, count);
}
extern "C" int hhe_fc_open_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *m, const uint64_t *vi, uint64_t *out,
                              size_t B)
{
    if (!m) return fail(HHE_ERR_INVALID, "hhe_fc_open: null argument");
    return fc_layers_run(c, {true, false, true, "hhe_fc_open"}, rk, gk, &m, 1, vi, out, B);
}
extern "C" int hhe_mlp_ks(hhe_ctx *c, const hhe_keyset *rk, const hhe_keyset *gk, const hhe_enc_matrix *const *mats, size_t n_layers,
                          const uint64_t *vi, uint64_t *out, size_t B)
{
    return fc_layers_run(c, {true, false, true, "hhe_mlp"}, rk, gk, mats, n_layers, vi, out, B);
}

// ====================================================================== plain-weights sum of rotations and the open layer on it
// hhe_rotate_plain_sum_ks and hhe_fc_open_plain_ks.  The definition is in include/hhe_gfx950.h; DESIGN.md section 4 "Plain-weights FC"
// has the schedule and the workspace.
void plain_rows_free(hhe_plain_rows *p)
{
    if (!p) return;
    rt_free(p->tab); p->self.release();
    delete p;
}
void plain_fc_free(hhe_plain_fc *m)
{
    if (!m) return;
    plain_rows_free(m->diag); rt_free(m->bias);
    delete m;
}
namespace {
// vals [n][count] host slot values -> a handle that is not yet registered with the context
int plain_rows_make(hhe_ctx *c, const char *who, const uint64_t *vals, size_t n, size_t count, hhe_plain_rows **out)
{
    const std::string w(who);
    if (n == 0 || count == 0 || count > c->n || n > ((size_t)1 << 20)) return fail(HHE_ERR_INVALID, w + ": no plaintext, or more slot values than slots");
    for (size_t i = 0; i < n * count; ++i)
        if (vals[i] >= c->t) return fail(HHE_ERR_INVALID, w + ": slot value not below the plain modulus");
    const size_t N = c->n, K = c->K;
    c->w = &c->lanes[0];
    hhe_plain_rows *p = new hhe_plain_rows();
    p->ctx = c; p->count = n;
    DevBuf dv(n * count * 8), plain(n * N * 8);
    p->tab = (u64 *)rt_malloc(2 * n * K * N * 8);
    if (!dv.p || !plain.p || !p->tab) { plain_rows_free(p); return dev_fail((w + ": table alloc").c_str()); }
    rt_stream st = c->w->stream;
    rt_h2d(dv.p, vals, n * count * 8, st);
    op_encode(c, dv.w(), n, (int)count, (int)count, -1, plain.w());
    // the lift of op_lift_ntt under every prime of the context, the special one included
    NttArgs a = ntt_args(c, plain.w(), p->tab, n * K, 0, (int)K);
    a.src_div = (int)K; a.load_op = LOAD_LIFT;
    k_ntt(a, false, st);
    op_elt(c, ELT_SHOUP, p->tab, nullptr, p->tab + n * K * N, n * K, 0, (int)K);
    if (rt_sync(st)) { plain_rows_free(p); return dev_fail(who); }
    p->bytes = 2 * n * K * N * 8;
    *out = p;
    return HHE_OK;
}
// the per-item pointer array k_perm takes, all entries the handle's table (matrix_reserve_self)
int plain_rows_reserve_self(hhe_ctx *c, hhe_plain_rows *p, size_t per)
{
    bool grew = false;
    int rc = p->self.reserve(c, per, "hhe_rotate_plain_sum: pointer table", &grew);
    if (rc || !grew) return rc;
    rt_stream st = c->lanes[0].stream;
    std::vector<const u64 *> h(p->self.cap, p->tab);
    if (rt_h2d((void *)p->self.p, h.data(), h.size() * sizeof(u64 *), st) || rt_sync(st)) {
        rc = dev_fail("hhe_rotate_plain_sum: pointer table");
        p->self.release();
        return rc;
    }
    return HHE_OK;
}
struct PlainSumPlan {
    hhe_plain_rows *rows = nullptr;
    std::vector<int> steps;      // pair k: rotate_rows by steps[k], times plaintext k
    std::vector<KsKid> kids;     // row k: the key, tables and element of pair k (step 0: element 1, step0 set, no key)
    const KsKid *d_kids = nullptr;
    bool rowk = false, any_rot = false, any_zero = false;
    std::vector<int> tail;       // the layer: y += rotate_rows(y, s) for s in tail, then + bias
    const u64 *bias = nullptr;
};
// host only: every step valid and every non-zero step (tail included) with a key of its own in the named set
int plain_sum_plan(const hhe_ctx *c, const int *steps, size_t n, PlainSumPlan &p)
{
    p.steps.assign(steps, steps + n);
    p.kids.assign(n, zeroed<KsKid>());
    for (size_t k = 0; k < n; ++k)
        if ((size_t)std::abs((long long)steps[k]) >= c->n / 2) return fail(HHE_ERR_INVALID, "step count too large");
    auto own_key = [&](int step) { return c->gks->gk.count(galois_elt_from_step(c, step)) != 0; };
    for (size_t k = 0; k < n; ++k) {
        KsKid &kd = p.kids[k];
        if (steps[k] == 0) { kd.elt = 1; kd.step0 = 1; p.any_zero = true; continue; }
        if (!own_key(steps[k])) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
        kd.elt = galois_elt_from_step(c, steps[k]);
        p.any_rot = true;
    }
    for (int s : p.tail)
        if (!own_key(s)) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
    p.rowk = use_row_kernel(c);
    return HHE_OK;
}
// what the chunks read that is made once per call, on the main lane before they fork (rot_plan_tables)
int plain_sum_tables(hhe_ctx *c, PlainSumPlan &p, size_t per)
{
    int rc;
    for (KsKid &kd : p.kids) {
        if (kd.step0) continue;
        if (!(kd.key = galois_key(c, kd.elt))) return HHE_ERR_NO_GALOIS_KEY;
        if ((rc = fc_corr(c, kd.elt, kd.key, &kd.corr))) return rc;
        if (p.rowk && (rc = ensure_key_shoup(c, kd.key, &kd.key_s))) return rc;
    }
    if (ensure_qsp_poly(c)) return dev_fail("hhe_rotate_plain_sum: workspace");
    if ((rc = plain_rows_reserve_self(c, p.rows, per))) return rc;
    if (!p.rowk) return HHE_OK;
    if ((rc = c->d_rot_kids.reserve(c, p.kids.size(), "hhe_rotate_plain_sum: child table"))) return rc;
    if (rt_h2d(c->d_rot_kids.p, p.kids.data(), p.kids.size() * sizeof(KsKid), c->w->stream) || rt_sync(c->w->stream)) return dev_fail("hhe_rotate_plain_sum: child table");
    p.d_kids = c->d_rot_kids.p;
    return HHE_OK;
}
// The primitive for one chunk on the current lane, reserved for 2 * per items: in / out [per][2][L][N].  ws_d holds c0hat | the rotated c1
// of the exact form, ws_ct[2] c1hat (step 0), ws_T the digit transforms, ws_S the sums of one child | the sums over the children, both
// split as the fused finish reads them.
//   fast, row kernels: shared digits, ONE launch of ks_plain_sum_row_kernel, the finish.
//   fast, elsewhere:   shared digits; per child the inner product through the map (ks_mac_kernel, KS_PERM) and the products by its plaintext.
//   exact:             per child the digits of the rotated c1 itself, the plain inner product, the same products.
// The last two end in one inverse transform of the 2K sums and the same finish.  out may be in: nothing reads `in` after the sums
int plain_sum_chunk(hhe_ctx *c, const PlainSumPlan &p, const u64 *in, u64 *out, size_t per, bool fast)
{
    Lane &w = *c->w;
    const int L = c->L, K = c->K;
    const size_t n = c->n, ln = (size_t)L * n, ctw = c->ct_words(), nk = p.steps.size();
    u64 *c0hat = w.ws_d, *rot1 = w.ws_d + per * ln, *c1hat = w.ws_ct[2];
    u64 *S = w.ws_S, *acc = w.ws_S + per * 2 * K * n;
    const KsSplit ss = ks_split(c, S, per), sa = ks_split(c, acc, per);
    op_c0hat(c, in, c0hat, per);
    if (p.any_zero) op_c0hat(c, in + ln, c1hat, per);
    if (fast && p.any_rot) fc_parent_digits(c, in, w.ws_T, per);
    const NttArgs ksf = ks_ksf_args(c, sa, per, nullptr, ctw, 1, 0, out);
    if (fast && p.rowk) {
        KsRowArgs x = ks_row_args(c, nullptr, nullptr, per, &sa);
        x.T = w.ws_T; x.c0hat = c0hat; x.c1hat = c1hat; x.kids = p.d_kids; x.kid_B = (int)per; x.n_kids = (int)nk;
        x.plain = p.rows->tab; x.plain_s_off = p.rows->s_off();
        if (k_ks_perm_row(ntt_args(c, nullptr, nullptr, 0, 0, K), x, w.stream)) return dev_fail("hhe_rotate_plain_sum: key-switch row kernel");
        ks_finish_split(c, sa, ksf, per, false);
        return HHE_OK;
    }
    rt_memset(acc, 0, per * 2 * K * n * 8, w.stream);
    for (size_t k = 0; k < nk; ++k) {
        const KsKid &kd = p.kids[k];
        const u64 *D = p.rows->tab + k * K * n;
        // q_sp * NTT(galois(c0)) times the plaintext into the first sum (for step 0 also c1 into the second)
        PermArgs pa = perm_args(c, per * L, c0hat, sa.W, 2 * ln);
        pa.elt = kd.elt; pa.mac = 1; pa.mul_ptrs = p.rows->self.p; pa.mul_shift = k * K * n;
        k_perm(pa, w.stream);
        if (kd.step0) {
            pa.in = c1hat; pa.out = sa.W + ln;
            k_perm(pa, w.stream);
            continue;
        }
        KsMacArgs m = ks_mac_args(c, w.ws_T, kd.key, S, per);
        m.S_sp = ss.Usp;
        if (fast) { m.perm_elt = kd.elt; m.corr = kd.corr; }
        else {
            k_galois(galois_args(c, per, galois_einv(c, kd.elt), in + ln, 2 * ln, rot1, ln), w.stream);
            k_ntt(ks_digit_args(c, rot1, ln, w.ws_T, per), false, w.stream);
        }
        k_ks_mac(m, w.stream);
        k_elt(elt_args(c, ss.W, D, sa.W, per * 2 * L, 0, L, L), ELT_MAC, w.stream);
        k_elt(elt_args(c, ss.Usp, D + (size_t)(K - 1) * n, sa.Usp, per * 2, K - 1, 1, 1), ELT_MAC, w.stream);
    }
    ks_finish_split(c, sa, ksf, per, true);
    return HHE_OK;
}
// the primitive, and with a tail or a bias the layer built on it: one driver over the checked chunks
int plain_sum_run(hhe_ctx *c, const char *who, const hhe_keyset *gk, PlainSumPlan &p, const int *steps, size_t n, const u64 *in, u64 *out, size_t B)
{
    int rc = check_sets(c, gk);
    if (rc) return rc;
    KeyScope keys(c, gk, nullptr);
    if ((rc = plain_sum_plan(c, steps, n, p))) return rc;
    Lane &main = c->lanes[0];
    c->w = &main;
    // a lane holds the sums of one child and the sums over the children of its items (ws_S), c0hat and one rotated c1 (ws_d): 2 * per
    // stays within the HHE_CHUNK items a lane is reserved for elsewhere
    const size_t per = std::min(B, std::max<size_t>(1, c->chunk / 2));
    if ((rc = plain_sum_tables(c, p, per))) return rc;
    const ChunkPlan cp(B, per, c->nstreams);
    const size_t ctw = c->ct_words();
    const bool fast = c->rot_hoist != 0, layer = !p.tail.empty() || p.bias;
    Parked park{in, out, ctw, "hhe_rotate_plain_sum: results in place", out};
    rc = run_chunks_checked(c, cp, who, "hhe_rotate_plain_sum", fast, c->rot_hoist == 2, c->plain_sum_fallbacks,
        [&](Lane &ln, bool) { return lane_reserve(c, ln, 2 * per); },
        [&](Lane &ln, size_t, size_t b0, size_t bc, bool f) -> int {
            u64 *res = park.res + b0 * ctw;
            if (!layer) return plain_sum_chunk(c, p, in + b0 * ctw, res, bc, f);
            u64 *y = ln.ws_ct[0];
            int r = plain_sum_chunk(c, p, in + b0 * ctw, y, bc, f);
            for (size_t i = 0; i < p.tail.size() && !r; ++i) r = op_prep_rows(c, y, p.tail[i], ln.ws_ct[1], bc);
            if (r) return r;
            if (p.bias) op_add_plain(c, y, p.bias, nullptr, 0, true, false, false, res, bc);
            else rt_d2d(res, y, bc * ctw * 8, ln.stream);
            return HHE_OK;
        }, &park);
    if (!rc) { c->plain_sum_launches = fast && p.rowk ? 1 : 0; c->plain_sum_mod_downs = 1; }
    return rc;
}
}  // namespace

extern "C" int hhe_plain_rows_create(hhe_ctx *c, const uint64_t *vals, size_t n, size_t count, hhe_plain_rows **out)
{
    HHE_LOCK(c);
    if (!c || !vals || !out) return fail(HHE_ERR_INVALID, "hhe_plain_rows_create: null argument");
    hhe_plain_rows *p = nullptr;
    int rc = plain_rows_make(c, "hhe_plain_rows_create", vals, n, count, &p);
    if (rc) return rc;
    c->plain_rows.push_back(p);
    *out = p;
    return HHE_OK;
}
extern "C" void hhe_plain_rows_destroy(hhe_plain_rows *p)
{
    if (!p) return;
    hhe_ctx *c = p->ctx;
    HHE_LOCK(c);
    sync_ctx(c);
    c->plain_rows.erase(std::remove(c->plain_rows.begin(), c->plain_rows.end(), p), c->plain_rows.end());
    plain_rows_free(p);
}
extern "C" size_t hhe_plain_rows_bytes(const hhe_plain_rows *p) { return p ? p->bytes : 0; }
extern "C" int hhe_rotate_plain_sum_ks(hhe_ctx *c, const hhe_keyset *gk, const hhe_plain_rows *rows, const int *steps, size_t n,
                                       const uint64_t *ct, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || !rows || !steps || !ct || !out || B == 0 || n == 0) return fail(HHE_ERR_INVALID, "hhe_rotate_plain_sum: null argument, empty batch or no pair");
    if (rows->ctx != c) return fail(HHE_ERR_INVALID, "plain rows belong to another context");
    if (n > rows->count) return fail(HHE_ERR_INVALID, "hhe_rotate_plain_sum: more pairs than the handle has plaintexts");
    PlainSumPlan p;
    p.rows = const_cast<hhe_plain_rows *>(rows);
    return plain_sum_run(c, "hhe_rotate_plain_sum", gk, p, steps, n, ct, out, B);
}

extern "C" int hhe_plain_fc_create_open(hhe_ctx *c, const uint64_t *M, size_t rows, size_t cols, const uint64_t *bias, hhe_plain_fc **out)
{
    HHE_LOCK(c);
    if (!c || !M || !out) return fail(HHE_ERR_INVALID, "hhe_plain_fc_create_open: null argument");
    size_t r, cc;
    int rc = fc_dims(true, c->n, rows, cols, r, cc);
    if (rc) return rc;
    for (size_t i = 0; bias && i < rows; ++i)
        if (bias[i] >= c->t) return fail(HHE_ERR_INVALID, "hhe_plain_fc_create_open: bias entry not below the plain modulus");
    std::vector<u64> vals(r * cc);
    if ((rc = hhe_fc_open_diagonals(c->t, M, rows, cols, vals.data()))) return rc;
    hhe_plain_fc *m = new hhe_plain_fc();
    m->ctx = c; m->rows = rows; m->cols = cols; m->r = r; m->c = cc;
    for (size_t e = 0; e < r; ++e) m->steps.push_back(-(int)e);
    if ((rc = plain_rows_make(c, "hhe_plain_fc_create_open", vals.data(), r, cc, &m->diag))) { plain_fc_free(m); return rc; }
    if (bias) {
        DevBuf bv(rows * 8);
        m->bias = (u64 *)rt_malloc(c->n * 8);
        if (!bv.p || !m->bias) { plain_fc_free(m); return dev_fail("hhe_plain_fc_create_open: table alloc"); }
        rt_stream st = c->w->stream;
        rt_h2d(bv.p, bias, rows * 8, st);
        op_encode(c, bv.w(), 1, (int)rows, (int)rows, -1, m->bias);
        if (rt_sync(st)) { plain_fc_free(m); return dev_fail("hhe_plain_fc_create_open"); }
    }
    m->bytes = m->diag->bytes + (bias ? c->n * 8 : 0);
    c->plain_fcs.push_back(m);
    *out = m;
    return HHE_OK;
}
extern "C" void hhe_plain_fc_destroy(hhe_plain_fc *m)
{
    if (!m) return;
    hhe_ctx *c = m->ctx;
    HHE_LOCK(c);
    sync_ctx(c);
    c->plain_fcs.erase(std::remove(c->plain_fcs.begin(), c->plain_fcs.end(), m), c->plain_fcs.end());
    plain_fc_free(m);
}
extern "C" size_t hhe_plain_fc_bytes(const hhe_plain_fc *m) { return m ? m->bytes : 0; }
extern "C" int hhe_fc_open_plain_ks(hhe_ctx *c, const hhe_keyset *gk, const hhe_plain_fc *mat, const uint64_t *vi, uint64_t *out, size_t B)
{
    HHE_LOCK(c);
    if (!c || !mat || !vi || !out || B == 0) return fail(HHE_ERR_INVALID, "hhe_fc_open_plain: null argument or empty batch");
    if (mat->ctx != c) return fail(HHE_ERR_INVALID, "plain matrix belongs to another context");
    PlainSumPlan p;
    p.rows = mat->diag;
    for (size_t s = mat->r; s < mat->c; s <<= 1) p.tail.push_back((int)s);
    p.bias = mat->bias;
    return plain_sum_run(c, "hhe_fc_open_plain", gk, p, mat->steps.data(), mat->steps.size(), vi, out, B);
}

extern "C" int hhe_add_many(hhe_ctx *c, const uint64_t *in, size_t K, uint64_t *out, size_t B, int size)
{
    HHE_LOCK(c);
    if (!c || !in || !out || K == 0 || B == 0 || size < 2 || size > 3) return fail(HHE_ERR_INVALID, "hhe_add_many: bad arguments");
    const size_t polys = B * size * c->L;
    if (K > 0x7fffffff || polys > ((size_t)0x7fffffff >> (c->logn - 1))) return fail(HHE_ERR_INVALID, "hhe_add_many: batch too large");
    c->w = &c->lanes[0];
    k_elt(elt_args(c, in, nullptr, out, polys, 0, c->L, (int)K), ELT_ADDMANY, c->w->stream);
    ++c->add_many_launches;
    return HHE_OK;
}

// hhe_internal.h -- host-side context of libhhe_gfx950.so (not part of the C ABI).
#pragma once
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "hhe_common.h"
#include "hhe_launch.h"
#include "hhe_kscache.h"
#include "../../include/hhe_gfx950.h"

struct hhe_ctx;
void hhe_set_error(const std::string &msg);
void sync_ctx(hhe_ctx *c);  // waits for every stream of the context

struct DevBuf {  // scoped device allocation (freed on every exit path unless released)
    void *p = nullptr;
    explicit DevBuf(size_t bytes) { p = rt_malloc(bytes ? bytes : 8); }
    ~DevBuf() { if (p) rt_free(p); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    u64 *w() const { return (u64 *)p; }
    u64 *release() { u64 *r = (u64 *)p; p = nullptr; return r; }
};
// Grow-only device workspace of a context, a lane or a handle; `cap` counts elements of T.  A request within the capacity costs
// nothing.  Growth waits for every stream of the context (something in flight may still read the old buffer), frees, allocates;
// when the allocation fails the buffer is left empty ({nullptr, 0}), so the next request of any size allocates again.
template <class T> struct GrowBuf {
    T *p = nullptr;
    size_t cap = 0;
    // HHE_OK, or HHE_ERR_DEVICE with the error text "<what>: <runtime message>"; *grew: the buffer is a new one (contents undefined)
    int reserve(hhe_ctx *c, size_t count, const char *what, bool *grew = nullptr)
    {
        if (grew) *grew = false;
        if (count <= cap) return HHE_OK;
        sync_ctx(c);
        release();
        if (!(p = (T *)rt_malloc(count * sizeof(T)))) {
            hhe_set_error(std::string(what) + ": " + rt_last_error());
            return HHE_ERR_DEVICE;
        }
        cap = count;
        if (grew) *grew = true;
        return HHE_OK;
    }
    void release() { rt_free((void *)p); p = nullptr; cap = 0; }  // the caller has waited for the readers
};

// Grow-only host staging of a context: page-locked where the runtime offers it (rt_host_malloc), else from malloc; `cap` counts words.
// The caller has waited for every copy that reads the old block before it grows (GrowBuf's rule; contents are not kept).
struct HostStage {
    u64 *p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    int reserve(hhe_ctx *c, size_t words, const char *what)
    {
        if (words <= cap) return HHE_OK;
        sync_ctx(c);
        release();
        pinned = rt_host_malloc && rt_host_free;
        p = (u64 *)(pinned ? rt_host_malloc(words * 8) : malloc(words * 8));
        if (!p) { hhe_set_error(std::string(what) + ": host staging allocation failed"); return HHE_ERR_DEVICE; }
        cap = words;
        return HHE_OK;
    }
    void release()
    {
        if (p) { if (pinned) rt_host_free(p); else free(p); }
        p = nullptr; cap = 0;
    }
};

struct BlockTables {   // public per-(nonce, block index) data of one PASTA block, device resident
    u64 *diag = nullptr;  // [4][128][L][N] lifted + NTT'd diagonals (multiply_plain operands)
    u64 *rc = nullptr;    // [4][N] round-constant plaintexts (coefficients mod t)
    u64 *pdiag = nullptr; // diag composed with the NTT-domain index map of rotate_rows(-1): pdiag[x] = diag[pi(x)]
    u64 *bsgs = nullptr;  // [4][128][L][N] babystep-giantstep variant of diag (lazy)
    size_t bytes = 0;     // device footprint of this entry
    u64 last_call = 0;    // the transciphering call that used it last (block_call): entries of the running call are never evicted
};

constexpr int HHE_MAX_STREAMS = 4;
constexpr int HHE_RELIN_SLOTS = 4;
// One seal::RelinKeys / seal::GaloisKeys object with its identity: the reference's CSP holds several made by the same key
// generator with different randomness (analyst_he_gk with all default elements, csp_he_gk with the flatten steps, two RelinKeys;
// Analyst.cpp:62-94) and names the one it uses at every call (CSP.cpp:238-242, 271-278, 306, 312-316); which keys a rotation
// finds decides both its NAF decomposition and the ciphertext words.  Tables derived from a key live with the set (gk_corr) or
// are keyed by the key's device address (hhe_ctx::d_key_shoup), so two sets never share one.
struct hhe_keyset {
    hhe_ctx *ctx = nullptr;
    u64 serial = 0;                    // identity of the set's present content (hhe_ctx::next_serial): re-drawn whenever a key of the set is uploaded,
                                       // replaced or cleared, never reused; what a kept keystream records of the key sets it was evaluated under (KsCache)
    u64 *rk = nullptr;                 // RelinKeys::key(2): [L][2][K][N]
    std::map<u32, u64 *> gk;           // by Galois element: [L][2][K][N] each
    std::map<u32, u64 *> gk_corr;      // per Galois key of THIS set: shared-digit correction [2][K][N] (KsCorrArgs), built on first FC use
};
// One public (plain) matrix of a packed affine layer, resident with everything derived from it (hhe_matrix_create).  Not part of the
// block-table cache: it lives until hhe_matrix_destroy (or its context goes).
struct hhe_matrix {
    hhe_ctx *ctx = nullptr;
    size_t dim = 0;
    int n1 = 0, n2 = 0;          // babystep-giantstep split; 0 / 0: diagonal method
    u64 *tab = nullptr;          // diagonal: [dim][L][N] multipliers in the frame of rotate_rows(+1) | their Shoup quotients; BSGS: [dim][L][N]
    u64 *bias = nullptr;         // [N] plaintext of the bias (coefficients mod t), or null
    GrowBuf<const u64 *> self;   // device pointers, all = tab: the per-item pointer array the kernels take (refilled when it grows)
    size_t bytes = 0;            // device footprint of tab + bias
};
// The encrypted weight matrix of a packed encrypted FC layer, resident (hhe_enc_matrix_create): its r generalized diagonals as the second
// operand of a BEHZ product, i.e. extended to q u B_sk and transformed, once.  Lives until hhe_enc_matrix_destroy (or its context goes).
struct hhe_enc_matrix {
    hhe_ctx *ctx = nullptr;
    size_t rows = 0, cols = 0, r = 0, c = 0;
    bool open = false;           // hhe_enc_matrix_create_open: the diagonals that do not wrap, r and c of the open shape
    u64 *wq = nullptr;           // [r][2][L][N]: NTT form under the data primes
    u64 *wb = nullptr;           // [r][2][L+1][N]: NTT form of the extension to B_sk
    size_t bytes = 0;            // device footprint of wq + wb
};
// Plaintexts as the right operands of hhe_rotate_plain_sum_ks, resident (hhe_plain_rows_create): each encoded, lifted to its centred
// representative under ALL K primes of the context (the special one included) and transformed, with Shoup quotients.
struct hhe_plain_rows {
    hhe_ctx *ctx = nullptr;
    size_t count = 0;
    u64 *tab = nullptr;          // [count][K][N] words | [count][K][N] their Shoup quotients
    GrowBuf<const u64 *> self;   // device pointers, all = tab: the per-item pointer array k_perm takes (refilled when it grows)
    size_t bytes = 0;            // device footprint of tab
    size_t s_off() const;        // words from a word of tab to its quotient
};
// A rows x cols layer under plain weights (hhe_plain_fc_create_open): the plain-rows form of its r open diagonals, the steps -e they
// are paired with, and the plaintext of the bias
struct hhe_plain_fc {
    hhe_ctx *ctx = nullptr;
    size_t rows = 0, cols = 0, r = 0, c = 0;
    hhe_plain_rows *diag = nullptr;  // owned by the handle (not in hhe_ctx::plain_rows)
    u64 *bias = nullptr;             // [N] plaintext of the bias (coefficients mod t), or null
    std::vector<int> steps;          // 0, -1, .., -(r-1)
    size_t bytes = 0;
};
// one stream + the per-batch workspaces of the ops: lane_reserve allocates the fixed set for `cap` ciphertexts under that one
// capacity; the GrowBuf members belong to single schedules, grow on their own and go with the lane's workspaces (free_lane)
struct Lane {
    rt_stream stream = nullptr;
    void *ev_done = nullptr;
    bool own_stream = false;
    size_t cap = 0;
    u64 *ws_T = nullptr;     // [B][L][K][N]
    u64 *ws_S = nullptr;     // [B][2][K][N]
    u64 *ws_d = nullptr;     // [B][L][N]
    u64 *ws_ct[4] = {nullptr, nullptr, nullptr, nullptr};  // [B][2][L][N] each ([B][3][N] at L = 1: lane_reserve)
    u64 *ws_ct3 = nullptr;   // [B][3][L][N]
    u64 *ws_plain = nullptr; // [B][N]
    u64 *ws_vals = nullptr;  // [B][128]
    u64 *bz_aq = nullptr, *bz_bq = nullptr;  // [B][2][L][N]
    u64 *bz_ab = nullptr, *bz_bb = nullptr;  // [B][2][L+1][N]
    u64 *bz_dq = nullptr;    // [B][3][L][N]
    u64 *bz_db = nullptr;    // [B][3][L+1][N]
    const u64 **d_ptrs = nullptr;  // [2*cap] per-item public-table pointers (diag | rc)
    size_t ptr_cap = 0;
    GrowBuf<u64> ws_rot;     // [16][B][2][L][N]: PASTA's babystep rotations, and the FC's product + per-depth buffers of the unshared walk
    GrowBuf<u64> ws_aff;     // [n1 + n2][B][2][L][N] baby-step ciphertexts | inner sums of hhe_packed_affine (BSGS)
    GrowBuf<u64> ws_fcp;     // [r][B][2][L][N] rotations | [r][B][3][L][N] products of a chunk of hhe_fc_packed_ks ([B][3][L][N], the one summed product, for hhe_fc_packed_sum_ks)
    GrowBuf<u64> ws_rotm;    // hoisted rotations: ciphertexts of the trie nodes a chunk does not write straight into its output, [nodes][B][2][L][N]
    // FC shared digits: one slot per trie node that is still needed -- the digit transforms of its un-rotated c1 (tp [B][L][K][N]) and its
    // ciphertext (ct [B][2][L][N]); refs = 1 while the depth-first walk is below the node + 1 per queued leaf key switch that reads it
    struct FcSlot { u64 *tp = nullptr, *ct = nullptr, *c0hat = nullptr; int refs = 0; int tp_polys = 0; };  // c0hat [B][L][N]: NTT form of the node's c0 (nodes with a non-leaf child)  // tp_polys: K, or 1 when tp holds the special-prime transforms only
    std::vector<FcSlot> fc_slots;
    std::vector<u64 *> csum_bufs;  // FC leaves: integer sums of parents' c1 per Galois element, [B][L][N] each (sized like the slots)
    size_t fc_slot_cap = 0;  // items the slots were sized for
    GrowBuf<u64> ws_leaf;    // FC leaf groups: special-limb sums [B][2][G][N] | their inverse transforms [B][2][G][N], G = HHE_LEAF_GROUP
    u32 *zero_flag = nullptr; // device flag of the chunk this lane is evaluating (shared-digit FC)
    // host staging of small per-call inputs (mask values, pointer tables): it outlives the asynchronous copy, and the next
    // user waits for that copy (ev_stage) before overwriting it
    std::vector<u64> h_stage;
    std::vector<const u64 *> h_ptrs;
    void *ev_stage = nullptr;
    bool stage_pending = false;
    std::vector<std::pair<void *, void *>> prof_ev;  // hhe_ctx_profile: event pairs around the launches of ks_row_kernel on this lane's stream
    size_t prof_used = 0;
};

struct hhe_ctx {
    // every C-ABI entry point that takes the context holds this lock for its whole duration: concurrent callers (the
    // reference's gRPC handlers run concurrently, CSPRPC.cpp:201-203) are serialised per context; different contexts are
    // independent.  Recursive because hhe_decompose / the FC call other entry points.
    std::recursive_mutex mu;
    int profile = 0;               // hhe_ctx_profile: bracket the ks_row_kernel launches with timed events
    u64 prof_items = 0;            // ciphertexts covered by the bracketed launches since the last read
    int logn = 0, K = 0, L = 0, device = 0;
    size_t n = 0;
    u64 t = 0;
    std::vector<u64> q;            // K coefficient primes
    std::vector<u64> bsk;          // L+1: B_0..B_{L-1}, m_sk
    u64 gamma = 0;
    std::vector<u64> roots;        // psi per coefficient prime
    int nmod = 0;                  // K + (L+1) + 1
    int mod_t = 0;                 // index of the plain modulus
    int digit_reduce = 1;          // 0 when every data prime is below 4x every key prime (lazy NTT input range)
    std::vector<int> pm_ok;        // per ModDev index: the modulus has the pseudo-Mersenne form the lazy butterflies fold with (ModDev::pm_ok)
    u64 fc_fallbacks = 0;          // how often the shared-digit path had to be recomputed exactly
    int fc_shared = 1;             // FC rotation trie: children of a node share the digit transforms of its c1 (HHE_FC_SHARED; 2 = force the fallback, tests)
    int fc_leaf_group = HHE_LEAF_GROUP;  // FC rotation trie: leaf key switches per launch, across the nodes whose digits are resident (HHE_FC_LEAFGROUP; 1 = one leaf at a time)
    int fc_row_fused = 1;          // FC non-leaf children at N >= 4096: inner product + inverse row pass in one kernel (ks_perm_row_kernel; HHE_FC_ROWFUSED=0: separate launches)
    u64 fc_csum_closes = 0;        // how many c1 sums were closed (digits + transforms + one inner product); diagnostics, hhe_ctx_query("fc_csum_closes")
    int fc_csum_group = HHE_CSUM_GROUP;  // parents per csum_add launch (HHE_FC_CSUMGROUP, 1..HHE_CSUM_GROUP)
    int fc_c0hat = 1;              // FC non-leaf children through ks_perm_row_kernel: galois(c0) enters in the NTT domain (KsRowArgs::c0hat) instead of a gather in the KSF epilogue (HHE_FC_C0HAT=0)
    int fc_csum = 1;               // FC leaves: data-limb sums through per-element integer sums of the parents' c1 (one inner product per element instead of one per leaf; HHE_FC_CSUM=0: per leaf)
    u64 *d_qsp_poly = nullptr;     // [L][N]: the constant q_sp mod q_j in every slot (multiplier of the NTT form of a node's c0, FcSlot::c0hat)
    u64 *d_zero_corr = nullptr;    // [2][K][N] zeros: the correction table of the closing product of a c1 sum (its digits are already those of the rotated sum)
    int fc_leaf_sums = 1;          // FC rotation trie: postpone the inverse transforms of leaf key switches (linear part summed first)
    size_t fc_chunk = 160;         // items per internal chunk of hhe_fc_row (0 = whole batch); ms per MNIST sample (784x10, 16 samples): 64: 60.5, 80: 60.6, 96: 60.6, 128: 59.5, 160: 58.4
                                   // (round 1: 40: 67.1, 80: 64.9, 160: 64.0); the trie's small launches (2 polynomials per item) want more than one round of workgroups
    int matmul_mode = 1;           // 1: fused 20-transform pipeline (default), 0: op-by-op schedule
    int shared_l0 = 12;            // fused pipeline, first affine layer: in calls of at least this many items its rotation chain runs once, on the one key
                                   // ciphertext every item starts from, and an item only multiplies its diagonals into the shared rotated states
                                   // (HHE_SHARED_L0; 1: every call, 0: never = per-item chain).  A few items cost what one costs (latency-bound either
                                   // way), so below the threshold sharing saves nothing and adds the sum launches: ms per call shared / per item at 4, 8, 12, 16, 32 items: 38.4 / 36.3, 44.5 / 44.1, 54.7 / 58.2, 61.7 / 66.8, 98.5 / 113.4
    size_t l0_budget = (size_t)512 << 20;  // bytes the operand table of that chain may take (HHE_SHARED_L0_MB); a chain that needs more runs in blocks of steps
    GrowBuf<u64> l0_tab;           // [3][S][L][N] operands of S chain steps (L0Capture), exactly that size (allocated on first use, freed with the context)
    GrowBuf<const u64 *> l0_ptrs;  // per-item diagonal tables of the running call
    size_t l0_steps() const { return l0_tab.cap / ((size_t)3 * L * n); }
    int dedup = 1;                 // transciphering: the keystream ciphertext of a block counter is evaluated once per call and every item with that counter
                                   // only subtracts it from its own encoded words (HHE_DEDUP; 0: every item evaluates its own).  What is kept across calls: ks_cache
    GrowBuf<u64> ks_tab;           // [M][2][L][N]: the keystream ciphertexts the running call evaluates, in order of first appearance ([U]: with copies of the kept ones behind them, unfused finishing pass)
    // the finishing pass res = Enc(c_b) - KS over all B items of a call (its chunks are larger than the lanes' ciphertext workspaces):
    int fin_fused = 1;             // two kernels (LOAD_ENCODE row pass, STORE_ADD_PLAIN strided pass) instead of clear + scatter + transform + add_plain
                                   // (HHE_FIN_FUSED; 0: launch for launch).  Off where no test runs the fused kernels' geometry (N = 2^16: fin_fused_ok)
    FinArgs *d_fin = nullptr;      // the fused kernels' constants, written once
    int fin_item = -1;             // the whole finishing pass of an item in one workgroup, its plaintext kept in LDS (fin_item_kernel; HHE_FIN_ITEM): 0 never,
                                   // 1 whenever the context is eligible (fin_item_on), -1 (unset) from fin_item_min items on
    size_t fin_item_min = 64;      // an item occupies one CU whatever the batch: a small call is faster spread over the tiles of the two-pass kernels (measured: slower up to 32 items, level at 48, faster from 64)
                                   // (DESIGN.md "Finishing pass in one workgroup")
    u32 *d_fin_itw = nullptr;      // [N][2] u32 inverse twiddles mod t (FinArgs::itw); null where t needs more than 30 bits or N > 2^15
    bool fin_scale32 = false;      // FinArgs carries the constants of the item kernel's 32-bit plaintext scaling (fin_scale32_ok and HHE_FIN_SCALE32 != 0): its launches take fin_item32_kernel
    u64 fin_item_launches = 0;     // launches of fin_item_kernel (hhe_ctx_query("fin_item_launches"))
    u32 *d_slot_inv = nullptr;     // [N] inverse of slot_map (FinArgs::slot_inv)
    GrowBuf<u64> fin_dev;          // [B] per item: pointer to its keystream (fused) or its slot of ks_tab as u32 (unfused) | [B][128] the items' words,
                                   // zero padded | [B][N] the intermediate of the transform mod t (unfused: the plaintexts)
    HostStage fin_host;            // [KsCache::MAX_SNAPSHOTS] flags of the key comparison, read back | the first two parts of fin_dev as they are uploaded;
                                   // where it is page-locked the item kernel reads the words here and they are not uploaded
    std::vector<unsigned char> fin_tab_shadow;  // what the table part of fin_dev holds: the bytes of the last upload into it (fin_tab_upload, hhe_api.cpp), which
                                   // skips an upload of the same bytes; empty = unknown: fin_dev grew (fin_reserve) or a call of another item count, whose
                                   // words and intermediate lie where this table was, has begun (fin_tab_items)
    size_t fin_tab_items = 0;      // the item count of the call the shadow belongs to: the parts of fin_dev behind the table start at fin_tab_words(B)
    u64 fin_tab_uploads = 0;       // uploads into the table part that were enqueued (hhe_ctx_query("fin_tab_uploads")), and
    u64 fin_word_uploads = 0;      // uploads of the words into fin_dev (hhe_ctx_query("fin_word_uploads")): none where the item kernel reads the staging
    void *ev_cmp = nullptr;        // recorded behind the read-back of the flags
    size_t last_unique = 0;        // distinct (nonce, counter) pairs of the last transciphering call: U, or B when it ran per item (a call in groups: summed over its groups)
    size_t last_evaluated = 0;     // keystream chains the last call ran (= last_unique unless kept keystreams were found), and
    size_t last_hits = 0;          // the counters it found a kept keystream for
    KsCache ks_cache;              // keystream ciphertexts kept across calls, per counter (hhe_kscache.h; HHE_KS_CACHE, HHE_KS_CACHE_MB); it stands aside
                                   // under HHE_DEDUP=0 and while hhe_ctx_profile is enabled (a profiled call exists to time the chain)
    GrowBuf<u64> ks_flags;         // [KsCache::MAX_SNAPSHOTS]: raised where enc_key differs from a snapshot (ELT_DIFF)
    KsConsts ksc{};
    u64 *d_moddown = nullptr;      // modulus switching: per pair j < m < L three words at mod_down_pair(m, j) (hhe_common.h), written once
    u64 mod_switch_launches = 0;   // kernel launches of hhe_mod_switch (hhe_ctx_query("mod_switch_launches"))
    u64 key_proj_launches = 0;     // kernel launches of hhe_keyset_derive_level into sets of this context: one per key (hhe_ctx_query("key_proj_launches"))
    int noise_form = 0;           // the form the last hhe_noise_budget launch took: its limb count (register form) or 0 (LDS form) (hhe_ctx_query("noise_form"))

    // device tables
    ModDev *d_mods = nullptr;
    u64 *d_tables = nullptr;
    BehzDev *d_behz = nullptr;
    u32 *d_slot_map = nullptr;
    std::vector<u32> slot_map;

    // argument templates
    KsFinishArgs ksf{};
    AddPlainArgs apl{};

    // keys: the default set (hhe_set_galois_key, relin slot 0) and the further relin slots are key sets owned by the context;
    // `sets` are the ones callers created (hhe_keyset_create).  gks / rks = the sets the running entry point named (KeyScope).
    hhe_keyset keys0;
    hhe_keyset rk_slots[HHE_RELIN_SLOTS];      // [0] unused (slot 0 is keys0.rk)
    std::vector<hhe_keyset *> sets;
    std::vector<hhe_matrix *> mats;            // plain-matrix handles created on this context
    std::vector<hhe_enc_matrix *> enc_mats;    // encrypted-matrix handles created on this context
    std::vector<hhe_plain_rows *> plain_rows;  // plain-rows handles created on this context
    std::vector<hhe_plain_fc *> plain_fcs;     // plain-weights layer handles created on this context
    u64 plain_sum_fallbacks = 0;               // chunks of hhe_rotate_plain_sum_ks / hhe_fc_open_plain_ks recomputed from per-child digits ("plain_sum_fallbacks")
    u64 plain_sum_launches = 0, plain_sum_mod_downs = 0;  // of the last such call, per chunk: launches of ks_plain_sum_row_kernel; finish launches of the primitive
    u64 fc_packed_key_switches = 0;            // Galois key switches per item of the last hhe_fc_packed_ks call (hhe_ctx_query("fc_packed_key_switches"))
    u64 add_many_launches = 0;                 // launches of the sum kernel, by hhe_add_many and by the packed FC (hhe_ctx_query("add_many_launches"))
    u64 behz_sum_cap = 0;                      // most products hhe_multiply_sum floors as one sum (hhe_ctx_query("behz_sum_cap"); the condition is in hhe_gfx950.h)
    int sum_fold_q = 1, sum_fold_bsk = 1;      // tensor_sum_fold of the widest data prime / B_sk prime ("multiply_sum_fold_q" / "multiply_sum_fold_bsk")
    u64 multiply_sum_launches = 0;             // launches of the summed tensor kernel: one per modulus set per hhe_multiply_sum call or packed FC chunk
    u64 tensor_launches = 0, square_launches = 0;  // launches of the one-product tensor kernels (plain or broadcast) / of the squaring kernel ("tensor_launches" / "square_launches")
    u64 mlp_layers = 0, mlp_key_switches = 0;  // of the last hhe_mlp_ks call: its layers; Galois key switches per item summed over them ("mlp_layers" / "mlp_key_switches")
    u64 fc_packed_floors = 0;                  // polynomials floored per item by the last packed encrypted FC call: 3 r, or 3 for hhe_fc_packed_sum_ks
    int rot_hoist = 1;                         // hhe_rotate_rows_many_ks and the hoisted packed FC: 1 = children of a trie node share the digit transforms of its c1
                                               // (HHE_ROT_HOIST; 0: every step through op_rotate_rows, 2: every chunk also recomputed that way -- tests)
    u64 rot_many_fallbacks = 0;                // chunks recomputed step by step because a digit load met a zero residue (hhe_ctx_query("rot_many_fallbacks"))
    u64 rot_many_key_switches = 0, rot_many_launches = 0;  // of the last call: the trie's nodes; multi-child launches of ks_perm_row_kernel per chunk
    GrowBuf<KsKid> d_rot_kids;                 // the per-child tables of the running call's trie, node after node (KsRowArgs::kids)
    hhe_keyset *gks = &keys0, *rks = &keys0;
    u64 next_serial = 0;                       // the last hhe_keyset::serial handed out
    std::map<const u64 *, u64 *> d_key_shoup;  // per key-switch key (by device address): Shoup quotients of its words (fused row kernel), built on first use
    hhe_keyset *relin_set(int slot) { return slot == 0 ? &keys0 : &rk_slots[slot]; }

    // device scratch of hhe_decompose (all blocks of the records) and hhe_fc_row (one flag per chunk)
    GrowBuf<u64> d_blocks;
    GrowBuf<u32> d_flags;

    // PASTA public tables
    std::map<PastaPair, BlockTables> blocks;     // by (nonce, counter); the entry points without a nonce name the pairs under PASTA_NONCE
    int public_device = -1;                      // where the randomness of missing pairs is drawn (HHE_PUBLIC_DEVICE): 0 host (pasta3_block_randomness + upload),
                                                 // 1 device (per-pair XOF + matrix expansion, ensure_blocks), -1 (unset): by the number of missing pairs, public_device_min
    size_t last_public_built = 0;                // pairs whose randomness the last call drew on the device (hhe_ctx_query("public_device_built"))
    size_t last_groups = 0;                      // groups the last transciphering call ran its items in (hhe_ctx_query("transcipher_groups"))
    size_t block_bytes = 0;                      // footprint of all cached block tables
    size_t block_cache_limit = (size_t)32 << 30; // bytes (hhe_pasta3_set_block_cache_limit, HHE_BLOCK_CACHE_MB): beyond it the least recently used counters go
    u64 block_call = 0;                          // running number of the transciphering calls
    u64 *d_feistel_mask = nullptr;  // [L][N] NTT form of the sbox_feistel mask plaintext

    // execution lanes: lane 0 runs on the caller's stream (generic ops); lanes 1.. are internal streams on which the batched
    // calls (transciphering, FC row, packed affine layer) process chunks of a batch concurrently, each with its own workspace
    // (ChunkPlan / run_chunks in hhe_api.cpp)
    Lane lanes[1 + HHE_MAX_STREAMS];
    Lane *w = &lanes[0];
    int nstreams = 1;      // internal streams used by hhe_pasta3_transcipher (0 = caller's stream only).  One: since the row kernel lost its
                           // exposed round trips two overlapping chunks give the same throughput (289 vs 289 /s) and make every kernel's duration depend on its neighbour
    size_t chunk = 128;    // items per chunk (HHE_CHUNK); measured 211 /s at 32, 221 at 64, 225 at 128 items (round 1)
    void *ev_fork = nullptr; // recorded on the main stream when the chunks fork; every used lane waits for it

    size_t ct_words() const { return (size_t)2 * L * n; }
    size_t ksk_words() const { return (size_t)L * 2 * K * n; }
};

// number theory (hhe_context.cpp)
bool nt_is_prime(u64 v);
bool nt_get_primes(u64 factor, int bits, size_t count, std::vector<u64> &out);
u64 nt_minimal_primitive_root(u64 degree, u64 q);
u64 nt_invmod(u64 a, u64 m);
u64 nt_mulmod(u64 a, u64 b, u64 m);
u64 nt_powmod(u64 a, u64 e, u64 m);
std::vector<int> nt_naf(int value);
u32 galois_elt_from_step(const hhe_ctx *c, int step);

// PASTA-3 public randomness (hhe_pasta_public.cpp)
void pasta3_block_randomness(u64 t, u64 nonce, u64 block, u64 *mats, u64 *rcs);

// 1 when every modulus of an NTT launch over ModDev indices [mod_base, mod_base + mod_cycle) has the pseudo-Mersenne form
// q = 2^b - c, 33 <= b <= 60 (ModDev::pm_ok; SEAL's own coefficient primes do, the 61-bit BEHZ base and t = 65537 do not): the
// kernels then use the truncated Shoup product and fold the butterfly ranges once per register round (NttArgs::lazy8)
inline int ntt_lazy8(const hhe_ctx *c, int mod_base, int mod_cycle)
{
    for (int i = mod_base; i < mod_base + mod_cycle; ++i)
        if (!c->pm_ok[i]) return 0;
    return 1;
}
// the fused key-switch row kernel runs when the row pass has one of its sizes AND every key-level modulus has the pseudo-Mersenne
// form its arithmetic is written for; other contexts take the separate-kernel path (any N, any primes < 2^61).  SEAL's primes of
// 42 bits and more at these degrees have the form; smaller ones (BFVDefault(4096): 36+36+37 bits) and primes that are not just
// below a power of two do not.  hhe_ctx_query("row_kernel") reports the decision.
inline bool use_row_kernel(const hhe_ctx *c) { return k_ks_row_supported(c->logn) && ntt_lazy8(c, 0, c->K); }

struct CtxLock {  // null-safe scoped lock of a context (entry points check their arguments after taking it)
    std::unique_lock<std::recursive_mutex> l;
    explicit CtxLock(const hhe_ctx *c) { if (c) l = std::unique_lock<std::recursive_mutex>(const_cast<hhe_ctx *>(c)->mu); }
};
#define HHE_LOCK(c) CtxLock hhe_lock_guard_(c)

// names the key objects of one entry point for the ops below it (null = the context's default set); restored on exit
struct KeyScope {
    hhe_ctx *c;
    hhe_keyset *g0, *r0;
    KeyScope(hhe_ctx *c_, const hhe_keyset *gk, const hhe_keyset *rk) : c(c_), g0(c_->gks), r0(c_->rks)
    {
        c->gks = gk ? const_cast<hhe_keyset *>(gk) : &c->keys0;
        c->rks = rk ? const_cast<hhe_keyset *>(rk) : &c->keys0;
    }
    ~KeyScope() { c->gks = g0; c->rks = r0; }
};
// upload into a set (hhe_context.cpp); words are validated against the key-level primes first
int keyset_put_galois(hhe_keyset *ks, u32 elt, const u64 *ksk);
int keyset_put_relin(hhe_keyset *ks, const u64 *ksk);
void keyset_clear(hhe_keyset *ks);
// a key generated on the device enters a set under the rules of the uploads (serial re-drawn, tables derived from a replaced key dropped);
// the set takes ownership of `key` ([L][2][K][N] device words, reduced by construction).  elt is valid (the caller checked the whole list)
void keyset_adopt_relin(hhe_keyset *ks, u64 *key);
void keyset_adopt_galois(hhe_keyset *ks, u32 elt, u64 *key);
void keyset_new_serial(hhe_keyset *ks);  // the set's content changes: keystreams kept under its old serial go

int lane_reserve(hhe_ctx *c, Lane &ln, size_t B);
int fin_reserve(hhe_ctx *c, size_t B);  // fin_dev and fin_host for a transciphering call of B items
inline size_t fin_tab_words(size_t B) { return (B + 1) & ~(size_t)1; }  // the table part of both, padded: what follows it is read and written 16 bytes at a time
// The fused finishing kernels run where a test runs their geometry: every N up to 2^15.  At N = 2^16 the strided pass has 256 points, a
// size no other N gives it, and the setup of a test there does not fit the suite's budget -- that size takes the separate launches.
inline bool fin_fused_on(const hhe_ctx *c) { return c->fin_fused && c->logn <= 15; }
// ... and the one-workgroup form of them where the transform mod t fits 32-bit words and N words fit LDS (hhe_fin_bodies.h)
inline bool fin_item_on(const hhe_ctx *c) { return c->fin_item != 0 && fin_fused_on(c) && c->d_fin_itw != nullptr; }
inline bool fin_item_for(const hhe_ctx *c, size_t B) { return fin_item_on(c) && (c->fin_item > 0 || B >= c->fin_item_min); }
void matrix_free(hhe_matrix *m);  // hhe_api.cpp: device memory of a handle and the handle
void enc_matrix_free(hhe_enc_matrix *m);
void plain_rows_free(hhe_plain_rows *p);
void plain_fc_free(hhe_plain_fc *m);
inline size_t hhe_plain_rows::s_off() const { return count * (size_t)ctx->K * ctx->n; }

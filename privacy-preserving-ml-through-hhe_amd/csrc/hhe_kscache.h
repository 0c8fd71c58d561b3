// hhe_kscache.h -- bookkeeping of the keystream ciphertexts a context keeps from one transciphering call to the next
// (DESIGN.md "one keystream per key").  Host code only, no device runtime beyond rt_malloc / rt_free: tests/cpp/kscache_main.cpp
// compiles it against logging stubs.
//
// The keystream ciphertext of a block is a function of the words of enc_key, the Galois and relinearization keys the call
// names, the (nonce, counter) pair (PastaPair; "counter" below) and use_bsgs.  What identifies them here:
//  - enc_key is the caller's device buffer, so only its words do: the cache keeps device copies (snapshots) of the key ciphertexts it
//    holds keystreams for, at most MAX_SNAPSHOTS of them, and the call compares enc_key against them word for word on the device
//    (ELT_DIFF; no hash).  An entry names its snapshot by a number that is never reused.
//  - a key set has a serial number, drawn from a counter of the context that never repeats and re-drawn whenever a key of the set is
//    uploaded, replaced or cleared (hhe_context.cpp); the entries made under the old serial are dropped at once (drop_serial).
// An entry belongs to its counter's block tables (hhe_ctx::blocks): it is made while they are resident and goes when they go
// (drop_counter from evict_blocks; clear from hhe_pasta3_clear_block_cache and the context's destruction).  Its memory is counted
// here, not in block_bytes, and bounded by `budget` (HHE_KS_CACHE_MB): the least recently used entries go first.
// Every path that frees device memory waits for the context's streams first (sync_ctx), once.
#pragma once
#include <map>
#include <vector>
#include "hhe_launch.h"

struct hhe_ctx;
void sync_ctx(hhe_ctx *c);

struct KsCache {
    static constexpr size_t MAX_SNAPSHOTS = 4;
    struct Snapshot { u64 *words; u64 id, last_use; };
    struct Entry {
        u64 *ct;          // [2][L][N], owned
        u64 snap;         // Snapshot::id of the key ciphertext it was evaluated from
        u64 gks, rks;     // serials of the Galois / relinearization key sets
        int bsgs;
        u64 last_use;     // the transciphering call (hhe_ctx::block_call) that made or used it last
        bool same_key(const Entry &o) const { return snap == o.snap && gks == o.gks && rks == o.rks && bsgs == o.bsgs; }
    };
    bool enabled = true;                  // HHE_KS_CACHE
    size_t budget = (size_t)256 << 20;    // bytes of keystream ciphertexts (HHE_KS_CACHE_MB); the snapshots are not counted
    size_t entry_bytes = 0;               // one ciphertext (set at context creation)
    size_t bytes = 0;
    u64 next_snap = 0;
    std::vector<Snapshot> snaps;
    std::map<PastaPair, std::vector<Entry>> by_counter;  // by (nonce, counter); a bare counter names the pair under PASTA_NONCE

    size_t entries() const
    {
        size_t k = 0;
        for (auto &kv : by_counter) k += kv.second.size();
        return k;
    }
    // the keystream of `counter` under the identity in `key` (ct and last_use ignored), or null; a hit is touched
    const u64 *find(const PastaPair &counter, const Entry &key, u64 now)
    {
        auto it = by_counter.find(counter);
        if (it == by_counter.end()) return nullptr;
        for (Entry &e : it->second)
            if (e.same_key(key)) { e.last_use = now; return e.ct; }
        return nullptr;
    }
    // the same without touching the hit: a call that predicts its key looks before it knows (hhe_api.cpp, transcipher_enqueue)
    const u64 *peek(const PastaPair &counter, const Entry &key) const
    {
        auto it = by_counter.find(counter);
        if (it == by_counter.end()) return nullptr;
        for (const Entry &e : it->second)
            if (e.same_key(key)) return e.ct;
        return nullptr;
    }
    // takes `words` (a device copy of a key ciphertext no resident snapshot equals); the least recently used snapshot makes room and
    // takes its entries with it.  Returns the new snapshot's number
    u64 add_snapshot(hhe_ctx *c, u64 *words, u64 now)
    {
        bool synced = false;
        while (snaps.size() >= MAX_SNAPSHOTS) {
            size_t v = 0;
            for (size_t i = 1; i < snaps.size(); ++i)
                if (snaps[i].last_use < snaps[v].last_use) v = i;
            const u64 id = snaps[v].id;
            wait(c, synced);
            rt_free(snaps[v].words);
            snaps.erase(snaps.begin() + v);
            drop_if(c, synced, [&](const PastaPair &, const Entry &e) { return e.snap == id; });
        }
        snaps.push_back({words, ++next_snap, now});
        return next_snap;
    }
    // takes e.ct.  Entries that the running call (`now`) neither made nor used go, least recently used first, while the budget is
    // passed; when that does not make room the new ciphertext is freed instead.  Returns whether it was kept
    bool insert(hhe_ctx *c, const PastaPair &counter, const Entry &e)
    {
        bool synced = false;
        drop_if(c, synced, [&](const PastaPair &ctr, const Entry &o) { return ctr == counter && o.same_key(e); });  // never two of one identity
        while (bytes + entry_bytes > budget) {
            PastaPair vc(0);
            const Entry *v = nullptr;
            for (auto &kv : by_counter)
                for (const Entry &o : kv.second)
                    if (o.last_use != e.last_use && (!v || o.last_use < v->last_use)) { v = &o; vc = kv.first; }
            if (!v) { wait(c, synced); rt_free(e.ct); return false; }
            const u64 *ct = v->ct;
            drop_if(c, synced, [&](const PastaPair &ctr, const Entry &o) { return ctr == vc && o.ct == ct; });
        }
        by_counter[counter].push_back(e);
        bytes += entry_bytes;
        return true;
    }
    void drop_counter(hhe_ctx *c, const PastaPair &counter)
    {
        bool synced = false;
        drop_if(c, synced, [&](const PastaPair &ctr, const Entry &) { return ctr == counter; });
    }
    void drop_serial(hhe_ctx *c, u64 serial)
    {
        bool synced = false;
        drop_if(c, synced, [&](const PastaPair &, const Entry &e) { return e.gks == serial || e.rks == serial; });
    }
    void clear(hhe_ctx *c)  // entries and snapshots
    {
        bool synced = false;
        drop_if(c, synced, [](const PastaPair &, const Entry &) { return true; });
        for (Snapshot &s : snaps) { wait(c, synced); rt_free(s.words); }
        snaps.clear();
    }

private:
    static void wait(hhe_ctx *c, bool &synced)
    {
        if (!synced) sync_ctx(c);
        synced = true;
    }
    template <class Pred> void drop_if(hhe_ctx *c, bool &synced, Pred pred)
    {
        for (auto it = by_counter.begin(); it != by_counter.end();) {
            std::vector<Entry> &v = it->second;
            for (size_t i = 0; i < v.size();) {
                if (!pred(it->first, v[i])) { ++i; continue; }
                wait(c, synced);
                rt_free(v[i].ct);
                bytes -= entry_bytes;
                v.erase(v.begin() + i);
            }
            it = v.empty() ? by_counter.erase(it) : std::next(it);
        }
    }
};

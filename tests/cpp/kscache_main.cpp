// kscache_main.cpp -- KsCache (csrc/hhe_kscache.h), the bookkeeping of the keystream ciphertexts a context keeps across calls, against
// stubs of the device runtime that log every call.  Built with -fsanitize=address,undefined by tests/test_cpp_kscache.py: device
// buffers are real heap blocks here, so a buffer freed twice, never freed, or read through a stale entry is the sanitizer's finding;
// the log checks in addition that every path that frees waits for the context's streams first, and once.
// No library is linked: the header and the stubs below are the whole program.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>
#include "hhe_kscache.h"

static std::vector<std::string> calls;  // "sync", "free" in the order they happened
static std::set<void *> live;           // device buffers handed out and not freed yet
static int double_frees = 0;

void *rt_malloc(size_t bytes)
{
    void *p = malloc(bytes);
    live.insert(p);
    return p;
}
void rt_free(void *p)
{
    if (!p) return;
    calls.push_back("free");
    if (!live.erase(p)) { ++double_frees; return; }
    free(p);
}
void sync_ctx(hhe_ctx *) { calls.push_back("sync"); }

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
// what happened since the last look: `frees` buffers freed, behind exactly one wait (none when nothing was freed)
static bool freed(size_t frees)
{
    std::vector<std::string> want;
    if (frees) want.push_back("sync");
    want.insert(want.end(), frees, "free");
    const bool ok = calls == want;
    if (!ok) for (auto &s : calls) printf("  call: %s\n", s.c_str());
    calls.clear();
    return ok;
}
constexpr size_t EB = 64;  // bytes of one "ciphertext"
static u64 *buf(u64 tag)
{
    u64 *p = (u64 *)rt_malloc(EB);
    p[0] = tag;
    return p;
}
static KsCache::Entry key(u64 snap, u64 gks, u64 rks, int bsgs, u64 now, u64 tag = 0) { return KsCache::Entry{tag ? buf(tag) : nullptr, snap, gks, rks, bsgs, now}; }
// a found keystream is a live buffer that holds what was inserted
static bool holds(const u64 *p, u64 tag) { return p && live.count((void *)p) && p[0] == tag; }

int main()
{
    hhe_ctx *c = nullptr;  // only handed to the sync_ctx stub
    {
        KsCache k;
        k.entry_bytes = EB;
        k.budget = 3 * EB;
        // insert and hit: the identity is (counter, snapshot, both serials, use_bsgs)
        const u64 s1 = k.add_snapshot(c, buf(1000), 1);
        CHECK(s1 == 1 && k.snaps.size() == 1 && freed(0));
        CHECK(k.insert(c, 0, key(s1, 7, 7, 0, 1, 11)) && k.insert(c, 1, key(s1, 7, 7, 0, 1, 12)));
        CHECK(k.entries() == 2 && k.bytes == 2 * EB && freed(0));
        CHECK(holds(k.find(0, key(s1, 7, 7, 0, 0), 2), 11) && holds(k.find(1, key(s1, 7, 7, 0, 0), 2), 12));
        CHECK(!k.find(2, key(s1, 7, 7, 0, 0), 2) && !k.find(0, key(s1 + 1, 7, 7, 0, 0), 2) && !k.find(0, key(s1, 8, 7, 0, 0), 2) &&
              !k.find(0, key(s1, 7, 8, 0, 0), 2) && !k.find(0, key(s1, 7, 7, 1, 0), 2));
        // the same identity again replaces: never two of one
        CHECK(k.insert(c, 0, key(s1, 7, 7, 0, 2, 13)) && k.entries() == 2 && k.bytes == 2 * EB && freed(1));
        CHECK(holds(k.find(0, key(s1, 7, 7, 0, 0), 2), 13));
        // evict by budget: call 3 uses counter 1 and adds two entries; the least recently used one it did not touch (counter 0) goes
        CHECK(holds(k.find(1, key(s1, 7, 7, 0, 0), 3), 12));
        CHECK(k.insert(c, 2, key(s1, 7, 7, 0, 3, 14)) && k.entries() == 3 && freed(0));
        CHECK(k.insert(c, 3, key(s1, 7, 7, 0, 3, 15)) && k.entries() == 3 && k.bytes == 3 * EB && freed(1));
        CHECK(!k.find(0, key(s1, 7, 7, 0, 0), 3) && holds(k.find(1, key(s1, 7, 7, 0, 0), 3), 12));
        // ... and when everything resident belongs to the running call, the new one is not kept (and freed)
        CHECK(!k.insert(c, 4, key(s1, 7, 7, 0, 3, 16)) && k.entries() == 3 && k.bytes == 3 * EB && freed(1));
        CHECK(!k.find(4, key(s1, 7, 7, 0, 0), 3));
        // evict by block table: the counter's entries of every identity, nobody else's
        k.budget = 100 * EB;
        CHECK(k.insert(c, 2, key(s1, 9, 7, 1, 4, 17)) && k.entries() == 4);
        k.drop_counter(c, 2);
        CHECK(freed(2) && k.entries() == 2 && k.bytes == 2 * EB && !k.by_counter.count(2));
        CHECK(!k.find(2, key(s1, 7, 7, 0, 0), 4) && !k.find(2, key(s1, 9, 7, 1, 0), 4) && holds(k.find(3, key(s1, 7, 7, 0, 0), 4), 15));
        k.drop_counter(c, 2);  // nothing there: no wait, no free
        CHECK(freed(0));
        // key-set destroy / re-draw: the entries that name the serial on either side
        CHECK(k.insert(c, 5, key(s1, 20, 7, 0, 5, 18)) && k.insert(c, 5, key(s1, 7, 20, 0, 5, 19)) && k.insert(c, 6, key(s1, 21, 21, 0, 5, 20)));
        k.drop_serial(c, 20);
        CHECK(freed(2) && k.entries() == 3 && !k.find(5, key(s1, 20, 7, 0, 0), 5) && !k.find(5, key(s1, 7, 20, 0, 0), 5));
        CHECK(holds(k.find(6, key(s1, 21, 21, 0, 0), 5), 20) && holds(k.find(1, key(s1, 7, 7, 0, 0), 5), 12));
        k.drop_serial(c, 7);
        CHECK(freed(2) && k.entries() == 1);
        // snapshots: the fifth drops the least recently used one and the entries evaluated from it
        k.snaps[0].last_use = 6;
        u64 s[5] = {s1};
        for (int i = 1; i < 4; ++i) {
            s[i] = k.add_snapshot(c, buf(1000 + i), 6 + i);
            CHECK(s[i] == s1 + i && freed(0) && k.insert(c, 6, key(s[i], 21, 21, 0, 6 + i, 30 + i)));
        }
        CHECK(k.snaps.size() == 4 && k.entries() == 4);
        k.snaps[0].last_use = 20;  // s1 was matched by a later call: s[1] is the oldest now
        s[4] = k.add_snapshot(c, buf(1004), 21);
        CHECK(s[4] == s1 + 4 && k.snaps.size() == 4 && freed(2) && k.entries() == 3);
        CHECK(!k.find(6, key(s[1], 21, 21, 0, 0), 21) && holds(k.find(6, key(s1, 21, 21, 0, 0), 21), 20) && holds(k.find(6, key(s[2], 21, 21, 0, 0), 21), 32));
        for (auto &sn : k.snaps) CHECK(sn.id != s[1] && live.count(sn.words));
        // clear: entries and snapshots, one wait; the cache is usable afterwards and numbers go on
        k.clear(c);
        CHECK(freed(3 + 4) && k.entries() == 0 && k.bytes == 0 && k.snaps.empty() && k.by_counter.empty() && live.empty());
        k.clear(c);
        CHECK(freed(0));
        const u64 s6 = k.add_snapshot(c, buf(1005), 30);
        CHECK(s6 == s1 + 5 && k.insert(c, 0, key(s6, 1, 1, 0, 30, 40)) && holds(k.find(0, key(s6, 1, 1, 0, 0), 31), 40));
        // context destroy = clear with entries and a snapshot resident
        k.clear(c);
        CHECK(freed(2) && live.empty());
    }
    CHECK(calls.empty() && live.empty() && double_frees == 0);
    printf("kscache OK\n");
    return 0;
}

// growbuf_main.cpp -- GrowBuf<T> (csrc/hhe_internal.h), the grow-only device workspace of the host driver, against stubs of the
// device runtime that log every call: what it allocates, when it waits, and what it leaves behind when the allocation fails.
// No library is linked: the header and the stubs below are the whole program.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "hhe_internal.h"

static std::vector<std::string> calls;  // "sync", "malloc <bytes>", "free <id>" in the order they happened
static bool fail_next_malloc = false;
static std::string last_error;
static char arena[64];                  // allocation i is &arena[i]: never dereferenced
static int next_id = 1;

void *rt_malloc(size_t bytes)
{
    calls.push_back("malloc " + std::to_string(bytes));
    if (fail_next_malloc) { fail_next_malloc = false; return nullptr; }
    return &arena[next_id++];
}
void rt_free(void *p)
{
    if (p) calls.push_back("free " + std::to_string((int)((char *)p - arena)));
}
const char *rt_last_error() { return "out of memory (stub)"; }
void sync_ctx(hhe_ctx *) { calls.push_back("sync"); }
void hhe_set_error(const std::string &msg) { last_error = msg; }

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
static bool log_is(std::vector<std::string> want)
{
    const bool ok = calls == want;
    if (!ok) for (auto &s : calls) printf("  call: %s\n", s.c_str());
    calls.clear();
    return ok;
}

int main()
{
    hhe_ctx *c = nullptr;  // only handed to the sync_ctx stub
    GrowBuf<u64> b;
    bool grew = true;
    CHECK(b.p == nullptr && b.cap == 0);
    // first growth: wait, (nothing to free), allocate count * sizeof(T) bytes
    CHECK(b.reserve(c, 10, "ws", &grew) == HHE_OK && grew && b.cap == 10 && b.p == (u64 *)&arena[1]);
    CHECK(log_is({"sync", "malloc 80"}));
    // below and at the capacity: no call at all, same buffer
    CHECK(b.reserve(c, 3, "ws", &grew) == HHE_OK && !grew && b.reserve(c, 10, "ws") == HHE_OK && b.cap == 10 && b.p == (u64 *)&arena[1]);
    CHECK(log_is({}));
    // growth: exactly one wait, before the free
    CHECK(b.reserve(c, 11, "ws", &grew) == HHE_OK && grew && b.cap == 11 && b.p == (u64 *)&arena[2]);
    CHECK(log_is({"sync", "free 1", "malloc 88"}));
    // failed growth: the old buffer is gone, nothing is left, the error names the workspace and the runtime's message
    fail_next_malloc = true;
    grew = true;
    CHECK(b.reserve(c, 20, "rot workspace", &grew) == HHE_ERR_DEVICE && !grew && b.p == nullptr && b.cap == 0);
    CHECK(last_error == "rot workspace: out of memory (stub)");
    CHECK(log_is({"sync", "free 2", "malloc 160"}));
    // a size that used to fit allocates again instead of handing out the null pointer
    CHECK(b.reserve(c, 5, "ws", &grew) == HHE_OK && grew && b.p == (u64 *)&arena[3] && b.cap == 5);
    CHECK(log_is({"sync", "malloc 40"}));
    // release frees once and may be repeated; a release followed by a reserve is how a buffer shrinks
    b.release();
    CHECK(b.p == nullptr && b.cap == 0 && log_is({"free 3"}));
    b.release();
    CHECK(b.p == nullptr && b.cap == 0 && log_is({}));
    CHECK(b.reserve(c, 2, "ws") == HHE_OK && b.cap == 2 && log_is({"sync", "malloc 16"}));
    // the capacity counts elements of T
    GrowBuf<const u64 *> ptrs;
    GrowBuf<u32> flags;
    CHECK(ptrs.reserve(c, 3, "ptrs") == HHE_OK && flags.reserve(c, 3, "flags") == HHE_OK && ptrs.cap == 3 && flags.cap == 3);
    CHECK(log_is({"sync", "malloc " + std::to_string(3 * sizeof(void *)), "sync", "malloc 12"}));
    printf("growbuf OK\n");
    return 0;
}

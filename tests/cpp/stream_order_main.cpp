// stream_order_main.cpp -- TESTS ONLY.  The stream model of the emulator (tests/emu/emu_order.cpp) on its own: a stand-alone host
// program over the rt_* layer of csrc/hhe_launch.h and two trivial operations (fill a buffer, copy a buffer), built by
// tests/test_cpp_stream_order.py with -fsanitize=address,undefined.  Every rule of the lazy order is shown in both directions: the
// consumer that was not ordered behind its producer reads the poison, the one that was reads the data.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iprivacy-preserving-ml-through-hhe_amd/csrc -Itests/emu \
//       tests/cpp/stream_order_main.cpp tests/emu/emu_order.cpp -o stream_order
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "emu_order.h"

static constexpr size_t W = 16;
static u64 POISON;

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static void k_fill(u64 *dst, u64 v, rt_stream s) { emu_enqueue(s, [=] { for (size_t i = 0; i < W; ++i) dst[i] = v; }); }
static void k_copy(u64 *dst, const u64 *src, rt_stream s) { emu_enqueue(s, [=] { for (size_t i = 0; i < W; ++i) dst[i] = src[i]; }); }
static bool all(const u64 *p, u64 v)
{
    for (size_t i = 0; i < W; ++i)
        if (p[i] != v) return false;
    return true;
}
static u64 *dev() { return (u64 *)rt_malloc(W * 8); }
struct Stats { uint64_t deferred, forced, max_pending, forces; };
static Stats stats()
{
    uint64_t o[4];
    emu_order_stats(o);
    return {o[0], o[1], o[2], o[3]};
}

static void lazy_rules()
{
    setenv("HHE_EMU_ORDER", "lazy", 1);
    POISON = emu_poison_word();
    rt_stream A = rt_stream_create(), B = rt_stream_create();
    CHECK(A && B && A != B);
    void *ev = rt_event_create(), *ev2 = rt_event_create();

    {   // new memory is poisoned; nothing runs at the enqueue
        u64 *X = dev();
        CHECK(all(X, POISON));
        const Stats s0 = stats();
        k_fill(X, 7, A);
        CHECK(all(X, POISON));
        const Stats s1 = stats();
        CHECK(s1.deferred == s0.deferred + 1 && s1.forced == s0.forced);
        CHECK(rt_sync(A) == 0 && all(X, 7));
        const Stats s2 = stats();
        CHECK(s2.forced == s1.forced + 1 && s2.forces == s1.forces + 1 && s2.max_pending >= 1);
        rt_free(X);
    }
    {   // missing event: the consumer on B reads what the producer on A has not written yet
        u64 *X = dev(), *Y = dev();
        k_fill(X, 7, A);
        k_copy(Y, X, B);
        rt_sync(B);
        CHECK(all(Y, POISON) && all(X, POISON));
        rt_sync(A);
        CHECK(all(X, 7) && all(Y, POISON));
        rt_free(X); rt_free(Y);
    }
    {   // ... and with record + wait it reads the data; forcing B ran A's prefix up to the record, nothing behind it
        u64 *X = dev(), *Y = dev(), *Z = dev();
        k_fill(X, 7, A);
        rt_event_record(ev, A);
        k_fill(Z, 9, A);
        rt_stream_wait_event(B, ev);
        k_copy(Y, X, B);
        rt_sync(B);
        CHECK(all(Y, 7) && all(X, 7) && all(Z, POISON));
        rt_sync(A);
        CHECK(all(Z, 9));
        rt_free(X); rt_free(Y); rt_free(Z);
    }
    {   // event binding: a wait binds to the record enqueued before it, not to a later record of the same event
        u64 *X = dev(), *Y = dev();
        k_fill(X, 1, A);
        rt_event_record(ev, A);
        rt_stream_wait_event(B, ev);
        k_fill(X, 2, A);
        rt_event_record(ev, A);
        k_copy(Y, X, B);
        rt_sync(B);
        CHECK(all(Y, 1) && all(X, 1));
        // the host's wait takes the record enqueued last
        rt_event_sync(ev);
        CHECK(all(X, 2));
        rt_free(X); rt_free(Y);
    }
    {   // a wait for an event that was never recorded is a no-op; an event synced before any record returns at once
        u64 *X = dev(), *Y = dev();
        void *never = rt_event_create();
        k_fill(X, 3, A);
        rt_stream_wait_event(B, never);
        k_fill(Y, 4, B);
        CHECK(rt_event_sync(never) == 0);
        CHECK(all(X, POISON) && all(Y, POISON));
        rt_sync(B);
        CHECK(all(Y, 4) && all(X, POISON));  // minimal force: A's unrelated work stays pending
        rt_sync(A);
        CHECK(all(X, 3));
        rt_event_destroy(never);
        rt_free(X); rt_free(Y);
    }
    {   // minimal force through a chain: C waits for B's record, B's prefix waits for A's
        rt_stream C = rt_stream_create();
        u64 *X = dev(), *Y = dev(), *Z = dev(), *U = dev();
        k_fill(X, 5, A);
        rt_event_record(ev, A);
        rt_stream_wait_event(B, ev);
        k_copy(Y, X, B);
        rt_event_record(ev2, B);
        k_fill(U, 6, B);  // behind the record: not needed by C
        rt_stream_wait_event(C, ev2);
        k_copy(Z, Y, C);
        rt_stream_destroy(C);  // forces C, and through its wait markers B and A up to the records
        CHECK(all(Z, 5) && all(U, POISON));
        rt_sync(B);
        CHECK(all(U, 6));
        rt_free(X); rt_free(Y); rt_free(Z); rt_free(U);
    }
    {   // the NULL stream is a stream like any other
        u64 *X = dev(), *Y = dev();
        k_fill(X, 1, nullptr);
        k_copy(Y, X, A);
        rt_sync(A);
        CHECK(all(Y, POISON) && all(X, POISON));
        rt_sync(nullptr);
        CHECK(all(X, 1));
        rt_free(X); rt_free(Y);
    }
    {   // host memory.  Page-locked H2D reads the buffer when it runs, pageable H2D took the bytes at the call
        u64 *X = dev(), *Y = dev();
        u64 *P = (u64 *)rt_host_malloc(W * 8);
        CHECK(P && all(P, POISON));
        std::vector<u64> H(W, 1);
        for (size_t i = 0; i < W; ++i) P[i] = 1;
        rt_h2d(X, P, W * 8, A);
        rt_h2d(Y, H.data(), W * 8, A);
        for (size_t i = 0; i < W; ++i) P[i] = H[i] = 2;  // after the enqueue
        CHECK(all(X, POISON) && all(Y, POISON));
        rt_sync(A);
        CHECK(all(X, 2) && all(Y, 1));
        // an offset into a page-locked block is page-locked too
        P[W - 1] = 3;
        rt_h2d(X, P + W - 1, 8, A);
        P[W - 1] = 4;
        rt_sync(A);
        CHECK(X[0] == 4);
        // pageable D2H holds the host: the stream is forced, the words are there on return
        k_fill(X, 5, A);
        k_fill(Y, 6, B);
        rt_d2h(H.data(), X, W * 8, A);
        CHECK(all(H.data(), 5) && all(Y, 1));  // B's work stays pending
        // page-locked D2H is an operation of its stream
        k_fill(X, 7, A);
        rt_d2h(P, X, W * 8, A);
        CHECK(!all(P, 7));
        rt_event_record(ev, A);
        rt_event_sync(ev);
        CHECK(all(P, 7));
        rt_sync(B);
        // d2d and memset are operations too
        rt_memset(X, 0, W * 8, A);
        rt_d2d(Y, X, W * 8, A);
        CHECK(all(X, 7) && all(Y, 6));
        rt_sync(A);
        CHECK(all(X, 0) && all(Y, 0));
        rt_host_free(P);
        rt_free(X); rt_free(Y);
    }
    {   // free: releasing device memory forces everything; releasing nothing forces nothing
        u64 *X = dev(), *Y = dev(), *Z = dev();
        k_fill(X, 8, A);
        k_fill(Y, 9, B);
        rt_free(nullptr);
        rt_host_free(nullptr);
        CHECK(all(X, POISON) && all(Y, POISON));
        rt_free(Z);
        CHECK(all(X, 8) && all(Y, 9));
        u64 *P = (u64 *)rt_host_malloc(8);
        k_fill(X, 1, A);
        rt_host_free(P);
        CHECK(all(X, 1));
        rt_free(X); rt_free(Y);
    }
    {   // the order is read only while nothing is pending: work enqueued behind pending work is deferred whatever the variable says
        u64 *X = dev(), *Y = dev();
        k_fill(X, 1, A);
        setenv("HHE_EMU_ORDER", "eager", 1);
        k_fill(Y, 2, B);
        CHECK(all(X, POISON) && all(Y, POISON));
        emu_device_sync();
        CHECK(all(X, 1) && all(Y, 2));
        setenv("HHE_EMU_ORDER", "lazy", 1);
        rt_free(X); rt_free(Y);
    }
    rt_event_destroy(ev); rt_event_destroy(ev2);
    rt_stream_destroy(A); rt_stream_destroy(B);
}

static void eager_rules(const char *value)
{
    if (value) setenv("HHE_EMU_ORDER", value, 1);
    else unsetenv("HHE_EMU_ORDER");
    const Stats s0 = stats();
    rt_stream A = rt_stream_create(), B = rt_stream_create();
    void *ev = rt_event_create();
    u64 *X = (u64 *)rt_malloc(W * 8), *Y = (u64 *)rt_malloc(W * 8);
    u64 *P = (u64 *)rt_host_malloc(W * 8);
    std::vector<u64> H(W, 3);
    // everything has run on return, streams and events mean nothing
    k_fill(X, 7, A);
    CHECK(all(X, 7));
    k_copy(Y, X, B);
    CHECK(all(Y, 7));
    CHECK(rt_event_record(ev, A) == 0 && rt_stream_wait_event(B, ev) == 0 && rt_event_sync(ev) == 0);
    rt_h2d(X, H.data(), W * 8, A);
    CHECK(all(X, 3));
    for (size_t i = 0; i < W; ++i) P[i] = 4;
    rt_h2d(Y, P, W * 8, B);
    CHECK(all(Y, 4));
    rt_d2h(P, X, W * 8, A);
    CHECK(all(P, 3));
    rt_memset(X, 0, W * 8, nullptr);
    CHECK(all(X, 0));
    rt_d2d(Y, X, W * 8, A);
    CHECK(all(Y, 0));
    CHECK(rt_sync(A) == 0 && rt_sync(nullptr) == 0);
    const Stats s1 = stats();
    CHECK(s1.deferred == s0.deferred && s1.forced == s0.forced && s1.forces == s0.forces);
    rt_host_free(P);
    rt_free(X); rt_free(Y);
    rt_event_destroy(ev);
    rt_stream_destroy(A); rt_stream_destroy(B);
}

int main()
{
    eager_rules(nullptr);
    eager_rules("eager");
    lazy_rules();
    eager_rules("eager");  // and back, in the same process
    const Stats s = stats();
    CHECK(s.deferred > 0 && s.forced == s.deferred && s.forces > 0 && s.max_pending >= 4);
    printf("stream_order OK: %llu deferred, %llu forces, %llu pending at most\n", (unsigned long long)s.deferred,
           (unsigned long long)s.forces, (unsigned long long)s.max_pending);
    return 0;
}

// emu_order.cpp -- TESTS ONLY.  The device runtime of csrc/hhe_launch.h for the emulator, with a model of what HIP promises about
// the order of asynchronous work and nothing more.
//
// HHE_EMU_ORDER unset or "eager" (the default): every operation runs inside the call that enqueues it; streams and events mean
// nothing.  The host schedule cannot be wrong in a way this order shows.
//
// HHE_EMU_ORDER=lazy: an operation runs as LATE as the stream semantics allow.
//   * Every kernel launch, rt_h2d, rt_d2d, rt_memset, and rt_d2h into page-locked memory is appended to the FIFO of its stream.  The
//     NULL stream is a stream like any other: the library's own streams are non-blocking, nothing is ordered with it implicitly.
//   * rt_event_record appends a marker.  rt_stream_wait_event binds to the record enqueued last at the time of the call (none: no-op).
//   * Force points: rt_sync and rt_stream_destroy (that stream), rt_event_sync (up to the bound record), rt_d2h into pageable memory
//     (HIP holds the host there: the stream, then the copy), rt_free / rt_host_free (hipFree waits for the whole device: everything).
//   * A force runs, for every wait marker in the prefix of its stream up to the point, the other stream's prefix up to the bound
//     record (recursively, in order of appearance), THEN the prefix itself -- and NOTHING else.  That is the adversary, and it is
//     deterministic: work the schedule did not order before the forcing point stays pending and runs after its consumer; work of
//     another stream that was ordered only at a join runs before everything this stream enqueued ahead of the join, unless it was
//     made to wait for that too (the fork).  A cycle of waits aborts.
//   * rt_h2d out of page-locked memory (rt_host_malloc) reads the host buffer when it runs; out of pageable memory the bytes are
//     taken at the call, as the runtime's staging copy does.
//   * New device and page-locked memory is filled with a poison word, so something read before it was written shows in the output.
// The order is read from the environment whenever nothing is pending, so one loaded library serves eager and lazy contexts of one
// process.  One mutex guards the queues; operations of the lazy order run under it, those of the eager order outside it (contexts
// on two threads overlap as before).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include <sys/mman.h>
#include "emu_order.h"

namespace {

// The poison word is the address of a large readable and writable mapping of zeros.  A schedule bug then shows as wrong words in
// a failing test, not as a crash of the whole session: a pointer table read before its upload ran leads the kernel bodies into the
// mapping, and both 32-bit halves of the word are small (an index table read too early stays near its array).  The fixed place is
// only preferred; where it is taken the mapping lies wherever the system puts it.
constexpr size_t POISON_SPAN = (size_t)4 << 30;
uint64_t poison_word()
{
    static const uint64_t word = [] {
        void *want = (void *)0x1000001000ULL;
        void *p = mmap(want, POISON_SPAN, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE | MAP_FIXED_NOREPLACE, -1, 0);
        if (p == MAP_FAILED) p = mmap(nullptr, POISON_SPAN, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) { fprintf(stderr, "emu: no room for the poison mapping\n"); abort(); }
        return (uint64_t)p;
    }();
    return word;
}
void poison_fill(void *p, size_t bytes)
{
    const uint64_t w = poison_word();
    for (size_t i = 0; i + 8 <= bytes; i += 8) memcpy((char *)p + i, &w, 8);
    memcpy((char *)p + (bytes & ~(size_t)7), &w, bytes & 7);
}

enum OpKind { OP_RUN, OP_RECORD, OP_WAIT };
struct Op {
    OpKind kind;
    std::function<void()> fn;  // OP_RUN
    uint64_t sid, pos;         // OP_WAIT: the other stream (by id) and the length of its prefix that must have run
    bool resolved = false;     // OP_WAIT: that prefix has been forced
};
struct Stream {
    uint64_t id;
    std::deque<Op> q;           // operations [done, enq) of the stream
    uint64_t done = 0, enq = 0;
    std::vector<uint64_t> resolving;  // the wait markers of this stream a force is inside of (cycle detection)
};
struct Event {
    bool recorded = false;
    uint64_t sid = 0, pos = 0;  // the last record: stream id (0: nothing left to wait for) and the prefix that ends with its marker
};

std::mutex g_mu;
std::map<rt_stream, Stream *> g_by_handle;
std::map<uint64_t, std::unique_ptr<Stream>> g_by_id;  // the owner, in order of creation: the order in which "everything" is forced
std::map<const char *, size_t> g_host; // page-locked allocations
uint64_t g_next_id = 0, g_pending = 0;
uint64_t g_deferred = 0, g_forced_ops = 0, g_max_pending = 0, g_forces = 0;
bool g_lazy = false;

bool lazy_now()  // g_mu held
{
    if (!g_pending) {
        const char *e = getenv("HHE_EMU_ORDER");
        if (e && *e && strcmp(e, "eager") && strcmp(e, "lazy")) { fprintf(stderr, "emu: HHE_EMU_ORDER must be eager or lazy\n"); abort(); }
        g_lazy = e && !strcmp(e, "lazy");
    }
    return g_lazy;
}
Stream *stream_of(rt_stream h)  // g_mu held; a handle the library did not create is the caller's stream (NULL included)
{
    auto it = g_by_handle.find(h);
    if (it != g_by_handle.end()) return it->second;
    Stream *s = new Stream;
    s->id = ++g_next_id;
    g_by_handle[h] = s;
    g_by_id[s->id].reset(s);
    return s;
}
void append(Stream *s, Op op)
{
    s->q.push_back(std::move(op));
    ++s->enq;
    if (++g_pending > g_max_pending) g_max_pending = g_pending;
}
// g_mu held.  Two passes over the prefix.  First everything its wait markers are bound to, in order of appearance: another stream's
// work is ordered with this stream's only through those markers, so it may run BEFORE this stream's earlier operations -- a lane that
// was not made to wait for the fork runs ahead of what the main stream enqueued before it.  Then the stream's own operations.
void run_to(Stream *s, uint64_t upto)
{
    if (s->done >= upto) return;
    if (!s->resolving.empty() && upto > s->resolving.back()) {
        fprintf(stderr, "emu: cycle of stream waits: a stream waits for a record behind its own wait\n");
        abort();
    }
    for (uint64_t i = s->done; i < upto; ++i) {
        if (i < s->done) continue;  // a nested force of this stream has run past it
        Op &op = s->q[i - s->done];
        if (op.kind != OP_WAIT || op.resolved) continue;
        op.resolved = true;
        const uint64_t sid = op.sid, pos = op.pos;
        auto it = g_by_id.find(sid);
        if (it == g_by_id.end()) continue;  // a destroyed stream has run completely
        s->resolving.push_back(i);
        run_to(it->second.get(), pos);
        s->resolving.pop_back();
    }
    while (s->done < upto) {
        Op op = std::move(s->q.front());
        s->q.pop_front();
        if (op.kind == OP_RUN) { op.fn(); ++g_forced_ops; }
        ++s->done;
        --g_pending;
    }
}
void force_all()
{
    for (auto &kv : g_by_id) run_to(kv.second.get(), kv.second->enq);
}
bool page_locked(const void *p)
{
    auto it = g_host.upper_bound((const char *)p);
    if (it == g_host.begin()) return false;
    --it;
    return (const char *)p < it->first + it->second;
}
void enqueue_or_run(rt_stream h, std::function<void()> op)
{
    {
        std::lock_guard<std::mutex> l(g_mu);
        if (lazy_now()) {
            append(stream_of(h), Op{OP_RUN, std::move(op), 0, 0, false});
            ++g_deferred;
            return;
        }
    }
    op();
}

}  // namespace

void emu_enqueue(rt_stream s, std::function<void()> op) { enqueue_or_run(s, std::move(op)); }

extern "C" void emu_order_stats(uint64_t out[4])
{
    std::lock_guard<std::mutex> l(g_mu);
    out[0] = g_deferred; out[1] = g_forced_ops; out[2] = g_max_pending; out[3] = g_forces;
}
extern "C" void emu_device_sync()
{
    std::lock_guard<std::mutex> l(g_mu);
    if (g_pending) { ++g_forces; force_all(); }
}
extern "C" uint64_t emu_poison_word() { return poison_word(); }
extern "C" void emu_order_window()
{
    std::lock_guard<std::mutex> l(g_mu);
    g_max_pending = g_pending;
}

const char *rt_backend_name() { return "cpu-emulator(tests-only)"; }
const char *rt_last_error() { return "emu"; }
int rt_set_device(int) { return 0; }

void *rt_malloc(size_t b)
{
    if (!b) b = 8;
    void *p = malloc(b);
    std::lock_guard<std::mutex> l(g_mu);
    if (p && lazy_now()) poison_fill(p, b);
    return p;
}
// hipFree waits for the whole device before it releases the block.  That wait is also what hides a use-after-free of the host
// schedule on the GPU: work still in flight on ANY stream finishes before the memory goes, so freeing a buffer a lane still reads
// is not visible there either -- only a release that does not pass through the runtime (a pooled allocator) would show it.
void rt_free(void *p)
{
    if (!p) return;  // hipFree(nullptr) returns at once
    {
        std::lock_guard<std::mutex> l(g_mu);
        if (g_pending) { ++g_forces; force_all(); }
    }
    free(p);
}
void *rt_host_malloc(size_t b)
{
    if (!b) b = 8;
    void *p = malloc(b);
    if (!p) return nullptr;
    std::lock_guard<std::mutex> l(g_mu);
    g_host[(const char *)p] = b;
    if (lazy_now()) poison_fill(p, b);
    return p;
}
void rt_host_free(void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> l(g_mu);
        if (g_pending) { ++g_forces; force_all(); }  // hipHostFree waits like hipFree
        g_host.erase((const char *)p);
    }
    free(p);
}

int rt_h2d(void *d, const void *s, size_t n, rt_stream st)
{
    bool pinned;
    {
        std::lock_guard<std::mutex> l(g_mu);
        if (!lazy_now()) pinned = true;  // runs at once either way
        else pinned = page_locked(s);
    }
    if (pinned) { enqueue_or_run(st, [=] { memcpy(d, s, n); }); return 0; }
    auto staged = std::make_shared<std::vector<char>>((const char *)s, (const char *)s + n);  // the caller may rewrite its array on return
    enqueue_or_run(st, [=] { memcpy(d, staged->data(), n); });
    return 0;
}
int rt_d2h(void *d, const void *s, size_t n, rt_stream st)
{
    {
        std::lock_guard<std::mutex> l(g_mu);
        if (lazy_now() && !page_locked(d)) {  // pageable: the host is held until the copy is done
            Stream *q = stream_of(st);
            ++g_forces;
            run_to(q, q->enq);
            memcpy(d, s, n);
            return 0;
        }
    }
    enqueue_or_run(st, [=] { memcpy(d, s, n); });
    return 0;
}
int rt_d2d(void *d, const void *s, size_t n, rt_stream st) { enqueue_or_run(st, [=] { memmove(d, s, n); }); return 0; }
int rt_memset(void *d, int v, size_t n, rt_stream st) { enqueue_or_run(st, [=] { memset(d, v, n); }); return 0; }

int rt_sync(rt_stream st)
{
    std::lock_guard<std::mutex> l(g_mu);
    if (!lazy_now()) return 0;
    Stream *s = stream_of(st);
    ++g_forces;
    run_to(s, s->enq);
    return 0;
}
rt_stream rt_stream_create()
{
    std::lock_guard<std::mutex> l(g_mu);
    Stream *s = new Stream;
    s->id = ++g_next_id;
    g_by_handle[(rt_stream)s] = s;
    g_by_id[s->id].reset(s);
    return (rt_stream)s;
}
void rt_stream_destroy(rt_stream st)
{
    std::lock_guard<std::mutex> l(g_mu);
    auto it = g_by_handle.find(st);
    if (it == g_by_handle.end()) return;
    Stream *s = it->second;
    if (s->enq > s->done) { ++g_forces; run_to(s, s->enq); }
    g_by_handle.erase(it);
    g_by_id.erase(s->id);
}
void *rt_event_create() { return new Event; }
void rt_event_destroy(void *ev) { delete (Event *)ev; }
void *rt_event_create_timed() { return new Event; }
float rt_event_elapsed_ms(void *, void *) { return 0.f; }
int rt_event_record(void *ev, rt_stream st)
{
    if (!ev) return -1;
    Event *e = (Event *)ev;
    std::lock_guard<std::mutex> l(g_mu);
    e->recorded = true;
    if (!lazy_now()) { e->sid = 0; e->pos = 0; return 0; }
    Stream *s = stream_of(st);
    append(s, Op{OP_RECORD, nullptr, 0, 0, false});
    e->sid = s->id;
    e->pos = s->enq;
    return 0;
}
int rt_event_sync(void *ev)
{
    if (!ev) return -1;
    Event *e = (Event *)ev;
    std::lock_guard<std::mutex> l(g_mu);
    if (!e->recorded || !e->sid) return 0;
    auto it = g_by_id.find(e->sid);
    if (it == g_by_id.end()) return 0;
    ++g_forces;
    run_to(it->second.get(), e->pos);
    return 0;
}
int rt_stream_wait_event(rt_stream st, void *ev)
{
    if (!ev) return -1;
    Event *e = (Event *)ev;
    std::lock_guard<std::mutex> l(g_mu);
    if (!lazy_now() || !e->recorded || !e->sid) return 0;
    append(stream_of(st), Op{OP_WAIT, nullptr, e->sid, e->pos, false});
    return 0;
}

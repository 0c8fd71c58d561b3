// emu_order.h -- TESTS ONLY.  The stream model of the emulator (emu_order.cpp): the device runtime of csrc/hhe_launch.h (rt_*) and
// the one call through which a launcher hands its work to a stream.
#pragma once
#include <cstdint>
#include <functional>
#include "hhe_launch.h"

// `op` is one operation of stream `s` (a kernel launch, captured by value).  Eager order: it runs before the call returns.  Lazy
// order (HHE_EMU_ORDER=lazy): it is appended to the stream's FIFO and runs when something forces the stream up to it.
void emu_enqueue(rt_stream s, std::function<void()> op);

extern "C" {
// out[0] operations deferred (lazy order), out[1] operations that ran at a force point, out[2] the largest number pending at once,
// out[3] forces -- since the library was loaded (out[2]: since the last emu_order_window).  A test of the lazy order that sees
// out[0] unchanged has tested nothing.
void emu_order_stats(uint64_t out[4]);
// starts a new window for out[2]: the largest number pending at once is counted from what is pending now
void emu_order_window();
// hipDeviceSynchronize: runs everything pending on every stream
void emu_device_sync();
// the word rt_malloc / rt_host_malloc fill new memory with under the lazy order: the address of a readable mapping of zeros
uint64_t emu_poison_word();
}

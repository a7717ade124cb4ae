// device_blocks.hpp -- the small persistent device allocation a forward chain keeps per (host thread, device, stream) for the counters
// its workgroups bump with atomics.  The chain's kernels put the zeros back themselves, so no zero-fill launch precedes a forward -- and
// so two calls in flight must not share a block: hence one per stream.  A chain keeps one thread_local instance: the blocks are freed
// when the thread exits or on r2_thread_release(), and a thread that cycles through more streams than the table holds evicts the least
// recently used block (round 4: never freed, and the fast paths silently switched themselves off after 64 / 256 streams -- ADVICE r4).
// dirty: a chain armed the block's counters and has not yet seen them reset by its own kernels.  Found dirty by the next call -- one
// that aborted half way -- the block is zero-filled first.
#pragma once
#include "host_tables.hpp"
#include <hip/hip_runtime.h>
#include <utility>

namespace r2 {

class DeviceBlocks {
public:
    // the block of (dev, s), `bytes` long (the same for every call of one instance), all zero on the stream before the caller's first
    // kernel and marked dirty until clean(); nullptr: no block can be had
    void *acquire(int dev, hipStream_t s, size_t bytes)
    {
        Block *b = blocks_.find_or_insert({dev, s});
        if (!b->p && hipMalloc(&b->p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            b->p = nullptr;
            return nullptr;
        }
        if (b->dirty && hipMemsetAsync(b->p, 0, bytes, s) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        b->dirty = true;
        return b->p;
    }
    // the block of (dev, s) has been through a whole call: its kernels have put the zeros back
    void clean(int dev, hipStream_t s)
    {
        if (Block *b = blocks_.find({dev, s})) b->dirty = false;
    }
    void release() { blocks_.clear(); }

private:
    struct Block { void *p = nullptr; bool dirty = true; };
    struct Free {
        void operator()(const std::pair<int, hipStream_t> &key, Block &b) const
        {
            int cur = 0;
            if (!b.p) return;
            if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); return; }
            if (cur != key.first && hipSetDevice(key.first) != hipSuccess) { (void)hipGetLastError(); return; }
            if (hipFree(b.p) != hipSuccess) (void)hipGetLastError();   // (its last call may still run: hipFree waits for the device)
            if (cur != key.first) (void)hipSetDevice(cur);
        }
    };
    LruTable<std::pair<int, hipStream_t>, Block, 16, Free> blocks_;
};

}  // namespace r2

// Host only: a library-owned device ring, allocated on first use, whose slices are handed out in call order.  A slice comes round
// again RING elements later — long after the launch that used it has retired (launches of one stream run in order, a training
// step ends with a join of its streams); a captured graph keeps the slices of its nodes, and graphs / eager steps of one engine
// never run at the same time.  One call may take at most CAP elements.  ZERO: the ring is zeroed once, for users that leave their
// slice at zero (arrival counters).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>

template <typename T, size_t RING, size_t CAP, bool ZERO>
class T2VRing {
    T* ring_ = nullptr;
    std::atomic<size_t> pos_{0};
    std::atomic<int> state_{0};         // 0 = not allocated, 1 = a thread is allocating, 2 = there
public:
    // false when the ring cannot be allocated: the runtime's error is cleared (the caller falls back or reports it itself) and
    // the next call tries again
    bool available() {
        if (state_.load(std::memory_order_acquire) == 2) return true;
        int expect = 0;
        if (state_.compare_exchange_strong(expect, 1)) {
            T* p = nullptr;
            bool ok = hipMalloc((void**)&p, RING * sizeof(T)) == hipSuccess;
            if (ok && ZERO) ok = hipMemset(p, 0, RING * sizeof(T)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
            if (!ok) { (void)hipGetLastError(); state_.store(0); return false; }
            ring_ = p;
            state_.store(2, std::memory_order_release);
            return true;
        }
        while (state_.load(std::memory_order_acquire) == 1) { }
        return state_.load() == 2;
    }
    // the next n elements, or nullptr (n over the cap, no ring); a slice that would wrap starts over at the top
    T* take(size_t n) {
        if (n > CAP || !available()) return nullptr;
        size_t at = pos_.fetch_add(n) % RING;
        if (at + n > RING) { pos_.store(n); at = 0; }
        return ring_ + at;
    }
};

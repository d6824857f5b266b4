// Slot bookkeeping of the round driver's upload ring (plain C++; the HIP
// calls are passed in, so a host-only check can drive it with fakes).
//
// A slot is handed out round-robin. It stays busy from acquire() until the
// work recorded for it has completed; acquire() asks `done(i)` and, where
// that says no, calls `wait(i)`, which must block until it has. A busy slot
// is never handed out without one of the two having vouched for it.
#pragma once

#include <cstddef>

template <int N>
class SlotRing {
public:
    SlotRing()
    {
        for (int i = 0; i < N; ++i) busy_[i] = false;
    }

    template <typename Done, typename Wait>
    int acquire(Done&& done, Wait&& wait)
    {
        int i = next_;
        if (busy_[i] && !done(i)) wait(i);
        busy_[i] = true;
        next_ = (i + 1) % N;
        return i;
    }

    // acquire() handed slot i out but nothing was recorded for it (the
    // enqueue failed): it holds no work, and it is the next one again
    void abandon(int i)
    {
        busy_[i] = false;
        next_ = i;
    }

    bool busy(int i) const { return busy_[i]; }
    static constexpr int size() { return N; }

private:
    bool busy_[N];
    int next_ = 0;
};

// Capacity after growth: geometric, and at least what is needed now.
static inline size_t grown_capacity(size_t have, size_t need)
{
    if (need <= have) return have;
    size_t cap = have ? have : 256;
    while (cap < need) cap *= 2;
    return cap;
}

// The owner of a context's stream-ordered device memory (DevArena), the typed
// growable array allocated from it (DevBuf) and the capacity policy of every
// buffer group (grown_cap).  Host-only and free of HIP: the allocator is a
// policy `Mem` with stream_t, error_t (value-initialised: success) and
//   error_t alloc_async(void **p, size_t bytes, stream_t st)
//   error_t free_async(void *p, stream_t st)
//   void free_now(void *p)
// (curve_ctx.hpp: the HIP calls; tests/host/test_devbuf.cpp: malloc, counted).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace zmqg {

// The capacity for `need`: `cur` when that fits, else "current or floor, doubled
// until it reaches need".
inline uint64_t grown_cap(uint64_t cur, uint64_t floor, uint64_t need)
{
    if (need <= cur)
        return cur;
    uint64_t cap = cur ? cur : floor;
    while (cap < need)
        cap *= 2;
    return cap;
}

// Records what it has handed out (growth is rare and there are a few dozen
// entries: a vector), so the context frees everything with one call.
template <class Mem>
struct DevArena {
    typedef typename Mem::stream_t stream_t;
    typedef typename Mem::error_t error_t;
    std::vector<void *> held;

    error_t alloc(void **p, size_t bytes, stream_t st)
    {
        held.reserve(held.size() + 1); // (recording cannot fail after the allocation)
        const error_t e = Mem::alloc_async(p, bytes, st);
        if (e == error_t())
            held.push_back(*p);
        return e;
    }
    error_t release(void *p, stream_t st)
    {
        const error_t e = Mem::free_async(p, st);
        if (e == error_t())
            held.erase(std::find(held.begin(), held.end(), p));
        return e;
    }
    void free_all() // not stream-ordered: once the streams are idle
    {
        for (void *p : held)
            Mem::free_now(p);
        held.clear();
    }
};

// `count` elements of T plus kSlack bytes.  Either {null, 0} or an array with
// room for `count` elements; reads as its pointer at the launch sites.
template <class T, size_t kSlack = 64>
struct DevBuf {
    T *p = nullptr;
    size_t count = 0;

    operator T *() const { return p; }

    // Room for n elements on `st`: nothing when n fits.  Else the old array is
    // released before the new one is allocated (the contents are not kept; peak
    // memory does not rise), and a failure leaves {null, 0}.
    template <class Arena>
    typename Arena::error_t reserve(Arena &a, size_t n, typename Arena::stream_t st)
    {
        typedef typename Arena::error_t error_t;
        error_t e = error_t();
        if (n <= count || (p && (e = a.release(p, st)) != error_t()))
            return e;
        p = nullptr;
        count = 0;
        if ((e = a.alloc((void **) &p, n * sizeof(T) + kSlack, st)) == error_t())
            count = n;
        else
            p = nullptr;
        return e;
    }
};

} // namespace zmqg

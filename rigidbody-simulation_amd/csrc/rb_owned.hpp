// rb_owned.hpp — the two owners of a world's memory (host units only): device
// memory and pinned host memory.  Move-only; what one holds is released when
// it is reset, replaced or destroyed, with the device of its allocation
// current (free_world, and every entry point, sets the world's).  Allocation
// reports through fail(): RB_ENOMEM out of memory, RB_ENODEV otherwise.
#pragma once
#include <stddef.h>

namespace rb {
namespace host __attribute__((visibility("hidden"))) {

// A device buffer that only grows: afterwards *buf holds `need` bytes or more.
// (The capacity is zero while the buffer is being replaced: an error in between
// leaves an empty buffer, not a dangling one.)
int grow(void **buf, size_t *cap, size_t need);

struct DevMem {
    void *p = nullptr;
    size_t bytes = 0;
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevMem &operator=(DevMem &&o) noexcept {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevMem() { reset(); }
    void reset();                                               // empty
    int grow(size_t need) { return host::grow(&p, &bytes, need); }
    int alloc(size_t n) { reset(); return grow(n); }            // exactly n bytes, in place of what it held
    int alloc_uncached(size_t n);                               // the same, fine-grained and uncached (a mailbox peers write)
};
template <typename T> struct DevBuf : DevMem {
    T *get() const { return static_cast<T *>(p); }
    operator T *() const { return get(); }
};

struct HostMem {
    void *p = nullptr, *d = nullptr;
    HostMem() = default;
    HostMem(HostMem &&o) noexcept : p(o.p), d(o.d) { o.p = o.d = nullptr; }
    HostMem &operator=(HostMem &&o) noexcept {
        if (this != &o) { reset(); p = o.p; d = o.d; o.p = o.d = nullptr; }
        return *this;
    }
    ~HostMem() { reset(); }
    void reset();
    // n pinned bytes (hipHostMalloc's flags); with hipHostMallocMapped among them, d is their device alias
    int alloc(size_t n, unsigned flags = 0);
};
template <typename T> struct HostBuf : HostMem {
    T *get() const { return static_cast<T *>(p); }
    operator T *() const { return get(); }
    T *dev() const { return static_cast<T *>(d); }
};

}  // namespace host
}  // namespace rb

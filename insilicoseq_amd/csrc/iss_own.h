// iss_own.h -- the one owning handle of the host side (plain C++17, no HIP: tests/own_host_main.cpp instantiates it with a counting
// release).  Owned<T, Free> holds a T* that its struct allocated and releases it exactly once; a raw T* beside it is a view into
// somebody else's block.  It converts to T*, so reads of a handle are written like reads of a pointer.
#pragma once

#include <utility>

namespace iss_own {

template <typename T, void (*Free)(void *)>
struct Owned {
    Owned() = default;
    explicit Owned(T *p) : p_(p) {}
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p_(o.release()) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) reset(o.release());
        return *this;
    }
    ~Owned() { reset(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    // releases what is held, then holds p
    void reset(T *p = nullptr) {
        T *old = std::exchange(p_, p);
        if (old) Free(const_cast<void *>(static_cast<const void *>(old)));
    }
    // gives the pointer up without releasing it
    T *release() { return std::exchange(p_, nullptr); }

private:
    T *p_ = nullptr;
};

}  // namespace iss_own

// Move-only owning handles for what the engine's lazily allocated features hold: device memory, pinned host memory, a timing-disabled event.  One pointer wide; the
// resource kind is a policy { static void *acquire(size_t bytes); static void release(void *) noexcept; } so that the handle's own logic can be checked on the host
// against a stub (tests/c/owned_check.cpp defines MG4_OWNED_NO_HIP and brings its own policy).
// All-or-nothing allocation of a group needs no code of its own: allocate into locals, then move them into the members -- a throw in between frees the locals.
#pragma once
#include <cstddef>
#include <utility>

namespace mg4 {

template <typename T, typename Kind> class Owned {
    T *p_ = nullptr;
public:
    Owned() = default;
    explicit Owned(size_t bytes) : p_(static_cast<T *>(Kind::acquire(bytes))) {}   // acquire throws on failure
    Owned(Owned &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    void reset() noexcept { if (p_) Kind::release(p_); p_ = nullptr; }
    void abandon() noexcept { p_ = nullptr; }                                // leak on purpose (Engine::~Engine with a stream that never drains)
    T *get() const { return p_; }
    operator T *() const { return p_; }                                      // reads like the raw pointer it replaces: tests, arithmetic, kernel arguments
    template <typename U> U *as() const { return reinterpret_cast<U *>(p_); }
};
template <typename... H> inline void reset_all(H &...h) noexcept { (h.reset(), ...); }
template <typename... H> inline void abandon_all(H &...h) noexcept { (h.abandon(), ...); }

}  // namespace mg4

#ifndef MG4_OWNED_NO_HIP
#include <type_traits>

#include "common.hpp"
namespace mg4 {
struct DeviceMem { static void *acquire(size_t bytes) { void *p = nullptr; HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1)); return p; } static void release(void *p) noexcept { HIP_IGNORE(hipFree(p)); } };
struct PinnedMem { static void *acquire(size_t bytes) { void *p = nullptr; HIP_CHECK(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault)); return p; } static void release(void *p) noexcept { HIP_IGNORE(hipHostFree(p)); } };
struct WaitEvent {   // hipEventDisableTiming: something to wait on, never to measure with
    static void *acquire(size_t) { hipEvent_t e = nullptr; HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return e; }
    static void release(void *e) noexcept { HIP_IGNORE(hipEventDestroy(static_cast<hipEvent_t>(e))); }
};
struct SideStream {   // a non-blocking stream next to the context's own (copies that overlap its kernels); ordered against it with events only
    static void *acquire(size_t) { hipStream_t s = nullptr; HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return s; }
    static void release(void *s) noexcept { HIP_IGNORE(hipStreamDestroy(static_cast<hipStream_t>(s))); }
};
using OwnedStream = Owned<std::remove_pointer_t<hipStream_t>, SideStream>;  // converts to hipStream_t; OwnedStream(0) creates it
template <typename T> using DevPtr = Owned<T, DeviceMem>;
template <typename T> using PinPtr = Owned<T, PinnedMem>;
using OwnedEvent = Owned<std::remove_pointer_t<hipEvent_t>, WaitEvent>;     // converts to hipEvent_t; OwnedEvent(0) creates it
}  // namespace mg4
#endif

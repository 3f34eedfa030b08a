// owned_hip.h -- the owners of owned.h on HIP: device and page-locked memory, streams, events and id tables as members of a handle, and the one rule by which a
// handle is destroyed.  A handle declares its stream before its buffers, so that the buffers go first and the stream last.  Host code only.
#pragma once
#include "host_util.h"
#include "device_util.h"
#include "owned.h"

struct DevAlloc { static hipError_t alloc(void** out, size_t bytes) { return hipMalloc(out, bytes); } static void release(void* p) { (void)hipFree(p); } };
struct PinnedAlloc { static hipError_t alloc(void** out, size_t bytes) { return hipHostMalloc(out, bytes, hipHostMallocDefault); } static void release(void* p) { (void)hipHostFree(p); } };
typedef Owned<DevAlloc> DevMem;
typedef Owned<PinnedAlloc> PinnedMem;
typedef OwnedList<DevAlloc> DevList;
typedef OwnedTable<DevAlloc, CorbIdTable> OwnedIdTable;

inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }

// a non-blocking stream.  Destruction destroys it and waits for nothing: whoever destroys a handle synchronises first (handle_destroy)
class OwnedStream {
    hipStream_t s_ = nullptr;
public:
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    OwnedStream(OwnedStream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    OwnedStream& operator=(OwnedStream&& o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~OwnedStream() { reset(); }
    hipError_t create() { reset(); return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    operator hipStream_t() const { return s_; }
};

class OwnedEvent {
    hipEvent_t e_ = nullptr;
public:
    OwnedEvent() = default;
    OwnedEvent(const OwnedEvent&) = delete;
    OwnedEvent& operator=(const OwnedEvent&) = delete;
    OwnedEvent(OwnedEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    OwnedEvent& operator=(OwnedEvent&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
    ~OwnedEvent() { reset(); }
    hipError_t create(unsigned int flags) { reset(); return hipEventCreateWithFlags(&e_, flags); }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    operator hipEvent_t() const { return e_; }
};

// The destroy rule of every handle: the device (a failed selection is not an obstacle: what the handle holds is released all the same), the pending work of the
// handle's stream if it has one, then the members in reverse order of declaration.  What is not memory (a communicator, captured graphs) is the caller's, before.
template <class H> auto handle_stream(H* h, int) -> decltype((hipStream_t)h->stream) { return h->stream; }
template <class H> hipStream_t handle_stream(H*, long) { return nullptr; }
template <class H> void handle_destroy(H* h)
{
    if (!h) return;
    (void)corb_select_device(h->device);
    if (hipStream_t s = handle_stream(h, 0)) (void)hipStreamSynchronize(s);
    delete h;
}

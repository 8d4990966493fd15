// hip_own.h -- owners of what the host code of render_kernels.hip acquires from HIP: device memory, streams, events and the
// current device.  Each is move-only and gives back what it holds in its destructor, so that an early return releases
// everything.  Host code only: no kernel reads this file.  (DESIGN.md "Ownership of device resources".)
#pragma once
#include <hip/hip_runtime.h>

namespace apt {

// Device memory of `count` elements of T.  hipFree waits for the device, so memory a kernel may still read is released safely.
template <class T> class DeviceBuffer {
    T *p_ = nullptr;
  public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(T *owned) : p_(owned) {}                 // takes over what release() or hipMalloc handed out
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.release()) {}
    ~DeviceBuffer() { if (p_) (void)hipFree(p_); }
    hipError_t alloc(size_t count) { return hipMalloc(&p_, count * sizeof(T)); }   // once, on an empty buffer
    T *get() const { return p_; }
    T *release() { T *p = p_; p_ = nullptr; return p; }            // hands ownership on
};

class Stream {
    hipStream_t s_ = nullptr;
  public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s_, flags); }
    hipStream_t get() const { return s_; }
};

class Event {
    hipEvent_t e_ = nullptr;
  public:
    Event() = default;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    hipError_t create() { return hipEventCreate(&e_); }
    hipEvent_t get() const { return e_; }
};

// Makes a device current again on the way out: the one current now (none when that cannot be read), or the one named.
class DeviceScope {
    int dev_ = -1;
  public:
    DeviceScope() { if (hipGetDevice(&dev_) != hipSuccess) dev_ = -1; }
    explicit DeviceScope(int dev) : dev_(dev) {}
    ~DeviceScope() { if (dev_ >= 0) (void)hipSetDevice(dev_); }
};

} // namespace apt

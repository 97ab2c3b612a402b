// rf_hip_host.hpp -- what the host side of every HIP unit shares: the error check, the owner of a device allocation, the owner of a stream and the device check.
// Host code only: nothing here is compiled for the device.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <stdexcept>
#include <string>

#define RF_HIP(expr)                                                                                          \
    do                                                                                                        \
    {                                                                                                         \
        const hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                                 \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " in " #expr);      \
    } while (0)

namespace rf
{
// One device allocation of `count` elements, freed with its owner.  alloc / upload replace what is held (synchronous: the caller knows that nothing still uses it);
// ensure only ever grows.
template<typename T>
struct DeviceBuffer
{
    T*     ptr = nullptr;
    size_t count = 0;

    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }

    void alloc(size_t n)
    {
        release();
        if (n) RF_HIP(hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T)));
        count = n;
    }
    void ensure(size_t n)
    {
        if (n > count) alloc(n);
    }
    void upload(const T* src, size_t n)
    {
        alloc(n);
        if (n) RF_HIP(hipMemcpy(ptr, src, n * sizeof(T), hipMemcpyHostToDevice));
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
};

// -> the number of HIP devices; std::runtime_error when there is none
inline int requireAnyDevice()
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) throw std::runtime_error("rayfinder_amd: no HIP device available (this library has no CPU fallback)");
    return count;
}

// Make device `ordinal` current; std::runtime_error when there is no device, std::invalid_argument when the ordinal names none
inline void requireDevice(int ordinal)
{
    const int count = requireAnyDevice();
    if (ordinal < 0 || ordinal >= count) throw std::invalid_argument("device ordinal out of range");
    RF_HIP(hipSetDevice(ordinal));
}

// A non-blocking stream of device `deviceOrdinal` (made current: requireDevice), for the length of a scope: synchronised, then destroyed.  The buffers its work uses
// are declared AFTER it and a Drain after them, so that leaving the scope -- by return or by exception -- synchronises the stream, frees the buffers and destroys the
// stream, in that order (StagedFrame, rf_frame_sums.hpp, is the one place that does).
struct ScopedStream
{
    hipStream_t handle = nullptr;

    explicit ScopedStream(int deviceOrdinal)
    {
        requireDevice(deviceOrdinal);
        RF_HIP(hipStreamCreateWithFlags(&handle, hipStreamNonBlocking));
    }
    ScopedStream(const ScopedStream&) = delete;
    ScopedStream& operator=(const ScopedStream&) = delete;
    ~ScopedStream()
    {
        (void)hipStreamSynchronize(handle);
        (void)hipStreamDestroy(handle);
    }

    struct Drain
    {
        const ScopedStream& stream;
        ~Drain() { (void)hipStreamSynchronize(stream.handle); }
    };
};
} // namespace rf

// somar_amd/csrc/devbuf.h -- the one owner of device memory: every hipMalloc / hipFree of the library is in here.
// Kernel-facing structs (LevelDev, BoxBicg, MetricPtrs, ...) and the C ABI stay plain views of raw pointers, filled from get().
#pragma once
#include <atomic>
#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"

namespace somar {

// bytes held by every live DevBuf of the process (somar_device_bytes_live): exact where hipMemGetInfo, on a device that other
// processes use at the same moment, is not
inline std::atomic<long long>& device_bytes_live()
{
    static std::atomic<long long> live{0};
    return live;
}

template <class T>
class DevBuf {
public:
    DevBuf() noexcept {}
    explicit DevBuf(size_t n) : n_(n)   // uninitialised
    {
        SOMAR_HIP(hipMalloc(&p_, n * sizeof(T)));
        device_bytes_live() += (long long)(n * sizeof(T));
    }
    static DevBuf zeros(size_t n)   // enqueues the memset; the caller synchronises where it has to
    {
        DevBuf b(n);
        SOMAR_HIP(hipMemset(b.p_, 0, n * sizeof(T)));
        return b;
    }
    static DevBuf from(const std::vector<T>& v)   // empty for an empty vector
    {
        if (v.empty()) return DevBuf();
        DevBuf b(v.size());
        SOMAR_HIP(hipMemcpy(b.p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return b;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() noexcept
    {
        if (!p_) return;
        (void)hipFree(p_);
        device_bytes_live() -= (long long)(n_ * sizeof(T));
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    // a view for launches and kernel-facing structs; not of a temporary, which would free it at once
    operator T*() const& { return p_; }
    operator T*() const&& = delete;

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

static_assert(!std::is_copy_constructible<DevBuf<double>>::value && std::is_nothrow_move_constructible<DevBuf<double>>::value,
              "DevBuf is move-only");

}  // namespace somar

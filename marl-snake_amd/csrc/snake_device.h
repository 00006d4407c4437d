// snake_device.h -- DeviceGuard, shared by the launchers of snake_kernels.hip
// (snake_launch.inc), policy_kernels.hip and greedy_kernels.hip, and the byte
// test the last two share. Include after <hip/hip_runtime.h> and snake_internal.h.
#pragma once

namespace snake {

// Every launch runs with the caller stream's device current: the side stream and
// events are created on it, and a SnakeVecEnv on cuda:1 works whatever device the
// calling thread has current (restored on return).
struct DeviceGuard {
    int dev = -1, prev = -1;
    explicit DeviceGuard(hipStream_t s)
    {
        if (hipGetDevice(&prev) != hipSuccess) { set_error("hipGetDevice failed"); return; }
        if (s == nullptr) { dev = prev; return; }
        if (hipStreamGetDevice(s, &dev) != hipSuccess) {
            set_error("hipStreamGetDevice failed");
            dev = -1;
            return;
        }
        if (dev != prev && hipSetDevice(dev) != hipSuccess) {
            set_error("hipSetDevice(%d) failed", dev);
            dev = -1;
        }
    }
    ~DeviceGuard()
    {
        if (prev >= 0 && dev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
};

// 0x80 in every byte of x that equals 1 (exact per byte: no carry crosses a byte);
// the channel == 1 tests of policy_kernels.hip and greedy_kernels.hip
__device__ __forceinline__ uint32_t bytes_eq1(uint32_t x)
{
    const uint32_t y = x ^ 0x01010101u;
    const uint32_t t = (y & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return ~(t | y | 0x7f7f7f7fu);
}

}  // namespace snake

// snake_device.h -- DeviceGuard, shared by the launchers of snake_kernels.hip
// (snake_launch.inc) and of the policy, greedy, genome and replay kernels, and
// the launch status the last four report. Include after <hip/hip_runtime.h> and
// snake_internal.h.
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

// After a kernel launch: SNAKE_OK, or SNAKE_E_LAUNCH with "<kernel> launch failed: ..."
inline int launch_status(const char *kernel)
{
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return SNAKE_OK;
    set_error("%s launch failed: %s", kernel, hipGetErrorString(err));
    return SNAKE_E_LAUNCH;
}

}  // namespace snake

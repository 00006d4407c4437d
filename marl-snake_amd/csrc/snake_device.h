// snake_device.h -- the library's one device rule and its one launch status,
// shared by every launcher: snake_kernels.hip (snake_launch.inc), the policy,
// greedy, graph, genome, replay and pyrandom kernels and the DQN family.
// Include after <hip/hip_runtime.h> and snake_internal.h.
#pragma once

namespace snake {

// Every launch runs with the caller stream's device current (a null stream: the
// device that is current already): the side stream and events are created on
// it, what a launcher caches per device is keyed by `dev`, and an object on
// cuda:1 works whatever device the calling thread has current (restored on
// return). dev < 0, and the error set, where the runtime refuses.
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

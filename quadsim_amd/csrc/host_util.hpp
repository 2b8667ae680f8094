// host_util.hpp -- host-only helpers of the C ABI: the last-error text (fail), HIP_TRY, roctx ranges, the device guard
// A fragment of quadsim_hip.hip (ONE translation unit), included there right after include/quadsim.h, nowhere else.
#pragma once

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return fail(QS_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// roctx ranges around the hot entry points (trace readability under rocprofv3 --marker-trace): resolved at run time and
// only when QS_ROCTX=1, so the library carries no link-time dependency on a profiler library
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    bool on = false;
};
inline Roctx &roctx()
{
    static Roctx r = [] {
        Roctx x;
        const char *en = getenv("QS_ROCTX");
        if (en && atoi(en)) {
            void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
            if (h) {
                x.push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
                x.pop = (int (*)())dlsym(h, "roctxRangePop");
                x.on = x.push && x.pop;
            }
        }
        return x;
    }();
    return r;
}
struct Range {
    bool on;
    explicit Range(const char *name) : on(roctx().on) { if (on) roctx().push(name); }
    ~Range() { if (on) roctx().pop(); }
};

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace

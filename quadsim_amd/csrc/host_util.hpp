// host_util.hpp -- host-only helpers of the C ABI: the last-error text (fail), HIP_TRY, roctx ranges, the device guard, and
// the one path of user buffers to the kernels (HostStage, UserIO)
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

// Staging of a QS_IO_HOST handle (the single-env gym shims, the layer-1 context, C callers): a device buffer plus a pinned,
// device-mapped host mirror of the same size.  Both stay null on a QS_IO_DEVICE handle.
struct HostStage {
    char *dev = nullptr, *pin = nullptr, *pin_dev = nullptr;    // pin_dev: the mirror's device address
    size_t bytes = 0;
};

// The user buffers of ONE call of an entry point.  The entry point puts the caller's pointers where the kernel will read them
// (its StepArgs, its locals), declares each with in / out / inout and its element count, and brackets the launches with push()
// and pull().  Device handle: nothing happens, the kernel works on the caller's memory.  Host handle: push() lays the declared
// buffers out in the staging buffer as 256-B aligned slices -- in | inout | out, whatever the order of declaration -- grows the
// buffer if it must, copies the in / inout slices into the mirror and REPLACES each declared pointer by the address of its slice;
// pull() waits for the stream and copies the inout / out slices back to the caller.  A null pointer stays null and takes no room.
// Up to kDirectBytes the kernels read and write the mapped mirror in place (a step of a few envs costs one launch and one
// stream sync, no copy engine); larger calls take ONE DMA in ([0, inout_end)) and ONE DMA out ([in_end, end)) of the device
// buffer.  Above kMirrorBytes the mirror's extra pass over host memory costs more than it saves, and each slice is copied
// straight between the caller's memory and the device buffer (profiles/host_io/README.md has the measurement).
// `inout` is for outputs the kernel writes only some rows of: the others keep the caller's values.
#ifndef QS_MIRROR_BYTES          // A/B builds for tools/host_io_rate.py --sweep: 65536 never takes the mirror's DMA, 1 << 40 always
#define QS_MIRROR_BYTES (1u << 20)
#endif
constexpr size_t kDirectBytes = 64u << 10, kMirrorBytes = QS_MIRROR_BYTES;
struct UserIO {
    enum Dir { kIn = 0, kInOut = 1, kOut = 2 };
    struct Slice { void **slot; void *user; size_t bytes, off; Dir dir; };
    HostStage *hs;              // null: device handle
    hipStream_t stream;
    Slice sl[8];
    int count = 0;
    bool too_many = false;
    size_t edge[4] = {0, 0, 0, 0};      // slices of direction d occupy [edge[d], edge[d + 1])
    enum { kInPlace, kMirror, kCopy } via = kInPlace;
    UserIO(HostStage *host_stage, hipStream_t s) : hs(host_stage), stream(s) {}

    template <class T> void in(T *&p, size_t n) { add((void **)&p, n * sizeof(T), kIn); }
    template <class T> void inout(T *&p, size_t n) { add((void **)&p, n * sizeof(T), kInOut); }
    template <class T> void out(T *&p, size_t n) { add((void **)&p, n * sizeof(T), kOut); }
    void add(void **slot, size_t bytes, Dir dir)
    {
        if (!hs || !*slot) return;
        if (count == 8) { too_many = true; return; }       // push() refuses the call
        sl[count++] = Slice{slot, *slot, bytes, 0, dir};
    }
    int push()
    {
        if (!hs) return QS_OK;
        if (too_many) return fail(QS_ERR_INVALID, "UserIO: more than 8 buffers in one call");
        size_t off = 0;
        for (int d = kIn; d <= kOut; ++d) {
            edge[d] = off;
            for (Slice *s = sl; s < sl + count; ++s)
                if (s->dir == d) { s->off = off; off += (s->bytes + 255) & ~size_t(255); }
        }
        edge[3] = off;
        if (hs->bytes < off) {
            const size_t want = (off + off / 4 + 4095) & ~size_t(4095);     // headroom: a caller whose n grows does not reallocate at every call
            HIP_TRY(hipStreamSynchronize(stream));
            if (hs->dev) HIP_TRY(hipFree(hs->dev));
            if (hs->pin) HIP_TRY(hipHostFree(hs->pin));
            *hs = HostStage{};
            HIP_TRY(hipMalloc((void **)&hs->dev, want));
            HIP_TRY(hipHostMalloc((void **)&hs->pin, want, hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer((void **)&hs->pin_dev, hs->pin, 0));
            hs->bytes = want;
        }
        via = off <= kDirectBytes ? kInPlace : off <= kMirrorBytes ? kMirror : kCopy;
        for (Slice *s = sl; s < sl + count; ++s) {
            if (s->dir != kOut && via == kCopy) HIP_TRY(hipMemcpyAsync(hs->dev + s->off, s->user, s->bytes, hipMemcpyHostToDevice, stream));
            else if (s->dir != kOut) memcpy(hs->pin + s->off, s->user, s->bytes);
            *s->slot = (via == kInPlace ? hs->pin_dev : hs->dev) + s->off;
        }
        if (via == kMirror && edge[kOut]) HIP_TRY(hipMemcpyAsync(hs->dev, hs->pin, edge[kOut], hipMemcpyHostToDevice, stream));
        return QS_OK;
    }
    int pull()
    {
        if (!hs) return QS_OK;
        if (via == kMirror && edge[3] > edge[kInOut])
            HIP_TRY(hipMemcpyAsync(hs->pin + edge[kInOut], hs->dev + edge[kInOut], edge[3] - edge[kInOut], hipMemcpyDeviceToHost, stream));
        for (Slice *s = sl; s < sl + count && via == kCopy; ++s)
            if (s->dir != kIn) HIP_TRY(hipMemcpyAsync(s->user, hs->dev + s->off, s->bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (Slice *s = sl; s < sl + count && via != kCopy; ++s)
            if (s->dir != kIn) memcpy(s->user, hs->pin + s->off, s->bytes);
        return QS_OK;
    }
};

}  // namespace

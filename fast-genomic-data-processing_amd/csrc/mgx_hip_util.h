// mgx_hip_util.h -- what the HIP translation units share, each piece once: the HIP error check (HIP_TRY), a context's device
// pick and streams, the owner of a context's or a batch's buffers, events and streams, the arrays that grow on demand, the
// error message kept across a destroy and, for the I/O units, the guarded 16-byte load and the workgroup scan.  Internal to
// libmgx.so, HIP only.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "mgx_common.h"

extern "C" const char* mgx_last_error(void);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) { mgx::set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -EIO; } \
    } while (0)

#pragma GCC visibility push(hidden)
namespace mgx_hip {

// A context's device: `device` as the caller gave it -> an ordinal below n_dev in *out.  -1 takes the next of `next` (round-robin),
// or device 0 without a counter; negative_is_zero: every negative ordinal means 0 (the BGZF calls).  No HIP call.
inline int resolve_device(int device, int n_dev, std::atomic<unsigned>* next, bool negative_is_zero, int* out) {
    if (n_dev <= 0) { mgx::set_error("no HIP device is visible (this library has no CPU fallback)"); return -ENODEV; }
    if (device == -1 && next) device = (int)(next->fetch_add(1) % (unsigned)n_dev);
    else if (device == -1 || (device < 0 && negative_is_zero)) device = 0;
    if (device < 0 || device >= n_dev) { mgx::set_error("device %d out of range (0..%d)", device, n_dev - 1); return -EINVAL; }
    *out = device;
    return 0;
}
// ... and that device made current
inline int pick_device(int* device, std::atomic<unsigned>* next, bool negative_is_zero = false) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess) { (void)hipGetLastError(); n_dev = 0; }
    if (const int rc = resolve_device(*device, n_dev, next, negative_is_zero, device)) return rc;
    HIP_TRY(hipSetDevice(*device));
    return 0;
}

// A non-blocking stream.  cu_pattern, unless 0 or 0xFF, is an optional CU partition (a context's flags bits 8..15: an 8-bit
// pattern repeated over the n_cu CU indices): lets a VALU-bound PairHMM context and an HBM-bound sort context share one GPU
// side by side instead of queueing behind each other (BASELINE.json configs[4]).  high_priority holds for a stream
// without a mask only.
inline hipError_t make_stream(hipStream_t* s, int n_cu = 0, unsigned cu_pattern = 0, bool high_priority = false) {
    if (cu_pattern != 0 && cu_pattern != 0xFFu) {
        std::vector<uint32_t> mask((n_cu + 31) / 32, 0);
        for (int cu = 0; cu < n_cu; ++cu) if ((cu_pattern >> (cu & 7)) & 1u) mask[cu >> 5] |= 1u << (cu & 31);
        return hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data());
    }
    if (!high_priority) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    int least = 0, greatest = 0;
    if (const hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest)) return e;
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
}

// The device buffers, pinned buffers, events and streams of a batch or a context: what it allocated it frees, in one place,
// the streams last.  The first failure sticks (`err`, and the call's name in `failed`): the calls after it do nothing and
// return false like it, so a create checks once at its end.
struct Owner {
    std::vector<void*> dev, pinned;
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;
    hipError_t err = hipSuccess;
    const char* failed = nullptr;

    bool ok() const { return err == hipSuccess; }
    template <typename T> bool device(T** p, size_t bytes) { if (ok() && note(hipMalloc((void**)p, bytes), "hipMalloc")) dev.push_back(*p); return ok(); }
    template <typename T> bool pin(T** p, size_t bytes) { if (ok() && note(hipHostMalloc((void**)p, bytes, hipHostMallocDefault), "hipHostMalloc")) pinned.push_back(*p); return ok(); }
    bool event(hipEvent_t* e, unsigned flags = hipEventDefault) { if (ok() && note(hipEventCreateWithFlags(e, flags), "hipEventCreate")) events.push_back(*e); return ok(); }
    bool stream(hipStream_t* s, int n_cu = 0, unsigned cu_pattern = 0, bool high_priority = false) {
        if (ok() && note(make_stream(s, n_cu, cu_pattern, high_priority), "hipStreamCreate")) streams.push_back(*s);
        return ok();
    }
    // the result of any other call of a create (made only while ok()), so that it shares the one check
    bool note(hipError_t e, const char* what) {
        if (e != hipSuccess && ok()) { err = e; failed = what; (void)hipGetLastError(); }
        return e == hipSuccess;
    }
    void release() {
        for (void* p : pinned) (void)hipHostFree(p);
        for (void* p : dev) (void)hipFree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
        pinned.clear(); dev.clear(); events.clear(); streams.clear();
    }
    // what a create returns once !ok(), with the message: the first failure, for `what`
    int error(const char* what) const { mgx::set_error("%s failed for %s: %s", failed, what, hipGetErrorString(err)); return -EIO; }
    void reset() { release(); err = hipSuccess; failed = nullptr; }      // for an owner that is refilled
    Owner() = default;
    Owner(const Owner&) = delete; Owner& operator=(const Owner&) = delete;
    ~Owner() { release(); }
};

// A device array of T that grows on demand; growing discards the contents.  `want` >= n is the element count a growth asks
// for (each user keeps its growth rule).
template <typename T>
struct DevArray {
    T* p = nullptr; size_t cap = 0;
    int reserve(size_t n, size_t want) {
        if (n <= cap) return 0;
        release();
        if (hipMalloc((void**)&p, want * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); p = nullptr; mgx::set_error("hipMalloc of %zu bytes failed", want * sizeof(T)); return -ENOMEM; }
        cap = want;
        return 0;
    }
    int reserve(size_t n) { return reserve(n, n); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    void swap(DevArray& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    DevArray() = default;
    DevArray(DevArray&& o) noexcept { swap(o); }
    DevArray& operator=(DevArray&& o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~DevArray() { release(); }
};
// ... and its like in pinned host memory, in bytes
struct PinBuf {
    char* p = nullptr; size_t cap = 0;
    int reserve(size_t n, size_t want) {
        if (n <= cap) return 0;
        release();
        if (hipHostMalloc((void**)&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; mgx::set_error("hipHostMalloc of %zu bytes failed", want); return -ENOMEM; }
        cap = want;
        return 0;
    }
    int reserve(size_t n) { return reserve(n, n); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    void swap(PinBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept { swap(o); }
    PinBuf& operator=(PinBuf&& o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~PinBuf() { release(); }
};

// a device buffer with a pinned mirror, grown on demand: by a quarter and 256 bytes over n unless the caller says what it wants
struct Mirror {
    uint8_t* dev = nullptr; uint8_t* pin = nullptr; size_t cap = 0;
    int reserve(size_t n, size_t want) {
        if (n <= cap) return 0;
        release();
        if (hipMalloc((void**)&dev, want) != hipSuccess || hipHostMalloc((void**)&pin, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); release(); mgx::set_error("allocation of %zu bytes failed", want); return -ENOMEM;
        }
        cap = want;
        return 0;
    }
    int reserve(size_t n) { return reserve(n, n + n / 4 + 256); }
    void release() { if (dev) (void)hipFree(dev); if (pin) (void)hipHostFree(pin); dev = pin = nullptr; cap = 0; }
    void swap(Mirror& o) { std::swap(dev, o.dev); std::swap(pin, o.pin); std::swap(cap, o.cap); }
    Mirror() = default;
    Mirror(Mirror&& o) noexcept { swap(o); }
    Mirror& operator=(Mirror&& o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~Mirror() { release(); }
};

// rc, with the message that came with it kept across a destroy (which may set another)
template <typename Destroy> int keep_error(int rc, Destroy destroy) {
    const std::string msg = rc ? mgx_last_error() : "";
    destroy();
    if (rc) mgx::set_error("%s", msg.c_str());
    return rc;
}

// 16 bytes at base + g (g a multiple of 16, base 16-byte aligned), zeros from offset n on: no read at or past n
__device__ __forceinline__ uint4 load16_below(const uint8_t* base, uint64_t g, uint64_t n) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (g + 16 <= n) v = *(const uint4*)(base + g);
    else if (g < n) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) if (g + k < n) w[k / 4] |= (uint32_t)base[g + k] << (8 * (k % 4));
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}

// Exclusive scan of one value per thread over a workgroup of kScanBlock threads (Hillis-Steele in sh[kScanBlock]).
// Afterwards sh[] holds the inclusive sums, sh[kScanBlock - 1] the total; the caller puts a barrier in front of its
// next write to sh.
constexpr uint32_t kScanBlock = 256;
template <typename T>
__device__ __forceinline__ T block_scan_exclusive(T v, T* sh) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kScanBlock; d <<= 1) { const T o = tid >= d ? sh[tid - d] : 0; __syncthreads(); sh[tid] += o; __syncthreads(); }
    return sh[tid] - v;
}

}  // namespace mgx_hip
#pragma GCC visibility pop

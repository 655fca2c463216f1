// mgx_hip_util.h -- what the HIP translation units share, each piece once: the HIP error check (HIP_TRY: all of them) and, for
// the I/O units (mgx_bgzf.hip, mgx_store.hip, mgx_bgzf_inflate.hip, mgx_bam.hip, mgx_sam.hip), the owner of a batch's buffers
// and events, the guarded 16-byte load, the workgroup scan and the error message kept across a destroy.  Internal to
// libmgx.so, HIP only.
#pragma once
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <string>
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

// The device buffers, pinned buffers and events of a batch: what it allocated it frees, in one place.  The first failure
// sticks (`err`, and the call's name in `failed`): the calls after it do nothing and return false like it, so a create
// checks once at its end.
struct Owner {
    std::vector<void*> dev, pinned;
    std::vector<hipEvent_t> events;
    hipError_t err = hipSuccess;
    const char* failed = nullptr;

    bool ok() const { return err == hipSuccess; }
    template <typename T> bool device(T** p, size_t bytes) { if (ok() && note(hipMalloc((void**)p, bytes), "hipMalloc")) dev.push_back(*p); return ok(); }
    template <typename T> bool pin(T** p, size_t bytes) { if (ok() && note(hipHostMalloc((void**)p, bytes, hipHostMallocDefault), "hipHostMalloc")) pinned.push_back(*p); return ok(); }
    bool event(hipEvent_t* e, unsigned flags = hipEventDefault) { if (ok() && note(hipEventCreateWithFlags(e, flags), "hipEventCreate")) events.push_back(*e); return ok(); }
    // the result of any other call of a create (made only while ok()), so that it shares the one check
    bool note(hipError_t e, const char* what) {
        if (e != hipSuccess && ok()) { err = e; failed = what; (void)hipGetLastError(); }
        return e == hipSuccess;
    }
    void release() {
        for (void* p : pinned) (void)hipHostFree(p);
        for (void* p : dev) (void)hipFree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        pinned.clear(); dev.clear(); events.clear();
    }
    Owner() = default;
    Owner(const Owner&) = delete; Owner& operator=(const Owner&) = delete;
    ~Owner() { release(); }
};

// a device buffer with a pinned mirror, grown on demand
struct Mirror {
    uint8_t* dev = nullptr; uint8_t* pin = nullptr; size_t cap = 0;
    int reserve(size_t n) {
        if (n <= cap) return 0;
        release();
        const size_t want = n + n / 4 + 256;
        if (hipMalloc((void**)&dev, want) != hipSuccess || hipHostMalloc((void**)&pin, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); release(); mgx::set_error("allocation of %zu bytes failed", want); return -ENOMEM;
        }
        cap = want;
        return 0;
    }
    void release() { if (dev) (void)hipFree(dev); if (pin) (void)hipHostFree(pin); dev = pin = nullptr; cap = 0; }
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

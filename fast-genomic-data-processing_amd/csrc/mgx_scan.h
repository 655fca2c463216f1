// mgx_scan.h -- the device-wide exclusive scan of the I/O code (SAM text input: tile counts and record sizes; the record
// store: the records' places in the stream): out[i] = f(0) + ... + f(i - 1) for i in [0, n], n = min(*n_dev, n_max)
// (n_dev may be NULL), so out[n] is the total.  Three launches, 256 threads x 16 values per workgroup; the middle one
// is a single workgroup over the workgroups' sums (256 per round).  No kernel waits for another workgroup.
#pragma once
#include "mgx_hip_util.h"

namespace mgx_hip {
namespace {                                // kernels: every translation unit that scans has them in its own code object

constexpr uint32_t kScanPer = 16, kScanChunk = kScanBlock * kScanPer;       // values per thread / per workgroup

template <typename T> struct ScanArray { const T* v; __device__ uint64_t operator()(uint64_t i) const { return v[i]; } };      // f(i) = v[i]

__device__ uint64_t scan_count(const uint64_t* n_dev, uint64_t n_max) { return n_dev ? min(*n_dev, n_max) : n_max; }

__device__ uint64_t block_sum(uint64_t v, uint64_t* sh) {            // sh: kScanBlock words; returns the sum to every thread
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t d = kScanBlock / 2; d >= 1; d >>= 1) { if (tid < d) sh[tid] += sh[tid + d]; __syncthreads(); }
    const uint64_t r = sh[0];
    __syncthreads();
    return r;
}

template <typename F>
__global__ __launch_bounds__(kScanBlock) void k_scan_sums(F f, const uint64_t* n_dev, uint64_t n_max, uint64_t* part) {
    __shared__ uint64_t sh[kScanBlock];
    const uint64_t n = scan_count(n_dev, n_max);
    const uint64_t lo = (uint64_t)blockIdx.x * kScanChunk;
    if (lo >= n && blockIdx.x) return;                         // uniform
    uint64_t s = 0;
    for (uint32_t k = 0; k < kScanPer; ++k) { const uint64_t i = lo + (uint64_t)threadIdx.x * kScanPer + k; if (i < n) s += f(i); }
    const uint64_t r = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(kScanBlock) void k_scan_parts(const uint64_t* n_dev, uint64_t n_max, uint64_t* part) {      // one workgroup, in place, exclusive
    __shared__ uint64_t sh[kScanBlock];
    __shared__ uint64_t carry;
    const uint64_t n = scan_count(n_dev, n_max);
    const uint64_t n_parts = (n + kScanChunk - 1) / kScanChunk;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint64_t p0 = 0; p0 < n_parts; p0 += kScanBlock) {
        const uint64_t i = p0 + tid;
        const uint64_t before = block_scan_exclusive(i < n_parts ? part[i] : 0, sh);
        if (i < n_parts) part[i] = carry + before;
        __syncthreads();
        if (tid == 0) carry += sh[kScanBlock - 1];
        __syncthreads();
    }
}

template <typename F>
__global__ __launch_bounds__(kScanBlock) void k_scan_write(F f, const uint64_t* n_dev, uint64_t n_max, const uint64_t* part, uint64_t* out) {
    __shared__ uint64_t sh[kScanBlock];
    const uint64_t n = scan_count(n_dev, n_max);
    const uint64_t lo = (uint64_t)blockIdx.x * kScanChunk;
    if (n == 0) { if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0; return; }
    if (lo >= n) return;                                       // uniform
    const uint32_t tid = threadIdx.x;
    uint64_t x[kScanPer], s = 0;
    for (uint32_t k = 0; k < kScanPer; ++k) { const uint64_t i = lo + (uint64_t)tid * kScanPer + k; x[k] = i < n ? f(i) : 0; s += x[k]; }
    const uint64_t before = block_scan_exclusive(s, sh);
    uint64_t run = part[blockIdx.x] + before;
    for (uint32_t k = 0; k < kScanPer; ++k) {
        const uint64_t i = lo + (uint64_t)tid * kScanPer + k;
        if (i < n) { out[i] = run; run += x[k]; if (i + 1 == n) out[n] = run; }
    }
}

// part: n_max / kScanChunk + 2 words of device memory; out: n_max + 1.  The caller checks hipGetLastError behind its launches.
template <typename F>
void scan_exclusive(hipStream_t s, F f, const uint64_t* n_dev, uint64_t n_max, uint64_t* part, uint64_t* out) {
    const dim3 grid((uint32_t)(n_max / kScanChunk + 1)), block(kScanBlock);
    hipLaunchKernelGGL(k_scan_sums<F>, grid, block, 0, s, f, n_dev, n_max, part);
    hipLaunchKernelGGL(k_scan_parts, dim3(1), block, 0, s, n_dev, n_max, part);
    hipLaunchKernelGGL(k_scan_write<F>, grid, block, 0, s, f, n_dev, n_max, (const uint64_t*)part, out);
}

}  // namespace
}  // namespace mgx_hip

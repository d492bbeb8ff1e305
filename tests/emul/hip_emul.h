// hip_emul.h -- TEST INFRASTRUCTURE ONLY.
// Minimal stand-in for <hip/hip_runtime.h> that lets surtr_amd/csrc/*.hip be
// compiled by g++ as a single-lane, single-thread-per-workgroup emulation
// (SURTR_EMUL: wave = 1 lane, workgroup = 1 thread, blocks run one after the
// other).  It exists so the CPU test tier can exercise the *kernel logic* of
// the product against the oracle without a GPU; it cannot show races and is
// never loaded by surtr_amd (engine.py only opens libsurtr_hip.so).
#pragma once
// geometry and capacities of the emulation: one lane per wave, one thread per workgroup; small thresholds so that small test
// meshes still go through the culling, the separate pre-pass kernel and the global-scratch fallback of the one-wave kernels
#define SURTR_LANES 1
#define SURTR_LSH 0
#define SURTR_WG 1
#define SURTR_SB 1u
#ifndef SURTR_KEEPALL_V
#define SURTR_KEEPALL_V 12u
#endif
#define SURTR_PREP_MINV 48u
// one vertex per "64-block" and per sphere group here: the LDS tables of k_prep_pairs (static arrays in this build) are sized so
// that the test meshes take the same paths as 50 000-vertex pieces do on the device
#define SURTR_PREP_NB 65536u
#define SURTR_MAIN_THREADS 1u      // (one thread per workgroup in this build)
#define SURTR_PS_NB 57344u
#define SURTR_SMALL_LV 64
#define SURTR_SMALL_LH 512
#include <cstdio>
#define SURTR_DBG(...) fprintf(stderr, __VA_ARGS__)
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)

struct uint2 { uint32_t x, y; };
struct float4 { float x, y, z, w; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { uint2 r; r.x = x; r.y = y; return r; }
static inline float4 make_float4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
struct dim3 { uint32_t x, y, z; dim3(uint32_t a = 1, uint32_t b = 1, uint32_t c = 1) : x(a), y(b), z(c) {} };

struct EmulIdx { uint32_t x = 0, y = 0, z = 0; };
static EmulIdx threadIdx, blockIdx, blockDim, gridDim;

static inline void __syncthreads() {}
template <class T> static inline T __shfl_up(T v, int, int) { return v; }
template <class T> static inline T __shfl_down(T v, int, int) { return v; }
template <class T> static inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }
template <class T> static inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
template <class T> static inline T atomicMin(T* p, T v) { T o = *p; if (v < o) *p = v; return o; }
template <class T> static inline T atomicCAS(T* p, T cmp, T v) { T o = *p; if (o == cmp) *p = v; return o; }

// one lane per wave: the cross-lane primitives degenerate to the identity
static inline unsigned long long __ballot(bool p) { return p ? 1ull : 0ull; }
static inline int __syncthreads_or(int p) { return p; }
static inline bool __all(bool p) { return p; }
template <class T> static inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
template <class T> static inline T atomicExch(T* p, T v) { T o = *p; *p = v; return o; }
static inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
static inline void __builtin_amdgcn_s_sleep(int) {}
static inline void __threadfence() {}
static inline void __threadfence_block() {}
static inline int __builtin_amdgcn_readlane(int v, int) { return v; }
static inline int __builtin_amdgcn_update_dpp(int old, int, int, int, int, bool) { return old; }      // lane 0 never has a source lane
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

typedef int hipError_t;
typedef void* hipStream_t;
typedef void* hipEvent_t;
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2 };
enum { hipSuccess = 0 };
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
struct hipDeviceProp_t { int multiProcessorCount; };
static inline const char* hipGetErrorString(hipError_t) { return "emulated"; }
static inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
static inline hipError_t hipSetDevice(int) { return hipSuccess; }
static inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) { p->multiProcessorCount = 1; return hipSuccess; }
static inline hipError_t hipMemGetInfo(size_t* f, size_t* t) { *f = (size_t)8 << 30; *t = (size_t)16 << 30; return hipSuccess; }
// Allocation bookkeeping shared by every translation unit of the library (tests/test_alloc_failures.py reaches it through ctypes):
// the number of live allocations, the hipMalloc calls since the last surtr_emul_fail_alloc, and the one of them (0-based; -1: none)
// that fails.
//
// RED ZONES (tests/test_capacity_limits.py).  Every device block lies between two zones of EMUL_ZONE bytes filled with
// EMUL_ZONE_BYTE: the front zone ends at the payload's first byte, the back zone begins at the byte after its last one (the
// size is not rounded up, so a write one element past the end lands in the zone).  The payload is zeroed and starts on a
// 256-byte boundary, as hipMalloc's does (the image arena is read in 16-byte words).  hipFree checks both zones of the block it
// frees; surtr_emul_guard_check() checks those of every live block as well and returns the number of damaged blocks seen so far.
// The zones catch WRITES only, and only those that land within EMUL_ZONE bytes of a block: a read past the end returns the fill
// byte and goes unnoticed, and so does a write that jumps over the zone or lands elsewhere in the same block -- another workgroup's slice
// of a scratch pool, for one (see BLOCK ORDER below: no order puts the working slice next to a zone).
#define EMUL_ZONE 4096u
#define EMUL_ZONE_BYTE 0xA5
struct EmulBlock { EmulBlock *prev, *next; size_t n; uint64_t magic; bool counted; };      // at the start of the front zone's page
static_assert(sizeof(EmulBlock) <= 256, "the block header and EMUL_ZONE bytes of fill share the 256 + EMUL_ZONE bytes before the payload");
struct EmulAllocs { long live = 0, calls = 0, fail_at = -1, damaged = 0; EmulBlock* head = nullptr; int reverse = 0; };
inline EmulAllocs& emul_allocs() { static EmulAllocs a; return a; }
inline bool emul_block_damaged(const EmulBlock* b)
{
    const unsigned char* front = (const unsigned char*)b + 256, *back = front + EMUL_ZONE + b->n;
    for (size_t i = 0; i < EMUL_ZONE; ++i) if (front[i] != EMUL_ZONE_BYTE || back[i] != EMUL_ZONE_BYTE) return true;
    return false;
}
extern "C" __attribute__((used, visibility("default"))) inline long surtr_emul_live_allocs() { return emul_allocs().live; }
extern "C" __attribute__((used, visibility("default"))) inline long surtr_emul_alloc_calls() { return emul_allocs().calls; }
extern "C" __attribute__((used, visibility("default"))) inline void surtr_emul_fail_alloc(long k) { emul_allocs().calls = 0; emul_allocs().fail_at = k; }
extern "C" __attribute__((used, visibility("default"))) inline long surtr_emul_guard_check()
{
    EmulAllocs& a = emul_allocs();
    for (EmulBlock* b = a.head; b; b = b->next)
        if (!b->counted && emul_block_damaged(b))
        {
            b->counted = true; ++a.damaged;
            fprintf(stderr, "hip_emul: a red zone of the live device block %p (%zu bytes) is damaged\n", (void*)((char*)b + 256 + EMUL_ZONE), b->n);
        }
    return a.damaged;
}
// BLOCK ORDER.  surtr_emul_block_order(1) makes every launch run its blocks last to first.  Forward, block 0 takes every ticket
// of a queue; reversed, block grid - 1 does, on scratch slice (wg_base +) grid - 1, and whatever a kernel assumes about "block 0
// runs first" shows.  WHAT THIS DOES NOT GIVE: a scratch pool holds more slices than a launch has blocks (the Mesh clip's pool is
// max_wg + n_wg_big + 32 catcher slices, a grid is min(pairs, max_wg); pool_small and pool_half likewise), so the working slice is
// followed by another slice in either order, not by the pool's red zone.  A write past the end of a scratch SLICE -- or past one
// of its arrays, each rounded up to 256 bytes -- lands in memory that no zone covers: only a changed event (the bit comparisons)
// or a probe at the exact threshold (tests/test_capacity_limits.py, scratch_threshold_case) can show it.  One case there arranges
// for the working slice to BE the pool's last (scratch-torus40-last: 32 catcher blocks reversed, block 31 on the last slice, CH a
// multiple of 64): that one ends at the zone, for the slice's last array only.  The zones do cover every
// buffer that is one block: the arena's arrays, the tables, the blobs.  A kernel that waits for a
// lower-numbered block of its own launch would not end when reversed and would have to stay forward, by name, here.  Reading
// every loop of csrc/ for one found none: no kernel scans with a look-back, and the only loop that waits on another workgroup at
// all is the polling catcher of k_clip_pairs_catch, which waits for words that ANOTHER launch (k_clip_pairs_main) writes and
// leaves after a bounded number of polls when that kernel is not running beside it -- in either order.
extern "C" __attribute__((used, visibility("default"))) inline void surtr_emul_block_order(int reverse) { emul_allocs().reverse = reverse != 0; }
static inline hipError_t hipMalloc(void** p, size_t n)
{
    EmulAllocs& a = emul_allocs();
    if (a.calls++ == a.fail_at) { *p = nullptr; return 2; }      // (hipErrorOutOfMemory)
    *p = nullptr;
    if (n == 0) n = 1;
    const size_t total = (256 + EMUL_ZONE + n + EMUL_ZONE + 255) & ~(size_t)255;
    unsigned char* raw = (unsigned char*)aligned_alloc(256, total);
    if (!raw) return 1;
    EmulBlock* b = (EmulBlock*)raw;
    memset(raw, 0, 256);
    memset(raw + 256, EMUL_ZONE_BYTE, EMUL_ZONE);
    memset(raw + 256 + EMUL_ZONE, 0, n);
    memset(raw + 256 + EMUL_ZONE + n, EMUL_ZONE_BYTE, total - (256 + EMUL_ZONE + n));
    b->n = n; b->magic = 0x5355525452454D55ull; b->counted = false;
    b->prev = nullptr; b->next = a.head; if (a.head) a.head->prev = b; a.head = b;
    ++a.live;
    *p = raw + 256 + EMUL_ZONE;
    return hipSuccess;
}
static inline hipError_t hipFree(void* p)
{
    if (!p) return hipSuccess;
    EmulAllocs& a = emul_allocs();
    EmulBlock* b = (EmulBlock*)((unsigned char*)p - EMUL_ZONE - 256);
    if (b->magic != 0x5355525452454D55ull) { fprintf(stderr, "hip_emul: hipFree of %p, which is no live device block\n", p); abort(); }
    if (!b->counted && emul_block_damaged(b))
    {
        ++a.damaged;
        fprintf(stderr, "hip_emul: a red zone of the device block %p (%zu bytes) was damaged when it was freed\n", p, b->n);
    }
    if (b->prev) b->prev->next = b->next; else a.head = b->next;
    if (b->next) b->next->prev = b->prev;
    b->magic = 0;
    --a.live;
    free(b);
    return hipSuccess;
}
static inline hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { if (n) memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { if (n) memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
static inline hipError_t hipMemset(void* d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
// streams and events: everything runs in program order
static inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = nullptr; return hipSuccess; }
static inline hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
static inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = nullptr; return hipSuccess; }
static inline hipError_t hipEventCreate(hipEvent_t* e) { *e = nullptr; return hipSuccess; }
static inline hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
static inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }

// the two hipCUB device algorithms the host code calls (stable LSD radix sort of pairs by key bits; exclusive sum)
#include <algorithm>
#include <vector>
namespace hipcub {
struct DeviceRadixSort
{
    template <class K, class V>
    static hipError_t SortPairs(void* tmp, size_t& tmp_bytes, const K* kin, K* kout, const V* vin, V* vout, int n, int begin_bit, int end_bit, hipStream_t)
    {
        if (!tmp) { tmp_bytes = 16; return hipSuccess; }
        std::vector<int> ord(n);
        for (int i = 0; i < n; ++i) ord[i] = i;
        const K mask = end_bit >= (int)(8 * sizeof(K)) ? ~(K)0 : (((K)1 << end_bit) - 1);
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return ((kin[a] & mask) >> begin_bit) < ((kin[b] & mask) >> begin_bit); });
        for (int i = 0; i < n; ++i) { kout[i] = kin[ord[i]]; vout[i] = vin[ord[i]]; }
        return hipSuccess;
    }
};
struct DeviceScan
{
    template <class T>
    static hipError_t ExclusiveSum(void* tmp, size_t& tmp_bytes, const T* in, T* out, int n, hipStream_t)
    {
        if (!tmp) { tmp_bytes = 16; return hipSuccess; }
        T run = 0;
        for (int i = 0; i < n; ++i) { const T v = in[i]; out[i] = run; run += v; }
        return hipSuccess;
    }
};
} // namespace hipcub

#define hipLaunchKernelGGL(kern, grid, block, shmem, stream, ...)                         \
    do {                                                                                   \
        dim3 g_ = (grid), b_ = (block);                                                    \
        gridDim.x = g_.x; blockDim.x = b_.x;                                               \
        const bool rev_ = emul_allocs().reverse != 0;                                      \
        for (uint32_t bn_ = 0; bn_ < g_.x; ++bn_)                                          \
            for (uint32_t ti_ = 0; ti_ < b_.x; ++ti_) { blockIdx.x = rev_ ? g_.x - 1u - bn_ : bn_; threadIdx.x = ti_; kern(__VA_ARGS__); } \
    } while (0)
template <class T> static inline T __shfl(T v, int, int) { return v; }

// dpe_common.h -- internal helpers shared by the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/dpe_hip.h"
#include "dpe_consts.h"

namespace dpe {

void set_error(const char *fmt, ...);

#define DPE_CHECK_HIP(expr)                                                              \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            dpe::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,                 \
                           hipGetErrorString(e_));                                       \
            return -1;                                                                   \
        }                                                                                \
    } while (0)

#define DPE_REQUIRE(cond, ...)                                                           \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            dpe::set_error(__VA_ARGS__);                                                 \
            return -1;                                                                   \
        }                                                                                \
    } while (0)

void gen_ca_code_host(int prn, int8_t *chips);  // dpe_util.hip

#ifdef __HIPCC__   // device helpers: the host-only sources (dpe_chanmgr.hip, dpe_ekf.hip) also build with a plain C++ compiler
// 64-lane butterfly sum; every lane ends with the total.
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// 64-lane sums on the VALU (DPP, no LDS traffic): quad swaps, half-row and row mirrors, then the two
// row broadcasts; lane 63 ends up with the total.  N independent values are reduced step-major so
// that the VALU->DPP read hazard of one chain is covered by the other chains (no s_nop padding).
template <int N>
__device__ __forceinline__ void dpp_sum_lane63(float (&v)[N])
{
    static_assert(N >= 3, "the step-major interleave must cover the 2 wait states of a VALU->DPP hazard");
    // in-place v_add_f32 with a DPP source: one instruction per value per step; rows masked off by
    // row_mask keep their value.  (Written as asm: the compiler's own lowering of update_dpp costs
    // three instructions per step and pairs the adds into v_pk_add, which cannot take DPP.)
#define DPE_DPP_STEP(mod) \
    _Pragma("unroll") for (int i = 0; i < N; ++i) asm volatile("v_add_f32_dpp %0, %0, %0 " mod : "+v"(v[i]));
    DPE_DPP_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
    DPE_DPP_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
    DPE_DPP_STEP("row_half_mirror row_mask:0xf bank_mask:0xf")
    DPE_DPP_STEP("row_mirror row_mask:0xf bank_mask:0xf")
    DPE_DPP_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
    DPE_DPP_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
#undef DPE_DPP_STEP
}

// Sums within each DPP row (16 lanes): after the four row-local steps every lane of a row holds the row total.
template <int N>
__device__ __forceinline__ void dpp_sum_rows(float (&v)[N])
{
    static_assert(N >= 3, "the step-major interleave must cover the 2 wait states of a VALU->DPP hazard");
#define DPE_DPP_STEP(mod) \
    _Pragma("unroll") for (int i = 0; i < N; ++i) asm volatile("v_add_f32_dpp %0, %0, %0 " mod : "+v"(v[i]));
    DPE_DPP_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
    DPE_DPP_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
    DPE_DPP_STEP("row_half_mirror row_mask:0xf bank_mask:0xf")
    DPE_DPP_STEP("row_mirror row_mask:0xf bank_mask:0xf")
#undef DPE_DPP_STEP
}

// wave-uniform total of v (read back from lane 63)
__device__ __forceinline__ float lane63(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
#endif  // __HIPCC__

// Optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg).
struct KernelProfiler {
    bool enabled = false;
    unsigned mask = ~0u;   // slots that carry events while enabled (a pair of events costs ~1 % of a short step)
    static constexpr int kSlots = 8;
    std::vector<hipEvent_t> ev[kSlots];   // pairs: start, stop
    void begin(int slot, hipStream_t st)
    {
        if (!enabled || !((mask >> slot) & 1u)) return;
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        ev[slot].push_back(a);
        ev[slot].push_back(b);
        (void)hipEventRecord(a, st);
    }
    void end(int slot, hipStream_t st)
    {
        if (!enabled || !((mask >> slot) & 1u) || ev[slot].empty()) return;
        (void)hipEventRecord(ev[slot].back(), st);
    }
    // total milliseconds and launch count per slot since the last call; frees the events
    void collect(float *ms, int *count)
    {
        for (int s = 0; s < kSlots; ++s) {
            ms[s] = 0.f;
            count[s] = (int)ev[s].size() / 2;
            for (size_t i = 0; i + 1 < ev[s].size(); i += 2) {
                float t = 0.f;
                (void)hipEventSynchronize(ev[s][i + 1]);
                if (hipEventElapsedTime(&t, ev[s][i], ev[s][i + 1]) == hipSuccess) ms[s] += t;
                (void)hipEventDestroy(ev[s][i]);
                (void)hipEventDestroy(ev[s][i + 1]);
            }
            ev[s].clear();
        }
    }
};


// Replays a whole Update (parameter upload, memsets, kernels, result copies) as one hipGraph launch when
// the call repeats with the same shape and device pointers -- the closed-loop receiver calls Update
// once per 20 ms window with identical arguments apart from the pinned parameter block, so the ~8
// enqueue calls collapse into one.  Off by default; dpe_*_set_graph() turns it on.
// The captured sequences hold no memset nodes: on ROCm 7.2 / gfx950 a captured hipMemsetAsync gave wrong
// buffer contents from the second replay on (measured, round 1), so zeroing is done by kernels or avoided.
struct GraphCache {
    struct Key {
        const void *p0, *p1;
        long long a;
        int w, k, flags;
        hipStream_t st;
        bool operator==(const Key &o) const
        {
            return p0 == o.p0 && p1 == o.p1 && a == o.a && w == o.w && k == o.k && flags == o.flags && st == o.st;
        }
    };
    bool enabled = false;
    bool capturing = false;
    Key pending{};
    std::vector<std::pair<Key, hipGraphExec_t>> items;   // a handful: one per SampleBlock ring slot
    static constexpr size_t kMaxItems = 64;
    // 1: replayed, nothing left to enqueue; 0: caller enqueues (being captured when enabled); -1: error
    int begin(const Key &k, hipStream_t st)
    {
        if (!enabled || st == nullptr) return 0;   // the legacy default stream cannot be captured
        for (auto &it : items)
            if (it.first == k) return hipGraphLaunch(it.second, st) == hipSuccess ? 1 : -1;
        if (items.size() >= kMaxItems) clear();
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) return -1;
        capturing = true;
        pending = k;
        return 0;
    }
    // closes the capture opened by begin() and runs it once; no-op when nothing is being captured
    int end(hipStream_t st)
    {
        if (!capturing) return 0;
        capturing = false;
        hipGraph_t g = nullptr;
        if (hipStreamEndCapture(st, &g) != hipSuccess || !g) return -1;
        hipGraphExec_t e = nullptr;
        const hipError_t rc = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (rc != hipSuccess) return -1;
        items.emplace_back(pending, e);
        return hipGraphLaunch(e, st) == hipSuccess ? 0 : -1;
    }
    void clear()
    {
        for (auto &it : items) (void)hipGraphExecDestroy(it.second);
        items.clear();
    }
    // drops an unfinished capture when Update leaves early on an error
    struct Guard {
        GraphCache &g;
        hipStream_t st;
        ~Guard()
        {
            if (!g.capturing) return;
            g.capturing = false;
            hipGraph_t x = nullptr;
            (void)hipStreamEndCapture(st, &x);
            if (x) (void)hipGraphDestroy(x);
        }
    };
};

#ifdef __HIPCC__
// Small per-call parameter blocks (channel / SV coefficients of ONE window) travel in the kernel-argument
// segment instead of through an H2D copy: the block is the kernel's FIRST argument and is read through
// the kernarg segment pointer.  Both candidates are cast to the constant address space so that the
// wave-uniform reads stay scalar loads (s_load) whichever source is selected.
template <typename T>
__device__ __forceinline__ const T *params_ptr(const T *global_ptr, int useKernarg)
{
    typedef const T __attribute__((address_space(4))) *c_t;
    c_t k = (c_t)__builtin_amdgcn_kernarg_segment_ptr();
    c_t g = (c_t)(unsigned long long)global_ptr;
    return (const T *)(useKernarg ? k : g);
}
#endif

#ifdef __HIPCC__
// Batch parameter blocks (a few KB to a few hundred KB per Update) go to the device with a small KERNEL that reads the pinned
// staging block directly instead of a hipMemcpyAsync: an in-stream copy command costs ~5-8 us of stream time on this stack,
// a kernel boundary 1.5-2 us (measured: config H step 0.320 -> 0.31x ms, two such copies per step).
// (clearWord / clearMask: a status word whose per-launch bits the same kernel clears -- no memset command in the stream)
__global__ static void upload_params_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, int n16, int *__restrict__ clearWord, int clearMask)
{
    if (clearWord && blockIdx.x == 0 && threadIdx.x == 0) atomicAnd(clearWord, ~clearMask);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x) dst[i] = src[i];
}
static inline void upload_params(void *dst_dev, const void *src_pinned_devptr, size_t bytes, hipStream_t st, int *clearWord = nullptr, int clearMask = 0)
{
    const int n16 = (int)((bytes + 15) / 16);
    const int blocks = n16 / 256 + 1 > 64 ? 64 : n16 / 256 + 1;
    hipLaunchKernelGGL(upload_params_kernel, dim3(blocks), dim3(256), 0, st, (uint4 *)dst_dev, (const uint4 *)src_pinned_devptr, n16, clearWord, clearMask);
}
#endif

// n counters of a handle read back behind everything its last call enqueued on `st`; -1 with the error set
static inline int read_counters(unsigned long long *host, const unsigned long long *dev, size_t n, hipStream_t st)
{
    DPE_CHECK_HIP(hipMemcpyAsync(host, dev, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    DPE_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static inline T *dev_alloc(size_t n)
{
    void *p = nullptr;
    if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) return nullptr;
    return static_cast<T *>(p);
}

}  // namespace dpe

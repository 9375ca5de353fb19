// dpe_stream_plan.h -- what the sample-stream stages (front end, excisor, array combiner: dpe_fe_plan.h, dpe_ix_plan.h,
// dpe_arr_plan.h) hold in common, as plain C++.  A handle keeps nothing of the record; a call turns its outputs into a needed input
// range cut to the record [0, recordLength), checks it against what the buffer holds, writes int16 or fp32 I/Q and counts what it
// clipped.  The output of one stage is the record of the next, so the index limits, the record cut and the int16 word stand here
// once.  Nothing of HIP is included (DPE_STREAM_HD); host/test_fe_plan.cpp holds the quantiser to numpy.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/dpe_hip.h"

#if defined(__HIPCC__)
#define DPE_STREAM_HD __host__ __device__ inline
#else
#define DPE_STREAM_HD inline
#endif

// a refusal inside a function that returns true with the reason in `msg` (of `len` bytes)
#define DPE_STREAM_REFUSE(cond, ...)             \
    do {                                         \
        if (cond) {                              \
            snprintf(msg, len, __VA_ARGS__);     \
            return true;                         \
        }                                        \
    } while (0)

namespace dpe {

constexpr int64_t kStreamMaxCount = INT64_C(1) << 30;   // outputs per call
constexpr int64_t kStreamMaxIndex = INT64_C(1) << 55;   // every output index of a call lies below it: (index + count) D + T stays far inside 64 bits
constexpr int64_t kStreamMaxHeld = INT64_C(1) << 61;    // first sample and count of what a buffer holds
static_assert(kStreamMaxIndex + kStreamMaxCount <= kStreamMaxHeld, "an output index of one stage has to be a legal held index of the next");

// [lo, hi) cut to the record [0, recordLength) (recordLength < 0: no end); hi >= lo afterwards
inline void stream_cut(int64_t recordLength, int64_t &lo, int64_t &hi)
{
    if (lo < 0) lo = 0;
    if (recordLength >= 0 && hi > recordLength) hi = recordLength;
    if (hi < lo) hi = lo;
}
// multiples of step in [first, end), first >= 0
inline int64_t stream_multiples(int64_t first, int64_t end, int64_t step)
{
    return end <= first ? 0 : (end - 1) / step - (first + step - 1) / step + 1;
}

// ---- the int16 I/Q word: I in the low half, Q in the high half.  Rounds half to even, clips to the rails and adds the clipped
// components to `clipped`.
DPE_STREAM_HD int stream_quantise(float re, float im, unsigned &clipped)
{
    const float ri = rintf(re), rq = rintf(im);
    clipped += (ri < -32768.f || ri > 32767.f) + (rq < -32768.f || rq > 32767.f);
    const int qi = (int)fminf(fmaxf(ri, -32768.f), 32767.f), qq = (int)fminf(fmaxf(rq, -32768.f), 32767.f);
    return (qi & 0xFFFF) | (qq << 16);
}
template <typename T>   // int or float
DPE_STREAM_HD void stream_unpack(int w, T &i, T &q)
{
    i = (T)(short)(w & 0xFFFF);
    q = (T)(w >> 16);
}
#if defined(__HIPCC__)
// output `at` of a stream: the fp32 pair as it is, or its int16 word
__device__ __forceinline__ void stream_store(void *out, long long at, float re, float im, int outF32, unsigned &clipped)
{
    typedef float pair __attribute__((ext_vector_type(2)));
    if (outF32) reinterpret_cast<pair *>(out)[at] = pair{re, im};
    else reinterpret_cast<int *>(out)[at] = stream_quantise(re, im, clipped);
}
#endif

// ---- the refusals the stages share, each with the stage's tag ("[Excisor]") and the call's name ("process").  true: refused.
inline bool stream_format_problem(const char *tag, const char *call, int outputFormat, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(outputFormat != DPE_FE_OUT_I16 && outputFormat != DPE_FE_OUT_F32, "%s %s: output format %d is neither DPE_FE_OUT_I16 nor DPE_FE_OUT_F32",
                      tag, call, outputFormat);
    return false;
}
inline bool stream_gain_problem(const char *tag, const char *call, double gain, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(!std::isfinite(gain), "%s %s: gain not finite", tag, call);
    return false;
}
// what the buffer holds, [xFirst, xFirst + xCount), and the record
inline bool stream_held_problem(const char *tag, const char *call, int64_t xFirst, int64_t xCount, int64_t recordLength, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(xFirst < 0 || xCount < 0 || xFirst > kStreamMaxHeld || xCount > kStreamMaxHeld, "%s %s: input range %lld + %lld negative or beyond 2^61",
                      tag, call, (long long)xFirst, (long long)xCount);
    DPE_STREAM_REFUSE(recordLength < -1, "%s %s: record length %lld (-1: no end)", tag, call, (long long)recordLength);
    return false;
}
inline bool stream_outputs_problem(const char *tag, const char *call, int64_t outFirst, int64_t outCount, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(outCount < 1 || outCount > kStreamMaxCount, "%s %s: %lld outputs outside 1..2^30 per call", tag, call, (long long)outCount);
    DPE_STREAM_REFUSE(outFirst < 0 || outFirst > kStreamMaxIndex - outCount, "%s %s: first output %lld with %lld outputs outside 0..2^55", tag, call,
                      (long long)outFirst, (long long)outCount);
    return false;
}
// the `noun`s ("outputs", "frames", "blocks") [first, first + count) need [lo, hi); `holder`: "the buffer holds" / "the buffers hold"
inline bool stream_coverage_problem(const char *tag, const char *call, const char *noun, const char *holder, int64_t first, int64_t count, int64_t lo,
                                    int64_t hi, int64_t xFirst, int64_t xCount, char *msg, size_t len)
{
    DPE_STREAM_REFUSE(lo < hi && (lo < xFirst || hi > xFirst + xCount), "%s %s: %s %lld..%lld need the input samples %lld..%lld, %s %lld..%lld", tag, call, noun,
                      (long long)first, (long long)(first + count - 1), (long long)lo, (long long)(hi - 1), holder, (long long)xFirst,
                      (long long)(xFirst + xCount - 1));
    return false;
}

}  // namespace dpe

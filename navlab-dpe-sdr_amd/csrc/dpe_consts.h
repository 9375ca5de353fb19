// dpe_consts.h -- the reference's physical constants: plain C++, shared by the HIP translation units (through dpe_common.h) and
// by the host-only headers that a plain C++ compiler builds (dpe_bcs_plan.h).
#pragma once

// host and device under hipcc, plain functions for a host compiler: the one definition every shared-arithmetic header uses
#ifdef __HIPCC__
#define DPE_HD __host__ __device__
#else
#define DPE_HD
#endif

namespace dpe {

// cudarecv/utils/inc/consthelper.h:5-27 -- bit-for-bit
constexpr double kC = 299792458.0;
constexpr double kPi = 3.1415926535898;
constexpr double kFL1 = 1.57542e9;
constexpr double kFCA = 1.023e6;
constexpr double kTCA = 0.001;
constexpr double kOEDot = 7.2921151467e-5;
constexpr int kLCA = 1023;
constexpr int kPrnMax = 37;

}  // namespace dpe

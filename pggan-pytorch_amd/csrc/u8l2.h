// What the three exact uint8 squared-L2 units (csrc/nn_search.hip, csrc/prd.hip, csrc/shift_search.hip) all need: the int8-MFMA operand
// types, the XOR that turns four uint8 into four int8, the norm of 16 such bytes, the 16-byte load whose absent bytes are zero in the
// shifted domain, and the 1-D launch grid.  The head of csrc/nn_search.hip says why the shift is an XOR with 0x80808080 and why a
// piece at or past D must shift to zero; the units' own heads state their bounds.
#ifndef PGGAN_CSRC_U8L2_H
#define PGGAN_CSRC_U8L2_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace u8l2 {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr unsigned SHIFT = 0x80808080u;
constexpr long long I64_MAX = 0x7fffffffffffffffLL;

__device__ __forceinline__ v4i shifted(const uint4& v)
{
    v4i r;
    r.x = (int)(v.x ^ SHIFT); r.y = (int)(v.y ^ SHIFT); r.z = (int)(v.z ^ SHIFT); r.w = (int)(v.w ^ SHIFT);
    return r;
}

// acc + the sum of the squares of 16 shifted bytes
__device__ __forceinline__ int sumsq16(const v4i& v, int acc)
{
    acc = __builtin_amdgcn_sdot4(v.x, v.x, acc, false);
    acc = __builtin_amdgcn_sdot4(v.y, v.y, acc, false);
    acc = __builtin_amdgcn_sdot4(v.z, v.z, acc, false);
    return __builtin_amdgcn_sdot4(v.w, v.w, acc, false);
}

// 16 bytes at p when valid, else the bytes that shift to zero
__device__ __forceinline__ uint4 load16(const uint8_t* p, bool valid)
{
    uint4 v = make_uint4(SHIFT, SHIFT, SHIFT, SHIFT);
    if (valid) v = *reinterpret_cast<const uint4*>(p);
    return v;
}

inline int grid_for(long long total, int block = 256, int cap = 4096)
{
    long long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace u8l2

#endif

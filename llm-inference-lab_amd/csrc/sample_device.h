// Device building blocks shared by the samplers (csrc/sample.hip, csrc/spec_sample.hip): the Philox4x32-10 draw, the
// row walkers and the total order of Gumbel scores. Arithmetic as oracle/sampling_ref.py.
#pragma once

#include <hip/hip_fp16.h>

#include "common.h"

namespace sd {

constexpr int kSampleThreads = 1024;
constexpr int kIdxBits = 20;
constexpr uint32_t kTagCdf = 0x5EED0001u, kTagGumbel = 0x5EED0002u;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t& r0) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = static_cast<uint32_t>(p1);
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = static_cast<uint32_t>(p0);
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r0 = c0;
}

__device__ __forceinline__ float load_logit(const void* row, int dtype, int i) {
  if (dtype == SD_F32) return static_cast<const float*>(row)[i];
  if (dtype == SD_BF16) return bf16_bits_to_float(static_cast<const uint16_t*>(row)[i]);
  return __half2float(static_cast<const __half*>(row)[i]);
}

// larger key = larger value; NaN largest; -0 == +0
__device__ __forceinline__ uint32_t order_key(float x) {
  if (x != x) return 0xFFFFFFFFu;
  if (x == 0.f) x = 0.f;
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t composite_key(float x, int i) {
  return (static_cast<uint64_t>(order_key(x)) << kIdxBits) | static_cast<uint64_t>(((1u << kIdxBits) - 1u) - static_cast<uint32_t>(i));
}

// f(value, index) for every element of the row, 16-byte loads when the row allows it.
// The visiting order differs between the two forms; every use below is order-independent.
template <typename F>
__device__ __forceinline__ void for_each_logit(const void* row, int dtype, int V, int tid, F&& f) {
  const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  if (dtype == SD_F32 && aligned && (V & 3) == 0) {
    const float4* p = static_cast<const float4*>(row);
    for (int v = tid; v < (V >> 2); v += kSampleThreads) {
      const float4 q = p[v];
      f(q.x, 4 * v); f(q.y, 4 * v + 1); f(q.z, 4 * v + 2); f(q.w, 4 * v + 3);
    }
  } else if (dtype == SD_BF16 && aligned && (V & 7) == 0) {
    const uint4* p = static_cast<const uint4*>(row);
    for (int v = tid; v < (V >> 3); v += kSampleThreads) {
      const uint4 q = p[v];
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f(__uint_as_float(w[j] << 16), 8 * v + 2 * j);
        f(__uint_as_float(w[j] & 0xffff0000u), 8 * v + 2 * j + 1);
      }
    }
  } else {
    for (int i = tid; i < V; i += kSampleThreads) f(load_logit(row, dtype, i), i);
  }
}

__device__ __forceinline__ bool better_d(double v, int i, double bv, int bi) {
  const bool vn = (v != v), bn = (bv != bv);
  if (vn | bn) {
    if (vn & bn) return i < bi;
    return vn;
  }
  return (v > bv) | ((v == bv) & (i < bi));
}

}  // namespace sd

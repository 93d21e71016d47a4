// Device building blocks shared by the samplers (csrc/sample.hip, csrc/spec_sample.hip), one definition each: the row
// walkers, the composite key and its selection pieces (bitonic sort, radix select), the kept set of a temperature -> top-k
// -> top-p shaped row (row_survivors: the ONE definition of "tie at the cut"), the Philox4x32-10 draws (uniform, Gumbel
// noise) and the inversion of a uniform through weights. The workgroup reductions and the total order of scores
// (better_d) are in common.h. Arithmetic as oracle/sampling_ref.py.
#pragma once

#include <hip/hip_fp16.h>

#include "common.h"

namespace sd {

constexpr int kSampleThreads = 1024;
constexpr int kIdxBits = 20;
constexpr uint32_t kTagCdf = 0x5EED0001u, kTagGumbel = 0x5EED0002u;
constexpr uint32_t kTagAccept = 0x5EED0003u;   // acceptance uniform of shaped speculative sampling (csrc/spec_sample.hip)
constexpr int kSampleMaxK = 1024;     // top_k limit
constexpr int kSampleCap = 2048;      // bucket size at which the radix passes stop
constexpr int kSampleSort = 4096;     // >= kSampleMaxK + kSampleCap, power of two

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

__device__ __forceinline__ int key_index(uint64_t c) {
  constexpr uint32_t kIdxMask = (1u << kIdxBits) - 1u;
  return static_cast<int>(kIdxMask - static_cast<uint32_t>(c & kIdxMask));
}

// f(value, index) for every element of a bf16 row, each loaded word stored to dst as well when dst is not null: 16-byte accesses,
// vector v = tid + 1024 j, when both pointers are 16-byte aligned and V % 8 == 0, else element i = tid + 1024 j.
template <typename F>
__device__ __forceinline__ void copy_and_visit_bf16_row(const uint16_t* src, uint16_t* dst, int V, int tid, F&& f) {
  if ((((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) && (V & 7) == 0) {
    const uint4* p = reinterpret_cast<const uint4*>(src);
    uint4* o = reinterpret_cast<uint4*>(dst);
    for (int v = tid; v < (V >> 3); v += kSampleThreads) {
      const uint4 q = p[v];
      if (dst) o[v] = q;
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f(__uint_as_float(w[j] << 16), 8 * v + 2 * j);
        f(__uint_as_float(w[j] & 0xffff0000u), 8 * v + 2 * j + 1);
      }
    }
  } else {
    for (int i = tid; i < V; i += kSampleThreads) {
      const uint16_t w = src[i];
      if (dst) dst[i] = w;
      f(bf16_bits_to_float(w), i);
    }
  }
}

// f(value, index) for every element of the row, 16-byte loads when the row allows it.
// The visiting order differs between the two forms; every use below is order-independent.
template <typename F>
__device__ __forceinline__ void for_each_logit(const void* row, int dtype, int V, int tid, F&& f) {
  if (dtype == SD_BF16) return copy_and_visit_bf16_row(static_cast<const uint16_t*>(row), nullptr, V, tid, f);
  if (dtype == SD_F32 && (reinterpret_cast<uintptr_t>(row) & 15) == 0 && (V & 3) == 0) {
    const float4* p = static_cast<const float4*>(row);
    for (int v = tid; v < (V >> 2); v += kSampleThreads) {
      const float4 q = p[v];
      f(q.x, 4 * v); f(q.y, 4 * v + 1); f(q.z, 4 * v + 2); f(q.w, 4 * v + 3);
    }
  } else {
    for (int i = tid; i < V; i += kSampleThreads) f(load_logit(row, dtype, i), i);
  }
}

// The two selection pieces below are called by every thread of a 1024-thread workgroup (barriers inside) on LDS of the caller.
// Descending bitonic sort of keys[0, n), n a power of two.
__device__ __forceinline__ void sort_desc(uint64_t* keys, int n) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < n / 2; t += kSampleThreads) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const uint64_t x = keys[lo], y = keys[hi];
        if ((x < y) == desc) { keys[lo] = y; keys[hi] = x; }
      }
      __syncthreads();
    }
  }
}

struct RadixPick {   // what wave 0 hands the workgroup after a pass: the chosen digit, the keys above it, the keys in it
  uint32_t digit, above, bucket;
};

// Radix select of the k-th largest composite key of the row (k 1-based), most significant digits first, in up to 5 passes
// of 11/11/10/10/10 bits: a pass histograms the next digit of the keys that match the prefix decided so far (hist: 2048
// words) and wave 0 picks the digit that holds the k-th. The passes stop once that digit's bucket holds <= stop_bucket keys
// (0: never, all 52 bits are decided). Returns the decided high bits, right-aligned, and their number in `decided`: the
// k-th key itself when decided == 52, else every key whose top `decided` bits are >= the return value is a candidate.
__device__ __forceinline__ uint64_t radix_select(const void* row, int dtype, int V, int k, uint32_t stop_bucket, uint32_t* hist,
                                                 RadixPick& pick, int& decided) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int widths[5] = {11, 11, 10, 10, 10};
  uint64_t prefix = 0;       // decided high bits (right-aligned)
  int need = k;              // rank of the wanted element inside the current bucket (1-based from the top)
  decided = 0;
  for (int p = 0; p < 5; ++p) {
    const int w = widths[p];
    const int shift = 52 - decided - w;
    for (int i = tid; i < 2048; i += kSampleThreads) hist[i] = 0;
    __syncthreads();
    for_each_logit(row, dtype, V, tid, [&](float x, int i) {
      const uint64_t c = composite_key(x, i);
      if ((c >> (shift + w)) == prefix) atomicAdd(&hist[(c >> shift) & ((1u << w) - 1u)], 1u);
    });
    __syncthreads();
    if (wave == 0) {
      // lane l owns digits [32 l, 32 l + 32); scan from the top digit down
      const int nb = 1 << w;
      uint32_t local = 0;
      for (int j = 0; j < 32; ++j) {
        const int d = lane * 32 + j;
        if (d < nb) local += hist[d];
      }
      uint32_t incl = local;  // suffix sum over lanes >= this one
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_down(incl, off, 64);
        if (lane + off < 64) incl += o;
      }
      uint32_t above = incl - local;
      if (above < static_cast<uint32_t>(need) && incl >= static_cast<uint32_t>(need)) {
        for (int j = 31; j >= 0; --j) {
          const int d = lane * 32 + j;
          if (d >= nb) continue;
          const uint32_t h = hist[d];
          if (above + h >= static_cast<uint32_t>(need)) {
            pick = RadixPick{static_cast<uint32_t>(d), above, h};
            break;
          }
          above += h;
        }
      }
    }
    __syncthreads();
    prefix = (prefix << w) | pick.digit;
    decided += w;
    need -= static_cast<int>(pick.above);
    const uint32_t bucket = pick.bucket;
    __syncthreads();
    if (bucket <= stop_bucket) break;
  }
  return prefix;
}

// ---------------------------------------------------------------------------------------------------------------------
// The kept set of a row under temperature -> top-k -> top-p (oracle/sampling_ref.py: filtered_distribution), by one
// 1024-thread workgroup; the steps are described at the top of csrc/sample.hip. On return (after a barrier) the LDS block
// holds, in sorted order (value descending, index ascending):
//   sel[j] = token id, ev[j] = float64 weight exp(x_j / T - max), j < n_keep;  z = their sum, added sequentially.
// A row whose top value is not finite is the point mass on its first id: n_keep = 1, ev[0] = 1, z = 1.
// ---------------------------------------------------------------------------------------------------------------------
struct SurvivorLds {
  uint64_t sel[kSampleSort];
  double ev[kSampleMaxK];
  uint32_t hist[2048];
  double z;
  uint32_t cnt;
  RadixPick pick;
  int n_keep;
};

// k = min(top_k, V) in 1..kSampleMaxK; every thread of the workgroup calls it (barriers inside)
__device__ __forceinline__ void row_survivors(SurvivorLds& L, const void* row, int dtype, int V, int k, float temperature, float top_p) {
  const int tid = threadIdx.x;
  // gather every element whose composite key, shifted right by `shift`, is >= `bound`
  auto gather = [&](uint64_t bound, int shift) {
    if (tid == 0) L.cnt = 0;
    for (int i = tid; i < kSampleSort; i += kSampleThreads) L.sel[i] = 0;
    __syncthreads();
    for_each_logit(row, dtype, V, tid, [&](float x, int i) {
      const uint64_t c = composite_key(x, i);
      if ((c >> shift) >= bound) {
        const uint32_t slot = atomicAdd(&L.cnt, 1u);
        if (slot < static_cast<uint32_t>(kSampleSort)) L.sel[slot] = c + 1;  // 0 stays "empty" and sorts last
      }
    });
    __syncthreads();
  };

  // ---- 1a. fast path: the k-th largest thread maximum bounds the k-th largest element from below
  {
    uint64_t best = 0;
    for_each_logit(row, dtype, V, tid, [&](float x, int i) {
      const uint64_t c = composite_key(x, i);
      best = c > best ? c : best;
    });
    L.sel[tid] = best;  // threads without an element hold 0: below every real key
    __syncthreads();
    sort_desc(L.sel, kSampleThreads);
    const uint64_t tau = L.sel[k - 1];  // k <= min(1024, V): at least k threads saw an element
    __syncthreads();
    gather(tau, 0);
  }

  // ---- 1b. fallback: radix select on the composite key, most significant digits first
  if (L.cnt > static_cast<uint32_t>(kSampleSort)) {
    int decided;
    const uint64_t prefix = radix_select(row, dtype, V, k, kSampleCap, L.hist, L.pick, decided);
    gather(prefix, 52 - decided);
  }

  // ---- 2. sort the candidates (>= k of them, the k largest among them) descending
  int n_sort = 2;  // next power of two >= gathered count (workgroup-uniform)
  while (n_sort < static_cast<int>(L.cnt)) n_sort <<= 1;
  sort_desc(L.sel, n_sort);

  // ---- 3. the k survivors in sorted order: weights in float64
  const double T = static_cast<double>(temperature);
  const bool scale = (temperature > 0.f) && (temperature != 1.0f);
  int my_idx = 0;
  if (tid < k) {
    my_idx = key_index(L.sel[tid] - 1);
    double v = static_cast<double>(load_logit(row, dtype, my_idx));
    if (scale) v = v / T;
    L.ev[tid] = v;
  }
  __syncthreads();
  const double m = L.ev[0];
  __syncthreads();
  if (tid < k) {
    double e = exp(L.ev[tid] - m);
    if (e != e) e = 0.0;
    L.ev[tid] = e;
  }
  // sel[] is reused for the token ids of the survivors
  __syncthreads();
  if (tid < k) L.sel[tid] = static_cast<uint64_t>(my_idx);
  __syncthreads();
  if (tid == 0) {
    int n_keep = 1;
    double z2 = 1.0;
    if (is_finite_d(m)) {
      n_keep = k;
      if (top_p < 1.0f) {
        const double tp = static_cast<double>(top_p);
        double z = 0.0;
        for (int i = 0; i < k; ++i) z += L.ev[i];
        double cum = 0.0;
        n_keep = 0;
        for (int i = 0; i < k; ++i) {
          cum += L.ev[i] / z;
          if (i == 0 || !(cum > tp)) n_keep = i + 1;
          else break;
        }
      }
      z2 = 0.0;
      for (int i = 0; i < n_keep; ++i) z2 += L.ev[i];
    } else {
      L.ev[0] = 1.0;   // -inf / NaN / +inf on top: the point mass on the first id
    }
    L.n_keep = n_keep;
    L.z = z2;
  }
  __syncthreads();
}

// index of the weight a uniform u in [0, 1) lands on: the first j with u * z < w[0] + .. + w[j] (sequential), else the last
__device__ __forceinline__ int invert_weights(const double* w, int n, double z, double u) {
  const double target = u * z;
  double c = 0.0;
  for (int i = 0; i < n; ++i) {
    c += w[i];
    if (target < c) return i;
  }
  return n - 1;
}

// the uniform r0 * 2^-32 of Philox counter (draw, stream, 0, tag)
__device__ __forceinline__ double philox_uniform(uint32_t draw, uint32_t sid, uint32_t tag, uint32_t seed_lo, uint32_t seed_hi) {
  uint32_t r0;
  philox4x32_10(draw, sid, 0u, tag, seed_lo, seed_hi, r0);
  return static_cast<double>(r0) * 2.3283064365386963e-10;  // 2^-32
}

// the Gumbel noise -log(-log(u)), u = (r0 + 0.5) * 2^-32 in (0, 1), of Philox counter (draw, stream, element, kTagGumbel)
__device__ __forceinline__ double gumbel_noise(uint32_t draw, uint32_t sid, int i, uint32_t seed_lo, uint32_t seed_hi) {
  uint32_t r0;
  philox4x32_10(draw, sid, static_cast<uint32_t>(i), kTagGumbel, seed_lo, seed_hi, r0);
  const double u = (static_cast<double>(r0) + 0.5) * 2.3283064365386963e-10;  // 2^-32
  return -log(-log(u));
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-row parameters (sd_row_sampling, include/specdec_hip.h): the ONE normalisation of a table entry, used by every _rows
// kernel. The table is device memory the host cannot check at launch, so whatever bits an entry holds come out as values the
// scalar kernels accept: top_k in 0..kSampleMaxK after the clamp to V, top_p in (0, 1], temperature > 0, penalties the scalar
// entries take. `spec`: the speculative-sampling kernels, where the full-vocabulary nucleus is a greedy row too.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ sd_row_sampling normalise_row_sampling(const sd_row_sampling* table, int b, int V, bool spec) {
  // a 32-byte entry of a 16-byte aligned table: two 16-byte loads
  const uint4 w0 = reinterpret_cast<const uint4*>(table)[2 * b], w1 = reinterpret_cast<const uint4*>(table)[2 * b + 1];
  sd_row_sampling e;
  e.temperature = __uint_as_float(w0.x);
  e.top_k = static_cast<int32_t>(w0.y);
  e.top_p = __uint_as_float(w0.z);
  e.seed_lo = w0.w;
  e.seed_hi = w1.x;
  e.repetition_penalty = __uint_as_float(w1.y);
  e.presence_penalty = __uint_as_float(w1.z);
  e.frequency_penalty = __uint_as_float(w1.w);
  if (e.top_k < 0) e.top_k = 0;
  if (e.top_p >= 1.0f) e.top_p = 1.0f;
  const bool greedy = !(e.temperature > 0.f) || min(e.top_k, V) > kSampleMaxK || !(e.top_p > 0.f) ||
                      (spec && e.top_k == 0 && e.top_p < 1.0f);
  if (greedy) {
    e.temperature = 1.0f;
    e.top_k = 1;
    e.top_p = 1.0f;
  }
  const bool pen_ok = e.repetition_penalty > 0.f && (e.presence_penalty - e.presence_penalty == 0.f) &&
                      (e.frequency_penalty - e.frequency_penalty == 0.f);
  if (!pen_ok) {
    e.repetition_penalty = 1.0f;
    e.presence_penalty = 0.f;
    e.frequency_penalty = 0.f;
  }
  return e;
}

// the Philox key words of a 64-bit seed
inline uint32_t seed_lo32(uint64_t seed) { return static_cast<uint32_t>(seed); }
inline uint32_t seed_hi32(uint64_t seed) { return static_cast<uint32_t>(seed >> 32); }

}  // namespace sd

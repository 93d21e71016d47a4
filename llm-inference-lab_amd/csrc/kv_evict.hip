// KV eviction for gfx950 (the rolling context window): in ONE cache row of a bound dense cache, positions
// [keep + drop, n_pos) become positions [keep, n_pos - drop) — all layers, all KV heads, K and V in ONE launch, in place.
// The first `keep` positions (the attention sinks) and every other row are not touched; the `drop` positions after the
// sinks are what is forgotten. Layouts as in kv_fork.hip (include/specdec_hip.h):
//   K: [n_layers][B][Hkv][Lmax][D]        V: [n_layers][B][Hkv][D][Lmax]   (bf16)
//   V moves bit for bit along each d row. Source and destination of an element are `drop` elements apart and drop % 8 == 0,
//      so both sit in the same 16-byte phase: the destination units that lie whole inside [keep, n_pos - drop) go as uint4,
//      the elements of the (at most two) units that straddle an edge one by one. A unit is never widened past the range
//      that may be read or written.
//   K is stored AFTER RoPE, so a key that moves to a position `drop` lower is rotated by -drop: with the rotate-half pairing
//      (i, i + D/2), c = cos[drop][i] and s = sin[drop][i] of the model's own fp32 tables, a' = a c + b s and
//      b' = b c - a s, in fp32 from the stored bf16 values, rounded once to bf16. A position row is D * 2 bytes: K is
//      always whole units, whatever `keep` is.
//
// THE HAZARD AND THE OWNERSHIP RULE. The move overlaps itself whenever n_pos - keep - drop > drop: positions that are
// destinations early are sources later. Nothing here relies on an order between workgroups, on atomics or on waiting:
//   * The data splits into independent LANES. A V lane is one d row of one (layer, head). A K lane is one 16-byte unit
//     column of the first half of D together with its partner unit in the second half, of one (layer, head): position p
//     of a lane only ever feeds position p - drop of the SAME lane.
//   * Every lane is owned by exactly ONE workgroup, whole: workgroup x == 0 of a (layer, head) owns all its D / 16 K lanes
//     (so it reads and writes whole, contiguous position rows), workgroup x >= 1 owns the kEvictRows V lanes
//     d in [(x - 1) * kEvictRows, x * kEvictRows). No other workgroup reads or writes a byte of them.
//   * The owner walks its lanes in ASCENDING chunks of kEvictChunk destination positions (V chunks are cut at multiples
//     of 8 positions). Per chunk: all loads of all threads -> s_waitcnt vmcnt(0) -> __syncthreads() -> all stores.
//     Chunk i stores below the positions chunk i + 1 loads (destinations are `drop` >= 8 below their sources and chunks
//     ascend), and what it overwrites was loaded by chunk i itself or an earlier one — before this barrier, by every
//     thread of the workgroup. One barrier per chunk is therefore enough, and the chunk count depends on the arguments
//     only: every thread reaches every barrier.
// Offsets are 64-bit as in kv_fork.hip (n_layers * B * Hkv * Lmax * D passes 2^31 elements at 8B dimensions).

#include "common.h"
#include "kernels.h"

namespace sd {

constexpr int kEvictThreads = 256;
constexpr int kEvictChunk = 128;   // destination positions per chunk (tests/test_hip_kv_evict_gpu.py crosses three of them)
constexpr int kEvictRows = 16;     // V lanes (d rows) per workgroup: 16 rows x 16 units = one unit per thread and chunk
constexpr int kEvictKItems = kEvictChunk * (128 / 16) / kEvictThreads;   // K (position, lane) items per thread at D = 128
static_assert(kEvictRows * (kEvictChunk / 8) == kEvictThreads, "one V unit per thread and chunk");
static_assert(kEvictThreads % (128 / 16) == 0, "a thread keeps one K lane: its cos / sin values are loaded once");

struct EvictArgs {
  uint16_t* k;
  uint16_t* v;
  const float* rope_cos;   // row `drop` of the model's tables: [D / 2]
  const float* rope_sin;
  int B, Hkv, Lmax, D;
  int row, keep, drop, n_pos;
};

__device__ __forceinline__ uint32_t rotate_back_pair(uint32_t a2, uint32_t b2, const float* c, const float* s, uint32_t* b_out) {
  const float a0 = __uint_as_float(a2 << 16), a1 = __uint_as_float(a2 & 0xffff0000u);
  const float b0 = __uint_as_float(b2 << 16), b1 = __uint_as_float(b2 & 0xffff0000u);
  const uint32_t ra = static_cast<uint32_t>(float_to_bf16_bits(a0 * c[0] + b0 * s[0])) |
                      (static_cast<uint32_t>(float_to_bf16_bits(a1 * c[1] + b1 * s[1])) << 16);
  *b_out = static_cast<uint32_t>(float_to_bf16_bits(b0 * c[0] - a0 * s[0])) |
           (static_cast<uint32_t>(float_to_bf16_bits(b1 * c[1] - a1 * s[1])) << 16);
  return ra;
}

__global__ __launch_bounds__(kEvictThreads) void kv_evict_kernel(EvictArgs a) {
  const int lh = blockIdx.y;                 // layer * Hkv + head
  const int layer = lh / a.Hkv, head = lh - layer * a.Hkv;
  const int64_t seg = static_cast<int64_t>(a.Lmax) * a.D;                        // elements of one (layer, row, head)
  const int64_t base = ((static_cast<int64_t>(layer) * a.B + a.row) * a.Hkv + head) * seg;
  const int end = a.n_pos - a.drop;          // destinations are [keep, end)
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    // ---- K: all D / 16 lanes of this (layer, head). Item = (position, lane j): units j and j + D / 16 of the position row.
    uint16_t* __restrict__ kp = a.k + base;
    const int upp = a.D >> 4;                // lanes = pair units per position: 2, 4 or 8
    const int j = tid & (upp - 1);           // kEvictThreads % upp == 0: the same lane for every item of this thread
    float c[8], s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      c[e] = a.rope_cos[j * 8 + e];
      s[e] = a.rope_sin[j * 8 + e];
    }
    const int half = a.D >> 1;
    const int pos_per_pass = kEvictThreads / upp;
    for (int p0 = a.keep; p0 < end; p0 += kEvictChunk) {
      const int p1 = p0 + kEvictChunk < end ? p0 + kEvictChunk : end;
      uint4 va[kEvictKItems], vb[kEvictKItems];
#pragma unroll
      for (int it = 0; it < kEvictKItems; ++it) {
        const int p = p0 + it * pos_per_pass + tid / upp;                         // destination position
        if (it * pos_per_pass < kEvictChunk && p < p1) {
          const uint16_t* src = kp + static_cast<int64_t>(p + a.drop) * a.D + j * 8;
          va[it] = *reinterpret_cast<const uint4*>(src);
          vb[it] = *reinterpret_cast<const uint4*>(src + half);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the loads have returned, not merely been issued
      __syncthreads();
#pragma unroll
      for (int it = 0; it < kEvictKItems; ++it) {
        const int p = p0 + it * pos_per_pass + tid / upp;
        if (it * pos_per_pass < kEvictChunk && p < p1) {
          uint4 ra, rb;
          ra.x = rotate_back_pair(va[it].x, vb[it].x, c + 0, s + 0, &rb.x);
          ra.y = rotate_back_pair(va[it].y, vb[it].y, c + 2, s + 2, &rb.y);
          ra.z = rotate_back_pair(va[it].z, vb[it].z, c + 4, s + 4, &rb.z);
          ra.w = rotate_back_pair(va[it].w, vb[it].w, c + 6, s + 6, &rb.w);
          uint16_t* dst = kp + static_cast<int64_t>(p) * a.D + j * 8;
          *reinterpret_cast<uint4*>(dst) = ra;
          *reinterpret_cast<uint4*>(dst + half) = rb;
        }
      }
    }
  } else {
    // ---- V: kEvictRows lanes (d rows). Per chunk a thread has one destination unit [q, q + 8) of one row.
    const int d = (blockIdx.x - 1) * kEvictRows + tid / (kEvictChunk / 8);
    uint16_t* __restrict__ vp = a.v + base + static_cast<int64_t>(d) * a.Lmax;
    const int u = tid & (kEvictChunk / 8 - 1);
    for (int p0 = a.keep & ~7; p0 < end; p0 += kEvictChunk) {
      const int q = p0 + u * 8;
      const int lo = q > a.keep ? q : a.keep, hi = q + 8 < end ? q + 8 : end;    // this unit's destinations: [lo, hi)
      const bool whole = hi - lo == 8;
      uint4 val = {0u, 0u, 0u, 0u};
      uint16_t el[8];
      if (whole) {
        val = *reinterpret_cast<const uint4*>(vp + q + a.drop);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) el[e] = (q + e >= lo && q + e < hi) ? vp[q + e + a.drop] : static_cast<uint16_t>(0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (whole) {
        *reinterpret_cast<uint4*>(vp + q) = val;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (q + e >= lo && q + e < hi) vp[q + e] = el[e];
      }
    }
  }
}

// Callers have validated row, keep, drop and n_pos against the bound geometry and the model's tables (sd_model_kv_evict).
int launch_kv_evict(uint16_t* k, uint16_t* v, const float* rope_cos, const float* rope_sin, int n_layers, int B, int Hkv, int Lmax, int D,
                    int row, int keep, int drop, int n_pos, hipStream_t st) {
  if (n_pos - keep - drop <= 0) return 0;
  SD_REQUIRE(D == 32 || D == 64 || D == 128, "kv_evict: head_dim %d (32, 64 or 128)", D);
  SD_REQUIRE(Lmax % 8 == 0 && drop % 8 == 0, "kv_evict: Lmax %d and drop %d must be multiples of 8", Lmax, drop);
  SD_REQUIRE(static_cast<int64_t>(n_layers) * Hkv <= 65535, "kv_evict: %d layers x %d kv heads exceed the grid", n_layers, Hkv);
  SD_REQUIRE(static_cast<int64_t>(Lmax) * D < (1ll << 31), "kv_evict: %d positions x head_dim %d per head exceed 2^31", Lmax, D);
  EvictArgs a{};
  a.k = k, a.v = v;
  a.rope_cos = rope_cos + static_cast<size_t>(drop) * (D / 2);
  a.rope_sin = rope_sin + static_cast<size_t>(drop) * (D / 2);
  a.B = B, a.Hkv = Hkv, a.Lmax = Lmax, a.D = D;
  a.row = row, a.keep = keep, a.drop = drop, a.n_pos = n_pos;
  hipLaunchKernelGGL(kv_evict_kernel, dim3(1 + D / kEvictRows, n_layers * Hkv), dim3(kEvictThreads), 0, st, a);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd

// KV fork for gfx950: the first n_pos positions of one cache slot copied into other slots of the same bound cache — all
// layers, all KV heads, K and V in ONE launch.
//
// A "slot" is what a cache tensor is indexed by after the layer: a batch row of a dense cache (Lslot = Lmax positions) or
// a page of a paged pool (Lslot = page_len positions). Both have the layouts of include/specdec_hip.h:
//   K: [n_layers][n_slots][Hkv][Lslot][D]        V: [n_layers][n_slots][Hkv][D][Lslot]   (bf16)
// so one body serves sd_model_kv_fork (one source row, R destination rows) and sd_model_kv_copy_pages (a list of
// source -> destination page pairs). The lists travel in the kernel's argument block (<= kForkMaxList entries per
// launch, the host splits longer ones): no device allocation, no host-to-device copy, no synchronisation.
//
// Pure byte movement, like kv_append.hip: consecutive lanes take consecutive 16-byte units, so a wave moves 1 KiB of
// contiguous bytes per dwordx4 instruction. Every source unit is loaded ONCE and stored to all `fan` destinations of
// its group — that is what makes this a kernel and not R x 2 x n_layers strided memcpys.
//   K, per (layer, head): n_pos * D contiguous bf16 — always whole units (D is 32, 64 or 128).
//   V, per (layer, head): D rows of n_pos elements at stride Lslot. Row starts are 16-byte aligned (Lslot % 8 == 0);
//      whole units go as uint4, the last n_pos % 8 elements one by one: a tail is never widened to a full unit, so
//      positions >= n_pos of a destination are neither read nor written.
// The grid's y is the (layer, head) pair and z the (group, tensor) pair; offsets of a slot are 64-bit (n_layers * B *
// Hkv * Lmax * D passes 2^31 elements at 8B dimensions with 32 K positions).

#include "common.h"
#include "kernels.h"

namespace sd {

constexpr int kForkThreads = 256;
constexpr int kForkMaxBlocksX = 64;   // per (layer, head, group, tensor): the rest of a long segment is grid-strided

struct ForkArgs {
  uint16_t* k;
  uint16_t* v;
  int n_slots, Hkv, Lslot, D;
  int n_pos;
  int fan;                       // destinations per group (>= 1); group g stores to dst[g * fan .. g * fan + fan)
  int32_t src[kForkMaxList];     // per group
  int32_t dst[kForkMaxList];     // n_groups * fan <= kForkMaxList entries
};

__global__ __launch_bounds__(kForkThreads) void kv_fork_kernel(ForkArgs a) {
  const int lh = blockIdx.y;                 // layer * Hkv + head
  const int g = blockIdx.z >> 1;
  const int layer = lh / a.Hkv, head = lh - layer * a.Hkv;
  const int64_t seg = static_cast<int64_t>(a.Lslot) * a.D;                       // elements of one (layer, slot, head)
  // element offset of (layer, slot 0, head); a slot adds slot * Hkv * seg
  const int64_t base = (static_cast<int64_t>(layer) * a.n_slots * a.Hkv + head) * seg;
  const int64_t slot_stride = static_cast<int64_t>(a.Hkv) * seg;
  const int64_t s_off = base + a.src[g] * slot_stride;
  const int32_t* __restrict__ dsts = a.dst + g * a.fan;
  const int stride = gridDim.x * kForkThreads;
  if ((blockIdx.z & 1) == 0) {
    // ---- K: n_pos * D contiguous elements = n_pos * D / 8 units
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(a.k + s_off);
    const int units = a.n_pos * (a.D >> 3);
    for (int u = blockIdx.x * kForkThreads + threadIdx.x; u < units; u += stride) {
      const uint4 val = src[u];
      for (int r = 0; r < a.fan; ++r) reinterpret_cast<uint4*>(a.k + base + dsts[r] * slot_stride)[u] = val;
    }
  } else {
    // ---- V: D rows of n_pos elements at stride Lslot; per row vu whole units, then one item for the tail
    const int vu = a.n_pos >> 3, tail = a.n_pos & 7;
    const int per_row = vu + (tail ? 1 : 0);
    const int items = a.D * per_row;
    for (int i = blockIdx.x * kForkThreads + threadIdx.x; i < items; i += stride) {
      const int d = i / per_row, j = i - d * per_row;
      const int64_t off = static_cast<int64_t>(d) * a.Lslot + (j << 3);            // within the (layer, slot, head) segment
      if (j < vu) {
        const uint4 val = *reinterpret_cast<const uint4*>(a.v + s_off + off);
        for (int r = 0; r < a.fan; ++r) *reinterpret_cast<uint4*>(a.v + base + dsts[r] * slot_stride + off) = val;
      } else {
        for (int e = 0; e < tail; ++e) {
          const uint16_t val = a.v[s_off + off + e];
          for (int r = 0; r < a.fan; ++r) a.v[base + dsts[r] * slot_stride + off + e] = val;
        }
      }
    }
  }
}

// src: n_groups entries; dst: n_groups * fan entries, group-major. Callers have validated every index against n_slots,
// n_pos against Lslot, and that no destination is a source or listed twice (slots of one launch must not overlap).
int launch_kv_fork(uint16_t* k, uint16_t* v, int n_layers, int n_slots, int Hkv, int Lslot, int D, const int32_t* src,
                   const int32_t* dst, int n_groups, int fan, int n_pos, hipStream_t st) {
  if (n_groups <= 0 || fan <= 0 || n_pos <= 0) return 0;
  SD_REQUIRE(Lslot % 8 == 0 && D % 8 == 0, "kv_fork: Lmax / page_len %d and head_dim %d must be multiples of 8", Lslot, D);
  SD_REQUIRE(n_pos <= Lslot, "kv_fork: n_pos=%d exceeds %d", n_pos, Lslot);
  SD_REQUIRE(static_cast<int64_t>(n_layers) * Hkv <= 65535, "kv_fork: %d layers x %d kv heads exceed the grid", n_layers, Hkv);
  SD_REQUIRE(static_cast<int64_t>(Lslot) * D < (1ll << 31), "kv_fork: %d positions x head_dim %d per head exceed 2^31", Lslot, D);
  const int units = n_pos * (D / 8);                                   // K units per segment; V has no more items
  int gx = (units + kForkThreads - 1) / kForkThreads;
  if (gx > kForkMaxBlocksX) gx = kForkMaxBlocksX;
  ForkArgs a{};
  a.k = k, a.v = v;
  a.n_slots = n_slots, a.Hkv = Hkv, a.Lslot = Lslot, a.D = D, a.n_pos = n_pos;
  if (n_groups == 1) {
    // one source, `fan` destinations: chunks of <= kForkMaxList destinations (a chunk re-reads the source)
    for (int r0 = 0; r0 < fan; r0 += kForkMaxList) {
      const int n = fan - r0 < kForkMaxList ? fan - r0 : kForkMaxList;
      a.fan = n;
      a.src[0] = src[0];
      for (int i = 0; i < n; ++i) a.dst[i] = dst[r0 + i];
      hipLaunchKernelGGL(kv_fork_kernel, dim3(gx, n_layers * Hkv, 2), dim3(kForkThreads), 0, st, a);
      SD_LAUNCH_CHECK();
    }
    return 0;
  }
  SD_REQUIRE(fan == 1, "kv_fork: a list of pairs has one destination per source");
  for (int g0 = 0; g0 < n_groups; g0 += kForkMaxList) {
    const int n = n_groups - g0 < kForkMaxList ? n_groups - g0 : kForkMaxList;
    a.fan = 1;
    for (int i = 0; i < n; ++i) a.src[i] = src[g0 + i], a.dst[i] = dst[g0 + i];
    hipLaunchKernelGGL(kv_fork_kernel, dim3(gx, n_layers * Hkv, 2 * n), dim3(kForkThreads), 0, st, a);
    SD_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace sd

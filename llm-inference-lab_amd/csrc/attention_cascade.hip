// Cascade attention for gfx950: rows forked from one prompt read the shared keys ONCE per (group, kv head), not once per row.
//
// attention_mfma_kernel (attention.hip) runs one workgroup per (row, kv head, 16-query tile) and each streams the whole cache of
// its row: n completions of one long prompt read the same keys n times per layer. Here a per-row table `share` (AttnArgs:
// {leader, shared_len} per bound row, sd_model_set_shared_prefix) says that keys [0, shared_len[b]) of row b are bit-identical to
// the same positions of row leader[b], and one launch does two kinds of work (blockIdx.z picks the kind):
//
//   prefix   one workgroup per (group, kv head, SET of up to NT = 4 query tiles, key split). The query rows of a group are its
//            member rows x G query heads x M positions, stacked densely (member-major) into 16-row tiles; a set is 64 stacked
//            rows. Per 32-key block of the LEADER's cache a wave loads the K fragments and the V^T fragments once and uses
//            them from registers for every tile of the set: NT x D/32 MFMAs for S^T, an online softmax per tile, NT x D/16
//            MFMAs for P.V (the lane layouts of attention_tile, so P is the next A operand unpermuted). The 4 waves take the
//            blocks round-robin; a group's keys are split over workgroups as the plain kernel splits them (one per 512 keys of
//            the group's longest shared length). No causal mask: shared_len[b] <= the row's first query position, so every shared
//            key is visible to every query of the row; the only mask is key < shared_len[row], per query row, because members
//            of one group may share different lengths.
//   suffix   one workgroup per (row, kv head, tile, key split): keys [shared_len[b], pos0 + M) of the row's OWN cache with the
//            causal mask. A row in no group has shared_len 0: the plain computation, block order and merge order included.
//   merge    every workgroup leaves a fp32 (O, max, sum) partial per query row it served in the mode's own workspace, slot
//            `split` (suffix) or n_split + split (prefix) of the row's (row, kv head, tile), and arrives on that tile's counter.
//            The number of arrivals a tile expects follows from the table and the rows' lengths alone, so every arriver
//            computes the same figure; the last one merges by log-sum-exp and stores bf16. The hand-over is the split-KV one:
//            agent-scope relaxed stores and loads of the partials, one acq_rel arrival, the counter reset by the last arrival.
//            Nothing waits. A tile that expects one arrival (ungrouped row, one split) is stored directly.
//
// The grid is fixed from B, M, l_max and the head counts (attention_cascade_plan): a prefix workgroup sits at grid row b and
// serves the group whose FIRST member in the pass is row b; every other one returns at entry, before any barrier, so a captured
// step stays valid while groups form and dissolve. Register budget (D = 128, 256 threads): Q fragments NT x 16 + accumulators
// NT x 32 + one block's K / V fragments 64 dwords per lane; see DESIGN.md for the compiler's count.

#include <stdlib.h>

#include "attention_device.h"

namespace sd {

constexpr int kCascadeNT = 4;                              // query tiles a prefix workgroup serves from one load of a block
constexpr int kCascadeSetRows = kCascadeNT * kAttnRows;    // stacked query rows of a set
constexpr int kCascadeMaxRows = kSkinnyMaxT;               // rows of a pass (B * M <= kSkinnyMaxT)
constexpr int kCascadeThreads = 256, kCascadeWaves = 4;

// workgroups a stretch of `blocks` 32-key blocks is split over: the plain kernel's rule (one per 512 keys, at most ns)
__device__ __forceinline__ int cascade_split(int ns, int blocks) {
  return ns > 1 ? min(ns, max(1, (blocks + kAttnSplitBlocks - 1) / kAttnSplitBlocks)) : 1;
}
// sets whose stacked rows meet tile tq of the group's member number j (1 or 2)
__device__ __forceinline__ int cascade_touch(int j, int tq, int R) {
  const int lo = j * R + kAttnRows * tq, hi = j * R + min(kAttnRows * tq + kAttnRows, R) - 1;
  return hi / kCascadeSetRows - lo / kCascadeSetRows + 1;
}
// workgroups that serve the suffix of a row whose first query sits at pos0
__device__ __forceinline__ int cascade_suffix_split(const AttnArgs& a, int pos0, int shared_len) {
  const int n_keys = max(0, min(pos0 + static_cast<int>(a.M), a.l_max));
  return cascade_split(a.n_split, (n_keys + kAttnBlock - 1) / kAttnBlock - (shared_len >> 5));
}

// Row b of the pass in the table: its own entry and, for a member, its number among the pass's members of the group, and
// the group's longest shared length. Wave-uniform scalar reads.
struct CascadeRow { int len, ordinal, grp_len; };
__device__ __forceinline__ CascadeRow cascade_row(const AttnArgs& a, int b) {
  const int32_t* sh = a.share + 2 * a.row0;
  CascadeRow r{sh[2 * b + 1], 0, 0};
  if (r.len <= 0) { r.len = 0; return r; }
  const int leader = sh[2 * b];
  for (int i = 0; i < a.B; ++i)
    if (sh[2 * i] == leader && sh[2 * i + 1] > 0) {
      if (i < b) ++r.ordinal;
      r.grp_len = max(r.grp_len, sh[2 * i + 1]);
    }
  return r;
}

// every load of one 32-key block of cache row `row` (a row of the BOUND batch): the fragments of attention_tile
template <int D, bool PAGED>
__device__ __forceinline__ void cascade_load_block(const AttnArgs& a, int row, int kvh, int key0, int g, int n, u32x4 (&kf)[2][D / 32],
                                                   u32x4 (&vf)[D / 16]) {
  const int vstride = PAGED ? (1 << a.page_shift) : a.l_max;
  const uint16_t *kc, *vt;
  int kbase = key0;
  if constexpr (PAGED) {
    const int pg = __builtin_amdgcn_readfirstlane(a.block_table[row * (a.l_max >> a.page_shift) + (key0 >> a.page_shift)]);
    kc = static_cast<const uint16_t*>(a.k_cache) + ((static_cast<size_t>(pg) * a.n_kv_heads + kvh) << a.page_shift) * D;
    vt = static_cast<const uint16_t*>(a.v_cache) + ((static_cast<size_t>(pg) * a.n_kv_heads + kvh) * D << a.page_shift);
    kbase = key0 & (vstride - 1);
  } else {
    const size_t slab = (static_cast<size_t>(row) * a.n_kv_heads + kvh) * a.l_max * D;
    kc = static_cast<const uint16_t*>(a.k_cache) + slab;
    vt = static_cast<const uint16_t*>(a.v_cache) + slab;
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    int key = kbase + 8 * (n >> 2) + 4 * u + (n & 3);
    if (!PAGED && key >= a.l_max) key = a.l_max - 1;   // stay inside the cache; masked by the caller's limit
    const uint16_t* krow = kc + static_cast<size_t>(key) * D + g * 8;
#pragma unroll
    for (int s = 0; s < D / 32; ++s) kf[u][s] = *reinterpret_cast<const u32x4*>(krow + s * 32);
  }
  int kofs = kbase + 8 * g;
  if (!PAGED && kofs + 8 > a.l_max) kofs = a.l_max - 8;
  const uint16_t* vrow = vt + static_cast<size_t>(n) * vstride + kofs;
#pragma unroll
  for (int i = 0; i < D / 16; ++i) vf[i] = *reinterpret_cast<const u32x4*>(vrow + static_cast<size_t>(16 * i) * vstride);
}

// one 16-row query tile against a loaded block: S^T, the online softmax of the lane's query row (keys < lim are visible), P.V.
// The arithmetic, in order, of attention_tile's block.
template <int D>
__device__ __forceinline__ void cascade_tile_block(float scale, const u32x4 (&kf)[2][D / 32], const u32x4 (&vf)[D / 16],
                                                   const u32x4 (&qf)[D / 32], int key0, int g, int lim, f32x4_t (&oacc)[D / 16], float& m_run,
                                                   float& l_run) {
  f32x4_t st[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    st[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < D / 32; ++s)
      st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf[u][s]), __builtin_bit_cast(bf16x8_t, qf[s]), st[u], 0, 0, 0);
  }
  float sc[8];
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = key0 + 8 * g + 4 * u + r;
      const float v = (key < lim) ? st[u][r] * scale : -INFINITY;
      sc[4 * u + r] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float m_new = fmaxf(m_run, mx);
  float alpha = 1.f, psum = 0.f;
  float p[8];
  if (m_new > -INFINITY) {
    alpha = (m_run > -INFINITY) ? __expf(m_run - m_new) : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p[j] = (sc[j] > -INFINITY) ? __expf(sc[j] - m_new) : 0.f;
      psum += p[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = 0.f;
  }
  psum += __shfl_xor(psum, 16, 64);
  psum += __shfl_xor(psum, 32, 64);
  l_run = l_run * alpha + psum;
  m_run = m_new;
  const u32x4 pf = {pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), pack_bf16x2(p[4], p[5]), pack_bf16x2(p[6], p[7])};
  float al[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) al[r] = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
  for (int i = 0; i < D / 16; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) oacc[i][r] *= al[r];
    oacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, pf), __builtin_bit_cast(bf16x8_t, vf[i]), oacc[i], 0, 0, 0);
  }
}

// LDS of a workgroup: the waves' partials of ONE tile, O[4][16][D], max[4][16], sum[4][16] (attention_tile's carve)
template <int D>
struct CascadeLds {
  float *o, *m, *l;
  __device__ explicit CascadeLds(unsigned char* smem)
      : o(reinterpret_cast<float*>(smem)), m(o + kCascadeWaves * kAttnRows * D), l(m + kCascadeWaves * kAttnRows) {}
};

template <int D>
__device__ __forceinline__ void cascade_waves_to_lds(const CascadeLds<D>& s, int wave, int g, int n, const f32x4_t (&oacc)[D / 16], float m_run,
                                                     float l_run) {
  if (g == 0) {
    s.m[wave * kAttnRows + n] = m_run;
    s.l[wave * kAttnRows + n] = l_run;
  }
#pragma unroll
  for (int i = 0; i < D / 16; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) s.o[(wave * kAttnRows + 4 * g + r) * D + 16 * i + n] = oacc[i][r];
}

// element (r, d) of the tile over the 4 waves: un-normalised numerator, denominator and the max they refer to
template <int D>
__device__ __forceinline__ void cascade_wave_merge(const CascadeLds<D>& s, int r, int d, float& num, float& den, float& mm) {
  mm = -INFINITY;
#pragma unroll
  for (int w = 0; w < kCascadeWaves; ++w) mm = fmaxf(mm, s.m[w * kAttnRows + r]);
  num = 0.f; den = 0.f;
#pragma unroll
  for (int w = 0; w < kCascadeWaves; ++w) {
    const float mw = s.m[w * kAttnRows + r];
    const float f = (mw > -INFINITY) ? __expf(mw - mm) : 0.f;
    num += f * s.o[(w * kAttnRows + r) * D + d];
    den += f * s.l[w * kAttnRows + r];
  }
}

template <int D>
__device__ __forceinline__ float* cascade_slot(const AttnArgs& a, int tile_index, int slot) {
  constexpr int PS = kAttnRows * (D + 2);   // floats per partial: O[16][D], max[16], sum[16]
  return a.split_ws + (static_cast<size_t>(tile_index) * (a.n_split + a.c_split) + slot) * PS;
}

// The last arrival of tile (b, kvh, tile): its s_s suffix partials (slots 0 ..) and s_p prefix partials (slots n_split ..) merged by
// log-sum-exp, in that order, and stored as bf16. Whole workgroup; ends on a barrier (the caller may merge another tile).
template <int D>
__device__ __forceinline__ void cascade_merge(const AttnArgs& a, int b, int kvh, int tile, int s_s, int s_p, unsigned char* smem) {
  constexpr int PS = kAttnRows * (D + 2);
  const int G = a.n_q_heads / a.n_kv_heads, M = a.M, R = G * M;
  const int tiles = (R + kAttnRows - 1) / kAttnRows, rows = min(kAttnRows, R - tile * kAttnRows);
  const int tid = threadIdx.x, n_parts = s_s + s_p;
  const float* base = cascade_slot<D>(a, (b * a.n_kv_heads + kvh) * tiles + tile, 0);
  float* pm = reinterpret_cast<float*>(smem);          // [n_parts][16] max
  float* pl = pm + 2 * kAttnMaxSplit * kAttnRows;      // [n_parts][16] sum
  for (int i = tid; i < n_parts * kAttnRows; i += kCascadeThreads) {
    const int part = i / kAttnRows, r = i - part * kAttnRows;
    const float* src = base + static_cast<size_t>(part < s_s ? part : a.n_split + part - s_s) * PS + kAttnRows * D;
    pm[i] = __hip_atomic_load(src + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pl[i] = __hip_atomic_load(src + kAttnRows + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  constexpr int CPR = D / 8;
  const int qstride = a.n_q_heads * D;
  uint16_t* out = static_cast<uint16_t*>(a.out);
  for (int c = tid; c < rows * CPR; c += kCascadeThreads) {
    const int r = c / CPR, d0 = (c - r * CPR) * 8;
    float mm = -INFINITY;
    for (int part = 0; part < n_parts; ++part) mm = fmaxf(mm, pm[part * kAttnRows + r]);
    float num[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    const float* src = base + r * D + d0;
#pragma unroll 4
    for (int part = 0; part < n_parts; ++part) {
      const size_t at = static_cast<size_t>(part < s_s ? part : a.n_split + part - s_s) * PS;
      const float4 v0 = coherent_load_f4(src + at);
      const float4 v1 = coherent_load_f4(src + at + 4);
      const float ms = pm[part * kAttnRows + r];
      const float f = (ms > -INFINITY) ? __expf(ms - mm) : 0.f;
      den += f * pl[part * kAttnRows + r];
      num[0] += f * v0.x; num[1] += f * v0.y; num[2] += f * v0.z; num[3] += f * v0.w;
      num[4] += f * v1.x; num[5] += f * v1.y; num[6] += f * v1.z; num[7] += f * v1.w;
    }
    const float inv = (den > 0.f) ? 1.0f / den : 0.f;
    const int rr = tile * kAttnRows + r, gh = rr / M, m = rr - gh * M;
    uint16_t* dst = out + static_cast<size_t>(b * M + m) * qstride + (kvh * G + gh) * D + d0;
    const u32x4 o = {pack_bf16x2(num[0] * inv, num[1] * inv), pack_bf16x2(num[2] * inv, num[3] * inv),
                     pack_bf16x2(num[4] * inv, num[5] * inv), pack_bf16x2(num[6] * inv, num[7] * inv)};
    *reinterpret_cast<u32x4*>(dst) = o;
  }
  __syncthreads();
}

// ---- suffix: row b's own keys from shared_len[b] on, causally: attention_tile's loop with a first block other than 0 ----------
template <int D, bool PAGED>
__device__ __forceinline__ void cascade_suffix(const AttnArgs& a, int kvh, int b, int tile, int split, unsigned char* smem) {
  constexpr int NKS = D / 32, NDT = D / 16;
  const int G = a.n_q_heads / a.n_kv_heads, M = a.M, R = G * M;
  const int r_base = tile * kAttnRows, rows = min(kAttnRows, R - r_base);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, n = lane & 15;
  const CascadeLds<D> lds(smem);

  const CascadeRow cr = cascade_row(a, b);
  const int pos0 = a.pos_base[b] + a.pos_off;
  const int n_keys = max(0, min(pos0 + M, a.l_max));
  const int n_blocks = (n_keys + kAttnBlock - 1) / kAttnBlock, first = cr.len >> 5;
  const int s_eff = cascade_split(a.n_split, n_blocks - first);
  if (split >= s_eff) return;   // workgroup-uniform, before any barrier
  const int s_p = cr.len > 0 ? cascade_split(a.c_split, cr.grp_len >> 5) : 0;
  const int expected = s_eff + (cr.len > 0 ? s_p * cascade_touch(cr.ordinal, tile, R) : 0);

  const int qstride = a.n_q_heads * D;
  u32x4 qf[NKS];
  int my_m = 0;
  {
    const uint16_t* q = static_cast<const uint16_t*>(a.q);
    const bool valid = n < rows;
    const int rr = r_base + (valid ? n : 0);
    const int gh = rr / M, m = rr - gh * M;
    my_m = m;
    const uint16_t* qrow = q + static_cast<size_t>(b * M + m) * qstride + (kvh * G + gh) * D + g * 8;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      if (valid) qf[s] = *reinterpret_cast<const u32x4*>(qrow + s * 32);
      else qf[s] = u32x4{0u, 0u, 0u, 0u};
    }
  }
  f32x4_t oacc[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) oacc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const int lim = min(pos0 + my_m + 1, n_keys);   // keys below it are visible to this lane's query
  for (int blk = first + split * kCascadeWaves + wave; blk < n_blocks; blk += kCascadeWaves * s_eff) {
    u32x4 kf[2][NKS], vf[NDT];
    cascade_load_block<D, PAGED>(a, a.row0 + b, kvh, blk * kAttnBlock, g, n, kf, vf);
    cascade_tile_block<D>(a.scale, kf, vf, qf, blk * kAttnBlock, g, lim, oacc, m_run, l_run);
  }
  cascade_waves_to_lds<D>(lds, wave, g, n, oacc, m_run, l_run);
  __syncthreads();
  uint16_t* out = static_cast<uint16_t*>(a.out);
  if (expected == 1) {   // a row in no group, one workgroup: the plain kernel's store
    for (int i = tid; i < rows * D; i += kCascadeThreads) {
      const int r = i / D, d = i - r * D;
      float num, den, mm;
      cascade_wave_merge<D>(lds, r, d, num, den, mm);
      const float v = (den > 0.f) ? num / den : 0.f;
      const int rr = r_base + r, gh = rr / M, m = rr - gh * M;
      out[static_cast<size_t>(b * M + m) * qstride + (kvh * G + gh) * D + d] = float_to_bf16_bits(v);
    }
    return;
  }
  const int tiles = (R + kAttnRows - 1) / kAttnRows;
  const int tile_index = (b * a.n_kv_heads + kvh) * tiles + tile;
  float* mine = cascade_slot<D>(a, tile_index, split);
  for (int i = tid; i < kAttnRows * D; i += kCascadeThreads) {
    const int r = i / D, d = i - r * D;
    float num, den, mm;
    cascade_wave_merge<D>(lds, r, d, num, den, mm);
    __hip_atomic_store(mine + i, num, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (d == 0) {
      __hip_atomic_store(mine + kAttnRows * D + r, mm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(mine + kAttnRows * D + kAttnRows + r, den, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // the hand-over of attention_tile: barrier, one acq_rel arrival by thread 0, barrier
  __syncthreads();
  unsigned* flag = reinterpret_cast<unsigned*>(lds.m);
  if (tid == 0) {
    const unsigned old = __hip_atomic_fetch_add(a.split_cnt + tile_index, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (old == static_cast<unsigned>(expected - 1));
    *flag = last ? 1u : 0u;
    if (last) __hip_atomic_store(a.split_cnt + tile_index, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (*flag == 0u) return;
  __syncthreads();   // (the flag word lies in the region the merge overwrites)
  cascade_merge<D>(a, b, kvh, tile, s_eff, s_p, smem);
}

// ---- prefix: the leader's keys [0, longest shared length of the set) for up to NT stacked query tiles of one group -------------
template <int D, bool PAGED>
__device__ __forceinline__ void cascade_prefix(const AttnArgs& a, int kvh, int b, int set, int split, unsigned char* smem) {
  constexpr int NKS = D / 32, NDT = D / 16, NT = kCascadeNT;
  __shared__ int mem_b[kCascadeMaxRows], mem_len[kCascadeMaxRows];   // the group's members in the pass, ascending
  __shared__ unsigned last_flag[kCascadeSetRows];                    // per (member, tile) this set meets: this workgroup merges it
  const int G = a.n_q_heads / a.n_kv_heads, M = a.M, R = G * M;
  const int tiles = (R + kAttnRows - 1) / kAttnRows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, n = lane & 15;
  const CascadeLds<D> lds(smem);

  // ---- is there work here? (wave-uniform scalar reads; every return is before the first barrier)
  const int32_t* sh = a.share + 2 * a.row0;
  const int leader = sh[2 * b];
  if (sh[2 * b + 1] <= 0) return;                                   // row b is in no group
  for (int i = 0; i < b; ++i)
    if (sh[2 * i] == leader && sh[2 * i + 1] > 0) return;           // the group belongs to the grid row of its first member
  int n_mem = 0, grp_len = 0;
  for (int i = b; i < a.B; ++i)
    if (sh[2 * i] == leader && sh[2 * i + 1] > 0) {
      if (tid == 0) { mem_b[n_mem] = i; mem_len[n_mem] = sh[2 * i + 1]; }
      ++n_mem;
      grp_len = max(grp_len, sh[2 * i + 1]);
    }
  const int set_lo = set * kCascadeSetRows, total = n_mem * R;
  if (set_lo >= total) return;
  const int s_p = cascade_split(a.c_split, grp_len >> 5);
  if (split >= s_p) return;
  __syncthreads();
  const int set_hi = min(total, set_lo + kCascadeSetRows);
  const int nt_here = (set_hi - set_lo + kAttnRows - 1) / kAttnRows;
  const int j0 = set_lo / R, j1 = (set_hi - 1) / R;
  int set_len = 0;
  for (int j = j0; j <= j1; ++j) set_len = max(set_len, mem_len[j]);
  const int n_blocks = set_len >> 5;

  // ---- Q fragments and the shared length of the lane's query row, per tile
  const int qstride = a.n_q_heads * D;
  u32x4 qf[NT][NKS];
  int lim[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int sr = set_lo + kAttnRows * t + n;
    const bool valid = sr < set_hi;
    const int srr = valid ? sr : set_lo;
    const int j = srr / R, r = srr - j * R, gh = r / M, m = r - gh * M;
    const uint16_t* qrow = static_cast<const uint16_t*>(a.q) + static_cast<size_t>(mem_b[j] * M + m) * qstride + (kvh * G + gh) * D + g * 8;
    lim[t] = valid ? mem_len[j] : 0;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      if (valid) qf[t][s] = *reinterpret_cast<const u32x4*>(qrow + s * 32);
      else qf[t][s] = u32x4{0u, 0u, 0u, 0u};
    }
  }
  f32x4_t oacc[NT][NDT];
  float m_run[NT], l_run[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    m_run[t] = -INFINITY;
    l_run[t] = 0.f;
#pragma unroll
    for (int i = 0; i < NDT; ++i) oacc[t][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  // ---- the blocks: loaded once, used by every tile of the set
  for (int blk = split * kCascadeWaves + wave; blk < n_blocks; blk += kCascadeWaves * s_p) {
    u32x4 kf[2][NKS], vf[NDT];
    cascade_load_block<D, PAGED>(a, leader, kvh, blk * kAttnBlock, g, n, kf, vf);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt_here) cascade_tile_block<D>(a.scale, kf, vf, qf[t], blk * kAttnBlock, g, lim[t], oacc[t], m_run[t], l_run[t]);
  }
  // ---- tile by tile through the LDS carve: the 4 waves merged, each query row's partial to ITS row's slot n_split + split
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t >= nt_here) continue;   // workgroup-uniform
    cascade_waves_to_lds<D>(lds, wave, g, n, oacc[t], m_run[t], l_run[t]);
    __syncthreads();
    const int rows_here = min(kAttnRows, set_hi - set_lo - kAttnRows * t);
    for (int i = tid; i < rows_here * D; i += kCascadeThreads) {
      const int row = i / D, d = i - row * D;
      const int sr = set_lo + kAttnRows * t + row;
      const int j = sr / R, r = sr - j * R;
      float num, den, mm;
      cascade_wave_merge<D>(lds, row, d, num, den, mm);
      float* dst = cascade_slot<D>(a, (mem_b[j] * a.n_kv_heads + kvh) * tiles + (r >> 4), a.n_split + split);
      __hip_atomic_store(dst + (r & 15) * D + d, num, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (d == 0) {
        __hip_atomic_store(dst + kAttnRows * D + (r & 15), mm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(dst + kAttnRows * D + kAttnRows + (r & 15), den, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
  }
  // ---- arrivals: one per (member, tile) whose rows this set holds (at most 64: each owns a stacked row of the set). Thread i takes
  // pair i; the barrier above ordered every thread's stores before it, its acq_rel arrival releases them (attention_tile's hand-over)
  int n_pairs = 0;
  for (int j = j0; j <= j1; ++j)
    for (int tq = 0; tq < tiles; ++tq) {
      const int lo = j * R + kAttnRows * tq, hi = j * R + min(kAttnRows * tq + kAttnRows, R);
      if (hi <= set_lo || lo >= set_hi) continue;
      if (n_pairs == tid) {
        const int bq = mem_b[j], tile_index = (bq * a.n_kv_heads + kvh) * tiles + tq;
        const int expected = cascade_suffix_split(a, a.pos_base[bq] + a.pos_off, mem_len[j]) + s_p * cascade_touch(j, tq, R);
        const unsigned old = __hip_atomic_fetch_add(a.split_cnt + tile_index, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = (old == static_cast<unsigned>(expected - 1));
        last_flag[tid] = last ? 1u : 0u;
        if (last) __hip_atomic_store(a.split_cnt + tile_index, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      ++n_pairs;
    }
  __syncthreads();
  int pair = 0;
  for (int j = j0; j <= j1; ++j)
    for (int tq = 0; tq < tiles; ++tq) {
      const int lo = j * R + kAttnRows * tq, hi = j * R + min(kAttnRows * tq + kAttnRows, R);
      if (hi <= set_lo || lo >= set_hi) continue;
      if (last_flag[pair++] == 0u) continue;   // workgroup-uniform
      const int bq = mem_b[j];
      cascade_merge<D>(a, bq, kvh, tq, cascade_suffix_split(a, a.pos_base[bq] + a.pos_off, mem_len[j]), s_p, smem);
    }
}

template <int D, bool PAGED>
__global__ __launch_bounds__(kCascadeThreads) void attention_cascade_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int G = a.n_q_heads / a.n_kv_heads, tiles = (G * a.M + kAttnRows - 1) / kAttnRows;
  const int n_suffix = tiles * a.n_split;
  int z = blockIdx.z;
  if (z < n_suffix) {
    cascade_suffix<D, PAGED>(a, blockIdx.x, blockIdx.y, z / a.n_split, z % a.n_split, smem);
  } else {
    z -= n_suffix;
    cascade_prefix<D, PAGED>(a, blockIdx.x, blockIdx.y, z / a.c_split, z % a.c_split, smem);
  }
}

// one table entry, on the stream (a kernel, so that a captured step may follow it without a host copy in between)
__global__ void cascade_set_entry_kernel(int32_t* share, int row, int leader, int shared_len) {
  share[2 * row] = leader;
  share[2 * row + 1] = shared_len;
}
int launch_cascade_set_entry(int32_t* share, int row, int leader, int shared_len, hipStream_t st) {
  hipLaunchKernelGGL(cascade_set_entry_kernel, dim3(1), dim3(1), 0, st, share, row, leader, shared_len);
  SD_LAUNCH_CHECK();
  return 0;
}

int attention_cascade_plan(int n_q_heads, int n_kv_heads, int head_dim, int B, int M, int l_max, int page_shift, CascadePlan& plan) {
  AttnPlan base{};
  if (int rc = attention_plan(n_q_heads, n_kv_heads, head_dim, B, M, l_max, page_shift, true, kAttnSplitSlots, base)) return rc;
  SD_REQUIRE(l_max % kAttnBlock == 0, "attention: a cascade launch needs l_max %% 32 == 0 (got %d)", l_max);
  SD_REQUIRE(B <= kCascadeMaxRows, "attention: a cascade launch holds at most %d rows (got %d)", kCascadeMaxRows, B);
  const int R = n_q_heads / n_kv_heads * M;
  const int stacked_tiles = (B * R + kAttnRows - 1) / kAttnRows;
  const int sets = (stacked_tiles + kCascadeNT - 1) / kCascadeNT;
  // prefix split: the plain rule over the workgroups one group of all B rows would have (Hkv * sets)
  int ps = 1;
  if (!getenv(debug_env::kNoAttnSplit)) {
    ps = l_max / (kAttnBlock * kAttnSplitBlocks);
    if (ps > kAttnMaxSplit) ps = kAttnMaxSplit;
    if (ps > 512 / (n_kv_heads * sets)) ps = 512 / (n_kv_heads * sets);
    if (ps < 1) ps = 1;
  }
  plan = CascadePlan{base.tiles, base.n_split, sets, ps, n_kv_heads * B * base.tiles * (base.n_split + ps),
                     n_kv_heads, B, base.tiles * base.n_split + sets * ps};
  return 0;
}

size_t attention_cascade_ws_bytes(int head_dim, int slots) { return static_cast<size_t>(slots) * kAttnRows * (head_dim + 2) * sizeof(float); }

static size_t cascade_smem_bytes(int D) {
  const size_t n = sizeof(float) * (static_cast<size_t>(kCascadeWaves) * kAttnRows * D + 2 * kCascadeWaves * kAttnRows);
  const size_t merge = sizeof(float) * 2 * (2 * kAttnMaxSplit) * kAttnRows;   // (max, sum) of up to 32 + 32 partials
  return n > merge ? n : merge;
}

template <int D>
static void launch_cascade_d(const AttnArgs& a, dim3 grid, hipStream_t st) {
  const size_t smem = cascade_smem_bytes(D);
  if (a.block_table) hipLaunchKernelGGL((attention_cascade_kernel<D, true>), grid, dim3(kCascadeThreads), smem, st, a);
  else hipLaunchKernelGGL((attention_cascade_kernel<D, false>), grid, dim3(kCascadeThreads), smem, st, a);
}

int launch_attention_cascade(const AttnArgs& a_in, hipStream_t st) {
  AttnArgs a = a_in;
  SD_REQUIRE(a.share && a.split_ws && a.split_cnt, "attention: a cascade launch needs the shared-prefix table and its workspace (sd_model_set_cascade)");
  SD_REQUIRE(!a.kv8, "attention: cascade attention is not available with an fp8 (e4m3) kv dtype");
  SD_REQUIRE(!a.skip_k, "attention: cascade attention is not available with per-row adaptive K");
  CascadePlan pl{};
  if (int rc = attention_cascade_plan(a.n_q_heads, a.n_kv_heads, a.head_dim, a.B, a.M, a.l_max, a.block_table ? static_cast<int>(a.page_shift) : -1, pl))
    return rc;
  SD_REQUIRE(pl.slots <= a.split_slots, "attention: the cascade workspace holds %d partial tiles, this launch needs %d", a.split_slots, pl.slots);
  a.n_split = pl.n_split;
  a.c_split = pl.p_split;
  const dim3 grid(pl.grid_x, pl.grid_y, pl.grid_z);
  switch (a.head_dim) {
    case 32: launch_cascade_d<32>(a, grid, st); break;
    case 64: launch_cascade_d<64>(a, grid, st); break;
    default: launch_cascade_d<128>(a, grid, st); break;
  }
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd

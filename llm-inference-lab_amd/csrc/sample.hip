// Sampled bonus token on the device: temperature -> top-k -> top-p -> one categorical draw.
//
// Replaces sample_bonus_token_from_logits (src/specdec/core/pipeline.py:48-147, do_sample=True),
// which the reference runs on the host per row per step with a full sort over the vocabulary
// (:107) and torch.multinomial on the global generator. Here one 1024-thread workgroup per row:
//
//   1. a lower bound of the k-th largest logit on a 52-bit composite key
//        [32-bit order-preserving value key][20-bit inverted index]
//      (so "value descending, then index ascending" is a total order and ties at the cut are
//      decided the same way everywhere). Fast path: every thread keeps the maximum of the elements
//      it scans (16-byte loads; the row is L2/MALL resident, the lm_head epilogue has just written
//      it); the k-th largest of the 1024 thread maxima (bitonic sort in LDS) cannot exceed the k-th
//      largest element, so everything below it is out. For real logits that leaves ~k..2k
//      candidates. If more than 4096 survive (maxima concentrated in few threads), fall back to a
//      radix select: each pass histograms the next 10-11 key bits of the elements that match the
//      prefix decided so far in LDS, one wave picks the digit holding the k-th element, and the
//      passes stop as soon as that digit's bucket fits the candidate buffer;
//   2. one gather scan of everything at or above the bound, bitonic sort in LDS (<= 4096 keys);
//   3. the k survivors: x/T, exp(x/T - max), nucleus cut on the inclusive cumulative probability
//      (first token always kept), inversion of ONE Philox4x32-10 uniform through the cumulative
//      sums — in float64, sequentially in sorted order, exactly as oracle/sampling_ref.py.
//
// Without top-k and top-p the draw is a Gumbel-max over the whole row (one Philox value per
// element, block argmax): no ordered prefix sum over 128 K probabilities.
// Full-vocabulary nucleus sampling (top_p < 1 without top_k): sample_nucleus_kernel below, rank blocks of 1024.
//
// Per-row parameters (sd_sample_token_rows, sd_row_sampling in include/specdec_hip.h): the three draws are __device__ functions
// over the argument block and an LDS block; sample_rows_kernel reads row b's table entry, normalises it
// (normalise_row_sampling, sample_device.h) and calls the one launch_sample would have launched for those parameters.

#include "engine.h"
#include "sample_device.h"

namespace sd {

struct SampleArgs {
  const void* logits;
  int dtype;               // SD_F32 / SD_BF16 / SD_F16
  int64_t row_stride;      // elements between rows
  int V;
  const int32_t* pos;      // nullable: row of batch entry b = b * rows_per_b + pos[b]
  int rows_per_b;
  const int32_t* active;   // nullable: entries with active[b] == 0 are skipped (no draw consumed)
  float temperature;
  int top_k;
  float top_p;             // >= 1: no nucleus cut
  uint32_t seed_lo, seed_hi;
  uint32_t* draw;          // nullable: per-entry draw counters, read then incremented
  uint32_t draw0;          // draw index when `draw` is NULL
  const int32_t* stream_id;  // nullable: Philox stream of entry b (default b)
  int32_t* out;            // [B]
};

// The three draws of one row, each by one 1024-thread workgroup on an LDS block of its caller: the scalar kernels below call
// them with the launch's parameters, sample_rows_kernel with the row's own.
__device__ __forceinline__ void sample_topk_row(SurvivorLds& L, const SampleArgs& a, int b) {
  const int tid = threadIdx.x;
  if (a.active && a.active[b] == 0) return;
  const int rowi = b * a.rows_per_b + (a.pos ? a.pos[b] : 0);
  const char* row = static_cast<const char*>(a.logits) + static_cast<size_t>(rowi) * a.row_stride * (a.dtype == SD_F32 ? 4 : 2);
  // steps 1-3: the kept set, its weights and their sum (sample_device.h)
  row_survivors(L, row, a.dtype, a.V, min(a.top_k, a.V), a.temperature, a.top_p);
  if (tid == 0) {
    const uint32_t d = a.draw ? a.draw[b] : a.draw0;
    const uint32_t sid = a.stream_id ? static_cast<uint32_t>(a.stream_id[b]) : static_cast<uint32_t>(b);
    const int pick = invert_weights(L.ev, L.n_keep, L.z, philox_uniform(d, sid, kTagCdf, a.seed_lo, a.seed_hi));
    a.out[b] = static_cast<int32_t>(L.sel[pick]);
    if (a.draw) a.draw[b] = a.draw[b] + 1u;
  }
}

// ------------------------------------------------------------------------------
// Full-vocabulary nucleus sampling: top_p < 1 WITHOUT top_k (sample_bonus_token_from_logits with top_k = None,
// src/specdec/core/pipeline.py:105-125: sort the whole row, cumulative softmax, drop a token when the inclusive
// cumulative probability exceeds top_p, the first is always kept). No full sort here: the row is consumed in RANK BLOCKS
// of 1024 — an exact radix select (5 passes over the L2-resident row) finds the composite key of rank 1024 (r+1), the
// elements between it and the previous block's key are gathered and sorted in LDS, and thread 0 continues the cumulative
// sum where the previous block stopped. A peaked distribution (any trained model) ends inside the first block; a flat one
// walks on, 1024 ranks at a time, up to the whole vocabulary. Arithmetic as oracle/sampling_ref.py (float64):
//   v_i = x_i / T, m = max v, e_i = exp(v_i - m),
//   Z   = sum_s ( sum_j e[s + 1024 j] )  — per-slot sums s = 0..1023 (j ascending), then the slots in order,
//   cum += e_i / Z in sorted order; kept while i == 0 or !(cum > top_p); the draw inverts one Philox uniform through
//   the kept weights in sorted order.
// ------------------------------------------------------------------------------
struct NucleusLds {
  uint32_t hist[2048];
  uint64_t sel[kSampleThreads];
  double ev[kSampleThreads];
  uint32_t s_cnt;
  RadixPick s_radix;
  double s_z, s_cum, s_z2, s_u, s_c;
  int s_done, s_keep, s_pick;
  uint64_t s_best;
};

__device__ __forceinline__ void sample_nucleus_row(NucleusLds& N, const SampleArgs& a, int b) {
  uint32_t* const hist = N.hist;
  uint64_t* const sel = N.sel;
  double* const ev = N.ev;
  uint32_t& s_cnt = N.s_cnt;
  RadixPick& s_radix = N.s_radix;
  double &s_z = N.s_z, &s_cum = N.s_cum, &s_z2 = N.s_z2, &s_u = N.s_u, &s_c = N.s_c;
  int &s_done = N.s_done, &s_keep = N.s_keep, &s_pick = N.s_pick;
  uint64_t& s_best = N.s_best;
  const int tid = threadIdx.x, lane = tid & 63;
  if (a.active && a.active[b] == 0) return;
  const int rowi = b * a.rows_per_b + (a.pos ? a.pos[b] : 0);
  const char* row = static_cast<const char*>(a.logits) + static_cast<size_t>(rowi) * a.row_stride * (a.dtype == SD_F32 ? 4 : 2);
  const int V = a.V;
  const double T = static_cast<double>(a.temperature);
  const bool scale = (a.temperature > 0.f) && (a.temperature != 1.0f);
  auto scaled = [&](int i) {
    double v = static_cast<double>(load_logit(row, a.dtype, i));
    return scale ? v / T : v;
  };

  // ---- the top element (largest composite key) and the normaliser
  if (tid == 0) s_best = 0;
  __syncthreads();
  {
    uint64_t best = 0;
    for (int i = tid; i < V; i += kSampleThreads) {
      const uint64_t c = composite_key(load_logit(row, a.dtype, i), i);
      best = c > best ? c : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    if (lane == 0) atomicMax(reinterpret_cast<unsigned long long*>(&s_best), static_cast<unsigned long long>(best));
  }
  __syncthreads();
  const int top_idx = key_index(s_best);
  const double m = scaled(top_idx);
  if (!is_finite_d(m)) {                     // -inf / NaN / +inf on top: the reference falls back to argmax (:129-131)
    if (tid == 0) {
      a.out[b] = top_idx;
      if (a.draw) a.draw[b] = a.draw[b] + 1u;
    }
    return;
  }
  {
    double p = 0.0;
    for (int i = tid; i < V; i += kSampleThreads) {
      double e = exp(scaled(i) - m);
      if (e != e) e = 0.0;
      p += e;
    }
    ev[tid] = p;
  }
  __syncthreads();
  if (tid == 0) {
    double z = 0.0;
    for (int s2 = 0; s2 < kSampleThreads; ++s2) z += ev[s2];
    s_z = z;
    s_cum = 0.0;
    s_z2 = 0.0;
    s_keep = 0;
    s_done = 0;
  }
  __syncthreads();

  // block r: the elements of ranks (1024 r, min(1024 (r+1), V)], sorted descending into sel[] / ev[]; returns their count
  auto load_block = [&](int r, uint64_t upper_excl, uint64_t& thr_out) -> int {
    const int k_hi = min((r + 1) * kSampleThreads, V);
    int decided;   // 52: stop_bucket = 0 runs every pass, the prefix is the exact composite key of rank k_hi
    const uint64_t thr = radix_select(row, a.dtype, V, k_hi, 0, hist, s_radix, decided);
    thr_out = thr;
    if (tid == 0) s_cnt = 0;
    sel[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += kSampleThreads) {
      const uint64_t c = composite_key(load_logit(row, a.dtype, i), i);
      if (c >= thr && c < upper_excl) {
        const uint32_t slot = atomicAdd(&s_cnt, 1u);
        if (slot < static_cast<uint32_t>(kSampleThreads)) sel[slot] = c + 1;
      }
    }
    __syncthreads();
    sort_desc(sel, kSampleThreads);   // 0 = empty, last
    const int n = k_hi - r * kSampleThreads;
    if (tid < n) {
      const int idx = key_index(sel[tid] - 1);
      double e = exp(scaled(idx) - m);
      if (e != e) e = 0.0;
      ev[tid] = e;
      sel[tid] = static_cast<uint64_t>(idx);
    }
    __syncthreads();
    return n;
  };

  // ---- phase A: how many tokens the nucleus keeps, and their total weight
  const double tp = static_cast<double>(a.top_p);
  const int n_blocks = (V + kSampleThreads - 1) / kSampleThreads;
  uint64_t upper = ~0ull;
  int blocks_used = 0;
  for (int r = 0; r < n_blocks; ++r) {
    uint64_t thr;
    const int n = load_block(r, upper, thr);
    upper = thr;
    blocks_used = r + 1;
    if (tid == 0) {
      double cum = s_cum, z2 = s_z2;
      int keep = s_keep, done = 0;
      for (int i = 0; i < n; ++i) {
        cum += ev[i] / s_z;
        if ((r == 0 && i == 0) || !(cum > tp)) {
          ++keep;
          z2 += ev[i];
        } else {
          done = 1;
          break;
        }
      }
      s_cum = cum;
      s_z2 = z2;
      s_keep = keep;
      s_done = done;
    }
    __syncthreads();
    if (s_done) break;
  }
  // ---- phase B: invert one uniform through the kept weights, in sorted order
  if (tid == 0) {
    const uint32_t d = a.draw ? a.draw[b] : a.draw0;
    const uint32_t sid = a.stream_id ? static_cast<uint32_t>(a.stream_id[b]) : static_cast<uint32_t>(b);
    s_u = philox_uniform(d, sid, kTagCdf, a.seed_lo, a.seed_hi);
    s_c = 0.0;
    s_pick = -1;
  }
  __syncthreads();
  const int n_keep = s_keep;
  if (blocks_used == 1) {              // the common case: block 0 is still in LDS
    if (tid == 0) s_pick = static_cast<int>(sel[invert_weights(ev, n_keep, s_z2, s_u)]);
  } else {
    const double target = s_u * s_z2;  // invert_weights, continued from block to block with the running sum in s_c
    upper = ~0ull;
    int last_tok = top_idx;
    for (int r = 0; r * kSampleThreads < n_keep; ++r) {
      uint64_t thr;
      const int n = load_block(r, upper, thr);
      upper = thr;
      const int lim = min(n, n_keep - r * kSampleThreads);
      if (tid == 0) {
        double c = s_c;
        for (int i = 0; i < lim; ++i) {
          c += ev[i];
          if (target < c) { s_pick = static_cast<int>(sel[i]); break; }
        }
        s_c = c;
      }
      last_tok = static_cast<int>(sel[lim - 1]);   // (every thread reads the same LDS word)
      __syncthreads();
      if (s_pick >= 0) break;
    }
    if (tid == 0 && s_pick < 0) s_pick = last_tok;  // target == total weight (rounding): the last kept token
  }
  __syncthreads();
  if (tid == 0) {
    a.out[b] = s_pick;
    if (a.draw) a.draw[b] = a.draw[b] + 1u;
  }
}

struct GumbelLds {
  double sv[kSampleThreads / kWave];
  int si[kSampleThreads / kWave];
};

__device__ __forceinline__ void sample_gumbel_row(GumbelLds& G, const SampleArgs& a, int b) {
  double* const sv = G.sv;
  int* const si = G.si;
  const int tid = threadIdx.x;
  if (a.active && a.active[b] == 0) return;
  const int rowi = b * a.rows_per_b + (a.pos ? a.pos[b] : 0);
  const char* row = static_cast<const char*>(a.logits) + static_cast<size_t>(rowi) * a.row_stride * (a.dtype == SD_F32 ? 4 : 2);
  const double T = static_cast<double>(a.temperature);
  const bool scale = (a.temperature > 0.f) && (a.temperature != 1.0f);
  const uint32_t d = a.draw ? a.draw[b] : a.draw0;
  const uint32_t sid = a.stream_id ? static_cast<uint32_t>(a.stream_id[b]) : static_cast<uint32_t>(b);
  double bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < a.V; i += kSampleThreads) {
    double v = static_cast<double>(load_logit(row, a.dtype, i));
    if (scale) v = v / T;
    const double s = v + gumbel_noise(d, sid, i, a.seed_lo, a.seed_hi);
    if (better_d(s, i, bv, bi)) { bv = s; bi = i; }
  }
  block_arg_best<kSampleThreads / kWave, double, better_d>(bv, bi, sv, si);
  if (tid == 0) {
    a.out[b] = bi;
    if (a.draw) a.draw[b] = a.draw[b] + 1u;
  }
}

__global__ __launch_bounds__(kSampleThreads) void sample_topk_kernel(const SampleArgs a) {
  __shared__ SurvivorLds L;
  sample_topk_row(L, a, blockIdx.x);
}

__global__ __launch_bounds__(kSampleThreads) void sample_nucleus_kernel(const SampleArgs a) {
  __shared__ NucleusLds N;
  sample_nucleus_row(N, a, blockIdx.x);
}

__global__ __launch_bounds__(kSampleThreads) void sample_gumbel_kernel(const SampleArgs a) {
  __shared__ GumbelLds G;
  sample_gumbel_row(G, a, blockIdx.x);
}

// Per-row parameters (sd_sample_token_rows): row b's workgroup normalises table[b] and takes, workgroup-uniformly, the path
// launch_sample picks for those parameters. Only one path runs per workgroup: the three LDS blocks overlay each other.
union SampleRowsLds {
  SurvivorLds topk;
  NucleusLds nucleus;
  GumbelLds gumbel;
};

__global__ __launch_bounds__(kSampleThreads) void sample_rows_kernel(const SampleArgs a0, const sd_row_sampling* table) {
  __shared__ SampleRowsLds U;
  const int b = blockIdx.x;
  if (a0.active && a0.active[b] == 0) return;
  const sd_row_sampling e = normalise_row_sampling(table, b, a0.V, false);
  SampleArgs a = a0;
  a.temperature = e.temperature;
  a.top_k = e.top_k;
  a.top_p = e.top_p;
  a.seed_lo = e.seed_lo;
  a.seed_hi = e.seed_hi;
  if (a.top_k > 0) sample_topk_row(U.topk, a, b);
  else if (a.top_p < 1.0f) sample_nucleus_row(U.nucleus, a, b);
  else sample_gumbel_row(U.gumbel, a, b);
}

// (the fields in declaration order, the seed split into the two Philox key words)
static SampleArgs sample_args(const void* logits, int dtype, int64_t row_stride, int V, const int32_t* pos, int rows_per_b,
                              const int32_t* active, const DrawSpec& d, int32_t* out) {
  return SampleArgs{logits, dtype, row_stride, V, pos, rows_per_b, active, d.temperature, d.top_k, d.top_p, seed_lo32(d.seed),
                    seed_hi32(d.seed), d.draw, d.draw0, d.stream_id, out};
}

// table: per-row parameters (the scalar ones of `a` are ignored), else null
int launch_sample(const SampleArgs& a, int B, hipStream_t st, const sd_row_sampling* table = nullptr) {
  SD_REQUIRE(a.logits && a.out, "sample: NULL logits/out");
  SD_REQUIRE(a.dtype == SD_F32 || a.dtype == SD_BF16 || a.dtype == SD_F16, "sample: logits dtype %d", a.dtype);
  SD_REQUIRE(B >= 1 && B <= 65535 && a.V >= 1 && a.V <= (1 << kIdxBits), "sample: B=%d V=%d out of range", B, a.V);
  SD_REQUIRE(a.rows_per_b >= 1, "sample: rows_per_b=%d", a.rows_per_b);
  if (table) {
    SD_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "sample: the row table must be 16-byte aligned");
    hipLaunchKernelGGL(sample_rows_kernel, dim3(B), dim3(kSampleThreads), 0, st, a, table);
    SD_LAUNCH_CHECK();
    return 0;
  }
  SD_REQUIRE(a.temperature == a.temperature, "sample: temperature is NaN");
  if (a.top_k > 0) {
    SD_REQUIRE((a.top_k < a.V ? a.top_k : a.V) <= kSampleMaxK, "sample: top_k=%d > %d is not supported", a.top_k, kSampleMaxK);
    hipLaunchKernelGGL(sample_topk_kernel, dim3(B), dim3(kSampleThreads), 0, st, a);
  } else if (a.top_p < 1.0f) {
    hipLaunchKernelGGL(sample_nucleus_kernel, dim3(B), dim3(kSampleThreads), 0, st, a);
  } else {
    hipLaunchKernelGGL(sample_gumbel_kernel, dim3(B), dim3(kSampleThreads), 0, st, a);
  }
  SD_LAUNCH_CHECK();
  return 0;
}

// the step's draw: entry b samples from row b*(K+1) + accept_len[b] of the verify logits
int launch_sample_step(const SpecState& s, const void* logits, int V, const DrawSpec& d, hipStream_t st) {
  return launch_sample(sample_args(logits, SD_BF16, V, V, s.accept_len, s.K + 1, s.active, d, s.sampled), s.B, st, d.table);
}

}  // namespace sd

using namespace sd;

extern "C" int sd_sample_token(const void* logits, int logits_dtype, int64_t row_stride, int B, int V,
                               const int32_t* pos, int rows_per_b, const int32_t* active, float temperature,
                               int top_k, float top_p, uint64_t seed, uint32_t* draw_counters, uint32_t draw0,
                               const int32_t* stream_id, int32_t* out_ids, void* stream) {
  clear_error();
  const DrawSpec d{temperature, top_k, top_p, seed, draw_counters, draw0, stream_id};
  return launch_sample(sample_args(logits, logits_dtype, row_stride, V, pos, rows_per_b, active, d, out_ids), B,
                       static_cast<hipStream_t>(stream));
}

extern "C" size_t sd_row_sampling_bytes(void) { return sizeof(sd_row_sampling); }

extern "C" int sd_sample_token_rows(const void* logits, int logits_dtype, int64_t row_stride, int B, int V, const int32_t* pos,
                                    int rows_per_b, const int32_t* active, const sd_row_sampling* table, uint32_t* draw_counters,
                                    uint32_t draw0, const int32_t* stream_id, int32_t* out_ids, void* stream) {
  clear_error();
  SD_REQUIRE(table, "sample_token_rows: NULL table");
  SD_REQUIRE(B >= 1, "sample_token_rows: B=%d", B);
  SD_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "sample_token_rows: the row table must be 16-byte aligned");
  const DrawSpec d{1.0f, 0, 1.0f, 0, draw_counters, draw0, stream_id, table};   // the scalars are not in the launch
  return launch_sample(sample_args(logits, logits_dtype, row_stride, V, pos, rows_per_b, active, d, out_ids), B,
                       static_cast<hipStream_t>(stream), table);
}

// Per-token log-probs and top-N alternatives of a logits row (sd_token_logprobs, sd_specdec_set_logprobs): what the row — the
// distribution a token was checked against or drawn from, at temperature 1 — says about the token that was emitted.
//
//   logprob(t) = (x_t - m) - log S,  m = max_v x_v,  S = sum_v e^{x_v - m} over the STORED values (bf16 / f16 / f32)
//   rank(t)    = #{v : x_v > x_t, or x_v == x_t and v < t}: the ties of the argmax kernels (argmax_better, common.h), so rank 0 is
//                "t is the row's argmax"
//   top N      the N = min(top_n, V) largest entries in composite-key order (value descending, index ascending): ids and log-probs
//
// ONE LAUNCH, one 1024-thread workgroup per row, structured as typical_row_kernel (csrc/typical_accept.hip):
//   pass 1     the (m, S) stream and the rank, in one walk over the row (the walkers of sample_device.h)
//   top N      radix_select for the N-th composite key (the passes stop once the digit's bucket holds <= kLpBucket keys), gather of
//              the keys at or above the decided prefix (fewer than N above it, <= kLpBucket inside it: they fit kLpSort), sort_desc,
//              the first N. Composite keys are unique: the result does not depend on where the passes stopped.
//
// THE STREAM is typical_accept.hip's at T = 1 without the entropy term: a thread folds its elements into a running (m, S), a new
// maximum m' rescaling S by e^{m - m'}; partials merge the same way. An element at -inf is skipped (it adds exactly 0), a partial
// that has seen nothing finite is the identity of the merge. All fp32; every term of S is > 0 and S >= 1.
//
// ORDER. A thread's elements are fixed by V and the row's alignment; the wave merges on the xor tree and lane 0's result is taken;
// thread 0 merges the 16 wave partials in wave order. The selection's LDS atomics are integer counts and slot numbers whose effect
// the sort removes. Bit-identical run to run and under graph replay. No global atomics, no waiting, no allocation.
//
// EDGES. x_t = -inf: logprob -inf, rank by the formula. Fewer than N finite entries: the rest follow in key order with log-prob
// -inf. A row with no finite element, and a token id outside [0, V) (never read): logprob NaN, rank -1, top ids -1 (log-probs
// NaN) — the "no record" value, which the step also writes for every position that emitted nothing.
//
// Compiled with the flags of every other file (build.py): no per-file flag. expf / logf are the device library's, as in
// typical_accept.hip, and tests/logprobs_ref.py carries their 1-ulp terms.

#include "engine.h"
#include "sample_device.h"

namespace sd {

constexpr int kLpMaxTop = 20;
constexpr int kLpBucket = 44;   // (kLpMaxTop - 1) + kLpBucket <= kLpSort
constexpr int kLpSort = 64;
constexpr int kLpWaves = kSampleThreads / kWave;

struct LogprobPart {
  float m, S;   // maximum (-inf: nothing finite seen), sum e^{x - m}
};

__device__ __forceinline__ LogprobPart logprob_merge(const LogprobPart& a, const LogprobPart& b) {
  if (b.m == -INFINITY) return a;
  if (a.m == -INFINITY) return b;
  const bool a_top = a.m >= b.m;
  const LogprobPart& hi = a_top ? a : b;
  const LogprobPart& lo = a_top ? b : a;
  return LogprobPart{hi.m, hi.S + lo.S * expf(lo.m - hi.m)};
}

struct LogprobLds {
  uint64_t sel[kLpSort];
  uint32_t hist[2048];
  float m[kLpWaves], S[kLpWaves];
  int rank[kLpWaves];
  float row_m, row_logS;
  uint32_t cnt;
  RadixPick pick;
};

// where one row's results go: the op's four arrays, or the words of the step's pinned block (ids null)
struct LogprobOut {
  float* logprob;
  int32_t* rank;
  int32_t* top_ids;     // [N]
  float* top_logprob;   // [N]
};

__device__ __forceinline__ float nan_f() { return __uint_as_float(0x7fc00000u); }

// the "no record" value, by one thread
__device__ __forceinline__ void logprob_none(const LogprobOut& o, int N) {
  *o.logprob = nan_f();
  *o.rank = -1;
  for (int j = 0; j < N; ++j) {
    o.top_ids[j] = -1;
    o.top_logprob[j] = nan_f();
  }
}

// Every thread of the workgroup calls it (barriers inside); N = min(top_n, V) in 0..kLpMaxTop.
__device__ __forceinline__ void token_logprob_row(LogprobLds& L, const void* row, int dtype, int V, int t, int N, const LogprobOut& o) {
  const int tid = threadIdx.x;
  const bool t_ok = t >= 0 && t < V;   // an id outside the vocabulary is never read
  const float xt = t_ok ? load_logit(row, dtype, t) : -INFINITY;

  LogprobPart p{-INFINITY, 0.f};
  int rank = 0;
  for_each_logit(row, dtype, V, tid, [&](float x, int v) {
    rank += argmax_better(x, v, xt, t) ? 1 : 0;
    if (x == -INFINITY) return;
    if (x <= p.m) {
      p.S += expf(x - p.m);
    } else if (p.m == -INFINITY) {
      p = LogprobPart{x, 1.f};
    } else {          // a new maximum
      p.S = p.S * expf(p.m - x) + 1.f;
      p.m = x;
    }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const LogprobPart q{__shfl_xor(p.m, off, 64), __shfl_xor(p.S, off, 64)};
    p = logprob_merge(p, q);
    rank += __shfl_xor(rank, off, 64);
  }
  if ((tid & (kWave - 1)) == 0) {
    const int w = tid / kWave;
    L.m[w] = p.m; L.S[w] = p.S;
    L.rank[w] = rank;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kLpWaves; ++w) {
      p = logprob_merge(p, LogprobPart{L.m[w], L.S[w]});
      rank += L.rank[w];
    }
    L.row_m = p.m;
    L.row_logS = logf(p.S);
    if (p.m == -INFINITY || !t_ok) {
      logprob_none(o, N);
    } else {
      *o.logprob = (xt - p.m) - L.row_logS;
      *o.rank = rank;
    }
  }
  __syncthreads();
  const float m = L.row_m, logS = L.row_logS;
  if (N == 0 || m == -INFINITY || !t_ok) return;   // (workgroup-uniform)

  int decided;
  const uint64_t prefix = radix_select(row, dtype, V, N, kLpBucket, L.hist, L.pick, decided);
  const int shift = 52 - decided;
  if (tid == 0) L.cnt = 0;
  if (tid < kLpSort) L.sel[tid] = 0;
  __syncthreads();
  for_each_logit(row, dtype, V, tid, [&](float x, int i) {
    const uint64_t c = composite_key(x, i);
    if ((c >> shift) >= prefix) {
      const uint32_t slot = atomicAdd(&L.cnt, 1u);
      if (slot < static_cast<uint32_t>(kLpSort)) L.sel[slot] = c + 1;   // 0 stays "empty" and sorts last
    }
  });
  __syncthreads();
  sort_desc(L.sel, kLpSort);
  if (tid < N) {
    const int id = key_index(L.sel[tid] - 1);
    o.top_ids[tid] = id;
    o.top_logprob[tid] = (load_logit(row, dtype, id) - m) - logS;   // -inf for an entry at -inf
  }
}

__device__ __forceinline__ const char* logprob_row_ptr(const void* logits, int dtype, int64_t row_stride, size_t r) {
  return static_cast<const char*>(logits) + r * static_cast<size_t>(row_stride) * (dtype == SD_F32 ? 4 : 2);
}

struct TokenLogprobArgs {
  const void* logits;         // [R] rows of V elements of `dtype`, row_stride elements apart
  int dtype;
  int64_t row_stride;
  int V, N;
  const int32_t* token_ids;   // [R]
  float* out_logprob;         // [R]
  int32_t* out_rank;          // [R]
  int32_t* out_top_ids;       // [R][N]
  float* out_top_logprob;     // [R][N]
};

__global__ __launch_bounds__(kSampleThreads) void token_logprobs_kernel(const TokenLogprobArgs a) {
  __shared__ LogprobLds L;
  const size_t r = blockIdx.x;
  const LogprobOut o{a.out_logprob + r, a.out_rank + r, a.out_top_ids + r * a.N, a.out_top_logprob + r * a.N};
  token_logprob_row(L, logprob_row_ptr(a.logits, a.dtype, a.row_stride, r), a.dtype, a.V, a.token_ids[r], a.N, o);
}

// The stage of the step: workgroup (i, b) describes new_tok[b][i] by row (b, i) of the verify pass — the target's distribution after
// d_1..d_i, which that token was checked against or drawn from in every select mode — iff the row is active and i < n_new[b]; every
// other workgroup writes the "no record" value, so a record of two launches ago is never taken for this step's. The words go to the
// pinned block's slot of the step counter's parity, read BEFORE pack_record (the next launch) advances it: the slot the step record
// of the same launch goes to.
struct StepLogprobArgs {
  const void* logits;         // [B][K+1][V] bf16
  int V, N, K;
  const int32_t* new_tok;     // [B][K+1]
  const int32_t* n_new;       // [B]
  const int32_t* active;      // [B]
  const int32_t* step_counter;
  int32_t* host_words;        // pinned: [2][B][K+1][2 + 2N]
};

__global__ __launch_bounds__(kSampleThreads) void step_logprobs_kernel(const StepLogprobArgs a) {
  __shared__ LogprobLds L;
  const int i = blockIdx.x, b = blockIdx.y, M = a.K + 1, W = 2 + 2 * a.N, B = gridDim.y;
  const int slot = *a.step_counter & 1;
  const size_t r = static_cast<size_t>(b) * M + i;
  int32_t* const w = a.host_words + (static_cast<size_t>(slot) * B * M + r) * W;
  const LogprobOut o{reinterpret_cast<float*>(w), w + 1, w + 2, reinterpret_cast<float*>(w + 2 + a.N)};
  if (!a.active[b] || i >= a.n_new[b]) {   // (workgroup-uniform)
    if (threadIdx.x == 0) logprob_none(o, a.N);
    return;
  }
  token_logprob_row(L, logprob_row_ptr(a.logits, SD_BF16, a.V, r), SD_BF16, a.V, a.new_tok[r], a.N, o);
}

// Every check of the row pass in one place: the stand-alone op and the step setter both go through it. 0 = ok.
int check_logprob_params(const char* who, int V, int top_n) {
  SD_REQUIRE(V >= 1, "%s: V=%d", who, V);
  SD_REQUIRE(V <= (1 << kIdxBits), "%s: V=%d above the %d ids of a composite key", who, V, 1 << kIdxBits);
  SD_REQUIRE(top_n >= 0 && top_n <= kLpMaxTop, "%s: top_n %d outside 0..%d", who, top_n, kLpMaxTop);
  return 0;
}

int logprob_words(int V, int top_n) { return 2 + 2 * (top_n < V ? top_n : V); }

// the parameters are checked (check_logprob_params) by the caller
int launch_step_logprobs(const SpecState& s, const void* logits, int V, int top_n, const int32_t* step_counter, int32_t* host_words,
                         hipStream_t st) {
  SD_REQUIRE(logits && step_counter && host_words, "step_logprobs: NULL buffer");
  const StepLogprobArgs a{logits, V, top_n < V ? top_n : V, s.K, s.new_tok, s.n_new, s.active, step_counter, host_words};
  hipLaunchKernelGGL(step_logprobs_kernel, dim3(s.K + 1, s.B), dim3(kSampleThreads), 0, st, a);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd

using namespace sd;

extern "C" int sd_token_logprobs(const void* logits, int logits_dtype, int64_t row_stride, int R, int V, const int32_t* token_ids,
                                 int top_n, float* out_logprob, int32_t* out_rank, int32_t* out_top_ids, float* out_top_logprob,
                                 void* stream) {
  clear_error();
  SD_REQUIRE(logits && token_ids && out_logprob && out_rank, "token_logprobs: NULL argument");
  SD_REQUIRE(logits_dtype == SD_F32 || logits_dtype == SD_BF16 || logits_dtype == SD_F16, "token_logprobs: logits dtype %d", logits_dtype);
  SD_REQUIRE(R >= 1, "token_logprobs: R=%d", R);
  if (int rc = check_logprob_params("token_logprobs", V, top_n)) return rc;
  SD_REQUIRE(top_n == 0 || (out_top_ids && out_top_logprob), "token_logprobs: NULL top-N outputs with top_n %d", top_n);
  SD_REQUIRE(row_stride >= V, "token_logprobs: row_stride %lld below V (%d)", static_cast<long long>(row_stride), V);
  SD_REQUIRE(((reinterpret_cast<uintptr_t>(out_logprob) | reinterpret_cast<uintptr_t>(out_rank) | reinterpret_cast<uintptr_t>(out_top_ids) |
               reinterpret_cast<uintptr_t>(out_top_logprob) | reinterpret_cast<uintptr_t>(token_ids)) & 3) == 0,
             "token_logprobs: misaligned ids / outputs");
  const TokenLogprobArgs a{logits, logits_dtype, row_stride, V, top_n < V ? top_n : V, token_ids, out_logprob, out_rank, out_top_ids,
                           out_top_logprob};
  hipLaunchKernelGGL(token_logprobs_kernel, dim3(R), dim3(kSampleThreads), 0, static_cast<hipStream_t>(stream), a);
  SD_LAUNCH_CHECK();
  return 0;
}

// The draft's confidence in its own token, and the decision the confidence-gated step makes from it between two draft forwards
// (sd_draft_confidence, sd_specdec_set_draft_confidence; the contract is in include/specdec_hip.h).
//
//   c = 1 / sum_v exp(x_v - max_v x_v)     over the STORED values of a logits row: the temperature-1 softmax probability of the
//                                          row's largest value, which is the value the fused argmax picked its token at
//
// THE STREAM is typical_row_kernel's (csrc/typical_accept.hip) without W and at T = 1, where its one division is exact and
// dropped: a thread folds its elements into (m, S), a new maximum m' rescaling S by e^{m - m'}; partials merge the same way; an
// element at -inf is skipped (it adds exactly 0) and a partial that has seen nothing finite is the identity of the merge. A NaN
// element makes S NaN for good (every later rescale and merge multiplies or adds it), +inf ends as m = +inf: both, and a row of
// -inf alone, give c = NaN. All fp32; every term of S is > 0.
//
// ORDER. A thread's elements are fixed by V and the row's alignment (the walkers of sample_device.h); the wave merges on the xor
// tree, thread 0 merges the 16 wave partials in wave order. Bit-identical run to run. No atomics, no waiting, no allocation.
//
// TWO KERNELS over the one device function: draft_confidence_kernel (the op: c of caller rows) and confidence_judge_kernel (the
// step: c of the row draft forward i has just stored, then the row's stop / continue decision).

#include "engine.h"
#include "sample_device.h"

namespace sd {

struct ConfPart {
  float m, S;   // maximum (-inf: nothing finite seen), sum e^{x - m}
};

__device__ __forceinline__ ConfPart conf_merge(const ConfPart& a, const ConfPart& b) {
  if (b.m == -INFINITY) return a;
  if (a.m == -INFINITY) return b;
  const bool a_top = a.m >= b.m;
  const ConfPart& hi = a_top ? a : b;
  const ConfPart& lo = a_top ? b : a;
  return ConfPart{hi.m, hi.S + lo.S * expf(lo.m - hi.m)};
}

struct ConfLds {
  float m[kSampleThreads / kWave], S[kSampleThreads / kWave];
};

// The confidence of one row, by every thread of a 1024-thread workgroup (one barrier inside); the result is valid in thread 0.
__device__ __forceinline__ float row_confidence(ConfLds& L, const void* row, int dtype, int V, int tid) {
  ConfPart p{-INFINITY, 0.f};
  for_each_logit(row, dtype, V, tid, [&](float x, int) {
    if (x == -INFINITY) return;
    if (x <= p.m) {
      p.S += expf(x - p.m);
    } else if (p.m == -INFINITY) {
      p = ConfPart{x, 1.f};
    } else {          // a new maximum (or a NaN / +inf element, which poisons the row)
      p.S = p.S * expf(p.m - x) + 1.f;
      p.m = x;
    }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) p = conf_merge(p, ConfPart{__shfl_xor(p.m, off, 64), __shfl_xor(p.S, off, 64)});
  if ((tid & (kWave - 1)) == 0) {
    L.m[tid / kWave] = p.m;
    L.S[tid / kWave] = p.S;
  }
  __syncthreads();
  if (tid != 0) return 0.f;
  for (int w = 1; w < kSampleThreads / kWave; ++w) p = conf_merge(p, ConfPart{L.m[w], L.S[w]});
  const bool finite_max = p.m - p.m == 0.f;   // not -inf (nothing finite), +inf or NaN
  return finite_max ? 1.0f / p.S : __uint_as_float(0x7fc00000u);   // (a NaN element under a finite maximum left S = NaN)
}

__global__ __launch_bounds__(kSampleThreads) void draft_confidence_kernel(const void* logits, int dtype, int64_t row_stride, int V, float* conf) {
  __shared__ ConfLds L;
  const int b = blockIdx.x;
  const char* row = static_cast<const char*>(logits) + static_cast<size_t>(b) * static_cast<size_t>(row_stride) * (dtype == SD_F32 ? 4 : 2);
  const float c = row_confidence(L, row, dtype, V, threadIdx.x);
  if (threadIdx.x == 0) conf[b] = c;
}

struct JudgeArgs {
  const uint16_t* rows;      // row b at rows + b * row_stride
  long long row_stride;
  int V, i, K;
  float tau;
  const int32_t* active;     // [B]
  int32_t* k_row;            // [B]: K while the row has not stopped in this step
  int32_t* gate_next;        // the word draft forward i + 1 is gated on
  float* conf_out;           // nullable [B][K]
  int first;                 // the step's first judgement: the other slots of conf_out's row are NaN until a later one writes them
  const int32_t* skip_k;     // the word forward i itself was gated on (null: it always runs)
  int skip_i;
};

// One workgroup per row. Rows decide alone: a row that stops writes its own k_row, every row that continues stores the SAME
// constant into the next forward's word, so whichever store lands last the word reads i + 2.
__global__ __launch_bounds__(kSampleThreads) void confidence_judge_kernel(const JudgeArgs a) {
  SD_SKIP_IF_INACTIVE(a.skip_k, a.skip_i);   // forward i did not run: no row is still drafting, and the next word stays shut
  __shared__ ConfLds L;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float c = row_confidence(L, a.rows + static_cast<size_t>(b) * static_cast<size_t>(a.row_stride), SD_BF16, a.V, tid);
  if (tid != 0) return;
  if (a.conf_out) {
    float* out = a.conf_out + static_cast<size_t>(b) * a.K;
    if (a.first)
      for (int j = 0; j < a.K; ++j)
        if (j != a.i) out[j] = __uint_as_float(0x7fc00000u);
    out[a.i] = c;
  }
  if (a.active[b] == 0 || a.k_row[b] < a.K) return;   // a row that does not advance keeps no forward alive; a stopped row rides along
  if (c >= a.tau) *a.gate_next = a.i + 2;             // (a NaN compares false: it stops the row)
  else a.k_row[b] = a.i + 1;
}

int launch_confidence_judge(const SpecState& s, const uint16_t* rows, long long row_stride, int V, int i, const ConfRule& r, bool first,
                            const int32_t* skip_k, int skip_i, hipStream_t st) {
  SD_REQUIRE(rows && s.conf && s.conf_gate, "confidence_judge: the mode is not set");
  SD_REQUIRE(i >= r.min_k - 1 && i <= s.K - 2 && row_stride >= V, "confidence_judge: forward %d of K=%d (min_k %d), stride %lld < V=%d", i, s.K,
             r.min_k, row_stride, V);
  const JudgeArgs a{rows, row_stride, V, i, s.K, r.tau, s.active, s.k_row, s.conf_gate + i + 1, r.conf_out, first ? 1 : 0, skip_k, skip_i};
  hipLaunchKernelGGL(confidence_judge_kernel, dim3(s.B), dim3(kSampleThreads), 0, st, a);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd

using namespace sd;

extern "C" int sd_draft_confidence(const void* logits, int logits_dtype, int64_t row_stride, int B, int V, float* conf, void* stream) {
  clear_error();
  SD_REQUIRE(logits && conf, "draft_confidence: NULL argument");
  SD_REQUIRE(logits_dtype == SD_F32 || logits_dtype == SD_BF16 || logits_dtype == SD_F16, "draft_confidence: logits dtype %d", logits_dtype);
  SD_REQUIRE(B >= 1 && B <= 65535, "draft_confidence: B=%d out of range 1..65535", B);
  SD_REQUIRE(V >= 1, "draft_confidence: V=%d", V);
  SD_REQUIRE(row_stride >= V, "draft_confidence: row_stride %lld below V (%d)", static_cast<long long>(row_stride), V);
  SD_REQUIRE((reinterpret_cast<uintptr_t>(logits) & (dtype_size(logits_dtype) - 1)) == 0 && (reinterpret_cast<uintptr_t>(conf) & 3) == 0,
             "draft_confidence: misaligned logits / conf");
  hipLaunchKernelGGL(draft_confidence_kernel, dim3(B), dim3(kSampleThreads), 0, static_cast<hipStream_t>(stream), logits, logits_dtype, row_stride, V,
                     conf);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t sd_specdec_draft_confidence_bytes(int B, int V) {
  if (B <= 0 || V <= 0) return 0;
  return static_cast<size_t>(B) * 2 * V * 2;   // [B][2][V] bf16: the two positions of draft forward 0; later forwards store [B][1][V]
}

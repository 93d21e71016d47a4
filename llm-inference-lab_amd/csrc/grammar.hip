// Grammar-constrained decoding inside the step: token automata. Restated on the CPU in tests/grammar_ref.py; the contract is
// written out at sd_logit_process_fsm in include/specdec_hip.h, the compiler (regular expressions, closed answer lists) is
// specdec_hip/grammar.py.
//
// Tables, caller-owned device memory:
//   next  : uint16 [S][V], the automaton over TOKENS: next[s][v] = state after token v in state s, 0xFFFF = v is not allowed in s.
//   allow : uint32 [S][ceil(V / 32)], bit v % 32 of word v / 32 = next[s][v] != 0xFFFF, pad bits 0. Built here from `next`
//           (fsm_build_masks_kernel), so there is one source of truth.
//   state : int32 [B], a row's state between steps: -1 = unconstrained, 0..S-1, anything else = DEAD (only eos is allowed;
//           the kernels keep DEAD as 0xFFFF). A token outside [0, V) or one the state does not allow leads to DEAD; DEAD stays.
//
// The mask itself is one more line of the logit processors' transform and lives in their kernel (csrc/logit_proc.hip,
// logit_process_kernel<true>): no launch is added to the step. Where a launch finds the state of its position is written at
// lp_fsm_state there: the draft forwards' launches chain through a position table, one dependent lookup each; the verify
// launch reads that table and does the one lookup its row is ahead of it. No spin-wait, no atomics, no grid barrier.
//
// Here: the mask builder (a wave ballots 64 entries into two words; a row is split over ceil(V / 4096) workgroups as the
// processors split theirs), the advance after the accept stage (one lane per row walks its emitted tokens, as
// logit_counts_add_kernel does), and the C entry points.

#pragma clang fp contract(off)

#include "engine.h"

namespace sd {

constexpr int kFsmThreads = 256;
constexpr int kFsmChunk = 4096;   // entries of a table row per workgroup

size_t fsm_mask_bytes(int S, int V) {
  if (S <= 0 || V <= 0) return 0;
  return (static_cast<size_t>(S) * ((V + 31) / 32) * sizeof(uint32_t) + 15) / 16 * 16;
}

__global__ __launch_bounds__(kFsmThreads) void fsm_build_masks_kernel(const uint16_t* next, int V, uint32_t* allow) {
  const int s = blockIdx.y, tid = threadIdx.x, W = (V + 31) >> 5;
  const uint16_t* row = next + static_cast<size_t>(s) * V;
  uint32_t* out = allow + static_cast<size_t>(s) * W;
  const int base = blockIdx.x * kFsmChunk;
  for (int it = 0; it < kFsmChunk / kFsmThreads; ++it) {   // (uniform trip count: every lane reaches every ballot)
    const int v = base + it * kFsmThreads + tid;
    const bool ok = v < V && row[v] != 0xFFFFu;
    const unsigned long long m = __ballot(ok);
    if ((tid & (kWave - 1)) == 0) {   // v is a multiple of 64 here: words v / 32 and v / 32 + 1, where the row has them
      const int w = v >> 5;
      if (w < W) out[w] = static_cast<uint32_t>(m);
      if (w + 1 < W) out[w + 1] = static_cast<uint32_t>(m >> 32);
    }
  }
}

int launch_fsm_build_masks(const uint16_t* next, int S, int V, uint32_t* allow, size_t allow_bytes, hipStream_t st) {
  SD_REQUIRE(next && allow, "fsm_build_masks: NULL table");
  SD_REQUIRE(S >= 1 && S <= kFsmMaxStates && V >= 1, "fsm_build_masks: S=%d V=%d (S in 1..%d)", S, V, kFsmMaxStates);
  SD_REQUIRE(allow_bytes >= fsm_mask_bytes(S, V), "fsm_build_masks: mask table %zu B < %zu B", allow_bytes, fsm_mask_bytes(S, V));
  SD_REQUIRE(((reinterpret_cast<uintptr_t>(next) | reinterpret_cast<uintptr_t>(allow)) & 15) == 0,
             "fsm_build_masks: tables must be 16-byte aligned");
  hipLaunchKernelGGL(fsm_build_masks_kernel, dim3((V + kFsmChunk - 1) / kFsmChunk, S), dim3(kFsmThreads), 0, st, next, V, allow);
  SD_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(kWave) void fsm_advance_kernel(const uint16_t* next, int S, int V, int32_t* fsm_state, int B,
                                                            const int32_t* tokens, int tok_stride, const int32_t* n_new, int max_new,
                                                            const int32_t* active) {
  const int b = blockIdx.x * kWave + threadIdx.x;
  if (b >= B || (active && active[b] == 0)) return;
  int s = fsm_state[b];
  if (s < 0) return;
  if (s >= S) s = kFsmDead;
  int n = n_new[b];
  n = n < 0 ? 0 : (n > max_new ? max_new : n);
  for (int j = 0; j < n; ++j) s = fsm_step(next, S, V, s, tokens[static_cast<size_t>(b) * tok_stride + j]);
  fsm_state[b] = s;
}

int launch_fsm_advance(const uint16_t* next, int S, int V, int32_t* fsm_state, int B, const int32_t* tokens, int tok_stride,
                       const int32_t* n_new, int max_new, const int32_t* active, hipStream_t st) {
  SD_REQUIRE(next && fsm_state && tokens && n_new, "fsm_advance: NULL argument");
  SD_REQUIRE(S >= 1 && S <= kFsmMaxStates, "fsm_advance: S=%d states (1..%d)", S, kFsmMaxStates);
  SD_REQUIRE(B >= 1 && V >= 1 && max_new >= 0 && tok_stride >= max_new, "fsm_advance: B=%d V=%d max_new=%d stride=%d", B, V, max_new, tok_stride);
  hipLaunchKernelGGL(fsm_advance_kernel, dim3((B + kWave - 1) / kWave), dim3(kWave), 0, st, next, S, V, fsm_state, B, tokens, tok_stride,
                     n_new, max_new, active);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_fsm_mask_bytes(int S, int V) { return fsm_mask_bytes(S, V); }

extern "C" int sd_fsm_build_masks(const void* next, int S, int V, void* allow, size_t allow_bytes, void* stream) {
  clear_error();
  return launch_fsm_build_masks(static_cast<const uint16_t*>(next), S, V, static_cast<uint32_t*>(allow), allow_bytes,
                                static_cast<hipStream_t>(stream));
}

extern "C" int sd_fsm_advance(const void* next, int S, int V, int32_t* fsm_state, int B, const int32_t* tokens, int tok_stride,
                              const int32_t* n_new, int max_new, const int32_t* active, void* stream) {
  clear_error();
  return launch_fsm_advance(static_cast<const uint16_t*>(next), S, V, fsm_state, B, tokens, tok_stride, n_new, max_new, active,
                            static_cast<hipStream_t>(stream));
}

extern "C" int sd_logit_process_fsm(void* rows, int64_t row_stride, int B, int R, int V, const void* counts, const float* bias,
                                    const int32_t* tokens, int tok_stride, int n_tokens, const int32_t* active, float repetition_penalty,
                                    float presence_penalty, float frequency_penalty, int32_t* ids_out, int ids_stride, void* workspace,
                                    size_t workspace_bytes, const void* next, const void* allow, int S, const int32_t* fsm_state, int eos_id,
                                    void* stream) {
  clear_error();
  FsmBind f{};
  f.next = static_cast<const uint16_t*>(next);
  f.allow = static_cast<const uint32_t*>(allow);
  f.S = S;
  f.state = fsm_state;
  f.eos_id = eos_id;
  const LogitStage g{static_cast<const uint16_t*>(counts), bias, repetition_penalty, presence_penalty, frequency_penalty, workspace,
                     workspace_bytes, &f};
  return launch_logit_process({rows, row_stride, B, R, V}, g, tokens, tok_stride, n_tokens, active, ids_out, ids_stride,
                              static_cast<hipStream_t>(stream));
}

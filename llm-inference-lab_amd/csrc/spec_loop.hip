// The draft-then-verify step for gfx950: sd_specdec_* behind the C-ABI (include/specdec_hip.h).
//
// Host-side C++ only. One step proposes K tokens (a draft model, EAGLE-lite rows, the target's own next token, or Medusa
// heads), verifies them in one target forward and advances the loop state — all enqueued on caller-provided HIP streams
// through the model forwards of csrc/engine.hip (models made and bound by csrc/model.hip), never synchronising, and graph-capturable: all per-row dynamic quantities
// (lengths, tokens) live in device memory and are read by the kernels. Which launches a step consists of is decided once per
// enqueue by plan_step; enqueue_step and its pieces only follow the plan.
//
// What it replaces in the reference: the device-facing half of the step loop of SpeculativePipeline.generate_batch
// (pipeline.py:2306-2846: draft stream / verify stream / event waits). The reference verifies by letting the base
// model generate K tokens autoregressively (speculative_scheduler.py:192-199); here
// the target scores all K+1 positions in ONE forward over (last, d_1..d_K), which
// under greedy decoding yields the same accepted prefix and bonus token.

#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <new>
#include <vector>

#include "engine.h"

using namespace sd;

static constexpr int kStageInts = 24;   // per row: 8 ints of set_row, then (accepted, proposed, hist_n, k) + 4 doubles

struct sd_specdec {
  sd_model* draft = nullptr;
  sd_model* target = nullptr;
  int B = 0, K = 0, mode = 0;
  SpecState st{};
  int32_t* dev_block = nullptr;   // all device state in one allocation
  int32_t* step_counter = nullptr; // device: steps executed (its parity selects the record slot)
  int32_t* host_record = nullptr;  // pinned, device-accessible: [2 slots][B][rec]
  hipEvent_t ev_done[2] = {nullptr, nullptr};   // recorded after launch i on the target stream (i & 1)
  long launches = 0;
  int32_t* host_stage = nullptr;  // pinned staging for set_row / set_adaptive_row: [B][kStageInts]
  int a_initial = 0;
  int rec = 0;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipStream_t graph_st_t = nullptr, graph_st_d = nullptr;
  long steps = 0;
  // ---- the sampling stage: one bundle (csrc/engine.h) per thing a setter binds, and beside it the [B][K+1][V] bf16 buffer the
  // mode can lend the verify forward (plan_step picks one). Every buffer is caller-owned unless it says otherwise.
  // Per-row parameters (sd_specdec_set_row_sampling): ONE device table [B], read by the kernels at run time, kept in every
  // bundle a launch takes it from (bonus.table == spec_draw.table == stage.table). While it is bound the draws, the statistics
  // and the process launches are the _rows kernels, and the bundles' scalars are not in those launches.
  int sample = 0;                  // sampled bonus token (sd_specdec_set_sampling)
  DrawSpec bonus;
  void* logits = nullptr;
  // speculative sampling (sd_specdec_set_spec_sampling): draft tokens drawn from q, accept by p/q, residual redraw. The two
  // sampling modes are mutually exclusive; each reads the draw description its own setter filled.
  int spec = 0;
  DrawSpec spec_draw;              // top_k / top_p: sd_specdec_set_spec_shaping (top_k > 0 = both distributions shaped)
  void* spec_q = nullptr;          // [B][K][V] bf16 draft logits
  void* spec_p = nullptr;          // target logits; until the verify forward overwrites it, its first rows are where each draft
                                   // forward leaves the logits of its pass ([B][M][V])
  int32_t* spec_flags = nullptr;   // [2][B][K+1] device, the loop's own: accept flags, candidate next tokens
  // logit processors (sd_specdec_set_logit_processors): every logits row is stored, processed in place, then consumed
  int lp = 0;
  LogitStage stage;                // fsm: &fsm_bind while a grammar is bound (sd_specdec_set_grammar: one more line of the transform)
  void* lp_logits = nullptr;       // used while neither sampling mode owns a buffer
  FsmBind fsm_bind{};              // tables and per-row state are the caller's; pos: [B][K+1], the loop's own (allocated at first use)
  int32_t* fsm_pos = nullptr;
  // lossy acceptance (sd_specdec_set_acceptance): the rule judges the stored verify rows in place of the exact-match scan
  AcceptRule accept;               // rule 0 = off
  void* acc_logits = nullptr;      // used while the sampled-bonus mode does not lend its own
  void* acc_ws = nullptr;          // flags and records of the two launches (the loop's own, allocated at first use)
  // confidence-gated draft length (sd_specdec_set_draft_confidence): on while st.conf; every judged draft forward stores its pass's
  // rows in conf_logits ([B][2][V] bf16) and a judgement launch follows its hand-over
  ConfRule conf;
  uint16_t* conf_logits = nullptr;
  // per-token log-probs (sd_specdec_set_logprobs): one launch between the accept stage and the record describes every emitted token
  // by its stored verify row; the words go to a pinned block of the loop's own, slotted like host_record
  int logprobs = 0;
  int logprobs_top = 0;            // top_n, 0..20
  void* logprobs_logits = nullptr; // used while no other mode stores the verify rows
  int32_t* host_logprobs = nullptr; // pinned: [2][B][K+1][logprob_words(V, top_n)], allocated at first use for top_n = 20
  // persistent Medusa heads (sd_specdec_set_medusa): K packed [V][d] matrices + their fp32 row scales (fp8)
  std::vector<const void*> heads;
  std::vector<const float*> head_scales;
  int32_t* head_rows = nullptr;    // [B] device: row of the target's residual stream each head reads
  size_t head_stride = 0;          // bytes between consecutive heads when they sit at a constant stride (one launch), else 0
  // EAGLE-lite (sd_specdec_set_eagle): extrapolated hidden rows instead of a draft model; caller-owned workspace
  bool draft_taps = false;         // the draft's persistent passes also store their stage rows (debug)
  bool want_fwd0_select = false;   // device-selected form of draft forward 0 (storage carved at create; eligibility per capture)
  int eagle = 0;
  float eagle_alpha = 0.7f;
  uint16_t* eagle_H = nullptr;     // [B*K][d]
  uint16_t* eagle_prev = nullptr;  // [B][d] last extrapolated row of the previous step
  int32_t* eagle_has = nullptr;    // [B]
};

// Forget the captured step, if there is one: the next graph step captures again. The captured launches hold the loop state and
// every mode's parameters by value, so each setter calls this — under its own condition — when what it changes is in the graph.
static void drop_graph(sd_specdec* s) {
  if (!s->exec) return;
  (void)hipGraphExecDestroy(s->exec);
  (void)hipGraphDestroy(s->graph);
  s->exec = nullptr;
  s->graph = nullptr;
}

namespace sd {

// Argmax of n_heads vocabulary-sized matrices over T activation rows: what the Medusa step, the EAGLE step and
// sd_model_head_argmax all run. The matrices have the lm_head's shape (and, unless `prenormed`, its final norm in front);
// id of (matrix j, row t) -> ids[(t / M) * ids_stride + t % M + j].
struct HeadEval {
  const void* x = nullptr;          // bf16 rows of d_model elements (stride d_model)
  const int32_t* x_row = nullptr;   // nullable, device [T]: row t reads row x_row[t] of x
  int T = 0, M = 1;                 // rows, rows per batch row (the id layout; M == 1 whenever n_heads > 1)
  int n_heads = 0;
  const void* const* W = nullptr;          // [n_heads]
  const float* const* scale = nullptr;     // [n_heads] fp32 row scales (w8), else null
  size_t stride = 0;                // bytes between consecutive matrices when constant (one launch), else 0 (one launch each)
  int packed = 1, w8 = 0;
  bool prenormed = false;           // the rows are final-norm outputs already: PRO_NONE, no norm weights
  int32_t* ids = nullptr;
  int ids_stride = 0;
  float* vals = nullptr;            // nullable: the fp32 value attached to each winning index, laid out as ids (debug entry only)
  int* launch_info = nullptr;       // nullable, host [2]: matrix launches enqueued, 1 if the rows were gathered first (debug entry only)
};

// Matrices at a constant stride are evaluated by ONE lm_head-shaped launch (grid y = matrix: same x rows, same geometry,
// per-matrix argmax partials) and one finalize over n_heads x T results; otherwise one launch + finalize per matrix.
static int enqueue_head_argmax(sd_model* m, const HeadEval& e, hipStream_t st) {
  const sd_model_config& c = m->cfg;
  const int T = e.T, nh = e.n_heads;
  GemvArgs h = matrix_args(m, 4 * c.n_layers);   // the lm_head's shape and final norm; the matrices' own weights below
  h.packed = e.packed;
  h.w8 = e.w8;
  h.w12_main = h.w12_ovf = nullptr;   // (the lm_head's W12 copy does not describe e.W)
  h.w12_table = nullptr;
  h.x = e.x;
  h.x_row = e.x_row;
  h.T = T;
  h.M = e.M;
  if (e.prenormed) {
    h.prologue = PRO_NONE;
    h.norm_w = h.norm_b = nullptr;
    h.norm_eps = 0.f;
  }
  if (e.x_row && T > m->small_t) {   // more rows than a GEMV pass: gather them (the attention-output buffer is free after the verify forward)
    if (int rc = launch_medusa_gather(e.x, e.x_row, m->attn, T, c.d_model, st)) return rc;
    h.x = m->attn;
    h.x_row = nullptr;
    if (e.launch_info) e.launch_info[1] = 1;
  }
  int ppw = 1;
  const int grid = gemv_grid(h, &ppw);
  if (nh >= 2 && T <= m->small_t && e.stride && e.M == 1 &&
      static_cast<size_t>(nh) * T * grid <= static_cast<size_t>(kSkinnyMaxT) * kMaxPartials) {
    h.W = e.W[0];
    h.w_scale = e.scale ? e.scale[0] : nullptr;
    h.batch_bytes = e.stride;
    h.n_batch = nh;
    if (int rc = launch_gemv(h, EPI_ARGMAX, st)) return rc;
    if (e.launch_info) e.launch_info[0] = 1;
    // result (matrix j, row t) = "token" j * T + t of the partials -> ids[t][j]
    if (int rc = launch_argmax_finalize(m->part_val, m->part_idx, nh * T, grid, -T, e.ids_stride, e.ids, st)) return rc;
    if (e.vals)
      if (int rc = launch_argmax_value(m->part_val, m->part_idx, nh * T, grid, -T, e.ids_stride, e.vals, st)) return rc;
    return 0;
  }
  for (int i = 0; i < nh; ++i) {
    h.w_scale = e.scale ? e.scale[i] : nullptr;
    h.W = e.W[i];
    if (int rc = launch_gemv(h, EPI_ARGMAX, st)) return rc;
    if (e.launch_info) e.launch_info[0] += 1;
    if (int rc = launch_argmax_finalize(m->part_val, m->part_idx, T, grid, e.M, e.ids_stride, e.ids + i, st)) return rc;
    if (e.vals)
      if (int rc = launch_argmax_value(m->part_val, m->part_idx, T, grid, e.M, e.ids_stride, e.vals + i, st)) return rc;
  }
  return 0;
}

// draft tokens of the NEXT step from the heads: d_{i+1} = argmax head_i(final_norm(h)), h = the residual row of the
// position that produced the last emitted token -> verify_tok[b][i + 1] (enqueue_head_argmax).
static int enqueue_medusa_heads(sd_specdec* s, hipStream_t st) {
  sd_model* m = s->target;
  if (int rc = launch_medusa_rows(s->st, s->head_rows, st)) return rc;
  HeadEval e;
  e.x = m->x;
  e.x_row = s->head_rows;
  e.T = s->B;
  e.n_heads = s->K;
  e.W = s->heads.data();
  e.scale = s->head_scales.empty() ? nullptr : s->head_scales.data();
  e.stride = s->head_stride;
  e.w8 = s->head_scales.empty() ? 0 : 1;
  e.ids = s->st.verify_tok + 1;
  e.ids_stride = s->K + 1;
  if (int rc = enqueue_head_argmax(m, e, st)) return rc;
  return launch_medusa_commit(s->st, st);
}

// ---- one plan per enqueue: every decision of a step, made once from the loop's modes (no HIP call, no write)
enum Proposer { PROPOSE_DRAFT, PROPOSE_EAGLE, PROPOSE_SELF, PROPOSE_HEADS };   // draft model / EAGLE-lite / tied self-draft / Medusa heads alone
// how the emitted tokens are chosen; SELECT_TYPICAL: the draft's ids while the rule keeps them, then the target's argmax or draw
enum Select { SELECT_GREEDY, SELECT_SAMPLED_BONUS, SELECT_SPEC, SELECT_TYPICAL };
enum Handover { HAND_FINALIZE, HAND_NEXT, HAND_DRAW };                         // how d_{i+1} leaves draft forward i

struct StepPlan {
  Proposer proposer;
  bool heads;         // Medusa heads propose the NEXT step's tokens after the verify (set_medusa on an EAGLE loop keeps both)
  Select select;
  bool lp;            // logit processors: the forwards store their rows (into the buffer of the sampling mode that is on, else the
                      // mode's own), the rows are processed in place and the argmax of the processed row replaces the fused one
  bool two;           // the draft forwards run on a stream of their own, forked from and joined to the target's
  // both forms of forward 0 with the device picking one: only while the draft's 1- and 2-token passes are persistent launches
  // (a pass that is not needed then costs one launch that returns at entry, not 80) — decided per capture, the model may have
  // been re-bound or its persistent passes switched off since the loop was created
  bool fwd0_select;
  // a draft forward that is ONE pass leaves the lm_head partials of all its tokens in the model's workspace: ids and the hand-over
  // of d_{i+1} are then one launch (draft_finalize_kernel) instead of two
  bool one_pass_d;
  // HAND_FINALIZE: that one launch. HAND_NEXT: launch_draft_next over the ids the forward (or the processed row) left.
  // HAND_DRAW (speculative sampling): every draft forward stores its logits, d_{i+1} is DRAWN from the last position's row
  Handover hand;
  // greedy steps whose verify forward is ONE pass: ids, accept scan, state advance and the step record are one launch over the
  // lm_head's partials (verify_tail_kernel) instead of three
  bool tail;
  void* p_buf;        // [B][K+1][V] bf16 or null: where the verify forward stores its logits
  uint16_t* q_pass;   // p_buf or null: where each draft forward stores the logits of its pass first (the verify overwrites them)
  int32_t* ids_d;     // draft_ids or null: where a draft forward leaves its fused argmax ids (only HAND_NEXT reads them unprocessed)
  // confidence-gated draft length: forwards conf_first .. K-2 are judged (store their pass's rows in conf_buf, then the judgement
  // launch), forwards conf_first+1 .. K-1 are gated on their word of SpecState::conf_gate. conf_first = K: the mode is off (or K = 1)
  int conf_first;
  uint16_t* conf_buf;
  bool logprobs;      // the log-prob launch between the accept stage and the record (reads p_buf)
};

static StepPlan plan_step(const sd_specdec& s, bool two_streams) {
  StepPlan p{};
  p.proposer = s.draft ? PROPOSE_DRAFT : (s.eagle ? PROPOSE_EAGLE : (s.heads.empty() ? PROPOSE_SELF : PROPOSE_HEADS));
  p.heads = !s.heads.empty();
  p.select = s.accept.rule ? SELECT_TYPICAL : (s.sample ? SELECT_SAMPLED_BONUS : (s.spec ? SELECT_SPEC : SELECT_GREEDY));   // (the setters keep them apart)
  const bool spec = p.select == SELECT_SPEC;
  p.lp = s.lp != 0;
  p.two = two_streams && s.draft;
  p.fwd0_select = s.draft && s.st.fwd0_w && s.B == 1 && persist_pass_ok(s.draft, 2, 1, 2);
  p.one_pass_d = s.draft && s.B * 2 <= s.draft->max_t;
  p.hand = spec ? HAND_DRAW : ((!p.lp && p.one_pass_d) ? HAND_FINALIZE : HAND_NEXT);
  p.tail = p.select == SELECT_GREEDY && !p.lp && verify_tail_fits(s.st) && s.B * (s.K + 1) <= s.target->max_t;
  if (p.select == SELECT_SAMPLED_BONUS) p.p_buf = s.logits;
  else if (p.select == SELECT_TYPICAL) p.p_buf = s.sample ? s.logits : s.acc_logits;
  else if (spec) p.p_buf = s.spec_p;
  else if (p.lp) p.p_buf = s.lp_logits;
  p.logprobs = s.logprobs != 0;
  if (p.logprobs) {   // the rows must be stored: a greedy step lends the mode's own buffer and takes the three launches, not the fused tail
    if (!p.p_buf) p.p_buf = s.logprobs_logits;
    p.tail = false;
  }
  p.q_pass = (spec || p.lp) ? static_cast<uint16_t*>(p.p_buf) : nullptr;
  p.ids_d = (p.hand == HAND_NEXT && !p.lp) ? s.st.draft_ids : nullptr;
  p.conf_first = (s.st.conf && s.draft) ? s.conf.min_k - 1 : s.K;   // (the setter keeps the mode apart from spec, lp and the rules)
  p.conf_buf = s.st.conf ? s.conf_logits : nullptr;
  return p;
}

// a forward of the step: every row of the loop, positions counted from cur_len; the caller names the tokens and what it wants out
static ForwardCall step_forward(const SpecState& st) {
  ForwardCall f;
  f.pos_base = st.cur_len;
  f.B = st.B;
  return f;
}

// ---- the proposers that are not a draft model, on the target stream (Medusa heads propose after the verify: enqueue_verify)
static int enqueue_target_proposer(sd_specdec* s, const StepPlan& p, hipStream_t st_t) {
  const int B = s->B, K = s->K;
  sd_model* m = s->target;
  if (p.proposer == PROPOSE_EAGLE) {
    // EAGLE-lite: residual row of `last` (1-token forward, head skipped) -> K extrapolated rows -> one lm_head launch
    const sd_model_config& c = m->cfg;
    ForwardCall f = step_forward(s->st);
    f.tokens = s->st.verify_tok;
    f.tok_stride = K + 1;
    f.skip_head = 1;
    if (int rc = model_forward(m, f, st_t)) return rc;
    if (int rc = launch_eagle_extrapolate(m->x, s->eagle_H, s->eagle_prev, s->eagle_has, c.final_norm_w, c.final_norm_b, c.norm_eps,
                                          s->eagle_alpha, c.d_model, B, K, c.arch == SD_ARCH_LLAMA ? 1 : 0, st_t))
      return rc;
    const void* const w_head = m->mat(4 * c.n_layers, c.lm_head);
    const float* const sc_head = m->scale(4 * c.n_layers);
    HeadEval e;
    e.x = s->eagle_H;
    e.T = B * K;
    e.M = K;
    e.n_heads = 1;
    e.W = &w_head;
    e.scale = sc_head ? &sc_head : nullptr;
    e.packed = m->is_packed();
    e.w8 = m->w8();
    e.prenormed = true;        // the rows are final-norm outputs already
    e.ids = s->st.verify_tok + 1;
    e.ids_stride = K + 1;
    if (int rc = enqueue_head_argmax(m, e, st_t)) return rc;
    return launch_medusa_commit(s->st, st_t);
  }
  if (p.proposer == PROPOSE_SELF) {
    // self-draft (Medusa-lite, tied heads): the target's own next token, K times
    ForwardCall f = step_forward(s->st);
    f.tokens = s->st.verify_tok;
    f.tok_stride = K + 1;
    f.ids_out = s->st.draft_ids;
    f.ids_stride = 2;
    if (int rc = model_forward(m, f, st_t)) return rc;
    return launch_medusa_fill(s->st, st_t);
  }
  return 0;
}

// ---- the draft loop
// The draft model for the duration of this loop's forwards: the stage taps are the loop's choice, and skip_k / skip_i (set per
// forward) gate every launch of a forward. Taps and skip_k are put back on every way out.
struct DraftScope {
  sd_model* m;
  bool saved;
  DraftScope(sd_model* m_, bool taps) : m(m_), saved(m_->persist_taps) { m->persist_taps = taps; }
  ~DraftScope() {
    m->persist_taps = saved;
    m->skip_k = nullptr;
  }
};

// What follows draft forward i, a pass of M tokens whose last position is row `rows - 1` of the [B][rows] layout of ids and logits
// (rows = M, but for the 1-token form of forward 0: M = 1 in the 2-row layout), gated like the forward by the draft's skip_k /
// skip_i. more_forms: the other form of forward 0 is still to come; exactly one of the two runs and both leave the last position's
// row and id in the same place, so whatever is not gated by the form's own word is launched once, after the second.
// The judgement launch of the confidence-gated step comes last, behind the hand-over, gated on the forward's own word.
static int after_draft_forward(sd_specdec* s, const StepPlan& p, int i, int M, int rows, bool more_forms, hipStream_t st_d) {
  const sd_model* d = s->draft;
  const int V = s->target->cfg.vocab;
  const int32_t* const gate = (i == 0) ? nullptr : d->skip_k;   // forward 0 always runs (its skip_k only picks the form)
  if (p.hand == HAND_FINALIZE) {
    if (int rc = launch_draft_finalize(d->part_val, d->part_idx, d->head_grid, M, i, s->st.draft_ids + (rows - M), s->st, d->skip_k, d->skip_i, st_d))
      return rc;
    if (more_forms) return 0;
  } else {
    if (more_forms) return 0;
    if (p.lp)   // the forward left the logits of its positions in q_pass: process row rows - 1 of every batch row with d_1..d_i
      if (int rc = launch_logit_process({p.q_pass + static_cast<size_t>(rows - 1) * V, static_cast<long long>(rows) * V, s->B, 1, V}, s->stage,
                                        s->st.draft_tok, s->K, i, s->st.active, p.hand == HAND_DRAW ? nullptr : s->st.draft_ids + (rows - 1), 2,
                                        st_d))
        return rc;
    if (int rc = p.hand == HAND_DRAW ? launch_spec_draft_draw(s->st, p.q_pass, rows, rows - 1, s->spec_q, i, V, s->spec_draw, st_d)
                                     : launch_draft_next(rows, i, s->st, gate, st_d))
      return rc;
  }
  if (i < p.conf_first || i > s->K - 2) return 0;
  // the confidence of the last position's row decides, row by row, whether forward i + 1 is needed
  return launch_confidence_judge(s->st, p.conf_buf + static_cast<size_t>(rows - 1) * V, static_cast<long long>(rows) * V, V, i, s->conf,
                                 i == p.conf_first, gate, i, st_d);
}

// forward 0 over (prev, last) at positions cur_len-1, cur_len; then one token each
static int enqueue_draft(sd_specdec* s, const StepPlan& p, hipStream_t st_d) {
  sd_model* d = s->draft;
  const SpecState& st = s->st;
  const int V = s->target->cfg.vocab;
  DraftScope scope(d, s->draft_taps);
  // where forward i stores the rows of its pass: the sampling-side buffer, or the confidence buffer of a judged forward
  const auto pass_rows = [&](int i) { return (i >= p.conf_first && i <= s->K - 2) ? p.conf_buf : p.q_pass; };
  int i = 0;
  if (p.fwd0_select) {
    // both forms of forward 0, the device picks (SpecState::fwd0_w, written by accept_kernel): the 2-token pass, then the
    // 1-token pass over `last` alone, whose id and logits row land where the 2-token pass leaves its second ones
    d->skip_k = st.fwd0_w;
    d->skip_i = 1;
    ForwardCall f2 = step_forward(st);
    f2.tokens = st.tok2;
    f2.tok_stride = f2.M = 2;
    f2.pos_off = -1;
    f2.ids_out = p.ids_d;
    f2.ids_stride = 2;
    f2.logits_out = pass_rows(0);
    if (int rc = model_forward(d, f2, st_d)) return rc;
    if (int rc = after_draft_forward(s, p, 0, 2, 2, true, st_d)) return rc;
    d->skip_k = st.fwd0_w + 1;
    ForwardCall f1 = step_forward(st);
    f1.tokens = st.tok2 + 1;
    f1.tok_stride = 2;
    f1.ids_out = p.ids_d ? p.ids_d + 1 : nullptr;
    f1.ids_stride = 2;
    f1.logits_out = pass_rows(0) ? pass_rows(0) + V : nullptr;
    if (int rc = model_forward(d, f1, st_d)) return rc;
    if (int rc = after_draft_forward(s, p, 0, 1, 2, false, st_d)) return rc;
    i = 1;
  }
  for (; i < s->K; ++i) {
    const int M = (i == 0) ? 2 : 1;
    // per-row adaptive K: forward i >= 1 only matters while some row proposes more than i tokens
    d->skip_k = (st.adaptive && i >= 1) ? st.k_active : nullptr;
    // confidence-gated: forward i > conf_first runs only once a row's judgement of forward i - 1 has opened its word
    if (i > p.conf_first) d->skip_k = st.conf_gate + i;
    d->skip_i = i;
    ForwardCall f = step_forward(st);
    f.tokens = (i == 0) ? st.tok2 : st.next_tok;
    f.tok_stride = f.M = M;
    f.pos_off = (i == 0) ? -1 : i;
    f.ids_out = p.ids_d;
    f.ids_stride = 2;
    f.logits_out = pass_rows(i);
    if (int rc = model_forward(d, f, st_d)) return rc;
    if (int rc = after_draft_forward(s, p, i, M, M, false, st_d)) return rc;
  }
  return 0;
}

// ---- verify: one forward over (last, d_1..d_K), then whatever turns its ids or logits into the step's emitted tokens and record
static int enqueue_verify(sd_specdec* s, const StepPlan& p, hipStream_t st_t) {
  const int B = s->B, K = s->K, V = s->target->cfg.vocab;
  const unsigned* const st_word_d = (s->draft && s->draft->p_sync) ? s->draft->p_sync + 1 : nullptr;
  const unsigned* const st_word_t = s->target->p_sync ? s->target->p_sync + 1 : nullptr;
  ForwardCall f = step_forward(s->st);
  f.tokens = s->st.verify_tok;
  f.tok_stride = f.M = K + 1;
  f.ids_out = p.tail ? nullptr : s->st.target_ids;
  f.ids_stride = K + 1;
  f.logits_out = p.p_buf;
  if (int rc = model_forward(s->target, f, st_t)) return rc;
  if (p.lp)   // all B * (K+1) rows in one launch: row (b, i) is conditioned on d_1..d_i; the processed argmax replaces the fused ids
    if (int rc = launch_logit_process({p.p_buf, V, B, K + 1, V}, s->stage, s->st.draft_tok, K, -1, s->st.active, s->st.target_ids, K + 1, st_t))
      return rc;
  if (p.tail) {
    if (int rc = launch_verify_tail(s->st, s->target->part_val, s->target->part_idx, s->target->head_grid, s->mode, s->host_record, s->rec,
                                    s->step_counter, st_word_d, st_word_t, st_t))
      return rc;
  } else {
    if (p.select == SELECT_SAMPLED_BONUS) {
      // accept length -> draw the token after the accepted prefix from the stored logits of that position
      if (int rc = launch_accept_len(s->st, st_t)) return rc;
      if (int rc = launch_sample_step(s->st, s->logits, V, s->bonus, st_t)) return rc;
    } else if (p.select == SELECT_TYPICAL) {
      // the rule on every stored (processed) row -> accept length; the token after the accepted prefix is the target's id of that
      // position, or drawn from its row when the sampled-bonus mode is on
      if (int rc = launch_typical_step(s->st, p.p_buf, V, s->accept, !s->sample, s->acc_ws, st_t)) return rc;
      if (s->sample)
        if (int rc = launch_sample_step(s->st, s->logits, V, s->bonus, st_t)) return rc;
    } else if (p.select == SELECT_SPEC) {
      // every position's ratio, flag and candidate in parallel -> accept length and the token after the accepted prefix
      if (int rc = launch_spec_step(s->st, s->spec_p, s->spec_q, V, s->spec_draw, s->spec_flags, s->spec_flags + static_cast<size_t>(B) * (K + 1), st_t))
        return rc;
    }
    const int use_sampled = (p.select == SELECT_SPEC || p.select == SELECT_TYPICAL) ? 2 : (p.select == SELECT_SAMPLED_BONUS ? 1 : 0);
    if (int rc = launch_accept(s->st, s->mode, use_sampled, st_t)) return rc;
    if (p.lp)   // the emitted tokens of every active row enter its counts
      if (int rc = launch_logit_counts_add(const_cast<uint16_t*>(s->stage.counts), B, V, s->st.new_tok, K + 1, s->st.n_new, K + 1, s->st.active, st_t)) return rc;
    if (p.lp && s->stage.fsm)   // and advance its automaton state
      if (int rc = launch_fsm_advance(s->fsm_bind.next, s->fsm_bind.S, V, const_cast<int32_t*>(s->fsm_bind.state), B, s->st.new_tok, K + 1,
                                      s->st.n_new, K + 1, s->st.active, st_t))
        return rc;
    if (p.logprobs)   // new_tok and n_new are final, the rows are the processed ones; the slot is read before pack_record advances the counter
      if (int rc = launch_step_logprobs(s->st, p.p_buf, V, s->logprobs_top, s->step_counter, s->host_logprobs, st_t)) return rc;
    if (int rc = launch_pack_record(s->st, s->host_record, s->rec, s->step_counter, st_word_d, st_word_t, st_t)) return rc;
  }
  // persistent Medusa heads: the proposals of the next step, after the record of this one has left
  return p.heads ? enqueue_medusa_heads(s, st_t) : 0;
}

static int enqueue_step(sd_specdec* s, hipStream_t st_t, hipStream_t st_d) {
  const StepPlan p = plan_step(*s, st_d != st_t);
  if (int rc = enqueue_target_proposer(s, p, st_t)) return rc;
  if (p.two) {
    SD_HIP_CHECK(hipEventRecord(s->ev_fork, st_t));
    SD_HIP_CHECK(hipStreamWaitEvent(st_d, s->ev_fork, 0));
  }
  SD_REQUIRE(p.select != SELECT_TYPICAL || (s->draft && p.p_buf && s->acc_ws),
             "specdec_step: the acceptance rule needs a draft model and a logits buffer (sd_specdec_set_acceptance)");
  SD_REQUIRE(!p.logprobs || (s->draft && p.p_buf && s->host_logprobs), "specdec_step: log-probs need a draft model and a logits buffer (sd_specdec_set_logprobs)");
  SD_REQUIRE(!p.lp || (s->draft && p.p_buf), "specdec_step: logit processors need a draft model and a logits buffer (sd_specdec_set_logit_processors)");
  if (p.proposer == PROPOSE_DRAFT)
    if (int rc = enqueue_draft(s, p, st_d)) return rc;
  if (p.two) {
    SD_HIP_CHECK(hipEventRecord(s->ev_join, st_d));
    SD_HIP_CHECK(hipStreamWaitEvent(st_t, s->ev_join, 0));
  }
  return enqueue_verify(s, p, st_t);
}

}  // namespace sd

// The layout of dev_block (int32 words), stated once: against a null base it only measures, against the allocation it assigns
// the loop's pointers. Returns the words the block needs.
static size_t carve_state(sd_specdec* s, int32_t* base, bool fwd0) {
  const size_t B = static_cast<size_t>(s->B), K = static_cast<size_t>(s->K);
  size_t off = 0;
  const auto take = [&](size_t n) {
    int32_t* const p = base ? base + off : nullptr;
    off += n;
    return p;
  };
  SpecState& st = s->st;
  st.B = s->B;
  st.K = s->K;
  st.cur_len = take(B);
  st.active = take(B);
  st.tok2 = take(2 * B);
  st.next_tok = take(B);
  st.draft_ids = take(2 * B);
  st.draft_tok = take(B * K);
  st.verify_tok = take(B * (K + 1));
  st.target_ids = take(B * (K + 1));
  st.accept_len = take(B);
  st.n_new = take(B);
  st.new_tok = take(B * (K + 1));
  st.sampled = take(B);
  s->step_counter = take(4);
  const size_t pad = off & 1;              // the doubles below: 8-byte aligned (hipMalloc is 256-byte aligned)
  off += pad;
  st.ctl_hist = reinterpret_cast<double*>(take(B * 8));
  st.ctl = take(B * 4);
  st.k_row = take(B);
  st.k_active = take(1);
  st.adaptive = 0;
  int32_t* const w = take(2);              // every block has the two words; only a loop that selects forward 0 on the device uses them
  st.fwd0_w = fwd0 ? w : nullptr;
  st.conf = 0;
  st.conf_gate = take(8);                  // one word per draft forward (K <= 8); zero = shut, as the block starts
  return off + 3 - pad;                   // spare words behind the last field: the size depends on B and K alone
}

extern "C" int sd_specdec_create(sd_model* draft, sd_model* target, int B, int K, int emit_mode, sd_specdec** out) {
  clear_error();
  SD_REQUIRE(target && out, "specdec_create: NULL argument");   // draft == NULL: self-draft (Medusa-lite, tied heads)
  SD_REQUIRE(B >= 1 && K >= 1 && K <= 8, "specdec_create: B=%d K=%d (K in 1..8)", B, K);
  SD_REQUIRE(B * (K + 1) <= 65535, "specdec_create: batch too large");
  SD_REQUIRE((!draft || draft->B >= B) && target->B >= B, "specdec_create: models must be bound with batch >= %d", B);
  SD_REQUIRE(!draft || draft->cfg.vocab == target->cfg.vocab, "specdec_create: draft/target vocabularies differ");
  SD_REQUIRE(emit_mode == SD_EMIT_BONUS || emit_mode == SD_EMIT_DRAFT, "specdec_create: emit_mode %d", emit_mode);
  // verify of B rows must fit the passes of the target forward: any B works (tiled)
  sd_specdec* s = new (std::nothrow) sd_specdec();
  SD_REQUIRE(s, "specdec_create: out of memory");
  s->draft = draft;
  s->target = target;
  // nobody reads the hidden rows of a loop's draft: its persistent passes skip the stage taps (csrc/persist.hip, TAPS). The
  // choice belongs to the LOOP (enqueue_draft sets it around the draft's forwards): the same model object used elsewhere — as a
  // standalone model, or as another loop's target — keeps its taps.
  s->draft_taps = getenv(debug_env::kPersistTaps) != nullptr;
  s->B = B;
  s->K = K;
  s->mode = emit_mode;
  s->rec = 7 + 3 * K;
  // device-selected form of draft forward 0: one sequence, a draft whose 1- and 2-token passes are persistent launches (a pass
  // that is not needed then costs one launch that returns at entry, not 80)
  const bool fwd0 = draft && B == 1 && draft->persist_cap >= 2 && !getenv(debug_env::kNoFwd0Select);
  const size_t n_total = carve_state(s, nullptr, fwd0);
  hipError_t e = hipMalloc(&s->dev_block, n_total * sizeof(int32_t));
  if (e != hipSuccess) {
    delete s;
    SD_REQUIRE(false, "specdec_create: hipMalloc failed: %s", hipGetErrorString(e));
  }
  (void)hipMemset(s->dev_block, 0, n_total * sizeof(int32_t));
  carve_state(s, s->dev_block, fwd0);
  if (s->st.fwd0_w) {
    const int32_t init[2] = {2, 1};
    (void)hipMemcpy(s->st.fwd0_w, init, sizeof(init), hipMemcpyHostToDevice);
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&s->host_record), sizeof(int32_t) * 2 * B * s->rec, hipHostMallocDefault) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_done[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_done[1], hipEventDisableTiming) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&s->host_stage), sizeof(int32_t) * (B * kStageInts + 4), hipHostMallocDefault) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess) {
    sd_specdec_destroy(s);
    SD_REQUIRE(false, "specdec_create: pinned memory / event creation failed");
  }
  *out = s;
  return 0;
}

extern "C" int sd_specdec_destroy(sd_specdec* s) {
  if (!s) return 0;
  if (s->exec) (void)hipGraphExecDestroy(s->exec);
  if (s->graph) (void)hipGraphDestroy(s->graph);
  if (s->ev_done[0]) (void)hipEventDestroy(s->ev_done[0]);
  if (s->ev_done[1]) (void)hipEventDestroy(s->ev_done[1]);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  if (s->host_record) (void)hipHostFree(s->host_record);
  if (s->host_stage) (void)hipHostFree(s->host_stage);
  if (s->dev_block) (void)hipFree(s->dev_block);
  if (s->head_rows) (void)hipFree(s->head_rows);
  if (s->spec_flags) (void)hipFree(s->spec_flags);
  if (s->fsm_pos) (void)hipFree(s->fsm_pos);
  if (s->acc_ws) (void)hipFree(s->acc_ws);
  if (s->host_logprobs) (void)hipHostFree(s->host_logprobs);
  delete s;
  return 0;
}

extern "C" int sd_specdec_set_row(sd_specdec* s, int b, int seq_len, int prev_tok, int last_tok, int active,
                                  void* stream) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_row: NULL");
  SD_REQUIRE(b >= 0 && b < s->B, "specdec_set_row: row %d out of range", b);
  SD_REQUIRE(seq_len >= 1, "specdec_set_row: seq_len=%d (need at least one token)", seq_len);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the staging slot of row b must not be rewritten while a previous copy is in flight
  SD_HIP_CHECK(hipStreamSynchronize(st));
  int32_t* h = s->host_stage + b * kStageInts;
  h[0] = seq_len - 1;  // cur_len: position of `last`
  h[1] = active ? 1 : 0;
  h[2] = prev_tok;
  h[3] = last_tok;
  SD_HIP_CHECK(hipMemcpyAsync(s->st.cur_len + b, h + 0, 4, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.active + b, h + 1, 4, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.tok2 + 2 * b, h + 2, 8, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.verify_tok + static_cast<size_t>(b) * (s->K + 1), h + 3, 4, hipMemcpyHostToDevice, st));
  if (s->st.fwd0_w) {   // whatever the caller did to the caches: the next step recomputes prev's K/V
    h[4] = 2;
    h[5] = 1;
    SD_HIP_CHECK(hipMemcpyAsync(s->st.fwd0_w, h + 4, 8, hipMemcpyHostToDevice, st));
  }
  return 0;
}

// Per-row adaptive K. The captured step keeps the shape K = max_k; row b's proposals past k_row[b]
// do not count (accept length clamped, bonus token = the target's token after the clamped prefix), and accept_kernel
// moves k_row[b] by the reference's rule. enable: all rows restart (k = initial_k, history = [0.0] — the reference's
// first get_k call reports acceptance_rate 0.0 before any step).
extern "C" int sd_specdec_set_adaptive(sd_specdec* s, int enable, int initial_k, int min_k, int max_k, int step_size,
                                       double target_rate, void* stream) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_adaptive: NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  drop_graph(s);   // unconditional: the captured kernels hold the loop state by value
  if (!enable) {
    s->st.adaptive = 0;
    return 0;
  }
  SD_REQUIRE(min_k >= 1 && min_k <= max_k && max_k <= s->K, "specdec_set_adaptive: need 1 <= min_k (%d) <= max_k (%d) <= K of the loop (%d)", min_k, max_k, s->K);
  SD_REQUIRE(initial_k >= min_k && initial_k <= max_k, "specdec_set_adaptive: initial_k %d outside [%d, %d]", initial_k, min_k, max_k);
  SD_REQUIRE(step_size >= 1, "specdec_set_adaptive: step_size %d", step_size);
  SD_REQUIRE(target_rate == target_rate, "specdec_set_adaptive: target rate is NaN");
  SD_REQUIRE(s->heads.empty() && !s->eagle, "specdec_set_adaptive: stateful draft modes keep a fixed K");
  SD_REQUIRE(!s->spec, "specdec_set_adaptive: speculative sampling keeps a fixed K (disable it first)");
  SD_REQUIRE(!s->lp, "specdec_set_adaptive: logit processors keep a fixed K (disable sd_specdec_set_logit_processors first)");
  SD_REQUIRE(!s->accept.rule, "specdec_set_adaptive: the acceptance rule keeps a fixed K (disable sd_specdec_set_acceptance first)");
  SD_REQUIRE(!s->st.conf, "specdec_set_adaptive: confidence-gated draft length is on (disable sd_specdec_set_draft_confidence first)");
  SD_REQUIRE(!s->logprobs, "specdec_set_adaptive: per-token log-probs keep a fixed K (disable sd_specdec_set_logprobs first)");
  s->st.adaptive = 1;
  s->st.a_min = min_k;
  s->st.a_max = max_k;
  s->st.a_step = step_size;
  s->st.a_hi = target_rate + 0.1;
  s->st.a_lo = target_rate - 0.1;
  s->a_initial = initial_k;
  for (int b = 0; b < s->B; ++b)
    if (int rc = sd_specdec_set_adaptive_row(s, b, initial_k, 0, 0, 1, nullptr, st)) return rc;
  return 0;
}

// (Re)write one row's controller state — a new sequence in the row's slot, or the host's in-order view after the host
// rules overrode steps that were launched ahead. hist: hist_n <= 4 rates, oldest first (NULL: [0.0]).
extern "C" int sd_specdec_set_adaptive_row(sd_specdec* s, int b, int k, int accepted, int proposed, int hist_n, const double* hist,
                                           void* stream) {
  clear_error();
  SD_REQUIRE(s && s->st.adaptive, "specdec_set_adaptive_row: adaptive K is not enabled");
  SD_REQUIRE(b >= 0 && b < s->B, "specdec_set_adaptive_row: row %d out of range", b);
  SD_REQUIRE(k >= s->st.a_min && k <= s->st.a_max, "specdec_set_adaptive_row: k=%d outside [%d, %d]", k, s->st.a_min, s->st.a_max);
  SD_REQUIRE(hist_n >= 0 && hist_n <= 4 && accepted >= 0 && proposed >= 0, "specdec_set_adaptive_row: bad counters");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SD_HIP_CHECK(hipStreamSynchronize(st));   // the staging slot must not be rewritten under a copy in flight
  int32_t* h = s->host_stage + b * kStageInts + 8;
  double* hd = reinterpret_cast<double*>(h + 4);
  h[0] = accepted;
  h[1] = proposed;
  h[2] = hist ? hist_n : 1;
  h[3] = k;
  for (int i = 0; i < 4; ++i) hd[i] = (hist && i < hist_n) ? hist[i] : 0.0;
  SD_HIP_CHECK(hipMemcpyAsync(s->st.ctl + 4 * b, h, 16, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.ctl_hist + 4 * b, hd, 32, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.k_row + b, h + 3, 4, hipMemcpyHostToDevice, st));
  // k_active (which draft forwards run) is recomputed at the end of every step; until then: all of them
  int32_t* ka = s->host_stage + s->B * kStageInts;
  *ka = s->st.a_max;
  SD_HIP_CHECK(hipMemcpyAsync(s->st.k_active, ka, 4, hipMemcpyHostToDevice, st));
  return 0;
}

extern "C" int sd_specdec_set_sampling(sd_specdec* s, int enable, float temperature, int top_k, float top_p,
                                       uint64_t seed, void* logits_buf, size_t logits_bytes, uint32_t* draw_counters,
                                       const int32_t* stream_ids) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_sampling: NULL");
  drop_graph(s);   // unconditional, on or off: the captured step holds the sampling launches and their parameters
  if (!enable) {
    s->sample = 0;
    return 0;
  }
  SD_REQUIRE(s->mode == SD_EMIT_BONUS, "specdec_set_sampling: only the bonus-token emit mode (generate_batch) samples");
  SD_REQUIRE(!s->spec, "specdec_set_sampling: speculative sampling is enabled (sd_specdec_set_spec_sampling); the two modes are mutually exclusive");
  SD_REQUIRE(logits_buf && draw_counters, "specdec_set_sampling: NULL logits buffer / draw counters");
  const size_t need = static_cast<size_t>(s->B) * (s->K + 1) * s->target->cfg.vocab * 2;
  SD_REQUIRE(logits_bytes >= need, "specdec_set_sampling: logits buffer %zu B < %zu B ([B][K+1][V] bf16)", logits_bytes, need);
  SD_REQUIRE(temperature == temperature && temperature >= 0.f, "specdec_set_sampling: temperature %g", temperature);
  SD_REQUIRE(top_k <= 0 || (top_k < s->target->cfg.vocab ? top_k : s->target->cfg.vocab) <= 1024, "specdec_set_sampling: top_k=%d > 1024", top_k);
  s->sample = 1;
  s->bonus = DrawSpec{temperature, top_k, top_p, seed, draw_counters, 0, stream_ids, s->bonus.table};
  s->logits = logits_buf;
  return 0;
}

extern "C" int sd_specdec_set_spec_sampling(sd_specdec* s, int enable, float temperature, uint64_t seed, void* draft_logits_buf,
                                            size_t draft_logits_bytes, void* target_logits_buf, size_t target_logits_bytes,
                                            uint32_t* draw_counters, const int32_t* stream_ids) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_spec_sampling: NULL");
  if (!enable) {
    if (s->spec) drop_graph(s);   // only if the mode was on: otherwise the captured step holds none of it
    s->spec = 0;
    return 0;
  }
  SD_REQUIRE(s->mode == SD_EMIT_BONUS, "specdec_set_spec_sampling: only the bonus-token emit mode (generate_batch); SD_EMIT_DRAFT is not supported");
  SD_REQUIRE(s->draft, "specdec_set_spec_sampling: needs a draft model (self-draft, Medusa heads and EAGLE loops propose without a distribution q)");
  SD_REQUIRE(!s->st.adaptive, "specdec_set_spec_sampling: per-row adaptive K is not supported (disable sd_specdec_set_adaptive first)");
  SD_REQUIRE(!s->accept.rule, "specdec_set_spec_sampling: an acceptance rule is on (sd_specdec_set_acceptance); speculative sampling has its own");
  SD_REQUIRE(!s->st.conf, "specdec_set_spec_sampling: confidence-gated draft length is on (disable sd_specdec_set_draft_confidence first)");
  SD_REQUIRE(!s->sample, "specdec_set_spec_sampling: the sampled-bonus mode is enabled (sd_specdec_set_sampling); the two modes are mutually exclusive");
  SD_REQUIRE(temperature == temperature && temperature > 0.f, "specdec_set_spec_sampling: temperature %g (must be > 0)", temperature);
  SD_REQUIRE(draft_logits_buf && target_logits_buf && draw_counters, "specdec_set_spec_sampling: NULL logits buffer / draw counters");
  const size_t V = static_cast<size_t>(s->target->cfg.vocab);
  const size_t need_q = static_cast<size_t>(s->B) * s->K * V * 2, need_p = static_cast<size_t>(s->B) * (s->K + 1) * V * 2;
  SD_REQUIRE(draft_logits_bytes >= need_q, "specdec_set_spec_sampling: draft logits buffer %zu B < %zu B ([B][K][V] bf16)", draft_logits_bytes, need_q);
  SD_REQUIRE(target_logits_bytes >= need_p, "specdec_set_spec_sampling: target logits buffer %zu B < %zu B ([B][K+1][V] bf16)", target_logits_bytes, need_p);
  SD_REQUIRE(((reinterpret_cast<uintptr_t>(draft_logits_buf) | reinterpret_cast<uintptr_t>(target_logits_buf)) & 15) == 0,
             "specdec_set_spec_sampling: logits buffers must be 16-byte aligned");
  if (!s->spec_flags) SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->spec_flags), sizeof(int32_t) * 2 * s->B * (s->K + 1)));
  drop_graph(s);   // the captured step holds the other mode's launches, or this mode's parameters
  s->spec = 1;
  s->spec_draw.temperature = temperature;   // (top_k / top_p are sd_specdec_set_spec_shaping's, the table sd_specdec_set_row_sampling's)
  s->spec_draw.seed = seed;
  s->spec_draw.draw = draw_counters;
  s->spec_draw.stream_id = stream_ids;
  s->spec_q = draft_logits_buf;
  s->spec_p = target_logits_buf;
  return 0;
}

extern "C" int sd_specdec_set_logit_processors(sd_specdec* s, int enable, float repetition_penalty, float presence_penalty,
                                               float frequency_penalty, void* counts, size_t counts_bytes, const float* bias,
                                               size_t bias_bytes, void* logits_buf, size_t logits_bytes, void* workspace,
                                               size_t workspace_bytes_) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_logit_processors: NULL");
  if (!enable) {
    if (s->lp) drop_graph(s);   // only if the mode was on: otherwise the captured step holds none of it
    s->lp = 0;
    s->stage.fsm = nullptr;     // the grammar is a line of this stage
    return 0;
  }
  SD_REQUIRE(s->draft, "specdec_set_logit_processors: needs a draft model (self-draft, Medusa heads and EAGLE loops propose from no logits row)");
  SD_REQUIRE(!s->st.adaptive, "specdec_set_logit_processors: per-row adaptive K is not supported (disable sd_specdec_set_adaptive first)");
  SD_REQUIRE(!s->st.conf, "specdec_set_logit_processors: confidence-gated draft length is on (disable sd_specdec_set_draft_confidence first)");
  SD_REQUIRE(repetition_penalty == repetition_penalty && repetition_penalty > 0.f,
             "specdec_set_logit_processors: repetition_penalty %g (must be > 0)", repetition_penalty);
  SD_REQUIRE(presence_penalty - presence_penalty == 0.f && frequency_penalty - frequency_penalty == 0.f,
             "specdec_set_logit_processors: presence_penalty %g / frequency_penalty %g must be finite", presence_penalty, frequency_penalty);
  const size_t V = static_cast<size_t>(s->target->cfg.vocab), BV = static_cast<size_t>(s->B) * V;
  SD_REQUIRE(counts && counts_bytes >= BV * 2, "specdec_set_logit_processors: counts buffer %zu B < %zu B ([B][V] uint16)", counts_bytes, BV * 2);
  SD_REQUIRE(!bias || bias_bytes >= BV * 4, "specdec_set_logit_processors: bias buffer %zu B < %zu B ([B][V] float32)", bias_bytes, BV * 4);
  const size_t need_p = BV * (s->K + 1) * 2, need_ws = logit_process_workspace(s->B, s->K + 1, static_cast<int>(V));
  SD_REQUIRE(logits_buf || s->sample || s->spec, "specdec_set_logit_processors: NULL logits buffer (no sampling mode is on to lend its own)");
  SD_REQUIRE(!logits_buf || logits_bytes >= need_p, "specdec_set_logit_processors: logits buffer %zu B < %zu B ([B][K+1][V] bf16)", logits_bytes, need_p);
  SD_REQUIRE(workspace && workspace_bytes_ >= need_ws, "specdec_set_logit_processors: workspace %zu B < %zu B", workspace_bytes_, need_ws);
  SD_REQUIRE(((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(logits_buf) |
               reinterpret_cast<uintptr_t>(workspace)) & 15) == 0, "specdec_set_logit_processors: buffers must be 16-byte aligned");
  drop_graph(s);   // the captured step holds the unprocessed launches, or this mode's parameters
  s->lp = 1;
  s->stage = LogitStage{static_cast<uint16_t*>(counts), bias, repetition_penalty, presence_penalty, frequency_penalty, workspace, workspace_bytes_,
                        s->stage.fsm, s->stage.table};
  s->lp_logits = logits_buf;
  return 0;
}

extern "C" int sd_specdec_set_grammar(sd_specdec* s, int enable, const void* next, const void* allow, int S, int32_t* fsm_state, int eos_id) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_grammar: NULL");
  if (!enable) {
    if (s->stage.fsm) drop_graph(s);   // only if a grammar was bound: otherwise the captured step holds none of it
    s->stage.fsm = nullptr;
    return 0;
  }
  SD_REQUIRE(s->draft, "specdec_set_grammar: needs a draft model (self-draft, Medusa heads and EAGLE loops propose from no logits row)");
  SD_REQUIRE(!s->st.adaptive, "specdec_set_grammar: per-row adaptive K is not supported (disable sd_specdec_set_adaptive first)");
  SD_REQUIRE(!s->st.conf, "specdec_set_grammar: confidence-gated draft length is on (disable sd_specdec_set_draft_confidence first)");
  SD_REQUIRE(s->lp, "specdec_set_grammar: the logit-processor stage is off (sd_specdec_set_logit_processors first; identity penalties will do)");
  SD_REQUIRE(S >= 1 && S <= kFsmMaxStates, "specdec_set_grammar: S=%d states (1..%d)", S, kFsmMaxStates);
  SD_REQUIRE(eos_id >= 0 && eos_id < s->target->cfg.vocab, "specdec_set_grammar: eos_id %d outside [0, %d)", eos_id, s->target->cfg.vocab);
  SD_REQUIRE(next && allow && fsm_state, "specdec_set_grammar: NULL automaton table / mask table / state");
  SD_REQUIRE(((reinterpret_cast<uintptr_t>(next) | reinterpret_cast<uintptr_t>(allow)) & 15) == 0 && (reinterpret_cast<uintptr_t>(fsm_state) & 3) == 0,
             "specdec_set_grammar: tables must be 16-byte aligned (the state 4-byte)");
  if (!s->fsm_pos) {
    SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->fsm_pos), sizeof(int32_t) * s->B * (s->K + 1)));
    SD_HIP_CHECK(hipMemset(s->fsm_pos, 0xff, sizeof(int32_t) * s->B * (s->K + 1)));   // (-1; every entry is written before it is read)
  }
  drop_graph(s);   // the captured step holds the launches without the mask, or another grammar's tables
  s->fsm_bind = FsmBind{static_cast<const uint16_t*>(next), static_cast<const uint32_t*>(allow), S, fsm_state, eos_id, s->fsm_pos, s->K + 1};
  s->stage.fsm = &s->fsm_bind;
  return 0;
}

extern "C" int sd_specdec_set_spec_shaping(sd_specdec* s, int top_k, float top_p) {
  clear_error();
  SD_REQUIRE(top_p == top_p && top_p > 0.f, "specdec_set_spec_shaping: top_p %g (must be > 0)", top_p);
  SD_REQUIRE(top_k > 0 || top_p >= 1.0f, "specdec_set_spec_shaping: top_p = %g without top_k (the full-vocabulary nucleus) is not supported; "
             "give a top_k in 1..1024", top_p);
  SD_REQUIRE(top_k <= 1024, "specdec_set_spec_shaping: top_k=%d > 1024 is not supported", top_k);
  SD_REQUIRE(s, "specdec_set_spec_shaping: NULL");
  drop_graph(s);   // unconditional, whether or not speculative sampling is on: the captured step holds the launches of the other shape
  s->spec_draw.top_k = top_k > 0 ? top_k : 0;
  s->spec_draw.top_p = top_k > 0 ? top_p : 1.0f;
  return 0;
}

extern "C" int sd_specdec_set_row_sampling(sd_specdec* s, const sd_row_sampling* table) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_row_sampling: NULL");
  if (table) {
    SD_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "specdec_set_row_sampling: the row table must be 16-byte aligned");
    SD_REQUIRE(!s->accept.rule, "specdec_set_row_sampling: an acceptance rule is on (sd_specdec_set_acceptance): its parameters are the loop's, not a row's");
    SD_REQUIRE(!s->st.conf, "specdec_set_row_sampling: confidence-gated draft length is on (disable sd_specdec_set_draft_confidence first)");
    SD_REQUIRE(s->sample || s->spec || s->lp, "specdec_set_row_sampling: neither a sampling mode nor the logit-processor stage is on "
               "(sd_specdec_set_sampling / sd_specdec_set_spec_sampling / sd_specdec_set_logit_processors first)");
  }
  drop_graph(s);   // unconditional: the captured step holds either the scalar launches or the row launches
  s->bonus.table = s->spec_draw.table = s->stage.table = table;
  return 0;
}

extern "C" int sd_specdec_set_acceptance(sd_specdec* s, int rule, float temperature, float epsilon, float delta, int agree_k,
                                         void* logits_buf, size_t logits_bytes) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_acceptance: NULL");
  if (rule == SD_ACCEPT_OFF) {
    if (s->accept.rule) drop_graph(s);   // only if a rule was on: otherwise the captured step holds none of it
    s->accept.rule = SD_ACCEPT_OFF;
    return 0;
  }
  const int V = s->target->cfg.vocab;
  const AcceptRule r{rule, temperature, epsilon, delta, agree_k};
  if (int rc = check_typical_params("specdec_set_acceptance", r, s->K, V)) return rc;
  SD_REQUIRE(s->mode == SD_EMIT_BONUS, "specdec_set_acceptance: only the bonus-token emit mode (generate_batch); SD_EMIT_DRAFT is not supported");
  SD_REQUIRE(!s->eagle, "specdec_set_acceptance: EAGLE loops are not supported (the rule judges a draft model's proposals)");
  SD_REQUIRE(s->heads.empty(), "specdec_set_acceptance: Medusa heads are not supported (the rule judges a draft model's proposals)");
  SD_REQUIRE(s->draft, "specdec_set_acceptance: the tied self-draft is not supported (the rule judges a draft model's proposals)");
  SD_REQUIRE(!s->spec, "specdec_set_acceptance: speculative sampling is enabled (sd_specdec_set_spec_sampling); it has its own acceptance rule");
  SD_REQUIRE(!s->st.adaptive, "specdec_set_acceptance: per-row adaptive K is not supported (disable sd_specdec_set_adaptive first)");
  SD_REQUIRE(!s->st.conf, "specdec_set_acceptance: confidence-gated draft length is on (disable sd_specdec_set_draft_confidence first)");
  SD_REQUIRE(!s->stage.table, "specdec_set_acceptance: a row-sampling table is bound (sd_specdec_set_row_sampling); unbind it first");
  SD_REQUIRE(logits_buf || s->sample, "specdec_set_acceptance: NULL logits buffer (the sampled-bonus mode is not on to lend its own)");
  const size_t need = static_cast<size_t>(s->B) * (s->K + 1) * V * 2;
  SD_REQUIRE(!logits_buf || logits_bytes >= need, "specdec_set_acceptance: logits buffer %zu B < %zu B ([B][K+1][V] bf16)", logits_bytes, need);
  SD_REQUIRE((reinterpret_cast<uintptr_t>(logits_buf) & 15) == 0, "specdec_set_acceptance: the logits buffer must be 16-byte aligned");
  if (!s->acc_ws) SD_HIP_CHECK(hipMalloc(&s->acc_ws, typical_accept_workspace(s->B, s->K)));
  drop_graph(s);   // the captured step holds the exact-match launches, or this rule's parameters
  s->accept = r;
  s->acc_logits = logits_buf;
  return 0;
}

// Confidence-gated draft length (the contract is in include/specdec_hip.h). The device decides alone: the judgement launches of the
// draft loop rewrite k_row inside every step and the step's last launch puts it back, so there is no per-row state to set or repair.
// The caller has drained the loop's streams (k_row is rewritten here, on no stream).
extern "C" int sd_specdec_set_draft_confidence(sd_specdec* s, int enable, float tau, int min_k, void* logits_buf, size_t logits_bytes,
                                               float* conf_out) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_draft_confidence: NULL");
  drop_graph(s);   // unconditional, on or off: the captured step holds the judgement launches, the gates and the rule by value
  if (!enable) {
    s->st.conf = 0;
    return 0;
  }
  SD_REQUIRE(tau > 0.f && tau <= 1.0f, "specdec_set_draft_confidence: tau %g outside (0, 1]", tau);   // (a NaN compares false)
  SD_REQUIRE(min_k >= 1 && min_k <= s->K, "specdec_set_draft_confidence: min_k %d outside 1..K (%d)", min_k, s->K);
  SD_REQUIRE(s->draft, "specdec_set_draft_confidence: needs a draft model (self-draft, Medusa heads and EAGLE loops have no draft forward to judge)");
  SD_REQUIRE(s->mode == SD_EMIT_BONUS, "specdec_set_draft_confidence: only the bonus-token emit mode (generate_batch); SD_EMIT_DRAFT is not supported");
  SD_REQUIRE(!s->st.adaptive, "specdec_set_draft_confidence: per-row adaptive K is on (disable sd_specdec_set_adaptive first)");
  SD_REQUIRE(!s->spec, "specdec_set_draft_confidence: speculative sampling is enabled (sd_specdec_set_spec_sampling); it keeps a fixed K");
  SD_REQUIRE(!s->accept.rule, "specdec_set_draft_confidence: an acceptance rule is on (sd_specdec_set_acceptance); it keeps a fixed K");
  SD_REQUIRE(!s->lp, "specdec_set_draft_confidence: logit processors / a grammar are on (sd_specdec_set_logit_processors); they keep a fixed K");
  SD_REQUIRE(!s->stage.table, "specdec_set_draft_confidence: a row-sampling table is bound (sd_specdec_set_row_sampling); unbind it first");
  SD_REQUIRE(!s->logprobs, "specdec_set_draft_confidence: per-token log-probs are on (sd_specdec_set_logprobs); they keep a fixed K");
  const size_t need = sd_specdec_draft_confidence_bytes(s->B, s->target->cfg.vocab);
  SD_REQUIRE(logits_buf, "specdec_set_draft_confidence: NULL logits buffer");
  SD_REQUIRE(logits_bytes >= need, "specdec_set_draft_confidence: logits buffer %zu B < %zu B ([B][2][V] bf16)", logits_bytes, need);
  SD_REQUIRE((reinterpret_cast<uintptr_t>(logits_buf) & 15) == 0 && (reinterpret_cast<uintptr_t>(conf_out) & 3) == 0,
             "specdec_set_draft_confidence: the logits buffer must be 16-byte aligned (conf_out 4-byte)");
  // every row starts a step at K with every gated forward shut (rows that a disabled adaptive K left elsewhere included)
  std::vector<int32_t> init(static_cast<size_t>(s->B), s->K);
  SD_HIP_CHECK(hipMemcpy(s->st.k_row, init.data(), sizeof(int32_t) * s->B, hipMemcpyHostToDevice));
  SD_HIP_CHECK(hipMemset(s->st.conf_gate, 0, sizeof(int32_t) * 8));
  if (conf_out) {   // NaN until a judgement writes it: with min_k == K (or K == 1) no forward is judged and no launch ever does
    const uint32_t nan_bits = 0x7fc00000u;
    std::vector<float> nans(static_cast<size_t>(s->B) * s->K, __builtin_bit_cast(float, nan_bits));
    SD_HIP_CHECK(hipMemcpy(conf_out, nans.data(), sizeof(float) * nans.size(), hipMemcpyHostToDevice));
  }
  s->st.conf = 1;
  s->conf = ConfRule{tau, min_k, conf_out};
  s->conf_logits = static_cast<uint16_t*>(logits_buf);
  return 0;
}

// Per-token log-probs inside the step (the contract is in include/specdec_hip.h). The caller has drained the loop.
extern "C" int sd_specdec_set_logprobs(sd_specdec* s, int enable, int top_n, void* logits_buf, size_t logits_bytes) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_logprobs: NULL");
  if (!enable) {
    if (s->logprobs) drop_graph(s);   // only if the mode was on: otherwise the captured step holds none of it
    s->logprobs = 0;
    return 0;
  }
  const int V = s->target->cfg.vocab;
  if (int rc = check_logprob_params("specdec_set_logprobs", V, top_n)) return rc;
  SD_REQUIRE(s->draft, "specdec_set_logprobs: needs a draft model (self-draft, Medusa heads and EAGLE loops are not supported)");
  SD_REQUIRE(s->mode == SD_EMIT_BONUS, "specdec_set_logprobs: only the bonus-token emit mode (generate_batch); SD_EMIT_DRAFT is not supported");
  SD_REQUIRE(!s->st.adaptive, "specdec_set_logprobs: per-row adaptive K is not supported (disable sd_specdec_set_adaptive first)");
  SD_REQUIRE(!s->st.conf, "specdec_set_logprobs: confidence-gated draft length is on (disable sd_specdec_set_draft_confidence first)");
  const size_t need = static_cast<size_t>(s->B) * (s->K + 1) * V * 2;
  SD_REQUIRE(logits_buf, "specdec_set_logprobs: NULL logits buffer");
  SD_REQUIRE(logits_bytes >= need, "specdec_set_logprobs: logits buffer %zu B < %zu B ([B][K+1][V] bf16)", logits_bytes, need);
  SD_REQUIRE((reinterpret_cast<uintptr_t>(logits_buf) & 15) == 0, "specdec_set_logprobs: the logits buffer must be 16-byte aligned");
  if (!s->host_logprobs) {
    const size_t words = static_cast<size_t>(2) * s->B * (s->K + 1) * logprob_words(V, 20);
    SD_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&s->host_logprobs), sizeof(int32_t) * words, hipHostMallocDefault));
  }
  drop_graph(s);   // the captured step holds the launches without the stage, or another top_n
  s->logprobs = 1;
  s->logprobs_top = top_n;
  s->logprobs_logits = logits_buf;
  return 0;
}

extern "C" size_t sd_specdec_eagle_bytes(int B, int K, int d_model) {
  if (B <= 0 || K <= 0 || d_model <= 0) return 0;
  return (static_cast<size_t>(B) * K * d_model + static_cast<size_t>(B) * d_model) * 2 + static_cast<size_t>(B) * 4 + 1024;
}

// workspace layout: [state rows B x d bf16][has_prev B x int32][extrapolated rows B*K x d bf16] — the state sits at
// offsets that do not depend on K, so loops of different K over the same workspace (adaptive K) share it
extern "C" int sd_specdec_set_eagle(sd_specdec* s, float alpha, void* workspace, size_t workspace_bytes_) {
  clear_error();
  SD_REQUIRE(s && workspace, "specdec_set_eagle: NULL argument");
  SD_REQUIRE(!s->draft, "specdec_set_eagle: the loop was created with a draft model (pass draft = NULL)");
  SD_REQUIRE(s->heads.empty(), "specdec_set_eagle: the loop already has Medusa heads");
  const int d = s->target->cfg.d_model;
  SD_REQUIRE(workspace_bytes_ >= sd_specdec_eagle_bytes(s->B, s->K, d), "specdec_set_eagle: workspace too small");
  SD_REQUIRE(s->B * s->K <= s->target->max_t, "specdec_set_eagle: B*K = %d rows exceed one lm_head pass (%d)", s->B * s->K, s->target->max_t);
  SD_REQUIRE(!s->exec, "specdec_set_eagle: call before the first captured step");
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
  s->eagle_prev = reinterpret_cast<uint16_t*>(p);
  p += (static_cast<size_t>(s->B) * d * 2 + 255) & ~static_cast<size_t>(255);
  s->eagle_has = reinterpret_cast<int32_t*>(p);
  p += (static_cast<size_t>(s->B) * 4 + 255) & ~static_cast<size_t>(255);
  s->eagle_H = reinterpret_cast<uint16_t*>(p);
  s->eagle_alpha = alpha;
  s->eagle = 1;
  return 0;
}

extern "C" int sd_specdec_reset_eagle(sd_specdec* s, void* stream) {
  clear_error();
  SD_REQUIRE(s && s->eagle, "specdec_reset_eagle: EAGLE mode is not set");
  SD_HIP_CHECK(hipMemsetAsync(s->eagle_has, 0, static_cast<size_t>(s->B) * 4, static_cast<hipStream_t>(stream)));
  return 0;
}

// bytes between consecutive heads when they sit at a constant, ascending stride (-> one launch for all of them), else 0
static size_t constant_stride(int n_heads, const void* const* packed_heads) {
  if (n_heads < 2) return 0;
  const char* h0 = static_cast<const char*>(packed_heads[0]);
  const char* h1 = static_cast<const char*>(packed_heads[1]);
  bool even = h1 > h0;
  for (int i = 2; even && i < n_heads; ++i)
    even = static_cast<const char*>(packed_heads[i]) - static_cast<const char*>(packed_heads[i - 1]) == h1 - h0;
  return even ? static_cast<size_t>(h1 - h0) : 0;
}

extern "C" int sd_specdec_set_medusa(sd_specdec* s, int n_heads, const void* const* packed_heads, int weight_dtype) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_medusa: NULL");
  SD_REQUIRE(!s->draft, "specdec_set_medusa: the loop was created with a draft model (pass draft = NULL)");
  SD_REQUIRE(n_heads == s->K && packed_heads, "specdec_set_medusa: need K = %d heads, got %d", s->K, n_heads);
  SD_REQUIRE(weight_dtype == SD_BF16 || weight_dtype == SD_FP8_E4M3, "specdec_set_medusa: weight_dtype %d", weight_dtype);
  const sd_model_config& c = s->target->cfg;
  SD_REQUIRE(s->B <= s->target->small_t || (s->B <= s->target->max_t && c.n_heads * c.head_dim >= c.d_model),
             "specdec_set_medusa: batch %d exceeds one pass of the head kernels (%d rows)", s->B, s->target->max_t);
  SD_REQUIRE(s->B * (s->K + 1) <= s->target->max_t, "specdec_set_medusa: the verify pass must be a single pass (B*(K+1) = %d > %d)",
             s->B * (s->K + 1), s->target->max_t);
  drop_graph(s);   // the captured step holds the heads' launches by address
  s->heads.clear();
  s->head_scales.clear();
  for (int i = 0; i < n_heads; ++i) {
    SD_REQUIRE(packed_heads[i], "specdec_set_medusa: head %d is NULL", i);
    s->heads.push_back(packed_heads[i]);
    if (weight_dtype == SD_FP8_E4M3) {
      const MatShape h = matrix_shape(c, 4);   // the fp32 row scales follow the packed bytes (sd_pack_head)
      s->head_scales.push_back(reinterpret_cast<const float*>(static_cast<const char*>(packed_heads[i]) + packed_fp8_weight_bytes(h.n_pairs, h.K)));
    }
  }
  s->head_stride = getenv(debug_env::kMedusaPerHead) ? 0 : constant_stride(n_heads, packed_heads);
  if (!s->head_rows) SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->head_rows), sizeof(int32_t) * s->B));
  return 0;
}

// The step's head evaluation (enqueue_head_argmax) on caller-supplied rows: ids and the value attached to each of them.
extern "C" int sd_model_head_argmax(sd_model* m, const void* x_bf16, int n_rows, const int32_t* row_idx, int B, int n_heads,
                                    const void* const* packed_heads, int weight_dtype, int flags, int32_t* ids, float* vals,
                                    int* launch_info, void* stream) {
  clear_error();
  SD_REQUIRE(m && m->x && x_bf16 && packed_heads && ids, "model_head_argmax: NULL argument / model not bound");
  SD_REQUIRE(n_heads >= 1 && n_heads <= 64, "model_head_argmax: n_heads=%d (1..64)", n_heads);
  SD_REQUIRE(weight_dtype == SD_BF16 || weight_dtype == SD_FP8_E4M3, "model_head_argmax: weight_dtype %d", weight_dtype);
  SD_REQUIRE((flags & ~(SD_HEADS_PER_HEAD | SD_HEADS_NORMALISED)) == 0, "model_head_argmax: unknown flags %#x", flags);
  const sd_model_config& c = m->cfg;
  SD_REQUIRE(weight_dtype == SD_BF16 || c.d_model % 64 == 0, "model_head_argmax: fp8 heads need d_model (%d) in whole 64-k steps", c.d_model);
  SD_REQUIRE(B >= 1 && n_rows >= 1 && (row_idx || B <= n_rows), "model_head_argmax: B=%d rows of %d", B, n_rows);
  SD_REQUIRE(B <= m->small_t || (B <= m->max_t && (!row_idx || c.n_heads * c.head_dim >= c.d_model)),
             "model_head_argmax: batch %d exceeds one pass of the head kernels (%d rows)", B, m->max_t);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (row_idx) {   // a debug entry: the indices are checked on the host before any kernel follows them
    std::vector<int32_t> host(static_cast<size_t>(B));
    SD_HIP_CHECK(hipMemcpyAsync(host.data(), row_idx, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    SD_HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b)
      SD_REQUIRE(host[b] >= 0 && host[b] < n_rows, "model_head_argmax: row_idx[%d] = %d outside the %d rows", b, host[b], n_rows);
  }
  std::vector<const void*> heads;
  std::vector<const float*> scales;
  const MatShape hs = matrix_shape(c, 4);
  for (int i = 0; i < n_heads; ++i) {
    SD_REQUIRE(packed_heads[i], "model_head_argmax: head %d is NULL", i);
    SD_REQUIRE((reinterpret_cast<uintptr_t>(packed_heads[i]) & 255) == 0, "model_head_argmax: head %d is not 256-byte aligned", i);
    heads.push_back(packed_heads[i]);
    if (weight_dtype == SD_FP8_E4M3)   // the fp32 row scales follow the packed bytes (sd_pack_head)
      scales.push_back(reinterpret_cast<const float*>(static_cast<const char*>(packed_heads[i]) + packed_fp8_weight_bytes(hs.n_pairs, hs.K)));
  }
  HeadEval e;
  e.x = x_bf16;
  e.x_row = row_idx;
  e.T = B;
  e.n_heads = n_heads;
  e.W = heads.data();
  e.scale = scales.empty() ? nullptr : scales.data();
  e.stride = (flags & SD_HEADS_PER_HEAD) ? 0 : constant_stride(n_heads, packed_heads);
  e.w8 = scales.empty() ? 0 : 1;
  e.prenormed = (flags & SD_HEADS_NORMALISED) != 0;
  e.ids = ids;
  e.ids_stride = n_heads;
  e.vals = vals;
  if (launch_info) launch_info[0] = launch_info[1] = 0;
  e.launch_info = launch_info;
  return enqueue_head_argmax(m, e, st);
}

extern "C" int sd_eagle_extrapolate(const void* x_bf16, void* H, void* prev, int32_t* has_prev, const void* norm_w, const void* norm_b,
                                    float eps, float alpha, int d_model, int B, int K, int rms, void* stream) {
  clear_error();
  SD_REQUIRE(x_bf16 && H && prev && has_prev && norm_w, "eagle_extrapolate: NULL argument");
  SD_REQUIRE(rms || norm_b, "eagle_extrapolate: LayerNorm needs the bias");
  SD_REQUIRE(d_model >= 1 && B >= 1 && B <= 65535 && K >= 1 && K <= 8, "eagle_extrapolate: d_model=%d B=%d K=%d (K in 1..8)", d_model, B, K);
  return launch_eagle_extrapolate(x_bf16, H, prev, has_prev, norm_w, norm_b, eps, alpha, d_model, B, K, rms ? 1 : 0,
                                  static_cast<hipStream_t>(stream));
}

extern "C" int sd_specdec_step(sd_specdec* s, void* stream_target, void* stream_draft, int use_graph) {
  clear_error();
  SD_REQUIRE(s, "specdec_step: NULL");
  hipStream_t st_t = static_cast<hipStream_t>(stream_target);
  hipStream_t st_d = stream_draft ? static_cast<hipStream_t>(stream_draft) : st_t;
  s->steps++;
  if (!use_graph || s->steps == 1) {
    // the first step always runs eagerly: it also performs the one-time kernel
    // attribute setup that must not happen inside a capture
    if (int rc = enqueue_step(s, st_t, st_d)) return rc;
    SD_HIP_CHECK(hipEventRecord(s->ev_done[s->launches & 1], st_t));
    s->launches++;
    return 0;
  }
  if (s->graph_st_t != st_t || s->graph_st_d != st_d) drop_graph(s);   // captured on other streams
  if (!s->exec) {
    SD_HIP_CHECK(hipStreamBeginCapture(st_t, hipStreamCaptureModeRelaxed));
    const int rc = enqueue_step(s, st_t, st_d);
    hipGraph_t g = nullptr;
    const hipError_t ee = hipStreamEndCapture(st_t, &g);
    if (rc != 0) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    SD_HIP_CHECK(ee);
    s->graph = g;
    SD_HIP_CHECK(hipGraphInstantiate(&s->exec, s->graph, nullptr, nullptr, 0));
    s->graph_st_t = st_t;
    s->graph_st_d = st_d;
  }
  SD_HIP_CHECK(hipGraphLaunch(s->exec, st_t));
  SD_HIP_CHECK(hipEventRecord(s->ev_done[s->launches & 1], st_t));   // completion of THIS step (sd_specdec_wait)
  s->launches++;
  return 0;
}

extern "C" int sd_specdec_invalidate(sd_specdec* s) {
  clear_error();
  SD_REQUIRE(s, "specdec_invalidate: NULL");
  drop_graph(s);
  s->steps = 0;   // the next step runs eagerly (kernels of the other path may still need their one-time attribute setup)
  return 0;
}

extern "C" long sd_specdec_launches(const sd_specdec* s) { return s ? s->launches : 0; }

extern "C" long sd_specdec_graph_nodes(const sd_specdec* s) {
  if (!s || !s->graph) return 0;
  size_t n = 0;
  return hipGraphGetNodes(s->graph, nullptr, &n) == hipSuccess ? static_cast<long>(n) : -1;
}

extern "C" int sd_specdec_wait(sd_specdec* s, long launch_index) {
  clear_error();
  SD_REQUIRE(s, "specdec_wait: NULL");
  SD_REQUIRE(launch_index >= 0 && launch_index < s->launches && launch_index + 2 >= s->launches,
             "specdec_wait: step %ld is not one of the last two launches (%ld launched)", launch_index, s->launches);
  SD_HIP_CHECK(hipEventSynchronize(s->ev_done[launch_index & 1]));
  return 0;
}

extern "C" int sd_specdec_sync(sd_specdec* s, void* stream) {
  clear_error();
  (void)s;
  SD_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return 0;
}

// two slots of [B][record_ints]: the record of launch i is in slot i & 1
extern "C" const int32_t* sd_specdec_record(const sd_specdec* s) { return s ? s->host_record : nullptr; }

extern "C" int sd_specdec_record_ints(const sd_specdec* s) { return s ? s->rec : 0; }

// two slots of [B][K+1][words]: the log-prob words of launch i are in slot i & 1 (null / 0 until sd_specdec_set_logprobs enabled the mode)
extern "C" const int32_t* sd_specdec_logprobs(const sd_specdec* s) { return s ? s->host_logprobs : nullptr; }

extern "C" int sd_specdec_logprob_words(const sd_specdec* s) {
  return (s && s->logprobs) ? logprob_words(s->target->cfg.vocab, s->logprobs_top) : 0;
}

// The model behind sd_model_*: its lifetime and storage. Create / destroy, the W12 copies, the workspace layout, the dense and paged
// binds, KV shared between cache rows, and the small setters and getters. The forward that runs on it is csrc/engine.hip.
// Host-side C++ behind the C-ABI (include/specdec_hip.h).

#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <new>
#include <vector>

#include "engine.h"

namespace sd {

// One CU (three waves) walks a head's whole cache in the persistent launch, where the launch path splits long rows over up to 32
// workgroups — 1B dimensions, 1 token, us per forward persistent / launches at 128 ... 4096 cached positions: 588 / 675,
// 605 / 694, 651 / 721, 723 / 764, 888 / 767, 1186 / 777 (profiles/round3_persist_ab.md): the persistent launch serves rows of
// up to this many positions (where the two lines cross: 723 + 0.161 (L - 1024) against 764 + 0.003 (L - 1024) us at L = 1283;
// round 4's context sweep: 5.07 ms per step on the persistent launch at 1400-1536 positions against 4.96 on the launch path at 2048).
constexpr int kPersistMaxCtx = 1280;

// The caller's workspace, described once: the byte offset of every region from the 256-byte-aligned base, and the bytes to ask for.
// x .. act: the staged rows of a pass (engine.h StagedRows), kSkinnyMaxT rows each; the head's argmax partials; the split-KV partial
// tiles and, inside the same region, their arrival counters (attention.hip); the row statistics; the persistent forward's region.
struct WorkspaceLayout { size_t x, q, attn, act, part_val, part_idx, attn_ws, attn_cnt, xstat, persist, bytes; };

static WorkspaceLayout workspace_layout(const sd_model_config& c) {
  const size_t T = kSkinnyMaxT;
  size_t n = 0;
  auto region = [&n](size_t bytes) { const size_t at = n; n += align_up(bytes, 256); return at; };
  const size_t head_rows = T * c.n_heads * c.head_dim * 2, partials = T * kMaxPartials * 4;
  WorkspaceLayout w{};
  w.x = region(T * c.d_model * 2);
  w.q = region(head_rows);
  w.attn = region(head_rows);
  w.act = region(T * c.d_ff * 2);
  w.part_val = region(partials);
  w.part_idx = region(partials);
  w.attn_ws = region(attention_split_ws_bytes(c.head_dim));
  w.attn_cnt = w.attn_ws + attention_split_tiles_bytes(c.head_dim);
  w.xstat = region(sizeof(float) * 2 * kStatPlane);
  w.persist = region(persist_workspace(c).bytes);
  w.bytes = n + 256;   // (the base is aligned up inside the caller's buffer)
  return w;
}

// the matrices of `classes` onto a copy of `form`; the other matrices keep what they stream
static int model_add_w12(sd_model* m, const void* w12, const uint32_t* n_wide, unsigned classes, int form) {
  SD_REQUIRE(w12 && n_wide, "model_set_w12: NULL buffer or counts");
  SD_REQUIRE(form == W12_CODES || form == W12_SPLIT, "model_set_w12: form %d (SD_W12_FORM_CODES or SD_W12_FORM_SPLIT)", form);
  SD_REQUIRE(m->is_packed() && !m->w8() && m->cfg.weight_dtype == SD_BF16, "model_set_w12: W12 is a copy of packed bf16 weights");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(w12) & 255) == 0, "model_set_w12: the buffer must be 256-byte aligned");
  const sd_model_config& c = m->cfg;
  if (m->w12.empty()) m->w12.assign(4 * c.n_layers + 1, sd_model::W12Mat{nullptr, nullptr, nullptr, W12_NONE});
  for (int i = 0; i <= 4 * c.n_layers; ++i) {
    const int which = matrix_which(c, i);
    const MatShape sh = matrix_shape(c, which);
    if (!w12_taken(sh.n_pairs, sh.K, n_wide[i]) || !((classes >> which) & 1)) continue;
    const W12Layout l = w12_layout(sh.n_pairs, sh.K, n_wide[i]);
    const char* p = static_cast<const char*>(w12) + w12_offset(c, n_wide, i);
    m->w12[i] = {p, reinterpret_cast<const uint32_t*>(p + l.main_bytes + l.ovf_bytes), p + l.main_bytes, form};
  }
  return 0;
}

// ---- persistent forward: the op table on the device and the tokens per pass it takes for this model, device and cache
static int setup_persist(sd_model* m) {
  const sd_model_config& c = m->cfg;
  m->persist_t = 0;
  m->persist_cap = 0;
  m->len_hint = m->Lmax;
  if (!m->host_status) SD_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m->host_status), 64, hipHostMallocDefault));
  *m->host_status = 0u;
  int dev = 0;
  hipDeviceProp_t prop{};
  SD_HIP_CHECK(hipGetDevice(&dev));
  SD_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  if (!persist_model_ok(c, m->is_packed() != 0, m->w8() != 0, prop.multiProcessorCount)) return 0;
  std::vector<PersistOp> ops;
  for (int i = 0; i <= 4 * c.n_layers; ++i) {
    const int which = matrix_which(c, i);   // = PersistKind
    const MatShape sh = matrix_shape(c, which);
    const GemvGeom q = gemv_geometry(sh.n_pairs, sh.K);
    PersistOp o{};
    o.W = m->packed[i];
    o.norm_w = matrix_weights(c, i).norm_w;
    o.pair_bytes = static_cast<unsigned>(4 * sh.K);
    o.n_pairs = sh.n_pairs;
    o.ppw = q.ppw;
    o.tile_pairs = q.tile_pairs;
    o.K = sh.K;
    o.kind = which;
    o.layer = i >> 2;
    ops.push_back(o);
  }
  SD_HIP_CHECK(hipMemcpy(m->p_ops, ops.data(), ops.size() * sizeof(PersistOp), hipMemcpyHostToDevice));
  // (a cache whose rows are not whole 8-key vectors cannot be walked by the launch's attention: launch path)
  m->persist_cap = persist_cache_ok(m->Lmax) ? persist_max_tokens(c) : 0;
  // tokens per pass the persistent launch takes (0 = off), by measurement (same box, 128 cached positions, us per forward,
  // persistent / launches; profiles/round3_persist_ab.md): Llama-3.2-1B dimensions 1 token 596 / 698, 2 tokens 677 / 718,
  // 3 tokens 838 / 741; Llama-3.2-3B dimensions 1 token 1506 / 1495, 2 tokens 1640 / 1540. So: 2 tokens up to
  // d_model = 2048 (the draft), off above it (the target's passes stay on launches).
  // And by context (kPersistMaxCtx): by the rows' CURRENT lengths as the caller bounds them (sd_model_set_length_hint; the
  // default bound is the cache size: sessions that size the cache to prompt + budget need not say anything).
  const char* env = getenv(debug_env::kPersistMaxT);
  const int want = env ? atoi(env) : (c.d_model <= 2048 ? 2 : 0);
  m->persist_t = m->persist_cap < want ? m->persist_cap : want;
  m->ctx_limit = env ? m->Lmax : kPersistMaxCtx;   // (the measurement override also lifts the context bound)
  return 0;
}

static int carve_workspace(sd_model* m, void* workspace) {
  const WorkspaceLayout w = workspace_layout(m->cfg);
  char* base = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(workspace), 256));
  m->x = reinterpret_cast<uint16_t*>(base + w.x);
  m->q = reinterpret_cast<uint16_t*>(base + w.q);
  m->attn = reinterpret_cast<uint16_t*>(base + w.attn);
  m->act = reinterpret_cast<uint16_t*>(base + w.act);
  m->part_val = reinterpret_cast<float*>(base + w.part_val);
  m->part_idx = reinterpret_cast<int*>(base + w.part_idx);
  m->attn_ws = reinterpret_cast<float*>(base + w.attn_ws);
  m->attn_cnt = reinterpret_cast<unsigned*>(base + w.attn_cnt);
  m->xstat = reinterpret_cast<float*>(base + w.xstat);
  SD_HIP_CHECK(hipMemset(m->attn_cnt, 0, kAttnSplitSlots * sizeof(unsigned)));
  m->probe_pos = reinterpret_cast<int32_t*>(m->attn_cnt);   // a zero word (the counters rest at zero between launches)
  // ---- persistent forward: sync words, op table, granule buffers (all zero: tag 0 is never a valid tag)
  const PersistWorkspace pw = persist_workspace(m->cfg);
  char* pp = base + w.persist;
  SD_HIP_CHECK(hipMemset(pp, 0, pw.bytes));
  m->p_sync = reinterpret_cast<unsigned*>(pp + pw.sync);
  m->p_ops = reinterpret_cast<PersistOp*>(pp + pw.ops);
  m->p_gran = reinterpret_cast<unsigned long long*>(pp + pw.gran);
  m->p_gran_parity = pw.gran_parity;
  return setup_persist(m);
}

// What both binds do once their own arguments have passed: the cache description (block_table null: dense rows of Lmax positions),
// a fresh prompt route, count and record, and the carve.
static int bind_caches(sd_model* m, void* k, void* v, int B, int Lmax, const int32_t* block_table, int page_shift, int max_pages,
                       int n_pages, void* workspace) {
  m->k_cache = static_cast<uint16_t*>(k);
  m->v_cache = static_cast<uint16_t*>(v);
  m->B = B; m->Lmax = Lmax;
  m->block_table = block_table;
  m->page_shift = page_shift; m->max_pages = max_pages; m->n_pages = n_pages;
  m->prefill_backend = SD_PREFILL_AUTO;
  m->prefill_mc = 0;
  for (int64_t& n : m->prefill_count) n = 0;
  return carve_workspace(m, workspace);
}

}  // namespace sd

// ============================================================================ C-ABI
using namespace sd;

extern "C" int sd_model_create(const sd_model_config* cfg, sd_model** out) {
  clear_error();
  SD_REQUIRE(cfg && out, "model_create: NULL argument");
  SD_REQUIRE(cfg->arch == SD_ARCH_LLAMA || cfg->arch == SD_ARCH_GPT2, "model_create: arch %d", cfg->arch);
  SD_REQUIRE(cfg->weight_dtype == SD_BF16 || cfg->weight_dtype == SD_FP8_E4M3,
             "model_create: weight_dtype %d (SD_BF16, or SD_FP8_E4M3 = stream the fp8 copy made by sd_pack_weights)", cfg->weight_dtype);
  SD_REQUIRE(cfg->weight_dtype != SD_FP8_E4M3 || cfg->packed, "model_create: fp8 storage needs the packed buffer of sd_pack_weights");
  SD_REQUIRE(cfg->n_layers > 0 && cfg->d_model > 0 && cfg->n_heads > 0 && cfg->n_kv_heads > 0 &&
                 cfg->head_dim > 0 && cfg->d_ff > 0 && cfg->vocab > 0 && cfg->max_pos > 0,
             "model_create: non-positive dimension");
  SD_REQUIRE(cfg->d_model % 8 == 0 && cfg->d_ff % 8 == 0 && (cfg->n_heads * cfg->head_dim) % 8 == 0,
             "model_create: d_model, d_ff and Hq*D must be multiples of 8");
  SD_REQUIRE(cfg->head_dim % 2 == 0 && cfg->n_heads % cfg->n_kv_heads == 0, "model_create: head layout");
  // the kernels' argument blocks carry these in 8-bit fields (GemvArgs / AttnArgs), and the attention kernel is instantiated
  // for these head sizes only: a direct C caller gets an error, not a truncated geometry
  SD_REQUIRE(cfg->n_heads <= 255 && cfg->n_kv_heads <= 255, "model_create: at most 255 heads (got %d / %d kv)", cfg->n_heads, cfg->n_kv_heads);
  SD_REQUIRE(cfg->head_dim == 32 || cfg->head_dim == 64 || cfg->head_dim == 128, "model_create: head_dim %d (32, 64 or 128)", cfg->head_dim);
  SD_REQUIRE(cfg->tok_emb && cfg->lm_head && cfg->final_norm_w && cfg->layers, "model_create: NULL weights");
  if (cfg->arch == SD_ARCH_LLAMA) SD_REQUIRE(cfg->rope_cos && cfg->rope_sin, "model_create: Llama needs rope tables");
  if (cfg->arch == SD_ARCH_GPT2) SD_REQUIRE(cfg->pos_emb && cfg->final_norm_b, "model_create: GPT-2 needs pos_emb and ln_f bias");
  sd_model* m = new (std::nothrow) sd_model();
  SD_REQUIRE(m, "model_create: out of memory");
  m->cfg = *cfg;
  m->layers.assign(cfg->layers, cfg->layers + cfg->n_layers);
  m->cfg.layers = m->layers.data();
  for (int l = 0; l < cfg->n_layers; ++l) {
    const sd_layer_weights& w = m->layers[l];
    if (!(w.attn_norm_w && w.wqkv && w.wo && w.mlp_norm_w && w.w_up && w.w_down)) {
      delete m;
      SD_REQUIRE(false, "model_create: layer %d has NULL weights", l);
    }
  }
  {
    // 64-token passes need every matrix of the model to be a shape gemm_skinny.hip covers
    const sd_model_config& c = m->cfg;
    const int HqD = c.n_heads * c.head_dim;
    const bool w8 = cfg->weight_dtype == SD_FP8_E4M3;
    auto covers = [&](int T) {
      for (int i = 0; i < 5; ++i)
        if (!gemm_skinny_covers(T, matrix_shape(c, i).n_pairs, matrix_shape(c, i).K, w8)) return false;
      return true;
    };
    // the most tokens every matrix of the model can take in one pass: 128, 64 (x chunks of a pass must fit the LDS) ...
    int cover_t = 0;
    for (int T = kSkinnyMaxT; T >= 16 && !cover_t; T >>= 1)
      if (covers(T)) cover_t = T;
    const bool ok = cover_t != 0;
    const char* env = getenv(debug_env::kMaxPassTokens);  // testing knob: 9 forces the small-T kernel everywhere
    int want = env ? atoi(env) : cover_t;
    if (want > cover_t) want = cover_t;
    int kmax = c.d_model > HqD ? c.d_model : HqD;
    if (c.d_ff > kmax) kmax = c.d_ff;
    m->small_t = gemv_max_tokens(kmax);  // e.g. 5 for d_ff = 14336: x rows must fit the CU's LDS
    if (want < m->small_t) want = m->small_t;
    m->max_t = ok ? want : m->small_t;
  }
  if (cfg->weight_dtype == SD_FP8_E4M3) {
    // every matrix must split into whole 64-k steps per K slice
    for (int i = 0; i < 5; ++i) {
      const MatShape sh = matrix_shape(m->cfg, i);
      const GemvGeom q = gemv_geometry(sh.n_pairs, sh.K);
      if (sh.K % 64 != 0 || q.kw % 64 != 0 || q.kw * q.ksplit != sh.K) {
        delete m;
        SD_REQUIRE(false, "model_create: fp8 storage does not cover a matrix with K=%d (K slice %d)", sh.K, q.kw);
      }
    }
  }
  if (cfg->packed) {
    const char* base = static_cast<const char*>(cfg->packed);
    for (int i = 0; i <= 4 * cfg->n_layers; ++i) {
      m->packed.push_back(base + packed_offset(m->cfg, i));
      const MatShape sh = matrix_shape(m->cfg, matrix_which(m->cfg, i));
      if (cfg->weight_dtype == SD_FP8_E4M3)   // the fp32 row scales follow the packed bytes
        m->scales.push_back(reinterpret_cast<const float*>(base + packed_offset(m->cfg, i) + packed_fp8_weight_bytes(sh.n_pairs, sh.K)));
    }
  }
  *out = m;
  return 0;
}

extern "C" int sd_model_destroy(sd_model* m) {
  delete m;
  return 0;
}

extern "C" int sd_model_set_w12(sd_model* m, const void* w12, const uint32_t* n_wide, unsigned classes) {
  clear_error();
  SD_REQUIRE(m, "model_set_w12: NULL model");
  m->w12.clear();
  if (!w12) return 0;   // back to the bf16 streams
  return model_add_w12(m, w12, n_wide, classes, W12_CODES);
}

extern "C" int sd_model_set_w12_form(sd_model* m, const void* w12, const uint32_t* n_wide, unsigned classes, int form) {
  clear_error();
  SD_REQUIRE(m, "model_set_w12_form: NULL model");
  return model_add_w12(m, w12, n_wide, classes, form);
}

extern "C" int sd_model_pass_tokens(const sd_model* m) { return m ? m->max_t : 0; }

extern "C" size_t sd_model_workspace_bytes(const sd_model* m) { return m ? workspace_layout(m->cfg).bytes : 0; }

extern "C" size_t sd_model_kv_bytes(const sd_model* m, int B, int Lmax) {
  if (!m || B <= 0 || Lmax <= 0) return 0;
  return static_cast<size_t>(m->cfg.n_layers) * B * m->cfg.n_kv_heads * Lmax * m->cfg.head_dim * 2;
}

extern "C" int sd_model_bind(sd_model* m, void* k_cache, void* v_cache, int B, int Lmax, void* workspace,
                             size_t workspace_bytes_) {
  clear_error();
  SD_REQUIRE(m && k_cache && v_cache && workspace, "model_bind: NULL argument");
  SD_REQUIRE(B >= 1 && Lmax >= 1, "model_bind: B=%d Lmax=%d", B, Lmax);
  SD_REQUIRE(workspace_bytes_ >= workspace_layout(m->cfg).bytes, "model_bind: workspace too small");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(k_cache) & 15) == 0 && (reinterpret_cast<uintptr_t>(v_cache) & 15) == 0,
             "model_bind: caches must be 16-byte aligned");
  return bind_caches(m, k_cache, v_cache, B, Lmax, nullptr, 0, 0, 0, workspace);
}

extern "C" size_t sd_model_kv_pool_bytes(const sd_model* m, int n_pages, int page_len) {
  if (!m || n_pages <= 0 || page_len <= 0) return 0;
  return static_cast<size_t>(m->cfg.n_layers) * n_pages * m->cfg.n_kv_heads * page_len * m->cfg.head_dim * 2;
}

// Paged KV: rows do not own Lmax positions each; they own pages of page_len positions out of a pool shared by all
// rows, through a caller-maintained table (the counterpart of the reference's cache manager growing / realigning
// per-sequence tensors, kv_cache_manager.py:194-199, :353-479 — here a row grows by a table entry).
extern "C" int sd_model_bind_paged(sd_model* m, void* k_pool, void* v_pool, int n_pages, int page_len, const int32_t* block_table,
                                   int max_pages_per_row, int B, void* workspace, size_t workspace_bytes_) {
  clear_error();
  SD_REQUIRE(m && k_pool && v_pool && block_table && workspace, "model_bind_paged: NULL argument");
  SD_REQUIRE(B >= 1 && n_pages >= 1 && max_pages_per_row >= 1, "model_bind_paged: B=%d pages=%d max_pages=%d", B, n_pages, max_pages_per_row);
  int shift = 0;
  while ((1 << shift) < page_len) ++shift;
  SD_REQUIRE((1 << shift) == page_len && page_len >= 32 && page_len <= 65536, "model_bind_paged: page_len %d must be a power of two >= 32", page_len);
  SD_REQUIRE(workspace_bytes_ >= workspace_layout(m->cfg).bytes, "model_bind_paged: workspace too small");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(k_pool) & 15) == 0 && (reinterpret_cast<uintptr_t>(v_pool) & 15) == 0,
             "model_bind_paged: pools must be 16-byte aligned");
  return bind_caches(m, k_pool, v_pool, B, max_pages_per_row * page_len, block_table, shift, max_pages_per_row, n_pages, workspace);
}

// ---- KV shared between cache rows (csrc/kv_fork.hip) -----------------------------------------------------------------
// Both entries check the arguments that need no model first, then the model, then the indices against its geometry:
// nothing is enqueued unless every check passed.
extern "C" int sd_model_kv_fork(sd_model* m, int src_row, const int32_t* dst_rows, int n_dst, int n_pos, void* stream) {
  clear_error();
  SD_REQUIRE(n_dst >= 0, "kv_fork: n_dst=%d", n_dst);
  SD_REQUIRE(n_dst == 0 || dst_rows, "kv_fork: NULL dst_rows with n_dst=%d", n_dst);
  SD_REQUIRE(n_pos >= 0, "kv_fork: n_pos=%d is negative", n_pos);
  SD_REQUIRE(src_row >= 0, "kv_fork: src_row %d is negative", src_row);
  for (int i = 0; i < n_dst; ++i) {
    SD_REQUIRE(dst_rows[i] >= 0, "kv_fork: destination row %d is negative", dst_rows[i]);
    SD_REQUIRE(dst_rows[i] != src_row, "kv_fork: destination row %d is the source row", dst_rows[i]);
  }
  SD_REQUIRE(m, "kv_fork: NULL model");
  SD_REQUIRE(m->k_cache && m->x, "kv_fork: model not bound (sd_model_bind)");
  SD_REQUIRE(!m->block_table, "kv_fork: this model is bound to a paged cache (rows share pages: sd_model_kv_copy_pages)");
  SD_REQUIRE(src_row < m->B, "kv_fork: src_row %d outside the bound batch of %d", src_row, m->B);
  SD_REQUIRE(n_pos <= m->Lmax, "kv_fork: n_pos=%d exceeds Lmax=%d", n_pos, m->Lmax);
  std::vector<char> seen(static_cast<size_t>(m->B), 0);
  for (int i = 0; i < n_dst; ++i) {
    SD_REQUIRE(dst_rows[i] < m->B, "kv_fork: destination row %d outside the bound batch of %d", dst_rows[i], m->B);
    SD_REQUIRE(!seen[dst_rows[i]], "kv_fork: destination row %d is listed twice", dst_rows[i]);
    seen[dst_rows[i]] = 1;
  }
  if (n_dst == 0 || n_pos == 0) return 0;
  const sd_model_config& c = m->cfg;
  return launch_kv_fork(m->k_cache, m->v_cache, c.n_layers, m->B, c.n_kv_heads, m->Lmax, c.head_dim, &src_row, dst_rows, 1, n_dst,
                        n_pos, static_cast<hipStream_t>(stream));
}

extern "C" int sd_model_kv_copy_pages(sd_model* m, const int32_t* src_pages, const int32_t* dst_pages, int n_pairs, int n_pos,
                                      void* stream) {
  clear_error();
  SD_REQUIRE(n_pairs >= 0, "kv_copy_pages: n_pairs=%d", n_pairs);
  SD_REQUIRE(n_pairs == 0 || (src_pages && dst_pages), "kv_copy_pages: NULL page list with n_pairs=%d", n_pairs);
  SD_REQUIRE(n_pos >= 0, "kv_copy_pages: n_pos=%d is negative", n_pos);
  for (int i = 0; i < n_pairs; ++i) {
    SD_REQUIRE(src_pages[i] >= 0 && dst_pages[i] >= 0, "kv_copy_pages: pair %d (%d -> %d) has a negative page index", i, src_pages[i],
               dst_pages[i]);
    SD_REQUIRE(src_pages[i] != dst_pages[i], "kv_copy_pages: pair %d copies page %d onto itself", i, src_pages[i]);
  }
  SD_REQUIRE(m, "kv_copy_pages: NULL model");
  SD_REQUIRE(m->k_cache && m->x, "kv_copy_pages: model not bound (sd_model_bind_paged)");
  SD_REQUIRE(m->block_table, "kv_copy_pages: this model is bound to a dense cache (sd_model_kv_fork)");
  const int page_len = 1 << m->page_shift;
  SD_REQUIRE(n_pos <= page_len, "kv_copy_pages: n_pos=%d exceeds page_len=%d", n_pos, page_len);
  // the pairs of a call run concurrently: a destination must not be a source or another pair's destination
  std::vector<char> role(static_cast<size_t>(m->n_pages), 0);   // 1 = source, 2 = destination
  for (int i = 0; i < n_pairs; ++i) {
    SD_REQUIRE(src_pages[i] < m->n_pages && dst_pages[i] < m->n_pages, "kv_copy_pages: pair %d (%d -> %d) outside the pool of %d pages", i,
               src_pages[i], dst_pages[i], m->n_pages);
    role[src_pages[i]] |= 1;
  }
  for (int i = 0; i < n_pairs; ++i) {
    SD_REQUIRE(role[dst_pages[i]] == 0, "kv_copy_pages: destination page %d is %s", dst_pages[i],
               (role[dst_pages[i]] & 2) ? "listed twice" : "also a source of this call");
    role[dst_pages[i]] |= 2;
  }
  if (n_pairs == 0 || n_pos == 0) return 0;
  const sd_model_config& c = m->cfg;
  return launch_kv_fork(m->k_cache, m->v_cache, c.n_layers, m->n_pages, c.n_kv_heads, page_len, c.head_dim, src_pages, dst_pages, n_pairs,
                        1, n_pos, static_cast<hipStream_t>(stream));
}

// ---- KV eviction inside one cache row (csrc/kv_evict.hip): the arguments that need no model, then the model, then its geometry
extern "C" int sd_model_kv_evict(sd_model* m, int row, int keep, int drop, int n_pos, void* stream) {
  clear_error();
  SD_REQUIRE(row >= 0, "kv_evict: row %d is negative", row);
  SD_REQUIRE(keep >= 0, "kv_evict: keep=%d is negative", keep);
  SD_REQUIRE(drop >= 1 && drop % 8 == 0, "kv_evict: drop=%d must be a positive multiple of 8", drop);
  SD_REQUIRE(static_cast<int64_t>(keep) + drop <= n_pos, "kv_evict: keep=%d + drop=%d exceed n_pos=%d", keep, drop, n_pos);
  SD_REQUIRE(m, "kv_evict: NULL model");
  SD_REQUIRE(m->k_cache && m->x, "kv_evict: model not bound (sd_model_bind)");
  SD_REQUIRE(!m->block_table, "kv_evict: this model is bound to a paged cache (eviction covers dense caches)");
  const sd_model_config& c = m->cfg;
  SD_REQUIRE(c.arch == SD_ARCH_LLAMA, "kv_evict: a GPT-2 model has learned positions in its hidden states: nothing to re-rotate");
  SD_REQUIRE(row < m->B, "kv_evict: row %d outside the bound batch of %d", row, m->B);
  SD_REQUIRE(drop < c.max_pos, "kv_evict: drop=%d is outside the model's %d rope positions", drop, c.max_pos);
  SD_REQUIRE(n_pos <= m->Lmax, "kv_evict: n_pos=%d exceeds Lmax=%d", n_pos, m->Lmax);
  if (n_pos == keep + drop) return 0;
  return launch_kv_evict(m->k_cache, m->v_cache, c.rope_cos, c.rope_sin, c.n_layers, m->B, c.n_kv_heads, m->Lmax, c.head_dim, row, keep,
                         drop, n_pos, static_cast<hipStream_t>(stream));
}

extern "C" int sd_model_set_persist_tokens(sd_model* m, int max_tokens) {
  clear_error();
  SD_REQUIRE(m && m->x, "set_persist_tokens: NULL argument / model not bound");
  SD_REQUIRE(max_tokens >= 0, "set_persist_tokens: max_tokens=%d", max_tokens);
  m->persist_t = max_tokens < m->persist_cap ? max_tokens : m->persist_cap;
  return 0;
}

extern "C" int sd_model_persist_tokens(const sd_model* m) { return m ? m->persist_t : 0; }

extern "C" int sd_model_set_length_hint(sd_model* m, int max_len) {
  clear_error();
  SD_REQUIRE(m && m->x, "set_length_hint: NULL argument / model not bound");
  m->len_hint = (max_len <= 0 || max_len > m->Lmax) ? m->Lmax : max_len;
  return 0;
}

extern "C" int sd_model_set_persist_taps(sd_model* m, int enable) {
  clear_error();
  SD_REQUIRE(m, "set_persist_taps: NULL model");
  m->persist_taps = enable != 0;
  return 0;
}

extern "C" int sd_model_persist_active(const sd_model* m, int T) {
  // 1 when a pass of T tokens of one row would run as the persistent launch right now (tokens, length hint, paging)
  return (m && T >= 1 && sd::persist_pass_ok(m, T, 1, T)) ? 1 : 0;
}

extern "C" int sd_prefill_backend_available(int backend) {
  if (backend == SD_PREFILL_ROCBLAS) return prefill_gemm_library_present() ? 1 : 0;
  return (backend == SD_PREFILL_AUTO || backend == SD_PREFILL_PASSES || backend == SD_PREFILL_NATIVE) ? 1 : 0;
}

extern "C" int sd_model_set_prefill_backend(sd_model* m, int backend) {
  clear_error();
  SD_REQUIRE(m, "set_prefill_backend: NULL model");
  SD_REQUIRE(backend >= SD_PREFILL_AUTO && backend <= SD_PREFILL_NATIVE, "set_prefill_backend: unknown backend %d", backend);
  const bool gpt2 = m->cfg.arch == SD_ARCH_GPT2;
  if (backend == SD_PREFILL_ROCBLAS) {
    SD_REQUIRE(!gpt2, "set_prefill_backend: rocBLAS prefill serves Llama models only (this model is GPT-2)");
    SD_REQUIRE(!m->w8() && m->cfg.weight_dtype == SD_BF16,
               "set_prefill_backend: rocBLAS prefill multiplies the bf16 HF-layout weights, not this model's fp8 storage");
    SD_REQUIRE(!m->block_table, "set_prefill_backend: rocBLAS prefill serves dense KV only (this model is bound to a paged cache)");
    SD_REQUIRE(prefill_gemm_available(), "set_prefill_backend: rocBLAS could not be opened");
  } else if (backend == SD_PREFILL_NATIVE) {
    const char* why = prefill_native_refusal(m->cfg, m->is_packed() != 0);
    SD_REQUIRE(!why, "set_prefill_backend: %s", why);
  }
  m->prefill_backend = backend;
  return 0;
}

extern "C" int sd_model_prefill_backend(const sd_model* m) { return m ? m->prefill_backend : -1; }

extern "C" int64_t sd_model_prefill_count(const sd_model* m, int backend) {
  if (!m || backend < SD_PREFILL_PASSES || backend > SD_PREFILL_NATIVE) return -1;
  return m->prefill_count[backend];
}

extern "C" const uint32_t* sd_model_status_word(const sd_model* m) { return m ? m->host_status : nullptr; }

extern "C" int sd_model_engine_status(sd_model* m, uint32_t* status_out, void* stream) {
  clear_error();
  SD_REQUIRE(m && status_out, "engine_status: NULL argument");
  *status_out = 0;
  if (!m->p_sync) return 0;
  SD_HIP_CHECK(hipMemcpyAsync(status_out, m->p_sync + 1, 4, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  SD_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int sd_model_engine_status_clear(sd_model* m, void* stream) {
  clear_error();
  SD_REQUIRE(m, "engine_status_clear: NULL argument");
  if (!m->p_sync) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SD_HIP_CHECK(hipStreamSynchronize(st));   // every workgroup of a failed launch has left
  unsigned w[2] = {0u, 0u};
  SD_HIP_CHECK(hipMemcpy(w, m->p_sync, 8, hipMemcpyDeviceToHost));
  // past the failed launch's tags (it did not advance the counter): granules it left behind can never match again
  w[0] = (w[0] + 2u) & 0x7fffffu;
  w[1] = 0u;
  SD_HIP_CHECK(hipMemcpy(m->p_sync, w, 8, hipMemcpyHostToDevice));
  if (m->host_status) *m->host_status = 0u;
  return 0;
}

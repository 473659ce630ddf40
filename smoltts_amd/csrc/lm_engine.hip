// DualAR engine: orchestrates the kernels into prefill / frame-decode launch sequences.
//
// One frame == one SingleBatchGenerator.__next__ of the reference (lm/generate.py:59-171) for every
// slot of the session at once:  slow transformer step (forward_generate, lm/rq_transformer.py:173-192)
// -> argmax -> n_fast depth-transformer steps with a per-frame KV cache (forward_generate_fast :194-220,
// generate.py:110-141) -> commit of the (1 + n_fast)-high column.  Sampling, the column feedback, the
// stop rule and the position counters all live on the device, so a frame is a fixed launch sequence that
// is captured once into a hipGraph and replayed (the reference synchronises with the host 9x per frame).
//
// Dataflow between kernels (x3.h): the residual stream x stays fp32; whoever produces x also publishes
// it as the bf16x3 operand of the next GEMM (times that GEMM's RMSNorm weight) plus partial sums of
// squares, so each transformer block is exactly five launches:
//   wqkv GEMM (+RMSNorm scale, RoPE, KV write) -> attention (writes wo's operand) -> wo GEMM (+residual,
//   publishes w1|w3's operand) -> w1|w3 GEMM (+RMSNorm scale, SwiGLU, writes w2's operand) -> w2 GEMM
//   (+residual, publishes the next block's / head's operand).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "argmax_dev.h"
#include "embed_dev.h"

using namespace smoltts;

struct SmolttsEngine {
  SmolttsLMConfig cfg;
  SmolttsLMWeights w;
  const char* arena;
  size_t arena_bytes;
  // derived table (smoltts_engine_build_fast_qkv; caller-owned memory): q | k | v of depth layer 0 for every row of the fast
  // embedding table, before RoPE -- [fast_emb_rows][(fast heads + 2 fast kv heads) * 64] fp32; nullptr = not built
  const float* fast_qkv;
};

constexpr int STAGE_RING = 8;
constexpr int GRAPH_FORMS = 64;  // the values of SmolttsSession.form (pick_form)
// the bits of a form (form_of), and of h_form[b]: what slot b asks for -- its slow token / its depth codes sampled, its filter entry
// on, its length entry on, its slow token scored, its alignment window on
constexpr int FORM_SLOW = 1, FORM_FAST = 2, FORM_FILTER = 4, FORM_LENGTH = 8, FORM_SCORE = 16, FORM_ALIGN = 32;
// the captured graphs of a form: one decode frame (slow step + tail); the tail alone (slow head + depth steps + commit) as run after
// a prefill; `multi_frames` consecutive decode frames in one graph (fewer graph launches per tick / chunk)
enum GraphKind { GRAPH_FRAME, GRAPH_TAIL, GRAPH_MULTI, GRAPH_KINDS };

// STAGE_RING pinned host areas of `area` bytes each, used in turn as the source of async copies; ev[k] is recorded behind the copies
// out of area k, and the host waits for it before it writes that area again (ring_create / _destroy / _take / _sent)
struct PinnedRing {
  char* base;
  size_t area;
  hipEvent_t ev[STAGE_RING];
  bool live[STAGE_RING];
  int next;
};

struct SmolttsSession {
  SmolttsEngine* e;
  int B, max_seq, max_rows, max_frames;
  int stop_on_eos;
  float temp, fast_temp, min_p;  // <= 0: greedy (lm/generate.py:88-99,118-132)
  uint64_t seed;
  // activations
  float *xr, *qr;            // prefill rows: fp32 residual stream [max_rows][dim], q [max_rows][Hq*64]
  float *xt, *xf;            // decode/tail rows: [B][dim], [B][fast_dim]
  float* qt;                 // [B][max(Hq, fast Hq)*64]
  char *x3n, *x3n2, *x3a, *x3h;  // X3 operands: normed stream (2 consumers), attention out, SwiGLU out
  float* ssq;                // [rows][dim/16] partial sums of squares of the stream
  // side workspace of smoltts_lm_prefill_side (prompt rows of NEW tenants beside the decode frames of the others): a second set
  // of everything the slow layers write that is not a KV-cache row
  float *sd_xr, *sd_qr;
  char *sd_x3n, *sd_x3a, *sd_x3h;
  float* sd_ssq;
  float* logits;             // [B][max(vocab, codebook)]: the depth heads' rows
  float* logits_slow;        // [B][vocab]: the slow head's rows (picked by the commit kernel at the end of the frame)
  // caches
  char *kc, *vc;             // [n_layer][B][KV][max_seq][64] in fp32 or bf16 (kv_format)
  int kv_format;
  float *fkc, *fvc;          // [n_fast_layer][B][FKV][n_fast][64]
  // integer state
  int *cur_col, *new_col;    // [B][1+n_fast]
  int *pos, *frames, *done, *mask, *iota, *fastpos;  // [B] each; fastpos [n_fast][B]
  int* salt;                   // [B] tenants a slot has had: mixed into the sampling seed
  int *stage_slots, *stage_last;                     // [B]
  float* margin;             // [B]
  float* attn_part;          // key-split slow attention: partial records (ATT_SPLIT_PART_FLOATS)
  int* attn_ticket;          // ... and arrival tickets [ATT_SPLIT_MAX_PAIRS]: zeroed at creation and again by every commit kernel (end of frame)
  int* margin_at;            // [B] frame * 64 + step of the slot's smallest top-2 gap
  int* codes;                // [B][max_frames][1+n_fast]
  PinnedRing stage_ring;       // host staging of the prefill calls' lists (stage_upload): areas of 2*B ints
  // captured graphs, one set per form (pick_form; index 0 outside slot mode), each created when first needed; null = not built
  hipGraphExec_t graphs[GRAPH_KINDS][GRAPH_FORMS];
  int form;                       // the form the next launches are built / replayed in (pick_form)
  // slot mode (smoltts_session_set_slot_sampling): per-slot sampling entries
  bool slot_mode;
  SmolttsSlotSampling* slot_tab;      // [B] read by the picks; null until slot mode
  SmolttsSlotSampling* slot_tab_area; // where it is carved (the slab's tail): [B] table, [B] upload entries, [B] upload slots
  uint8_t* h_form;                    // [B] host mirror of every per-slot table, as FORM_* bits: chooses the graph form
  PinnedRing slot_ring;               // host staging of the table uploads (upload_slot_entries): areas of B entries + B slots of the largest entry
  // ... and per-slot filter entries (smoltts_session_set_slot_filters)
  SmolttsSlotFilters* filt_tab;       // [B] read by the sampled picks of slot mode; all zero = off
  SmolttsSlotFilters* filt_tab_area;  // [B] table, [B] upload entries, [B] upload slots
  // ... and per-slot length entries (smoltts_session_set_slot_length)
  SmolttsSlotLength* len_tab;         // [B] read by the slow picks of slot mode (greedy and sampled); all zero = off
  SmolttsSlotLength* len_tab_area;    // [B] table, [B] upload entries, [B] upload slots
  // ... and per-slot score flags (smoltts_session_set_slot_score): host only (FORM_SCORE of h_form).  In a form with that bit every
  // row's slow pick is scored and the host reads the slots it asked about.
  float* logprob;                     // [B][max_frames]: the log-probability of each emitted slow id, written by the scored forms
  // ... and per-slot alignment windows (smoltts_session_set_slot_align) for the chosen (layer, head) pairs
  // (smoltts_session_set_align_heads).  Table, upload area and rows live in the caller's buffer, not in the slab.
  int n_align;                        // chosen pairs, sorted by layer; 0 = off
  int align_layer[SMOLTTS_MAX_ALIGN_HEADS], align_head[SMOLTTS_MAX_ALIGN_HEADS];
  int* align_win;                     // [B][2] (t0, t1) read by attn_align_kernel; t1 <= t0 = off
  int* align_up;                      // upload area: [B][2] entries, [B] slots
  float* align_out;                   // [B][max_frames][n_align][2] (m, s1); m = -1: not measured
  int flight_limit;            // SMOLTTS_MAX_FRAMES_IN_FLIGHT as read at creation (0 = unbounded)
  int multi_frames;            // frames per multi-frame graph (1 = single-frame graphs only): SMOLTTS_FRAMES_PER_GRAPH, else
                               // smoltts_session_set_frames_per_graph, else min(n_frames, 4) of the largest decode call so far
  bool multi_fixed;            // set by the environment or the API: decode calls do not change it
  bool multi_env;              // set by SMOLTTS_FRAMES_PER_GRAPH: the API does not change it either
  bool prefilled;
  // bounded run-ahead of the host over the GPU (smoltts_lm_decode): an event every `flight_group` frame graphs, the host
  // waits for the one recorded two groups ago before it launches further
  hipEvent_t flight_ev[2];
  bool flight_live[2];
  int flight_cur, flight_count, flight_group;
  // measurement aid of THIS session (smoltts_session_measure_duplicate): launches of one kernel class are issued twice
  int dup_code, dup_n;
  bool use_qkv_table;          // depth layer-0 q | k | v from the engine's table where it exists (SMOLTTS_OPT_QKV_TABLE)
  bool commit_picks;           // slow token and last depth code picked inside the commit kernel (SMOLTTS_OPT_COMMIT_PICKS)
  bool split_attn;             // slow attention of few rows over two workgroups per (row, kv head) (SMOLTTS_OPT_SPLIT_ATTN)
  int stream_w;                // which weights of a decode frame are loaded with the non-temporal hint (SMOLTTS_OPT_STREAM_W, bit mask)
  bool fuse_depth_attn;        // depth attention worked out inside the wo launch (SMOLTTS_OPT_FUSE_DEPTH_ATTN)
  bool fp8_prefill;            // prompt rows (M >= 256) of an fp8 engine on the fp8 x fp8 MFMA (SMOLTTS_OPT_FP8_PREFILL; not the parity path)
  bool fuse_pick;              // greedy depth codes picked inside the next step's layer-0 attention + wo launch (SMOLTTS_OPT_FUSE_PICK)
  float* cand;                 // [B][codebook_size / 16][4]: the depth head GEMM's tile candidates for that pick
  float* cand_slow;            // [B][vocab_size / 16][4]: the slow head GEMM's, for the commit kernel's greedy pick
};

namespace {

int imax(int a, int b) { return a > b ? a : b; }

size_t carve(SmolttsSession* s, char* base) {
  const SmolttsLMConfig& c = s->e->cfg;
  Carver cv{base, 0};
  const size_t B = s->B, R = s->max_rows, H = 1 + c.n_fast;
  const size_t R16 = (R + 15) / 16 * 16, B16 = (B + 15) / 16 * 16;
  const size_t dq = (size_t)imax(c.n_head, c.fast_n_head) * 64;
  const size_t dmax = imax(c.dim, c.fast_dim), imx = imax(c.inter, c.fast_inter);
  s->xr = cv.take<float>(R * c.dim);
  s->qr = cv.take<float>(R * c.n_head * 64);
  s->xt = cv.take<float>(B * c.dim);
  s->xf = cv.take<float>(B * c.fast_dim);
  s->qt = cv.take<float>(B * dq);
  s->x3n = cv.take<char>(R16 * dmax * 6);
  s->x3n2 = cv.take<char>(B16 * dmax * 6);
  s->x3a = cv.take<char>(R16 * dmax * 6);
  s->x3h = cv.take<char>(R16 * imx * 6);
  s->ssq = cv.take<float>(R16 * (dmax / 16));
  s->sd_xr = cv.take<float>(R * c.dim);
  s->sd_qr = cv.take<float>(R * c.n_head * 64);
  s->sd_x3n = cv.take<char>(R16 * (size_t)c.dim * 6);
  s->sd_x3a = cv.take<char>(R16 * (size_t)c.dim * 6);
  s->sd_x3h = cv.take<char>(R16 * (size_t)c.inter * 6);
  s->sd_ssq = cv.take<float>(R16 * (c.dim / 16));
  s->logits = cv.take<float>(B * (size_t)imax(c.vocab_size, c.codebook_size));
  s->logits_slow = cv.take<float>(B * (size_t)c.vocab_size);
  s->cand = cv.take<float>(B * (size_t)((c.codebook_size + 15) / 16) * 4);
  s->cand_slow = cv.take<float>(B * (size_t)((c.vocab_size + 15) / 16) * 4);
  const size_t kv = (size_t)c.n_layer * B * c.n_kv_head * s->max_seq * 64 * (s->kv_format == SMOLTTS_KV_BF16 ? 2 : 4);
  s->kc = cv.take<char>(kv);
  s->vc = cv.take<char>(kv);
  const size_t fkv = (size_t)c.n_fast_layer * B * c.fast_n_kv_head * c.n_fast * 64;
  s->fkc = cv.take<float>(fkv);
  s->fvc = cv.take<float>(fkv);
  s->cur_col = cv.take<int>(B * H);
  s->new_col = cv.take<int>(B * H);
  s->pos = cv.take<int>(B);
  s->frames = cv.take<int>(B);
  s->salt = cv.take<int>(B);
  s->done = cv.take<int>(B);
  s->mask = cv.take<int>(B);
  s->iota = cv.take<int>(B);
  s->fastpos = cv.take<int>((size_t)c.n_fast * B);
  s->stage_slots = cv.take<int>(B);
  s->stage_last = cv.take<int>(B);
  s->margin = cv.take<float>(B);
  s->attn_part = cv.take<float>(ATT_SPLIT_PART_FLOATS);
  s->attn_ticket = cv.take<int>(ATT_SPLIT_MAX_PAIRS);
  s->margin_at = cv.take<int>(B);
  s->codes = cv.take<int>(B * (size_t)s->max_frames * H);
  s->logprob = cv.take<float>(B * (size_t)s->max_frames);
  // slot mode only (smoltts_session_set_slot_sampling): the table, then the upload area (B entries, B slot numbers) -- the
  // tail of the slab, in use once the session enters slot mode
  s->slot_tab_area = cv.take<SmolttsSlotSampling>(2 * B + (B * sizeof(int) + sizeof(SmolttsSlotSampling) - 1) / sizeof(SmolttsSlotSampling));
  s->filt_tab_area = cv.take<SmolttsSlotFilters>(2 * B + (B * sizeof(int) + sizeof(SmolttsSlotFilters) - 1) / sizeof(SmolttsSlotFilters));
  s->len_tab_area = cv.take<SmolttsSlotLength>(2 * B + (B * sizeof(int) + sizeof(SmolttsSlotLength) - 1) / sizeof(SmolttsSlotLength));
  return cv.off;
}

__global__ void init_state_kernel(int B, int n_fast, int* iota, int* fastpos, int* pos, int* frames, int* done, int* mask,
                                  float* margin, int* margin_at, int* cur_col, int* new_col, int* salt, int* attn_ticket) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  for (int i = b; i < ATT_SPLIT_MAX_PAIRS; i += gridDim.x * blockDim.x) attn_ticket[i] = 0;
  if (b >= B) return;
  margin_at[b] = 0;
  iota[b] = b;
  for (int i = 0; i < n_fast; ++i) fastpos[i * B + b] = i;
  pos[b] = 0; frames[b] = 0; done[b] = 1; mask[b] = 0; salt[b] = 0;
  margin[b] = INFINITY;
  for (int i = 0; i <= n_fast; ++i) { cur_col[b * (1 + n_fast) + i] = 0; new_col[b * (1 + n_fast) + i] = 0; }
}

// Slot mode: table[slots[i]] = entries[i] for the n entries of one upload (distinct slots), for each of the three per-slot tables
template <typename Entry>
__global__ void slot_scatter_kernel(int n, const Entry* entries, const int* slots, Entry* table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) table[slots[i]] = entries[i];
}

// Restart the listed slots: position = prompt length, counters cleared; only they commit this frame.
__global__ void slot_reset_kernel(int B, int n_slots, const int* slots, const int* last_row, const int* row_pos, int* pos,
                                  int* frames, int* done, int* mask, float* margin, int* salt) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int hit = -1;
  for (int i = 0; i < n_slots; ++i)
    if (slots[i] == b) hit = i;
  mask[b] = hit >= 0;
  if (hit >= 0) {
    pos[b] = row_pos[last_row[hit]] + 1;
    frames[b] = 0; done[b] = 0; margin[b] = INFINITY;
    salt[b] += 1;  // a new tenant: its samples must not repeat the previous tenant's (same seed, slot and frame numbers)
  }
}

// Deferred start: the prompt's KV rows are in place; the slot is armed so that the next decode frame takes the last prompt
// column as its slow-step input at that column's position and emits frame 0 in its own tail (no separate tail launch).
__global__ void slot_start_kernel(int B, int H, int n_slots, const int* slots, const int* last_row, const int* row_pos,
                                  const int* grid, int* pos, int* frames, int* done, float* margin, int* cur_col, int* salt) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < n_slots; ++i)
    if (slots[i] == b) {
      const int lr = last_row[i];
      pos[b] = row_pos[lr];
      frames[b] = 0; done[b] = 0; margin[b] = INFINITY;
      salt[b] += 1;
      for (int k = 0; k < H; ++k) cur_col[b * H + k] = grid[(long)lr * H + k];
    }
}

// Chunked prefill: the listed slots stay idle (done, masked) and their position counter is parked just
// behind the chunk, where the idle slot's decode rows may scribble without harm (the next chunk rewrites
// that cache row before any attention reads it).
__global__ void slot_park_kernel(int B, int n_slots, const int* slots, const int* last_row, const int* row_pos, int* pos,
                                 int* done, int* mask) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < n_slots; ++i)
    if (slots[i] == b) { pos[b] = row_pos[last_row[i]] + 1; done[b] = 1; mask[b] = 0; }
}

// The same with the parking positions given by the host (smoltts_lm_park_slots): the slots of tenants whose prompts are about to
// be prefilled beside the running frames.
__global__ void slot_parkpos_kernel(int B, int n_slots, const int* slots, const int* where, int* pos, int* done, int* mask) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < n_slots; ++i)
    if (slots[i] == b) { pos[b] = where[i]; done[b] = 1; mask[b] = 0; }
}

// End of frame (lm/generate.py:143-171) and start of the next one, one workgroup per slot:
//  (1) commit (when `do_commit` and the slot's mask is set): publish the column, advance counters, apply the stop rule.
//      `advance_pos`: the slow step of this frame consumed one new token (decode) vs. the prompt (prefill).  A slot also
//      stops when its context is full (the next token would land at position max_seq: no KV row, no RoPE row for it) --
//      the reference's torch model has the same hard limit (max_seq_len buffers, modeling/...:180-199).
//  (2) mask = !done for the next frame (only live slots commit there);
//  (3) embed the slot's current column as the next slow step's input row (residual stream + X3 operand + sum of squares
//      for layer 0), so a decode frame starts with the first QKV GEMM: no separate mask / embed launches.
// Invariant between API calls: (xt, x3n, ssq) hold the embedded current columns of all slots and mask == !done.
struct CommitArgs {
  int B, H, max_frames, max_seq, im_end, stop_on_eos, advance_pos, do_commit;
  int* new_col;
  int *mask, *cur_col, *codes, *pos, *frames, *done;
  // the two picks nothing else in the frame waits for happen here instead of in launches of their own: the slow token
  // (lm/generate.py:88-99: only the commit needs it) and the last depth code (no further step consumes it); null = already in new_col
  const float* slow_logits; int slow_cols; SampleArgs slow_sa;
  const float* last_logits; int last_cols; SampleArgs last_sa;
  float* margin;
  // greedy picks from the head GEMMs' tile candidates (SmolttsGemm3Args.cand_out_dev) instead of the rows of logits: one wave
  // each, side by side, 2.4 KB instead of 9.5 + 8 KB per slot to look at; null = from the logits (argmax_row: sampling)
  const float* slow_cand; int slow_tiles;
  const float* last_cand; int last_tiles;
  float* logprob;    // SCORE: [B][max_frames], the slow id's log-probability beside its codes row
  int* attn_ticket;  // the key-split attention's arrival tickets: back to zero at the end of every frame, so that no history (an
                     // interrupted launch, a caller's odd count) can invert a later launch's "who arrived last" decision
};

// FILTERS: the instantiation whose picks read SampleArgs.filters (slot mode's sampled forms); LENGTH: the one whose slow pick
// reads SampleArgs.length (slot mode's forms with a length entry on).  The stop rule below sees the id the patched row gave.
// SCORE: the one whose slow pick also gives the id's log-probability (slot mode's forms in which some slot scores), stored at
// logprob[b][f] with the codes of frame f.
template <bool FILTERS, bool LENGTH, bool SCORE>
__global__ __launch_bounds__(256) void commit_embed_kernel(CommitArgs a, EmbedTables t, float* xt, EmitDev emit) {
  __shared__ int s_col[64];
  __shared__ float sh4[4];
  __shared__ ArgmaxScratch s_pick[2];
  const int b = blockIdx.x, tid = threadIdx.x, H = a.H;  // H <= 64: the whole commit happens inside wave 0, in program order
  if (b == 0 && a.attn_ticket)
    for (int i = tid; i < ATT_SPLIT_MAX_PAIRS; i += blockDim.x) a.attn_ticket[i] = 0;
  int id_slow = 0, id_last = 0;
  const bool c_slow = a.slow_logits && a.slow_cand, c_last = a.last_logits && a.last_cand;
  if (c_slow || c_last) {  // (uniform) greedy picks from tile candidates: wave 0 the slow token, wave 1 the last depth code
    __shared__ int s_id[2];
    __shared__ float s_gap[2];
    const int wave = tid >> 6, lane = tid & 63;
    if ((wave == 0 && c_slow) || (wave == 1 && c_last)) {
      const float* cand = wave == 0 ? a.slow_cand + (size_t)b * a.slow_tiles * 4 : a.last_cand + (size_t)b * a.last_tiles * 4;
      Top2 t = cand_pick_wave(cand, wave == 0 ? a.slow_tiles : a.last_tiles, lane);
      if (t.i1 < 0 || t.i1 >= (wave == 0 ? a.slow_cols : a.last_cols)) t.i1 = 0;  // all-NaN row: stay inside the tables
      if (lane == 0) { s_id[wave] = t.i1; s_gap[wave] = t.v1 - t.v2; }
    }
    __syncthreads();
    if (tid == 0 && a.margin && a.mask[b]) {  // argmax_row's gap records, in its order: the slow token's, then the last code's
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (!(k == 0 ? c_slow : c_last)) continue;
        const SampleArgs& sa = k == 0 ? a.slow_sa : a.last_sa;
        if (s_gap[k] < a.margin[b]) {
          a.margin[b] = s_gap[k];
          if (sa.margin_at) sa.margin_at[b] = (sa.frames ? sa.frames[b] : sa.frame_base + b) * 64 + sa.step;
        }
      }
    }
    if (c_slow) id_slow = s_id[0];
    if (c_last) id_last = s_id[1];
  }
  float lp_slow = 0.f;
  ScoreScratch* sc = nullptr;
  if constexpr (SCORE) {
    __shared__ ScoreScratch s_score;
    sc = &s_score;
  }
  if constexpr (FILTERS) {
    __shared__ FilterScratch s_filt[2];
    if (a.slow_logits && !c_slow) id_slow = argmax_row<true, LENGTH, SCORE>(a.slow_logits + (long)b * a.slow_cols, a.slow_cols, (a.slow_cols & 3) == 0, b, a.margin, a.mask, a.slow_sa, s_pick[0], &s_filt[0], sc, &lp_slow);
    if (a.last_logits && !c_last) id_last = argmax_row<true>(a.last_logits + (long)b * a.last_cols, a.last_cols, (a.last_cols & 3) == 0, b, a.margin, a.mask, a.last_sa, s_pick[1], &s_filt[1]);
  } else {
    if (a.slow_logits && !c_slow) id_slow = argmax_row<false, LENGTH, SCORE>(a.slow_logits + (long)b * a.slow_cols, a.slow_cols, (a.slow_cols & 3) == 0, b, a.margin, a.mask, a.slow_sa, s_pick[0], nullptr, sc, &lp_slow);
    if (a.last_logits && !c_last) id_last = argmax_row(a.last_logits + (long)b * a.last_cols, a.last_cols, (a.last_cols & 3) == 0, b, a.margin, a.mask, a.last_sa, s_pick[1]);
  }
  int f = 0;
  bool live = false;
  if (tid < 64) { f = a.frames[b]; live = a.do_commit && a.mask[b]; }
  const bool publish = live && f < a.max_frames;
  int slow_now = 0;
  if (tid < H) {
    int nv = a.new_col[b * H + tid];
    if (a.slow_logits && tid == 0) nv = id_slow;
    if (a.last_logits && tid == H - 1) nv = id_last;
    if ((a.slow_logits && tid == 0) || (a.last_logits && tid == H - 1)) a.new_col[b * H + tid] = nv;  // (the host-visible column stays whole)
    const int v = publish ? nv : a.cur_col[b * H + tid];
    s_col[tid] = v;
    if (publish) {
      a.cur_col[b * H + tid] = v;
      a.codes[((long)b * a.max_frames + f) * H + tid] = v;
      if constexpr (SCORE) {
        if (tid == 0 && a.logprob && a.slow_logits && !c_slow) a.logprob[(long)b * a.max_frames + f] = lp_slow;
      }
    }
  }
  slow_now = a.slow_logits ? id_slow : a.new_col[b * H];  // (tid 0 reads what it may just have written itself)
  if (tid == 0) {
    int d = a.done[b];
    if (live) {
      int p = a.pos[b];
      if (a.advance_pos) a.pos[b] = ++p;
      if (publish) a.frames[b] = f + 1;
      if ((a.stop_on_eos && slow_now == a.im_end) || f + 1 >= a.max_frames || p >= a.max_seq) a.done[b] = d = 1;
    }
    a.mask[b] = !d;
  }
  __syncthreads();
  embed_row(t, s_col, b, xt, emit, sh4);
}

// `fmt` = the engine's weight_format; an fp8 matrix is its tiles (N*K bytes, N % 16 == 0) followed by N row scales
SmolttsGemm3Args base3(int fmt, const void* w, const void* x3, int M, int N, int K, int epilogue) {
  SmolttsGemm3Args a;
  memset(&a, 0, sizeof(a));
  a.w_dev = w; a.x3_dev = x3; a.M = M; a.N = N; a.K = K; a.epilogue = epilogue;
  a.w_format = fmt;
  if (fmt == SMOLTTS_W_FP8) a.w_scale_dev = reinterpret_cast<const float*>(static_cast<const char*>(w) + (size_t)N * K);
  return a;
}

// Measurement aid (smoltts_session_measure_duplicate): kernel classes are named by their GEMM epilogue (+ N), or
// 100 = short-cache (depth) attention, 101 = long-cache (slow) attention.  Only idempotent launches can be doubled
// (EPI_RESID accumulates into its own input).
bool dup_hit(const SmolttsSession* s, int code, int N) { return s->dup_code == code && (s->dup_n <= 0 || s->dup_n == N); }

int launch_gemm3_m(const SmolttsSession* s, const SmolttsGemm3Args& a, hipStream_t st) {
  ST_TRY(launch_gemm3(a, st));
  if (a.epilogue != SMOLTTS_EPI_RESID && dup_hit(s, a.epilogue, a.N)) ST_TRY(launch_gemm3(a, st));
  return SMOLTTS_OK;
}

// One pre-norm block (modeling/model/rq_transformer.py:492-501) over `M` rows of the fp32 stream x (in place).
// `in_x3`/ssq: x published for the wqkv GEMM by whoever produced x; `next`: where the block publishes its output.
int run_block(const SmolttsSession* s, const SmolttsBlockWeights& bw, int dim, int n_head, int n_kv, int inter, float* x,
              float* q, int M, const int* row_pos, const int* row_slot, const float* rope, void* kc, void* vc,
              int cache_len, const char* in_x3, const EmitArgs& next, hipStream_t st, bool first_pos = false,
              int kv_format = SMOLTTS_KV_F32, int iota_pos = -1, bool qkv_done = false, int w_stream = 0,
              const SmolttsPickArgs* pick = nullptr) {
  // pick: the rows' codes of the previous depth step have not been picked yet -- this block's attention + wo launch does it
  // (q | k | v out of the table, residual = the picked embedding row: SmolttsPickArgs); implies qkv_done and the fused attention
  // w_stream: 1 = every matrix of the block, or a mask of SMOLTTS_STREAM_W_DEPTH_* bits (which of a depth block's matrices)
  // qkv_done: q and the cache rows of this block are in place already (gathered from the engine's fast_qkv table by the
  // kernel that picked the row's code): no wqkv launch
  // iota_pos >= 0: row r is slot r at that position (the depth steps): the attention kernel needs no row_pos / row_slot loads
  // first_pos: every row is at position 0 (depth step 0), so attention over its single key is the row's own V: the QKV
  // epilogue publishes V as wo's operand and the attention launch is skipped.
  const SmolttsEngine* e = s->e;
  const char* A = e->arena;
  const float eps = e->cfg.norm_eps;
  if (!qkv_done) {  // RMSNorm scale + QKV + RoPE + cache write
    SmolttsGemm3Args a = base3(e->cfg.weight_format, A + bw.wqkv, in_x3, M, (n_head + 2 * n_kv) * 64, dim, SMOLTTS_EPI_QKV_ROPE);
    a.fp8_activations = s->fp8_prefill;
    a.ssq_in_dev = s->ssq; a.eps = eps; a.out_dev = q; a.ldo = n_head * 64;
    a.rope_dev = rope; a.row_pos_dev = row_pos; a.row_slot_dev = row_slot;
    a.k_cache_dev = (float*)kc; a.v_cache_dev = (float*)vc; a.n_q_heads = n_head; a.n_kv_heads = n_kv; a.cache_len = cache_len;
    a.kv_format = kv_format; a.w_stream = (w_stream & (1 | SMOLTTS_STREAM_W_DEPTH_QKVO)) != 0;
    if (first_pos) a.v_x3_dev = s->x3a;
    ST_TRY(launch_gemm3_m(s, a, st));
  }
  // depth steps 1..: the <= 8-key attention is recomputed by every workgroup of the wo launch for its own rows (gemm3.hip
  // attn_wo_kernel): one launch less per layer
  const bool fused_attn = !first_pos && iota_pos > 0 && s->fuse_depth_attn && kv_format == SMOLTTS_KV_F32 &&
                          smoltts_gemm3_attn_fusable(n_head, n_kv, cache_len) && dim == n_head * 64;
  if (!first_pos && !fused_attn) {
    const int reps = dup_hit(s, cache_len <= 16 ? 100 : 101, 0) ? 2 : 1;
    for (int i = 0; i < reps; ++i)
      ST_TRY(launch_attention(q, kc, vc, row_pos, row_slot, M, n_head, n_kv, cache_len, 0, nullptr, s->x3a, st, kv_format, iota_pos,
                              s->split_attn ? s->attn_part : nullptr, s->attn_ticket));
  }
  {  // x += attn . Wo^T ; publish x * ffn_norm for w1|w3
    SmolttsGemm3Args a = base3(e->cfg.weight_format, A + bw.wo, s->x3a, M, dim, dim, SMOLTTS_EPI_RESID);
    a.fp8_activations = s->fp8_prefill;
    a.resid_dev = x; a.out_dev = x; a.ldo = dim;
    a.emit_a_dev = s->x3n; a.gamma_a_dev = (const float*)(A + bw.ffn_norm); a.ssq_out_dev = s->ssq; a.w_stream = (w_stream & (1 | SMOLTTS_STREAM_W_DEPTH_QKVO)) != 0;
    if (fused_attn) {
      a.attn_q_dev = q; a.attn_pos = iota_pos; a.k_cache_dev = (float*)kc; a.v_cache_dev = (float*)vc;
      a.n_q_heads = n_head; a.n_kv_heads = n_kv; a.cache_len = cache_len; a.kv_format = SMOLTTS_KV_F32;
      a.pick = pick;
    }
    ST_REQUIRE(pick == nullptr || fused_attn, SMOLTTS_E_STATE, "run_block: a pick needs the fused depth attention");
    ST_TRY(launch_gemm3(a, st));
  }
  {  // h = silu(w1 n) * (w3 n), n = RMSNorm(x); written as w2's operand
    SmolttsGemm3Args a = base3(e->cfg.weight_format, A + bw.w13, s->x3n, M, 2 * inter, dim, SMOLTTS_EPI_SWIGLU);
    a.fp8_activations = s->fp8_prefill;
    a.ssq_in_dev = s->ssq; a.eps = eps; a.x3_out_dev = s->x3h; a.w_stream = (w_stream & (1 | SMOLTTS_STREAM_W_DEPTH_W13)) != 0;
    ST_TRY(launch_gemm3_m(s, a, st));
  }
  {  // x += h . W2^T ; publish for the next consumer(s)
    SmolttsGemm3Args a = base3(e->cfg.weight_format, A + bw.w2, s->x3h, M, dim, inter, SMOLTTS_EPI_RESID);
    a.fp8_activations = s->fp8_prefill;
    a.resid_dev = x; a.out_dev = x; a.ldo = dim;
    a.emit_a_dev = next.x3a; a.gamma_a_dev = next.gamma_a; a.emit_b_dev = next.x3b; a.gamma_b_dev = next.gamma_b;
    a.ssq_out_dev = next.ssq; a.w_stream = (w_stream & (1 | SMOLTTS_STREAM_W_DEPTH_W2)) != 0;
    ST_TRY(launch_gemm3(a, st));
  }
  return SMOLTTS_OK;
}

const float* gamma_at(const SmolttsEngine* e, uint64_t off) { return (const float*)(e->arena + off); }

// What the producer of the slow hidden state publishes: head operand (x * norm) and the depth
// transformer's first operand (x * fast_layers[0].attention_norm, or raw x for fast_project_in).
EmitArgs slow_hidden_emit(const SmolttsSession* s) {
  const SmolttsEngine* e = s->e;
  EmitArgs em{s->x3n, gamma_at(e, e->w.norm), s->x3n2,
              e->cfg.has_fast_project_in ? nullptr : gamma_at(e, e->w.fast_layers[0].attn_norm), s->ssq};
  return em;
}

// xt[slots[i]] = xr[last_row[i]]
__global__ __launch_bounds__(256) void scatter_last_kernel(const float* xr, const int* slots, const int* last_row, int dim,
                                                           float* xt) {
  const int i = blockIdx.x;
  const long src = last_row[i], dst = slots[i];
  for (int d = threadIdx.x * 4; d < dim; d += 256 * 4)
    *reinterpret_cast<float4*>(xt + dst * dim + d) = *reinterpret_cast<const float4*>(xr + src * dim + d);
}

EmbedTables embed_tables(const SmolttsEngine* e) {
  const SmolttsLMConfig& c = e->cfg;
  const char* A = e->arena;
  return EmbedTables{(const uint16_t*)(A + e->w.text_emb), (const uint16_t*)(A + e->w.codebook_emb), c.dim, c.codebook_size,
                     c.duplicate_code_0 ? 0 : c.codebook_size, c.embed_mask_mode, c.semantic_start_id, c.semantic_end_id,
                     c.vocab_size, c.codebook_size * c.num_codebooks, c.n_fast};
}

// Whether some row samples its slow token / depth codes: the session-wide temperatures, or in slot mode the form of the launches
// being built (pick_form).  A part that no row samples is built exactly as the session-wide greedy one.
bool slow_sampled(const SmolttsSession* s) { return s->slot_mode ? (s->form & FORM_SLOW) != 0 : s->temp > 0.f; }
bool fast_sampled(const SmolttsSession* s) { return s->slot_mode ? (s->form & FORM_FAST) != 0 : s->fast_temp > 0.f; }
// Whether some slot's length entry is on (slot mode only): the slow pick then reads the row of logits with every row's own entries,
// as in a form whose slow token is sampled -- the head GEMM's tile candidates hold unpatched values
bool length_on(const SmolttsSession* s) { return s->slot_mode && (s->form & FORM_LENGTH) != 0; }
// Whether some slot scores its slow token (slot mode only): the slow pick then reads the row of logits, by the same rule -- the score
// sums over the whole row, which the tile candidates do not hold
bool score_on(const SmolttsSession* s) { return s->slot_mode && (s->form & FORM_SCORE) != 0; }

// The pick arguments of step 0 (slow token) / step >= 1 (depth codes).  Slot mode, sampling form: every row reads its own entry
// (a greedy row then takes the argmax inside argmax_row); greedy form: plain greedy arguments.
SampleArgs pick_args(const SmolttsSession* s, int step) {
  if (s->slot_mode) {
    const bool sampled = step == 0 ? slow_sampled(s) : fast_sampled(s);
    const bool length = step == 0 && length_on(s);
    const bool score = step == 0 && score_on(s);
    SampleArgs sa{0.f, 0.f, 0, step, 0, s->frames, nullptr, s->margin_at, sampled || length || score ? s->slot_tab : nullptr};
    if (length) { sa.length = s->len_tab; sa.im_end = s->e->cfg.im_end_id; }
    if (score) { sa.logprob = s->logprob; sa.logprob_stride = s->max_frames; }
    if (sampled && (s->form & FORM_FILTER)) {  // the filters of the sampled rows; the penalty's history: this step's column of the slot's emitted frames
      sa.filters = s->filt_tab;
      sa.hist = s->codes + step; sa.hist_slot_stride = (int64_t)s->max_frames * (1 + s->e->cfg.n_fast);
      sa.hist_frame_stride = 1 + s->e->cfg.n_fast; sa.hist_frames = s->max_frames;
    }
    return sa;
  }
  if (step == 0) return SampleArgs{s->temp, s->min_p, s->seed, 0, 0, s->frames, s->salt, s->margin_at, nullptr};
  return SampleArgs{s->fast_temp, s->fast_temp > 0.f ? s->min_p : 0.f, s->seed, step, 0, s->frames, s->salt, s->margin_at, nullptr};
}

// The commit kernel's greedy picks read the head GEMMs' tile candidates where run_tail has had them written (same conditions there)
bool commit_cand_slow(const SmolttsSession* s) { return s->commit_picks && s->fuse_pick && !slow_sampled(s) && !length_on(s) && !score_on(s) && s->B < 256; }
bool commit_cand_last(const SmolttsSession* s) { return s->commit_picks && s->fuse_pick && !fast_sampled(s) && s->B < 256; }

// commit (optional) + next-frame mask + embedding of every slot's current column (see commit_embed_kernel); `picks`: the
// frame's slow token and last depth code are still logits (run_tail) and are picked here
int launch_commit_embed(SmolttsSession* s, int do_commit, int advance_pos, hipStream_t st, bool picks = false) {
  const SmolttsEngine* e = s->e;
  const SmolttsLMConfig& c = e->cfg;
  ST_REQUIRE(1 + c.n_fast <= 64 && c.dim % 64 == 0, SMOLTTS_E_INVALID, "commit: grid height > 64 or dim %% 64 != 0");
  CommitArgs a;
  memset(&a, 0, sizeof(a));
  a.B = s->B; a.H = 1 + c.n_fast; a.max_frames = s->max_frames; a.max_seq = s->max_seq; a.im_end = c.im_end_id;
  a.stop_on_eos = s->stop_on_eos; a.advance_pos = advance_pos; a.do_commit = do_commit;
  a.new_col = s->new_col; a.mask = s->mask; a.cur_col = s->cur_col; a.codes = s->codes; a.pos = s->pos; a.frames = s->frames; a.done = s->done;
  a.margin = s->margin;
  a.attn_ticket = s->attn_ticket;
  if (picks) {
    a.logprob = s->logprob;
    a.slow_logits = s->logits_slow; a.slow_cols = c.vocab_size;
    a.slow_sa = pick_args(s, 0);
    a.last_logits = s->logits; a.last_cols = c.codebook_size;
    a.last_sa = pick_args(s, c.n_fast);
    if (commit_cand_slow(s)) { a.slow_cand = s->cand_slow; a.slow_tiles = (c.vocab_size + 15) / 16; }
    if (commit_cand_last(s)) { a.last_cand = s->cand; a.last_tiles = (c.codebook_size + 15) / 16; }
  }
  const EmitDev em{s->x3n, gamma_at(e, e->w.layers[0].attn_norm), nullptr, nullptr, s->ssq};
  const bool filters = picks && (a.slow_sa.filters || a.last_sa.filters), length = picks && a.slow_sa.length;
  const bool score = picks && a.slow_sa.logprob;
#define ST_COMMIT(F, L, S) hipLaunchKernelGGL((commit_embed_kernel<F, L, S>), dim3(s->B), dim3(256), 0, st, a, embed_tables(e), s->xt, em)
#define ST_COMMIT_S(F, L) \
  { if (score) ST_COMMIT(F, L, true); else ST_COMMIT(F, L, false); }
  if (length) {
    if (filters) ST_COMMIT_S(true, true) else ST_COMMIT_S(false, true)
  } else {
    if (filters) ST_COMMIT_S(true, false) else ST_COMMIT_S(false, false)
  }
#undef ST_COMMIT_S
#undef ST_COMMIT
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

// Slow head + the depth transformer for all B slots; columns land in new_col, commit applies `mask`.
// Precondition: xt holds the pre-norm slow hidden and has been published via slow_hidden_emit().
int run_tail(SmolttsSession* s, int advance_pos, hipStream_t st) {
  const SmolttsEngine* e = s->e;
  const SmolttsLMConfig& c = e->cfg;
  const char* A = e->arena;
  const int B = s->B, H = 1 + c.n_fast;
  {  // logits = RMSNorm(x) . E^T   (lm/rq_transformer.py:184-189); the token is picked by the commit kernel: nothing before it needs it
    SmolttsGemm3Args a = base3(c.weight_format, A + e->w.head, s->x3n, B, c.vocab_size, c.dim, SMOLTTS_EPI_STORE);
    a.ssq_in_dev = s->ssq; a.eps = c.norm_eps; a.out_dev = s->logits_slow; a.ldo = c.vocab_size; a.w_stream = (s->stream_w & SMOLTTS_STREAM_W_SLOW_HEAD) != 0;
    if (commit_cand_slow(s)) a.cand_out_dev = s->cand_slow;
    ST_TRY(launch_gemm3_m(s, a, st));
  }
  const bool picks = s->commit_picks;
  if (!picks) {  // (A/B: the pick as a launch of its own)
    const SampleArgs slow_sa = pick_args(s, 0);
    ST_TRY(launch_argmax(s->logits_slow, B, c.vocab_size, c.vocab_size, s->new_col, H, s->margin, s->mask, nullptr, 0, 0, nullptr,
                         nullptr, &slow_sa, st));
  }
  float* xf = s->xt;  // fast input = pre-norm slow hidden (lm/rq_transformer.py:191)
  const char* first_x3 = s->x3n2;
  const EmitArgs to_fast0{s->x3n, gamma_at(e, e->w.fast_layers[0].attn_norm), nullptr, nullptr, s->ssq};
  if (c.has_fast_project_in) {  // Linear(dim, fast_dim) with bias (modeling :339-342)
    SmolttsGemm3Args a = base3(c.weight_format, A + e->w.fast_proj_w, s->x3n2, B, c.fast_dim, c.dim, SMOLTTS_EPI_STORE);
    a.bias_dev = (const float*)(A + e->w.fast_proj_b); a.out_dev = s->xf; a.ldo = c.fast_dim;
    a.emit_a_dev = to_fast0.x3a; a.gamma_a_dev = to_fast0.gamma_a; a.ssq_out_dev = s->ssq;
    ST_TRY(launch_gemm3(a, st));
    xf = s->xf;
    first_x3 = s->x3n;
  }
  const size_t fl_stride = (size_t)B * c.fast_n_kv_head * c.n_fast * 64;
  const bool table = e->fast_qkv != nullptr && s->use_qkv_table;
  // greedy depth codes are picked by the launch that consumes them (the next step's layer-0 attention + wo: SmolttsPickArgs)
  const bool pick_fused = s->fuse_pick && table && s->fuse_depth_attn && !fast_sampled(s) && B < 256 && c.codebook_size % 16 == 0 &&
                          c.fast_dim == c.fast_n_head * 64 && smoltts_gemm3_attn_fusable(c.fast_n_head, c.fast_n_kv_head, c.n_fast);
  SmolttsPickArgs pk;
  memset(&pk, 0, sizeof(pk));
  bool pk_pending = false;  // step i - 1's code is still candidates in s->cand
  for (int i = 0; i < c.n_fast; ++i) {
    for (int l = 0; l < c.n_fast_layer; ++l) {
      const EmitArgs next{s->x3n,
                          gamma_at(e, l + 1 < c.n_fast_layer ? e->w.fast_layers[l + 1].attn_norm : e->w.fast_norm),
                          nullptr, nullptr, s->ssq};
      ST_TRY(run_block(s, e->w.fast_layers[l], c.fast_dim, c.fast_n_head, c.fast_n_kv_head, c.fast_inter, xf, s->qt, B,
                       s->fastpos + (size_t)i * B, s->iota, (const float*)(A + e->w.fast_rope), s->fkc + l * fl_stride,
                       s->fvc + l * fl_stride, c.n_fast, (i == 0 && l == 0) ? first_x3 : s->x3n, next, st, /*first_pos=*/i == 0,
                       SMOLTTS_KV_F32, /*iota_pos=*/i, /*qkv_done=*/table && i > 0 && l == 0,
                       /*w_stream=*/s->stream_w & (SMOLTTS_STREAM_W_DEPTH_QKVO | SMOLTTS_STREAM_W_DEPTH_W13 | SMOLTTS_STREAM_W_DEPTH_W2),
                       (pk_pending && l == 0) ? &pk : nullptr));
      if (l == 0) pk_pending = false;
    }
    {  // fast_norm + depthwise head slice i  (lm/rq_transformer.py:209-217)
      const size_t wrow = (size_t)i * e->w.fast_head_step_stride;  // rows; a row tile is 16 rows
      const size_t wbytes = c.weight_format == SMOLTTS_W_FP8 ? wrow * (c.fast_dim + 4) : wrow * c.fast_dim * 2;
      SmolttsGemm3Args a = base3(c.weight_format, A + e->w.fast_head + wbytes, s->x3n, B, c.codebook_size, c.fast_dim, SMOLTTS_EPI_STORE);
      a.ssq_in_dev = s->ssq; a.eps = c.norm_eps; a.out_dev = s->logits; a.ldo = c.codebook_size;
      a.w_stream = (s->stream_w & SMOLTTS_STREAM_W_DEPTH_HEAD) != 0;  // each head slice is read once per frame
      if (pick_fused && i + 1 < c.n_fast) a.cand_out_dev = s->cand;
      if (i + 1 == c.n_fast && commit_cand_last(s)) a.cand_out_dev = s->cand;  // (no pick is pending on the buffer at the last step)
      ST_TRY(launch_gemm3_m(s, a, st));
    }
    const SampleArgs fast_sa = pick_args(s, 1 + i);
    if (i + 1 == c.n_fast) {  // the last code has no consumer inside the frame: picked by the commit kernel
      if (!picks)
        ST_TRY(launch_argmax(s->logits, B, c.codebook_size, c.codebook_size, s->new_col + 1 + i, H, s->margin, s->mask, nullptr, 0, 0,
                             nullptr, nullptr, &fast_sa, st));
      break;
    }
    const int off = c.depthwise_wte ? (c.duplicate_code_0 ? i : i + 1) * c.codebook_size : 0;  // generate.py:136-140
    float* xnext = c.has_fast_project_in ? s->xf : s->xt;
    if (pick_fused) {  // no launch here: layer 0 of step i + 1 picks (the residual row it starts from is the embedding row itself)
      pk.cand_dev = s->cand; pk.cand_tiles = c.codebook_size / 16; pk.qkv_table_dev = e->fast_qkv;
      pk.rope_dev = (const float*)(A + e->w.fast_rope); pk.emb_dev = A + e->w.fast_emb; pk.emb_row_offset = off;
      pk.ids_dev = s->new_col + 1 + i; pk.ids_stride = H; pk.margin_dev = s->margin; pk.margin_mask_dev = s->mask;
      pk.margin_at_dev = s->margin_at; pk.frames_dev = s->frames; pk.step = 1 + i;
      pk_pending = true;
      xf = xnext;
      continue;
    }
    // the next step's layer-0 q | k | v come out of the engine's table (position i + 1) where it has been built: the row then
    // needs no X3 operand of its own, only the fp32 residual
    QkvGather qg;
    memset(&qg, 0, sizeof(qg));
    if (table)
      qg = QkvGather{e->fast_qkv, (const float*)(A + e->w.fast_rope), s->qt, s->fkc, s->fvc, c.fast_n_head, c.fast_n_kv_head, c.n_fast, i + 1};
    ST_TRY(launch_argmax(s->logits, B, c.codebook_size, c.codebook_size, s->new_col + 1 + i, H, s->margin, s->mask,
                         (const void*)(A + e->w.fast_emb), off, c.fast_dim, xnext, table ? nullptr : &to_fast0, &fast_sa, st,
                         table ? &qg : nullptr));
    xf = xnext;
  }
  return launch_commit_embed(s, /*do_commit=*/1, advance_pos, st, picks);
}

// mask[r] = row r of a smoltts_lm_measure_rows call is measured (attn_align_kernel's row mask)
__global__ void measure_mask_kernel(int n, const int* row_frame, int* mask) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) mask[r] = row_frame[r] >= 0;
}

// Slow transformer over M rows of x (already embedded and published for layer 0).
// `measure_frames` (smoltts_lm_measure_rows; prompt rows only): the chosen heads are measured on these rows too, row r as frame
// measure_frames[r] of its slot (< 0: not measured).  `emit_head` (the same call, when it scores): the last block publishes the
// slow head's operand (x * norm, sums of squares) for all M rows, as the last block of a decode frame does for its B rows.
int run_slow_layers(SmolttsSession* s, float* x, float* q, int M, const int* row_pos, const int* row_slot, bool publish_hidden,
                    hipStream_t st, const int* measure_frames = nullptr, bool emit_head = false) {
  const SmolttsEngine* e = s->e;
  const SmolttsLMConfig& c = e->cfg;
  const size_t l_stride = (size_t)s->B * c.n_kv_head * s->max_seq * 64 * (s->kv_format == SMOLTTS_KV_BF16 ? 2 : 4);  // bytes
  for (int l = 0; l < c.n_layer; ++l) {
    EmitArgs next{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (l + 1 < c.n_layer) next = EmitArgs{s->x3n, gamma_at(e, e->w.layers[l + 1].attn_norm), nullptr, nullptr, s->ssq};
    else if (publish_hidden) next = slow_hidden_emit(s);
    else if (emit_head) next = EmitArgs{s->x3n, gamma_at(e, e->w.norm), nullptr, nullptr, s->ssq};
    ST_TRY(run_block(s, e->w.layers[l], c.dim, c.n_head, c.n_kv_head, c.inter, x, q, M, row_pos, row_slot,
                     (const float*)(e->arena + e->w.rope), s->kc + l * l_stride, s->vc + l * l_stride, s->max_seq, s->x3n, next, st,
                     /*first_pos=*/false, s->kv_format, -1, false, /*w_stream=*/((s->stream_w & SMOLTTS_STREAM_W_SLOW) && M <= 128)
                         ? ((s->stream_w & SMOLTTS_STREAM_W_SLOW_ONLY_W13) ? SMOLTTS_STREAM_W_DEPTH_W13 : ((s->stream_w & SMOLTTS_STREAM_W_SLOW_NOT_W13) ? (SMOLTTS_STREAM_W_DEPTH_W2 | SMOLTTS_STREAM_W_DEPTH_QKVO) : 1)) : 0));
    const bool frame_align = publish_hidden && (s->form & FORM_ALIGN);
    if (frame_align || (measure_frames && s->n_align > 0)) {
      // decode frames of a form with bit 5: where this layer's chosen heads look, from q (untouched until the next layer's wqkv
      // launch) and the layer's K rows 0 .. pos -- one more link of the frame's serial chain; row r is slot r (row_slot = iota).
      // Measured prompt rows: the same launch with the rows' own frames; its row mask (row_frame >= 0) goes through x3h, which
      // nothing reads between this block's w2 launch and the next block's w13 launch
      int p0 = 0, np = 0;
      for (int i = 0; i < s->n_align; ++i) {
        if (s->align_layer[i] < l) p0 = i + 1;
        if (s->align_layer[i] == l) ++np;
      }
      const int* frames = s->frames;
      const int* row_mask = s->mask;
      if (np > 0 && !frame_align) {
        frames = measure_frames;
        row_mask = reinterpret_cast<const int*>(s->x3h);
        hipLaunchKernelGGL(measure_mask_kernel, dim3((M + 255) / 256), dim3(256), 0, st, M, measure_frames, reinterpret_cast<int*>(s->x3h));
        ST_CHECK_HIP(hipGetLastError());
      }
      if (np > 0)
        ST_TRY(launch_attention_align(q, s->kc + l * l_stride, s->kv_format, row_pos, row_slot, frames, row_mask, s->align_win,
                                      s->align_head + p0, np, p0, s->n_align, M, c.n_head, c.n_kv_head, s->max_seq, s->max_frames,
                                      s->align_out, st));
    }
  }
  return SMOLTTS_OK;
}

int embed_rows(SmolttsSession* s, const int* cols, int M, float* x, hipStream_t st) {
  const SmolttsEngine* e = s->e;
  const SmolttsLMConfig& c = e->cfg;
  const char* A = e->arena;
  const int cb_first = c.duplicate_code_0 ? 0 : c.codebook_size;
  const EmitArgs em{s->x3n, gamma_at(e, e->w.layers[0].attn_norm), nullptr, nullptr, s->ssq};
  return launch_embed(cols, M, c.n_fast, A + e->w.text_emb, A + e->w.codebook_emb, c.dim, c.codebook_size, cb_first,
                      c.embed_mask_mode, c.semantic_start_id, c.semantic_end_id, c.vocab_size, c.codebook_size * c.num_codebooks,
                      x, &em, st);
}

// One decode frame.  Precondition (the session invariant): xt / x3n / ssq hold the embedded current columns, mask == !done.
int run_decode_frame(SmolttsSession* s, hipStream_t st) {
  ST_TRY(run_slow_layers(s, s->xt, s->qt, s->B, s->pos, s->iota, /*publish_hidden=*/true, st));
  return run_tail(s, /*advance_pos=*/1, st);
}

// ---- PinnedRing.  ring_destroy tolerates a zeroed ring and leaves one; ring_create is all or nothing (the error under the caller's name)
void ring_destroy(PinnedRing* r) {
  for (int k = 0; k < STAGE_RING; ++k)
    if (r->ev[k]) (void)hipEventDestroy(r->ev[k]);
  if (r->base) (void)hipHostFree(r->base);
  memset(r, 0, sizeof(*r));
}

int ring_create(const char* what, PinnedRing* r, size_t area) {
  memset(r, 0, sizeof(*r));
  r->area = area;
  const char* failed = hipHostMalloc((void**)&r->base, area * STAGE_RING, hipHostMallocDefault) != hipSuccess ? "hipHostMalloc" : nullptr;
  if (failed) r->base = nullptr;
  for (int k = 0; k < STAGE_RING && !failed; ++k)
    if (hipEventCreateWithFlags(&r->ev[k], hipEventDisableTiming) != hipSuccess) {
      r->ev[k] = nullptr;
      failed = "hipEventCreate";
    }
  if (!failed) return SMOLTTS_OK;
  ring_destroy(r);
  set_error("%s: %s failed", what, failed);
  return SMOLTTS_E_HIP;
}

// The next area, once the copies that last read it are through: the host's only wait, and only when STAGE_RING uploads are queued
int ring_take(PinnedRing* r, char** area, int* k) {
  *k = r->next;
  r->next = (*k + 1) % STAGE_RING;
  if (r->live[*k]) ST_CHECK_HIP(hipEventSynchronize(r->ev[*k]));
  *area = r->base + (size_t)*k * r->area;
  return SMOLTTS_OK;
}

// Behind the async copies out of area k
int ring_sent(PinnedRing* r, int k, hipStream_t st) {
  ST_CHECK_HIP(hipEventRecord(r->ev[k], st));
  r->live[k] = true;
  return SMOLTTS_OK;
}

// What enter_slot_mode makes; after it the session is outside slot mode and owns nothing of it (a later call may enter again)
void leave_slot_mode(SmolttsSession* s) {
  ring_destroy(&s->slot_ring);
  delete[] s->h_form;
  s->h_form = nullptr;
  s->slot_tab = nullptr; s->filt_tab = nullptr; s->len_tab = nullptr;
  s->slot_mode = false;
}

// Slot / last-row lists of a prefill call -> device, through the session's pinned staging buffer.  Only the previous
// upload is waited for (an event), never the stream: a serving loop calls this while earlier frames are still running.
int stage_upload(SmolttsSession* s, const int32_t* slots_host, const int32_t* last_row_host, int n_slots, hipStream_t st) {
  // a ring of pinned areas: the host only waits when STAGE_RING uploads are still queued behind other work on `st`
  // (a serving loop uploads while a tick of frame graphs is pending; waiting for the previous upload would stall it)
  char* area;
  int k;
  ST_TRY(ring_take(&s->stage_ring, &area, &k));
  int* h = reinterpret_cast<int*>(area);
  for (int i = 0; i < n_slots; ++i) { h[i] = slots_host[i]; h[s->B + i] = last_row_host[i]; }
  ST_CHECK_HIP(hipMemcpyAsync(s->stage_slots, h, sizeof(int) * n_slots, hipMemcpyHostToDevice, st));
  ST_CHECK_HIP(hipMemcpyAsync(s->stage_last, h + s->B, sizeof(int) * n_slots, hipMemcpyHostToDevice, st));
  return ring_sent(&s->stage_ring, k, st);
}

// Forget captured graphs: the kinds of the mask (bit GraphKind), in every form or (form_bit != 0) in the forms with that bit
void drop_graphs(SmolttsSession* s, unsigned kinds = ~0u, int form_bit = 0) {
  for (int k = 0; k < GRAPH_KINDS; ++k)
    for (int f = 0; f < GRAPH_FORMS; ++f) {
      hipGraphExec_t& g = s->graphs[k][f];
      if (g && (kinds >> k & 1) && (form_bit == 0 || (f & form_bit))) {
        (void)hipGraphExecDestroy(g);
        g = nullptr;
      }
    }
}

void set_stop_on_eos(SmolttsSession* s, int stop_on_eos) {
  if (s->stop_on_eos != stop_on_eos) drop_graphs(s);  // the flag is baked into the captured commit nodes
  s->stop_on_eos = stop_on_eos;
}

// The slot list of an entry call and the list beside it: every slot's last prompt row, or (`positions`) its parking position
int check_slot_lists(const char* what, const SmolttsSession* s, const int32_t* slots_host, const int32_t* second_host, int n_slots,
                     int second_limit, bool positions = false) {
  ST_REQUIRE(n_slots > 0 && n_slots <= s->B, SMOLTTS_E_CAPACITY, "%s: %d slots, session holds %d", what, n_slots, s->B);
  for (int i = 0; i < n_slots; ++i) {
    ST_TRY(check_slot(what, slots_host[i], s->B));
    const int v = second_host[i];
    ST_REQUIRE(v >= 0 && v < second_limit, SMOLTTS_E_INVALID,
               positions ? "%s: position %d outside the cache (%d)" : "%s: last_row %d out of range", what, v, second_limit);
  }
  return SMOLTTS_OK;
}

// KV rows of n_rows prompt rows, through the prefill workspace of the session given (the side call passes its shadow session)
int prefill_rows(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev, const int32_t* row_pos_dev, int n_rows,
                 hipStream_t st, const int32_t* measure_frames_dev = nullptr, bool emit_head = false) {
  ST_TRY(embed_rows(s, grid_dev, n_rows, s->xr, st));
  return run_slow_layers(s, s->xr, s->qr, n_rows, row_pos_dev, row_slot_dev, /*publish_hidden=*/false, st, measure_frames_dev, emit_head);
}

// The staged slots (stage_upload) become live at their last prompt column; their first decode frame recomputes that column's row
int arm_slots(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_pos_dev, int n_slots, hipStream_t st) {
  hipLaunchKernelGGL(slot_start_kernel, dim3((s->B + 63) / 64), dim3(64), 0, st, s->B, 1 + s->e->cfg.n_fast, n_slots, s->stage_slots,
                     s->stage_last, row_pos_dev, grid_dev, s->pos, s->frames, s->done, s->margin, s->cur_col, s->salt);
  ST_CHECK_HIP(hipGetLastError());
  ST_TRY(launch_commit_embed(s, /*do_commit=*/0, 0, st));  // mask = !done; embed every slot's (new) current column
  s->prefilled = true;
  return SMOLTTS_OK;
}

// The form of the frame launches: bit 0 = some slot samples its slow token, bit 1 = some slot samples its depth codes, bit 2 = some
// slot's filter entry is on (the sampled picks are then the FILTERS instantiations; without it they are the parent's kernels), bit 3 =
// some slot's length entry is on (the slow pick is then the LENGTH instantiation over the row of logits; it acts on greedy rows too, so
// it outlives the rule that clears the filter bit), bit 4 = some slot scores its slow token (the slow pick is then the SCORE
// instantiation over the row of logits; greedy rows are scored too, so it is not cleared either), bit 5 = some slot's alignment
// window is on (every decode frame then queues attn_align_kernel behind the blocks of the chosen layers; no pick changes).  Outside slot mode always 0 (the session-wide temperatures are baked into the one set; changing them drops it).  Called by every entry
// point that launches or captures picks, after the last change of the table.
int form_of(const SmolttsSession* s) {
  int f = 0;
  if (s->slot_mode)
    for (int b = 0; b < s->B; ++b) f |= s->h_form[b];
  if ((f & (FORM_SLOW | FORM_FAST)) == 0) f &= ~FORM_FILTER;  // nothing samples: the filters have nothing to act on
  if (s->n_align <= 0) f &= ~FORM_ALIGN;                      // no head is chosen: the windows have nothing to measure
  return f;
}
void pick_form(SmolttsSession* s) { s->form = form_of(s); }
// h_form[slot]: the bits of `mask` become `bits`
void set_form_bits(SmolttsSession* s, int slot, int mask, int bits) { s->h_form[slot] = (uint8_t)((s->h_form[slot] & ~mask) | bits); }

// Record `body` (a fixed launch sequence on the given stream) into an executable graph.
template <typename F>
int capture_graph(hipStream_t st, hipGraphExec_t* exec, F body) {
  hipStream_t cap = st;
  bool own = false;
  if (cap == nullptr) {  // the legacy default stream cannot be captured
    ST_CHECK_HIP(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
    own = true;
  }
  ST_CHECK_HIP(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
  const int rc = body(cap);
  hipGraph_t graph = nullptr;
  const hipError_t ee = hipStreamEndCapture(cap, &graph);
  if (own) (void)hipStreamDestroy(cap);
  if (rc != SMOLTTS_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  ST_CHECK_HIP(ee);
  const hipError_t ei = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  ST_CHECK_HIP(ei);
  return SMOLTTS_OK;
}

bool graphs_enabled() {
  const char* no_graph = getenv("SMOLTTS_NO_GRAPH");
  return !(no_graph && no_graph[0] == '1');
}

// s->graphs[kind][s->form], captured from `body` when first needed (a failed capture leaves the entry empty)
template <typename F>
int ensure_graph(SmolttsSession* s, GraphKind kind, hipStream_t st, F body) {
  if (s->graphs[kind][s->form]) return SMOLTTS_OK;
  hipGraphExec_t made = nullptr;
  ST_TRY(capture_graph(st, &made, body));
  s->graphs[kind][s->form] = made;
  return SMOLTTS_OK;
}

int run_decode_frame(SmolttsSession* s, hipStream_t st);

// The graph of `multi_frames` consecutive frames (every graph launch costs the GPU a gap between the last node of one graph and
// the first of the next); a graph of several frames is that many frames queued at once, so it stays inside the run-ahead bound.
int ensure_multi_graph(SmolttsSession* s, int n_frames, hipStream_t st) {
  if (s->flight_limit > 0 && s->multi_frames > s->flight_limit) s->multi_frames = s->flight_limit;
  const int mf = s->multi_frames;
  if (mf > 1 && n_frames >= mf)
    ST_TRY(ensure_graph(s, GRAPH_MULTI, st, [&](hipStream_t cap) {
      for (int i = 0; i < mf; ++i) ST_TRY(run_decode_frame(s, cap));
      return (int)SMOLTTS_OK;
    }));
  return SMOLTTS_OK;
}

// ---- slot mode
// One upload of a per-slot table, on the host and on the device alike: B entries, then B slot numbers
template <typename Entry>
constexpr size_t upload_bytes(size_t B) { return B * (sizeof(Entry) + sizeof(int)); }
constexpr size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
// the caller's alignment buffer: [B][2] window table | upload area | rows, each part 16-byte aligned
size_t align_table_bytes(const SmolttsSession* s) { return round16((size_t)s->B * 2 * sizeof(int)); }
size_t align_header_bytes(const SmolttsSession* s) { return align_table_bytes(s) + round16(upload_bytes<int2>(s->B)); }

// Enter slot mode (first per-slot call of either kind): host mirror, pinned ring, events; every slot greedy with seed 0 and
// its filters off
int enter_slot_mode(SmolttsSession* s, hipStream_t st) {
  if (s->slot_mode) return SMOLTTS_OK;
  const size_t B = s->B;
  const int rc = [&]() -> int {
    s->h_form = new (std::nothrow) uint8_t[B]();
    ST_REQUIRE(s->h_form, SMOLTTS_E_INVALID, "session_set_slot_sampling: out of host memory");
    // an area holds one upload of any table: every call writes at the start of the area it takes
    const size_t area = std::max({upload_bytes<SmolttsSlotSampling>(B), upload_bytes<SmolttsSlotFilters>(B),
                                  upload_bytes<SmolttsSlotLength>(B), upload_bytes<int2>(B)});
    ST_TRY(ring_create("session_set_slot_sampling", &s->slot_ring, round16(area)));
    s->slot_tab = s->slot_tab_area;
    s->filt_tab = s->filt_tab_area;
    s->len_tab = s->len_tab_area;
    ST_CHECK_HIP(hipMemsetAsync(s->slot_tab, 0, B * sizeof(SmolttsSlotSampling), st));
    ST_CHECK_HIP(hipMemsetAsync(s->filt_tab, 0, B * sizeof(SmolttsSlotFilters), st));
    ST_CHECK_HIP(hipMemsetAsync(s->len_tab, 0, B * sizeof(SmolttsSlotLength), st));
    return SMOLTTS_OK;
  }();
  if (rc != SMOLTTS_OK) {
    leave_slot_mode(s);  // (slot mode is not entered, and nothing of it is left behind)
    return rc;
  }
  s->slot_mode = true;
  drop_graphs(s);  // (the session-wide set: slot mode builds its own)
  return SMOLTTS_OK;
}

// One upload of `n` entries of a per-slot table: table_dev[slots_host[i]] = entry i.  check(i) validates the caller's values of entry
// i (it may refuse with a status); fill(i, entry) writes the entry and updates the host mirror.  Every check passes before anything
// changes: a refused call leaves the session as it was.  The host copies the entries and their slot numbers into the next area of the
// pinned ring and queues one copy (into up_dev: [B] entries, [B] slots) + one scatter launch on `st`; it waits only for the upload that
// last used that area (an event), never for the stream.
template <typename Entry, typename Check, typename Fill>
int upload_slot_entries(SmolttsSession* s, const char* what, const int32_t* slots_host, int n, Entry* up_dev, Entry* table_dev,
                        hipStream_t st, Check check, Fill fill) {
  ST_REQUIRE(n >= 0 && n <= s->B, SMOLTTS_E_CAPACITY, "%s: %d entries, session holds %d slots", what, n, s->B);
  for (int i = 0; i < n; ++i) {
    ST_TRY(check_slot(what, slots_host[i], s->B));
    for (int j = 0; j < i; ++j) ST_REQUIRE(slots_host[j] != slots_host[i], SMOLTTS_E_INVALID, "%s: slot %d listed twice", what, slots_host[i]);
    ST_TRY(check(i));
  }
  ST_TRY(enter_slot_mode(s, st));
  if (n == 0) return SMOLTTS_OK;
  const size_t B = s->B;
  char* area;
  int k;
  ST_TRY(ring_take(&s->slot_ring, &area, &k));
  Entry* h = reinterpret_cast<Entry*>(area);
  int* hi = reinterpret_cast<int*>(h + B);
  for (int i = 0; i < n; ++i) {
    fill(i, h[i]);
    hi[i] = slots_host[i];
  }
  ST_CHECK_HIP(hipMemcpyAsync(up_dev, h, upload_bytes<Entry>(B), hipMemcpyHostToDevice, st));
  ST_TRY(ring_sent(&s->slot_ring, k, st));
  hipLaunchKernelGGL(slot_scatter_kernel<Entry>, dim3((n + 63) / 64), dim3(64), 0, st, n, up_dev, reinterpret_cast<const int*>(up_dev + B), table_dev);
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

int check_offsets(const SmolttsLMConfig& c, const SmolttsLMWeights& w, size_t bytes) {
  auto ok = [&](uint64_t off, size_t need) { return off % 16 == 0 && off + need <= bytes; };
  ST_REQUIRE(c.weight_format == SMOLTTS_W_BF16 || c.weight_format == SMOLTTS_W_FP8, SMOLTTS_E_INVALID,
             "engine: unknown weight_format %d", c.weight_format);
  const bool f8 = c.weight_format == SMOLTTS_W_FP8;
  // bytes of one Linear [rows][k]: bf16 tiles, or e4m3 tiles + fp32 row scales
  auto mat = [&](size_t rows, size_t k) { return f8 ? rows * (k + 4) : rows * k * 2; };
  const size_t d = c.dim, fd = c.fast_dim;
  if (f8)
    ST_REQUIRE(c.vocab_size % 16 == 0 && c.codebook_size % 16 == 0, SMOLTTS_E_INVALID, "engine: fp8 weights need vocab and codebook sizes %% 16 == 0");
  ST_REQUIRE(ok(w.text_emb, (size_t)c.vocab_size * d * 2) && ok(w.head, mat(c.vocab_size, d)) &&
                 ok(w.codebook_emb, (size_t)c.codebook_size * c.num_codebooks * d * 2) && ok(w.norm, d * 4) &&
                 ok(w.fast_norm, fd * 4) && ok(w.rope, (size_t)c.max_seq_len * 64 * 4) && ok(w.fast_rope, (size_t)c.n_fast * 64 * 4),
             SMOLTTS_E_INVALID, "engine: weight offsets outside the arena or misaligned");
  const size_t head_rows = (size_t)(c.n_fast - 1) * w.fast_head_step_stride + c.codebook_size;
  ST_REQUIRE(ok(w.fast_head, mat(head_rows, fd)), SMOLTTS_E_INVALID, "engine: fast_head outside the arena");
  ST_REQUIRE(w.fast_head_step_stride % 16 == 0, SMOLTTS_E_INVALID, "engine: fast_head_step_stride must be a multiple of 16");
  if (c.has_fast_project_in)
    ST_REQUIRE(ok(w.fast_proj_w, mat(fd, d)) && ok(w.fast_proj_b, fd * 4), SMOLTTS_E_INVALID, "engine: fast_project_in outside the arena");
  for (int l = 0; l < c.n_layer + c.n_fast_layer; ++l) {
    const bool fast = l >= c.n_layer;
    const SmolttsBlockWeights& b = fast ? w.fast_layers[l - c.n_layer] : w.layers[l];
    const size_t dd = fast ? fd : d, hh = fast ? c.fast_n_head : c.n_head, kk = fast ? c.fast_n_kv_head : c.n_kv_head;
    const size_t ii = fast ? c.fast_inter : c.inter;
    ST_REQUIRE(ok(b.attn_norm, dd * 4) && ok(b.ffn_norm, dd * 4) && ok(b.wqkv, mat((hh + 2 * kk) * 64, dd)) &&
                   ok(b.wo, mat(dd, dd)) && ok(b.w13, mat(2 * ii, dd)) && ok(b.w2, mat(dd, ii)),
               SMOLTTS_E_INVALID, "engine: layer %d weight offsets outside the arena or misaligned", l);
  }
  return SMOLTTS_OK;
}

// ---- voice prefixes (smoltts_session_save_prefix / _install_prefix): rows [0, P) of a slot's slow KV cache in a caller-owned slab
//   [SmolttsPrefixHeader, padded to PREFIX_HDR bytes][layer][K | V][kv head][P][64] in the session's KV dtype
// Every (layer, K/V, kv head) run is contiguous in the slab and in the cache ([layer][slot][kv head][max_seq][64]), and its bytes
// are a multiple of 128: a copy of 16-byte units.  One launch moves up to SMOLTTS_PREFIX_MAX_INSTALL runs sets; blockIdx.y picks
// the (descriptor, run), blockIdx.x a PREFIX_BLOCK_BYTES piece of it, and each lane has PREFIX_UNROLL loads in flight before it stores.
constexpr int PREFIX_HDR = 256;
constexpr int PREFIX_THREADS = 256, PREFIX_UNROLL = 4;
constexpr int PREFIX_BLOCK_BYTES = PREFIX_THREADS * PREFIX_UNROLL * 16;  // 16 KiB per workgroup

struct PrefixDesc {
  char* prefix;  // slab (header first)
  int slot;
  int n_positions;
};

struct PrefixCopyArgs {
  char *kc, *vc;
  uint64_t layer_bytes;  // bytes of one layer of the cache (all slots)
  int n_kv_head, max_seq, row_bytes, runs;  // runs = n_layer * 2 * n_kv_head per descriptor
  int n;
  int to_cache;          // 1: slab -> cache (install), 0: cache -> slab (save; writes the header too)
  SmolttsPrefixHeader header;  // save: the header written into the slab
  PrefixDesc d[SMOLTTS_PREFIX_MAX_INSTALL];
};

__global__ __launch_bounds__(PREFIX_THREADS) void prefix_copy_kernel(PrefixCopyArgs a) {
  const int d = blockIdx.y / a.runs, r = blockIdx.y % a.runs;
  if (d >= a.n) return;
  const PrefixDesc desc = a.d[d];
  const int l = r / (2 * a.n_kv_head), kv = (r / a.n_kv_head) & 1, h = r % a.n_kv_head;
  const uint64_t run_bytes = (uint64_t)desc.n_positions * a.row_bytes;
  char* slab_run = desc.prefix + PREFIX_HDR + (uint64_t)r * run_bytes;
  char* cache_run = (kv ? a.vc : a.kc) + (uint64_t)l * a.layer_bytes + ((uint64_t)desc.slot * a.n_kv_head + h) * a.max_seq * a.row_bytes;
  if (a.to_cache) {
    // the slab must carry the header the host validated (a slab paired with another slab's header copies nothing)
    const SmolttsPrefixHeader* hd = reinterpret_cast<const SmolttsPrefixHeader*>(desc.prefix);
    if (hd->magic != SMOLTTS_PREFIX_MAGIC || hd->n_positions != desc.n_positions) return;
  } else if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    *reinterpret_cast<SmolttsPrefixHeader*>(desc.prefix) = a.header;
  }
  const uint4* src = reinterpret_cast<const uint4*>(a.to_cache ? slab_run : cache_run);
  uint4* dst = reinterpret_cast<uint4*>(a.to_cache ? cache_run : slab_run);
  const uint64_t units = run_bytes / 16;
  const uint64_t base = (uint64_t)blockIdx.x * (PREFIX_BLOCK_BYTES / 16);
  if (base >= units) return;  // (a shorter prefix of the launch)
  if (base + PREFIX_BLOCK_BYTES / 16 <= units) {  // whole piece: every load issued before the first store
    uint4 v[PREFIX_UNROLL];
#pragma unroll
    for (int k = 0; k < PREFIX_UNROLL; ++k) v[k] = src[base + k * PREFIX_THREADS + threadIdx.x];
#pragma unroll
    for (int k = 0; k < PREFIX_UNROLL; ++k) dst[base + k * PREFIX_THREADS + threadIdx.x] = v[k];
  } else {  // the run's last piece
    for (uint64_t u = base + threadIdx.x; u < units; u += PREFIX_THREADS) dst[u] = src[u];
  }
}

size_t prefix_data_bytes(const SmolttsLMConfig& c, int n_positions, int kv_format) {
  return (size_t)c.n_layer * 2 * c.n_kv_head * n_positions * 64 * (kv_format == SMOLTTS_KV_BF16 ? 2 : 4);
}

SmolttsPrefixHeader prefix_header(const SmolttsSession* s, int n_positions) {
  const SmolttsLMConfig& c = s->e->cfg;
  SmolttsPrefixHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = SMOLTTS_PREFIX_MAGIC;
  h.n_positions = n_positions;
  h.n_layer = c.n_layer;
  h.n_kv_head = c.n_kv_head;
  h.kv_format = s->kv_format;
  h.head_dim = 64;
  h.data_bytes = prefix_data_bytes(c, n_positions, s->kv_format);
  return h;
}

PrefixCopyArgs prefix_args(const SmolttsSession* s, int to_cache) {
  const SmolttsLMConfig& c = s->e->cfg;
  PrefixCopyArgs a;
  memset(&a, 0, sizeof(a));
  a.kc = s->kc; a.vc = s->vc;
  a.row_bytes = 64 * (s->kv_format == SMOLTTS_KV_BF16 ? 2 : 4);
  a.layer_bytes = (uint64_t)s->B * c.n_kv_head * s->max_seq * a.row_bytes;
  a.n_kv_head = c.n_kv_head; a.max_seq = s->max_seq;
  a.runs = c.n_layer * 2 * c.n_kv_head;
  a.to_cache = to_cache;
  return a;
}

int launch_prefix_copy(const PrefixCopyArgs& a, int max_positions, hipStream_t st) {
  const uint64_t run_bytes = (uint64_t)max_positions * a.row_bytes;
  const dim3 grid((unsigned)((run_bytes + PREFIX_BLOCK_BYTES - 1) / PREFIX_BLOCK_BYTES), (unsigned)(a.n * a.runs));
  hipLaunchKernelGGL(prefix_copy_kernel, grid, dim3(PREFIX_THREADS), 0, st, a);
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

}  // namespace

extern "C" {

int smoltts_engine_create(const SmolttsLMConfig* cfg, const SmolttsLMWeights* offsets, const void* arena_dev,
                          size_t arena_bytes, SmolttsEngine** out) {
  ST_REQUIRE(cfg && offsets && arena_dev && out, SMOLTTS_E_INVALID, "engine_create: null argument");
  const SmolttsLMConfig& c = *cfg;
  ST_REQUIRE(c.n_layer > 0 && c.n_layer <= SMOLTTS_MAX_LAYERS && c.n_fast_layer > 0 && c.n_fast_layer <= SMOLTTS_MAX_FAST_LAYERS,
             SMOLTTS_E_INVALID, "engine_create: layer counts out of range");
  ST_REQUIRE(c.dim == c.n_head * 64 && c.fast_dim == c.fast_n_head * 64, SMOLTTS_E_INVALID,
             "engine_create: dim must equal n_head * 64 (head_dim 64 only)");
  ST_REQUIRE(c.dim % 32 == 0 && c.fast_dim % 32 == 0 && c.inter % 32 == 0 && c.fast_inter % 32 == 0, SMOLTTS_E_INVALID,
             "engine_create: dims must be multiples of 32");
  ST_REQUIRE(c.n_head % c.n_kv_head == 0 && c.fast_n_head % c.fast_n_kv_head == 0 && c.n_head / c.n_kv_head <= 4 &&
                 c.fast_n_head / c.fast_n_kv_head <= 4,
             SMOLTTS_E_INVALID, "engine_create: unsupported GQA grouping");
  ST_REQUIRE(c.vocab_size % 16 == 0 && c.codebook_size % 16 == 0, SMOLTTS_E_INVALID,
             "engine_create: vocab_size and codebook_size must be multiples of 16");
  ST_REQUIRE(c.n_fast == c.num_codebooks - (c.duplicate_code_0 ? 0 : 1) && c.n_fast >= 1 && c.n_fast <= 32, SMOLTTS_E_INVALID,
             "engine_create: n_fast inconsistent with num_codebooks/duplicate_code_0");
  ST_REQUIRE(c.has_fast_project_in == (c.fast_dim != c.dim), SMOLTTS_E_INVALID,
             "engine_create: has_fast_project_in must be set exactly when fast_dim != dim");
  ST_REQUIRE(c.max_seq_len > 0, SMOLTTS_E_INVALID, "engine_create: max_seq_len");
  ST_TRY(check_offsets(c, *offsets, arena_bytes));
  SmolttsEngine* e = new (std::nothrow) SmolttsEngine;
  ST_REQUIRE(e, SMOLTTS_E_INVALID, "engine_create: out of host memory");
  e->cfg = c; e->w = *offsets; e->arena = (const char*)arena_dev; e->arena_bytes = arena_bytes;
  e->fast_qkv = nullptr;
  *out = e;
  return SMOLTTS_OK;
}

void smoltts_engine_destroy(SmolttsEngine* e) { delete e; }

// ---- derived table: depth layer-0 q | k | v of every fast-embedding row (see QkvGather in argmax_dev.h)
// Rows a depth step can be fed with: code + offset of the steps that have a successor (lm/generate.py:134-140).
static long fast_emb_rows_used(const SmolttsLMConfig& c) {
  if (c.n_fast < 2) return 0;
  return c.depthwise_wte ? (long)(c.duplicate_code_0 ? c.n_fast - 1 : c.n_fast) * c.codebook_size : (long)c.codebook_size;
}
constexpr int QKV_BUILD_ROWS = 128;  // rows per GEMM launch of the build: the decode kernels' own variant (M <= 128)

size_t smoltts_engine_fast_qkv_bytes(const SmolttsEngine* e) {
  if (!e) return 0;
  const SmolttsLMConfig& c = e->cfg;
  const long rows = fast_emb_rows_used(c);
  if (rows <= 0) return 0;
  const size_t nqkv = (size_t)(c.fast_n_head + 2 * c.fast_n_kv_head) * 64;
  const size_t table = align_up((size_t)rows * nqkv * sizeof(float));
  const size_t x3 = align_up((size_t)QKV_BUILD_ROWS * c.fast_dim * 6), ssq = align_up((size_t)QKV_BUILD_ROWS * (c.fast_dim / 16) * sizeof(float));
  return table + x3 + ssq;
}

int smoltts_engine_build_fast_qkv(SmolttsEngine* e, void* slab_dev, size_t slab_bytes, void* stream) {
  ST_REQUIRE(e && slab_dev, SMOLTTS_E_INVALID, "engine_build_fast_qkv: null argument");
  const SmolttsLMConfig& c = e->cfg;
  const size_t need = smoltts_engine_fast_qkv_bytes(e);
  ST_REQUIRE(need > 0, SMOLTTS_E_INVALID, "engine_build_fast_qkv: this model has no depth step with a successor");
  ST_REQUIRE(slab_bytes >= need && ((uintptr_t)slab_dev & 255) == 0, SMOLTTS_E_CAPACITY,
             "engine_build_fast_qkv: slab has %zu bytes (256-byte aligned), %zu needed", slab_bytes, need);
  const long rows = fast_emb_rows_used(c);
  ST_REQUIRE(e->w.fast_emb % 16 == 0 && e->w.fast_emb + (size_t)rows * c.fast_dim * 2 <= e->arena_bytes, SMOLTTS_E_INVALID,
             "engine_build_fast_qkv: the fast embedding table (%ld rows) lies outside the arena", rows);
  hipStream_t st = (hipStream_t)stream;
  const char* A = e->arena;
  const int nqkv = (c.fast_n_head + 2 * c.fast_n_kv_head) * 64;
  Carver cv{(char*)slab_dev, 0};
  float* table = cv.take<float>((size_t)rows * nqkv);
  char* x3 = cv.take<char>((size_t)QKV_BUILD_ROWS * c.fast_dim * 6);
  float* ssq = cv.take<float>((size_t)QKV_BUILD_ROWS * (c.fast_dim / 16));
  e->fast_qkv = nullptr;
  const SmolttsBlockWeights& bw = e->w.fast_layers[0];
  const EmitArgs em{x3, gamma_at(e, bw.attn_norm), nullptr, nullptr, ssq};
  for (long r0 = 0; r0 < rows; r0 += QKV_BUILD_ROWS) {
    const int n = (int)(rows - r0 < QKV_BUILD_ROWS ? rows - r0 : QKV_BUILD_ROWS);
    // the row exactly as the picking kernel would publish it (X3 of E[row] * attention_norm + its sum of squares) ...
    ST_TRY(launch_emb_rows_pack(A + e->w.fast_emb, r0, n, c.fast_dim, em, st));
    // ... through the decode path's own wqkv GEMM (same accumulation order), the RMSNorm scale applied, RoPE left to the gather
    SmolttsGemm3Args a = base3(c.weight_format, A + bw.wqkv, x3, n, nqkv, c.fast_dim, SMOLTTS_EPI_STORE);
    a.ssq_in_dev = ssq; a.eps = c.norm_eps; a.out_dev = table + (size_t)r0 * nqkv; a.ldo = nqkv;
    ST_TRY(launch_gemm3(a, st));
  }
  ST_CHECK_HIP(hipStreamSynchronize(st));  // the scratch part of the slab is dead from here; the table part must outlive the engine's sessions
  e->fast_qkv = table;
  return SMOLTTS_OK;
}

size_t smoltts_session_slab_bytes(const SmolttsEngine* e, int32_t max_batch, int32_t max_seq, int32_t max_rows,
                                  int32_t max_frames) {
  return smoltts_session_slab_bytes_kv(e, max_batch, max_seq, max_rows, max_frames, SMOLTTS_KV_F32);
}

size_t smoltts_session_slab_bytes_kv(const SmolttsEngine* e, int32_t max_batch, int32_t max_seq, int32_t max_rows,
                                     int32_t max_frames, int32_t kv_format) {
  if (!e || max_batch <= 0 || max_seq <= 0 || max_rows <= 0 || max_frames <= 0) return 0;
  if (kv_format != SMOLTTS_KV_F32 && kv_format != SMOLTTS_KV_BF16) return 0;
  SmolttsSession tmp;
  memset(&tmp, 0, sizeof(tmp));
  tmp.e = const_cast<SmolttsEngine*>(e);
  tmp.kv_format = kv_format;
  tmp.B = max_batch; tmp.max_seq = max_seq; tmp.max_rows = max_rows; tmp.max_frames = max_frames;
  return carve(&tmp, nullptr);
}

int smoltts_session_create(SmolttsEngine* e, void* slab_dev, size_t slab_bytes, int32_t max_batch, int32_t max_seq,
                           int32_t max_rows, int32_t max_frames, SmolttsSession** out) {
  return smoltts_session_create_kv(e, slab_dev, slab_bytes, max_batch, max_seq, max_rows, max_frames, SMOLTTS_KV_F32, out);
}

int smoltts_session_create_kv(SmolttsEngine* e, void* slab_dev, size_t slab_bytes, int32_t max_batch, int32_t max_seq,
                              int32_t max_rows, int32_t max_frames, int32_t kv_format, SmolttsSession** out) {
  ST_REQUIRE(e && slab_dev && out, SMOLTTS_E_INVALID, "session_create: null argument");
  ST_REQUIRE(kv_format == SMOLTTS_KV_F32 || kv_format == SMOLTTS_KV_BF16, SMOLTTS_E_INVALID, "session_create: unknown kv_format %d", kv_format);
  ST_REQUIRE(kv_format == SMOLTTS_KV_F32 || max_seq > 16, SMOLTTS_E_INVALID, "session_create: a bf16 KV cache needs max_seq > 16");
  ST_REQUIRE(max_batch > 0 && max_batch <= 4096 && max_rows > 0 && max_frames > 0, SMOLTTS_E_INVALID, "session_create: bad sizes");
  ST_REQUIRE(max_seq > 0 && max_seq <= e->cfg.max_seq_len, SMOLTTS_E_CAPACITY,
             "session_create: max_seq %d exceeds the RoPE table (%d)", max_seq, e->cfg.max_seq_len);
  ST_REQUIRE(((uintptr_t)slab_dev & 255) == 0, SMOLTTS_E_INVALID, "session_create: slab must be 256-byte aligned");
  const size_t need = smoltts_session_slab_bytes_kv(e, max_batch, max_seq, max_rows, max_frames, kv_format);
  ST_REQUIRE(slab_bytes >= need, SMOLTTS_E_CAPACITY, "session_create: slab has %zu bytes, %zu needed", slab_bytes, need);
  SmolttsSession* s = new (std::nothrow) SmolttsSession;
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_create: out of host memory");
  memset(s, 0, sizeof(*s));
  s->e = e; s->B = max_batch; s->max_seq = max_seq; s->max_rows = max_rows; s->max_frames = max_frames;
  s->dup_code = -1;
  s->use_qkv_table = true;
  s->commit_picks = true;
  s->split_attn = true;
  s->stream_w = SMOLTTS_STREAM_W_DEFAULT;
  s->fuse_depth_attn = true;
  s->fuse_pick = true;
  s->kv_format = kv_format;
  carve(s, (char*)slab_dev);
  // from here a failure sets its message and hands the half-built session to smoltts_session_destroy
  if (const int rc = ring_create("session_create", &s->stage_ring, sizeof(int) * 2 * max_batch); rc != SMOLTTS_OK) {
    smoltts_session_destroy(s);
    return rc;
  }
  {  // frames the host may run ahead of the GPU: SMOLTTS_MAX_FRAMES_IN_FLIGHT (default 64; 0 = unbounded).  A profiler that
     // rewrites every dispatch into several packets (rocprofv3 --pmc) needs a small bound and one frame per graph: its
     // command line sets both variables explicitly (tools/collect_pmc.sh) -- the library itself never looks for a profiler.
    const char* lim = getenv("SMOLTTS_MAX_FRAMES_IN_FLIGHT");
    const int limit = lim ? atoi(lim) : 64;
    s->flight_group = limit > 0 ? (limit + 1) / 2 : 0;
    for (int k = 0; k < 2; ++k)
      if (hipEventCreateWithFlags(&s->flight_ev[k], hipEventDisableTiming) != hipSuccess) s->flight_group = 0;
    const char* fpg = getenv("SMOLTTS_FRAMES_PER_GRAPH");  // frames captured into one graph where that many remain to be launched
    s->multi_frames = fpg ? atoi(fpg) : 0;  // 0: follows the calls (smoltts_session_set_frames_per_graph, or min(n_frames, 4) of the largest call so far)
    if (s->multi_frames < 0 || s->multi_frames > 16) s->multi_frames = 1;
    s->multi_fixed = s->multi_env = fpg != nullptr;
    s->flight_limit = limit;
  }
  hipLaunchKernelGGL(init_state_kernel, dim3((max_batch + 63) / 64), dim3(64), 0, 0, max_batch, e->cfg.n_fast, s->iota,
                     s->fastpos, s->pos, s->frames, s->done, s->mask, s->margin, s->margin_at, s->cur_col, s->new_col, s->salt, s->attn_ticket);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipStreamSynchronize(0);
  if (err != hipSuccess) {
    set_error("session_create: init kernel failed: %s", hipGetErrorString(err));
    smoltts_session_destroy(s);
    return SMOLTTS_E_HIP;
  }
  *out = s;
  return SMOLTTS_OK;
}

// (copes with a half-built, zero-initialised session: smoltts_session_create_kv's failures end here)
void smoltts_session_destroy(SmolttsSession* s) {
  if (!s) return;
  drop_graphs(s);
  ring_destroy(&s->stage_ring);
  for (int k = 0; k < 2; ++k)
    if (s->flight_ev[k]) (void)hipEventDestroy(s->flight_ev[k]);
  leave_slot_mode(s);
  delete s;
}

int smoltts_lm_prefill(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev, const int32_t* row_pos_dev,
                       int32_t n_rows, const int32_t* slots_host, const int32_t* last_row_host, int32_t n_slots,
                       int32_t stop_on_eos, void* stream) {
  ST_REQUIRE(s && grid_dev && row_slot_dev && row_pos_dev && slots_host && last_row_host, SMOLTTS_E_INVALID,
             "lm_prefill: null argument");
  ST_REQUIRE(n_rows > 0 && n_rows <= s->max_rows, SMOLTTS_E_CAPACITY, "lm_prefill: %d rows, session holds %d", n_rows, s->max_rows);
  ST_TRY(check_slot_lists("lm_prefill", s, slots_host, last_row_host, n_slots, n_rows));
  hipStream_t st = (hipStream_t)stream;
  const SmolttsEngine* e = s->e;
  const SmolttsLMConfig& c = e->cfg;
  set_stop_on_eos(s, stop_on_eos);
  pick_form(s);
  ST_TRY(stage_upload(s, slots_host, last_row_host, n_slots, st));
  hipLaunchKernelGGL(slot_reset_kernel, dim3((s->B + 63) / 64), dim3(64), 0, st, s->B, n_slots, s->stage_slots, s->stage_last,
                     row_pos_dev, s->pos, s->frames, s->done, s->mask, s->margin, s->salt);
  ST_CHECK_HIP(hipGetLastError());
  ST_TRY(prefill_rows(s, grid_dev, row_slot_dev, row_pos_dev, n_rows, st));
  hipLaunchKernelGGL(scatter_last_kernel, dim3(n_slots), dim3(256), 0, st, s->xr, s->stage_slots, s->stage_last, c.dim, s->xt);
  ST_CHECK_HIP(hipGetLastError());
  {  // publish the slow hidden rows of all B slots (rows of slots not being started are masked at commit)
    const EmitArgs em = slow_hidden_emit(s);
    ST_TRY(launch_x3_pack(s->xt, c.dim, s->B, c.dim, em.x3a, em.gamma_a, em.x3b, em.gamma_b, em.ssq, st));
  }
  // frame 0: the tail is the same ~180 launches after every prefill -> replayed from a graph (host launch time is what
  // a single short prompt waits for)
  if (graphs_enabled()) {
    ST_TRY(ensure_graph(s, GRAPH_TAIL, st, [&](hipStream_t cap) { return run_tail(s, /*advance_pos=*/0, cap); }));
    ST_CHECK_HIP(hipGraphLaunch(s->graphs[GRAPH_TAIL][s->form], st));
  } else {
    ST_TRY(run_tail(s, /*advance_pos=*/0, st));
  }
  s->prefilled = true;
  return SMOLTTS_OK;
}

int smoltts_lm_prefill_chunk(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev, const int32_t* row_pos_dev,
                             int32_t n_rows, const int32_t* slots_host, const int32_t* last_row_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(s && grid_dev && row_slot_dev && row_pos_dev && slots_host && last_row_host, SMOLTTS_E_INVALID,
             "lm_prefill_chunk: null argument");
  ST_REQUIRE(n_rows > 0 && n_rows <= s->max_rows, SMOLTTS_E_CAPACITY, "lm_prefill_chunk: %d rows, session holds %d", n_rows, s->max_rows);
  ST_TRY(check_slot_lists("lm_prefill_chunk", s, slots_host, last_row_host, n_slots, n_rows));
  hipStream_t st = (hipStream_t)stream;
  ST_TRY(stage_upload(s, slots_host, last_row_host, n_slots, st));
  hipLaunchKernelGGL(slot_park_kernel, dim3((s->B + 63) / 64), dim3(64), 0, st, s->B, n_slots, s->stage_slots, s->stage_last, row_pos_dev,
                     s->pos, s->done, s->mask);
  ST_CHECK_HIP(hipGetLastError());
  ST_TRY(prefill_rows(s, grid_dev, row_slot_dev, row_pos_dev, n_rows, st));
  return launch_commit_embed(s, /*do_commit=*/0, 0, st);  // the prompt rows went through x3n / ssq: re-publish the decode rows
}

int smoltts_lm_prefill_deferred(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev, const int32_t* row_pos_dev,
                                int32_t n_rows, const int32_t* slots_host, const int32_t* last_row_host, int32_t n_slots,
                                int32_t stop_on_eos, void* stream) {
  ST_REQUIRE(s && grid_dev && row_slot_dev && row_pos_dev && slots_host && last_row_host, SMOLTTS_E_INVALID,
             "lm_prefill_deferred: null argument");
  ST_REQUIRE(n_rows > 0 && n_rows <= s->max_rows, SMOLTTS_E_CAPACITY, "lm_prefill_deferred: %d rows, session holds %d", n_rows, s->max_rows);
  ST_TRY(check_slot_lists("lm_prefill_deferred", s, slots_host, last_row_host, n_slots, n_rows));
  hipStream_t st = (hipStream_t)stream;
  set_stop_on_eos(s, stop_on_eos);
  ST_TRY(stage_upload(s, slots_host, last_row_host, n_slots, st));
  // KV rows of the whole prompt (the last column's row is recomputed by the first decode frame, identically)
  ST_TRY(prefill_rows(s, grid_dev, row_slot_dev, row_pos_dev, n_rows, st));
  return arm_slots(s, grid_dev, row_pos_dev, n_slots, st);
}

// ---- prompt prefill beside the decode frames (serving: the refill of a slot no longer stops the other slots' ticks)
//   tick stream:   ... tick k-1 | park(new slots) | tick k ............ | start(new slots) | tick k+1 (their frame 0) ...
//   side stream:                     (host saw the park done) prefill_side(new prompts)  ^ host saw it done
// The side call shares nothing with the frames but the KV cache, and of that only rows 0 .. T-2 of the parked slots: their idle
// decode rows write at the parking position T-1 (rewritten by the tenant's first frame) and read garbage nobody keeps.
int smoltts_lm_park_slots(SmolttsSession* s, const int32_t* slots_host, const int32_t* pos_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(s && slots_host && pos_host, SMOLTTS_E_INVALID, "lm_park_slots: null argument");
  ST_TRY(check_slot_lists("lm_park_slots", s, slots_host, pos_host, n_slots, s->max_seq, /*positions=*/true));
  hipStream_t st = (hipStream_t)stream;
  ST_TRY(stage_upload(s, slots_host, pos_host, n_slots, st));
  hipLaunchKernelGGL(slot_parkpos_kernel, dim3((s->B + 63) / 64), dim3(64), 0, st, s->B, n_slots, s->stage_slots, s->stage_last, s->pos, s->done, s->mask);
  ST_CHECK_HIP(hipGetLastError());
  return launch_commit_embed(s, /*do_commit=*/0, 0, st);  // mask = !done for the next frame
}

int smoltts_lm_prefill_side(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev, const int32_t* row_pos_dev,
                            int32_t n_rows, void* stream) {
  ST_REQUIRE(s && grid_dev && row_slot_dev && row_pos_dev, SMOLTTS_E_INVALID, "lm_prefill_side: null argument");
  ST_REQUIRE(n_rows > 0 && n_rows <= s->max_rows, SMOLTTS_E_CAPACITY, "lm_prefill_side: %d rows, session holds %d", n_rows, s->max_rows);
  SmolttsSession side = *s;  // the same engine, caches and options; every activation buffer of the slow layers swapped for the side set
  side.xr = s->sd_xr; side.qr = s->sd_qr; side.x3n = s->sd_x3n; side.x3a = s->sd_x3a; side.x3h = s->sd_x3h; side.ssq = s->sd_ssq;
  side.split_attn = false;  // (the key-split attention's records and tickets belong to the frames)
  side.dup_code = -1;
  hipStream_t st = (hipStream_t)stream;
  return prefill_rows(&side, grid_dev, row_slot_dev, row_pos_dev, n_rows, st);
}

// Rows [r0, r0 + n) of an X3 operand of 32 * nchunks columns and of its sums of squares [rows][2 * nchunks] -> rows [0, n) of another
// operand and array: 16-byte copies, one workgroup per row (x3.h has the layout)
__global__ __launch_bounds__(256) void x3_rows_gather_kernel(const char* src, const float* ssq_src, int r0, int nchunks, char* dst,
                                                             float* ssq_dst) {
  const int md = blockIdx.x, ms = r0 + md;
  for (int i = threadIdx.x; i < nchunks * 12; i += 256) {
    const int c = i / 12, piece = (i % 12) >> 2, q = i & 3;
    const size_t so = ((size_t)(ms >> 4) * nchunks + c) * 3072 + piece * 1024 + (size_t)(q * 16 + (ms & 15)) * 16;
    const size_t dp = ((size_t)(md >> 4) * nchunks + c) * 3072 + piece * 1024 + (size_t)(q * 16 + (md & 15)) * 16;
    *reinterpret_cast<uint4*>(dst + dp) = *reinterpret_cast<const uint4*>(src + so);
  }
  for (int i = threadIdx.x; i < 2 * nchunks; i += 256) ssq_dst[(size_t)md * 2 * nchunks + i] = ssq_src[(size_t)ms * 2 * nchunks + i];
}

// Forced alignment: the rows of a non-final prefill chunk, measured.  The last block publishes the head's
// operand for every row, as a decode frame's does; the slow head then reads max_batch rows at a time -- copied to the front of
// x3n2, their sums of squares to xt, both of which the closing commit_embed launch rewrites or nothing reads before the next
// frame rewrites them -- into the rows the decode frames' head writes: no workspace of its own, the GEMM forms of the decode
// frames, and a row's logits are the bits a decode frame computes for it (tests/test_forced_align_gpu.py).
int smoltts_lm_measure_rows(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev, const int32_t* row_pos_dev,
                            const int32_t* row_frame_dev, const int32_t* target_dev, int32_t n_rows, float* logprob_dev, void* stream) {
  ST_REQUIRE(s && grid_dev && row_slot_dev && row_pos_dev && row_frame_dev, SMOLTTS_E_INVALID, "lm_measure_rows: null argument");
  ST_REQUIRE(logprob_dev == nullptr || target_dev, SMOLTTS_E_INVALID, "lm_measure_rows: scores need targets");
  ST_REQUIRE(n_rows > 0 && n_rows <= s->max_rows, SMOLTTS_E_CAPACITY, "lm_measure_rows: %d rows, session holds %d", n_rows, s->max_rows);
  hipStream_t st = (hipStream_t)stream;
  const SmolttsEngine* e = s->e;
  const SmolttsLMConfig& c = e->cfg;
  ST_REQUIRE(c.dim % 32 == 0, SMOLTTS_E_INVALID, "lm_measure_rows: dim %% 32 != 0");
  ST_TRY(prefill_rows(s, grid_dev, row_slot_dev, row_pos_dev, n_rows, st, row_frame_dev, /*emit_head=*/logprob_dev != nullptr));
  if (logprob_dev) {
    for (int r0 = 0; r0 < n_rows; r0 += s->B) {
      const int n = n_rows - r0 < s->B ? n_rows - r0 : s->B;
      hipLaunchKernelGGL(x3_rows_gather_kernel, dim3(n), dim3(256), 0, st, s->x3n, s->ssq, r0, c.dim / 32, s->x3n2, s->xt);
      ST_CHECK_HIP(hipGetLastError());
      SmolttsGemm3Args a = base3(c.weight_format, e->arena + e->w.head, s->x3n2, n, c.vocab_size, c.dim, SMOLTTS_EPI_STORE);
      a.ssq_in_dev = s->xt; a.eps = c.norm_eps; a.out_dev = s->logits_slow; a.ldo = c.vocab_size;
      ST_TRY(launch_gemm3(a, st));
      ST_TRY(launch_score_rows(s->logits_slow, n, c.vocab_size, c.vocab_size, target_dev + r0, logprob_dev + r0, st));
    }
  }
  return launch_commit_embed(s, /*do_commit=*/0, 0, st);  // the rows went through x3n / ssq: re-publish the decode rows
}

int smoltts_lm_start_slots(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_pos_dev, const int32_t* slots_host,
                           const int32_t* last_row_host, int32_t n_slots, int32_t stop_on_eos, void* stream) {
  ST_REQUIRE(s && grid_dev && row_pos_dev && slots_host && last_row_host, SMOLTTS_E_INVALID, "lm_start_slots: null argument");
  ST_TRY(check_slot_lists("lm_start_slots", s, slots_host, last_row_host, n_slots, s->max_rows));
  hipStream_t st = (hipStream_t)stream;
  set_stop_on_eos(s, stop_on_eos);
  ST_TRY(stage_upload(s, slots_host, last_row_host, n_slots, st));
  return arm_slots(s, grid_dev, row_pos_dev, n_slots, st);
}

int smoltts_lm_decode(SmolttsSession* s, int32_t n_frames, void* stream) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "lm_decode: null session");
  ST_REQUIRE(s->prefilled, SMOLTTS_E_STATE, "lm_decode: call smoltts_lm_prefill first");
  ST_REQUIRE(n_frames >= 0, SMOLTTS_E_INVALID, "lm_decode: n_frames < 0");
  hipStream_t st = (hipStream_t)stream;
  pick_form(s);
  if (!graphs_enabled()) {
    for (int f = 0; f < n_frames; ++f) ST_TRY(run_decode_frame(s, st));
    return SMOLTTS_OK;
  }
  ST_TRY(ensure_graph(s, GRAPH_FRAME, st, [&](hipStream_t cap) { return run_decode_frame(s, cap); }));
  // Bounded run-ahead: a frame is ~230 AQL packets, and nothing stops a caller from queueing hundreds of frames.  The
  // hardware queue holds 16K packets; the runtime copes with a full ring, but a profiler that rewrites every dispatch into
  // several packets (rocprofv3 --pmc: counter start / stop + serialisation barriers around each kernel) overflows its
  // intercept queue and the run hangs behind the queued graph launches (round 1: gpurun_out/probe_d.log stops at the
  // first un-synchronised run of 63 frame graphs, while 3 frames per synchronisation completed).  So the host never
  // runs more than SMOLTTS_MAX_FRAMES_IN_FLIGHT frames ahead: it records an event every half limit and, before queueing
  // more, waits for the event of two groups ago -- the GPU queue never drains, the host merely stops piling up packets.
  // Frames are launched `multi_frames` at a time where that many remain: every graph launch costs the GPU a gap between the
  // last node of one graph and the first of the next (measured: the frame rate of a 32-frame chunk rises by the gaps saved).
  if (!s->multi_fixed && n_frames >= 2) {  // follows the calls: a later, longer call (a tick after a 2-frame warm-up) re-captures
    // (4 since round 4: with 181 launches per frame graphs of 1 / 2 / 4 / 8 / 16 frames give 27.5 / 27.58 / 27.61 / 27.47 / 27.25k
    // frames/s in the bench, profiles/r04_ab_frames_per_graph.txt; round 3's 216-launch frame was best at 8)
    const int want = n_frames < 4 ? n_frames : 4;
    if (want > s->multi_frames) {
      s->multi_frames = want;
      drop_graphs(s, 1u << GRAPH_MULTI);
    }
  }
  ST_TRY(ensure_multi_graph(s, n_frames, st));
  const hipGraphExec_t frame = s->graphs[GRAPH_FRAME][s->form], multi = s->graphs[GRAPH_MULTI][s->form];
  const int mf = multi ? s->multi_frames : 1;
  for (int f = 0; f < n_frames;) {
    if (s->flight_group > 0 && s->flight_count >= s->flight_group) {
      const int k = s->flight_cur;
      ST_CHECK_HIP(hipEventRecord(s->flight_ev[k], st));
      s->flight_live[k] = true;
      if (s->flight_live[k ^ 1]) ST_CHECK_HIP(hipEventSynchronize(s->flight_ev[k ^ 1]));
      s->flight_cur = k ^ 1;
      s->flight_count = 0;
    }
    if (mf > 1 && n_frames - f >= mf) {
      ST_CHECK_HIP(hipGraphLaunch(multi, st));
      s->flight_count += mf;
      f += mf;
    } else {
      ST_CHECK_HIP(hipGraphLaunch(frame, st));
      s->flight_count++;
      f++;
    }
  }
  return SMOLTTS_OK;
}

// Sampling mode of the session (reference GenerationSettings, lm/generate.py:12-16): temp / fast_temp <= 0
// select greedy argmax for the slow / depth tokens; min_p <= 0 disables the filter.  Takes effect from
// the next frame (the captured graph is dropped).
int smoltts_session_set_sampling(SmolttsSession* s, float temp, float fast_temp, float min_p, uint64_t seed) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_set_sampling: null session");
  ST_REQUIRE(min_p < 1.0f, SMOLTTS_E_INVALID, "session_set_sampling: min_p must be < 1");
  s->temp = temp; s->fast_temp = fast_temp; s->min_p = min_p; s->seed = seed;
  drop_graphs(s);
  return SMOLTTS_OK;
}

// Slot mode: per-slot entries (include/smoltts_hip.h), uploaded on `stream` by upload_slot_entries.
int smoltts_session_set_slot_sampling(SmolttsSession* s, const int32_t* slots_host, int32_t n, const float* temp_host,
                                      const float* fast_temp_host, const float* min_p_host, const uint64_t* seed_host, void* stream) {
  ST_REQUIRE(s && (n == 0 || (slots_host && temp_host && fast_temp_host && min_p_host && seed_host)), SMOLTTS_E_INVALID,
             "session_set_slot_sampling: null argument");
  return upload_slot_entries(
      s, "session_set_slot_sampling", slots_host, n, s->slot_tab_area + s->B, s->slot_tab_area, (hipStream_t)stream,
      [&](int i) -> int {
        ST_REQUIRE(temp_host[i] == temp_host[i] && fast_temp_host[i] == fast_temp_host[i] && min_p_host[i] >= 0.f && min_p_host[i] < 1.f,
                   SMOLTTS_E_INVALID, "session_set_slot_sampling: slot %d: temperatures must be numbers, 0 <= min_p < 1", slots_host[i]);
        return SMOLTTS_OK;
      },
      [&](int i, SmolttsSlotSampling& en) {
        en.temp = temp_host[i]; en.fast_temp = fast_temp_host[i]; en.min_p = min_p_host[i]; en.reserved = 0; en.seed = seed_host[i];
        set_form_bits(s, slots_host[i], FORM_SLOW | FORM_FAST, (en.temp > 0.f ? FORM_SLOW : 0) | (en.fast_temp > 0.f ? FORM_FAST : 0));
      });
}

// The filter entries of slot mode, uploaded like the sampling entries.  Whether any entry is on is a bit of the graph form
// (pick_form): no graph is dropped here.
int smoltts_session_set_slot_filters(SmolttsSession* s, const int32_t* slots_host, int32_t n, const float* top_p_host,
                                     const int32_t* top_k_host, const float* penalty_host, const int32_t* window_host, void* stream) {
  ST_REQUIRE(s && (n == 0 || (slots_host && top_p_host && top_k_host && penalty_host && window_host)), SMOLTTS_E_INVALID,
             "session_set_slot_filters: null argument");
  return upload_slot_entries(
      s, "session_set_slot_filters", slots_host, n, s->filt_tab_area + s->B, s->filt_tab_area, (hipStream_t)stream,
      [&](int i) -> int {
        const float r = penalty_host[i];
        ST_REQUIRE(top_p_host[i] >= 0.f && top_p_host[i] <= 1.f && top_k_host[i] >= 0 && (r == 0.f || (r >= 1.f && r <= SMOLTTS_FILTER_MAX_PENALTY)) &&
                       window_host[i] >= 0 && window_host[i] <= SMOLTTS_FILTER_MAX_WINDOW,
                   SMOLTTS_E_INVALID, "session_set_slot_filters: slot %d: 0 <= top_p <= 1, top_k >= 0, penalty 0 or in [1, %g], 0 <= window <= %d",
                   slots_host[i], (double)SMOLTTS_FILTER_MAX_PENALTY, SMOLTTS_FILTER_MAX_WINDOW);
        return SMOLTTS_OK;
      },
      [&](int i, SmolttsSlotFilters& en) {
        memset(&en, 0, sizeof(en));
        const float r = penalty_host[i];
        en.top_p = top_p_host[i] < 1.f ? top_p_host[i] : 0.f;
        en.top_k = top_k_host[i];
        if (r > 1.f && window_host[i] > 0) { en.penalty = r; en.inv_penalty = 1.0f / r; en.window = window_host[i]; }
        set_form_bits(s, slots_host[i], FORM_FILTER, en.top_p > 0.f || en.top_k > 0 || en.window > 0 ? FORM_FILTER : 0);
      });
}

// The length entries of slot mode, uploaded like the other two tables.  Whether any entry is on is bit 3 of the graph form
// (pick_form): no graph is dropped here.
int smoltts_session_set_slot_length(SmolttsSession* s, const int32_t* slots_host, int32_t n, const int32_t* min_frames_host,
                                    const float* eos_bias_host, void* stream) {
  ST_REQUIRE(s && (n == 0 || (slots_host && min_frames_host && eos_bias_host)), SMOLTTS_E_INVALID, "session_set_slot_length: null argument");
  return upload_slot_entries(
      s, "session_set_slot_length", slots_host, n, s->len_tab_area + s->B, s->len_tab_area, (hipStream_t)stream,
      [&](int i) -> int {
        const float b = eos_bias_host[i];
        ST_REQUIRE(min_frames_host[i] >= 0 && min_frames_host[i] <= SMOLTTS_LENGTH_MAX_FRAMES && b - b == 0.f, SMOLTTS_E_INVALID,
                   "session_set_slot_length: slot %d: 0 <= min_frames <= %d, eos_bias finite", slots_host[i], SMOLTTS_LENGTH_MAX_FRAMES);
        return SMOLTTS_OK;
      },
      [&](int i, SmolttsSlotLength& en) {
        memset(&en, 0, sizeof(en));
        en.min_frames = min_frames_host[i];
        en.eos_bias = eos_bias_host[i];
        set_form_bits(s, slots_host[i], FORM_LENGTH, en.min_frames > 0 || en.eos_bias != 0.f ? FORM_LENGTH : 0);
      });
}

size_t smoltts_session_align_bytes(SmolttsSession* s, int32_t n) {
  if (!s || n <= 0 || n > SMOLTTS_MAX_ALIGN_HEADS) return 0;
  return align_header_bytes(s) + (size_t)s->B * s->max_frames * n * 2 * sizeof(float);
}

// The chosen (layer, head) pairs and the caller's buffer for the window table and the rows.  The launches of a form with bit 5 are
// built from both, so the captured graphs of those forms are dropped; every window starts off.
int smoltts_session_set_align_heads(SmolttsSession* s, const int32_t* layers_host, const int32_t* heads_host, int32_t n, void* out_dev,
                                    size_t out_bytes) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_set_align_heads: null session");
  ST_REQUIRE(n >= 0 && n <= SMOLTTS_MAX_ALIGN_HEADS, SMOLTTS_E_CAPACITY, "session_set_align_heads: %d pairs (at most %d)", n,
             SMOLTTS_MAX_ALIGN_HEADS);
  ST_REQUIRE(n == 0 || (layers_host && heads_host && out_dev), SMOLTTS_E_INVALID, "session_set_align_heads: null argument");
  const SmolttsLMConfig& c = s->e->cfg;
  for (int i = 0; i < n; ++i) {
    ST_REQUIRE(layers_host[i] >= 0 && layers_host[i] < c.n_layer && heads_host[i] >= 0 && heads_host[i] < c.n_head, SMOLTTS_E_INVALID,
               "session_set_align_heads: pair %d = (layer %d, head %d) outside the model (%d layers, %d heads)", i, layers_host[i],
               heads_host[i], c.n_layer, c.n_head);
    ST_REQUIRE(i == 0 || layers_host[i - 1] <= layers_host[i], SMOLTTS_E_INVALID, "session_set_align_heads: pairs must be sorted by layer");
  }
  if (n > 0) {
    ST_REQUIRE(((uintptr_t)out_dev & 15) == 0, SMOLTTS_E_INVALID, "session_set_align_heads: the buffer must be 16-byte aligned");
    const size_t need = smoltts_session_align_bytes(s, n);
    ST_REQUIRE(out_bytes >= need, SMOLTTS_E_CAPACITY, "session_set_align_heads: buffer has %zu bytes, %zu needed", out_bytes, need);
  }
  // frames in flight, on any stream, may be replaying a graph of these forms or writing the buffer this call replaces
  ST_CHECK_HIP(hipDeviceSynchronize());
  drop_graphs(s, ~0u, FORM_ALIGN);
  s->n_align = 0; s->align_win = nullptr; s->align_up = nullptr; s->align_out = nullptr;
  for (int b = 0; s->h_form && b < s->B; ++b) set_form_bits(s, b, FORM_ALIGN, 0);
  if (n == 0) return SMOLTTS_OK;
  ST_CHECK_HIP(hipMemsetAsync(out_dev, 0, align_table_bytes(s), nullptr));
  ST_CHECK_HIP(hipStreamSynchronize(nullptr));
  for (int i = 0; i < n; ++i) { s->align_layer[i] = layers_host[i]; s->align_head[i] = heads_host[i]; }
  s->align_win = reinterpret_cast<int*>(out_dev);
  s->align_up = reinterpret_cast<int*>((char*)out_dev + align_table_bytes(s));
  s->align_out = reinterpret_cast<float*>((char*)out_dev + align_header_bytes(s));
  s->n_align = n;
  return SMOLTTS_OK;
}

namespace {
// out[slots[i]][*][*] = (-1, 0) for the n listed slots: "not measured"
__global__ __launch_bounds__(256) void align_fill_kernel(const int* slots, long per_slot, float* out) {
  float2* o = reinterpret_cast<float2*>(out) + (long)slots[blockIdx.y] * per_slot;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per_slot; i += (long)gridDim.x * 256) o[i] = make_float2(-1.f, 0.f);
}
}  // namespace

// The alignment windows of slot mode, uploaded like the other tables, and behind them the fill of the listed slots' rows.  Whether
// any window is on is bit 5 of the graph form.
int smoltts_session_set_slot_align(SmolttsSession* s, const int32_t* slots_host, int32_t n, const int32_t* t0_host,
                                   const int32_t* t1_host, void* stream) {
  ST_REQUIRE(s && (n == 0 || (slots_host && t0_host && t1_host)), SMOLTTS_E_INVALID, "session_set_slot_align: null argument");
  ST_REQUIRE(s->n_align > 0, SMOLTTS_E_STATE, "session_set_slot_align: call smoltts_session_set_align_heads first");
  hipStream_t st = (hipStream_t)stream;
  ST_TRY(upload_slot_entries(
      s, "session_set_slot_align", slots_host, n, reinterpret_cast<int2*>(s->align_up), reinterpret_cast<int2*>(s->align_win), st,
      [&](int i) -> int {
        ST_REQUIRE(t0_host[i] >= 0 && t0_host[i] <= s->max_seq && t1_host[i] >= 0 && t1_host[i] <= s->max_seq, SMOLTTS_E_INVALID,
                   "session_set_slot_align: slot %d: window [%d, %d) outside 0 .. %d", slots_host[i], t0_host[i], t1_host[i], s->max_seq);
        return SMOLTTS_OK;
      },
      [&](int i, int2& en) {
        en = make_int2(t0_host[i], t1_host[i]);
        set_form_bits(s, slots_host[i], FORM_ALIGN, en.y > en.x ? FORM_ALIGN : 0);
      }));
  if (n == 0) return SMOLTTS_OK;
  const long per_slot = (long)s->max_frames * s->n_align;
  const unsigned gx = (unsigned)((per_slot + 255) / 256 < 64 ? (per_slot + 255) / 256 : 64);
  hipLaunchKernelGGL(align_fill_kernel, dim3(gx, n), dim3(256), 0, st, s->align_up + 2 * s->B, per_slot, s->align_out);
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

// Diagnostic: the form the next frame launches would be built / replayed in (what pick_form would choose now), or a negative
// status.  Reads the host mirrors only; the session is not changed.
int smoltts_session_graph_form(SmolttsSession* s) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_graph_form: null session");
  return form_of(s);
}

int smoltts_session_alignment(SmolttsSession* s, float** out_dev, int32_t* n_pairs) {
  ST_REQUIRE(s && out_dev, SMOLTTS_E_INVALID, "session_alignment: null argument");
  *out_dev = s->n_align > 0 ? s->align_out : nullptr;
  if (n_pairs) *n_pairs = s->n_align;
  return SMOLTTS_OK;
}

// Measurement aid of this session only: while code >= 0, every launch of that kernel class inside this session's frames
// (GEMM epilogue code, N == n_filter when n_filter > 0; 100 / 101 = depth / slow attention) is issued twice; the captured
// graphs are dropped.  (t_dup - t_base) / extra launches is the kernel's duration in situ.
int smoltts_session_measure_duplicate(SmolttsSession* s, int32_t code, int32_t n_filter) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_measure_duplicate: null session");
  ST_REQUIRE(code != SMOLTTS_EPI_RESID, SMOLTTS_E_INVALID, "session_measure_duplicate: EPI_RESID launches are not idempotent");
  s->dup_code = code; s->dup_n = n_filter;
  drop_graphs(s);
  return SMOLTTS_OK;
}

// Launch-structure options of a session (both default on; switching one drops the captured graphs): the ids are the same
// either way -- the switches exist for A/B runs and tests.
int smoltts_session_set_option(SmolttsSession* s, int32_t option, int32_t value) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_set_option: null session");
  switch (option) {
    case SMOLTTS_OPT_QKV_TABLE: s->use_qkv_table = value != 0; break;
    case SMOLTTS_OPT_COMMIT_PICKS: s->commit_picks = value != 0; break;
    case SMOLTTS_OPT_SPLIT_ATTN: s->split_attn = value != 0; break;
    case SMOLTTS_OPT_STREAM_W: s->stream_w = value; break;
    case SMOLTTS_OPT_FUSE_DEPTH_ATTN: s->fuse_depth_attn = value != 0; break;
    case SMOLTTS_OPT_FUSE_PICK: s->fuse_pick = value != 0; break;
    case SMOLTTS_OPT_FP8_PREFILL: s->fp8_prefill = value != 0; break;
    default:
      set_error("session_set_option: unknown option %d", option);
      return SMOLTTS_E_INVALID;
  }
  drop_graphs(s);
  return SMOLTTS_OK;
}

// Forget the captured frame graph (the next smoltts_lm_decode captures it again).
int smoltts_session_drop_graph(SmolttsSession* s) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_drop_graph: null session");
  drop_graphs(s);
  return SMOLTTS_OK;
}

// Frames per multi-frame graph of this session (1 = single-frame graphs only, 0 = follow the decode calls again); with a
// stream and after a prefill, the graphs are captured here (a warm-up step) instead of inside the first decode call.
int smoltts_session_set_frames_per_graph(SmolttsSession* s, int32_t n, void* stream) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_set_frames_per_graph: null session");
  ST_REQUIRE(n >= 0 && n <= 16, SMOLTTS_E_INVALID, "session_set_frames_per_graph: %d frames per graph (0..16)", n);
  if (s->multi_env) n = s->multi_frames;  // SMOLTTS_FRAMES_PER_GRAPH wins (a profiler run pins one frame per graph)
  if (n != s->multi_frames) drop_graphs(s, 1u << GRAPH_MULTI);
  s->multi_frames = n;
  s->multi_fixed = n > 0;
  if (n > 0 && s->prefilled && graphs_enabled()) {
    hipStream_t st = (hipStream_t)stream;
    pick_form(s);
    ST_TRY(ensure_graph(s, GRAPH_FRAME, st, [&](hipStream_t cap) { return run_decode_frame(s, cap); }));
    ST_TRY(ensure_multi_graph(s, n, st));
  }
  return SMOLTTS_OK;
}

int smoltts_session_outputs(SmolttsSession* s, int32_t** codes_dev, int32_t** n_frames_dev, int32_t** done_dev,
                            float** margin_dev) {
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "session_outputs: null session");
  if (codes_dev) *codes_dev = s->codes;
  if (n_frames_dev) *n_frames_dev = s->frames;
  if (done_dev) *done_dev = s->done;
  if (margin_dev) *margin_dev = s->margin;
  return SMOLTTS_OK;
}

// Which slots score their slow token: host flags only (nothing is uploaded: a form with bit 4 scores every row, and the host reads
// the slots it asked about).  The first per-slot call of any kind enters slot mode; here its tables are zeroed on the null stream
// and waited for, since this call has no stream to order them on.
int smoltts_session_set_slot_score(SmolttsSession* s, const int32_t* slots_host, int32_t n, const int32_t* on_host) {
  ST_REQUIRE(s && (n == 0 || (slots_host && on_host)), SMOLTTS_E_INVALID, "session_set_slot_score: null argument");
  ST_REQUIRE(n >= 0 && n <= s->B, SMOLTTS_E_CAPACITY, "session_set_slot_score: %d entries, session holds %d slots", n, s->B);
  for (int i = 0; i < n; ++i) ST_TRY(check_slot("session_set_slot_score", slots_host[i], s->B));
  if (!s->slot_mode) {
    ST_TRY(enter_slot_mode(s, nullptr));
    ST_CHECK_HIP(hipStreamSynchronize(nullptr));
  }
  for (int i = 0; i < n; ++i) set_form_bits(s, slots_host[i], FORM_SCORE, on_host[i] != 0 ? FORM_SCORE : 0);
  return SMOLTTS_OK;
}

int smoltts_session_logprobs(SmolttsSession* s, float** logprob_dev, int32_t* stride) {
  ST_REQUIRE(s && logprob_dev, SMOLTTS_E_INVALID, "session_logprobs: null argument");
  *logprob_dev = s->logprob;
  if (stride) *stride = s->max_frames;
  return SMOLTTS_OK;
}

int smoltts_session_slow_logits(SmolttsSession* s, float** logits_dev, int32_t* ld) {
  ST_REQUIRE(s && logits_dev, SMOLTTS_E_INVALID, "session_slow_logits: null argument");
  *logits_dev = s->logits_slow;
  if (ld) *ld = s->e->cfg.vocab_size;
  return SMOLTTS_OK;
}

int smoltts_session_kv_cache(SmolttsSession* s, void** k_dev, void** v_dev, uint64_t* layer_bytes) {
  ST_REQUIRE(s && k_dev && v_dev && layer_bytes, SMOLTTS_E_INVALID, "session_kv_cache: null argument");
  const SmolttsLMConfig& c = s->e->cfg;
  *k_dev = s->kc; *v_dev = s->vc;
  *layer_bytes = (uint64_t)s->B * c.n_kv_head * s->max_seq * 64 * (s->kv_format == SMOLTTS_KV_BF16 ? 2 : 4);
  return SMOLTTS_OK;
}

int smoltts_session_fast_kv_cache(SmolttsSession* s, float** k_dev, float** v_dev, uint64_t* layer_bytes) {
  ST_REQUIRE(s && k_dev && v_dev && layer_bytes, SMOLTTS_E_INVALID, "session_fast_kv_cache: null argument");
  const SmolttsLMConfig& c = s->e->cfg;
  *k_dev = s->fkc; *v_dev = s->fvc;
  *layer_bytes = (uint64_t)s->B * c.fast_n_kv_head * c.n_fast * 64 * sizeof(float);
  return SMOLTTS_OK;
}

int smoltts_session_margin_at(SmolttsSession* s, int32_t** margin_at_dev) {
  ST_REQUIRE(s && margin_at_dev, SMOLTTS_E_INVALID, "session_margin_at: null argument");
  *margin_at_dev = s->margin_at;
  return SMOLTTS_OK;
}

size_t smoltts_prefix_kv_bytes(const SmolttsEngine* e, int32_t n_positions, int32_t kv_format) {
  if (!e || n_positions <= 0 || (kv_format != SMOLTTS_KV_F32 && kv_format != SMOLTTS_KV_BF16)) return 0;
  return PREFIX_HDR + prefix_data_bytes(e->cfg, n_positions, kv_format);
}

int smoltts_session_save_prefix(SmolttsSession* s, int32_t slot, int32_t n_positions, void* prefix_dev,
                                SmolttsPrefixHeader* header_host, void* stream) {
  ST_REQUIRE(s && prefix_dev, SMOLTTS_E_INVALID, "session_save_prefix: null argument");
  ST_REQUIRE(slot >= 0 && slot < s->B, SMOLTTS_E_INVALID, "session_save_prefix: slot %d out of range (%d slots)", slot, s->B);
  ST_REQUIRE(n_positions > 0 && n_positions + 1 <= s->max_seq, SMOLTTS_E_CAPACITY,
             "session_save_prefix: %d positions + 1 exceed max_seq %d", n_positions, s->max_seq);
  ST_REQUIRE(((uintptr_t)prefix_dev & 255) == 0, SMOLTTS_E_INVALID, "session_save_prefix: slab not 256-byte aligned");
  PrefixCopyArgs a = prefix_args(s, /*to_cache=*/0);
  a.header = prefix_header(s, n_positions);
  a.n = 1;
  a.d[0] = PrefixDesc{(char*)prefix_dev, slot, n_positions};
  ST_TRY(launch_prefix_copy(a, n_positions, (hipStream_t)stream));
  if (header_host) *header_host = a.header;
  return SMOLTTS_OK;
}

int smoltts_session_install_prefix(SmolttsSession* s, const void* const* prefix_dev_host, const SmolttsPrefixHeader* header_host,
                                   const int32_t* slots_host, int32_t n, void* stream) {
  ST_REQUIRE(s && prefix_dev_host && header_host && slots_host, SMOLTTS_E_INVALID, "session_install_prefix: null argument");
  ST_REQUIRE(n > 0 && n <= s->B, SMOLTTS_E_CAPACITY, "session_install_prefix: %d prefixes, session holds %d slots", n, s->B);
  const SmolttsLMConfig& c = s->e->cfg;
  for (int i = 0; i < n; ++i) {
    const SmolttsPrefixHeader& h = header_host[i];
    ST_REQUIRE(prefix_dev_host[i] && ((uintptr_t)prefix_dev_host[i] & 255) == 0, SMOLTTS_E_INVALID,
               "session_install_prefix: prefix %d is null or not 256-byte aligned", i);
    ST_REQUIRE(slots_host[i] >= 0 && slots_host[i] < s->B, SMOLTTS_E_INVALID, "session_install_prefix: slot %d out of range (%d slots)",
               slots_host[i], s->B);
    for (int j = 0; j < i; ++j)
      ST_REQUIRE(slots_host[j] != slots_host[i], SMOLTTS_E_INVALID, "session_install_prefix: slot %d listed twice", slots_host[i]);
    ST_REQUIRE(h.magic == SMOLTTS_PREFIX_MAGIC && h.head_dim == 64, SMOLTTS_E_INVALID, "session_install_prefix: prefix %d has no valid header", i);
    ST_REQUIRE(h.kv_format == s->kv_format, SMOLTTS_E_INVALID, "session_install_prefix: prefix %d holds kv format %d, the session %d", i,
               h.kv_format, s->kv_format);
    ST_REQUIRE(h.n_layer == c.n_layer && h.n_kv_head == c.n_kv_head, SMOLTTS_E_INVALID,
               "session_install_prefix: prefix %d is %d layers x %d kv heads, the session's model %d x %d", i, h.n_layer, h.n_kv_head,
               c.n_layer, c.n_kv_head);
    ST_REQUIRE(h.n_positions > 0 && h.n_positions + 1 <= s->max_seq, SMOLTTS_E_CAPACITY,
               "session_install_prefix: prefix %d of %d positions + 1 exceeds max_seq %d", i, h.n_positions, s->max_seq);
    ST_REQUIRE(h.data_bytes == prefix_data_bytes(c, h.n_positions, h.kv_format), SMOLTTS_E_INVALID,
               "session_install_prefix: prefix %d header size mismatch", i);
  }
  hipStream_t st = (hipStream_t)stream;
  for (int i0 = 0; i0 < n; i0 += SMOLTTS_PREFIX_MAX_INSTALL) {  // one launch per SMOLTTS_PREFIX_MAX_INSTALL prefixes
    PrefixCopyArgs a = prefix_args(s, /*to_cache=*/1);
    a.n = n - i0 < SMOLTTS_PREFIX_MAX_INSTALL ? n - i0 : SMOLTTS_PREFIX_MAX_INSTALL;
    int pmax = 0;
    for (int k = 0; k < a.n; ++k) {
      a.d[k] = PrefixDesc{(char*)prefix_dev_host[i0 + k], slots_host[i0 + k], header_host[i0 + k].n_positions};
      pmax = imax(pmax, a.d[k].n_positions);
    }
    ST_TRY(launch_prefix_copy(a, pmax, st));
  }
  return SMOLTTS_OK;
}

}  // extern "C"

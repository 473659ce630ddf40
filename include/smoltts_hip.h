/*
 * libsmoltts_hip.so — C ABI of the MI355X (gfx950) DualAR + Mimi decode hot path.
 *
 * The reference (EndlessReform/smoltts) has no FFI: its hot path is Python objects calling MLX
 * ops.  The seams this ABI replaces are (paths relative to the reference tree):
 *
 *   smoltts_lm_prefill / smoltts_lm_decode     <- RQTransformer.forward_generate + the 8x
 *       forward_generate_fast loop + argmax, i.e. one SingleBatchGenerator.__next__
 *       (mlx_inference/src/smoltts_mlx/lm/rq_transformer.py:173-220, lm/generate.py:59-171),
 *       generalised from batch 1 to B independent utterance slots
 *   smoltts_mimi_decode / smoltts_mimi_decode_step <- MimiModel.decode / decode_step
 *       (mlx_inference/src/smoltts_mlx/codec/mimi.py:88-104)
 *   smoltts_k_*                                 <- single operators (RMSNorm+Linear, RoPE, SDPA,
 *       SwiGLU, embed, argmax, conv-as-GEMM, LayerNorm) exported for unit parity tests
 *
 * Conventions: plain C types only; every pointer named *_dev is a device (HBM) address owned by
 * the caller (e.g. torch.Tensor.data_ptr()); the library never allocates or frees caller memory
 * and keeps all per-session state inside the caller-allocated slab, so one engine can serve many
 * sessions and one host thread per stream can drive it.  `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Every function returns 0 on success or a negative SMOLTTS_E_*
 * code; smoltts_last_error() returns a thread-local message.  No exceptions cross the boundary.
 */
#ifndef SMOLTTS_HIP_H
#define SMOLTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMOLTTS_ABI_VERSION 9

enum {
  SMOLTTS_OK = 0,
  SMOLTTS_E_INVALID = -1,   /* bad argument / unsupported shape */
  SMOLTTS_E_HIP = -2,       /* a HIP runtime call failed */
  SMOLTTS_E_STATE = -3,     /* call sequence error (e.g. decode before prefill) */
  SMOLTTS_E_CAPACITY = -4   /* slab / sequence / batch capacity exceeded */
};

const char* smoltts_last_error(void);
int smoltts_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Weight tile format ("T16x32"): a row-major [N][K] matrix is stored as tiles of 16 rows x 32
 * columns, tile (nt, kc) at element offset (nt * K/32 + kc) * 512, inside a tile in fp32-MFMA
 * fragment order: lane l = 16*q + r (r = row in tile, q = 0..3) owns the 8 consecutive
 * elements [r][8q .. 8q+8).  bf16 tiles: 16 bytes per lane, lane-linear (one 1 KiB wave load).
 * fp32 tiles: two 1 KiB halves, half h holds elements [r][8q+4h .. 8q+4h+4) of every lane.
 * N is padded to a multiple of 16 with zero rows; K must be a multiple of 32.
 * smoltts_amd/packing.py produces it.
 * ------------------------------------------------------------------------------------------- */

/* "W3" tiles (Mimi many-row GEMMs, smoltts_amd/csrc/gemm_b3.hip): an fp32 [N][K] matrix as three bf16 pieces hi + mid + lo
 * (== the fp32 value exactly); tile (nt, kc) is 3 KiB at (nt * K/32 + kc) * 3072: piece p at + p * 1024 in the bf16 T16x32
 * lane order above.  smoltts_amd/packing.py (tile_w3) produces it. */

/* Byte offsets into the LM weight arena. */
typedef struct SmolttsBlockWeights {
  uint64_t attn_norm;   /* fp32 [dim] */
  uint64_t wqkv;        /* bf16 T16x32 [(H+2KV)*64][dim], rows q|k|v */
  uint64_t wo;          /* bf16 T16x32 [dim][dim] */
  uint64_t ffn_norm;    /* fp32 [dim] */
  uint64_t w13;         /* bf16 T16x32 [2*inter][dim], row 2i = w1 row i, row 2i+1 = w3 row i */
  uint64_t w2;          /* bf16 T16x32 [dim][inter] */
} SmolttsBlockWeights;

#define SMOLTTS_MAX_LAYERS 64
#define SMOLTTS_MAX_FAST_LAYERS 16

typedef struct SmolttsLMConfig {
  int32_t dim, n_layer, n_head, n_kv_head, inter;
  int32_t fast_dim, n_fast_layer, fast_n_head, fast_n_kv_head, fast_inter;
  int32_t vocab_size, codebook_size, num_codebooks;
  int32_t n_fast;             /* fast steps per frame = num_codebooks - (duplicate_code_0 ? 0 : 1) */
  int32_t duplicate_code_0;
  int32_t depthwise_wte;
  int32_t has_fast_project_in;/* Linear(dim, fast_dim) with bias between slow hidden and fast input */
  int32_t embed_mask_mode;    /* 0: zero codebook-embedding sum where code0 == 0 (torch);
                                 1: zero it where the text token is outside [semantic_start, semantic_end] (MLX) */
  int32_t semantic_start_id, semantic_end_id, im_end_id;
  int32_t max_seq_len;        /* rows of the slow RoPE table */
  float norm_eps;
  int32_t weight_format;      /* SMOLTTS_W_BF16 (0) | SMOLTTS_W_FP8 (1): format of every "T16x32" Linear below.
                                 fp8: each matrix is its e4m3 tiles (rows * K bytes) followed by fp32 row scales
                                 [rows]; the depthwise head is one such block per step (stride rows * (K + 4) bytes) */
} SmolttsLMConfig;

typedef struct SmolttsLMWeights {
  uint64_t text_emb;      /* bf16 row-major [vocab][dim] */
  uint64_t codebook_emb;  /* bf16 row-major [codebook_size*num_codebooks][dim] */
  uint64_t fast_emb;      /* bf16 row-major [fast rows][fast_dim] */
  uint64_t norm;          /* fp32 [dim] */
  uint64_t head;          /* bf16 T16x32 [vocab][dim] (tied: same values as text_emb) */
  uint64_t fast_norm;     /* fp32 [fast_dim] */
  uint64_t fast_head;     /* bf16 T16x32 [n_fast*codebook_size][fast_dim]; step i uses rows
                             [i*codebook_size, (i+1)*codebook_size) (all steps share rows [0, cs)
                             when the checkpoint has no depthwise output) */
  uint64_t fast_head_step_stride; /* rows between consecutive steps: codebook_size or 0 */
  uint64_t fast_proj_w;   /* bf16 T16x32 [fast_dim][dim], only if has_fast_project_in */
  uint64_t fast_proj_b;   /* fp32 [fast_dim] */
  uint64_t rope;          /* fp32 [max_seq_len][32][2] (cos, sin) */
  uint64_t fast_rope;     /* fp32 [n_fast][32][2] */
  SmolttsBlockWeights layers[SMOLTTS_MAX_LAYERS];
  SmolttsBlockWeights fast_layers[SMOLTTS_MAX_FAST_LAYERS];
} SmolttsLMWeights;

enum {  /* storage of the slow transformer's KV cache */
  SMOLTTS_KV_F32 = 0,   /* fp32 (default): K/V exactly as computed */
  SMOLTTS_KV_BF16 = 1   /* bf16: K (after RoPE) and V rounded to nearest even once, when written; half the attention stream.
                           Changes the arithmetic (the oracle mirrors it with kv_bf16=True); the reference keeps K/V in its
                           activation dtype (lm/cache.py:6-22), i.e. bf16 for a bf16 checkpoint */
};

typedef struct SmolttsEngine SmolttsEngine;
typedef struct SmolttsSession SmolttsSession;

/* Engine = immutable model (config + weight arena pointers). The arena must outlive the engine. */
int smoltts_engine_create(const SmolttsLMConfig* cfg, const SmolttsLMWeights* offsets,
                          const void* arena_dev, size_t arena_bytes, SmolttsEngine** out);
void smoltts_engine_destroy(SmolttsEngine* e);

/* Derived table of an engine (optional, caller-owned memory like everything else): row e of the depth transformer's
 * embedding table (fast_embeddings, lm/generate.py:134-140) always enters depth layer 0 as RMSNorm(E[e]) -> wqkv, so its
 * q | k | v (before RoPE) can be looked up instead of computed: [rows][(fast heads + 2 fast kv heads) * 64] fp32 (150m: 73 MB).
 * With the table in place a frame has 7 launches fewer: the kernel that picks a depth code also gathers the next step's
 * layer-0 q / k / v (RoPE for its position applied on the way) and that step starts with its attention.  The values are the
 * decode path's own (same GEMM kernel, same accumulation order).
 *   smoltts_engine_fast_qkv_bytes   slab size (table + build scratch); 0 if the model has no depth step with a successor
 *   smoltts_engine_build_fast_qkv   fills the table (synchronises `stream`); the slab must outlive the engine's sessions.
 * Sessions use the table from their next captured frame on; smoltts_session_set_option(s, SMOLTTS_OPT_QKV_TABLE, 0) keeps one on
 * the GEMM path. */
size_t smoltts_engine_fast_qkv_bytes(const SmolttsEngine* e);
int smoltts_engine_build_fast_qkv(SmolttsEngine* e, void* slab_dev, size_t slab_bytes, void* stream);

/* Session = B utterance slots with KV caches, all inside one caller-allocated device slab.
 * max_rows bounds the prompt rows one smoltts_lm_prefill call may carry; max_frames bounds the
 * frames a slot may emit (output ring). */
size_t smoltts_session_slab_bytes(const SmolttsEngine* e, int32_t max_batch, int32_t max_seq,
                                  int32_t max_rows, int32_t max_frames);
int smoltts_session_create(SmolttsEngine* e, void* slab_dev, size_t slab_bytes, int32_t max_batch,
                           int32_t max_seq, int32_t max_rows, int32_t max_frames,
                           SmolttsSession** out);
/* The same with a choice of KV-cache storage (SMOLTTS_KV_*); the plain forms above are kv_format = SMOLTTS_KV_F32. */
size_t smoltts_session_slab_bytes_kv(const SmolttsEngine* e, int32_t max_batch, int32_t max_seq,
                                     int32_t max_rows, int32_t max_frames, int32_t kv_format);
int smoltts_session_create_kv(SmolttsEngine* e, void* slab_dev, size_t slab_bytes, int32_t max_batch,
                              int32_t max_seq, int32_t max_rows, int32_t max_frames, int32_t kv_format,
                              SmolttsSession** out);
void smoltts_session_destroy(SmolttsSession* s);

/* Prefill: run the slow transformer over n_rows prompt tokens (packed over utterances) and emit
 * frame 0 of every listed slot (slow head + n_fast depth steps, greedy).
 *   grid_dev      int32 [n_rows][1 + n_fast]   prompt columns (text id, code rows)
 *   row_slot_dev  int32 [n_rows]               slot of each row
 *   row_pos_dev   int32 [n_rows]               position of each row inside its utterance (0-based)
 *   slots_host    int32 [n_slots]              slots being (re)started (host memory)
 *   last_row_host int32 [n_slots]              index of each slot's last prompt row (host memory)
 * Slot state (position, frame counter, done flag) is reset for the listed slots; other slots are
 * untouched.  Asynchronous on `stream`. */
int smoltts_lm_prefill(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev,
                       const int32_t* row_pos_dev, int32_t n_rows, const int32_t* slots_host,
                       const int32_t* last_row_host, int32_t n_slots, int32_t stop_on_eos,
                       void* stream);

/* Chunked prompt prefill (BASELINE config 5): run the slow transformer over n_rows further prompt rows of
 * idle slots, filling their KV rows only — no frame is emitted and the listed slots stay idle, so decode
 * calls for the other slots may run between chunks.  Rows attend to their slot's earlier positions:
 * chunks of a slot must arrive in position order, and its last chunk goes through smoltts_lm_prefill
 * (row_pos continuing where the chunks stopped), which emits frame 0.  Arguments as smoltts_lm_prefill. */
int smoltts_lm_prefill_chunk(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev,
                             const int32_t* row_pos_dev, int32_t n_rows, const int32_t* slots_host,
                             const int32_t* last_row_host, int32_t n_slots, void* stream);

/* Prefill without the frame-0 tail (continuous batching: a decode call follows anyway): fills the KV rows of the prompt
 * and arms the listed slots so that the *next decode frame* takes the last prompt column as its input and emits the
 * slot's frame 0.  Same arguments as smoltts_lm_prefill; the ids produced are the same. */
int smoltts_lm_prefill_deferred(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev,
                                const int32_t* row_pos_dev, int32_t n_rows, const int32_t* slots_host,
                                const int32_t* last_row_host, int32_t n_slots, int32_t stop_on_eos,
                                void* stream);

/* Prompt prefill BESIDE the decode frames of the same session (ABI 5; serving: refilling a slot no longer stops the other slots).
 * Three calls replace smoltts_lm_prefill_deferred:
 *   smoltts_lm_park_slots   (frame stream) the listed slots -- idle, their previous tenants gone -- are frozen with their position
 *                           counter at pos_host[i] = the new prompt's last position T-1: the rows their idle decode steps write
 *                           land there, where the tenant's first frame writes anyway;
 *   smoltts_lm_prefill_side (any stream, once the park has RUN: wait for it on the host or by event) KV-cache rows of the prompt
 *                           rows, computed on a workspace of its own -- it shares nothing with concurrently running frames but the
 *                           KV rows 0 .. T-2 of the parked slots;
 *   smoltts_lm_start_slots  (frame stream, once the side call has finished) arms the slots exactly as the deferred prefill does:
 *                           the next decode frame takes the last prompt column as its input and emits frame 0.
 * Same arguments as smoltts_lm_prefill_deferred, split over the calls; grid_dev / row_pos_dev must stay valid until the start call
 * has run.  Ids are those of the in-line prefill (same kernels, same order; tests/test_side_prefill_gpu.py). */
int smoltts_lm_park_slots(SmolttsSession* s, const int32_t* slots_host, const int32_t* pos_host, int32_t n_slots, void* stream);
int smoltts_lm_prefill_side(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev, const int32_t* row_pos_dev,
                            int32_t n_rows, void* stream);
int smoltts_lm_start_slots(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_pos_dev, const int32_t* slots_host,
                           const int32_t* last_row_host, int32_t n_slots, int32_t stop_on_eos, void* stream);

/* (ABI 9, additive) Forced alignment: MEASURE n_rows further prompt rows of idle slots instead of only storing them (DESIGN.md
 * section 23).  The rows go through the slow transformer exactly as in a non-final smoltts_lm_prefill_chunk -- the same KV rows by
 * the same kernels in the same order, on the session's prefill workspace, chunks in position order -- but the call takes no slot
 * list and parks nothing: the rows' slots are idle and already parked at or behind the last position that will be measured
 * (smoltts_lm_park_slots).  No frame is emitted, no slot is armed, nothing is captured and no graph is dropped.
 *   Alignment rows: while heads are chosen (smoltts_session_set_align_heads), one smoltts_k_attention_align launch is queued behind
 *   the block of each layer that has chosen heads, with the workspace's q rows, the slots' windows (smoltts_session_set_slot_align)
 *   and row_frame_dev: row r writes out[row_slot[r]][row_frame_dev[r]][pair]; a row with row_frame_dev[r] < 0 (or >= max_frames)
 *   writes nothing.
 *   Scores: with logprob_dev != NULL the rows get the final norm and the slow head, max_batch rows at a time through the rows the
 *   decode frames' slow head writes (smoltts_session_slow_logits: overwritten), and logprob_dev[r] receives the score of column
 *   target_dev[r] under row r's fp32 logits -- the definition at smoltts_session_set_slot_score, no length entry and no penalty.  A
 *   row with target_dev[r] outside [0, vocab_size) writes nothing (the caller checks its ids on the host).  target_dev may be NULL
 *   when logprob_dev is.
 * grid_dev / row_slot_dev / row_pos_dev as in smoltts_lm_prefill; frame-stream call, like smoltts_lm_prefill_chunk. */
int smoltts_lm_measure_rows(SmolttsSession* s, const int32_t* grid_dev, const int32_t* row_slot_dev, const int32_t* row_pos_dev,
                            const int32_t* row_frame_dev, const int32_t* target_dev, int32_t n_rows, float* logprob_dev, void* stream);

/* Decode n_frames further frames for every slot of the session: each frame feeds the previous
 * column back (slow step at the slot's next position), then slow head + n_fast depth steps, all
 * greedy and on device; the frame loop is a captured hipGraph replayed n_frames times.  Slots that
 * are done (emitted <|im_end|> with stop_on_eos, reached max_frames, or filled their context: the next
 * token would land at position max_seq) are frozen.
 *
 * Host behaviour: the call queues graph launches on `stream` and returns, EXCEPT that the host never runs more than
 * SMOLTTS_MAX_FRAMES_IN_FLIGHT frames (environment, read when the session is created; default 64, 0 = unbounded) ahead of
 * the GPU: every half bound it records an event and, before queueing further, waits (hipEventSynchronize, blocking the
 * calling thread) for the event of two groups ago.  One host thread that drives several sessions therefore overlaps them
 * only up to that many frames each.  Frames go out `frames per graph` at a time where that many remain (see
 * smoltts_session_set_frames_per_graph; SMOLTTS_FRAMES_PER_GRAPH overrides).  The library never inspects a profiler's
 * environment: a counter-collecting profiler run sets SMOLTTS_MAX_FRAMES_IN_FLIGHT=2 SMOLTTS_FRAMES_PER_GRAPH=1 itself
 * (tools/collect_pmc.sh). */
int smoltts_lm_decode(SmolttsSession* s, int32_t n_frames, void* stream);

/* Frames captured into one multi-frame graph of this session: n = 1 single-frame graphs only, 2..16 that many, 0 = follow
 * the decode calls (min(n_frames, 4) of the largest call so far -- the default).  Called after a prefill with n > 0 it also
 * captures the graphs now (on `stream`), so that the first decode call of a request does not pay the capture. */
int smoltts_session_set_frames_per_graph(SmolttsSession* s, int32_t n, void* stream);
/* Launch-structure options of a session (A/B runs, tests): the ids produced are the same either way; the captured graphs are dropped.
 *   SMOLTTS_OPT_QKV_TABLE     depth layer-0 q | k | v out of the engine's fast_qkv table where it has been built (default 1)
 *   SMOLTTS_OPT_COMMIT_PICKS  the frame's slow token and last depth code picked inside the commit kernel instead of in
 *                             launches of their own (default 1)
 *   SMOLTTS_OPT_SPLIT_ATTN    decode attention over the slow cache with the keys of a (row, kv head) pair on two workgroups,
 *                             merged in part order inside the launch (<= 128 pairs, i.e. B <= 32 at 4 kv heads; default 1).
 *                             fp32 sums in a different order than the one-workgroup kernel: same ids except at near-ties
 *   SMOLTTS_OPT_FUSE_DEPTH_ATTN  (ABI 5) depth steps 1..: the attention over the <= 8-entry cache is worked out by the wo launch
 *                             itself (SmolttsGemm3Args.attn_q_dev) instead of by a launch of its own (default 1; applies where
 *                             smoltts_gemm3_attn_fusable); every sum formed in the stand-alone kernels' order: bit-identical to them */
#define SMOLTTS_OPT_QKV_TABLE 1
#define SMOLTTS_OPT_COMMIT_PICKS 2
#define SMOLTTS_OPT_SPLIT_ATTN 3
#define SMOLTTS_OPT_FUSE_DEPTH_ATTN 5
#define SMOLTTS_OPT_FP8_PREFILL 7  /* (ABI 5; default 0) engines with fp8 weights: prompt prefills of >= 256 rows run their GEMMs with fp8
                                      activations on the fp8 MFMA (SmolttsGemm3Args.fp8_activations): faster first chunk, prompt KV rows
                                      approximate -- ids are then no longer guaranteed to equal the reference greedy decode */
#define SMOLTTS_OPT_FUSE_PICK 6  /* (ABI 5) greedy depth codes picked inside the next step's layer-0 attention + wo launch (SmolttsPickArgs)
                                    instead of by a launch of their own (default 1; needs the fast_qkv table, the fused depth
                                    attention and greedy depth tokens); same ids, same gap records */
#define SMOLTTS_OPT_STREAM_W 4  /* value = mask of SMOLTTS_STREAM_W_*: which weights of a decode frame are loaded with the non-temporal
                                  hint (read once per frame: keeping them out of the caches leaves room for the depth layers'
                                  weights, which are re-read for each of the 8 depth steps) */
#define SMOLTTS_STREAM_W_SLOW 1        /* the slow transformer's blocks */
#define SMOLTTS_STREAM_W_SLOW_HEAD 2   /* the slow head */
#define SMOLTTS_STREAM_W_DEPTH_HEAD 4  /* the depth head slices (one per step) */
#define SMOLTTS_STREAM_W_DEPTH_W13 8   /* experiments: parts of the depth blocks */
#define SMOLTTS_STREAM_W_DEPTH_W2 16
#define SMOLTTS_STREAM_W_DEPTH_QKVO 32
#define SMOLTTS_STREAM_W_SLOW_ONLY_W13 64   /* with _SLOW: only the slow blocks' w1|w3 (the rest of the slow weights stays cacheable) */
#define SMOLTTS_STREAM_W_SLOW_NOT_W13 128   /* with _SLOW: everything of the slow blocks but w1|w3 */
/* default: the slow blocks' w1|w3 (94 MB at 150m) and the slow head stream past the caches; what is left -- the depth
 * transformer (94 MB, re-read 8 times per frame) and the rest of the slow blocks (83 MB) -- fits the 256 MB Infinity Cache together */
#define SMOLTTS_STREAM_W_DEFAULT (SMOLTTS_STREAM_W_SLOW | SMOLTTS_STREAM_W_SLOW_HEAD | SMOLTTS_STREAM_W_SLOW_ONLY_W13)
int smoltts_session_set_option(SmolttsSession* s, int32_t option, int32_t value);

/* Sampling mode (reference GenerationSettings, lm/generate.py:12-16): temp / fast_temp <= 0 select
 * greedy argmax for the slow / depth tokens (the default), otherwise exact categorical sampling from
 * softmax(logits / temp) with a counter-based generator keyed by (seed, slot, frame, step); min_p > 0
 * keeps only tokens with p >= min_p * p_max (applied to the depth tokens only when fast_temp > 0). */
int smoltts_session_set_sampling(SmolttsSession* s, float temp, float fast_temp, float min_p, uint64_t seed);

/* (ABI 6) Per-slot sampling ("slot mode").  One entry per slot; a slot whose temp (slow token) / fast_temp (depth codes) is <= 0
 * picks that token greedily (torch.argmax, margin bookkeeping as above).  min_p is the effective cut (0 = none; applied to the
 * depth codes only when fast_temp > 0).  A sampled row of slot mode draws with the REQUEST key
 *   u = uniform01(seed, 0, frames[slot], step, column)       (smoltts_amd/csrc/argmax_dev.h)
 * -- the entry's own seed, unsalted, and the slot's frame counter (0 at the tenant's frame 0): the draw does not depend on the
 * slot, on the slot's earlier tenants or on the other slots of the batch.  Step 0 is the slow token, step i the depth code i - 1. */
typedef struct SmolttsSlotSampling {
  float temp;
  float fast_temp;
  float min_p;
  uint32_t reserved;  /* 0 */
  uint64_t seed;
} SmolttsSlotSampling;

/* Set the entries of slots_host[0 .. n) (the arrays are read before the call returns).  The first call switches the session to
 * slot mode for good (every other slot starts greedy, seed 0); smoltts_session_set_sampling no longer affects the picks then.
 * The entries are uploaded on `stream` from a pinned staging ring of the session (the host never waits for the stream) and
 * are seen by the first pick behind them on that stream.  The session's frame graphs come in one captured set per form --
 * slow token greedy for every slot or not, depth codes greedy for every slot or not -- chosen from the entries at each decode /
 * prefill call: a form where no slot samples is exactly the session-wide greedy launch sequence.  Calls that set entries
 * and the frames that read them must be ordered on one stream. */
int smoltts_session_set_slot_sampling(SmolttsSession* s, const int32_t* slots_host, int32_t n, const float* temp_host,
                                      const float* fast_temp_host, const float* min_p_host, const uint64_t* seed_host, void* stream);

/* (ABI 6, additive) Per-slot filters of the sampled picks: top_k, top_p and a windowed repetition penalty, beside the slot's
 * SmolttsSlotSampling entry.  They apply to a row only when that row is sampled (temp > 0 for the slow token, fast_temp > 0 for the
 * depth codes: the rule min_p follows); a greedy row ignores them.  On the fp32 logits x of the row, in this order:
 *   1. penalty r > 1 over a window of W frames: the ids this step produced in the request's last min(W, frame counter) frames
 *      (step 0: the slow id, step i: depth code i - 1; read from the session's codes array, so the history restarts with the frame
 *      counter) get x' = x * inv_penalty if x > 0, else x * penalty -- one rounded fp32 multiply; the row maximum is the penalised one;
 *   2. top_k > 0: keep the columns with x' >= the k-th largest x' (duplicates counted, ties kept);
 *   3. 0 < top_p < 1, on the columns top_k kept: z = (x' - max) * (1 / temp), p = exp(z); keep column j iff the mass of the kept
 *      columns with z > z_j is < top_p * total (a threshold: ties stand or fall together);
 *   4. min_p and the Gumbel key of the request as before.
 * An all-zero entry is off, and a slot whose entry is off picks exactly what it picks without the table.  The thresholds are
 * found by bisection with order-independent (integer-valued) reductions: the ids do not depend on the slot or the batch.
 * Host model: smoltts_amd/sampling.py (filtered_keys / filtered_pick). */
typedef struct SmolttsSlotFilters {
  float top_p;        /* <= 0 or >= 1: off */
  int32_t top_k;      /* <= 0 or >= columns: off */
  float penalty;      /* <= 1: off */
  float inv_penalty;  /* fp32(1 / penalty) */
  int32_t window;     /* frames of history, 1 .. 64; <= 0: off */
  int32_t reserved[3];
} SmolttsSlotFilters;
#define SMOLTTS_FILTER_MAX_WINDOW 64
#define SMOLTTS_FILTER_MAX_PENALTY 1000.0f /* what this entry accepts; the public interface (config.RequestSampling) stops at 10 */

/* Set the filter entries of slots_host[0 .. n): top_p in [0, 1] (0 and 1: off), top_k >= 0 (0: off), penalty 0 or in
 * [1, SMOLTTS_FILTER_MAX_PENALTY] (0 and 1: off), window in [0, 64] (0: penalty off).  Uploaded like the sampling entries (pinned
 * ring, no host wait, ordered on `stream`); the first call of either kind puts the session in slot mode.  "Some slot's entry is on"
 * is one more bit of the graph form: while every entry is off, the frames launch exactly the kernels they launch without this table. */
int smoltts_session_set_slot_filters(SmolttsSession* s, const int32_t* slots_host, int32_t n, const float* top_p_host,
                                     const int32_t* top_k_host, const float* penalty_host, const int32_t* window_host, void* stream);

/* (ABI 9, additive) Per-slot length control of the slow pick: a minimum number of frames and a bias on the end-of-speech logit,
 * beside the slot's other two entries.  Unlike the filters it acts on greedy and sampled rows alike.  On the fp32 slow logits x of
 * the row (step 0 only; the depth codes are never touched), in front of everything else the pick does:
 *   1. x[im_end] = x[im_end] + eos_bias            -- one rounded fp32 add;
 *   2. if frames[slot] < min_frames: x[im_end] = -inf.
 * The repetition penalty, top_k, top_p, min_p, the Gumbel key and the greedy top-2 (the margin bookkeeping) all see the patched
 * row.  frames[slot] is the slot's frame counter, read on the device when the row is picked (a multi-frame graph crosses the
 * boundary inside one replay): with min_frames = m the earliest frame whose slow id can be im_end is frame index m, so at least
 * m audio frames precede it.  An all-zero entry is off, and a slot whose entry is off picks exactly what it picks without the
 * table.  Host model: smoltts_amd/sampling.py (length_patch). */
typedef struct SmolttsSlotLength {
  int32_t min_frames;   /* <= 0: off.  While frames[slot] < min_frames the im_end column cannot be picked */
  float   eos_bias;     /* 0: off.  Added to the im_end logit: one rounded fp32 add */
  int32_t reserved[2];  /* 0 */
} SmolttsSlotLength;
#define SMOLTTS_LENGTH_MAX_FRAMES 1073741824 /* 2^30: what this entry accepts; the public interface (config.RequestSampling) stops at 1024 */

/* Set the length entries of slots_host[0 .. n): min_frames in [0, SMOLTTS_LENGTH_MAX_FRAMES] (0: off), eos_bias any finite number
 * (0: off).  Uploaded like the other two tables (pinned ring, no host wait, ordered on `stream`); the first call of any of the three
 * puts the session in slot mode.  "Some slot's length entry is on" is bit 3 of the graph form.  In a form that has it the slow token
 * is picked from the row of logits (as in a form whose slow token is sampled), not from the head GEMM's tile candidates, which hold
 * unpatched values.  While every entry is off, the frames launch exactly the kernels they launch without this table. */
int smoltts_session_set_slot_length(SmolttsSession* s, const int32_t* slots_host, int32_t n, const int32_t* min_frames_host,
                                    const float* eos_bias_host, void* stream);

/* (ABI 9, additive) Score the slow token of slots_host[0 .. n): on_host[i] != 0 switches slot slots_host[i]'s score on.  Host flags
 * only: nothing is uploaded and the call takes no stream (the first per-slot call of any kind puts the session in slot mode; when
 * this is that call it waits for the device once).  The score of a frame is the log-probability, at temperature 1, of the slow id
 * the slot emitted, under the fp32 row x' its pick saw -- after the length entry and the repetition penalty, before temperature,
 * top_k, top_p and min_p:
 *   z_j = fp32(x'_j - max x');  q_j = floor(expf(z_j) * 2^40);  S = sum_j q_j (exact);  lp = z_picked - (log S - 40 ln 2), as fp32.
 * "Some slot scores" is bit 4 of the graph form.  In a form that has it the slow token is picked from the row of logits (as in a
 * form whose slow token is sampled) and every row is scored; no id changes.  While no slot scores, the frames launch exactly the
 * kernels they launch without this call.  Depth codes are not scored.  Host model: smoltts_amd/sampling.py (pick_logprob). */
int smoltts_session_set_slot_score(SmolttsSession* s, const int32_t* slots_host, int32_t n, const int32_t* on_host);

/* (ABI 9, additive) The scores: float [max_batch][*stride], entry [slot][f] written with frame f of a slot while the form has bit
 * 4 (any slot of such a form, asked or not); other entries keep what they held.  stride = max_frames; may be NULL. */
int smoltts_session_logprobs(SmolttsSession* s, float** logprob_dev, int32_t* stride);

/* (ABI 9, additive) Where chosen heads of the slow attention look while a frame is produced.  For a decode row of slot s at position
 * pos that produces frame f, and a chosen (layer, query head) pair: p = the softmax over keys 0 .. pos of that head, the distribution
 * the slow attention weighs V with; over the slot's text window [t0, t1) clipped to the visible keys
 *   m = sum_{j in window} p_j  (the mass on the text),   s1 = sum_{j in window} p_j (j - t0)  (the first moment)
 * are written to out[s][f][pair] = (m, s1); the host forms the centroid s1 / m.  Host model and the fit to times: smoltts_amd/align.py.
 *
 * smoltts_session_set_align_heads chooses the pairs: n <= SMOLTTS_MAX_ALIGN_HEADS (layer, head) pairs sorted by layer (ties in any
 * order), each inside the model; n = 0 turns the feature off (out_dev may then be NULL).  out_dev is caller-owned, 16-byte aligned,
 * out_bytes >= smoltts_session_align_bytes(s, n): the call places the session's [max_batch] window table (and the upload area of
 * smoltts_session_set_slot_align) in front of the float rows [max_batch][max_frames][n][2] and zeroes the table on the null stream
 * (waited for: the call takes no stream).  The session slab is untouched.  The call first waits for the whole device
 * (hipDeviceSynchronize), with n = 0 as well: frames in flight on any stream may be replaying a graph of a form with bit 5 or writing
 * the buffer being replaced; then the captured graphs of those forms are dropped.  Not for the serving loop's hot path.
 * smoltts_session_align_bytes: the size of that buffer for n pairs (0 for n outside 1 .. SMOLTTS_MAX_ALIGN_HEADS): a size helper,
 * as smoltts_session_slab_bytes is for the slab. */
#define SMOLTTS_MAX_ALIGN_HEADS 16
size_t smoltts_session_align_bytes(SmolttsSession* s, int32_t n);
int smoltts_session_set_align_heads(SmolttsSession* s, const int32_t* layers_host, const int32_t* heads_host, int32_t n, void* out_dev,
                                    size_t out_bytes);

/* (ABI 9, additive) Set the windows of slots_host[0 .. n): 0 <= t0, t1 <= max_seq; t1 <= t0 switches the slot's measurement off.
 * Uploaded like the slot length entries (pinned ring, no host wait, ordered on `stream`; the first per-slot call of any kind puts
 * the session in slot mode), and behind the upload the rows out[slot][*][*] of the listed slots are filled with (m, s1) = (-1, 0),
 * "not measured": a frame whose slow step ran as a prefill row (frame 0 after smoltts_lm_prefill) keeps that value.  "Some slot's
 * window is on" is bit 5 of the graph form: in a form that has it every decode frame queues one launch behind the block of each
 * layer that has chosen heads, in the frame's one serial chain.  A row writes nothing while its slot is masked, its window is off,
 * frames[slot] >= max_frames or its position lies outside the cache.  No id changes; while every window is off, the frames launch
 * exactly the kernels they launch without this call. */
int smoltts_session_set_slot_align(SmolttsSession* s, const int32_t* slots_host, int32_t n, const int32_t* t0_host,
                                   const int32_t* t1_host, void* stream);

/* (ABI 9, additive) Diagnostic, for tests: reads host state only and changes nothing.  The graph form the next frame launches
 * would take (>= 0: bit 0 / 1 = some slot samples its slow token / its
 * depth codes, bit 2 = filters, bit 3 = length entries, bit 4 = scores, bit 5 = alignment windows), or a negative status. */
int smoltts_session_graph_form(SmolttsSession* s);

/* (ABI 9, additive) The rows: float [max_batch][max_frames][*n_pairs][2] inside the caller's buffer (NULL, 0 while off). */
int smoltts_session_alignment(SmolttsSession* s, float** out_dev, int32_t* n_pairs);

/* (ABI 9, additive) Diagnostic: the slow head's fp32 logits of the latest frame, [max_batch][*ld] (ld = vocab_size; may be NULL),
 * as the slow pick read them -- in front of the length entry and the penalty.  Overwritten by every frame. */
int smoltts_session_slow_logits(SmolttsSession* s, float** logits_dev, int32_t* ld);

/* Device pointers to the session's results (valid for the session's lifetime):
 *   codes      int32 [max_batch][max_frames][1 + n_fast]   emitted columns (slow id, codes)
 *   n_frames   int32 [max_batch]                            frames emitted so far per slot
 *   done       int32 [max_batch]
 *   margin     float [max_batch]   smallest top-1/top-2 logit gap seen by the slot's argmaxes */
int smoltts_session_outputs(SmolttsSession* s, int32_t** codes_dev, int32_t** n_frames_dev,
                            int32_t** done_dev, float** margin_dev);
/* Diagnostics: the slow transformer's KV cache of the session -- k / v [n_layer][max_batch][n_kv_head][max_seq][64] in the session's
 * kv format (fp32 or bf16), `layer_bytes` apart per layer.  Read-only use (tests compare cache rows between launch structures). */
int smoltts_session_kv_cache(SmolttsSession* s, void** k_dev, void** v_dev, uint64_t* layer_bytes);
/* (ABI 6, additive) Diagnostics: the depth transformer's KV cache of the session -- k / v
 * [n_fast_layer][max_batch][fast_n_kv_head][n_fast][64], fp32 always (whatever the session's kv format), `layer_bytes` apart per
 * layer; k is the value after RoPE.  Entry i of a slot holds depth step i of the slot's latest frame until the next frame
 * overwrites it.  Read-only use (tests hold the rows to a float64 oracle, per layer and step). */
int smoltts_session_fast_kv_cache(SmolttsSession* s, float** k_dev, float** v_dev, uint64_t* layer_bytes);
/* int32 [max_batch]: where each slot's smallest gap occurred, frame * 64 + step (step 0 = slow id, i = depth code i-1). */
int smoltts_session_margin_at(SmolttsSession* s, int32_t** margin_at_dev);

/* (ABI 6) Voice prefixes: the slow KV rows of a prompt prefix (a cloned voice's speaker turns), computed once and copied into the
 * slots of later requests, whose own turns are then prefilled from position P on.  A prefix slab is caller-owned device memory,
 * 256-byte aligned, of smoltts_prefix_kv_bytes(): a header (SmolttsPrefixHeader, padded to 256 bytes), then K and V of positions
 * [0, P) as [n_layer][K | V][n_kv_head][P][64] in the KV format it was saved from -- exactly the bytes the cache holds.  The same
 * header is returned on the host by the save call; the install call checks that host copy against the session and the install
 * kernel checks the slab's own header against it (a slab with another header is left out of the copy). */
#define SMOLTTS_PREFIX_MAGIC 0x58464250u  /* "PBFX" */
#define SMOLTTS_PREFIX_MAX_INSTALL 16     /* prefixes per install launch; more are installed by further launches */
typedef struct SmolttsPrefixHeader {
  uint32_t magic;       /* SMOLTTS_PREFIX_MAGIC */
  int32_t n_positions;  /* P */
  int32_t n_layer;
  int32_t n_kv_head;
  int32_t kv_format;    /* SMOLTTS_KV_* */
  int32_t head_dim;     /* 64 */
  uint64_t data_bytes;  /* bytes after the 256-byte header */
} SmolttsPrefixHeader;
/* Bytes of a prefix slab of n_positions positions (0 for bad arguments). */
size_t smoltts_prefix_kv_bytes(const SmolttsEngine* e, int32_t n_positions, int32_t kv_format);
/* Copy rows [0, n_positions) of `slot`'s slow KV cache (every layer and kv head) into prefix_dev, and the header in front of them;
 * *header_host (may be NULL) receives the header.  Asynchronous on `stream`: the rows are those the stream has written by then. */
int smoltts_session_save_prefix(SmolttsSession* s, int32_t slot, int32_t n_positions, void* prefix_dev,
                                SmolttsPrefixHeader* header_host, void* stream);
/* Write prefix prefix_dev_host[i] (header header_host[i], as returned by the save) into rows [0, P_i) of slot slots_host[i], for n
 * distinct slots with any mix of prefixes and lengths: one launch per SMOLTTS_PREFIX_MAX_INSTALL prefixes, descriptors passed by
 * value.  Rows >= P_i of those slots and every other slot are untouched.  Allocates, uploads and synchronises nothing (capturable).
 * Refused (nothing launched): a null or misaligned pointer, a slot out of range or listed twice, a header of another kv format,
 * layer or kv-head count, or P_i + 1 > max_seq.  The slots' position counters are not touched: the prompt rows that follow go
 * in at row_pos P_i, ... (a prefill, a chunk, or smoltts_lm_park_slots + smoltts_lm_prefill_side) before the slots decode again. */
int smoltts_session_install_prefix(SmolttsSession* s, const void* const* prefix_dev_host, const SmolttsPrefixHeader* header_host,
                                   const int32_t* slots_host, int32_t n, void* stream);

/* ------------------------------------------------------------------------------ Mimi decoder */
#define SMOLTTS_MIMI_MAX_LAYERS 16

typedef struct SmolttsMimiLayerWeights {
  uint64_t ln1_w, ln1_b;     /* fp32 [512] */
  uint64_t wqkv;             /* fp32 T16x32 [1536][512]; q and k rows permuted per head so that the
                                half-split RoPE pair (j, j+32) sits at rows (2j, 2j+1) */
  uint64_t wo;               /* fp32 T16x32 [512][512] */
  uint64_t ls1;              /* fp32 [512] attention layer scale */
  uint64_t ln2_w, ln2_b;
  uint64_t fc1;              /* fp32 T16x32 [2048][512] */
  uint64_t fc2;              /* fp32 T16x32 [512][2048] */
  uint64_t ls2;
  uint64_t wqkv3, wo3, fc13, fc23;  /* the same four matrices as "W3" tiles (below); 0 = absent (fp32 kernels only) */
} SmolttsMimiLayerWeights;

typedef struct SmolttsMimiConv {
  uint64_t w;                /* fp32 T16x32 [N][K] GEMM form, see DESIGN.md "convolutions as GEMMs" */
  uint64_t b;                /* fp32 [N] (bias repeated per phase for transposed convs) */
  int32_t cin, cout, k, stride, transposed;
  uint64_t w3;               /* the same GEMM matrix as "W3" tiles; 0 = absent */
} SmolttsMimiConv;

typedef struct SmolttsMimiConfig {
  int32_t num_codebooks;     /* codebooks consumed per frame (8) */
  int32_t n_layers;          /* decoder transformer layers (8) */
  int32_t window;            /* attention window in positions; 0 = unbounded (reference MLX behaviour) */
  int32_t max_positions;     /* rows of the RoPE table / KV capacity per slot (2 per frame) */
} SmolttsMimiConfig;

typedef struct SmolttsMimiWeights {
  uint64_t rvq_table;        /* fp32 [num_codebooks][2048][512]: codebook rows already projected by
                                their group's output_proj */
  uint64_t upsample_w;       /* fp32 [4][512] depthwise ConvTranspose taps, tap-major */
  uint64_t rope;             /* fp32 [max_positions][32][2] */
  SmolttsMimiLayerWeights layers[SMOLTTS_MIMI_MAX_LAYERS];
  SmolttsMimiConv convs[14]; /* SEANet decoder in execution order: conv0, then per ratio
                                (convtr, res.conv3, res.conv1) x4, then the final conv (14 in all) */
  uint64_t final_w;          /* fp32 [3][64]: the output conv (64 -> 1, k3) tap-major, for the fused last stage; its bias is
                                convs[13].b */
} SmolttsMimiWeights;

typedef struct SmolttsMimi SmolttsMimi;
typedef struct SmolttsMimiSession SmolttsMimiSession;

int smoltts_mimi_create(const SmolttsMimiConfig* cfg, const SmolttsMimiWeights* offsets,
                        const void* arena_dev, size_t arena_bytes, SmolttsMimi** out);
void smoltts_mimi_destroy(SmolttsMimi* m);

/* Session: per-slot streaming state (upsample carry, transformer KV, conv halos) + scratch for
 * up to max_chunk_frames frames per slot per call. */
size_t smoltts_mimi_slab_bytes(const SmolttsMimi* m, int32_t max_batch, int32_t max_chunk_frames);
int smoltts_mimi_session_create(SmolttsMimi* m, void* slab_dev, size_t slab_bytes, int32_t max_batch,
                                int32_t max_chunk_frames, SmolttsMimiSession** out);
void smoltts_mimi_session_destroy(SmolttsMimiSession* s);
/* Forget all streaming state of the session (start new utterances in every slot). */
int smoltts_mimi_reset(SmolttsMimiSession* s, void* stream);

/* Forget the streaming state of the listed slots only (slots_host: host memory): the other slots' streams continue.
 * Every slot keeps its own transformer position, so streams of different utterances can share one session. */
int smoltts_mimi_reset_slots(SmolttsMimiSession* s, const int32_t* slots_host, int32_t n_slots, void* stream);

/* (ABI 6) Reference-quirk switch, default 0.  SMOLTTS_MIMI_OPT_STATELESS_UPSAMPLE = 1: every decode call up-samples its frames
 * as if they were the whole utterance (no tap overlap carried in from the previous call), which is what the reference's
 * decode_step does (mlx_inference/src/smoltts_mlx/codec/mimi.py:73-77,101-104: self.upsample(embeddings) on the call's frames
 * alone; transformer cache and SEANet state are carried as here).  With one frame per call this reproduces the reference's
 * SmolTTS.stream (__init__.py:83-95) sample for sample; chunked decode then no longer equals the batch decode -- which is the
 * reference's defect, kept switchable like the other two torch / MLX disagreements.  Takes effect from the
 * next decode call; returns SMOLTTS_E_INVALID for an unknown option or a value other than 0 / 1.
 *
 * SMOLTTS_MIMI_OPT_PRODUCTS = 3 | 6 (default 6): how many of the bf16 x bf16 products of the split operands the codec's matrix-core
 * kernels form (every Linear, conv, ConvTranspose and the chunk attention of many-row calls, and the fused SEANet stages at any
 * chunk size; the skinny GEMMs of few-row calls are fp32-MFMA kernels and do not change).  6: every product of weight >= 2^-16 -- fp32-grade, PCM RMS ~1e-7 against the fp32 oracle.  3: the products of
 * weight >= 2^-8 only -- half the matrix-core work, the lo pieces are never loaded: a 1024-frame chunk decodes 23 % faster at a PCM
 * RMS error of 7e-7 against the fp32 oracle (signal RMS 0.2-0.4; the contract's bar is 1e-4).  The reference's own codec runs fp32
 * (codec/mimi.py:107,147: format "fp32" unless "bf16" is asked for), hence the default. */
#define SMOLTTS_MIMI_OPT_STATELESS_UPSAMPLE 1
#define SMOLTTS_MIMI_OPT_PRODUCTS 2
int smoltts_mimi_session_set_option(SmolttsMimiSession* s, int32_t option, int32_t value);

/* Decode n_frames new frames for slots [0, batch): codes_dev int32 [batch][codes_stride] where
 * frame f of slot b starts at codes_dev[b*codes_stride + f*frame_stride + code_offset] and holds
 * num_codebooks ints; pcm_dev float [batch][pcm_stride] receives 1920*n_frames samples per slot.
 * Streaming state is carried between calls, so decoding F frames in chunks equals decoding them
 * at once (== MimiModel.decode of the whole code grid). */
int smoltts_mimi_decode_chunk(SmolttsMimiSession* s, const int32_t* codes_dev, int64_t codes_stride,
                              int32_t frame_stride, int32_t code_offset, int32_t batch,
                              int32_t n_frames, float* pcm_dev, int64_t pcm_stride, void* stream);

/* ------------------------------------------------------------------------------ Mimi encoder
 * Voice-clone prompts: MimiModel.encode (mlx_inference/src/smoltts_mlx/codec/mimi.py:64-71) =
 * SEANet encoder (codec/seanet.py:52-96) -> encoder transformer (codec/transformer.py:134-150) ->
 * downsample conv (mimi.py:37-46) -> split RVQ encode (codec/rvq.py:99-116,157-177).  One utterance
 * per call, whole signal at once, as in the reference (no streaming encode there either). */
typedef struct SmolttsMimiEncConfig {
  int32_t num_codebooks;     /* codebooks produced per frame: 1 semantic + (num_codebooks-1) acoustic */
  int32_t n_layers;          /* encoder transformer layers (8) */
  int32_t window;            /* attention window in positions (25 Hz); 0 = unbounded (reference MLX) */
  int32_t max_positions;     /* rows of the RoPE table = longest signal in 960-sample steps */
  int32_t extra_right;       /* 0: the stride-alignment padding goes on the left with the causal padding
                                (reference, codec/conv.py:25-41); 1: on the right (transformers.MimiConv1d) */
} SmolttsMimiEncConfig;

typedef struct SmolttsMimiEncWeights {
  uint64_t conv0_w;          /* fp32 [64][8]: the 7 taps of encoder.layers.0 (1 -> 64 channels), 8th = 0 */
  uint64_t conv0_b;          /* fp32 [64] */
  SmolttsMimiConv convs[13]; /* per ratio 4,5,6,8: res.conv3, res.conv1, strided conv (k = 2*ratio); then the
                                final conv k3 (1024 -> 512); GEMM form [cout][k*cin] */
  SmolttsMimiLayerWeights layers[SMOLTTS_MIMI_MAX_LAYERS];
  uint64_t rope;             /* fp32 [max_positions][32][2] */
  uint64_t downsample_w;     /* fp32 T16x32 [512][4*512], no bias */
  uint64_t in_proj[2];       /* fp32 T16x32 [256][512]: semantic, acoustic group input_proj */
  uint64_t codebooks_t;      /* fp32 T16x32 [num_codebooks][2048][256]: embed_sum / max(usage, 1e-5) */
  uint64_t codebooks;        /* the same rows, row-major (residual update) */
  uint64_t codebook_sq;      /* fp32 [num_codebooks][2048] squared norms of the rows */
} SmolttsMimiEncWeights;

typedef struct SmolttsMimiEncoder SmolttsMimiEncoder;

int smoltts_mimi_encoder_create(const SmolttsMimiEncConfig* cfg, const SmolttsMimiEncWeights* offsets,
                                const void* arena_dev, size_t arena_bytes, SmolttsMimiEncoder** out);
void smoltts_mimi_encoder_destroy(SmolttsMimiEncoder* e);
/* Frames produced for n_samples of 24 kHz audio: ceil(ceil(n/960)/2). */
int32_t smoltts_mimi_encode_frames(int32_t n_samples);
size_t smoltts_mimi_encode_workspace_bytes(const SmolttsMimiEncoder* e, int32_t n_samples);
/* Read-only map of the workspace smoltts_mimi_encode carves for n_samples (tests, diagnostics): row counts, and byte offsets
 * from the workspace base of the fp32 channel-last buffers the chain leaves behind.  Stage i = 0..3 (ratios 4, 5, 6, 8) has
 * C = 64 << i channels and T[i] rows; T[4] = the 25 Hz transformer positions, F = 12.5 Hz frames.  Launches nothing. */
typedef struct SmolttsMimiEncLayout {
  int32_t T[5];            /* rows entering stage i (T[0] = samples); T[4] = transformer positions */
  int32_t extra[4];        /* stride-alignment rows of stage i's strided conv */
  int32_t left[4];         /* zero rows in front of the data in yelu[i] (ratio, plus extra unless extra_right) */
  int32_t F;               /* frames = ceil(T[4] / 2) */
  int32_t ds_extra;        /* stride-alignment rows of the downsample conv */
  int32_t ds_left;         /* edge rows in front of the data in ds */
  uint64_t xraw[4];        /* [T[i]][C]: stage input x_i, raw (conv0 / the previous strided conv) */
  uint64_t xelu[4];        /* [2 + T[i]][C]: ELU(x_i) behind 2 zero rows */
  uint64_t helu[4];        /* [T[i]][C/2]: ELU(conv k3(ELU x_i)) */
  uint64_t yelu[4];        /* [ratio + extra[i] + T[i]][C]: ELU(x_i + conv k1(h_i)) behind left[i] zero rows */
  uint64_t zelu;           /* [2 + T[4]][1024]: ELU of the last strided conv behind 2 zero rows */
  uint64_t kc;             /* [n_layers][8][T[4]][64]: K after RoPE, head dims in the kernel's interleaved-pair order */
  uint64_t vc;             /* [n_layers][8][T[4]][64]: V */
  uint64_t layer_stride;   /* bytes between two layers' K (or V) caches */
  uint64_t ds;             /* [2 + ds_extra + T[4]][512]: transformer output behind ds_left edge rows */
  uint64_t emb;            /* [F][512]: latents (unused when the call passed emb_dev) */
  uint64_t res;            /* [F][256]: the acoustic group's residual after the last codebook */
  uint64_t dots;           /* [F][2048]: residual . codebook rows of the last codebook */
  uint64_t total;          /* == smoltts_mimi_encode_workspace_bytes */
} SmolttsMimiEncLayout;
int smoltts_mimi_encode_layout(const SmolttsMimiEncoder* e, int32_t n_samples, SmolttsMimiEncLayout* out);
/* pcm_dev float [n_samples] -> codes_dev int32 [num_codebooks][frames] (row q = codebook q).
 * Optional outputs (NULL to skip): emb_dev float [frames][512] pre-quantisation latents; gap_dev float
 * [num_codebooks][frames] squared-distance gap between the chosen and the second-nearest entry. */
int smoltts_mimi_encode(SmolttsMimiEncoder* e, const float* pcm_dev, int32_t n_samples, int32_t* codes_dev,
                        float* emb_dev, float* gap_dev, void* workspace_dev, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------ Streamed output formats
 * The codec's 24 kHz fp32 PCM -> 16-bit little-endian PCM at 8000 / 16000 / 22050 / 44100 / 48000 Hz, or 8 kHz G.711 mu-law
 * bytes, chunk by chunk (smoltts_amd/csrc/resample.hip).  Over a whole stream the samples equal
 * scipy.signal.resample_poly(x, up, down) with scipy's default filter (up / down = out_rate / 24000 in lowest terms,
 * half_len = 10 max(up, down), h = firwin(2 half_len + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up, zero padding at both
 * ends), quantised as rint(clip(y, -1, 1) * 32767); mu-law is Sun's linear2ulaw of that int16 (bias 0x84, clip 32635).
 * After N inputs output m is final when half_len + m down <= up N - 1: each call emits the outputs that became final in it and,
 * behind them, the tail up to ceil(N up / down) computed as if the input ended at N (at most 20 samples).  Outputs are summed in
 * fp64 in a fixed order, so the bytes do not depend on how the input is chunked. */
#define SMOLTTS_RESAMPLE_OFF 0   /* slot not converted (its stream stays fp32 at 24 kHz): no outputs, its state does not move */
#define SMOLTTS_RESAMPLE_S16 1   /* int16 little-endian, 2 bytes per sample */
#define SMOLTTS_RESAMPLE_ULAW 2  /* G.711 mu-law, 1 byte per sample, out_rate 8000 only */

typedef struct SmolttsResampler SmolttsResampler;

/* Pure host, no device: the filter of out_rate in double (2 half_len + 1 taps into taps[cap]; taps may be NULL to query
 * up / down / half_len, each of which may be NULL).  SMOLTTS_E_INVALID for an unsupported rate, SMOLTTS_E_CAPACITY when cap is
 * too small. */
int smoltts_resample_design(int32_t out_rate, double* taps, int32_t cap, int32_t* up, int32_t* down, int32_t* half_len);

/* Device slab of a resampler for max_batch slots (256-byte aligned, caller-owned): the polyphase tap tables, each slot's rate and
 * encoding, and two copies of each slot's stream state (<= 64 history samples, int64 input / output positions).  Every slot
 * starts off.  create uploads the tap tables synchronously. */
size_t smoltts_resampler_bytes(int32_t max_batch);
int smoltts_resampler_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsResampler** out);
void smoltts_resampler_destroy(SmolttsResampler* r);
/* Bytes per output row that any slot needs for a call of n_in input samples (finals + tail, at the widest rate). */
size_t smoltts_resampler_out_bytes(int32_t n_in);

/* Start new streams in the listed slots (host arrays) with their rate and encoding (SMOLTTS_RESAMPLE_*; out_rate is ignored
 * for SMOLTTS_RESAMPLE_OFF); the other slots' streams continue.  Stream-ordered. */
int smoltts_resampler_reset_slots(SmolttsResampler* r, const int32_t* slots_host, const int32_t* out_rates_host,
                                  const int32_t* encodings_host, int32_t n_slots, void* stream);

/* One launch for slots [0, batch): slot b consumes valid_in_dev[b] (clamped to [0, n_in]; NULL = n_in) samples of
 * pcm_dev float [batch][pcm_stride] and writes its outputs of this call, finals then tail, to out_dev bytes [batch][out_stride];
 * counts_dev int32 [batch][2] = (finals, tail).  Slots that are off write (0, 0).  Calls on one resampler must be ordered on
 * one stream (the slot states alternate between their two copies). */
int smoltts_resample_chunk(SmolttsResampler* r, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                           const int32_t* valid_in_dev, void* out_dev, int64_t out_stride, int32_t* counts_dev, void* stream);

/* ------------------------------------------------------------------------------ Speaking speed
 * A pitch-preserving time stretch of the codec's 24 kHz fp32 PCM, chunk by chunk (smoltts_amd/csrc/tsm.hip, DESIGN.md
 * section 11; the numpy model is smoltts_amd/tsm.py): WSOLA with hop L = 240, a periodic Hann of W = 480 and an integer-exact
 * search over the lags [-192, 192], speed carried as speed_q = round(speed * 65536) in [16384, 262144].  Segment positions are
 * integer functions of the int16 codes rint(clip(x, -1, 1) * 32767), so the output does not depend on how the input is chunked.
 * A stream of N input samples gives exactly M = ceil(N 65536 / speed_q) output samples; speed_q 65536 is the identity and turns
 * a slot off. */
typedef struct SmolttsTsm SmolttsTsm;

/* Device slab of a stretcher for max_batch slots (256-byte aligned, caller-owned): the window, each slot's speed, and two copies
 * of each slot's stream state (2048 input samples of history, the open half-window, int64 counters).  Every slot starts off.
 * create uploads the window synchronously. */
size_t smoltts_tsm_bytes(int32_t max_batch);
int smoltts_tsm_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsTsm** out);
void smoltts_tsm_destroy(SmolttsTsm* t);
/* Output samples per row that a call of n_in input samples needs (any speed, flush included). */
size_t smoltts_tsm_out_samples(int32_t n_in);

/* Start new streams in the listed slots (host arrays) at their speed_q (65536: the slot is off); the other slots' streams
 * continue.  Stream-ordered. */
int smoltts_tsm_reset_slots(SmolttsTsm* t, const int32_t* slots_host, const int32_t* speed_q_host, int32_t n_slots, void* stream);

/* One launch for slots [0, batch): slot b consumes valid_in_dev[b] (clamped to [0, n_in]; NULL = n_in) samples of pcm_dev float
 * [batch][pcm_stride]; last_dev[b] nonzero (NULL = none) ends the slot's stream with them and flushes it.  Slot b writes the
 * output samples that became final in this call to out_dev float [batch][out_stride] (out_stride >= smoltts_tsm_out_samples(n_in))
 * and their number to counts_dev[b]; slots that are off, or flushed before, write 0.  Calls on one stretcher must be ordered on
 * one stream (the slot states alternate between their two copies). */
int smoltts_tsm_chunk(SmolttsTsm* t, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                      const int32_t* valid_in_dev, const int32_t* last_dev, float* out_dev, int64_t out_stride,
                      int32_t* counts_dev, void* stream);

/* Tests and tools: slot's current state (k = next segment, p_{k-1}, input consumed, output emitted, flushed) into
 * state_host[5]; synchronises the stream. */
int smoltts_tsm_slot_state(SmolttsTsm* t, int32_t slot, int64_t* state_host, void* stream);

/* ------------------------------------------------------------------------------ FLAC
 * Lossless framing of a stream (smoltts_amd/csrc/flac.hip; the numpy model and parity oracle is
 * smoltts_amd/flac.py): RFC 9639 frames, mono, 16 bits, variable blocking (the coded number is the sample number of the block's
 * first sample), subframes CONSTANT / FIXED 0..4 with partitioned Rice residuals / VERBATIM, fewest bits wins.  Every choice is
 * an integer function of the int16 samples, so the bytes equal the model's.  A slot holds back at most 15 samples: with 16 or
 * more pending, or any at its last call, it emits all of them as ceil(P / 4096) blocks sized as evenly as possible.  The stream
 * header (fLaC + STREAMINFO) is the host's. */
typedef struct SmolttsFlac SmolttsFlac;
enum {
  SMOLTTS_FLAC_OFF = 0,
  SMOLTTS_FLAC_F32 = 1, /* the slot reads fp32 PCM, quantised as rint(clip(x, -1, 1) * 32767) */
  SMOLTTS_FLAC_S16 = 2  /* the slot reads the resampler's int16 output */
};

/* Device slab of an encoder for max_batch slots (256-byte aligned, caller-owned): each slot's source and rate, and two copies of
 * each slot's stream state (the int64 position, up to 15 pending samples).  Every slot starts off. */
size_t smoltts_flac_bytes(int32_t max_batch);
int smoltts_flac_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsFlac** out);
void smoltts_flac_destroy(SmolttsFlac* f);
/* For calls in which a slot reads at most n_max samples: the blocks a slot may emit, and the output row bytes (2 (n_max + 15)
 * plus 20 per block: a frame of n samples takes at most 2 n + 17 bytes). */
int32_t smoltts_flac_max_blocks(int32_t n_max);
size_t smoltts_flac_out_bytes(int32_t n_max);

/* Start new streams in the listed slots (host arrays) at their rate (8000, 16000, 22050, 24000, 44100, 48000) and source
 * (SMOLTTS_FLAC_*; OFF switches the slot off); the other slots' streams continue.  Stream-ordered. */
int smoltts_flac_reset_slots(SmolttsFlac* f, const int32_t* slots_host, const int32_t* rates_host, const int32_t* sources_host,
                             int32_t n_slots, void* stream);

/* One launch for slots [0, batch), no host read.  An F32 slot b consumes valid_in_dev[b] (clamped to [0, n_in]; NULL = n_in)
 * samples of pcm_dev float [batch][pcm_stride]; an S16 slot consumes s16_counts_dev[2b] (+ s16_counts_dev[2b + 1] when it is
 * last) little-endian int16 samples of s16_dev [batch][s16_stride bytes] (the resampler's bytes and counts of the same pass).
 * last_dev[b] nonzero (NULL = none) ends the slot's stream with this call.  Slot b writes its frames to out_dev [batch]
 * [out_stride] (out_stride >= smoltts_flac_out_bytes(n_max), n_max the most samples a slot of the call can read) and
 * sizes_dev int32 [batch][max_blocks][2] = {byte offset in the row, bytes} per frame in order, {0, 0} past its last; slots
 * that are off write {0, 0} only.  Calls on one encoder must be ordered on one stream (the states alternate between copies). */
int smoltts_flac_chunk(SmolttsFlac* f, const float* pcm_dev, int64_t pcm_stride, int32_t n_in, const int32_t* valid_in_dev,
                       const void* s16_dev, int64_t s16_stride, const int32_t* s16_counts_dev, int32_t batch,
                       const int32_t* last_dev, void* out_dev, int64_t out_stride, int32_t* sizes_dev, int32_t max_blocks,
                       void* stream);

/* ------------------------------------------------------------------------------ Seam
 * The segments of a long text joined into one stream on the codec's 24 kHz fp32 PCM (smoltts_amd/csrc/seam.hip, DESIGN.md
 * section 13; the numpy model is smoltts_amd/seam.py).  Blocks of 240 samples from a segment's start are silent when
 * max|x| < 2^-8.  A segment that is not the stream's first drops leading silent blocks (at most 1 s); one that is not the
 * stream's last holds back trailing silent blocks (at most 1 s) and, at its end, replaces the held run of r samples by its first
 * min(r, G) samples and G - min(r, G) zeros, G the seam's pause.  The first segment may open with `lead` zeros and the last
 * close with G zeros.  The output does not depend on how a segment is cut into calls. */
typedef struct SmolttsSeam SmolttsSeam;
enum {  /* segment flags of smoltts_seam_reset_slots */
  SMOLTTS_SEAM_FIRST = 1,  /* the stream's first segment: its head is kept, `lead` zeros go in front of it */
  SMOLTTS_SEAM_FINAL = 2,  /* the stream's last segment: its tail is kept, G zeros follow it */
  SMOLTTS_SEAM_OFF = 4     /* switch the slot off */
};

/* Device slab of a seam stage for max_batch slots (256-byte aligned, caller-owned): two copies of each slot's state (counters and
 * 24576 samples of history).  Every slot starts off; create clears the slab synchronously. */
size_t smoltts_seam_bytes(int32_t max_batch);
int smoltts_seam_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsSeam** out);
void smoltts_seam_destroy(SmolttsSeam* s);
/* Output samples per row that a call of n_in input samples needs when no open slot owes more than max_zeros zeros (its lead
 * plus its pause, as given to smoltts_seam_reset_slots; at most 480000). */
size_t smoltts_seam_out_samples(int32_t n_in, int32_t max_zeros);

/* Open a segment in each listed slot (host arrays): its pause G in samples (0..240000), its flags (SMOLTTS_SEAM_*) and, for a
 * FIRST segment, the zeros in front of it (lead_host may be NULL: none).  The other slots continue.  Stream-ordered. */
int smoltts_seam_reset_slots(SmolttsSeam* s, const int32_t* slots_host, const int32_t* pause_host, const int32_t* flags_host,
                             const int32_t* lead_host, int32_t n_slots, void* stream);

/* One launch for slots [0, batch): slot b consumes valid_in_dev[b] (clamped to [0, n_in]; NULL = n_in) samples of pcm_dev float
 * [batch][pcm_stride]; seg_end_dev[b] nonzero ends the slot's segment with them, last_dev[b] nonzero ends the stream (a held run
 * is then released unchanged); either may be NULL.  max_zeros: the most zeros (lead + pause) any open slot owes.  Slot b writes
 * the samples that became final in this call to out_dev float [batch][out_stride] (out_stride >= smoltts_seam_out_samples(n_in,
 * max_zeros)) and their number to counts_dev[b]; slots without an open segment write 0.  Calls on one seam stage must be
 * ordered on one stream (the slot states alternate between their copies). */
int smoltts_seam_chunk(SmolttsSeam* s, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                       const int32_t* valid_in_dev, const int32_t* seg_end_dev, const int32_t* last_dev, int32_t max_zeros,
                       float* out_dev, int64_t out_stride, int32_t* counts_dev, void* stream);

/* Tests and tools: slot's state (n_in, judged, ec, head, open, lead, pause, flags) into state_host[8]; synchronises the stream. */
int smoltts_seam_slot_state(SmolttsSeam* s, int32_t slot, int64_t* state_host, void* stream);

/* ------------------------------------------------------------------------------ Trim
 * Leading and trailing silence cut and pauses capped per request on the codec's 24 kHz fp32 PCM, first of the stages behind the
 * codec and in front of the seam (smoltts_amd/csrc/trim.hip; the numpy model, matched bit for bit, is
 * smoltts_amd/trim.py).  Blocks are the seam's: 240 samples counted from the segment's first sample, the last one of a segment
 * may be partial.  A block is silent when max|x| < thr, compared in float32; a NaN is not silence.  A run is a maximal sequence
 * of consecutive silent blocks, r its length in blocks.  Per segment: its flags (SMOLTTS_SEAM_FIRST / _FINAL; a plain stream
 * is FIRST|FINAL), trim, and P, the pause cap in blocks (0: none, else 10..200).  Constants: HEAD_KEEP = 2, TAIL_KEEP = 10,
 * HOLD = 200 blocks.  What is kept of a run, the first matching case applies:
 *   1. trim, FIRST, and the run starts at block 0: its last min(r, HEAD_KEEP) blocks (this also covers an all-silent segment);
 *   2. trim, FINAL, and the run reaches the segment's end: its first min(r, K) blocks, K = TAIL_KEEP when P == 0, else
 *      min(TAIL_KEEP, ceil(P/2)); exception: when P == 0 and r - K > HOLD, its first r - HOLD blocks, so the tail never loses
 *      more than 2 s;
 *   3. P > 0 and r > P: its first ceil(P/2) and its last floor(P/2) blocks;
 *   4. otherwise all of it.
 * Non-silent blocks are always kept; the output is the kept blocks in order.  Every cut lies in samples below thr, so there are
 * no fades, as in the seam.  The output does not depend on how a segment is cut into calls; a non-silent block leaves in the call
 * that completes it, together with whatever was held in front of it; a slot holds at most HOLD blocks and a partial block. */
typedef struct SmolttsTrim SmolttsTrim;

/* Device slab of a trim stage for max_batch slots (256-byte aligned, caller-owned): two copies of each slot's state (counters and
 * 48240 held samples).  Every slot starts off; create clears the slab synchronously. */
size_t smoltts_trim_bytes(int32_t max_batch);
int smoltts_trim_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsTrim** out);
void smoltts_trim_destroy(SmolttsTrim* t);
/* Output samples per row that a call of n_in input samples needs (the held blocks released in front of them); 0 when n_in is
 * negative or above 61440, the most one call takes. */
size_t smoltts_trim_out_samples(int32_t n_in);

/* Open a segment in each listed slot (host arrays): its flags (SMOLTTS_SEAM_FIRST / _FINAL; SMOLTTS_SEAM_OFF switches the slot
 * off), whether cases 1 and 2 apply (trim_host, nonzero: yes), its pause cap P in blocks (0, or 10..200) and its threshold
 * (0 < thr <= 1).  The other slots continue.  Stream-ordered. */
int smoltts_trim_reset_slots(SmolttsTrim* t, const int32_t* slots_host, const int32_t* flags_host, const int32_t* trim_host,
                             const int32_t* pause_host, const float* thr_host, int32_t n_slots, void* stream);

/* One launch for slots [0, batch): slot b consumes valid_in_dev[b] (clamped to [0, n_in]; NULL = n_in) samples of pcm_dev float
 * [batch][pcm_stride]; seg_end_dev[b] or last_dev[b] nonzero ends the slot's segment with them (either may be NULL; a run that
 * `last` cuts short in a segment that is not FINAL is released by cases 3 and 4).  Slot b writes the samples that became final
 * in this call to out_dev float [batch][out_stride] (out_stride >= smoltts_trim_out_samples(n_in)) and their number to
 * counts_dev[b]; slots without an open segment write 0.  Calls on one trim stage must be ordered on one stream (the slot states
 * alternate between their copies). */
int smoltts_trim_chunk(SmolttsTrim* t, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                       const int32_t* valid_in_dev, const int32_t* seg_end_dev, const int32_t* last_dev, float* out_dev,
                       int64_t out_stride, int32_t* counts_dev, void* stream);

/* Tests and tools: slot's state (n_in, judged, emitted, held, dropped_head, dropped_pause, dropped_tail: samples; open) into
 * state_host[8]; synchronises the stream. */
int smoltts_trim_slot_state(SmolttsTrim* t, int32_t slot, int64_t* state_host, void* stream);

/* ------------------------------------------------------------------------------ Loudness
 * Per-slot loudness normalisation of the codec's 24 kHz fp32 PCM by the ITU-R BS.1770-4 meter (smoltts_amd/csrc/loudness.hip,
 * DESIGN.md section 14; the numpy model, reproduced bit for bit, is smoltts_amd/loudness.py).  A stream's gain is piecewise
 * linear between knots at 2400-sample hop boundaries, on a grid of 1/64 dB within +-20 dB; both knots of a hop are fixed from
 * the samples in front of it, so a slot emits exactly the samples it reads.  The output does not depend on how a stream is cut
 * into calls. */
typedef struct SmolttsLoudness SmolttsLoudness;

/* Device slab of a loudness stage for max_batch slots (256-byte aligned, caller-owned): two copies of each slot's state and the
 * stage's tables.  tables_host: smoltts_loudness_table_doubles() doubles (loudness.Tables.packed: the filters' coefficients, the
 * 240-step transition matrix, the absolute gate, the ceiling, the knots' gains and their squares); the device computes no
 * power or logarithm.  Every slot starts off; create clears the slab and uploads the tables synchronously. */
size_t smoltts_loudness_bytes(int32_t max_batch);
int32_t smoltts_loudness_table_doubles(void);
int smoltts_loudness_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, const double* tables_host, int32_t n_tables,
                            SmolttsLoudness** out);
void smoltts_loudness_destroy(SmolttsLoudness* s);

/* Start a new stream in each listed slot (host arrays): its target as the mean square that reads the target loudness (0 switches
 * the slot off; at most 1) and its first knot in 1/64 dB (-1280..1280; start_knot_host may be NULL: 0).  The other slots
 * continue.  Stream-ordered. */
int smoltts_loudness_reset_slots(SmolttsLoudness* s, const int32_t* slots_host, const double* target_power_host,
                                 const int32_t* start_knot_host, int32_t n_slots, void* stream);

/* One launch for slots [0, batch): slot b consumes valid_in_dev[b] (clamped to [0, n_in]; NULL = n_in) samples of pcm_dev float
 * [batch][pcm_stride] and writes as many to out_dev float [batch][out_stride] (out_stride >= n_in), their number to
 * counts_dev[b]; slots that are off write 0.  Calls on one stage must be ordered on one stream. */
int smoltts_loudness_chunk(SmolttsLoudness* s, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                           const int32_t* valid_in_dev, float* out_dev, int64_t out_stride, int32_t* counts_dev, void* stream);

/* A whole utterance of n samples measured in one launch (no slot involved): every complete hop's energy to hops_dev (room for
 * hops_len >= n / 2400 doubles), and result_dev[4] = {gated mean power, 0 when no block passes the absolute gate or n < 9600;
 * max |x|; blocks past the absolute gate; blocks past both gates}.  smoltts_loudness_scale: out = float(x * gain). */
int smoltts_loudness_measure(SmolttsLoudness* s, const float* pcm_dev, int32_t n, double* hops_dev, int64_t hops_len,
                             double* result_dev, void* stream);
int smoltts_loudness_scale(const float* pcm_dev, int64_t n, double gain, float* out_dev, void* stream);

/* Tests and tools: slot's state; ints_host[4] = pos, the open hop's two knots, on; values_host[531] = the filter's three states
 * (start, running, zero-state pass), the open sub-block's and hop's energies, the last three hop energies, the peak, the target
 * power, the ring of 512 block powers.  Synchronises the stream. */
int smoltts_loudness_slot_state(SmolttsLoudness* s, int32_t slot, int64_t* ints_host, double* values_host, void* stream);

/* ------------------------------------------------------------------------------ Watermark
 * A keyed spread-spectrum mark added to the codec's 24 kHz fp32 PCM (smoltts_amd/csrc/watermark.hip; the
 * numpy model, reproduced bit for bit, and the detector are smoltts_amd/watermark.py).  Chips of +-1 on a period of 15360
 * samples, scaled per 480-sample block by gain * sqrt(mean square of the block in front), shaped by a 65-tap band-pass
 * (500-3400 Hz) and added in fp64.  A block's gain comes from the block in front of it, so a slot emits exactly the samples it
 * reads.  The output does not depend on how a stream is cut into calls.  One key per stage. */
typedef struct SmolttsWatermark SmolttsWatermark;

/* Device slab of a watermark stage for max_batch slots (256-byte aligned, caller-owned): two copies of each slot's state and the
 * stage's tables.  tables_host: smoltts_watermark_table_doubles() doubles (watermark.Watermark.packed: the 65 taps, then the
 * key's 15360 chips as +1.0 / -1.0); the device hashes nothing.  Every slot starts off; create clears the slab and uploads the
 * tables synchronously. */
size_t smoltts_watermark_bytes(int32_t max_batch);
int32_t smoltts_watermark_table_doubles(void);
int smoltts_watermark_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, const double* tables_host, int32_t n_tables,
                             SmolttsWatermark** out);
void smoltts_watermark_destroy(SmolttsWatermark* s);

/* Start a new stream in each listed slot (host arrays) at its gain 10^(strength_db / 20) (0 switches the slot off; at most 1).
 * The other slots continue.  Stream-ordered. */
int smoltts_watermark_reset_slots(SmolttsWatermark* s, const int32_t* slots_host, const double* gain_host, int32_t n_slots,
                                  void* stream);

/* One launch for slots [0, batch): slot b consumes valid_in_dev[b] (clamped to [0, n_in]; NULL = n_in) samples of pcm_dev float
 * [batch][pcm_stride] and writes as many to out_dev float [batch][out_stride] (out_stride >= n_in), their number to
 * counts_dev[b]; slots that are off write 0 and leave their rows alone.  Calls on one stage must be ordered on one stream. */
int smoltts_watermark_chunk(SmolttsWatermark* s, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                            const int32_t* valid_in_dev, float* out_dev, int64_t out_stride, int32_t* counts_dev, void* stream);

/* A whole utterance of n samples marked from position 0 at `gain` in one launch (no slot involved): the samples a stream gives. */
int smoltts_watermark_embed(SmolttsWatermark* s, const float* pcm_dev, int32_t n, double gain, float* out_dev, void* stream);

/* Tests and tools: slot's state; ints_host[2] = pos, on; values_host[5] = the open sub-block's sum, the open block's folded
 * sub-blocks, the open and the previous block's gain, the slot's gain.  Synchronises the stream. */
int smoltts_watermark_slot_state(SmolttsWatermark* s, int32_t slot, int64_t* ints_host, double* values_host, void* stream);

/* ------------------------------------------------------------------------------ Limiter
 * A look-ahead peak limiter on the codec's 24 kHz fp32 PCM, the last float stage (smoltts_amd/csrc/limiter.hip, DESIGN.md section
 * 22; the numpy model, reproduced bit for bit, is smoltts_amd/limiter.py).  The peak of a sample is the largest magnitude of
 * itself and of three 12-tap interpolated values between it and the next one; the required gain is ceiling / peak where the
 * peak passes the ceiling, else 1; a sample's gain is the smaller of its own required gain and the mean of 121 minima of the
 * required gain, each over 1200 samples of hold and 120 of look-ahead.  A slot holds back 126 samples; a stream's end flushes
 * them.  Where nothing near passes the ceiling the gain is exactly 1 and the samples leave unchanged.  The output does not
 * depend on how a stream is cut into calls. */
typedef struct SmolttsLimiter SmolttsLimiter;

/* Device slab of a limiter stage for max_batch slots (256-byte aligned, caller-owned): two copies of each slot's state (126
 * samples, 1440 required gains, the position, the ceiling, the smallest gain so far) and the stage's table.  tables_host:
 * smoltts_limiter_table_doubles() doubles (limiter.packed: the three phases' 12 taps); the device designs nothing.  Every slot
 * starts off; create clears the slab and uploads the table synchronously. */
size_t smoltts_limiter_bytes(int32_t max_batch);
int32_t smoltts_limiter_table_doubles(void);
int smoltts_limiter_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, const double* tables_host, int32_t n_tables,
                           SmolttsLimiter** out);
void smoltts_limiter_destroy(SmolttsLimiter* l);
/* Output samples per row that a call of n_in input samples needs (n_in + 126: the held samples a stream's end releases); 0 when
 * n_in is negative or above 61440, the most one call takes. */
size_t smoltts_limiter_out_samples(int32_t n_in);

/* Start a new stream in each listed slot (host arrays) under its ceiling 10^(peak_limit_db / 20) (0 switches the slot off; at
 * most 1).  The other slots continue.  Stream-ordered. */
int smoltts_limiter_reset_slots(SmolttsLimiter* l, const int32_t* slots_host, const double* ceiling_host, int32_t n_slots,
                                void* stream);

/* One launch for slots [0, batch): slot b consumes valid_in_dev[b] (clamped to [0, n_in]; NULL = n_in) samples of pcm_dev float
 * [batch][pcm_stride]; last_dev[b] nonzero (last_dev may be NULL) ends the slot's stream with them.  Slot b writes the samples
 * that became final in this call to out_dev float [batch][out_stride] (out_stride >= smoltts_limiter_out_samples(n_in)) and
 * their number to counts_dev[b]: so far max(0, consumed - 126) in total, and all of them once the stream has ended.  Slots that
 * are off write 0 and leave their rows alone, as do slots whose stream has ended.  Calls on one stage must be ordered on one
 * stream. */
int smoltts_limiter_chunk(SmolttsLimiter* l, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                          const int32_t* valid_in_dev, const int32_t* last_dev, float* out_dev, int64_t out_stride,
                          int32_t* counts_dev, void* stream);

/* A whole utterance of n samples limited under `ceiling` (0 < ceiling <= 1) in one launch (no slot involved): n samples to
 * out_dev, the samples a stream gives, and result_dev[0] = the smallest gain applied (1 when nothing was limited). */
int smoltts_limiter_apply(SmolttsLimiter* l, const float* pcm_dev, int32_t n, double ceiling, float* out_dev, double* result_dev,
                          void* stream);

/* Tests and tools: slot's state; ints_host[3] = pos, on, ended; values_host[1568] = the ceiling, the smallest gain so far, the
 * 1440 required gains of samples pos - 1446 .. pos - 7, the 126 samples pos - 126 .. pos - 1.  Synchronises the stream. */
int smoltts_limiter_slot_state(SmolttsLimiter* l, int32_t slot, int64_t* ints_host, double* values_host, void* stream);

/* ------------------------------------------------------------------------------ Streamed alignment fit
 * (ABI 9, additive) The causal fit of streamed character timestamps (smoltts_amd/csrc/align_fit.hip; the
 * numpy model, reproduced bit for bit, is smoltts_amd/align.py StreamFit).  A slot holds one stream's fit: the frames it has
 * consumed, the stack of pooled blocks and the token starts committed so far, in frames, fp64.  A start is committed once a block
 * at or above the token's level began `lag` frames back, and is never revised. */
typedef struct SmolttsAlignFit SmolttsAlignFit;

/* Device slab of a fitter for max_batch slots (256-byte aligned, caller-owned): per slot a header, a stack of max_frames blocks
 * and max_tokens starts.  0 for sizes outside 1 .. 65536 slots, 1 .. 2^20 frames or tokens.  Every slot starts off. */
size_t smoltts_align_fit_bytes(int32_t max_batch, int32_t max_frames, int32_t max_tokens);
int smoltts_align_fit_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, int32_t max_frames, int32_t max_tokens,
                             SmolttsAlignFit** out);
void smoltts_align_fit_destroy(SmolttsAlignFit* a);

/* Start a stream in (or, n_tokens < 0, switch off) slots_host[0 .. n_slots): n_tokens_host the text's tokens (0 .. max_tokens),
 * lag_host the lag in frames (1 .. 64), cap_frames_host the frames the slot's request may have (1 .. max_frames): the stream
 * ends there, or where the session's done flag stands with a frame.  A bad value refuses the call with its group of 16 slots
 * unlaunched.  Ordered on `stream`; queue it where the slot's frame counter is 0 by the time of the next push. */
int smoltts_align_fit_reset_slots(SmolttsAlignFit* a, const int32_t* slots_host, const int32_t* n_tokens_host, const int32_t* lag_host,
                                  const int32_t* cap_frames_host, int32_t n_slots, void* stream);

/* One launch over every slot: slot b consumes rows_dev float [max_batch][max_frames][n_pairs][2] (smoltts_session_alignment; 8-byte
 * aligned, max_frames the handle's) from the frame it has seen up to min(n_frames_dev[b], its budget), and gives every remaining
 * token its start once (done_dev[b] != 0 and n_frames_dev[b] > 0) or n_frames_dev[b] >= its budget: with F the frames consumed.
 * A slot that is off or has ended, or whose counter is negative, is left alone. */
int smoltts_align_fit_push(SmolttsAlignFit* a, const float* rows_dev, int32_t n_pairs, int32_t max_frames, const int32_t* n_frames_dev,
                           const int32_t* done_dev, void* stream);

/* Device pointers (valid for the handle's lifetime): starts double [max_batch][*max_tokens], entries [b][0 .. committed[b]) final;
 * committed int32 [max_batch].  Each may be NULL. */
int smoltts_align_fit_outputs(SmolttsAlignFit* a, double** starts_dev, int32_t** committed_dev, int32_t* max_tokens);

/* --------------------------------------------------------------- operator-level test entry points */
enum {  /* prologue applied to the activation operand */
  SMOLTTS_PRO_NONE = 0,
  SMOLTTS_PRO_RMSNORM = 1,  /* x * rsqrt(mean(x^2)+eps) * gamma */
  SMOLTTS_PRO_ELU = 2,
  SMOLTTS_PRO_LAYERNORM = 3 /* fp32 weights: nn.LayerNorm over the K values of a row: gamma_dev = weight, beta_dev = bias, eps;
                               fused into the GEMM where its kernel can (few rows; K = 512 at chunk size), otherwise applied by the
                               stand-alone kernel into ln_scratch_dev [M][K] first */
};
enum {  /* epilogue */
  SMOLTTS_EPI_STORE = 0,        /* out = acc (+ bias) */
  SMOLTTS_EPI_RESID = 1,        /* out = resid + acc (+ bias) */
  SMOLTTS_EPI_SWIGLU = 2,       /* rows interleaved (gate, up): out[n/2] = silu(gate) * up */
  SMOLTTS_EPI_GELU = 3,         /* out = gelu_erf(acc) */
  SMOLTTS_EPI_SCALE_RESID = 4,  /* out = resid + scale[n] * acc */
  SMOLTTS_EPI_QKV_ROPE = 5      /* interleaved RoPE on q,k; q -> out, k/v -> caches */
};

typedef struct SmolttsGemmArgs {
  const void* w_dev;          /* T16x32 tiles */
  int32_t w_is_fp32;          /* 0: bf16, 1: fp32 */
  const float* x_dev;         /* activations; row m at x + (m / rows_per_batch) * x_bstride
                                 + (m % rows_per_batch) * ldx   (rows_per_batch 0 => m * ldx) */
  int64_t ldx, x_bstride;
  int32_t rows_per_batch;
  int32_t M, N, K;
  int32_t prologue, epilogue;
  const float* gamma_dev;     /* RMSNorm weight [K] */
  float eps;
  const float* bias_dev;      /* [N] or NULL */
  const float* scale_dev;     /* [N], EPI_SCALE_RESID */
  const float* resid_dev;     /* row m at resid + (m / rpb) * r_bstride + (m % rpb) * ldr;
                                 ldr == 0 => same addressing as out */
  int64_t ldr, r_bstride;
  float* out_dev;             /* row m at out + (m / rows_per_batch) * o_bstride + (m % rpb) * ldo */
  int64_t ldo, o_bstride;
  int32_t elu_out;            /* STORE / RESID: store ELU(result) (the consumer then needs no ELU prologue); N < 4 included */
  float* raw_out_dev;         /* STORE: optional second copy of the un-activated result, row stride ldo; N < 4 included */
  int64_t raw_bstride;
  /* EPI_QKV_ROPE */
  const float* rope_dev;      /* [pos][32][2]; q rows are rotated by the entry at row_pos even where that lies outside
                                 [0, cache_len) (such rows write no K / V): the table must reach every row_pos given */
  const int32_t* row_pos_dev; /* [M] */
  const int32_t* row_slot_dev;/* [M] */
  float* k_cache_dev;         /* [slots][n_kv][cache_len][64] */
  float* v_cache_dev;
  int32_t n_q_heads, n_kv_heads, cache_len; /* both head counts >= 1: N = (n_q_heads + 2 n_kv_heads) * 64 >= 192 */
  const void* w3_dev;         /* optional, fp32 weights only: the same matrix as "W3" tiles; many-row calls (M >= 256, N >= 64,
                                 no prologue or the ELU one) then run on the bf16 matrix cores with split operands (fp32-grade results) */
  float* splitk_ws_dev;       /* optional, with w3_dev: workspace for split-K partial sums (long K over few tiles) ... */
  int64_t splitk_ws_floats;   /* ... and its size in floats (4 * M * N needed; smaller = no split) */
  const float* beta_dev;      /* PRO_LAYERNORM: bias [K] */
  float* ln_scratch_dev;      /* PRO_LAYERNORM: [M][K] floats for the calls whose kernel has no such prologue */
  void* k_cache3_dev;         /* EPI_QKV_ROPE, optional (both or neither): the same K / V rows also as bf16x3 PIECE caches, the operands */
  void* v_cache3_dev;         /* of smoltts_k_attention_rows3 (layouts there); SMOLTTS_KV3_BYTES(slots, n_kv, cache_len) bytes each, */
                              /* zero-filled once by the owner (unwritten positions are multiplied by zero weights: they must be finite) */
  int32_t b3_products;        /* (ABI 6) calls that run on bf16x3 pieces (w3_dev): 3 = three MFMA products per operand pair (hi*hi, mid*hi, */
                              /* hi*mid: 2^-16-grade results, lo pieces never loaded), anything else = six (fp32-grade, the default) */
} SmolttsGemmArgs;

/* bytes of one bf16x3 piece cache: per (slot, kv head) 6 bytes per value over cache_len rounded up to whole 32-position blocks */
#define SMOLTTS_KV3_BYTES(slots, n_kv, cache_len) ((size_t)(slots) * (size_t)(n_kv) * (size_t)(((cache_len) + 31) / 32 * 32) * 384u)

int smoltts_k_gemm(const SmolttsGemmArgs* a, void* stream);

/* bf16-MFMA GEMM of the DualAR transformer (smoltts_amd/csrc/gemm3.hip).  The activation operand is
 * in the "X3" format (smoltts_amd/csrc/x3.h): rows in tiles of 16, K in chunks of 32, block
 * (row tile, chunk, piece p in 0..2) = 1 KiB at ((tile * K/32 + chunk) * 3 + p) * 1024 holding for
 * lane l = 16*q + r the 8 bf16 of piece p of x[16*tile + r][32*chunk + 8q .. +8); the three pieces
 * sum exactly to the fp32 value (already multiplied by the consumer's RMSNorm weight).  Buffer
 * size: ceil(M/16)*16 * K * 6 bytes. */
enum {  /* weight formats of the DualAR Linears */
  SMOLTTS_W_BF16 = 0,  /* bf16 T16x32 tiles (1 KiB per 16 rows x 32 columns) */
  SMOLTTS_W_FP8 = 1    /* fp8 e4m3 (OCP) T16x32 tiles (512 B) + one fp32 scale per output row: w = q * scale */
};

typedef struct SmolttsGemm3Args {
  const void* w_dev;           /* T16x32 [N][K] in w_format */
  const void* x3_dev;          /* X3 operand [M][K] */
  int32_t M, N, K;
  int32_t epilogue;            /* SMOLTTS_EPI_STORE | _RESID | _SWIGLU | _QKV_ROPE */
  const float* ssq_in_dev;     /* [M][K/16] partial sums of squares of the un-normed input rows: the result
                                  rows are scaled by rsqrt(sum/K + eps); NULL = input not normed */
  float eps;
  const float* bias_dev;       /* [N] or NULL */
  const float* resid_dev;      /* EPI_RESID: fp32 [M][ldo] */
  float* out_dev;              /* fp32 [M][ldo]: STORE / RESID result, QKV_ROPE q rows */
  int64_t ldo;
  void* x3_out_dev;            /* EPI_SWIGLU: X3 [M][N/2] of silu(gate) * up */
  /* STORE / RESID: also publish the result for the next GEMM(s): X3 of out * gamma (gamma NULL = 1),
   * up to two consumers, and the per-(row, 16-column tile) sums of squares [M][N/16] */
  void* emit_a_dev; const float* gamma_a_dev;
  void* emit_b_dev; const float* gamma_b_dev;
  float* ssq_out_dev;
  /* EPI_QKV_ROPE */
  const float* rope_dev; const int32_t* row_pos_dev; const int32_t* row_slot_dev;
  float* k_cache_dev; float* v_cache_dev;
  int32_t n_q_heads, n_kv_heads, cache_len;
  int32_t w_format;            /* SMOLTTS_W_BF16 | SMOLTTS_W_FP8 */
  const float* w_scale_dev;    /* SMOLTTS_W_FP8: [N] row scales; NULL otherwise */
  void* v_x3_dev;              /* EPI_QKV_ROPE, optional: every row sits at position 0, so its attention output is its own
                                  V row (softmax over one key): V is also written as the X3 operand [M][n_q_heads*64] of
                                  the output projection (each kv head repeated for its query heads) and no attention
                                  launch is needed */
  int32_t kv_format;           /* EPI_QKV_ROPE: SMOLTTS_KV_F32 | SMOLTTS_KV_BF16 storage of k_cache_dev / v_cache_dev */
  int32_t w_stream;            /* != 0: these weights are read once now and not again before the caches have turned over (the slow
                                  layers of a decode frame): their loads carry the non-temporal hint, so that they do not push the
                                  depth transformer's weights -- re-read 8 times per frame -- out of the Infinity Cache (M <= 128 only) */
  /* EPI_RESID with the attention of a depth step as its activation operand (ABI 5): attn_q_dev != NULL means x3_dev is not read;
   * instead every workgroup works out, for the rows it multiplies, softmax(q K^T / 8) V over keys 0 .. attn_pos of the row's own
   * slot (row r == slot r) in k_cache_dev / v_cache_dev [M][n_kv_heads][cache_len][64] fp32 -- the output of
   * smoltts_k_attention for those rows -- and feeds it to the matrix cores as bf16x3 pieces through LDS.  One launch instead of
   * two per depth layer, with the same bits (every sum in the order smoltts_k_attention + this launch without the prologue form it, at
 * up to 128 rows); needs smoltts_gemm3_attn_fusable(n_q_heads, n_kv_heads, cache_len) and K == n_q_heads * 64. */
  const float* attn_q_dev;     /* fp32 [M][n_q_heads*64] (RoPE applied: the q rows an EPI_QKV_ROPE launch wrote) */
  int32_t attn_pos;
  /* EPI_STORE (ABI 5): also leave, for every (row, 16-column tile) of the result, the tile's largest value, the first column that
   * holds it (int32 bits) and the runner-up: float [M][ceil(N/16)][4] (4th unused) -- what a greedy pick needs of a row of logits
   * (M < 256: the many-row kernel has no such epilogue) */
  float* cand_out_dev;
  /* the attention prologue with the PICK in front of it (ABI 5; NULL = off): the rows are depth step attn_pos of a frame whose
   * previous head GEMM left cand_out_dev; see SmolttsPickArgs.  attn_q_dev and resid_dev are then not read. */
  const struct SmolttsPickArgs* pick;
  /* SMOLTTS_W_FP8 weights, M >= 256 (prompt rows) only (ABI 5): != 0 runs the GEMM on the fp8 matrix-core instruction
   * (v_mfma_f32_16x16x32_fp8_fp8) -- the weight tiles as they are, the activation operand's leading bf16 piece rounded to e4m3
   * -- instead of three exact bf16 MFMAs per chunk: BASELINE configs[4]'s "fp8 MFMA prefill".  The result then carries the
   * activations' fp8 rounding (~2^-4 relative per element, ~1e-3 of the output scale): NOT the parity path. */
  int32_t fp8_activations;
} SmolttsGemm3Args;

/* Greedy pick of the previous depth step's code inside the launch that consumes it (depth layer 0 of the next step, whose q | k | v
 * come out of the engine's fast_qkv table): every workgroup merges its rows' tile candidates (first maximal column, as
 * torch.argmax), gathers q and the new key's K / V rows of the picked embedding row from the table (RoPE for attn_pos applied on the
 * way, bit-identical to the stand-alone picking kernel's), takes the residual row from the embedding table, and runs attention + wo
 * as with attn_q_dev.  The workgroups of column group 0 also record the id, the top-2 gap bookkeeping of smoltts_k_argmax and the
 * new K / V cache rows.  One launch fewer per depth step (lm/generate.py:118-141). */
typedef struct SmolttsPickArgs {
  const float* cand_dev;          /* [M][cand_tiles][4] from the head GEMM's cand_out_dev */
  int32_t cand_tiles;             /* codebook_size / 16 */
  const float* qkv_table_dev;     /* fp32 [emb rows][(n_q_heads + 2 n_kv_heads) * 64], before RoPE */
  const float* rope_dev;          /* fp32 [pos][32][2] */
  const void* emb_dev;            /* bf16 [emb rows][K]: the residual row of a picked id */
  int32_t emb_row_offset;         /* embedding / table row = id + emb_row_offset (depthwise tables: lm/generate.py:136-140) */
  int32_t* ids_dev;               /* row r's id -> ids_dev[r * ids_stride] */
  int32_t ids_stride;
  float* margin_dev;              /* [M] smallest top-2 gap so far (updated where margin_mask_dev[r] != 0), or NULL */
  const int32_t* margin_mask_dev;
  int32_t* margin_at_dev;         /* [M] frames_dev[r] * 64 + step of that gap, or NULL */
  const int32_t* frames_dev;
  int32_t step;
} SmolttsPickArgs;

/* 1 when the attention prologue above exists for this head layout (<= 12 query heads, groups of <= 4 per kv head, <= 8 cache entries) */
int smoltts_gemm3_attn_fusable(int32_t n_q_heads, int32_t n_kv_heads, int32_t cache_len);

int smoltts_k_gemm3(const SmolttsGemm3Args* a, void* stream);
/* fp32 rows [n_rows][ldx] -> X3 operand(s) (+ sums of squares), for tests and operands without a fused producer */
int smoltts_k_x3_pack(const float* x_dev, int64_t ldx, int32_t n_rows, int32_t dim, void* x3a_dev,
                      const float* gamma_a_dev, void* x3b_dev, const float* gamma_b_dev, float* ssq_dev,
                      void* stream);

/* Measurement aid of ONE session (bench.py, tools/marginal_cost.py): while code >= 0, every launch of that kernel class
 * inside this session's frames is issued twice -- code = the GEMM's epilogue (and N == n_filter when n_filter > 0;
 * EPI_RESID is refused: not idempotent), 100 = depth (<= 16 keys) attention, 101 = slow attention.  The session's
 * captured graphs are dropped; time a frame graph with and without it: the difference per extra launch is the kernel's
 * in-situ duration.  Other sessions are unaffected (there is no process-global debug state in this library; the event /
 * cycle-stamp hooks of tools/ exist only in diagnostic builds with -DSMOLTTS_DEBUG_HOOKS, built to a separate path). */
int smoltts_session_measure_duplicate(SmolttsSession* s, int32_t code, int32_t n_filter);
/* Forget the captured frame graphs (the next smoltts_lm_decode captures again). */
int smoltts_session_drop_graph(SmolttsSession* s);

/* GQA attention of one query row per (row, kv head) over the slot's cache prefix:
 * keys [max(0, pos+1-window), pos]; q_dev/out_dev [n_rows][n_q_heads*64]; out_x3_dev (optional) receives
 * the same rows as an X3 operand; either output may be NULL. */
int smoltts_k_attention(const float* q_dev, const float* k_cache_dev, const float* v_cache_dev,
                        const int32_t* row_pos_dev, const int32_t* row_slot_dev, int32_t n_rows,
                        int32_t n_q_heads, int32_t n_kv_heads, int32_t cache_len, int32_t window,
                        float* out_dev, void* out_x3_dev, void* stream);

/* The same over a cache stored in kv_format (SMOLTTS_KV_BF16: caches of more than 16 entries). */
int smoltts_k_attention_kv(const float* q_dev, const void* k_cache_dev, const void* v_cache_dev,
                           const int32_t* row_pos_dev, const int32_t* row_slot_dev, int32_t n_rows,
                           int32_t n_q_heads, int32_t n_kv_heads, int32_t cache_len, int32_t window,
                           float* out_dev, void* out_x3_dev, int32_t kv_format, void* stream);
/* (ABI 9, additive) Text mass and first moment of chosen query heads over the keys the attention above sees with window 0
 * (smoltts_session_set_align_heads has the definition), as one launch: q_dev [n_rows][n_q_heads*64]; k_cache_dev
 * [slots][n_kv_heads][cache_len][64] in kv_format; row r is slot row_slot_dev[r] at position row_pos_dev[r] and produces frame
 * row_frame_dev[r]; windows_dev int32 [slots][2] = (t0, t1); heads_host: n_heads <= SMOLTTS_MAX_ALIGN_HEADS query heads;
 * out_dev float [slots][max_frames][n_heads][2].  A row writes nothing when row_mask_dev[r] == 0, its slot's t1 <= t0, its frame
 * index is outside [0, max_frames) or its position outside the cache. */
int smoltts_k_attention_align(const float* q_dev, const void* k_cache_dev, int32_t kv_format, const int32_t* row_pos_dev,
                              const int32_t* row_slot_dev, const int32_t* row_frame_dev, const int32_t* row_mask_dev,
                              const int32_t* windows_dev, const int32_t* heads_host, int32_t n_heads, int32_t n_rows, int32_t n_q_heads,
                              int32_t n_kv_heads, int32_t cache_len, int32_t max_frames, float* out_dev, void* stream);
/* (ABI 9, additive) The score of a GIVEN column of each of n_rows rows of fp32 logits (row r at logits_dev + r * ld, n_cols wide,
 * any width): logprob_dev[r] = the log-probability at temperature 1 of column target_dev[r], by the definition at
 * smoltts_session_set_slot_score with no length entry and no penalty.  One workgroup per row.  A -inf target column gives -inf; a
 * row whose target lies outside [0, n_cols) writes nothing.  Host model: smoltts_amd/sampling.py (pick_logprob). */
int smoltts_k_score_rows(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const int32_t* target_dev,
                         float* logprob_dev, void* stream);
/* The same with the keys of every (row, kv head) pair dealt over two workgroups and merged inside the launch (decode frames
 * at B <= 32: rows x kv heads <= 128, caches longer than 128 entries; other shapes run the one-workgroup kernels).
 * split_part_dev: 128 * 2 * (4 * 64 + 8) floats of scratch; split_ticket_dev: 128 int32 zeroed ONCE (tickets count up across
 * launches: two arrivals per pair and launch). */
int smoltts_k_attention_split(const float* q_dev, const void* k_cache_dev, const void* v_cache_dev, const int32_t* row_pos_dev,
                              const int32_t* row_slot_dev, int32_t n_rows, int32_t n_q_heads, int32_t n_kv_heads, int32_t cache_len,
                              int32_t window, float* out_dev, void* out_x3_dev, int32_t kv_format, float* split_part_dev,
                              int32_t* split_ticket_dev, void* stream);

/* Attention of MANY rows per slot (the codec transformer over a chunk: rows_per_slot consecutive positions per slot,
 * rows_per_slot % 32 == 0, n_rows % rows_per_slot == 0, one query head per kv head) on the bf16 matrix cores over the PIECE
 * caches an EPI_QKV_ROPE GEMM with k_cache3_dev / v_cache3_dev wrote: every K / V value as three bf16 pieces (hi + mid + lo ==
 * the fp32 value exactly), six products per operand pair as in the many-row GEMMs, fp32 accumulation, flash-style softmax.
 * Layouts, per (slot, head) at ((slot * n_heads + head) * ceil32(cache_len) * 384 bytes:
 *   K3: positions in tiles of 16, the 64 dims in two chunks of 32: block (tile, chunk, piece) = 1 KiB at
 *       ((tile * 2 + chunk) * 3 + piece) * 1024; lane l = 16 q + r holds the 8 bf16 K[16 tile + r][32 chunk + 8q .. + 8)
 *       (the "X3" row format of smoltts_amd/csrc/x3.h with K = 64);
 *   V3: positions in blocks of 32, dims in four tiles of 16: block (pb, dim tile t, piece) = 1 KiB at
 *       ((pb * 4 + t) * 3 + piece) * 1024; lane l = 16 q + r holds, for j = 0..7, V[32 pb + (j < 4 ? 4q + j : 16 + 4q + j - 4)][16 t + r]
 *       (the key order in which a lane of the score MFMA holds its eight probabilities of a 32-key block).
 * Same keys as smoltts_k_attention: [max(0, pos + 1 - window), pos] of the row's slot.
 * b3_products (ABI 8): as SmolttsGemmArgs.b3_products -- 3 = three products per operand pair (2^-16-grade: what a codec session with
 * SMOLTTS_MIMI_OPT_PRODUCTS runs), anything else = six. */
int smoltts_k_attention_rows3(const float* q_dev, const void* k_cache3_dev, const void* v_cache3_dev, const int32_t* row_pos_dev,
                              const int32_t* row_slot_dev, int32_t n_rows, int32_t rows_per_slot, int32_t n_heads, int32_t cache_len,
                              int32_t window, float* out_dev, int32_t b3_products, void* stream);

/* x[r] = E_text[cols[r][0]] + keep * sum_k E_cb[cols[r][1+k] + k*codebook_size] */
int smoltts_k_embed(const int32_t* cols_dev, int32_t n_rows, int32_t n_code_rows,
                    const void* text_emb_dev, const void* cb_emb_dev, int32_t dim,
                    int32_t codebook_size, int32_t cb_first_offset, int32_t mask_mode,
                    int32_t sem_start, int32_t sem_end, float* x_dev, void* stream);

/* ids[r] = first index of the row maximum; margin[r] = min(margin[r], top1 - top2). */
int smoltts_k_argmax(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld,
                     int32_t* ids_dev, int32_t ids_stride, float* margin_dev, void* stream);

/* ids[r] ~ softmax(logits[r] / temp) (min_p as above); row r uses the stream (seed, r, frame_base + r, step). */
int smoltts_k_sample(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, float temp, float min_p,
                     uint64_t seed, int32_t frame_base, int32_t step, int32_t* ids_dev, void* stream);

/* (ABI 6) One row per workgroup, row r with its own entry table_dev[r] at `step` (0: temp; > 0: fast_temp, min_p as in the
 * session) and the request key of slot mode with frame frames_dev[r] (NULL: r); ids_dev[r] receives the pick. */
int smoltts_k_sample_rows(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const SmolttsSlotSampling* table_dev,
                          const int32_t* frames_dev, int32_t step, int32_t* ids_dev, void* stream);

/* (ABI 6, additive) smoltts_k_sample_rows with row r's filters filters_dev[r] and an explicit history: history_dev [n_rows][64]
 * int32, newest first, of which row r's first min(history_len_dev[r], its window) ids are penalised. */
int smoltts_k_sample_rows_filtered(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const SmolttsSlotSampling* table_dev,
                                   const SmolttsSlotFilters* filters_dev, const int32_t* frames_dev, const int32_t* history_dev,
                                   const int32_t* history_len_dev, int32_t step, int32_t* ids_dev, void* stream);

/* (ABI 9, additive) smoltts_k_sample_rows / smoltts_k_sample_rows_filtered with row r's length entry length_dev[r] acting on
 * column im_end at step 0, the row's frame counter being frames_dev[r] (NULL: r).  filters_dev may be NULL (then the two history
 * arguments are ignored): the pick without filters. */
int smoltts_k_sample_rows_length(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const SmolttsSlotSampling* table_dev,
                                 const SmolttsSlotFilters* filters_dev, const int32_t* frames_dev, const int32_t* history_dev,
                                 const int32_t* history_len_dev, const SmolttsSlotLength* length_dev, int32_t im_end, int32_t step,
                                 int32_t* ids_dev, void* stream);

/* (ABI 9, additive) smoltts_k_sample_rows_length that also writes logprob_out_dev[r]: the log-probability, at temperature 1, of the
 * id row r emitted under the row as its pick saw it (smoltts_session_set_slot_score has the definition).  length_dev may be NULL too
 * (im_end is then ignored).  The ids are those of smoltts_k_sample_rows_length on the same arguments. */
int smoltts_k_sample_rows_scored(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const SmolttsSlotSampling* table_dev,
                                 const SmolttsSlotFilters* filters_dev, const int32_t* frames_dev, const int32_t* history_dev,
                                 const int32_t* history_len_dev, const SmolttsSlotLength* length_dev, int32_t im_end, int32_t step,
                                 int32_t* ids_dev, float* logprob_out_dev, void* stream);

int smoltts_k_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, int32_t n_rows,
                        int32_t dim, float eps, float* out_dev, void* stream);

/* Test entries of the Mimi decoder's fused stages (the kernels smoltts_mimi_decode_chunk runs, with the caller's buffers).
 *
 * Resnet block of a SEANet stage (128 channels): out[b][t] = ELU(x + conv_k1(ELU(conv_k3(ELU(x)))))[b][t], t < n_rows, causal.
 * x_dev / out_dev point at row 0 of slot 0, channel-last fp32, slot b at + b * x_bstride / o_bstride floats; the two rows in
 * front of every slot's x rows are read (the previous call's last two rows, zeros at a stream's start), nothing in front of
 * out_dev's rows is written.  w2_w3_dev / w3_w3_dev: W3 tiles of the GEMM forms [C/2][3C] (k = tap * C + channel) and [C][C/2]. */
int smoltts_k_seanet_resblock(int32_t channels, int32_t batch, int32_t n_rows, const float* x_dev, int64_t x_bstride,
                              const void* w2_w3_dev, const float* b2_dev, const void* w3_w3_dev, const float* b3_dev, float* out_dev,
                              int64_t o_bstride, int32_t b3_products, void* stream);

/* Last SEANet stage: ConvTranspose1d (128 -> 64, stride 4, kernel 8) + resnet block (64 -> 32 -> 64) + ELU + Conv1d k3 (64 -> 1):
 * pcm[b][4 t + j], t < n_rows, from in[b][t] = ELU(previous stage), channel-last with two halo rows in front of every slot's rows as
 * above.  slot_pos_dev[b] == 0 marks a stream's start: everything in front of the slot's row 0 is the convolutions' zero padding
 * (and its halo rows must be zero); otherwise the halo rows are data.  wt_w3_dev: W3 tiles of the ConvTranspose's GEMM form
 * [256 = j * 64 + channel][256 = (row t-1 | row t) x 128], bt_dev its bias repeated per phase [256]; final_w_dev fp32 [3][64]. */
int smoltts_k_seanet_last(int32_t batch, int32_t n_rows, const float* in_dev, int64_t in_bstride, const void* wt_w3_dev,
                          const float* bt_dev, const void* w2_w3_dev, const float* b2_dev, const void* w3_w3_dev, const float* b3_dev,
                          const float* final_w_dev, float final_b, float* pcm_dev, int64_t pcm_stride, const int32_t* slot_pos_dev,
                          int32_t b3_products, void* stream);

/* RVQ decode + up-sampling: e[b][f] = sum_q table[q][clamp(codes[b][f][code_offset + q], 0, 2047)] (table fp32 [nq][2048][512]),
 * tx[b][2 f + r] = e[f] * upw[r] + e[f - 1] * upw[r + 2] (upw fp32 [4][512]), e[-1] = carry_in_dev[b] (NULL: zero, the stateless
 * mode); carry_out_dev[b] = e[n_frames - 1].  tx_dev is [batch][2 n_frames][512]. */
int smoltts_k_rvq_upsample(const int32_t* codes_dev, int64_t codes_stride, int32_t frame_stride, int32_t code_offset, int32_t nq,
                           int32_t batch, int32_t n_frames, const float* table_dev, const float* upw_dev, const float* carry_in_dev,
                           float* carry_out_dev, float* tx_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMOLTTS_HIP_H */

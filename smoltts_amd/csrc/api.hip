// C-ABI glue: error reporting and the operator-level test entry points (include/smoltts_hip.h).
#include <stdarg.h>

#include "common.h"
#include "mimi_common.h"

namespace smoltts {
static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace smoltts

using namespace smoltts;

extern "C" {

const char* smoltts_last_error(void) { return g_err; }
int smoltts_abi_version(void) { return SMOLTTS_ABI_VERSION; }

int smoltts_k_gemm(const SmolttsGemmArgs* a, void* stream) {
  ST_REQUIRE(a, SMOLTTS_E_INVALID, "k_gemm: null args");
  return launch_gemm(*a, (hipStream_t)stream);
}

int smoltts_k_attention(const float* q_dev, const float* k_cache_dev, const float* v_cache_dev, const int32_t* row_pos_dev,
                        const int32_t* row_slot_dev, int32_t n_rows, int32_t n_q_heads, int32_t n_kv_heads,
                        int32_t cache_len, int32_t window, float* out_dev, void* out_x3_dev, void* stream) {
  return launch_attention(q_dev, k_cache_dev, v_cache_dev, row_pos_dev, row_slot_dev, n_rows, n_q_heads, n_kv_heads, cache_len,
                          window, out_dev, out_x3_dev, (hipStream_t)stream);
}

int smoltts_k_attention_kv(const float* q_dev, const void* k_cache_dev, const void* v_cache_dev, const int32_t* row_pos_dev,
                           const int32_t* row_slot_dev, int32_t n_rows, int32_t n_q_heads, int32_t n_kv_heads,
                           int32_t cache_len, int32_t window, float* out_dev, void* out_x3_dev, int32_t kv_format, void* stream) {
  return launch_attention(q_dev, k_cache_dev, v_cache_dev, row_pos_dev, row_slot_dev, n_rows, n_q_heads, n_kv_heads, cache_len,
                          window, out_dev, out_x3_dev, (hipStream_t)stream, kv_format);
}

int smoltts_k_attention_align(const float* q_dev, const void* k_cache_dev, int32_t kv_format, const int32_t* row_pos_dev,
                              const int32_t* row_slot_dev, const int32_t* row_frame_dev, const int32_t* row_mask_dev,
                              const int32_t* windows_dev, const int32_t* heads_host, int32_t n_heads, int32_t n_rows, int32_t n_q_heads,
                              int32_t n_kv_heads, int32_t cache_len, int32_t max_frames, float* out_dev, void* stream) {
  return launch_attention_align(q_dev, k_cache_dev, kv_format, row_pos_dev, row_slot_dev, row_frame_dev, row_mask_dev, windows_dev,
                                heads_host, n_heads, 0, n_heads, n_rows, n_q_heads, n_kv_heads, cache_len, max_frames, out_dev,
                                (hipStream_t)stream);
}

int smoltts_k_score_rows(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const int32_t* target_dev,
                         float* logprob_dev, void* stream) {
  return launch_score_rows(logits_dev, n_rows, n_cols, ld, target_dev, logprob_dev, (hipStream_t)stream);
}

int smoltts_k_attention_rows3(const float* q_dev, const void* k_cache3_dev, const void* v_cache3_dev, const int32_t* row_pos_dev,
                              const int32_t* row_slot_dev, int32_t n_rows, int32_t rows_per_slot, int32_t n_heads, int32_t cache_len,
                              int32_t window, float* out_dev, int32_t b3_products, void* stream) {
  return launch_attention_rows3(q_dev, k_cache3_dev, v_cache3_dev, row_pos_dev, row_slot_dev, n_rows, rows_per_slot, n_heads, cache_len,
                                window, out_dev, (hipStream_t)stream, b3_products);
}

int smoltts_k_attention_split(const float* q_dev, const void* k_cache_dev, const void* v_cache_dev, const int32_t* row_pos_dev,
                              const int32_t* row_slot_dev, int32_t n_rows, int32_t n_q_heads, int32_t n_kv_heads, int32_t cache_len,
                              int32_t window, float* out_dev, void* out_x3_dev, int32_t kv_format, float* split_part_dev,
                              int32_t* split_ticket_dev, void* stream) {
  ST_REQUIRE(split_part_dev && split_ticket_dev, SMOLTTS_E_INVALID, "k_attention_split: null scratch");
  return launch_attention(q_dev, k_cache_dev, v_cache_dev, row_pos_dev, row_slot_dev, n_rows, n_q_heads, n_kv_heads, cache_len,
                          window, out_dev, out_x3_dev, (hipStream_t)stream, kv_format, -1, split_part_dev, split_ticket_dev);
}

int smoltts_k_embed(const int32_t* cols_dev, int32_t n_rows, int32_t n_code_rows, const void* text_emb_dev,
                    const void* cb_emb_dev, int32_t dim, int32_t codebook_size, int32_t cb_first_offset, int32_t mask_mode,
                    int32_t sem_start, int32_t sem_end, float* x_dev, void* stream) {
  // table heights are unknown here: the test entry point trusts its caller's indices
  return launch_embed(cols_dev, n_rows, n_code_rows, text_emb_dev, cb_emb_dev, dim, codebook_size, cb_first_offset, mask_mode,
                      sem_start, sem_end, 0x7fffffff, 0x7fffffff, x_dev, nullptr, (hipStream_t)stream);
}

int smoltts_k_argmax(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, int32_t* ids_dev, int32_t ids_stride,
                     float* margin_dev, void* stream) {
  return launch_argmax(logits_dev, n_rows, n_cols, ld, ids_dev, ids_stride, margin_dev, nullptr, nullptr, 0, 0, nullptr, nullptr,
                       nullptr, (hipStream_t)stream);
}

int smoltts_k_sample(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, float temp, float min_p, uint64_t seed,
                     int32_t frame_base, int32_t step, int32_t* ids_dev, void* stream) {
  const SampleArgs sa{temp, min_p, seed, step, frame_base, nullptr, nullptr, nullptr};
  return launch_argmax(logits_dev, n_rows, n_cols, ld, ids_dev, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, &sa,
                       (hipStream_t)stream);
}

int smoltts_k_sample_rows(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const SmolttsSlotSampling* table_dev,
                          const int32_t* frames_dev, int32_t step, int32_t* ids_dev, void* stream) {
  ST_REQUIRE(table_dev, SMOLTTS_E_INVALID, "k_sample_rows: null table");
  const SampleArgs sa{0.f, 0.f, 0, step, 0, frames_dev, nullptr, nullptr, table_dev};
  return launch_argmax(logits_dev, n_rows, n_cols, ld, ids_dev, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, &sa,
                       (hipStream_t)stream);
}

int smoltts_k_sample_rows_filtered(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const SmolttsSlotSampling* table_dev,
                                   const SmolttsSlotFilters* filters_dev, const int32_t* frames_dev, const int32_t* history_dev,
                                   const int32_t* history_len_dev, int32_t step, int32_t* ids_dev, void* stream) {
  ST_REQUIRE(table_dev && filters_dev && history_dev && history_len_dev, SMOLTTS_E_INVALID, "k_sample_rows_filtered: null table");
  SampleArgs sa{0.f, 0.f, 0, step, 0, frames_dev, nullptr, nullptr, table_dev};
  sa.filters = filters_dev;
  sa.hist = history_dev; sa.hist_slot_stride = SMOLTTS_FILTER_MAX_WINDOW; sa.hist_frame_stride = 1; sa.hist_frames = SMOLTTS_FILTER_MAX_WINDOW;
  sa.hist_len = history_len_dev;
  return launch_argmax(logits_dev, n_rows, n_cols, ld, ids_dev, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, &sa,
                       (hipStream_t)stream);
}

int smoltts_k_sample_rows_length(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const SmolttsSlotSampling* table_dev,
                                 const SmolttsSlotFilters* filters_dev, const int32_t* frames_dev, const int32_t* history_dev,
                                 const int32_t* history_len_dev, const SmolttsSlotLength* length_dev, int32_t im_end, int32_t step,
                                 int32_t* ids_dev, void* stream) {
  ST_REQUIRE(table_dev && length_dev, SMOLTTS_E_INVALID, "k_sample_rows_length: null table");
  ST_REQUIRE(filters_dev == nullptr || (history_dev && history_len_dev), SMOLTTS_E_INVALID, "k_sample_rows_length: filters without a history");
  ST_REQUIRE(im_end >= 0 && im_end < n_cols, SMOLTTS_E_INVALID, "k_sample_rows_length: im_end %d outside the row (%d columns)", im_end, n_cols);
  SampleArgs sa{0.f, 0.f, 0, step, 0, frames_dev, nullptr, nullptr, table_dev};
  if (filters_dev) {
    sa.filters = filters_dev;
    sa.hist = history_dev; sa.hist_slot_stride = SMOLTTS_FILTER_MAX_WINDOW; sa.hist_frame_stride = 1; sa.hist_frames = SMOLTTS_FILTER_MAX_WINDOW;
    sa.hist_len = history_len_dev;
  }
  sa.length = length_dev;  // (read at step 0 only: argmax_row)
  sa.im_end = im_end;
  return launch_argmax(logits_dev, n_rows, n_cols, ld, ids_dev, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, &sa,
                       (hipStream_t)stream);
}

int smoltts_k_sample_rows_scored(const float* logits_dev, int32_t n_rows, int32_t n_cols, int64_t ld, const SmolttsSlotSampling* table_dev,
                                 const SmolttsSlotFilters* filters_dev, const int32_t* frames_dev, const int32_t* history_dev,
                                 const int32_t* history_len_dev, const SmolttsSlotLength* length_dev, int32_t im_end, int32_t step,
                                 int32_t* ids_dev, float* logprob_out_dev, void* stream) {
  ST_REQUIRE(table_dev && logprob_out_dev, SMOLTTS_E_INVALID, "k_sample_rows_scored: null table or output");
  ST_REQUIRE(filters_dev == nullptr || (history_dev && history_len_dev), SMOLTTS_E_INVALID, "k_sample_rows_scored: filters without a history");
  ST_REQUIRE(length_dev == nullptr || (im_end >= 0 && im_end < n_cols), SMOLTTS_E_INVALID,
             "k_sample_rows_scored: im_end %d outside the row (%d columns)", im_end, n_cols);
  SampleArgs sa{0.f, 0.f, 0, step, 0, frames_dev, nullptr, nullptr, table_dev};
  if (filters_dev) {
    sa.filters = filters_dev;
    sa.hist = history_dev; sa.hist_slot_stride = SMOLTTS_FILTER_MAX_WINDOW; sa.hist_frame_stride = 1; sa.hist_frames = SMOLTTS_FILTER_MAX_WINDOW;
    sa.hist_len = history_len_dev;
  }
  if (length_dev) { sa.length = length_dev; sa.im_end = im_end; }
  sa.logprob = logprob_out_dev;  // (stride 0: row r's value at [r])
  return launch_argmax(logits_dev, n_rows, n_cols, ld, ids_dev, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, &sa,
                       (hipStream_t)stream);
}

int smoltts_k_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, int32_t n_rows, int32_t dim, float eps,
                        float* out_dev, void* stream) {
  return launch_layernorm(x_dev, w_dev, b_dev, n_rows, dim, eps, out_dev, (hipStream_t)stream);
}

int smoltts_k_seanet_resblock(int32_t channels, int32_t batch, int32_t n_rows, const float* x_dev, int64_t x_bstride,
                              const void* w2_w3_dev, const float* b2_dev, const void* w3_w3_dev, const float* b3_dev, float* out_dev,
                              int64_t o_bstride, int32_t b3_products, void* stream) {
  MimiResblockArgs a;
  memset(&a, 0, sizeof(a));
  a.channels = channels; a.batch = batch; a.T = n_rows;
  a.x = x_dev; a.x_bstride = x_bstride;
  a.w2 = w2_w3_dev; a.b2 = b2_dev; a.w3 = w3_w3_dev; a.b3 = b3_dev;
  a.out = out_dev; a.o_bstride = o_bstride;
  a.b3_products = b3_products;
  return launch_seanet_resblock(a, (hipStream_t)stream);
}

int smoltts_k_seanet_last(int32_t batch, int32_t n_rows, const float* in_dev, int64_t in_bstride, const void* wt_w3_dev,
                          const float* bt_dev, const void* w2_w3_dev, const float* b2_dev, const void* w3_w3_dev, const float* b3_dev,
                          const float* final_w_dev, float final_b, float* pcm_dev, int64_t pcm_stride, const int32_t* slot_pos_dev,
                          int32_t b3_products, void* stream) {
  ST_REQUIRE(pcm_stride >= 4 * (int64_t)n_rows, SMOLTTS_E_INVALID, "k_seanet_last: pcm_stride %lld < 4 * %d rows", (long long)pcm_stride,
             n_rows);
  MimiLastStageArgs a;
  memset(&a, 0, sizeof(a));
  a.batch = batch; a.T = n_rows;
  a.in = in_dev; a.in_bstride = in_bstride;
  a.wt = wt_w3_dev; a.bt = bt_dev; a.w2 = w2_w3_dev; a.b2 = b2_dev; a.w3 = w3_w3_dev; a.b3 = b3_dev;
  a.final_w = final_w_dev; a.final_b = final_b;
  a.pcm = pcm_dev; a.pcm_stride = pcm_stride;
  a.slot_pos = slot_pos_dev; a.b3_products = b3_products;
  return launch_seanet_last(a, (hipStream_t)stream);
}

int smoltts_k_rvq_upsample(const int32_t* codes_dev, int64_t codes_stride, int32_t frame_stride, int32_t code_offset, int32_t nq,
                           int32_t batch, int32_t n_frames, const float* table_dev, const float* upw_dev, const float* carry_in_dev,
                           float* carry_out_dev, float* tx_dev, void* stream) {
  return launch_rvq_upsample(codes_dev, codes_stride, frame_stride, code_offset, nq, batch, n_frames, table_dev, upw_dev, carry_in_dev,
                             carry_out_dev, tx_dev, (hipStream_t)stream);
}

}  // extern "C"

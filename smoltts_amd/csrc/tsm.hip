// Per-request speaking speed: a pitch-preserving time stretch of the codec's 24 kHz fp32 PCM, chunk by chunk, in one launch per
// pass over every slot (include/smoltts_hip.h, "Speaking speed"; the numpy model is smoltts_amd/tsm.py).
//
// WSOLA with an integer-exact search: output segment k (L samples) starts at a_k = (k L speed_q + 2^15) >> 16 moved by the lag
// delta in [-kDelta, kDelta] (p_k = a_k + delta >= 0) minimising D(delta) = sum_{n<L} |q[p_k + n] - q[p_{k-1} + L + n]|, q the
// int16 code rint(clip(x, -1, 1) * 32767) in fp32, summed in int32; ties to the smaller |delta|, then the negative one, as the
// minimum of the key (D << 32) | rank(delta).  Overlap-add with a periodic Hann of W = 2L: y[kL + n] = ola[n] + w[n] x[p_k + n],
// then ola[n] = w[n + L] x[p_k + L + n].  p_{-1} = -L (the first L outputs are (w[n] + w[n + L]) x[n]), p_0 = 0.
// Segment k is computed once the input holds a_k + kDelta + W samples and (k + 1) L <= ceil(N 65536 / speed_q); a flush (last)
// reads zeros past the end N and computes segments while k L < M = ceil(N 65536 / speed_q), cutting the output at M.
#include "stage.h"

using namespace smoltts;

namespace {

constexpr int L = 240, W = 2 * L, kDelta = 192, kLags = 2 * kDelta + 1;
constexpr int kHist = 2048;    // input carried from call to call (a stream needs at most ~1.9k: DESIGN.md 11)
constexpr int kThreads = 256;  // 4 waves: lane t owns lags t and t + 256, and output sample t of a segment
constexpr int kPiece = 4096;   // LDS window of staged input; one segment needs at most ~1.9k of it
constexpr int kQOne = 65536;
static_assert(kLags <= 2 * kThreads && L <= kThreads, "tsm: lane layout");

struct TsmState {  // one half of the ping-pong pair, per slot
  int64_t k;       // next segment
  int64_t p_prev;  // p_{k-1}
  int64_t n_in;    // input samples consumed
  int64_t n_out;   // output samples emitted
  int32_t ended;   // flushed: the stream emits nothing more
  int32_t pad[7];
  float ola[L];        // the open half-window: w[n + L] x[p_{k-1} + L + n]
  float hist[kHist];   // input [n_in - kHist, n_in) (zeros before the stream's start)
};

__device__ __forceinline__ int to_q(float v) {  // fp32, as numpy: rint(clip(x, -1, 1) * 32767)
  return __float2int_rn(fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f);
}

__device__ __forceinline__ uint32_t lag_rank(int d) { return d == 0 ? 0u : (d < 0 ? (uint32_t)(-2 * d - 1) : (uint32_t)(2 * d)); }
__device__ __forceinline__ int rank_lag(uint32_t r) { return r == 0 ? 0 : ((r & 1u) ? -(int)((r + 1) >> 1) : (int)(r >> 1)); }

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// grid (max_batch), 256 lanes: workgroup b runs slot b's segments of this call serially.  States ping-pong between st_in and
// st_out (the host alternates them), so no workgroup reads what another one writes in the same launch; slots at or past `batch`
// only carry their state across, slots that are off (speed_q 0) write count 0 and nothing else.
__global__ __launch_bounds__(kThreads) void tsm_kernel(const float* __restrict__ pcm, int64_t pcm_stride, int batch, int n_in,
                                                       const int32_t* __restrict__ valid, const int32_t* __restrict__ last,
                                                       const int32_t* __restrict__ cfg_sq, const float* __restrict__ win,
                                                       const TsmState* __restrict__ st_in, TsmState* __restrict__ st_out,
                                                       float* __restrict__ out, int64_t out_stride, int32_t* __restrict__ counts) {
  __shared__ float xs[kPiece];
  __shared__ int16_t qs[kPiece];
  __shared__ uint64_t red[kThreads / 64];
  __shared__ int64_t sh_p;
  const int b = blockIdx.x, t = threadIdx.x;
  const int sq = cfg_sq[b];
  if (sq == 0) {
    if (b < batch && t == 0) counts[b] = 0;
    return;
  }
  const TsmState* si = st_in + b;
  TsmState* so = st_out + b;
  if (si->ended) {  // a flushed stream: only its counters matter until the slot is reset
    if (t == 0) {
      so->k = si->k; so->p_prev = si->p_prev; so->n_in = si->n_in; so->n_out = si->n_out; so->ended = 1;
      if (b < batch) counts[b] = 0;
    }
    return;
  }
  if (b >= batch) {  // not in this call: the state moves to the other half unchanged
    if (t < L) so->ola[t] = si->ola[t];
    for (int i = t; i < kHist; i += kThreads) so->hist[i] = si->hist[i];
    if (t == 0) {
      so->k = si->k; so->p_prev = si->p_prev; so->n_in = si->n_in; so->n_out = si->n_out; so->ended = 0;
    }
    return;
  }
  const int n = valid_count(valid, b, n_in);
  const int fl = last ? (last[b] != 0) : 0;
  const int64_t N0 = si->n_in, N1 = N0 + n;
  const int64_t mcap = (N1 * kQOne + sq - 1) / sq;  // M of the input so far
  const float* x = pcm + (int64_t)b * pcm_stride;
  // input sample j of the stream: the call's rows, the carried history, zeros outside
  auto sample = [&](int64_t j) -> float {
    if (j >= N1 || j < 0) return 0.0f;
    if (j >= N0) return x[j - N0];
    const int64_t h = j - (N0 - kHist);
    return h >= 0 ? si->hist[h] : 0.0f;
  };
  int64_t k = si->k, pprev = si->p_prev;
  const int64_t out0 = si->n_out;
  float ola = t < L ? si->ola[t] : 0.0f;
  const float w0 = t < L ? win[t] : 0.0f, w1 = t < L ? win[t + L] : 0.0f;
  float* orow = out + (int64_t)b * out_stride;
  int64_t s_lo = 0;
  bool staged = false;
  for (;;) {
    const int64_t a = (k * L * (int64_t)sq + 32768) >> 16;
    const bool ok = fl ? (k * L < mcap) : (a + kDelta + W <= N1 && (k + 1) * L <= mcap);
    if (!ok) break;
    const int64_t lo_c = a - kDelta > 0 ? a - kDelta : 0;
    const int64_t need_lo = pprev + L < lo_c ? pprev + L : lo_c, need_hi = a + kDelta + W;
    if (need_hi - need_lo > kPiece) break;  // (cannot happen: <= 1585 samples; keeps every LDS index in the window)
    if (!staged || need_lo < s_lo || need_hi > s_lo + kPiece) {
      __syncthreads();  // every lane is through with the previous window
      s_lo = need_lo;
      staged = true;
      for (int i = t; i < kPiece; i += kThreads) {
        const float v = sample(s_lo + i);
        xs[i] = v;
        qs[i] = (int16_t)to_q(v);
      }
      __syncthreads();
    }
    int64_t p = 0;
    if (k > 0) {
      // lane t scores lags t - kDelta and t + 256 - kDelta against the reference run q[p_{k-1} + L ..] (a broadcast read)
      const int rb = (int)(pprev + L - s_lo);
      const bool v0 = a - kDelta + t >= 0;
      const bool v1 = t + kThreads < kLags && a - kDelta + t + kThreads >= 0;
      const int c0 = v0 ? (int)(a - kDelta + t - s_lo) : 0;
      const int c1 = v1 ? (int)(a - kDelta + t + kThreads - s_lo) : 0;
      // (volatile: one 16-bit LDS read per code; merged into ds_read_b128 at the lanes' odd 2-byte offsets the reads were
      // misaligned, and a segment took ~10 us)
      const volatile __attribute__((address_space(3))) int16_t* q = (const volatile __attribute__((address_space(3))) int16_t*)qs;
      int acc0 = 0, acc1 = 0;
#pragma unroll 8
      for (int i = 0; i < L; ++i) {
        const int r = q[rb + i];
        acc0 += abs((int)q[c0 + i] - r);
        acc1 += abs((int)q[c1 + i] - r);
      }
      uint64_t key = v0 ? ((uint64_t)(uint32_t)acc0 << 32) | lag_rank(t - kDelta) : ~0ull;
      if (v1) key = umin64(key, ((uint64_t)(uint32_t)acc1 << 32) | lag_rank(t + kThreads - kDelta));
      for (int off = 32; off > 0; off >>= 1) key = umin64(key, (uint64_t)__shfl_xor((unsigned long long)key, off, 64));
      if ((t & 63) == 0) red[t >> 6] = key;
      __syncthreads();
      if (t == 0) {
        uint64_t m = red[0];
        for (int i = 1; i < kThreads / 64; ++i) m = umin64(m, red[i]);
        sh_p = a + rank_lag((uint32_t)(m & 0xffffffffu));
      }
      __syncthreads();
      p = sh_p;
    }
    if (t < L) {
      const int i = (int)(p - s_lo) + t;
      const float y = ola + w0 * xs[i];
      ola = w1 * xs[i + L];
      const int64_t pos = k * L + t;
      const int64_t o = pos - out0;
      if (pos < mcap && o < out_stride) orow[o] = y;
    }
    pprev = p;
    ++k;
  }
  const int64_t end = fl ? mcap : k * L;
  if (t < L) so->ola[t] = ola;
  for (int i = t; i < kHist; i += kThreads) so->hist[i] = sample(N1 - kHist + i);
  if (t == 0) {
    so->k = k;
    so->p_prev = pprev;
    so->n_in = N1;
    so->n_out = end;
    so->ended = fl;
    counts[b] = (int32_t)(end - out0);
  }
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  int32_t sq[kResetMax];
};

// workgroup i: slot args.slot[i] gets its speed and an empty stream in both state halves
__global__ __launch_bounds__(kThreads) void tsm_reset_kernel(ResetArgs a, int32_t* cfg_sq, TsmState* st0, TsmState* st1) {
  const int i = blockIdx.x, t = threadIdx.x;
  if (i >= a.n) return;
  const int b = a.slot[i];
  for (int j = t; j < kHist; j += kThreads) st0[b].hist[j] = st1[b].hist[j] = 0.0f;
  if (t < L) st0[b].ola[t] = st1[b].ola[t] = 0.0f;
  if (t == 0) {
    cfg_sq[b] = a.sq[i];
    st0[b].k = st1[b].k = 0;
    st0[b].p_prev = st1[b].p_prev = -L;
    st0[b].n_in = st1[b].n_in = st0[b].n_out = st1[b].n_out = 0;
    st0[b].ended = st1[b].ended = 0;
  }
}

}  // namespace

struct SmolttsTsm {
  int B;
  float* win_dev;
  int32_t* cfg_dev;
  PingPong<TsmState> st;
};

// the slab: the constant window, then what create clears (every slot off)
static size_t carve(SmolttsTsm* r, char* base) {
  Carver cv{base, 0};
  r->win_dev = cv.take<float>(W);
  r->cfg_dev = cv.take<int32_t>(r->B);
  r->st.carve(cv, r->B);
  return cv.off;
}

extern "C" {

size_t smoltts_tsm_bytes(int32_t max_batch) {
  return stage_bytes<SmolttsTsm>(max_batch);
}

size_t smoltts_tsm_out_samples(int32_t n_in) {
  if (n_in < 0) return 0;
  // after a call the next segment k was not computable: k L >= (N0 - kDelta - W) / 4 - 1 at speed 0.25; the call ends at or
  // before ceil(N1 / 0.25)
  return 4 * (size_t)n_in + 4 * (size_t)(kDelta + W) + L;
}

int smoltts_tsm_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsTsm** out) {
  SmolttsTsm* r = nullptr;
  size_t need = 0;
  ST_TRY(stage_create("tsm_create", slab_dev, slab_bytes, max_batch, out, &r, &need));
  float w[W];
  for (int n = 0; n < W; ++n) w[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)W));  // periodic Hann, fp64 -> fp32
  const bool ok = hipMemcpy(r->win_dev, w, sizeof(w), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(r->cfg_dev, 0, need - ((char*)r->cfg_dev - (char*)slab_dev)) == hipSuccess;  // every slot off
  if (!ok) {
    delete r;
    set_error("tsm_create: hipMemcpy / hipMemset failed");
    return SMOLTTS_E_HIP;
  }
  *out = r;
  return SMOLTTS_OK;
}

void smoltts_tsm_destroy(SmolttsTsm* r) {
  delete r;
}

int smoltts_tsm_reset_slots(SmolttsTsm* r, const int32_t* slots_host, const int32_t* speed_q_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(r && slots_host && speed_q_host && n_slots > 0, SMOLTTS_E_INVALID, "tsm_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    const int sq = speed_q_host[k];
    ST_REQUIRE(sq == kQOne || (sq >= 16384 && sq <= 262144), SMOLTTS_E_INVALID,
               "tsm_reset_slots: speed_q %d outside [16384, 262144]", sq);
    a.sq[i] = sq == kQOne ? 0 : sq;  // speed 1: the slot is off
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("tsm_reset_slots", r->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    hipLaunchKernelGGL(tsm_reset_kernel, dim3(a.n), dim3(kThreads), 0, (hipStream_t)stream, a, r->cfg_dev, r->st.half[0], r->st.half[1]);
  });
}

int smoltts_tsm_chunk(SmolttsTsm* r, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                      const int32_t* valid_in_dev, const int32_t* last_dev, float* out_dev, int64_t out_stride,
                      int32_t* counts_dev, void* stream) {
  ST_TRY(check_chunk("tsm_chunk", r, pcm_dev && out_dev && counts_dev, batch, true, n_in, pcm_stride));
  const int64_t need = (int64_t)smoltts_tsm_out_samples(n_in);
  ST_REQUIRE(out_stride >= need, SMOLTTS_E_CAPACITY, "tsm_chunk: out_stride %lld < %lld samples", (long long)out_stride, (long long)need);
  hipLaunchKernelGGL(tsm_kernel, dim3(r->B), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, pcm_stride, batch, n_in, valid_in_dev,
                     last_dev, r->cfg_dev, r->win_dev, r->st.cur(), r->st.next(), out_dev, out_stride, counts_dev);
  ST_CHECK_HIP(hipGetLastError());
  r->st.flip();
  return SMOLTTS_OK;
}

int smoltts_tsm_slot_state(SmolttsTsm* r, int32_t slot, int64_t* state_host, void* stream) {
  ST_REQUIRE(r && state_host && slot >= 0 && slot < r->B, SMOLTTS_E_INVALID, "tsm_slot_state: bad argument");
  const TsmState* s = r->st.cur() + slot;
  int64_t v[4];
  int32_t ended = 0;
  ST_CHECK_HIP(hipMemcpyAsync(v, &s->k, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
  ST_CHECK_HIP(hipMemcpyAsync(&ended, &s->ended, sizeof(ended), hipMemcpyDeviceToHost, (hipStream_t)stream));
  ST_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (int i = 0; i < 4; ++i) state_host[i] = v[i];
  state_host[4] = ended;
  return SMOLTTS_OK;
}

}  // extern "C"

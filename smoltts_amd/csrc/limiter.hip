// A look-ahead peak limiter on the codec's 24 kHz fp32 PCM, the last float stage, in one launch per pass over every slot
// (include/smoltts_hip.h, "Limiter"; the numpy model, which this file reproduces bit for bit, is
// smoltts_amd/limiter.py).
//
// A row is worked in rounds of at most kRound samples.  A round that takes the stream from f to f + n: lane i sets the required
// gain r of samples f - 6 + i, i + 1024, ... (their last interpolator tap has arrived: three 12-tap phases in ascending tap
// order, the maximum of their magnitudes and the sample's own, c / p where that passes c) behind the kHist values of r the
// round in front left in LDS; the minimum of every aligned block of kBlk values of r goes to LDS; lane u sets m of samples
// f - 246 + u, ...: the minimum over r's window of kWin values as the 40 blocks inside it and the 41 values at its two ends
// (the minimum is order-free, so this gives the model's bits); lane i sums the 121 values of m behind sample f - 126 + i oldest
// first, and writes the sample times the smaller of that mean and its own r.  The slot keeps the last 126 samples and the last
// kHist values of r, so the numbers do not depend on how calls cut the stream; a stream's end pushes the held samples out with
// zeros behind them, whose r is 1.
//
// Every fp64 operation is a single rounded multiply, add or divide, a minimum, a maximum or a compare in the model's order (no
// contraction in this file).  The device designs nothing: the interpolator is uploaded at create.
#include "stage.h"

#pragma clang fp contract(off)

using namespace smoltts;

namespace {

constexpr int kL = 120, kR = 1200, kLo = 5, kHi = 6, kTaps = kLo + kHi + 1, kHold = kL + kHi;
constexpr int kWin = kR + kL + 1, kMean = kL + 1, kHist = kR + 2 * kL;
constexpr int kThreads = 1024;  // 16 waves: the chains of LDS reads below hide behind one another only with many waves in flight
constexpr int kRound = 1920, kBlk = 32, kBlocks = (kHist + kRound) / kBlk;
constexpr int kKeep = (kHist + kThreads - 1) / kThreads;  // values of r a lane carries to the next round
constexpr int kTab = 3 * kTaps;
constexpr int kCallMax = 61440, kApplyMax = 1 << 26;
constexpr int kFull = (kWin - kBlk + 1) / kBlk, kEnds = kWin - kFull * kBlk;  // whole blocks inside every window; the rest, at its two ends
static_assert(kBlk == 32 && (kHist + kRound) % kBlk == 0 && kFull == 40 && kEnds == 41, "limiter: block minimum layout");

struct LimState {  // one half of the ping-pong pair, per slot
  double r[kHist];  // r of samples pos - 1446 .. pos - 7 (1 before the stream)
  double c;         // the ceiling, 10^(peak_limit_db / 20)
  double min_g;     // the smallest gain applied so far
  int64_t pos;      // samples consumed
  float x[kHold];   // samples pos - 126 .. pos - 1 (0 before the stream)
  int32_t on, ended;
};
static_assert(sizeof(LimState) == 8 * kHist + 24 + 4 * kHold + 8, "limiter: state layout");

struct Scratch {  // per workgroup, in LDS
  double r[kHist + kRound];        // r of samples f - 1446 .. f + n - 7
  double m[kRound + kL];           // m of samples f - 246 .. f + n - 127
  double xs[kRound + kTaps - 1];   // samples f - 11 .. f + n - 1; at the row's end the lanes' smallest gains
  double bm[kBlocks];              // min r[32 k .. 32 k + 31]
};
static_assert(kRound + kTaps - 1 >= kThreads, "limiter: the reduction borrows xs");
static_assert(sizeof(Scratch) <= 65536, "limiter: LDS");

// sample j of a call of n samples at x; the 126 in front of it are the slot's (hist; null: zeros), those behind it zeros
__device__ __forceinline__ float x_at(const float* __restrict__ hist, const float* __restrict__ x, int n, int j) {
  if (j < 0) return hist ? hist[kHold + j] : 0.0f;
  return j < n ? x[j] : 0.0f;
}

// numpy's maximum: a NaN on either side stays
__device__ __forceinline__ double max_nan(double p, double a) {
  return p != p ? p : ((a > p || a != a) ? a : p);
}

// n samples of one stream at position pos0 from x, the samples that become final to y; `last`: the stream ends behind them.
// in / out: the slot's state before and after (both null: a stream that starts here and keeps nothing).  Returns the smallest
// gain of the call (1 without output), the same in every lane.
__device__ __forceinline__ double limit_row(Scratch& sc, const double* __restrict__ tab, const LimState* __restrict__ in,
                                            LimState* __restrict__ out, double c, int64_t pos0, const float* __restrict__ x, int n,
                                            bool last, float* __restrict__ y) {
  const int t = threadIdx.x;
  const float* hist = in ? in->x : nullptr;
  for (int i = t; i < kHist; i += kThreads) sc.r[i] = in ? in->r[i] : 1.0;
  const int nv = n + (last ? kHold : 0);               // the zeros behind the end push the held samples out
  const int64_t end = last ? pos0 + n : INT64_MAX;     // r is 1 from here on
  const int64_t base = pos0 > kHold ? pos0 - kHold : 0;  // y[0]'s position
  double gmin = 1.0;
  for (int done = 0; done < nv;) {
    const int mi = nv - done < kRound ? nv - done : kRound;
    const int64_t f = pos0 + done;
    for (int i = t; i < mi + kTaps - 1; i += kThreads) sc.xs[i] = (double)x_at(hist, x, n, done - (kTaps - 1) + i);
    __syncthreads();
    for (int i = t; i < mi; i += kThreads) {  // r of sample f - 6 + i
      const int64_t at = f - kHi + i;
      double p = __builtin_fabs(sc.xs[i + kLo]);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) acc = acc + tab[q * kTaps + k] * sc.xs[i + k];
        p = max_nan(p, __builtin_fabs(acc));
      }
      sc.r[kHist + i] = (at >= 0 && at < end && p > c) ? c / p : 1.0;
    }
    __syncthreads();
    for (int k = t; k < (kHist + mi) / kBlk; k += kThreads) {  // (lane k starts at element k of its block: no two lanes on a bank)
      double v = 1.0;
      for (int j = 0; j < kBlk; ++j) v = __builtin_fmin(v, sc.r[k * kBlk + ((j + k) & (kBlk - 1))]);
      sc.bm[k] = v;
    }
    __syncthreads();
    for (int u = t; u < mi + kL; u += kThreads) {  // m of sample f - 246 + u: min r[u .. u + kWin - 1] (every r <= 1)
      // the kFull blocks behind the one u lies in are inside every window; what is left of the window, kEnds values, lies
      // in front of them (the rest of u's block) and behind them: trip counts that do not depend on u
      double v[4] = {1.0, 1.0, 1.0, 1.0};
      if (f - kHold - kL + u >= 0) {
        const int b0 = u / kBlk, head = kBlk - u % kBlk;
#pragma unroll
        for (int k = 0; k < kFull; ++k) v[k & 3] = __builtin_fmin(v[k & 3], sc.bm[b0 + 1 + k]);
#pragma unroll
        for (int j = 0; j < kEnds; ++j) v[j & 3] = __builtin_fmin(v[j & 3], sc.r[u + j + (j >= head ? kFull * kBlk : 0)]);
      }
      sc.m[u] = __builtin_fmin(__builtin_fmin(v[0], v[1]), __builtin_fmin(v[2], v[3]));
    }
    __syncthreads();
    for (int i = t; i < mi; i += kThreads) {  // sample f - 126 + i
      double s = 0.0;
#pragma unroll 11
      for (int k = 0; k < kMean; ++k) s = s + sc.m[i + k];
      const double g = __builtin_fmin(sc.r[kR + kL + i], s / (double)kMean);
      gmin = __builtin_fmin(gmin, g);
      const int64_t at = f - kHold + i;
      if (at >= 0) y[at - base] = (float)((double)x_at(hist, x, n, done - kHold + i) * g);
    }
    __syncthreads();
    double keep[kKeep];  // the last kHist values of r move to the front
#pragma unroll
    for (int q = 0; q < kKeep; ++q) keep[q] = t + q * kThreads < kHist ? sc.r[mi + t + q * kThreads] : 0.0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kKeep; ++q)
      if (t + q * kThreads < kHist) sc.r[t + q * kThreads] = keep[q];
    done += mi;
  }
  __syncthreads();
  sc.xs[t] = gmin;
  __syncthreads();
  if (out) {
    for (int i = t; i < kHist; i += kThreads) out->r[i] = sc.r[i];
    if (t < kHold) out->x[t] = x_at(hist, x, n, n - kHold + t);
  }
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) sc.xs[t] = __builtin_fmin(sc.xs[t], sc.xs[t + s]);
    __syncthreads();
  }
  return sc.xs[0];
}

// grid (max_batch), 1024 lanes: workgroup b runs slot b.  States ping-pong between st_in and st_out (the host alternates them);
// slots at or past `batch` and slots whose stream has ended only carry their state across, slots that are off write count 0
// and leave their rows alone.
__global__ __launch_bounds__(kThreads) void limiter_kernel(const float* __restrict__ pcm, int64_t pcm_stride, int batch, int n_in,
                                                           const int32_t* __restrict__ valid, const int32_t* __restrict__ last,
                                                           const double* __restrict__ tab, const LimState* __restrict__ st_in,
                                                           LimState* __restrict__ st_out, float* __restrict__ out, int64_t out_stride,
                                                           int32_t* __restrict__ counts) {
  __shared__ Scratch sc;
  const int b = blockIdx.x, t = threadIdx.x;
  const LimState* in = st_in + b;
  LimState* o = st_out + b;
  if (!in->on) {
    if (t == 0) {
      o->on = 0;
      if (b < batch) counts[b] = 0;
    }
    return;
  }
  const double c = in->c, g0 = in->min_g;
  const int64_t pos = in->pos;
  const int ended = in->ended;
  const bool live = b < batch && !ended;
  const int n = live ? valid_count(valid, b, n_in) : 0;
  const bool fin = live && last && last[b] != 0;
  const int64_t row = live ? b : 0;
  const double g = limit_row(sc, tab, in, o, c, pos, pcm + row * pcm_stride, n, fin, out + row * out_stride);
  if (t == 0) {
    o->c = c;
    o->min_g = __builtin_fmin(g0, g);
    o->pos = pos + n;
    o->on = 1;
    o->ended = ended | (fin ? 1 : 0);
    if (b < batch) {
      const int64_t before = pos > kHold ? pos - kHold : 0, after = fin ? pos + n : (pos + n > kHold ? pos + n - kHold : 0);
      counts[b] = live ? (int32_t)(after - before) : 0;
    }
  }
}

// A whole utterance from position 0 to its end, one workgroup, no slot; result[0] = its smallest gain
__global__ __launch_bounds__(kThreads) void limiter_apply_kernel(const float* __restrict__ x, int n, double c, const double* __restrict__ tab,
                                                                 float* __restrict__ y, double* __restrict__ result) {
  __shared__ Scratch sc;
  const double g = limit_row(sc, tab, nullptr, nullptr, c, 0, x, n, true, y);
  if (threadIdx.x == 0) result[0] = g;
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  double ceiling[kResetMax];
};

// workgroup i: slot args.slot[i] starts a stream (or is switched off) in both state halves
__global__ __launch_bounds__(kThreads) void limiter_reset_kernel(ResetArgs a, LimState* st0, LimState* st1) {
  const int i = blockIdx.x, t = threadIdx.x;
  if (i >= a.n) return;
  LimState* s[2] = {st0 + a.slot[i], st1 + a.slot[i]};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    for (int j = t; j < kHist; j += kThreads) s[h]->r[j] = 1.0;
    if (t < kHold) s[h]->x[t] = 0.0f;
    if (t == 0) {
      s[h]->c = a.ceiling[i];
      s[h]->min_g = 1.0;
      s[h]->pos = 0;
      s[h]->on = a.ceiling[i] > 0.0 ? 1 : 0;
      s[h]->ended = 0;
    }
  }
}

}  // namespace

struct SmolttsLimiter {
  int B;
  PingPong<LimState> st;
  double* tab;
};

static size_t carve(SmolttsLimiter* r, char* base) {
  Carver cv{base, 0};
  r->st.carve(cv, r->B);
  r->tab = cv.take<double>(kTab);
  return cv.off;
}

static bool ceiling_ok(double c, bool may_be_off) {
  return (c > 0.0 && c <= 1.0) || (may_be_off && c == 0.0);  // (a NaN fails)
}

extern "C" {

size_t smoltts_limiter_bytes(int32_t max_batch) {
  return stage_bytes<SmolttsLimiter>(max_batch);
}

int32_t smoltts_limiter_table_doubles(void) {
  return kTab;
}

int smoltts_limiter_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, const double* tables_host, int32_t n_tables,
                           SmolttsLimiter** out) {
  ST_REQUIRE(tables_host && n_tables == kTab, SMOLTTS_E_INVALID, "limiter_create: tables of %d doubles, %d expected", n_tables, kTab);
  for (int i = 0; i < kTab; ++i)
    ST_REQUIRE(tables_host[i] >= -1.0 && tables_host[i] <= 1.0, SMOLTTS_E_INVALID, "limiter_create: tap %d is not within +-1", i);
  SmolttsLimiter* r = nullptr;
  size_t need = 0;
  ST_TRY(stage_create("limiter_create", slab_dev, slab_bytes, max_batch, out, &r, &need));
  if (hipMemset(slab_dev, 0, need) != hipSuccess ||  // every slot off
      hipMemcpy(r->tab, tables_host, kTab * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    delete r;
    set_error("limiter_create: clearing the slab or uploading the tables failed");
    return SMOLTTS_E_HIP;
  }
  *out = r;
  return SMOLTTS_OK;
}

void smoltts_limiter_destroy(SmolttsLimiter* r) {
  delete r;
}

size_t smoltts_limiter_out_samples(int32_t n_in) {
  return n_in < 0 || n_in > kCallMax ? 0 : (size_t)n_in + kHold;
}

int smoltts_limiter_reset_slots(SmolttsLimiter* r, const int32_t* slots_host, const double* ceiling_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(r && slots_host && ceiling_host && n_slots > 0, SMOLTTS_E_INVALID, "limiter_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    ST_REQUIRE(ceiling_ok(ceiling_host[k], true), SMOLTTS_E_INVALID, "limiter_reset_slots: ceiling %g outside [0, 1]", ceiling_host[k]);
    a.ceiling[i] = ceiling_host[k];
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("limiter_reset_slots", r->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    hipLaunchKernelGGL(limiter_reset_kernel, dim3(a.n), dim3(kThreads), 0, (hipStream_t)stream, a, r->st.half[0], r->st.half[1]);
  });
}

int smoltts_limiter_chunk(SmolttsLimiter* r, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                          const int32_t* valid_in_dev, const int32_t* last_dev, float* out_dev, int64_t out_stride, int32_t* counts_dev,
                          void* stream) {
  ST_TRY(check_chunk("limiter_chunk", r, pcm_dev && out_dev && counts_dev, batch, true, n_in, pcm_stride));
  ST_REQUIRE(n_in <= kCallMax, SMOLTTS_E_INVALID, "limiter_chunk: n_in %d above %d", n_in, kCallMax);
  ST_REQUIRE(out_stride >= (int64_t)n_in + kHold, SMOLTTS_E_CAPACITY, "limiter_chunk: out_stride %lld < %d samples", (long long)out_stride,
             n_in + kHold);
  hipLaunchKernelGGL(limiter_kernel, dim3(r->B), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, pcm_stride, batch, n_in, valid_in_dev,
                     last_dev, r->tab, r->st.cur(), r->st.next(), out_dev, out_stride, counts_dev);
  ST_CHECK_HIP(hipGetLastError());
  r->st.flip();
  return SMOLTTS_OK;
}

int smoltts_limiter_apply(SmolttsLimiter* r, const float* pcm_dev, int32_t n, double ceiling, float* out_dev, double* result_dev,
                          void* stream) {
  ST_REQUIRE(r && pcm_dev && out_dev && result_dev, SMOLTTS_E_INVALID, "limiter_apply: null argument");
  ST_REQUIRE(n >= 0 && n <= kApplyMax, SMOLTTS_E_INVALID, "limiter_apply: n %d (0..%d)", n, kApplyMax);
  ST_REQUIRE(ceiling_ok(ceiling, false), SMOLTTS_E_INVALID, "limiter_apply: ceiling %g outside (0, 1]", ceiling);
  hipLaunchKernelGGL(limiter_apply_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, n, ceiling, r->tab, out_dev, result_dev);
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

int smoltts_limiter_slot_state(SmolttsLimiter* r, int32_t slot, int64_t* ints_host, double* values_host, void* stream) {
  ST_REQUIRE(r && ints_host && values_host && slot >= 0 && slot < r->B, SMOLTTS_E_INVALID, "limiter_slot_state: bad argument");
  LimState* s = new (std::nothrow) LimState;
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "limiter_slot_state: out of host memory");
  hipError_t e = hipMemcpyAsync(s, r->st.cur() + slot, sizeof(LimState), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess) {
    ints_host[0] = s->pos; ints_host[1] = s->on; ints_host[2] = s->ended;
    values_host[0] = s->c; values_host[1] = s->min_g;
    for (int i = 0; i < kHist; ++i) values_host[2 + i] = s->r[i];
    for (int i = 0; i < kHold; ++i) values_host[2 + kHist + i] = (double)s->x[i];
  }
  delete s;
  ST_CHECK_HIP(e);
  return SMOLTTS_OK;
}

}  // extern "C"

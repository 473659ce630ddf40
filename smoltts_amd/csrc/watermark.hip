// A keyed spread-spectrum watermark added to the codec's 24 kHz fp32 PCM, in one launch per pass over every slot
// (include/smoltts_hip.h, "Watermark"; the numpy model, which this file reproduces bit for bit, is
// smoltts_amd/watermark.py).
//
// A row is worked in rounds of at most kRound samples cut on the stream's own grid of kSub samples.  Phase 1: lane i sums x^2
// over sub-block i, sample after sample; lane k then folds, in order, the sums that fall into the round's k-th block (the
// first goes on from the open block's energy), and where a block of kBlock samples completes every lane sets the gain of the
// block behind it, a * sqrt(E / kBlock).  The round's chips, scaled by their blocks' gains, go to LDS with the kTaps - 1
// samples in front of them (at most two blocks back: the slot keeps the open and the previous block's gain).  Phase 2: lane t
// writes samples t, t + 256, ...: kTaps multiply-adds each, in ascending tap order.  A call that ends inside a sub-block keeps
// its running sum, so the numbers do not depend on how calls cut the stream.
//
// Every fp64 operation is a single rounded multiply, add, divide or square root in the model's order (no contraction in this
// file; the only fused operations are the explicit ones of sqrt_rn's test).  The device hashes nothing and designs nothing:
// the chip table and the shaping filter are uploaded at create.
#include "stage.h"

#pragma clang fp contract(off)

using namespace smoltts;

namespace {

constexpr int kBlock = 480, kPeriod = 32 * kBlock, kTaps = 65, kSub = 16, kPer = kBlock / kSub;
constexpr int kThreads = 256;             // 4 waves
constexpr int kRound = kThreads * kSub;   // samples of a round: one sub-block per lane
constexpr int kPerLane = kRound / kThreads;
constexpr int kGains = (kBlock - 1 + kRound) / kBlock + 2;  // the previous block, the open one, and every block a round can complete
constexpr int kH = 0, kChip = kTaps, kTab = kTaps + kPeriod;
constexpr int kEmbedMax = 1 << 26;

struct MarkState {  // one half of the ping-pong pair, per slot
  double e_sub;   // sum of x^2 over the open sub-block so far
  double e_blk;   // the open block's complete sub-blocks, folded
  double g_cur;   // gain of block pos / kBlock
  double g_prev;  // gain of the block in front of it
  double a;       // 10^(strength_db / 20)
  int64_t pos;    // samples consumed
  int32_t on, pad;
};
static_assert(sizeof(MarkState) == 56, "watermark: state layout");

struct Scratch {  // per workgroup, in LDS
  double u[kRound + kTaps - 1];  // g * chip of the round's samples, behind the kTaps - 1 in front of them
  double e[kThreads];            // the round's sub-block sums
  double eb[kGains];             // the sums of the blocks they fall into
  double g[kGains];
};

// The correctly rounded square root of v >= 0.  The hardware's estimate s is moved by one unit in the last place while the
// neighbours' products say so: s is the nearest double to sqrt(v) exactly when s_down * s < v <= s * s_up (v lies on a coarser
// grid than the half-way points' squares, so the two products decide), and a fused multiply-add gives the sign of s * s_up - v
// without a rounding that could change it.  Two rounds cover an estimate two units off.
__device__ __forceinline__ double sqrt_rn(double v) {
  if (!(v > 0.0)) return 0.0;
  double s = __builtin_sqrt(v);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double up = __longlong_as_double(__double_as_longlong(s) + 1);
    const double dn = __longlong_as_double(__double_as_longlong(s) - 1);
    if (__builtin_fma(s, up, -v) < 0.0) s = up;
    else if (__builtin_fma(dn, s, -v) >= 0.0) s = dn;
  }
  return s;
}

// n samples of one stream from x to y; s (the same in every lane) is the stream's state before and after
__device__ __forceinline__ void mark_row(Scratch& sc, MarkState& s, const double* __restrict__ tab, const float* __restrict__ x,
                                         float* __restrict__ y, int n) {
  const int t = threadIdx.x;
  for (int done = 0; done < n;) {
    const int r = (int)(s.pos % kSub);
    const int m = n - done < kRound - r ? n - done : kRound - r;
    const int npc = (r + m + kSub - 1) / kSub;  // <= kThreads
    const float* xr = x + done;
    if (t < npc) {  // phase 1: this lane's sub-block (the first goes on from the open one's sum)
      const int lo = t * kSub - r > 0 ? t * kSub - r : 0;
      const int hi = (t + 1) * kSub - r < m ? (t + 1) * kSub - r : m;
      double e = (t == 0 && r != 0) ? s.e_sub : 0.0;
      for (int j = lo; j < hi; ++j) {
        const double v = (double)xr[j];
        e = e + v * v;
      }
      sc.e[t] = e;
    }
    if (t == 0) {
      sc.g[0] = s.g_prev;
      sc.g[1] = s.g_cur;
    }
    __syncthreads();
    // the complete sub-blocks fall into at most kGains - 1 blocks: lane k folds block k's, in order (the first goes on from
    // the open block's sum)
    const int64_t pos0 = s.pos;
    const int b0 = (int)(pos0 % kBlock);
    const int q0 = (b0 - r) / kSub;    // complete sub-blocks of the open block in front of this round
    const int nfull = (r + m) / kSub;  // sub-blocks this round completes: the first nfull
    const int nseg = nfull ? (q0 + nfull + kPer - 1) / kPer : 0;
    if (t < nseg) {
      const int lo = t == 0 ? 0 : t * kPer - q0;
      const int hi = (t + 1) * kPer - q0 < nfull ? (t + 1) * kPer - q0 : nfull;
      double acc = t == 0 ? s.e_blk : 0.0;
      for (int i = lo; i < hi; ++i) acc = acc + sc.e[i];
      sc.eb[t] = acc;
    }
    __syncthreads();
    int ng = 2;
    for (int k = 0; k < nseg; ++k) {  // every lane: the blocks that complete set the gain of the block behind them
      const double eb = sc.eb[k];
      if ((k + 1) * kPer - q0 > nfull) {  // the open block
        s.e_blk = eb;
        break;
      }
      s.g_prev = s.g_cur;
      s.g_cur = s.a * sqrt_rn(eb / (double)kBlock);
      s.e_blk = 0.0;
      if (t == 0) sc.g[ng] = s.g_cur;  // (ng < kGains: a round completes at most kGains - 2 blocks)
      ++ng;
    }
    s.e_sub = (r + m) % kSub != 0 ? sc.e[npc - 1] : 0.0;
    s.pos = pos0 + m;
    __syncthreads();
    const int o0 = b0 - (kTaps - 1);                               // sc.u[j]'s offset from the start of block pos0 / kBlock
    const int c0 = (int)(pos0 % kPeriod) + kPeriod - (kTaps - 1);  // its chip, before the modulo
    for (int j = t; j < kRound + kTaps - 1; j += kThreads) {       // (zeros behind the round's samples: phase 2 reads them unasked)
      const int rel = o0 + j;
      sc.u[j] = j < m + kTaps - 1 ? sc.g[rel >= 0 ? rel / kBlock + 1 : 0] * tab[kChip + (c0 + j) % kPeriod] : 0.0;
    }
    __syncthreads();
    double w[kPerLane];
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) w[i] = 0.0;
    for (int k = 0; k < kTaps; ++k) {  // phase 2
      const double hk = tab[kH + k];
#pragma unroll
      for (int i = 0; i < kPerLane; ++i) w[i] = w[i] + hk * sc.u[t + i * kThreads + (kTaps - 1) - k];
    }
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int j = t + i * kThreads;
      if (j < m) y[done + j] = (float)((double)xr[j] + w[i]);
    }
    __syncthreads();
    done += m;
  }
}

// grid (max_batch), 256 lanes: workgroup b runs slot b.  States ping-pong between st_in and st_out (the host alternates them);
// slots at or past `batch` only carry their state across, slots that are off write count 0.
__global__ __launch_bounds__(kThreads) void watermark_kernel(const float* __restrict__ pcm, int64_t pcm_stride, int batch, int n_in,
                                                             const int32_t* __restrict__ valid, const double* __restrict__ tab,
                                                             const MarkState* __restrict__ st_in, MarkState* __restrict__ st_out,
                                                             float* __restrict__ out, int64_t out_stride, int32_t* __restrict__ counts) {
  __shared__ Scratch sc;
  const int b = blockIdx.x, t = threadIdx.x;
  MarkState s = st_in[b];
  if (!s.on) {
    if (t == 0) {
      st_out[b].on = 0;
      if (b < batch) counts[b] = 0;
    }
    return;
  }
  if (b < batch) {
    const int n = valid_count(valid, b, n_in);
    mark_row(sc, s, tab, pcm + (int64_t)b * pcm_stride, out + (int64_t)b * out_stride, n);
    if (t == 0) counts[b] = n;
  }
  if (t == 0) st_out[b] = s;
}

// A whole utterance from position 0, one workgroup, no slot
__global__ __launch_bounds__(kThreads) void watermark_embed_kernel(const float* __restrict__ x, int n, double gain,
                                                                   const double* __restrict__ tab, float* __restrict__ y) {
  __shared__ Scratch sc;
  MarkState s = {0.0, 0.0, 0.0, 0.0, gain, 0, 1, 0};
  mark_row(sc, s, tab, x, y, n);
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  double gain[kResetMax];
};

// lane i: slot args.slot[i] starts a stream (or is switched off) in both state halves
__global__ void watermark_reset_kernel(ResetArgs a, MarkState* st0, MarkState* st1) {
  const int i = threadIdx.x;
  if (i >= a.n) return;
  const MarkState s = {0.0, 0.0, 0.0, 0.0, a.gain[i], 0, a.gain[i] > 0.0 ? 1 : 0, 0};
  st0[a.slot[i]] = s;
  st1[a.slot[i]] = s;
}

}  // namespace

struct SmolttsWatermark {
  int B;
  PingPong<MarkState> st;
  double* tab;
};

static size_t carve(SmolttsWatermark* r, char* base) {
  Carver cv{base, 0};
  r->st.carve(cv, r->B);
  r->tab = cv.take<double>(kTab);
  return cv.off;
}

static bool gain_ok(double g) {
  return g >= 0.0 && g <= 1.0;  // (a NaN fails)
}

extern "C" {

size_t smoltts_watermark_bytes(int32_t max_batch) {
  return stage_bytes<SmolttsWatermark>(max_batch);
}

int32_t smoltts_watermark_table_doubles(void) {
  return kTab;
}

int smoltts_watermark_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, const double* tables_host, int32_t n_tables,
                             SmolttsWatermark** out) {
  ST_REQUIRE(tables_host && n_tables == kTab, SMOLTTS_E_INVALID, "watermark_create: tables of %d doubles, %d expected", n_tables, kTab);
  for (int i = 0; i < kPeriod; ++i)
    ST_REQUIRE(tables_host[kChip + i] == 1.0 || tables_host[kChip + i] == -1.0, SMOLTTS_E_INVALID, "watermark_create: chip %d is not +-1", i);
  SmolttsWatermark* r = nullptr;
  size_t need = 0;
  ST_TRY(stage_create("watermark_create", slab_dev, slab_bytes, max_batch, out, &r, &need));
  if (hipMemset(slab_dev, 0, need) != hipSuccess ||  // every slot off
      hipMemcpy(r->tab, tables_host, kTab * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    delete r;
    set_error("watermark_create: clearing the slab or uploading the tables failed");
    return SMOLTTS_E_HIP;
  }
  *out = r;
  return SMOLTTS_OK;
}

void smoltts_watermark_destroy(SmolttsWatermark* r) {
  delete r;
}

int smoltts_watermark_reset_slots(SmolttsWatermark* r, const int32_t* slots_host, const double* gain_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(r && slots_host && gain_host && n_slots > 0, SMOLTTS_E_INVALID, "watermark_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    ST_REQUIRE(gain_ok(gain_host[k]), SMOLTTS_E_INVALID, "watermark_reset_slots: gain %g outside [0, 1]", gain_host[k]);
    a.gain[i] = gain_host[k];
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("watermark_reset_slots", r->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    hipLaunchKernelGGL(watermark_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, r->st.half[0], r->st.half[1]);
  });
}

int smoltts_watermark_chunk(SmolttsWatermark* r, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                            const int32_t* valid_in_dev, float* out_dev, int64_t out_stride, int32_t* counts_dev, void* stream) {
  ST_TRY(check_chunk("watermark_chunk", r, pcm_dev && out_dev && counts_dev, batch, true, n_in, pcm_stride));
  ST_REQUIRE(out_stride >= n_in, SMOLTTS_E_CAPACITY, "watermark_chunk: out_stride %lld < %d samples", (long long)out_stride, n_in);
  hipLaunchKernelGGL(watermark_kernel, dim3(r->B), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, pcm_stride, batch, n_in,
                     valid_in_dev, r->tab, r->st.cur(), r->st.next(), out_dev, out_stride, counts_dev);
  ST_CHECK_HIP(hipGetLastError());
  r->st.flip();
  return SMOLTTS_OK;
}

int smoltts_watermark_embed(SmolttsWatermark* r, const float* pcm_dev, int32_t n, double gain, float* out_dev, void* stream) {
  ST_REQUIRE(r && pcm_dev && out_dev, SMOLTTS_E_INVALID, "watermark_embed: null argument");
  ST_REQUIRE(n >= 0 && n <= kEmbedMax, SMOLTTS_E_INVALID, "watermark_embed: n %d (0..%d)", n, kEmbedMax);
  ST_REQUIRE(gain_ok(gain), SMOLTTS_E_INVALID, "watermark_embed: gain %g outside [0, 1]", gain);
  if (n == 0) return SMOLTTS_OK;
  hipLaunchKernelGGL(watermark_embed_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, n, gain, r->tab, out_dev);
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

int smoltts_watermark_slot_state(SmolttsWatermark* r, int32_t slot, int64_t* ints_host, double* values_host, void* stream) {
  ST_REQUIRE(r && ints_host && values_host && slot >= 0 && slot < r->B, SMOLTTS_E_INVALID, "watermark_slot_state: bad argument");
  MarkState s;
  hipError_t e = hipMemcpyAsync(&s, r->st.cur() + slot, sizeof(MarkState), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  ST_CHECK_HIP(e);
  ints_host[0] = s.pos; ints_host[1] = s.on;
  values_host[0] = s.e_sub; values_host[1] = s.e_blk; values_host[2] = s.g_cur; values_host[3] = s.g_prev; values_host[4] = s.a;
  return SMOLTTS_OK;
}

}  // extern "C"

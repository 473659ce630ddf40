// Streamed output formats: the codec's 24 kHz fp32 PCM -> 16-bit PCM at 8 / 16 / 22.05 / 44.1 / 48 kHz or 8 kHz G.711 mu-law,
// chunk by chunk, in one launch per pass over every slot (include/smoltts_hip.h, "Streamed output formats").
//
// Resampling is scipy.signal.resample_poly(x, up, down) with its default filter: half_len = 10 max(up, down),
// h = firwin(2 half_len + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up, zero padding at both ends, i.e.
//   y[m] = sum_j x[j] h[half_len + m down - j up].
// After N inputs an output m is final when half_len + m down <= up N - 1; each call emits the outputs that became final and,
// behind them, the tail up to ceil(N up / down) computed as if the input ended at N.  Every output is summed over ascending j
// in fp64 (fp32 taps and sums put ~0.15 % of the int16 samples one code off scipy's float64 result), so the bytes do not
// depend on where the chunk boundaries fall.
#include <math.h>

#include "stage.h"

using namespace smoltts;

namespace {

constexpr int kHist = 64;       // input samples carried from call to call (2 half_len / up <= 60 for every rate)
constexpr int kTile = 256;      // outputs per workgroup, one per lane
constexpr int kWindow = 1024;   // LDS window: ((kTile - 1) down + 2 half_len) / up + 2 <= 827 floats
constexpr int kRates = 5;

struct RateSpec { int rate, up, down; };
constexpr RateSpec kSpecs[kRates] = {{8000, 1, 3}, {16000, 2, 3}, {22050, 147, 160}, {44100, 147, 80}, {48000, 2, 1}};

struct SlotCfg {   // device copy, per slot
  int32_t up, down, half_len, enc;
  int32_t tap_off;  // element offset of the rate's polyphase table
  int32_t taps_per_phase;
  int32_t pad[2];
};

struct SlotState {  // one half of the ping-pong pair, per slot
  int64_t n_in, n_out;  // inputs received, final outputs emitted
  float hist[kHist];    // inputs [n_in - 64, n_in) (zeros before the stream's start)
};

int spec_index(int rate) {
  for (int i = 0; i < kRates; ++i)
    if (kSpecs[i].rate == rate) return i;
  return -1;
}
int half_len_of(const RateSpec& s) { return 10 * (s.up > s.down ? s.up : s.down); }
int taps_per_phase(const RateSpec& s) { return 2 * half_len_of(s) / s.up + 1; }

double bessel_i0(double x) {  // power series: every term positive, converges to full double precision for |x| <= 5
  double sum = 1.0, term = 1.0;
  const double q = 0.25 * x * x;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

// scipy.signal.firwin(n, cutoff, window=("kaiser", beta)) * gain: windowed sinc, scaled to unit DC gain, times gain
void design(const RateSpec& s, double* h) {
  const int half = half_len_of(s), n = 2 * half + 1;
  const double cutoff = 1.0 / (double)(s.up > s.down ? s.up : s.down), beta = 5.0, alpha = 0.5 * (n - 1);
  const double i0b = bessel_i0(beta);
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const double m = (double)i - alpha, x = cutoff * m;
    const double sinc = x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x);
    const double r = m / alpha;
    const double w = bessel_i0(beta * sqrt(1.0 - r * r)) / i0b;
    h[i] = cutoff * sinc * w;
    sum += h[i];
  }
  for (int i = 0; i < n; ++i) h[i] = h[i] / sum * (double)s.up;
}

__device__ __forceinline__ int16_t to_s16(double y) {
  y = fmin(fmax(y, -1.0), 1.0);
  return (int16_t)__double2int_rn(y * 32767.0);
}

__device__ __forceinline__ uint8_t s16_to_ulaw(int s) {  // G.711 mu-law of a 16-bit sample (Sun's linear2ulaw, no 14-bit cut)
  const int sign = s < 0 ? 0x80 : 0;
  int mag = s < 0 ? -s : s;
  mag = (mag > 32635 ? 32635 : mag) + 0x84;
  const int seg = (31 - __clz(mag)) - 7;
  const int mant = (mag >> (seg + 3)) & 0xF;
  return (uint8_t)~(sign | (seg << 4) | mant);
}

// final outputs after n inputs
__device__ __forceinline__ int64_t n_final(int64_t n, int up, int down, int half) {
  const int64_t t = (int64_t)up * n - 1 - half;
  return t < 0 ? 0 : t / down + 1;
}

// grid (tiles, max_batch), 256 lanes: workgroup (t, b) computes outputs [t*256, t*256 + 256) of slot b's call; workgroup (0, b)
// also writes the slot's counts and its next state.  States ping-pong between st_in and st_out (the host alternates them), so
// no workgroup reads what another one writes in the same launch; slots at or past `batch` only carry their state across.
__global__ __launch_bounds__(kTile) void resample_kernel(const float* __restrict__ pcm, int64_t pcm_stride, int batch, int n_in,
                                                         const int32_t* __restrict__ valid, const SlotCfg* __restrict__ cfgs,
                                                         const double* __restrict__ taps, const SlotState* __restrict__ st_in,
                                                         SlotState* __restrict__ st_out, uint8_t* __restrict__ out, int64_t out_stride,
                                                         int32_t* __restrict__ counts) {
  __shared__ float win[kWindow];
  const int b = blockIdx.y, tid = threadIdx.x;
  const SlotCfg c = cfgs[b];
  const SlotState* si = st_in + b;
  const int64_t N0 = si->n_in, M0 = si->n_out;
  int n = 0;
  if (b < batch && c.enc != SMOLTTS_RESAMPLE_OFF) {
    n = valid_count(valid, b, n_in);
  }
  const int64_t N1 = N0 + n;
  const float* x = pcm + (int64_t)(b < batch ? b : 0) * pcm_stride;
  const bool on = b < batch && c.enc != SMOLTTS_RESAMPLE_OFF;
  const int64_t M1 = on ? n_final(N1, c.up, c.down, c.half_len) : M0;
  const int64_t end = on ? ((int64_t)c.up * N1 + c.down - 1) / c.down : M0;  // ceil(N1 up / down): the stream's length so far
  if (blockIdx.x == 0) {
    SlotState* so = st_out + b;
    if (tid < kHist) {
      const int64_t j = N1 - kHist + tid;
      float v = 0.0f;
      if (j >= N0) v = x[j - N0];
      else if (j >= N0 - kHist && j >= 0) v = si->hist[j - (N0 - kHist)];
      so->hist[tid] = v;
    }
    if (tid == 0) {
      so->n_in = N1;
      so->n_out = M1;
      if (b < batch) {
        counts[2 * b] = (int32_t)(M1 - M0);
        counts[2 * b + 1] = (int32_t)(end > M1 ? end - M1 : 0);
      }
    }
  }
  if (!on) return;
  const int64_t ma = M0 + (int64_t)blockIdx.x * kTile;
  if (ma >= end) return;
  const int64_t mb = ma + kTile < end ? ma + kTile : end;
  const int up = c.up, down = c.down, half = c.half_len;
  // inputs this tile reads: j in [ceil((ma down - half) / up), floor(((mb - 1) down + half) / up)], inside [max(0, N0 - 64), N1)
  int64_t jlo_num = ma * down - half;
  int64_t j_lo = jlo_num <= 0 ? -((-jlo_num) / up) : (jlo_num + up - 1) / up;
  const int64_t j_min = N0 - kHist > 0 ? N0 - kHist : 0;
  if (j_lo < j_min) j_lo = j_min;
  int64_t j_hi = ((mb - 1) * down + half) / up;
  if (j_hi > N1 - 1) j_hi = N1 - 1;
  int w = (int)(j_hi - j_lo + 1);
  w = w < 0 ? 0 : (w > kWindow ? kWindow : w);
  for (int i = tid; i < w; i += kTile) {
    const int64_t j = j_lo + i;
    win[i] = j >= N0 ? x[j - N0] : si->hist[j - (N0 - kHist)];
  }
  __syncthreads();
  const int64_t m = ma + tid;
  if (m >= mb) return;
  // taps of output m: h[k0 - j up] for j ascending, k0 = half + m down; in the rate's polyphase table (phase r = k0 mod up,
  // row i = k0 div up - j holds h[r + i up]) that is one row read backwards
  const int64_t k0 = half + m * down;
  const int64_t q = k0 / up;
  const int r = (int)(k0 - q * up);
  const int imax = (2 * half - r) / up;
  int64_t jl = q - imax, jh = q;
  if (jl < j_lo) jl = j_lo;
  if (jh > j_lo + w - 1) jh = j_lo + w - 1;
  const double* hp = taps + c.tap_off + (int64_t)r * c.taps_per_phase;
  double acc = 0.0;
  for (int64_t j = jl; j <= jh; ++j) acc = fma((double)win[j - j_lo], hp[q - j], acc);
  const int64_t o = m - M0;
  uint8_t* row = out + (int64_t)b * out_stride;
  const int16_t s = to_s16(acc);
  if (c.enc == SMOLTTS_RESAMPLE_S16) {
    if (2 * o + 2 <= out_stride) {
      row[2 * o] = (uint8_t)(s & 0xff);
      row[2 * o + 1] = (uint8_t)((uint16_t)s >> 8);
    }
  } else if (o + 1 <= out_stride) {
    row[o] = s16_to_ulaw(s);
  }
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  SlotCfg cfg[kResetMax];
};

// workgroup i: slot args.slot[i] gets its new configuration and an empty stream in both state halves
__global__ __launch_bounds__(64) void resample_reset_kernel(ResetArgs a, SlotCfg* cfgs, SlotState* st0, SlotState* st1) {
  const int i = blockIdx.x, t = threadIdx.x;
  if (i >= a.n) return;
  const int b = a.slot[i];
  st0[b].hist[t] = 0.0f;
  st1[b].hist[t] = 0.0f;
  if (t == 0) {
    cfgs[b] = a.cfg[i];
    st0[b].n_in = st0[b].n_out = 0;
    st1[b].n_in = st1[b].n_out = 0;
  }
}

size_t taps_count() {
  size_t n = 0;
  for (const RateSpec& s : kSpecs) n += (size_t)s.up * taps_per_phase(s);
  return n;
}

}  // namespace

struct SmolttsResampler {
  int B;
  SlotCfg* cfg_dev;
  PingPong<SlotState> st;
  double* taps_dev;
  int tap_off[kRates];
  SlotCfg* cfg_host;  // mirror of cfg_dev (sizes the grid)
};

// the slab: the constant tap tables, then what create clears (every slot off, every stream empty)
static size_t carve(SmolttsResampler* r, char* base) {
  Carver cv{base, 0};
  r->taps_dev = cv.take<double>(taps_count());
  r->cfg_dev = cv.take<SlotCfg>(r->B);
  r->st.carve(cv, r->B);
  return cv.off;
}

extern "C" {

int smoltts_resample_design(int32_t out_rate, double* taps, int32_t cap, int32_t* up, int32_t* down, int32_t* half_len) {
  const int i = spec_index(out_rate);
  ST_REQUIRE(i >= 0, SMOLTTS_E_INVALID, "resample_design: unsupported output rate %d (8000, 16000, 22050, 44100, 48000)", out_rate);
  const RateSpec& s = kSpecs[i];
  if (up) *up = s.up;
  if (down) *down = s.down;
  if (half_len) *half_len = half_len_of(s);
  if (taps) {
    const int n = 2 * half_len_of(s) + 1;
    ST_REQUIRE(cap >= n, SMOLTTS_E_CAPACITY, "resample_design: %d taps need room, cap is %d", n, cap);
    design(s, taps);
  }
  return SMOLTTS_OK;
}

size_t smoltts_resampler_bytes(int32_t max_batch) {
  return stage_bytes<SmolttsResampler>(max_batch);
}

size_t smoltts_resampler_out_bytes(int32_t n_in) {
  if (n_in < 0) return 0;
  size_t most = 0;
  for (const RateSpec& s : kSpecs) {
    const size_t n = ((size_t)n_in * s.up + half_len_of(s)) / s.down + 2;  // outputs one call can emit, final and tail
    most = n > most ? n : most;
  }
  return 2 * most;  // s16; mu-law takes half
}

int smoltts_resampler_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsResampler** out) {
  SmolttsResampler* r = nullptr;
  size_t need = 0;
  ST_TRY(stage_create("resampler_create", slab_dev, slab_bytes, max_batch, out, &r, &need));
  r->cfg_host = static_cast<SlotCfg*>(calloc((size_t)max_batch, sizeof(SlotCfg)));
  // polyphase tables: phase ph of a rate holds h[ph], h[ph + up], h[ph + 2 up], ... (zero past the filter's end)
  double* host = static_cast<double*>(calloc(taps_count(), sizeof(double)));
  double* h = static_cast<double*>(malloc(sizeof(double) * (2 * 1600 + 1)));
  if (!r->cfg_host || !host || !h) {
    free(r->cfg_host); free(host); free(h);
    delete r;
    set_error("resampler_create: out of host memory");
    return SMOLTTS_E_INVALID;
  }
  size_t off = 0;
  for (int i = 0; i < kRates; ++i) {
    const RateSpec& s = kSpecs[i];
    const int n = 2 * half_len_of(s) + 1, L = taps_per_phase(s);
    design(s, h);
    r->tap_off[i] = (int)off;
    for (int ph = 0; ph < s.up; ++ph)
      for (int k = 0; k < L; ++k)
        if (ph + k * s.up < n) host[off + (size_t)ph * L + k] = h[ph + k * s.up];
    off += (size_t)s.up * L;
  }
  const bool ok = hipMemcpy(r->taps_dev, host, taps_count() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(r->cfg_dev, 0, need - ((char*)r->cfg_dev - (char*)slab_dev)) == hipSuccess;  // every slot off, every stream empty
  free(host);
  free(h);
  if (!ok) {
    free(r->cfg_host);
    delete r;
    set_error("resampler_create: hipMemcpy / hipMemset failed");
    return SMOLTTS_E_HIP;
  }
  *out = r;
  return SMOLTTS_OK;
}

void smoltts_resampler_destroy(SmolttsResampler* r) {
  if (!r) return;
  free(r->cfg_host);
  delete r;
}

int smoltts_resampler_reset_slots(SmolttsResampler* r, const int32_t* slots_host, const int32_t* out_rates_host,
                                  const int32_t* encodings_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(r && slots_host && out_rates_host && encodings_host && n_slots > 0, SMOLTTS_E_INVALID, "resampler_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    const int enc = encodings_host[k], rate = out_rates_host[k];
    ST_REQUIRE(enc == SMOLTTS_RESAMPLE_OFF || enc == SMOLTTS_RESAMPLE_S16 || enc == SMOLTTS_RESAMPLE_ULAW, SMOLTTS_E_INVALID,
               "resampler_reset_slots: unknown encoding %d", enc);
    SlotCfg& c = a.cfg[i];  // (zeroed)
    c.enc = enc;
    if (enc != SMOLTTS_RESAMPLE_OFF) {
      const int s = spec_index(rate);
      ST_REQUIRE(s >= 0, SMOLTTS_E_INVALID, "resampler_reset_slots: unsupported output rate %d", rate);
      ST_REQUIRE(enc != SMOLTTS_RESAMPLE_ULAW || rate == 8000, SMOLTTS_E_INVALID, "resampler_reset_slots: mu-law is 8 kHz only");
      c.up = kSpecs[s].up;
      c.down = kSpecs[s].down;
      c.half_len = half_len_of(kSpecs[s]);
      c.tap_off = r->tap_off[s];
      c.taps_per_phase = taps_per_phase(kSpecs[s]);
    }
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("resampler_reset_slots", r->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    for (int i = 0; i < a.n; ++i) r->cfg_host[a.slot[i]] = a.cfg[i];
    hipLaunchKernelGGL(resample_reset_kernel, dim3(a.n), dim3(kHist), 0, (hipStream_t)stream, a, r->cfg_dev, r->st.half[0], r->st.half[1]);
  });
}

int smoltts_resample_chunk(SmolttsResampler* r, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                           const int32_t* valid_in_dev, void* out_dev, int64_t out_stride, int32_t* counts_dev, void* stream) {
  ST_TRY(check_chunk("resample_chunk", r, pcm_dev && out_dev && counts_dev, batch, true, n_in, pcm_stride));
  // the grid covers the most outputs any listed slot can emit in this call, at its own rate and encoding
  int64_t most = 0, row = 0;
  for (int b = 0; b < batch; ++b) {
    const SlotCfg& c = r->cfg_host[b];
    if (c.enc == SMOLTTS_RESAMPLE_OFF) continue;
    const int64_t n = ((int64_t)n_in * c.up + c.half_len) / c.down + 2;
    most = n > most ? n : most;
    const int64_t bytes = n * (c.enc == SMOLTTS_RESAMPLE_S16 ? 2 : 1);
    row = bytes > row ? bytes : row;
  }
  ST_REQUIRE(out_stride >= row, SMOLTTS_E_CAPACITY, "resample_chunk: out_stride %lld < %lld bytes", (long long)out_stride, (long long)row);
  const int tiles = most > 0 ? (int)((most + kTile - 1) / kTile) : 1;
  hipLaunchKernelGGL(resample_kernel, dim3(tiles, r->B), dim3(kTile), 0, (hipStream_t)stream, pcm_dev, pcm_stride, batch, n_in,
                     valid_in_dev, r->cfg_dev, r->taps_dev, r->st.cur(), r->st.next(), (uint8_t*)out_dev, out_stride, counts_dev);
  ST_CHECK_HIP(hipGetLastError());
  r->st.flip();
  return SMOLTTS_OK;
}

}  // extern "C"

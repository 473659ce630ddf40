// Loudness normalisation of the codec's 24 kHz fp32 PCM by the ITU-R BS.1770-4 meter, in one launch per pass over every slot
// (include/smoltts_hip.h, "Loudness"; the numpy model, which this file reproduces bit for bit, is
// smoltts_amd/loudness.py).
//
// The K-weighting filter (two biquads, fp64) does not run as one chain per slot: the row is cut on the stream's own grid of
// kSub samples, lane i filters piece i from a zero state, one lane carries the true states from piece to piece with the
// kSub-step transition matrix, and every lane filters its piece again from its true start state, summing y^2.  A call that ends
// inside a sub-block keeps both passes' running states, so the numbers do not depend on how calls cut the stream.  The walk over
// the pieces then closes hops (kHop samples), puts each new block's mean square into the slot's ring, and after every hop sets
// the knot behind the next one: the gated power of the ring against the squared-gain table, at most kSlew steps from the last
// knot, capped by the running peak.  The gain of a sample is linear between its hop's two knots.
//
// Every fp64 operation is a single rounded multiply, add or divide in the model's order (no contraction in this file), and the
// sums over blocks have a fixed shape: lane t adds elements t, t + 256, ... in order, the lanes are summed as a tree of
// neighbours.
#include "stage.h"

#pragma clang fp contract(off)

using namespace smoltts;

namespace {

constexpr int kSub = 240, kHop = 2400, kPer = kHop / kSub;
constexpr int kRing = 512;
constexpr int kKMax = 1280, kKnots = 2 * kKMax + 1, kSlew = 32;
constexpr int kThreads = 256;  // 4 waves; also the width of the summation tree
constexpr int kPerLane = (kKnots + kThreads - 1) / kThreads;  // knots of the gain tables a lane compares
constexpr int kCoef = 0, kTrans = 10, kGate = 26, kCeil = 27, kGain = 28, kGain2 = kGain + kKnots, kTab = kGain2 + kKnots;
constexpr double kBlockLen = 4.0 * kHop, kRel = 0.1;
constexpr int kMeasureMax = 1 << 26;
constexpr int kAhead = 16;  // samples a lane loads ahead of its filter chain (its loads are 960 bytes from its neighbours')

struct FilterState {
  double s_start[4];  // the true state at the open sub-block's start
  double s_run[4];    // the state at pos of the pass from s_start
  double z_run[4];    // the state at pos of the pass from zero
  double e_sub;       // sum of y^2 over the open sub-block so far
};

struct LoudState {  // one half of the ping-pong pair, per slot
  FilterState f;
  double e_hop;      // energy of the open hop's complete sub-blocks
  double hops[3];    // the last complete hops' energies, oldest first
  double ptarget;    // the target as a mean square
  double ring[kRing];  // block j's mean square at j % kRing
  int64_t pos;       // samples consumed
  float peak;        // max |x| so far
  int32_t ka, kb;    // the knots at both ends of the open hop
  int32_t on;
};
static_assert(sizeof(LoudState) % 8 == 0, "loudness: state is copied as 8-byte words");

struct Scratch {  // per workgroup, in LDS
  double zend[kThreads][4];
  double start[kThreads + 1][4];
  double e[kThreads];
  double ga[kThreads], d[kThreads];
  float pk[kThreads];
  double red[4];
  int redn[4];
};

// one sample through both biquads (c: shelf b0 b1 b2 a1 a2, high pass b0 b1 b2 a1 a2)
__device__ __forceinline__ double step(const double* c, double x, double* s) {
  const double y1 = c[0] * x + s[0];
  const double n1 = (c[1] * x - c[3] * y1) + s[1];
  const double n2 = c[2] * x - c[4] * y1;
  const double y2 = c[5] * y1 + s[2];
  const double n3 = (c[6] * y1 - c[8] * y2) + s[3];
  const double n4 = c[7] * y1 - c[9] * y2;
  s[0] = n1; s[1] = n2; s[2] = n3; s[3] = n4;
  return y2;
}

// sum of (v, n) over the workgroup in the fixed tree order; every lane gets the result
__device__ __forceinline__ void tree_sum(Scratch& sc, double& v, int& n) {
  for (int off = 1; off < 64; off <<= 1) {
    v = v + __shfl_xor(v, off, 64);
    n += __shfl_xor(n, off, 64);
  }
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) {
    sc.red[t >> 6] = v;
    sc.redn[t >> 6] = n;
  }
  __syncthreads();
  v = (sc.red[0] + sc.red[1]) + (sc.red[2] + sc.red[3]);
  n = (sc.redn[0] + sc.redn[1]) + (sc.redn[2] + sc.redn[3]);
}

// the mean power of the n blocks z(j) that pass both gates (0: none passes the absolute gate); n1: how many pass it
template <typename Z>
__device__ __forceinline__ double gated_power(Scratch& sc, Z z, int n, double gate_abs, int& n1, int& n2) {
  const int t = threadIdx.x;
  double s = 0.0;
  int c = 0;
  for (int j = t; j < n; j += kThreads) {
    const double v = z(j);
    const bool a = v > gate_abs;
    s = s + (a ? v : 0.0);
    c += a;
  }
  tree_sum(sc, s, c);
  n1 = c;
  n2 = 0;
  if (c == 0) return 0.0;
  const double rel = (s / (double)c) * kRel;
  s = 0.0;
  c = 0;
  for (int j = t; j < n; j += kThreads) {
    const double v = z(j);
    const bool a = v > gate_abs && v > rel;
    s = s + (a ? v : 0.0);
    c += a;
  }
  tree_sum(sc, s, c);
  n2 = c;
  return s / (double)c;
}

// One round of the filter: m samples at x, the first r samples into a sub-block (pos % kSub), in npc <= kThreads pieces.
// Leaves every piece's energy and peak in sc.e / sc.pk and f at the round's end.
__device__ __forceinline__ void filter_round(Scratch& sc, FilterState& f, const double* __restrict__ tab, const float* __restrict__ x,
                                             int r, int m, int npc) {
  const int t = threadIdx.x;
  double c[10];
  for (int k = 0; k < 10; ++k) c[k] = tab[kCoef + k];
  const int lo = t * kSub - r > 0 ? t * kSub - r : 0;
  const int hi = (t + 1) * kSub - r < m ? (t + 1) * kSub - r : m;
  const bool mine = t < npc, open = t == 0 && r != 0;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  if (mine) {  // pass 1: from zero (piece 0 goes on from the open sub-block's pass)
    if (open) for (int k = 0; k < 4; ++k) z[k] = f.z_run[k];
    float pk = 0.0f;
    int j = lo;
    for (; j + kAhead <= hi; j += kAhead) {  // the loads of kAhead samples go out before the chain needs the first
      float v[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) v[k] = x[j + k];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        pk = fmaxf(pk, fabsf(v[k]));
        step(c, (double)v[k], z);
      }
    }
    for (; j < hi; ++j) {
      const float v = x[j];
      pk = fmaxf(pk, fabsf(v));
      step(c, (double)v, z);
    }
    for (int k = 0; k < 4; ++k) sc.zend[t][k] = z[k];
    sc.pk[t] = pk;
  }
  __syncthreads();
  if (t == 0) {  // the true start states, piece by piece
    double M[16], s[4];
    for (int k = 0; k < 16; ++k) M[k] = tab[kTrans + k];
    for (int k = 0; k < 4; ++k) sc.start[0][k] = s[k] = f.s_start[k];
    const int ndone = (r + m) / kSub;  // pieces that end on the grid: the first ndone
    for (int i = 0; i < ndone; ++i) {
      double nx[4];
      for (int k = 0; k < 4; ++k)
        nx[k] = (((M[4 * k] * s[0] + M[4 * k + 1] * s[1]) + M[4 * k + 2] * s[2]) + M[4 * k + 3] * s[3]) + sc.zend[i][k];
      for (int k = 0; k < 4; ++k) sc.start[i + 1][k] = s[k] = nx[k];
    }
  }
  __syncthreads();
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  double e = 0.0;
  if (mine) {  // pass 2: from the true state
    for (int k = 0; k < 4; ++k) s[k] = open ? f.s_run[k] : sc.start[t][k];
    if (open) e = f.e_sub;
    int j = lo;
    for (; j + kAhead <= hi; j += kAhead) {
      float v[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) v[k] = x[j + k];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        const double y = step(c, (double)v[k], s);
        e = e + y * y;
      }
    }
    for (; j < hi; ++j) {
      const double y = step(c, (double)x[j], s);
      e = e + y * y;
    }
    sc.e[t] = e;
  }
  __syncthreads();  // (f is read above by lane 0)
  if (t == npc - 1) {
    const bool done = (r + m) % kSub == 0;
    for (int k = 0; k < 4; ++k) {
      f.s_start[k] = done ? sc.start[npc][k] : sc.start[npc - 1][k];
      f.s_run[k] = done ? sc.start[npc][k] : s[k];
      f.z_run[k] = done ? 0.0 : z[k];
    }
    f.e_sub = done ? 0.0 : e;
  }
  __syncthreads();
}

// grid (max_batch), 256 lanes: workgroup b runs slot b.  States ping-pong between st_in and st_out (the host alternates them);
// slots at or past `batch` only carry their state across, slots that are off write count 0.
__global__ __launch_bounds__(kThreads) void loudness_kernel(const float* __restrict__ pcm, int64_t pcm_stride, int batch, int n_in,
                                                            const int32_t* __restrict__ valid, const double* __restrict__ tab,
                                                            const LoudState* __restrict__ st_in, LoudState* __restrict__ st_out,
                                                            float* __restrict__ out, int64_t out_stride, int32_t* __restrict__ counts) {
  __shared__ Scratch sc;
  __shared__ LoudState st;
  const int b = blockIdx.x, t = threadIdx.x;
  const LoudState* si = st_in + b;
  LoudState* so = st_out + b;
  if (!si->on) {
    if (t == 0) {
      so->on = 0;
      if (b < batch) counts[b] = 0;
    }
    return;
  }
  constexpr int kWords = sizeof(LoudState) / 8;
  if (b >= batch) {  // not in this call
    for (int i = t; i < kWords; i += kThreads) ((uint64_t*)so)[i] = ((const uint64_t*)si)[i];
    return;
  }
  for (int i = t; i < kWords; i += kThreads) ((uint64_t*)&st)[i] = ((const uint64_t*)si)[i];
  const int n = valid_count(valid, b, n_in);
  const float* x = pcm + (int64_t)b * pcm_stride;
  float* y = out + (int64_t)b * out_stride;
  const double gate_abs = tab[kGate], ceiling = tab[kCeil];
  double g1[kPerLane], g2[kPerLane];  // this lane's share of the gain tables
  for (int k = 0; k < kPerLane; ++k) {
    const int i = t + k * kThreads;
    g1[k] = i < kKnots ? tab[kGain + i] : 0.0;
    g2[k] = i < kKnots ? tab[kGain2 + i] : 0.0;
  }
  __syncthreads();
  // the walk's running values, the same in every lane
  int64_t pos = st.pos;
  int ka = st.ka, kb = st.kb;
  float peak = st.peak;
  double e_hop = st.e_hop, h0 = st.hops[0], h1 = st.hops[1], h2 = st.hops[2];
  const double ptarget = st.ptarget;
  for (int done = 0; done < n;) {
    const int r = (int)(pos % kSub);
    const int m = n - done < kThreads * kSub - r ? n - done : kThreads * kSub - r;
    const int npc = (r + m + kSub - 1) / kSub;
    filter_round(sc, st.f, tab, x + done, r, m, npc);
    const int64_t pos0 = pos;
    for (int i = 0; i < npc; ++i) {
      if (t == 0) {
        const double ga = tab[kGain + ka + kKMax];
        sc.ga[i] = ga;
        sc.d[i] = (tab[kGain + kb + kKMax] - ga) / (double)kHop;
      }
      peak = fmaxf(peak, sc.pk[i]);
      const int end = (i + 1) * kSub - r;
      pos = pos0 + (end < m ? end : m);
      if (end > m) break;  // the open sub-block: its energy stays in st.f
      e_hop = e_hop + sc.e[i];
      if (pos % kHop != 0) continue;
      // a hop is complete: its block enters the ring, and the knot behind the next hop is set
      const int64_t nh = pos / kHop;
      if (nh >= 4) {
        __syncthreads();  // (the ring's readers of the last hop are through)
        if (t == 0) st.ring[(nh - 4) % kRing] = (((h0 + h1) + h2) + e_hop) / kBlockLen;
        __syncthreads();
      }
      h0 = h1; h1 = h2; h2 = e_hop;
      e_hop = 0.0;
      int n1, n2;
      const double p = gated_power(sc, [&](int j) { return st.ring[j]; }, kRing, gate_abs, n1, n2);
      // knots whose squared gain keeps p at or under the target, knots whose gain keeps the peak at or under the ceiling
      double cw = 0.0;
      int cnt = 0;
      const double pk = (double)peak;
      for (int k = 0; k < kPerLane; ++k) {
        const bool in = t + k * kThreads < kKnots;
        cnt += (in && g2[k] * p <= ptarget) ? 1 : 0;
        cnt += (in && g1[k] * pk <= ceiling) ? 0x10000 : 0;
      }
      tree_sum(sc, cw, cnt);
      int nw = kb;
      if (n1) {
        int want = (cnt & 0xffff) - 1 - kKMax;
        want = want < -kKMax ? -kKMax : want;
        const int mv = want - kb;
        nw = kb + (mv < -kSlew ? -kSlew : (mv > kSlew ? kSlew : mv));
      }
      int cap = (cnt >> 16) - 1 - kKMax;
      cap = cap < -kKMax ? -kKMax : cap;
      nw = nw < cap ? nw : cap;
      ka = kb;
      kb = nw;
    }
    __syncthreads();
    for (int j = t; j < m; j += kThreads) {
      const int i = (j + r) / kSub;
      const int o = (int)((pos0 + j) % kHop);
      const double g = sc.ga[i] + (double)o * sc.d[i];
      y[done + j] = (float)((double)x[done + j] * g);
    }
    __syncthreads();
    done += m;
  }
  if (t == 0) {
    st.pos = pos; st.ka = ka; st.kb = kb; st.peak = peak;
    st.e_hop = e_hop; st.hops[0] = h0; st.hops[1] = h1; st.hops[2] = h2;
    counts[b] = n;
  }
  __syncthreads();
  for (int i = t; i < kWords; i += kThreads) ((uint64_t*)so)[i] = ((const uint64_t*)&st)[i];
}

// A whole utterance, one workgroup: every complete hop's energy to ws[h], then res = {gated mean power (0: nothing measured),
// peak, blocks past the absolute gate, blocks past both}.
__global__ __launch_bounds__(kThreads) void loudness_measure_kernel(const float* __restrict__ x, int n, const double* __restrict__ tab,
                                                                    double* __restrict__ ws, double* __restrict__ res) {
  __shared__ Scratch sc;
  __shared__ FilterState f;
  const int t = threadIdx.x;
  if (t < (int)(sizeof(FilterState) / 8)) ((double*)&f)[t] = 0.0;
  __syncthreads();
  float peak = 0.0f;
  double e_hop = 0.0;
  int sub = 0;  // complete sub-blocks so far
  for (int done = 0; done < n;) {
    const int m = n - done < kThreads * kSub ? n - done : kThreads * kSub;  // (rounds start on the grid)
    const int npc = (m + kSub - 1) / kSub;
    filter_round(sc, f, tab, x + done, 0, m, npc);
    for (int i = 0; i < npc; ++i) {
      peak = fmaxf(peak, sc.pk[i]);
      if ((i + 1) * kSub > m) break;
      e_hop = e_hop + sc.e[i];
      if (++sub % kPer == 0) {
        if (t == 0) ws[sub / kPer - 1] = e_hop;
        e_hop = 0.0;
      }
    }
    __syncthreads();
    done += m;
  }
  __threadfence_block();
  __syncthreads();
  const int nblk = sub / kPer - 3;
  int n1 = 0, n2 = 0;
  const double p = gated_power(sc, [&](int j) { return (((ws[j] + ws[j + 1]) + ws[j + 2]) + ws[j + 3]) / kBlockLen; },
                               nblk > 0 ? nblk : 0, tab[kGate], n1, n2);
  if (t == 0) {
    res[0] = p;
    res[1] = (double)peak;
    res[2] = (double)n1;
    res[3] = (double)n2;
  }
}

__global__ __launch_bounds__(kThreads) void loudness_scale_kernel(const float* __restrict__ x, int64_t n, double g, float* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    y[i] = (float)((double)x[i] * g);
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  int32_t knot[kResetMax];
  int32_t on[kResetMax];
  double ptarget[kResetMax];
};

// workgroup i: slot args.slot[i] starts a stream (or is switched off) in both state halves
__global__ void loudness_reset_kernel(ResetArgs a, LoudState* st0, LoudState* st1) {
  const int i = blockIdx.x;
  if (i >= a.n) return;
  LoudState* h[2] = {st0 + a.slot[i], st1 + a.slot[i]};
  constexpr int kWords = sizeof(LoudState) / 8;
  for (int k = 0; k < 2; ++k)
    for (int w = threadIdx.x; w < kWords; w += blockDim.x) ((uint64_t*)h[k])[w] = 0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 0; k < 2; ++k) {
    h[k]->ptarget = a.ptarget[i];
    h[k]->ka = h[k]->kb = a.knot[i];
    h[k]->on = a.on[i];
  }
}

}  // namespace

struct SmolttsLoudness {
  int B;
  PingPong<LoudState> st;
  double* tab;
};

static size_t carve(SmolttsLoudness* r, char* base) {
  Carver cv{base, 0};
  r->st.carve(cv, r->B);
  r->tab = cv.take<double>(kTab);
  return cv.off;
}

extern "C" {

size_t smoltts_loudness_bytes(int32_t max_batch) {
  return stage_bytes<SmolttsLoudness>(max_batch);
}

int32_t smoltts_loudness_table_doubles(void) {
  return kTab;
}

int smoltts_loudness_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, const double* tables_host, int32_t n_tables,
                            SmolttsLoudness** out) {
  ST_REQUIRE(tables_host && n_tables == kTab, SMOLTTS_E_INVALID, "loudness_create: tables of %d doubles, %d expected", n_tables, kTab);
  SmolttsLoudness* r = nullptr;
  size_t need = 0;
  ST_TRY(stage_create("loudness_create", slab_dev, slab_bytes, max_batch, out, &r, &need));
  if (hipMemset(slab_dev, 0, need) != hipSuccess ||  // every slot off
      hipMemcpy(r->tab, tables_host, kTab * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    delete r;
    set_error("loudness_create: clearing the slab or uploading the tables failed");
    return SMOLTTS_E_HIP;
  }
  *out = r;
  return SMOLTTS_OK;
}

void smoltts_loudness_destroy(SmolttsLoudness* r) {
  delete r;
}

int smoltts_loudness_reset_slots(SmolttsLoudness* r, const int32_t* slots_host, const double* target_power_host,
                                 const int32_t* start_knot_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(r && slots_host && target_power_host && n_slots > 0, SMOLTTS_E_INVALID, "loudness_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    const double p = target_power_host[k];
    const int kn = start_knot_host ? start_knot_host[k] : 0;
    ST_REQUIRE(p >= 0.0 && p <= 1.0, SMOLTTS_E_INVALID, "loudness_reset_slots: target power %g outside [0, 1]", p);  // (a NaN fails)
    ST_REQUIRE(kn >= -kKMax && kn <= kKMax, SMOLTTS_E_INVALID, "loudness_reset_slots: start knot %d outside [%d, %d]", kn, -kKMax,
               kKMax);
    a.ptarget[i] = p;
    a.knot[i] = kn;
    a.on[i] = p > 0.0;
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("loudness_reset_slots", r->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    hipLaunchKernelGGL(loudness_reset_kernel, dim3(a.n), dim3(kThreads), 0, (hipStream_t)stream, a, r->st.half[0], r->st.half[1]);
  });
}

int smoltts_loudness_chunk(SmolttsLoudness* r, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                           const int32_t* valid_in_dev, float* out_dev, int64_t out_stride, int32_t* counts_dev, void* stream) {
  ST_TRY(check_chunk("loudness_chunk", r, pcm_dev && out_dev && counts_dev, batch, true, n_in, pcm_stride));
  ST_REQUIRE(out_stride >= n_in, SMOLTTS_E_CAPACITY, "loudness_chunk: out_stride %lld < %d samples", (long long)out_stride, n_in);
  hipLaunchKernelGGL(loudness_kernel, dim3(r->B), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, pcm_stride, batch, n_in,
                     valid_in_dev, r->tab, r->st.cur(), r->st.next(), out_dev, out_stride, counts_dev);
  ST_CHECK_HIP(hipGetLastError());
  r->st.flip();
  return SMOLTTS_OK;
}

int smoltts_loudness_measure(SmolttsLoudness* r, const float* pcm_dev, int32_t n, double* hops_dev, int64_t hops_len, double* result_dev,
                             void* stream) {
  ST_REQUIRE(r && pcm_dev && hops_dev && result_dev, SMOLTTS_E_INVALID, "loudness_measure: null argument");
  ST_REQUIRE(n >= 0 && n <= kMeasureMax, SMOLTTS_E_INVALID, "loudness_measure: n %d (0..%d)", n, kMeasureMax);
  ST_REQUIRE(hops_len >= n / kHop, SMOLTTS_E_CAPACITY, "loudness_measure: room for %lld hop energies, %d needed", (long long)hops_len,
             n / kHop);
  hipLaunchKernelGGL(loudness_measure_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, n, r->tab, hops_dev, result_dev);
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

int smoltts_loudness_scale(const float* pcm_dev, int64_t n, double gain, float* out_dev, void* stream) {
  ST_REQUIRE(pcm_dev && out_dev && n >= 0, SMOLTTS_E_INVALID, "loudness_scale: bad argument");
  ST_REQUIRE(gain >= 0.0 && gain <= 1e6, SMOLTTS_E_INVALID, "loudness_scale: gain %g", gain);
  if (n == 0) return SMOLTTS_OK;
  const int64_t blocks = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(loudness_scale_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kThreads), 0, (hipStream_t)stream,
                     pcm_dev, n, gain, out_dev);
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

int smoltts_loudness_slot_state(SmolttsLoudness* r, int32_t slot, int64_t* ints_host, double* values_host, void* stream) {
  ST_REQUIRE(r && ints_host && values_host && slot >= 0 && slot < r->B, SMOLTTS_E_INVALID, "loudness_slot_state: bad argument");
  LoudState* s = new (std::nothrow) LoudState;
  ST_REQUIRE(s, SMOLTTS_E_INVALID, "loudness_slot_state: out of host memory");
  hipError_t e = hipMemcpyAsync(s, r->st.cur() + slot, sizeof(LoudState), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) {
    delete s;
    ST_CHECK_HIP(e);
  }
  ints_host[0] = s->pos; ints_host[1] = s->ka; ints_host[2] = s->kb; ints_host[3] = s->on;
  double* v = values_host;
  for (int k = 0; k < 4; ++k) *v++ = s->f.s_start[k];
  for (int k = 0; k < 4; ++k) *v++ = s->f.s_run[k];
  for (int k = 0; k < 4; ++k) *v++ = s->f.z_run[k];
  *v++ = s->f.e_sub;
  *v++ = s->e_hop;
  for (int k = 0; k < 3; ++k) *v++ = s->hops[k];
  *v++ = (double)s->peak;
  *v++ = s->ptarget;
  for (int k = 0; k < kRing; ++k) *v++ = s->ring[k];
  delete s;
  return SMOLTTS_OK;
}

}  // extern "C"

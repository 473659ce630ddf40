// The seam between the segments of a long text: the codec's 24 kHz fp32 PCM of consecutive segments joined into one stream, in
// one launch per pass over every slot (include/smoltts_hip.h, "Seam"; the numpy model is smoltts_amd/seam.py).
//
// Blocks of kBlock samples counted from the segment's first sample are silent when max|x| < 2^-8.  The head of a segment that is
// not the stream's first drops leading silent blocks while the dropped samples stay <= kD; the tail of a segment that is not
// the stream's last holds back a run of silent blocks (at most kH samples: a longer run releases its oldest ones), releases it
// unchanged in front of a non-silent block, and at the segment's end replaces the held run of r samples by its first min(r, G)
// samples and G - min(r, G) zeros.  So one call's output is always zeros(lead) ++ segment[e0, ec) ++ zeros(z1): the state is
// three positions (judged, ec, n_in) and the samples [ec, n_in) that are still held or undecided.
#include "stage.h"

using namespace smoltts;

namespace {

constexpr int kBlock = 240;
constexpr int kRate = 24000, kH = kRate, kD = kRate;
constexpr int kMaxPause = 10 * kRate;
constexpr int kHist = 24576;        // >= kH + kBlock - 1: the held run and a partial block
constexpr int kThreads = 256;       // 4 waves
constexpr int kLanesPerBlock = 8;   // lanes that reduce one block's max-abs
constexpr int kRound = kThreads / kLanesPerBlock;  // blocks judged per round
static_assert(kHist >= kH + kBlock - 1, "seam: history too short");

struct SeamState {  // one half of the ping-pong pair, per slot
  int64_t n_in;     // samples of the segment consumed
  int64_t judged;   // samples of the segment in judged blocks
  int64_t ec;       // samples of the segment emitted or dropped ([ec, judged) is the held run)
  int32_t head;     // still dropping leading silence
  int32_t open;     // a segment is open (0: the slot is off, or its segment has ended)
  int32_t lead;     // zeros owed in front of the next output (the stream's first segment)
  int32_t pause;    // G: zeros at the segment's end (the seam's pause, or the trailing silence of the stream's last segment)
  int32_t flags;    // SMOLTTS_SEAM_FIRST | SMOLTTS_SEAM_FINAL
  int32_t pad[9];
  float hist[kHist];  // segment samples [n_in - kHist, n_in); only [ec, n_in) is kept up to date
};

__device__ __forceinline__ void copy_counters(const SeamState* si, SeamState* so) {
  so->n_in = si->n_in; so->judged = si->judged; so->ec = si->ec;
  so->head = si->head; so->open = si->open; so->lead = si->lead; so->pause = si->pause; so->flags = si->flags;
}

// grid (max_batch), 256 lanes: workgroup b runs slot b.  States ping-pong between st_in and st_out (the host alternates them);
// slots at or past `batch` only carry their state across, slots without an open segment write count 0.
__global__ __launch_bounds__(kThreads) void seam_kernel(const float* __restrict__ pcm, int64_t pcm_stride, int batch, int n_in,
                                                        const int32_t* __restrict__ valid, const int32_t* __restrict__ seg_end,
                                                        const int32_t* __restrict__ last, const SeamState* __restrict__ st_in,
                                                        SeamState* __restrict__ st_out, float* __restrict__ out,
                                                        int64_t out_stride, int32_t* __restrict__ counts) {
  __shared__ int32_t quiet[kRound];
  __shared__ int64_t sh[4];  // e0, ec, z0 + len, total
  const int b = blockIdx.x, t = threadIdx.x;
  const SeamState* si = st_in + b;
  SeamState* so = st_out + b;
  const int64_t N0 = si->n_in;
  if (!si->open) {
    if (t == 0) {
      so->open = 0;
      if (b < batch) counts[b] = 0;
    }
    return;
  }
  if (b >= batch) {  // not in this call: the live samples and the counters move to the other half
    const int64_t lo = si->ec - (N0 - kHist);
    for (int64_t i = (lo > 0 ? lo : 0) + t; i < kHist; i += kThreads) so->hist[i] = si->hist[i];
    if (t == 0) copy_counters(si, so);
    return;
  }
  int n = valid ? valid[b] : n_in;
  n = n < 0 ? 0 : (n > n_in ? n_in : n);
  const int lst = last ? (last[b] != 0) : 0;
  const int end = lst || (seg_end ? (seg_end[b] != 0) : 0);
  const int final_seg = (si->flags & SMOLTTS_SEAM_FINAL) != 0;
  const int64_t N1 = N0 + n;
  const float* x = pcm + (int64_t)b * pcm_stride;
  auto sample = [&](int64_t j) -> float {  // segment sample j, for j in [ec, N1)
    if (j >= N0) return x[j - N0];
    const int64_t h = j - (N0 - kHist);
    return h >= 0 ? si->hist[h] : 0.0f;
  };
  // thread 0's walk over the blocks (the other lanes only judge blocks)
  int64_t judged = si->judged, ec = si->ec, e0 = si->ec;
  int head = si->head;
  const int64_t j0 = si->judged;
  const int64_t span = N1 - j0;
  const int64_t nblk = span / kBlock + ((end && span % kBlock) ? 1 : 0);
  for (int64_t r0 = 0; r0 < nblk; r0 += kRound) {
    const int g = t / kLanesPerBlock, l = t % kLanesPerBlock;
    const int64_t blk = r0 + g;
    float m = 0.0f;
    if (blk < nblk) {
      const int64_t s = j0 + blk * kBlock;
      const int64_t e = s + kBlock < N1 ? s + kBlock : N1;
      for (int64_t j = s + l; j < e; j += kLanesPerBlock) {
        const float v = sample(j);
        m = v != v ? __builtin_inff() : fmaxf(m, fabsf(v));  // (a NaN is not silence, as in numpy)
      }
    }
    for (int off = kLanesPerBlock / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (l == 0) quiet[g] = m < 0.00390625f;
    __syncthreads();
    if (t == 0) {
      for (int i = 0; i < kRound && r0 + i < nblk; ++i) {
        const int64_t s = judged;
        const int64_t ln = N1 - s < kBlock ? N1 - s : kBlock;
        const int q = quiet[i];
        if (head) {
          if (q && s + ln <= kD) {
            judged = ec = e0 = s + ln;
            continue;
          }
          head = 0;
        }
        judged = s + ln;
        if (final_seg || !q) ec = judged;
        else if (judged - ec > kH) ec = judged - kH;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    int64_t z1 = 0;
    if (end) {
      if (final_seg || lst) {
        ec = N1;
        z1 = final_seg ? si->pause : 0;
      } else {
        const int64_t r = judged - ec;
        const int64_t keep = r < si->pause ? r : si->pause;
        ec += keep;
        z1 = si->pause - keep;
      }
    }
    const int64_t z0 = si->lead;
    sh[0] = e0;
    sh[1] = ec;
    sh[2] = z0 + (ec - e0);
    sh[3] = z0 + (ec - e0) + z1;
    counts[b] = (int32_t)(z0 + (ec - e0) + z1);
    so->n_in = N1; so->judged = judged; so->ec = ec; so->head = head;
    so->open = end ? 0 : 1;
    so->lead = 0; so->pause = si->pause; so->flags = si->flags;
  }
  __syncthreads();
  const int64_t s0 = sh[0], ec1 = sh[1], zl = sh[2], total = sh[3];
  const int64_t z0 = si->lead;
  float* orow = out + (int64_t)b * out_stride;
  for (int64_t i = t; i < total && i < out_stride; i += kThreads) orow[i] = (i >= z0 && i < zl) ? sample(s0 + i - z0) : 0.0f;
  if (!end) {  // carry the samples still held or undecided, [ec, N1)
    const int64_t lo = ec1 - (N1 - kHist);
    for (int64_t i = (lo > 0 ? lo : 0) + t; i < kHist; i += kThreads) so->hist[i] = sample(N1 - kHist + i);
  }
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  int32_t pause[kResetMax];
  int32_t flags[kResetMax];
  int32_t lead[kResetMax];
};

// workgroup i: slot args.slot[i] opens a segment (or is switched off) in both state halves
__global__ void seam_reset_kernel(ResetArgs a, SeamState* st0, SeamState* st1) {
  const int i = blockIdx.x;
  if (i >= a.n || threadIdx.x != 0) return;
  const int b = a.slot[i], f = a.flags[i];
  SeamState* h[2] = {st0 + b, st1 + b};
  for (int k = 0; k < 2; ++k) {
    h[k]->n_in = h[k]->judged = h[k]->ec = 0;
    h[k]->head = (f & SMOLTTS_SEAM_FIRST) ? 0 : 1;
    h[k]->open = (f & SMOLTTS_SEAM_OFF) ? 0 : 1;
    h[k]->lead = (f & SMOLTTS_SEAM_FIRST) ? a.lead[i] : 0;
    h[k]->pause = a.pause[i];
    h[k]->flags = f & (SMOLTTS_SEAM_FIRST | SMOLTTS_SEAM_FINAL);
  }
}

}  // namespace

struct SmolttsSeam {
  int B;
  PingPong<SeamState> st;
};

static size_t carve(SmolttsSeam* r, char* base) {
  Carver cv{base, 0};
  r->st.carve(cv, r->B);
  return cv.off;
}

extern "C" {

size_t smoltts_seam_bytes(int32_t max_batch) {
  return stage_bytes<SmolttsSeam>(max_batch);
}

size_t smoltts_seam_out_samples(int32_t n_in, int32_t max_zeros) {
  if (n_in < 0 || max_zeros < 0 || max_zeros > 2 * kMaxPause) return 0;
  // the held run and a partial block released, the call's samples, and the zeros (a first segment's lead, a segment's pause)
  return (size_t)n_in + (size_t)(kH + kBlock) + (size_t)max_zeros;
}

int smoltts_seam_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsSeam** out) {
  SmolttsSeam* r = nullptr;
  size_t need = 0;
  ST_TRY(stage_create("seam_create", slab_dev, slab_bytes, max_batch, out, &r, &need));
  if (hipMemset(slab_dev, 0, need) != hipSuccess) {  // every slot off
    delete r;
    set_error("seam_create: hipMemset failed");
    return SMOLTTS_E_HIP;
  }
  *out = r;
  return SMOLTTS_OK;
}

void smoltts_seam_destroy(SmolttsSeam* r) {
  delete r;
}

int smoltts_seam_reset_slots(SmolttsSeam* r, const int32_t* slots_host, const int32_t* pause_host, const int32_t* flags_host,
                             const int32_t* lead_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(r && slots_host && pause_host && flags_host && n_slots > 0, SMOLTTS_E_INVALID, "seam_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    const int p = pause_host[k], f = flags_host[k], ld = lead_host ? lead_host[k] : 0;
    ST_REQUIRE(p >= 0 && p <= kMaxPause && ld >= 0 && ld <= kMaxPause, SMOLTTS_E_INVALID,
               "seam_reset_slots: pause %d / lead %d outside [0, %d]", p, ld, kMaxPause);
    ST_REQUIRE((f & ~(SMOLTTS_SEAM_FIRST | SMOLTTS_SEAM_FINAL | SMOLTTS_SEAM_OFF)) == 0, SMOLTTS_E_INVALID,
               "seam_reset_slots: bad flags %d", f);
    a.pause[i] = p;
    a.flags[i] = f;
    a.lead[i] = ld;
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("seam_reset_slots", r->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    hipLaunchKernelGGL(seam_reset_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, r->st.half[0], r->st.half[1]);
  });
}

int smoltts_seam_chunk(SmolttsSeam* r, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                       const int32_t* valid_in_dev, const int32_t* seg_end_dev, const int32_t* last_dev, int32_t max_zeros,
                       float* out_dev, int64_t out_stride, int32_t* counts_dev, void* stream) {
  ST_TRY(check_chunk("seam_chunk", r, pcm_dev && out_dev && counts_dev, batch, true, n_in, pcm_stride));
  ST_REQUIRE(max_zeros >= 0 && max_zeros <= 2 * kMaxPause, SMOLTTS_E_INVALID, "seam_chunk: max_zeros %d", max_zeros);
  const int64_t need = (int64_t)smoltts_seam_out_samples(n_in, max_zeros);
  ST_REQUIRE(out_stride >= need, SMOLTTS_E_CAPACITY, "seam_chunk: out_stride %lld < %lld samples", (long long)out_stride, (long long)need);
  hipLaunchKernelGGL(seam_kernel, dim3(r->B), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, pcm_stride, batch, n_in,
                     valid_in_dev, seg_end_dev, last_dev, r->st.cur(), r->st.next(), out_dev, out_stride, counts_dev);
  ST_CHECK_HIP(hipGetLastError());
  r->st.flip();
  return SMOLTTS_OK;
}

int smoltts_seam_slot_state(SmolttsSeam* r, int32_t slot, int64_t* state_host, void* stream) {
  ST_REQUIRE(r && state_host && slot >= 0 && slot < r->B, SMOLTTS_E_INVALID, "seam_slot_state: bad argument");
  const SeamState* s = r->st.cur() + slot;
  int64_t v[3];
  int32_t w[5];
  ST_CHECK_HIP(hipMemcpyAsync(v, &s->n_in, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
  ST_CHECK_HIP(hipMemcpyAsync(w, &s->head, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
  ST_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (int i = 0; i < 3; ++i) state_host[i] = v[i];
  for (int i = 0; i < 5; ++i) state_host[3 + i] = w[i];
  return SMOLTTS_OK;
}

}  // extern "C"

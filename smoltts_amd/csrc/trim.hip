// Silence trimming per request: leading and trailing silence cut and pauses capped on the codec's 24 kHz fp32 PCM, in one launch
// per pass over every slot, first of the stages behind the codec (include/smoltts_hip.h, "Trim"; the numpy model,
// matched bit for bit, is smoltts_amd/trim.py).
//
// Blocks of kBlock samples counted from the segment's first sample are silent when max|x| < thr (float32; a NaN is not silence).
// Of a run of r silent blocks the first matching case keeps: (1) trim, FIRST, the run starts at block 0: its last min(r, 2)
// blocks; (2) trim, FINAL, the run reaches the segment's end: its first min(r, K) blocks, K = 10 without a pause cap P and
// min(10, ceil(P/2)) with one, or its first r - 200 blocks when P == 0 and r - K > 200; (3) P > 0 and r > P: its first ceil(P/2)
// and last floor(P/2) blocks; (4) all of it.  Non-silent blocks are always kept, and samples are only copied or dropped.
//
// Unlike the seam's, one call's output is not one range of the segment.  The blocks a slot still holds back travel compacted in
// its state: list A (blocks K .. ceil(P/2) - 1 of a run in a trimmed FINAL segment with a cap, which a non-silent block keeps and
// the segment's end drops), then queue B (the run's newest blocks), then the samples of the block that is not complete yet.  A
// call's candidates are the held blocks and the blocks it completes; thread 0 walks the new ones and marks every candidate
// dropped, emitted or held in LDS, with its offset in the output row or in the next state, and then every lane copies.
#include "stage.h"

using namespace smoltts;

namespace {

constexpr int kBlock = 240;
constexpr int kHeadKeep = 2, kTailKeep = 10, kHold = 200;  // blocks
constexpr int kMaxIn = 61440;                              // samples of one call at most (256 blocks)
constexpr int kHist = kHold * kBlock + kBlock;             // the held blocks and a partial one
constexpr int kMaxNew = (kMaxIn + kBlock - 1) / kBlock + 1;  // blocks one call completes at most (the old partial one, and a last one)
constexpr int kMaxCand = kHold + kMaxNew;
constexpr int kThreads = 256;      // 4 waves
constexpr int kLanesPerBlock = 8;  // lanes that reduce one block's max-abs
constexpr int kRound = kThreads / kLanesPerBlock;  // blocks judged per round
enum { kDrop = 0, kEmit = 1, kHeld = 2 };

struct TrimState {  // one half of the ping-pong pair, per slot
  int64_t n_in;           // samples of the segment consumed
  int64_t judged;         // samples of the segment in judged blocks
  int64_t emitted;        // samples of the segment written out
  int64_t blocks;         // blocks judged
  int64_t dropped_head, dropped_pause, dropped_tail;  // samples dropped by cases 1, 3 and 2
  int64_t run_drop;       // samples case 3 dropped from the open run (they are the tail's if the run reaches a trimmed end)
  int32_t r;              // blocks of the open run (0: none)
  int32_t heldA, heldB;   // blocks in list A and in queue B
  int32_t open;           // a segment is open (0: the slot is off, or its segment has ended)
  int32_t flags;          // SMOLTTS_SEAM_FIRST | SMOLTTS_SEAM_FINAL
  int32_t trim;           // cases 1 and 2 apply
  int32_t P;              // the pause cap in blocks (0: none)
  float thr;              // the silence threshold
  float hist[kHist];      // A's blocks, B's blocks, then the n_in - judged samples of the incomplete block
};

__device__ __forceinline__ void copy_counters(const TrimState* si, TrimState* so) {
  so->n_in = si->n_in; so->judged = si->judged; so->emitted = si->emitted; so->blocks = si->blocks;
  so->dropped_head = si->dropped_head; so->dropped_pause = si->dropped_pause; so->dropped_tail = si->dropped_tail;
  so->run_drop = si->run_drop; so->r = si->r; so->heldA = si->heldA; so->heldB = si->heldB; so->open = si->open;
  so->flags = si->flags; so->trim = si->trim; so->P = si->P; so->thr = si->thr;
}

// grid (max_batch), 256 lanes: workgroup b runs slot b.  States ping-pong between st_in and st_out (the host alternates them);
// slots at or past `batch` only carry their state across, slots without an open segment write count 0.
__global__ __launch_bounds__(kThreads) void trim_kernel(const float* __restrict__ pcm, int64_t pcm_stride, int batch, int n_in,
                                                        const int32_t* __restrict__ valid, const int32_t* __restrict__ seg_end,
                                                        const int32_t* __restrict__ last, const TrimState* __restrict__ st_in,
                                                        TrimState* __restrict__ st_out, float* __restrict__ out,
                                                        int64_t out_stride, int32_t* __restrict__ counts) {
  __shared__ int32_t quiet[kMaxNew];
  __shared__ int32_t status[kMaxCand];
  __shared__ int32_t offs[kMaxCand];
  __shared__ int32_t sh[2];  // samples emitted, samples held
  const int b = blockIdx.x, t = threadIdx.x;
  const TrimState* si = st_in + b;
  TrimState* so = st_out + b;
  if (!si->open) {
    if (t == 0) {
      copy_counters(si, so);
      if (b < batch) counts[b] = 0;
    }
    return;
  }
  const int held0 = si->heldA + si->heldB;           // held blocks: candidates [0, held0)
  const int part0 = (int)(si->n_in - si->judged);    // samples of the incomplete block, behind them in hist
  if (b >= batch) {  // not in this call: the live samples and the counters move to the other half
    const int live = held0 * kBlock + part0;
    for (int i = t; i < live && i < kHist; i += kThreads) so->hist[i] = si->hist[i];
    if (t == 0) copy_counters(si, so);
    return;
  }
  const int n = valid_count(valid, b, n_in);
  const int end = (last && last[b] != 0) || (seg_end && seg_end[b] != 0);
  const float* x = pcm + (int64_t)b * pcm_stride;
  const float* tail = si->hist + held0 * kBlock;
  auto fresh = [&](int v) -> float {  // sample v of the incomplete block followed by the call's samples
    return v < part0 ? tail[v] : x[v - part0];
  };
  const int span = part0 + n;
  const int nfull = span / kBlock;
  const int lastlen = (end && span % kBlock) ? span % kBlock : kBlock;  // the length of the call's last block
  const int nblk = nfull + ((end && span % kBlock) ? 1 : 0);
  const int ncand = held0 + nblk;
  const float thr = si->thr;
  for (int r0 = 0; r0 < nblk; r0 += kRound) {
    const int g = t / kLanesPerBlock, l = t % kLanesPerBlock;
    const int blk = r0 + g;
    float m = 0.0f;
    if (blk < nblk) {
      const int s = blk * kBlock;
      const int e = s + kBlock < span ? s + kBlock : span;
      for (int j = s + l; j < e; j += kLanesPerBlock) {
        const float v = fresh(j);
        m = v != v ? __builtin_inff() : fmaxf(m, fabsf(v));  // (a NaN is not silence, as in numpy)
      }
    }
    for (int off = kLanesPerBlock / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (l == 0 && blk < nblk) quiet[blk] = m < thr;
  }
  for (int i = t; i < ncand; i += kThreads) status[i] = kHeld;
  __syncthreads();
  if (t == 0) {
    const int P = si->P, a = (P + 1) / 2, c = P / 2;
    const int first = si->trim && (si->flags & SMOLTTS_SEAM_FIRST), final_seg = si->trim && (si->flags & SMOLTTS_SEAM_FINAL);
    const int K = P == 0 ? kTailKeep : (kTailKeep < a ? kTailKeep : a);
    int A0 = 0, A1 = si->heldA, B0 = si->heldA, B1 = held0;  // candidate ranges of list A and queue B
    int r = si->r;
    int64_t blocks = si->blocks, judged = si->judged, run_drop = si->run_drop;
    int64_t d_head = si->dropped_head, d_pause = si->dropped_pause, d_tail = si->dropped_tail;
    auto push_b = [&](int ci) {
      if (B0 == B1) B0 = B1 = ci;
      ++B1;
    };
    auto release = [&](int what) {  // every held block leaves: emitted, or dropped
      for (int i = A0; i < A1; ++i) status[i] = what;
      for (int i = B0; i < B1; ++i) status[i] = what;
      A0 = A1 = B0 = B1 = 0;
    };
    auto pause = [&](int ci) {  // a block past the first ceil(P/2) of a run: only the newest floor(P/2) stay
      push_b(ci);
      if (B1 - B0 > c) {
        status[B0++] = kDrop;
        d_pause += kBlock;
        run_drop += kBlock;
      }
    };
    for (int j = 0; j < nblk; ++j) {
      const int ci = held0 + j;
      if (!quiet[j]) {
        release(kEmit);
        r = 0;
        run_drop = 0;
        status[ci] = kEmit;
      } else {
        const int i = r++;
        if (first && blocks == i) {  // the run started at block 0
          push_b(ci);
          if (B1 - B0 > kHeadKeep) {
            status[B0++] = kDrop;
            d_head += kBlock;
          }
        } else if (final_seg) {
          if (i < K) {
            status[ci] = kEmit;
          } else if (P == 0) {
            push_b(ci);
            if (B1 - B0 > kHold) status[B0++] = kEmit;
          } else if (i < a) {
            if (A0 == A1) A0 = A1 = ci;
            ++A1;
          } else {
            pause(ci);
          }
        } else if (P > 0 && i >= a) {
          pause(ci);
        } else {
          status[ci] = kEmit;
        }
      }
      ++blocks;
      judged += j == nblk - 1 ? lastlen : kBlock;
    }
    if (end) {
      if (r > 0 && !(first && blocks == r) && final_seg) {
        int64_t held = (int64_t)(A1 - A0 + B1 - B0) * kBlock;
        if (nblk > 0 && status[ncand - 1] == kHeld) held -= kBlock - lastlen;  // (the segment's partial last block)
        d_tail += held + run_drop;
        d_pause -= run_drop;
        release(kDrop);
      } else {
        release(kEmit);
      }
    }
    int o = 0, h = 0;
    for (int i = 0; i < ncand; ++i) {
      const int len = i == ncand - 1 && nblk > 0 ? lastlen : kBlock;
      if (status[i] == kEmit) {
        offs[i] = o;
        o += len;
      } else if (status[i] == kHeld) {
        offs[i] = h;
        h += len;
      }
    }
    sh[0] = o;
    sh[1] = h;
    counts[b] = o;
    so->n_in = si->n_in + n; so->judged = judged; so->emitted = si->emitted + o; so->blocks = blocks;
    so->dropped_head = d_head; so->dropped_pause = d_pause; so->dropped_tail = d_tail; so->run_drop = run_drop;
    so->r = r; so->heldA = A1 - A0; so->heldB = B1 - B0; so->open = end ? 0 : 1;
    so->flags = si->flags; so->trim = si->trim; so->P = si->P; so->thr = si->thr;
  }
  __syncthreads();
  const int h_total = sh[1];
  float* orow = out + (int64_t)b * out_stride;
  const int work = ncand * kBlock;
  for (int idx = t; idx < work; idx += kThreads) {
    const int ci = idx / kBlock, j = idx % kBlock;
    const int st = status[ci];
    if (st == kDrop || (ci == ncand - 1 && nblk > 0 && j >= lastlen)) continue;
    const float v = ci < held0 ? si->hist[idx] : fresh((ci - held0) * kBlock + j);
    const int64_t at = offs[ci] + j;
    if (st == kEmit) {
      if (at < out_stride) orow[at] = v;
    } else if (at < kHist) {
      so->hist[at] = v;
    }
  }
  if (!end) {  // the incomplete block follows the held ones
    const int rest = span - nfull * kBlock;
    for (int i = t; i < rest; i += kThreads)
      if (h_total + i < kHist) so->hist[h_total + i] = fresh(nfull * kBlock + i);
  }
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  int32_t flags[kResetMax];
  int32_t trim[kResetMax];
  int32_t pause[kResetMax];
  float thr[kResetMax];
};

// workgroup i: slot args.slot[i] opens a segment (or is switched off) in both state halves
__global__ void trim_reset_kernel(ResetArgs a, TrimState* st0, TrimState* st1) {
  const int i = blockIdx.x;
  if (i >= a.n || threadIdx.x != 0) return;
  const int b = a.slot[i], f = a.flags[i];
  TrimState* h[2] = {st0 + b, st1 + b};
  for (int k = 0; k < 2; ++k) {
    h[k]->n_in = h[k]->judged = h[k]->emitted = h[k]->blocks = 0;
    h[k]->dropped_head = h[k]->dropped_pause = h[k]->dropped_tail = h[k]->run_drop = 0;
    h[k]->r = h[k]->heldA = h[k]->heldB = 0;
    h[k]->open = (f & SMOLTTS_SEAM_OFF) ? 0 : 1;
    h[k]->flags = f & (SMOLTTS_SEAM_FIRST | SMOLTTS_SEAM_FINAL);
    h[k]->trim = a.trim[i] != 0;
    h[k]->P = a.pause[i];
    h[k]->thr = a.thr[i];
  }
}

}  // namespace

struct SmolttsTrim {
  int B;
  PingPong<TrimState> st;
};

static size_t carve(SmolttsTrim* r, char* base) {
  Carver cv{base, 0};
  r->st.carve(cv, r->B);
  return cv.off;
}

extern "C" {

size_t smoltts_trim_bytes(int32_t max_batch) {
  return stage_bytes<SmolttsTrim>(max_batch);
}

size_t smoltts_trim_out_samples(int32_t n_in) {
  if (n_in < 0 || n_in > kMaxIn) return 0;
  return (size_t)n_in + (size_t)kHist;  // the held blocks and the partial block released, and the call's samples
}

int smoltts_trim_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsTrim** out) {
  SmolttsTrim* r = nullptr;
  size_t need = 0;
  ST_TRY(stage_create("trim_create", slab_dev, slab_bytes, max_batch, out, &r, &need));
  if (hipMemset(slab_dev, 0, need) != hipSuccess) {  // every slot off
    delete r;
    set_error("trim_create: hipMemset failed");
    return SMOLTTS_E_HIP;
  }
  *out = r;
  return SMOLTTS_OK;
}

void smoltts_trim_destroy(SmolttsTrim* r) {
  delete r;
}

int smoltts_trim_reset_slots(SmolttsTrim* r, const int32_t* slots_host, const int32_t* flags_host, const int32_t* trim_host,
                             const int32_t* pause_host, const float* thr_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(r && slots_host && flags_host && trim_host && pause_host && thr_host && n_slots > 0, SMOLTTS_E_INVALID,
             "trim_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    const int p = pause_host[k], f = flags_host[k];
    const float thr = thr_host[k];
    ST_REQUIRE(p == 0 || (p >= 10 && p <= kHold), SMOLTTS_E_INVALID, "trim_reset_slots: pause cap %d outside 0 and [10, %d] blocks", p,
               kHold);
    ST_REQUIRE(thr > 0.0f && thr <= 1.0f, SMOLTTS_E_INVALID, "trim_reset_slots: threshold %g outside (0, 1]", (double)thr);
    ST_REQUIRE((f & ~(SMOLTTS_SEAM_FIRST | SMOLTTS_SEAM_FINAL | SMOLTTS_SEAM_OFF)) == 0, SMOLTTS_E_INVALID,
               "trim_reset_slots: bad flags %d", f);
    a.flags[i] = f;
    a.trim[i] = trim_host[k] != 0;
    a.pause[i] = p;
    a.thr[i] = thr;
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("trim_reset_slots", r->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    hipLaunchKernelGGL(trim_reset_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, r->st.half[0], r->st.half[1]);
  });
}

int smoltts_trim_chunk(SmolttsTrim* r, const float* pcm_dev, int64_t pcm_stride, int32_t batch, int32_t n_in,
                       const int32_t* valid_in_dev, const int32_t* seg_end_dev, const int32_t* last_dev, float* out_dev,
                       int64_t out_stride, int32_t* counts_dev, void* stream) {
  ST_TRY(check_chunk("trim_chunk", r, pcm_dev && out_dev && counts_dev, batch, true, n_in, pcm_stride));
  ST_REQUIRE(n_in <= kMaxIn, SMOLTTS_E_INVALID, "trim_chunk: n_in %d above %d samples a call", n_in, kMaxIn);
  const int64_t need = (int64_t)smoltts_trim_out_samples(n_in);
  ST_REQUIRE(out_stride >= need, SMOLTTS_E_CAPACITY, "trim_chunk: out_stride %lld < %lld samples", (long long)out_stride, (long long)need);
  hipLaunchKernelGGL(trim_kernel, dim3(r->B), dim3(kThreads), 0, (hipStream_t)stream, pcm_dev, pcm_stride, batch, n_in,
                     valid_in_dev, seg_end_dev, last_dev, r->st.cur(), r->st.next(), out_dev, out_stride, counts_dev);
  ST_CHECK_HIP(hipGetLastError());
  r->st.flip();
  return SMOLTTS_OK;
}

int smoltts_trim_slot_state(SmolttsTrim* r, int32_t slot, int64_t* state_host, void* stream) {
  ST_REQUIRE(r && state_host && slot >= 0 && slot < r->B, SMOLTTS_E_INVALID, "trim_slot_state: bad argument");
  const TrimState* s = r->st.cur() + slot;
  int64_t v[8];
  int32_t w[4];
  ST_CHECK_HIP(hipMemcpyAsync(v, &s->n_in, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
  ST_CHECK_HIP(hipMemcpyAsync(w, &s->r, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
  ST_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  state_host[0] = v[0];
  state_host[1] = v[1];
  state_host[2] = v[2];
  state_host[3] = (int64_t)(w[1] + w[2]) * kBlock;
  state_host[4] = v[4];
  state_host[5] = v[5];
  state_host[6] = v[6];
  state_host[7] = w[3];
  return SMOLTTS_OK;
}

}  // extern "C"

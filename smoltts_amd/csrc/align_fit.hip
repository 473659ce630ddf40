// The causal fit of streamed character timestamps, one launch per tick over every slot (include/smoltts_hip.h, "Streamed
// alignment fit"; the numpy model, which this file reproduces bit for bit, is smoltts_amd/align.py StreamFit).
//
// A slot's state lives in a caller-owned slab: a header, the stack of pooled blocks (value, weight, first and last weighted
// frame; at most one block per frame) and the committed starts in fp64.  Workgroup b (one wave) runs slot b: it consumes the
// slot's alignment rows from the frame it has seen up to the session's frame counter, cut at the slot's frame budget, and once
// the slot has ended by the rule the host closes a stream with (stream_ends: the done flag with a frame, or the budget) it gives
// every remaining token its start.  In rounds of 64 frames, lane l sums the chosen heads' m and s1 of frame l in ascending pair
// order into LDS; lane 0 then walks the round's frames: push, pool while the block below is larger, commit while a block at or
// above the next token's level began at least `lag` frames back.  The search for that block starts at the top of the stack,
// where the uncommitted levels live.  No state is shared between workgroups, so there is one copy of it and no hand-off.
//
// Every exit is uniform over the workgroup and stands in front of the first address formed from a counter: slot off or
// finished, a header or a counter out of range, nothing new.  Every fp64 operation is a single rounded multiply, add or divide
// or a compare in the model's order (no contraction in this file).
#include "stage.h"

#pragma clang fp contract(off)

using namespace smoltts;

namespace {

constexpr int kLanes = 64;
constexpr int kMinLag = 1, kMaxLag = 64;
constexpr double kMinMass = 0.05;  // align.MIN_MASS

struct FitHeader {  // per slot
  int32_t seen;       // frames consumed
  int32_t committed;  // starts that are final
  int32_t depth;      // blocks on the stack
  int32_t n;          // the text's tokens
  int32_t lag;
  int32_t finished;
  int32_t on;
  int32_t cap;        // the frames the slot's request may have (its stream ends there)
};
static_assert(sizeof(FitHeader) == 32, "align_fit: header layout");

struct FitView {  // the slab's regions
  FitHeader* hdr;   // [B]
  double* v;        // [B][F] fitted value of a block
  double* w;        // [B][F] its weight
  int32_t* f0;      // [B][F] its first weighted frame
  int32_t* f1;      // [B][F] ... and its last
  double* starts;   // [B][T]
  int32_t* counts;  // [B] committed, for the host's snapshot
};

// The first block (from the top) at or above `level`: depth when none is.  v is non-decreasing over the stack.
__device__ __forceinline__ int first_at(const double* __restrict__ v, int depth, double level) {
  int j = depth;
  while (j > 0 && v[j - 1] >= level) --j;
  return j;
}

// fit's crossing of `level` in front of block j (0 < j < depth)
__device__ __forceinline__ double crossing(const double* __restrict__ v, const int32_t* __restrict__ f0, const int32_t* __restrict__ f1,
                                           int j, double level) {
  const double xa = (double)f1[j - 1] + 0.5, xb = (double)f0[j] + 0.5;
  return xa + (level - v[j - 1]) / (v[j] - v[j - 1]) * (xb - xa);
}

// grid (max_batch), one wave: workgroup b runs slot b
__global__ __launch_bounds__(kLanes) void align_fit_kernel(const float* __restrict__ rows, int n_pairs, int max_frames, int max_tokens,
                                                           const int32_t* __restrict__ frames, const int32_t* __restrict__ done, FitView s) {
  __shared__ double sh_mass[kLanes], sh_s[kLanes];
  __shared__ int32_t sh_ok[kLanes];
  const int b = blockIdx.x, lane = threadIdx.x;
  FitHeader* hp = s.hdr + b;
  const FitHeader h = *hp;
  if (!h.on || h.finished) return;
  const int cnt = frames[b], dn = done[b];
  if (cnt < 0) return;
  if (h.cap < 1 || h.cap > max_frames || h.lag < kMinLag || h.n < 0 || h.n > max_tokens || h.seen < 0 || h.seen > h.cap || h.depth < 0 ||
      h.depth > h.seen || h.committed < (h.n > 0 ? 1 : 0) || h.committed > h.n)
    return;
  const int F = cnt < h.cap ? cnt : h.cap;  // (cap <= max_frames: the rows' extent)
  const bool ends = (dn != 0 && cnt > 0) || cnt >= h.cap;  // stream_ends
  if (F <= h.seen && !ends) return;

  double* __restrict__ v = s.v + (size_t)b * max_frames;
  double* __restrict__ w = s.w + (size_t)b * max_frames;
  int32_t* __restrict__ f0 = s.f0 + (size_t)b * max_frames;
  int32_t* __restrict__ f1 = s.f1 + (size_t)b * max_frames;
  double* __restrict__ st = s.starts + (size_t)b * max_tokens;
  const float* __restrict__ row = rows + (size_t)b * max_frames * n_pairs * 2;
  int depth = h.depth, committed = h.committed;  // (lane 0's are the live ones)

  for (int base = h.seen; base < F; base += kLanes) {
    const int f = base + lane;
    if (f < F) {
      const float* r = row + (size_t)f * n_pairs * 2;
      bool measured = n_pairs > 0;
      double mass = 0.0, sum = 0.0;
      for (int p = 0; p < n_pairs; ++p) {
        const float2 ms = *reinterpret_cast<const float2*>(r + 2 * p);
        measured = measured && ms.x >= 0.0f;
        mass = mass + (double)ms.x;
        sum = sum + (double)ms.y;
      }
      sh_mass[lane] = mass;
      sh_s[lane] = sum;
      sh_ok[lane] = measured && mass >= kMinMass;
    }
    __syncthreads();
    if (lane == 0) {
      const int m = F - base < kLanes ? F - base : kLanes;
      for (int k = 0; k < m; ++k) {
        if (!sh_ok[k]) continue;
        const int fr = base + k;
        const double mass = sh_mass[k];
        v[depth] = sh_s[k] / mass;  // depth < seen + k + 1 <= max_frames: at most one block per frame
        w[depth] = mass;
        f0[depth] = fr;
        f1[depth] = fr;
        ++depth;
        while (depth > 1 && v[depth - 2] > v[depth - 1]) {  // pool the two last blocks
          const double wa = w[depth - 2], wb = w[depth - 1];
          const double ww = wa + wb;
          v[depth - 2] = (v[depth - 2] * wa + v[depth - 1] * wb) / ww;
          w[depth - 2] = ww;
          f1[depth - 2] = f1[depth - 1];
          --depth;
        }
        while (committed < h.n) {
          const double level = (double)committed - 0.5;
          const int j = first_at(v, depth, level);
          if (j == depth || fr - f0[j] < h.lag) break;
          const double c = j == 0 ? 0.0 : crossing(v, f0, f1, j, level);
          const double prev = st[committed - 1];
          st[committed] = prev > c ? prev : c;
          ++committed;
        }
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    if (ends) {  // finish(F)
      const double total = (double)F;
      const double share = total / (double)(h.n > 1 ? h.n : 1);
      while (committed < h.n) {
        double c;
        if (depth == 0) {
          c = (double)committed * share;
        } else {
          const double level = (double)committed - 0.5;
          const int j = first_at(v, depth, level);
          c = j == depth ? total : (j == 0 ? 0.0 : crossing(v, f0, f1, j, level));
        }
        const double prev = st[committed - 1];
        c = prev > c ? prev : c;
        st[committed] = total < c ? total : c;
        ++committed;
      }
    }
    hp->seen = F > h.seen ? F : h.seen;
    hp->committed = committed;
    hp->depth = depth;
    hp->finished = ends ? 1 : 0;
    s.counts[b] = committed;
  }
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  int32_t tokens[kResetMax];  // < 0: off
  int32_t lag[kResetMax];
  int32_t cap[kResetMax];
};

// lane i: slot args.slot[i] starts a stream (or is switched off)
__global__ __launch_bounds__(kLanes) void align_fit_reset_kernel(ResetArgs a, FitView s, int max_tokens) {
  const int i = threadIdx.x;
  if (i >= a.n) return;
  const int b = a.slot[i];
  const bool on = a.tokens[i] >= 0;
  FitHeader h;
  h.seen = 0;
  h.committed = on && a.tokens[i] > 0 ? 1 : 0;
  h.depth = 0;
  h.n = on ? a.tokens[i] : 0;
  h.lag = a.lag[i];
  h.finished = 0;
  h.on = on ? 1 : 0;
  h.cap = a.cap[i];
  s.hdr[b] = h;
  s.counts[b] = h.committed;
  if (h.committed) s.starts[(size_t)b * max_tokens] = 0.0;
}

}  // namespace

struct SmolttsAlignFit {
  int B, F, T;  // slots, max_frames, max_tokens
  FitView s;
};

static size_t carve(SmolttsAlignFit* r, char* base) {
  Carver cv{base, 0};
  const size_t B = r->B, F = r->F, T = r->T;
  r->s.hdr = cv.take<FitHeader>(B);
  r->s.v = cv.take<double>(B * F);
  r->s.w = cv.take<double>(B * F);
  r->s.f0 = cv.take<int32_t>(B * F);
  r->s.f1 = cv.take<int32_t>(B * F);
  r->s.starts = cv.take<double>(B * T);
  r->s.counts = cv.take<int32_t>(B);
  return cv.off;
}

static bool sizes_ok(int32_t max_batch, int32_t max_frames, int32_t max_tokens) {
  return max_batch > 0 && max_batch <= (1 << 16) && max_frames > 0 && max_frames <= (1 << 20) && max_tokens > 0 && max_tokens <= (1 << 20);
}

extern "C" {

size_t smoltts_align_fit_bytes(int32_t max_batch, int32_t max_frames, int32_t max_tokens) {
  if (!sizes_ok(max_batch, max_frames, max_tokens)) return 0;
  SmolttsAlignFit tmp;
  tmp.B = max_batch; tmp.F = max_frames; tmp.T = max_tokens;
  return carve(&tmp, nullptr);
}

int smoltts_align_fit_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, int32_t max_frames, int32_t max_tokens,
                             SmolttsAlignFit** out) {
  ST_REQUIRE(slab_dev && out && sizes_ok(max_batch, max_frames, max_tokens), SMOLTTS_E_INVALID, "align_fit_create: bad argument");
  ST_REQUIRE(((uintptr_t)slab_dev & 255) == 0, SMOLTTS_E_INVALID, "align_fit_create: slab must be 256-byte aligned");
  const size_t need = smoltts_align_fit_bytes(max_batch, max_frames, max_tokens);
  ST_REQUIRE(slab_bytes >= need, SMOLTTS_E_CAPACITY, "align_fit_create: slab has %zu bytes, %zu needed", slab_bytes, need);
  SmolttsAlignFit* r = new (std::nothrow) SmolttsAlignFit;
  ST_REQUIRE(r, SMOLTTS_E_INVALID, "align_fit_create: out of host memory");
  r->B = max_batch; r->F = max_frames; r->T = max_tokens;
  carve(r, (char*)slab_dev);
  if (hipMemset(slab_dev, 0, need) != hipSuccess) {  // every slot off
    delete r;
    set_error("align_fit_create: clearing the slab failed");
    return SMOLTTS_E_HIP;
  }
  *out = r;
  return SMOLTTS_OK;
}

void smoltts_align_fit_destroy(SmolttsAlignFit* r) {
  delete r;
}

int smoltts_align_fit_reset_slots(SmolttsAlignFit* r, const int32_t* slots_host, const int32_t* n_tokens_host, const int32_t* lag_host,
                                  const int32_t* cap_frames_host, int32_t n_slots, void* stream) {
  ST_REQUIRE(r && slots_host && n_tokens_host && lag_host && cap_frames_host && n_slots > 0, SMOLTTS_E_INVALID,
             "align_fit_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    const int32_t n = n_tokens_host[k];
    if (n < 0) {  // off: the other values are not read
      a.tokens[i] = -1; a.lag[i] = kMinLag; a.cap[i] = 1;
      return SMOLTTS_OK;
    }
    ST_REQUIRE(n <= r->T, SMOLTTS_E_CAPACITY, "align_fit_reset_slots: %d tokens above max_tokens %d", n, r->T);
    ST_REQUIRE(lag_host[k] >= kMinLag && lag_host[k] <= kMaxLag, SMOLTTS_E_INVALID, "align_fit_reset_slots: lag %d outside %d..%d",
               lag_host[k], kMinLag, kMaxLag);
    ST_REQUIRE(cap_frames_host[k] >= 1 && cap_frames_host[k] <= r->F, SMOLTTS_E_INVALID,
               "align_fit_reset_slots: frame budget %d outside 1..%d", cap_frames_host[k], r->F);
    a.tokens[i] = n; a.lag[i] = lag_host[k]; a.cap[i] = cap_frames_host[k];
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("align_fit_reset_slots", r->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    hipLaunchKernelGGL(align_fit_reset_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, a, r->s, r->T);
  });
}

int smoltts_align_fit_push(SmolttsAlignFit* r, const float* rows_dev, int32_t n_pairs, int32_t max_frames, const int32_t* n_frames_dev,
                           const int32_t* done_dev, void* stream) {
  ST_REQUIRE(r && rows_dev && n_frames_dev && done_dev, SMOLTTS_E_INVALID, "align_fit_push: null argument");
  ST_REQUIRE(n_pairs >= 1 && n_pairs <= 16, SMOLTTS_E_INVALID, "align_fit_push: n_pairs %d (1..16)", n_pairs);
  ST_REQUIRE(((uintptr_t)rows_dev & 7) == 0, SMOLTTS_E_INVALID, "align_fit_push: rows must be 8-byte aligned");
  ST_REQUIRE(max_frames == r->F, SMOLTTS_E_INVALID, "align_fit_push: rows of %d frames, the handle has %d", max_frames, r->F);
  hipLaunchKernelGGL(align_fit_kernel, dim3(r->B), dim3(kLanes), 0, (hipStream_t)stream, rows_dev, n_pairs, r->F, r->T, n_frames_dev,
                     done_dev, r->s);
  ST_CHECK_HIP(hipGetLastError());
  return SMOLTTS_OK;
}

int smoltts_align_fit_outputs(SmolttsAlignFit* r, double** starts_dev, int32_t** committed_dev, int32_t* max_tokens) {
  ST_REQUIRE(r, SMOLTTS_E_INVALID, "align_fit_outputs: null handle");
  if (starts_dev) *starts_dev = r->s.starts;
  if (committed_dev) *committed_dev = r->s.counts;
  if (max_tokens) *max_tokens = r->T;
  return SMOLTTS_OK;
}

}  // extern "C"

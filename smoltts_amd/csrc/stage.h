// What the post-codec stream stages (resample.hip, tsm.hip, seam.hip, flac.hip) share.  A stage is a handle over a caller-owned
// slab holding, per slot, a configuration and a ping-pong pair of states: <stage>_reset_slots writes both halves of the listed
// slots, <stage>_chunk is one launch over every slot that reads the current half and writes the next one.  A stage supplies its
// kernels, its state structs, one global carve(handle*, base) (Carver, common.h) and the checks of its own arguments.
#pragma once
#include <new>

#include "common.h"

namespace smoltts {

// ---- device
// valid[b] (n_in without a list) inside [0, n_in].  seam_kernel and flac_kernel keep these lines inline: through the helper the
// compiler schedules them differently, and their instruction streams are pinned.
__device__ __forceinline__ int valid_count(const int32_t* valid, int b, int n_in) {
  const int n = valid ? valid[b] : n_in;
  return n < 0 ? 0 : (n > n_in ? n_in : n);
}

// ---- host
// The two halves of the per-slot state: a chunk launch reads cur() and writes next() (so no workgroup reads what another one
// writes in the same launch), then the host flips.
template <typename T>
struct PingPong {
  T* half[2];
  unsigned parity;  // half[parity] holds the slots' current state
  void carve(Carver& cv, size_t n) {
    half[0] = cv.take<T>(n);
    half[1] = cv.take<T>(n);
    parity = 0;
  }
  const T* cur() const { return half[parity]; }
  T* next() const { return half[parity ^ 1]; }
  void flip() { parity ^= 1; }
};

// <stage>_bytes
template <typename H>
size_t stage_bytes(int32_t max_batch) {
  H tmp;
  tmp.B = max_batch;
  return max_batch > 0 ? carve(&tmp, nullptr) : 0;
}

// <stage>_create: the slab checked under the call's name, then a handle carved over it (*need: the slab's bytes in use).  The
// caller owns the handle from here on and deletes it if a later step fails.
template <typename H>
int stage_create(const char* what, void* slab_dev, size_t slab_bytes, int32_t max_batch, H** out, H** made, size_t* need) {
  ST_REQUIRE(slab_dev && out && max_batch > 0, SMOLTTS_E_INVALID, "%s: bad argument", what);
  ST_REQUIRE(((uintptr_t)slab_dev & 255) == 0, SMOLTTS_E_INVALID, "%s: slab must be 256-byte aligned", what);
  *need = stage_bytes<H>(max_batch);
  ST_REQUIRE(slab_bytes >= *need, SMOLTTS_E_CAPACITY, "%s: slab has %zu bytes, %zu needed", what, slab_bytes, *need);
  H* h = new (std::nothrow) H;
  ST_REQUIRE(h, SMOLTTS_E_INVALID, "%s: out of host memory", what);
  h->B = max_batch;
  carve(h, (char*)slab_dev);
  *made = h;
  return SMOLTTS_OK;
}

// <stage>_reset_slots: the listed slots in groups of kResetMax, one launch of the stage's reset kernel per group, the group's
// entries travelling as kernel arguments.  Args starts with {int32_t n; int32_t slot[kResetMax]; ...}; fill(args, i, k) checks
// the stage's own values of the k-th listed slot and writes them to entry i (it may refuse with an error code); launch(args)
// launches the reset kernel.
constexpr int kResetMax = 16;
template <typename Args, typename Fill, typename Launch>
int reset_in_groups(const char* what, int B, const int32_t* slots_host, int n_slots, Fill fill, Launch launch) {
  for (int i0 = 0; i0 < n_slots; i0 += kResetMax) {
    Args a;
    memset(&a, 0, sizeof(a));
    a.n = n_slots - i0 < kResetMax ? n_slots - i0 : kResetMax;
    for (int i = 0; i < a.n; ++i) {
      ST_TRY(check_slot(what, slots_host[i0 + i], B));
      ST_TRY(fill(a, i, i0 + i));
      a.slot[i] = slots_host[i0 + i];
    }
    launch(a);
    ST_CHECK_HIP(hipGetLastError());
  }
  return SMOLTTS_OK;
}

// <stage>_chunk: `rest` = the stage's other pointers are there; a call without fp32 input (has_pcm false: the FLAC stage fed
// int16 samples) has no n_in to check
template <typename H>
int check_chunk(const char* what, const H* h, bool rest, int batch, bool has_pcm, int n_in, int64_t pcm_stride) {
  ST_REQUIRE(h && rest, SMOLTTS_E_INVALID, "%s: null argument", what);
  ST_REQUIRE(batch > 0 && batch <= h->B, SMOLTTS_E_INVALID, "%s: batch %d (1..%d)", what, batch, h->B);
  ST_REQUIRE(!has_pcm || (n_in >= 0 && pcm_stride >= n_in), SMOLTTS_E_INVALID, "%s: n_in %d, pcm_stride %lld", what, n_in,
             (long long)pcm_stride);
  return SMOLTTS_OK;
}

}  // namespace smoltts

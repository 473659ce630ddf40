// Row argmax / sampling (device side), shared by argmax_kernel (small_ops.hip) and the frame loop's commit kernel
// (lm_engine.hip), which picks the slow token and the last depth code itself (two launches fewer per frame).
//
// torch.argmax / mx.argmax semantics: index of the first maximal element (lm/generate.py:88-99,118-132).  Also tracks the
// top-1 / top-2 gap (parity diagnostics).  Sampling (temp > 0): exact categorical sampling from softmax(logits / temp) by
// the Gumbel-max trick with a counter-based generator, optionally restricted to tokens with p >= min_p * p_max.
#pragma once
#include "x3.h"

namespace smoltts {

struct Top2 {
  float v1;
  int i1;
  float v2;
};
__device__ __forceinline__ Top2 top2_merge(Top2 a, Top2 b) {
  Top2 o;
  const bool a_first = (a.v1 > b.v1) || (a.v1 == b.v1 && a.i1 < b.i1);
  if (a_first) {
    o.v1 = a.v1; o.i1 = a.i1; o.v2 = fmaxf(a.v2, b.v1);
  } else {
    o.v1 = b.v1; o.i1 = b.i1; o.v2 = fmaxf(b.v2, a.v1);
  }
  return o;
}

// Counter-based uniform in (0, 1): a function of (seed, slot, frame, step, column) only, so sampling is
// reproducible under graph replay and independent of launch geometry.
//   session-wide mode: uniform01(seed + 0x9E3779B97F4A7C15 * salt[r], r, frame, step, col)  (slot r's salt = its tenant count)
//   slot mode (SampleArgs.table): the REQUEST key uniform01(table[r].seed, 0, frames[r], step, col) -- the request's own seed and
//   frame number only, so a request draws the same numbers in any slot, after any tenants, beside any companions.
// Host model: smoltts_amd/sampling.py.
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ float uniform01(uint64_t seed, int slot, int frame, int step, int col) {
  uint32_t h = mix32((uint32_t)seed ^ 0x9E3779B9U * (uint32_t)(slot + 1));
  h = mix32(h ^ (uint32_t)(seed >> 32) ^ 0x85EBCA6BU * (uint32_t)(frame + 1));
  h = mix32(h ^ 0xC2B2AE35U * (uint32_t)(step + 1));
  h = mix32(h ^ 0x27D4EB2FU * (uint32_t)(col + 1));
  return ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f);
}

struct ArgmaxScratch {  // LDS of one call; a workgroup that makes several calls gives each its own (no barrier in between needed)
  Top2 sh[4];
  Top2 sh2[4];
  int id;
};

// ---- per-request filters of a sampled row (SmolttsSlotFilters, include/smoltts_hip.h; host model: smoltts_amd/sampling.py) ----
// Order: repetition penalty -> top_k -> top_p -> min_p -> Gumbel key.  Both thresholds are found by bisection over an
// order-preserving integer image of the floats (32 rounds for top_k over the penalised logits, 31 for top_p over -z >= 0), one
// workgroup reduction per round.  Every reduced value is an exact integer (counts; masses quantised to multiples of 2^-40 and
// summed in fp64, exact up to 2^53), so the sums do not depend on the order, the lane or the launch geometry.
struct FilterScratch {  // LDS of the filter rounds: two slots used in turn, so that one barrier per round is enough
  double m[2][4];
  int c[2][4];
};

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true); }
template <bool ROWS32>
__device__ __forceinline__ uint32_t swap_u32(uint32_t x, int lane) {  // the value of lane ^ 16 (ROWS32: lane ^ 32), as top2_swap
  const bool upper = (lane & (ROWS32 ? 32 : 16)) != 0;
  if (ROWS32) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return upper ? r[0] : r[1];
  }
  const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
  return upper ? r[0] : r[1];
}
// Wave sums on the VALU (the butterfly of cand_pick_wave): every lane returns the total.
__device__ __forceinline__ int wave_sum_i32(int x, int lane) {
  x += (int)dpp_u32<0xB1>(x);
  x += (int)dpp_u32<0x4E>(x);
  x += (int)dpp_u32<0x141>(x);
  x += (int)dpp_u32<0x140>(x);
  x += (int)swap_u32<false>(x, lane);
  x += (int)swap_u32<true>(x, lane);
  return x;
}
#define ST_F64_STEP(FETCH)                                                         \
  {                                                                                \
    const uint64_t b_ = (uint64_t)__double_as_longlong(x);                         \
    const uint32_t lo_ = FETCH((uint32_t)b_), hi_ = FETCH((uint32_t)(b_ >> 32));   \
    x += __longlong_as_double((long long)(((uint64_t)hi_ << 32) | lo_));           \
  }
__device__ __forceinline__ double wave_sum_f64(double x, int lane) {  // exact for the integer-valued masses: any order gives the same bits
#define ST_SWAP16(V) swap_u32<false>((V), lane)
#define ST_SWAP32(V) swap_u32<true>((V), lane)
  ST_F64_STEP(dpp_u32<0xB1>)
  ST_F64_STEP(dpp_u32<0x4E>)
  ST_F64_STEP(dpp_u32<0x141>)
  ST_F64_STEP(dpp_u32<0x140>)
  ST_F64_STEP(ST_SWAP16)
  ST_F64_STEP(ST_SWAP32)
#undef ST_SWAP16
#undef ST_SWAP32
  return x;
}
#undef ST_F64_STEP
__device__ __forceinline__ int wg_sum_i32(int x, FilterScratch& F, int round, int lane, int wave) {
  x = wave_sum_i32(x, lane);
  int* sh = F.c[round & 1];
  if (lane == 0) sh[wave] = x;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ double wg_sum_f64(double x, FilterScratch& F, int round, int lane, int wave) {
  x = wave_sum_f64(x, lane);
  double* sh = F.m[round & 1];
  if (lane == 0) sh[wave] = x;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// Order-preserving image of a float (a > b <=> ord_key(a) > ord_key(b); -0 and +0 share one key)
__device__ __forceinline__ uint32_t ord_key(float x) {
  uint32_t b = __float_as_uint(x);
  if (x == 0.f) b = 0;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
// z <= 0 -> the bits of -z (sign cleared: one image for both zeros): a smaller image is a larger z
__device__ __forceinline__ uint32_t nz_bits(float z) { return __float_as_uint(z) & 0x7FFFFFFFu; }
// mass of a column: exp(z) rounded down to a multiple of 2^-40, held as the integer it is a multiple of (exact in fp32)
__device__ __forceinline__ float mass_q(float z) { return floorf(expf(z) * 0x1p40f); }
__device__ __forceinline__ float penalised(float x, float r, float inv_r) { return x > 0.f ? x * inv_r : x * r; }

// LDS of the SCORE pass of one call: the waves' partial mass sums and the picked column's z (sampled rows)
struct ScoreScratch {
  double m[4];
  float z;
};

// One workgroup of exactly 256 threads picks the id of logits row `row` (n_cols entries); every thread returns it.
// `r`: the row's index into margin / margin_mask / the sampling arrays.  Greedy rows update margin[r] / margin_at[r].
// FILTERS: the instantiation that reads sa.filters (slot mode's sampled forms; `F` is its LDS).  A row whose entry is off, and
// every greedy row, takes one uniform branch and then the instructions of the plain instantiation.
// LENGTH: the instantiation that reads sa.length (slot mode's forms with a length entry on; SmolttsSlotLength, host model
// smoltts_amd/sampling.py length_patch).  At step 0 the row's im_end column gets the entry's bias (one rounded fp32 add) and, while
// the row's frame counter is below min_frames, -inf -- as the value is read, in front of the penalty, so greedy and sampled picks,
// every filter and the top-2 gap see the patched row.  The row always has other finite columns: its maximum stays finite, a -inf
// column gives z = -inf, mass 0 and key -inf and is never picked.  A row whose entry is off takes one uniform branch.
// SCORE: the instantiation that also gives the log-probability, at temperature 1, of the id it returns under the row as the pick
// sees it (after the length entry and the penalty, before temperature, top_k, top_p and min_p; host model smoltts_amd/sampling.py
// pick_logprob): z_j = fp32(x'_j - max x'), q_j = mass_q(z_j), S = sum q_j (exact in fp64 in any order), lp = z_picked -
// (log S - 40 ln 2).  One more pass over the row behind the top-2 merge and one workgroup sum on `C`; a sampled row carries its z
// beside the winning key.  Thread 0 computes the value and gets it in *lp_out.  The pass reads and writes nothing the pick uses:
// the id is the one the other instantiations return.
template <bool FILTERS = false, bool LENGTH = false, bool SCORE = false>
__device__ __forceinline__ int argmax_row(const float* row, int n_cols, bool ld_vec, int r, float* margin, const int* margin_mask,
                                          const SampleArgs& sa, ArgmaxScratch& S, FilterScratch* F = nullptr, ScoreScratch* C = nullptr,
                                          float* lp_out = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the row's sampling parameters (uniform in the workgroup: scalar loads, no divergence)
  float temp = sa.temp, min_p = sa.min_p;
  uint64_t seed = sa.seed;
  int key_slot = r;
  if (sa.table) {
    const SmolttsSlotSampling en = sa.table[r];
    temp = sa.step == 0 ? en.temp : en.fast_temp;
    min_p = temp > 0.f ? en.min_p : 0.f;
    seed = en.seed;
    key_slot = 0;
  }
  const bool vec = (n_cols & 3) == 0 && ld_vec && n_cols <= 8 * 1024;
  // the row's length entry (uniform): lcol = the patched column, or -1 (off, or not the slow pick)
  int lcol = -1;
  float lbias = 0.f;
  bool lblock = false;
  if constexpr (LENGTH) {
    if (sa.length && sa.step == 0 && (unsigned)sa.im_end < (unsigned)n_cols) {
      const SmolttsSlotLength le = sa.length[r];
      lblock = (sa.frames ? sa.frames[r] : sa.frame_base + r) < le.min_frames;
      lbias = le.eos_bias;
      if (lblock || lbias != 0.f) lcol = sa.im_end;
    }
  }
  // scalar paths: the value of column J as the pick sees it
#define ST_LFIX(X, J) ((LENGTH && (J) == lcol) ? (lblock ? -INFINITY : (X) + lbias) : (X))
  // the row's filters (uniform).  History id h sits in lane h of every wave: the loops over it read it with v_readlane.
  int top_k = 0, hn = 0, hid = -1;
  float top_p = 0.f, pen = 1.f, inv_pen = 1.f;
  bool fon = false;
  uint32_t vmask = 0;                      // vector path: bit i * 4 + c = column tid * 4 + i * 1024 + c is in the history
  uint64_t pm0 = 0, pm1 = 0, pm2 = 0, pm3 = 0;  // scalar path: bit c of pm[g] = column tid + 256 * (g * 64 + c) is
  if constexpr (FILTERS) {
    if (sa.filters && temp > 0.f) {
      const SmolttsSlotFilters fe = sa.filters[r];
      top_k = fe.top_k > 0 && fe.top_k < n_cols ? fe.top_k : 0;
      top_p = fe.top_p > 0.f && fe.top_p < 1.f ? fe.top_p : 0.f;
      if (fe.penalty > 1.f && fe.window > 0 && sa.hist) {
        const int w = fe.window < 64 ? fe.window : 64;
        int f = 0;
        if (sa.hist_len) {
          hn = sa.hist_len[r];
        } else {
          f = sa.frames ? sa.frames[r] : 0;
          hn = f < sa.hist_frames ? f : sa.hist_frames;
        }
        hn = hn < w ? hn : w;
        if (hn < 0) hn = 0;
        if (lane < hn) hid = sa.hist[(long)r * sa.hist_slot_stride + (long)(sa.hist_len ? lane : f - 1 - lane) * sa.hist_frame_stride];
        pen = fe.penalty; inv_pen = fe.inv_penalty;
        for (int h = 0; h < hn; ++h) {
          const int id = __builtin_amdgcn_readlane(hid, h);
          if ((unsigned)id >= (unsigned)n_cols) continue;
          if (vec) {
            if (((id >> 2) & 255) == tid) vmask |= 1u << (((id >> 10) << 2) | (id & 3));
          } else if ((id & 255) == tid) {
            const int c = id >> 8;
            if ((c >> 6) == 0) pm0 |= 1ull << (c & 63);
            if ((c >> 6) == 1) pm1 |= 1ull << (c & 63);
            if ((c >> 6) == 2) pm2 |= 1ull << (c & 63);
            if ((c >> 6) == 3) pm3 |= 1ull << (c & 63);
          }
        }
      }
      fon = top_k > 0 || top_p > 0.f || hn > 0;
    }
  }
  // scalar path of a filtered row: BODY(value after the penalty, column), columns ascending within a thread
#define ST_SGROUP(PM, G, BODY)                                          \
  for (int c_ = 0; c_ < 64; ++c_) {                                     \
    const int j_ = tid + 256 * ((G) * 64 + c_);                         \
    if (j_ >= n_cols) break;                                            \
    float x_ = row[j_];                                                 \
    x_ = ST_LFIX(x_, j_);                                               \
    if (((PM) >> c_) & 1) x_ = penalised(x_, pen, inv_pen);             \
    BODY(x_, j_)                                                        \
  }
#define ST_SCOLS(BODY)                                                                       \
  {                                                                                          \
    ST_SGROUP(pm0, 0, BODY) ST_SGROUP(pm1, 1, BODY) ST_SGROUP(pm2, 2, BODY) ST_SGROUP(pm3, 3, BODY) \
    for (int j_ = tid + 65536; j_ < n_cols; j_ += 256) {                                     \
      float x_ = row[j_];                                                                    \
      x_ = ST_LFIX(x_, j_);                                                                  \
      bool hit_ = false;                                                                     \
      for (int h_ = 0; h_ < hn; ++h_) hit_ |= __builtin_amdgcn_readlane(hid, h_) == j_;      \
      if (hit_) x_ = penalised(x_, pen, inv_pen);                                            \
      BODY(x_, j_)                                                                           \
    }                                                                                        \
  }
  Top2 t{-INFINITY, 0x7fffffff, -INFINITY};
#define ST_TAKE(V, J)                                                                               \
  {                                                                                                 \
    const float v_ = (V);                                                                           \
    if (v_ > t.v1) { /* strictly greater keeps the earliest index inside a thread (j ascending) */ \
      t.v2 = t.v1; t.v1 = v_; t.i1 = (J);                                                           \
    } else if (v_ > t.v2) {                                                                         \
      t.v2 = v_;                                                                                    \
    }                                                                                               \
  }
  // the whole row in one round trip: up to 8 float4 per thread, all requested before the first compare (a scalar loop is a
  // chain of n_cols / 256 dependent L2 latencies: 8 for a 2048-entry codebook); kept for the sampling pass
  float4 v[8];
  if (vec) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = tid * 4 + i * 1024;
      v[i] = j < n_cols ? *reinterpret_cast<const float4*>(row + j) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    }
    if constexpr (LENGTH) {
      if (lcol >= 0 && ((lcol >> 2) & 255) == tid) {  // the length entry, patched into the one row register that holds im_end
        const uint32_t lmask = 1u << (((lcol >> 10) << 2) | (lcol & 3));
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if ((lmask >> (i * 4)) & 1) v[i].x = lblock ? -INFINITY : v[i].x + lbias;
          if ((lmask >> (i * 4 + 1)) & 1) v[i].y = lblock ? -INFINITY : v[i].y + lbias;
          if ((lmask >> (i * 4 + 2)) & 1) v[i].z = lblock ? -INFINITY : v[i].z + lbias;
          if ((lmask >> (i * 4 + 3)) & 1) v[i].w = lblock ? -INFINITY : v[i].w + lbias;
        }
      }
    }
    if constexpr (FILTERS) {
      if (vmask) {  // the penalty, patched into the row registers before the first pass
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if ((vmask >> (i * 4)) & 1) v[i].x = penalised(v[i].x, pen, inv_pen);
          if ((vmask >> (i * 4 + 1)) & 1) v[i].y = penalised(v[i].y, pen, inv_pen);
          if ((vmask >> (i * 4 + 2)) & 1) v[i].z = penalised(v[i].z, pen, inv_pen);
          if ((vmask >> (i * 4 + 3)) & 1) v[i].w = penalised(v[i].w, pen, inv_pen);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = tid * 4 + i * 1024;
      if (j < n_cols) { ST_TAKE(v[i].x, j) ST_TAKE(v[i].y, j + 1) ST_TAKE(v[i].z, j + 2) ST_TAKE(v[i].w, j + 3) }
    }
  } else if (FILTERS && fon) {
    ST_SCOLS(ST_TAKE)
  } else {
    for (int j = tid; j < n_cols; j += 256) ST_TAKE(ST_LFIX(row[j], j), j)
  }
#undef ST_TAKE
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Top2 b;
    b.v1 = __shfl_xor(t.v1, o); b.i1 = __shfl_xor(t.i1, o); b.v2 = __shfl_xor(t.v2, o);
    t = top2_merge(t, b);
  }
  if (lane == 0) S.sh[wave] = t;
  __syncthreads();
  Top2 a = top2_merge(top2_merge(S.sh[0], S.sh[1]), top2_merge(S.sh[2], S.sh[3]));
  double score_s = 0.0;  // SCORE: the row's total mass at temperature 1, in units of 2^-40
  float score_z = 0.f;   // ... and the picked column's z (a greedy pick is the maximum: 0)
  if constexpr (SCORE) {  // before top_k takes its columns out of the row registers
    double m = 0.0;
#define ST_SUM(V, J) m += (double)mass_q((V) - a.v1);
    if (vec) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { ST_SUM(v[i].x, 0) ST_SUM(v[i].y, 0) ST_SUM(v[i].z, 0) ST_SUM(v[i].w, 0) }  // (an absent column is -inf: mass 0)
    } else if (FILTERS && fon) {
      ST_SCOLS(ST_SUM)
    } else {
      for (int j = tid; j < n_cols; j += 256) ST_SUM(ST_LFIX(row[j], j), j)
    }
#undef ST_SUM
    m = wave_sum_f64(m, lane);
    if (lane == 0) C->m[wave] = m;
    __syncthreads();
    score_s = (C->m[0] + C->m[1]) + (C->m[2] + C->m[3]);
  }
  if (temp > 0.f) {  // uniform: second pass over the row with perturbed keys
    const int frame = sa.frames ? sa.frames[r] : sa.frame_base + r;
    if (!sa.table && sa.salt) seed += 0x9E3779B97F4A7C15ULL * (uint64_t)sa.salt[r];
    const float inv_t = 1.0f / temp;
    const float cut = min_p > 0.f ? logf(min_p) : -INFINITY;
    // the filters' thresholds: a column stays iff ord_key(x') >= tk (top_k) and nz_bits(z) <= wu (top_p)
    uint32_t tk = 0, wu = 0x7FFFFFFFu;
    if constexpr (FILTERS) {
      int round = 0;
      if (top_k > 0) {  // tk = the image of the k-th largest value: the largest image that at least k columns reach
        for (int bit = 31; bit >= 0; --bit) {
          const uint32_t cand = tk | (1u << bit);
          int c = 0;
#define ST_CNT(V, J) c += ord_key(V) >= cand;
          if (vec) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              if (tid * 4 + i * 1024 < n_cols) { ST_CNT(v[i].x, 0) ST_CNT(v[i].y, 0) ST_CNT(v[i].z, 0) ST_CNT(v[i].w, 0) }
            }
          } else {
            ST_SCOLS(ST_CNT)
          }
#undef ST_CNT
          if (wg_sum_i32(c, *F, round++, lane, wave) >= top_k) tk = cand;
        }
        if (vec) {  // the columns top_k removes leave the row registers
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            if (ord_key(v[i].x) < tk) v[i].x = -INFINITY;
            if (ord_key(v[i].y) < tk) v[i].y = -INFINITY;
            if (ord_key(v[i].z) < tk) v[i].z = -INFINITY;
            if (ord_key(v[i].w) < tk) v[i].w = -INFINITY;
          }
        }
      }
      if (top_p > 0.f) {  // wu = the largest image whose strictly-more-probable mass is below top_p * total
        float fq[32];     // vector path: the columns' masses (an absent column's is 0)
        double s = 0.0;
#define ST_MASS(V, J) if (ord_key(V) >= tk) s += (double)mass_q(((V) - a.v1) * inv_t);
        if (vec) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            fq[i * 4] = mass_q((v[i].x - a.v1) * inv_t); fq[i * 4 + 1] = mass_q((v[i].y - a.v1) * inv_t);
            fq[i * 4 + 2] = mass_q((v[i].z - a.v1) * inv_t); fq[i * 4 + 3] = mass_q((v[i].w - a.v1) * inv_t);
            s += ((double)fq[i * 4] + (double)fq[i * 4 + 1]) + ((double)fq[i * 4 + 2] + (double)fq[i * 4 + 3]);
          }
        } else {
          ST_SCOLS(ST_MASS)
        }
#undef ST_MASS
        const double P = (double)top_p * wg_sum_f64(s, *F, round++, lane, wave);
        wu = 0;
        for (int bit = 30; bit >= 0; --bit) {
          const uint32_t cand = wu | (1u << bit);
          double m = 0.0;
#define ST_ABOVE(V, Q) if (nz_bits(((V) - a.v1) * inv_t) < cand) m += (double)(Q);
#define ST_ABOVE_S(V, J) if (ord_key(V) >= tk) ST_ABOVE(V, mass_q(((V) - a.v1) * inv_t))
          if (vec) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              ST_ABOVE(v[i].x, fq[i * 4]) ST_ABOVE(v[i].y, fq[i * 4 + 1]) ST_ABOVE(v[i].z, fq[i * 4 + 2]) ST_ABOVE(v[i].w, fq[i * 4 + 3])
            }
          } else {
            ST_SCOLS(ST_ABOVE_S)
          }
#undef ST_ABOVE_S
#undef ST_ABOVE
          if (wg_sum_f64(m, *F, round++, lane, wave) < P) wu = cand;
        }
      }
    }
    Top2 k{-INFINITY, 0x7fffffff, -INFINITY};
    float kz = 0.f;  // SCORE: x' - max of this thread's best column
#define ST_KEY(V, J)                                                  \
  {                                                                   \
    const float z = ((V) - a.v1) * inv_t; /* <= 0 */                  \
    if (z >= cut && (!FILTERS || nz_bits(z) <= wu)) {                 \
      const float u = uniform01(seed, key_slot, frame, sa.step, (J)); \
      const float key = z - logf(-logf(u));                           \
      if (key > k.v1) {                                               \
        k.v1 = key; k.i1 = (J);                                       \
        if constexpr (SCORE) kz = (V) - a.v1;                         \
      }                                                               \
    }                                                                 \
  }
#define ST_KEY_S(V, J) if (ord_key(V) >= tk) ST_KEY(V, J)
    if (vec) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = tid * 4 + i * 1024;
        if (j < n_cols) { ST_KEY(v[i].x, j) ST_KEY(v[i].y, j + 1) ST_KEY(v[i].z, j + 2) ST_KEY(v[i].w, j + 3) }
      }
    } else if (FILTERS && fon) {
      ST_SCOLS(ST_KEY_S)
    } else {
      for (int j = tid; j < n_cols; j += 256) ST_KEY(ST_LFIX(row[j], j), j)
    }
#undef ST_KEY_S
#undef ST_KEY
    const int ki = k.i1;  // this thread's own best column (columns belong to one thread each)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      Top2 b;
      b.v1 = __shfl_xor(k.v1, o); b.i1 = __shfl_xor(k.i1, o); b.v2 = -INFINITY;
      k = top2_merge(k, b);
    }
    if (lane == 0) S.sh2[wave] = k;
    __syncthreads();
    const Top2 w = top2_merge(top2_merge(S.sh2[0], S.sh2[1]), top2_merge(S.sh2[2], S.sh2[3]));
    a.i1 = w.i1;
    if constexpr (SCORE) {  // the winner's owner hands its z over
      if (ki == w.i1) C->z = kz;
      __syncthreads();
      score_z = C->z;
    }
  }
#undef ST_SCOLS
#undef ST_SGROUP
#undef ST_LFIX
  if (a.i1 < 0 || a.i1 >= n_cols) a.i1 = 0;  // all-NaN row: stay inside the tables
  if (tid == 0) {
    if (temp <= 0.f && margin && (margin_mask == nullptr || margin_mask[r])) {
      const float gap = a.v1 - a.v2;
      if (gap < margin[r]) {  // also remember where the slot's smallest gap occurred: frame * 64 + step (0 = slow id)
        margin[r] = gap;
        if (sa.margin_at) sa.margin_at[r] = (sa.frames ? sa.frames[r] : sa.frame_base + r) * 64 + sa.step;
      }
    }
  }
  if constexpr (SCORE)
    if (tid == 0) *lp_out = (float)((double)score_z - (log(score_s) - 40.0 * 0.6931471805599453094));
  return a.i1;  // the same value in every thread (merged from LDS)
}

// The picked id of one row from the head GEMM's tile candidates (SmolttsGemm3Args.cand_out_dev layout), by a whole wave: every lane returns it.
// The merge across lanes stays on the VALU (DPP inside 16-lane rows, v_permlane16/32_swap across them): six dependent
// ds_bpermute round trips per row -- what __shfl_xor compiles to -- were most of what the pick added to the launch.
template <int CTRL>
__device__ __forceinline__ Top2 top2_dpp(Top2 t) {
  Top2 b;
  b.v1 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t.v1), CTRL, 0xF, 0xF, true));
  b.i1 = __builtin_amdgcn_update_dpp(0, t.i1, CTRL, 0xF, 0xF, true);
  b.v2 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t.v2), CTRL, 0xF, 0xF, true));
  return top2_merge(t, b);
}
template <bool ROWS32>
__device__ __forceinline__ Top2 top2_swap(Top2 t, int lane) {  // partner = lane ^ 16 (ROWS32: lane ^ 32)
  const unsigned a[3] = {__float_as_uint(t.v1), (unsigned)t.i1, __float_as_uint(t.v2)};
  unsigned o[3];
  const bool upper = (lane & (ROWS32 ? 32 : 16)) != 0;  // after swap(x, x): the lower lane's partner value is result 1, the upper's result 0
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (ROWS32) {
      const auto r = __builtin_amdgcn_permlane32_swap(a[i], a[i], false, false);
      o[i] = upper ? r[0] : r[1];
    } else {
      const auto r = __builtin_amdgcn_permlane16_swap(a[i], a[i], false, false);
      o[i] = upper ? r[0] : r[1];
    }
  }
  return top2_merge(t, Top2{__uint_as_float(o[0]), (int)o[1], __uint_as_float(o[2])});
}
__device__ __forceinline__ Top2 cand_pick_wave(const float* cand, int tiles, int lane) {
  Top2 t{-INFINITY, 0x7fffffff, -INFINITY};
  for (int j = lane; j < tiles; j += 64) {
    const float4 c = *reinterpret_cast<const float4*>(cand + (size_t)j * 4);
    t = top2_merge(t, Top2{c.x, __float_as_int(c.y), c.z});
  }
  t = top2_dpp<0xB1>(t);   // lane ^ 1
  t = top2_dpp<0x4E>(t);   // lane ^ 2
  t = top2_dpp<0x141>(t);  // the other quad of the half row
  t = top2_dpp<0x140>(t);  // the other half row
  t = top2_swap<false>(t, lane);
  t = top2_swap<true>(t, lane);
  return t;
}

// Projections of a depth-transformer input row that are known before the row is: row e of the fast embedding table always
// enters layer 0 as RMSNorm(E[e]) -> wqkv, so q | k | v (before RoPE) are a table lookup [rows][nqkv] instead of a GEMM launch
// (smoltts_engine_build_fast_qkv).  The kernel that picks the code gathers them, applies RoPE for the row's position and writes
// q and the depth cache rows exactly as the wqkv GEMM's epilogue would (gemm3.hip EPI_QKV_ROPE).
struct QkvGather {
  const float* table;   // [emb rows][nqkv] fp32, pre-RoPE; nullptr = off
  const float* rope;    // fp32 [pos][32][2]
  float* q_out;         // [rows][n_q_heads * 64]
  float* kc;            // depth cache of layer 0: [slot][kv head][cache_len][64]
  float* vc;
  int n_q_heads, n_kv_heads, cache_len, pos;
};

// The row's q | k | v: loaded by `qkv_gather_load` (up to QG_MAX float4 per thread, all requested at once, together with the RoPE
// rows they need -- a loop over the row would be one dependent L2 round trip per iteration), finished by `qkv_gather_store`.
// RoPE of the two (even, odd) pairs of a float4 of table values: rounded products, rounded sums (no contraction) -- the one
// place that defines these bits, shared by the picking kernel's gather (small_ops.hip) and by the pick inside the attention + wo
// launch (gemm3.hip attn_wo_kernel), which must publish the same q / K rows.
__device__ __forceinline__ float4 rope_gathered4(float4 v, float4 cs) {
#pragma clang fp contract(off)
  const float o0 = v.x * cs.x - v.y * cs.y, o1 = v.y * cs.x + v.x * cs.y;
  const float o2 = v.z * cs.z - v.w * cs.w, o3 = v.w * cs.z + v.z * cs.w;
  return make_float4(o0, o1, o2, o3);
}

constexpr int QG_MAX = 2;  // 256 threads x 2 x 4 floats = rows of up to 2048 values (150m: 1280); longer rows take more rounds
struct QkvRegs { float4 v[QG_MAX], cs[QG_MAX]; };

__device__ __forceinline__ void qkv_gather_load(const QkvGather& g, long erow, int base, QkvRegs& o) {
  const int qd = g.n_q_heads * 64, kd = g.n_kv_heads * 64, nqkv = qd + 2 * kd;
  const float* trow = g.table + erow * nqkv;
#pragma unroll
  for (int i = 0; i < QG_MAX; ++i) {
    const int n0 = base + (threadIdx.x + i * 256) * 4;
    o.v[i] = n0 < nqkv ? *reinterpret_cast<const float4*>(trow + n0) : make_float4(0.f, 0.f, 0.f, 0.f);
    o.cs[i] = n0 < qd + kd ? *reinterpret_cast<const float4*>(g.rope + ((long)g.pos * 32 + ((n0 & 63) >> 1)) * 2) : make_float4(1.f, 0.f, 1.f, 0.f);
  }
}

__device__ __forceinline__ void qkv_gather_store(const QkvGather& g, int r, int base, const QkvRegs& in) {
  const int qd = g.n_q_heads * 64, kd = g.n_kv_heads * 64, nqkv = qd + 2 * kd;
#pragma unroll
  for (int i = 0; i < QG_MAX; ++i) {
    const int n0 = base + (threadIdx.x + i * 256) * 4;
    if (n0 >= nqkv) continue;
    float4 v = in.v[i];
    if (n0 < qd + kd) v = rope_gathered4(v, in.cs[i]);
    if (n0 < qd) {
      *reinterpret_cast<float4*>(g.q_out + (long)r * qd + n0) = v;
    } else {
      const int nn = n0 - qd;
      float* dst = nn < kd ? g.kc : g.vc;
      const int h = (nn < kd ? nn : nn - kd) >> 6, d = nn & 63;
      *reinterpret_cast<float4*>(dst + (((long)r * g.n_kv_heads + h) * g.cache_len + g.pos) * 64 + d) = v;
    }
  }
}

}  // namespace smoltts

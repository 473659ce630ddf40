// FLAC framing of streamed speech: int16 samples (the resampler's output) or the codec's / stretcher's fp32 PCM -> FLAC frames,
// chunk by chunk, in one launch per pass over every slot (include/smoltts_hip.h, "FLAC"; the numpy model and
// parity oracle is smoltts_amd/flac.py).
//
// RFC 9639 streamable subset: mono, 16 bits, variable blocking (the coded number is the first sample's number), subframes
// CONSTANT / FIXED 0..4 with a partitioned Rice residual (method 00, p <= 8, k <= 14) / VERBATIM, fewest bits wins.  A slot
// holds back at most 15 samples; with 16 or more pending (or any at its last call) it emits all of them as m = ceil(P / 4096)
// blocks, the first P mod m one sample longer.
//
// One 256-lane workgroup per block.  For each FIXED order, lane t sums (u >> k), k = 0..14, over its share of a finest
// partition; a butterfly of those sums over lanes gives every coarser partition order (groups of 2^l lanes are the
// partitions of order 8 - l), where the group picks its k.  The winner is packed by an exclusive scan of per-sample code
// lengths and 32-bit atomicOr into a zeroed LDS bit buffer; its CRC-16 is the XOR of per-lane segment CRCs, each multiplied by
// x^(8 bytes behind the segment) mod 0x8005 (CRC with init 0 and no xorout is linear).
#include "stage.h"

using namespace smoltts;

namespace {

constexpr int kT = 256;            // lanes per workgroup
constexpr int kMaxN = 4096;        // samples per block
constexpr int kPer = kMaxN / kT;   // packing: samples per lane
constexpr int kHold = 15;          // samples a slot may hold back
constexpr int kSlack = 20;         // a frame of n samples takes at most 2 n + 17 bytes (14 header, 1 subframe header, 2 CRC)
constexpr int kWords = 2056;       // bit buffer: 8 * 14 + 8 + 16 * 4096 bits, plus the word a last write may touch
constexpr int kK = 15;             // Rice parameters 0..14
constexpr int kRates = 6;

struct RateCode { int rate, code; };
constexpr RateCode kRateCodes[kRates] = {{8000, 4}, {16000, 5}, {22050, 6}, {24000, 7}, {44100, 9}, {48000, 10}};

struct FlacCfg {    // device copy, per slot
  int32_t src;      // SMOLTTS_FLAC_OFF / _F32 / _S16
  int32_t rate_code;
};

struct FlacState {  // one half of the ping-pong pair, per slot
  int64_t pos;      // sample number of the first pending sample
  int32_t npend;    // pending samples (<= 15)
  int32_t pad;
  int16_t pend[16];
};

constexpr uint16_t mulmod_c(uint16_t a, uint16_t b) {
  uint32_t r = 0;
  for (int i = 15; i >= 0; --i) {
    r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
    if ((b >> i) & 1) r ^= a;
  }
  return (uint16_t)r;
}
// x^(8 2^j) mod 0x8005, j = 0..13 (a frame has fewer than 2^14 bytes)
constexpr uint16_t kP0 = 0x0100, kP1 = mulmod_c(kP0, kP0), kP2 = mulmod_c(kP1, kP1), kP3 = mulmod_c(kP2, kP2),
                   kP4 = mulmod_c(kP3, kP3), kP5 = mulmod_c(kP4, kP4), kP6 = mulmod_c(kP5, kP5), kP7 = mulmod_c(kP6, kP6),
                   kP8 = mulmod_c(kP7, kP7), kP9 = mulmod_c(kP8, kP8), kP10 = mulmod_c(kP9, kP9), kP11 = mulmod_c(kP10, kP10),
                   kP12 = mulmod_c(kP11, kP11), kP13 = mulmod_c(kP12, kP12);

__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 15; i >= 0; --i) {
    r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}

__device__ __forceinline__ uint32_t xpow8(uint32_t m) {  // x^(8 m) mod 0x8005
  const uint32_t p[14] = {kP0, kP1, kP2, kP3, kP4, kP5, kP6, kP7, kP8, kP9, kP10, kP11, kP12, kP13};
  uint32_t acc = 1;
#pragma unroll
  for (int j = 0; j < 14; ++j)
    if ((m >> j) & 1u) acc = mulmod(acc, p[j]);
  return acc;
}

__device__ __forceinline__ int to_q(float v) {  // fp32, as numpy: rint(clip(x, -1, 1) * 32767)
  return __float2int_rn(fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f);
}

__device__ __forceinline__ uint32_t zig(int r) { return r >= 0 ? (uint32_t)r << 1 : ((uint32_t)(-r) << 1) - 1u; }

__device__ __forceinline__ int fixed_res(const int32_t* x, int i, int o) {
  switch (o) {
    case 0: return x[i];
    case 1: return x[i] - x[i - 1];
    case 2: return x[i] - 2 * x[i - 1] + x[i - 2];
    case 3: return x[i] - 3 * x[i - 1] + 3 * x[i - 2] - x[i - 3];
    default: return x[i] - 4 * x[i - 1] + 6 * x[i - 2] - 4 * x[i - 3] + x[i - 4];
  }
}

// OR `width` (<= 25) bits of `v` into the big-endian bit buffer at bit `pos`
__device__ __forceinline__ void put_bits(uint32_t* buf, int pos, uint32_t v, int width) {
  const uint64_t sh = (uint64_t)(v & ((1u << width) - 1u)) << (64 - width - (pos & 31));
  const int w = pos >> 5;
  const uint32_t hi = (uint32_t)(sh >> 32), lo = (uint32_t)sh;
  if (hi) atomicOr(&buf[w], hi);
  if (lo) atomicOr(&buf[w + 1], lo);
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// header bytes of a frame: 4 fixed, the coded sample number (1..7), the block size extension (0..2), CRC-8
__device__ __forceinline__ int utf8_len(uint64_t v) {
  return v < 0x80 ? 1 : v < (1ull << 11) ? 2 : v < (1ull << 16) ? 3 : v < (1ull << 21) ? 4 : v < (1ull << 26) ? 5 : v < (1ull << 31) ? 6 : 7;
}
__device__ __forceinline__ int block_code(int n) {
  switch (n) {
    case 192: return 1;
    case 576: return 2;
    case 1152: return 3;
    case 2304: return 4;
    case 256: return 8;
    case 512: return 9;
    case 1024: return 10;
    case 2048: return 11;
    case 4096: return 12;
    default: return n <= 256 ? 6 : 7;
  }
}
__device__ __forceinline__ int header_bytes(uint64_t first, int n) {
  const int c = block_code(n);
  return 4 + utf8_len(first) + (c == 6 ? 1 : c == 7 ? 2 : 0) + 1;
}

__device__ __forceinline__ uint32_t crc8_byte(uint32_t crc, uint32_t byte) {
  crc ^= byte;
#pragma unroll
  for (int i = 0; i < 8; ++i) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xFFu : (crc << 1) & 0xFFu;
  return crc;
}

// lane 0: the frame header at bit 0 of the buffer
__device__ void write_header(uint32_t* buf, uint64_t first, int n, int rate_code) {
  const int c = block_code(n);
  uint32_t crc = 0;
  int pos = 0;
  auto byte = [&](uint32_t v) {
    put_bits(buf, pos, v, 8);
    crc = crc8_byte(crc, v);
    pos += 8;
  };
  byte(0xFF);
  byte(0xF9);
  byte((uint32_t)(c << 4 | rate_code));
  byte(0x08);  // mono, 16 bits, reserved 0
  const int nb = utf8_len(first);
  if (nb == 1) {
    byte((uint32_t)first);
  } else {
    const uint32_t lead = nb < 7 ? (((0xFFu << (8 - nb)) & 0xFFu) | (uint32_t)(first >> (6 * (nb - 1)))) : 0xFEu;
    byte(lead);
    for (int i = nb - 2; i >= 0; --i) byte(0x80u | (uint32_t)((first >> (6 * i)) & 0x3F));
  }
  if (c == 6) byte((uint32_t)(n - 1));
  if (c == 7) {
    byte((uint32_t)((n - 1) >> 8));
    byte((uint32_t)((n - 1) & 0xFF));
  }
  put_bits(buf, pos, crc, 8);
}

// grid (max blocks, max_batch), 256 lanes: workgroup (j, b) encodes block j of what slot b emits in this call; workgroup (0, b)
// also writes the slot's next state.  States ping-pong between st_in and st_out (the host alternates them), so no workgroup reads
// what another one writes in the same launch; slots at or past `batch` only carry their state across.  Block j of slot b goes to
// out[b] at byte 2 s_j + kSlack j (s_j its first pending-sample index) and sizes[b][j] = {offset, bytes}; {0, 0} past the last.
__global__ __launch_bounds__(kT) void flac_kernel(const float* __restrict__ pcm, int64_t pcm_stride, int n_in,
                                                  const int32_t* __restrict__ valid, const uint8_t* __restrict__ s16,
                                                  int64_t s16_stride, const int32_t* __restrict__ s16_counts, int batch,
                                                  const int32_t* __restrict__ last, const FlacCfg* __restrict__ cfgs,
                                                  const FlacState* __restrict__ st_in, FlacState* __restrict__ st_out,
                                                  uint8_t* __restrict__ out, int64_t out_stride, int32_t* __restrict__ sizes,
                                                  int max_blocks) {
  __shared__ int32_t xs[kMaxN];
  __shared__ uint32_t buf[kWords];
  __shared__ uint16_t crctab[256];
  __shared__ uint8_t kp[5][511];        // [order][(2^p - 1) + partition]: its Rice parameter
  __shared__ uint32_t wsum[4][kK];      // per wave: sum over the wave's lanes of (u >> k)
  __shared__ uint64_t wtot[4][9];       // per wave: bits of its partitions at order p
  __shared__ uint32_t wscan[4];
  __shared__ uint32_t wcrc[4];
  const int b = blockIdx.y, j = blockIdx.x, t = threadIdx.x, wv = t >> 6, ln = t & 63;
  const FlacCfg c = cfgs[b];
  const FlacState* si = st_in + b;
  const bool on = b < batch && c.src != SMOLTTS_FLAC_OFF;
  int n = 0;
  if (on) {
    if (c.src == SMOLTTS_FLAC_F32) {
      n = !pcm ? 0 : valid ? valid[b] : n_in;
      n = n < 0 ? 0 : (n > n_in ? n_in : n);
    } else if (s16 && s16_counts) {
      n = s16_counts[2 * b] + ((last && last[b]) ? s16_counts[2 * b + 1] : 0);
      const int cap = (int)(s16_stride / 2);
      n = n < 0 ? 0 : (n > cap ? cap : n);
    }
  }
  const bool lst = on && last && last[b] != 0;
  const int np = si->npend;
  const int P = np + n;
  const bool emit = on && (P > kHold || (lst && P > 0));
  const int m = emit ? (P + kMaxN - 1) / kMaxN : 0;
  const float* xf = pcm + (int64_t)(b < batch ? b : 0) * pcm_stride;
  const uint8_t* xh = s16 ? s16 + (int64_t)(b < batch ? b : 0) * s16_stride : nullptr;
  auto sample = [&](int e) -> int {  // pending-stream sample e (< P)
    if (e < np) return si->pend[e];
    e -= np;
    if (c.src == SMOLTTS_FLAC_F32) return to_q(xf[e]);
    return (int)(int16_t)(uint16_t)(xh[2 * e] | (xh[2 * e + 1] << 8));
  };
  if (j == 0) {
    FlacState* so = st_out + b;
    if (t < 16) so->pend[t] = (on && !emit) ? (t < P ? (int16_t)sample(t) : (int16_t)0) : (on ? (int16_t)0 : si->pend[t]);
    if (t == 0) {
      so->pos = si->pos + (emit ? P : 0);
      so->npend = on ? (emit ? 0 : P) : np;
      so->pad = 0;
    }
  }
  if (b >= batch || j >= max_blocks) return;
  if (j >= m) {
    if (t == 0) {
      sizes[2 * (b * max_blocks + j)] = 0;
      sizes[2 * (b * max_blocks + j) + 1] = 0;
    }
    return;
  }
  const int base = P / m, extra = P % m;
  const int nb = base + (j < extra ? 1 : 0);
  const int sj = j * base + (j < extra ? j : extra);
  const uint64_t first = (uint64_t)(si->pos + sj);
  for (int i = t; i < nb; i += kT) xs[i] = sample(sj + i);
  for (int i = t; i < kWords; i += kT) buf[i] = 0;
  {
    uint32_t r = (uint32_t)t << 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xFFFFu : (r << 1) & 0xFFFFu;
    crctab[t] = (uint16_t)r;
  }
  __syncthreads();
  int differs = 0;
  for (int i = t; i < nb; i += kT) differs |= xs[i] != xs[0];
  const bool all_equal = !__syncthreads_or(differs);

  // ---- FIXED orders: bits of the best partition order of each
  uint64_t cand[5];
  int cand_p[5];
  const int omax = nb - 1 < 4 ? nb - 1 : 4;
#pragma unroll
  for (int o = 0; o < 5; ++o) {
    cand[o] = ~0ull;
    cand_p[o] = 0;
    if (o > omax) continue;  // (uniform)
    int pmax = 0;
    while (pmax < 8 && nb % (2 << pmax) == 0 && (nb >> (pmax + 1)) > o) ++pmax;
    const int lg = 8 - pmax;                       // lanes per finest partition: 2^lg
    const int s = nb >> pmax, G = 1 << lg;
    const int cs = (s + G - 1) / G;
    const int q = t >> lg, g = t & (G - 1);
    int lo = q * s + g * cs, hi = lo + cs;
    if (hi > (q + 1) * s) hi = (q + 1) * s;
    if (lo < o) lo = o;
    uint32_t S[kK];
#pragma unroll
    for (int k = 0; k < kK; ++k) S[k] = 0;
    for (int i = lo; i < hi; ++i) {
      const uint32_t u = zig(fixed_res(xs, i, o));
#pragma unroll
      for (int k = 0; k < kK; ++k) S[k] += u >> k;
    }
    uint64_t tot[9];
#pragma unroll
    for (int p = 0; p < 9; ++p) tot[p] = 0;
#pragma unroll
    for (int l = 0; l <= 6; ++l) {
      if (l > 0) {
#pragma unroll
        for (int k = 0; k < kK; ++k) S[k] += __shfl_xor(S[k], 1 << (l - 1));
      }
      const int p = 8 - l;
      if (p <= pmax) {  // groups of 2^l lanes are the partitions of order p
        const int qp = t >> l;
        const uint64_t cnt = (uint64_t)((nb >> p) - (qp == 0 ? o : 0));
        uint64_t best = ~0ull;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < kK; ++k) {
          const uint64_t cost = 4 + cnt * (uint64_t)(k + 1) + S[k];
          if (cost < best) { best = cost; bk = k; }
        }
        if ((t & ((1 << l) - 1)) == 0) {
          kp[o][(1 << p) - 1 + qp] = (uint8_t)bk;
          tot[p] = best;
        }
      }
    }
#pragma unroll
    for (int p = 2; p < 9; ++p) {
      const uint64_t v = wave_sum64(tot[p]);
      if (ln == 0) wtot[wv][p] = v;
    }
    if (ln == 0) {
#pragma unroll
      for (int k = 0; k < kK; ++k) wsum[wv][k] = S[k];
    }
    __syncthreads();
    // partition orders 1 and 0 (groups of 128 and 256 lanes) and the choice of p: every lane, from the waves' sums
    uint64_t bestbits = ~0ull;
    int bestp = 0;
    for (int p = 0; p <= pmax; ++p) {
      uint64_t bits = 0;
      if (p >= 2) {
        bits = wtot[0][p] + wtot[1][p] + wtot[2][p] + wtot[3][p];
      } else {
        for (int qp = 0; qp < (1 << p); ++qp) {
          const uint64_t cnt = (uint64_t)((nb >> p) - (qp == 0 ? o : 0));
          uint64_t best = ~0ull;
          int bk = 0;
          for (int k = 0; k < kK; ++k) {
            const uint64_t sk = p == 0 ? (uint64_t)wsum[0][k] + wsum[1][k] + wsum[2][k] + wsum[3][k]
                                       : (uint64_t)wsum[2 * qp][k] + wsum[2 * qp + 1][k];
            const uint64_t cost = 4 + cnt * (uint64_t)(k + 1) + sk;
            if (cost < best) { best = cost; bk = k; }
          }
          if (t == 0) kp[o][(1 << p) - 1 + qp] = (uint8_t)bk;
          bits += best;
        }
      }
      if (bits < bestbits) { bestbits = bits; bestp = p; }
    }
    cand[o] = 8 + 16 * (uint64_t)o + 6 + bestbits;
    cand_p[o] = bestp;
    __syncthreads();  // (wsum / wtot are reused by the next order)
  }
  // ---- the choice: CONSTANT, FIXED 0..4, VERBATIM; ties in that order
  int kind = 2, ord = 0, pord = 0;
  uint64_t bestb = ~0ull;
  if (all_equal) { kind = 0; bestb = 24; }
#pragma unroll
  for (int o = 0; o < 5; ++o)
    if (cand[o] < bestb) { bestb = cand[o]; kind = 1; ord = o; pord = cand_p[o]; }
  if (8 + 16 * (uint64_t)nb < bestb) kind = 2;
  const int H = header_bytes(first, nb);
  // ---- packing: exclusive scan of the code lengths of samples [kPer t, kPer t + kPer)
  const int sp = nb >> pord;
  auto code_len = [&](int i) -> int {
    if (kind == 0) return i == 0 ? 16 : 0;
    if (kind == 2 || i < ord) return 16;
    const int q = i / sp;
    const int k = kp[ord][(1 << pord) - 1 + q];
    const uint32_t u = zig(fixed_res(xs, i, ord));
    const int start = q * sp > ord ? q * sp : ord;
    return (int)(u >> k) + 1 + k + (i == ord ? 6 : 0) + (i == start ? 4 : 0);
  };
  int mine = 0;
  for (int e = 0; e < kPer; ++e) {
    const int i = t * kPer + e;
    if (i < nb) mine += code_len(i);
  }
  int incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d);
    if (ln >= d) incl += v;
  }
  if (ln == 63) wscan[wv] = (uint32_t)incl;
  __syncthreads();
  int wbase = 0;
  for (int w = 0; w < wv; ++w) wbase += (int)wscan[w];
  const int total = (int)(wscan[0] + wscan[1] + wscan[2] + wscan[3]);
  const int sub0 = 8 * H + 8;
  int pos = sub0 + wbase + incl - mine;
  for (int e = 0; e < kPer; ++e) {
    const int i = t * kPer + e;
    if (i >= nb) break;
    if (kind == 0) {
      if (i == 0) put_bits(buf, pos, (uint32_t)(uint16_t)xs[0], 16);
    } else if (kind == 2 || i < ord) {
      put_bits(buf, pos, (uint32_t)(uint16_t)xs[i], 16);
    } else {
      const int q = i / sp;
      const int k = kp[ord][(1 << pord) - 1 + q];
      const uint32_t u = zig(fixed_res(xs, i, ord));
      const int start = q * sp > ord ? q * sp : ord;
      int at = pos;
      if (i == ord) { put_bits(buf, at, (uint32_t)pord, 6); at += 6; }
      if (i == start) { put_bits(buf, at, (uint32_t)k, 4); at += 4; }
      put_bits(buf, at + (int)(u >> k), (1u << k) | (u & ((1u << k) - 1u)), k + 1);
    }
    pos += code_len(i);
  }
  if (t == 0) {
    write_header(buf, first, nb, c.rate_code);
    const uint32_t type = kind == 0 ? 0u : kind == 2 ? 1u : (uint32_t)(8 + ord);
    put_bits(buf, 8 * H, type << 1, 8);
  }
  __syncthreads();
  // ---- bytes and CRC-16
  const int B = (sub0 + total + 7) / 8;
  const int64_t off = 2 * (int64_t)sj + (int64_t)kSlack * j;
  uint8_t* row = out + (int64_t)b * out_stride + off;
  auto byte_at = [&](int i) -> uint32_t { return (buf[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu; };
  for (int i = t; i < B; i += kT) row[i] = (uint8_t)byte_at(i);
  const int seg = (B + kT - 1) / kT;
  const int a = t * seg, e = a + seg < B ? a + seg : B;
  uint32_t crc = 0;
  for (int i = a; i < e; ++i) crc = ((crc << 8) & 0xFFFFu) ^ crctab[((crc >> 8) ^ byte_at(i)) & 0xFFu];
  uint32_t part = a < e ? mulmod(crc, xpow8((uint32_t)(B - e))) : 0u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) part ^= __shfl_xor(part, d);
  if (ln == 0) wcrc[wv] = part;
  __syncthreads();
  if (t == 0) {
    const uint32_t f = wcrc[0] ^ wcrc[1] ^ wcrc[2] ^ wcrc[3];
    row[B] = (uint8_t)(f >> 8);
    row[B + 1] = (uint8_t)(f & 0xFF);
    sizes[2 * (b * max_blocks + j)] = (int32_t)off;
    sizes[2 * (b * max_blocks + j) + 1] = B + 2;
  }
}

struct ResetArgs {
  int32_t n;
  int32_t slot[kResetMax];
  FlacCfg cfg[kResetMax];
};

// workgroup i: slot args.slot[i] gets its configuration and an empty stream in both state halves
__global__ __launch_bounds__(64) void flac_reset_kernel(ResetArgs a, FlacCfg* cfgs, FlacState* st0, FlacState* st1) {
  const int i = blockIdx.x, t = threadIdx.x;
  if (i >= a.n) return;
  const int b = a.slot[i];
  if (t < 16) st0[b].pend[t] = st1[b].pend[t] = 0;
  if (t == 0) {
    cfgs[b] = a.cfg[i];
    st0[b].pos = st1[b].pos = 0;
    st0[b].npend = st1[b].npend = 0;
    st0[b].pad = st1[b].pad = 0;
  }
}

int rate_code(int rate) {
  for (const RateCode& r : kRateCodes)
    if (r.rate == rate) return r.code;
  return -1;
}

int blocks_for(int64_t n_max) { return (int)((n_max + kHold + kMaxN - 1) / kMaxN); }

}  // namespace

struct SmolttsFlac {
  int B;
  FlacCfg* cfg_dev;
  PingPong<FlacState> st;
  FlacCfg* cfg_host;  // mirror of cfg_dev (sizes the grid)
};

static size_t carve(SmolttsFlac* f, char* base) {
  Carver cv{base, 0};
  f->cfg_dev = cv.take<FlacCfg>(f->B);
  f->st.carve(cv, f->B);
  return cv.off;
}

extern "C" {

size_t smoltts_flac_bytes(int32_t max_batch) {
  return stage_bytes<SmolttsFlac>(max_batch);
}

int32_t smoltts_flac_max_blocks(int32_t n_max) {
  if (n_max < 0) return 0;
  return blocks_for(n_max);
}

size_t smoltts_flac_out_bytes(int32_t n_max) {
  if (n_max < 0) return 0;
  return 2 * ((size_t)n_max + kHold) + (size_t)kSlack * blocks_for(n_max);
}

int smoltts_flac_create(void* slab_dev, size_t slab_bytes, int32_t max_batch, SmolttsFlac** out) {
  SmolttsFlac* f = nullptr;
  size_t need = 0;
  ST_TRY(stage_create("flac_create", slab_dev, slab_bytes, max_batch, out, &f, &need));
  f->cfg_host = static_cast<FlacCfg*>(calloc((size_t)max_batch, sizeof(FlacCfg)));
  if (!f->cfg_host) {
    delete f;
    set_error("flac_create: out of host memory");
    return SMOLTTS_E_INVALID;
  }
  if (hipMemset(slab_dev, 0, need) != hipSuccess) {  // every slot off, every stream empty
    free(f->cfg_host);
    delete f;
    set_error("flac_create: hipMemset failed");
    return SMOLTTS_E_HIP;
  }
  *out = f;
  return SMOLTTS_OK;
}

void smoltts_flac_destroy(SmolttsFlac* f) {
  if (!f) return;
  free(f->cfg_host);
  delete f;
}

int smoltts_flac_reset_slots(SmolttsFlac* f, const int32_t* slots_host, const int32_t* rates_host, const int32_t* sources_host,
                             int32_t n_slots, void* stream) {
  ST_REQUIRE(f && slots_host && rates_host && sources_host && n_slots > 0, SMOLTTS_E_INVALID, "flac_reset_slots: bad argument");
  auto fill = [&](ResetArgs& a, int i, int k) -> int {
    const int src = sources_host[k], rate = rates_host[k];
    ST_REQUIRE(src == SMOLTTS_FLAC_OFF || src == SMOLTTS_FLAC_F32 || src == SMOLTTS_FLAC_S16, SMOLTTS_E_INVALID,
               "flac_reset_slots: unknown source %d", src);
    FlacCfg& c = a.cfg[i];  // (zeroed)
    c.src = src;
    if (src != SMOLTTS_FLAC_OFF) {
      c.rate_code = rate_code(rate);
      ST_REQUIRE(c.rate_code > 0, SMOLTTS_E_INVALID, "flac_reset_slots: unsupported rate %d", rate);
    }
    return SMOLTTS_OK;
  };
  return reset_in_groups<ResetArgs>("flac_reset_slots", f->B, slots_host, n_slots, fill, [&](const ResetArgs& a) {
    for (int i = 0; i < a.n; ++i) f->cfg_host[a.slot[i]] = a.cfg[i];
    hipLaunchKernelGGL(flac_reset_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a, f->cfg_dev, f->st.half[0], f->st.half[1]);
  });
}

int smoltts_flac_chunk(SmolttsFlac* f, const float* pcm_dev, int64_t pcm_stride, int32_t n_in, const int32_t* valid_in_dev,
                       const void* s16_dev, int64_t s16_stride, const int32_t* s16_counts_dev, int32_t batch,
                       const int32_t* last_dev, void* out_dev, int64_t out_stride, int32_t* sizes_dev, int32_t max_blocks,
                       void* stream) {
  // a slot whose source is not given this call reads nothing; the grid and rows cover the most any other slot can read
  ST_TRY(check_chunk("flac_chunk", f, out_dev && sizes_dev, batch, pcm_dev != nullptr, n_in, pcm_stride));
  ST_REQUIRE(!s16_dev || (s16_counts_dev && s16_stride >= 0), SMOLTTS_E_INVALID, "flac_chunk: int16 samples without counts");
  int64_t n_max = 0;
  for (int b = 0; b < batch; ++b) {
    const FlacCfg& c = f->cfg_host[b];
    if (c.src == SMOLTTS_FLAC_F32 && pcm_dev) n_max = n_in > n_max ? n_in : n_max;
    if (c.src == SMOLTTS_FLAC_S16 && s16_dev) n_max = s16_stride / 2 > n_max ? s16_stride / 2 : n_max;
  }
  ST_REQUIRE(n_max < (1 << 30), SMOLTTS_E_INVALID, "flac_chunk: %lld samples per call", (long long)n_max);
  ST_REQUIRE(max_blocks >= blocks_for(n_max), SMOLTTS_E_CAPACITY, "flac_chunk: max_blocks %d < %d", max_blocks, blocks_for(n_max));
  ST_REQUIRE(out_stride >= (int64_t)smoltts_flac_out_bytes((int32_t)n_max), SMOLTTS_E_CAPACITY, "flac_chunk: out_stride %lld < %zu bytes",
             (long long)out_stride, smoltts_flac_out_bytes((int32_t)n_max));
  hipLaunchKernelGGL(flac_kernel, dim3(max_blocks, f->B), dim3(kT), 0, (hipStream_t)stream, pcm_dev, pcm_stride, n_in, valid_in_dev,
                     (const uint8_t*)s16_dev, s16_stride, s16_counts_dev, batch, last_dev, f->cfg_dev, f->st.cur(), f->st.next(),
                     (uint8_t*)out_dev, out_stride, sizes_dev, max_blocks);
  ST_CHECK_HIP(hipGetLastError());
  f->st.flip();
  return SMOLTTS_OK;
}

}  // extern "C"

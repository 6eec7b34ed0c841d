// kvq_scores.hip — kvq_key_scores: how much attention mass every stored key receives from the queries of the last S stored
// tokens (include/kvq_hip.h), straight from the quantised store. The primitive under attention-guided eviction (H2O: S = 1
// per decode step, accumulated; SnapKV: the last S prompt queries). Its own translation unit: kvq_attn.hip and attn/*.inc are
// not touched, so the few helpers this file shares with them in spirit (the code conversion, the lane swaps, the launch plan)
// are restated here.
//
// The normaliser of a query row is known only after its whole key range has been scored, so the store is read twice; K is
// 1 or 0.5 byte per element, and parking [rows, T] fp32 scores in HBM instead would move 4x the K bytes at 256 rows.
//   key_scores_stats_k  pass 1. Grid (64-row query block, split over T, batch row x kv head), 256 threads = 4 waves x 16 query
//     rows; the extend kernel's tile recipe: 64-token tiles, codes converted exactly to f16 / bf16 integers in LDS,
//     S^T = K Q^T on v_mfma_f32_16x16x32_{f16,bf16} (lane (x, g): query row x, tokens 16 i + 4 g + r), the K scale applied to
//     the product, the next tile requested before this one is reduced. Only the running (m, l) of each row survive: a single
//     split writes the row's log-sum-exp itself, several splits write (m, l) pairs.
//   key_scores_lse_k    merges the splits' pairs into one log-sum-exp per row (one thread per row, splits in order).
//   key_scores_mass_k   pass 2. Grid (run of token tiles, batch row x kv head). The workgroup stages each of its tiles once and
//     walks ALL query blocks of the kv head over it with the operands swapped, S = Q K^T (lane (x, g): token 16 i + x, query rows
//     4 g + r), so that the sum over query rows is four adds in the lane, two lane swaps and one LDS exchange between the four
//     waves, always in the same order. Every mass element has exactly one owner: no float atomics, bit-identical reruns.
// Tiles that lie in the future of every row of a query block (pass 1) or of a wave (pass 2) are skipped.
#include "kvq_common.h"

#include <math.h>

namespace kvq {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kQB = 64;          // query rows per block
constexpr int kTC = 64;          // tokens per tile
constexpr int kMaxSplit = 64;    // pass 1: splits over the stored tokens
constexpr int kTargetWG = 1024;  // workgroups a launch aims for

struct ScoreArgs {
  const void* q;
  int64_t q_sb, q_sh, q_ss;  // elements
  const uint8_t* k;
  int64_t k_sb, k_sh, k_st;  // bytes
  const float* k_scale;
  float* mass;
  int64_t m_sb, m_sh;  // elements
  float* lse;          // [B*Hkv][nqb*64] log-sum-exp of every query row, log2 domain
  float* pairs;        // nsplit > 1: [B*Hkv][nsplit][nqb*64] (m, l)
  float scale_log2;    // sm_scale * log2(e)
  uint32_t B, Hkv, nq, T, S, M, nqb, nsplit, tps;  // M = S * nq rows per kv head; tps = tiles per split (pass 1)
  uint32_t tpr;                                    // tiles per run (pass 2)
  uint32_t accumulate;
};

template <int DT>
struct Mfma;
template <>
struct Mfma<KVQ_F16> {
  __device__ static inline f32x4 mma(const u32x4 a, const u32x4 b, const f32x4 c) {
    f16x8 ah, bh;
    __builtin_memcpy(&ah, &a, 16);
    __builtin_memcpy(&bh, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
  }
};
template <>
struct Mfma<KVQ_BF16> {
  __device__ static inline f32x4 mma(const u32x4 a, const u32x4 b, const f32x4 c) {
    bf16x8 ah, bh;
    __builtin_memcpy(&ah, &a, 16);
    __builtin_memcpy(&bh, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
  }
};

// exchanges across the four 16-lane rows of a wave (v_permlane16_swap / v_permlane32_swap of a value with itself)
__device__ inline float xor16_max(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ inline float xor32_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ inline float xor16_add(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ inline float xor32_add(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// The raw bytes of 16 stored codes of one token row, and their values as floats (exact).
template <int BITS>
struct Codes16;
template <>
struct Codes16<8> {
  static constexpr int kBytes = 16;
  u32x4 w;
  template <bool NT>
  __device__ inline void load(const uint8_t* p) {
    if constexpr (NT) w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    else w = *reinterpret_cast<const u32x4*>(p);
  }
  __device__ inline void zero() { w = u32x4{0u, 0u, 0u, 0u}; }
  __device__ inline void values(float (&u)[16]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t x = w[i] ^ 0x80808080u;  // code + 128
      u[4 * i] = (float)(x & 0xFFu) - 128.f;
      u[4 * i + 1] = (float)((x >> 8) & 0xFFu) - 128.f;
      u[4 * i + 2] = (float)((x >> 16) & 0xFFu) - 128.f;
      u[4 * i + 3] = (float)(x >> 24) - 128.f;
    }
  }
};
template <>
struct Codes16<4> {
  static constexpr int kBytes = 8;
  u32x2 w;
  template <bool NT>
  __device__ inline void load(const uint8_t* p) {
    if constexpr (NT) w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    else w = *reinterpret_cast<const u32x2*>(p);
  }
  __device__ inline void zero() { w = u32x2{0x88888888u, 0x88888888u}; }  // nibble 8 = code 0
  __device__ inline void values(float (&u)[16]) const {  // nibble = code + 8, the even element in the HIGH nibble
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t hi = (w[i] >> 4) & 0x0F0F0F0Fu, lo = w[i] & 0x0F0F0F0Fu;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        u[8 * i + 2 * b] = (float)((hi >> (8 * b)) & 0xFFu) - 8.f;
        u[8 * i + 2 * b + 1] = (float)((lo >> (8 * b)) & 0xFFu) - 8.f;
      }
    }
  }
};

// One 64-token K tile on its way from the store into LDS: load() requests the workgroup's share of tokens [t0, t0 + 64) into
// registers (tokens at or past t_end are NOT read: zero codes, scale 0), stage() converts them to DT integers in the image
// s_k[token][d] (row pitch HD + 8 elements: 16-byte aligned rows, 4-bank shift per row) with the scales in s_sk.
template <int KBITS, int HD, int DT, bool NT>
struct KTile {
  static constexpr int KLD = HD + 8;
  static constexpr int UPR = HD / 16;           // 16-code units per token row
  static constexpr int SU = kTC * UPR / 256;    // units per thread: 1 or 2
  Codes16<KBITS> kr[SU];
  float skr;
  __device__ inline void load(const uint8_t* krow, const int64_t k_st, const float* k_scale, const uint32_t t0,
                              const uint32_t t_end, const uint32_t tid) {
#pragma unroll
    for (int i = 0; i < SU; ++i) {
      const uint32_t u = tid + 256u * i, o = u / UPR, c = u - o * UPR, t = t0 + o;
      if (t < t_end) kr[i].template load<NT>(krow + (int64_t)t * k_st + c * Codes16<KBITS>::kBytes);
      else kr[i].zero();
    }
    skr = 0.f;
    if (tid < (uint32_t)kTC && t0 + tid < t_end) skr = k_scale[t0 + tid];
  }
  __device__ inline void stage(uint16_t* s_k, float* s_sk, const uint32_t tid) const {
#pragma unroll
    for (int i = 0; i < SU; ++i) {
      const uint32_t u = tid + 256u * i, o = u / UPR, c = u - o * UPR;
      float kv[16];
      kr[i].values(kv);
      u32x4 w0, w1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w0[j] = Elem<DT>::pack2(kv[2 * j], kv[2 * j + 1]);
        w1[j] = Elem<DT>::pack2(kv[8 + 2 * j], kv[8 + 2 * j + 1]);
      }
      *reinterpret_cast<u32x4*>(&s_k[o * KLD + c * 16u]) = w0;
      *reinterpret_cast<u32x4*>(&s_k[o * KLD + c * 16u + 8u]) = w1;
    }
    if (tid < (uint32_t)kTC) s_sk[tid] = skr;
  }
};

// ---------------------------------------------------------------------------------------------------------------- pass 1
template <int KBITS, int HD, int DT>
__global__ __launch_bounds__(256) void key_scores_stats_k(const ScoreArgs a) {
  constexpr int KS = HD / 32;
  typedef KTile<KBITS, HD, DT, false> Tile;  // plain loads: pass 2 reads the same rows again
  constexpr int KLD = Tile::KLD;
  __shared__ __attribute__((aligned(16))) uint16_t s_k[kTC * KLD];
  __shared__ float s_sk[kTC];

  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, x = lane & 15u, g = lane >> 4;
  const uint32_t qb = blockIdx.x, sp = blockIdx.y, bk = blockIdx.z;
  const uint32_t b = bk / a.Hkv, hk = bk - b * a.Hkv;
  const uint32_t T0 = a.T - a.S;  // position of query row s: T0 + s; it sees the stored tokens t <= T0 + s

  // this lane's query row (rows beyond M compute on zeros as the last position and are never written)
  const uint32_t row = qb * kQB + w * 16u + x;
  const bool row_ok = row < a.M;
  const uint32_t s_row = row_ok ? row / a.nq : a.S - 1u;
  const uint32_t h_row = row_ok ? row - s_row * a.nq : 0u;
  const uint32_t p_row = T0 + s_row;
  u32x4 qf[KS];
  if (row_ok) {
    const uint16_t* qp = reinterpret_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_sb + (int64_t)(hk * a.nq + h_row) * a.q_sh +
                         (int64_t)s_row * a.q_ss + 8u * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const u32x4*>(qp + 32 * ks);
  } else {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = u32x4{0u, 0u, 0u, 0u};
  }
  const uint32_t m_end = a.M < qb * kQB + kQB ? a.M : qb * kQB + kQB;
  const uint32_t p_blk = T0 + (m_end - 1u) / a.nq;  // last position of the workgroup's rows: later tokens are seen by none
  const uint32_t wrow0 = qb * kQB + w * 16u;
  const bool wave_live = wrow0 < a.M;
  const uint32_t p_wave = wave_live ? T0 + ((a.M < wrow0 + 16u ? a.M : wrow0 + 16u) - 1u) / a.nq : 0u;

  const uint32_t st0 = sp * a.tps * (uint32_t)kTC;
  uint32_t st1 = st0 + a.tps * (uint32_t)kTC;
  st1 = st1 < p_blk + 1u ? st1 : p_blk + 1u;  // <= T
  const uint32_t n_st = st1 > st0 ? (st1 - st0 + kTC - 1u) / kTC : 0u;
  const uint8_t* krow = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh;

  Tile tile;
  float m = -INFINITY, l = 0.f;
  if (n_st) tile.load(krow, a.k_st, a.k_scale, st0, st1, tid);
  for (uint32_t it = 0; it < n_st; ++it) {
    const uint32_t t0 = st0 + it * kTC;
    tile.stage(s_k, s_sk, tid);
    __syncthreads();
    if (it + 1u < n_st) tile.load(krow, a.k_st, a.k_scale, t0 + kTC, st1, tid);  // in flight while this tile is reduced
    if (wave_live && t0 <= p_wave) {
      f32x4 sc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          sc[i] = Mfma<DT>::mma(*reinterpret_cast<const u32x4*>(&s_k[(16u * i + x) * KLD + 32u * ks + 8u * g]), qf[ks], sc[i]);
      }
      float p[4][4];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t o = 16u * i + 4u * g + r;
          p[i][r] = t0 + o <= p_row ? sc[i][r] * s_sk[o] * a.scale_log2 : -INFINITY;  // p_row < st1: never a token not read
          mx = fmaxf(mx, p[i][r]);
        }
      mx = xor32_max(xor16_max(mx));
      const float m_new = fmaxf(m, mx);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      float lsum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) lsum += __builtin_amdgcn_exp2f(p[i][r] - m_use);
      l = l * __builtin_amdgcn_exp2f(m - m_use) + lsum;
      m = m_new;
    }
    __syncthreads();
  }
  l = xor32_add(xor16_add(l));
  if (!row_ok || g != 0u) return;
  const int64_t rows = (int64_t)a.nqb * kQB;
  if (a.nsplit == 1u) {
    a.lse[(int64_t)bk * rows + row] = m + log2f(l);  // every row sees token 0: l > 0
  } else {
    const int64_t prow = ((int64_t)bk * a.nsplit + sp) * rows + row;
    a.pairs[2 * prow] = m;  // a split past the row's position: (-inf, 0)
    a.pairs[2 * prow + 1] = l;
  }
}

// ------------------------------------------------------------------------------------------------- log-sum-exp of the splits
__global__ __launch_bounds__(256) void key_scores_lse_k(const ScoreArgs a) {
  const uint32_t row = blockIdx.x * 256u + threadIdx.x, bk = blockIdx.y;
  if (row >= a.M) return;
  const int64_t rows = (int64_t)a.nqb * kQB;
  const float* pp = a.pairs + 2 * ((int64_t)bk * a.nsplit * rows + row);
  float m = -INFINITY;
  for (uint32_t sp = 0; sp < a.nsplit; ++sp) m = fmaxf(m, pp[2 * (int64_t)sp * rows]);  // split 0 holds token 0: finite
  float l = 0.f;
  for (uint32_t sp = 0; sp < a.nsplit; ++sp) {
    const float ms = pp[2 * (int64_t)sp * rows], ls = pp[2 * (int64_t)sp * rows + 1];
    l += ls * exp2f(ms - m);  // (-inf, 0): + 0
  }
  a.lse[(int64_t)bk * rows + row] = m + log2f(l);
}

// ---------------------------------------------------------------------------------------------------------------- pass 2
template <int KBITS, int HD, int DT>
__global__ __launch_bounds__(256) void key_scores_mass_k(const ScoreArgs a) {
  constexpr int KS = HD / 32;
  typedef KTile<KBITS, HD, DT, true> Tile;
  constexpr int KLD = Tile::KLD;
  __shared__ __attribute__((aligned(16))) uint16_t s_k[kTC * KLD];
  __shared__ float s_sk[kTC];
  __shared__ float s_red[4][kTC];

  const uint32_t tid = threadIdx.x, lane = tid & 63u, x = lane & 15u, g = lane >> 4;
  const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t run = blockIdx.x, bk = blockIdx.y;
  const uint32_t b = bk / a.Hkv, hk = bk - b * a.Hkv;
  const uint32_t T0 = a.T - a.S;
  const uint32_t ntiles = (a.T + kTC - 1u) / kTC;
  const uint32_t tile0 = run * a.tpr;
  const uint32_t tile1 = tile0 + a.tpr < ntiles ? tile0 + a.tpr : ntiles;
  const uint8_t* krow = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh;
  const uint16_t* qbase = reinterpret_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_sb + (int64_t)(hk * a.nq) * a.q_sh + 8u * g;
  const float* lse = a.lse + (int64_t)bk * a.nqb * kQB;
  float* mrow = a.mass + (int64_t)b * a.m_sb + (int64_t)hk * a.m_sh;

  // the Q operand of this lane for query block qb: row wrow0 + x (zeros beyond M)
  auto load_q = [&](const uint32_t qb, u32x4 (&qf)[KS]) {
    const uint32_t row = qb * kQB + w * 16u + x;
    if (row < a.M) {
      const uint32_t s = row / a.nq, h = row - s * a.nq;
      const uint16_t* qp = qbase + (int64_t)h * a.q_sh + (int64_t)s * a.q_ss;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const u32x4*>(qp + 32 * ks);
    } else {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) qf[ks] = u32x4{0u, 0u, 0u, 0u};
    }
  };

  Tile tile;
  if (tile0 < tile1) tile.load(krow, a.k_st, a.k_scale, tile0 * kTC, a.T, tid);
  for (uint32_t ti = tile0; ti < tile1; ++ti) {
    const uint32_t t0 = ti * kTC;
    tile.stage(s_k, s_sk, tid);
    __syncthreads();
    if (ti + 1u < tile1) tile.load(krow, a.k_st, a.k_scale, t0 + kTC, a.T, tid);
    float macc[4] = {0.f, 0.f, 0.f, 0.f};
    float sk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sk[i] = s_sk[16u * i + x] * a.scale_log2;
    // the first query block with a row that sees token t0: position T0 + s >= t0
    const uint32_t s_first = t0 > T0 ? t0 - T0 : 0u;
    const uint32_t qb0 = s_first * a.nq / kQB;
    u32x4 qf[KS], qn[KS];
    load_q(qb0, qf);
    for (uint32_t qb = qb0; qb < a.nqb; ++qb) {
      if (qb + 1u < a.nqb) load_q(qb + 1u, qn);  // in flight while this block is reduced
      const uint32_t wrow0 = qb * kQB + w * 16u;  // uniform in the wave
      const uint32_t wrow1 = a.M < wrow0 + 16u ? a.M : wrow0 + 16u;
      if (wrow0 < a.M && T0 + (wrow1 - 1u) / a.nq >= t0) {  // some row of the wave sees the tile's first token
        // rows 4 g + r of the wave: their log-sum-exp, and the last token each sees (-1: a row beyond M sees none)
        float lr[4];
        int32_t lim[4];
        const bool diag = t0 + (uint32_t)kTC - 1u > T0 + wrow0 / a.nq;  // uniform: the tile reaches past the wave's first row
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t rr = wrow0 + 4u * g + r;
          const bool ok = rr < a.M;
          lr[r] = ok ? lse[rr] : 0.f;
          lim[r] = ok ? (diag ? (int32_t)(T0 + rr / a.nq) : 0x7FFFFFFF) : -1;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            sc = Mfma<DT>::mma(qf[ks], *reinterpret_cast<const u32x4*>(&s_k[(16u * i + x) * KLD + 32u * ks + 8u * g]), sc);
          const int32_t t = (int32_t)(t0 + 16u * i + x);  // tokens at or past T lie beyond every row's position
          float e[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) e[r] = t <= lim[r] ? __builtin_amdgcn_exp2f(sc[r] * sk[i] - lr[r]) : 0.f;
          macc[i] += (e[0] + e[1]) + (e[2] + e[3]);
        }
      }
      if (qb + 1u < a.nqb) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = qn[ks];
      }
    }
    // the four row groups of the wave, then the four waves, always in this order
#pragma unroll
    for (int i = 0; i < 4; ++i) macc[i] = xor32_add(xor16_add(macc[i]));
    if (g == 0u) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s_red[w][16u * i + x] = macc[i];
    }
    __syncthreads();
    if (tid < (uint32_t)kTC && t0 + tid < a.T) {
      const float tot = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
      float* mp = mrow + t0 + tid;
      *mp = a.accumulate ? *mp + tot : tot;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
// Pass 1's launch shape, as the extend kernel plans its own: query blocks x splits x (batch row, kv head), about kTargetWG
// workgroups, at least two tiles per split. *ns_bound: the split count before rounding to whole tiles per split (>= nsplit,
// monotone in T: what the workspace is sized for).
static void stats_plan(const kvq_extend_dims_t* d, uint32_t* nqb, uint32_t* nsplit, uint32_t* tps, uint32_t* ns_bound) {
  const int64_t nq = d->Hq / d->Hkv, M = d->S * nq;
  const int64_t qbn = (M + kQB - 1) / kQB;
  const int64_t ntiles = (d->T + kTC - 1) / kTC;
  const int64_t base = qbn * d->B * d->Hkv;
  int64_t ns = (kTargetWG + base - 1) / base;
  const int64_t by_tiles = (ntiles + 1) / 2;
  if (ns > by_tiles) ns = by_tiles;
  if (ns > kMaxSplit) ns = kMaxSplit;
  if (ns < 1) ns = 1;
  const int64_t per = (ntiles + ns - 1) / ns;
  *nqb = (uint32_t)qbn;
  *tps = (uint32_t)per;
  *nsplit = (uint32_t)((ntiles + per - 1) / per);
  *ns_bound = (uint32_t)ns;
}

static const char* scores_dims_error(const kvq_extend_dims_t* d) {
  if (d->B <= 0 || d->Hq <= 0 || d->Hkv <= 0 || d->T <= 0 || d->S <= 0 || d->D <= 0) return "B, Hq, Hkv, T, S, D must be positive";
  if (d->Hq % d->Hkv != 0 || d->Hq / d->Hkv > 16) return "need Hq % Hkv == 0 and Hq / Hkv <= 16";
  if (d->B * d->Hkv >= 65536) return "B * Hkv must stay below 65536";
  if (d->T >= (int64_t(1) << 31) - kTC || d->S >= (int64_t(1) << 24)) return "T must stay below 2^31 and S below 2^24";
  if (d->S > d->T) return "the S query rows are those of the last S stored tokens: need S <= T";
  if (d->D != 64 && d->D != 128) return "head_dim must be 64 or 128";
  return nullptr;
}

// lse rows, then the (m, l) pairs of the splits
static int64_t scores_workspace_floats(const kvq_extend_dims_t* d) {
  uint32_t nqb, ns, tps, nsb;
  stats_plan(d, &nqb, &ns, &tps, &nsb);
  const int64_t rows = d->B * d->Hkv * (int64_t)nqb * kQB;
  return rows + (nsb > 1u ? rows * nsb * 2 : 0);
}

template <int KBITS, int HD, int DT>
static void launch_scores(const ScoreArgs& a, const uint32_t nruns, hipStream_t st) {
  KVQ_LAUNCH((key_scores_stats_k<KBITS, HD, DT>), dim3(a.nqb, a.nsplit, a.B * a.Hkv), dim3(256), 0, st, a);
  if (a.nsplit > 1u) KVQ_LAUNCH(key_scores_lse_k, dim3((a.M + 255u) / 256u, a.B * a.Hkv), dim3(256), 0, st, a);
  KVQ_LAUNCH((key_scores_mass_k<KBITS, HD, DT>), dim3(nruns, a.B * a.Hkv), dim3(256), 0, st, a);
}

template <int KBITS>
static void launch_scores_by_shape(const ScoreArgs& a, const uint32_t nruns, const int D, const int dtype, hipStream_t st) {
  if (D == 128) {
    if (dtype == KVQ_F16) launch_scores<KBITS, 128, KVQ_F16>(a, nruns, st);
    else launch_scores<KBITS, 128, KVQ_BF16>(a, nruns, st);
  } else {
    if (dtype == KVQ_F16) launch_scores<KBITS, 64, KVQ_F16>(a, nruns, st);
    else launch_scores<KBITS, 64, KVQ_BF16>(a, nruns, st);
  }
}

}  // namespace kvq

extern "C" {

int64_t kvq_key_scores_workspace(const kvq_extend_dims_t* d) {
  if (!d || kvq::scores_dims_error(d)) return -1;
  return kvq::scores_workspace_floats(d);
}

int kvq_key_scores(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const uint8_t* k_store, const kvq_strides_t* k_st,
                   const float* k_scales, int k_bits, float* mass, int64_t mass_sb, int64_t mass_sh, int accumulate, int dtype,
                   float sm_scale, float* workspace, int64_t workspace_floats, const kvq_extend_dims_t* d, void* stream) {
  using namespace kvq;
  const char* name = "kvq_key_scores";
  if (!d || !q || !k_store || !k_st || !k_scales || !mass || !workspace) {
    set_error("%s: NULL q / k_store / strides / k_scales / mass / workspace / dims", name);
    return KVQ_E_NULL;
  }
  if (const char* why = scores_dims_error(d)) {
    set_error("%s: bad dims B=%lld Hq=%lld Hkv=%lld T=%lld S=%lld D=%lld: %s", name, (long long)d->B, (long long)d->Hq,
              (long long)d->Hkv, (long long)d->T, (long long)d->S, (long long)d->D, why);
    return KVQ_E_DIMS;
  }
  if (dtype != KVQ_F16 && dtype != KVQ_BF16) {
    set_error("%s: dtype %d not supported (KVQ_F16, KVQ_BF16)", name, dtype);
    return KVQ_E_DTYPE;
  }
  if (k_bits != 8 && k_bits != 4) {
    set_error("%s: k_bits must be 8 or 4", name);
    return KVQ_E_DIMS;
  }
  const int kal = k_bits == 8 ? 16 : 8;
  if (!aligned(k_store, kal) || k_st->b % kal || k_st->h % kal || k_st->t % kal) {
    set_error("%s: store rows must be %d byte aligned", name, kal);
    return KVQ_E_DIMS;
  }
  if (k_st->t < d->D * k_bits / 8) {
    set_error("%s: store token stride shorter than a row", name);
    return KVQ_E_DIMS;
  }
  if (!aligned(q, 16) || q_sb % 8 || q_sh % 8 || q_ss % 8) {
    set_error("%s: q must be 16-byte aligned with strides that are multiples of 8 elements", name);
    return KVQ_E_DIMS;
  }
  if (!aligned(mass, 4) || (d->Hkv > 1 && mass_sh < d->T) || (d->B > 1 && mass_sb < d->T) || mass_sh < 0 || mass_sb < 0) {
    set_error("%s: mass must be fp32 [B, Hkv, >= T] with the tokens contiguous (strides b=%lld h=%lld, T=%lld)", name,
              (long long)mass_sb, (long long)mass_sh, (long long)d->T);
    return KVQ_E_DIMS;
  }
  const int64_t need = scores_workspace_floats(d);
  if (workspace_floats < need) {
    set_error("%s: workspace of %lld floats, %lld needed", name, (long long)workspace_floats, (long long)need);
    return KVQ_E_DIMS;
  }
  if (!aligned(workspace, 4)) {
    set_error("%s: workspace must be 4-byte aligned", name);
    return KVQ_E_DIMS;
  }
  if (const int rc = check_device(mass, name)) return rc;

  ScoreArgs a;
  a.q = q; a.q_sb = q_sb; a.q_sh = q_sh; a.q_ss = q_ss;
  a.k = k_store; a.k_sb = k_st->b; a.k_sh = k_st->h; a.k_st = k_st->t;
  a.k_scale = k_scales;
  a.mass = mass; a.m_sb = mass_sb; a.m_sh = mass_sh;
  a.scale_log2 = sm_scale * 1.4426950408889634f;
  a.B = (uint32_t)d->B; a.Hkv = (uint32_t)d->Hkv; a.nq = (uint32_t)(d->Hq / d->Hkv);
  a.T = (uint32_t)d->T; a.S = (uint32_t)d->S; a.M = (uint32_t)(d->S * (d->Hq / d->Hkv));
  uint32_t nsb;
  stats_plan(d, &a.nqb, &a.nsplit, &a.tps, &nsb);
  a.lse = workspace;
  a.pairs = workspace + (int64_t)a.B * a.Hkv * a.nqb * kQB;
  a.accumulate = accumulate ? 1u : 0u;
  // pass 2: runs of token tiles, about kTargetWG workgroups
  const int64_t ntiles = (d->T + kTC - 1) / kTC;
  int64_t nruns = (kTargetWG + d->B * d->Hkv - 1) / (d->B * d->Hkv);
  if (nruns > ntiles) nruns = ntiles;
  a.tpr = (uint32_t)((ntiles + nruns - 1) / nruns);
  nruns = (ntiles + a.tpr - 1) / a.tpr;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (k_bits == 8) launch_scores_by_shape<8>(a, (uint32_t)nruns, (int)d->D, dtype, st);
  else launch_scores_by_shape<4>(a, (uint32_t)nruns, (int)d->D, dtype, st);
  return check_launch(name);
}

}  // extern "C"

// kvq_quant.hip — per-token symmetric INT8 / packed-INT4 quantise kernels for gfx950.
//
// Replaces quantize_int8_per_tensor / quantize_int4_per_tensor_packed
// (src/quantization/ops.py:10-65) as they are applied slice by slice ([B,H,1,D]) by
// QuantizedLayerKV.append (ops.py:174-210): ONE scale per (group, token) over all B*H*D values.
//
//   s32    = max( max|x| / QMAX, eps )            fp32, IEEE division      (ops.py:28, :49)
//   q      = clamp( rint(x32 / s32), QMIN, QMAX )  half-to-even, true division (ops.py:29, :50)
//   stored = RN_in_dtype(s32), kept widened to fp32 in the scale table     (ops.py:30, :65)
//   INT4: nibble = q + 8, even d -> high nibble, odd D padded with nibble 8 (ops.py:52-63)
//   NaN / inf: a slice that holds one stores code 0 throughout and the scale NaN (a NaN in it) or +inf — torch's
//   abs().max() and clamp(min=eps) keep a NaN, its int8 cast of a NaN quotient stores 0 (include/kvq_hip.h; scale_of, quant1)
//
// Roofline: HBM stream, single pass: 2 B in + 1 B (INT8) or 0.5 B (INT4) out per fp16 element.
// Fused kernel: a workgroup owns a tile of TT tokens x all B*H rows of one group. Rows are T*D
// apart in memory, so each row contributes one contiguous TT*D run (coalesced 16 B/lane
// loads). The tile stays PACKED in registers between the abs-max pass and the quantise pass.
//   abs-max   packed u16 max of sign-masked halves -> DPP over the D/8 lanes of a (row, token) ->
//             register max across rows (one-wave tiles, REGMAX) or LDS ds_max_u32 (larger tiles)
//   quotient  x * RN(1/s32) with a distance-to-half-integer guard and an IEEE-divide fallback:
//             bit-exact rint(x / s32) at a third of the cost of dividing every element
//   stores    staged through LDS in output order, 16 B/lane, non-temporal
// Shipped launch shape: ONE WAVE per workgroup (64 threads, 4096-element tile): no barrier costs
// anything and waves of different tiles run decoupled. Larger B*H*D -> quant_tokens_sweep_k;
// odd / unaligned shapes -> the generic two-pass pair.
#include <type_traits>

#include "kvq_common.h"

namespace kvq {

constexpr int kNVMax = 8;                         // 16-byte (8-element) vectors per thread per tile
constexpr int kTileElems = kBlock * kNVMax * 8;   // 16384 elements
constexpr int kMaxTT = 64;

struct QuantArgs {
  PtrTable in;  // per-group input base pointers (this launch's groups)
  Strides is;   // input strides in elements (g unused)
  uint8_t* q;   // store base for this launch's first group
  Strides qs;   // store strides in bytes
  float* scales;
  int64_t ssg;
  float* absmax_ws;  // [G, T] floats (two-pass path)
  float eps;
  uint32_t G, B, H, T, D;
  // fused path
  uint32_t R;        // B*H
  uint32_t TT;       // tokens per tile (power of two)
  int32_t dvshift;   // log2(D/8)
  int32_t vshift;    // log2(TT * D/8)
  uint32_t nvec;     // R * TT * D/8 vectors per full tile
  uint32_t rpc;      // sweep kernel: rows per sweep step
  uint32_t dv;       // sweep kernel, D/8 not a power of two (or > 64): D/8
  uint32_t vpr;      // sweep kernel, same case: TT * D/8 vectors per row run
  uint32_t t_begin;  // first token of this launch's first tile
  int32_t nt_loads;  // non-temporal input loads
  int32_t nt_stores; // non-temporal output stores (tunable quant_nt_stores; -1 = as nt_loads)
  int32_t blk;       // workgroup size of the fused kernel (256, or 64 = one wave per tile)
  int32_t nv;        // vectors per lane per tile (8, or 4 for the small one-wave tile)
  int32_t bh_contig; // rows addressable as r * stride_h on both sides
  uint32_t xcd_group;  // consecutive tiles per XCD for the fused one-tile kernel (0 / 1 = round robin)
  int32_t acc;         // abs-max phase: keep what the table already holds (max with it) instead of overwriting
};

// ---------------------------------------------------------------------------- fused single pass

// DPP lane exchange inside a 16-lane row (single VALU op, no LDS traffic)
template <int CTRL>
__device__ inline uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
// unsigned max over aligned groups of 2^LOGW consecutive lanes; every lane gets the group max.
// Order-preserving for the bit patterns of non-negative floats / halves.
__device__ inline uint32_t group_umax(uint32_t v, int logw) {
  if (logw > 0) v = max(v, dpp_u32<0xB1>(v));   // quad_perm(1,0,3,2): lane ^ 1
  if (logw > 1) v = max(v, dpp_u32<0x4E>(v));   // quad_perm(2,3,0,1): lane ^ 2
  if (logw > 2) v = max(v, dpp_u32<0x141>(v));  // row_half_mirror: quads of an 8-lane half
  if (logw > 3) v = max(v, dpp_u32<0x140>(v));  // row_mirror: halves of a 16-lane row
  if (logw > 4) v = max(v, (uint32_t)__shfl_xor((int)v, 16));
  if (logw > 5) v = max(v, (uint32_t)__shfl_xor((int)v, 32));
  return v;
}

// rint(x / s32) + BIAS for 8 elements, returned in the low mantissa bits of
// (1.5 * 2^23 + BIAS + q): bit-exact with IEEE division at a fraction of its cost.
// Fast path: p = x * r with r = RN(1/s32). |p - x/s32| <= 2^-23 |p| (at most two roundings) and
// the correctly rounded quotient RN(x/s32) is within 2^-24 |p| of x/s32, with |p| <= QMAX (1 + 2^-22)
// because |x| <= amax and s32 >= RN(amax/QMAX). So if p is farther than
// m = 1.5 * 2^-22 * QMAX (twice the error bound) from every half-integer, then p, x/s32 and
// RN(x/s32) all round to the same integer; "within m of a half-integer" is |d| >= 0.5 - m with
// d = p - rint(p); thr = guard_threshold(s32) is that 0.5 - m. Otherwise (INT8: ~1 element in 11,000; INT4: ~1 in
// 200,000) the 8-element vector is redone with the IEEE divide.
// Rounding: adding 1.5 * 2^23 (even) rounds p to the nearest integer, ties to even — the same
// integer as rint(p) — and leaves it in two's complement in the low mantissa bits.
// No clamp is needed when s32 comes from the data's own abs-max: the quotient is bounded by
// QMAX (1 + 2^-23), which rounds to QMAX (the reference's clamp never fires either).
// CLAMP: the abs-max is the CALLER's (kvq_quant_tokens_from_absmax) and may be smaller than the
// data, so the quotient is unbounded. The magic sum is clamped to [magic + QMIN, magic + QMAX]
// (one v_med3_f32 per element: every sum is a float of the same sign, ordered like the integer it
// holds), and so is the division fallback. The guard still decides on the unclamped sum: a
// quotient past QMAX + 1/2 clamps to the same code whichever integer it rounds to.
// Non-finite input: a token whose scale is NaN or +inf stores code 0 in every element (kvq_common.h, quant1), and under
// a caller's finite scale a NaN element does (±inf clamps to QMAX / QMIN like any quotient past the range). Neither is
// a magic sum's low byte — fma(inf, 0, magic) is a NaN whose low byte is 0: INT4 nibble 0 — so such a vector takes the
// division path (its threshold drops below zero), which maps a NaN quotient to 0. The test on s32 is per token (the
// data's own abs-max: nothing per element); CLAMP adds the vector's has_nan().
// The guard's threshold for a token: kThr, or a value below every |d| when the token's scale is NaN or +inf. A per-token
// VALUE that the guard's own comparison reads (a kernel computes it where it computes the reciprocal); the opaque move
// keeps the compiler from turning it into mask arithmetic per vector (three scalar instructions each: 2 % of
// quant_wide_k's time).
template <int BITS>
__device__ inline float guard_threshold(float s32) {
  float thr = s32 < INFINITY ? 0.5f - 1.5f * QRange<BITS>::qmax * 0x1p-22f : -1.0f;
  asm("" : "+v"(thr));
  return thr;
}

template <int BITS, bool CLAMP = false, class V>
__device__ inline void quotient_bits8(const V& v, float s32, float r, float thr, uint32_t (&qb)[8]) {
  constexpr float kBias = BITS == 8 ? 0.0f : 8.0f;
  constexpr float kMagic = 12582912.0f + kBias;  // 1.5 * 2^23 + BIAS
  constexpr float kLo = kMagic + QRange<BITS>::qmin, kHi = kMagic + QRange<BITS>::qmax;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 r2 = {r, r}, magic2 = {kMagic, kMagic};
  if constexpr (CLAMP) {
    if (v.has_nan()) thr = -1.0f;
  }
  float worst = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // two elements per v_pk_*_f32
    const f32x2 x2 = {v.get(2 * k), v.get(2 * k + 1)};
    // sum = RN(x*r + magic) = magic + rint(x*r): the fma rounds the EXACT product, which is
    // within 2^-24 |p| of x/s32 (only r is rounded), inside the same margin
    const f32x2 sum = __builtin_elementwise_fma(x2, r2, magic2);
    const f32x2 d = __builtin_elementwise_fma(x2, r2, magic2 - sum);  // x*r - rint(x*r), one rounding
    worst = fmaxf(worst, fmaxf(fabsf(d[0]), fabsf(d[1])));              // one v_max3_f32 with |.| modifiers
    if constexpr (CLAMP) {
      qb[2 * k] = __float_as_uint(__builtin_amdgcn_fmed3f(sum[0], kLo, kHi));
      qb[2 * k + 1] = __float_as_uint(__builtin_amdgcn_fmed3f(sum[1], kLo, kHi));
    } else {
      qb[2 * k] = __float_as_uint(sum[0]);
      qb[2 * k + 1] = __float_as_uint(sum[1]);
    }
  }
  if (__builtin_expect(worst >= thr, 0)) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float q = rintf(v.get(j) / s32);
      q = q != q ? 0.0f : q;
      qb[j] = __float_as_uint((CLAMP ? __builtin_amdgcn_fmed3f(q, QRange<BITS>::qmin, QRange<BITS>::qmax) : q) + kMagic);
    }
  }
}

// low bytes of 4 words -> one word {b0, b1, b2, b3} (3 ops per 4 elements)
__device__ inline uint32_t gather_low_bytes(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3) {
  const uint32_t lo = __builtin_amdgcn_perm(q1, q0, 0x0C0C0400u);  // {q0.b0, q1.b0, 0, 0}
  const uint32_t hi = __builtin_amdgcn_perm(q3, q2, 0x04000C0Cu);  // {0, 0, q2.b0, q3.b0}
  return lo | hi;
}
// INT8: the two's complement low byte of the magic sum is q
__device__ inline u32x2 pack_i8(const uint32_t (&qb)[8]) {
  u32x2 w;
  w[0] = gather_low_bytes(qb[0], qb[1], qb[2], qb[3]);
  w[1] = gather_low_bytes(qb[4], qb[5], qb[6], qb[7]);
  return w;
}
// INT4: low byte = q + 8 in [1, 15] (clean high nibble); even element -> HIGH nibble (ops.py:61-63)
__device__ inline uint32_t pack_i4(const uint32_t (&qb)[8]) {
  const uint32_t a = gather_low_bytes(qb[0], qb[1], qb[2], qb[3]);  // bytes n0..n3
  const uint32_t b = gather_low_bytes(qb[4], qb[5], qb[6], qb[7]);  // bytes n4..n7
  const uint32_t ta = (a << 4) | (a >> 8);  // byte0 = n0<<4|n1, byte2 = n2<<4|n3
  const uint32_t tb = (b << 4) | (b >> 8);
  return __builtin_amdgcn_perm(tb, ta, 0x06040200u);  // {ta.b0, ta.b2, tb.b0, tb.b2}
}

// ROWU: the tile has >= 256 vectors per row, so in round i every lane of the block works on the
// same row (row index and its offsets are scalar) and (t, d) offsets collapse to wv * 8.
// FULL: every tile of the launch is complete (kBlock * kNVMax vectors, TT tokens inside T), so no
// lane is ever predicated off: no validity masks, no exec juggling.
// BLK: workgroup size. 64 = one wave per workgroup: the three barriers cost nothing and waves of
// different tiles run fully decoupled (tile = 4096 elements).
// REGMAX (one-wave tiles whose row run is at most 64 vectors): a lane keeps the same
// (token, d-vector) in every round and only the row changes, so the abs-max across rows is a
// register max (plus one lane exchange per halving of the row run below 64 vectors), the scale is
// computed per lane, and the kernel needs no LDS, atomics or barriers for it.
// NV: 16-byte vectors per lane per tile (tile = BLK * NV * 8 elements).
// GEO128: the tile geometry of the Llama prefill shape as compile-time constants (8 rows of head_dim 128, 4 tokens per
// one-wave tile: 64 vectors per row run, 16 lanes per token) instead of kernel arguments — the same code with its
// shifts, masks and lane-exchange loops folded.
// NTL / NTS: non-temporal input loads / output stores, COMPILE-TIME (a run-time `if (flag) nt_load else load` is merged
// by the compiler into one plain load: the kernel ran without non-temporal accesses until the end of round 2).
template <int IDT, int BITS, bool ROWU, bool LDS_OUT, bool FULL, int BLK = kBlock, int REGMAX = 0, int NV = kNVMax, bool GEO128 = false,
          bool NTL = true, bool NTS = true>
__global__ __launch_bounds__(BLK) void quant_tokens_fused_k(const QuantArgs a) {
  static_assert(!GEO128 || (BLK == 64 && NV == 8 && REGMAX == 1 && ROWU && FULL), "GEO128: the one-wave register-max tile");
  const uint32_t g_vshift = GEO128 ? 6u : a.vshift, g_dvshift = GEO128 ? 4u : a.dvshift, g_TT = GEO128 ? 4u : a.TT;
  const uint32_t g_R = GEO128 ? 8u : a.R, g_D = GEO128 ? 128u : a.D, g_nvec = GEO128 ? 512u : a.nvec;
  __shared__ __attribute__((aligned(16))) uint32_t s_out[LDS_OUT ? BLK * NV * 8 * BITS / 32 : 4];
  __shared__ uint32_t s_amax[kMaxTT];
  __shared__ float s_scale[kMaxTT], s_rcp[kMaxTT];
  const uint32_t tid = threadIdx.x;
  const uint32_t g = blockIdx.y;
  const uint32_t t0 = a.t_begin + (GEO128 ? blockIdx.x : xcd_grouped_item(blockIdx.x, a.xcd_group, gridDim.x)) * g_TT;
  const uint32_t DV = g_D >> 3;
  const uint32_t wmask = (1u << g_vshift) - 1u;
  // is.t == D and qs.t == Dq (or a single token per tile), so within a row the tile is one
  // contiguous run: element offset = wv * 8
  const char* in = reinterpret_cast<const char*>(a.in.p[g]) + (int64_t)t0 * (GEO128 ? 128 : a.is.t) * Elem<IDT>::size;
  uint8_t* qbase = a.q + (int64_t)g * a.qs.g + (int64_t)t0 * (GEO128 ? (int64_t)(128 * BITS / 8) : a.qs.t);
  constexpr int QV = BITS;  // bytes stored per 8-element vector: 8 (INT8) or 4 (INT4)

  if constexpr (REGMAX == 0) {
    for (uint32_t i = tid; i < (uint32_t)kMaxTT; i += BLK) s_amax[i] = 0u;
    __syncthreads();
  }

  // pass 1: load the tile (stays in registers), per-(row, token) abs-max -> LDS max across rows
  Vec8<IDT> x[NV];
  bool valid[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    uint32_t r, wv;
    if constexpr (ROWU) {
      r = (uint32_t)(i * BLK) >> g_vshift;
      wv = ((uint32_t)(i * BLK) & wmask) + tid;
    } else {
      const uint32_t v = i * BLK + tid;
      r = v >> g_vshift;
      wv = v & wmask;
    }
    valid[i] = FULL || (((uint32_t)(i * BLK) + tid < g_nvec) && (t0 + (wv >> g_dvshift) < a.T));
    if (valid[i]) {
      const char* src = in + ((int64_t)r * a.is.h + (int64_t)wv * 8) * Elem<IDT>::size;
      if constexpr (NTL) x[i].load_nt(src);
      else x[i].load(src);
    }
  }
  // REGMAX = number of lane identities: 1 = the row run is one round wide (or narrower), 2 = two
  // rounds wide (rounds alternate between the run's two halves)
  constexpr int RM = REGMAX > 0 ? REGMAX : 1;
  float reg_s32[RM], reg_rcp[RM], reg_thr[RM];
  if constexpr (REGMAX > 0) {
    uint32_t m[RM];
#pragma unroll
    for (int p = 0; p < RM; ++p) m[p] = 0u;
#pragma unroll
    for (int i = 0; i < NV; ++i) m[i % RM] = max(m[i % RM], x[i].absmax_bits());  // across the tile's rows
#pragma unroll
    for (int p = 0; p < RM; ++p) {
      uint32_t mp = group_umax(m[p], g_dvshift);  // across the D/8 lanes of the token
      if constexpr (RM == 1)
        for (int sh = g_vshift; sh < 6; ++sh) mp = max(mp, (uint32_t)__shfl_xor((int)mp, 1 << sh));  // row run < one wave
      reg_s32[p] = scale_of<BITS>(Vec8<IDT>::bits_to_f32(mp), a.eps);
      reg_rcp[p] = 1.0f / reg_s32[p];
      reg_thr[p] = guard_threshold<BITS>(reg_s32[p]);
      const uint32_t wv = (uint32_t)(p * BLK) + tid;  // this lane's vector in the row run, rounds i % RM == p
      if ((tid & (DV - 1u)) == 0u && (RM > 1 || (tid >> g_vshift) == 0u))
        a.scales[(int64_t)g * a.ssg + t0 + ((wv & wmask) >> g_dvshift)] = Elem<IDT>::round_trip(reg_s32[p]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (FULL || (uint32_t)(i * BLK) < g_nvec) {  // uniform: whole waves reach the lane exchanges
        const uint32_t wv = ((uint32_t)(i * BLK) + tid) & wmask;
        uint32_t m = valid[i] ? x[i].absmax_bits() : 0u;
        m = group_umax(m, g_dvshift);  // the D/8 lanes of one (row, token)
        if (valid[i] && (wv & (DV - 1u)) == 0u) atomicMax(&s_amax[wv >> g_dvshift], m);
      }
    }
    __syncthreads();

    // per-token scale, its reciprocal (both IEEE divides, once per token) and the stored scale
    if (tid < g_TT && (FULL || t0 + tid < a.T)) {
      const float amax = Vec8<IDT>::bits_to_f32(s_amax[tid]);
      const float s32 = scale_of<BITS>(amax, a.eps);
      s_scale[tid] = s32;
      s_rcp[tid] = 1.0f / s32;
      a.scales[(int64_t)g * a.ssg + t0 + tid] = Elem<IDT>::round_trip(s32);
    }
    __syncthreads();
  }

  // pass 2: scale, round, pack, store
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!FULL && !valid[i]) continue;
    uint32_t r, wv;
    if constexpr (ROWU) {
      r = (uint32_t)(i * BLK) >> g_vshift;
      wv = ((uint32_t)(i * BLK) & wmask) + tid;
    } else {
      const uint32_t v = i * BLK + tid;
      r = v >> g_vshift;
      wv = v & wmask;
    }
    const uint32_t tl = wv >> g_dvshift;
    uint32_t qb[8];
    if constexpr (REGMAX > 0) quotient_bits8<BITS>(x[i], reg_s32[i % RM], reg_rcp[i % RM], reg_thr[i % RM], qb);
    else quotient_bits8<BITS>(x[i], s_scale[tl], s_rcp[tl], guard_threshold<BITS>(s_scale[tl]), qb);
    if constexpr (LDS_OUT) {
      // stage the packed bytes in LDS in output order (row-major, wv * QV within the row run)
      const uint32_t widx = ((r << g_vshift) + wv) * (QV / 4);
      if constexpr (BITS == 8) {
        const u32x2 w = pack_i8(qb);
        s_out[widx] = w[0];
        s_out[widx + 1] = w[1];
      } else {
        s_out[widx] = pack_i4(qb);
      }
    } else {
      uint8_t* qp = qbase + (int64_t)r * a.qs.h + (int64_t)wv * QV;
      if constexpr (BITS == 8) *reinterpret_cast<u32x2*>(qp) = pack_i8(qb);
      else *reinterpret_cast<uint32_t*>(qp) = pack_i4(qb);
    }
  }

  if constexpr (LDS_OUT) {
    // 16 B per lane, 1 KiB contiguous per wave store: each row of the tile is one run of
    // TT * Dq bytes in the store (ablation: the direct 4 B/lane stores cost ~100 us of 354)
    __syncthreads();
    const uint32_t row_shift = g_vshift + (BITS == 8 ? 3 : 2);  // log2(bytes per full row run)
    const uint32_t row_bytes = 1u << row_shift;
    uint32_t nt = FULL ? g_TT : a.T - t0;
    if (nt > g_TT) nt = g_TT;
    const uint32_t valid_bytes = nt * (g_D * BITS / 8);  // ragged last tile: shorter runs
    const uint32_t total = g_R << row_shift;
    for (uint32_t k = tid * 16u; k < total; k += BLK * 16u) {
      const uint32_t r = k >> row_shift;
      const uint32_t off = k & (row_bytes - 1u);
      if (off < valid_bytes) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(&s_out[k >> 2]);
        if constexpr (NTS) __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(qbase + (int64_t)r * a.qs.h + off));
        else *reinterpret_cast<u32x4*>(qbase + (int64_t)r * a.qs.h + off) = w;
      }
    }
  }
}

// ---------------------------------------------------------------------------- compile-time tile (what ships for the BASELINE shapes)
// The shapes the benchmarks are quoted on — R = B*H head rows of head_dim D with f16 / bf16 input: 8 x 128 (Llama-3-8B),
// 16 x 64 (gpt2-medium), 12 x 64 (gpt2), 8 x 64 — as ONE WAVE per tile of TT tokens with the whole geometry in the
// template: lane = (row-in-instruction, token, 8-element d-vector); every load instruction of the wave reads RPI = 64 /
// (TT * D/8) rows' contiguous TT*D-element runs (1 KiB, or 2 x 512 B); the abs-max across the rows is a register max
// (+ one lane exchange when two rows share an instruction), across a token's D/8 lanes DPP; the scale is per lane.
// Addressing is by BUFFER instructions: a per-wave descriptor of the group's rows (scalar), a lane offset that never
// changes, the row as the instruction's scalar offset — no 64-bit vector address arithmetic, no pointer per row. A
// ragged last tile costs nothing: lanes of tokens past T carry an out-of-range offset (loads return 0, which cannot
// raise an abs-max; stores are dropped), so ONE instantiation serves complete and ragged tiles.
// Same arithmetic, same order of operations per element as quant_tokens_fused_k (quotient_bits8 / pack_*): bit-identical.
// The row loads and output stores are non-temporal (buffer aux immediate 2; the other cache policies measured slower,
// profiles/r03f_*).
struct QuantTileArgs {
  PtrTable in;      // per-group input base pointers
  uint8_t* q;       // store base of this launch's first group
  float* scales;
  float* absmax;    // split phases: [G, T] fp32 table of this launch's first group
  int64_t qs_g;     // bytes
  int64_t ssg;
  uint32_t is_h;    // input row stride in BYTES
  uint32_t qs_h;    // store row stride in bytes
  uint32_t T;
  uint32_t rows;    // B*H rows of a group; blockIdx.z walks them R at a time (fused: rows == R, gridDim.z == 1)
  float eps;
};

// PHASE 0: the fused quantise (abs-max, scale, quantise: one pass over the tile).
// Split phases of a batch-sharded slice (the scale spans the WHOLE batch, ops.py:27,48, so the abs-max table
// crosses ranks between the two): the same tile walk over R-row groups of a group's B_local*H rows (blockIdx.z),
//   PHASE 1: abs-max of the R rows -> atomicMax into absmax[g, t] (the host zeroes the table first; non-negative floats
//            order like their bit patterns); plain loads, so the rows stay in the Infinity Cache for phase 2
//   PHASE 2: quantise the R rows with scale max(absmax[g, t] / QMAX, eps) (the table completed by all_reduce(MAX)),
//            non-temporal loads (last use); row group 0 stores the scales.
template <int IDT, int BITS, int R, int DV, int TT, int PHASE = 0>
__global__ __launch_bounds__(kWave) void quant_tile_k(const QuantTileArgs a) {
  static_assert(IDT != KVQ_F32, "two-byte inputs");
  constexpr int LPR = TT * DV;              // lanes per row run
  static_assert(LPR == 64 || LPR == 32, "a row run is one wave or half a wave wide");
  constexpr int RPI = 64 / LPR;             // rows per load instruction
  static_assert(R % RPI == 0, "rows pair up");
  constexpr int NV = R / RPI;               // 16-byte vectors per lane
  constexpr int D = DV * 8;
  constexpr int QV = BITS;                  // bytes stored per 8-element vector
  constexpr int ROWB = LPR * QV;            // bytes of one row's run in the store
  constexpr int OUTB = R * ROWB;            // bytes of the tile in the store
  constexpr int NST = (OUTB + 1023) / 1024; // 16 B per lane store instructions
  constexpr uint32_t kOut = 0x80000000u;    // offset no descriptor of ours covers
  __shared__ __attribute__((aligned(16))) uint32_t s_out[PHASE == 1 ? 4 : NST * 256];
  const uint32_t lane = threadIdx.x;
  const uint32_t g = blockIdx.y;
  const uint32_t t0 = blockIdx.x * TT;
  const uint32_t nt = a.T - t0 < (uint32_t)TT ? a.T - t0 : (uint32_t)TT;  // uniform
  const uint32_t r0 = PHASE == 0 ? 0u : blockIdx.z * (uint32_t)R;
  const uint32_t nr = PHASE == 0 ? (uint32_t)R : (a.rows - r0 < (uint32_t)R ? a.rows - r0 : (uint32_t)R);  // rows of this group (uniform)
  const uint32_t sub = RPI == 1 ? 0u : lane / LPR, wv = lane % LPR, tok = wv / DV;

  // rows past nr and tokens past nt are outside the descriptor: loads return 0 (no effect on an abs-max), stores are dropped
  const char* ibase = reinterpret_cast<const char*>(a.in.p[g]) + (int64_t)r0 * a.is_h + (int64_t)t0 * (D * 2);
  const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(ibase), 0,
                                                                        (int)((nr - 1u) * a.is_h + nt * (D * 2)), 0x00020000);
  const uint32_t ioff = tok < nt ? sub * a.is_h + wv * 16u : kOut;
  Vec8<IDT> x[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i)
    x[i].w = __builtin_amdgcn_raw_buffer_load_b128(irs, ioff, (uint32_t)(i * RPI) * a.is_h, PHASE == 1 ? 0 : 2 /* non-temporal */);

  constexpr int DVSH = DV == 16 ? 4 : 3;
  float s32;
  if constexpr (PHASE == 2) {
    s32 = scale_of<BITS>(tok < nt ? a.absmax[(int64_t)g * a.T + t0 + tok] : 0.0f, a.eps);
  } else {
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < NV; ++i) m = max(m, x[i].absmax_bits());  // across the lane's rows
    if constexpr (RPI == 2) m = max(m, (uint32_t)__shfl_xor((int)m, 32));
    m = group_umax(m, DVSH);  // across the D/8 lanes of the token
    if constexpr (PHASE == 1) {
      if ((lane % DV) == 0u && sub == 0u && tok < nt)
        atomicMax(reinterpret_cast<uint32_t*>(a.absmax) + (int64_t)g * a.T + t0 + tok, __float_as_uint(Vec8<IDT>::bits_to_f32(m)));
      return;
    }
    s32 = scale_of<BITS>(Vec8<IDT>::bits_to_f32(m), a.eps);
  }
  const float rcp = 1.0f / s32, thr = guard_threshold<BITS>(s32);
  if ((lane % DV) == 0u && sub == 0u && tok < nt && r0 == 0u) a.scales[(int64_t)g * a.ssg + t0 + tok] = Elem<IDT>::round_trip(s32);

#pragma unroll
  for (int i = 0; i < NV; ++i) {
    uint32_t qb[8];
    quotient_bits8<BITS, PHASE == 2>(x[i], s32, rcp, thr, qb);  // phase 2: the caller's table may be below the data
    const uint32_t widx = (((uint32_t)(i * RPI) + sub) * LPR + wv) * (QV / 4);  // output order: row-major, wv * QV inside the run
    if constexpr (BITS == 8) {
      const u32x2 w = pack_i8(qb);
      *reinterpret_cast<u32x2*>(&s_out[widx]) = w;
    } else {
      s_out[widx] = pack_i4(qb);
    }
  }
  // one wave: its LDS queue is in order; only the compiler must not move the reads above the writes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  uint8_t* obase = a.q + (int64_t)g * a.qs_g + (int64_t)r0 * a.qs_h + (int64_t)t0 * (D * BITS / 8);
  const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(obase, 0, (int)((nr - 1u) * a.qs_h + nt * (D * BITS / 8)), 0x00020000);
  // 16 B piece k = 1024 j + 16 lane of the staged tile: row k / ROWB, byte k % ROWB of the row's run
  const uint32_t lrow = lane * 16u / ROWB, loff = lane * 16u % ROWB;
  const uint32_t ooff = loff < nt * (uint32_t)(D * BITS / 8) ? lrow * a.qs_h + loff : kOut;
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(&s_out[j * 256 + lane * 4]);
    const uint32_t off = (OUTB % 1024 == 0 || (uint32_t)j * 1024u + lane * 16u < (uint32_t)OUTB) ? ooff : kOut;
    __builtin_amdgcn_raw_buffer_store_b128(w, ors, off, (uint32_t)(j * (1024 / ROWB)) * a.qs_h, 2 /* non-temporal */);
  }
}

// ---------------------------------------------------------------------------- wide tile (single pass, 16384 < B*H*D <= 131072)
// A batched slice too large for the one-wave tile — an un-sharded batch of 32 / 64 rows of Llama-3-8B: R = B*H = 256 / 512
// head rows of 128 — still read ONCE: a 1024-thread workgroup owns TT tokens x ALL R rows (TT * R * D = up to 131072
// elements = 256 KiB of fp16) and keeps them in REGISTERS (NV = 16 vectors of 8 elements per lane, 64 of the 128 VGPRs a
// lane of such a workgroup has), one workgroup per CU. Lane = (row-in-round, token, d-vector): in round i it holds row
// i * RPR + lane_row, so its (token, d-vector) never changes and the abs-max across rows is a register max, then DPP across
// the token's D/8 lanes, a lane exchange across the rows that share a wave, ONE LDS atomic per token per wave. Every load is
// issued before the first is used; the row of a round is the lane's first row plus a uniform stride per round (the host
// admits only layouts where that holds: B*H rows evenly spaced, or rows-per-round a multiple of H).
// Same arithmetic per element as every other quantise kernel (quotient_bits8 / pack_*): bit-identical.
// Against the alternatives for these shapes (Llama-3-8B batch 64 x 512 tokens, profiles/r03w_*): two passes of the one-wave
// tile kernels 3.6 TB/s of single-pass bytes, the swept tile 2.5.
struct QuantWideArgs {
  PtrTable in;
  uint8_t* q;
  float* scales;
  int64_t qs_g, ssg;
  int64_t is_b, is_h, qs_b, qs_h;  // BYTES
  int64_t is_round, qs_round;      // bytes between a lane's rows of consecutive rounds
  uint32_t H, R, T, D;
  uint32_t vshift, dvshift;        // log2(vectors per row run = TT * D/8), log2(D/8)
  float eps;
};

template <int IDT, int BITS, int BLK, int NV>
__global__ __launch_bounds__(BLK) void quant_wide_k(const QuantWideArgs a) {
  static_assert(IDT != KVQ_F32, "two-byte inputs (an fp32 tile of this size does not fit the register file)");
  __shared__ uint32_t s_amax[kMaxTT];
  __shared__ float s_scale[kMaxTT], s_rcp[kMaxTT];
  const uint32_t tid = threadIdx.x, g = blockIdx.y;
  const uint32_t TT = 1u << (a.vshift - a.dvshift), DV = 1u << a.dvshift;
  const uint32_t t0 = blockIdx.x * TT;
  const uint32_t wv = tid & ((1u << a.vshift) - 1u), lr = tid >> a.vshift, tl = wv >> a.dvshift;
  const uint32_t RPR = (uint32_t)BLK >> a.vshift;  // rows per round
  const bool tok_ok = t0 + tl < a.T;
  const uint32_t lb = lr / a.H, lh = lr - lb * a.H;
  const char* in = reinterpret_cast<const char*>(a.in.p[g]) + (int64_t)lb * a.is_b + (int64_t)lh * a.is_h + ((int64_t)t0 * a.D + (int64_t)wv * 8) * 2;
  uint8_t* qp = a.q + (int64_t)g * a.qs_g + (int64_t)lb * a.qs_b + (int64_t)lh * a.qs_h + (int64_t)t0 * (a.D * BITS / 8) + (int64_t)wv * BITS;
  if (tid < (uint32_t)kMaxTT) s_amax[tid] = 0u;
  __syncthreads();

  Vec8<IDT> x[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    x[i].w = u32x4{0u, 0u, 0u, 0u};  // rows past R, tokens past T: cannot raise an abs-max, never stored
    if (tok_ok && (uint32_t)i * RPR + lr < a.R) x[i].load_nt(in + (int64_t)i * a.is_round);
  }
  uint32_t m = 0u;
#pragma unroll
  for (int i = 0; i < NV; ++i) m = max(m, x[i].absmax_bits());
  m = group_umax(m, (int)a.dvshift);                                                            // the token's D/8 lanes
  for (uint32_t sh = a.vshift; sh < 6u; ++sh) m = max(m, (uint32_t)__shfl_xor((int)m, 1 << sh));  // rows sharing the wave
  if ((wv & (DV - 1u)) == 0u && ((tid & 63u) >> a.vshift) == 0u && tok_ok) atomicMax(&s_amax[tl], m);
  __syncthreads();
  if (tid < TT && t0 + tid < a.T) {
    const float s32 = scale_of<BITS>(Vec8<IDT>::bits_to_f32(s_amax[tid]), a.eps);
    s_scale[tid] = s32;
    s_rcp[tid] = 1.0f / s32;
    a.scales[(int64_t)g * a.ssg + t0 + tid] = Elem<IDT>::round_trip(s32);
  }
  __syncthreads();
  const float s32 = s_scale[tl], rcp = s_rcp[tl], thr = guard_threshold<BITS>(s32);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (tok_ok && (uint32_t)i * RPR + lr < a.R) {
      uint32_t qb[8];
      quotient_bits8<BITS>(x[i], s32, rcp, thr, qb);
      uint8_t* dst = qp + (int64_t)i * a.qs_round;
      if constexpr (BITS == 8) __builtin_nontemporal_store(pack_i8(qb), reinterpret_cast<u32x2*>(dst));
      else __builtin_nontemporal_store(pack_i4(qb), reinterpret_cast<uint32_t*>(dst));
    }
  }
}



// ---------------------------------------------------------------------------- swept tile (any R)
// Batched slices whose B*H*D exceeds the register tile (e.g. B = 64): the workgroup still owns
// TT tokens x all R rows of one group, but sweeps the rows twice in steps of `rpc` rows — once for
// the per-token abs-max (LDS), once to quantise. The second sweep re-reads what the workgroup has
// just read (tile sized to stay cache-resident), no global atomics, no workspace.
// POW2 = false: D/8 is not a power of two (D = 80, 96, 160, 192 ...) or exceeds one wave: index
// decomposition by 32-bit division and one LDS atomic per lane instead of the DPP group max.
template <int IDT, int BITS, bool POW2>
__global__ __launch_bounds__(kBlock) void quant_tokens_sweep_k(const QuantArgs a) {
  __shared__ uint32_t s_amax[kMaxTT];
  __shared__ float s_scale[kMaxTT], s_rcp[kMaxTT];
  const uint32_t tid = threadIdx.x;
  const uint32_t g = blockIdx.y;
  const uint32_t t0 = a.t_begin + blockIdx.x * a.TT;
  const uint32_t DV = a.D >> 3;
  const uint32_t wmask = POW2 ? (1u << a.vshift) - 1u : 0u;
  const char* in = reinterpret_cast<const char*>(a.in.p[g]) + (int64_t)t0 * a.is.t * Elem<IDT>::size;
  uint8_t* qbase = a.q + (int64_t)g * a.qs.g + (int64_t)t0 * a.qs.t;
  constexpr int QV = BITS;
  // vector index in a sweep step -> (row in step, vector in the row's TT-token run, token in tile)
  auto split = [&](uint32_t v, uint32_t& rl, uint32_t& wv, uint32_t& tl) {
    if constexpr (POW2) {
      rl = v >> a.vshift;
      wv = v & wmask;
      tl = wv >> a.dvshift;
    } else {
      rl = v / a.vpr;
      wv = v - rl * a.vpr;
      tl = wv / a.dv;
    }
  };
  auto in_row = [&](uint32_t r) -> int64_t {
    return a.bh_contig ? (int64_t)r * a.is.h : (int64_t)(r / a.H) * a.is.b + (int64_t)(r % a.H) * a.is.h;
  };
  auto q_row = [&](uint32_t r) -> int64_t {
    return a.bh_contig ? (int64_t)r * a.qs.h : (int64_t)(r / a.H) * a.qs.b + (int64_t)(r % a.H) * a.qs.h;
  };

  if (tid < kMaxTT) s_amax[tid] = 0u;
  __syncthreads();

  for (uint32_t r0 = 0; r0 < a.R; r0 += a.rpc) {  // sweep 1: abs-max
    const uint32_t rows = a.R - r0 < a.rpc ? a.R - r0 : a.rpc;
    const uint32_t nv = POW2 ? rows << a.vshift : rows * a.vpr;
#pragma unroll
    for (int i = 0; i < kNVMax; ++i) {
      if ((uint32_t)(i * kBlock) < nv) {  // uniform
        const uint32_t v = i * kBlock + tid;
        uint32_t rl, wv, tl;
        split(v, rl, wv, tl);
        const bool ok = v < nv && t0 + tl < a.T;
        uint32_t m = 0u;
        if (ok) {
          Vec8<IDT> x;
          x.load(in + (in_row(r0 + rl) + (int64_t)wv * 8) * Elem<IDT>::size);
          m = x.absmax_bits();
        }
        if constexpr (POW2) {
          m = group_umax(m, a.dvshift);
          if (ok && (wv & (DV - 1u)) == 0u) atomicMax(&s_amax[tl], m);
        } else {
          if (ok) atomicMax(&s_amax[tl], m);
        }
      }
    }
  }
  __syncthreads();
  if (tid < a.TT && t0 + tid < a.T) {
    const float amax = Vec8<IDT>::bits_to_f32(s_amax[tid]);
    const float s32 = scale_of<BITS>(amax, a.eps);
    s_scale[tid] = s32;
    s_rcp[tid] = 1.0f / s32;
    a.scales[(int64_t)g * a.ssg + t0 + tid] = Elem<IDT>::round_trip(s32);
  }
  __syncthreads();

  for (uint32_t r0 = 0; r0 < a.R; r0 += a.rpc) {  // sweep 2: quantise
    const uint32_t rows = a.R - r0 < a.rpc ? a.R - r0 : a.rpc;
    const uint32_t nv = POW2 ? rows << a.vshift : rows * a.vpr;
#pragma unroll
    for (int i = 0; i < kNVMax; ++i) {
      const uint32_t v = i * kBlock + tid;
      uint32_t rl, wv, tl;
      split(v, rl, wv, tl);
      if (v < nv && t0 + tl < a.T) {
        const uint32_t r = r0 + rl;
        Vec8<IDT> x;
        x.load(in + (in_row(r) + (int64_t)wv * 8) * Elem<IDT>::size);
        uint32_t qb[8];
        quotient_bits8<BITS>(x, s_scale[tl], s_rcp[tl], guard_threshold<BITS>(s_scale[tl]), qb);
        uint8_t* qp = qbase + q_row(r) + (int64_t)wv * QV;
        if constexpr (BITS == 8) *reinterpret_cast<u32x2*>(qp) = pack_i8(qb);
        else *reinterpret_cast<uint32_t*>(qp) = pack_i4(qb);
      }
    }
  }
}

// ---------------------------------------------------------------------------- generic two-pass
// Any D (odd included), any strides / alignment, any B*H*D size.
template <int IDT>
__global__ __launch_bounds__(kBlock) void absmax_tokens_generic_k(const QuantArgs a, uint32_t chunks_per_tok,
                                                                  int64_t chunk_elems) {
  __shared__ float s_red[kBlock / kWave];
  const uint32_t g = blockIdx.y;
  const uint32_t t = blockIdx.x / chunks_per_tok;
  const uint32_t c = blockIdx.x - t * chunks_per_tok;
  const int64_t RD = (int64_t)a.R * a.D;
  const int64_t i0 = (int64_t)c * chunk_elems;
  int64_t i1 = i0 + chunk_elems;
  if (i1 > RD) i1 = RD;
  const void* in = a.in.p[g];
  float m = 0.0f;
#pragma unroll 1  // generic fallback: four 64-bit divisions per element; unrolled it is 5,600 instructions per instantiation
  for (int64_t i = i0 + threadIdx.x; i < i1; i += kBlock) {
    const int64_t d = i % a.D;
    const int64_t r = i / a.D;
    const int64_t h = r % a.H;
    const int64_t b = r / a.H;
    m = max_nonneg(m, fabsf(load1<IDT>(in, b * a.is.b + h * a.is.h + (int64_t)t * a.is.t + d)));
  }
  m = block_max_nonneg(m, s_red);
  if (threadIdx.x == 0)
    atomicMax(reinterpret_cast<uint32_t*>(a.absmax_ws) + (int64_t)g * a.T + t, __float_as_uint(m));
}

// One thread per output byte: INT8 one element, INT4 two elements (second may be the odd-D pad).
template <int IDT, int BITS>
__global__ __launch_bounds__(kBlock) void quant_tokens_generic_k(const QuantArgs a, int64_t total_bytes) {
  const int64_t Dq = BITS == 8 ? a.D : (a.D + 1) / 2;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total_bytes; i += (int64_t)gridDim.x * kBlock) {
    const int64_t j = i % Dq;
    int64_t r = i / Dq;
    const int64_t t = r % a.T;
    r /= a.T;
    const int64_t h = r % a.H;
    r /= a.H;
    const int64_t b = r % a.B;
    const int64_t g = r / a.B;
    const float amax = a.absmax_ws[g * a.T + t];
    const float s32 = scale_of<BITS>(amax, a.eps);
    const void* in = a.in.p[g];
    const int64_t ioff = b * a.is.b + h * a.is.h + t * a.is.t;
    uint8_t* qp = a.q + g * a.qs.g + b * a.qs.b + h * a.qs.h + t * a.qs.t;
    if constexpr (BITS == 8) {
      qp[j] = (uint8_t)(int8_t)quant1<8>(load1<IDT>(in, ioff + j), s32);
    } else {
      const int hi = quant1<4>(load1<IDT>(in, ioff + 2 * j), s32) + 8;
      const int lo = (2 * j + 1 < (int64_t)a.D) ? quant1<4>(load1<IDT>(in, ioff + 2 * j + 1), s32) + 8 : 8;
      qp[j] = (uint8_t)(((hi & 0xF) << 4) | (lo & 0xF));
    }
    if (b == 0 && h == 0 && j == 0) a.scales[g * a.ssg + t] = Elem<IDT>::round_trip(s32);
  }
}

// ---------------------------------------------------------------------------- split phases (sharded batch)
// A [B>1,H,1,D] slice whose batch rows are split over ranks still has ONE scale per token (ops.py:27,48:
// abs().max() of the whole slice), so the fused kernels above cannot be used: the abs-max table must
// cross ranks between the reduction and the quantisation (one all_reduce(MAX) of [G,T] fp32).
//   absmax_tokens_tile_k        local rows -> absmax[g,t]
//   quant_tokens_scaled_tile_k  quantise with the GIVEN abs-max values; same quotient / pack / scale code as
//                               the fused kernels, so a 1-rank run is bit-identical with them
// 16-byte vectors; shapes that do not qualify (D % 8, D/8 not a power of two or > 64, token rows not contiguous,
// unaligned) take the generic pair (same arithmetic, scalar accesses; its abs-max table is zeroed first).
// Tile ownership as in the fused kernels: a workgroup owns TT tokens of one group (TT * D/8 = tvec vectors per row run,
// a power of two <= 256) and walks the R = B*H rows, nrs = 256 / tvec of them side by side. The abs-max kernel needs
// no global atomics (the tile's tokens are nobody else's: register max over the rows, DPP over the D/8 lanes of a
// token, LDS max across the side-by-side rows); the quantise kernel computes scale and reciprocal once per lane.
template <int IDT>
__global__ __launch_bounds__(kBlock) void absmax_tokens_tile_k(const QuantArgs a) {
  __shared__ uint32_t s_amax[kBlock];
  const uint32_t tid = threadIdx.x, g = blockIdx.y;
  const uint32_t tvec = 1u << a.vshift, nrs = kBlock >> a.vshift;
  const uint32_t rs = tid >> a.vshift, wv = tid & (tvec - 1u), tl = wv >> a.dvshift;
  const uint32_t t0 = blockIdx.x * a.TT;
  const bool ok = t0 + tl < a.T;
  const char* in = reinterpret_cast<const char*>(a.in.p[g]) + ((int64_t)t0 * a.is.t + (int64_t)wv * 8) * Elem<IDT>::size;
  if (tid < a.TT) s_amax[tid] = 0u;
  __syncthreads();
  uint32_t m = 0u;
  if (ok) {
    for (uint32_t r = rs; r < a.R; r += nrs) {
      Vec8<IDT> x;
      x.load(in + ((int64_t)(r / a.H) * a.is.b + (int64_t)(r % a.H) * a.is.h) * Elem<IDT>::size);
      m = max(m, x.absmax_bits());
    }
  }
  m = group_umax(m, a.dvshift);
  if (ok && (wv & ((1u << a.dvshift) - 1u)) == 0u) atomicMax(&s_amax[tl], m);
  __syncthreads();
  if (tid < a.TT && t0 + tid < a.T) {
    float* dst = a.absmax_ws + (int64_t)g * a.T + t0 + tid;
    const float v = Vec8<IDT>::bits_to_f32(s_amax[tid]);
    *dst = a.acc ? max_keep_nan(*dst, v) : v;  // the tile's tokens are nobody else's: no atomic needed
  }
}

template <int IDT, int BITS>
__global__ __launch_bounds__(kBlock) void quant_tokens_scaled_tile_k(const QuantArgs a) {
  const uint32_t tid = threadIdx.x, g = blockIdx.y;
  const uint32_t tvec = 1u << a.vshift, nrs = kBlock >> a.vshift;
  const uint32_t rs = tid >> a.vshift, wv = tid & (tvec - 1u), tl = wv >> a.dvshift;
  const uint32_t t0 = blockIdx.x * a.TT;
  if (t0 + tl >= a.T) return;
  constexpr int QV = BITS;
  const char* in = reinterpret_cast<const char*>(a.in.p[g]) + ((int64_t)t0 * a.is.t + (int64_t)wv * 8) * Elem<IDT>::size;
  uint8_t* q = a.q + (int64_t)g * a.qs.g + (int64_t)(t0 + tl) * a.qs.t + (int64_t)(wv & ((1u << a.dvshift) - 1u)) * QV;
  const float s32 = scale_of<BITS>(a.absmax_ws[(int64_t)g * a.T + t0 + tl], a.eps);
  const float rcp = 1.0f / s32, thr = guard_threshold<BITS>(s32);
  if (rs == 0u && (wv & ((1u << a.dvshift) - 1u)) == 0u) a.scales[(int64_t)g * a.ssg + t0 + tl] = Elem<IDT>::round_trip(s32);
  for (uint32_t r = rs; r < a.R; r += nrs) {
    const uint32_t b = r / a.H, h = r % a.H;
    Vec8<IDT> x;
    x.load(in + ((int64_t)b * a.is.b + (int64_t)h * a.is.h) * Elem<IDT>::size);
    uint32_t qb[8];
    quotient_bits8<BITS, true>(x, s32, rcp, thr, qb);  // the caller's table may be below the data
    uint8_t* qp = q + (int64_t)b * a.qs.b + (int64_t)h * a.qs.h;
    if constexpr (BITS == 8) *reinterpret_cast<u32x2*>(qp) = pack_i8(qb);
    else *reinterpret_cast<uint32_t*>(qp) = pack_i4(qb);
  }
}

// PHASE 1 for a slice of few tokens (a batch-sharded DECODE APPEND: T = 1; up to tunables().quant_few_tokens = 16). The tile walk gives every 8-row group its own
// one-wave workgroup, and all rows / 8 of them end in an atomicMax on the SAME word of the table: device-scope atomics from
// eight XCDs on one address are served one after the other — 21.5 us for the 8.4 MB of a batch-64 K + V append of 64 tensors
// (rocprofv3: profiles/r04z_rocprofv3_kernel_stats_shardq_append.csv, quant_tile_k<..., 1>). Here ONE 256-thread workgroup
// owns a (group, token): 256 / DV rows per pass, 8 independent 16-byte loads per thread in flight, LDS across its 4 waves,
// then ONE plain store — or a plain max with the word when the caller accumulates (no other workgroup of the launch touches
// it) — no atomics, and no memset launch in front. The maximum does not depend on the order: same table, bit for bit.
// Against the tile walk on [64, 64, 8, T, 128] fp16 (profiles/r04aa_absmax_few_tokens_sweep.jsonl): T = 1 4.3 vs 21.2 us, 2: 4.3 vs
// 11.6, 4: 7.9 vs 10.3, 8: 10.7 vs 13.0, 16: 20.9 vs 21.1, 32: 47.2 vs 48.9, 64: 94.4 vs 90.1 — the default threshold is 16.
template <int IDT, int DV>
__global__ __launch_bounds__(kBlock) void absmax_fewtokens_k(const QuantTileArgs a, const int accumulate) {
  static_assert(IDT != KVQ_F32, "two-byte inputs");
  constexpr int D = DV * 8;
  constexpr int RPP = kBlock / DV;  // rows per pass
  constexpr int UN = 8;
  __shared__ uint32_t s_m[kBlock / kWave];
  const uint32_t tid = threadIdx.x, t = blockIdx.x, g = blockIdx.y;
  const uint32_t piece = tid % DV, slot = tid / DV;
  const char* base = reinterpret_cast<const char*>(a.in.p[g]) + (int64_t)t * (D * 2) + piece * 16u;
  uint32_t m = 0u;
  for (uint32_t r0 = slot; r0 < a.rows; r0 += (uint32_t)(RPP * UN)) {
    Vec8<IDT> x[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const uint32_t r = r0 + (uint32_t)(u * RPP);
      x[u].w = u32x4{0u, 0u, 0u, 0u};
      if (r < a.rows) x[u].w = *reinterpret_cast<const u32x4*>(base + (int64_t)r * a.is_h);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) m = max(m, x[u].absmax_bits());
  }
  m = group_umax(m, 6);  // the whole wave
  if ((tid & 63u) == 0u) s_m[tid >> 6] = m;
  __syncthreads();
  if (tid == 0u) {
    m = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
    float* dst = a.absmax + (int64_t)g * a.T + t;
    float v = Vec8<IDT>::bits_to_f32(m);
    if (accumulate) v = max_keep_nan(v, *dst);
    *dst = v;
  }
}

// ---------------------------------------------------------------------------- host side

static uint32_t pow2_floor(uint64_t v) {
  uint32_t p = 1;
  while ((uint64_t)p * 2 <= v) p *= 2;
  return p;
}

// One validated call of a quantise entry point (phase 1 of the split pair: q == scales == nullptr).
struct QuantCall {
  const void* in_base;
  const void* const* in_ptrs;
  Strides is;           // input strides in elements
  Strides qs;           // store strides in bytes
  int dtype, esz, bits;  // bits of the store; 8 in the abs-max phase (which never looks at it)
  uint8_t* q;
  float* scales;
  int64_t ssg;
  float* absmax;        // [G, T] fp32: workspace of the quantise entry points (may be nullptr), table of the split phases
  float eps;
  bool accumulate;      // abs-max phase: max with what the table holds
  int64_t G, B, H, T, D, R;  // R = B * H
  hipStream_t st;
  const char* name;
};

static QuantCall quant_call(const char* name, int bits, const void* in_base, const void* const* in_ptrs,
                            const kvq_strides_t* in_st, int in_dtype, uint8_t* q, const kvq_strides_t* q_st, float* scales,
                            int64_t ssg, float* absmax, float eps, const kvq_dims_t* d, void* stream, bool accumulate) {
  QuantCall c = {};
  c.in_base = in_base;
  c.in_ptrs = in_ptrs;
  c.is = to_strides(in_st);
  if (q_st) c.qs = to_strides(q_st);
  c.dtype = in_dtype;
  c.esz = in_dtype == KVQ_F32 ? 4 : 2;
  c.bits = bits;
  c.q = q;
  c.scales = scales;
  c.ssg = ssg;
  c.absmax = absmax;
  c.eps = eps;
  c.accumulate = accumulate;
  c.G = d->G; c.B = d->B; c.H = d->H; c.T = d->T; c.D = d->D;
  c.R = d->B * d->H;
  c.st = reinterpret_cast<hipStream_t>(stream);
  c.name = name;
  return c;
}

static bool dims_too_large(const kvq_dims_t* d) {
  return d->B >= (int64_t(1) << 31) || d->H >= (int64_t(1) << 31) || d->T >= (int64_t(1) << 31) ||
         d->D >= (int64_t(1) << 31) || d->B * d->H >= (int64_t(1) << 31);
}

static int check_in_dtype(int in_dtype, const char* name) {
  if (in_dtype == KVQ_F16 || in_dtype == KVQ_BF16 || in_dtype == KVQ_F32) return 0;
  set_error("%s: unknown in_dtype %d", name, in_dtype);
  return KVQ_E_DTYPE;
}

// QuantArgs of groups [g0, g0 + gn): the fields every kernel reads; a family's launcher adds its geometry.
static int chunk_args(const QuantCall& c, int64_t g0, int64_t gn, QuantArgs& a) {
  a = {};
  if (const int rc = fill_ptrs(a.in, c.in_base, c.in_ptrs, g0, gn, c.is.g * c.esz, 0, c.name)) return rc;
  a.is = c.is;
  a.qs = c.qs;
  a.q = c.q ? c.q + g0 * c.qs.g : nullptr;
  a.scales = c.scales ? c.scales + g0 * c.ssg : nullptr;
  a.ssg = c.ssg;
  a.absmax_ws = c.absmax ? c.absmax + g0 * c.T : nullptr;
  a.eps = c.eps;
  a.G = (uint32_t)gn;
  a.B = (uint32_t)c.B; a.H = (uint32_t)c.H; a.T = (uint32_t)c.T; a.D = (uint32_t)c.D;
  a.R = (uint32_t)c.R;
  a.acc = c.accumulate ? 1 : 0;
  return 0;
}

// ---- routing of kvq_quant_i8_tokens / kvq_quant_i4_tokens (quant_route): first match wins ---------------------------
//  Tile      quant_tile_k<IDT,BITS,R,DV,TT,0>: quant_tile on, quant_force_two_pass off, fp16 / bf16; rows and tokens
//            contiguous on both sides, 16-byte row strides, 16-byte aligned store; (D, R) = (128, 8) [TT 4], (64, 8) [TT 8],
//            or (64, 12) / (64, 16) [TT 8] in fp16 only; both spans < 2^31; every group pointer non-null and aligned.
//  Wide      quant_wide_k<IDT,BITS,1024,16>: 16384 < R*D <= 131072, D/8 a power of two <= 64, fp16 / bf16, quant_wide on,
//            the rows of one round step evenly through strided batch rows, every group pointer aligned.
//  Split     quant_tile_k<...,1> then <...,2> (split_route's walk, both phases): R*D > 16384, D/8 a power of two <= 64,
//            a workspace, split_walk_ok.
//  fused single pass, per launch chunk whose group pointers are all non-null and aligned (D % 8 == 0, tokens contiguous,
//  16-byte input strides, store strides a multiple of the bytes of one stored vector):
//    Sweep     quant_tokens_sweep_k: R*D > 16384 or D/8 not a power of two / > 64; fp16 / bf16 (larger fp32 -> Generic).
//    Wave      quant_tokens_fused_k<...,64,...>: quant_block 64, fp16 / bf16, R*D <= 4096, 16-byte store rows, row runs of
//              >= 64 vectors, TT <= T. Complete tiles (512 vectors) on the FULL kernel (REGMAX when a round is one row),
//              the rest on the ragged one.
//    Block256  quant_tokens_fused_k<...,256,...>: the other fused shapes. Complete tiles with row runs of >= 256 vectors
//              and LDS-staged stores on the FULL kernel, the rest on the ragged one, LDS-staged unless
//              quant_direct_stores or the store rows are not 16-byte aligned.
//  Generic   absmax_tokens_generic_k + quant_tokens_generic_k, per chunk: the rest. Needs the workspace (KVQ_E_NULL).
enum class Quant { Tile, Wide, Split, Sweep, Wave, Block256, Generic };

struct QuantRoute {
  Quant fam;
  uint32_t tt;              // tokens per workgroup tile
  int32_t dvshift, vshift;  // log2(D/8), log2(tt * D/8): Wide, Wave, Block256
  uint32_t nvec;            // Wave, Block256: R * tt * D/8 vectors per tile
  uint32_t n_full;          // Wave, Block256: complete tiles launched on the FULL kernel; the rest go to the ragged one
  bool regmax;              // Wave: one round of the wave is one row
  bool lds_out;             // Block256: ragged tiles stage their stores through LDS
  uint32_t dv, vpr, rpc;    // Sweep: D/8, tt * D/8 vectors per row run, rows per sweep step
};

constexpr int kWideBlk = 1024;
constexpr int kWideNV = 16;

// Can the one-wave tile kernels over 8-row groups (quant_tile_k PHASE 1 / 2) serve this call? c.q == nullptr: the
// abs-max phase alone (no store side to check). Head_dim 64 takes the 256-thread pair.
static bool split_walk_ok(const QuantCall& c, bool all_aligned) {
  const Strides &is = c.is, &qs = c.qs;
  bool ok = tunables().quant_tile && c.dtype != KVQ_F32 && c.D == 128 && (c.T == 1 || is.t == c.D) &&
            (c.B == 1 || is.b == c.H * is.h) && (is.h * 2) % 16 == 0 && is.h >= 0 &&
            (c.R - 1) * is.h * 2 + 8 * c.D * 2 < (int64_t(1) << 31) && (c.R + 7) / 8 < 65536;
  if (c.q)
    ok = ok && (c.T == 1 || qs.t == c.D * c.bits / 8) && (c.B == 1 || qs.b == c.H * qs.h) && qs.h % 16 == 0 &&
         qs.g % 16 == 0 && qs.h >= 0 && (c.D * c.bits / 8) % 16 == 0 && aligned(c.q, 16) &&
         (c.R - 1) * qs.h + 8 * c.D < (int64_t(1) << 31);
  return ok && all_aligned;
}

static QuantRoute quant_route(const QuantCall& c, bool all_aligned, bool chunk_aligned) {
  const Tunables& tu = tunables();
  const Strides &is = c.is, &qs = c.qs;
  const int64_t R = c.R, D = c.D, Dq = c.bits == 8 ? D : (D + 1) / 2;
  const int64_t qvec = c.bits == 8 ? 8 : 4;  // bytes stored per 8-element vector
  const bool two_byte = c.dtype != KVQ_F32;
  const bool t_contig = c.T == 1 || (is.t == D && qs.t == Dq);
  const bool in_contig = c.B == 1 || is.b == c.H * is.h, q_contig = c.B == 1 || qs.b == c.H * qs.h;
  const int dvshift = D % 8 == 0 ? ilog2_exact(D / 8) : -1;
  QuantRoute r = {};

  if (tu.quant_tile && !tu.quant_force_two_pass && two_byte && in_contig && q_contig && t_contig && (is.h * 2) % 16 == 0 &&
      qs.h % 16 == 0 && qs.g % 16 == 0 && (D * c.bits / 8) % 16 == 0 && aligned(c.q, 16) && is.h >= 0 && qs.h >= 0) {
    r.tt = D == 128 && R == 8 ? 4 : D == 64 && (R == 8 || ((R == 12 || R == 16) && c.dtype == KVQ_F16)) ? 8 : 0;
    const int64_t span_in = (R - 1) * is.h * 2 + (int64_t)r.tt * D * 2, span_q = (R - 1) * qs.h + (int64_t)r.tt * Dq;
    if (r.tt && span_in < (int64_t(1) << 31) && span_q < (int64_t(1) << 31) && all_aligned) {
      r.fam = Quant::Tile;
      return r;
    }
  }

  const bool anydv = D % 8 == 0 && (dvshift < 0 || D / 8 > kWave);  // swept tile with division-based indexing
  const bool big = anydv || R * D > kTileElems;                     // larger than the register tile
  const int64_t wide_cap = (int64_t)kWideBlk * kWideNV * 8;          // elements a wide workgroup holds
  if (big && !anydv && two_byte && tu.quant_wide != 0 && !tu.quant_force_two_pass && t_contig && (is.b * c.esz) % 16 == 0 &&
      (is.h * c.esz) % 16 == 0 && qs.b % qvec == 0 && qs.h % qvec == 0 && qs.g % qvec == 0 && aligned(c.q, qvec) &&
      R * D <= wide_cap) {
    uint32_t tt = pow2_floor((uint64_t)(wide_cap / (R * D)));
    if (tt > (uint32_t)kMaxTT) tt = kMaxTT;
    while (tt > 1 && tt / 2 >= (uint64_t)c.T) tt /= 2;
    const int vshift = dvshift + ilog2_exact((int64_t)tt);
    const int64_t rpr = kWideBlk >> vshift;  // rows per round, >= 2: tt * D/8 <= cap / (8 R) < 512 since R * D > 16384
    if ((in_contig || rpr % c.H == 0) && (q_contig || rpr % c.H == 0) && all_aligned) {
      r.fam = Quant::Wide;
      r.tt = tt;
      r.dvshift = dvshift;
      r.vshift = vshift;
      return r;
    }
  }

  if (big && !anydv && c.absmax && !tu.quant_force_two_pass && split_walk_ok(c, all_aligned)) {
    r.fam = Quant::Split;
    return r;
  }

  const bool fused = !tu.quant_force_two_pass && D % 8 == 0 && D <= kTileElems && t_contig &&
                     (big ? two_byte : in_contig && q_contig) && (is.b * c.esz) % 16 == 0 && qs.b % qvec == 0 &&
                     (is.h * c.esz) % 16 == 0 && (is.t * c.esz) % 16 == 0 && qs.h % qvec == 0 && qs.t % qvec == 0 &&
                     qs.g % qvec == 0 && aligned(c.q, qvec);
  if (!fused || !chunk_aligned) {
    r.fam = Quant::Generic;
    return r;
  }

  if (big) {  // power-of-two shapes this large take Wide or Split when they can
    int64_t tt = (256 * 1024) / (R * D * c.esz);
    if (tt < 1) tt = 1;
    if (tt > kMaxTT) tt = kMaxTT;
    if (tt * (D / 8) > kBlock * kNVMax) tt = (kBlock * kNVMax) / (D / 8);  // >= 1: D <= kTileElems
    if (tt > c.T) tt = c.T;
    r.fam = Quant::Sweep;
    r.tt = (uint32_t)tt;
    r.dv = (uint32_t)(D / 8);
    r.vpr = (uint32_t)(tt * (D / 8));
    r.rpc = (uint32_t)((kBlock * kNVMax) / r.vpr);
    return r;
  }

  // LDS-staged 16-byte stores need 16-byte aligned row runs in the store
  const bool store16 = (D * c.bits / 8) % 16 == 0 && qs.g % 16 == 0 && qs.h % 16 == 0 && qs.t % 16 == 0 && aligned(c.q, 16);
  r.dvshift = dvshift;
  const int64_t tile64 = 64 * kNVMax * 8;
  if (two_byte && tu.quant_block == 64 && R * D <= tile64 && store16) {
    uint32_t t64 = pow2_floor((uint64_t)(tile64 / (R * D)));
    if (t64 > (uint32_t)kMaxTT) t64 = kMaxTT;
    if ((int64_t)t64 * (D / 8) >= 64 && (int64_t)t64 <= c.T) {  // every row run >= 64 vectors (ROWU)
      r.fam = Quant::Wave;
      r.tt = t64;
      r.vshift = dvshift + ilog2_exact(t64);
      r.nvec = (uint32_t)(R * t64 * (D / 8));
      r.regmax = (1 << r.vshift) == 64;
      r.n_full = r.nvec == (uint32_t)(64 * kNVMax) ? (uint32_t)(c.T / t64) : 0u;
      return r;
    }
  }
  uint32_t tt = pow2_floor((uint64_t)(kTileElems / (R * D)));
  if (tt > (uint32_t)kMaxTT) tt = kMaxTT;
  while (tt > 1 && tt / 2 >= (uint64_t)c.T) tt /= 2;  // do not over-tile short appends
  r.fam = Quant::Block256;
  r.tt = tt;
  r.vshift = dvshift + ilog2_exact(tt);
  r.nvec = (uint32_t)(R * tt * (D / 8));
  r.lds_out = !tu.quant_direct_stores && store16;
  r.n_full = r.nvec == (uint32_t)(kBlock * kNVMax) && r.vshift >= 8 && r.lds_out ? (uint32_t)(c.T / tt) : 0u;
  return r;
}

// ---- routing of the split phases (split_route; kvq_absmax_tokens[_acc] = phase 1, kvq_quant_tokens_from_absmax = 2) ---
//  Few      absmax_fewtokens_k<IDT,16>: phase 1, split_walk_ok, T <= quant_few_tokens and R > 8. One workgroup per
//           (group, token), no memset. (split_walk_ok means D = 128: the <IDT,8> instantiation is never launched.)
//  Walk     quant_tile_k<IDT,BITS,8,16,4,PHASE>: split_walk_ok. Phase 1 (BITS 8) zeroes the whole table once per call
//           unless it accumulates, then takes the atomicMax of 8-row groups.
//  Vec      absmax_tokens_tile_k / quant_tokens_scaled_tile_k: D/8 a power of two <= 64, tokens contiguous, 16-byte input
//           strides (phase 2: store strides in whole stored vectors), every group pointer of the launch chunk aligned.
//  Generic  absmax_tokens_generic_k / quant_tokens_generic_k, per chunk: the rest. Phase 1 zeroes the chunk's table
//           first unless it accumulates.
enum class Split { Few, Walk, Vec, Generic };

struct SplitRoute {
  Split fam;
  uint32_t tt;              // tokens per workgroup tile (Walk, Vec)
  int32_t dvshift, vshift;  // Vec: log2(D/8), log2(tt * D/8)
};

static SplitRoute split_route(const QuantCall& c, int phase, bool walk, bool chunk_aligned) {
  SplitRoute r = {};
  if (walk) {
    r.fam = phase == 1 && c.T <= tunables().quant_few_tokens && c.R > 8 ? Split::Few : Split::Walk;
    r.tt = c.D == 128 ? 4 : 8;
    return r;
  }
  const Strides &is = c.is, &qs = c.qs;
  const int64_t qvec = c.bits == 8 ? 8 : 4;
  const int dvshift = c.D % 8 == 0 ? ilog2_exact(c.D / 8) : -1;
  bool vec = chunk_aligned && dvshift >= 0 && dvshift <= 6 && (c.T == 1 || is.t == c.D) && (is.b * c.esz) % 16 == 0 &&
             (is.h * c.esz) % 16 == 0 && (is.t * c.esz) % 16 == 0;
  if (phase == 2)
    vec = vec && qs.g % qvec == 0 && qs.b % qvec == 0 && qs.h % qvec == 0 && qs.t % qvec == 0 && aligned(c.q, qvec);
  if (!vec) {
    r.fam = Split::Generic;
    return r;
  }
  uint32_t tt = pow2_floor((uint64_t)(kBlock >> dvshift));  // tile = TT tokens x D/8 vectors <= 256 vectors per row run
  while (tt > 1 && tt / 2 >= (uint64_t)c.T) tt /= 2;
  r.fam = Split::Vec;
  r.tt = tt;
  r.dvshift = dvshift;
  r.vshift = dvshift + ilog2_exact(tt);
  return r;
}

// ---- one launcher per family; `a` holds the chunk's groups -----------------------------------------------------------

static QuantTileArgs tile_args(const QuantCall& c, const QuantArgs& a) {
  QuantTileArgs ta;
  ta.in = a.in;
  ta.q = a.q;
  ta.scales = a.scales;
  ta.absmax = a.absmax_ws;
  ta.qs_g = c.qs.g;
  ta.ssg = c.ssg;
  ta.is_h = (uint32_t)(c.is.h * 2);
  ta.qs_h = (uint32_t)c.qs.h;
  ta.T = (uint32_t)c.T;
  ta.rows = (uint32_t)c.R;
  ta.eps = c.eps;
  return ta;
}

template <int BITS>
static void launch_tile(const QuantCall& c, const QuantRoute& r, const QuantArgs& a) {
  QuantTileArgs ta = tile_args(c, a);
  ta.absmax = nullptr;
  const dim3 grid((unsigned)((c.T + r.tt - 1) / r.tt), a.G);
  if (c.dtype == KVQ_F16) {
    if (c.D == 128) KVQ_LAUNCH((quant_tile_k<KVQ_F16, BITS, 8, 16, 4>), grid, dim3(kWave), 0, c.st, ta);
    else if (c.R == 8) KVQ_LAUNCH((quant_tile_k<KVQ_F16, BITS, 8, 8, 8>), grid, dim3(kWave), 0, c.st, ta);
    else if (c.R == 12) KVQ_LAUNCH((quant_tile_k<KVQ_F16, BITS, 12, 8, 8>), grid, dim3(kWave), 0, c.st, ta);
    else KVQ_LAUNCH((quant_tile_k<KVQ_F16, BITS, 16, 8, 8>), grid, dim3(kWave), 0, c.st, ta);
  } else if (c.D == 128) {
    KVQ_LAUNCH((quant_tile_k<KVQ_BF16, BITS, 8, 16, 4>), grid, dim3(kWave), 0, c.st, ta);
  } else {
    KVQ_LAUNCH((quant_tile_k<KVQ_BF16, BITS, 8, 8, 8>), grid, dim3(kWave), 0, c.st, ta);
  }
}

template <int BITS>
static void launch_wide(const QuantCall& c, const QuantRoute& r, const QuantArgs& a) {
  const bool in_contig = c.B == 1 || c.is.b == c.H * c.is.h, q_contig = c.B == 1 || c.qs.b == c.H * c.qs.h;
  const int64_t rpr = kWideBlk >> r.vshift;
  QuantWideArgs wa;
  wa.in = a.in;
  wa.q = a.q;
  wa.scales = a.scales;
  wa.qs_g = c.qs.g;
  wa.ssg = c.ssg;
  wa.is_h = c.is.h * c.esz;
  wa.is_b = in_contig ? c.H * wa.is_h : c.is.b * c.esz;
  wa.qs_h = c.qs.h;
  wa.qs_b = q_contig ? c.H * wa.qs_h : c.qs.b;
  wa.is_round = in_contig ? rpr * wa.is_h : rpr / c.H * wa.is_b;
  wa.qs_round = q_contig ? rpr * wa.qs_h : rpr / c.H * wa.qs_b;
  wa.H = (uint32_t)c.H;
  wa.R = (uint32_t)c.R;
  wa.T = (uint32_t)c.T;
  wa.D = (uint32_t)c.D;
  wa.vshift = (uint32_t)r.vshift;
  wa.dvshift = (uint32_t)r.dvshift;
  wa.eps = c.eps;
  const dim3 grid((unsigned)((c.T + r.tt - 1) / r.tt), a.G);
  if (c.dtype == KVQ_F16) KVQ_LAUNCH((quant_wide_k<KVQ_F16, BITS, kWideBlk, kWideNV>), grid, dim3(kWideBlk), 0, c.st, wa);
  else KVQ_LAUNCH((quant_wide_k<KVQ_BF16, BITS, kWideBlk, kWideNV>), grid, dim3(kWideBlk), 0, c.st, wa);
}

// Sweep, Wave, Block256: complete tiles [0, n_full) on the FULL kernel, tiles [n_full, tiles) on the ragged one
template <int IDT, int BITS>
static void launch_fused(const QuantCall& c, const QuantRoute& r, QuantArgs a) {
  a.TT = r.tt;
  a.dvshift = r.dvshift;
  a.vshift = r.vshift;
  a.nvec = r.nvec;
  a.dv = r.dv;
  a.vpr = r.vpr;
  a.rpc = r.rpc;
  a.bh_contig = c.B == 1 || (c.is.b == c.H * c.is.h && c.qs.b == c.H * c.qs.h);
  const unsigned tiles = (unsigned)((c.T + r.tt - 1) / r.tt), n_full = r.n_full, rest = tiles - n_full;
  const dim3 full_grid(n_full, a.G), rest_grid(rest, a.G);
  QuantArgs t = a;
  t.t_begin = n_full * r.tt;
  if (r.fam == Quant::Sweep) {
    if constexpr (IDT != KVQ_F32) KVQ_LAUNCH((quant_tokens_sweep_k<IDT, BITS, false>), dim3(tiles, a.G), dim3(kBlock), 0, c.st, a);
  } else if (r.fam == Quant::Wave) {
    if constexpr (IDT != KVQ_F32) {
      if (n_full && r.regmax)
        KVQ_LAUNCH((quant_tokens_fused_k<IDT, BITS, true, true, true, 64, true>), full_grid, dim3(64), 0, c.st, a);
      else if (n_full)
        KVQ_LAUNCH((quant_tokens_fused_k<IDT, BITS, true, true, true, 64>), full_grid, dim3(64), 0, c.st, a);
      if (rest) KVQ_LAUNCH((quant_tokens_fused_k<IDT, BITS, true, true, false, 64>), rest_grid, dim3(64), 0, c.st, t);
    }
  } else {
    if (n_full) KVQ_LAUNCH((quant_tokens_fused_k<IDT, BITS, true, true, true>), full_grid, dim3(kBlock), 0, c.st, a);
    if (rest && r.lds_out)
      KVQ_LAUNCH((quant_tokens_fused_k<IDT, BITS, false, true, false>), rest_grid, dim3(kBlock), 0, c.st, t);
    else if (rest)
      KVQ_LAUNCH((quant_tokens_fused_k<IDT, BITS, false, false, false>), rest_grid, dim3(kBlock), 0, c.st, t);
  }
}

// The generic pair, either half or both: abs-max into the chunk's [gn, T] table (zeroed first unless the caller
// accumulates), then quantise with it. 0, or KVQ_E_LAUNCH when the memset fails.
template <int IDT>
static int launch_generic(const QuantCall& c, const QuantArgs& a, bool absmax_phase, int quant_bits) {
  if (absmax_phase) {
    if (!c.accumulate && hipMemsetAsync(a.absmax_ws, 0, sizeof(float) * (size_t)(a.G * c.T), c.st) != hipSuccess)
      return check_launch(c.name);
    const int64_t chunk_elems = (int64_t)kBlock * 16;
    const uint32_t cpt = (uint32_t)((c.R * c.D + chunk_elems - 1) / chunk_elems);
    KVQ_LAUNCH((absmax_tokens_generic_k<IDT>), dim3((unsigned)(c.T * cpt), a.G), dim3(kBlock), 0, c.st, a, cpt, chunk_elems);
  }
  if (quant_bits) {
    const int64_t Dq = quant_bits == 8 ? c.D : (c.D + 1) / 2;
    const int64_t total = (int64_t)a.G * c.B * c.H * c.T * Dq;
    int64_t blocks = (total + kBlock - 1) / kBlock;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (quant_bits == 8) KVQ_LAUNCH((quant_tokens_generic_k<IDT, 8>), dim3((unsigned)blocks), dim3(kBlock), 0, c.st, a, total);
    else KVQ_LAUNCH((quant_tokens_generic_k<IDT, 4>), dim3((unsigned)blocks), dim3(kBlock), 0, c.st, a, total);
  }
  return 0;
}

// One split phase over all launch chunks (validated by the entry point, or by quant_tokens on the Split route).
static int run_split(const QuantCall& c, int phase) {
  const bool walk = split_walk_ok(c, ptrs_aligned16(c.in_base, c.in_ptrs, 0, c.G, c.is.g * c.esz));
  return for_launch_chunks(c.G, kPtrsPerLaunch, [&](int64_t g0, int64_t gn) -> int {
    QuantArgs a;
    if (const int rc = chunk_args(c, g0, gn, a)) return rc;
    const SplitRoute r = split_route(c, phase, walk, ptrs_aligned16(c.in_base, c.in_ptrs, g0, gn, c.is.g * c.esz));
    if (r.fam == Split::Walk && phase == 1 && !c.accumulate && g0 == 0 &&
        hipMemsetAsync(c.absmax, 0, sizeof(float) * (size_t)(c.G * c.T), c.st) != hipSuccess)
      return check_launch(c.name);
    int rc = 0;
    by_dtype(c.dtype, [&](auto idt) {
      constexpr int IDT = decltype(idt)::value;
      if (r.fam == Split::Few || r.fam == Split::Walk) {
        if constexpr (IDT != KVQ_F32) {
          const QuantTileArgs ta = tile_args(c, a);
          if (r.fam == Split::Few) {
            const dim3 grid((unsigned)c.T, a.G);
            if (c.D == 128) KVQ_LAUNCH((absmax_fewtokens_k<IDT, 16>), grid, dim3(kBlock), 0, c.st, ta, a.acc);
            else KVQ_LAUNCH((absmax_fewtokens_k<IDT, 8>), grid, dim3(kBlock), 0, c.st, ta, a.acc);
          } else {
            const dim3 grid((unsigned)((c.T + r.tt - 1) / r.tt), a.G, (unsigned)((c.R + 7) / 8));
            if (phase == 1) KVQ_LAUNCH((quant_tile_k<IDT, 8, 8, 16, 4, 1>), grid, dim3(kWave), 0, c.st, ta);
            else if (c.bits == 8) KVQ_LAUNCH((quant_tile_k<IDT, 8, 8, 16, 4, 2>), grid, dim3(kWave), 0, c.st, ta);
            else KVQ_LAUNCH((quant_tile_k<IDT, 4, 8, 16, 4, 2>), grid, dim3(kWave), 0, c.st, ta);
          }
        }
      } else if (r.fam == Split::Vec) {
        QuantArgs v = a;
        v.TT = r.tt;
        v.dvshift = r.dvshift;
        v.vshift = r.vshift;
        const dim3 grid((unsigned)((c.T + r.tt - 1) / r.tt), a.G);
        if (phase == 1) KVQ_LAUNCH((absmax_tokens_tile_k<IDT>), grid, dim3(kBlock), 0, c.st, v);
        else if (c.bits == 8) KVQ_LAUNCH((quant_tokens_scaled_tile_k<IDT, 8>), grid, dim3(kBlock), 0, c.st, v);
        else KVQ_LAUNCH((quant_tokens_scaled_tile_k<IDT, 4>), grid, dim3(kBlock), 0, c.st, v);
      } else {
        rc = launch_generic<IDT>(c, a, phase == 1, phase == 2 ? c.bits : 0);
      }
    });
    return rc ? rc : check_launch(c.name);
  });
}

template <int BITS>
static int quant_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, int in_dtype,
                        uint8_t* q, const kvq_strides_t* q_st, float* scales, int64_t ssg, float* absmax_ws,
                        float eps, const kvq_dims_t* d, void* stream, const char* name) {
  if (const int rc = check_group_call(in_st && q_st && q && scales, in_base, in_ptrs, q, d, name)) return rc;
  if (const int rc = check_in_dtype(in_dtype, name)) return rc;
  if (d->G * d->B * d->H * d->T * d->D == 0) return 0;
  if (dims_too_large(d)) {
    set_error("%s: bad dims: too large", name);
    return KVQ_E_DIMS;
  }
  const QuantCall c = quant_call(name, BITS, in_base, in_ptrs, in_st, in_dtype, q, q_st, scales, ssg, absmax_ws, eps, d,
                                 stream, false);
  const bool all_aligned = ptrs_aligned16(in_base, in_ptrs, 0, c.G, c.is.g * c.esz);
  // Split is decided for the whole call (no chunk's own alignment enters it): phase 1 over every chunk, then phase 2
  if (quant_route(c, all_aligned, all_aligned).fam == Quant::Split) {
    QuantCall p1 = c;
    p1.q = nullptr;
    p1.qs = {};
    p1.scales = nullptr;
    const int rc = run_split(p1, 1);
    return rc ? rc : run_split(c, 2);
  }
  return for_launch_chunks(c.G, kPtrsPerLaunch, [&](int64_t g0, int64_t gn) -> int {
    const QuantRoute r = quant_route(c, all_aligned, ptrs_aligned16(in_base, in_ptrs, g0, gn, c.is.g * c.esz));
    QuantArgs a;
    if (const int rc = chunk_args(c, g0, gn, a)) return rc;
    if (r.fam == Quant::Generic && !absmax_ws) {
      set_error("%s: absmax_ws workspace required for this shape or alignment (two-pass path)", name);
      return KVQ_E_NULL;
    }
    int rc = 0;
    if (r.fam == Quant::Tile) launch_tile<BITS>(c, r, a);
    else if (r.fam == Quant::Wide) launch_wide<BITS>(c, r, a);
    else
      by_dtype(in_dtype, [&](auto idt) {
        constexpr int IDT = decltype(idt)::value;
        if (r.fam == Quant::Generic) rc = launch_generic<IDT>(c, a, true, BITS);
        else launch_fused<IDT, BITS>(c, r, a);
      });
    return rc ? rc : check_launch(name);
  });
}

// validation of the split-phase entry points; phase 1: q == q_st == scales == nullptr
static int split_phase(int phase, const char* name, int bits, const void* in_base, const void* const* in_ptrs,
                       const kvq_strides_t* in_st, int in_dtype, uint8_t* q, const kvq_strides_t* q_st, float* scales,
                       int64_t ssg, float* absmax, float eps, const kvq_dims_t* d, void* stream, bool accumulate) {
  if (const int rc = check_group_call(in_st && absmax && (phase == 1 || (q && q_st && scales)), in_base, in_ptrs, absmax, d, name))
    return rc;
  if (dims_too_large(d)) {
    set_error("%s: bad dims: too large", name);
    return KVQ_E_DIMS;
  }
  if (const int rc = check_in_dtype(in_dtype, name)) return rc;
  if (phase == 2 && bits != 8 && bits != 4) {
    set_error("%s: bits must be 8 or 4", name);
    return KVQ_E_DIMS;
  }
  if (d->G * d->B * d->H * d->T * d->D == 0) return 0;
  return run_split(quant_call(name, bits, in_base, in_ptrs, in_st, in_dtype, q, q_st, scales, ssg, absmax, eps, d, stream,
                              accumulate), phase);
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_quant_i8_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, int in_dtype,
                        int8_t* q, const kvq_strides_t* q_st, float* scales, int64_t scale_stride_g,
                        float* absmax_ws, float eps, const kvq_dims_t* dims, void* stream) {
  return quant_tokens<8>(in_base, in_ptrs, in_st, in_dtype, reinterpret_cast<uint8_t*>(q), q_st, scales,
                         scale_stride_g, absmax_ws, eps, dims, stream, "kvq_quant_i8_tokens");
}

int kvq_quant_i4_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, int in_dtype,
                        uint8_t* packed, const kvq_strides_t* p_st, float* scales, int64_t scale_stride_g,
                        float* absmax_ws, float eps, const kvq_dims_t* dims, void* stream) {
  return quant_tokens<4>(in_base, in_ptrs, in_st, in_dtype, packed, p_st, scales, scale_stride_g, absmax_ws, eps,
                         dims, stream, "kvq_quant_i4_tokens");
}

int kvq_absmax_tokens(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, int in_dtype,
                      float* absmax, const kvq_dims_t* dims, void* stream) {
  return split_phase(1, "kvq_absmax_tokens", 8, in_base, in_ptrs, in_st, in_dtype, nullptr, nullptr, nullptr, 0, absmax,
                     0.0f, dims, stream, false);
}

int kvq_absmax_tokens_acc(const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st, int in_dtype,
                          float* absmax, const kvq_dims_t* dims, void* stream) {
  return split_phase(1, "kvq_absmax_tokens_acc", 8, in_base, in_ptrs, in_st, in_dtype, nullptr, nullptr, nullptr, 0, absmax,
                     0.0f, dims, stream, true);
}

int kvq_quant_tokens_from_absmax(int bits, const void* in_base, const void* const* in_ptrs, const kvq_strides_t* in_st,
                                 int in_dtype, uint8_t* q, const kvq_strides_t* q_st, float* scales,
                                 int64_t scale_stride_g, const float* absmax, float eps, const kvq_dims_t* dims,
                                 void* stream) {
  return split_phase(2, "kvq_quant_tokens_from_absmax", bits, in_base, in_ptrs, in_st, in_dtype, q, q_st, scales,
                     scale_stride_g, const_cast<float*>(absmax), eps, dims, stream, false);
}

}  // extern "C"

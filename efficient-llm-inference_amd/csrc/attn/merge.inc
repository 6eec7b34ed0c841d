// merge.inc — part of kvq_attn.hip (one translation unit, included in this order): the merge kernels (chained, one-round-trip, one wave per head) + the new token's quantise-append
constexpr int kAttnMfmaTC = 128;

constexpr int kAttnMaxSplit = 4096;  // merge: LDS weights + 16 (m, l) pairs per thread; T <= 512 Ki tokens at 128 per split

// A new-token slice past the register path (more than 8,192 elements: batch > 8 at 8 kv heads x 128). The generic routine
// walked it with ONE workgroup, element by element, twice: 40 us at batch 16 and 158 us at batch 64 on top of a 17 / 43 us
// attention (profiles/r04ac_decode_step_by_batch.jsonl; with this routine: + 3 / + 10 us, the merge launch 7.9 / 8.9 us under
// rocprofv3 against 4.0 / 4.9 without an append) — every layer of every decode step. Here the slice is cut into
// a.nparts pieces (host: one per 8,192 elements), one workgroup each: EVERY workgroup takes the abs-max of the WHOLE slice
// (16-byte loads, 16 in flight per thread; 128 KiB at most, the same lines for all of them) — so nothing crosses workgroups —
// and quantises only its own piece, with the generic routine's expressions per element (IEEE divide, round-half-even):
// the same bytes and the same scale. Host-checked preconditions: D % 8 == 0, 16-byte aligned rows of x, store rows aligned
// to the 8 / 4 bytes a vector's codes take.
template <int IDT>
__device__ inline void quant_new_token_parts(const NewTokenArgs& a, const uint32_t w, const uint32_t part, float* s_red) {
  constexpr int UN = 32;  // 65,536 elements (the host's bound) = 32 vectors per thread: every load of the abs-max pass is in flight at once
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const uint32_t tid = threadIdx.x;
  const uint32_t DV = a.D >> 3, nvec = a.B * a.H * DV;
  const uint16_t* x = reinterpret_cast<const uint16_t*>(a.x[w]);
  auto src = [&](const uint32_t v, uint32_t& b, uint32_t& h, uint32_t& piece) -> const u32x4* {
    const uint32_t row = v / DV;
    piece = v - row * DV;
    b = row / a.H;
    h = row - b * a.H;
    return reinterpret_cast<const u32x4*>(x + (int64_t)b * a.xs_b[w] + (int64_t)h * a.xs_h[w] + piece * 8u);
  };
  auto elem = [](const u32x4& r, const int e) -> float { return Elem<IDT>::widen((uint16_t)((r[e >> 1] >> (16 * (e & 1))) & 0xFFFFu)); };
  // this workgroup's own piece first: its (at most OWN) vectors per thread are requested together with the whole slice and stay in
  // registers across the reduction, so the routine is ONE memory round trip (a second pass that re-read them measured 8.5 us per
  // launch at batch 16 where the merge workgroups of the same launch take 4)
  constexpr int OWN = 4;  // chunk <= OWN * kAttnBlock vectors: the host cuts one piece per 8,192 elements
  const uint32_t chunk = (nvec + a.nparts - 1u) / a.nparts;
  const uint32_t lo = part * chunk, hi = lo + chunk < nvec ? lo + chunk : nvec;
  u32x4 own[OWN];
  uint32_t ob[OWN], oh[OWN], op[OWN];
#pragma unroll
  for (int k = 0; k < OWN; ++k) {
    const uint32_t v = lo + tid + (uint32_t)(k * kAttnBlock);
    own[k] = u32x4{0u, 0u, 0u, 0u};
    ob[k] = oh[k] = op[k] = 0u;
    if (v < hi) own[k] = *src(v, ob[k], oh[k], op[k]);
  }
  // abs-max on the bit patterns: |x| of a half / bfloat16 is its low 15 bits, and those order like the values, +inf above
  // every finite value and a NaN above +inf (the reference's abs().max() keeps a NaN too): two elements per packed
  // unsigned max, one conversion at the end
  u16x2 mb = {0, 0};
  // the slice walk advances kAttnBlock vectors = RPP rows per step: (b, h) move by a uniform (quotient, remainder) of RPP / H
  // instead of two integer divisions per vector (72 divisions per thread were most of this routine's time)
  const uint32_t dvsh = DV == 16u ? 4u : 3u;  // host: head_dim 128 or 64
  const uint32_t RPP = (uint32_t)kAttnBlock >> dvsh, qstep = RPP / a.H, rstep = RPP - qstep * a.H;
  const uint32_t wpiece = tid & (DV - 1u);
  uint32_t wb = (tid >> dvsh) / a.H, wh = (tid >> dvsh) - wb * a.H;
  for (uint32_t v0 = tid; v0 < nvec; v0 += (uint32_t)(kAttnBlock * UN)) {
    u32x4 r[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const uint32_t v = v0 + (uint32_t)(u * kAttnBlock);
      r[u] = u32x4{0u, 0u, 0u, 0u};
      if (v < nvec) r[u] = *reinterpret_cast<const u32x4*>(x + (int64_t)wb * a.xs_b[w] + (int64_t)wh * a.xs_h[w] + wpiece * 8u);
      wb += qstep;
      wh += rstep;
      if (wh >= a.H) {
        wh -= a.H;
        ++wb;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t absb = r[u][c] & 0x7FFF7FFFu;
        u16x2 pair;
        __builtin_memcpy(&pair, &absb, 4);
        mb = __builtin_elementwise_max(mb, pair);
      }
  }
  float m = Elem<IDT>::widen(mb[0] > mb[1] ? mb[0] : mb[1]);
  m = block_max_nonneg(m, s_red);
  auto codes8 = [&](const u32x4& r, const float s32) -> u32x2 {
    u32x2 o = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e >> 2] |= ((uint32_t)(uint8_t)(int8_t)quant1<8>(elem(r, e), s32)) << (8 * (e & 3));
    return o;
  };
  auto codes4 = [&](const u32x4& r, const float s32) -> uint32_t {
    uint32_t o = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // even index -> high nibble
      const int h4 = quant1<4>(elem(r, 2 * j), s32) + 8, l4 = quant1<4>(elem(r, 2 * j + 1), s32) + 8;
      o |= (uint32_t)(((h4 & 0xF) << 4) | (l4 & 0xF)) << (8 * j);
    }
    return o;
  };
  if (a.bits[w] == 8) {
    const float s32 = scale_of<8>(m, a.eps);
    if (tid == 0u && part == 0u) *a.scale[w] = Elem<IDT>::round_trip(s32);
#pragma unroll
    for (int k = 0; k < OWN; ++k)
      if (lo + tid + (uint32_t)(k * kAttnBlock) < hi)
        *reinterpret_cast<u32x2*>(a.q[w] + (int64_t)ob[k] * a.qs_b[w] + (int64_t)oh[k] * a.qs_h[w] + op[k] * 8u) = codes8(own[k], s32);
    for (uint32_t v = lo + tid + (uint32_t)(OWN * kAttnBlock); v < hi; v += kAttnBlock) {  // (pieces the host never cuts: past OWN vectors per thread)
      uint32_t b, h, piece;
      const u32x4 r = *src(v, b, h, piece);
      *reinterpret_cast<u32x2*>(a.q[w] + (int64_t)b * a.qs_b[w] + (int64_t)h * a.qs_h[w] + piece * 8u) = codes8(r, s32);
    }
  } else {
    const float s32 = scale_of<4>(m, a.eps);
    if (tid == 0u && part == 0u) *a.scale[w] = Elem<IDT>::round_trip(s32);
#pragma unroll
    for (int k = 0; k < OWN; ++k)
      if (lo + tid + (uint32_t)(k * kAttnBlock) < hi)
        *reinterpret_cast<uint32_t*>(a.q[w] + (int64_t)ob[k] * a.qs_b[w] + (int64_t)oh[k] * a.qs_h[w] + op[k] * 4u) = codes4(own[k], s32);
    for (uint32_t v = lo + tid + (uint32_t)(OWN * kAttnBlock); v < hi; v += kAttnBlock) {
      uint32_t b, h, piece;
      const u32x4 r = *src(v, b, h, piece);
      *reinterpret_cast<uint32_t*>(a.q[w] + (int64_t)b * a.qs_b[w] + (int64_t)h * a.qs_h[w] + piece * 4u) = codes4(r, s32);
    }
  }
}

// decode_attn_merge_k and decode_attn_merge_padded_k: one kernel text (merge_chained_kernel.inc), compiled twice; twice more with
// the score modifiers of the kvq_*_ex calls (KVQ_MERGE_MOD 1: decode_attn_merge_mod_k, decode_attn_merge_padded_mod_k)
#define KVQ_MERGE_MOD 0
#define KVQ_MERGE_PADDED 0
#include "merge_chained_kernel.inc"
#undef KVQ_MERGE_PADDED
#define KVQ_MERGE_PADDED 1
#include "merge_chained_kernel.inc"
#undef KVQ_MERGE_PADDED
#undef KVQ_MERGE_MOD
#define KVQ_MERGE_MOD 1
#define KVQ_MERGE_PADDED 0
#include "merge_chained_kernel.inc"
#undef KVQ_MERGE_PADDED
#define KVQ_MERGE_PADDED 1
#include "merge_chained_kernel.inc"
#undef KVQ_MERGE_PADDED
#undef KVQ_MERGE_MOD

// ---------------------------------------------------------------------------- merge, one round trip
// The merge above is a chain of dependent round trips (new-token dot -> (m, l) -> (m, l) again -> rows in two
// batches -> new-token V): at batch 1 nothing hides them and a call costs 5 us for 2 MB (9 us inside a decode
// step, where every operand was written by the kernel before and is cold in this XCD's L2). This variant, for up
// to kAttnBlock splits, REQUESTS everything the workgroup reads before it waits for anything — the device-side
// token count, its (m, l) pair, the new token's q / k / v elements and the first kMergePF partial rows of each
// thread (rows past the live splits are read too: the workspace holds them, their values are never used) — and
// synchronises its waves with LDS-only barriers (`__syncthreads()` would drain the outstanding global loads).
// Same arithmetic in the same order as decode_attn_merge_k: bit-identical results.
constexpr int kMergePF = 16;
// A word another kernel wrote, read through the CONSTANT address space: with a uniform address that is an s_load the
// compiler tracks itself (issued where it stands, waited for at the first use), where a global-space load becomes a
// vector load that is waited for on the spot. Only for memory no store of THIS kernel touches.
__device__ __forceinline__ int scalar_load_i32(const int* p) {
  return *reinterpret_cast<const __attribute__((address_space(4))) int*>(reinterpret_cast<uintptr_t>(p));
}
__device__ __forceinline__ void lds_barrier() {  // this workgroup's LDS traffic only; global loads stay in flight
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// The new token's K (w = 0) / V (w = 1) slice quantised into slot T of its store by ONE workgroup, as
// quant_new_token_block does, but in one round trip: every element pair is requested up front (with the device-side
// slot number), stays in registers between the abs-max and the stores, and the workgroup meets at ONE LDS-only
// barrier. Same expressions per element (IEEE divide, round-half-even), so the stored bytes and scale are the
// generic routine's. Uniform precondition (checked by the caller): even D, 2-element-aligned rows, at most
// 2 * kAttnBlock * kNewPairs elements.
constexpr int kNewPairs = 16;
__device__ inline bool new_token_fits_registers(const NewTokenArgs& a, uint32_t w) {
  return (a.D & 1u) == 0u && (uint64_t)a.B * a.H * a.D <= 2ull * kAttnBlock * kNewPairs && ((a.xs_b[w] | a.xs_h[w]) & 1) == 0 &&
         (reinterpret_cast<uintptr_t>(a.x[w]) & 3u) == 0u;
}
template <int IDT>
__device__ inline void quant_new_token_regs(const NewTokenArgs& a, const uint32_t w, float* s_red, const int* t_dev, const uint32_t t_bound,
                                            const void* valid) {
  const uint32_t tid = threadIdx.x;
  const uint32_t np = a.B * a.H * a.D / 2u;  // element pairs
  // the device-side slot number: a SCALAR load (uniform address), issued here and waited for by the compiler at
  // its first use below the fence
  const uint32_t t_raw = (uint32_t)scalar_load_i32(t_dev ? t_dev : reinterpret_cast<const int*>(valid));
  const uint16_t* x = reinterpret_cast<const uint16_t*>(a.x[w]);
  uint32_t raw[kNewPairs];
  uint32_t row[kNewPairs], col[kNewPairs];  // (b, h) row and element offset of the pair
#pragma unroll
  for (int k = 0; k < kNewPairs; ++k) {
    const uint32_t p = tid + (uint32_t)k * kAttnBlock;
    const uint32_t e = 2u * (p < np ? p : np - 1u);
    row[k] = e / a.D;
    col[k] = e - row[k] * a.D;
    const int64_t off = (int64_t)(row[k] / a.H) * a.xs_b[w] + (int64_t)(row[k] % a.H) * a.xs_h[w] + col[k];
    raw[k] = *reinterpret_cast<const uint32_t*>(x + off);
  }
  __builtin_amdgcn_sched_barrier(0);
  const int64_t slot = t_dev ? (int64_t)(t_raw < t_bound ? t_raw : t_bound) : 0;  // host-side T: a.q / a.scale point at the slot already
  float lo[kNewPairs], hi[kNewPairs];
  float m = 0.0f;  // max_nonneg throughout: a NaN element is the slice's abs-max, as in the reference
#pragma unroll
  for (int k = 0; k < kNewPairs; ++k) {
    lo[k] = Elem<IDT>::widen((uint16_t)(raw[k] & 0xFFFFu));
    hi[k] = Elem<IDT>::widen((uint16_t)(raw[k] >> 16));
    if (tid + (uint32_t)k * kAttnBlock < np) m = max_nonneg(m, max_nonneg(fabsf(lo[k]), fabsf(hi[k])));
  }
  m = __uint_as_float(wave_umax(__float_as_uint(m)));
  if ((tid & 63u) == 0u) s_red[tid >> 6] = m;
  lds_barrier();
  m = max_nonneg(max_nonneg(s_red[0], s_red[1]), max_nonneg(s_red[2], s_red[3]));
  uint8_t* qbase = a.q[w] + slot * a.qs_t[w];
  if (a.bits[w] == 8) {
    const float s32 = scale_of<8>(m, a.eps);
    if (tid == 0u) a.scale[w][slot] = Elem<IDT>::round_trip(s32);
#pragma unroll
    for (int k = 0; k < kNewPairs; ++k) {
      if (tid + (uint32_t)k * kAttnBlock < np) {
        uint8_t* dst = qbase + (int64_t)(row[k] / a.H) * a.qs_b[w] + (int64_t)(row[k] % a.H) * a.qs_h[w] + col[k];
        dst[0] = (uint8_t)(int8_t)quant1<8>(lo[k], s32);
        dst[1] = (uint8_t)(int8_t)quant1<8>(hi[k], s32);
      }
    }
  } else {
    const float s32 = scale_of<4>(m, a.eps);
    if (tid == 0u) a.scale[w][slot] = Elem<IDT>::round_trip(s32);
#pragma unroll
    for (int k = 0; k < kNewPairs; ++k) {
      if (tid + (uint32_t)k * kAttnBlock < np) {
        const int h4 = quant1<4>(lo[k], s32) + 8, l4 = quant1<4>(hi[k], s32) + 8;  // even index -> high nibble
        qbase[(int64_t)(row[k] / a.H) * a.qs_b[w] + (int64_t)(row[k] % a.H) * a.qs_h[w] + (col[k] >> 1)] = (uint8_t)(((h4 & 0xF) << 4) | (l4 & 0xF));
      }
    }
  }
}

// the one-wave / one-round-trip merges and their padded forms: one text (merge_fast_kernel.inc), compiled twice; twice more with
// the score modifiers of the kvq_*_ex calls (KVQ_MERGE_MOD 1: the *_mod / *_mod_k forms)
#define KVQ_MERGE_MOD 0
#define KVQ_MERGE_PADDED 0
#include "merge_fast_kernel.inc"
#undef KVQ_MERGE_PADDED
#define KVQ_MERGE_PADDED 1
#include "merge_fast_kernel.inc"
#undef KVQ_MERGE_PADDED
#undef KVQ_MERGE_MOD
#define KVQ_MERGE_MOD 1
#define KVQ_MERGE_PADDED 0
#include "merge_fast_kernel.inc"
#undef KVQ_MERGE_PADDED
#define KVQ_MERGE_PADDED 1
#include "merge_fast_kernel.inc"
#undef KVQ_MERGE_PADDED
#undef KVQ_MERGE_MOD

// common.inc — part of kvq_attn.hip (one translation unit, included in this order): AttnArgs, element helpers, wave reductions (everything the attention kernels share)

constexpr int kAttnBlock = 256;
constexpr int kAttnMaxTS = 1024;  // tokens per workgroup (LDS: NQ * TS floats)
constexpr int kAttnUnroll = 4;    // tokens in flight per lane

struct AttnArgs {
  const void* q;
  int64_t q_sb, q_sh;  // elements
  const uint8_t* k;
  int64_t k_sb, k_sh, k_st;  // bytes
  const float* k_scale;
  const uint8_t* v;
  int64_t v_sb, v_sh, v_st;
  const float* v_scale;
  const void* kn;
  int64_t kn_sb, kn_sh;
  const void* vn;
  int64_t vn_sb, vn_sh;
  void* out;
  int64_t o_sb, o_sh;
  float* ws;        // [B*Hq*nsplit][2] (m, l), then at acc_off [B*Hq*nsplit][D]
  int64_t acc_off;  // floats
  float sm_scale;
  uint32_t B, Hq, Hkv, T, D, TS, nsplit, nq;
  int32_t lpt_shift;  // log2(D / 16): lanes per token
  int32_t dtype;      // KVQ_F16 | KVQ_BF16 (q, k_new, v_new, out)
  int32_t mfma;       // host: the MFMA partial kernel serves this call
  uint32_t stream_tpw;  // host: > 0 = the streaming MFMA kernel, that many 64-token tiles per wave
  uint32_t lds;         // host: 1 = the LDS-staged streaming kernel (decode_attn_lds_mfma_k) serves the streaming plan
  // kvq_decode_step_dev: the stored-token count lives in DEVICE memory (a captured HIP graph replays
  // the same launch for every decode step). T above is then the host's upper bound: it sizes the grid and
  // the workspace; workgroups past the real count exit, the merge reads ceil(T / TS) partials.
  const int32_t* t_dev;
  // A padded call (kvq_*_padded): kv_start [B] int32 in device memory, row b's keys before kv_start[b] are padding. nullptr
  // otherwise; only the *_padded_k kernels read it (kv_start_of).
  const int32_t* kv_start;
  uint32_t ws_bytes;  // unused (0): a field of an in-launch merge that measured slower (round 4, r04b); it keeps the layout
  // Sliding window of a device-side count (0 = none; the host-count path offsets the store on the host instead). The last
  // field, in the slot of that merge's unused fold flag: the struct keeps its size, so no kernel argument moves.
  int32_t window;
};

// Score modifiers of a kvq_*_ex call: one more argument of the *_mod_k kernels (AttnArgs keeps its size; no other kernel sees it).
//   softcap c > 0: every scaled score s becomes c tanh(s / c) before masking and softmax (Gemma 2's attn_logit_softcapping)
//   sinks: DEVICE [Hq] fp32, one more softmax term per query head without a value row (gpt-oss's s_aux); only the merges and the
//          extend kernels read it, the host never does
// cap_k = 2 log2(e) / c, filled by the host: tanh(x) = 1 - 2 / (2^(2 log2(e) x) + 1) is one v_exp_f32 and one v_rcp_f32 and
// saturates cleanly (2^big = inf -> 1, 2^-big = 0 -> -1).
struct AttnMod {
  float softcap, cap_k;
  const float* sinks;
};
// c tanh(s / c) of a score in the natural-log domain (c = 0: s itself)
__device__ __forceinline__ float softcap_score(const float s, const AttnMod& mod) {
  if (!(mod.softcap > 0.0f)) return s;
  return fmaf(-2.0f * mod.softcap, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(s * mod.cap_k) + 1.0f), mod.softcap);
}
// The same for kernels that keep their scores in the log2 domain (s2 = s log2(e)): c2 tanh(s2 / c2) with c2 = c log2(e), as
// two constants taken once per kernel: cap2 = c2 and k2 = 2 log2(e) / c2 = cap_k ln(2).
struct Cap2 {
  float c, k;
};
__device__ __forceinline__ Cap2 cap_log2(const AttnMod& mod) { return Cap2{mod.softcap * 1.44269504088896341f, mod.cap_k * 0.693147180559945309f}; }
__device__ __forceinline__ float softcap2(const float s2, const Cap2 cap) {
  return fmaf(-2.0f * cap.c, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(s2 * cap.k) + 1.0f), cap.c);
}

// stored tokens this launch attends: the host's count, or the device word of a graph-replayed step
// (clamped to the host's bound: a count the caller let run past it can make the result wrong, never the accesses)
__device__ inline uint32_t live_tokens(const AttnArgs& a) {
  if (!a.t_dev) return a.T;
  const uint32_t t = (uint32_t)__builtin_nontemporal_load(a.t_dev);
  return t < a.T ? t : a.T;
}
// Under a device-side count with a sliding window of W keys the query at position t sees stored tokens [lo, t) with
// lo = max(0, t + 1 - W): the first visible row. Callers add lo to their row and scale bases and attend live = t - lo
// tokens. Only ever evaluated inside a t_dev branch or a device-count instantiation.
__device__ inline uint32_t window_lo(const AttnArgs& a, const uint32_t t) {
  return (a.window > 0 && t + 1u > (uint32_t)a.window) ? t + 1u - (uint32_t)a.window : 0u;
}
// live_tokens() with the window applied: the count of visible stored tokens and (lo) where they start
__device__ inline uint32_t live_window(const AttnArgs& a, uint32_t& lo) {
  lo = 0u;
  if (!a.t_dev) return a.T;
  const uint32_t t = live_tokens(a);
  lo = window_lo(a, t);
  return t - lo;
}

// ---- left-padded batches (kvq_*_padded): row b's keys before kv_start[b] are padding -------------------------------------
// kv_start[b] of a padded launch (AttnArgs::kv_start). The address is workgroup-uniform and no kernel of the launch
// stores to the array: read through the constant address space it is a scalar load, issued where it stands and waited for at
// its first use (merge.inc's scalar_load_i32 does the same for *t_dev).
__device__ __forceinline__ int32_t kv_start_of(const AttnArgs& a, const uint32_t b) {
  return *reinterpret_cast<const __attribute__((address_space(4))) int32_t*>(reinterpret_cast<uintptr_t>(a.kv_start) + 4u * (uintptr_t)b);
}
// First stored row a padded decode query of a batch row sees, from the live count t (host's T or the clamped device word), the
// row's start as loaded and whether the launch has a new token (query position t) or not (t - 1; the host refuses t = 0 then):
// lo = max(window's lower bound, start), the start clamped to [0, t] (a bad value can make the result wrong, never an access out
// of bounds). The row attends stored [lo, t): t - lo tokens, possibly none. The partial kernels and the merges of a padded
// launch all derive lo with this one function.
__device__ __forceinline__ uint32_t padded_lo(const AttnArgs& a, const uint32_t t, const int32_t start, const bool has_new) {
  const uint32_t keys = t + (has_new ? 1u : 0u);  // the query's position + 1
  const uint32_t wlo = (a.window > 0 && keys > (uint32_t)a.window) ? keys - (uint32_t)a.window : 0u;
  const uint32_t s = start < 0 ? 0u : ((uint32_t)start < t ? (uint32_t)start : t);
  return wlo > s ? wlo : s;
}

// Tiles per wave of the LDS-staged ring kernel when the token count is a DEVICE word (a captured decode graph: the launch
// arguments, nsplit among them, come from the host's upper bound): the live tiles are spread over all nsplit waves of a
// (batch row, kv head) — ceil(tiles / nsplit) each — so that every wave of the launch works whatever the count is. The ring
// kernel and the merge kernels derive it from the same count with this one function; tc = tokens per tile (a.TS / a.stream_tpw).
__device__ inline uint32_t ring_dev_tpw(const AttnArgs& a, const uint32_t T, const uint32_t tc) {
  const uint32_t ntiles = (T + tc - 1u) / tc;
  const uint32_t tpw = (ntiles + a.nsplit - 1u) / a.nsplit;
  return tpw ? tpw : 1u;
}
// tokens per split as the merge sees them: the host's, or the ring kernel's device-side choice above
__device__ inline uint32_t live_split_tokens(const AttnArgs& a, const uint32_t T) {
  if (!a.t_dev || a.stream_tpw == 0u) return a.TS;
  const uint32_t tc = a.TS / a.stream_tpw;
  return ring_dev_tpw(a, T, tc) * tc;
}
// The same for a padded launch, lt = the batch row's live count: the padded ring kernel spreads a row's live tiles over the
// launch's waves whether the count is the host's or a device word (a host-count padded call has no host-side lo).
__device__ inline uint32_t padded_split_tokens(const AttnArgs& a, const uint32_t lt) {
  if (a.stream_tpw == 0u) return a.TS;
  const uint32_t tc = a.TS / a.stream_tpw;
  return ring_dev_tpw(a, lt, tc) * tc;
}

__device__ inline f16x2 bits_h2(uint32_t u) {
  f16x2 h;
  __builtin_memcpy(&h, &u, 4);
  return h;
}
__device__ inline uint32_t h2_bits(f16x2 h) {
  uint32_t u;
  __builtin_memcpy(&u, &h, 4);
  return u;
}
__device__ inline float load_elem(const void* p, int64_t i, int dtype) {
  const uint16_t b = reinterpret_cast<const uint16_t*>(p)[i];
  return dtype == KVQ_F16 ? Elem<KVQ_F16>::widen(b) : Elem<KVQ_BF16>::widen(b);
}

// 16 consecutive query elements as 8 f16 pairs (bf16 queries are converted: exact for the normal
// f16 range). PERM4: pair order of the INT4 path, per 8 elements (q0,q2) (q4,q6) (q1,q3) (q5,q7).
template <bool PERM4>
__device__ inline void convert_q16(const u32x4 a, const u32x4 b, int dtype, f16x2 (&qv)[8]) {
  uint32_t w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  if (dtype == KVQ_BF16) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f16x2 h = {(f16)__uint_as_float(w[j] << 16), (f16)__uint_as_float(w[j] & 0xFFFF0000u)};
      w[j] = h2_bits(h);
    }
  }
  if constexpr (PERM4) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const uint32_t w0 = w[4 * g], w1 = w[4 * g + 1], w2 = w[4 * g + 2], w3 = w[4 * g + 3];
      w[4 * g + 0] = __builtin_amdgcn_perm(w1, w0, 0x05040100u);  // (q0, q2)
      w[4 * g + 1] = __builtin_amdgcn_perm(w3, w2, 0x05040100u);  // (q4, q6)
      w[4 * g + 2] = __builtin_amdgcn_perm(w1, w0, 0x07060302u);  // (q1, q3)
      w[4 * g + 3] = __builtin_amdgcn_perm(w3, w2, 0x07060302u);  // (q5, q7)
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) qv[j] = bits_h2(w[j]);
}

// Raw bytes of 16 stored elements of one token row.
template <int BITS>
struct Raw16;
template <>
struct Raw16<8> {
  u32x4 w;
  __device__ inline void load(const uint8_t* p) { w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }
  // exact f16 pairs of the int8 values: byte ^ 0x80 = q + 128; 0x6400 | u is the f16 1024 + u
  __device__ inline void to_h2(f16x2 (&kp)[8]) const {
    const f16x2 bias = {(f16)1152.0f, (f16)1152.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t x = w[i] ^ 0x80808080u;
      kp[2 * i] = bits_h2(__builtin_amdgcn_perm(0x64646464u, x, 0x04010400u)) - bias;      // (e0, e1)
      kp[2 * i + 1] = bits_h2(__builtin_amdgcn_perm(0x64646464u, x, 0x04030402u)) - bias;  // (e2, e3)
    }
  }
  // q + 128 as floats (bias folded by the caller)
  __device__ inline void to_f32_biased(float (&u)[16]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t x = w[i] ^ 0x80808080u;
      u[4 * i] = (float)(x & 0xFFu);
      u[4 * i + 1] = (float)((x >> 8) & 0xFFu);
      u[4 * i + 2] = (float)((x >> 16) & 0xFFu);
      u[4 * i + 3] = (float)(x >> 24);
    }
  }
  static constexpr float kBias = 128.0f;
  static constexpr int kBytes = 16;
};
template <>
struct Raw16<4> {
  u32x2 w;
  __device__ inline void load(const uint8_t* p) { w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p)); }
  // nibble = q + 8, even element in the HIGH nibble (ops.py:61-63); pair order per 8 elements:
  // (e0,e2) (e4,e6) (e1,e3) (e5,e7) — convert_q16<true> arranges the query the same way
  __device__ inline void to_h2(f16x2 (&kp)[8]) const {
    const f16x2 bias = {(f16)1032.0f, (f16)1032.0f};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t hi = (w[i] >> 4) & 0x0F0F0F0Fu;  // elements 0, 2, 4, 6
      const uint32_t lo = w[i] & 0x0F0F0F0Fu;         // elements 1, 3, 5, 7
      kp[4 * i + 0] = bits_h2(__builtin_amdgcn_perm(0x64646464u, hi, 0x04010400u)) - bias;
      kp[4 * i + 1] = bits_h2(__builtin_amdgcn_perm(0x64646464u, hi, 0x04030402u)) - bias;
      kp[4 * i + 2] = bits_h2(__builtin_amdgcn_perm(0x64646464u, lo, 0x04010400u)) - bias;
      kp[4 * i + 3] = bits_h2(__builtin_amdgcn_perm(0x64646464u, lo, 0x04030402u)) - bias;
    }
  }
  __device__ inline void to_f32_biased(float (&u)[16]) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t hi = (w[i] >> 4) & 0x0F0F0F0Fu;
      const uint32_t lo = w[i] & 0x0F0F0F0Fu;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        u[8 * i + 2 * b] = (float)((hi >> (8 * b)) & 0xFFu);
        u[8 * i + 2 * b + 1] = (float)((lo >> (8 * b)) & 0xFFu);
      }
    }
  }
  static constexpr float kBias = 8.0f;
  static constexpr int kBytes = 8;
};

template <int CTRL>
__device__ inline uint32_t dpp_u32_attn(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
// sum over aligned groups of 2^logw consecutive lanes (logw <= 4), every lane gets the sum
__device__ inline float group_fadd(float v, int logw) {
  if (logw > 0) v += __uint_as_float(dpp_u32_attn<0xB1>(__float_as_uint(v)));
  if (logw > 1) v += __uint_as_float(dpp_u32_attn<0x4E>(__float_as_uint(v)));
  if (logw > 2) v += __uint_as_float(dpp_u32_attn<0x141>(__float_as_uint(v)));
  if (logw > 3) v += __uint_as_float(dpp_u32_attn<0x140>(__float_as_uint(v)));
  return v;
}

// Exchanges across the four 16-lane rows of a wave WITHOUT the LDS crossbar (__shfl_xor is ds_bpermute: an LDS round
// trip on the wave's critical path): v_permlane16_swap / v_permlane32_swap of a value with a copy of itself leave
// {own, partner} in the two results for the partner 16 (32) lanes away; max and + are commutative, so every lane
// computes the same bits a __shfl_xor butterfly would.
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
// max over the wave, in every lane: DPP butterflies inside a 16-lane row, lane swaps across the rows
__device__ inline float wave_fmax(float v) {
  v = fmaxf(v, __uint_as_float(dpp_u32_attn<0xB1>(__float_as_uint(v))));   // lane ^ 1
  v = fmaxf(v, __uint_as_float(dpp_u32_attn<0x4E>(__float_as_uint(v))));   // lane ^ 2
  v = fmaxf(v, __uint_as_float(dpp_u32_attn<0x141>(__float_as_uint(v))));  // row_half_mirror
  v = fmaxf(v, __uint_as_float(dpp_u32_attn<0x140>(__float_as_uint(v))));  // row_mirror
  return xor32_max(xor16_max(v));
}
// unsigned max over the wave, in every lane (wave_fmax's exchanges): the abs-max of non-negative floats by their bit
// patterns, which keeps a NaN (kvq_common.h, max_nonneg)
__device__ inline uint32_t wave_umax(uint32_t v) {
  v = max(v, dpp_u32_attn<0xB1>(v));
  v = max(v, dpp_u32_attn<0x4E>(v));
  v = max(v, dpp_u32_attn<0x141>(v));
  v = max(v, dpp_u32_attn<0x140>(v));
  const auto r16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = max(r16[0], r16[1]);
  const auto r32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return max(r32[0], r32[1]);
}
// sum over the wave, in every lane (same exchanges as wave_fmax: no LDS round trips; every lane adds in the same order)
__device__ inline float wave_fsum(float v) {
  v += __uint_as_float(dpp_u32_attn<0xB1>(__float_as_uint(v)));
  v += __uint_as_float(dpp_u32_attn<0x4E>(__float_as_uint(v)));
  v += __uint_as_float(dpp_u32_attn<0x141>(__float_as_uint(v)));
  v += __uint_as_float(dpp_u32_attn<0x140>(__float_as_uint(v)));
  return xor32_add(xor16_add(v));
}

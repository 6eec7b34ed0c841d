// tile_mfma.inc — part of kvq_attn.hip (one translation unit, included in this order): AttnTile + decode_attn_partial_mfma_k: one wave per split, both products on the matrix cores
// ---------------------------------------------------------------------------- MFMA variant
// Grouped-query heads (3..16 query heads per kv head, head_dim 64 or 128): the per-element VALU cost of
// the kernel above grows with the group size (one dot2 / fma per element and head) and it ends up
// VALU-bound (llama 4:1 grouping: 2.1 TB/s at batch 8). Here both products run on the matrix
// cores as 16x16x32 f16 MFMAs with the heads padded to 16 columns; the VALU only converts
// int8 / nibbles to f16 (exactly) and transposes V bytes in registers.
//   ONE WAVE per workgroup, TC tokens, no barriers between phases.
//   S = K Q^T : A = K tile (row = token x, k = 8 of the lane group's d), B = Q^T (col = head x),
//               C: lane (x, g) holds head x, tokens 16 i + 4 g + r  (i = tile, r = 0..3)
//   O = P V   : A = P, taken from the lane's OWN score registers of tiles 2s, 2s+1 (the k order
//               of a 32-token step is defined as tokens 32 s + 4 g + j, 32 s + 16 + 4 g + (j-4), so
//               no lane movement); B = V with col x <-> d = 8 x + n for MFMA n = 0..7, so the lane
//               reads 8 contiguous bytes (4 for INT4) of 8 token rows and transposes them 8x8 in
//               registers; C: lane (x, g) holds heads 4 g + r of d = 8 x + n.
// P is scaled by sv[t] / max sv before the f16 pack (range), the output by max sv afterwards.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ inline f16x8 pack_h8(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  u32x4 w = {a, b, c, d};
  f16x8 h;
  __builtin_memcpy(&h, &w, 16);
  return h;
}
// bytes (u0..u3) of x, each meaning value u - BIAS -> two f16 pairs, exact
template <int BIAS>
__device__ inline void bytes_to_h4(uint32_t x, uint32_t& lo, uint32_t& hi) {
  const f16x2 bias = {(f16)(1024.0f + BIAS), (f16)(1024.0f + BIAS)};
  lo = h2_bits(bits_h2(__builtin_amdgcn_perm(0x64646464u, x, 0x04010400u)) - bias);
  hi = h2_bits(bits_h2(__builtin_amdgcn_perm(0x64646464u, x, 0x04030402u)) - bias);
}
// 4x4 byte transpose: rows a0..a3 -> columns c0..c3 (c_n = byte n of every row)
__device__ inline void transpose4x4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t (&c)[4]) {
  const uint32_t t0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u);
  const uint32_t t1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
  const uint32_t t2 = __builtin_amdgcn_perm(a3, a2, 0x05010400u);
  const uint32_t t3 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
  c[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
  c[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
  c[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
  c[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// INT8 K without any conversion: the stored bytes ARE the A operand of v_mfma_i32_16x16x64_i8 (lane (x, g): row x,
// k = 16 g .. 16 g + 15 of a 64-wide k-block = the 16 bytes the K load of chunk c already holds). The query becomes
// two int8 planes per head, q ~= aq (q1 + q2 / 254) with aq = max|q| / 127 (error <= max|q| / 64,516 per element,
// finer than the f16 input's own 2^-11 for all but the smallest elements), so S = aq (K.q1 + K.q2 / 254) with both
// products exact in int32. Saves the byte -> f16 conversion of K (5 vector instructions per 4 elements).
typedef int i32x4 __attribute__((ext_vector_type(4)));
struct QPlanes {
  i32x4 p1, p2;
};
// 16 query values = 8 dwords of f16 pairs (already in element order) -> 16 bytes per plane
__device__ inline QPlanes quantize_q16(const uint32_t (&w)[8], const float inv) {
  QPlanes o;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t b1 = 0u, b2 = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f16x2 h = bits_h2(w[2 * d + (j >> 1)]);
      const float t = (float)h[j & 1] * inv;
      const float q1 = rintf(t);
      const float q2 = rintf((t - q1) * 254.0f);
      b1 |= ((uint32_t)(int)q1 & 0xFFu) << (8 * j);
      b2 |= ((uint32_t)(int)q2 & 0xFFu) << (8 * j);
    }
    o.p1[d] = (int)b1;
    o.p2[d] = (int)b2;
  }
  return o;
}
__device__ inline float absmax_h2(const uint32_t wd) {
  const f16x2 h = bits_h2(wd & 0x7FFF7FFFu);
  return fmaxf((float)h[0], (float)h[1]);
}

// One wave's tile of TC tokens starting at t0 (nt valid ones, 1 <= nt <= TC) of kv head hk, batch row b:
// on return lane (x, g) holds m (log2 domain) and l of head x, and acc[c][r] = head 4 g + r, element
// d = DVN x + e(c) (see attn_tile_store) of sum_t p[t] sv[t] v_int[t, d] / svmax. s_ks / s_vs: TC floats of
// LDS each, private to this wave.
// (Requesting EVERY V step together with the K rows — one round trip for the whole tile — was measured at batch 1,
// where the launch is a single round of waves and registers are free: 10.5 us vs 9.6 us for the partial kernel,
// profiles/r02s_attn_b1_vfirst.txt. The staggered requests below stay.)
template <int KBITS, int VBITS, int TC, int HD, bool KI8 = false>
struct AttnTile {
  static_assert(HD == 64 || HD == 128, "head_dim of the MFMA kernel");
  static_assert(!KI8 || KBITS == 8, "the int8 MFMA path is for INT8 keys");
  static constexpr int NT = TC / 16;   // 16-token score tiles
  static constexpr int NS = TC / 32;   // 32-token P V steps
  static constexpr int KS = HD / 32;   // k-steps of the score product
  static constexpr int DVN = HD / 16;  // MFMAs (d values per lane) of a P V step
  // K row bytes per lane group and load: 16 (8 for INT4 at head_dim 64); loads per row and lane
  static constexpr int CBK = (HD * KBITS / 8) / 4 < 16 ? 8 : 16;
  static constexpr int NL = (HD * KBITS / 8) / (4 * CBK);
  static constexpr int EPC = CBK * 8 / KBITS;  // elements per chunk
  static constexpr int SPL = EPC / 8;          // k-steps per load
  static_assert(NL * SPL == KS, "k-step bookkeeping");
  static constexpr int VB = DVN * VBITS / 8;   // V bytes per lane and row: 8, 4 or 2
  float m, l, svmax;
  f32x4 acc[DVN];

  // CAP (the soft-capped kernel, decode_attn_partial_mfma_mod_k): every scaled score becomes c tanh(s / c), in the log2 domain
  // the scores are kept in (cap: cap_log2 of the call's AttnMod), before the masks and the softmax
  template <bool CAP = false>
  __device__ __forceinline__ void run(const AttnArgs& a, const uint32_t b, const uint32_t hk, const uint32_t t0, const uint32_t nt,
                                      float* s_ks, float* s_vs, const Cap2 cap = Cap2{}) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t x = lane & 15u, g = lane >> 4;

  // K / V rows are read with BUFFER loads: descriptor (uniform base of this split's rows, size =
  // the split's valid bytes) + a 32-bit offset (constant lane part + uniform row part: one v_add per
  // load instead of 64-bit address arithmetic); rows past the split's end are out of the descriptor's
  // range and read as zeros instead of being clamped or branched around (their scores are masked to
  // -inf, their P is exactly 0), and nothing outside the split's rows is ever touched.
  const bool full = nt == (uint32_t)TC;  // uniform
  const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a.v + (int64_t)b * a.v_sb + (int64_t)hk * a.v_sh + (int64_t)t0 * a.v_st), 0,
      (int)(nt * (uint32_t)a.v_st), 0x00020000);
  const uint32_t v_lane = 4u * g * (uint32_t)a.v_st + (uint32_t)VB * x;
  // V rows of a 32-token step, raw bytes (two dwords hold up to 8 bytes)
  struct VRaw {
    uint32_t w0, w1;
  };
  auto load_v_step = [&](int s, VRaw (&dst)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t row = 32 * s + 16 * (j >> 2) + (j & 3);  // + 4 g from the lane offset
      // the row offset rides in the VECTOR offset (one v_add): that is the operand the range check covers
      const uint32_t off = v_lane + row * (uint32_t)a.v_st;
      if constexpr (VB == 8) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(v_rsrc, off, 0, kKvAux);
        dst[j].w0 = v[0];
        dst[j].w1 = v[1];
      } else if constexpr (VB == 4) {
        dst[j].w0 = __builtin_amdgcn_raw_buffer_load_b32(v_rsrc, off, 0, kKvAux);
        dst[j].w1 = 0u;
      } else {
        dst[j].w0 = (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(v_rsrc, off, 0, kKvAux);
        dst[j].w1 = 0u;
      }
    }
  };
  // mixed mode (INT8 K, INT4 V): every later step fits the registers the K rows free (3 waves per SIMD
  // either way); the other kind pairs keep one step of look-ahead
  // (requesting EVERY V row up front, behind the K rows, measured slower at batch 1 — 10.3 vs 9.7 us per launch:
  // the V requests queue in front of other waves' K rows, which the score product waits for)
  constexpr bool V_EARLY = KBITS == 8 && VBITS == 4;
  VRaw vr[V_EARLY ? NS : 2][8];

  // ---- S = K Q^T: tile i, token row x -----------------------------------------------------------
  f32x4 sc[NT];
  f16x8 qb[KS];
  svmax = 0.0f;
  {
    const uint8_t* kb = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh + (int64_t)t0 * a.k_st;
    uint32_t raw[NT][NL][CBK / 4];
    const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(kb), 0, (int)(nt * (uint32_t)a.k_st), 0x00020000);
    const uint32_t k_lane = x * (uint32_t)a.k_st + (uint32_t)CBK * g;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
#pragma unroll
      for (int c = 0; c < NL; ++c) {
        const uint32_t off = k_lane + 16 * i * (uint32_t)a.k_st + 4 * CBK * c;
        if constexpr (CBK == 16) {
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, off, 0, kKvAux);
#pragma unroll
          for (int j = 0; j < 4; ++j) raw[i][c][j] = v[j];
        } else {
          const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(k_rsrc, off, 0, kKvAux);
          raw[i][c][0] = v[0];
          raw[i][c][1] = v[1];
        }
      }
    }
    load_v_step(0, vr[0]);
    // query and scales are REQUESTED here too, before anything waits: one round trip for all of it.
    // k-step (c, wi) of this lane group covers d = EPC (4 c + g) + 8 wi + j (INT4: j in pair order)
    uint32_t w[4 * KS];
    {
      const uint32_t hx = x < a.nq ? x : 0u;  // padded heads read head 0 and are zeroed below
      const char* qp = reinterpret_cast<const char*>(a.q) + ((int64_t)b * a.q_sb + (int64_t)(hk * a.nq + hx) * a.q_sh) * 2;
#pragma unroll
      for (int c = 0; c < NL; ++c)
#pragma unroll
        for (int wi = 0; wi < SPL; ++wi) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(qp + (EPC * (4 * c + g) + 8 * wi) * 2);
#pragma unroll
          for (int j = 0; j < 4; ++j) w[4 * (c * SPL + wi) + j] = v[j];
        }
    }
    constexpr int SR = (TC + kWave - 1) / kWave;  // TC = 32: the upper half of the wave idles here
    float ksv[SR], vsv[SR];
#pragma unroll
    for (int r = 0; r < SR; ++r) {
      const uint32_t i = r * kWave + lane;
      const uint32_t ic = i < nt ? i : nt - 1u;
      ksv[r] = a.k_scale[t0 + ic];
      vsv[r] = a.v_scale[t0 + ic];
    }
    // scores are kept in the log2 domain (one v_exp_f32 per probability); V scales are staged
    // already divided by the split's largest one (the f16 pack of P needs the range, see header)
#pragma unroll
    for (int r = 0; r < SR; ++r) {
      const uint32_t i = r * kWave + lane;
      if (i >= nt) vsv[r] = 0.0f;
      svmax = fmaxf(svmax, vsv[r]);
    }
    svmax = wave_fmax(svmax);
    const float svn = svmax > 0.0f ? 1.0f / svmax : 0.0f;
#pragma unroll
    for (int r = 0; r < SR; ++r) {
      const uint32_t i = r * kWave + lane;
      if (TC >= kWave || i < (uint32_t)TC) {
        s_ks[i] = ksv[r] * (a.sm_scale * 1.44269504088896341f);
        s_vs[i] = vsv[r] * svn;
      }
    }
    // ---- Q^T operands: head x, the 8 d's of this lane group per k-step (zeros for padded heads) ----
    {
      if (a.dtype == KVQ_BF16) {
#pragma unroll
        for (int j = 0; j < 4 * KS; ++j) {
          const f16x2 h = {(f16)__uint_as_float(w[j] << 16), (f16)__uint_as_float(w[j] & 0xFFFF0000u)};
          w[j] = h2_bits(h);
        }
      }
      if constexpr (KBITS == 4) {
#pragma unroll
        for (int c = 0; c < KS; ++c) {
          const uint32_t w0 = w[4 * c], w1 = w[4 * c + 1], w2 = w[4 * c + 2], w3 = w[4 * c + 3];
          w[4 * c + 0] = __builtin_amdgcn_perm(w1, w0, 0x05040100u);  // (q0, q2)
          w[4 * c + 1] = __builtin_amdgcn_perm(w3, w2, 0x05040100u);  // (q4, q6)
          w[4 * c + 2] = __builtin_amdgcn_perm(w1, w0, 0x07060302u);  // (q1, q3)
          w[4 * c + 3] = __builtin_amdgcn_perm(w3, w2, 0x07060302u);  // (q5, q7)
        }
      }
      if (x >= a.nq) {
#pragma unroll
        for (int j = 0; j < 4 * KS; ++j) w[j] = 0u;
      }
#pragma unroll
      for (int c = 0; c < KS; ++c) qb[c] = pack_h8(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
    }
    QPlanes qi[KI8 ? NL : 1];
    float aq = 1.0f;
    if constexpr (KI8) {  // the head's two int8 planes (w is zero for padded heads: planes 0, aq irrelevant)
      float qm = 0.0f;
#pragma unroll
      for (int j = 0; j < 4 * KS; ++j) qm = fmaxf(qm, absmax_h2(w[j]));
      qm = xor32_max(xor16_max(qm));
      aq = qm > 0.0f ? qm / 127.0f : 1.0f;
      const float inv = qm > 0.0f ? 127.0f / qm : 0.0f;
#pragma unroll
      for (int c = 0; c < NL; ++c) {
        uint32_t wc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wc[j] = w[8 * c + j];
        qi[c] = quantize_q16(wc, inv);
      }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      f32x4 c4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (KI8) {
        i32x4 c1 = {0, 0, 0, 0}, c2 = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < NL; ++c) {
          const i32x4 ka = {(int)raw[i][c][0], (int)raw[i][c][1], (int)raw[i][c][2], (int)raw[i][c][3]};
          c1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ka, qi[c].p1, c1, 0, 0, 0);
          c2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ka, qi[c].p2, c2, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) c4[r] = fmaf((float)c2[r], 1.0f / 254.0f, (float)c1[r]) * aq;
        sc[i] = c4;
        continue;
      }
#pragma unroll
      for (int c = 0; c < NL; ++c) {
        if constexpr (KBITS == 8) {  // two words = 8 elements = one k-step
#pragma unroll
          for (int wi = 0; wi < SPL; ++wi) {
            uint32_t h[4];
            bytes_to_h4<128>(raw[i][c][2 * wi] ^ 0x80808080u, h[0], h[1]);
            bytes_to_h4<128>(raw[i][c][2 * wi + 1] ^ 0x80808080u, h[2], h[3]);
            c4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(pack_h8(h[0], h[1], h[2], h[3]), qb[c * SPL + wi], c4, 0, 0, 0);
          }
        } else {  // one word = 8 elements = one k-step
#pragma unroll
          for (int wi = 0; wi < SPL; ++wi) {
            uint32_t h[4];
            bytes_to_h4<8>((raw[i][c][wi] >> 4) & 0x0F0F0F0Fu, h[0], h[1]);  // (e0,e2) (e4,e6)
            bytes_to_h4<8>(raw[i][c][wi] & 0x0F0F0F0Fu, h[2], h[3]);         // (e1,e3) (e5,e7)
            c4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(pack_h8(h[0], h[1], h[2], h[3]), qb[c * SPL + wi], c4, 0, 0, 0);
          }
        }
      }
      sc[i] = c4;
    }
    // the K registers are free now: request the remaining V steps ahead of the softmax
    if constexpr (V_EARLY) {
#pragma unroll
      for (int s = 1; s < NS; ++s) load_v_step(s, vr[s]);
    }
  }
  // this wave's own LDS writes above are read below by other lanes of the SAME wave: the LDS queue of a
  // wave is in order, so only the compiler has to be kept from moving the reads up
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- softmax over this split for head x (log2 domain); P scaled by sv / max sv ------------------
  m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const f32x4 ks = *reinterpret_cast<const f32x4*>(&s_ks[16 * i + 4 * g]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sc[i][r] *= ks[r];
      if constexpr (CAP) sc[i][r] = softcap2(sc[i][r], cap);
    }
  }
  if (!full) {  // uniform: only a ragged last tile pays for the masks
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((uint32_t)(16 * i + 4 * g + r) >= nt) sc[i][r] = -INFINITY;
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, sc[i][r]);
  }
  m = xor32_max(xor16_max(m));
  l = 0.0f;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const f32x4 sv = *reinterpret_cast<const f32x4*>(&s_vs[16 * i + 4 * g]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f(sc[i][r] - m);  // tokens past nt: exp2(-inf) = 0
      l += p;
      sc[i][r] = p * sv[r];
    }
  }
  l = xor32_add(xor16_add(l));

  // ---- O = P V: column x <-> d = DVN x + e(c) for MFMA c ---------------------------------------------
#pragma unroll
  for (int n = 0; n < DVN; ++n) acc[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if constexpr (!V_EARLY) {
        if (s + 1 < NS) load_v_step(s + 1, vr[(s + 1) & 1]);
      }
      const int vi = V_EARLY ? s : (s & 1);  // constant after unrolling
      // the lane's 8 token rows of this step as byte images, 4 elements per dword:
      //   head_dim 128: img[0] = elements 0..3 (INT4: 0,2,4,6), img[1] = 4..7 (INT4: 1,3,5,7)
      //   head_dim 64:  img[0] = elements 0..3 (INT4: 0,2,1,3)
      uint32_t img[DVN / 4][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t w0 = vr[vi][j].w0, w1 = vr[vi][j].w1;
        if constexpr (HD == 128 && VBITS == 8) {
          img[0][j] = w0 ^ 0x80808080u;
          img[1][j] = w1 ^ 0x80808080u;
        } else if constexpr (HD == 128) {
          img[0][j] = (w0 >> 4) & 0x0F0F0F0Fu;
          img[1][j] = w0 & 0x0F0F0F0Fu;
        } else if constexpr (VBITS == 8) {
          img[0][j] = w0 ^ 0x80808080u;
        } else {
          img[0][j] = ((w0 >> 4) & 0x0F0Fu) | ((w0 & 0x0F0Fu) << 16);
        }
      }
      const f16x8 pa = pack_h8(Elem<KVQ_F16>::pack2(sc[2 * s][0], sc[2 * s][1]), Elem<KVQ_F16>::pack2(sc[2 * s][2], sc[2 * s][3]),
                               Elem<KVQ_F16>::pack2(sc[2 * s + 1][0], sc[2 * s + 1][1]),
                               Elem<KVQ_F16>::pack2(sc[2 * s + 1][2], sc[2 * s + 1][3]));
      constexpr int BIAS = VBITS == 8 ? 128 : 8;
#pragma unroll
      for (int half = 0; half < DVN / 4; ++half) {
        uint32_t ca[4], cb[4];
        transpose4x4(img[half][0], img[half][1], img[half][2], img[half][3], ca);  // tokens j = 0..3
        transpose4x4(img[half][4], img[half][5], img[half][6], img[half][7], cb);  // tokens j = 4..7
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          uint32_t h[4];
          bytes_to_h4<BIAS>(ca[n], h[0], h[1]);
          bytes_to_h4<BIAS>(cb[n], h[2], h[3]);
          acc[4 * half + n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, pack_h8(h[0], h[1], h[2], h[3]), acc[4 * half + n], 0, 0, 0);
        }
      }
    }
  }

  }

  // acc values of row r (head 4 g + r) in element order: o8[e] for d = DVN x + e
  __device__ __forceinline__ void ordered(const int r, const float scale, float (&o8)[DVN]) const {
#pragma unroll
    for (int c = 0; c < DVN; ++c) {
      int e = c;
      if constexpr (VBITS == 4 && HD == 128) e = c < 4 ? 2 * c : 2 * (c - 4) + 1;
      if constexpr (VBITS == 4 && HD == 64) e = c == 1 ? 2 : (c == 2 ? 1 : c);
      o8[e] = acc[c][r] * scale;
    }
  }
};

// decode_attn_partial_mfma_k, decode_attn_partial_mfma_window_k and decode_attn_partial_mfma_padded_k: one kernel text
// (partial_mfma_kernel.inc), compiled three times; a fourth time as decode_attn_partial_mfma_mod_k, the soft-capped form
#define KVQ_PARTIAL_VARIANT 0
#include "partial_mfma_kernel.inc"
#undef KVQ_PARTIAL_VARIANT
#define KVQ_PARTIAL_VARIANT 1
#include "partial_mfma_kernel.inc"
#undef KVQ_PARTIAL_VARIANT
#define KVQ_PARTIAL_VARIANT 2
#include "partial_mfma_kernel.inc"
#undef KVQ_PARTIAL_VARIANT
#define KVQ_PARTIAL_VARIANT 3
#include "partial_mfma_kernel.inc"
#undef KVQ_PARTIAL_VARIANT

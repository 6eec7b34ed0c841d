// stream.inc — part of kvq_attn.hip (one translation unit, included in this order): AttnStream (online softmax across a wave's tiles; consume / consume_direct): the tile arithmetic of the ring kernel (ring.inc)
// ---------------------------------------------------------------------------- streaming tile arithmetic
// (issue / ROLL served the register-staged streaming kernel, which lost to the ring kernel; commit ab16b19 has it.)
// Larger batches (more tiles than wave slots): ONE wave walks `tpw` consecutive TC-token tiles of its
// (batch row, kv head) with the NEXT tile's K / V rows and scales requested before the current tile is
// reduced (two register sets, ping-pong), carries the softmax online across its tiles
//   m' = max(m, m_tile), alpha = 2^(m - m'), l = l alpha + sum p, acc = acc alpha (svref / svref') + P~ V
// and writes ONE partial at the end: a wave's loads and arithmetic overlap, the per-wave start-up (query
// operands, descriptors) is paid once per tpw tiles, and the split partials shrink by tpw.
// Same operand layouts as AttnTile (see its header). P is scaled by sv[t] / svref with svref the largest
// V scale seen so far (non-decreasing), the accumulator carries the matching 1 / svref.
// ROLL: the registers of the tile being reduced are re-requested piece by piece for the tile after next as soon as
// each piece has been consumed (K rows per 16-token group after its score MFMAs, V rows after their byte images are
// built, scales after they are staged): close to two tiles per wave stay in flight instead of one, which is what
// the bytes in flight the HBM needs at this bandwidth ask for (Little's law: 6 TB/s x ~5 us under load = 30 MB; one
// 12 KB tile per wave x 2048 waves is 24 MB). Batch 8, 16 K tokens: 49.4 -> 44.8 us per call.
// (Also measured: the INT4 V tile as 16-byte loads redistributed through an LDS image — 4 load instructions instead
// of 16: 2 us faster with the arithmetic removed, nothing with it, slower together with ROLL; not kept.)
// TG = 4 (int8 keys, at most 4 query heads per kv head — Llama-3 / Mistral grouping, 64-token tiles): the score product
// as ONE 16 x 16 output per int8 plane for the whole tile instead of four with 12 of 16 columns padding. Column j = (token
// group j >> 2, head j & 3): the MFMA of token group tg and d-half c multiplies that group's K rows by a query operand that
// is zero outside the four columns of tg, and all eight accumulate into the same registers (block-diagonal over the
// contraction: the same sixteen MFMAs per tile). Every lane then holds 4 real scores (head x & 3, tokens 16 (x >> 2) + 4 g
// + q) instead of 16 of which 12 are padding: a quarter of the softmax arithmetic (scale, max, exp2, sum, V-scale, f16
// pack); P reaches the P·V operand layout (row = head, 8 tokens per lane) by three DPP row rotations of two registers.
template <int KBITS, int VBITS, int TC, int HD, bool KI8 = false, bool ROLL = false, int TG = 1>
struct AttnStream {
  static_assert(TG == 1 || (TG == 4 && KI8 && TC == 64), "TG = 4: int8 keys, 64-token tiles");
  typedef AttnTile<KBITS, VBITS, TC, HD> TL;
  static constexpr int NT = TL::NT, NS = TL::NS, KS = TL::KS, DVN = TL::DVN, CBK = TL::CBK, NL = TL::NL, SPL = TL::SPL, VB = TL::VB;
  static constexpr int SR = (TC + kWave - 1) / kWave;
  struct Raw {  // one tile in flight: K rows, V rows, scales — as loaded
    uint32_t k[NT][NL][CBK / 4];
    uint32_t v[NS][8][VB == 8 ? 2 : 1];
    float ks[SR], vs[SR];
  };
  f16x8 qb[KS];
  QPlanes qi[KI8 ? NL : 1];  // INT8 K through the int8 MFMA: the query as two int8 planes, aq their scale
  QPlanes qt[TG == 4 ? 4 : 1][TG == 4 ? NL : 1];  // TG = 4: qi masked to the columns of token group tg
  float aq;
  float m, l, svref;
  f32x4 acc[DVN];

  __device__ __forceinline__ void init(const AttnArgs& a, const uint32_t b, const uint32_t hk) {
    const uint32_t lane = threadIdx.x & 63u, x = lane & 15u, g = lane >> 4;
    uint32_t w[4 * KS];
    const uint32_t xh = TG == 4 ? (x & 3u) : x;  // the head this lane's column stands for
    const uint32_t hx = xh < a.nq ? xh : 0u;     // padded heads read head 0 and are zeroed below
    const char* qp = reinterpret_cast<const char*>(a.q) + ((int64_t)b * a.q_sb + (int64_t)(hk * a.nq + hx) * a.q_sh) * 2;
#pragma unroll
    for (int c = 0; c < NL; ++c)
#pragma unroll
      for (int wi = 0; wi < SPL; ++wi) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(qp + (TL::EPC * (4 * c + g) + 8 * wi) * 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[4 * (c * SPL + wi) + j] = v[j];
      }
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
    if (xh >= a.nq) {
#pragma unroll
      for (int j = 0; j < 4 * KS; ++j) w[j] = 0u;
    }
#pragma unroll
    for (int c = 0; c < KS; ++c) qb[c] = pack_h8(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
    aq = 1.0f;
    if constexpr (KI8) {
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
      if constexpr (TG == 4) {
        const i32x4 zero = {0, 0, 0, 0};
#pragma unroll
        for (int tg = 0; tg < 4; ++tg)
#pragma unroll
          for (int c = 0; c < NL; ++c) {
            qt[tg][c].p1 = (x >> 2) == (uint32_t)tg ? qi[c].p1 : zero;
            qt[tg][c].p2 = (x >> 2) == (uint32_t)tg ? qi[c].p2 : zero;
          }
      }
    }
    m = -INFINITY;
    l = 0.0f;
    svref = 0.0f;
#pragma unroll
    for (int n = 0; n < DVN; ++n) acc[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  // where a tile's rows come from: buffer descriptors over its valid rows (nt == 0: every load returns zeros and
  // touches no memory — the "tile" past a wave's last one)
  struct Src {
    __amdgpu_buffer_rsrc_t k, v;
    uint32_t t0, nt;
  };
  __device__ __forceinline__ Src src(const AttnArgs& a, const uint32_t b, const uint32_t hk, const uint32_t t0, const uint32_t nt) const {
    Src s;
    s.k = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh + (int64_t)t0 * a.k_st), 0,
                                            (int)(nt * (uint32_t)a.k_st), 0x00020000);
    s.v = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.v + (int64_t)b * a.v_sb + (int64_t)hk * a.v_sh + (int64_t)t0 * a.v_st), 0,
                                            (int)(nt * (uint32_t)a.v_st), 0x00020000);
    s.t0 = t0;
    s.nt = nt;
    return s;
  }
  // the pieces of a tile's request; nothing waits here
  __device__ __forceinline__ void issue_k(const AttnArgs& a, const Src& s, const int i, Raw& r) const {  // 16-token group i
    const uint32_t lane = threadIdx.x & 63u, x = lane & 15u, g = lane >> 4;
    const uint32_t k_lane = x * (uint32_t)a.k_st + (uint32_t)CBK * g;
#pragma unroll
    for (int c = 0; c < NL; ++c) {
      const uint32_t off = k_lane + 16 * i * (uint32_t)a.k_st + 4 * CBK * c;
      if constexpr (CBK == 16) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(s.k, off, 0, kKvAux);
#pragma unroll
        for (int j = 0; j < 4; ++j) r.k[i][c][j] = v[j];
      } else {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(s.k, off, 0, kKvAux);
        r.k[i][c][0] = v[0];
        r.k[i][c][1] = v[1];
      }
    }
  }
  __device__ __forceinline__ void issue_v(const AttnArgs& a, const Src& s, const int sidx, Raw& r) const {  // 32-token step sidx
    const uint32_t lane = threadIdx.x & 63u, x = lane & 15u, g = lane >> 4;
    const uint32_t v_lane = 4u * g * (uint32_t)a.v_st + (uint32_t)VB * x;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t row = 32 * sidx + 16 * (j >> 2) + (j & 3);  // + 4 g from the lane offset
      const uint32_t off = v_lane + row * (uint32_t)a.v_st;
      if constexpr (VB == 8) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(s.v, off, 0, kKvAux);
        r.v[sidx][j][0] = v[0];
        r.v[sidx][j][1] = v[1];
      } else if constexpr (VB == 4) {
        r.v[sidx][j][0] = __builtin_amdgcn_raw_buffer_load_b32(s.v, off, 0, kKvAux);
      } else {
        r.v[sidx][j][0] = (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(s.v, off, 0, kKvAux);
      }
    }
  }
  __device__ __forceinline__ void issue_scales(const AttnArgs& a, const Src& s, Raw& r) const {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int q = 0; q < SR; ++q) {
      const uint32_t i = q * kWave + lane;
      const uint32_t ic = i < s.nt ? i : (s.nt ? s.nt - 1u : 0u);
      r.ks[q] = a.k_scale[s.t0 + ic];
      r.vs[q] = i < s.nt ? a.v_scale[s.t0 + ic] : 0.0f;
    }
  }
  __device__ __forceinline__ void issue(const AttnArgs& a, const Src& s, Raw& r) const {  // the whole tile
#pragma unroll
    for (int i = 0; i < NT; ++i) issue_k(a, s, i, r);
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) issue_v(a, s, sidx, r);
    issue_scales(a, s, r);
  }

  // fold one loaded tile into the running (m, l, acc); s_ks / s_vs: TC floats each, s_al: 16 floats (this wave's)
  // nx (ROLL): the tile after next, whose rows take over r's registers as this tile's pieces are consumed
  // CAP (the soft-capped ring kernel, decode_attn_lds_mfma_mod_k; consume_direct takes it the same way): every scaled score becomes
  // c tanh(s / c) in the log2 domain (cap: cap_log2 of the call's AttnMod), before the masks and the online softmax
  template <bool CAP = false>
  __device__ __forceinline__ void consume(const AttnArgs& a, const uint32_t nt, Raw& r, const Src& nx, float* s_ks, float* s_vs, float* s_al,
                                          const Cap2 cap = Cap2{}) {
    const uint32_t lane = threadIdx.x & 63u, x = lane & 15u, g = lane >> 4;
    const bool full = nt == (uint32_t)TC;  // uniform
    // ---- scales: K side with sm_scale log2(e) folded in, V side relative to the running reference ----------
    float svmax = 0.0f;
#pragma unroll
    for (int q = 0; q < SR; ++q) svmax = fmaxf(svmax, r.vs[q]);
    svmax = wave_fmax(svmax);
    const float svnew = fmaxf(svref, svmax);
    const float svn = svnew > 0.0f ? 1.0f / svnew : 0.0f;
    const float ratio = svnew > 0.0f ? svref * svn : 1.0f;  // <= 1; the first tile's accumulator is 0 anyway
    svref = svnew;
#pragma unroll
    for (int q = 0; q < SR; ++q) {
      const uint32_t i = q * kWave + lane;
      if (TC >= kWave || i < (uint32_t)TC) {
        s_ks[i] = r.ks[q] * (a.sm_scale * 1.44269504088896341f);
        s_vs[i] = r.vs[q] * svn;
      }
    }
    if constexpr (ROLL) issue_scales(a, nx, r);
    uint32_t pp[NS][4];  // P of this tile as the P·V operand: 8 tokens of head x per lane and 32-token step, f16 pairs
    float alpha;
    if constexpr (TG == 4) {
      // ---- S = K Q^T, one output for the tile: column x = (token group x >> 2, head x & 3) ---------------------------
      i32x4 c1 = {0, 0, 0, 0}, c2 = {0, 0, 0, 0};
#pragma unroll
      for (int tg = 0; tg < 4; ++tg) {
#pragma unroll
        for (int c = 0; c < NL; ++c) {
          const i32x4 ka = {(int)r.k[tg][c][0], (int)r.k[tg][c][1], (int)r.k[tg][c][2], (int)r.k[tg][c][3]};
          c1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ka, qt[tg][c].p1, c1, 0, 0, 0);
          c2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ka, qt[tg][c].p2, c2, 0, 0, 0);
        }
        if constexpr (ROLL) issue_k(a, nx, tg, r);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // s_ks / s_vs written above by this wave's lanes
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // ---- online softmax (log2 domain): 4 scores per lane, tokens tb .. tb + 3 of head x & 3 -------------------------
      const uint32_t tb = 16u * (x >> 2) + 4u * g;
      const f32x4 ks = *reinterpret_cast<const f32x4*>(&s_ks[tb]);
      float s4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        s4[q] = fmaf((float)c2[q], 1.0f / 254.0f, (float)c1[q]) * aq * ks[q];
        if constexpr (CAP) s4[q] = softcap2(s4[q], cap);
      }
      if (!full) {  // uniform: only a ragged last tile pays for the masks
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (tb + (uint32_t)q >= nt) s4[q] = -INFINITY;
      }
      float mt = fmaxf(fmaxf(s4[0], s4[1]), fmaxf(s4[2], s4[3]));
      // across the head's 16 lanes: the four token groups of the row (rotations by 8 and 4 lanes), the four rows
      mt = fmaxf(mt, __uint_as_float(dpp_u32_attn<0x128>(__float_as_uint(mt))));
      mt = fmaxf(mt, __uint_as_float(dpp_u32_attn<0x124>(__float_as_uint(mt))));
      mt = xor32_max(xor16_max(mt));
      const float mnew = fmaxf(m, mt);                 // finite: every tile holds >= 1 token
      alpha = __builtin_amdgcn_exp2f(m - mnew);        // first tile: 2^(-inf) = 0
      const f32x4 sv = *reinterpret_cast<const f32x4*>(&s_vs[tb]);
      float lt = 0.0f, pv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float p = __builtin_amdgcn_exp2f(s4[q] - mnew);  // tokens past nt: 2^(-inf) = 0
        lt += p;
        pv[q] = p * sv[q];
      }
      lt += __uint_as_float(dpp_u32_attn<0x128>(__float_as_uint(lt)));
      lt += __uint_as_float(dpp_u32_attn<0x124>(__float_as_uint(lt)));
      lt = xor32_add(xor16_add(lt));
      l = l * alpha + lt;
      m = mnew;
      // P·V operand of lane x (row = head x for x < 4; the other rows are padding): token group i comes from lane x + 4 i
      // of the row (row_ror:n hands lane i the value of lane i - n)
      const uint32_t p01 = Elem<KVQ_F16>::pack2(pv[0], pv[1]), p23 = Elem<KVQ_F16>::pack2(pv[2], pv[3]);
      pp[0][0] = p01;
      pp[0][1] = p23;
      pp[0][2] = dpp_u32_attn<0x12C>(p01);
      pp[0][3] = dpp_u32_attn<0x12C>(p23);
      pp[1][0] = dpp_u32_attn<0x128>(p01);
      pp[1][1] = dpp_u32_attn<0x128>(p23);
      pp[1][2] = dpp_u32_attn<0x124>(p01);
      pp[1][3] = dpp_u32_attn<0x124>(p23);
    } else {
    // ---- S = K Q^T ------------------------------------------------------------------------------------------
    f32x4 sc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      f32x4 c4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (KI8) {
        i32x4 c1 = {0, 0, 0, 0}, c2 = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < NL; ++c) {
          const i32x4 ka = {(int)r.k[i][c][0], (int)r.k[i][c][1], (int)r.k[i][c][2], (int)r.k[i][c][3]};
          c1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ka, qi[c].p1, c1, 0, 0, 0);
          c2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ka, qi[c].p2, c2, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) c4[q] = fmaf((float)c2[q], 1.0f / 254.0f, (float)c1[q]) * aq;
        sc[i] = c4;
        if constexpr (ROLL) issue_k(a, nx, i, r);
        continue;
      }
#pragma unroll
      for (int c = 0; c < NL; ++c) {
#pragma unroll
        for (int wi = 0; wi < SPL; ++wi) {
          uint32_t h[4];
          if constexpr (KBITS == 8) {
            bytes_to_h4<128>(r.k[i][c][2 * wi] ^ 0x80808080u, h[0], h[1]);
            bytes_to_h4<128>(r.k[i][c][2 * wi + 1] ^ 0x80808080u, h[2], h[3]);
          } else {
            bytes_to_h4<8>((r.k[i][c][wi] >> 4) & 0x0F0F0F0Fu, h[0], h[1]);  // (e0,e2) (e4,e6)
            bytes_to_h4<8>(r.k[i][c][wi] & 0x0F0F0F0Fu, h[2], h[3]);         // (e1,e3) (e5,e7)
          }
          c4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(pack_h8(h[0], h[1], h[2], h[3]), qb[c * SPL + wi], c4, 0, 0, 0);
        }
      }
      sc[i] = c4;
      if constexpr (ROLL) issue_k(a, nx, i, r);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // s_ks / s_vs written above by this wave's lanes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- online softmax (log2 domain) -------------------------------------------------------------------------
    float mt = -INFINITY;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const f32x4 ks = *reinterpret_cast<const f32x4*>(&s_ks[16 * i + 4 * g]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sc[i][q] *= ks[q];
        if constexpr (CAP) sc[i][q] = softcap2(sc[i][q], cap);
      }
    }
    if (!full) {  // uniform: only a ragged last tile pays for the masks
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((uint32_t)(16 * i + 4 * g + q) >= nt) sc[i][q] = -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) mt = fmaxf(mt, sc[i][q]);
    }
    mt = xor32_max(xor16_max(mt));
    const float mnew = fmaxf(m, mt);                          // finite: every tile holds >= 1 token
    alpha = __builtin_amdgcn_exp2f(m - mnew);     // first tile: 2^(-inf) = 0
    float lt = 0.0f;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const f32x4 sv = *reinterpret_cast<const f32x4*>(&s_vs[16 * i + 4 * g]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float p = __builtin_amdgcn_exp2f(sc[i][q] - mnew);  // tokens past nt: 2^(-inf) = 0
        lt += p;
        sc[i][q] = p * sv[q];
      }
    }
    lt = xor32_add(xor16_add(lt));
    l = l * alpha + lt;
    m = mnew;
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) {
      pp[sidx][0] = Elem<KVQ_F16>::pack2(sc[2 * sidx][0], sc[2 * sidx][1]);
      pp[sidx][1] = Elem<KVQ_F16>::pack2(sc[2 * sidx][2], sc[2 * sidx][3]);
      pp[sidx][2] = Elem<KVQ_F16>::pack2(sc[2 * sidx + 1][0], sc[2 * sidx + 1][1]);
      pp[sidx][3] = Elem<KVQ_F16>::pack2(sc[2 * sidx + 1][2], sc[2 * sidx + 1][3]);
    }
    }
    // the accumulator rows of this lane are heads 4 g + q: their alpha lives in lanes x = 4 g + q
    if (g == 0u) s_al[x] = alpha * ratio;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const f32x4 al = *reinterpret_cast<const f32x4*>(&s_al[4 * g]);
#pragma unroll
    for (int n = 0; n < DVN; ++n) acc[n] *= al;
    // ---- O += P V ---------------------------------------------------------------------------------------------
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) {
      uint32_t img[DVN / 4][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t w0 = r.v[sidx][j][0];
        if constexpr (HD == 128 && VBITS == 8) {
          img[0][j] = w0 ^ 0x80808080u;
          img[1][j] = r.v[sidx][j][VB == 8 ? 1 : 0] ^ 0x80808080u;
        } else if constexpr (HD == 128) {
          img[0][j] = (w0 >> 4) & 0x0F0F0F0Fu;
          img[1][j] = w0 & 0x0F0F0F0Fu;
        } else if constexpr (VBITS == 8) {
          img[0][j] = w0 ^ 0x80808080u;
        } else {
          img[0][j] = ((w0 >> 4) & 0x0F0Fu) | ((w0 & 0x0F0Fu) << 16);
        }
      }
      if constexpr (ROLL) issue_v(a, nx, sidx, r);
      const f16x8 pa = pack_h8(pp[sidx][0], pp[sidx][1], pp[sidx][2], pp[sidx][3]);
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
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the next tile's staging writes stay below this tile's LDS reads
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }

  // ---- TG = 4, scales straight from the LDS slot (the LDS-staged kernel) -------------------------------------------------
  // The same tile reduction with the wave's serial chain cut down: what a tile costs one wave per SIMD is less its arithmetic
  // (builds without any MFMA, V conversion and exp2 run 1 us faster out of 40, profiles/r03skip_*) than the LDS round trips
  // and lane exchanges between its steps. Here
  //   * the K / V scales are read as f32x4 from the slot the DMA left them in (no staging write, no wave barrier);
  //   * the V reference scale is the wave's own maximum, taken once before the first tile (`svref`, `svn` fixed by the
  //     kernel): no per-tile wave maximum, no rescale ratio;
  //   * l is summed per lane and reduced across the head's lanes once, at the end (`reduce_l`);
  //   * alpha reaches the accumulator rows by v_readlane (heads 0..3 live in lanes 0..3; rows 4..15 are padding) instead of
  //     an LDS round trip, and the rescale is skipped while no head's maximum moved;
  //   * nothing is written to LDS, so no fence closes the tile.
  // sc_slot: the slot's 64 K scales followed by its 64 V scales. Same sums as consume() up to the order l is added in.
  float svn;  // 1 / svref (0 when every V scale of the wave is 0)
  template <bool CAP = false>
  __device__ __forceinline__ void consume_direct(const AttnArgs& a, const uint32_t nt, Raw& r, const float* sc_slot, const Cap2 cap = Cap2{}) {
    static_assert(TG == 4, "the one-output score product");
    const uint32_t lane = threadIdx.x & 63u, x = lane & 15u, g = lane >> 4;
    const bool full = nt == (uint32_t)TC;  // uniform
    i32x4 c1 = {0, 0, 0, 0}, c2 = {0, 0, 0, 0};
#pragma unroll
    for (int tg = 0; tg < 4; ++tg) {
#pragma unroll
      for (int c = 0; c < NL; ++c) {
        const i32x4 ka = {(int)r.k[tg][c][0], (int)r.k[tg][c][1], (int)r.k[tg][c][2], (int)r.k[tg][c][3]};
        c1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ka, qt[tg][c].p1, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ka, qt[tg][c].p2, c2, 0, 0, 0);
      }
    }
    const uint32_t tb = 16u * (x >> 2) + 4u * g;
    const f32x4 ks = *reinterpret_cast<const f32x4*>(sc_slot + tb);
    const f32x4 sv = *reinterpret_cast<const f32x4*>(sc_slot + 64 + tb);
    const float kq = aq * (a.sm_scale * 1.44269504088896341f);
    float s4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      s4[q] = fmaf((float)c2[q], 1.0f / 254.0f, (float)c1[q]) * (kq * ks[q]);
      if constexpr (CAP) s4[q] = softcap2(s4[q], cap);
    }
    if (!full) {  // uniform: only a ragged last tile pays for the masks (its rows past nt hold an older tile's bytes)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (tb + (uint32_t)q >= nt) s4[q] = -INFINITY;
    }
    float mt = fmaxf(fmaxf(s4[0], s4[1]), fmaxf(s4[2], s4[3]));
    mt = fmaxf(mt, __uint_as_float(dpp_u32_attn<0x128>(__float_as_uint(mt))));
    mt = fmaxf(mt, __uint_as_float(dpp_u32_attn<0x124>(__float_as_uint(mt))));
    mt = xor32_max(xor16_max(mt));
    const float mnew = fmaxf(m, mt);                       // finite: every tile holds >= 1 token
    const float alpha = __builtin_amdgcn_exp2f(m - mnew);  // first tile: 2^(-inf) = 0
    m = mnew;
    float lt = 0.0f, pv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float p = __builtin_amdgcn_exp2f(s4[q] - mnew);  // tokens past nt: 2^(-inf) = 0
      lt += p;
      pv[q] = p * (full || tb + (uint32_t)q < nt ? sv[q] * svn : 0.0f);
    }
    l = l * alpha + lt;  // this lane's share of the head's sum (reduce_l() at the end)
    const uint32_t p01 = Elem<KVQ_F16>::pack2(pv[0], pv[1]), p23 = Elem<KVQ_F16>::pack2(pv[2], pv[3]);
    uint32_t pp[NS][4];
    pp[0][0] = p01;
    pp[0][1] = p23;
    pp[0][2] = dpp_u32_attn<0x12C>(p01);
    pp[0][3] = dpp_u32_attn<0x12C>(p23);
    pp[1][0] = dpp_u32_attn<0x128>(p01);
    pp[1][1] = dpp_u32_attn<0x128>(p23);
    pp[1][2] = dpp_u32_attn<0x124>(p01);
    pp[1][3] = dpp_u32_attn<0x124>(p23);
    // accumulator rows of this lane = heads 4 g + q; heads 0..3 (the real ones) keep their alpha in lanes 0..3
    f32x4 al;
#pragma unroll
    for (int q = 0; q < 4; ++q) al[q] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(alpha), q));
    if (!(al[0] == 1.0f && al[1] == 1.0f && al[2] == 1.0f && al[3] == 1.0f)) {  // uniform
#pragma unroll
      for (int n = 0; n < DVN; ++n) acc[n] *= al;
    }
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) {
      uint32_t img[DVN / 4][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t w0 = r.v[sidx][j][0];
        if constexpr (HD == 128 && VBITS == 8) {
          img[0][j] = w0 ^ 0x80808080u;
          img[1][j] = r.v[sidx][j][VB == 8 ? 1 : 0] ^ 0x80808080u;
        } else if constexpr (HD == 128) {
          img[0][j] = (w0 >> 4) & 0x0F0F0F0Fu;
          img[1][j] = w0 & 0x0F0F0F0Fu;
        } else if constexpr (VBITS == 8) {
          img[0][j] = w0 ^ 0x80808080u;
        } else {
          img[0][j] = ((w0 >> 4) & 0x0F0Fu) | ((w0 & 0x0F0Fu) << 16);
        }
      }
      const f16x8 pa = pack_h8(pp[sidx][0], pp[sidx][1], pp[sidx][2], pp[sidx][3]);
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
  // consume_direct's per-lane shares of l -> the head's sum, in every lane of the head
  __device__ __forceinline__ void reduce_l() {
    l += __uint_as_float(dpp_u32_attn<0x128>(__float_as_uint(l)));
    l += __uint_as_float(dpp_u32_attn<0x124>(__float_as_uint(l)));
    l = xor32_add(xor16_add(l));
  }
};
